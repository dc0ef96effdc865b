"""GPU: bit-identity of the f16x3 render kernel (siren16_kernel) at the places a change of its layer seams can break --
the hand-over from layer 0 to layer 1 at the start of a second and third sub-tile, the values carried over a layer
boundary, the invalid-point clones of a short last sub-tile, and the layer-7 record itself (not only what the second pass
makes of it).  tests/test_gpu_render_bitexact.py drives every instantiation on whole single sub-tiles; these cases add:
    render 8x8x18, B = 2, every output                     siren16_kernel<0, false, 0>, batch index, short sub-tiles
    render 64x64x18, every output                          16 rays x 18 samples = 288 points per workgroup: two full
                                                           sub-tiles and one of 32 points, rays straddling both seams
    point query, N = 130, with raw                         siren16_kernel<1, false, 0>: one full sub-tile plus two points
    first / second pass of an evaluated image 8x8x24       siren16_kernel<0, false, 1> / <0, false, 2>: SHA-256 of the record
    first pass of an evaluated image 64x64x24              16 rays x 24 samples: three full sub-tiles per workgroup, record
(The rays per workgroup are the launcher's choice, pick_rays_per_wg in csrc/siren.hip: 7 at 8x8x18 with B = 2, 3 at 8x8x24,
16 at 64x64.  Every workgroup of the record cases runs all its sub-tiles, so every byte of the record is written.)
Large outputs are compared by SHA-256 of their bytes, everything else element by element with torch.equal.

Record the fixture (on the GPU, from the commit whose numerics are the yardstick):
    python tests/test_gpu_render_seams.py --record"""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from conftest import GOLDEN, full_state_dict  # noqa: E402

import e3dge_amd  # noqa: E402,F401
from e3dge_amd import synthetic as syn  # noqa: E402
from e3dge_amd import volume_renderer as vr  # noqa: E402
from e3dge_amd.camera_utils import generate_camera_params  # noqa: E402
from e3dge_amd.volume_renderer import VolumeFeatureRenderer  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURE = os.path.join(GOLDEN, "render_seams_bitexact.npz")
OUT_KEYS = ('gen_thumb_imgs', 'features', 'xyz', 'depth', 'mask', 'sdf', 'hit_prob', 'points', 'rays_d', 'viewdirs', 'dists')


def _digest(t):
    return np.frombuffer(hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).digest(), dtype=np.uint8).copy()


def _renderer(sd, res, S, local=False):
    r = VolumeFeatureRenderer(syn.rendering_opt(N_samples=S, enable_local_model=local, L_pred_tex_modulations=local),
                              out_im_res=res, mode='test')
    own = {k: (syn.synthetic_tensor('renderer.' + k, v.shape) * 0.05 if 'netLocal' in k else
               sd['renderer.' + k.replace('network.netGlobal.', 'network.')]) for k, v in r.state_dict().items()}
    r.load_state_dict(own)
    r.siren.mfma_mode = "f16x3"
    return r.to(DEV).eval()


def _record_of(renderer):
    rec = vr._BACKBONE.get(renderer)
    assert rec is not None and rec['buf'] is not None, "the first pass left no layer-7 record"
    return rec['buf']


def cases():
    """name -> numpy array of every recorded output."""
    out = {}
    assert os.environ.get("E3DGE_REUSE_BACKBONE", "1") != "0", "the record cases need the backbone hand-over"
    with torch.no_grad():
        _, sd = full_state_dict(res=8, n_samples=18)          # (the renderer's weights do not depend on res / n_samples)
        wr2, _ = syn.synthetic_inputs(2, seed=7, device=DEV)
        wr1 = wr2[:1].contiguous()

        # 1. plain render 8x8x18, B = 2, every output key
        r = _renderer(sd, 8, 18)
        cam = generate_camera_params(8, DEV, locations=torch.tensor([[0.2, -0.15], [-0.25, 0.1]], device=DEV))
        o = r(cam[0], cam[1], cam[2], cam[3], styles=wr2)
        for k in OUT_KEYS:
            out["b2_" + k] = o[k].cpu().numpy()

        # 2. plain render 64x64x18: 288 points per workgroup (128 + 128 + 32)
        r64 = _renderer(sd, 64, 18)
        cam64 = generate_camera_params(64, DEV, locations=torch.tensor([[0.1, 0.05]], device=DEV))
        o = r64(cam64[0], cam64[1], cam64[2], cam64[3], styles=wr1)
        for k in OUT_KEYS:
            out["wide_" + k + "_sha256"] = _digest(o[k])
        out["wide_gen_thumb_imgs"] = o['gen_thumb_imgs'].cpu().numpy()
        out["wide_depth"] = o['depth'].cpu().numpy()

        # 3. point query (MODE 1), N = 130, with raw
        g = torch.Generator().manual_seed(23)
        pts = (torch.rand(1, 130, 3, generator=g) * 0.6 - 0.3).to(DEV)
        vd = torch.nn.functional.normalize(torch.randn(1, 130, 3, generator=g), dim=-1).to(DEV)
        sdf, raw = r.siren.query_points(pts, vd, wr1, r.box_scale, want_raw=True)
        out["query_sdf"] = sdf.cpu().numpy()
        out["query_raw"] = raw.cpu().numpy()

        # 4. evaluated image 8x8x24 with a local branch: the record itself, then what the second pass makes of it
        rl = _renderer(sd, 8, 24, local=True)
        cam8 = generate_camera_params(8, DEV, locations=torch.tensor([[-0.1, 0.2]], device=DEV))
        feats = syn.synthetic_local_feats(1, 8, 24, device=DEV)
        p1 = rl(cam8[0], cam8[1], cam8[2], cam8[3], styles=wr1)
        torch.cuda.synchronize()
        out["pass1_record_sha256"] = _digest(_record_of(rl))
        for k in OUT_KEYS:
            out["pass1_" + k] = p1[k].cpu().numpy()
        p2 = rl(cam8[0], cam8[1], cam8[2], cam8[3], styles=wr1, local_data_batch={'feats': feats})
        for k in ('gen_thumb_imgs', 'features'):
            out["pass2_" + k] = p2[k].cpu().numpy()

        # 5. first pass 64x64x24 with a local branch: 256 workgroups x 3 full sub-tiles, the record
        rl64 = _renderer(sd, 64, 24, local=True)
        p1 = rl64(cam64[0], cam64[1], cam64[2], cam64[3], styles=wr1)
        torch.cuda.synchronize()
        out["wide_pass1_record_sha256"] = _digest(_record_of(rl64))
        for k in ('gen_thumb_imgs', 'features', 'sdf', 'hit_prob'):
            out["wide_pass1_" + k + "_sha256"] = _digest(p1[k])
        vr.release_record_buffers(rl64)
    return out


@pytest.fixture(scope="module")
def computed():
    if not os.path.exists(FIXTURE):
        pytest.fail("bit-identity fixture missing (record it: python tests/test_gpu_render_seams.py --record)")
    return cases()


def test_seam_outputs_bit_identical(computed):
    ref = np.load(FIXTURE)
    assert set(ref.files) == set(computed), sorted(set(ref.files) ^ set(computed))
    bad = [k for k in sorted(computed) if not torch.equal(torch.from_numpy(computed[k]), torch.from_numpy(ref[k]))]
    assert not bad, f"not bit-identical: {bad}"


def test_seam_outputs_deterministic(computed):
    again = cases()
    for k, v in computed.items():
        assert torch.equal(torch.from_numpy(v), torch.from_numpy(again[k])), k


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_gpu_render_seams.py --record")
    res = cases()
    np.savez_compressed(FIXTURE, **res)
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes")
