"""GPU: the f16x3 render kernel (siren16_kernel) must stay BIT-identical across changes that only move instructions, LDS
layout or launch details.  Every instantiation the renderer runs is driven once on fixed inputs and compared with
torch.equal against outputs recorded on the MI355X:
    render 16x16x24, every output                       siren16_kernel<0, false, 0>
    render 8x8x24 saving its pre-sine arguments         siren16_kernel<0, true, 0>
    point query with raw (and a saving point query)     siren16_kernel<1, false / true, 0>
    first / second pass of an evaluated image 8x8x24    siren16_kernel<0, false, 1> / <0, false, 2>
Saved-argument buffers (megabytes) are compared by SHA-256 of their bytes; everything else element by element.

Record the fixtures (on the GPU, from the commit whose numerics are the yardstick):
    python tests/test_gpu_render_bitexact.py --record"""
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
from e3dge_amd.camera_utils import generate_camera_params  # noqa: E402
from e3dge_amd.volume_renderer import VolumeFeatureRenderer  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURES = {"render": os.path.join(GOLDEN, "render_bitexact_16x24.npz"),
            "misc": os.path.join(GOLDEN, "render_bitexact_misc.npz")}
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


def _zeroed_saved_buffer(B, N):
    # saved_state_buffer's storage, zero-filled: padding rows the kernel leaves alone then hash the same on every run
    return torch.zeros((B, (N + 15) // 16 * 16, 9, 256), device=DEV, dtype=torch.float32)


def cases():
    """name -> tensor (numpy) of every recorded output, in two groups (one fixture file each)."""
    out = {"render": {}, "misc": {}}
    assert os.environ.get("E3DGE_REUSE_BACKBONE", "1") != "0", "case 4 needs the backbone hand-over"
    with torch.no_grad():
        # 1. plain render, 16x16x24, every output
        _, sd = full_state_dict(res=16, n_samples=24)
        r = _renderer(sd, 16, 24)
        wr, _ = syn.synthetic_inputs(1, seed=3, device=DEV)
        cam = generate_camera_params(16, DEV, locations=torch.tensor([[0.15, -0.1]], device=DEV))
        poses, focal, near, far = cam[:4]
        o = r(poses, focal, near, far, styles=wr)
        for k in OUT_KEYS:
            out["render"]["plain_" + k] = o[k].cpu().numpy()

        # 2. saving render, 8x8x24 (pre-sine arguments of all nine layers)
        _, sd8 = full_state_dict(res=8, n_samples=24)
        r8 = _renderer(sd8, 8, 24)
        cam8 = generate_camera_params(8, DEV, locations=torch.tensor([[-0.1, 0.2]], device=DEV))
        film = r8.siren.film_params(wr)
        buf = _zeroed_saved_buffer(1, 8 * 8 * 24)
        o = r8.render_with_film(film, cam8[1], cam8[0], cam8[2], cam8[3], None, save_args=buf[:, :8 * 8 * 24])
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            out["misc"]["save_" + k] = o[k].cpu().numpy()
        out["misc"]["save_args_sha256"] = _digest(buf)

        # 3. point queries (MODE 1): raw outputs, and the saving query
        g = torch.Generator().manual_seed(11)
        pts = (torch.rand(1, 200, 3, generator=g) * 0.6 - 0.3).to(DEV)
        vd = torch.nn.functional.normalize(torch.randn(1, 200, 3, generator=g), dim=-1).to(DEV)
        sdf, raw = r8.siren.query_points(pts, vd, wr, r8.box_scale, want_raw=True)
        out["misc"]["query_sdf"] = sdf.cpu().numpy()
        out["misc"]["query_raw"] = raw.cpu().numpy()
        qbuf = _zeroed_saved_buffer(1, 200)
        sdf_s, _ = r8.siren.query_points(pts, vd, wr, r8.box_scale, want_raw=False, save_args=qbuf[:, :200])
        torch.cuda.synchronize()
        out["misc"]["query_save_sdf"] = sdf_s.cpu().numpy()
        out["misc"]["query_save_args_sha256"] = _digest(qbuf)

        # 4. evaluated image: first pass leaves the layer-7 record, second pass (texture FiLM) starts from it
        rl = _renderer(sd8, 8, 24, local=True)
        feats = syn.synthetic_local_feats(1, 8, 24, device=DEV)
        p1 = rl(cam8[0], cam8[1], cam8[2], cam8[3], styles=wr)
        p2 = rl(cam8[0], cam8[1], cam8[2], cam8[3], styles=wr, local_data_batch={'feats': feats})
        for k in OUT_KEYS:
            out["misc"]["pass1_" + k] = p1[k].cpu().numpy()
        for k in ('gen_thumb_imgs', 'features'):
            out["misc"]["pass2_" + k] = p2[k].cpu().numpy()
    return out


@pytest.fixture(scope="module")
def computed():
    if not all(os.path.exists(f) for f in FIXTURES.values()):
        pytest.fail("bit-identity fixtures missing (record them: python tests/test_gpu_render_bitexact.py --record)")
    return cases()


@pytest.mark.parametrize("group", sorted(FIXTURES))
def test_render_outputs_bit_identical(computed, group):
    ref = np.load(FIXTURES[group])
    got = computed[group]
    assert set(ref.files) == set(got), sorted(set(ref.files) ^ set(got))
    bad = [k for k in sorted(got) if not torch.equal(torch.from_numpy(got[k]), torch.from_numpy(ref[k]))]
    assert not bad, f"not bit-identical: {bad}"


def test_render_is_deterministic(computed):
    again = cases()
    for group, d in computed.items():
        for k, v in d.items():
            assert torch.equal(torch.from_numpy(v), torch.from_numpy(again[group][k])), (group, k)


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_gpu_render_bitexact.py --record")
    res = cases()
    for group, path in FIXTURES.items():
        np.savez_compressed(path, **res[group])
        print(path, os.path.getsize(path), "bytes")
