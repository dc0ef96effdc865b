"""GPU: run-to-run identity of the f16x3 inference renders (siren16_kernel<0, false, CACHE>).

The inference renders issue the two LDS-DMA pieces of a weight chunk from inside the k-steps of a tile instead of right
behind its barrier.  That does not touch the arithmetic; what such a
change could break is the chunk pipeline (a buffer overwritten while a wave still reads it, a chunk read before it has
landed), and a race shows as differences between runs of the same launch.  Every case renders eight times in a row with
the same inputs; every output of every repeat must be torch.equal to the first one:
    render 8x8x24, B = 2        3 rays per workgroup: short sub-tiles, invalid-point clones, batch index
    render 64x64x18             288 points per workgroup: two full sub-tiles and one of 32 points
    first + second pass 8x8x24  the record path: the second pass's pipe cycles over the view layer's 16 chunks
The 64x64x18 render and the 8x8x24 pair are cases of tests/golden/render_seams_bitexact.npz too (same weights, styles and
cameras as tests/test_gpu_render_seams.py): their first repeat must equal what that file holds, so all eight do.  The file
is read only."""
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
REPEATS = 8


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


@pytest.fixture(scope="module")
def setup():
    assert os.path.exists(FIXTURE), "tests/golden/render_seams_bitexact.npz is missing"
    _, sd = full_state_dict(res=8, n_samples=18)          # (the renderer's weights do not depend on res / n_samples)
    wr2, _ = syn.synthetic_inputs(2, seed=7, device=DEV)
    return sd, wr2, wr2[:1].contiguous(), np.load(FIXTURE)


def _same(first, again, what):
    bad = [k for k in first if not torch.equal(first[k], again[k])]
    assert not bad, f"{what}: differs from the first run in {bad}"


def test_render_8x8x24_b2_repeats(setup):
    sd, wr2, _, _ = setup
    r = _renderer(sd, 8, 24)
    cam = generate_camera_params(8, DEV, locations=torch.tensor([[0.2, -0.15], [-0.25, 0.1]], device=DEV))
    first = None
    with torch.no_grad():
        for i in range(REPEATS):
            o = r(cam[0], cam[1], cam[2], cam[3], styles=wr2)
            o = {k: o[k].clone() for k in OUT_KEYS}
            if first is None:
                first = o
                assert all(bool(torch.isfinite(v).all()) for v in first.values())
            else:
                _same(first, o, f"8x8x24 B=2, repeat {i}")


def test_render_64x64x18_repeats_and_fixture(setup):
    sd, _, wr1, ref = setup
    r = _renderer(sd, 64, 18)
    cam = generate_camera_params(64, DEV, locations=torch.tensor([[0.1, 0.05]], device=DEV))
    first = None
    with torch.no_grad():
        for i in range(REPEATS):
            o = r(cam[0], cam[1], cam[2], cam[3], styles=wr1)
            o = {k: o[k].clone() for k in OUT_KEYS}
            if first is None:
                first = o
            else:
                _same(first, o, f"64x64x18, repeat {i}")
    bad = [k for k in OUT_KEYS if not np.array_equal(_digest(first[k]), ref["wide_" + k + "_sha256"])]
    bad += [k for k in ('gen_thumb_imgs', 'depth') if not torch.equal(first[k].cpu(), torch.from_numpy(ref["wide_" + k]))]
    assert not bad, f"64x64x18: not the fixture's values: {bad}"


def test_two_pass_8x8x24_repeats_and_fixture(setup):
    sd, _, wr1, ref = setup
    assert os.environ.get("E3DGE_REUSE_BACKBONE", "1") != "0", "the pair needs the backbone hand-over"
    rl = _renderer(sd, 8, 24, local=True)
    cam = generate_camera_params(8, DEV, locations=torch.tensor([[-0.1, 0.2]], device=DEV))
    feats = syn.synthetic_local_feats(1, 8, 24, device=DEV)
    first = None
    with torch.no_grad():
        for i in range(REPEATS):
            p1 = rl(cam[0], cam[1], cam[2], cam[3], styles=wr1)
            o = {"pass1_" + k: p1[k].clone() for k in OUT_KEYS}
            rec = vr._BACKBONE.get(rl)
            assert rec is not None and rec['buf'] is not None, "the first pass left no layer-7 record"
            o["pass1_record"] = rec['buf'].clone()
            p2 = rl(cam[0], cam[1], cam[2], cam[3], styles=wr1, local_data_batch={'feats': feats})
            o.update({"pass2_" + k: p2[k].clone() for k in ('gen_thumb_imgs', 'features')})
            if first is None:
                first = o
            else:
                _same(first, o, f"two passes 8x8x24, repeat {i}")
    vr.release_record_buffers(rl)
    bad = [k for k in first if k != "pass1_record" and not torch.equal(first[k].cpu(), torch.from_numpy(ref[k]))]
    if not np.array_equal(_digest(first["pass1_record"]), ref["pass1_record_sha256"]):
        bad.append("pass1_record")
    assert not bad, f"two passes 8x8x24: not the fixture's values: {bad}"
