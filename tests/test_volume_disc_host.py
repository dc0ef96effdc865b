"""The camera-pose predictor, host side: the state-dict surface of e3dge_amd.volume_discriminator.VolumeRenderDiscriminator, its torch
composition on the CPU against the recording of the reference (tests/golden/volume_disc.npz, tools/gen_golden_volume_disc.py), AddCoords
against its fp32 formula, the sizes and refusals of the C-ABI entries of csrc/volume_disc.hip, the path selection, and image2camsettings.

The CPU path is the reference's torch operations in the reference's order under oracle.cpu_numerics, so every recorded tensor -- logits,
viewpoints, taps and poses -- is reproduced bit for bit, and the test asserts that."""
import ctypes
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, build, synthetic as syn, volume_discriminator as vd
from e3dge_amd.camera_utils import generate_camera_params
from e3dge_amd.volume_discriminator import AddCoords, VolumeRenderDiscriminator, image2camsettings
from test_discriminator_host import golden_images
from test_idloss_host import tap_samples

INVALID = -1                                                        # E3DGE_ERR_INVALID_ARG
SIZES = (16, 32, 64, 128)
CASES = [(size, b) for size in (16, 32, 64) for b in (1, 2, 3)] + [(128, 1)]      # (renderer_spatial_output_dim, batch) of the recording
VARIANTS = (None, 'wide')
RENDER_SIZE = 64                                                    # renderer_output_size of the recorded poses
CAMERA = syn.rendering_opt().camera


def case_id(case, variant=None):
    return "s{}b{}".format(*case) + ("" if variant is None else "_" + variant)


def tap_name(t):
    return "stem" if t == 0 else f"block{t - 1}"


@functools.lru_cache(maxsize=None)
def module_cpu(size, variant=None):
    m = syn.load_synthetic_volume_discriminator(VolumeRenderDiscriminator(syn.model_opt(renderer_spatial_output_dim=size)), variant=variant)
    for p in m.parameters():
        p.requires_grad_(False)
    return m.eval()


# ---- the layer table, restated by hand -------------------------------------------------------------------------------------------
def channels(res):
    return 400 if res <= 16 else {32: 256, 64: 128, 128: 64}[res]


def layers(size):
    """[(name, cin, cout, K, input plane)] in launch order: the stem, per block the skip (where the channel count changes), conv1, conv2,
    then the final layer.  K counts the two coordinate channels of the 3x3 layers."""
    out, cin, res = [("stem", 3, channels(size), 3, size)], channels(size), size
    while res > 2:
        cout = channels(res // 2)
        if cin != cout:
            out.append(("skip", cin, cout, cin, res))
        out += [("conv1", cin, cout, 9 * (cin + 2), res), ("conv2", cout, cout, 9 * (cout + 2), res)]
        cin, res = cout, res // 2
    return out + [("final", cin, 3, 4 * cin, 2)]


def up(x, m):
    return (x + m - 1) // m * m


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_packed_and_workspace_sizes_equal_the_layer_table(lib, size):
    assert "volume_disc.hip" in build.SOURCES
    table = layers(size)
    assert len(table) == {16: 8, 32: 11, 64: 14, 128: 17}[size]      # = the launches of one forward
    assert [k for name, _, _, k, _ in table if name.startswith("conv")][-3:] == [3618] * 3 and (size != 64 or table[2][3] == 1170 and table[5][3] == 2322)
    # per layer: the A-fragment image (M padded to 16, K to 32), then the bias; the final layer's weight as it is
    assert lib.e3dge_vdisc_packed_floats(size) == sum((cout * k if name == "final" else up(cout, 16) * up(k, 32)) + cout for name, _, cout, k, _ in table)
    # two block inputs / outputs, one conv1 output, one skip output, each of the largest layer: no (C + 2)-channel and no second full-size tensor
    x = max([channels(size) * size * size] + [cout * (res // 2) ** 2 for name, _, cout, _, res in table if name == "conv2"])
    t = max(cout * res * res for name, _, cout, _, res in table if name == "conv1")
    s = max([cout * (res // 2) ** 2 for name, _, cout, _, res in table if name == "skip"] + [0])
    for n in (1, 3, 256):
        assert lib.e3dge_vdisc_ws_bytes(n, size) == 4 * n * (2 * x + t + s)
    m = VolumeRenderDiscriminator(syn.model_opt(renderer_spatial_output_dim=size))
    assert len(m.sources()) == 2 * len(table) and {id(p) for p in m.sources()} == {id(p) for p in m.parameters()}
    # (the sources are in state-dict order, a block's skip last; the table is in launch order, the skip first)
    assert sorted(tuple(p.shape) for p in m.sources()[::2]) == sorted((cout, cin + (2 if name.startswith("conv") else 0)) +
                                                                      {"stem": (1, 1), "skip": (1, 1), "final": (2, 2)}.get(name, (3, 3)) for name, cin, cout, _, _ in table)
    assert [k for k, v in m.state_dict().items()] == [k for k, v in m.named_parameters()] and all(a is b for a, b in zip(m.sources(), m.parameters()))
    assert m.tap_shapes(2) == [(2, channels(size), size, size)] + [(2, cout, res // 2, res // 2) for name, _, cout, _, res in table if name == "conv2"]


def test_bad_arguments_are_refused_before_any_launch(lib):
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)                                        # never followed
    err = lib.e3dge_last_error
    assert lib.e3dge_vdisc_packed_floats(48) == INVALID and b"size=48" in err()
    assert lib.e3dge_vdisc_ws_bytes(1, 48) == INVALID and lib.e3dge_vdisc_ws_bytes(0, 64) == INVALID and b"n=0" in err()
    assert lib.e3dge_vdisc_ws_bytes(257, 64) == INVALID
    ptrs = (ctypes.c_void_p * 32)(*([p] * 32))
    assert lib.e3dge_vdisc_pack_weights(p, ctypes.addressof(ptrs), 28, 48, None) == INVALID and b"size=48" in err()
    assert lib.e3dge_vdisc_pack_weights(p, ctypes.addressof(ptrs), 27, 64, None) == INVALID and b"28 source" in err()
    assert lib.e3dge_vdisc_pack_weights(None, ctypes.addressof(ptrs), 28, 64, None) == INVALID and b"null" in err()
    ptrs[5] = None
    assert lib.e3dge_vdisc_pack_weights(p, ctypes.addressof(ptrs), 28, 64, None) == INVALID and b"source 5" in err()

    def args():
        a = _lib.VdiscArgs()
        a.packed = a.images = a.logits = a.viewpoints = a.ws = p
        a.n, a.size, a.ws_bytes = 2, 64, 1 << 42
        return a

    fwd = lambda a: lib.e3dge_vdisc_forward(ctypes.byref(a), None)
    for field, value, word in [("packed", None, b"null"), ("images", None, b"null"), ("logits", None, b"null"), ("viewpoints", None, b"null"),
                               ("ws", None, b"null"), ("n", 0, b"n=0"), ("n", 257, b"n=257"), ("size", 48, b"size=48"), ("size", 8, b"size=8"),
                               ("ws_bytes", lib.e3dge_vdisc_ws_bytes(2, 64) - 1, b"workspace")]:
        a = args()
        setattr(a, field, value)
        assert fwd(a) == INVALID, field
        assert word in err(), (field, err())
    assert lib.e3dge_vdisc_forward(None, None) == INVALID

    conv = lambda n, cin, cout, h, w, form, skip_mode=0, out=p, skip=None, floats=1 << 40: lib.e3dge_vdisc_conv(out, p, p, p, skip, p, floats, n, cin, cout, h, w,
                                                                                                               form, skip_mode, None)
    assert conv(2, 3, 16, 4, 4, _lib.VDISC_FORM_CONV, out=None) == INVALID and b"null" in err()
    assert conv(0, 3, 16, 4, 4, _lib.VDISC_FORM_CONV) == INVALID and b"n=0" in err()
    assert conv(2, 3, 16, 4, 4, 5) == INVALID and b"form=5" in err()
    for form in (_lib.VDISC_FORM_CONV_POOL, _lib.VDISC_FORM_SKIP):   # odd planes in the pooled forms
        for h, w in ((5, 4), (4, 7)):
            assert conv(2, 3, 16, h, w, form, _lib.VDISC_SKIP_READ, skip=p) == INVALID and b"even" in err(), (form, h, w)
    assert conv(2, 16, 16, 4, 4, _lib.VDISC_FORM_CONV_POOL, 0, skip=p) == INVALID and b"skip_mode" in err()
    assert conv(2, 16, 16, 4, 4, _lib.VDISC_FORM_CONV_POOL, _lib.VDISC_SKIP_POOL) == INVALID and b"skip_mode" in err()
    assert conv(2, 3, 16, 1, 4, _lib.VDISC_FORM_CONV) == INVALID and b"at least 2" in err()
    assert conv(2, 3, 16, 4, 4, _lib.VDISC_FORM_CONV, floats=16 * 64 - 1) == INVALID and b"wfrag" in err()


# ---- the module -------------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_are_the_reference_ones_and_a_strict_load_works():
    recorded = json.load(open(os.path.join(GOLDEN, "volume_disc_state_dict_keys.json")))
    for size in (64, 16):
        m = VolumeRenderDiscriminator(syn.model_opt(renderer_spatial_output_dim=size))
        sd = m.state_dict()
        assert sorted(sd) == recorded[str(size)]["keys"]
        assert {k: list(v.shape) for k, v in sd.items()} == recorded[str(size)]["shapes"]
        other = VolumeRenderDiscriminator(syn.model_opt(renderer_spatial_output_dim=size))
        other.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
        assert m.in_channel == 400 and m.init_size == size and len(m.convs) == int(math.log2(size))
    # the constructor's ranges (stylesdf_model.py:1215-1219, :1326-1329)
    m = VolumeRenderDiscriminator(syn.model_opt(renderer_spatial_output_dim=64))
    b = m.convs[1].conv1.activation.bias
    assert 0.5 * math.sqrt(1 / (128 * 9)) < float(b.detach().abs().max()) <= math.sqrt(1 / (128 * 9)) * (1 + 1e-6)      # (fp32 rounding of the range's end)
    w = m.convs[1].conv1.conv.conv.weight
    assert float(w.detach().abs().max()) <= 1 / math.sqrt(130 * 9) * (1 + 1e-6) and float(m.convs[0].activation.bias.detach().abs().max()) <= math.sqrt(1 / 3) * (1 + 1e-6)


def test_synthetic_variants():
    sd = module_cpu(64).state_dict()                                 # variant None: the constructor's ranges
    for k, bound in [("convs.0.conv.weight", 1 / math.sqrt(3)), ("convs.0.activation.bias", math.sqrt(1 / 3)),
                     ("convs.1.conv1.conv.conv.weight", 1 / math.sqrt(130 * 9)), ("convs.1.conv1.activation.bias", math.sqrt(1 / (128 * 9))),
                     ("convs.1.conv2.activation.bias", math.sqrt(1 / (256 * 9))), ("convs.1.skip.conv.weight", 1 / math.sqrt(128)),
                     ("convs.1.skip.conv.bias", 1 / math.sqrt(128)), ("final_conv.conv.weight", 1 / math.sqrt(1600)), ("final_conv.conv.bias", 1 / math.sqrt(1600))]:
        assert 0.8 * bound < float(sd[k].abs().max()) <= bound * (1 + 1e-6), k
    wide = module_cpu(64, 'wide')
    taps = []
    with torch.no_grad():
        wide.forward_torch(golden_images(2, 64), taps)
    assert all(0.3 < float(t.std()) < 3.0 for t in taps), [float(t.std()) for t in taps]
    with pytest.raises(ValueError, match="variant"):
        syn.load_synthetic_volume_discriminator(VolumeRenderDiscriminator(syn.model_opt(renderer_spatial_output_dim=16)), variant='stress')


@pytest.mark.parametrize("variant", VARIANTS, ids=["init", "wide"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_cpu_path_reproduces_the_recording_bit_for_bit(case, variant):
    size, B = case
    gold, key = load_golden("volume_disc"), case_id(case, variant) + "/"
    m = module_cpu(size, variant)
    x = golden_images(B, size)
    logits, views, taps = m.run(x, taps=True)
    assert logits.shape == (B, 1) and views.shape == (B, 2) and logits.dtype == views.dtype == torch.float32
    assert np.array_equal(logits.numpy(), gold[key + "logits"]) and np.array_equal(views.numpy(), gold[key + "viewpoints"])
    assert [tuple(t.shape) for t in taps] == m.tap_shapes(B)
    for i, v in enumerate(taps):
        assert np.array_equal(v.reshape(-1)[tap_samples(v.numel())].numpy(), gold[key + "tap_" + tap_name(i)]), tap_name(i)
        assert float(v.double().sum()) == float(gold[key + "sum_" + tap_name(i)]), tap_name(i)
    out = m(x)                                                       # forward(): the reference's pair
    assert isinstance(out, tuple) and len(out) == 2 and torch.equal(out[0], logits) and torch.equal(out[1], views)
    if size == 64:
        cam = image2camsettings(m, x, CAMERA, RENDER_SIZE, is_thumb=True)
        assert np.array_equal(cam["poses"].numpy(), gold[key + "poses"])


def test_addcoords_equals_the_fp32_formula_on_a_non_square_plane():
    x = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).reshape(2, 3, 5, 7)
    out = AddCoords()(x)
    assert out.shape == (2, 5, 5, 7) and torch.equal(out[:, :3], x)
    f = np.float32
    yy = np.array([f(f(f(i) / f(4)) * f(2)) - f(1) for i in range(5)], dtype=np.float32)
    xx = np.array([f(f(f(j) / f(6)) * f(2)) - f(1) for j in range(7)], dtype=np.float32)
    assert yy.dtype == np.float32 and yy[0] == -1 and yy[-1] == 1 and xx[0] == -1 and xx[-1] == 1
    for b in range(2):
        assert np.array_equal(out[b, 3].numpy(), np.broadcast_to(yy[:, None], (5, 7)))     # yy first: constant along a row
        assert np.array_equal(out[b, 4].numpy(), np.broadcast_to(xx[None, :], (5, 7)))
    assert not np.array_equal(xx[:5], yy)


def test_path_selection(monkeypatch):
    m = module_cpu(16)
    x = golden_images(2, 16)
    monkeypatch.delenv("E3DGE_VOLUME_DISC", raising=False)
    assert vd.backend() == "hip"
    assert not m.uses_hip(x) and not m.uses_hip(x.double())          # CPU inputs

    class FakeCuda:                                                  # what uses_hip reads of a GPU tensor
        requires_grad = False

        def __init__(self, shape, dtype=torch.float32):
            self.shape, self.dtype, self.ndim, self.device = shape, dtype, len(shape), torch.device("cuda", 0)

    gpu = FakeCuda((2, 3, 16, 16))
    assert m.uses_hip(gpu)
    assert not m.uses_hip(FakeCuda((2, 3, 16, 16), torch.float64)) and not m.uses_hip(FakeCuda((2, 3, 16, 16), torch.float16))
    assert not m.uses_hip(FakeCuda((2, 3, 32, 32))) and not m.uses_hip(FakeCuda((2, 4, 16, 16))) and not m.uses_hip(FakeCuda((2, 3, 16, 8)))
    assert not m.uses_hip(FakeCuda((0, 3, 16, 16))) and not m.uses_hip(FakeCuda((3, 16, 16)))
    assert module_cpu(128).uses_hip(FakeCuda((1, 3, 128, 128)))
    monkeypatch.setenv("E3DGE_VOLUME_DISC", "torch")
    assert not m.uses_hip(gpu)
    monkeypatch.setenv("E3DGE_VOLUME_DISC", "eager")
    with pytest.raises(ValueError, match="E3DGE_VOLUME_DISC"):
        m.uses_hip(gpu)
    monkeypatch.delenv("E3DGE_VOLUME_DISC")
    m.train()
    try:
        assert not m.uses_hip(gpu)
    finally:
        m.eval()
    trainable = syn.load_synthetic_volume_discriminator(VolumeRenderDiscriminator(syn.model_opt(renderer_spatial_output_dim=16))).eval()
    assert all(p.requires_grad for p in trainable.parameters()) and not trainable.uses_hip(gpu)
    with torch.no_grad():
        assert trainable.uses_hip(gpu)                               # no gradient is wanted
    wants = FakeCuda((2, 3, 16, 16))
    wants.requires_grad = True
    assert not m.uses_hip(wants)
    # the torch composition is differentiable
    leaf = x.clone().requires_grad_(True)
    trainable(leaf)[1].sum().backward()
    assert float(leaf.grad.abs().max()) > 0 and all(p.grad is not None for p in trainable.parameters())


def test_image2camsettings_returns_the_camera_dict_of_its_locations():
    m = module_cpu(64, 'wide')
    big = torch.nn.functional.interpolate(golden_images(2, 64), scale_factor=4, mode="bilinear", align_corners=False)
    cam = image2camsettings(m, big, CAMERA, RENDER_SIZE)
    with torch.no_grad():
        _, pred = m(vd._pool_64(big))
    want = generate_camera_params(RENDER_SIZE, "cpu", 2, locations=pred, uniform=CAMERA.uniform, azim_range=CAMERA.azim, elev_range=CAMERA.elev,
                                  fov_ang=CAMERA.fov, dist_radius=CAMERA.dist_radius, return_calibs=True)
    assert set(cam) == set(want) == {"poses", "extrinsics", "focal", "near", "far", "viewpoint", "intrinsics", "calibs", "locations", "azim_range", "elev_range"}
    for k, v in want.items():
        if torch.is_tensor(v):
            assert cam[k].shape == v.shape and torch.equal(cam[k], v), k
        else:
            assert cam[k] == v, k
    assert cam["poses"].shape == (2, 3, 4) and cam["calibs"].shape == (2, 4, 4) and cam["focal"].shape == cam["near"].shape == (2, 1, 1)
    assert torch.equal(cam["locations"], pred) and not cam["locations"].requires_grad
    thumb = image2camsettings(m, golden_images(2, 64), CAMERA, RENDER_SIZE, is_thumb=True)
    with torch.no_grad():
        assert torch.equal(thumb["locations"], m(golden_images(2, 64))[1]) and not torch.equal(thumb["poses"], cam["poses"])
    with pytest.raises(AssertionError, match="volume_discriminator input img dim"):
        image2camsettings(m, golden_images(2, 32), CAMERA, RENDER_SIZE, is_thumb=True)
