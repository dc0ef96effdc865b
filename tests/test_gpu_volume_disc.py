"""GPU: the camera-pose predictor on the kernel of csrc/volume_disc.hip -- vdisc_conv_kernel through its debug entry in every form at the
smallest shapes where it can go wrong, the whole network at sizes 16 to 128 against the float64 torch composition and against the recording
of the reference (tests/golden/volume_disc.npz), bit reproducibility, batch independence, the weight cache, the dispatch rules and
image2camsettings.

Bound, per tensor (tests/test_encoder_host.parity_bound): max|hip - f64| <= max(2e-6 max|f64|, 3 max|f32 - f64|) with f32 and f64 the CPU
composition; against the recording the last factor is 4.  Outputs are pre-filled with NaN.  Every error is recorded with conftest.record.

Tile widths (ig_tile_width counts two images): a 16-channel layer runs one 16-pixel tile per workgroup up to 2048 pixels and two from 4096
(c3_64x64); the four-wide tile needs two channel blocks at 4096 pixels (c3_64x64_cout80, and the stem and the first block of the network at
size 64 and 128)."""
import copy
import functools
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, record

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, synthetic as syn, volume_discriminator as vd
from e3dge_amd.camera_utils import generate_camera_params
from e3dge_amd.volume_discriminator import AddCoords, VolumeRenderDiscriminator, image2camsettings
import test_volume_disc_host as host
from test_encoder_host import parity_bound
from test_idloss_host import tap_samples

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEM, CONV, CONV_POOL, SKIP, FINAL = _lib.VDISC_FORM_STEM, _lib.VDISC_FORM_CONV, _lib.VDISC_FORM_CONV_POOL, _lib.VDISC_FORM_SKIP, _lib.VDISC_FORM_FINAL
READ, POOL = _lib.VDISC_SKIP_READ, _lib.VDISC_SKIP_POOL


def rnd(rs, *shape, scale=1.0):
    return torch.from_numpy((scale * rs.standard_normal(shape)).astype(np.float32))


def dist(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def g(t):
    return None if t is None else t.to(DEV).contiguous()


def new_module_gpu(size, variant=None):
    """A private network on the GPU with the CPU module's values."""
    m = VolumeRenderDiscriminator(syn.model_opt(renderer_spatial_output_dim=size))
    m.load_state_dict(host.module_cpu(size, variant).state_dict(), strict=True)
    m = m.to(DEV).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


@functools.lru_cache(maxsize=None)
def module_gpu(size, variant=None):
    """Shared, never modified."""
    return new_module_gpu(size, variant)


# ---- 1. vdisc_conv_kernel ---------------------------------------------------------------------------------------------------------------
# name: (form, skip mode, cin, cout, (h, w), batch)
LAUNCH = {
    "c3_4x4": (CONV, 0, 3, 16, (4, 4), 2),                           # K = 45: two staged tiles, the second partial; coordinate taps in the padding
    "c6_6x10_cout80": (CONV, 0, 6, 80, (6, 10), 2),                  # non-square; 60 pixels: a partial last tile; a full channel block + 16 rows (IDLE waves)
    "c34_8x8": (CONV, 0, 34, 16, (8, 8), 2),                         # K = 324: ten and a bit staged tiles
    "c3_32x32": (CONV, 0, 3, 16, (32, 32), 2),
    "c3_64x64": (CONV, 0, 3, 16, (64, 64), 2),                       # two pixel tiles per workgroup
    "c3_64x64_cout80": (CONV, 0, 3, 80, (64, 64), 2),                # four pixel tiles per workgroup
    "pool_read_4x4": (CONV_POOL, READ, 16, 16, (4, 4), 2),           # exactly one quad-ordered tile
    "pool_read_6x10": (CONV_POOL, READ, 16, 16, (6, 10), 2),         # 15 quads: a partial quad tile
    "pool_identity_8x8": (CONV_POOL, POOL, 80, 80, (8, 8), 2),       # the block input pooled in the epilogue
    "skip_16_80_6x10": (SKIP, 0, 16, 80, (6, 10), 2),                # 1x1 on the pooled gather
    "stem_6x10": (STEM, 0, 3, 80, (6, 10), 2),                       # 1x1, K = 3, with activation
    "final_2x2": (FINAL, 0, 80, 3, (2, 2), 3),                       # 2x2 without padding, M = 3: the float64 dot-product kernel
}
COORD = (CONV, CONV_POOL)


def extrapolated_coords(x):
    """cat(x, yy, xx) already padded by one pixel, the coordinates continued into the padding (what the reference does NOT do)."""
    n, _, h, w = x.shape
    yy = (torch.arange(-1, h + 1, dtype=torch.float32) / (h - 1) * 2 - 1).to(x.dtype).reshape(1, 1, h + 2, 1).expand(n, 1, h + 2, w + 2)
    xx = (torch.arange(-1, w + 1, dtype=torch.float32) / (w - 1) * 2 - 1).to(x.dtype).reshape(1, 1, 1, w + 2).expand(n, 1, h + 2, w + 2)
    return torch.cat((F.pad(x, [1] * 4), yy, xx), dim=1)


def launch_reference(t, form, skip_mode, extrapolate=False, pre=False):
    """The torch composition of one launch, in the dtype of its tensors (the coordinates are AddCoords' float32 values in both)."""
    x, w, b = t["x"], t["w"], t["b"].reshape(1, -1, 1, 1)
    if form in COORD:
        y = F.conv2d(extrapolated_coords(x), w) if extrapolate else F.conv2d(AddCoords()(x), w, padding=1)
    elif form == SKIP:
        y = F.conv2d(F.avg_pool2d(x, 2), w)
    else:
        y = F.conv2d(x, w)
    y = y + b
    if pre or form in (SKIP, FINAL):
        return y
    y = F.leaky_relu(y, 0.2)
    if form == CONV_POOL:
        y = (F.avg_pool2d(y, 2) + (t["skip"] if skip_mode == READ else F.avg_pool2d(t["skip"], 2))) / math.sqrt(2)
    return y


@functools.lru_cache(maxsize=None)
def launch_case(name):
    """The tensors of a case of LAUNCH with its float64 and float32 CPU results; the liveness conditions are asserted here."""
    form, skip_mode, cin, cout, (h, w), n = LAUNCH[name]
    rs = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    ks = 3 if form in COORD else 2 if form == FINAL else 1
    cw = cin + (2 if form in COORD else 0)
    gain = 2.0 if form == SKIP else 1.0                              # (the skip reads a four-pixel average: half the deviation)
    t = dict(x=rnd(rs, n, cin, h, w), w=rnd(rs, cout, cw, ks, ks, scale=gain * math.sqrt(2.0 / (cw * ks * ks))), b=rnd(rs, cout, scale=0.1), skip=None)
    if form == CONV_POOL:
        t["skip"] = rnd(rs, n, cout, h // 2, w // 2) if skip_mode == READ else rnd(rs, n, cout, h, w, scale=2.0)
    d = {k: None if v is None else v.double() for k, v in t.items()}
    f64, f32 = launch_reference(d, form, skip_mode), launch_reference(t, form, skip_mode)
    oh, ow = {STEM: (h, w), CONV: (h, w), CONV_POOL: (h // 2, w // 2), SKIP: (h // 2, w // 2), FINAL: (h - 1, w - 1)}[form]
    assert tuple(f64.shape) == (n, cout, oh, ow)
    assert float(f64.std()) > 0.5                                    # He-scaled weights: a zero output cannot pass
    if form in (STEM, CONV, CONV_POOL):
        positive = float((launch_reference(d, form, skip_mode, pre=True) > 0).double().mean())
        assert 0.10 <= positive <= 0.90, positive                    # each leaky_relu branch holds at least 10 % of the pre-activations
    return t, f64, f32, (oh, ow)


def run_launch(name, t, shape):
    form, skip_mode, cin, cout, (h, w), n = LAUNCH[name]
    out = torch.full(shape, float('nan'), device=DEV)
    k = {STEM: cin, CONV: 9 * (cin + 2), CONV_POOL: 9 * (cin + 2), SKIP: cin, FINAL: 4 * cin}[form]
    floats = cout * k if form == FINAL else (cout + 15) // 16 * 16 * ((k + 31) // 32 * 32)
    wfrag = torch.empty(floats, device=DEV)
    _lib.launch("e3dge_vdisc_conv", out, g(t["x"]), g(t["w"]), g(t["b"]), g(t["skip"]), wfrag, floats, n, cin, cout, h, w, form, skip_mode)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("name", sorted(LAUNCH))
def test_conv_kernel(name):
    form, skip_mode, cin, cout, (h, w), n = LAUNCH[name]
    t, f64, f32, (oh, ow) = launch_case(name)
    got = run_launch(name, t, (n, cout, oh, ow))
    bound = parity_bound(f64, f32)
    if name == "c3_4x4":
        # zero in the padding against coordinates continued into it (-1.67 at 4 x 4): some border output must tell the two apart
        other = launch_reference({k: None if v is None else v.double() for k, v in t.items()}, form, skip_mode, extrapolate=True)
        border = torch.ones((oh, ow), dtype=torch.bool)
        border[1:-1, 1:-1] = False
        assert torch.equal(other[:, :, ~border], f64[:, :, ~border]) or float((other - f64)[:, :, ~border].abs().max()) <= 1e-12
        assert float((other - f64)[:, :, border].abs().max()) > 100 * bound
    err = dist(got, f64)
    record("volume_disc_conv_kernel", case=name, err=err, bound=bound, f32_err=dist(f32, f64), top=float(f64.abs().max()))
    print(name, dict(err=err, bound=bound))
    assert not torch.isnan(got).any()
    assert err <= bound, (name, err, bound)


# ---- 2. the whole network ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cpu_runs(size, B, variant):
    """(float64, float32) CPU compositions of a case: (logits, viewpoints, taps) each; computed once, never modified."""
    m = host.module_cpu(size, variant)
    x = host.golden_images(B, size)
    with torch.no_grad():
        f32 = m.run(x, taps=True)
        f64 = copy.deepcopy(m).double().run(x.double(), taps=True)
    return f64, f32


@functools.lru_cache(maxsize=None)
def hip_run(size, B, variant):
    m = module_gpu(size, variant)
    x = host.golden_images(B, size).to(DEV)
    assert m.uses_hip(x)
    logits, views, taps = m.run(x, taps=True)
    torch.cuda.synchronize()
    return logits.cpu(), views.cpu(), [t.cpu() for t in taps]


def named(run):
    logits, views, taps = run
    return dict(logits=logits, viewpoints=views, **{host.tap_name(i): t for i, t in enumerate(taps)})


@pytest.mark.parametrize("variant", host.VARIANTS, ids=["init", "wide"])
@pytest.mark.parametrize("case", host.CASES, ids=host.case_id)
def test_network_against_float64_and_the_recording(case, variant):
    size, B = case
    f64, f32 = (named(r) for r in cpu_runs(size, B, variant))
    got = named(hip_run(size, B, variant))
    gold, key = load_golden("volume_disc"), host.case_id(case, variant) + "/"
    assert got["logits"].shape == (B, 1) and got["viewpoints"].shape == (B, 2)
    if B >= 2:                                                       # a kernel that ignores the image cannot pass
        v = f64["viewpoints"]
        apart = min(float((v[i] - v[j]).abs().max()) for i in range(B) for j in range(i))
        assert apart >= 1000 * parity_bound(v, f32["viewpoints"], 4), (apart, parity_bound(v, f32["viewpoints"], 4))
    failed = []
    for k in f64:
        assert got[k].shape == f64[k].shape and not torch.isnan(got[k]).any(), k
        err, bound = dist(got[k], f64[k]), parity_bound(f64[k], f32[k])
        name = "tap_" + k if k not in ("logits", "viewpoints") else k
        rec = torch.from_numpy(gold[key + name])
        mine = got[k] if name == k else got[k].reshape(-1)[tap_samples(got[k].numel())]
        err_rec, bound_rec = dist(mine, rec), parity_bound(f64[k], f32[k], 4)
        record("volume_disc_network", case=host.case_id(case, variant), tensor=k, err=err, bound=bound, err_recording=err_rec, bound_recording=bound_rec,
               f32_err=dist(f32[k], f64[k]), top=float(f64[k].abs().max()))
        print(host.case_id(case, variant), k, dict(err=err, bound=bound, err_recording=err_rec, bound_recording=bound_rec))
        if err > bound or err_rec > bound_rec:
            failed.append((k, err, bound, err_rec, bound_rec))
    assert not failed, failed


# ---- 3. reproducibility and independence ------------------------------------------------------------------------------------------------
def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("size", [16, 64])
def test_bit_reproducible_and_batch_independent(size):
    m = module_gpu(size, 'wide')
    x = host.golden_images(3, size).to(DEV)
    first = named(m.run(x, taps=True))
    again = named(m.run(x, taps=True))
    for k in first:
        assert bits_equal(first[k], again[k]), k
    for i in range(3):
        alone = named(m.run(x[i:i + 1].clone(), taps=True))
        for k in first:
            assert bits_equal(alone[k], first[k][i:i + 1]), (k, i)
    pair = m(x[:2])                                                  # forward(): the pair, without taps
    assert isinstance(pair, tuple) and len(pair) == 2 and bits_equal(pair[0], first["logits"][:2]) and bits_equal(pair[1], first["viewpoints"][:2])


def test_weight_cache_and_invalidate():
    m = new_module_gpu(16, 'wide')
    x = host.golden_images(2, 16).to(DEV)
    image = m.packed(x.device)
    assert m.packed(x.device) is image and image.numel() == _lib.query("e3dge_vdisc_packed_floats", 16)
    base = m(x)[1].clone()
    m.final_conv.conv.bias.data[1] += 1.0                            # a write through .data is not seen ...
    assert m.packed(x.device) is image and bits_equal(m(x)[1], base)
    m.invalidate()                                                   # ... until the cache is dropped
    assert m.packed(x.device) is not image
    moved = m(x)[1]
    assert dist(moved[:, 0], base[:, 0] + 1.0) <= 1e-6 and bits_equal(moved[:, 1].contiguous(), base[:, 1].contiguous())
    with torch.no_grad():
        m.final_conv.conv.bias[1] -= 1.0                             # an in-place write bumps the version: a new image by itself
    assert bits_equal(m(x)[1], base)
    cpu = VolumeRenderDiscriminator(syn.model_opt(renderer_spatial_output_dim=16)).eval()
    for p in cpu.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match="VolumeRenderDiscriminator weights"):
        cpu.forward_hip(x)                                           # weights on another device: refused, not followed


def test_torch_backend_and_cpu_inputs_take_the_torch_path(monkeypatch):
    m = module_gpu(16, 'wide')
    x = host.golden_images(2, 16)
    names = []
    real = _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda name, *a: (names.append(name), real(name, *a))[1])
    hip = m(x.to(DEV))
    assert "e3dge_vdisc_forward" in names
    del names[:]
    monkeypatch.setenv("E3DGE_VOLUME_DISC", "torch")
    assert not m.uses_hip(x.to(DEV))
    eager = m(x.to(DEV))
    monkeypatch.delenv("E3DGE_VOLUME_DISC")
    on_cpu = host.module_cpu(16, 'wide')(x)
    torch.cuda.synchronize()
    assert not [n for n in names if n.startswith("e3dge_vdisc")]
    f64, f32 = (named(r) for r in cpu_runs(16, 2, 'wide'))
    assert torch.equal(on_cpu[1], f32["viewpoints"]) and on_cpu[1].device.type == "cpu"
    for got, k in zip(eager, ("logits", "viewpoints")):
        assert got.device.type == "cuda" and dist(got, f64[k]) <= 10 * parity_bound(f64[k], f32[k]) + 1e-5 * float(f64[k].abs().max()), k
        assert dist(got, hip[("logits", "viewpoints").index(k)]) <= 1e-4 * float(f64[k].abs().max())


# ---- 4. image2camsettings -----------------------------------------------------------------------------------------------------------------
def test_image2camsettings_on_the_gpu_and_one_render():
    from e3dge_amd.stylesdf_model import G_pred_latents
    res, n_samples, B = 8, 18, 2                                      # the smallest renderer fixture (tests/golden/renderer_8x18.npz)
    m = module_gpu(64, 'wide')
    big = F.interpolate(host.golden_images(B, 64), scale_factor=4, mode="bilinear", align_corners=False).contiguous()
    cam = image2camsettings(m, big.to(DEV), host.CAMERA, res)
    torch.cuda.synchronize()
    c = host.CAMERA
    settings = lambda loc: generate_camera_params(res, "cpu", B, locations=loc, uniform=c.uniform, azim_range=c.azim, elev_range=c.elev, fov_ang=c.fov,
                                                  dist_radius=c.dist_radius, return_calibs=True)
    cpu = host.module_cpu(64, 'wide')
    with torch.no_grad():
        thumb = F.adaptive_avg_pool2d(big.double(), (64, 64))
        want = settings(copy.deepcopy(cpu).double()(thumb)[1].float())      # (generate_camera_params computes in float32: the float64 locations, rounded once)
        f32 = settings(cpu(F.adaptive_avg_pool2d(big, (64, 64)))[1])
    assert set(cam) == set(want)
    for k in ("poses", "focal", "near", "far", "calibs", "extrinsics", "viewpoint", "locations"):
        assert cam[k].device.type == "cuda" and cam[k].shape == want[k].shape, k
        err, bound = dist(cam[k], want[k]), parity_bound(want[k].double(), f32[k])
        record("volume_disc_image2camsettings", tensor=k, err=err, bound=bound)
        print(k, dict(err=err, bound=bound))
        assert err <= bound, (k, err, bound)
    gen = G_pred_latents(syn.model_opt(size=64, channel_multiplier=1, renderer_spatial_output_dim=res), syn.rendering_opt(N_samples=n_samples),
                         full_pipeline=False)
    syn.load_synthetic(gen)
    gen = gen.to(DEV).eval().requires_grad_(False)
    wr = syn.synthetic_inputs(B, seed=6, device=DEV)[0]
    with torch.no_grad():
        out = gen([wr], cam["poses"], cam["focal"], cam["near"], cam["far"], input_is_latent=True, renderer_only=True)
    torch.cuda.synchronize()
    assert out["features"].shape[0] == B and bool(torch.isfinite(out["features"]).all())
