"""GPU: the 2-D residual aligner on the kernels of csrc/aligner.hip -- aln_conv_kernel and aln_up2_kernel through their debug entries at
the smallest shapes where they can go wrong, the whole network at 256^2 against the float64 torch composition and against the recording
of the reference (tests/golden/aligner.npz), bit reproducibility, batch independence, align(), the weight cache and the dispatch rules.

Bound, per tensor (tests/test_gpu_encoder.py): max|hip - f64| <= max(2e-6 max|f64|, 3 max|f32 - f64|) with f32 and f64 the CPU composition;
against the recording the last factor is 4.  Outputs are pre-filled with NaN.  Every error is recorded with conftest.record."""
import copy
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, record

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, synthetic as syn
from e3dge_amd.alignment import ResidualAligner
import test_aligner_host as host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rnd(rs, *shape, scale=1.0):
    return torch.from_numpy((scale * rs.standard_normal(shape)).astype(np.float32))


def dist(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def g(t):
    return None if t is None else t.to(DEV).contiguous()


def new_module_gpu(weights=0):
    """A private aligner on the GPU with the CPU module's values."""
    m = ResidualAligner(syn.aligner_opt())
    m.load_state_dict(host.module_cpu(seed=weights).state_dict(), strict=True)
    m = m.to(DEV).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


@functools.lru_cache(maxsize=None)
def module_gpu():
    """Shared, never modified."""
    return new_module_gpu()


# ---- 1. aln_conv_kernel ---------------------------------------------------------------------------------------------------------------
# name: (cin, split, up4, cout, (h, w), ksize, stride, leading affine, trailing affine, PReLU, shortcut mode).  Every case has B = 2.
# cout 3 / 16 / 32 / 48 / 64: one to four channel tiles, the partial tile 3 and the three-tile 48.  K 27 (under one staged tile), 54, 16 and
# 112 (1x1), 1008 (31.5 tiles).  Planes: (3, 3) fewer pixels than a tile, (5, 7), (9, 13) odd with stride 2 and a partial last tile,
# (32, 32); (128, 128) is the one plane here past aln_tile_width's threshold (two pixel tiles per wave).
CONV = {
    "k27_cout3_affine_prelu": (3, 3, 0, 3, (3, 3), 3, 1, True, True, True, 0),
    "k54_stem_up4": (6, 3, 1, 16, (32, 32), 3, 1, False, True, True, 0),
    "k54_stride2_odd_read": (6, 6, 0, 32, (9, 13), 3, 2, True, True, False, 2),
    "k16_1x1_stride2": (16, 16, 0, 32, (9, 13), 1, 2, False, True, False, 0),
    "k112_1x1_two_sources": (112, 64, 0, 64, (5, 7), 1, 1, False, True, False, 0),
    "k1008_two_sources": (112, 64, 0, 64, (32, 32), 3, 1, True, False, True, 0),
    "k72_cout48_stride2_pick": (8, 5, 0, 48, (9, 13), 3, 2, True, True, False, 1),
    "k72_cout48_up4_affine": (8, 5, 1, 48, (32, 32), 3, 1, True, False, True, 0),
    "k27_cout3_pick": (3, 3, 0, 3, (5, 7), 3, 1, False, True, False, 1),
    "k16_1x1_cout3": (16, 16, 0, 3, (3, 3), 1, 1, False, True, False, 0),
    "k27_two_pixel_tiles": (3, 0, 0, 16, (128, 128), 3, 1, True, True, True, 2),
}


def conv_reference(t, ks, stride, mode):
    """The torch composition of one launch, in the dtype of its tensors."""
    x = t["in0"] if t["in1"] is None else t["in1"] if t["in0"] is None else None
    if x is None:
        second = t["in1"]
        if second.shape[-1] != t["in0"].shape[-1]:
            second = F.interpolate(second, size=t["in0"].shape[-2:])                 # nearest, as the call site (e3dge_full_runner.py:255)
        x = torch.cat((t["in0"], second), dim=1)
    if t["in_ab"] is not None:
        x = x * t["in_ab"][:, 0].reshape(1, -1, 1, 1) + t["in_ab"][:, 1].reshape(1, -1, 1, 1)       # before the zero padding, as a leading BN
    y = F.conv2d(x, t["w"], stride=stride, padding=1 if ks == 3 else 0)
    if t["epi_ab"] is not None:
        y = y * t["epi_ab"][:, 0].reshape(1, -1, 1, 1) + t["epi_ab"][:, 1].reshape(1, -1, 1, 1)
    if t["slope"] is not None:
        y = F.prelu(y, t["slope"])
    if mode == 1:
        y = y + t["shortcut"][:, :, ::stride, ::stride]
    elif mode == 2:
        y = y + t["shortcut"]
    return y


def conv_case(name):
    """The tensors of a case of CONV with its float64 and float32 CPU results; the liveness conditions are asserted here."""
    cin, split, up4, cout, (h, w), ks, stride, lead, trail, prelu, mode = CONV[name]
    n = 2
    rs = np.random.RandomState(zlib_seed(name))
    oh, ow = (h + (2 if ks == 3 else 0) - ks) // stride + 1, (w + (2 if ks == 3 else 0) - ks) // stride + 1
    t = dict(in0=rnd(rs, n, split, h, w) if split else None,
             in1=(rnd(rs, n, cin - split, h // 4, w // 4) if up4 else rnd(rs, n, cin - split, h, w)) if split < cin else None,
             w=rnd(rs, cout, cin, ks, ks, scale=math.sqrt(2.0 / (cin * ks * ks))), in_ab=None, epi_ab=None, slope=None, shortcut=None)
    if lead:                                                         # |b| >= 0.3: an affine applied to a padded tap would show on the border
        sign = torch.from_numpy(rs.choice([-1.0, 1.0], size=cin).astype(np.float32))
        t["in_ab"] = torch.stack((1.0 + 0.2 * rnd(rs, cin), sign * (0.3 + 0.3 * rnd(rs, cin).abs())), dim=1)
        assert float(t["in_ab"][:, 1].abs().min()) >= 0.3
    if trail:
        t["epi_ab"] = torch.stack((1.0 + 0.2 * rnd(rs, cout), 0.1 * rnd(rs, cout)), dim=1)
    if prelu:
        t["slope"] = torch.from_numpy(rs.uniform(0.05, 0.5, size=cout).astype(np.float32))
    if mode:
        t["shortcut"] = rnd(rs, n, cout, h, w) if mode == 1 else rnd(rs, n, cout, oh, ow)
    f64 = conv_reference({k: None if v is None else v.double() for k, v in t.items()}, ks, stride, mode)
    f32 = conv_reference(t, ks, stride, mode)
    assert tuple(f64.shape) == (n, cout, oh, ow)
    assert float(f64.std()) > 0.5                                    # a zero output cannot pass
    if prelu:
        pre = conv_reference({**{k: None if v is None else v.double() for k, v in t.items()}, "slope": None, "shortcut": None}, ks, stride, 0)
        positive = float((pre > 0).double().mean())
        assert 0.10 <= positive <= 0.90, positive                    # each branch holds at least 10 % of the outputs
    return t, f64, f32, (oh, ow)


@pytest.mark.parametrize("name", sorted(CONV))
def test_conv_kernel(name):
    cin, split, up4, cout, (h, w), ks, stride, _, _, _, mode = CONV[name]
    n = 2
    t, f64, f32, (oh, ow) = conv_case(name)
    out = torch.full((n, cout, oh, ow), float('nan'), device=DEV)
    floats = (cout + 15) // 16 * 16 * ((cin * ks * ks + 31) // 32 * 32)
    wfrag = torch.empty(floats, device=DEV)
    _lib.launch("e3dge_aln_conv", out, g(t["in0"]), g(t["in1"]), g(t["w"]), g(t["in_ab"]), g(t["epi_ab"]), g(t["slope"]), g(t["shortcut"]), wfrag, floats,
                n, cin, split, up4, cout, h, w, ks, stride, mode)
    torch.cuda.synchronize()
    got = out.cpu()
    bound = host.parity_bound(f64, f32)
    border = torch.ones((oh, ow), dtype=torch.bool)
    border[1:-1, 1:-1] = False
    rec = dict(err=dist(got, f64), f32=dist(f32, f64), bound=bound, border_err=dist(got[..., border], f64[..., border]),
               interior_err=dist(got[..., ~border], f64[..., ~border]) if (~border).any() else 0.0, std=float(f64.std()))
    record("aligner_conv", case=name, **rec)
    print(name, {k: f"{v:.2e}" for k, v in rec.items()})
    assert not bool(torch.isnan(got).any())
    assert rec['interior_err'] <= bound, rec
    assert rec['border_err'] <= bound, rec                           # an affine on a padded tap, a wrong pad or stride shows here


def zlib_seed(name):
    import zlib
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


# ---- 2. aln_up2_kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (32, 32)], ids=str)
def test_up2_kernel(hw):
    n, c = 2, 3
    rs = np.random.RandomState(400 + hw[0])
    x = rnd(rs, n, c, *hw)
    size = (2 * hw[0], 2 * hw[1])
    f64, f32 = F.interpolate(x.double(), size=size, mode='bilinear'), F.interpolate(x, size=size, mode='bilinear')
    out = torch.full((n, c) + size, float('nan'), device=DEV)
    _lib.launch("e3dge_aln_up2", out, g(x), n * c, hw[0], hw[1])
    torch.cuda.synchronize()
    rec = dict(err=dist(out, f64), f32=dist(f32, f64), bound=host.parity_bound(f64, f32))
    record("aligner_up2", case=str(hw), **rec)
    print(hw, {k: f"{v:.2e}" for k, v in rec.items()})
    assert float(f64.std()) > 0.5
    assert not bool(torch.isnan(out).any())
    assert rec['err'] <= rec['bound'], rec


# ---- 3. the whole network -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gpu_results(n):
    """The output and the seven taps of the leading n images of the recorded input, twice; computed once, never modified."""
    gn, seed = host.GOLDEN_CASE
    x = host.aligner_input(gn, seed)[:n].to(DEV)
    m = module_gpu()
    assert m._runs_hip(x)
    runs = []
    for _ in range(2):
        taps = {}
        with torch.no_grad():
            out = m.forward_hip(x, taps=taps)
        runs.append(dict(out=out, **taps))
    torch.cuda.synchronize()
    return runs


@pytest.mark.parametrize("n", [1, 2])
def test_whole_network_against_float64(n):
    gn, seed = host.GOLDEN_CASE
    t64, t32 = host.cpu_results(gn, seed)
    got = gpu_results(n)[0]
    with torch.no_grad():
        assert torch.equal(module_gpu()(host.aligner_input(gn, seed)[:n].to(DEV)), got["out"])      # forward() is that path
    worst = []
    for k in host.TENSORS:
        a, b = t64[k][:n], t32[k][:n]                                # (an image's CPU values: the composition has no cross-image term in eval)
        assert got[k].shape == a.shape and got[k].dtype == torch.float32, k
        rec = dict(err=dist(got[k], a), f32=dist(b, a), bound=host.parity_bound(a, b), std=float(a.std()))
        record("aligner_network", batch=n, tensor=k, over_bound=rec['err'] / rec['bound'], **rec)
        print(n, k, {q: f"{v:.2e}" for q, v in rec.items()})
        assert rec['std'] > 0.5, (k, rec)                            # alive
        assert not bool(torch.isnan(got[k]).any()), k
        if rec['err'] > rec['bound']:
            worst.append((k, rec))
    assert not worst, worst
    assert torch.equal(got["out"], got["dfea3"])


def test_whole_network_against_the_recording():
    gold = load_golden("aligner")
    n, _ = host.GOLDEN_CASE
    got = gpu_results(n)[0]
    worst = []
    for k in host.TENSORS:
        t = got[k].cpu()
        flat = t.reshape(-1)
        f64_max, f32_err = float(gold[f"{k}_f64_max"]), float(gold[f"{k}_err"])
        bound = max(2e-6 * f64_max, 4 * f32_err)
        err = float(np.abs(flat[host.samples(flat.numel())].double().numpy() - gold[f"{k}_f64"]).max())
        # the sum: independent errors of at most `bound` per element add up to about sqrt(numel) bound; the reference's own fp32 sum is
        # |f32 sum - f64 sum| away.  Four times the larger of the two (tests/test_gpu_encoder.py).
        sum_err = abs(float(t.double().sum()) - float(gold[f"{k}_f64_sum"]))
        sum_bound = 4 * max(abs(float(gold[f"{k}_f32_sum"]) - float(gold[f"{k}_f64_sum"])), math.sqrt(flat.numel()) * bound)
        rec = dict(err=err, bound=bound, f32=f32_err, sum_err=sum_err, sum_bound=sum_bound)
        record("aligner_network_recording", tensor=k, **rec)
        print(k, {q: f"{v:.2e}" for q, v in rec.items()})
        if err > bound or sum_err > sum_bound:
            worst.append((k, rec))
    assert not worst, worst


def test_two_runs_are_bit_identical_and_an_image_does_not_depend_on_the_batch():
    first, second = gpu_results(2)
    alone = gpu_results(1)[0]
    for k in host.TENSORS:
        assert torch.equal(first[k], second[k]), k
        assert torch.equal(first[k][:1], alone[k]), k
    assert float(first["out"][1].std()) > 0 and not torch.equal(first["out"][0], first["out"][1])


# ---- 4. align() ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thumb_size", [64, 256])
def test_align_equals_the_composed_native_call(thumb_size, monkeypatch):
    m = module_gpu()
    x = host.aligner_input(2, 5)
    res_gt = x[:, :3].contiguous().to(DEV)
    thumb = (x[:, 3:, ::4, ::4] if thumb_size == 64 else x[:, 3:]).contiguous().to(DEV)
    with torch.no_grad():
        composed = torch.cat((res_gt, F.interpolate(thumb, (256, 256))), dim=1)
        assert m._runs_hip(composed) and m._runs_hip(res_gt, thumb)
        want = m(composed)
        monkeypatch.setattr(torch, "cat", None)                      # nothing is concatenated or up-sampled on the native path
        monkeypatch.setattr(F, "interpolate", None)
        got = m.align(res_gt, thumb)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and float(got.std()) > 0.5 and not bool(torch.isnan(got).any())


# ---- 5. the weight cache --------------------------------------------------------------------------------------------------------------
def test_weight_cache_follows_the_weights():
    """load_state_dict and an in-place edit bump the parameters' versions: the packed image is rebuilt.  A write through `.data` bumps
    nothing: the old image is served until invalidate()."""
    x = host.aligner_input(1, 7)
    xg = x.to(DEV)
    m = new_module_gpu()
    ref = copy.deepcopy(host.module_cpu())                           # a private CPU twin that takes the same edits

    def check(step):
        with torch.no_grad():
            got = m(xg)
            t64, t32 = copy.deepcopy(ref).double()(x.double()), ref(x)
        torch.cuda.synchronize()
        rec = dict(err=dist(got, t64), f32=dist(t32, t64), bound=host.parity_bound(t64, t32))
        record("aligner_weight_cache", step=step, **rec)
        return got, rec

    with torch.no_grad():
        before = m(xg)                                               # (against float64: test_whole_network_against_float64)
    second = host.module_cpu(seed=1).state_dict()
    m.load_state_dict(second)
    ref.load_state_dict(second)
    loaded, rec = check("load_state_dict")
    assert rec['err'] <= rec['bound'], rec
    assert dist(loaded, before) > 100 * rec['bound']                 # the second set is a different network
    with torch.no_grad():
        m.dconv_layer3[2].res_layer[2].weight.mul_(0.25)
        ref.dconv_layer3[2].res_layer[2].weight.mul_(0.25)
    edited, rec = check("in_place")
    assert rec['err'] <= rec['bound'], rec
    assert dist(edited, loaded) > 100 * rec['bound']
    m.dconv_layer3[2].res_layer[4].bias.data.add_(1.0)
    ref.dconv_layer3[2].res_layer[4].bias.data.add_(1.0)
    with torch.no_grad():
        stale = m(xg)
    assert torch.equal(stale, edited)                                # no version moved: the cached image is served
    m.invalidate()
    fresh, rec = check("data_then_invalidate")
    assert rec['err'] <= rec['bound'], rec
    assert dist(fresh, edited) > 0.5


# ---- 6. dispatch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["train", "requires_grad", "env"])
def test_what_the_kernels_do_not_cover_runs_the_torch_layers(how, monkeypatch):
    m = new_module_gpu()
    x = host.aligner_input(1, 8).to(DEV)
    if how == "train":
        m.train()
    elif how == "requires_grad":
        m.conv_layer1[0].weight.requires_grad_(True)
    else:
        monkeypatch.setenv("E3DGE_ALIGNER", "torch")
    assert not m._runs_hip(x)
    native, torch_out = [], []
    monkeypatch.setattr(_lib, "launch", lambda name, *a: native.append(name))
    layers = m.forward_torch
    monkeypatch.setattr(m, "forward_torch", lambda *a, **k: torch_out.append(layers(*a, **k)) or torch_out[-1])
    y = m(x)
    torch.cuda.synchronize()
    assert not native and len(torch_out) == 1 and y is torch_out[0]  # the torch layers' result, and no native call
    assert tuple(y.shape) == (1, 3, 256, 256) and bool(torch.isfinite(y).all())
    assert y.requires_grad == (how == "requires_grad")
