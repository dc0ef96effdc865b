"""The hourglass image filter on the HIP kernels (csrc/hgfilter.hip, e3dge_amd.hg_filter) against the module's own torch composition on
the CPU -- which reproduces the recording of the reference bit for bit (tests/test_hgfilter_host.py) --: once in float64 (truth), once
in float32 (the reference's own arithmetic).

Bound, per tensor (tests/test_gpu_idloss.py):  max|hip - f64| <= max(2e-6 max|f64|, 3 max|f32 - f64|)
against the recording:                         max|hip - rec| <= max(2e-6 max|f64|, 4 max|f32 - f64|)"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, record

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, synthetic as syn
from e3dge_amd.hg_filter import ResidualImageFilter
from test_hgfilter_host import CASES, case_inputs, cpu_results, module_cpu, run_case, samples, tensor_names

DEV = "cuda:0"


def dist(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def bound_of(t64, t32, factor=3):
    return max(2e-6 * float(t64.abs().max()), factor * dist(t32, t64))


def rnd(rs, *shape, scale=1.0, shift=0.0):
    return torch.from_numpy(shift + scale * rs.standard_normal(shape)).float()


# ---- one convolution at a time ----------------------------------------------------------------------------------------------------
# name: n, Cin, Cout, H, W, kernel, stride, reflect, norm (groups or 0) + ReLU in the gather, bias, (out channels, out c0) or None: slice + residual
CONV_CASES = {
    "stem7x7s2": (2, 64, 64, 32, 48, 7, 2, False, 0, True, None),
    "3x3_256to128_4x6": (2, 256, 128, 4, 6, 3, 1, False, 32, False, None),
    "3x3_64to32_5x7": (2, 64, 32, 5, 7, 3, 1, False, 32, False, None),
    "3x3_32to32_5x7": (2, 32, 32, 5, 7, 3, 1, False, 32, False, None),
    "1x1_128to256_norm": (2, 128, 256, 5, 7, 1, 1, False, 32, False, None),
    "1x1_256to256_bias": (2, 256, 256, 5, 7, 1, 1, False, 0, True, None),
    "reflect_3to32": (2, 3, 32, 16, 24, 3, 1, True, 0, False, None),
    "reflect_1to32": (2, 1, 32, 16, 24, 3, 1, True, 0, False, None),
    "reflect_32to32_inorm": (2, 32, 32, 16, 24, 3, 1, True, 32, False, None),
    "slice_residual": (2, 64, 32, 5, 7, 3, 1, False, 32, False, (128, 64)),
    # the wider pixel tiles (ig_tile_width: 32 and 64 pixels), each with a partial last tile, and 64 pixels with two idle waves
    "3x3_128to256_33x37": (2, 128, 256, 33, 37, 3, 1, False, 32, False, None),
    "1x1_128to256_40x52": (2, 128, 256, 40, 52, 1, 1, False, 32, True, None),
    "reflect_3to32_96x97": (2, 3, 32, 96, 97, 3, 1, True, 0, False, None),
}


@functools.lru_cache(maxsize=None)
def conv_case(name):
    n, ci, co, H, W, k, s, reflect, groups, bias, sl = CONV_CASES[name]
    rs = np.random.RandomState(500 + sorted(CONV_CASES).index(name))
    d = dict(x=rnd(rs, n, ci, H, W) + rnd(rs, n, ci, 1, 1, scale=0.5), w=rnd(rs, co, ci, k, k, scale=(2.0 / (ci * k * k)) ** 0.5))
    d['gamma'], d['beta'] = (rnd(rs, ci, scale=0.2, shift=1.0), rnd(rs, ci, scale=0.2)) if groups else (None, None)     # beta != 0: relu(b) != 0
    d['bias'] = rnd(rs, co, scale=0.2) if bias else None
    OH, OW = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    d['res'] = rnd(rs, n, sl[0], OH, OW) if sl else None

    def ref(dtype):
        x = d['x'].to(dtype)
        if groups:
            x = F.relu(F.group_norm(x, groups, d['gamma'].to(dtype), d['beta'].to(dtype), 1e-5))
        if reflect:
            x = F.pad(x, (1, 1, 1, 1), mode='reflect')
        y = F.conv2d(x, d['w'].to(dtype), None if d['bias'] is None else d['bias'].to(dtype), stride=s, padding=0 if reflect else k // 2)
        return y, (y + d['res'].to(dtype)[:, sl[1]:sl[1] + co] if sl else y)
    (d['raw64'], d['f64']), (d['raw32'], d['f32']) = ref(torch.float64), ref(torch.float32)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_one_convolution_matches_float64(name):
    n, ci, co, H, W, k, s, reflect, groups, bias, sl = CONV_CASES[name]
    d = conv_case(name)
    g = lambda t: None if t is None else t.to(DEV)
    x, w = g(d['x']), g(d['w'])
    OH, OW = d['f64'].shape[2:]
    ab = None
    if groups:
        ab = torch.full((n, ci, 2), float('nan'), device=DEV)
        _lib.launch("e3dge_hgf_norm", ab, x, g(d['gamma']), g(d['beta']), n, ci, 0, ci, groups, H, W)
    out_c, c0 = sl if sl else (co, 0)
    out = torch.full((n, out_c, OH, OW), float('nan'), device=DEV)
    raw = torch.full((n, co, OH, OW), float('nan'), device=DEV)
    wfrag = torch.empty(co * ((ci * k * k + 31) // 32 * 32), device=DEV)
    _lib.launch("e3dge_hgf_conv", out, raw, x, w, wfrag, ab, g(d['bias']), g(d['res']), n, ci, co, H, W, k, s, int(reflect), out_c, c0,
                sl[0] if sl else 0, c0)
    torch.cuda.synchronize()
    got = out[:, c0:c0 + co].cpu()
    bound = bound_of(d['f64'], d['f32'])
    border = torch.ones((OH, OW), dtype=torch.bool)
    border[1:-1, 1:-1] = False
    rec = dict(err=dist(got, d['f64']), f32=dist(d['f32'], d['f64']), bound=bound, border_err=dist(got[..., border], d['f64'][..., border]),
               interior_err=dist(got[..., ~border], d['f64'][..., ~border]) if (~border).any() else 0.0,
               raw_err=dist(raw, d['raw64']), raw_bound=bound_of(d['raw64'], d['raw32']))
    record("hgfilter_conv", case=name, **rec)
    print(name, {k_: f"{v:.2e}" for k_, v in rec.items()})
    assert rec['interior_err'] <= bound, rec
    assert rec['border_err'] <= bound, rec                                           # relu(b) on a zero-padded tap, or a wrong mirror, fails here
    assert rec['raw_err'] <= rec['raw_bound'], rec
    if sl:                                                                           # nothing outside the slice was written
        rest = torch.cat([out[:, :c0], out[:, c0 + co:]], 1)
        assert bool(torch.isnan(rest).all())
    assert float(d['raw64'].std()) > 0.3


# ---- group statistics ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def norm_case(C, H, W, mean, instance):
    rs = np.random.RandomState(900 + C + 7 * H + int(mean) + instance)
    x = rnd(rs, 2, C, H, W) + mean + rnd(rs, 2, 1, 1, 1, scale=0.1)
    gamma, beta = rnd(rs, C, scale=0.2, shift=1.0), rnd(rs, C, scale=0.2)
    groups = C if instance else 32
    ref = lambda dt: F.group_norm(x.to(dt), groups, gamma.to(dt), beta.to(dt), 1e-5)
    return x, gamma, beta, groups, ref(torch.float64), ref(torch.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("mean", [0.0, 100.0])
@pytest.mark.parametrize("C,H,W,instance", [(32, 4, 6, 0), (64, 5, 7, 0), (256, 32, 48, 0), (256, 4, 6, 0), (32, 32, 48, 0), (32, 5, 7, 1), (32, 32, 48, 1)])
def test_group_statistics_match_float64(C, H, W, instance, mean):
    x, gamma, beta, groups, f64, f32 = norm_case(C, H, W, mean, instance)
    xg = x.to(DEV)
    ab = torch.full((2, C, 2), float('nan'), device=DEV)
    _lib.launch("e3dge_hgf_norm", ab, xg, gamma.to(DEV), beta.to(DEV), 2, C, 0, C, groups, H, W)
    got = torch.addcmul(ab[:, :, 1, None, None], ab[:, :, 0, None, None], xg)
    rec = dict(err=dist(got, f64), f32=dist(f32, f64), bound=bound_of(f64, f32))
    if instance:                                                                     # InstanceNorm2d(affine) is the case groups = C
        rec['instance_err'] = dist(F.instance_norm(x.double(), weight=gamma.double(), bias=beta.double(), eps=1e-5), f64)
    record("hgfilter_norm", C=C, H=H, W=W, mean=mean, instance=instance, **rec)
    print(C, H, W, mean, instance, {k: f"{v:.2e}" for k, v in rec.items()})
    assert rec['err'] <= rec['bound'], rec
    assert rec.get('instance_err', 0.0) <= 1e-12


@pytest.mark.gpu
def test_group_statistics_of_a_channel_slice():
    x, gamma, beta, _, _, _ = norm_case(64, 5, 7, 100.0, 0)
    wide = torch.cat([torch.randn(2, 32, 5, 7) * 50, x, torch.randn(2, 32, 5, 7) - 300], 1).to(DEV)
    ab, alone = torch.empty((2, 64, 2), device=DEV), torch.empty((2, 64, 2), device=DEV)
    _lib.launch("e3dge_hgf_norm", ab, wide, gamma.to(DEV), beta.to(DEV), 2, 128, 32, 64, 32, 5, 7)
    _lib.launch("e3dge_hgf_norm", alone, x.to(DEV), gamma.to(DEV), beta.to(DEV), 2, 64, 0, 64, 32, 5, 7)
    assert torch.equal(ab, alone)


# ---- pooling and up-sampling ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(2, 2), (4, 6), (8, 12)])
def test_pool_and_up_add_match_float64(H, W):
    rs = np.random.RandomState(40 + H)
    low, up1, big = rnd(rs, 2, 5, H, W), rnd(rs, 2, 5, 2 * H, 2 * W), rnd(rs, 2, 5, 2 * H, 2 * W)
    up = lambda dt: up1.to(dt) + F.interpolate(low.to(dt), scale_factor=2, mode='bicubic', align_corners=True)
    out = torch.full((2, 5, 2 * H, 2 * W), float('nan'), device=DEV)
    _lib.launch("e3dge_hgf_up_add", out, up1.to(DEV), low.to(DEV), 10, H, W)
    pooled = torch.full((2, 5, H, W), float('nan'), device=DEV)
    _lib.launch("e3dge_hgf_pool", pooled, big.to(DEV), 10, 2 * H, 2 * W)
    p64, p32 = F.avg_pool2d(big.double(), 2, stride=2), F.avg_pool2d(big, 2, stride=2)
    rec = dict(up_err=dist(out, up(torch.float64)), up_bound=bound_of(up(torch.float64), up(torch.float32)), pool_err=dist(pooled, p64),
               pool_bound=bound_of(p64, p32), pool_vs_f32=dist(pooled, p32))
    record("hgfilter_pool_up", H=H, W=W, **rec)
    print(H, W, {k: f"{v:.2e}" for k, v in rec.items()})
    assert rec['up_err'] <= rec['up_bound'] and rec['pool_err'] <= rec['pool_bound'], rec
    assert float((up(torch.float64) - up1.double()).abs().max()) > 0.5               # the up-sampled branch is not negligible


# ---- the whole filter -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def module_gpu(name):
    m = ResidualImageFilter(syn.pifu_opt(**CASES[name][0]))
    m.load_state_dict(module_cpu(name).state_dict())
    for p in m.parameters():
        p.requires_grad_(False)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def gpu_results(name):
    out = run_case(module_gpu(name), name, tuple(t.to(DEV) for t in case_inputs(name)))
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_filter_matches_float64_and_the_recording(name, monkeypatch):
    launched = []
    real = _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda n, *a: (launched.append(n), real(n, *a))[1])
    gpu_results.cache_clear()
    got = gpu_results(name)
    assert "e3dge_hgf_forward" in launched and (("e3dge_hgf_front" in launched) == CASES[name][4])      # the native path ran
    t64, t32, _ = cpu_results(name)
    gold = load_golden("hgfilter")
    rec, ok = {}, True
    for key in tensor_names(name):
        h = got[key]
        assert h.shape == t64[key].shape and h.dtype == torch.float32 and h.is_contiguous(), key
        f32 = dist(t32[key], t64[key])
        rec[key + '_err'], rec[key + '_f32'], rec[key + '_bound'] = dist(h, t64[key]), f32, bound_of(t64[key], t32[key])
        flat = h.reshape(-1).cpu()
        rec[key + '_rec_err'] = float(np.abs(flat[samples(flat.numel())].double().numpy() - gold[f"{name}_{key}"].astype(np.float64)).max())
        rec[key + '_rec_bound'] = bound_of(t64[key], t32[key], 4)
        ok &= rec[key + '_err'] <= rec[key + '_bound'] and rec[key + '_rec_err'] <= rec[key + '_rec_bound']
    if name == "default":
        last = tensor_names(name)[-3]
        rec['image0_rec_err'] = dist(got[last][0], torch.from_numpy(gold["default_last_image0"]))
        ok &= rec['image0_rec_err'] <= rec[last + '_rec_bound']
    record("hgfilter_parity", case=name, **rec)
    print(name, {k: f"{v:.2e}" for k, v in rec.items()})
    assert ok, rec


@pytest.mark.gpu
def test_two_runs_are_bit_identical_and_an_image_does_not_depend_on_the_batch():
    m = module_gpu("filter")
    image, depth = (t.to(DEV) for t in case_inputs("filter"))
    first = gpu_results("filter")
    again = run_case(m, "filter", (image, depth))
    alone = run_case(m, "filter", (image[:1].contiguous(), depth[:1].contiguous()))
    torch.cuda.synchronize()
    for key in tensor_names("filter"):
        assert torch.equal(first[key], again[key]), key
        assert torch.equal(first[key][:1], alone[key]), key


@pytest.mark.gpu
def test_other_paths_take_the_torch_composition(monkeypatch):
    m = ResidualImageFilter(syn.pifu_opt(num_stack=1, num_hourglass=1))
    syn.load_synthetic_hgfilter(m)
    m = m.to(DEV).eval()
    rs = np.random.RandomState(3)
    image, depth = rnd(rs, 1, 3, 16, 16).to(DEV), rnd(rs, 1, 1, 16, 16).to(DEV)
    launched = []
    real = _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda n, *a: (launched.append(n), real(n, *a))[1])
    hgf = lambda: [n for n in launched if n.startswith("e3dge_hgf_") and n != "e3dge_hgf_pack_weights"]
    out = m.filter(image, depth, return_feat=True)[0]                                # a trainable parameter, grad mode on
    assert not hgf() and out.requires_grad
    for p in m.parameters():
        p.requires_grad_(False)
    want = m.filter(image, depth, return_feat=True)[0]                               # frozen: the kernels, even with grad mode on
    assert hgf() == ["e3dge_hgf_front", "e3dge_hgf_forward"] and not want.requires_grad
    del launched[:]
    out = m.filter(image.clone().requires_grad_(True), depth, return_feat=True)[0]
    assert not hgf() and out.requires_grad
    monkeypatch.setenv("E3DGE_HGFILTER", "torch")
    out = m.filter(image, depth, return_feat=True)[0]
    assert not hgf()
    monkeypatch.delenv("E3DGE_HGFILTER")
    m.image_filter.conv1.weight.requires_grad_(True)
    with torch.no_grad():                                                            # grad mode off: no gradient is wanted
        got = m.filter(image, depth, return_feat=True)[0]
    assert hgf() == ["e3dge_hgf_front", "e3dge_hgf_forward"] and torch.equal(got, want)
    torch.cuda.synchronize()
    assert dist(out, want) <= 1e-3 * float(want.abs().max()) and float(want.std()) > 0.3     # the same function on both paths (library convolutions)
    with pytest.raises(DeprecationWarning):
        m.filter(image, depth, ref_feats=image)


@pytest.mark.gpu
def test_filter_output_is_accepted_as_feature_maps():
    from e3dge_amd.local_query import Fuse_sft_MLP, local_features_from_maps
    m = module_gpu("filter")
    image, depth = (t.to(DEV) for t in case_inputs("filter"))
    with torch.no_grad():
        ref_map = m.filter(image, depth, feat_key='ref_view', return_feat=True)[0]
        que_map = m.filter(image.flip(0), depth.flip(0), feat_key='que_view', return_feat=True)[0]
    B = image.shape[0]
    for t in (ref_map, que_map):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B, 256, 16, 24)
    torch.manual_seed(3)
    H, S = 8, 6
    fuse = Fuse_sft_MLP(257, 256).to(DEV)
    for p_ in fuse.parameters():
        torch.nn.init.normal_(p_, std=0.05)
    calib = torch.tensor([[[2.0, 0.0, 0.0, 0.0], [0.0, 2.0, 0.0, 0.0], [0.0, 0.0, 1.0, 2.0]]], device=DEV).expand(B, 3, 4).contiguous()
    batch = dict(feature_maps={'ref': ref_map, 'que': que_map}, ref_calibs=calib, que_calibs=calib.clone(),
                 points=(torch.rand(B, H, H, S, 3, device=DEV) - 0.5), xyz=(torch.rand(B, 3, H, H, device=DEV) - 0.5), fuse_sft_block=fuse)
    with torch.no_grad():
        feats, in_img = local_features_from_maps(batch)
    torch.cuda.synchronize()
    assert tuple(feats.shape) == (B, H, H, S, 301) and bool(torch.isfinite(feats).all()) and float(feats[..., :256].std()) > 0
