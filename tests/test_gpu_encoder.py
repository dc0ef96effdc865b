"""GPU: the E0 image encoder on the kernels of csrc/encoder.h -- each new kernel through its debug entry at small shapes, the whole network at
64^2 and 48^2 against the float64 torch composition and at 256^2 against the recording of the reference (tests/golden/encoder.npz), bit
reproducibility, batch independence, and the identity network's embeddings around an encoder forward (the body shares its kernels).

Bound, per tensor (tests/test_gpu_idloss.py, tests/test_gpu_hgfilter.py): max|hip - f64| <= max(2e-6 max|f64|, 3 max|f32 - f64|) with f32 and f64
the CPU composition; against the recording the last factor is 4.  Every error is recorded with conftest.record."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, record

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, synthetic as syn
from e3dge_amd.encoders import HybridGradualStyleEncoder_V2
from e3dge_amd.id_loss import IDLoss
import test_encoder_host as host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOPE = 0.01


def rnd(rs, *shape, scale=1.0):
    return torch.from_numpy((scale * rs.standard_normal(shape)).astype(np.float32))


def dist(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def bound_of(t64, t32, factor=3):
    return host.parity_bound(t64, t32, factor)


def g(t):
    return t.to(DEV).contiguous()


@functools.lru_cache(maxsize=None)
def module_gpu(**over):
    """The case's encoder on the GPU with the CPU module's values; shared, never modified."""
    with torch.device("meta"):
        m = HybridGradualStyleEncoder_V2(50, 'ir_se', 9, host.options(**over))
    m = m.to_empty(device="cpu")
    m.load_state_dict(host.module_cpu(**over).state_dict(), strict=True)
    m = m.to(DEV).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


# ---- 1. lateral -------------------------------------------------------------------------------------------------------------------------
LATERAL = {                        # name: (cin, coarse (h, w), fine (h, w))
    "small_odd": (64, (3, 5), (6, 10)),
    "square": (128, (16, 16), (32, 32)),
    "wide_partial_tile": (256, (20, 26), (40, 52)),
    "scale_zero": (128, (1, 1), (2, 2)),
}


@pytest.mark.parametrize("name", sorted(LATERAL))
def test_lateral_kernel(name):
    cin, (ch, cw), (h, w) = LATERAL[name]
    n, cout = 2, 512
    rs = np.random.RandomState(100 + cin + h)
    coarse, x = rnd(rs, n, cout, ch, cw), rnd(rs, n, cin, h, w)
    wt, b = rnd(rs, cout, cin, 1, 1, scale=math.sqrt(1.0 / cin)), rnd(rs, cout, scale=0.3)
    ref = lambda c, x_, w_, b_: F.interpolate(c, size=(h, w), mode='bilinear', align_corners=True) + F.conv2d(x_, w_, b_)
    f64, f32 = ref(coarse.double(), x.double(), wt.double(), b.double()), ref(coarse, x, wt, b)
    out = torch.full((n, cout, h, w), float('nan'), device=DEV)
    wfrag = torch.empty(cout * ((cin + 31) // 32 * 32), device=DEV)
    _lib.launch("e3dge_enc_lateral", out, g(coarse), g(x), g(wt), g(b), wfrag, n, cin, cout, ch, cw, h, w)
    torch.cuda.synchronize()
    rec = dict(err=dist(out, f64), f32=dist(f32, f64), bound=bound_of(f64, f32))
    record("encoder_lateral", case=name, **rec)
    print(name, {k: f"{v:.2e}" for k, v in rec.items()})
    assert float(f64.std()) > 0.5
    assert not bool(torch.isnan(out).any())
    assert rec['err'] <= rec['bound'], rec


# ---- 2. grouped head convolution ---------------------------------------------------------------------------------------------------------
HEAD_CONV = {                      # name: (heads, shared, cin, cout, (h, w))
    "shared": (3, 1, 512, 256, (16, 16)),
    "per_head": (3, 0, 256, 256, (8, 8)),
    "odd": (3, 0, 256, 256, (5, 7)),
    "one_head": (1, 1, 512, 512, (33, 37)),
}


@pytest.mark.parametrize("name", sorted(HEAD_CONV))
def test_grouped_head_conv_kernel(name):
    G, shared, cin, cout, (h, w) = HEAD_CONV[name]
    n = 2
    oh, ow = (h + 1) // 2, (w + 1) // 2
    rs = np.random.RandomState(200 + cin + h + G)
    x = rnd(rs, n, cin, h, w) if shared else rnd(rs, G, n, cin, h, w)
    wt = rnd(rs, G, cout, cin, 3, 3, scale=math.sqrt(2.0 / (9 * cin)))           # He
    b = -0.3 + rnd(rs, G, cout, scale=0.05)                                      # negative: the two LeakyReLU branches are not mirror images

    def ref(x_, w_, b_):
        return torch.stack([F.leaky_relu(F.conv2d(x_ if shared else x_[i], w_[i], b_[i], stride=2, padding=1), SLOPE) for i in range(G)])
    f64, f32 = ref(x.double(), wt.double(), b.double()), ref(x, wt, b)
    assert tuple(f64.shape) == (G, n, cout, oh, ow)
    positive = float((f64 > 0).double().mean())
    assert 0.10 <= positive <= 0.90, positive                                    # each branch holds at least 10 % of the outputs
    out = torch.full((G, n, cout, oh, ow), float('nan'), device=DEV)
    wfrag = torch.empty(G * cout * ((9 * cin + 31) // 32 * 32), device=DEV)
    _lib.launch("e3dge_enc_head_conv", out, g(x), g(wt), g(b), wfrag, n, G, shared, cin, cout, h, w)
    torch.cuda.synchronize()
    got = out.cpu()
    bound = bound_of(f64, f32)
    border = torch.ones((oh, ow), dtype=torch.bool)
    border[1:-1, 1:-1] = False
    rec = dict(err=dist(got, f64), f32=dist(f32, f64), bound=bound, border_err=dist(got[..., border], f64[..., border]),
               interior_err=dist(got[..., ~border], f64[..., ~border]) if (~border).any() else 0.0, positive=positive)
    record("encoder_head_conv", case=name, **rec)
    print(name, {k: f"{v:.2e}" for k, v in rec.items()})
    assert not bool(torch.isnan(got).any())
    assert rec['interior_err'] <= bound, rec
    assert rec['border_err'] <= bound, rec                                       # a wrong pad or stride shows here


# ---- 3. head tail -----------------------------------------------------------------------------------------------------------------------
TAIL = {                           # name: (heads, channels, start, n_convs)
    "two_by_two_then_three": (3, 256, 2, 4),
    "two_by_two_only": (1, 512, 2, 1),
    "from_one_by_one": (3, 256, 1, 3),
}


@pytest.mark.parametrize("name", sorted(TAIL))
def test_head_tail_kernel(name):
    G, C, start, L = TAIL[name]
    n = 2
    rs = np.random.RandomState(300 + C + start + L)
    x = rnd(rs, G, n, C, start, start)
    cw = rnd(rs, G, L, C, C, 3, 3, scale=math.sqrt(2.0 / C))                     # He over the live taps of a 1 x 1 map
    cw[:, 0] *= 1.0 / start
    cb = rnd(rs, G, L, C, scale=0.2)
    lw, lb = rnd(rs, G, C, C), rnd(rs, G, C, scale=0.05)

    def ref(x_, cw_, cb_, lw_, lb_):
        outs = []
        for i in range(G):
            y = x_[i]
            for l in range(L):
                y = F.leaky_relu(F.conv2d(y, cw_[i, l], cb_[i, l], stride=2, padding=1), SLOPE)
            assert tuple(y.shape[-2:]) == (1, 1)
            outs.append(F.linear(y.reshape(-1, C), lw_[i] * (1 / math.sqrt(C)), bias=lb_[i] * 1))       # EqualLinear, lr_mul 1
        return torch.stack(outs, dim=1)
    f64, f32 = ref(*(t.double() for t in (x, cw, cb, lw, lb))), ref(x, cw, cb, lw, lb)
    floats = G * C * (C * (L + 4) + L + 1 + 2 * n)

    def run(conv_w):
        out = torch.full((n, G, C), float('nan'), device=DEV)
        scratch = torch.full((floats,), float('nan'), device=DEV)
        _lib.launch("e3dge_enc_head_tail", out, g(x), g(conv_w), g(cb), g(lw), g(lb), scratch, floats, n, G, C, start, L)
        torch.cuda.synchronize()
        return out.cpu()
    got = run(cw)
    rec = dict(err=dist(got, f64), f32=dist(f32, f64), bound=bound_of(f64, f32), std=float(f64.std()))
    record("encoder_head_tail", case=name, **rec)
    print(name, {k: f"{v:.2e}" for k, v in rec.items()})
    assert rec['std'] > 0.3
    assert not bool(torch.isnan(got).any())
    assert rec['err'] <= rec['bound'], rec
    dead = cw.clone()                                                            # the dead taps are not read: NaN there changes no bit
    live = torch.zeros((L, 3, 3), dtype=torch.bool)
    live[:, 1, 1] = True
    if start == 2:
        live[0, 1:, 1:] = True
    dead[:, ~live.reshape(L, 1, 1, 3, 3).expand(L, C, C, 3, 3)] = float('nan')
    assert int(torch.isnan(dead).sum()) == G * C * C * (9 * L - (L - 1) - start * start)
    assert torch.equal(run(dead), got)


# ---- 4. the whole network against the float64 composition ---------------------------------------------------------------------------------
def gpu_tensors(name):
    over, n, size = host.CASES[name]
    x = host.encoder_input(n, size, sorted(host.CASES).index(name) + 1).to(DEV)
    m = module_gpu(**over)
    assert m._runs_hip(x)
    with torch.no_grad():
        out = m.run(x, return_featmap=True, pool=False)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", ["s64", "s48", "tex64"])
def test_whole_network_against_float64(name):
    t64, t32 = host.cpu_results(name)
    assert set(t64) == set(host.TENSORS)
    stds = {k: float(t.std()) for k, t in t64.items()}
    assert stds["thumb_out"] >= 0.03 and stds["stylegan_out"] >= 0.03 and stds["feat_maps"] >= 0.5 and stds["p32"] >= 0.5, stds      # alive
    out = gpu_tensors(name)
    assert isinstance(out, dict) and sorted(out) == ['feat_maps', 'p32', 'pred_latents']
    got = host.as_tensors(out)
    worst = []
    for k in host.TENSORS:
        assert got[k].shape == t64[k].shape and got[k].dtype == torch.float32, k
        rec = dict(err=dist(got[k], t64[k]), f32=dist(t32[k], t64[k]), bound=bound_of(t64[k], t32[k]), std=stds[k])
        record("encoder_network", case=name, tensor=k, **rec)
        print(name, k, {q: f"{v:.2e}" for q, v in rec.items()})
        if rec['err'] > rec['bound']:
            worst.append((k, rec))
    assert not worst, worst
    assert torch.equal(got["stylegan_out"][:, 0], got["stylegan_out"][:, 9])


def test_whole_network_without_the_decoder_head():
    t64, t32 = host.cpu_results("nodec")
    assert set(t64) == {"thumb_out"} and float(t64["thumb_out"].std()) >= 0.03
    out = gpu_tensors("nodec")
    assert isinstance(out, list) and out[1] is None
    rec = dict(err=dist(out[0], t64["thumb_out"]), f32=dist(t32["thumb_out"], t64["thumb_out"]), bound=bound_of(t64["thumb_out"], t32["thumb_out"]))
    record("encoder_network", case="nodec", tensor="thumb_out", **rec)
    assert rec['err'] <= rec['bound'], rec
    # no p128 work: the forward takes a NULL stylegan_out and a workspace without the p128 map, and the maps equal the full module's
    over, n, size = host.CASES["nodec"]
    m = module_gpu(**over)
    x = host.encoder_input(n, size, sorted(host.CASES).index("nodec") + 1).to(DEV)
    assert _lib.query("e3dge_enc_ws_bytes", n, size, 128, 128, 0) + n * 512 * (size // 2) ** 2 * 4 <= _lib.query("e3dge_enc_ws_bytes", n, size, 128, 128, 1)
    thumb, sg, p32, p64 = m.forward_hip(x)
    full = module_gpu().forward_hip(x)
    torch.cuda.synchronize()
    assert sg is None and torch.equal(thumb, out[0]) and torch.equal(thumb, full[0]) and torch.equal(p32, full[2]) and torch.equal(p64, full[3])


# ---- 5. 256^2 against the recording of the reference -----------------------------------------------------------------------------------------
def test_whole_network_at_256_against_the_recording():
    gold = load_golden("encoder")
    n, size, seed = host.GOLDEN_CASE
    x = host.encoder_input(n, size, seed).to(DEV)
    m = module_gpu()
    assert m._runs_hip(x)
    with torch.no_grad():
        got = host.as_tensors(m(x, return_featmap=True))
    torch.cuda.synchronize()
    worst = []
    for k in host.TENSORS:
        t = got[k].cpu()
        flat = t.reshape(-1)
        f64_max, f32_err = float(gold[f"{k}_f64_max"]), float(gold[f"{k}_err"])
        bound = max(2e-6 * f64_max, 4 * f32_err)
        err = float(np.abs(flat[host.samples(flat.numel())].double().numpy() - gold[f"{k}_f64"]).max())
        # the sum: independent errors of at most `bound` per element add up to about sqrt(numel) bound; the reference's own fp32 sum is
        # |f32 sum - f64 sum| away.  Four times the larger of the two.
        sum_err = abs(float(t.double().sum()) - float(gold[f"{k}_f64_sum"]))
        sum_bound = 4 * max(abs(float(gold[f"{k}_f32_sum"]) - float(gold[f"{k}_f64_sum"])), math.sqrt(flat.numel()) * bound)
        rec = dict(err=err, bound=bound, f32=f32_err, sum_err=sum_err, sum_bound=sum_bound)
        record("encoder_network_256", tensor=k, **rec)
        print(k, {q: f"{v:.2e}" for q, v in rec.items()})
        if err > bound or sum_err > sum_bound:
            worst.append((k, rec))
    assert not worst, worst


# ---- 6. determinism and batch independence -----------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_an_image_does_not_depend_on_the_batch():
    m = module_gpu()
    x = host.encoder_input(3, 64, 11).to(DEV)
    a, b, alone = m.forward_hip(x), m.forward_hip(x), m.forward_hip(x[1:2].contiguous())
    torch.cuda.synchronize()
    for i, (p, q, r) in enumerate(zip(a, b, alone)):
        assert torch.equal(p, q), i
        assert torch.equal(p[1:2], r), i
    assert float(a[0][1].std()) > 0 and not torch.equal(a[0][0], a[0][1])


# ---- 7. the identity network around an encoder forward -------------------------------------------------------------------------------------
def test_idloss_embeddings_do_not_change_around_an_encoder_forward():
    idl = syn.load_synthetic_idloss(IDLoss()).to(DEV)
    imgs = host.encoder_input(2, 64, 12).clamp(-1, 1).to(DEV)
    with torch.no_grad():
        before = idl.embed(imgs).clone()
        module_gpu().forward_hip(host.encoder_input(2, 64, 13).to(DEV))
        after = idl.embed(imgs).clone()
    torch.cuda.synchronize()
    assert torch.equal(before, after) and bool(torch.isfinite(before).all()) and float(before.std()) > 0
