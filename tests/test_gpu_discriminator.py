"""The discriminator's HIP path (csrc/disc.hip, csrc/disc_bwd.h, e3dge_amd.discriminator) against the torch composition on the CPU -- the
reference's operations in the reference's order (tests/test_discriminator_host.py) --: once in float64 (truth), once in float32 (the
yardstick), and against the recording of the reference itself (tests/golden/discriminator.npz: |hip - recording| <= the bound + the
yardstick's own distance from the truth, since the recording is a float32 CPU run like the yardstick).

Bounds:  one convolution, one data gradient, the stddev scalars, logits and taps of the whole forward
                                                max|hip - f64| <= max(2e-6 max|f64|, 3 max|f32 - f64|)   (the identity term's per-convolution bound)
         the adjoint identity                   |<conv x, g> - <x, dgrad g>| <= bound(conv) sum|g| + bound(dgrad) sum|x|, in float64 on the HIP outputs
                                                (each side is within its per-element bound of the exact inner product, which are equal)
         the whole backward, branch-pinned      max|hip - f64| / max|f64| <= max(5e-5, 3 x the float32 restatement's), input gradient and each stage

Branch-pinned: truth and yardstick take every lrelu derivative's branch from the sign of the activations the HIP forward saved; the
pinned branches are checked against the float64 forward: (a) every disagreement has |pre64| <= 1e-4, (b) there are at most as many as
float64 elements with |pre64| < 1e-5.  The images are test_discriminator_host.golden_images (seed 2000 + size + batch): for them the
float32 CPU path itself meets (a) and (b) (tests/golden/discriminator_report.json: 0 to 2 flips against 20 to 741 near-zero elements)."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, record

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, discriminator as disc, losses, synthetic as syn
from e3dge_amd.discriminator import Discriminator
from e3dge_amd.op import FusedLeakyReLU
from test_discriminator_host import CASES, VARIANTS, case_id, golden_images, module_cpu, tap_name, torch_taps
from test_idloss_host import tap_samples

DEV = "cuda:0"
SQRT2 = 2 ** 0.5


def dist(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def conv_bound(f64, f32):
    return max(2e-6 * float(f64.abs().max()), 3 * dist(f32, f64))


def guarded(shape, guard):
    """A NaN-filled output of `shape` with `guard` NaNs behind it: (the flat buffer, the view)."""
    numel = int(np.prod(shape))
    flat = torch.full((numel + guard,), float('nan'), device=DEV)
    return flat, flat[:numel].view(shape)


def intact(flat, out):
    return bool(torch.isnan(flat[out.numel():]).all()) and not bool(torch.isnan(out).any())


@functools.lru_cache(maxsize=None)
def module_f64(init, cm, variant=None):
    m = syn.load_synthetic_discriminator(Discriminator(syn.discriminator_opt(init, cm)), variant=variant).double()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


@functools.lru_cache(maxsize=None)
def module_gpu(init, cm, variant=None):
    m = syn.load_synthetic_discriminator(Discriminator(syn.discriminator_opt(init, cm)), variant=variant).to(DEV)
    for p in m.parameters():
        p.requires_grad_(False)
    return m


# ---- single layers ----------------------------------------------------------------------------------------------------------------
# n, Cin, Cout, input size, kernel, stride, bias + lrelu, merge with an addend; batch 3: tile and image boundaries are crossed
LAYER_CASES = [
    (3, 3, 64, 16, 1, 1, True, False),                               # the stem: K = 3
    (3, 64, 64, 8, 3, 1, True, False),
    (3, 64, 128, 9, 3, 2, True, False),                              # on a blurred 9^2 plane -> 4^2
    (3, 64, 128, 7, 1, 2, False, True),                              # skip: 7^2 -> 4^2, no bias, the residual merge
    (3, 513, 512, 4, 3, 1, True, False),                             # final_conv: K = 4617, a ragged last k tile
]


@functools.lru_cache(maxsize=None)
def layer_case(i):
    n, ci, co, size, k, s, act, merge = LAYER_CASES[i]
    osize = size if s == 1 else (size - k) // 2 + 1
    rs = np.random.RandomState(300 + i)
    t = lambda *shape, scale=1.0: torch.from_numpy(scale * rs.standard_normal(shape)).float()
    d = dict(x=t(n, ci, size, size), w=t(co, ci, k, k), bias=t(co, scale=0.5) if act else None, addend=t(n, co, osize, osize) if merge else None,
             g=t(n, co, osize, osize), sign=t(n, co, osize, osize), gadd=t(n, ci, size, size), scale=1 / math.sqrt(ci * k * k), osize=osize)
    pad = k // 2 if s == 1 else 0

    def plain(x, dtype):
        return F.conv2d(x, d['w'].to(dtype) * d['scale'], stride=s, padding=pad)

    def fwd(dtype):
        v = plain(d['x'].to(dtype), dtype)
        if act:
            v = F.leaky_relu(v + d['bias'].to(dtype)[None, :, None, None], 0.2) * SQRT2
        if merge:
            v = (d['addend'].to(dtype) + v) / math.sqrt(2)
        return v

    def dgrad(dtype, pinned):
        x = torch.zeros(n, ci, size, size, dtype=dtype, requires_grad=True)
        g = d['g'].to(dtype)
        if pinned:
            g = g * torch.where(d['sign'] > 0, torch.tensor(SQRT2, dtype=dtype), torch.tensor(0.2 * SQRT2, dtype=dtype))
        out, = torch.autograd.grad(plain(x, dtype), x, g)
        return out + d['gadd'].to(dtype) if pinned else out

    for name, fn in [("fwd", fwd), ("plain", lambda dt: plain(d['x'].to(dt), dt)), ("dgrad", lambda dt: dgrad(dt, True)),
                     ("dplain", lambda dt: dgrad(dt, False))]:
        d[name + "64"], d[name + "32"] = fn(torch.float64), fn(torch.float32)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(LAYER_CASES)), ids=lambda i: "x".join(map(str, LAYER_CASES[i][:6])))
def test_one_convolution_and_its_data_gradient_match_float64(i):
    n, ci, co, size, k, s, act, merge = LAYER_CASES[i]
    d = layer_case(i)
    c = lambda t: None if t is None else t.to(DEV)
    osize = d['osize']
    wfrag = torch.empty((co + 15) // 16 * 16 * ((ci * k * k + 31) // 32 * 32), device=DEV)
    wfrag_t = torch.empty((ci + 15) // 16 * 16 * ((co * k * k + 31) // 32 * 32), device=DEV)
    outs = {}
    for name, bias, addend in [("fwd", c(d['bias']), c(d['addend'])), ("plain", None, None)]:
        flat, out = guarded((n, co, osize, osize), osize)
        _lib.launch("e3dge_disc_conv", out, c(d['x']), c(d['w']), wfrag, bias, addend, n, ci, co, size, size, k, s, int(act and name == "fwd"),
                    int(merge and name == "fwd"), float(d['scale']))
        torch.cuda.synchronize()
        assert intact(flat, out), name
        outs[name] = out.cpu()
    for name, sign, s_pos, s_neg, addend in [("dgrad", c(d['sign']), SQRT2, 0.2 * SQRT2, c(d['gadd'])), ("dplain", None, 1.0, 1.0, None)]:
        flat, out = guarded((n, ci, size, size), size)
        _lib.launch("e3dge_disc_conv_dgrad", out, c(d['g']), c(d['w']), wfrag_t, sign, float(s_pos), float(s_neg), addend, n, ci, co, size, size, k, s,
                    float(d['scale']))
        torch.cuda.synchronize()
        assert intact(flat, out), name
        outs[name] = out.cpu()
    rec, bounds = {}, {}
    for name in ("fwd", "plain", "dgrad", "dplain"):
        bounds[name] = conv_bound(d[name + "64"], d[name + "32"])
        rec[name] = dist(outs[name], d[name + "64"])
        rec[name + "_f32"], rec[name + "_bound"] = dist(d[name + "32"], d[name + "64"]), bounds[name]
    # <conv x, g> = <x, dgrad g>, in float64 on the HIP outputs
    x64, g64 = d['x'].double(), d['g'].double()
    lhs, rhs = float((outs["plain"].double() * g64).sum()), float((x64 * outs["dplain"].double()).sum())
    rec["adjoint"], rec["adjoint_bound"] = abs(lhs - rhs), bounds["plain"] * float(g64.abs().sum()) + bounds["dplain"] * float(x64.abs().sum())
    record("disc_layer", case=list(LAYER_CASES[i][:6]), **rec)
    print(LAYER_CASES[i], {k_: f"{v:.2e}" for k_, v in rec.items()})
    assert float(d["fwd64"].abs().max()) > 0.1 and float(d["dgrad64"].abs().max()) > 0.1
    for name in ("fwd", "plain", "dgrad", "dplain"):
        assert rec[name] <= bounds[name], (name, rec)
    assert rec["adjoint"] <= rec["adjoint_bound"], rec


# ---- minibatch standard deviation -------------------------------------------------------------------------------------------------
def stddev_torch(feat, dtype):
    """stylesdf_model.py:1598-1609 on (B, C, H, W): (the concatenated tensor, the B / group scalars)."""
    out = feat.to(dtype)
    batch, channel, height, width = out.shape
    group = disc.stddev_group(batch)
    s = out.reshape(group, -1, 1, channel, height, width)
    s = torch.sqrt(s.var(0, unbiased=False) + 1e-8).mean([2, 3, 4], keepdims=True).squeeze(2)
    return torch.cat([out, s.repeat(group, 1, height, width)], 1), s.reshape(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 2, 3, 4, 6, 8])
@pytest.mark.parametrize("shape", [(512, 4, 4), (40, 3, 3)], ids=["512x16", "40x9"])
def test_stddev_kernel_matches_torch(batch, shape):
    C, H, W = shape
    feat = torch.from_numpy(np.random.RandomState(batch * 100 + C).standard_normal((batch, C, H, W))).float()
    feat[:, ::3] *= 0.01                                             # small and large variances in one mean
    cat64, s64 = stddev_torch(feat, torch.float64)
    cat32, s32 = stddev_torch(feat, torch.float32)
    flat, cat = guarded((batch, C + 1, H, W), H * W)
    scalars = torch.full((s64.numel(),), float('nan'), device=DEV)
    _lib.launch("e3dge_disc_stddev", cat, scalars, feat.to(DEV), batch, C, H * W)
    torch.cuda.synchronize()
    assert intact(flat, cat) and not bool(torch.isnan(scalars).any())
    rec = dict(err=dist(scalars, s64), f32=dist(s32, s64), bound=conv_bound(s64, s32))
    record("disc_stddev", batch=batch, channels=C, **rec)
    print(batch, shape, {k: f"{v:.2e}" for k, v in rec.items()})
    assert rec['err'] <= rec['bound'], rec
    assert torch.equal(cat[:, :C].cpu(), feat)                       # the features are copied
    sub = batch // disc.stddev_group(batch)
    want = scalars.cpu()[torch.arange(batch) % sub]                  # sample b belongs to sub-batch b % (B / group)
    assert torch.equal(cat[:, C].cpu(), want[:, None, None].expand(batch, H, W))


@pytest.mark.gpu
def test_stddev_of_equal_samples_is_sqrt_eps():
    feat = torch.from_numpy(np.random.RandomState(7).standard_normal((1, 512, 4, 4))).float().repeat(4, 1, 1, 1)
    cat = torch.empty(4, 513, 4, 4, device=DEV)
    scalars = torch.empty(1, device=DEV)
    _lib.launch("e3dge_disc_stddev", cat, scalars, feat.to(DEV), 4, 512, 16)
    torch.cuda.synchronize()
    err = abs(float(scalars[0]) - 1e-4)
    record("disc_stddev_equal", err=err)
    assert err <= 2e-6 * 1e-4                                        # the variance is exactly 0: sqrt(1e-8)
    assert bool((cat[:, 512] == scalars[0]).all())


# ---- the whole network ------------------------------------------------------------------------------------------------------------
class _PinnedLrelu(torch.autograd.Function):
    """FusedLeakyReLU's forward on x (the bias already added); the derivative's branch comes from `mask` (True: positive)."""

    @staticmethod
    def forward(ctx, x, mask):
        ctx.save_for_backward(mask)
        return F.leaky_relu(x, negative_slope=0.2) * SQRT2

    @staticmethod
    def backward(ctx, g):
        mask, = ctx.saved_tensors
        return g * torch.where(mask, torch.tensor(SQRT2, dtype=g.dtype), torch.tensor(0.2 * SQRT2, dtype=g.dtype)), None


def pinned_run(m, x, masks, upstream=None):
    """The torch layers of module `m` (its dtype) in forward_torch's order, with every lrelu derivative pinned to `masks` (None: the
    forward's own branches).  The loss is (upstream * logits).sum(), or g_nonsaturating_loss(logits) when upstream is None.  Returns
    dict(logits, taps, grad, stages {tap: gradient}, pre: the lrelu inputs in network order)."""
    dtype = m.final_conv[0].weight.dtype
    leaf = x.to(dtype).clone().requires_grad_(True)
    it = iter(masks) if masks is not None else None
    pre, kept = [], {}

    def act(t, bias, view):
        t = t + bias.reshape(view)
        pre.append(t.detach())
        return _PinnedLrelu.apply(t, next(it) if it is not None else t.detach() > 0)

    def conv_layer(layers, t):
        for mod in layers:
            t = act(t, mod.bias, (1, -1, 1, 1)) if isinstance(mod, FusedLeakyReLU) else mod(t)
        return t

    def keep(tap, t):
        t.retain_grad()
        kept[tap] = t

    t = m.pool_256(leaf) if m.init_size == 256 else leaf
    t = conv_layer(m.convs[0], t)
    keep(disc.TAP_STEM, t)
    for i, b in enumerate(list(m.convs)[1:]):
        o = conv_layer(b.conv2, conv_layer(b.conv1, t))
        t = (o + b.skip(t)) / math.sqrt(2)
        keep(i, t)
    batch, channel, height, width = t.shape
    group = disc.stddev_group(batch)
    s = t.reshape(group, -1, 1, channel, height, width)
    s = torch.sqrt(s.var(0, unbiased=False) + 1e-8).mean([2, 3, 4], keepdims=True).squeeze(2)
    taps = {disc.TAP_STDDEV: s.detach().reshape(-1)}
    f = conv_layer(m.final_conv, torch.cat([t, s.repeat(group, 1, height, width)], 1))
    keep(disc.TAP_FINAL, f)
    l0 = m.final_linear[0]
    h = act(F.linear(f.reshape(batch, -1), l0.weight * l0.scale), l0.bias * l0.lr_mul, (1, -1))
    logits = m.final_linear[1](h)[:, :1]
    loss = losses.g_nonsaturating_loss(logits) if upstream is None else (upstream.to(dtype) * logits).sum()
    loss.backward()
    taps.update({k: v.detach() for k, v in kept.items() if k != disc.TAP_STEM})
    return dict(logits=logits.detach(), taps=taps, grad=leaf.grad, stages={k: v.grad for k, v in kept.items()}, pre=pre)


def upstream_of(n):
    return (torch.linspace(0.5, 1.5, n) if n > 1 else torch.ones(1)).reshape(n, 1) / n


def masks_of(m, saved, batch):
    saved = saved.cpu()
    return [saved[off:off + int(np.prod(shape))].view(shape) > 0 for name, off, shape in m.saved_layout(batch) if name != "last"]


BACKWARD = {((16, 1, 4, 16), None), ((16, 1, 6, 16), 'stress'), ((256, 1, 2, 256), None)}


@functools.lru_cache(maxsize=None)
def whole_case(case, variant):
    """The HIP run of one recorded case (taps; for the BACKWARD cases the backward with stages and the saved state) and the CPU runs in
    float64 and float32 (pinned to the HIP branches when there is a backward), computed once and never modified."""
    init, cm, B, size = case
    x = golden_images(B, size)
    mg = module_gpu(init, cm, variant)
    hip = {k: v for k, v in mg.run(x.to(DEV), taps=True).items()}
    u = None
    if (case, variant) in BACKWARD:
        u = upstream_of(B)
        b = mg.run_backward(x.to(DEV), u.to(DEV), stages=True)
        assert torch.equal(b['logits'], hip['logits'])               # the saving forward
        hip.update(grad=b['grad'].cpu(), stages={k: v.cpu() for k, v in b['stages'].items()}, masks=masks_of(mg, b['saved'], B))
    torch.cuda.synchronize()
    hip['logits'], hip['taps'] = hip['logits'].cpu(), {k: v.cpu() for k, v in hip['taps'].items()}
    if u is not None:
        t64 = pinned_run(module_f64(init, cm, variant), x, hip['masks'], u)
        t32 = pinned_run(module_cpu(init, cm, variant), x, hip['masks'], u)
        del t32['pre']
    else:
        with torch.no_grad():
            t64 = dict(zip(("logits", "taps"), torch_taps(module_f64(init, cm, variant), x.double())))
            t32 = dict(zip(("logits", "taps"), torch_taps(module_cpu(init, cm, variant), x)))
    return x, u, hip, t64, t32


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=["init", "stress"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_whole_forward_matches_the_recording_and_float64(case, variant):
    init, cm, B, size = case
    x, _, hip, t64, t32 = whole_case(case, variant)
    gold, key = load_golden("discriminator"), case_id(case, variant) + "/"
    assert hip['logits'].shape == (B, 1)
    failed = []
    for name, h, a, b in [("logits", hip['logits'], t64['logits'], t32['logits'])] + \
                         [(tap_name(t), hip['taps'][t], t64['taps'][t], t32['taps'][t]) for t in sorted(hip['taps'])]:
        assert h.shape == a.shape, name
        if name != "logits":
            idx = tap_samples(b.numel())
        rec = dict(err=dist(h, a), f32=dist(b, a), bound=conv_bound(a, b), top=float(a.abs().max()))
        if name == "logits":
            rec['vs_recording'] = float(np.abs(h.double().numpy() - gold[key + "logits"].astype(np.float64)).max())
        else:                                                        # against the recording itself: its samples and its sum
            rec['vs_recording'] = float(np.abs(h.reshape(-1)[idx].double().numpy() - gold[key + "tap_" + name].astype(np.float64)).max())
            rec['sum_err'] = abs(float(h.double().sum()) - float(gold[key + "sum_" + name]))
        record("disc_forward", case=case_id(case, variant), tap=name, **rec)
        print(case_id(case, variant), name, {k: f"{v:.2e}" for k, v in rec.items()})
        assert rec['top'] > 0
        # |hip - recording| <= |hip - f64| + |f32 - f64|, element by element and summed (the recording is a float32 CPU run like the yardstick)
        ok = rec['err'] <= rec['bound'] and rec['vs_recording'] <= rec['bound'] + rec['f32']
        if name != "logits":
            ok = ok and rec['sum_err'] <= h.numel() * (rec['bound'] + rec['f32'])
        if not ok:
            failed.append((name, rec))
    assert not failed, failed


@pytest.mark.gpu
@pytest.mark.parametrize("init,size", [(16, 16), (256, 256)])
def test_forward_is_reproducible_batch_independent_and_the_saving_form_is_identical(init, size):
    mg = module_gpu(init, 1)
    n = 4 if init == 16 else 2
    x = golden_images(n, size).to(DEV)
    a, b = mg.run(x, taps=True), mg.run(x, taps=True)
    with torch.no_grad():
        logits, taps, saved = mg._launch_forward(x, taps=True, save=True)
        alone = mg.run(x[1:2].contiguous(), taps=True)
    torch.cuda.synchronize()
    assert torch.equal(a['logits'], b['logits']) and torch.equal(a['logits'], logits)
    for t in a['taps']:
        assert torch.equal(a['taps'][t], b['taps'][t]), t            # two runs
        assert torch.equal(a['taps'][t], taps[t]), t                 # the state-saving forward
        if t < _lib.DISC_MAX_BLOCKS:                                 # pre-stddev features: alone and inside a batch
            assert torch.equal(a['taps'][t][1:2], alone['taps'][t]), t
    assert saved is not None and float(saved.view(torch.float32).abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("case,variant", sorted(BACKWARD, key=str), ids=lambda v: case_id(v) if isinstance(v, tuple) else str(v))
def test_whole_backward_matches_float64_with_pinned_branches(case, variant):
    init, cm, B, size = case
    x, u, hip, t64, t32 = whole_case(case, variant)
    flips, worst, near5, total = 0, 0.0, 0, 0
    assert len(hip['masks']) == len(t64['pre'])
    for mask, p64 in zip(hip['masks'], t64['pre']):
        assert mask.shape == p64.shape
        diff = mask != (p64 > 0)
        flips += int(diff.sum())
        if diff.any():
            worst = max(worst, float(p64[diff].abs().max()))
        near5 += int((p64.abs() < 1e-5).sum())
        total += p64.numel()
    rec = dict(flips=flips, worst_flip=worst, near_1e5=near5, lrelu_inputs=total)
    record("disc_backward_masks", case=case_id(case, variant), **rec)
    print(case_id(case, variant), rec)
    assert worst <= 1e-4, rec                                                        # (a)
    assert flips <= near5, rec                                                       # (b)
    order = [disc.TAP_FINAL] + list(range(len(module_cpu(init, cm).convs) - 2, -1, -1)) + [disc.TAP_STEM]
    failed = []
    for name, h, a, b in [(tap_name(t) if t != disc.TAP_STEM else "stem", hip['stages'][t], t64['stages'][t], t32['stages'][t]) for t in order] + \
                         [("image", hip['grad'], t64['grad'], t32['grad'])]:
        assert h.shape == a.shape, name
        top = float(a.abs().max())
        assert top > 0, name
        r = dict(err=dist(h, a) / top, f32=dist(b, a) / top, top=top)
        r['bound'] = max(5e-5, 3 * r['f32'])
        record("disc_backward", case=case_id(case, variant), stage=name, **r)
        print(case_id(case, variant), name, {k: f"{v:.2e}" for k, v in r.items()})
        if r['err'] > r['bound']:
            failed.append((name, r))
    assert not failed, failed


@pytest.mark.gpu
def test_asymmetric_blur_kernel_forward_and_backward_match_float64():
    """Every Blur.kernel of the discriminator is make_kernel([1, 3, 3, 1]): equal to its own 180-degree flip, so the flipped copy the
    backward reads (disc.hip: blur_flip) is the same image as the forward's and a dropped or doubled flip changes no bit of any other
    test.  Here the asymmetric 4 x 4 FIR of tests/test_fir_host.py (mixed signs, not rank one, sum|k| = 1) is written into every
    Blur.kernel of a GPU, a float32 CPU and a float64 CPU module of case d16c1b4s16: forward taps and logits by conv_bound, the backward's
    stage gradients and the image gradient by max(5e-5, 3 f32) relative with the branches pinned to the HIP forward's and the flip
    conditions (a) and (b) of this file."""
    from e3dge_amd.stylesdf_model import Blur
    from test_fir_host import asym_fir
    case = (16, 1, 4, 16)
    init, cm, B, size = case
    k32 = asym_fir().float()
    assert float((k32 - k32.flip(0, 1)).abs().max()) > 0.5 * float(k32.abs().max())

    def make(dtype, dev):
        m = syn.load_synthetic_discriminator(Discriminator(syn.discriminator_opt(init, cm))).to(dtype).to(dev)
        for p in m.parameters():
            p.requires_grad_(False)
        blurs = [mod for mod in m.modules() if isinstance(mod, Blur)]
        assert len(blurs) == 2 * (len(m.convs) - 1)
        with torch.no_grad():
            for mod in blurs:
                assert tuple(mod.kernel.shape) == (4, 4) and abs(float(mod.kernel.sum()) - 1) < 1e-6
                mod.kernel.copy_(k32.to(dtype))                       # the same fp32 taps in every precision
        return m
    mg, m32, m64 = make(torch.float32, DEV), make(torch.float32, "cpu"), make(torch.float64, "cpu")
    x, u = golden_images(B, size), upstream_of(B)
    assert mg.uses_hip(x.to(DEV))
    hip = mg.run(x.to(DEV), taps=True)
    b = mg.run_backward(x.to(DEV), u.to(DEV), stages=True)
    torch.cuda.synchronize()
    assert torch.equal(b['logits'], hip['logits'])
    masks = masks_of(mg, b['saved'], B)
    t64, t32 = pinned_run(m64, x, masks, u), pinned_run(m32, x, masks, u)
    sym64 = pinned_run(module_f64(init, cm), x, None, u)
    moved = dict(logits=dist(sym64['logits'], t64['logits']), grad=dist(sym64['grad'], t64['grad']) / float(t64['grad'].abs().max()))
    failed = []
    for name, h, a, c in [("logits", hip['logits'], t64['logits'], t32['logits'])] + \
                         [(tap_name(t), hip['taps'][t], t64['taps'][t], t32['taps'][t]) for t in sorted(hip['taps'])]:
        assert h.shape == a.shape, name
        rec = dict(err=dist(h, a), f32=dist(c, a), bound=conv_bound(a, c), top=float(a.abs().max()))
        record("disc_asym_blur_forward", tap=name, **rec)
        if not (rec['top'] > 0 and rec['err'] <= rec['bound']):
            failed.append((name, rec))
    flips, worst, near5 = 0, 0.0, 0
    assert len(masks) == len(t64['pre'])
    for mask, p64 in zip(masks, t64['pre']):
        diff = mask != (p64 > 0)
        flips += int(diff.sum())
        if diff.any():
            worst = max(worst, float(p64[diff].abs().max()))
        near5 += int((p64.abs() < 1e-5).sum())
    record("disc_asym_blur_masks", flips=flips, worst_flip=worst, near_1e5=near5, truth_moved_logits=moved['logits'], truth_moved_grad=moved['grad'])
    order = [disc.TAP_FINAL] + list(range(len(m32.convs) - 2, -1, -1)) + [disc.TAP_STEM]
    for name, h, a, c in [(tap_name(t) if t != disc.TAP_STEM else "stem", b['stages'][t], t64['stages'][t], t32['stages'][t]) for t in order] + \
                         [("image", b['grad'], t64['grad'], t32['grad'])]:
        assert h.shape == a.shape, name
        top = float(a.abs().max())
        r = dict(err=dist(h, a) / top, f32=dist(c, a) / top, top=top)
        r['bound'] = max(5e-5, 3 * r['f32'])
        record("disc_asym_blur_backward", stage=name, **r)
        if not (top > 0 and r['err'] <= r['bound']):
            failed.append((name, r))
    assert moved['grad'] > 0.05, moved                                # the asymmetric kernel is felt: 1000 x the backward's bound
    assert worst <= 1e-4 and flips <= near5, (flips, worst, near5)    # (a), (b)
    assert not failed, failed


@pytest.mark.gpu
def test_generator_loss_backward_through_the_pool_from_a_1024_leaf():
    """g_nonsaturating_loss(D(x)).backward() through the autograd Function, pool_256's adjoint included."""
    init, cm, B, size = 256, 1, 2, 1024
    mg = module_gpu(init, cm)
    x = golden_images(B, size)
    leaf = x.to(DEV).requires_grad_(True)
    logits = mg(leaf)
    assert logits.requires_grad and type(logits.grad_fn).__name__.startswith("_DiscriminatorFunction")
    losses.g_nonsaturating_loss(logits).backward()
    saved = mg.run_backward(x.to(DEV), upstream_of(B).to(DEV))['saved']           # the same forward: its branches
    torch.cuda.synchronize()
    masks = masks_of(mg, saved, B)
    t64 = pinned_run(module_f64(init, cm), x, masks)
    t32 = pinned_run(module_cpu(init, cm), x, masks)
    flips = sum(int((m != (p > 0)).sum()) for m, p in zip(masks, t64['pre']))
    near5 = sum(int((p.abs() < 1e-5).sum()) for p in t64['pre'])
    worst = max([float(p[m != (p > 0)].abs().max()) for m, p in zip(masks, t64['pre']) if bool((m != (p > 0)).any())] or [0.0])
    top = float(t64['grad'].abs().max())
    rec = dict(err=dist(leaf.grad, t64['grad']) / top, f32=dist(t32['grad'], t64['grad']) / top, top=top, flips=flips, near_1e5=near5, worst_flip=worst,
               logits=dist(logits.detach(), t64['logits']))
    rec['bound'] = max(5e-5, 3 * rec['f32'])
    record("disc_backward_pool1024", **rec)
    print({k: f"{v:.2e}" for k, v in rec.items()})
    assert leaf.grad.shape == x.shape and top > 0
    assert worst <= 1e-4 and flips <= near5, rec
    assert rec['err'] <= rec['bound'], rec
    with torch.no_grad():
        assert torch.equal(mg(leaf), logits.detach())                # the plain forward gives the same logits


@pytest.mark.gpu
def test_torch_path_with_trainable_parameters_still_trains_on_the_gpu():
    """Smoke check of the D-step against its own CPU run: library convolutions and the differentiable stream ops; 1e-3 relative leaves
    room for another summation order in every float32 layer and nothing else."""
    cpu = syn.load_synthetic_discriminator(Discriminator(syn.discriminator_opt(16, 1)))
    gpu = syn.load_synthetic_discriminator(Discriminator(syn.discriminator_opt(16, 1))).to(DEV)
    out = {}
    for name, m, dev in [("cpu", cpu, "cpu"), ("gpu", gpu, DEV)]:
        real = golden_images(2, 16).to(dev).requires_grad_(True)
        assert not m.uses_hip(real)
        pred = m(real)
        r1 = losses.d_r1_loss(pred, real)
        (losses.d_logistic_loss(pred, m(golden_images(2, 16).flip(0).to(dev))) + 5.0 * r1).backward()
        out[name] = dict(pred=pred.detach().cpu(), r1=r1.detach().cpu(), grads=[p.grad.cpu() for p in m.parameters()])
    torch.cuda.synchronize()
    rel = lambda a, b: dist(a, b) / max(float(b.abs().max()), 1e-30)
    rec = dict(pred=rel(out['gpu']['pred'], out['cpu']['pred']), r1=rel(out['gpu']['r1'], out['cpu']['r1']),
               grads=max(rel(a, b) for a, b in zip(out['gpu']['grads'], out['cpu']['grads'])))
    record("disc_torch_path_gpu", **rec)
    print({k: f"{v:.2e}" for k, v in rec.items()})
    assert float(out['gpu']['r1']) > 0 and all(float(g.abs().max()) > 0 for g in out['gpu']['grads'])
    assert max(rec.values()) <= 1e-3, rec
