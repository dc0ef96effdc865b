"""The backward of the hourglass image filter on the HIP kernels (csrc/hgfilter_bwd.h, e3dge_amd.hg_filter with differentiable=True)
against float64 autograd of the module's own torch composition on the CPU.

Single ops, per tensor (tests/test_gpu_hgfilter.py):  max|hip - f64| <= max(2e-6 max|f64|, 3 max|f32 - f64|)
The whole backward, per gradient tensor (tests/test_gpu_idloss_bwd.py):  max|hip - f64| / max|f64| <= max(5e-5, 3 x the float32 restatement's),
branch-pinned: the float64 truth and the float32 yardstick take every ReLU's branch from the HIP run (the library's own debug bytes,
e3dge_hgf_branch_bytes); how many branches differ from the unpinned float64 run is counted and recorded."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, record

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, hg_filter, synthetic as syn
from e3dge_amd.hg_filter import HGFilter, ResidualImageFilter
from test_gpu_hgfilter import CONV_CASES, DEV, bound_of, dist, norm_case, rnd
from test_hgfilter_host import golden_input


# ---- one data gradient at a time ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dgrad_case(name):
    """x, per-(image, channel) (a, b) with no a x + b within 1e-3 of zero (so the branch is the same in every precision), w, the upstream
    gradient inside a wider tensor where the forward case stores into a slice, an addend; float64 and float32 autograd of
    conv(relu(a x + b)) (or conv(x) where the forward case has no leading norm)."""
    n, ci, co, H, W, k, s, reflect, groups, bias, sl = CONV_CASES[name]
    rs = np.random.RandomState(1500 + sorted(CONV_CASES).index(name))
    d = dict(x=rnd(rs, n, ci, H, W), w=rnd(rs, co, ci, k, k, scale=(2.0 / (ci * k * k)) ** 0.5), ab=None)
    if groups:
        d['ab'] = torch.stack([rnd(rs, n, ci, scale=0.2, shift=1.0), rnd(rs, n, ci, scale=0.3)], -1).contiguous()
        a, b = d['ab'][..., 0, None, None].double(), d['ab'][..., 1, None, None].double()
        z = a * d['x'].double() + b
        d['x'] = torch.where(z.abs() < 1e-3, d['x'].double() + 0.01 / a, d['x'].double()).float()
        assert float((a * d['x'].double() + b).abs().min()) > 1e-3
    OH, OW = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    gc, g0 = sl if sl else (co, 0)
    d['g'] = rnd(rs, n, gc, OH, OW)
    d['addend'] = rnd(rs, n, ci, H, W) if sl or k == 7 else None

    def ref(dtype):
        x = d['x'].to(dtype).clone()
        z = (x * d['ab'][..., 0, None, None].to(dtype) + d['ab'][..., 1, None, None].to(dtype) if groups else x).requires_grad_(True)
        y = F.relu(z) if groups else z
        if reflect:
            y = F.pad(y, (1, 1, 1, 1), mode='reflect')
        w, b = d['w'].to(dtype).clone().requires_grad_(True), torch.zeros(co, dtype=dtype, requires_grad=True)
        out = F.conv2d(y, w, b, stride=s, padding=0 if reflect else k // 2)
        out.backward(d['g'][:, g0:g0 + co].to(dtype))
        return (z.grad if d['addend'] is None else d['addend'].to(dtype) + z.grad), w.grad, b.grad
    (d['f64'], d['w64'], d['b64']), (d['f32'], d['w32'], d['b32']) = ref(torch.float64), ref(torch.float32)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_one_data_gradient_matches_float64(name):
    n, ci, co, H, W, k, s, reflect, groups, bias, sl = CONV_CASES[name]
    d = dgrad_case(name)
    g = lambda t: None if t is None else t.to(DEV)
    gc, g0 = sl if sl else (co, 0)
    out = torch.full((n, ci, H, W), float('nan'), device=DEV)
    wfrag = torch.empty(((ci + 15) // 16 * 16) * ((co * k * k + 31) // 32 * 32), device=DEV)
    _lib.launch("e3dge_hgf_conv_dgrad", out, g(d['g']), g(d['w']), wfrag, g(d['x']) if groups else None, g(d['ab']), g(d['addend']), n, ci, co, H, W, k, s,
                int(reflect), gc, g0)
    torch.cuda.synchronize()
    got = out.cpu()
    bound = bound_of(d['f64'], d['f32'])
    border = torch.ones((H, W), dtype=torch.bool)
    border[2:-2, 2:-2] = False                                       # two rows: the mirror's extra taps land in row 1 and row H - 2
    rec = dict(err=dist(got, d['f64']), f32=dist(d['f32'], d['f64']), bound=bound, border_err=dist(got[..., border], d['f64'][..., border]),
               interior_err=dist(got[..., ~border], d['f64'][..., ~border]) if (~border).any() else 0.0)
    record("hgfilter_dgrad", case=name, **rec)
    print(name, {k_: f"{v:.2e}" for k_, v in rec.items()})
    assert rec['interior_err'] <= bound, rec
    assert rec['border_err'] <= bound, rec                           # a wrong mirror, or a gradient through a zero-padded tap, fails here
    assert float(d['f64'].std()) > 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_one_weight_gradient_matches_float64(name):
    n, ci, co, H, W, k, s, reflect, groups, bias, sl = CONV_CASES[name]
    d = dgrad_case(name)
    g = lambda t: None if t is None else t.to(DEV)
    gc, g0 = sl if sl else (co, 0)
    dw, db = torch.full((co, ci, k, k), float('nan'), device=DEV), torch.full((co,), float('nan'), device=DEV)
    ws = torch.empty(_lib.query("e3dge_hgf_wgrad_ws_floats", n, ci, co, H, W, k, s), device=DEV)
    _lib.launch("e3dge_hgf_conv_wgrad", dw, None if sl else db, g(d['g']), g(d['x']), g(d['ab']), n, ci, co, H, W, k, s, int(reflect), gc, g0, ws, ws.numel())
    torch.cuda.synchronize()
    border = torch.ones((k, k), dtype=torch.bool)                    # the taps that reach into the padding
    border[1:-1, 1:-1] = False
    rec = dict(err=dist(dw, d['w64']), f32=dist(d['w32'], d['w64']), bound=bound_of(d['w64'], d['w32']),
               border_err=dist(dw.cpu()[..., border], d['w64'][..., border]) if k > 1 else 0.0,
               bias_err=0.0 if sl else dist(db, d['b64']), bias_bound=bound_of(d['b64'], d['b32']))
    record("hgfilter_wgrad", case=name, **rec)
    print(name, {k_: f"{v:.2e}" for k_, v in rec.items()})
    assert rec['err'] <= rec['bound'] and rec['border_err'] <= rec['bound'], rec
    assert rec['bias_err'] <= rec['bias_bound'], rec
    assert float(d['w64'].std()) > 0.1


# ---- norm backward ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def norm_bwd_case(C, H, W, mean, instance):
    x, gamma, beta, groups, _, _ = norm_case(C, H, W, mean, instance)
    rs = np.random.RandomState(1900 + C + 7 * H + int(mean) + instance)
    gy, wide, add1 = rnd(rs, 2, C, H, W), rnd(rs, 2, C + 48, H, W), rnd(rs, 2, C, H, W)

    def ref(dt):
        xx, gm, bt = (t.to(dt).clone().requires_grad_(True) for t in (x, gamma, beta))
        F.group_norm(xx, groups, gm, bt, 1e-5).backward(gy.to(dt))
        return xx.grad, add1.to(dt) + (wide[:, 16:16 + C].to(dt) + xx.grad), gm.grad, bt.grad
    return x, gamma, groups, gy, wide, add1, ref(torch.float64), ref(torch.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("mean", [0.0, 100.0])
@pytest.mark.parametrize("C,H,W,instance", [(32, 4, 6, 0), (64, 5, 7, 0), (256, 32, 48, 0), (256, 4, 6, 0), (32, 32, 48, 0), (32, 5, 7, 1), (32, 32, 48, 1)])
def test_norm_backward_matches_float64(C, H, W, instance, mean):
    x, gamma, groups, gy, wide, add1, (g64, s64, dg64, db64), (g32, s32, dg32, db32) = norm_bwd_case(C, H, W, mean, instance)
    xg, gyg, gam = x.to(DEV), gy.to(DEV), gamma.to(DEV)
    coef = torch.empty((2, C, 5), device=DEV, dtype=torch.float64)
    plain, summed = torch.full((2, C, H, W), float('nan'), device=DEV), torch.full((2, C, H, W), float('nan'), device=DEV)
    dg, db = torch.full((C,), float('nan'), device=DEV), torch.full((C,), float('nan'), device=DEV)
    _lib.launch("e3dge_hgf_norm_bwd", plain, gyg, xg, gam, None, None, 0, 0, None, coef, dg, db, 2, C, 0, C, groups, H, W)
    _lib.launch("e3dge_hgf_norm_bwd", summed, gyg, xg, gam, None, wide.to(DEV), C + 48, 16, add1.to(DEV), coef, None, None, 2, C, 0, C, groups, H, W)
    rec = dict(err=dist(plain, g64), f32=dist(g32, g64), bound=bound_of(g64, g32), sum_err=dist(summed, s64), sum_bound=bound_of(s64, s32),
               dgamma_err=dist(dg, dg64), dgamma_bound=bound_of(dg64, dg32), dbeta_err=dist(db, db64), dbeta_bound=bound_of(db64, db32))
    record("hgfilter_norm_bwd", C=C, H=H, W=W, mean=mean, instance=instance, **rec)
    print(C, H, W, mean, instance, {k: f"{v:.2e}" for k, v in rec.items()})
    assert rec['err'] <= rec['bound'] and rec['sum_err'] <= rec['sum_bound'], rec
    assert rec['dgamma_err'] <= rec['dgamma_bound'] and rec['dbeta_err'] <= rec['dbeta_bound'], rec
    assert float(g64.std()) > 0.1 and float(dg64.std()) > 0.1


@pytest.mark.gpu
def test_norm_backward_through_its_own_relu():
    """The stem's norm: its activation is a tensor of its own, so the ReLU's branch multiplies g_y inside the norm backward."""
    x, gamma, beta, groups, _, _ = norm_case(64, 5, 7, 0.0, 0)
    rs = np.random.RandomState(77)
    gy = rnd(rs, 2, 64, 5, 7)
    y64 = F.group_norm(x.double(), groups, gamma.double(), beta.double(), 1e-5)
    x = torch.where(y64.abs() < 2e-3, x + 0.02, x)                   # no pre-activation within rounding of zero: one branch in every precision
    assert float(F.group_norm(x.double(), groups, gamma.double(), beta.double(), 1e-5).abs().min()) > 1e-4

    def ref(dt):
        xx = x.to(dt).clone().requires_grad_(True)
        F.relu(F.group_norm(xx, groups, gamma.to(dt), beta.to(dt), 1e-5)).backward(gy.to(dt))
        return xx.grad
    g64, g32 = ref(torch.float64), ref(torch.float32)
    xg = x.to(DEV)
    ab = torch.empty((2, 64, 2), device=DEV)
    _lib.launch("e3dge_hgf_norm", ab, xg, gamma.to(DEV), beta.to(DEV), 2, 64, 0, 64, groups, 5, 7)
    coef, got = torch.empty((2, 64, 5), device=DEV, dtype=torch.float64), torch.full((2, 64, 5, 7), float('nan'), device=DEV)
    _lib.launch("e3dge_hgf_norm_bwd", got, gy.to(DEV), xg, gamma.to(DEV), ab, None, 0, 0, None, coef, None, None, 2, 64, 0, 64, groups, 5, 7)
    rec = dict(err=dist(got, g64), f32=dist(g32, g64), bound=bound_of(g64, g32))
    record("hgfilter_norm_bwd_relu", **rec)
    assert rec['err'] <= rec['bound'], rec
    assert 0.1 < float((F.group_norm(x.double(), groups, gamma.double(), beta.double(), 1e-5) > 0).double().mean()) < 0.9      # both branches taken


# ---- pooling and up-sampling, adjoints ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(2, 2), (2, 3), (4, 6), (1, 2)])
def test_pool_and_bicubic_adjoints_match_float64(H, W):
    rs = np.random.RandomState(140 + 10 * H + W)
    g_up, g_pool, addend = rnd(rs, 2, 5, 2 * H, 2 * W), rnd(rs, 2, 5, H, W), rnd(rs, 2, 5, 2 * H, 2 * W)

    def ref(dt):
        low, big = torch.zeros(2, 5, H, W, dtype=dt, requires_grad=True), torch.zeros(2, 5, 2 * H, 2 * W, dtype=dt, requires_grad=True)
        F.interpolate(low, scale_factor=2, mode='bicubic', align_corners=True).backward(g_up.to(dt))
        F.avg_pool2d(big, 2, stride=2).backward(g_pool.to(dt))
        return low.grad, addend.to(dt) + big.grad
    (u64, p64), (u32, p32) = ref(torch.float64), ref(torch.float32)
    glow, gin = torch.full((2, 5, H, W), float('nan'), device=DEV), torch.full((2, 5, 2 * H, 2 * W), float('nan'), device=DEV)
    _lib.launch("e3dge_hgf_up_bwd", glow, g_up.to(DEV), 10, H, W)
    _lib.launch("e3dge_hgf_pool_bwd", gin, g_pool.to(DEV), addend.to(DEV), 10, 2 * H, 2 * W)
    # the adjoint of what the forward kernel computes: its matrix from unit impulses, one plane per low-resolution pixel
    eye = torch.eye(H * W, device=DEV).reshape(H * W, H, W).contiguous()
    cols = torch.empty((H * W, 2 * H, 2 * W), device=DEV)
    _lib.launch("e3dge_hgf_up_add", cols, torch.zeros_like(cols), eye, H * W, H, W)
    own = (cols.reshape(H * W, -1).double() @ g_up.to(DEV).reshape(10, -1).double().T).T.reshape(2, 5, H, W)
    fwd = F.interpolate(torch.eye(H * W, dtype=torch.float64).reshape(H * W, 1, H, W), scale_factor=2, mode='bicubic', align_corners=True)
    rec = dict(up_err=dist(glow, u64), up_bound=bound_of(u64, u32), up_vs_own_forward=dist(glow, own), forward_vs_torch=dist(cols, fwd[:, 0]),
               pool_err=dist(gin, p64), pool_bound=bound_of(p64, p32))
    record("hgfilter_pool_up_bwd", H=H, W=W, **rec)
    print(H, W, {k: f"{v:.2e}" for k, v in rec.items()})
    assert rec['up_err'] <= rec['up_bound'] and rec['pool_err'] <= rec['pool_bound'], rec
    assert rec['up_vs_own_forward'] <= rec['up_bound'], rec
    assert float(u64.std()) > 0.1


# ---- the whole backward -----------------------------------------------------------------------------------------------------------------
# name: (options, batch, height, width, through filter_maps from an image and a depth map, upstream gradient on normx)
BWD_CASES = {
    "A": (dict(num_stack=2, num_hourglass=2), 2, 32, 48, True, True),       # maps 8x12, lowest level 2x3; bl / al and the three-way fan-in of previous
    "B": (dict(num_stack=1, num_hourglass=3), 1, 32, 64, False, False),     # HGFilter alone; lowest level 1x2; normx's gradient absent
}


@functools.lru_cache(maxsize=None)
def bwd_module(name, dtype=torch.float32):
    return syn.load_synthetic_hgfilter(ResidualImageFilter(syn.pifu_opt(**BWD_CASES[name][0]), differentiable=True)).to(dtype).eval()       # trainable


@functools.lru_cache(maxsize=None)
def bwd_module_gpu(name):
    m = ResidualImageFilter(syn.pifu_opt(**BWD_CASES[name][0]), differentiable=True)
    m.load_state_dict(bwd_module(name).state_dict())
    return m.to(DEV).eval()


def used_parameters(m, name):
    """(key, parameter) of every parameter the forward of the case reads, in the order of the sources."""
    keys = {id(p): k for k, p in m.named_parameters()}                # (bn4 is also downsample.0: named_parameters lists it once, as bn4)
    src = m.image_filter.sources()
    if BWD_CASES[name][4]:
        src = src + hg_filter._front_sources(m.residual_conv) + hg_filter._front_sources(m.depth_conv)
    return [(keys[id(p)], p) for p in src]


def input_names(name):
    return ["image", "depth"] if BWD_CASES[name][4] else ["input"]


def grad_samples(numel, is_input):
    """The flat positions of a gradient tensor that tests/golden/hgfilter_grads.npz records: 256 of an input's, 64 of a parameter's."""
    return (np.arange(256 if is_input else 64, dtype=np.int64) * 2654435761 + 12345) % numel


@functools.lru_cache(maxsize=None)
def bwd_inputs(name):
    opts, n, H, W, through, with_normx = BWD_CASES[name]
    seed = 20 + sorted(BWD_CASES).index(name)
    inputs = (golden_input((n, 3, H, W), seed), golden_input((n, 1, H, W), 50 + seed)) if through else (golden_input((n, 64, H, W), seed),)
    rs = np.random.RandomState(2300 + seed)
    ups = [rnd(rs, n, 256, H // 4, W // 4) for _ in range(opts['num_stack'])] + [rnd(rs, n, 128, H // 4, W // 4) if with_normx else None]
    return inputs, ups


def run_backward(m, name, inputs, ups):
    """(the gradients to the inputs of the case, then to every used parameter; the outputs), from whichever path the module takes."""
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    outs, _, normx = m.filter_maps(*leaves) if BWD_CASES[name][4] else m.image_filter(leaves[0])
    pairs = [(o, g) for o, g in zip(list(outs) + [normx], ups) if g is not None]
    wrt = leaves + [p for _, p in used_parameters(m, name)]
    return torch.autograd.grad([o for o, _ in pairs], wrt, [g.to(o) for o, g in pairs], allow_unused=True), outs


def norms_in_branch_order(m, through):
    """The norm modules in the order of e3dge_hgf_branch_bytes (include/e3dge_hip.h)."""
    hg = m.image_filter
    blocks = [hg.conv2, hg.conv3, hg.conv4]
    for i in range(hg.num_modules):
        def level(d):
            q = hg._modules[f'm{i}']._modules
            inner = level(d - 1) if d > 1 else [q[f'b2_plus_{d}']]
            return [q[f'b1_{d}'], q[f'b2_{d}']] + inner + [q[f'b3_{d}']]
        blocks += level(hg.num_hourglass) + [hg._modules[f'top_m_{i}']]
    out = [hg.bn1]
    for b in blocks:
        out += [b.bn1, b.bn2, b.bn3] + ([b.bn4] if b.downsample is not None else [])
    out += [hg._modules[f'bn_end{i}'] for i in range(hg.num_modules)]
    if through:
        out += [net[1].conv[j] for net in (m.residual_conv, m.depth_conv) for j in (0, 3)]
    return out


def pinned_run(m, name, inputs, ups, masks):
    """run_backward with every ReLU's branch from `masks` ({norm module: bool tensor}; None: the run's own, which are returned)."""
    own, hooks = {}, []
    tiny = 1e-200 if inputs[0].dtype == torch.float64 else 1e-30

    def hook(mod, inp, out):
        own[mod] = (out > 0).detach()
        if masks is None:
            return None
        want = masks[mod]
        return out + (torch.where(want, out.clamp_min(tiny), out.clamp_max(0.0)) - out).detach()      # the branch pinned, the derivative untouched
    for q in m.modules():
        if isinstance(q, (torch.nn.GroupNorm, torch.nn.InstanceNorm2d)):
            hooks.append(q.register_forward_hook(hook))
    try:
        grads, _ = run_backward(m, name, inputs, ups)
    finally:
        for h in hooks:
            h.remove()
    return grads, own


@functools.lru_cache(maxsize=None)
def hip_backward(name):
    """(gradients, forward outputs, the run's ReLU branches as one byte tensor) of the HIP path."""
    inputs, ups = bwd_inputs(name)
    hg_filter._FilterNode.branches = got = []
    try:
        grads, outs = run_backward(bwd_module_gpu(name), name, [t.to(DEV) for t in inputs], ups)
        torch.cuda.synchronize()
    finally:
        hg_filter._FilterNode.branches = None
    assert len(got) == 1
    return [g.cpu() for g in grads], [o.detach() for o in outs], got[0].cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BWD_CASES))
def test_whole_backward_matches_branch_pinned_float64(name):
    through = BWD_CASES[name][4]
    inputs, ups = bwd_inputs(name)
    hip, _, branch = hip_backward(name)
    m64, m32 = bwd_module(name, torch.float64), bwd_module(name)
    in64 = [t.double() for t in inputs]
    free64, own = pinned_run(m64, name, in64, ups, None)
    order, masks64, off, differ, total = norms_in_branch_order(m64, through), {}, 0, 0, 0
    assert set(order) == set(own)
    for q in order:
        numel = own[q].numel()
        masks64[q] = branch[off:off + numel].reshape(own[q].shape).bool()
        assert bool((branch[off:off + numel] <= 1).all())
        differ += int((masks64[q] != own[q]).sum())
        total += numel
        off += (numel + 255) // 256 * 256
    assert off <= branch.numel() and differ <= 1e-3 * total, (differ, total)      # the bytes are this network's branches, not noise
    masks32 = dict(zip(norms_in_branch_order(m32, through), (masks64[q] for q in order)))
    t64, _ = pinned_run(m64, name, in64, ups, masks64)
    t32, _ = pinned_run(m32, name, list(inputs), ups, masks32)
    rec, ok = dict(branches=total, branches_differing_from_float64=differ), True
    names, gold = input_names(name), load_golden("hgfilter_grads")

    def against_the_recording(key, h, a, b):                         # the reference's own float32 autograd: the bound with 4 in place of 3
        flat, top = h.reshape(-1), float(a.abs().max())
        want = gold[f"{name}__{key}"].astype(np.float64)
        err = float(np.abs(flat[grad_samples(flat.numel(), key in names)].double().numpy() - want).max()) / top
        return err, max(5e-5, 4 * dist(b, a) / top)
    for key, h, a, b, f in zip(names, hip, t64, t32, free64):
        top = float(a.abs().max())
        rec[key + '_err'], rec[key + '_f32'], rec[key + '_unpinned'] = dist(h, a) / top, dist(b, a) / top, dist(h, f) / top
        rec[key + '_bound'] = max(5e-5, 3 * rec[key + '_f32'])
        rec[key + '_std'] = float(a.std())
        rec[key + '_rec_err'], rec[key + '_rec_bound'] = against_the_recording(key, h, a, b)
        ok &= rec[key + '_err'] <= rec[key + '_bound'] and h.shape == a.shape and h.dtype == torch.float32
        ok &= rec[key + '_rec_err'] <= rec[key + '_rec_bound']
    # every parameter the forward reads: the same bound per tensor; the record keeps the worst by kind
    keys = [k for k, _ in used_parameters(m64, name)]
    assert len(hip) == len(names) + len(keys) and all(t is not None for t in list(hip) + list(t64))
    failed, worst = [], {}
    for key, h, a, b in zip(keys, hip[len(names):], t64[len(names):], t32[len(names):]):
        top = float(a.abs().max())
        assert top > 0 and h.shape == a.shape, key
        err, f32 = dist(h, a) / top, dist(b, a) / top
        bound = max(5e-5, 3 * f32)
        kind = "conv" if a.ndim == 4 else "vector"                  # convolution weights; norm weights and every bias
        if err / bound > worst.get(kind, (0.0,))[0]:
            worst[kind] = (err / bound, err, f32, bound, key)
        if err > bound:
            failed.append((key, err, bound))
        rec_err, rec_bound = against_the_recording(key, h, a, b)
        rec['worst_rec_ratio'] = max(rec.get('worst_rec_ratio', 0.0), rec_err / rec_bound)
        if rec_err > rec_bound:
            failed.append((key + " (recording)", rec_err, rec_bound))
    for kind, (ratio, err, f32, bound, key) in worst.items():
        rec.update({f"worst_{kind}_err": err, f"worst_{kind}_f32": f32, f"worst_{kind}_bound": bound, f"worst_{kind}": key})
    rec['parameters'] = len(keys)
    ok &= not failed
    record("hgfilter_bwd_parity", case=name, **rec)
    print(name, {k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in rec.items()})
    assert ok, (rec, failed[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BWD_CASES))
def test_saving_forward_equals_the_plain_forward(name):
    m = bwd_module_gpu(name)
    inputs, _ = bwd_inputs(name)
    _, outs, _ = hip_backward(name)
    with torch.no_grad():
        plain, _, _ = m.filter_maps(*[t.to(DEV) for t in inputs]) if BWD_CASES[name][4] else m.image_filter(inputs[0].to(DEV))
    assert len(plain) == len(outs) and all(torch.equal(a, b) for a, b in zip(plain, outs))


@pytest.mark.gpu
def test_two_backward_runs_are_bit_identical_and_an_image_does_not_depend_on_the_batch():
    inputs, ups = bwd_inputs("A")
    first, _, _ = hip_backward("A")
    m = bwd_module_gpu("A")
    again, _ = run_backward(m, "A", [t.to(DEV) for t in inputs], ups)
    alone, _ = run_backward(m, "A", [t[:1].to(DEV).contiguous() for t in inputs], [g[:1].contiguous() for g in ups])
    for i, (a, b, c) in enumerate(zip(first, again, alone)):
        assert torch.equal(a, b.cpu()), i                            # the inputs' and every parameter's
        if i < 2:
            assert torch.equal(a[:1], c.cpu())                       # the image's and the depth map's of image 0


# ---- routing ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_routing_of_the_differentiable_filter(monkeypatch):
    m = ResidualImageFilter(syn.pifu_opt(num_stack=1, num_hourglass=1))
    syn.load_synthetic_hgfilter(m)
    m = m.to(DEV).eval()
    rs = np.random.RandomState(3)
    image, depth = rnd(rs, 1, 3, 16, 16).to(DEV), rnd(rs, 1, 1, 16, 16).to(DEV)
    launched = []
    real = _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda n, *a: (launched.append(n), real(n, *a))[1])
    hgf = lambda: [n for n in launched if n.startswith("e3dge_hgf_") and not n.startswith("e3dge_hgf_pack_weights")]
    fwd, bwd = ["e3dge_hgf_front_saving", "e3dge_hgf_forward_saving"], ["e3dge_hgf_backward", "e3dge_hgf_front_backward"]
    out = m.filter(image, depth, return_feat=True)[0]                                                # the default, trainable: the torch composition
    assert not hgf() and out.requires_grad and not m.differentiable
    m.differentiable = True                                                                          # settable as an attribute
    out = m.filter(image, depth, return_feat=True)[0]                                                # a trainable parameter: forward and backward native
    assert hgf() == fwd and out.requires_grad
    out.square().mean().backward()
    assert hgf() == fwd + bwd
    used = {id(p) for p in m.image_filter.sources()} | {id(p) for net in (m.residual_conv, m.depth_conv) for p in net.parameters()}
    for k, p in m.named_parameters():                                                                # unused parameters end with grad None, as under autograd
        assert (p.grad is not None) == (id(p) in used), k
    assert any(p.grad is None for p in m.downsample_channel_conv.parameters()) and m.image_filter.conv3.bn4.weight.grad is None
    assert all(float(p.grad.abs().max()) > 0 for p in m.parameters() if p.grad is not None)
    m.differentiable = False
    m.zero_grad(set_to_none=True)
    del launched[:]
    for p in m.parameters():
        p.requires_grad_(False)
    assert not m.differentiable and not ResidualImageFilter(syn.pifu_opt(num_stack=1, num_hourglass=1)).image_filter.differentiable
    out = m.filter(image.clone().requires_grad_(True), depth, return_feat=True)[0]                   # the default: the torch composition under grad
    assert not hgf() and out.requires_grad
    m.differentiable = True
    assert m.image_filter.differentiable
    leaf = image.clone().requires_grad_(True)
    out = m.filter(leaf, depth, return_feat=True)[0]                                                 # frozen parameters, an image that requires grad
    assert hgf() == fwd and out.requires_grad and not m.tmpx.requires_grad
    out.sum().backward()
    assert hgf() == fwd + bwd and leaf.grad is not None and all(p.grad is None for p in m.parameters())
    with torch.no_grad():
        want = m.filter(image, depth, return_feat=True)[0]
    assert torch.equal(out.detach(), want)
    del launched[:]
    monkeypatch.setenv("E3DGE_HGFILTER", "torch")
    out = m.filter(leaf, depth, return_feat=True)[0]
    assert not hgf() and out.requires_grad
    monkeypatch.delenv("E3DGE_HGFILTER")
    out = m.filter(image, depth.clone().requires_grad_(True), return_feat=True)[0]                   # the depth map alone
    assert hgf() == fwd
    # through the options, as LocalFilterHead / SirenLocalGlobal hand it on
    assert ResidualImageFilter(syn.pifu_opt(num_stack=1, num_hourglass=1, differentiable_filter=True)).differentiable
    # HGFilter alone
    del launched[:]
    hg = HGFilter(syn.pifu_opt(num_stack=1, num_hourglass=1), differentiable=True).to(DEV).eval()
    for p in hg.parameters():
        p.requires_grad_(False)
    x = rnd(rs, 1, 64, 16, 16).to(DEV).requires_grad_(True)
    outs, tmpx, normx = hg(x)
    normx.sum().backward()                                                                           # normx's gradient alone: no stack runs backward
    assert hgf() == ["e3dge_hgf_forward_saving", "e3dge_hgf_backward"] and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0


@pytest.mark.gpu
def test_a_second_differentiation_raises():
    m = bwd_module_gpu("A")
    inputs, ups = bwd_inputs("A")
    leaf = inputs[0][:1].to(DEV).requires_grad_(True)
    outs, _, _ = m.filter_maps(leaf, inputs[1][:1].to(DEV))
    g, = torch.autograd.grad(outs[-1].sum(), leaf, create_graph=True, retain_graph=True)
    assert not g.requires_grad                                       # no graph behind the gradient: nothing silently differentiates it as a constant
    with pytest.raises(RuntimeError):
        g.sum().backward()
    up = torch.ones_like(outs[-1], requires_grad=True)               # an upstream gradient that itself requires grad
    g, = torch.autograd.grad(outs[-1], leaf, up, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


@pytest.mark.gpu
def test_after_an_optimiser_step_the_backward_uses_the_new_weights():
    """One SGD step, then a second forward / backward: the packed images are rebuilt (the gradient differs from the first step's) and the
    gradient matches float64 autograd of the UPDATED weights within the whole backward's bound (unpinned: see the recorded count of
    differing branches in test_whole_backward_matches_branch_pinned_float64)."""
    opts = dict(num_stack=1, num_hourglass=1)
    m = syn.load_synthetic_hgfilter(ResidualImageFilter(syn.pifu_opt(**opts), differentiable=True)).to(DEV).eval()
    rs = np.random.RandomState(11)
    image, depth, up = golden_input((1, 3, 16, 16), 31), golden_input((1, 1, 16, 16), 81), rnd(rs, 1, 256, 4, 4)
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    w = m.image_filter.conv4.conv1.weight

    def step():
        opt.zero_grad(set_to_none=True)
        outs, _, _ = m.filter_maps(image.to(DEV), depth.to(DEV))
        (outs[-1] * up.to(DEV)).sum().backward()
        return w.grad.clone()
    first = step()
    opt.step()
    second = step()
    assert not torch.equal(first, second)
    for dt in (torch.float64, torch.float32):
        c = ResidualImageFilter(syn.pifu_opt(**opts))
        c.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
        c = c.to(dt).eval()
        outs, _, _ = c.filter_maps(image.to(dt), depth.to(dt))
        (outs[-1] * up.to(dt)).sum().backward()
        if dt == torch.float64:
            t64 = c.image_filter.conv4.conv1.weight.grad
        else:
            t32 = c.image_filter.conv4.conv1.weight.grad
    top = float(t64.abs().max())
    rec = dict(err=dist(second, t64) / top, f32=dist(t32, t64) / top, moved=dist(second, first) / top)
    rec['bound'] = max(5e-5, 3 * rec['f32'])
    record("hgfilter_bwd_after_step", **rec)
    print({k: f"{v:.2e}" for k, v in rec.items()})
    assert rec['err'] <= rec['bound'] < rec['moved'], rec
