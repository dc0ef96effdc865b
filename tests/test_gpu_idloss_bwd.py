"""The identity term's backward on the HIP kernels (csrc/idnet_bwd.h, IDLoss(differentiable=True)) against float64 autograd on the CPU
(truth) and the same in float32 (the yardstick).

Bounds:  one data gradient, the prep adjoint   max|hip - f64| <= max(2e-6 max|f64|, 3 max|f32 - f64|)       (the forward's per-convolution bound)
         the whole backward, branch-pinned     max|hip - f64| / max|f64| <= max(5e-5, 3 x the float32 restatement's), image gradient and each
                                               of the eight stage gradients (test_gpu_lpips_bwd.py's bound for gradients)

Branch-pinned: the gradient passes through 3.7 M PReLU branch decisions per image, and a float64 pre-activation within the forward's
rounding of zero may legitimately take the other branch in fp32.  Truth and yardstick therefore take every PReLU derivative's branch
from the mask the HIP forward saved; the masks themselves are checked against the float64 forward: (a) every disagreement with
pre64 > 0 has |pre64| <= 1e-4, (b) there are at most as many as float64 elements with |pre64| < 1e-5, (c) every SE hidden
pre-activation of the truth has |pre| >= 1e-4."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import record

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, graphs, synthetic as syn
from e3dge_amd.id_loss import CROP, IDLoss, TAP_NAMES, TAP_UNITS, mask_shapes, tap_shapes
from test_idloss_host import golden_images, module_cpu


@functools.lru_cache(maxsize=None)
def module_f64():
    return syn.load_synthetic_idloss(IDLoss()).double()


@functools.lru_cache(maxsize=None)
def module_gpu():
    return syn.load_synthetic_idloss(IDLoss()).to("cuda:0")


@functools.lru_cache(maxsize=None)
def module_gpu_diff():
    return syn.load_synthetic_idloss(IDLoss(differentiable=True)).to("cuda:0")


def dist(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def guarded(shape, guard):
    """A NaN-filled output of `shape` with `guard` NaNs behind it: (the flat buffer, the view)."""
    numel = int(np.prod(shape))
    flat = torch.full((numel + guard,), float('nan'), device="cuda:0")
    return flat, flat[:numel].view(shape)


# ---- one data gradient at a time --------------------------------------------------------------------------------------------------
DGRAD_CASES = [  # n, Cin, Cout, H, W, kernel, stride, input affine, epilogue (None / 'mask' / 'scale'), addend
    (2, 3, 64, 9, 11, 3, 1, False, None, False),                     # the M = 3 form
    (3, 64, 64, 13, 13, 3, 2, False, 'scale', True),                 # odd size under stride 2: 7^2 -> 13^2
    (1, 64, 128, 8, 8, 1, 2, False, None, False),
    (2, 128, 128, 7, 7, 3, 1, True, 'mask', True),
    (1, 256, 512, 14, 14, 3, 1, False, None, False),                 # K = 4608
]


@functools.lru_cache(maxsize=None)
def dgrad_case(i):
    n, ci, co, H, W, k, s, in_aff, epi, add = DGRAD_CASES[i]
    OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
    rs = np.random.RandomState(200 + i)
    t = lambda *shape, scale=1.0, shift=0.0: torch.from_numpy(shift + scale * rs.standard_normal(shape)).float()
    d = dict(g=t(n, co, OH, OW), w=t(co, ci, k, k, scale=(2.0 / (ci * k * k)) ** 0.5))
    d['in_ab'] = torch.stack([t(n, co, scale=0.2, shift=1.0), t(n, co, scale=0.5, shift=0.3)], 2).contiguous() if in_aff else None   # b != 0
    d['mask'] = torch.from_numpy(rs.randint(0, 2, size=(n, ci, H, W)).astype(np.uint8)) if epi == 'mask' else None
    d['slope'] = t(ci, scale=0.3, shift=0.05) if epi == 'mask' else None                        # both signs
    d['scale'] = t(ci, scale=0.2, shift=1.0) if epi == 'scale' else None
    d['addend'] = t(n, ci, H, W) if add else None
    if epi == 'mask':
        assert float(d['slope'].min()) < 0 < float(d['slope'].max())

    def ref(dtype):
        g = d['g'].to(dtype)
        if in_aff:
            g = d['in_ab'][..., 0].to(dtype)[:, :, None, None] * g + d['in_ab'][..., 1].to(dtype)[:, :, None, None]
        x = torch.zeros(n, ci, H, W, dtype=dtype, requires_grad=True)
        out, = torch.autograd.grad(F.conv2d(x, d['w'].to(dtype), stride=s, padding=k // 2), x, g)
        if epi == 'mask':
            out = out * torch.where(d['mask'].bool(), torch.ones((), dtype=dtype), d['slope'].to(dtype)[None, :, None, None])
        if epi == 'scale':
            out = out * d['scale'].to(dtype)[None, :, None, None]
        if add:
            out = out + d['addend'].to(dtype)
        return out
    d['f64'], d['f32'] = ref(torch.float64), ref(torch.float32)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(DGRAD_CASES)), ids=lambda i: "x".join(map(str, DGRAD_CASES[i][:7])))
def test_one_data_gradient_matches_float64(i):
    n, ci, co, H, W, k, s, in_aff, epi, add = DGRAD_CASES[i]
    d = dgrad_case(i)
    c = lambda t: None if t is None else t.cuda()
    flat, out = guarded(d['f64'].shape, W)
    wfrag = torch.empty((ci + 15) // 16 * 16 * ((co * k * k + 31) // 32 * 32), device="cuda:0")
    _lib.launch("e3dge_idnet_conv_bwd", out, c(d['g']), c(d['w']), wfrag, c(d['in_ab']), c(d['mask']), c(d['slope']), c(d['scale']), c(d['addend']),
                n, ci, co, H, W, k, s)
    torch.cuda.synchronize()
    assert bool(torch.isnan(flat[out.numel():]).all()) and not bool(torch.isnan(out).any())   # the guard row is untouched, all is written
    err, f32 = dist(out, d['f64']), dist(d['f32'], d['f64'])
    bound = max(2e-6 * float(d['f64'].abs().max()), 3 * f32)
    border = torch.ones(H, W, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    rec = dict(err=err, f32=f32, bound=bound, border_err=dist(out.cpu()[..., border], d['f64'][..., border]))
    record("idloss_dgrad", case=list(DGRAD_CASES[i][:7]), **rec)
    print(DGRAD_CASES[i], {k_: f"{v:.2e}" for k_, v in rec.items()})
    assert float(d['f64'].abs().max()) > 0.1
    assert err <= bound, rec
    assert rec['border_err'] <= bound, rec                                           # an affine applied on the padding fails here


# ---- crop and pool ----------------------------------------------------------------------------------------------------------------
def prep(m, z):
    if z.shape[2] != 256:
        z = m.id_loss_pool(z)
    return m.face_pool(z[:, :, CROP[0]:CROP[1], CROP[2]:CROP[3]])


def pre_image(size):
    """Rows and columns of a size x size image that reach the crop: [lo, hi) each."""
    lo = lambda v: v * size // 256
    hi = lambda v: -(-v * size // 256)
    return lo(CROP[0]), hi(CROP[1]), lo(CROP[2]), hi(CROP[3])


def outside_is_zero(grad):
    r0, r1, c0, c1 = pre_image(grad.shape[2])
    inside = torch.zeros(grad.shape[2:], dtype=torch.bool, device=grad.device)
    inside[r0:r1, c0:c1] = True
    return bool((grad[..., ~inside] == 0).all()) and float(grad[..., inside].abs().min()) >= 0 and float(grad.abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("size", [256, 300, 1024])
def test_prep_adjoint_matches_float64(size):
    n = 2
    g = torch.from_numpy(np.random.RandomState(size).standard_normal((n, 3, 112, 112))).float()

    def ref(dtype):
        x = torch.zeros(n, 3, size, size, dtype=dtype, requires_grad=True)
        return torch.autograd.grad(prep(module_cpu(), x), x, g.to(dtype))[0]
    f64, f32 = ref(torch.float64), ref(torch.float32)
    flat, out = guarded(f64.shape, size)
    _lib.launch("e3dge_idnet_prep_bwd", out, g.cuda(), n, size, size)
    torch.cuda.synchronize()
    assert bool(torch.isnan(flat[out.numel():]).all()) and not bool(torch.isnan(out).any())
    rec = dict(err=dist(out, f64), f32=dist(f32, f64))
    rec['bound'] = max(2e-6 * float(f64.abs().max()), 3 * rec['f32'])
    record("idloss_prep_bwd", size=size, **rec)
    print(size, {k: f"{v:.2e}" for k, v in rec.items()})
    assert rec['err'] <= rec['bound'], rec
    assert outside_is_zero(out)
    r0, r1, c0, c1 = pre_image(size)
    assert outside_is_zero(f64) and bool((f64[:, :, r0:r1, c0:c1] != 0).all())       # the pre-image is exactly that rectangle


# ---- the whole backward, branch-pinned --------------------------------------------------------------------------------------------
class _PinnedPReLU(torch.autograd.Function):
    """F.prelu forward; the derivative's branch comes from `mask` (1: positive)."""

    @staticmethod
    def forward(ctx, x, slope, mask):
        ctx.save_for_backward(slope, mask)
        return F.prelu(x, slope)

    @staticmethod
    def backward(ctx, g):
        slope, mask = ctx.saved_tensors
        return g * torch.where(mask, torch.ones((), dtype=g.dtype), slope[None, :, None, None]), None, None


def pinned_backward(m, y_hat, y, upstream, masks):
    """Autograd through the torch layers of module `m` (its dtype) with every PReLU derivative pinned to `masks`: dict(grad, stages:
    the eight stage gradients, pre: the 25 PReLU inputs, hidden_min: the smallest |SE hidden pre-activation|)."""
    dtype = m.facenet.input_layer[0].weight.dtype
    f = m.facenet
    leaf = y_hat.to(dtype).clone().requires_grad_(True)
    with torch.no_grad():
        fy = f(prep(m, y.to(dtype)))
    pre, stages, hidden_min = [], [], float('inf')
    keep = lambda t: (t.retain_grad(), stages.append(t))
    z = prep(m, leaf)
    keep(z)
    x = f.input_layer[1](f.input_layer[0](z))
    pre.append(x.detach())
    x = _PinnedPReLU.apply(x, f.input_layer[2].weight, masks[0])
    keep(x)
    for u, unit in enumerate(f.body):
        r = unit.res_layer
        t = r[1](r[0](x))
        pre.append(t.detach())
        t = r[4](r[3](_PinnedPReLU.apply(t, r[2].weight, masks[1 + u])))
        hid = r[5].fc1(r[5].avg_pool(t))
        hidden_min = min(hidden_min, float(hid.detach().abs().min()))
        x = t * torch.sigmoid(r[5].fc2(F.relu(hid))) + unit.shortcut_layer(x)
        if u in TAP_UNITS:
            keep(x)
    v = f.output_layer(x)
    keep(v)
    fh = v / torch.norm(v, 2, 1, True)
    (upstream.to(dtype) * (1 - (fh * fy).sum(1))).sum().backward()
    return dict(grad=leaf.grad, stages=[s.grad for s in stages], pre=pre, hidden_min=hidden_min)


def upstream_of(n):
    return torch.linspace(0.5, 1.5, n) if n > 1 else torch.ones(1)


@functools.lru_cache(maxsize=None)
def bwd_case(n, size):
    """(pred, gt, upstream, the HIP result of run_backward with stages and masks, float64 truth, float32 yardstick), computed once."""
    pred, gt = golden_images(n, size)
    u = upstream_of(n)
    grad, gs, ms = module_gpu().run_backward(pred.cuda(), gt.cuda(), u.cuda(), stages=True, masks=True)
    torch.cuda.synchronize()
    hip = dict(grad=grad.cpu(), stages=[t.cpu() for t in gs], masks=[t.cpu().bool() for t in ms])
    t64 = pinned_backward(module_f64(), pred, gt, u, hip['masks'])
    t32 = pinned_backward(module_cpu(), pred, gt, u, hip['masks'])
    del t32['pre']
    return pred, gt, u, hip, t64, t32


FLIP_CAPS = {(1, 256): 35, (2, 256): 80, (1, 1024): 72}             # float64 elements with |pre64| < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("n,size", [(1, 256), (2, 256), (1, 1024)], ids=["n1", "n2", "pool1024"])
def test_whole_backward_matches_float64_with_pinned_branches(n, size):
    pred, gt, u, hip, t64, t32 = bwd_case(n, size)
    assert [tuple(m.shape) for m in hip['masks']] == mask_shapes(n) and [tuple(s.shape) for s in hip['stages']] == tap_shapes(n)
    # conditions on the masks, on the float64 forward
    flips, worst, near5, total = 0, 0.0, 0, 0
    for mask, p64 in zip(hip['masks'], t64['pre']):
        diff = mask != (p64 > 0)
        flips += int(diff.sum())
        if diff.any():
            worst = max(worst, float(p64[diff].abs().max()))
        near5 += int((p64.abs() < 1e-5).sum())
        total += p64.numel()
    rec = dict(flips=flips, worst_flip=worst, near_1e5=near5, prelu_inputs=total, hidden_min=t64['hidden_min'])
    assert total == 3713024 * n
    assert worst <= 1e-4, rec                                                        # (a)
    assert flips <= near5 and flips <= FLIP_CAPS[(n, size)], rec                    # (b)
    assert t64['hidden_min'] >= 1e-4, rec                                            # (c)
    # the gradients, in the order the backward runs
    trio = lambda key, i: (hip[key][i], t64[key][i], t32[key][i]) if i is not None else (hip[key], t64[key], t32[key])
    order = [("head", 'stages', 7)] + [(TAP_NAMES[i], 'stages', i) for i in range(6, -1, -1)] + [("image", 'grad', None)]
    failed = []
    for name, key, i in order:
        h, a, b = trio(key, i)
        top = float(a.abs().max())
        assert top > 0, name
        rec[name + '_err'], rec[name + '_f32'] = dist(h, a) / top, dist(b, a) / top
        if rec[name + '_err'] > max(5e-5, 3 * rec[name + '_f32']):
            failed.append(name)
    record("idloss_bwd_parity", n=n, size=size, **rec)
    print(n, size, {k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in rec.items()})
    assert not failed, (failed, rec)                                                 # the first name is the first stage that went wrong
    assert outside_is_zero(hip['grad'])
    # autograd through the module is the same launch sequence
    m = module_gpu_diff()
    if n > 1:
        return                                                                       # (upstream = 1 / B only; the n = 2 case has its own weights)
    y_hat = pred.cuda().requires_grad_(True)
    m(y_hat, gt.cuda(), gt.cuda())[0].backward()
    want = m.run_backward(pred.cuda(), gt.cuda(), torch.full((n,), 1.0 / n, device="cuda:0"))[0]
    assert torch.equal(y_hat.grad, want) and torch.equal(want, hip['grad'].cuda())


@pytest.mark.gpu
def test_autograd_equals_run_backward_for_a_batch():
    pred, gt = golden_images(2, 256)
    m = module_gpu_diff()
    y_hat, y = pred.cuda().requires_grad_(True), gt.cuda()
    m(y_hat, y, y)[0].backward()
    want = m.run_backward(pred.cuda(), y, torch.full((2,), 0.5, device="cuda:0"))[0]
    assert float(want.abs().max()) > 0 and torch.equal(y_hat.grad, want)


# ---- exact properties -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_repeatability_batch_independence_and_the_saving_forward():
    pred, gt = golden_images(2, 256)
    m, d = module_gpu(), module_gpu_diff()
    p, g = pred.cuda(), gt.cuda()
    u = torch.tensor([0.75, 1.25], device="cuda:0")
    a = m.run_backward(p, g, u, stages=True, masks=True)
    b = m.run_backward(p, g, u, stages=True, masks=True)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1] + a[2], b[1] + b[2]))        # two runs
    for i in range(2):                                                               # alone, and at the other position
        alone = m.run_backward(p[i:i + 1], g[i:i + 1], u[i:i + 1])[0]
        assert torch.equal(alone[0], a[0][i]), i
    swapped = m.run_backward(p.flip(0), g.flip(0), u.flip(0))[0]
    assert torch.equal(swapped.flip(0), a[0])
    assert outside_is_zero(a[0])
    # the saving forward's embeddings and taps are e3dge_idnet_embed's
    plain_emb, plain_taps = m._embed_sets([p, g], taps=True)
    save_emb, save_taps, _ = m._embed_sets([p, g], taps=True, n_saved=2)
    assert torch.equal(plain_emb, save_emb) and all(torch.equal(x, y) for x, y in zip(plain_taps, save_taps))
    save_one = m._embed_sets([p, g], n_saved=1)[0]                                   # fewer saved images than a set holds
    assert torch.equal(plain_emb, save_one)
    # a differentiable module under no_grad is the plain module; with grad it returns the same values
    plain = m.run(p, g)
    with torch.no_grad():
        quiet = d.run(p.clone().requires_grad_(True), g)
    yh, yy, xx = p.clone().requires_grad_(True), g.clone().requires_grad_(True), g.clone().requires_grad_(True)
    graph = d.run(yh, yy, xx)
    assert graph['loss'].requires_grad and not quiet['loss'].requires_grad and not graph['dots'].requires_grad
    for k in ('embeddings', 'dots', 'loss', 'sim_improvement'):
        assert torch.equal(plain[k], quiet[k]), k
        assert torch.equal(plain[k], graph[k].detach()[:len(plain[k])] if k == 'embeddings' else graph[k].detach()), k
    graph['loss'].backward()
    assert yy.grad is None and xx.grad is None and yh.grad is not None               # y and x never get a gradient
    assert torch.equal(yh.grad, m.run_backward(p, g, torch.full((2,), 0.5, device="cuda:0"))[0])
    with pytest.raises(NotImplementedError, match="backward is not in this build"):
        m.run(yh, g)


@pytest.mark.gpu
def test_the_transposed_weight_image_follows_the_parameters():
    pred, gt = golden_images(1, 256)
    m = syn.load_synthetic_idloss(IDLoss()).to("cuda:0")
    p, g, u = pred.cuda(), gt.cuda(), torch.ones(1, device="cuda:0")
    grad = lambda mod: mod.run_backward(p, g, u)[0].clone()
    base = grad(m)
    with torch.no_grad():
        m.facenet.body[5].res_layer[3].weight[3, 2, 1, 1] += 0.25                    # in place: the version counter moves
    after = grad(m)
    assert not torch.equal(after, base)
    m.facenet.body[9].res_layer[1].weight.data[5, 1, 2, 2] += 0.25                   # through .data: a conv weight,
    m.facenet.body[2].res_layer[0].running_var.data.mul_(1.5)                        # a BN statistic
    m.facenet.body[12].res_layer[2].weight.data.add_(0.2)                            # and a PReLU slope
    assert torch.equal(grad(m), after)
    _lib.invalidate(m)                                                               # the project's one weight cache has to be told
    moved = grad(m)
    assert not torch.equal(moved, after)
    fresh = IDLoss().to("cuda:0")
    fresh.load_state_dict(m.state_dict())
    assert torch.equal(grad(fresh), moved)


# ---- autograd ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_autograd_adds_the_gradient_to_the_other_loss_terms():
    pred, gt = golden_images(2, 256)
    m = module_gpu_diff()
    id_lambda, B = 0.1, 2
    x, y = pred.cuda().requires_grad_(True), gt.cuda()
    (F.mse_loss(x, y) + id_lambda * m(x, y, y)[0]).backward()
    x2 = pred.cuda().requires_grad_(True)
    F.mse_loss(x2, y).backward()
    u = (torch.tensor(id_lambda, device="cuda:0") / B).expand(B).contiguous()        # the backward is linear in the upstream
    term = m.run_backward(x.detach(), y, u)[0]
    assert float(term.abs().max()) > 0
    want = x2.grad.double() + term.double()
    ulp = torch.abs(torch.nextafter(want.float(), torch.full_like(term, float("inf"))) - want.float()).double()
    assert ((x.grad.double() - want).abs() <= ulp).all()
    first, = torch.autograd.grad(m(x, y, y)[0], x, create_graph=True)                # once differentiable
    with pytest.raises(RuntimeError):
        first.sum().backward()


# ---- graph capture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_replay_equals_eager():
    pred, gt = golden_images(1, 256)
    m = module_gpu()
    p, g, u = pred.cuda(), gt.cuda(), torch.full((1,), 0.75, device="cuda:0")
    eager = m.run_backward(p, g, u)[0].clone()                                       # (warm: both weight images exist)

    def fn(a, b, w):
        return m.run_backward(a, b, w)[0]

    call = graphs.GraphedCall(fn, torch.zeros_like(p), torch.ones_like(g) * 0.5, torch.ones_like(u))
    replay = call(p, g, u)
    replay = (replay[0] if isinstance(replay, (tuple, list)) else replay).clone()
    torch.cuda.synchronize()
    assert float(eager.abs().max()) > 0 and torch.equal(replay, eager)
