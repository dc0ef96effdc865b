"""LPIPS backward on the HIP kernels (csrc/lpips_bwd.h, LPIPS.run_backward and LPIPS(differentiable=True)) against torch.autograd
through the plain-torch restatement of tests/test_gpu_lpips.py on the CPU: once in float64 (truth), once in float32 (the yardstick).

Bound (gradients):  max|hip - f64| / max|f64| <= max(5e-5, 3 x the float32 restatement's).

The gradient passes through step functions (ReLU, the pool's argmax), so a pre-activation or a pool window's top-two gap within
rounding of zero makes float32 and float64 take different branches: a property of the input, not of the kernels.  Every case therefore
first asserts, on the CPU truth, |pre-activation| >= 5e-6 everywhere and a top-two gap >= 1e-5 in every pool window with a positive
maximum.  A case that fails this gets another seed, never a wider bound."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import record

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, graphs, synthetic as syn
from e3dge_amd.lpips import LPIPS, CONVS, tap_shapes

from test_gpu_lpips import check_network_is_alive, make_pair, module_cpu, restate

CASES = [((1, 3, 31, 31), 66),        # 1x1 maps at conv 3..5: the 3x3 data gradients see only padding
         ((2, 3, 67, 67), 139),
         ((3, 3, 95, 71), 1)]         # non-square, N not a multiple of 16
CASE_IDS = ["x".join(map(str, s)) + f"-s{seed}" for s, seed in CASES]
MIN_PRE, MIN_GAP = 5e-6, 1e-5


def restate_grad(sd, x, y, dtype):
    """restate() of tests/test_gpu_lpips.py, operation for operation, with the five pre-activations kept: dict(per_image (B,), total (),
    pre: the five conv outputs before the ReLU (2B, C, H, W), x, y: the leaves)."""
    g = lambda k: sd[k].to(dtype)
    x, y = x.detach().clone().to(dtype).requires_grad_(True), y.detach().clone().to(dtype).requires_grad_(True)
    B = x.shape[0]
    z = (torch.cat([x, y]) - g('net.mean')) / g('net.std')
    taps, pre = [], []
    for i in range(11):
        if i in CONVS:
            _, _, _, s, p = CONVS[i]
            a = F.conv2d(z, g(f'net.layers.{i}.weight'), g(f'net.layers.{i}.bias'), stride=s, padding=p)
            pre.append(a)
            z = F.relu(a)
            taps.append(z / (torch.sqrt(torch.sum(z ** 2, dim=1, keepdim=True) + 1e-8) + 1e-10))
        elif i in (2, 5):
            z = F.max_pool2d(z, 3, 2)
    per_layer = torch.stack([F.conv2d((t[:B] - t[B:]) ** 2, g(f'lin.{l}.1.weight')).mean((1, 2, 3)) for l, t in enumerate(taps)], 1)
    return dict(per_image=per_layer.sum(1), total=per_layer.sum() / B, pre=pre, x=x, y=y)


def upstream(B):
    return torch.linspace(0.5, 1.5, B)


def grads_of(sd, pred, gt, dtype):
    """dict(gx, gy, pre: the gradients at the five pre-activations) for u = linspace(0.5, 1.5, B) through per_image, and (mx, my) through
    the scalar mean, all float64 on the CPU."""
    r = restate_grad(sd, pred, gt, dtype)
    B = pred.shape[0]
    leaves = [r['x'], r['y']] + r['pre']
    got = torch.autograd.grad((r['per_image'] * upstream(B).to(dtype)).sum(), leaves, retain_graph=True)
    mx, my = torch.autograd.grad(r['total'], [r['x'], r['y']])
    d = lambda t: t.detach().double()
    return dict(gx=d(got[0]), gy=d(got[1]), pre=[d(t) for t in got[2:]], mx=d(mx), my=d(my), per_image=d(r['per_image']),
                pre_values=[d(t) for t in r['pre']])


@functools.lru_cache(maxsize=None)
def case(shape, seed):
    """(pred, gt, float64 truth, float32 yardstick) on the CPU, computed once per case and shared; never modified."""
    pred, gt = make_pair(shape, seed)
    sd = module_cpu().state_dict()
    truth = grads_of(sd, pred, gt, torch.float64)
    truth['forward'] = restate(sd, pred, gt, torch.float64)
    return pred, gt, truth, grads_of(sd, pred, gt, torch.float32)


def check_no_near_ties(truth):
    """The conditions of the module docstring, on the float64 truth."""
    assert torch.equal(truth['per_image'], truth['forward']['per_image'].double())          # restate_grad IS restate
    check_network_is_alive(truth['forward'])
    for l, a in enumerate(truth['pre_values']):
        assert float(a.abs().min()) >= MIN_PRE, f"conv {l + 1}: a pre-activation of {float(a.abs().min()):.1e}"
    for l in range(2):
        f = F.relu(truth['pre_values'][l])
        n, c, h, w = f.shape
        win = F.unfold(f.reshape(n * c, 1, h, w), 3, stride=2)                               # (n c, 9, windows)
        top = win.topk(2, dim=1).values
        gap = (top[:, 0] - top[:, 1])[top[:, 0] > 0]
        assert float(gap.min()) >= MIN_GAP, f"pool {l + 1}: a window whose two largest values differ by {float(gap.min()):.1e}"


@functools.lru_cache(maxsize=None)
def module_gpu():
    return syn.load_synthetic_lpips(LPIPS()).to("cuda:0")


@functools.lru_cache(maxsize=None)
def module_gpu_differentiable():
    return syn.load_synthetic_lpips(LPIPS(differentiable=True)).to("cuda:0")


def rel(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def bound(f32):
    return max(5e-5, 3 * f32)


# ---- parity --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["x", "y", "both"])
@pytest.mark.parametrize("shape,seed", CASES, ids=CASE_IDS)
def test_input_gradients_match_float64_autograd(shape, seed, which):
    pred, gt, truth, f32 = case(shape, seed)
    check_no_near_ties(truth)
    want_x, want_y = which in ("x", "both"), which in ("y", "both")
    p, g, B = pred.cuda(), gt.cuda(), shape[0]
    gx, gy, _ = module_gpu().run_backward(p, g, upstream(B).cuda(), want_x=want_x, want_y=want_y)
    assert (gx is None) == (not want_x) and (gy is None) == (not want_y)
    m = module_gpu_differentiable()
    xa, ya = p.clone().requires_grad_(want_x), g.clone().requires_grad_(want_y)
    m(xa, ya).backward()                                                                    # once more through the scalar mean
    torch.cuda.synchronize()
    assert (xa.grad is None) == (not want_x) and (ya.grad is None) == (not want_y)
    rec = {}
    for name, got, key in (("x_per_image", gx, "gx"), ("y_per_image", gy, "gy"), ("x_mean", xa.grad, "mx"), ("y_mean", ya.grad, "my")):
        if got is not None:
            assert got.shape == shape and got.is_contiguous()
            rec[name + "_err"], rec[name + "_f32"] = rel(got, truth[key]), rel(f32[key], truth[key])
    record("lpips_bwd_parity", shape=list(shape), seed=seed, which=which, **rec)
    print(shape, seed, which, {k: f"{v:.2e}" for k, v in rec.items()})
    for name in [k[:-4] for k in rec if k.endswith("_err")]:
        assert rec[name + "_err"] <= bound(rec[name + "_f32"]), (name, rec)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,seed", CASES, ids=CASE_IDS)
def test_every_stage_matches_float64_autograd(shape, seed):
    """gpre[l] against autograd's gradient at the float64 restatement's pre-activation l: a failure names its layer."""
    pred, gt, truth, f32 = case(shape, seed)
    check_no_near_ties(truth)
    B = shape[0]
    p, g, u = pred.cuda(), gt.cuda(), upstream(B).cuda()
    m = module_gpu()
    _, _, both = m.run_backward(p, g, u, want_x=True, want_y=True, gpre=True)
    _, _, only_y = m.run_backward(p, g, u, want_x=False, want_y=True, gpre=True)
    torch.cuda.synchronize()
    rec = {}
    for l, (c, h, w) in enumerate(tap_shapes(*shape[2:])):
        assert both[l].shape == (2 * B, c, h, w) and only_y[l].shape == (B, c, h, w)
        rec[f"g{l + 1}_err"], rec[f"g{l + 1}_f32"] = rel(both[l], truth['pre'][l]), rel(f32['pre'][l], truth['pre'][l])
        assert torch.equal(only_y[l], both[l][B:]), f"G_{l + 1} of y depends on whether x gets a gradient"
    record("lpips_bwd_parity", shape=list(shape), seed=seed, which="stages", **rec)
    print(shape, seed, {k: f"{v:.2e}" for k, v in rec.items()})
    for l in range(4, -1, -1):                                                              # in the order the backward runs
        assert rec[f"g{l + 1}_err"] <= bound(rec[f"g{l + 1}_f32"]), (f"G_{l + 1}", rec)


# ---- exact properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_identity_repeatability_symmetry_and_batch_independence():
    shape, seed = CASES[2]
    pred, gt, truth, _ = case(shape, seed)
    check_no_near_ties(truth)
    m = module_gpu()
    p, g, u = pred.cuda(), gt.cuda(), upstream(3).cuda()
    zx, zy, zg = m.run_backward(p, p, u, want_x=True, want_y=True, gpre=True)
    assert (zx == 0).all() and (zy == 0).all() and all((t == 0).all() for t in zg)         # LPIPS(p, p) is a minimum
    ax, ay, ag = m.run_backward(p, g, u, want_x=True, want_y=True, gpre=True)
    bx, by, bg = m.run_backward(p, g, u, want_x=True, want_y=True, gpre=True)
    assert float(ax.abs().max()) > 0 and float(ay.abs().max()) > 0
    assert torch.equal(ax, bx) and torch.equal(ay, by) and all(torch.equal(s, t) for s, t in zip(ag, bg))      # two calls
    _, sy, _ = m.run_backward(g, p, u, want_x=False, want_y=True)
    assert torch.equal(ax, sy)                                                              # grad_x of (p, g) == grad_y of (g, p)
    sx, _, _ = m.run_backward(g, p, u, want_x=True, want_y=False)
    assert torch.equal(ay, sx)
    for i in range(3):                                                                      # a pair's gradient does not depend on its batch
        ox, oy, _ = m.run_backward(p[i:i + 1], g[i:i + 1], u[i:i + 1], want_x=True, want_y=True)
        assert torch.equal(ox[0], ax[i]) and torch.equal(oy[0], ay[i]), i
    # the forward under autograd is the forward
    d = module_gpu_differentiable()
    plain = m.run(p, g)
    with torch.enable_grad():
        graph = d.run(p.clone().requires_grad_(True), g)
    assert graph['per_image'].requires_grad and graph['mean'].requires_grad
    assert torch.equal(graph['per_image'].detach(), plain['per_image']) and torch.equal(graph['mean'].detach(), plain['mean'])


@pytest.mark.gpu
def test_wide_tiles_give_the_single_pair_gradient():
    """(10, 3, 256, 256) with both gradients: 20 gradient images, so the data-gradient launches of conv 5, 4 (4500 pixels, 4 and 6 channel
    tiles) and conv 2 (19220 pixels) take 64-pixel tiles and that of conv 3 (4500 pixels, 3 channel tiles) 32-pixel tiles under the
    forward's width rule, which the backward keeps; a single pair takes 16-pixel tiles in all four.  No float64 truth at
    this size: near-ties are unavoidable there."""
    pred, gt = make_pair((10, 3, 256, 256), seed=7)
    m = module_gpu()
    p, g = pred.cuda(), gt.cuda()
    u = upstream(10).cuda()
    ax, ay, _ = m.run_backward(p, g, u, want_x=True, want_y=True)
    assert float(ax.abs().max()) > 0
    for i in (0, 4, 9):
        ox, oy, _ = m.run_backward(p[i:i + 1], g[i:i + 1], u[i:i + 1], want_x=True, want_y=True)
        assert torch.equal(ox[0], ax[i]) and torch.equal(oy[0], ay[i]), i


# ---- autograd --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_autograd_adds_the_gradient_to_the_other_loss_terms():
    shape, seed = CASES[1]
    pred, gt, _, _ = case(shape, seed)
    B = shape[0]
    m = syn.load_synthetic_lpips(LPIPS()).to("cuda:0")
    m.differentiable = True
    x, y = pred.cuda().requires_grad_(True), gt.cuda()
    loss = F.mse_loss(x, y) + 0.8 * m(x, y)
    loss.backward()
    assert y.grad is None and x.grad.shape == shape
    x2 = pred.cuda().requires_grad_(True)
    F.mse_loss(x2, y).backward()
    # 0.8 * run_backward: the backward is linear in the upstream, which the Function forms as g_mean / B on the device
    u = (torch.tensor(0.8, device="cuda:0") / B).expand(B).contiguous()
    lp, none, _ = m.run_backward(x.detach(), y, u)
    assert none is None and float(lp.abs().max()) > 0
    want = x2.grad.double() + lp.double()
    ulp = torch.abs(torch.nextafter(want.float(), torch.full_like(lp, float("inf"))) - want.float()).double()
    assert ((x.grad.double() - want).abs() <= ulp).all()
    # per_image feeds a graph as well, and both inputs may want a gradient
    xa, ya = pred.cuda().requires_grad_(True), gt.cuda().requires_grad_(True)
    w = upstream(B).cuda()
    (m(xa, ya, per_image=True) * w).sum().backward()
    gx, gy, _ = m.run_backward(xa.detach(), ya.detach(), w, want_x=True, want_y=True)
    assert torch.equal(xa.grad, gx) and torch.equal(ya.grad, gy)
    # once differentiable
    xb = pred.cuda().requires_grad_(True)
    first, = torch.autograd.grad(m(xb, y), xb, create_graph=True)
    with pytest.raises(RuntimeError):
        first.sum().backward()
    m.differentiable = False
    with pytest.raises(NotImplementedError, match="LPIPS backward"):
        m(xb, y)


@pytest.mark.gpu
def test_the_transposed_weight_image_follows_the_parameters():
    pred, gt = make_pair((1, 3, 67, 67), seed=5)
    m = syn.load_synthetic_lpips(LPIPS()).to("cuda:0")
    p, g, u = pred.cuda(), gt.cuda(), torch.ones(1, device="cuda:0")
    grad = lambda: m.run_backward(p, g, u)[0].clone()
    base = grad()
    with torch.no_grad():
        m.net.layers[3].weight[3, 2, 1, 1] += 0.25                                           # in place: the version counter moves
    after = grad()
    assert not torch.equal(after, base)
    m.net.layers[3].weight.data[5, 1, 2, 2] += 0.25                                          # through .data: no version bump ...
    assert torch.equal(grad(), after)
    _lib.invalidate(m)                                                                       # ... so the cache has to be told
    assert not torch.equal(grad(), after)


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_replay_equals_eager():
    pred, gt = make_pair((1, 3, 67, 67), seed=5)
    m = module_gpu()
    p, g, u = pred.cuda(), gt.cuda(), torch.full((1,), 0.75, device="cuda:0")
    ex, ey, _ = m.run_backward(p, g, u, want_x=True, want_y=True)
    ex, ey = ex.clone(), ey.clone()

    def fn(a, b, w):
        gx, gy, _ = m.run_backward(a, b, w, want_x=True, want_y=True)
        return gx, gy

    call = graphs.GraphedCall(fn, torch.zeros_like(p), torch.ones_like(g) * 0.5, torch.ones_like(u))
    replay = [t.clone() for t in call(p, g, u)]
    torch.cuda.synchronize()
    assert float(ex.abs().max()) > 0 and torch.equal(replay[0], ex) and torch.equal(replay[1], ey)
