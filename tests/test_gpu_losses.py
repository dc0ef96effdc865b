"""The training loss on the HIP kernels of csrc/losses.hip (e3dge_amd.losses: AvgPool2d, LossClass) against float64.

Bound for every comparison with float64:  max|hip - f64| <= max(1e-6 max|f64|, 3 x max|torch float32 chain - f64|), the
float32 chain being the same torch operations on the same inputs.  Both distances go to conftest.record().  A comparison with the
recorded float32 reference values (tests/golden/losses_shape.npz) allows that bound plus the recording's own distance from float64.

Measured on the MI355X: every comparison passed; the closest is the LPIPS part of d pred at 64^2 (8.5e-11 against a bound of 9.3e-11,
three times the float32 chain's 3.1e-11), the pool and shape-term comparisons are decided by the 1e-6 floor with a factor of five or more to spare."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, maxerr, record

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, losses, synthetic as syn
from e3dge_amd.id_loss import IDLoss
from e3dge_amd.lpips import LPIPS
from e3dge_amd.sharded_eval import image_metrics_torch

from test_gpu_lpips import make_pair, module_cpu, restate
from test_losses_host import ALL_ON, LAMBDAS_A, PRED_KEYS, opt_of, shape_inputs

DEV = "cuda:0"


def check(name, got, truth, chain, extra=0.0, **info):
    """The module's bound; `truth` float64, `chain` the float32 torch chain.  Records before it asserts."""
    err, f32 = maxerr(got, truth), maxerr(chain, truth)
    bound = max(1e-6 * float(truth.detach().abs().max()), 3 * f32) + extra
    record("losses_" + name, err=err, f32_chain=f32, bound=bound, **info)
    print(name, info, f"err {err:.3e} f32 chain {f32:.3e} bound {bound:.3e}")
    assert err <= bound, (name, info, err, f32, bound)


# ---- pool ----------------------------------------------------------------------------------------------------------------------------
POOLS = [((2, 3, 32, 32), (8, 8)), ((1, 3, 64, 64), (64, 64)), ((1, 1, 48, 16), (24, 8)), ((1, 3, 1024, 1024), (256, 256))]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,out", POOLS, ids=lambda v: "x".join(map(str, v)))
def test_pool_forward_and_backward_match_float64(shape, out):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g).to(DEV).requires_grad_(True)
    up = torch.randn(shape[:2] + out, generator=g).to(DEV)
    pool = losses.AvgPool2d(out)
    f = pool.factor(x)
    assert f == shape[2] // out[0]
    y = pool(x)
    assert y.shape == shape[:2] + out and y.dtype == torch.float32
    y.backward(up)
    x32 = x.detach().clone().requires_grad_(True)
    y32 = F.adaptive_avg_pool2d(x32, out)
    y32.backward(up)
    y64 = F.adaptive_avg_pool2d(x.detach().double(), out)
    g64 = (up.double() / (f * f)).repeat_interleave(f, -2).repeat_interleave(f, -1)
    check("pool_fwd", y, y64, y32, shape=list(shape))
    check("pool_bwd", x.grad, g64, x32.grad, shape=list(shape))
    y2 = pool(x.detach())
    torch.cuda.synchronize()
    assert torch.equal(y2, y.detach())


@pytest.mark.gpu
def test_pool_takes_torch_for_strided_inputs_and_other_ratios():
    g = torch.Generator().manual_seed(5)
    pool = losses.AvgPool2d((8, 8))
    strided = torch.randn(2, 3, 32, 64, generator=g).to(DEV)[..., ::2]
    odd = torch.randn(1, 3, 20, 20, generator=g).to(DEV)
    for x in (strided, odd, torch.randn(1, 3, 32, 32, generator=g).to(DEV).double()):
        assert pool.factor(x) is None
        x = x.clone().requires_grad_(True) if x.is_contiguous() else x.requires_grad_(True)
        y = pool(x)
        assert torch.equal(y, F.adaptive_avg_pool2d(x, (8, 8)))
        gx, = torch.autograd.grad(y.sum(), x)
        assert gx.shape == x.shape
    x = torch.randn(1, 2, 16, 16, generator=g).to(DEV).requires_grad_(True)          # create_graph=True: the torch expression
    gx, = torch.autograd.grad(losses.AvgPool2d((4, 4))(x).pow(2).sum(), x, create_graph=True)
    assert gx.requires_grad
    x2 = x.detach().clone().requires_grad_(True)
    gx2, = torch.autograd.grad(F.adaptive_avg_pool2d(x2, (4, 4)).pow(2).sum(), x2, create_graph=True)
    assert maxerr(gx, gx2) <= 1e-6 * float(gx2.detach().abs().max())


# ---- shape terms ---------------------------------------------------------------------------------------------------------------------
def formulas(pred, gt, lam, flags):
    """builder.py:76-104 and gan_loss.py:18 as torch operations, in the dtype of the inputs: (total, dict of the enabled terms)."""
    d, total = {}, 0
    if flags.get("supervise_sdf") and lam["uniform_pts_sdf_lambda"] > 0:
        d["sdf_rec_loss"] = F.smooth_l1_loss(pred["uniform_points_sdf"].squeeze(), gt["uniform_points_sdf"].squeeze()) * lam["uniform_pts_sdf_lambda"]
        total = total + d["sdf_rec_loss"]
    if flags.get("supervise_surface") and lam["surf_sdf_lambda"] > 0:
        d["surf_rec_loss"] = F.smooth_l1_loss(pred["surface_sdf"], torch.zeros_like(pred["surface_sdf"])) * lam["surf_sdf_lambda"]
        total = total + d["surf_rec_loss"]
    if flags.get("supervise_surface_normal") and lam["surf_normal_lambda"] > 0:
        d["surface_norm_rec_loss"] = F.smooth_l1_loss(pred["surface_eikonal_term"].squeeze(), gt["surface_eikonal_term"].squeeze()) * lam["surf_normal_lambda"]
        total = total + d["surface_norm_rec_loss"]
    if flags.get("supervise_eikonal") and lam["eikonal_lambda"] > 0:
        d["eikonal_term"] = ((pred["eikonal_term"].norm(dim=-1) - 1) ** 2).mean() * lam["eikonal_lambda"]
        total = total + d["eikonal_term"]
    return total, d


def run_formulas(gold_like, lam, flags, dtype, upstream=1.0):
    pred = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in gold_like[0].items()}
    gt = {k: v.to(dtype) for k, v in gold_like[1].items()}
    total, d = formulas(pred, gt, lam, flags)
    grads = torch.autograd.grad(total * upstream, [pred[k] for k in PRED_KEYS], allow_unused=True)
    return total.detach(), {k: v.detach() for k, v in d.items()}, dict(zip(PRED_KEYS, grads))


def run_hip(gold_like, lam, flags, upstream=1.0):
    pred = {k: v.detach().requires_grad_(True) for k, v in gold_like[0].items()}           # (no copy: a copy would move the data pointer)
    lc = losses.LossClass(DEV, opt_of(**lam), lpips=object(), id_loss=object())
    total, d = lc.calc_shape_rec_loss(pred, gold_like[1], DEV, **flags)
    grads = torch.autograd.grad(total * upstream, [pred[k] for k in PRED_KEYS], allow_unused=True)
    torch.cuda.synchronize()
    return total.detach(), d, dict(zip(PRED_KEYS, grads))


def compare_with_formulas(name, inputs, lam, flags, upstream=1.0):
    """The HIP result against float64 autograd of the formulas, under the module's bound; returns the HIP and float64 results."""
    hip = run_hip(inputs, lam, flags, upstream)
    t64, t32 = run_formulas(inputs, lam, flags, torch.float64, upstream), run_formulas(inputs, lam, flags, torch.float32, upstream)
    check(name + "_total", hip[0], t64[0], t32[0])
    for k in losses.SHAPE_TERMS:
        if k in t64[1]:
            check(name + "_" + k, hip[1][k], t64[1][k], t32[1][k])
        else:
            assert float(hip[1][k]) == 0.0 and hip[1][k].shape == ()
    for k in PRED_KEYS:
        if t64[2][k] is None:
            assert hip[2][k] is None, k
        else:
            assert hip[2][k].shape == inputs[0][k].shape
            check(name + "_grad_" + k, hip[2][k], t64[2][k], t32[2][k])
    return hip, t64


@functools.lru_cache(maxsize=None)
def golden_on_device():
    gold = load_golden("losses_shape")
    pred, gt = shape_inputs(gold, DEV)
    return gold, ({k: v.detach() for k, v in pred.items()}, gt)


@pytest.mark.gpu
def test_shape_terms_match_the_golden_and_float64_autograd():
    gold, inputs = golden_on_device()
    hip, t64 = compare_with_formulas("shape_golden", inputs, LAMBDAS_A, ALL_ON)
    # against the recorded reference values: the module's bound plus the recording's own distance from float64
    for name, got, key, truth in [("total", hip[0], "a_loss", t64[0])] + [(k, hip[1][k], "a_term_" + k, t64[1][k]) for k in losses.SHAPE_TERMS] + \
                                 [("grad_" + k, hip[2][k], "a_grad_" + k, t64[2][k]) for k in PRED_KEYS]:
        rec = torch.from_numpy(np.asarray(gold[key]))
        own = maxerr(rec, truth)
        bound = max(1e-6 * float(truth.abs().max()), 3 * own) + own
        err = maxerr(got, rec)
        record("losses_shape_vs_recorded", what=name, err=err, recorded_vs_f64=own, bound=bound)
        assert err <= bound, (name, err, own, bound)
    e = inputs[0]["eikonal_term"].reshape(-1, 3)
    rows = (~e.bool().any(dim=1)).nonzero().reshape(-1)
    assert rows.numel() == 2 and not hip[2]["eikonal_term"].reshape(-1, 3)[rows].bool().any()       # exactly 0 at the zero vectors
    again = run_hip(inputs, LAMBDAS_A, ALL_ON)
    assert torch.equal(again[0], hip[0])
    for k in losses.SHAPE_TERMS:
        assert torch.equal(again[1][k], hip[1][k]), k
    for k in PRED_KEYS:
        assert torch.equal(again[2][k], hip[2][k]), k


@pytest.mark.gpu
def test_shape_terms_honour_the_upstream_gradient():
    _, inputs = golden_on_device()
    compare_with_formulas("shape_upstream", inputs, LAMBDAS_A, ALL_ON, upstream=0.37)


@pytest.mark.gpu
def test_shape_terms_at_sizes_off_the_block_and_vector_width():
    """4,099 points: three workgroups for the first segment, the last one 3 elements; 1,366 + 1 eikonal vectors; every segment's last
    group of four is partial."""
    g = torch.Generator().manual_seed(77)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    pred = dict(uniform_points_sdf=1.5 * r(1, 4099, 1), surface_sdf=r(1, 7, 9, 1), surface_eikonal_term=r(1, 7, 9, 1, 3), eikonal_term=r(1, 1367, 3))
    gt = dict(uniform_points_sdf=r(1, 4099, 1), surface_eikonal_term=F.normalize(r(1, 7, 9, 1, 3), dim=-1))
    compare_with_formulas("shape_odd", (pred, gt), LAMBDAS_A, ALL_ON)
    off = {k: torch.cat([v.reshape(-1)[:1], v.reshape(-1)])[1:].reshape(v.shape) for k, v in pred.items()}      # 4 bytes off the 16-byte grid
    assert all(v.data_ptr() % 16 == 4 for v in off.values())
    compare_with_formulas("shape_unaligned", (off, gt), LAMBDAS_A, ALL_ON)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["sdf", "surface_null_gt", "normal", "eikonal"])
def test_a_single_shape_term(which):
    _, inputs = golden_on_device()
    zero = dict(uniform_pts_sdf_lambda=0.0, surf_sdf_lambda=0.0, surf_normal_lambda=0.0, eikonal_lambda=0.0)
    key = dict(sdf="uniform_pts_sdf_lambda", surface_null_gt="surf_sdf_lambda", normal="surf_normal_lambda", eikonal="eikonal_lambda")[which]
    lam = dict(zero, **{key: 0.3})
    flags = ALL_ON if which != "sdf" else dict(supervise_sdf=True)                 # one call by its flags, three by their lambdas
    hip, _ = compare_with_formulas("shape_single_" + which, inputs, lam, flags)
    assert sum(g is not None for g in hip[2].values()) == 1


# ---- the 2-D loss under grad ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lpips_gpu():
    return syn.load_synthetic_lpips(LPIPS(differentiable=True)).to(DEV)


@functools.lru_cache(maxsize=None)
def idloss_gpu():
    return syn.load_synthetic_idloss(IDLoss(differentiable=True)).to(DEV)


def loss_class(l2, vgg, idl):
    return losses.LossClass(DEV, opt_of(l2_lambda=l2, vgg_lambda=vgg, id_lambda=idl), lpips=lpips_gpu(), id_loss=idloss_gpu())


@functools.lru_cache(maxsize=None)
def pair(size):
    return make_pair((2, 3, size, size), seed=size + 1)


@functools.lru_cache(maxsize=None)
def torch_2d(size, l2, vgg, dtype):
    """(loss, d loss / d pred) of image_metrics_torch on the CPU with the LPIPS module's layers restated in `dtype`; computed once."""
    pred, gt = pair(size)
    sd = module_cpu().state_dict()
    p, g = pred.detach().clone().to(dtype).requires_grad_(True), gt.to(dtype)           # (a copy: the pair is shared)
    lp = (lambda a, b: restate(sd, a, b, dtype)['total']) if vgg != 0 else None
    loss = image_metrics_torch(p, g, l2, lp, vgg)[3]
    return loss.detach(), torch.autograd.grad(loss, p)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("size", [64, 256])
@pytest.mark.parametrize("lambdas", [(1.0, 0.0, 0.0), (1.0, 0.8, 0.0), (1.0, 0.8, 0.1)], ids=lambda v: "-".join(map(str, v)))
def test_2d_rec_loss_under_grad(size, lambdas):
    l2, vgg, idl = lambdas
    pred, gt = pair(size)
    p, g = pred.to(DEV).requires_grad_(True), gt.to(DEV)
    lc = loss_class(*lambdas)
    out = lc.calc_2d_rec_loss(p, g, g, None)
    assert len(out) == 6 and out[4] == 0 and out[5] == 0
    loss, rec, lp, lid = out[:4]
    info = dict(size=size, lambdas=list(lambdas))
    if idl == 0:
        assert float(lid) == 0.0 and not lid.requires_grad
        grad, = torch.autograd.grad(loss, p)
        torch.cuda.synchronize()
        t64, t32 = torch_2d(size, l2, vgg, torch.float64), torch_2d(size, l2, vgg, torch.float32)
        check("2d_loss", loss, t64[0], t32[0], **info)
        check("2d_grad", grad, t64[1], t32[1], **info)
        return
    # the identity term on: the MSE and LPIPS contributions against float64, and the total as the sum of the three nodes' gradients
    parts = [torch.autograd.grad(t, p, retain_graph=True)[0] for t in (rec * l2, lp * vgg, lid * idl)]
    grad, = torch.autograd.grad(loss, p)
    torch.cuda.synchronize()
    for name, got, lam in (("mse", parts[0], (l2, 0.0)), ("lpips", parts[1], (0.0, vgg))):
        t64, t32 = torch_2d(size, *lam, torch.float64), torch_2d(size, *lam, torch.float32)
        check("2d_grad_" + name, got, t64[1], t32[1], **info)
    want = parts[0].double() + parts[1].double() + parts[2].double()
    slack = 2 * 2.0 ** -23 * (parts[0].double().abs() + parts[1].double().abs() + parts[2].double().abs())      # two float32 additions, any order
    worst = float(((grad.double() - want).abs() - slack).max())
    record("losses_2d_sum_of_nodes", worst_over_slack=worst, **info)
    assert worst <= 0.0
    assert float(parts[2].abs().max()) > 0


@pytest.mark.gpu
def test_columns_under_grad_equal_the_evaluation_bit_for_bit():
    pred, gt = pair(64)
    p, g = pred.to(DEV), gt.to(DEV)
    lc = loss_class(1.0, 0.8, 0.1)
    with torch.no_grad():
        loss0, d0 = lc(p, g, g, None, loss_dict=True)
    loss1, d1 = lc(p.clone().requires_grad_(True), g, g, None, loss_dict=True)
    torch.cuda.synchronize()
    assert list(d1) == list(d0) == ['loss_l2', 'loss_id', 'loss_lpips', 'loss', 'mae', 'PSNR', 'SSIM', 'ID_SIM']
    assert loss1.requires_grad and not loss0.requires_grad and torch.equal(loss1.detach(), loss0)
    for k in d0:
        assert torch.equal(d1[k].detach(), d0[k]), (k, float(d1[k]), float(d0[k]))
    for k in ('mae', 'PSNR', 'SSIM', 'ID_SIM'):
        assert not d1[k].requires_grad


@pytest.mark.gpu
def test_2d_rec_loss_under_grad_launches_the_squared_error_backward(monkeypatch):
    names = []
    real = _lib.launch

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "launch", spy)
    pred, gt = pair(64)
    p, g = pred.to(DEV).requires_grad_(True), gt.to(DEV)
    loss = loss_class(1.0, 0.0, 0.0).calc_2d_rec_loss(p, g, g, None)[0]
    assert "e3dge_image_metrics" in names and "e3dge_sqerr_bwd" not in names
    loss.backward()
    torch.cuda.synchronize()
    assert names.count("e3dge_sqerr_bwd") == 1 and "e3dge_lpips_backward" not in names
    assert p.grad is not None and p.grad.shape == p.shape


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pool_then_2d_rec_loss_end_to_end():
    _, gt = pair(256)
    gt = gt[:1]
    g = torch.Generator().manual_seed(9)
    image = torch.tanh(F.interpolate(gt, scale_factor=4, mode="bilinear", align_corners=False) + 0.3 * torch.randn(1, 3, 1024, 1024, generator=g))
    sd = module_cpu().state_dict()

    def chain(dtype):
        x = image.to(dtype).requires_grad_(True)
        lp = lambda a, b: restate(sd, a, b, dtype)['total']
        loss = image_metrics_torch(F.adaptive_avg_pool2d(x, (256, 256)), gt.to(dtype), 1.0, lp, 0.8)[3]
        return loss.detach(), torch.autograd.grad(loss, x)[0]
    x = image.to(DEV).requires_grad_(True)
    loss = loss_class(1.0, 0.8, 0.0).calc_2d_rec_loss(losses.AvgPool2d((256, 256))(x), gt.to(DEV), None, None)[0]
    loss.backward()
    torch.cuda.synchronize()
    t64, t32 = chain(torch.float64), chain(torch.float32)
    check("e2e_loss", loss, t64[0], t32[0])
    check("e2e_grad_image", x.grad, t64[1], t32[1])
