"""CPU: the training-loss additions of the C-ABI (csrc/losses.hip) -- the source list, argument validation -- and the
torch branches of e3dge_amd.losses against tests/golden/losses_shape.npz (tools/gen_golden_losses.py recorded it from the reference's
LossClass.calc_shape_rec_loss, gan_loss.eikonal_loss and AdaptiveAvgPool2d)."""
import ctypes
import types

import numpy as np
import pytest
import torch

from conftest import load_golden

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, losses

LAMBDAS_A = dict(uniform_pts_sdf_lambda=1.0, surf_sdf_lambda=0.1, surf_normal_lambda=0.05, eikonal_lambda=0.1)
LAMBDAS_B = dict(LAMBDAS_A, surf_sdf_lambda=0.0)
ALL_ON = dict(supervise_sdf=True, supervise_surface=True, supervise_surface_normal=True, supervise_eikonal=True)
PRED_KEYS = ("uniform_points_sdf", "surface_sdf", "surface_eikonal_term", "eikonal_term")


def shape_inputs(gold, device="cpu", dtype=torch.float32):
    """(pred dict of leaves, gt dict) from the fixture."""
    pred = {k: torch.from_numpy(gold["in_pred_" + k]).to(device=device, dtype=dtype).requires_grad_(True) for k in PRED_KEYS}
    gt = {k: torch.from_numpy(gold["in_gt_" + k]).to(device=device, dtype=dtype) for k in ("uniform_points_sdf", "surface_eikonal_term")}
    return pred, gt


def opt_of(**kw):
    base = dict(l2_lambda=1.0, vgg_lambda=0.0, id_lambda=0.0, **LAMBDAS_A)
    base.update(kw)
    return types.SimpleNamespace(**base)


def stub_loss_class(opt, calls=None):
    """A LossClass whose perceptual and identity criteria are plain callables (no network is built)."""
    def lp(x, y):
        return ((x - y) ** 2).mean() * 0.5

    def idl(y_hat, y, x):
        if calls is not None:
            calls.append("id")
        return (1 - (y_hat * y).mean()), 0.0, []
    return losses.LossClass("cpu", opt, lpips=lp, id_loss=idl)


def test_losses_source_is_part_of_the_build():
    from e3dge_amd import build
    assert "losses.hip" in build.SOURCES


def _fails(lib, rc, *words):
    assert rc == -1
    msg = lib.e3dge_last_error().decode()
    for w in words:
        assert w in msg, (w, msg)


def test_argument_validation_names_the_bad_field(lib):
    """Nothing is launched: every call fails (or is a no-op) before it touches the device; 64 stands for any non-null pointer."""
    P = 64
    _fails(lib, lib.e3dge_avgpool_fwd(None, P, 1, 8, 8, 2, None), "avgpool_fwd", "out")
    _fails(lib, lib.e3dge_avgpool_fwd(P, None, 1, 8, 8, 2, None), "avgpool_fwd", "in is null")
    _fails(lib, lib.e3dge_avgpool_fwd(P, P, 1, 8, 8, 3, None), "f=3")
    _fails(lib, lib.e3dge_avgpool_fwd(P, P, 1, 10, 8, 4, None), "in_h=10")
    _fails(lib, lib.e3dge_avgpool_fwd(P, P, -1, 8, 8, 2, None), "planes")
    _fails(lib, lib.e3dge_avgpool_bwd(None, P, 1, 8, 8, 2, None), "avgpool_bwd", "d_in")
    _fails(lib, lib.e3dge_avgpool_bwd(P, None, 1, 8, 8, 2, None), "avgpool_bwd", "d_out")
    assert lib.e3dge_avgpool_fwd(None, None, 0, 8, 8, 2, None) == 0 and lib.e3dge_avgpool_bwd(None, None, 0, 8, 8, 2, None) == 0
    _fails(lib, lib.e3dge_sqerr_bwd(P, P, P, -5, P, None), "sqerr_bwd", "n=-5")
    for i, field in enumerate(("d_pred", "pred", "gt")):
        ptrs = [P, P, P]
        ptrs[i] = None
        _fails(lib, lib.e3dge_sqerr_bwd(*ptrs, 16, P, None), "sqerr_bwd", field + " is null")
    _fails(lib, lib.e3dge_sqerr_bwd(P, P, P, 16, None, None), "scale_ptr")
    assert lib.e3dge_sqerr_bwd(None, None, None, 0, None, None) == 0
    _fails(lib, lib.e3dge_shape_loss_fwd(None, None), "shape_loss_fwd", "args")
    a = _lib.ShapeLossArgs()
    assert lib.e3dge_shape_loss_fwd(a, None) == 0 and lib.e3dge_shape_loss_bwd(a, None) == 0      # every segment off
    assert lib.e3dge_shape_loss_partial_floats(a) == 0
    a.seg[2].n = -3
    _fails(lib, lib.e3dge_shape_loss_fwd(a, None), "seg[2].n=-3")
    _fails(lib, lib.e3dge_shape_loss_bwd(a, None), "shape_loss_bwd", "seg[2].n=-3")
    a.seg[2].n = 5000
    assert lib.e3dge_shape_loss_partial_floats(a) == 3                                             # 2048 items per workgroup
    _fails(lib, lib.e3dge_shape_loss_fwd(a, None), "seg[2].pred is null")
    a.seg[2].pred, a.seg[2].kind = P, 7
    _fails(lib, lib.e3dge_shape_loss_fwd(a, None), "seg[2].kind=7")
    a.seg[2].kind, a.seg[2].gt = _lib.SHAPE_EIKONAL, P
    _fails(lib, lib.e3dge_shape_loss_fwd(a, None), "seg[2].gt")
    a.seg[2].gt = None
    _fails(lib, lib.e3dge_shape_loss_fwd(a, None), "terms is null")
    a.terms = P
    _fails(lib, lib.e3dge_shape_loss_fwd(a, None), "total is null")
    a.total = P
    _fails(lib, lib.e3dge_shape_loss_fwd(a, None), "partial is null")
    a.partial, a.partial_floats = P, 2
    _fails(lib, lib.e3dge_shape_loss_fwd(a, None), "partial_floats=2")
    _fails(lib, lib.e3dge_shape_loss_bwd(a, None), "seg[2].d_pred is null")
    a.seg[2].d_pred = P
    _fails(lib, lib.e3dge_shape_loss_bwd(a, None), "upstream is null")


@pytest.mark.parametrize("tag,lambdas,flags", [("a_", LAMBDAS_A, ALL_ON), ("b_", LAMBDAS_B, dict(ALL_ON, supervise_eikonal=False))])
def test_cpu_shape_terms_equal_the_reference_bit_for_bit(tag, lambdas, flags):
    gold = load_golden("losses_shape")
    pred, gt = shape_inputs(gold)
    lc = stub_loss_class(opt_of(**lambdas))
    loss, d = lc.calc_shape_rec_loss(pred, gt, "cpu", **flags)
    assert set(d) == {"surf_rec_loss", "sdf_rec_loss", "surface_norm_rec_loss", "eikonal_term"}
    assert np.array_equal(loss.detach().numpy(), gold[tag + "loss"])
    for t in losses.SHAPE_TERMS:
        assert np.array_equal(d[t].detach().numpy(), gold[tag + "term_" + t]), t
    grads = torch.autograd.grad(loss, [pred[k] for k in PRED_KEYS], allow_unused=True)
    for k, g in zip(PRED_KEYS, grads):
        if tag + "grad_" + k in gold.files:
            assert np.array_equal(g.numpy(), gold[tag + "grad_" + k]), k
        else:
            assert g is None, k
    if tag == "b_":                                                   # the skipped terms keep the reference's zero defaults
        assert float(d["surf_rec_loss"]) == 0.0 and float(d["eikonal_term"]) == 0.0
        assert d["surf_rec_loss"].shape == () and gold["b_term_surf_rec_loss"].shape == ()
    else:
        zero = gold["in_pred_eikonal_term"].reshape(-1, 3)
        rows = np.where(~zero.any(axis=1))[0]
        assert len(rows) == 2 and not grads[3].numpy().reshape(-1, 3)[rows].any()      # torch's sub-gradient at the zero vector


def test_calc_shape_rec_loss_asserts_like_the_reference():
    gold = load_golden("losses_shape")
    pred, gt = shape_inputs(gold)
    lc = stub_loss_class(opt_of())
    with pytest.raises(AssertionError, match="at least supervise"):
        lc.calc_shape_rec_loss(pred, gt, "cpu", supervise_sdf=False, supervise_surface_normal=False)


def test_cpu_eikonal_loss_and_pool_equal_the_recorded_values():
    gold = load_golden("losses_shape")
    e = torch.from_numpy(gold["in_pred_eikonal_term"])
    a, b = losses.eikonal_loss(e)
    assert np.array_equal(a.numpy(), gold["eik_loss"]) and np.array_equal(b.numpy(), gold["eik_surface_none"])
    a, b = losses.eikonal_loss(e, torch.from_numpy(gold["in_pred_uniform_points_sdf"]) * 0.01)
    assert np.array_equal(a.numpy(), gold["eik_loss_sdf"]) and np.array_equal(b.numpy(), gold["eik_surface"])
    pool = losses.AvgPool2d((8, 8))
    assert pool.factor(torch.from_numpy(gold["pool_in_32"])) is None              # CPU tensors take torch
    assert np.array_equal(pool(torch.from_numpy(gold["pool_in_32"])).numpy(), gold["pool_out_32"])
    assert np.array_equal(pool(torch.from_numpy(gold["pool_in_20"])).numpy(), gold["pool_out_20"])     # 20 -> 8: not an integer ratio
    assert losses.AvgPool2d(8).output_size == (8, 8)


def test_loss_class_surface_and_2d_return_values_on_cpu():
    calls = []
    lc = stub_loss_class(opt_of(vgg_lambda=0.8, id_lambda=0.0), calls)
    for name in ("criterionImg", "criterionLPIPS", "criterionID", "criterion3d_rec", "id_loss_pool", "uniform_pts_loss"):
        assert hasattr(lc, name), name
    assert isinstance(lc.id_loss_pool, losses.AvgPool2d) and lc.id_loss_pool.output_size == (256, 256)
    g = torch.Generator().manual_seed(3)
    pred = (torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).requires_grad_(True)
    gt = torch.rand(2, 3, 32, 32, generator=g) * 2 - 1
    out = lc.calc_2d_rec_loss(pred, gt, gt, None)
    assert len(out) == 6 and out[4] == 0 and out[5] == 0
    loss, l2, lp, lid = out[:4]
    mse = ((pred - gt) ** 2).mean()
    assert torch.equal(l2, mse) and torch.equal(lp, mse * 0.5) and torch.equal(loss, mse * 1.0 + (mse * 0.5) * 0.8)
    assert float(lid.detach()) == 0.0 and lid.shape == () and calls == []            # id_lambda = 0: a zero tensor, the module is not called
    loss2, d = lc(pred, gt, gt, None, loss_dict=True)
    assert list(d) == ['loss_l2', 'loss_id', 'loss_lpips', 'loss', 'mae', 'PSNR', 'SSIM', 'ID_SIM']
    assert torch.equal(loss2, loss) and torch.equal(d['loss'], loss) and float(d['ID_SIM'].detach()) == 1.0
    assert torch.equal(d['mae'], (pred - gt).abs().mean())
    gp, = torch.autograd.grad(loss2, pred)
    assert torch.allclose(gp, (1.0 + 0.4) * 2 * (pred - gt).detach() / pred.numel(), rtol=1e-5, atol=1e-9)
    lc_id = stub_loss_class(opt_of(id_lambda=0.1), calls)
    loss3, d3 = lc_id(pred, gt, gt, None, loss_dict=True)
    assert calls == ["id"] and torch.equal(d3['ID_SIM'], 1 - d3['loss_id'])
    assert torch.equal(loss3, (mse * 1.0 + (mse * 0.5) * 0.0) + d3['loss_id'] * 0.1)


def test_no_gpu_means_no_hip_branch():
    x = torch.randn(1, 3, 16, 16)
    assert losses.AvgPool2d((4, 4)).factor(x) is None and not losses._is_hip(x)
    assert torch.equal(losses.AvgPool2d((4, 4))(x), torch.nn.functional.adaptive_avg_pool2d(x, (4, 4)))
