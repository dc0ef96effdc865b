"""Fixture for the training loss (tests/test_losses_host.py, tests/test_gpu_losses.py).  Authoring time only, CPU only; the tests never
run this.

    python tools/gen_golden_losses.py

Calls the reference's LossClass.calc_shape_rec_loss (project/losses/builder.py:43-117) UNBOUND with a stand-in `self` that carries `opt`
and `criterion3d_rec = SmoothL1Loss()` -- LossClass.__init__ reads weight files -- and gan_loss.eikonal_loss (project/losses/gan_loss.py),
and writes tests/golden/losses_shape.npz:
    in_*                 the inputs: uniform_points_sdf (2,257,1) as 1.5 randn against randn (both Smooth-L1 branches), surface_sdf
                         (2,8,8,1), surface_eikonal_term (2,8,8,1,3) with its target, eikonal_term (2,8,8,18,3) with two vectors exactly 0
    a_*                  lambdas 1.0 / 0.1 / 0.05 / 0.1, every flag on: loss, the four dictionary entries, autograd's gradients to the four
                         predictions
    b_*                  surf_sdf_lambda = 0 and supervise_eikonal=False: the same, with the skipped terms at their zero defaults
    eik_*                eikonal_loss(eikonal_term) and eikonal_loss(eikonal_term, sdf): both values of the pair
    pool_*               AdaptiveAvgPool2d, the reference's id_loss_pool / pool_256 operator (builder.py:27): 32^2 -> 8^2 and 20^2 -> 8^2"""
import importlib
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLD = os.path.join(REPO, "tests", "golden")

import oracle.cpu_numerics  # noqa: E402,F401  (before any arithmetic)

LAMBDAS_A = dict(uniform_pts_sdf_lambda=1.0, surf_sdf_lambda=0.1, surf_normal_lambda=0.05, eikonal_lambda=0.1)
LAMBDAS_B = dict(LAMBDAS_A, surf_sdf_lambda=0.0)
PRED_KEYS = ("uniform_points_sdf", "surface_sdf", "surface_eikonal_term", "eikonal_term")
TERMS = ("sdf_rec_loss", "surf_rec_loss", "surface_norm_rec_loss", "eikonal_term")


def inputs():
    g = torch.Generator().manual_seed(20231)
    r = lambda *s: torch.randn(*s, generator=g)
    pred = dict(uniform_points_sdf=1.5 * r(2, 257, 1), surface_sdf=0.7 * r(2, 8, 8, 1), surface_eikonal_term=r(2, 8, 8, 1, 3),
                eikonal_term=r(2, 8, 8, 18, 3))
    pred["eikonal_term"][0, 1, 2, 3] = 0.0
    pred["eikonal_term"][1, 7, 0, 17] = 0.0
    gt = dict(uniform_points_sdf=r(2, 257, 1), surface_eikonal_term=torch.nn.functional.normalize(r(2, 8, 8, 1, 3), dim=-1))
    return pred, gt


def record(ref_cls, lambdas, pred, gt, **flags):
    me = types.SimpleNamespace(opt=types.SimpleNamespace(**lambdas), criterion3d_rec=torch.nn.SmoothL1Loss())
    leaves = {k: v.clone().requires_grad_(True) for k, v in pred.items()}
    loss, d = ref_cls.calc_shape_rec_loss(me, leaves, gt, 'cpu', **flags)
    used = PRED_KEYS
    grads = torch.autograd.grad(loss, [leaves[k] for k in used], allow_unused=True)
    out = {"loss": loss.detach().numpy()}
    for t in TERMS:
        out["term_" + t] = d[t].detach().numpy()
    for k, gr in zip(used, grads):
        if gr is not None:
            out["grad_" + k] = gr.numpy()
    return out


def main():
    from oracle import ref_harness, golden_store
    ref_harness.prepare()
    builder = importlib.import_module("project.losses.builder")
    gan_loss = importlib.import_module("project.losses.gan_loss")
    pred, gt = inputs()
    arrays = {"in_pred_" + k: v.numpy() for k, v in pred.items()}
    arrays.update({"in_gt_" + k: v.numpy() for k, v in gt.items()})
    everything = dict(supervise_sdf=True, supervise_surface=True, supervise_surface_normal=True, supervise_eikonal=True)
    for tag, lambdas, flags in (("a_", LAMBDAS_A, everything), ("b_", LAMBDAS_B, dict(everything, supervise_eikonal=False))):
        for k, v in record(builder.LossClass, lambdas, pred, gt, **flags).items():
            arrays[tag + k] = v
    frac = float((pred["uniform_points_sdf"] - gt["uniform_points_sdf"]).abs().gt(1).float().mean())
    e0, m0 = gan_loss.eikonal_loss(pred["eikonal_term"])
    e1, m1 = gan_loss.eikonal_loss(pred["eikonal_term"], pred["uniform_points_sdf"] * 0.01)
    arrays.update(eik_loss=e0.numpy(), eik_surface_none=m0.numpy(), eik_loss_sdf=e1.numpy(), eik_surface=m1.numpy())
    g = torch.Generator().manual_seed(20232)
    x32, x20 = torch.randn(2, 3, 32, 32, generator=g), torch.randn(1, 3, 20, 20, generator=g)
    pool = torch.nn.AdaptiveAvgPool2d((8, 8))
    arrays.update(pool_in_32=x32.numpy(), pool_out_32=pool(x32).numpy(), pool_in_20=x20.numpy(), pool_out_20=pool(x20).numpy())
    path = golden_store.save(GOLD, "losses_shape", arrays)
    print(dict(path=path, bytes=os.path.getsize(path), large_residual_fraction=round(frac, 3), torch=torch.__version__))


if __name__ == "__main__":
    main()
