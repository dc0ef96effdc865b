"""GPU: the fused per-image metrics kernel (e3dge_image_metrics) against the plain-torch formulation of the same columns
(sharded_eval.image_metrics_torch: MSE / L1 / PSNR / SSIM as losses/builder.py:130-184 defines them).  Tolerance: the sums
run over up to 3M elements in a different association order: 2e-5 relative per column.

The per-tile tests look below the batch means, where a few wrong pixels at a tile seam or a reflected border do not average out: every
row of the scratch buffer (one 32 x 32 tile of one plane: squared-error, absolute-error and SSIM-loss sums) against the float64
per-pixel reference of tests/test_fir_host.py (metrics_pixels_ref) summed over the same tile.  Bound: the project's standing one
(parity_bound of tests/test_encoder_host.py) per column over all tiles, f32 the same reference in float32 on the CPU; the per-image
sums with the bound times sqrt(rows)."""
import math

import numpy as np
import pytest
import torch

from conftest import record

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, sharded_eval as se

from test_encoder_host import parity_bound
from test_fir_host import EQUAL_TILE, METRIC_SHAPES, metrics_inputs, metrics_pixels_ref, metrics_tile_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("shape", [(1, 3, 1024, 1024), (2, 3, 50, 70), (1, 1, 5, 33), (1, 3, 256, 256)])
def test_image_metrics_kernel_vs_torch(shape):
    g = torch.Generator(device=DEV).manual_seed(shape[2])
    gt = torch.tanh(torch.randn(shape, device=DEV, generator=g))
    pred = torch.tanh(gt * 1.2 + 0.1 * torch.randn(shape, device=DEV, generator=g))
    a = se.image_metrics(pred, gt)
    b = se.image_metrics_torch(pred, gt)
    rel = float(((a - b).abs() / b.abs().clamp_min(1e-6)).max())
    record(f"image_metrics_{shape[2]}x{shape[3]}", max_rel_diff=rel, ssim=float(a[6]), psnr=float(a[5]))
    assert a.shape == (8,) and rel <= 2e-5, (a, b)
    same = se.image_metrics(gt, gt.clone())
    assert float(same[0]) == 0.0 and abs(float(same[6]) - 1) < 1e-6
    assert torch.equal(se.image_metrics(pred, gt), a)               # fixed-order fold: bit-reproducible
    half = se.image_metrics(pred, gt, l2_lambda=0.5)                # the row kernel (e3dge_image_metric_row) applies the weight
    assert float(half[3]) == 0.5 * float(a[0]) and torch.equal(half[[0, 4, 5, 6]], a[[0, 4, 5, 6]])
    assert float(a[1]) == 0.0 and float(a[2]) == 0.0 and float(a[7]) == 1.0


@pytest.mark.parametrize("shape", METRIC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_image_metrics_tile_rows_and_sums_against_float64(shape, lib):
    """e3dge_image_metrics through _lib.launch with a NaN-prefilled scratch of exactly e3dge_image_metrics_scratch_floats floats plus
    slack: every tile row and the per-image sums against float64; the slack stays NaN, the count is exact, and the tile on which
    pred == gt bit for bit (with the two pixels around it that its windows reach) sums to exactly 0 in all three columns."""
    B, C, H, W = shape
    pred, gt = metrics_inputs(shape)
    ty, tx = math.ceil(H / 32), math.ceil(W / 32)
    rows = B * C * ty * tx
    n = lib.e3dge_image_metrics_scratch_floats(B, C, H, W)
    assert n == rows * 3
    slack = 32
    scratch = torch.full((n + slack,), float("nan"), device=DEV)
    sums = torch.full((B * 4 + slack,), float("nan"), device=DEV)
    _lib.launch("e3dge_image_metrics", sums, scratch, pred.to(DEV), gt.to(DEV), B, C, H, W, 1.0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(scratch[n:]).all()) and bool(torch.isnan(sums[B * 4:]).all())
    got = scratch[:n].cpu().reshape(rows, 3)
    got_sums = sums[:B * 4].cpu().reshape(B, 4)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(got_sums).all())
    t64 = metrics_tile_rows(metrics_pixels_ref(pred.double(), gt.double()))
    t32 = metrics_tile_rows(metrics_pixels_ref(pred, gt))
    name = "image_metrics_tiles_" + "x".join(map(str, shape))
    checks = []
    for j, col in enumerate(("sq_err", "abs_err", "ssim_loss")):
        err = float((got[:, j].double() - t64[:, j]).abs().max())
        f32 = float((t32[:, j].double() - t64[:, j]).abs().max())
        bound = parity_bound(t64[:, j], t32[:, j])
        s64, s32 = t64[:, j].reshape(B, -1).sum(1), t32[:, j].reshape(B, -1).sum(1)
        s_err = float((got_sums[:, j].double() - s64).abs().max())
        s_bound = parity_bound(s64, s32) * math.sqrt(rows // B)
        record(f"{name}_{col}", err=err, f32=f32, bound=bound, rows=rows, worst_row=int((got[:, j].double() - t64[:, j]).abs().argmax()),
               sum_err=s_err, sum_f32=float((s32.double() - s64).abs().max()), sum_bound=s_bound)
        checks.append((col, err, bound, s_err, s_bound))
    zero_ok = None
    if shape in EQUAL_TILE:
        p, r, c = EQUAL_TILE[shape]
        row = got[(p * ty + r) * tx + c]
        zero_ok = bool((row == 0).all())
        record(name + "_equal_tile", sums_are_zero=zero_ok, row=row.tolist())
    assert got_sums[:, 3].tolist() == [float(C * H * W)] * B
    for col, err, bound, s_err, s_bound in checks:
        assert err <= bound, (shape, col, err, bound)
        assert s_err <= s_bound, (shape, col, "sum", s_err, s_bound)
    assert zero_ok in (None, True)
