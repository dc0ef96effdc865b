"""GPU: the two pieces the loss stack shares since ABI 17.

  * LPIPS's packed weight images, written by conv_igemm.h's packers (ig_pack / ig_pack_t / ig_copy) and one small kernel for conv 1's
    transposed block, against a numpy restatement of the layouts documented in csrc/conv_igemm.h and csrc/lpips_bwd.h: bit for bit
    (a packer only moves values; `* 1.0f` is exact).  Pack launches only.
  * The one metric-row entry (e3dge_image_metric_row) with its four pointer combinations against a numpy float32 restatement in the
    kernel's operation order.  Every operation of columns 0-4, 6 and 7 is a single correctly rounded fp32 add, multiply or divide, so
    those are equal; column 5 goes through log10f and keeps the 2e-5 relative bound of tests/test_gpu_metrics.py."""
import numpy as np
import pytest
import torch

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, synthetic as syn
from e3dge_amd.lpips import LPIPS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32


def fragment_image(a):
    """conv_igemm.h: image[(mt * KS4 + ks) * 64 + lane] = A[mt * 16 + (lane & 15)][ks * 4 + (lane >> 4)], K padded with zeros to 32."""
    m, k = a.shape
    assert m % 16 == 0
    kpad = (k + 31) // 32 * 32
    ap = np.zeros((m, kpad), f32)
    ap[:, :k] = a
    return ap.reshape(m // 16, 16, kpad // 4, 4).transpose(0, 2, 3, 1).reshape(-1)       # [mt][ks][lane >> 4][lane & 15]


def test_lpips_weight_images_are_the_documented_layouts():
    m = syn.load_synthetic_lpips(LPIPS()).to(DEV)
    src = [t.detach().cpu().numpy() for t in m._sources()]
    w, b, lin = src[:5], src[5:10], src[10:]
    want = np.concatenate([fragment_image(x.reshape(x.shape[0], -1)) for x in w] + [x.reshape(-1) for x in b] + [x.reshape(-1) for x in lin])
    got = m._packed(torch.device(DEV))
    assert got.numel() == want.size == _lib.load().e3dge_lpips_packed_floats()
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    # lpips_bwd.h: Wt_l[ci][(co, r, s)] = W_l[co][ci][ks - 1 - r][ks - 1 - s] for conv 2..5, then conv 1 as [c][co][11 x 11]
    want_t = np.concatenate([fragment_image(x[:, :, ::-1, ::-1].transpose(1, 0, 2, 3).reshape(x.shape[1], -1)) for x in w[1:]] +
                            [w[0].transpose(1, 0, 2, 3).reshape(-1)])
    got_t = m._packed_t(torch.device(DEV))
    assert got_t.numel() == want_t.size == _lib.load().e3dge_lpips_packed_t_floats()
    assert torch.equal(got_t.cpu(), torch.from_numpy(want_t))


SUMS = np.array([[3.25, 17.5, 0.8125, 48.0], [0.4375, 5.75, 1.3125, 48.0], [11.0625, 40.125, 2.6875, 48.0]], f32)   # (sse, sae, ssim loss, count)
LPIPS_PER_IMAGE = np.array([0.3171, 0.0442, 0.7509], f32)
ID_LOSS = np.array([0.2683], f32)
L2, VGG, ID = 0.7, 0.8, 0.1


def restate_row(sums, lp, idl, l2, vgg, idw):
    t = np.zeros(4, f32)
    tl = f32(0)
    for bi in range(sums.shape[0]):
        t = t + sums[bi]                                            # four independent fp32 chains in ascending b
        if lp is not None:
            tl = f32(tl + lp[bi])
    mse, mae, ssim_loss = f32(t[0] / t[3]), f32(t[1] / t[3]), f32(t[2] / t[3])
    lpips = f32(tl / f32(sums.shape[0])) if lp is not None else f32(0)
    loss_id = idl[0] if idl is not None else f32(0)
    loss = f32(mse * f32(l2))
    if lp is not None:
        loss = f32(loss + f32(lpips * f32(vgg)))
    if idl is not None:
        loss = f32(loss + f32(loss_id * f32(idw)))
    psnr = f32(10) * np.log10(f32(1) / f32(mse * f32(0.25)), dtype=f32)
    return np.array([mse, loss_id, lpips, loss, mae, psnr, f32(1) - ssim_loss, f32(1) - loss_id], f32)


@pytest.mark.parametrize("with_lpips,with_id", [(False, False), (True, False), (False, True), (True, True)])
def test_metric_row_entry_equals_the_float32_restatement(with_lpips, with_id):
    sums = torch.from_numpy(SUMS).to(DEV)
    lp = torch.from_numpy(LPIPS_PER_IMAGE).to(DEV) if with_lpips else None
    idl = torch.from_numpy(ID_LOSS).to(DEV) if with_id else None
    row = torch.full((8,), float("nan"), device=DEV)
    _lib.launch("e3dge_image_metric_row", row, sums, lp, idl, SUMS.shape[0], L2, VGG, ID)
    got = row.cpu().numpy()
    want = restate_row(SUMS, LPIPS_PER_IMAGE if with_lpips else None, ID_LOSS if with_id else None, L2, VGG, ID)
    print("metric row", with_lpips, with_id, got.tolist(), want.tolist())
    exact = [0, 1, 2, 3, 4, 6, 7]
    assert np.array_equal(got[exact], want[exact]), (got, want)
    assert abs(got[5] - want[5]) <= 2e-5 * abs(want[5]), (got[5], want[5])
    if not with_lpips:
        assert got[2] == 0.0
    if not with_id:
        assert got[1] == 0.0 and got[7] == 1.0
