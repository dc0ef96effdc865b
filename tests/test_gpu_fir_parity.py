"""GPU: the FIR kernels with ASYMMETRIC taps and tile seams against float64 (tests/test_fir_host.py has the FIR, the geometries and the
CPU proof that a dropped flip, a transposed tap index, swapped pads or a one-pixel shift moves the truth by > 1000 bounds).

  e3dge_upfirdn2d / _f16 / _f64   blur44_kernel (64 x 64 tiles), upfirdn2d_tiled_kernel<2,1,4,4> and <1,2,4,4> (32 x 64 tiles) and the
                                  generic kernel: y, gx (autograd of op.upfirdn2d, random gy), ggy; the second plane alone against its
                                  values in the batch, bit for bit; NaN-prefilled output with slack; the scalar-store branch on a
                                  misaligned base pointer; the grid-stride loop of the generic kernel.
  e3dge_blur_noise_bias_act       the epilogue form of blur44_kernel: noise of batch 1 / B / none, aligned and one float off, bias,
                                  out_amax.
  e3dge_torgb                     the skip up-sampler inside torgb_kernel, the three channel-group forms.

Truth: oracle/ops_ref.upfirdn2d_ref (or plain torch) in float64 on the CPU.  Bound: parity_bound of tests/test_encoder_host.py per
tensor -- max|hip - f64| <= max(2e-6 max|f64|, 3 max|f32 - f64|), f32 the same composition in float32 on the CPU; fp16 storage:
_half_close of tests/test_gpu_selftest_and_ops.py (one fp16 ulp of the fp32 oracle on the widened inputs, rounded once); fp64: 1e-13.
Every comparison is measured, written with conftest.record (err, f32, bound; seam band and interior apart for the tiled kernels), then
asserted.

Measured on the MI355X (the `fir_parity_*` lines of the parity report), largest error and the float32 composition's own for that tensor:
blur44_kernel 2.1e-7 (3.1e-7), up by 2 8.1e-7 (6.4e-7; taps sum to 4), down by 2 1.8e-7 (1.8e-7), generic 2.9e-7 (3.0e-7), the
epilogue form 4.1e-7 (3.2e-7), torgb 7.9e-7 (2.3e-6); never above 1.5 x the float32 composition's, largest err / bound 0.09; seam band
against interior 1.9e-7 / 2.1e-7 (blur), 2.0e-7 / 2.7e-7 (up), 1.8e-7 / 1.7e-7 (down); fp16 worst 1.0 ulp; fp64 4.4e-16."""
import numpy as np
import pytest
import torch

from conftest import record
from oracle import ops_ref

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, op

from test_encoder_host import parity_bound
from test_fir_host import GENERIC, GEOMETRIES, asym_fir
from test_gpu_selftest_and_ops import _half_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLACK = 64
SUFFIX = {torch.float32: "", torch.float16: "_f16", torch.float64: "_f64"}
INT_VIEW = {torch.float32: torch.int32, torch.float16: torch.int16, torch.float64: torch.int64}


def _err(got, want):
    return float((got.detach().double().cpu() - want.double()).abs().max()) if want.numel() else 0.0


def _measure(name, got, t64, t32, mask=None, **extra):
    """One comparison: measured, recorded, returned as (err, bound) for the assertion that follows."""
    got = got.detach().double().cpu()
    assert got.shape == t64.shape, (name, tuple(got.shape), tuple(t64.shape))
    d = (got - t64).abs()
    err, f32, bound = float(d.max()), float((t32.double() - t64).abs().max()), parity_bound(t64, t32)
    split = {}
    if mask is not None:
        m = mask.expand_as(d)
        split = dict(seam=float(d[m].max()) if bool(m.any()) else None, interior=float(d[~m].max()) if bool((~m).any()) else None,
                     seam_f32=float((t32.double() - t64).abs()[m].max()) if bool(m.any()) else None)
    record(name, err=err, f32=f32, bound=bound, finite=bool(torch.isfinite(got).all()), **split, **extra)
    return err, bound


def seam_mask(c):
    """(out_h, out_w) bool: outputs within 3 of a tile boundary of the case's kernel, and the whole last partial tile of each axis."""
    (oh, ow), (th, tw) = c.out_hw, c.tile
    def axis(n, t):
        i = torch.arange(n)
        near = torch.zeros(n, dtype=torch.bool)
        for b in range(t, n, t):
            near |= (i - b).abs() <= 3
        if n % t:
            near |= i >= n - n % t
        return near
    return axis(oh, th)[:, None] | axis(ow, tw)[None, :]


def launch_guarded(x, fir, c, offset=0):
    """e3dge_upfirdn2d[_f16|_f64] through _lib.launch on planes x (B, C, H, W): the input is a contiguous view `offset` elements into a
    larger buffer, the output likewise into a NaN-prefilled one with SLACK elements after it.  Returns y (B, C, out_h, out_w) after
    asserting that no NaN is inside and that everything around the view kept its bit pattern."""
    B, C, H, W = x.shape
    dt = x.dtype
    (oh, ow), (kh, kw) = c.out_hw, c.fir.shape
    k = fir.to(DEV, torch.float64 if dt == torch.float64 else torch.float32).contiguous()
    xbuf = torch.full((offset + x.numel() + SLACK,), float("nan"), device=DEV, dtype=dt)
    xv = xbuf[offset:offset + x.numel()]
    xv.copy_(x.reshape(-1))
    n = B * C * oh * ow
    ybuf = torch.full((offset + n + SLACK,), float("nan"), device=DEV, dtype=dt)
    before = ybuf.view(INT_VIEW[dt]).clone()
    yv = ybuf[offset:offset + n]
    assert xv.data_ptr() == xbuf.data_ptr() + offset * x.element_size() and yv.data_ptr() == ybuf.data_ptr() + offset * x.element_size()
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = c.up, c.down, c.pad
    _lib.launch("e3dge_upfirdn2d" + SUFFIX[dt], yv, xv, k, B * C, H, W, kh, kw, ux, uy, dx, dy, px0, px1, py0, py1)
    torch.cuda.synchronize()
    after = ybuf.view(INT_VIEW[dt])
    assert not bool(torch.isnan(yv).any()), c
    assert torch.equal(after[:offset], before[:offset]) and torch.equal(after[offset + n:], before[offset + n:]), c
    assert bool(torch.isnan(ybuf[:offset]).all()) and bool(torch.isnan(ybuf[offset + n:]).all())
    return yv.clone().reshape(B, C, oh, ow)


def _public(c, x, k):
    return op.upfirdn2d(x, k, up=c.up[0], down=c.down[0], pad=(c.pad[0], c.pad[1]))


def _oracle_grads(c, dtype):
    """(y, gx for the case's gy, ggy for the cotangent v = the case's x scaled) of the oracle on the CPU in dtype."""
    x = c.x(dtype).requires_grad_(True)
    y = c.ref(x)
    gx, = torch.autograd.grad(y, x, c.gy(dtype))
    v = (c.x(dtype) * 0.5 + 0.25).detach()
    return y.detach(), gx, c.ref(v)


# ---- the upfirdn2d entry points ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GEOMETRIES + [g for g in GENERIC if g.square and g.grads], ids=repr)
def test_upfirdn2d_fp32_values_and_gradients(c):
    """y, gx and ggy of one geometry in fp32 against float64; the guarded launch and the public op give the same bits; plane 1 alone
    equals its values in the batch."""
    y64, gx64, ggy64 = _oracle_grads(c, torch.float64)
    y32, gx32, ggy32 = _oracle_grads(c, torch.float32)
    mask = seam_mask(c) if c.tile else None
    x = c.x(torch.float32).to(DEV)
    k = c.fir.float().to(DEV)
    checks = []
    y = launch_guarded(x, c.fir, c)
    checks.append(("y",) + _measure(f"fir_parity_{c.name}_y", y, y64, y32, mask))
    xg = x.clone().requires_grad_(True)
    yp = _public(c, xg, k)
    same_bits = torch.equal(yp.detach(), y)
    gy = c.gy(torch.float32).to(DEV).requires_grad_(True)
    gx, = torch.autograd.grad(yp, xg, gy, create_graph=True)
    checks.append(("gx",) + _measure(f"fir_parity_{c.name}_gx", gx, gx64, gx32))
    v = (c.x(torch.float32) * 0.5 + 0.25).to(DEV)
    ggy, = torch.autograd.grad(gx, gy, v)
    checks.append(("ggy",) + _measure(f"fir_parity_{c.name}_ggy", ggy, ggy64, ggy32, mask))
    alone = _public(c, x[0:1, 1:2].contiguous(), k)
    alone_bits = torch.equal(alone, y[0:1, 1:2])
    record(f"fir_parity_{c.name}_bits", guarded_equals_public=same_bits, plane_alone_equals_batch=alone_bits)
    assert same_bits and alone_bits
    for what, err, bound in checks:
        assert err <= bound, (c, what, err, bound)


@pytest.mark.parametrize("c", [g for g in GENERIC if not (g.square and g.grads)], ids=repr)
def test_upfirdn2d_generic_kernel_values(c):
    """The generic kernel where the public op does not reach (up / down / pad per axis) and in its grid-stride loop: values."""
    x64 = c.x(torch.float64)
    y64, y32 = c.ref(x64), c.ref(x64.float())
    y = launch_guarded(c.x(torch.float32).to(DEV), c.fir, c)
    major = c.planes[0] * c.planes[1]
    raw = op.upfirdn2d_raw(c.x(torch.float32).to(DEV).reshape(major, *c.in_hw, 1), c.fir.float().to(DEV), *c.up, *c.down, *c.pad)
    assert torch.equal(raw.reshape(y.shape), y)
    err, bound = _measure(f"fir_parity_{c.name}_y", y, y64, y32, outputs=y.numel())
    assert err <= bound, (c, err, bound)


@pytest.mark.parametrize("c", GEOMETRIES, ids=repr)
def test_upfirdn2d_fp16_values_and_gradient(c):
    """Half storage of the tiled kernels: y and gx within one fp16 ulp of the fp32 oracle on the widened inputs, rounded once."""
    x16, gy16 = c.x(torch.float32).half(), c.gy(torch.float32).half()
    xr = x16.float().requires_grad_(True)
    want = c.ref(xr)
    want_gx, = torch.autograd.grad(want, xr, gy16.float())
    y = launch_guarded(x16.to(DEV), c.fir, c)
    xg = x16.to(DEV).requires_grad_(True)
    yp = _public(c, xg, c.fir.float().to(DEV))
    gx, = torch.autograd.grad(yp, xg, gy16.to(DEV))
    ok_y, w_y = _half_close(y, want.detach())
    ok_gx, w_gx = _half_close(gx, want_gx)
    record(f"fir_parity_{c.name}_f16", y_ulp=w_y, gx_ulp=w_gx, bound=1.0)
    assert y.dtype == gx.dtype == torch.float16 and torch.equal(yp.detach(), y)
    assert ok_y and ok_gx, (c, w_y, w_gx)


@pytest.mark.parametrize("c", [GEOMETRIES[0], GEOMETRIES[5], GEOMETRIES[9], GENERIC[0]], ids=repr)
def test_upfirdn2d_fp64_values(c):
    """The float64 entry (one geometry per branch of the fp32 dispatch: blur, up, down, generic) to 1e-13."""
    x = c.x(torch.float64)
    y = launch_guarded(x.to(DEV), c.fir, c)
    err = _err(y, c.ref(x))
    record(f"fir_parity_{c.name}_f64", err=err, bound=1e-13)
    assert y.dtype == torch.float64 and err <= 1e-13, (c, err)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("c", [GEOMETRIES[1], GEOMETRIES[6], GEOMETRIES[10]], ids=repr)
def test_upfirdn2d_misaligned_storage_takes_the_scalar_stores(c, dtype):
    """out_w % 4 == 0 with x and y one element into their buffers (4 bytes off for fp32, 2 for fp16: vec_ok wants 16 / 8): the scalar
    stores write the bits the vector stores write, and nothing before or after the view."""
    assert c.out_hw[1] % 4 == 0
    x = c.x(torch.float32).to(dtype).to(DEV)
    aligned = launch_guarded(x, c.fir, c)
    off = launch_guarded(x, c.fir, c, offset=1)
    same = torch.equal(aligned, off)
    record(f"fir_parity_{c.name}_misaligned_{SUFFIX[dtype] or '_f32'}", bit_identical=same)
    assert same, c


# ---- e3dge_blur_noise_bias_act: blur44_kernel's epilogue form --------------------------------------------------------------------------
EPI_GEOS = [((35, 67), (34, 66)), ((67, 69), (66, 68))]
EPI_MODES = [(None, False), (1, True), (2, True), (2, False), ("1u", True), ("2u", True), ("2u", False)]


@pytest.mark.parametrize("noise, with_bias", EPI_MODES, ids=lambda v: str(v))
@pytest.mark.parametrize("in_hw, out_hw", EPI_GEOS, ids=["34x66", "66x68"])
def test_blur_noise_bias_act_with_the_asymmetric_fir(in_hw, out_hw, noise, with_bias):
    """B = 2, C = 3 (plane % C, plane / C and the plane all differ), pad (1, 1): blur + noise_weight * noise + bias -> lrelu * scale
    against float64; `u`: the noise is a view one float into its buffer (the unaligned branch of the epilogue's noise loads)."""
    B, C = 2, 3
    g = torch.Generator().manual_seed(1000 + in_hw[0])
    x = torch.randn(B, C, *in_hw, generator=g)
    k = asym_fir()
    nb = None if noise is None else int(str(noise)[0])
    unaligned = isinstance(noise, str)
    nz = None if nb is None else torch.randn(nb, 1, *out_hw, generator=g)
    nw = torch.tensor([0.37])
    bias = torch.tensor([-0.30, 0.11, -0.17]) if with_bias else None
    alpha, scale = float(np.float32(0.2)), float(np.float32(2 ** 0.5))          # they travel as float

    def compose(dt):
        v = ops_ref.upfirdn2d_ref_simple(x.to(dt), k.to(dt), pad=(1, 1))
        if nz is not None:
            v = v + nw.to(dt) * nz.to(dt)
        if bias is not None:
            v = v + bias.to(dt).reshape(1, C, 1, 1)
        return v, torch.where(v > 0, v, v * alpha) * scale
    pre64, y64 = compose(torch.float64)
    _, y32 = compose(torch.float32)
    assert tuple(y64.shape) == (B, C, *out_hw)
    frac_pos = float((pre64 > 0).double().mean())
    assert 0.1 <= frac_pos <= 0.9, frac_pos                                     # both branches of the leaky relu are exercised

    def run(amax):
        n = B * C * out_hw[0] * out_hw[1]
        ybuf = torch.full((n + SLACK,), float("nan"), device=DEV)
        nzd = None
        if nz is not None:
            nbuf = torch.full((nz.numel() + 8,), float("nan"), device=DEV)
            nzd = nbuf[1:1 + nz.numel()] if unaligned else nbuf[:nz.numel()]
            nzd.copy_(nz.reshape(-1))
            assert (nzd.data_ptr() % 16 != 0) == unaligned
        _lib.launch("e3dge_blur_noise_bias_act", ybuf[:n], x.to(DEV), k.float().to(DEV), nzd, nw.to(DEV) if nz is not None else None,
                    None if bias is None else bias.to(DEV), alpha, scale, B, C, in_hw[0], in_hw[1], 1, 1, nb or 1, amax)
        torch.cuda.synchronize()
        assert bool(torch.isnan(ybuf[n:]).all()) and not bool(torch.isnan(ybuf[:n]).any())
        return ybuf[:n].clone().reshape(B, C, *out_hw)
    amax = torch.zeros(_lib.AMAX_FLOATS, device=DEV)
    y = run(amax)
    high = torch.full((_lib.AMAX_FLOATS,), 1000.0, device=DEV)
    y2 = run(high)
    tile_mask = torch.zeros(out_hw, dtype=torch.bool)                           # 64 x 64 tiles: the seam band and the last partial tile
    for b in range(64, max(out_hw), 64):
        tile_mask[max(b - 3, 0):b + 4, :] = True
        tile_mask[:, max(b - 3, 0):b + 4] = True
    tile_mask[64:, :] = True
    tile_mask[:, 64:] = True
    name = f"fir_parity_epi_{out_hw[0]}x{out_hw[1]}_noise{noise}_bias{int(with_bias)}"
    err, bound = _measure(name, y, y64, y32, tile_mask, frac_pos=frac_pos)
    amax_ok = float(amax.max()) == float(y.abs().max())
    kept = bool((high == 1000.0).all())
    record(name + "_amax", amax_is_the_maximum=amax_ok, preset_kept=kept, rerun_bit_identical=torch.equal(y, y2))
    assert err <= bound, (name, err, bound)
    assert amax_ok and kept and torch.equal(y, y2) and float(amax.min()) >= 0.0


# ---- e3dge_torgb: the skip up-sampler inside torgb_kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(4, 4), (8, 12), (36, 36)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("ci", [16, 128, 256])
def test_torgb_skip_upsampler_with_the_asymmetric_fir(ci, hw):
    """1 x 1 modulated product without demodulation + bias + upfirdn2d(skip, fir, up=2, pad=(2, 1)) against float64 in the three
    channel-group forms; with zero weight and bias the skip term alone, bit for bit what e3dge_upfirdn2d gives."""
    B, (H, W) = 2, hw
    g = torch.Generator().manual_seed(ci + H)
    x = torch.randn(B, ci, H, W, generator=g)
    w = torch.randn(3, ci, generator=g)
    s = 1 + 0.3 * torch.randn(B, ci, generator=g)
    bias = torch.tensor([0.21, -0.33, 0.05])
    skip = torch.randn(B, 3, H // 2, W // 2, generator=g)
    k = asym_fir(4.0)
    scale = float(np.float32(1 / np.sqrt(ci)))

    def compose(dt):
        wm = (scale * w.to(dt)).reshape(1, 3, ci) * s.to(dt).reshape(B, 1, ci)
        out = torch.einsum("bci,bihw->bchw", wm, x.to(dt)) + bias.to(dt).reshape(1, 3, 1, 1)
        return out + ops_ref.upfirdn2d_ref_simple(skip.to(dt), k.to(dt), up=2, pad=(2, 1))
    y64, y32 = compose(torch.float64), compose(torch.float32)

    def run(wd, bd):
        n = B * 3 * H * W
        ybuf = torch.full((n + SLACK,), float("nan"), device=DEV)
        _lib.launch("e3dge_torgb", ybuf[:n], x.to(DEV), wd, s.to(DEV), bd, skip.to(DEV), k.float().to(DEV), scale, B, ci, H, W)
        torch.cuda.synchronize()
        assert bool(torch.isnan(ybuf[n:]).all()) and not bool(torch.isnan(ybuf[:n]).any())
        return ybuf[:n].clone().reshape(B, 3, H, W)
    y = run(w.to(DEV), bias.to(DEV))
    name = f"fir_parity_torgb_ci{ci}_{H}x{W}"
    err, bound = _measure(name, y, y64, y32)
    only_skip = run(torch.zeros(3, ci, device=DEV), torch.zeros(3, device=DEV))
    up = op.upfirdn2d(skip.to(DEV), k.float().to(DEV), up=2, pad=(2, 1))
    same = torch.equal(only_skip, up)
    record(name + "_skip", bit_identical_to_upfirdn2d=same, max_diff=_err(only_skip, up.cpu()))
    assert err <= bound, (name, err, bound)
    assert same, name
