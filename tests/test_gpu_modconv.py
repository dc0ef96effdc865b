"""GPU: the fused modulated 3x3 convolution (e3dge_modconv3x3) against the oracle's restatement of
ModulatedConv2d / StyledConv (oracle/decoder_ref.py, bit-identical to the reference on the decoder goldens), and against
the float64 evaluation of the same.

Stated fp32 tolerance: outputs are O(1) (demodulated weights have unit norm); the fp32 oracle itself sits ~1e-6 from
float64.  Bound: |hip - oracle| <= 2e-5 * max(1, max|out|) and |hip - f64| <= 3x the fp32 oracle's own distance + 1e-6*max|out|
-- the split-f16 contraction (hi+lo operands, three products, fp32 accumulate) is as accurate as an fp32 convolution.  The fused
tails (stride 1 and up-sampling StyledConv) and the planar ToRGB (e3dge_torgb, from 16 channels at 4 x 4 to 1,024 channels, square or
not) are held to the same float64 bound; measured (absolute, outputs of magnitude 4 - 9): StyledConv 1.6e-6 - 4.6e-6 where the fp32 oracle is 1.3e-6 - 2.1e-6 from float64,
ToRGB 0.9e-6 - 1.9e-6 where the fp32 oracle is 0.6e-6 - 6.1e-6."""
import math

import numpy as np
import pytest
import torch

from conftest import maxerr, record
from oracle import decoder_ref

import e3dge_amd  # noqa: F401
from e3dge_amd import synthetic as syn
from e3dge_amd.stylesdf_model import ModulatedConv2d, StyledConv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_layer(cls, ci, co, upsample, seed, prefix='decoder.convs.0.'):
    m = cls(ci, co, 3, 512, upsample=upsample)
    sd = {k: syn.synthetic_tensor(prefix + k, v.shape, seed) for k, v in m.state_dict().items() if not k.endswith('kernel')}
    m.load_state_dict(sd, strict=False)
    return m.to(DEV).eval(), {prefix + k: v for k, v in sd.items()}


def _f64(sd):
    return {k: v.double() for k, v in sd.items()}


def _vs_f64(name, y, ref, t64):
    """The figures of test_modulated_conv_vs_oracle for any fused layer: the kernel and the fp32 oracle against the float64 evaluation of
    the same oracle function on the same inputs, recorded before anything is asserted.  The bound they serve,
    vs_f64 <= 3 oracle_vs_f64 + 1e-6 out_max, is that test's: three times what fp32 arithmetic itself loses, plus 1e-6 of the output's
    magnitude."""
    e = dict(vs_oracle=maxerr(y, ref), vs_f64=maxerr(y, t64), oracle_vs_f64=maxerr(ref, t64), out_max=max(1.0, float(t64.abs().max())))
    record(name, **e)
    return e


CASES = [  # ci, co, H, W, B, upsample
    (16, 32, 8, 8, 1, False), (32, 64, 20, 36, 2, False), (64, 64, 64, 64, 1, False), (48, 96, 33, 70, 1, False),
    (256, 128, 16, 16, 2, False), (64, 32, 128, 128, 1, False), (128, 128, 130, 66, 1, False),
    (16, 32, 8, 8, 1, True), (32, 64, 20, 36, 2, True), (128, 64, 64, 64, 1, True), (64, 32, 70, 130, 1, True),
    (48, 96, 9, 150, 1, True),
]


@pytest.mark.parametrize("ci,co,H,W,B,upsample", CASES)
def test_modulated_conv_vs_oracle(ci, co, H, W, B, upsample):
    m, sd = make_layer(ModulatedConv2d, ci, co, upsample, seed=ci + co, prefix='decoder.convs.0.conv.')
    rs = np.random.RandomState(H * W + ci)
    x = torch.from_numpy((rs.standard_normal((B, ci, H, W)) * (0.2 + 2 * rs.uniform(size=(1, ci, 1, 1)))).astype(np.float32)).to(DEV)
    style = torch.from_numpy(rs.standard_normal((B, 512)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        assert m.fused_ok(x)
        y = m(x, style)
        ref = decoder_ref.modulated_conv(sd, 'decoder.convs.0.conv.', x.cpu(), style.cpu(), True, upsample)
        t64 = decoder_ref.modulated_conv({k: v.double() for k, v in sd.items()}, 'decoder.convs.0.conv.', x.cpu().double(),
                                         style.cpu().double(), True, upsample)
    scale = max(1.0, float(t64.abs().max()))
    e = dict(vs_oracle=maxerr(y, ref), vs_f64=maxerr(y, t64), oracle_vs_f64=maxerr(ref, t64), out_max=scale)
    record(f"modconv_{ci}_{co}_{H}x{W}_b{B}_up{int(upsample)}", **e)
    assert tuple(y.shape) == tuple(ref.shape)
    assert e['vs_oracle'] <= 2e-5 * scale and e['vs_f64'] <= 3 * e['oracle_vs_f64'] + 1e-6 * scale, e


@pytest.mark.parametrize("ci,co,H,W,B", [(32, 32, 24, 40, 2), (64, 128, 64, 64, 1)])
def test_styled_conv_fused_tail(ci, co, H, W, B):
    """Stride-1 StyledConv: conv + noise + bias + lrelu in ONE launch; fixed noise per sample and shared noise."""
    m, sd = make_layer(StyledConv, ci, co, False, seed=7)
    rs = np.random.RandomState(3)
    x = torch.from_numpy(rs.standard_normal((B, ci, H, W)).astype(np.float32)).to(DEV)
    style = torch.from_numpy(rs.standard_normal((B, 512)).astype(np.float32)).to(DEV)
    for nb in (1, B):
        noise = torch.from_numpy(rs.standard_normal((nb, 1, H, W)).astype(np.float32)).to(DEV)
        with torch.no_grad():
            y = m(x, style, noise=noise)
            ref = decoder_ref.styled_conv(sd, 'decoder.convs.0.', x.cpu(), style.cpu(), noise.cpu())
            t64 = decoder_ref.styled_conv(_f64(sd), 'decoder.convs.0.', x.cpu().double(), style.cpu().double(), noise.cpu().double())
        e = _vs_f64(f"styled_conv_{ci}_{co}_{H}x{W}_b{B}_noise{nb}", y, ref, t64)
        assert maxerr(y, ref) <= 2e-5 * max(1.0, float(ref.abs().max())), (nb, maxerr(y, ref))
        assert e['vs_f64'] <= 3 * e['oracle_vs_f64'] + 1e-6 * e['out_max'], e
    with torch.no_grad():
        a, b = m(x, style), m(x, style)                     # random noise: runs, differs between calls
    assert torch.isfinite(a).all() and not torch.equal(a, b)


def test_operand_scaling_is_magnitude_invariant():
    """The activations are scaled by a power of two derived from max|s|*max|x|: the relative error must not depend on the
    input magnitude (1e-6 ... 1e+5), and huge inputs must not overflow the f16 operands."""
    m, sd = make_layer(ModulatedConv2d, 32, 32, False, seed=2, prefix='decoder.convs.0.conv.')
    rs = np.random.RandomState(1)
    x0 = rs.standard_normal((1, 32, 32, 32)).astype(np.float32)
    style = torch.from_numpy(rs.standard_normal((1, 512)).astype(np.float32)).to(DEV)
    for mag in (1e-6, 1.0, 1e5):
        x = torch.from_numpy(x0 * np.float32(mag)).to(DEV)
        with torch.no_grad():
            y = m(x, style)
            t64 = decoder_ref.modulated_conv({k: v.double() for k, v in sd.items()}, 'decoder.convs.0.conv.', x.cpu().double(),
                                             style.cpu().double(), True, False)
        rel = maxerr(y, t64) / float(t64.abs().max())
        record(f"modconv_magnitude_{mag:g}", rel_err=rel)
        assert torch.isfinite(y).all() and rel <= 2e-6, (mag, rel)
    z = torch.zeros(1, 32, 32, 32, device=DEV)
    with torch.no_grad():
        assert float(m(z, style).abs().max()) == 0.0


def test_backends_agree_and_fused_is_not_slower():
    """The 1024^2 decoder's eight 3x3 layers on both backends (fused kernel vs e3dge_modconv_weights + library convolution):
    same results; timings recorded (informational: a slower fused path is a warning, not a failure)."""
    import os
    import time
    shapes = [(256, 512, 64, False), (512, 256, 64, True), (256, 256, 128, False), (256, 128, 128, True), (128, 128, 256, False),
              (128, 64, 256, True), (64, 64, 512, False), (64, 32, 512, True), (32, 32, 1024, False)]
    tot = dict(hip=0.0, library=0.0)
    rows = {}
    for ci, co, res, up in shapes:
        m, _ = make_layer(StyledConv, ci, co, up, seed=ci)
        x = torch.randn(1, ci, res, res, device=DEV)
        style = torch.randn(1, 512, device=DEV)
        ores = 2 * res if up else res
        noise = torch.randn(1, 1, ores, ores, device=DEV)
        out = {}
        for be in ("hip", "library"):
            os.environ["E3DGE_MODCONV"] = be
            try:
                with torch.no_grad():
                    for _ in range(2):
                        y = m(x, style, noise=noise)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(5):
                        y = m(x, style, noise=noise)
                    torch.cuda.synchronize()
                    ms = (time.perf_counter() - t0) / 5 * 1e3
            finally:
                os.environ.pop("E3DGE_MODCONV", None)
            out[be] = (y, ms)
            tot[be] += ms
        err = maxerr(out["hip"][0], out["library"][0])
        gflop = 2 * 9 * ci * co * res * res / 1e9
        rows[f"{ci}->{co}@{res}{'up' if up else ''}"] = dict(hip_ms=out["hip"][1], library_ms=out["library"][1], max_abs_diff=err,
                                                            hip_tflops=gflop / out["hip"][1])
        assert err <= 5e-5 * max(1.0, float(out["library"][0].abs().max())), (ci, co, res, up, err)
    record("modconv_decoder_layers", total_hip_ms=tot["hip"], total_library_ms=tot["library"],
           **{k + "_" + kk: vv for k, v in rows.items() for kk, vv in v.items()})
    # (wall-clock over five calls per layer: a number for the report, not a gate -- one disturbed call on a shared box must not fail the
    # parity suite; the decoder's timings are measured properly by bench.py and tools/dec2_check.py)
    if not tot["hip"] < 1.5 * tot["library"]:
        import warnings
        warnings.warn(f"fused modulated convolutions slower than the library path in this run: {tot}")


def _torgb_case(ci, H, W, B, with_skip, seed):
    """ToRGB (fused_ok) on a (B, ci, H, W) activation: the kernel's output, the fp32 oracle's and the float64 oracle's."""
    from e3dge_amd.stylesdf_model import ToRGB
    m = ToRGB(ci, 512, upsample=True)
    sd = {k: syn.synthetic_tensor('decoder.to_rgbs.0.' + k, v.shape, ci) for k, v in m.state_dict().items() if not k.endswith('kernel')}
    m.load_state_dict(sd, strict=False)
    m = m.to(DEV).eval()
    sdp = {'decoder.to_rgbs.0.' + k: v for k, v in sd.items()}
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.standard_normal((B, ci, H, W)).astype(np.float32)).to(DEV)
    style = torch.from_numpy(rs.standard_normal((B, 512)).astype(np.float32)).to(DEV)
    skip = torch.from_numpy(rs.standard_normal((B, 3, H // 2, W // 2)).astype(np.float32)).to(DEV) if with_skip else None
    with torch.no_grad():
        assert m.fused_ok(x, skip)
        y = m(x, style, skip=skip)
        ref = decoder_ref.to_rgb(sdp, 'decoder.to_rgbs.0.', x.cpu(), style.cpu(), None if skip is None else skip.cpu())
        t64 = decoder_ref.to_rgb(_f64(sdp), 'decoder.to_rgbs.0.', x.cpu().double(), style.cpu().double(),
                                 None if skip is None else skip.cpu().double())
    assert tuple(y.shape) == (B, 3, H, W)
    return y, ref, t64


@pytest.mark.parametrize("ci,res,B,with_skip", [(32, 16, 2, True), (512, 64, 1, False), (64, 128, 1, True), (48, 36, 2, True)])
def test_torgb_fused(ci, res, B, with_skip):
    """ToRGB in one launch (1x1 modulated conv without demodulation + bias + FIR-up-sampled skip) against the oracle, fp32 and float64."""
    y, ref, t64 = _torgb_case(ci, res, res, B, with_skip, seed=res)
    e = maxerr(y, ref)
    record(f"torgb_{ci}_{res}_b{B}_skip{int(with_skip)}", max_abs_err=e, out_max=float(ref.abs().max()))
    f = _vs_f64(f"torgb_f64_{ci}_{res}_b{B}_skip{int(with_skip)}", y, ref, t64)
    assert e <= 1e-5 * max(1.0, float(ref.abs().max())), e
    assert f['vs_f64'] <= 3 * f['oracle_vs_f64'] + 1e-6 * f['out_max'], f


@pytest.mark.parametrize("ci,H,W,B,with_skip", [(16, 4, 4, 2, True),          # the smallest shape fused_ok admits: a 2 x 2 skip image
                                                (1024, 16, 16, 1, True),      # the largest channel count it admits
                                                (32, 8, 12, 2, False)])       # not square
def test_torgb_fused_edge_shapes(ci, H, W, B, with_skip):
    """The same two bounds at the ends of what ToRGB.fused_ok admits."""
    y, ref, t64 = _torgb_case(ci, H, W, B, with_skip, seed=ci + H * W)
    f = _vs_f64(f"torgb_f64_{ci}_{H}x{W}_b{B}_skip{int(with_skip)}", y, ref, t64)
    assert f['vs_oracle'] <= 1e-5 * max(1.0, float(ref.abs().max())), f
    assert f['vs_f64'] <= 3 * f['oracle_vs_f64'] + 1e-6 * f['out_max'], f


def test_up_layer_fused_tail_and_amax_tracking():
    """Up-sampling StyledConv: transposed conv by phase -> blur + noise + bias + lrelu in one pass; the amax buffer it leaves
    equals max|output| (the next layer's operand scale comes from it)."""
    from e3dge_amd import _lib
    m, sd = make_layer(StyledConv, 64, 32, True, seed=9)
    rs = np.random.RandomState(8)
    x = torch.from_numpy(rs.standard_normal((2, 64, 24, 40)).astype(np.float32)).to(DEV)
    style = torch.from_numpy(rs.standard_normal((2, 512)).astype(np.float32)).to(DEV)
    noise = torch.from_numpy(rs.standard_normal((1, 1, 48, 80)).astype(np.float32)).to(DEV)
    am = torch.zeros(_lib.AMAX_FLOATS, device=DEV)
    with torch.no_grad():
        y = m(x, style, noise=noise, out_amax=am)
        ref = decoder_ref.styled_conv(sd, 'decoder.convs.0.', x.cpu(), style.cpu(), noise.cpu(), upsample=True)
        t64 = decoder_ref.styled_conv(_f64(sd), 'decoder.convs.0.', x.cpu().double(), style.cpu().double(), noise.cpu().double(), upsample=True)
    e = _vs_f64("styled_conv_up_64_32_24x40_b2", y, ref, t64)
    assert maxerr(y, ref) <= 2e-5 * max(1.0, float(ref.abs().max())), maxerr(y, ref)
    assert e['vs_f64'] <= 3 * e['oracle_vs_f64'] + 1e-6 * e['out_max'], e
    assert float(am.max()) == float(y.abs().max())
    m2, sd2 = make_layer(StyledConv, 32, 32, False, seed=10)
    am2 = torch.zeros(_lib.AMAX_FLOATS, device=DEV)
    with torch.no_grad():
        z = m2(y, style, noise=noise, in_amax=am, out_amax=am2)
        ref2 = decoder_ref.styled_conv(sd2, 'decoder.convs.0.', y.cpu(), style.cpu(), noise.cpu())
        t64_2 = decoder_ref.styled_conv(_f64(sd2), 'decoder.convs.0.', y.cpu().double(), style.cpu().double(), noise.cpu().double())
    e2 = _vs_f64("styled_conv_after_up_32_32_48x80_b2", z, ref2, t64_2)
    assert e2['vs_f64'] <= 3 * e2['oracle_vs_f64'] + 1e-6 * e2['out_max'], e2
    assert maxerr(z, ref2) <= 2e-5 * max(1.0, float(ref2.abs().max())) and float(am2.max()) == float(z.abs().max())
