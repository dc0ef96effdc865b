"""CPU: the C-ABI of the renderer's parameter gradients -- the place of the fields appended to the two backward structs, and argument
checks that run before anything touches a GPU.  (The mirror itself is checked against the header in tests/test_abi_mirror.py.)"""
import ctypes

import pytest

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


NEW_SYMBOLS = ("e3dge_siren_wgrad", "e3dge_siren_wgrad_ws_floats")


def test_new_symbols_exported(lib):
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name), name


def test_appended_backward_fields_match_c():
    """(Their offsets against C: tests/test_abi_mirror.py.)"""
    S, R = _lib.SirenBwdArgs, _lib.RenderBwdArgs
    # appended at the end: every field that existed in ABI 15 keeps its place
    assert S.d_lin.offset > S.d_tex_beta.offset and R.d_lin.offset > R.phase.offset


def _err(lib):
    return (lib.e3dge_last_error() or b"").decode()


def test_siren_wgrad_rejects_null_and_other_precisions(lib):
    assert lib.e3dge_siren_wgrad(None, None) == -1
    assert "null" in _err(lib)
    fake = 1 << 20                                              # never dereferenced: the checks fail first
    a = _lib.SirenWgradArgs(args=fake, d_lin=fake, lin_amax=fake, pts=fake, d_w=fake, d_w_view_dirs=fake, d_w_first=fake,
                            d_w_sigma=fake, d_b_sigma=fake, d_w_rgb=fake, d_b_rgb=fake, ws=fake, ws_floats=1 << 40, n_pts=16,
                            batch=1, samples=1, precision=_lib.PREC_F16X3, box_scale=1.0)
    for prec in (_lib.PREC_F32, _lib.PREC_F16X3, _lib.PREC_F16X3_V1):
        a.precision = prec
        assert lib.e3dge_siren_wgrad(ctypes.byref(a), None) == -1
        assert "F16X3_G2" in _err(lib)
    a.precision = _lib.PREC_F16X3_G2
    a.d_w = None
    assert lib.e3dge_siren_wgrad(ctypes.byref(a), None) == -1
    assert "null output" in _err(lib)
    a.d_w, a.d_lin = fake, None
    assert lib.e3dge_siren_wgrad(ctypes.byref(a), None) == -1
    assert "null input" in _err(lib)
    a.d_lin, a.ws_floats = fake, 1
    assert lib.e3dge_siren_wgrad(ctypes.byref(a), None) == -1
    assert "workspace" in _err(lib)
    assert lib.e3dge_siren_wgrad_ws_floats(0, 16) == 0 and lib.e3dge_siren_wgrad_ws_floats(1, 0) == 0
    assert lib.e3dge_siren_wgrad_ws_floats(2, 1000) > lib.e3dge_siren_wgrad_ws_floats(1, 1000) > 8 * 256 * 256


def test_backward_d_lin_needs_g2(lib):
    fake = 1 << 20
    for prec in (_lib.PREC_F32, _lib.PREC_F16X3):
        a = _lib.SirenBwdArgs(packed=fake, film=fake, args=fake, wg=fake, wb=fake, partials=fake, dfilm=fake, dstyles=fake,
                              batch=1, precision=prec, n_pts=16, box_scale=1.0, d_lin=fake, lin_amax=fake)
        assert lib.e3dge_siren_bwd(ctypes.byref(a), None) == -1
        assert "F16X3_G2" in _err(lib)
        r = _lib.RenderBwdArgs(packed=fake, film=fake, args=fake, sdf=fake, dists=fake, points=fake, weights=fake, t_vals=fake,
                               near=fake, far=fake, wg=fake, wb=fake, sigmoid_beta=0.1, batch=1, height=4, width=4, n_samples=8,
                               precision=prec, d_rgb_pts=fake, d_sdf_pts=fake, partials=fake, dfilm=fake, dstyles=fake,
                               d_lin=fake, lin_amax=fake)
        assert lib.e3dge_siren_render_bwd(ctypes.byref(r), None) == -1
        assert "F16X3_G2" in _err(lib)
    a = _lib.SirenBwdArgs(packed=fake, film=fake, args=fake, wg=fake, wb=fake, partials=fake, dfilm=fake, dstyles=fake,
                          batch=1, precision=_lib.PREC_F16X3_G2, n_pts=16, box_scale=1.0, d_lin=fake, lin_amax=None)
    assert lib.e3dge_siren_bwd(ctypes.byref(a), None) == -1
    assert "lin_amax" in _err(lib)
