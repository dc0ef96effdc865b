"""LPIPS backward, host side: the C-ABI entries of csrc/lpips_bwd.h (packed-image sizes, argument checks that fail before any launch)
and the opt-in switch of e3dge_amd.lpips.LPIPS, as far as they need no GPU."""
import ctypes

import pytest
import torch

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, synthetic as syn
from e3dge_amd.lpips import LPIPS

INVALID = -1                                                        # E3DGE_ERR_INVALID_ARG


def test_the_forward_image_stays_and_the_transposed_one_holds_every_layer(lib):
    convs = 64 * 384 + 192 * 1600 + 384 * 1728 + 256 * 3456 + 256 * 2304
    assert lib.e3dge_lpips_packed_floats() == convs + 2 * (64 + 192 + 384 + 256 + 256)      # the forward image is as it was
    # W^T of conv 2..5: M = C_in, K = C_out k k (already multiples of 32), then conv 1
    pad = lambda k: (k + 31) // 32 * 32
    transposed = 64 * pad(192 * 25) + 192 * pad(384 * 9) + 384 * pad(256 * 9) + 256 * pad(256 * 9)
    assert lib.e3dge_lpips_packed_t_floats() >= transposed + 3 * 64 * 121


def good_args(keep, lib, both=False):
    """Arguments that pass every host-side check but the workspace size (the pointers are never followed)."""
    a = _lib.LpipsBwdArgs()
    buf = (ctypes.c_char * 64)()
    keep.append(buf)
    a.packed = a.packed_t = a.fwd_ws = a.upstream = a.grad_x = a.ws = ctypes.addressof(buf)
    if both:
        a.grad_y = ctypes.addressof(buf)
    a.batch, a.height, a.width = 1, 31, 40
    a.std[:] = [.458, .448, .450]
    a.fwd_ws_bytes = lib.e3dge_lpips_ws_bytes(1, 31, 40)
    a.ws_bytes = lib.e3dge_lpips_bwd_ws_bytes(1, 31, 40, int(both)) - 1        # too small: a "good" call stops here, before any launch
    return a


def test_bad_arguments_are_refused_before_any_launch(lib):
    keep = []
    bwd = lambda a: lib.e3dge_lpips_backward(ctypes.byref(a), None)
    for both in (False, True):
        a = good_args(keep, lib, both)
        assert a.ws_bytes > 0 and a.fwd_ws_bytes > 0
        assert bwd(a) == INVALID and b"workspace" in lib.e3dge_last_error()      # everything but the workspace is fine
    assert lib.e3dge_lpips_bwd_ws_bytes(1, 31, 40, 1) > lib.e3dge_lpips_bwd_ws_bytes(1, 31, 40, 0)
    a = good_args(keep, lib)
    a.ws_bytes = 1 << 40
    a.fwd_ws_bytes -= 1                                                          # the forward's workspace is checked as well
    assert bwd(a) == INVALID and b"workspace" in lib.e3dge_last_error()
    for field, value, word in [("packed", None, b"null"), ("packed_t", None, b"null"), ("fwd_ws", None, b"null"), ("upstream", None, b"null"),
                               ("ws", None, b"null"), ("grad_x", None, b"null"), ("batch", 0, b"batch"), ("batch", -3, b"batch"),
                               ("height", 30, b"height"), ("width", 30, b"width"), ("width", -5, b"width")]:
        a = good_args(keep, lib)
        setattr(a, field, value)                                                 # (grad_x = None leaves both gradients NULL)
        assert bwd(a) == INVALID, field
        assert word in lib.e3dge_last_error(), (field, lib.e3dge_last_error())
    a = good_args(keep, lib)
    a.std[2] = 0.0
    assert bwd(a) == INVALID and b"std" in lib.e3dge_last_error()
    a = good_args(keep, lib)
    a.grad_x, a.grad_y = None, ctypes.addressof(keep[0])                         # y alone is a valid request
    assert bwd(a) == INVALID and b"workspace" in lib.e3dge_last_error()
    assert lib.e3dge_lpips_backward(None, None) == INVALID
    assert lib.e3dge_lpips_bwd_ws_bytes(0, 64, 64, 0) == -1 and lib.e3dge_lpips_bwd_ws_bytes(1, 30, 64, 1) == -1
    assert lib.e3dge_lpips_bwd_ws_bytes(1, 64, 30, 0) == -1 and b"31" in lib.e3dge_last_error()
    p = ctypes.addressof(keep[0])
    five = (ctypes.c_void_p * 5)(*([p] * 5))
    hole = (ctypes.c_void_p * 5)(p, p, p, None, p)
    assert lib.e3dge_lpips_pack_weights_t(None, five, None) == INVALID and b"null" in lib.e3dge_last_error()
    assert lib.e3dge_lpips_pack_weights_t(p, None, None) == INVALID
    assert lib.e3dge_lpips_pack_weights_t(p, hole, None) == INVALID and b"layer 3" in lib.e3dge_last_error()


def test_the_switch_is_off_by_default_and_settable():
    m = syn.load_synthetic_lpips(LPIPS())
    assert m.differentiable is False and LPIPS(differentiable=True).differentiable is True
    x = torch.zeros(2, 3, 40, 40, requires_grad=True)
    y = torch.zeros(2, 3, 40, 40)
    with pytest.raises(NotImplementedError, match="LPIPS backward.*differentiable"):      # the refusal names the switch
        m(x, y)
    with pytest.raises(NotImplementedError, match="LPIPS backward"):
        m.run(y, x)
    m.differentiable = True
    for a, b in ((x, y), (y, x)):
        with pytest.raises(RuntimeError, match="GPU") as e:                               # the graph is wanted: only the device is wrong
            m(a, b)
        assert not isinstance(e.value, NotImplementedError)
    with pytest.raises(RuntimeError, match="GPU"):
        m.run_backward(y, y, torch.ones(2))
    with pytest.raises(ValueError, match="one shape"):
        m(x, torch.zeros(2, 3, 40, 41))
    assert list(m.state_dict().keys()) == list(LPIPS().state_dict().keys())               # the switch is no parameter or buffer
