"""Identity term backward, host side: the C-ABI entries of csrc/idnet_bwd.h (sizes, struct layouts, refusals before any launch) and
the Python switch of e3dge_amd.id_loss.IDLoss on CPU tensors, where the torch layers run under autograd (the reference's own path)."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

from conftest import REPO

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, synthetic as syn
from e3dge_amd.id_loss import CROP, IDLoss, mask_shapes
from test_idloss_host import make_pair

INVALID = -1                                                        # E3DGE_ERR_INVALID_ARG
PRELU_INPUTS, RES_FLOATS = 3713024, 1781248                         # per image


def test_transposed_image_saved_state_and_workspace_sizes(lib):
    conv = sum(p.numel() for n, p in IDLoss().named_parameters() if p.ndim == 4 and ".fc" not in n)
    # every conv weight once: K = (co, r, s) is a multiple of 32 already, only the input layer's M = 3 grows to 16
    assert conv < lib.e3dge_idnet_packed_t_floats() <= conv + 13 * 576 + 64 * 52
    assert sum(c * h * w for _, c, h, w in mask_shapes(1)) == PRELU_INPUTS
    for n in (1, 3):
        per = lib.e3dge_idnet_saved_bytes(n) / n
        assert PRELU_INPUTS + 4 * RES_FLOATS <= per <= 1.01 * (PRELU_INPUTS + 4 * RES_FLOATS) + 256 * 100
        assert lib.e3dge_idnet_bwd_ws_bytes(n, 256, 256) >= 4 * n * 3 * 64 * 112 * 112
    assert lib.e3dge_idnet_saved_bytes(0) == -1 and lib.e3dge_idnet_bwd_ws_bytes(0, 256, 256) == -1
    assert lib.e3dge_idnet_bwd_ws_bytes(1, 0, 256) == -1


@pytest.mark.parametrize("struct,mirror,names", [
    ("E3dgeIdnetSaveArgs", "IdnetSaveArgs", ["net", "saved", "saved_bytes", "n_saved"]),
    ("E3dgeIdnetBwdArgs", "IdnetBwdArgs", ["packed", "packed_t", "saved", "saved_bytes", "n", "height", "width", "grad_embeddings", "grad_images",
                                           "gstage", "masks", "ws", "ws_bytes"]),
    # the forward's structs keep their layouts
    ("E3dgeIdnetArgs", "IdnetArgs", ["packed", "images", "n_per_set", "n_sets", "height", "width", "embeddings", "taps", "ws", "ws_bytes"]),
    ("E3dgeIdLossArgs", "IdLossArgs", ["y_hat", "y", "x", "batch", "dots", "loss", "sim_improvement"])])
def test_struct_layouts_match_c(struct, mirror, names):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "e3dge_hip.h"\nint main(void) {\n  printf("%zu", sizeof(' + struct + '));\n' + \
          "".join(f'  printf(" %zu", offsetof({struct}, {n}));\n' for n in names) + "  return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    A = getattr(_lib, mirror)
    assert got == [ctypes.sizeof(A)] + [getattr(A, n).offset for n in names]
    if struct == "E3dgeIdnetArgs":
        assert got[0] == 136                                         # as before this addition


def test_bad_arguments_are_refused_before_any_launch(lib):
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)                                        # never followed

    def bwd_args():
        a = _lib.IdnetBwdArgs()
        a.packed = a.packed_t = a.saved = a.grad_embeddings = a.grad_images = a.ws = p
        a.n, a.height, a.width = 2, 256, 256
        a.saved_bytes = a.ws_bytes = 1 << 40
        return a

    bwd = lambda a: lib.e3dge_idnet_backward(ctypes.byref(a), None)
    a = bwd_args()
    a.ws_bytes = lib.e3dge_idnet_bwd_ws_bytes(2, 256, 256) - 1
    assert bwd(a) == INVALID and b"workspace" in lib.e3dge_last_error()
    a = bwd_args()
    a.saved_bytes = lib.e3dge_idnet_saved_bytes(2) - 1
    assert bwd(a) == INVALID and b"saved" in lib.e3dge_last_error()
    for field, value, word in [("packed", None, b"null"), ("packed_t", None, b"null"), ("saved", None, b"null"), ("grad_embeddings", None, b"null"),
                               ("grad_images", None, b"null"), ("ws", None, b"null"), ("n", 0, b"n="), ("height", 0, b"height"),
                               ("width", -3, b"width")]:
        a = bwd_args()
        setattr(a, field, value)
        assert bwd(a) == INVALID, field
        assert word in lib.e3dge_last_error(), (field, lib.e3dge_last_error())
    assert lib.e3dge_idnet_backward(None, None) == INVALID

    def save_args():
        s = _lib.IdnetSaveArgs()
        s.net.packed = s.net.embeddings = s.net.ws = s.saved = p
        s.net.images[0] = s.net.images[1] = p
        s.net.n_per_set, s.net.n_sets, s.net.height, s.net.width = 1, 2, 256, 256
        s.net.ws_bytes = s.saved_bytes = 1 << 40
        s.n_saved = 1
        return s

    save = lambda s: lib.e3dge_idnet_embed_save(ctypes.byref(s), None)
    s = save_args()
    s.saved_bytes = lib.e3dge_idnet_saved_bytes(1) - 1
    assert save(s) == INVALID and b"saved" in lib.e3dge_last_error()
    s = save_args()
    s.net.ws_bytes = lib.e3dge_idnet_ws_bytes(2) - 1
    assert save(s) == INVALID and b"workspace" in lib.e3dge_last_error()
    for n_saved in (0, 3):
        s = save_args()
        s.n_saved = n_saved
        assert save(s) == INVALID and b"n_saved" in lib.e3dge_last_error()
    s = save_args()
    s.saved = None
    assert save(s) == INVALID and b"null" in lib.e3dge_last_error()
    s = save_args()
    s.net.packed = None
    assert save(s) == INVALID and b"null" in lib.e3dge_last_error()
    assert lib.e3dge_idnet_embed_save(None, None) == INVALID

    src = _lib.IdnetPackSrc()
    assert lib.e3dge_idnet_pack_weights_t(p, None, None) == INVALID and lib.e3dge_idnet_pack_weights_t(None, ctypes.addressof(src), None) == INVALID
    src.conv_w[:] = [p] * len(src.conv_w)
    src.conv_w[50] = None
    assert lib.e3dge_idnet_pack_weights_t(p, ctypes.addressof(src), None) == INVALID and b"conv 50" in lib.e3dge_last_error()

    conv = lambda *sizes, out=p, mask=None, slope=None, scale=None: lib.e3dge_idnet_conv_bwd(out, p, p, p, None, mask, slope, scale, None, *sizes, None)
    assert conv(1, 3, 64, 9, 11, 3, 1, out=None) == INVALID and b"null" in lib.e3dge_last_error()
    assert conv(1, 3, 64, 9, 11, 3, 1, mask=p) == INVALID                          # a mask without slopes
    assert conv(1, 3, 64, 9, 11, 3, 1, mask=p, slope=p, scale=p) == INVALID        # two epilogues
    for sizes in [(0, 3, 64, 9, 11, 3, 1), (1, 0, 64, 9, 11, 3, 1), (1, 3, 0, 9, 11, 3, 1), (1, 3, 64, 0, 11, 3, 1), (1, 3, 64, 9, 11, 5, 1),
                  (1, 3, 64, 9, 11, 3, 3)]:
        assert conv(*sizes) == INVALID, sizes
    assert lib.e3dge_idnet_prep_bwd(None, p, 1, 256, 256, None) == INVALID and b"null" in lib.e3dge_last_error()
    assert lib.e3dge_idnet_prep_bwd(p, p, 0, 256, 256, None) == INVALID and b"n=" in lib.e3dge_last_error()
    assert lib.e3dge_idnet_prep_bwd(p, p, 1, 256, 0, None) == INVALID and b"width" in lib.e3dge_last_error()


def test_the_default_module_still_raises_and_the_switch_is_settable():
    m = IDLoss()
    assert m.differentiable is False and IDLoss(differentiable=True).differentiable is True
    x = torch.zeros(1, 3, 256, 256, requires_grad=True)
    y = torch.zeros(1, 3, 256, 256)
    with pytest.raises(NotImplementedError, match="backward is not in this build"):
        m(x, y, y)
    with pytest.raises(NotImplementedError, match="backward is not in this build"):
        m.run(y, x)
    with torch.no_grad():
        m.run(x, y)                                                  # no grad wanted: the plain forward
    m.differentiable = True
    assert not any(p.requires_grad for p in m.parameters())
    assert "differentiable" not in m.state_dict()
    with pytest.raises(NotImplementedError, match="embed"):
        m.embed(x)                                                   # the gradient exists for the loss only: no silent plain forward
    with pytest.raises(RuntimeError, match="GPU"):
        m.run_backward(y, y, torch.ones(1))                          # the debug entry is the HIP path


def test_cpu_gradient_is_plain_autograd_through_the_same_layers():
    """Size 64: the 256^2 pool in front of the crop is on the path too."""
    m = syn.load_synthetic_idloss(IDLoss(differentiable=True))
    plain = syn.load_synthetic_idloss(IDLoss())
    pred, gt = make_pair((2, 3, 64, 64), seed=5)
    _, other = make_pair((2, 3, 64, 64), seed=6)
    y_hat, y, x = pred.clone().requires_grad_(True), gt.clone().requires_grad_(True), other.clone().requires_grad_(True)
    loss, sim, logs = m(y_hat, y, x)
    with torch.no_grad():
        want_loss, want_sim, want_logs = plain(pred, gt, other)
    assert torch.equal(loss.detach(), want_loss) and sim == want_sim and logs == want_logs
    loss.backward()
    assert y.grad is None and x.grad is None and y_hat.grad is not None

    z = pred.clone().requires_grad_(True)
    f = plain.facenet
    prep = lambda t: plain.face_pool(plain.id_loss_pool(t)[:, :, CROP[0]:CROP[1], CROP[2]:CROP[3]])
    fh = f(prep(z))
    with torch.no_grad():
        fy = f(prep(gt))
    ref = sum(1 - fh[b].dot(fy[b]) for b in range(2)) / 2
    ref.backward()
    assert float(z.grad.abs().max()) > 0
    assert torch.equal(y_hat.grad, z.grad)
    # under no_grad, and for a y_hat that wants no gradient, the differentiable module is the plain one
    with torch.no_grad():
        assert torch.equal(m.run(y_hat, y)['loss'], plain.run(pred, gt)['loss'])
    assert not m.run(pred, y)['loss'].requires_grad
