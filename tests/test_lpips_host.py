"""LPIPS, host side: the C-ABI entries of csrc/lpips.hip (packed-image size, argument checks that fail before any launch; the mirror itself is
tests/test_abi_mirror.py) and
the Python surface of e3dge_amd.lpips / sharded_eval that needs no GPU."""
import ctypes

import pytest
import torch

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, sharded_eval, synthetic as syn
from e3dge_amd.lpips import LPIPS, tap_shapes

INVALID = -1                                                        # E3DGE_ERR_INVALID_ARG
STATE_DICT_KEYS = ["net.mean", "net.std"] + [f"net.layers.{i}.{p}" for i in (0, 3, 6, 8, 10) for p in ("weight", "bias")] + [
    f"lin.{i}.1.weight" for i in range(5)]


def test_packed_image_size(lib):
    # five conv images with K padded to a multiple of 32, five biases, five lin rows
    convs = 64 * 384 + 192 * 1600 + 384 * 1728 + 256 * 3456 + 256 * 2304
    assert lib.e3dge_lpips_packed_floats() == convs + 2 * (64 + 192 + 384 + 256 + 256)


def good_args(keep, lib):
    """Arguments that pass every host-side check but the workspace size (the pointers are never followed)."""
    a = _lib.LpipsArgs()
    buf = (ctypes.c_char * 64)()
    keep.append(buf)
    a.packed = a.x = a.y = a.per_image = a.ws = ctypes.addressof(buf)
    a.batch, a.height, a.width = 1, 31, 40
    a.mean[:] = [-.030, -.088, -.188]
    a.std[:] = [.458, .448, .450]
    a.ws_bytes = lib.e3dge_lpips_ws_bytes(1, 31, 40) - 1             # too small: a "good" call stops here, before any launch
    return a


def test_bad_arguments_are_refused_before_any_launch(lib):
    keep = []
    fwd = lambda a: lib.e3dge_lpips_forward(ctypes.byref(a), None)
    a = good_args(keep, lib)
    assert a.ws_bytes > 0
    assert fwd(a) == INVALID and b"workspace" in lib.e3dge_last_error()          # everything but the workspace is fine
    for field, value, word in [("packed", None, b"null"), ("x", None, b"null"), ("y", None, b"null"), ("per_image", None, b"null"),
                               ("ws", None, b"null"), ("batch", 0, b"batch"), ("height", 30, b"height"), ("width", 30, b"width"),
                               ("width", -5, b"width")]:
        a = good_args(keep, lib)
        a.ws_bytes = 1 << 40
        setattr(a, field, value)
        assert fwd(a) == INVALID, field
        assert word in lib.e3dge_last_error(), (field, lib.e3dge_last_error())
    a = good_args(keep, lib)
    a.ws_bytes = 1 << 40
    a.std[1] = 0.0
    assert fwd(a) == INVALID and b"std" in lib.e3dge_last_error()
    assert lib.e3dge_lpips_forward(None, None) == INVALID
    assert lib.e3dge_lpips_ws_bytes(0, 64, 64) == -1 and lib.e3dge_lpips_ws_bytes(1, 30, 64) == -1 and lib.e3dge_lpips_ws_bytes(1, 64, 30) == -1
    assert b"31" in lib.e3dge_last_error()
    # the workspace holds at least the five conv outputs of the 2B images
    acts = sum(c * h * w for c, h, w in tap_shapes(256, 256))
    assert lib.e3dge_lpips_ws_bytes(2, 256, 256) >= 4 * 4 * acts
    p = ctypes.addressof(keep[0])
    five = (ctypes.c_void_p * 5)(*([p] * 5))
    hole = (ctypes.c_void_p * 5)(p, p, None, p, p)
    assert lib.e3dge_lpips_pack_weights(None, five, five, five, None) == INVALID
    assert lib.e3dge_lpips_pack_weights(p, None, five, five, None) == INVALID
    assert lib.e3dge_lpips_pack_weights(p, five, five, hole, None) == INVALID and b"layer 2" in lib.e3dge_last_error()
    # the one row entry: a NULL lpips_per_image is a valid call (the column is 0), so only row, sums and batch can be refused
    assert lib.e3dge_image_metric_row(p, None, p, None, 1, 1.0, 0.8, 0.0, None) == INVALID and b"null" in lib.e3dge_last_error()
    assert lib.e3dge_image_metric_row(None, p, p, None, 1, 1.0, 0.8, 0.0, None) == INVALID and b"null" in lib.e3dge_last_error()
    assert lib.e3dge_image_metric_row(p, p, p, None, 0, 1.0, 0.8, 0.0, None) == INVALID and b"batch" in lib.e3dge_last_error()


def test_tap_shapes():
    assert tap_shapes(256, 256) == [(64, 63, 63), (192, 31, 31), (384, 15, 15), (256, 15, 15), (256, 15, 15)]
    assert tap_shapes(31, 31) == [(64, 7, 7), (192, 3, 3), (384, 1, 1), (256, 1, 1), (256, 1, 1)]
    assert tap_shapes(95, 71)[:3] == [(64, 23, 17), (192, 11, 8), (384, 5, 3)]


def test_state_dict_keys_are_the_references():
    m = LPIPS()
    assert list(m.state_dict().keys()) == STATE_DICT_KEYS
    assert m.net.mean.shape == (1, 3, 1, 1) and m.net.mean.reshape(-1).tolist() == pytest.approx([-.030, -.088, -.188])
    assert m.net.std.reshape(-1).tolist() == pytest.approx([.458, .448, .450])
    assert m.net.layers[3].weight.shape == (192, 64, 5, 5) and m.lin[2][1].weight.shape == (1, 384, 1, 1)
    assert not any(p.requires_grad for p in m.parameters())
    assert LPIPS(device="cpu", net_type="alex", version="0.1").net.layers[0].weight.device.type == "cpu"


def test_load_pretrained_reads_two_local_files(tmp_path):
    src = syn.load_synthetic_lpips(LPIPS(), seed=3)
    sd = src.state_dict()
    alex = {f"features.{i}.{p}": sd[f"net.layers.{i}.{p}"] for i in (0, 3, 6, 8, 10) for p in ("weight", "bias")}
    alex["classifier.1.weight"] = torch.zeros(4, 4)                               # torchvision's file carries the classifier too
    lin = {f"lin{i}.model.1.weight": sd[f"lin.{i}.1.weight"] for i in range(5)}
    torch.save(alex, tmp_path / "alexnet.pth")
    torch.save(lin, tmp_path / "alex.pth")
    m = LPIPS().load_pretrained(str(tmp_path / "alexnet.pth"), str(tmp_path / "alex.pth"))
    got = m.state_dict()
    assert list(got.keys()) == STATE_DICT_KEYS
    for k in STATE_DICT_KEYS:
        assert torch.equal(got[k], sd[k]), k
    del lin["lin4.model.1.weight"]
    torch.save(lin, tmp_path / "short.pth")
    with pytest.raises(RuntimeError, match="missing"):
        LPIPS().load_pretrained(str(tmp_path / "alexnet.pth"), str(tmp_path / "short.pth"))


def test_synthetic_weights_follow_the_recipe():
    sd = syn.load_synthetic_lpips(LPIPS()).state_dict()
    w = sd["net.layers.8.weight"]
    assert abs(float(w.std()) / (2.0 / (384 * 9)) ** 0.5 - 1) < 0.02
    assert abs(float(sd["net.layers.6.bias"].std()) / 0.1 - 1) < 0.15
    for i, c in enumerate((64, 192, 384, 256, 256)):
        lin = sd[f"lin.{i}.1.weight"]
        assert float(lin.min()) >= 0 and abs(float(lin.mean()) * c / 4 / 0.7979 - 1) < 0.2      # E|N(0,1)| = 0.7979
    assert torch.equal(syn.load_synthetic_lpips(LPIPS()).state_dict()["net.layers.0.weight"], sd["net.layers.0.weight"])


def test_python_surface_refuses_what_it_does_not_cover():
    for net in ("vgg", "squeeze"):
        with pytest.raises(NotImplementedError):
            LPIPS(net_type=net)
    m = syn.load_synthetic_lpips(LPIPS())
    x = torch.zeros(1, 3, 40, 40)
    with pytest.raises(RuntimeError, match="GPU"):
        m(x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        m(x, x, per_image=True)


def test_grad_requiring_inputs_and_bad_shapes_raise():
    m = LPIPS()
    x = torch.zeros(2, 3, 40, 40, requires_grad=True)
    y = torch.zeros(2, 3, 40, 40)
    with pytest.raises(NotImplementedError, match="LPIPS backward"):
        m(x, y)
    with pytest.raises(NotImplementedError, match="LPIPS backward"):
        m(y, x)
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):               # no graph is recorded: only the device is wrong
        m(x, y)
    with pytest.raises(ValueError, match="one shape"):
        m(y, torch.zeros(2, 3, 40, 41))
    with pytest.raises(ValueError, match="31"):
        m(torch.zeros(1, 3, 30, 64), torch.zeros(1, 3, 30, 64))


def test_image_metrics_torch_takes_a_callable():
    g = torch.Generator().manual_seed(0)
    pred, gt = torch.rand(1, 3, 24, 24, generator=g) * 2 - 1, torch.rand(1, 3, 24, 24, generator=g) * 2 - 1
    plain = sharded_eval.image_metrics_torch(pred, gt)
    assert float(plain[2]) == 0.0 and torch.equal(plain[3], plain[0])
    fake = lambda a, b: (a - b).abs().mean() * 0.5
    row = sharded_eval.image_metrics_torch(pred, gt, l2_lambda=2.0, lpips=fake, vgg_lambda=0.8)
    lp = fake(pred, gt)
    assert torch.equal(row[2], lp)
    assert float(row[3]) == pytest.approx(float(2.0 * plain[0] + 0.8 * lp), rel=1e-6)
    for c in (0, 1, 4, 5, 6, 7):
        assert torch.equal(row[c], plain[c])
    # CPU tensors go to the torch formulation through image_metrics as well
    assert torch.equal(sharded_eval.image_metrics(pred, gt, 2.0, fake, 0.8), row)
    assert torch.equal(sharded_eval.image_metrics(pred, gt), plain)
