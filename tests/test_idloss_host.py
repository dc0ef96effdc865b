"""Identity term, host side: the C-ABI entries of csrc/idnet.hip (sizes, struct layouts, refusals before any launch), the Python
surface of e3dge_amd.id_loss / sharded_eval that needs no GPU, the CPU path against the recording of the reference
(tools/gen_golden_idloss.py), and the conditions on the float64 CPU truth without which a dead network would pass every parity test."""
import ctypes
import functools
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import GOLDEN, REPO, load_golden

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, sharded_eval, synthetic as syn
from e3dge_amd.id_loss import IDLoss, TAP_NAMES, tap_shapes

INVALID = -1                                                        # E3DGE_ERR_INVALID_ARG


# ---- inputs by formula (tools/gen_golden_idloss.py records the reference on the same) ---------------------------------------------
def make_pair(shape, seed):
    """tests/test_gpu_lpips.make_pair: gt = tanh(5x5 box-filtered 3 N(0,1)), pred = tanh(1.2 gt + 0.5 N(0,1))."""
    rs = np.random.RandomState(seed)
    n = torch.from_numpy(rs.standard_normal(shape)).float()
    gt = torch.tanh(F.avg_pool2d(F.pad(3.0 * n, [2] * 4, mode='replicate'), 5, 1))
    pred = torch.tanh(1.2 * gt + 0.5 * torch.from_numpy(rs.standard_normal(shape)).float())
    return pred.contiguous(), gt.contiguous()


def golden_images(n, size):
    """(pred, gt) of the recording: n pairs of size x size."""
    return make_pair((n, 3, size, size), seed=1000 + size + n)


def tap_samples(numel, count=256):
    return torch.from_numpy(np.random.RandomState(numel % 65521).randint(0, numel, size=count))


@functools.lru_cache(maxsize=None)
def module_cpu():
    return syn.load_synthetic_idloss(IDLoss())


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------------
def test_packed_image_workspace_and_tile_sizes(lib):
    n_params = sum(p.numel() for p in IDLoss().parameters())
    bn_stats = sum(b.numel() for k, b in IDLoss().state_dict().items() if 'running_' in k)
    # every weight once (conv K padded to 32: only the input layer's 27 grows), BN as (a, b) pairs, blocks rounded up to 64 floats
    assert 0.999 * n_params < lib.e3dge_idnet_packed_floats() < 1.001 * (n_params + bn_stats)
    assert lib.e3dge_idnet_ws_bytes(2) >= 4 * 2 * (3 * 64 * 112 * 112)
    assert lib.e3dge_idnet_conv_tiles(64, 13, 13, 3, 2) >= 1


@pytest.mark.parametrize("struct,mirror,names", [
    ("E3dgeIdnetArgs", "IdnetArgs", ["packed", "images", "n_per_set", "n_sets", "height", "width", "embeddings", "taps", "ws", "ws_bytes"]),
    ("E3dgeIdLossArgs", "IdLossArgs", ["y_hat", "y", "x", "batch", "dots", "loss", "sim_improvement"]),
    ("E3dgeIdnetPackSrc", "IdnetPackSrc", ["conv_w", "bn_weight", "bn_bias", "bn_mean", "bn_var", "prelu", "se_fc1", "se_fc2", "head_w", "head_b"])])
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


def good_args(keep, lib):
    """Arguments that pass every host-side check but the workspace size (the pointers are never followed)."""
    a = _lib.IdnetArgs()
    buf = (ctypes.c_char * 64)()
    keep.append(buf)
    p = ctypes.addressof(buf)
    a.packed = a.embeddings = a.ws = p
    a.images[0] = a.images[1] = p
    a.n_per_set, a.n_sets, a.height, a.width = 1, 2, 256, 256
    a.ws_bytes = lib.e3dge_idnet_ws_bytes(2) - 1
    return a


def test_bad_arguments_are_refused_before_any_launch(lib):
    keep = []
    emb = lambda a: lib.e3dge_idnet_embed(ctypes.byref(a), None)
    a = good_args(keep, lib)
    assert a.ws_bytes > 0
    assert emb(a) == INVALID and b"workspace" in lib.e3dge_last_error()
    for field, value, word in [("packed", None, b"null"), ("embeddings", None, b"null"), ("ws", None, b"null"), ("n_per_set", 0, b"n_per_set"),
                               ("n_sets", 0, b"n_sets"), ("n_sets", 4, b"n_sets"), ("height", 0, b"height"), ("width", -3, b"width")]:
        a = good_args(keep, lib)
        a.ws_bytes = 1 << 40
        setattr(a, field, value)
        assert emb(a) == INVALID, field
        assert word in lib.e3dge_last_error(), (field, lib.e3dge_last_error())
    a = good_args(keep, lib)
    a.ws_bytes = 1 << 40
    a.images[1] = None
    assert emb(a) == INVALID and b"image set 1" in lib.e3dge_last_error()
    assert lib.e3dge_idnet_embed(None, None) == INVALID
    assert lib.e3dge_idnet_ws_bytes(0) == -1 and lib.e3dge_idnet_ws_bytes(-2) == -1
    p = ctypes.addressof(keep[0])
    src = _lib.IdnetPackSrc()
    assert lib.e3dge_idnet_pack_weights(p, None, None) == INVALID and lib.e3dge_idnet_pack_weights(None, ctypes.addressof(src), None) == INVALID
    for f, _ in _lib.IdnetPackSrc._fields_:
        if f in ("head_w", "head_b"):
            setattr(src, f, p)
        else:
            getattr(src, f)[:] = [p] * len(getattr(src, f))
    src.se_fc2[7] = None
    assert lib.e3dge_idnet_pack_weights(p, ctypes.addressof(src), None) == INVALID and b"se 7" in lib.e3dge_last_error()
    la = _lib.IdLossArgs(y_hat=p, y=p, x=p, batch=0, dots=p)
    assert lib.e3dge_id_loss(ctypes.byref(la), None) == INVALID and b"batch" in lib.e3dge_last_error()
    la = _lib.IdLossArgs(y_hat=p, y=p, x=None, batch=1, dots=p)
    assert lib.e3dge_id_loss(ctypes.byref(la), None) == INVALID and b"null" in lib.e3dge_last_error()
    conv = lambda *sizes, out=p: lib.e3dge_idnet_conv(out, p, p, p, None, None, None, None, *sizes, None)
    assert conv(1, 3, 64, 9, 11, 3, 1, out=None) == INVALID
    for sizes in [(0, 3, 64, 9, 11, 3, 1), (1, 0, 64, 9, 11, 3, 1), (1, 3, 48, 9, 11, 3, 1), (1, 3, 64, 0, 11, 3, 1), (1, 3, 64, 9, 11, 5, 1),
                  (1, 3, 64, 9, 11, 3, 3)]:
        assert conv(*sizes) == INVALID, sizes
    assert lib.e3dge_idnet_conv_tiles(48, 8, 8, 3, 1) == -1
    assert lib.e3dge_image_metric_row(p, p, None, None, 0, 1.0, 0.8, 10.0, None) == INVALID and b"batch" in lib.e3dge_last_error()
    assert lib.e3dge_image_metric_row(None, p, None, None, 1, 1.0, 0.8, 10.0, None) == INVALID


# ---- the module -------------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_are_the_references():
    keys = json.load(open(os.path.join(GOLDEN, "idloss_state_dict_keys.json")))
    m = IDLoss()
    assert sorted(m.state_dict().keys()) == keys
    assert "facenet.body.5.res_layer.5.fc1.weight" in keys and "facenet.output_layer.4.running_var" in keys
    assert not any(p.requires_grad for p in m.parameters()) and not m.training and not m.train().facenet.training
    assert tap_shapes(2)[2:7] == [(2, 64, 56, 56), (2, 128, 28, 28), (2, 256, 14, 14), (2, 512, 7, 7), (2, 512, 7, 7)] and len(TAP_NAMES) == 8


def test_load_pretrained_round_trips_one_local_file(tmp_path):
    sd = module_cpu().facenet.state_dict()
    torch.save(sd, tmp_path / "ir_se50.pth")
    m = IDLoss().load_pretrained(str(tmp_path / "ir_se50.pth"))
    for k, v in m.facenet.state_dict().items():
        assert torch.equal(v, sd[k]), k
    short = {k: v for k, v in sd.items() if k != "body.3.shortcut_layer.1.running_mean"}
    torch.save(short, tmp_path / "short.pth")
    with pytest.raises(RuntimeError, match="missing"):
        IDLoss().load_pretrained(str(tmp_path / "short.pth"))
    torch.save(dict(sd, extra=torch.zeros(1)), tmp_path / "extra.pth")
    with pytest.raises(RuntimeError, match="unexpected"):
        IDLoss().load_pretrained(str(tmp_path / "extra.pth"))


def test_synthetic_weights_follow_the_recipe():
    sd = module_cpu().state_dict()
    w = sd["facenet.body.9.res_layer.1.weight"]
    assert abs(float(w.std()) / (2.0 / (256 * 9)) ** 0.5 - 1) < 0.02
    w2 = sd["facenet.body.9.res_layer.3.weight"]
    assert abs(float(w2.std()) / (syn.ID_CONV2_GAIN * (2.0 / (256 * 9)) ** 0.5) - 1) < 0.02
    assert abs(float(sd["facenet.body.9.res_layer.2.weight"].mean()) - 0.25) < 0.02
    assert float(sd["facenet.body.9.res_layer.4.running_var"].min()) > 0.2 and float(sd["facenet.body.9.res_layer.4.running_var"].std()) > 0.1
    assert torch.equal(syn.load_synthetic_idloss(IDLoss()).state_dict()["facenet.input_layer.0.weight"], sd["facenet.input_layer.0.weight"])


def test_grad_requiring_inputs_and_bad_shapes_raise():
    m = IDLoss()
    x = torch.zeros(1, 3, 256, 256, requires_grad=True)
    y = torch.zeros(1, 3, 256, 256)
    with pytest.raises(NotImplementedError, match="backward is not in this build"):
        m(x, y, y)
    with pytest.raises(NotImplementedError, match="backward is not in this build"):
        m.run(y, x)
    with pytest.raises(ValueError, match="one shape"):
        m(y, torch.zeros(1, 3, 128, 128), y)
    with pytest.raises(ValueError, match="one shape"):
        m.embed(torch.zeros(1, 3, 256, 200))


def same_bits(got, want, what, report):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    d = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    report[what] = d
    return np.array_equal(got, want)


def test_cpu_path_reproduces_the_recording_of_the_reference():
    """Bit for bit under the pinned CPU arithmetic (oracle.cpu_numerics); the fall-back of <= 2e-6 is reported, not silently taken."""
    gold = load_golden("idloss_ir_se50")
    m = module_cpu()
    rep = {}
    pred, gt = golden_images(3, 256)
    emb, taps = m._embed_sets([gt], taps=True)
    exact = same_bits(emb.numpy(), gold["embeddings"], "embeddings", rep)
    exact &= same_bits(taps[-1].numpy(), gold["head"], "head", rep)
    for name, t in zip(TAP_NAMES, taps):
        exact &= same_bits(t.reshape(-1)[tap_samples(t.numel())].numpy(), gold["tap_" + name], "tap_" + name, rep)
        assert abs(float(t.double().sum()) - float(gold["sum_" + name])) <= 1e-9 * float(t.double().abs().sum()), name
    loss, sim, logs = m(pred, gt, gt)
    dots = np.array([[d["diff_target"], d["diff_input"], d["diff_views"]] for d in logs])
    exact &= same_bits(dots, gold["dots"], "dots", rep)
    exact &= same_bits(loss.numpy(), gold["loss"], "loss", rep)
    assert abs(sim - float(gold["sim_improvement"])) <= 1e-12
    pred4, gt4 = golden_images(1, 1024)
    res = m.run(pred4, gt4, gt4)
    exact &= same_bits(res["embeddings"].numpy(), gold["emb_1024"], "emb_1024", rep)
    exact &= same_bits(res["dots"].double().numpy(), gold["dots_1024"], "dots_1024", rep)
    exact &= same_bits(res["loss"].numpy(), gold["loss_1024"], "loss_1024", rep)
    print("bit for bit" if exact else "within 2e-6", rep)
    assert max(rep.values()) <= 2e-6, rep
    assert exact, rep


@functools.lru_cache(maxsize=None)
def alive_stats():
    """Statistics of the float64 CPU forward with the synthetic weights on the test pair and an unrelated image."""
    m = syn.load_synthetic_idloss(IDLoss()).double()
    pred, gt = make_pair((1, 3, 256, 256), 7)
    _, other = make_pair((1, 3, 256, 256), 8)
    st = dict(prelu=[], gate=[], rms=[])
    for mod in m.facenet.modules():
        if isinstance(mod, nn.PReLU):
            mod.register_forward_hook(lambda q, i, o: st['prelu'].append(float((i[0] > 0).double().mean())))
        if isinstance(mod, nn.Sigmoid):
            mod.register_forward_hook(lambda q, i, o: st['gate'].append((float(o.mean()), float(((o < 0.01) | (o > 0.99)).double().mean()))))
    rms = lambda q, i, o: st['rms'].append(float(o.pow(2).mean().sqrt()))
    m.facenet.input_layer.register_forward_hook(rms)
    for u in m.facenet.body:
        u.register_forward_hook(rms)
    e = m.embed(torch.cat([pred, gt, other]).double())
    st['target'], st['unrelated'] = float(e[0] @ e[1]), float(e[0] @ e[2])
    return st


def test_the_synthetic_network_is_alive():
    st = alive_stats()
    assert len(st['prelu']) == 25 and len(st['gate']) == 24 and len(st['rms']) == 25
    for i, a in enumerate(st['prelu']):
        assert 0.2 <= a <= 0.8, f"PReLU {i}: {a:.2f} of its inputs positive"
    for u, (mean, sat) in enumerate(st['gate']):
        assert 0.1 < mean < 0.9 and sat < 0.01, (u, mean, sat)
    for u, r in enumerate(st['rms'][1:]):
        assert st['rms'][0] / 100 <= r <= st['rms'][0] * 100, (u, r, st['rms'][0])
    assert 0.2 <= st['target'] <= 0.98, st['target']
    assert st['target'] >= st['unrelated'] + 0.05, (st['target'], st['unrelated'])


# ---- the metric row ---------------------------------------------------------------------------------------------------------------
def test_image_metrics_torch_takes_an_identity_callable():
    g = torch.Generator().manual_seed(0)
    pred, gt = torch.rand(1, 3, 24, 24, generator=g) * 2 - 1, torch.rand(1, 3, 24, 24, generator=g) * 2 - 1
    fake_lp = lambda a, b: (a - b).abs().mean() * 0.5
    plain = sharded_eval.image_metrics_torch(pred, gt, 2.0, fake_lp, 0.8)
    assert torch.equal(plain, sharded_eval.image_metrics_torch(pred, gt, 2.0, fake_lp, 0.8, id_loss=None, id_lambda=10.0))
    assert float(plain[1]) == 0.0 and float(plain[7]) == 1.0
    seen = []

    def fake_id(y_hat, y, x):
        seen.append((y_hat is pred, y is gt, x is y))
        return (y_hat - y).pow(2).mean() * 0.3, 0.0, []                          # the reference's triple

    row = sharded_eval.image_metrics_torch(pred, gt, 2.0, fake_lp, 0.8, id_loss=fake_id, id_lambda=10.0)
    lid = fake_id(pred, gt, gt)[0]
    assert seen[0] == (True, True, True)                                          # builder.py:165: x is y
    assert torch.equal(row[1], lid) and torch.equal(row[7], 1 - lid)
    assert torch.equal(row[3], (plain[0] * 2.0 + fake_lp(pred, gt) * 0.8) + lid * 10.0)
    for c in (0, 2, 4, 5, 6):
        assert torch.equal(row[c], plain[c])
    scalar = sharded_eval.image_metrics_torch(pred, gt, 2.0, None, 0.0, id_loss=lambda a, b, c: lid, id_lambda=10.0)
    assert torch.equal(scalar[1], lid) and torch.equal(scalar[3], plain[0] * 2.0 + lid * 10.0)
    # CPU tensors go to the torch formulation through image_metrics as well
    assert torch.equal(sharded_eval.image_metrics(pred, gt, 2.0, fake_lp, 0.8, fake_id, 10.0), row)
    assert torch.equal(sharded_eval.image_metrics(pred, gt, 2.0, fake_lp, 0.8), plain)
