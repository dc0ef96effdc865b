"""CPU: the entries of the trainable aligner's kernels around the convolutions (csrc/aligner_bwd.h, e3dge_aln_bn_* / _norm_bwd /
_prelu_bwd / _up2_bwd / _pick_bwd) -- the workspace size against a restatement and every refusal before a launch -- and the formulas the
kernels state (the (A, B, C) factors of the norm backward, the buffer update, the gather form of the bilinear x2 adjoint) against float64
autograd of the torch ops, so that a wrong sign or factor is found without a GPU.  tests/test_gpu_aligner_bwd.py runs the kernels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, alignment
from test_aligner_host import _last

SEGMENT = 4096                                                       # kAlnSeg: pixels of one partial sum


def norm_ws_bytes(n, c, h, w):
    """Two float64 partial sums per channel, image and segment of 4096 pixels, then three float64 factors per channel."""
    return 8 * (2 * c * n * ((h * w + SEGMENT - 1) // SEGMENT) + 3 * c)


def test_workspace_size_equals_its_restatement(lib):
    for n in (1, 2, 5, 256):
        for c, h, w in ((3, 1, 2), (16, 256, 256), (112, 64, 64), (64, 32, 32), (3, 64, 65), (4096, 1, 1)):
            assert lib.e3dge_aln_norm_ws_bytes(n, c, h, w) == norm_ws_bytes(n, c, h, w), (n, c, h, w)
    for bad in ((0, 3, 4, 4), (257, 3, 4, 4), (1, 0, 4, 4), (1, 4097, 4, 4), (1, 3, 0, 4), (1, 3, 4, 1025)):
        assert lib.e3dge_aln_norm_ws_bytes(*bad) == -1 and "n=" in _last(lib), bad


def test_entries_refuse_bad_arguments_before_a_launch(lib):
    """On a machine without a GPU a launch would fail with a launch error; a refusal is INVALID_ARG with a word that says why."""
    P, S, bad = 0x1000, None, -1                                     # a non-null address that is never dereferenced on the host
    ws = norm_ws_bytes(2, 8, 8, 8)

    def entry(name, keys, base):
        def call(**over):
            return getattr(lib, name)(*[{**base, **over}[k] for k in keys], S)
        return call
    shape = dict(n=2, c=8, h=8, w=8)
    out_of_range = [dict(n=0), dict(n=257), dict(c=0), dict(c=4097), dict(h=0), dict(w=0), dict(h=1025), dict(w=1025), dict(n=256, c=4096, h=1024, w=1024)]

    stats = entry("e3dge_aln_bn_stats", ("ab", "stats", "in0", "in1", "gamma", "beta", "ws", "ws_bytes", "n", "c", "split", "h", "w"),
                  dict(ab=P, stats=P, in0=P, in1=P, gamma=P, beta=P, ws=P, ws_bytes=ws, split=5, **shape))
    for over, word in [(dict(ab=None, stats=None), "null"), (dict(ws=None), "null"), (dict(gamma=None), "null"), (dict(beta=None), "null"),
                       (dict(in0=None), "null"), (dict(in1=None), "null"), (dict(split=-1), "split"), (dict(split=9), "split"),
                       (dict(ws_bytes=ws - 1), "workspace"), (dict(n=1, h=1, w=1), "batch statistics")] + [(o, "n=") for o in out_of_range]:
        assert stats(**over) == bad and word in _last(lib), (over, _last(lib))

    apply_ = entry("e3dge_aln_bn_apply", ("out", "inp", "ab", "slope", "sc", "sc_ab", "n", "c", "h", "w", "sh", "sw", "stride", "mode"),
                   dict(out=P, inp=P, ab=P, slope=P, sc=P, sc_ab=P, sh=8, sw=8, stride=1, mode=0, **shape))
    for over, word in [(dict(out=None), "null"), (dict(inp=None), "null"), (dict(ab=None), "null"), (dict(mode=-1), "shortcut_mode"), (dict(mode=4), "shortcut_mode"),
                       (dict(mode=1, sc=None), "shortcut_mode"), (dict(mode=2, sc=None), "shortcut_mode"), (dict(mode=3, sc_ab=None), "shortcut_mode"),
                       (dict(mode=1, stride=3), "stride"), (dict(mode=1, stride=0), "stride"), (dict(mode=1, stride=2), "picked"),
                       (dict(mode=1, stride=2, sh=15, sw=17), "picked"), (dict(mode=1, sh=9), "picked")] + [(o, "n=") for o in out_of_range]:
        assert apply_(**over) == bad and word in _last(lib), (over, _last(lib))

    norm = entry("e3dge_aln_norm_bwd", ("gx", "dgamma", "dbeta", "gy", "in0", "in1", "gamma", "stats", "rmean", "rvar", "add", "ws", "ws_bytes", "n", "c",
                                         "split", "h", "w", "train"),
                 dict(gx=P, dgamma=P, dbeta=P, gy=P, in0=P, in1=P, gamma=P, stats=P, rmean=P, rvar=P, add=P, ws=P, ws_bytes=ws, split=5, train=1, **shape))
    for over, word in [(dict(gx=None, dgamma=None, dbeta=None), "null"), (dict(gy=None), "null"), (dict(gamma=None), "null"), (dict(ws=None), "null"),
                       (dict(stats=None), "null"), (dict(train=0, rmean=None), "null"), (dict(train=0, rvar=None), "null"), (dict(in0=None), "null"),
                       (dict(in1=None), "null"), (dict(train=0, in0=None), "null"), (dict(train=2), "train"), (dict(train=-1), "train"), (dict(split=-1), "split"),
                       (dict(split=9), "split"), (dict(ws_bytes=ws - 1), "workspace")] + [(o, "n=") for o in out_of_range]:
        assert norm(**over) == bad and word in _last(lib), (over, _last(lib))

    prelu = entry("e3dge_aln_prelu_bwd", ("gx", "dslope", "gy", "pre", "slope", "ws", "ws_bytes", "n", "c", "h", "w"),
                  dict(gx=P, dslope=P, gy=P, pre=P, slope=P, ws=P, ws_bytes=ws, **shape))
    for over, word in [(dict(gx=None, dslope=None), "null"), (dict(gy=None), "null"), (dict(pre=None), "null"), (dict(slope=None), "null"), (dict(ws=None), "null"),
                       (dict(ws_bytes=ws - 1), "workspace")] + [(o, "n=") for o in out_of_range]:
        assert prelu(**over) == bad and word in _last(lib), (over, _last(lib))

    up = entry("e3dge_aln_up2_bwd", ("gx", "gy", "planes", "h", "w"), dict(gx=P, gy=P, planes=4, h=3, w=5))
    for over in [dict(gx=None), dict(gy=None), dict(planes=0), dict(planes=(1 << 20) + 1), dict(h=0), dict(w=0), dict(h=1025), dict(planes=1 << 20, h=1024, w=1024)]:
        assert up(**over) == bad, over
    pick = entry("e3dge_aln_pick_bwd", ("gx", "gy", "add", "planes", "h", "w", "stride"), dict(gx=P, gy=P, add=None, planes=4, h=9, w=13, stride=2))
    for over in [dict(gx=None), dict(gy=None), dict(planes=0), dict(h=0), dict(w=1025), dict(stride=0), dict(stride=3), dict(planes=1 << 20, h=1024, w=1024)]:
        assert pick(**over) == bad, over
    assert pick(stride=3) == bad and "stride" in _last(lib)


# ---- the kernels' formulas, restated in float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_norm_backward_factors_equal_autograd(train):
    """aln_norm_fold_kernel's (A, B, C): g_x = A g + B x + C, d gamma = Q, d beta = P, against float64 autograd of F.batch_norm."""
    rs = np.random.RandomState(3)
    n, c, h, w, eps = 2, 5, 3, 4, 1e-5
    x = torch.from_numpy(rs.standard_normal((n, c, h, w)) + 3.0).requires_grad_(True)
    gy, gamma, beta = (torch.from_numpy(rs.standard_normal(s)) for s in ((n, c, h, w), (c,), (c,)))
    gamma, beta = gamma.requires_grad_(True), beta.requires_grad_(True)
    rmean, rvar = torch.from_numpy(3.0 + 0.1 * rs.standard_normal(c)), torch.from_numpy(rs.uniform(0.5, 1.5, c))
    (F.batch_norm(x, rmean.clone(), rvar.clone(), gamma, beta, training=train, eps=eps) * gy).sum().backward()
    xd, M = x.detach(), n * h * w
    col = lambda v: v.reshape(1, c, 1, 1)
    mean, var = (xd.mean((0, 2, 3)), xd.var((0, 2, 3), unbiased=False)) if train else (rmean, rvar)
    rstd = 1.0 / torch.sqrt(var + eps)
    P, Q = gy.sum((0, 2, 3)), (gy * (xd - col(mean)) * col(rstd)).sum((0, 2, 3))
    A = gamma.detach() * rstd
    B = -A * Q * rstd / M if train else torch.zeros(c, dtype=torch.float64)
    C = -A * P / M - B * mean if train else torch.zeros(c, dtype=torch.float64)
    assert float((col(A) * gy + col(B) * xd + col(C) - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    assert float((Q - gamma.grad).abs().max()) <= 1e-12 * float(Q.abs().max()) and float((P - beta.grad).abs().max()) <= 1e-12 * float(P.abs().max())
    assert float(x.grad.std()) > 0.1


def test_buffer_update_formula_equals_batch_norm():
    """alignment._update_running_buffers: running <- (1 - m) running + m stat with the variance through M / (M - 1)."""
    rs = np.random.RandomState(4)
    n, c, h, w, m = 2, 5, 3, 4, 0.1
    x = torch.from_numpy(rs.standard_normal((n, c, h, w)) + 2.0)
    rmean, rvar = torch.from_numpy(rs.standard_normal(c)), torch.from_numpy(rs.uniform(0.5, 1.5, c))
    rm, rv = rmean.clone(), rvar.clone()
    F.batch_norm(x, rm, rv, None, None, training=True, momentum=m)
    M = n * h * w
    assert float(((1 - m) * rmean + m * x.mean((0, 2, 3)) - rm).abs().max()) <= 1e-14
    assert float(((1 - m) * rvar + m * x.var((0, 2, 3), unbiased=False) * (M / (M - 1)) - rv).abs().max()) <= 1e-14


@pytest.mark.parametrize("hw", [(1, 1), (1, 4), (3, 5), (8, 8)], ids=str)
def test_up2_adjoint_gather_window(hw):
    """aln_up2_bwd_kernel gathers input pixel (y, x) from output rows 2y - 2 .. 2y + 2 and columns 2x - 2 .. 2x + 2: no output pixel outside
    that window has a weight on it, and the window's weights reproduce autograd."""
    h, w = hw
    eye = torch.eye(h * w, dtype=torch.float64).reshape(h * w, 1, h, w)
    matrix = alignment.up2_bilinear(eye).reshape(h * w, 2 * h, 2 * w)                # row i: the output for a unit impulse at input pixel i
    assert torch.equal(matrix, F.interpolate(eye, size=(2 * h, 2 * w), mode='bilinear').reshape(h * w, 2 * h, 2 * w))
    for i in range(h * w):
        y, x = divmod(i, w)
        window = torch.zeros(2 * h, 2 * w, dtype=torch.bool)
        window[max(2 * y - 2, 0):2 * y + 3, max(2 * x - 2, 0):2 * x + 3] = True
        assert float(matrix[i][~window].abs().sum()) == 0.0, (hw, i)
        assert float(matrix[i].sum()) > 0


# ---- the convolution gradients' entries ---------------------------------------------------------------------------------------------------
def wgrad_ws_floats(n, cin, cout, h, w, ks, stride):
    """One (cout, cin ks^2) float32 partial per image and segment of 1024 output pixels."""
    out = lambda v: (v + (2 if ks == 3 else 0) - ks) // stride + 1
    return n * ((out(h) * out(w) + 1023) // 1024) * cout * cin * ks * ks


def test_wgrad_workspace_equals_its_restatement(lib):
    for n in (1, 2, 5, 256):
        for shape in ((6, 16, 256, 256, 3, 1), (16, 32, 256, 256, 1, 2), (32, 32, 256, 256, 3, 2), (112, 64, 64, 64, 3, 1), (16, 3, 256, 256, 3, 1), (3, 3, 9, 13, 3, 2)):
            assert lib.e3dge_aln_wgrad_ws_floats(n, *shape) == wgrad_ws_floats(n, *shape), (n, shape)
    for bad in ((0, 6, 16, 8, 8, 3, 1), (257, 6, 16, 8, 8, 3, 1), (1, 0, 16, 8, 8, 3, 1), (1, 6, 65, 8, 8, 3, 1), (1, 6, 16, 0, 8, 3, 1), (1, 6, 16, 8, 1025, 3, 1),
                (1, 6, 16, 8, 8, 2, 1), (1, 6, 16, 8, 8, 3, 3)):
        assert lib.e3dge_aln_wgrad_ws_floats(*bad) == -1 and "n=" in _last(lib), bad


def test_conv_gradient_entries_refuse_bad_arguments_before_a_launch(lib):
    P, S, bad = 0x1000, None, -1
    shape = [dict(n=0), dict(n=257), dict(cin=0), dict(cin=4097), dict(cout=0), dict(cout=65), dict(h=0), dict(w=1025), dict(ks=2), dict(ks=5), dict(stride=0),
             dict(stride=3)]
    keys = ("gx", "gy", "wt", "add0", "add1", "wfrag", "floats", "n", "cin", "cout", "h", "w", "ks", "stride")
    base = dict(gx=P, gy=P, wt=P, add0=None, add1=None, wfrag=P, floats=16 * 160, n=2, cin=8, cout=16, h=8, w=8, ks=3, stride=1)
    dgrad = lambda **o: lib.e3dge_aln_conv_dgrad(*[{**base, **o}[k] for k in keys], S)
    for over in [dict(gx=None), dict(gy=None), dict(wt=None), dict(wfrag=None), dict(floats=16 * 160 - 1)] + shape:
        assert dgrad(**over) == bad, over
    assert dgrad(floats=100) == bad and "wfrag" in _last(lib)
    assert dgrad(gy=None) == bad and "null" in _last(lib)
    ws = wgrad_ws_floats(2, 8, 16, 8, 8, 3, 1)
    keys = ("dw", "gy", "in0", "in1", "in_ab", "ws", "floats", "n", "cin", "split", "up4", "cout", "h", "w", "ks", "stride")
    base = dict(dw=P, gy=P, in0=P, in1=P, in_ab=None, ws=P, floats=ws, n=2, cin=8, split=5, up4=0, cout=16, h=8, w=8, ks=3, stride=1)
    wgrad = lambda **o: lib.e3dge_aln_conv_wgrad(*[{**base, **o}[k] for k in keys], S)
    for over in [dict(dw=None), dict(gy=None), dict(ws=None), dict(in0=None), dict(in1=None), dict(split=-1), dict(split=9), dict(up4=2), dict(up4=1, h=6),
                 dict(floats=ws - 1)] + shape:
        assert wgrad(**over) == bad, over
    assert wgrad(floats=ws - 1) == bad and "workspace" in _last(lib)
    assert wgrad(split=9) == bad and "split" in _last(lib)


# ---- the network's entries ---------------------------------------------------------------------------------------------------------------
import ctypes  # noqa: E402

from e3dge_amd import synthetic as syn  # noqa: E402
from e3dge_amd.alignment import ResidualAligner  # noqa: E402
import test_aligner_host as host  # noqa: E402
from test_aligner_host import _Fake, _up  # noqa: E402

P256 = 256 * 256


def unit_table():
    """(cin, depth, stride, input size) of the 18 units in launch order."""
    out = []
    for name, s in zip(alignment.STAGES, (256, 128, 64, 64, 128, 256)):
        for cin, depth, stride in alignment.STAGES[name]:
            out.append((cin, depth, stride, s))
            s //= stride
    return out


def bn_channels():
    return 16 + sum(cin + depth + (depth if cin != depth else 0) for cin, depth, _, _ in unit_table())


def norm_part_floats(n):
    return 2 * (2 * 112 * n * 16 + 3 * 112)                          # the widest BatchNorm input's partial sums, float64


def saved_bytes(n):
    """c0 and feat1; per unit the raw sums c1 and c2, the PReLU output t1, the raw 1x1 branch and the unit's output (the last unit writes
    the caller's); the three up-sampled maps; per call the (a, b) pairs and the statistics' partial sums.  Blocks on multiples of 64 floats."""
    total = 2 * _up(n * 16 * P256, 64)
    units = unit_table()
    for i, (cin, depth, stride, s) in enumerate(units):
        o = s // stride
        total += 2 * _up(n * depth * s * s, 64) + _up(n * depth * o * o, 64) * (1 + (cin != depth) + (i + 1 < len(units)))
    total += _up(n * 64 * 64 * 64, 64) + _up(n * 32 * 128 * 128, 64) + _up(n * 16 * P256, 64)
    return 4 * (total + _up(2 * bn_channels(), 64) + _up(norm_part_floats(n), 64))


def bwd_workspace_bytes(n):
    per_image = [16 * P256] * 4 + [32 * P256] * 3 + [16 * P256, 16 * P256, 32 * P256 // 4, 48 * P256 // 16, 16 * P256, 6 * P256]
    wg = max([wgrad_ws_floats(n, 6, 16, 256, 256, 3, 1)] + [max(wgrad_ws_floats(n, cin, depth, s, s, 3, 1), wgrad_ws_floats(n, depth, depth, s, s, 3, stride))
                                                            for cin, depth, stride, s in unit_table()])
    return 4 * (sum(_up(n * f, 64) for f in per_image) + _up(wg, 64) + _up(norm_part_floats(n), 64))


def test_network_size_entries_equal_their_restatement(lib):
    m = host.module_cpu()
    src = m.sources()
    assert lib.e3dge_aligner_grad_floats() == sum(t.numel() for t in src) == 596801 + 2 * bn_channels()
    assert lib.e3dge_aligner_stats_channels() == bn_channels() == sum(b.num_features for b in m.batch_norms()) and len(m.batch_norms()) == 46
    off = 0
    for i, t in enumerate(src):                                      # one slot per source tensor, in order, of its own size
        assert lib.e3dge_aligner_grad_offset(i) == off, i
        off += t.numel()
    assert lib.e3dge_aligner_grad_offset(len(src)) == off
    assert lib.e3dge_aligner_grad_offset(-1) == -1 and lib.e3dge_aligner_grad_offset(len(src) + 1) == -1
    image_t = lambda ci, co, ks: _up(_up(ci, 16) * _up(co * ks * ks, 32), 64)
    assert lib.e3dge_aligner_packed_t_floats() == image_t(6, 16, 3) + sum(image_t(ci, d, 3) + image_t(d, d, 3) + (image_t(ci, d, 1) if ci != d else 0)
                                                                           for ci, d, _, _ in unit_table())
    for n in (1, 2, 5, 256):
        assert lib.e3dge_aligner_saved_bytes(n) == saved_bytes(n), n
        assert lib.e3dge_aligner_bwd_workspace_bytes(n) == bwd_workspace_bytes(n), n
        assert lib.e3dge_aligner_branch_count(n) == n * (16 * P256 + sum(d * s * s for _, d, _, s in unit_table())), n
    assert lib.e3dge_aligner_branch_count(2) == 17563648             # the PReLU decisions of one B = 2 step
    for n in (0, -1, 257):
        for entry in (lib.e3dge_aligner_saved_bytes, lib.e3dge_aligner_bwd_workspace_bytes, lib.e3dge_aligner_branch_count):
            assert entry(n) == -1 and "n=" in _last(lib), n


def test_network_entries_refuse_bad_arguments_before_a_launch(lib):
    P, S, bad = 0x1000, None, -1
    adr = ctypes.addressof
    n_src = _lib.ALIGNER_SOURCES
    src = (ctypes.c_void_p * n_src)(*([P] * n_src))
    hole = (ctypes.c_void_p * n_src)(*([P] * (n_src - 1) + [None]))
    want = (ctypes.c_uint8 * n_src)(*([1] * n_src))
    total, total_t = lib.e3dge_aligner_packed_floats(), lib.e3dge_aligner_packed_t_floats()
    assert lib.e3dge_aligner_pack_t(None, total_t, adr(src), n_src, S) == bad and "null" in _last(lib)
    assert lib.e3dge_aligner_pack_t(P, total_t, None, n_src, S) == bad and "null" in _last(lib)
    assert lib.e3dge_aligner_pack_t(P, total_t - 1, adr(src), n_src, S) == bad and "packed" in _last(lib)
    assert lib.e3dge_aligner_pack_t(P, total_t, adr(src), n_src - 1, S) == bad and "n_src" in _last(lib)
    assert lib.e3dge_aligner_pack_t(P, total_t, adr(hole), n_src, S) == bad and "null" in _last(lib)
    saved, ws, channels, floats = lib.e3dge_aligner_saved_bytes(1), lib.e3dge_aligner_bwd_workspace_bytes(1), bn_channels(), lib.e3dge_aligner_grad_floats()

    def fwd(**over):
        f = dict(packed=P, packed_floats=total, src=adr(src), n_src=n_src, train=1, res_gt=P, thumb=P, n=1, size=256, split=3, thumb_up4=1, out=P, saved=P,
                 saved_bytes=saved, stats=P, stats_doubles=2 * channels)
        f.update(over)
        return _lib.AlignerSaveArgs(**f)
    assert lib.e3dge_aligner_forward_saving(None, S) == bad
    for over, word in [(dict(packed=None), "null"), (dict(res_gt=None), "null"), (dict(thumb=None), "null"), (dict(out=None), "null"), (dict(saved=None), "null"),
                       (dict(stats=None), "null"), (dict(src=None), "null"), (dict(src=adr(hole)), "null"), (dict(n=0), "n="), (dict(n=300), "n="),
                       (dict(size=64), "size"), (dict(split=-1), "split"), (dict(split=7), "split"), (dict(thumb_up4=2), "thumb_up4"), (dict(train=2), "train"),
                       (dict(n_src=n_src - 1), "n_src"), (dict(packed_floats=total - 1), "packed"), (dict(saved_bytes=saved - 1), "saved"), (dict(n=2), "saved"),
                       (dict(stats_doubles=2 * channels - 1), "stats")]:
        assert lib.e3dge_aligner_forward_saving(ctypes.byref(fwd(**over)), S) == bad and word in _last(lib), (over, _last(lib))

    def bwd(**over):
        f = dict(packed=P, packed_floats=total, packed_t=P, packed_t_floats=total_t, src=adr(src), want=adr(want), n_src=n_src, train=1, res_gt=P, thumb=P, g_out=P,
                 n=1, size=256, split=3, thumb_up4=1, want_input=1, saved=P, saved_bytes=saved, stats=P, d_res_gt=P, d_thumb=P, grads=P, grad_floats=floats, ws=P,
                 ws_bytes=ws)
        f.update(over)
        return _lib.AlignerBwdArgs(**f)
    assert lib.e3dge_aligner_backward(None, S) == bad
    for over, word in [(dict(packed=None), "null"), (dict(packed_t=None), "null"), (dict(src=None), "null"), (dict(want=None), "null"), (dict(g_out=None), "null"),
                       (dict(saved=None), "null"), (dict(ws=None), "null"), (dict(res_gt=None), "null"), (dict(thumb=None), "null"), (dict(stats=None), "null"),
                       (dict(d_res_gt=None), "null"), (dict(d_thumb=None), "null"), (dict(grads=None), "null"), (dict(src=adr(hole)), "null"), (dict(n=0), "n="),
                       (dict(n=257), "n="), (dict(size=128), "size"), (dict(split=7), "split"), (dict(thumb_up4=-1), "thumb_up4"), (dict(train=3), "train"),
                       (dict(want_input=2), "want_input"), (dict(n_src=5), "n_src"), (dict(packed_floats=total - 1), "packed"),
                       (dict(packed_t_floats=total_t - 1), "packed"), (dict(saved_bytes=saved - 1), "saved"), (dict(grad_floats=floats - 1), "gradient"),
                       (dict(ws_bytes=ws - 1), "workspace"), (dict(n=2), "saved")]:
        assert lib.e3dge_aligner_backward(ctypes.byref(bwd(**over)), S) == bad and word in _last(lib), (over, _last(lib))
    count = lib.e3dge_aligner_branch_count(1)
    keys = ("out", "out_bytes", "packed", "packed_floats", "saved", "saved_bytes", "n", "train")
    base = dict(out=P, out_bytes=count, packed=P, packed_floats=total, saved=P, saved_bytes=saved, n=1, train=0)
    branch = lambda **o: lib.e3dge_aligner_branch_bytes(*[{**base, **o}[k] for k in keys], S)
    for over, word in [(dict(out=None), "null"), (dict(packed=None), "null"), (dict(saved=None), "null"), (dict(n=0), "n="), (dict(train=2), "train"),
                       (dict(out_bytes=count - 1), "out of"), (dict(packed_floats=total - 1), "packed"), (dict(saved_bytes=saved - 1), "saved")]:
        assert branch(**over) == bad and word in _last(lib), (over, _last(lib))


# ---- dispatch --------------------------------------------------------------------------------------------------------------------------------
def test_differentiable_is_off_by_default_and_comes_from_the_options():
    assert not ResidualAligner(syn.aligner_opt()).differentiable
    assert ResidualAligner(syn.aligner_opt(), differentiable=True).differentiable
    assert not ResidualAligner(syn.aligner_opt(differentiable_aligner=True), differentiable=False).differentiable
    assert ResidualAligner(syn.aligner_opt(differentiable_aligner=True)).differentiable
    m = ResidualAligner(syn.aligner_opt())
    m.differentiable = True                                          # a settable attribute, as HGFilter's
    assert m.differentiable and list(m.state_dict()) == list(ResidualAligner(syn.aligner_opt()).state_dict())


def test_grad_dispatch_rules(monkeypatch):
    monkeypatch.setattr(torch, "is_tensor", lambda t: True)          # (_Fake stands in for a GPU tensor)
    monkeypatch.delenv("E3DGE_ALIGNER", raising=False)
    off = ResidualAligner(syn.aligner_opt())
    assert not off._runs_hip_grad(_Fake(requires_grad=True))         # off by default: today's paths
    off.train()
    assert not off._runs_hip_grad(_Fake(requires_grad=True)) and not off._runs_hip(_Fake(requires_grad=True))
    m = ResidualAligner(syn.aligner_opt(), differentiable=True)
    for mode in (True, False):                                       # both forms, with a wanted gradient
        m.train(mode)
        for p in m.parameters():
            p.requires_grad_(True)
        assert m._runs_hip_grad(_Fake()) and m._runs_hip_grad(_Fake(requires_grad=True))
        res = _Fake(shape=(2, 3, 256, 256))
        assert m._runs_hip_grad(res, _Fake(shape=(2, 3, 64, 64))) and m._runs_hip_grad(res, _Fake(shape=(2, 3, 256, 256), requires_grad=True))
        with torch.no_grad():
            assert not m._runs_hip_grad(_Fake(requires_grad=True))
        for p in m.parameters():
            p.requires_grad_(False)
        assert not m._runs_hip_grad(_Fake())                         # nothing requires grad
        assert m._runs_hip_grad(_Fake(requires_grad=True))           # the input alone
        m.dconv_layer3[2].res_layer[2].weight.requires_grad_(True)
        assert m._runs_hip_grad(_Fake())                             # one parameter alone
        wanted = _Fake(requires_grad=True)
        assert not m._runs_hip_grad(_Fake(device="cpu", requires_grad=True)) and not m._runs_hip_grad(_Fake(dtype=torch.float64, requires_grad=True))
        assert not m._runs_hip_grad(_Fake(dtype=torch.float16, requires_grad=True))
        for shape in [(2, 6, 64, 64), (2, 6, 256, 128), (2, 3, 256, 256), (2, 7, 256, 256), (6, 256, 256), (0, 6, 256, 256), (300, 6, 256, 256)]:
            assert not m._runs_hip_grad(_Fake(shape=shape, requires_grad=True)), shape
        for thumb in [_Fake(shape=(2, 3, 128, 128)), _Fake(shape=(1, 3, 64, 64)), _Fake(shape=(2, 4, 64, 64)), _Fake(shape=(2, 3, 64, 64), device="cuda:1")]:
            assert not m._runs_hip_grad(_Fake(shape=(2, 3, 256, 256), requires_grad=True), thumb), thumb.shape
        monkeypatch.setenv("E3DGE_ALIGNER", "torch")
        assert not m._runs_hip_grad(wanted)
        monkeypatch.delenv("E3DGE_ALIGNER")
        assert m._runs_hip_grad(wanted)
    m.train()
    m.conv_layer3[1].res_layer[4].momentum = None                    # the cumulative moving average stays on the torch layers
    assert not m._runs_hip_grad(_Fake(requires_grad=True))
    m.eval()
    assert m._runs_hip_grad(_Fake(requires_grad=True))               # (the eval form reads no momentum)
    for over in [dict(aligner_norm_type='instance'), dict(aligner_norm_type='none'), dict(aligner_demodulate=True)]:
        with torch.device("meta"):
            other = ResidualAligner(syn.aligner_opt(**over), differentiable=True)
        assert not other._runs_hip_grad(_Fake(requires_grad=True)), over


def test_train_mode_on_the_cpu_takes_the_torch_layers(monkeypatch):
    called = []
    monkeypatch.setattr(_lib, "launch", lambda name, *a: called.append(name))
    m = syn.load_synthetic_aligner(ResidualAligner(syn.aligner_opt(), differentiable=True)).train()
    x = host.aligner_input(1, 0).requires_grad_(True)
    assert not m._runs_hip_grad(x)
    m(x).sum().backward()
    assert not called and x.grad is not None and int(m.conv_layer1[1].num_batches_tracked) == 1


# ---- the float64 truth of a train-form step is alive -----------------------------------------------------------------------------------------
def test_train_form_truth_is_alive_and_its_zero_gradients_are_the_stated_set():
    """In the train form every trailing and shortcut BatchNorm bias whose unit's output reaches only batch-statistic BatchNorms has a
    mathematically zero gradient: all res_layer.4.bias and shortcut_layer.1.bias except those of dconv_layer3.1 and dconv_layer3.2 -- 24 of
    the 157 parameters.  tests/test_gpu_aligner_bwd.py bounds those by magnitude and the others by relative error."""
    m = syn.load_synthetic_aligner(ResidualAligner(syn.aligner_opt())).double().train()
    x = host.aligner_input(1, 0).double().requires_grad_(True)
    taps = {}
    out = m.forward_torch(x, taps)
    for t in taps.values():
        t.retain_grad()
    g = torch.from_numpy(np.random.RandomState(77).standard_normal((1, 3, 256, 256)))
    out.backward(g)
    amax = {k: float(p.grad.abs().max()) for k, p in m.named_parameters()}
    live = max(v for k, v in amax.items() if k.endswith(".bias"))
    zero = {k for k, v in amax.items() if v <= 1e-6 * live}
    stated = {f"{name}.{i}.{layer}.bias" for name in alignment.STAGES for i in range(3) for layer in ("res_layer.4", "shortcut_layer.1")
              if not (name == "dconv_layer3" and i >= 1)} & set(amax)
    assert zero == stated and len(zero) == 24 and len(amax) == 157
    assert min(v for k, v in amax.items() if k not in zero) > 1.0
    assert float(x.grad.std()) > 0.05
    for name, t in taps.items():                                     # each of the seven taps' paths reaches the input and carries a gradient
        assert t.grad is not None and float(t.grad.std()) > 1e-3, name


# ---- the recording of the reference's train-form step ---------------------------------------------------------------------------------------
def test_cpu_autograd_in_train_mode_reproduces_the_recording_bit_for_bit():
    """tools/gen_golden_aligner_grads.py: the reference's ResidualAligner in train(), one forward + backward at B = 2 in float32.  The module's
    torch layers under autograd give the same gradients and the same updated running buffers, bit for bit."""
    from conftest import load_golden
    from test_encoder_host import samples
    gold = load_golden("aligner_grads")
    names = [str(k) for k in gold["names"]]
    m = syn.load_synthetic_aligner(ResidualAligner(syn.aligner_opt())).train()
    x = host.aligner_input(2, 0).requires_grad_(True)
    g = torch.from_numpy(np.random.RandomState(77).standard_normal((2, 3, 256, 256)).astype(np.float32))
    (m(x) * g).sum().backward()
    grads = dict(dx=x.grad, **{k: p.grad for k, p in m.named_parameters()})
    assert list(grads) == names and len(names) == 158
    for i, k in enumerate(names):
        flat = grads[k].reshape(-1)
        assert np.array_equal(flat[samples(flat.numel())[:64]].numpy(), gold["samples_f32"][i]), k
        assert float(flat.double().sum()) == float(gold["sum_f32"][i]), k
    state = m.state_dict()
    for i, k in enumerate(map(str, gold["buffer_names"])):
        assert np.array_equal(state[k].numpy(), gold[f"buffer_{i}_f32"]), k
        assert float(np.abs(gold[f"buffer_{i}_f32"] - gold[f"buffer_{i}_f64"]).max()) < 1e-5
    assert float(gold["max_f64"][0]) > 10 and len(gold["buffer_names"]) == 6


# ---- the listings alignment.py derives ------------------------------------------------------------------------------------------------------
def test_running_statistic_slots_are_the_running_buffers_of_sources():
    """The derived slots against the state dict: the positions in sources() of the tensors whose keys end in running_mean / running_var."""
    m = ResidualAligner(syn.aligner_opt())
    src = m.sources()
    running = [t for k, t in m.state_dict(keep_vars=True).items() if k.endswith(("running_mean", "running_var"))]
    want = {i for i, t in enumerate(src) if any(t is r for r in running)}
    assert len(running) == 2 * len(m.batch_norms()) == 92 and len(want) == 92
    assert m.running_statistic_slots() == want
    assert all(src[i].requires_grad for i in range(len(src)) if i not in want)      # (everything else is a Parameter)


def test_bn_planes_are_what_every_batch_norm_sees():
    """_bn_planes against a forward hook on every BatchNorm of one B = 1 forward_torch, in batch_norms() order."""
    m = syn.load_synthetic_aligner(ResidualAligner(syn.aligner_opt())).eval()
    seen = {}

    def hook(mod, inp, out):
        seen[id(mod)] = inp[0].shape[-2] * inp[0].shape[-1]
    hooks = [bn.register_forward_hook(hook) for bn in m.batch_norms()]
    with torch.no_grad():
        m.forward_torch(host.aligner_input(1, 0))
    for h in hooks:
        h.remove()
    assert len(m.batch_norms()) == 46 == len({id(bn) for bn in m.batch_norms()})
    assert alignment._bn_planes(46) == [seen[id(bn)] for bn in m.batch_norms()]
