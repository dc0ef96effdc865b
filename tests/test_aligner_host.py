"""CPU: the 2-D residual aligner (e3dge_amd.alignment) -- its state-dict keys and its torch composition against the recording of the
reference's ResidualAligner (tools/gen_golden_aligner.py, bit for bit), the dispatch rules, align() against the call site's composition,
the restated bilinear x2 against F.interpolate, the size entries against a restatement and the refusals of the e3dge_aligner_* /
e3dge_aln_* entries.

Inputs are a formula (aligner_input); the weights are synthetic.load_synthetic_aligner's.  tests/test_gpu_aligner.py shares the helpers."""
import copy
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_golden

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, synthetic as syn
from e3dge_amd import alignment
from e3dge_amd.alignment import ResidualAligner
from test_encoder_host import parity_bound, samples  # noqa: F401  (the project's standing bound; the 256 sampled positions)

TENSORS = ("out",) + alignment.TAPS                                   # the output and the seven taps (dfea3 is the output)
GOLDEN_CASE = (2, 0)                                                  # batch, input seed of aligner.npz


def aligner_input(n, seed, size=256):
    """(n, 6, size, size): smooth structure plus noise, different per image and channel, unit scale."""
    rs = np.random.RandomState(9500 + seed)
    shape = (n, 6, size, size)
    yy, xx = np.meshgrid(np.linspace(-1, 1, size), np.linspace(-1, 1, size), indexing='ij')
    phase = rs.uniform(0, 2 * np.pi, size=(n, 6, 1, 1))
    freq = rs.uniform(1, 6, size=(n, 6, 1, 1))
    v = np.sin(freq * xx[None, None] + phase) * np.cos(0.5 * freq * yy[None, None] - phase) + 0.7 * rs.standard_normal(shape)
    return torch.from_numpy(v.astype(np.float32))


@functools.lru_cache(maxsize=None)
def _module_cpu(over, dtype, seed):
    if dtype != torch.float32:
        return copy.deepcopy(_module_cpu(over, torch.float32, seed)).to(dtype)
    m = syn.load_synthetic_aligner(ResidualAligner(syn.aligner_opt(**dict(over))), seed).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def module_cpu(dtype=torch.float32, seed=0, **over):
    """The aligner with the synthetic weights on the CPU; shared, never modified."""
    return _module_cpu(tuple(sorted(over.items())), dtype, seed)


def run_with_taps(m, x):
    taps = {}
    with torch.no_grad():
        out = m.forward_torch(x, taps)
    return dict(out=out, **taps)


@functools.lru_cache(maxsize=None)
def cpu_results(n, seed, weights=0):
    """(float64 truth, float32 torch composition) of TENSORS for aligner_input(n, seed); computed once, never modified."""
    x = aligner_input(n, seed)
    return run_with_taps(module_cpu(torch.float64, weights), x.double()), run_with_taps(module_cpu(torch.float32, weights), x)


# ---- keys -------------------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_equal_the_recording():
    recorded = json.load(open(os.path.join(GOLDEN, "aligner_state_dict_keys.json")))
    m = module_cpu()
    ours = list(m.state_dict())
    assert sorted(ours) == recorded["batch"] and len(ours) == 295
    assert sum(p.numel() for p in m.parameters()) == 596801
    for name in ("instance", "none", "demodulate"):
        with torch.device("meta"):
            o = dict(aligner_demodulate=True) if name == "demodulate" else dict(aligner_norm_type=name)
            other = ResidualAligner(syn.aligner_opt(**o))
        assert sorted(other.state_dict()) == recorded[name], name


def test_sources_are_every_read_tensor_once():
    m = module_cpu()
    src = m.sources()
    assert len({id(t) for t in src}) == len(src) == _lib.ALIGNER_SOURCES == 6 + 18 * 11 + 9 * 5
    tracked = {id(b) for k, b in m.named_buffers() if k.endswith("num_batches_tracked")}
    assert {id(t) for t in src} == ({id(p) for p in m.parameters()} | {id(b) for b in m.buffers()}) - tracked


def test_synthetic_weights_leave_nothing_at_its_initial_value():
    """With default initialisation a dropped or swapped BatchNorm changes nothing."""
    m = module_cpu()
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            assert float(mod.running_mean.abs().min()) > 0 and float((mod.running_var - 1).abs().min()) > 0, name
            assert float((mod.weight - 1).abs().min()) > 0 and float(mod.bias.abs().min()) > 0, name
            assert 0.5 < float(mod.running_var.min()) and float(mod.running_var.max()) < 1.5, name
        elif isinstance(mod, torch.nn.PReLU):
            w = mod.weight
            assert 0.25 <= float(w.min()) and float(w.max()) <= 0.75 and len(set(w.tolist())) == w.numel(), name


# ---- the recording ------------------------------------------------------------------------------------------------------------------
def test_cpu_path_reproduces_the_recording_bit_for_bit():
    gold = load_golden("aligner")
    n, seed = GOLDEN_CASE
    t32 = cpu_results(n, seed)[1]
    assert torch.equal(t32["out"], t32["dfea3"])
    with torch.no_grad():
        assert torch.equal(module_cpu()(aligner_input(n, seed)), t32["out"])         # forward() is that composition
    shapes = dict(zip(alignment.TAPS, alignment.TAP_SHAPES), out=(3, 256))
    for key in TENSORS:
        t = t32[key]
        c, s = shapes[key]
        assert t.dtype == torch.float32 and tuple(t.shape) == (n, c, s, s), key
        flat = t.reshape(-1)
        assert np.array_equal(flat[samples(flat.numel())].numpy(), gold[f"{key}_f32"]), key
        assert float(t.double().sum()) == float(gold[f"{key}_f32_sum"]), key


def test_other_sizes_raise_as_the_reference_does():
    m = module_cpu()
    for size in (64, 40):
        with pytest.raises(RuntimeError), torch.no_grad():
            m(aligner_input(1, 3, size))


# ---- dispatch -----------------------------------------------------------------------------------------------------------------------
class _Fake:
    """What _runs_hip looks at of an input, without a GPU."""

    def __init__(self, shape=(2, 6, 256, 256), device="cuda:0", dtype=torch.float32, requires_grad=False):
        self.shape, self.device, self.dtype, self.requires_grad, self.ndim = torch.Size(shape), torch.device(device), dtype, requires_grad, len(shape)


def test_dispatch_rules(monkeypatch):
    m = ResidualAligner(syn.aligner_opt()).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    monkeypatch.setattr(torch, "is_tensor", lambda t: True)          # (_Fake stands in for a GPU tensor)
    monkeypatch.delenv("E3DGE_ALIGNER", raising=False)
    assert m._runs_hip(_Fake()) and m._runs_hip(_Fake(shape=(1, 6, 256, 256)))
    assert not m._runs_hip(_Fake(device="cpu")) and not m._runs_hip(_Fake(dtype=torch.float64)) and not m._runs_hip(_Fake(dtype=torch.float16))
    for shape in [(2, 6, 64, 64), (2, 6, 40, 40), (2, 6, 256, 128), (2, 3, 256, 256), (2, 7, 256, 256), (6, 256, 256), (0, 6, 256, 256), (300, 6, 256, 256)]:
        assert not m._runs_hip(_Fake(shape=shape)), shape
    m.train()
    assert not m._runs_hip(_Fake())
    m.eval()
    assert not m._runs_hip(_Fake(requires_grad=True))
    with torch.no_grad():
        assert m._runs_hip(_Fake(requires_grad=True))
    m.conv_layer1[2].weight.requires_grad_(True)
    assert not m._runs_hip(_Fake())
    with torch.no_grad():
        assert m._runs_hip(_Fake())
    m.conv_layer1[2].weight.requires_grad_(False)
    monkeypatch.setenv("E3DGE_ALIGNER", "torch")
    assert not m._runs_hip(_Fake())
    monkeypatch.delenv("E3DGE_ALIGNER")
    assert m._runs_hip(_Fake())
    # the two-tensor form of align()
    res = _Fake(shape=(2, 3, 256, 256))
    assert m._runs_hip(res, _Fake(shape=(2, 3, 64, 64))) and m._runs_hip(res, _Fake(shape=(2, 3, 256, 256)))
    for thumb in [_Fake(shape=(2, 3, 128, 128)), _Fake(shape=(1, 3, 64, 64)), _Fake(shape=(2, 4, 64, 64)), _Fake(shape=(2, 3, 64, 64), device="cuda:1"),
                  _Fake(shape=(2, 3, 64, 64), dtype=torch.float16), _Fake(shape=(2, 3, 64, 64), requires_grad=True)]:
        assert not m._runs_hip(res, thumb), thumb.shape
    assert not m._runs_hip(_Fake(shape=(2, 3, 64, 64)), _Fake(shape=(2, 3, 64, 64)))
    for over in [dict(aligner_norm_type='instance'), dict(aligner_norm_type='none'), dict(aligner_demodulate=True)]:
        with torch.device("meta"):
            other = ResidualAligner(syn.aligner_opt(**over)).eval()
        assert not other.native_options() and not other._runs_hip(_Fake()), over


def test_paths_on_the_cpu_take_the_torch_layers(monkeypatch):
    called = []
    monkeypatch.setattr(_lib, "launch", lambda name, *a: called.append(name))
    m = module_cpu()
    n, seed = GOLDEN_CASE
    x = aligner_input(n, seed)
    assert not m._runs_hip(x)
    with torch.no_grad():
        assert torch.equal(m(x), cpu_results(n, seed)[1]["out"])
    assert not called


@pytest.mark.parametrize("over", [dict(aligner_norm_type='instance'), dict(aligner_norm_type='none'), dict(aligner_demodulate=True)], ids=str)
def test_the_other_options_run_the_torch_layers(over):
    m = module_cpu(**over)
    assert not any(isinstance(q, torch.nn.BatchNorm2d) for q in m.modules())
    assert any(isinstance(q, alignment.DemodulatedConv2d) for q in m.modules()) == bool(over.get("aligner_demodulate"))
    with torch.no_grad():
        y = m(aligner_input(1, 4))
    assert tuple(y.shape) == (1, 3, 256, 256) and bool(torch.isfinite(y).all()) and float(y.std()) > 0


def test_align_equals_the_composed_call_bit_for_bit():
    m = module_cpu()
    x = aligner_input(1, 5)
    res_gt = x[:, :3].contiguous()
    for thumb in (x[:, 3:, ::4, ::4].contiguous(), x[:, 3:].contiguous()):
        with torch.no_grad():
            want = m(torch.cat((res_gt, F.interpolate(thumb, (256, 256))), dim=1))
            got = m.align(res_gt, thumb)
        assert torch.equal(got, want) and float(got.std()) > 0


# ---- bilinear x2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [3, 16])
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (32, 32), (64, 64)], ids=str)
def test_up2_restatement_equals_interpolate_bit_for_bit(hw, channels):
    """(64, 64) is past the size where ATen changes the order of its roundings: the separable form, which is the kernel's."""
    rs = np.random.RandomState(hw[0] * 10 + channels)
    x = torch.from_numpy(rs.standard_normal((2, channels) + hw).astype(np.float32))
    want = F.interpolate(x, size=(2 * hw[0], 2 * hw[1]), mode='bilinear')
    assert torch.equal(alignment.up2_bilinear(x), want)
    assert torch.equal(F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False), want)


# ---- size entries ---------------------------------------------------------------------------------------------------------------------
def _up(v, m):
    return (v + m - 1) // m * m


def packed_floats():
    """The layout of e3dge_aligner_pack restated: every block on a multiple of 64 floats; a convolution is roundup(cout, 16) rows of
    roundup(cin ks^2, 32) floats, a BatchNorm 2 per channel, a PReLU 1 per channel."""
    conv = lambda ci, co, ks: _up(_up(co, 16) * _up(ci * ks * ks, 32), 64)
    total = conv(6, 16, 3) + _up(2 * 16, 64) + _up(16, 64)
    for units in alignment.STAGES.values():
        for ci, d, _ in units:
            total += _up(2 * ci, 64) + conv(ci, d, 3) + _up(d, 64) + conv(d, d, 3) + _up(2 * d, 64)
            if ci != d:
                total += conv(ci, d, 1) + _up(2 * d, 64)
    return total


def workspace_bytes(n):
    """feat1..4, dfea1..2, the widest first convolution of a unit (32 channels at 256^2), the 1x1 branch, two unit outputs and an
    up-sampled map (16 channels at 256^2 each)."""
    P = 256 * 256
    per_image = [16 * P, 32 * P // 4, 48 * P // 16, 64 * P // 64, 32 * P // 16, 16 * P // 4, 32 * P, 16 * P, 16 * P, 16 * P, 16 * P]
    return 4 * sum(_up(n * f, 64) for f in per_image)


def test_size_entries_equal_their_restatement(lib):
    assert lib.e3dge_aligner_packed_floats() == packed_floats()
    assert packed_floats() >= sum(p.numel() for p in module_cpu().parameters())
    for n in (1, 2, 5, 256):
        assert lib.e3dge_aligner_workspace_bytes(n) == workspace_bytes(n), n


# ---- refusals before any launch -------------------------------------------------------------------------------------------------------
def _last(lib):
    return lib.e3dge_last_error().decode()


def test_entries_refuse_bad_arguments_before_a_launch(lib):
    """Null and misshapen arguments on a machine without a GPU: a launch would fail with a launch error, a refusal is INVALID_ARG."""
    P, S = 0x1000, None                                              # a non-null address that is never dereferenced on the host
    bad = -1
    adr = ctypes.addressof
    for n in (0, -1, 257):
        assert lib.e3dge_aligner_workspace_bytes(n) == -1 and "n=" in _last(lib), n
    total = lib.e3dge_aligner_packed_floats()
    n_src = _lib.ALIGNER_SOURCES
    src = (ctypes.c_void_p * n_src)(*([P] * n_src))
    hole = (ctypes.c_void_p * n_src)(*([P] * (n_src - 1) + [None]))
    assert lib.e3dge_aligner_pack(None, total, adr(src), n_src, S) == bad and "null" in _last(lib)
    assert lib.e3dge_aligner_pack(P, total, None, n_src, S) == bad and "null" in _last(lib)
    assert lib.e3dge_aligner_pack(P, total - 1, adr(src), n_src, S) == bad and "packed" in _last(lib)
    assert lib.e3dge_aligner_pack(P, total, adr(src), n_src - 1, S) == bad and "n_src" in _last(lib)
    assert lib.e3dge_aligner_pack(P, total, adr(hole), n_src, S) == bad and "null" in _last(lib)
    ws = lib.e3dge_aligner_workspace_bytes(1)

    def fwd(**over):
        f = dict(packed=P, packed_floats=total, res_gt=P, thumb=P, n=1, size=256, split=3, thumb_up4=1, out=P, ws=P, ws_bytes=ws)
        f.update(over)
        return _lib.AlignerArgs(**f)
    assert lib.e3dge_aligner_forward(None, S) == bad
    for over, word in [(dict(packed=None), "null"), (dict(res_gt=None), "null"), (dict(thumb=None), "null"), (dict(out=None), "null"), (dict(ws=None), "null"),
                       (dict(split=6, res_gt=None), "null"), (dict(split=0, thumb=None), "null"), (dict(n=0), "n="), (dict(n=-2), "n="), (dict(n=300), "n="),
                       (dict(size=64), "size"), (dict(size=40), "size"), (dict(size=512), "size"), (dict(split=-1), "split"), (dict(split=7), "split"),
                       (dict(thumb_up4=2), "thumb_up4"), (dict(packed_floats=total - 1), "packed"), (dict(ws_bytes=ws - 1), "workspace"),
                       (dict(n=2), "workspace")]:
        assert lib.e3dge_aligner_forward(ctypes.byref(fwd(**over)), S) == bad and word in _last(lib), (over, _last(lib))
    keys = ("out", "in0", "in1", "w", "in_ab", "epi_ab", "slope", "shortcut", "wfrag", "floats", "n", "cin", "split", "up4", "cout", "h", "wd", "ks", "stride", "mode")
    base = dict(out=P, in0=P, in1=P, w=P, in_ab=P, epi_ab=P, slope=P, shortcut=P, wfrag=P, floats=16 * 96, n=2, cin=8, split=5, up4=0, cout=16, h=8, wd=8,
                ks=3, stride=1, mode=0)
    conv = lambda **o: lib.e3dge_aln_conv(*[{**base, **o}[k] for k in keys], S)
    for over in [dict(out=None), dict(w=None), dict(wfrag=None), dict(in0=None), dict(in1=None), dict(n=0), dict(n=257), dict(cin=0), dict(cout=0), dict(cout=65),
                 dict(cout=128), dict(split=-1), dict(split=9), dict(h=0), dict(wd=1025), dict(ks=2), dict(ks=5), dict(stride=0), dict(stride=3), dict(up4=2),
                 dict(up4=1, h=6), dict(mode=3), dict(mode=-1), dict(mode=1, shortcut=None), dict(mode=2, shortcut=None), dict(floats=16 * 96 - 1)]:
        assert conv(**over) == bad, over
    assert conv(cout=65) == bad and "cout" in _last(lib)
    assert conv(split=9) == bad and "split" in _last(lib)
    assert conv(floats=100) == bad and "wfrag" in _last(lib)
    up = lambda **o: lib.e3dge_aln_up2(*[{**dict(out=P, inp=P, planes=4, h=3, wd=5), **o}[k] for k in ("out", "inp", "planes", "h", "wd")], S)
    for over in [dict(out=None), dict(inp=None), dict(planes=0), dict(h=0), dict(wd=0), dict(h=1025)]:
        assert up(**over) == bad, over
