"""CPU: the hourglass image filter (e3dge_amd.hg_filter) -- its state-dict keys and its torch composition against the recording of the
reference's HGFilter / ResidualBlock (tools/gen_golden_hgfilter.py, bit for bit), the refusals of the e3dge_hgf_* entries, the opt-in
wiring into SirenLocalGlobal, and the conditions without which a dead network would pass every parity test, on the float64 truth.

Inputs are a formula (golden_input); the weights are synthetic.load_synthetic_hgfilter's.  tests/test_gpu_hgfilter.py shares the cases."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, synthetic as syn
from e3dge_amd.hg_filter import HGFilter, ResidualImageFilter

# name: (options over the defaults, batch, height, width, through filter() from an image and a depth map)
CASES = {
    "default": (dict(), 2, 64, 96, False),
    "deep": (dict(num_stack=2, num_hourglass=3), 1, 64, 64, False),
    "filter": (dict(), 2, 64, 96, True),
}
N_SAMPLES = 256


def golden_input(shape, seed):
    """Smooth structure plus noise, different per image and channel, O(1)."""
    rs = np.random.RandomState(7000 + seed)
    n, c, h, w = shape
    yy, xx = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing='ij')
    phase = rs.uniform(0, 2 * np.pi, size=(n, c, 1, 1))
    freq = rs.uniform(1, 6, size=(n, c, 1, 1))
    v = np.sin(freq * xx[None, None] + phase) * np.cos(0.5 * freq * yy[None, None] - phase) + 0.5 * rs.standard_normal(shape)
    return torch.from_numpy(v.astype(np.float32))


def samples(numel):
    """N_SAMPLES flat positions of a tensor of numel elements."""
    return (np.arange(N_SAMPLES, dtype=np.int64) * 2654435761 + 12345) % numel


def case_inputs(name):
    _, n, h, w, through_filter = CASES[name]
    seed = sorted(CASES).index(name)
    if through_filter:
        return golden_input((n, 3, h, w), seed), golden_input((n, 1, h, w), 50 + seed)
    return (golden_input((n, 64, h, w), seed),)


def tensor_names(name):
    return [f"out{i}" for i in range(syn.pifu_opt(**CASES[name][0]).num_stack)] + ["tmpx", "normx"]


@functools.lru_cache(maxsize=None)
def module_cpu(name, dtype=torch.float32):
    """The ResidualImageFilter of the case with the synthetic weights, on the CPU; shared, never modified."""
    m = syn.load_synthetic_hgfilter(ResidualImageFilter(syn.pifu_opt(**CASES[name][0]))).to(dtype).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def run_case(module, name, inputs, probe=None):
    """dict of the case's tensors from the torch composition (CPU) or whichever path the module takes (GPU)."""
    with torch.no_grad():
        if CASES[name][4]:
            outs, tmpx, normx = module.filter_maps(*inputs)
        elif probe is not None:
            outs, tmpx, normx = module.image_filter.forward_torch(inputs[0], probe)
        else:
            outs, tmpx, normx = module.image_filter(inputs[0])
    return dict(zip(tensor_names(name), list(outs) + [tmpx, normx]))


@functools.lru_cache(maxsize=None)
def cpu_results(name):
    """(float64 truth, float32 torch composition, alive statistics of the float64 run) of a case; computed once, never modified."""
    m64, relu_in, hooks, probe = module_cpu(name, torch.float64), [], [], []
    norms = [(k, q) for k, q in m64.named_modules() if isinstance(q, (torch.nn.GroupNorm, torch.nn.InstanceNorm2d))]
    for k, q in norms:                                                # every norm's output is a ReLU's input
        hooks.append(q.register_forward_hook(lambda mod, inp, out, k=k: relu_in.append((k, float((out > 0).double().mean())))))
    inputs = tuple(t.double() for t in case_inputs(name))
    t64 = run_case(m64, name, inputs, None if CASES[name][4] else probe)
    for h in hooks:
        h.remove()
    t32 = run_case(module_cpu(name), name, case_inputs(name))
    levels = [(s, lv, float(u1.abs().max()), float(u2.abs().max())) for s, lv, u1, u2 in probe]
    return t64, t32, dict(relu_in=relu_in, levels=levels)


def parity_bound(t64, t32, factor=3):
    """The project's standing bound per tensor (tests/test_gpu_idloss.py): max(2e-6 max|f64|, factor max|f32 - f64|)."""
    return max(2e-6 * float(t64.abs().max()), factor * float((t32.double() - t64).abs().max()))


# ---- keys -------------------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_equal_the_recording():
    recorded = json.load(open(os.path.join(GOLDEN, "hgfilter_state_dict_keys.json")))
    ours = list(module_cpu("default").state_dict())                  # whole: the reference's netLocal loads with strict=True
    assert sorted(ours) == sorted(recorded)
    assert sum(k.startswith("image_filter.") for k in ours) == 431
    sd = module_cpu("default").state_dict()
    assert "image_filter.conv2.bn4.weight" in sd and "image_filter.conv2.downsample.0.weight" in sd          # one parameter, two keys
    assert sd["image_filter.conv2.bn4.weight"].data_ptr() == sd["image_filter.conv2.downsample.0.weight"].data_ptr()
    assert "image_filter.conv3.bn4.weight" in sd and "image_filter.conv3.downsample.0.weight" not in sd
    assert sorted(k for k in sd if k.startswith("downsample_channel_conv.")) == ["downsample_channel_conv." + k for k in
                                                                                 ("bn.bias", "bn.weight", "conv.bias", "conv.weight")]
    assert tuple(sd["downsample_channel_conv.conv.weight"].shape) == (64, 512, 3, 3)


def test_sources_are_every_used_parameter_once():
    for name in ("default", "deep"):
        hg = module_cpu(name).image_filter
        S, D = hg.num_modules, hg.num_hourglass
        # the stem's 4, conv2 to conv4's 12 + 9 + 12, per stack 9 in each of the 3 D + 2 ConvBlocks and 6, 4 more for all but the last
        assert len(hg.sources()) == 37 + S * ((3 * D + 2) * 9 + 6) + (S - 1) * 4
        assert len({id(t) for t in hg.sources()}) == len(hg.sources())
        used = {id(p) for p in hg.parameters()} - {id(b.bn4.weight) for b in hg.modules() if hasattr(b, "bn4") and b.downsample is None} \
            - {id(b.bn4.bias) for b in hg.modules() if hasattr(b, "bn4") and b.downsample is None}
        assert {id(t) for t in hg.sources()} == used


# ---- the recording ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_cpu_path_reproduces_the_recording_bit_for_bit(name):
    gold = load_golden("hgfilter")
    _, t32, _ = cpu_results(name)
    for key, t in t32.items():
        assert t.dtype == torch.float32 and t.is_contiguous(), key
        flat = t.reshape(-1)
        assert np.array_equal(flat[samples(flat.numel())].numpy(), gold[f"{name}_{key}"]), (name, key)
        assert float(t.double().sum()) == float(gold[f"{name}_{key}_sum"]), (name, key)
    if name == "default":
        last = tensor_names(name)[-3]
        assert np.array_equal(t32[last][0].numpy(), gold["default_last_image0"])


def test_filter_surface_on_the_cpu():
    m = ResidualImageFilter(syn.pifu_opt())
    m.load_state_dict(module_cpu("filter").state_dict())
    image, depth = case_inputs("filter")
    with torch.no_grad():
        assert m.filter(image, depth) is None
        got = m.filter(image, depth, feat_key='que_view', return_feat=True)
    t32 = cpu_results("filter")[1]
    assert isinstance(got, list) and len(got) == 1 and torch.equal(got[0], t32["out3"])
    assert set(m.im_feat_dict) == {'ref_view', 'que_view'} and torch.equal(m.im_feat_dict['ref_view'][0], t32["out3"])
    assert torch.equal(m.tmpx, t32["tmpx"]) and torch.equal(m.normx, t32["normx"]) and not m.tmpx.requires_grad
    with pytest.raises(DeprecationWarning):
        m.filter(image, depth, ref_feats=torch.zeros(2, 512, 64, 96))
    outs, tmpx, normx = m.image_filter(torch.zeros(1, 64, 32, 32))
    assert [tuple(o.shape) for o in outs] == [(1, 256, 8, 8)] * 4 and tmpx.shape == (1, 64, 16, 16) and normx.shape == (1, 128, 8, 8)


# ---- a dead network would pass every parity test ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_float64_truth_is_alive(name):
    t64, t32, stats = cpu_results(name)
    o = syn.pifu_opt(**CASES[name][0])
    # the stem's, conv2 to conv4's 4 + 3 + 4, per stack 3 in each of the 3 D + 2 ConvBlocks and bn_end's; 2 in each front net
    assert len(stats['relu_in']) == 12 + o.num_stack * (9 * o.num_hourglass + 7) + (4 if CASES[name][4] else 0)
    dead = [(k, f) for k, f in stats['relu_in'] if not 0.10 <= f <= 0.90]
    assert not dead, dead
    outs = tensor_names(name)[:-2]
    for k in outs:
        assert float(t64[k].std()) >= 0.3, (k, float(t64[k].std()))
    for ka, kb in zip(outs, outs[1:]):                                # a stack that only copied its predecessor would pass parity
        assert float((t64[ka] - t64[kb]).abs().max()) > parity_bound(t64[kb], t32[kb]), (ka, kb)
    if not CASES[name][4]:
        assert len(stats['levels']) == len(outs) * syn.pifu_opt(**CASES[name][0]).num_hourglass
        weak = [lv for lv in stats['levels'] if lv[3] < 0.1 * lv[2]]
        assert not weak, weak


# ---- refusals before any launch ---------------------------------------------------------------------------------------------------------
def _last(lib):
    return lib.e3dge_last_error().decode()


def test_entries_refuse_bad_arguments_before_a_launch(lib):
    """Null and misshapen arguments on a machine without a GPU: a launch would fail with a launch error, a refusal is INVALID_ARG."""
    P, S = 0x1000, None                                              # a non-null address that is never dereferenced on the host
    bad = -1
    assert lib.e3dge_hgf_packed_floats(0, 2) == -1 and lib.e3dge_hgf_packed_floats(4, 5) == -1 and lib.e3dge_hgf_packed_floats(9, 2) == -1
    assert lib.e3dge_hgf_packed_floats(4, 2) > 0
    assert lib.e3dge_hgf_ws_bytes(1, 64, 64, 4, 2) > 0
    for args in [(0, 64, 64, 4, 2), (1, 60, 64, 4, 2), (1, 64, 72, 4, 2), (1, 48, 32, 2, 3), (1, 64, 64, 0, 2), (1, 8192, 64, 4, 2), (4097, 64, 64, 4, 2)]:
        assert lib.e3dge_hgf_ws_bytes(*args) == -1, args
    n_src = len(module_cpu("default").image_filter.sources())
    src = (ctypes.c_void_p * n_src)(*([P] * n_src))
    hole = (ctypes.c_void_p * n_src)(*([P] * (n_src - 1) + [None]))
    front_hole = (ctypes.c_void_p * _lib.HGF_FRONT_SRC)(*([P] * 15 + [None]))
    adr = ctypes.addressof
    assert lib.e3dge_hgf_pack_weights(None, adr(src), n_src, None, 4, 2, S) == bad and "null" in _last(lib)
    assert lib.e3dge_hgf_pack_weights(P, None, n_src, None, 4, 2, S) == bad
    assert lib.e3dge_hgf_pack_weights(P, adr(src), n_src - 1, None, 4, 2, S) == bad and "n_filter_src" in _last(lib)
    assert lib.e3dge_hgf_pack_weights(P, adr(hole), n_src, None, 4, 2, S) == bad and "null" in _last(lib)
    assert lib.e3dge_hgf_pack_weights(P, adr(src), n_src, adr(front_hole), 4, 2, S) == bad and "front" in _last(lib)
    assert lib.e3dge_hgf_pack_weights(P, adr(src), n_src, None, 4, 7, S) == bad
    ws = lib.e3dge_hgf_ws_bytes(1, 64, 64, 4, 2)

    def fwd(**over):
        f = dict(packed=P, input=P, n=1, height=64, width=64, num_stack=4, num_hourglass=2, tmpx=P, normx=P, ws=P, ws_bytes=ws)
        f.update(over)
        a = _lib.HgfArgs(**f)
        for i in range(4):
            a.outputs[i] = P
        return a
    assert lib.e3dge_hgf_forward(None, S) == bad
    for over, word in [(dict(packed=None), "null"), (dict(input=None), "null"), (dict(tmpx=None), "null"), (dict(normx=None), "null"),
                       (dict(ws=None), "null"), (dict(n=0), "n="), (dict(height=60), "height"), (dict(width=40), "width"), (dict(num_stack=9), "num_stack"),
                       (dict(num_hourglass=0), "num_hourglass"), (dict(num_hourglass=3, height=80), "height"), (dict(ws_bytes=ws - 1), "workspace")]:
        assert lib.e3dge_hgf_forward(ctypes.byref(fwd(**over)), S) == bad and word in _last(lib), (over, _last(lib))
    a = fwd()
    a.outputs[3] = None
    assert lib.e3dge_hgf_forward(ctypes.byref(a), S) == bad and "output 3" in _last(lib)
    front = lambda **o: lib.e3dge_hgf_front(*[{**dict(packed=P, image=P, depth=P, out=P, n=1, h=64, w=64, s=4, d=2, ws=P, ws_bytes=ws), **o}[k]
                                              for k in ("packed", "image", "depth", "out", "n", "h", "w", "s", "d", "ws", "ws_bytes")], S)
    for over in [dict(packed=None), dict(image=None), dict(depth=None), dict(out=None), dict(ws=None), dict(n=0), dict(h=72), dict(w=0), dict(s=0), dict(d=9),
                 dict(ws_bytes=3 * 32 * 64 * 64 * 4)]:                   # its three 32-channel planes alone need that much
        assert front(**over) == bad, over
    conv = lambda **o: lib.e3dge_hgf_conv(*[{**dict(out=P, raw=None, inp=P, w=P, wfrag=P, in_ab=None, bias=None, res=None, n=1, cin=8, cout=32, h=8, wd=8, ks=3,
                                                   st=1, reflect=0, oc=32, o0=0, rc=0, r0=0), **o}[k]
                                          for k in ("out", "raw", "inp", "w", "wfrag", "in_ab", "bias", "res", "n", "cin", "cout", "h", "wd", "ks", "st", "reflect",
                                                    "oc", "o0", "rc", "r0")], S)
    for over in [dict(out=None), dict(inp=None), dict(w=None), dict(wfrag=None), dict(n=0), dict(cin=0), dict(cout=24), dict(cout=0), dict(h=0), dict(wd=5000),
                 dict(ks=5), dict(ks=7, st=1), dict(ks=3, st=2), dict(ks=1, reflect=1), dict(reflect=1, h=1), dict(oc=16), dict(o0=8), dict(o0=-1),
                 dict(res=P, rc=16), dict(res=P, rc=32, r0=1)]:
        assert conv(**over) == bad, over
    norm = lambda **o: lib.e3dge_hgf_norm(*[{**dict(ab=P, x=P, g=P, b=P, n=1, ct=64, c0=0, c=64, groups=32, h=4, w=4), **o}[k]
                                          for k in ("ab", "x", "g", "b", "n", "ct", "c0", "c", "groups", "h", "w")], S)
    for over in [dict(ab=None), dict(x=None), dict(g=None), dict(b=None), dict(n=0), dict(c=0), dict(c0=1), dict(groups=0), dict(groups=48), dict(h=0),
                 dict(c=1024, ct=1024, groups=2)]:
        assert norm(**over) == bad, over
    for args in [(None, P, 1, 4, 4), (P, None, 1, 4, 4), (P, P, 0, 4, 4), (P, P, 1, 3, 4), (P, P, 1, 4, 0), (P, P, 1, 4, 8192)]:
        assert lib.e3dge_hgf_pool(*args, S) == bad, args
    for args in [(None, P, P, 1, 4, 4), (P, None, P, 1, 4, 4), (P, P, None, 1, 4, 4), (P, P, P, 0, 4, 4), (P, P, P, 1, 0, 4), (P, P, P, 1, 4, 4096)]:
        assert lib.e3dge_hgf_up_add(*args, S) == bad, args


# ---- wiring -----------------------------------------------------------------------------------------------------------------------------
def test_local_options_none_leaves_siren_local_global_unchanged():
    from e3dge_amd.volume_renderer import LocalTexHead, SirenLocalGlobal
    opt = syn.rendering_opt(L_pred_tex_modulations=True)
    plain = SirenLocalGlobal(opt=opt)
    assert type(plain.netLocal) is LocalTexHead and not hasattr(plain.netLocal, "filter")
    keys = list(plain.state_dict())
    assert all(k.startswith(("netGlobal.", "netLocal.local_feat_to_tex_modulations_linear.")) for k in keys)
    wired = SirenLocalGlobal(opt=opt, local_options=syn.pifu_opt())
    extra = [k for k in wired.state_dict() if k not in keys]
    assert [k for k in wired.state_dict() if k in keys] == keys
    assert extra and all(k.startswith(tuple("netLocal." + p for p in syn.HGFILTER_PARTS)) for k in extra)
    assert sum(k.startswith("netLocal.image_filter.") for k in extra) == 431
    assert callable(wired.netLocal.filter) and callable(wired.netLocal.tex_modulations_from_maps)
    assert SirenLocalGlobal(opt=syn.rendering_opt(), local_options=syn.pifu_opt()).netLocal is None


def test_paths_on_the_cpu_take_the_torch_composition(monkeypatch):
    called = []
    monkeypatch.setattr(_lib, "launch", lambda name, *a: called.append(name))
    m = module_cpu("deep")
    assert not m.image_filter._runs_hip(torch.zeros(1, 64, 64, 64)) and not m._runs_hip(torch.zeros(1, 3, 64, 64), torch.zeros(1, 1, 64, 64))
    with torch.no_grad():
        m.image_filter(torch.zeros(1, 64, 32, 32))
    assert not called
