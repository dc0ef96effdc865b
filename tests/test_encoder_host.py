"""CPU: the E0 image encoder (e3dge_amd.encoders) -- its state-dict keys and its torch composition against the recording of the
reference's HybridGradualStyleEncoder_V2 (tools/gen_golden_encoder.py, bit for bit), the gt_pool path, the dispatch rules, the refusals
of the e3dge_enc_* entries and image2latents against hand-written offsets.

Inputs are a formula (encoder_input); the weights are synthetic.load_synthetic_encoder's.  tests/test_gpu_encoder.py shares the helpers."""
import copy
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
from e3dge_amd import encoders
from e3dge_amd.encoders import HybridGradualStyleEncoder_V2, image2latents

N_SAMPLES = 256
TENSORS = ("thumb_out", "stylegan_out", "feat_maps", "p32")
GOLDEN_CASE = (2, 256, 0)                                            # batch, size, input seed of encoder.npz
# whole-network cases of the GPU test: options over encoder_opt(single_decoder_layer=True), batch, size
CASES = {
    "s64": (dict(), 2, 64),
    "s48": (dict(), 1, 48),
    "tex64": (dict(fpn_pigan_tex_layer_dim=64), 2, 64),
    "nodec": (dict(disable_decoder_fpn=True), 2, 64),
}


def encoder_input(n, size, seed):
    """Smooth structure plus noise, different per image and channel, O(1)."""
    rs = np.random.RandomState(9000 + seed)
    shape = (n, 3, size, size)
    yy, xx = np.meshgrid(np.linspace(-1, 1, size), np.linspace(-1, 1, size), indexing='ij')
    phase = rs.uniform(0, 2 * np.pi, size=(n, 3, 1, 1))
    freq = rs.uniform(1, 6, size=(n, 3, 1, 1))
    v = np.sin(freq * xx[None, None] + phase) * np.cos(0.5 * freq * yy[None, None] - phase) + 0.5 * rs.standard_normal(shape)
    return torch.from_numpy(v.astype(np.float32))


def samples(numel):
    """N_SAMPLES flat positions of a tensor of numel elements."""
    return (np.arange(N_SAMPLES, dtype=np.int64) * 2654435761 + 12345) % numel


def options(**over):
    return syn.encoder_opt(single_decoder_layer=True, **over)


@functools.lru_cache(maxsize=None)
def _module_cpu(over, dtype):
    if dtype != torch.float32:
        return copy.deepcopy(_module_cpu(over, torch.float32)).to(dtype)
    with torch.device("meta"):                                       # no initialiser runs: every entry of the state dict is loaded below
        m = HybridGradualStyleEncoder_V2(50, 'ir_se', 9, options(**dict(over)))
    m = syn.load_synthetic_encoder(m.to_empty(device="cpu")).to(dtype).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def module_cpu(dtype=torch.float32, **over):
    """The encoder with the synthetic weights on the CPU; shared, never modified."""
    return _module_cpu(tuple(sorted(over.items())), dtype)


def as_tensors(out):
    """dict of the returned tensors by the names of TENSORS (absent ones left out) from either of forward()'s structures."""
    if isinstance(out, dict):
        return dict(thumb_out=out['pred_latents'][0], stylegan_out=out['pred_latents'][1], feat_maps=out['feat_maps'], p32=out['p32'])
    return {k: t for k, t in zip(("thumb_out", "stylegan_out"), out) if t is not None}


@functools.lru_cache(maxsize=None)
def cpu_results(name):
    """(float64 truth, float32 torch composition) of a case of CASES; computed once, never modified."""
    over, n, size = CASES[name]
    x = encoder_input(n, size, sorted(CASES).index(name) + 1)
    with torch.no_grad():
        t64 = as_tensors(module_cpu(torch.float64, **over).run(x.double(), return_featmap=True, pool=False))
        t32 = as_tensors(module_cpu(**over).run(x, return_featmap=True, pool=False))
    return t64, t32


def parity_bound(t64, t32, factor=3):
    """The project's standing bound per tensor (tests/test_gpu_idloss.py): max(2e-6 max|f64|, factor max|f32 - f64|)."""
    return max(2e-6 * float(t64.abs().max()), factor * float((t32.double() - t64).abs().max()))


# ---- keys -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("single, count", [(False, 709), (True, 551)])
def test_state_dict_keys_equal_the_recording(single, count):
    recorded = json.load(open(os.path.join(GOLDEN, "encoder_state_dict_keys.json")))["single" if single else "scripts"]
    with torch.device("meta"):                                       # 258.6 M parameters are never initialised
        m = HybridGradualStyleEncoder_V2(50, 'ir_se', 9, syn.encoder_opt(single_decoder_layer=single))
    ours = list(m.state_dict())
    assert sorted(ours) == recorded and len(ours) == count
    if not single:
        n_par = sum(p.numel() for p in m.parameters())
        unread = sum(p.numel() for i in range(1, 10) for p in m.styles_stylegan[i].parameters())
        assert n_par == 258588352 and unread == 167550464            # 258.6 M, of which styles_stylegan.1-9 are 167.6 M
        assert not {id(t) for t in m.sources()} & {id(p) for i in range(1, 10) for p in m.styles_stylegan[i].parameters()}


def test_sources_are_every_read_parameter_once():
    m = module_cpu()
    src = m.sources()
    assert len({id(t) for t in src}) == len(src) == 6 + 24 * 13 + 3 * 5 + 6 + 10 * 16
    tracked = {id(b) for k, b in m.named_buffers() if k.endswith("num_batches_tracked")}
    assert {id(t) for t in src} == ({id(p) for p in m.parameters()} | {id(b) for b in m.buffers()}) - tracked
    assert len(module_cpu(disable_decoder_fpn=True).sources()) == len(src) - 16
    assert len(module_cpu(fpn_pigan_tex_layer_dim=64).sources()) == len(src) - 3 * 2


# ---- the recording ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden_forward():
    """The fp32 CPU forward of the recorded case; computed once, never modified."""
    n, size, seed = GOLDEN_CASE
    with torch.no_grad():
        return module_cpu()(encoder_input(n, size, seed), return_featmap=True)


def test_cpu_path_reproduces_the_recording_bit_for_bit():
    gold = load_golden("encoder")
    n, size, seed = GOLDEN_CASE
    out = golden_forward()
    assert isinstance(out, dict) and sorted(out) == ['feat_maps', 'p32', 'pred_latents']
    t32 = as_tensors(out)
    assert tuple(t32["thumb_out"].shape) == (n, 9, 256) and tuple(t32["stylegan_out"].shape) == (n, 10, 512)
    assert tuple(t32["feat_maps"].shape) == (n, 512, 64, 64) and tuple(t32["p32"].shape) == (n, 512, 32, 32)
    for key in TENSORS:
        t = t32[key]
        assert t.dtype == torch.float32
        flat = t.reshape(-1)
        assert np.array_equal(flat[samples(flat.numel())].numpy(), gold[f"{key}_f32"]), key
        assert float(t.double().sum()) == float(gold[f"{key}_f32_sum"]), key
    assert torch.equal(t32["stylegan_out"][:, 0], t32["stylegan_out"][:, 9])          # head 0 repeated to ten styles


def test_a_larger_input_is_pooled_to_256_first():
    m = module_cpu()
    x = encoder_input(1, 512, 5)
    calls = []
    hook = m.input_layer.register_forward_hook(lambda mod, inp, out: calls.append(inp[0]))
    try:
        with torch.no_grad():
            got = m(x)
            want = m.run(torch.nn.functional.adaptive_avg_pool2d(x, (256, 256)), pool=False)
    finally:
        hook.remove()
    assert tuple(calls[0].shape) == (1, 3, 256, 256) and torch.equal(calls[0], calls[1])
    assert isinstance(got, list) and len(got) == 2
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert isinstance(m.gt_pool, encoders.AvgPool2d) and m.gt_pool.output_size == (256, 256)


def test_without_the_decoder_head_the_second_latent_is_none():
    m = module_cpu(disable_decoder_fpn=True)
    assert not hasattr(m, "styles_stylegan") and not m.enable_decoder
    with torch.no_grad():
        out = m.run(encoder_input(1, 32, 6), return_featmap=True, pool=False)
    assert isinstance(out, list) and out[1] is None and tuple(out[0].shape) == (1, 9, 256)
    assert not HybridGradualStyleEncoder_V2(50, 'ir_se', 9, options(full_pipeline=False)).enable_decoder


# ---- dispatch -----------------------------------------------------------------------------------------------------------------------
class _Fake:
    """What _runs_hip looks at of an input, without a GPU."""

    def __init__(self, shape=(2, 3, 64, 64), device="cuda", dtype=torch.float32, requires_grad=False):
        self.shape, self.device, self.dtype, self.requires_grad, self.ndim = torch.Size(shape), torch.device(device), dtype, requires_grad, len(shape)


def test_dispatch_rules(monkeypatch):
    m = HybridGradualStyleEncoder_V2(50, 'ir_se', 9, options(disable_decoder_fpn=True, fpn_pigan_geo_layer_dim=32, fpn_pigan_tex_layer_dim=32)).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    others = {}
    with torch.device("meta"):
        for over in [dict(input_nc=1), dict(fpn_pigan_geo_layer_dim=16), dict(fpn_pigan_tex_layer_dim=256)]:
            others[str(over)] = HybridGradualStyleEncoder_V2(50, 'ir_se', 9, options(disable_decoder_fpn=True, **over)).eval()
        others["ir"] = HybridGradualStyleEncoder_V2(50, 'ir', 9, options(disable_decoder_fpn=True)).eval()
        others["100"] = HybridGradualStyleEncoder_V2(100, 'ir_se', 9, options(disable_decoder_fpn=True)).eval()
    monkeypatch.setattr(torch, "is_tensor", lambda t: True)          # (_Fake stands in for a GPU tensor)
    monkeypatch.delenv("E3DGE_ENCODER", raising=False)
    assert m._runs_hip(_Fake())
    assert not m._runs_hip(_Fake(device="cpu")) and not m._runs_hip(_Fake(dtype=torch.float64)) and not m._runs_hip(_Fake(dtype=torch.float16))
    for shape in [(2, 3, 40, 40), (2, 3, 16, 16), (2, 3, 512, 512), (2, 3, 64, 48), (2, 1, 64, 64), (3, 64, 64)]:
        assert not m._runs_hip(_Fake(shape=shape)), shape
    assert m._runs_hip(_Fake(shape=(1, 3, 32, 32))) and m._runs_hip(_Fake(shape=(4, 3, 256, 256))) and m._runs_hip(_Fake(shape=(1, 3, 48, 48)))
    m.train()
    assert not m._runs_hip(_Fake())
    m.eval()
    assert not m._runs_hip(_Fake(requires_grad=True))
    with torch.no_grad():
        assert m._runs_hip(_Fake(requires_grad=True))
    m.latlayer64.bias.requires_grad_(True)
    assert not m._runs_hip(_Fake())
    with torch.no_grad():
        assert m._runs_hip(_Fake())
    m.latlayer64.bias.requires_grad_(False)
    monkeypatch.setenv("E3DGE_ENCODER", "torch")
    assert not m._runs_hip(_Fake())
    monkeypatch.delenv("E3DGE_ENCODER")
    for name, other in others.items():
        assert not other.native_options() and not other._runs_hip(_Fake()), name


def test_paths_on_the_cpu_take_the_torch_composition(monkeypatch):
    called = []
    monkeypatch.setattr(_lib, "launch", lambda name, *a: called.append(name))
    m = module_cpu()
    x = encoder_input(1, 32, 7)
    assert not m._runs_hip(x)
    with torch.no_grad():
        m.run(x, pool=False)
    assert not called


# ---- refusals before any launch -------------------------------------------------------------------------------------------------------
def _last(lib):
    return lib.e3dge_last_error().decode()


def test_entries_refuse_bad_arguments_before_a_launch(lib):
    """Null and misshapen arguments on a machine without a GPU: a launch would fail with a launch error, a refusal is INVALID_ARG."""
    P, S = 0x1000, None                                              # a non-null address that is never dereferenced on the host
    bad = -1
    assert lib.e3dge_enc_packed_floats(256, 128, 128, 1) > lib.e3dge_enc_packed_floats(256, 128, 128, 0) > 0
    assert lib.e3dge_enc_packed_floats(64, 128, 128, 1) != lib.e3dge_enc_packed_floats(256, 128, 128, 1)       # live taps only: the image follows the size
    for args in [(16, 128, 128, 1), (40, 128, 128, 1), (512, 128, 128, 1), (256, 16, 128, 1), (256, 128, 256, 1), (256, 128, 100, 0), (256, 128, 128, 2)]:
        assert lib.e3dge_enc_packed_floats(*args) == -1, args
    assert lib.e3dge_enc_ws_bytes(1, 64, 128, 128, 1) > lib.e3dge_enc_ws_bytes(1, 64, 128, 128, 0) > 0       # no p128 without the decoder head
    for args in [(0, 64, 128, 128, 1), (257, 64, 128, 128, 1), (1, 72, 128, 128, 1), (1, 64, 8, 128, 1), (1, 64, 128, 128, -1)]:
        assert lib.e3dge_enc_ws_bytes(*args) == -1, args
    n_src = len(module_cpu().sources())
    src = (ctypes.c_void_p * n_src)(*([P] * n_src))
    hole = (ctypes.c_void_p * n_src)(*([P] * (n_src - 1) + [None]))
    adr = ctypes.addressof
    assert lib.e3dge_enc_pack_weights(None, adr(src), n_src, 64, 128, 128, 1, S) == bad and "null" in _last(lib)
    assert lib.e3dge_enc_pack_weights(P, None, n_src, 64, 128, 128, 1, S) == bad and "null" in _last(lib)
    assert lib.e3dge_enc_pack_weights(P, adr(src), n_src - 1, 64, 128, 128, 1, S) == bad and "n_src" in _last(lib)
    assert lib.e3dge_enc_pack_weights(P, adr(src), n_src, 64, 128, 128, 0, S) == bad and "n_src" in _last(lib)
    assert lib.e3dge_enc_pack_weights(P, adr(hole), n_src, 64, 128, 128, 1, S) == bad and "null" in _last(lib)
    assert lib.e3dge_enc_pack_weights(P, adr(src), n_src, 60, 128, 128, 1, S) == bad and "size" in _last(lib)
    ws = lib.e3dge_enc_ws_bytes(1, 64, 128, 128, 1)

    def fwd(**over):
        f = dict(packed=P, images=P, n=1, size=64, geo_dim=128, tex_dim=128, enable_decoder=1, thumb_out=P, stylegan_out=P, p32=P, p64=P, ws=P, ws_bytes=ws)
        f.update(over)
        return _lib.EncArgs(**f)
    assert lib.e3dge_enc_forward(None, S) == bad
    for over, word in [(dict(packed=None), "null"), (dict(images=None), "null"), (dict(thumb_out=None), "null"), (dict(stylegan_out=None), "null"),
                       (dict(p32=None), "null"), (dict(p64=None), "null"), (dict(ws=None), "null"), (dict(n=0), "n="), (dict(n=300), "n="),
                       (dict(size=24), "size"), (dict(size=272), "size"), (dict(size=100), "size"), (dict(geo_dim=48), "geo_dim"), (dict(tex_dim=0), "tex_dim"),
                       (dict(enable_decoder=3), "enable_decoder"), (dict(ws_bytes=ws - 1), "workspace"), (dict(n=2), "workspace")]:
        assert lib.e3dge_enc_forward(ctypes.byref(fwd(**over)), S) == bad and word in _last(lib), (over, _last(lib))
    lat = lambda **o: lib.e3dge_enc_lateral(*[{**dict(out=P, coarse=P, inp=P, w=P, bias=P, wfrag=P, n=1, cin=64, cout=512, ch=4, cw=4, h=8, wd=8), **o}[k]
                                              for k in ("out", "coarse", "inp", "w", "bias", "wfrag", "n", "cin", "cout", "ch", "cw", "h", "wd")], S)
    for over in [dict(out=None), dict(coarse=None), dict(inp=None), dict(w=None), dict(bias=None), dict(wfrag=None), dict(n=0), dict(cin=0), dict(cout=48),
                 dict(cout=0), dict(ch=0), dict(cw=9), dict(h=0), dict(wd=2000), dict(ch=16)]:
        assert lat(**over) == bad, over
    conv = lambda **o: lib.e3dge_enc_head_conv(*[{**dict(out=P, inp=P, w=P, bias=P, wfrag=P, n=1, heads=3, shared=1, cin=512, cout=256, h=8, wd=8), **o}[k]
                                                 for k in ("out", "inp", "w", "bias", "wfrag", "n", "heads", "shared", "cin", "cout", "h", "wd")], S)
    for over in [dict(out=None), dict(inp=None), dict(w=None), dict(bias=None), dict(wfrag=None), dict(n=0), dict(heads=0), dict(heads=17), dict(shared=2),
                 dict(cin=0), dict(cout=100), dict(h=0), dict(wd=1025)]:
        assert conv(**over) == bad, over
    need = 3 * 256 * (256 * (4 + 4) + 4 + 1 + 2 * 2)
    tail = lambda **o: lib.e3dge_enc_head_tail(*[{**dict(out=P, inp=P, cw=P, cb=P, lw=P, lb=P, scratch=P, floats=need, n=2, heads=3, c=256, start=2, convs=4), **o}[k]
                                                 for k in ("out", "inp", "cw", "cb", "lw", "lb", "scratch", "floats", "n", "heads", "c", "start", "convs")], S)
    for over in [dict(out=None), dict(inp=None), dict(cw=None), dict(cb=None), dict(lw=None), dict(lb=None), dict(scratch=None), dict(floats=1000), dict(n=0),
                 dict(heads=0), dict(c=96), dict(start=3), dict(start=0), dict(convs=0), dict(convs=9), dict(start=1, convs=-1)]:
        assert tail(**over) == bad, over
    assert tail(floats=need // 2) == bad and "scratch" in _last(lib)
    assert 3 * 256 * (256 * (4 + 4) + 4 + 1 + 2 * 2) == need          # the size include/e3dge_hip.h promises is enough


# ---- image2latents --------------------------------------------------------------------------------------------------------------------
def test_image2latents_adds_the_mean_latents():
    m = module_cpu()
    n, size, seed = GOLDEN_CASE
    x = encoder_input(n, size, seed)
    rs = np.random.RandomState(3)
    mean = [torch.from_numpy(rs.standard_normal((1, 9, 256)).astype(np.float32)), torch.from_numpy(rs.standard_normal((1, 10, 512)).astype(np.float32))]
    plain = golden_forward()
    with torch.no_grad():
        got = image2latents(m, x, mean, return_featmap=True)
    assert isinstance(got, dict)
    for i in range(2):
        want = torch.empty_like(plain['pred_latents'][i])
        for b in range(n):
            want[b] = mean[i][0] + plain['pred_latents'][i][b]
        assert torch.equal(got['pred_latents'][i], want)
    assert torch.equal(got['feat_maps'], plain['feat_maps']) and torch.equal(got['p32'], plain['p32'])
    nodec = module_cpu(disable_decoder_fpn=True)
    small = encoder_input(1, 32, 6)
    big = small.repeat_interleave(16, -1).repeat_interleave(16, -2)            # 512^2: pool_256 averages equal 2 x 2 blocks
    with torch.no_grad():
        out = image2latents(nodec, big, [mean[0][0], None])
        base = nodec(small.repeat_interleave(8, -1).repeat_interleave(8, -2))
    assert isinstance(out, list) and out[1] is None and torch.equal(out[0], mean[0] + base[0])
