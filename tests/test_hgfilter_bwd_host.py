"""CPU: the backward of the hourglass image filter (csrc/hgfilter_bwd.h) -- the refusals of its entries before any launch, the
routing of `differentiable` on a machine without a GPU, and the conditions without which a dead backward would pass the parity tests
of tests/test_gpu_hgfilter_bwd.py, on the float64 truth of its two cases."""
import ctypes

import numpy as np
import pytest
import torch

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, synthetic as syn
from e3dge_amd.hg_filter import HGFilter, ResidualImageFilter
from conftest import load_golden
from test_gpu_hgfilter_bwd import BWD_CASES, bwd_inputs, bwd_module, grad_samples, input_names, pinned_run, used_parameters


def _last(lib):
    return lib.e3dge_last_error().decode()


def test_backward_entries_refuse_bad_arguments_before_a_launch(lib):
    P, S, bad = 0x1000, None, -1                                     # a non-null address that is never dereferenced on the host
    ok = (1, 64, 64, 4, 2)
    for q in (lib.e3dge_hgf_saved_bytes, lib.e3dge_hgf_bwd_ws_bytes, lib.e3dge_hgf_branch_bytes):
        assert q(*ok) > 0
        for args in [(0, 64, 64, 4, 2), (1, 60, 64, 4, 2), (1, 64, 72, 4, 2), (1, 48, 32, 2, 3), (1, 64, 64, 0, 2), (1, 8192, 64, 4, 2), (4097, 64, 64, 4, 2)]:
            assert q(*args) == -1, args
    # the saved state holds at least every ConvBlock's two intermediate tensors: more than the forward's workspace
    assert lib.e3dge_hgf_saved_bytes(*ok) > lib.e3dge_hgf_ws_bytes(*ok)
    assert lib.e3dge_hgf_saved_bytes(2, 64, 64, 4, 2) > 1.9 * lib.e3dge_hgf_saved_bytes(*ok)
    assert lib.e3dge_hgf_packed_t_floats(0, 2) == -1 and lib.e3dge_hgf_packed_t_floats(4, 5) == -1 and lib.e3dge_hgf_packed_t_floats(4, 2) > 0
    n_src = len(ResidualImageFilter(syn.pifu_opt()).image_filter.sources())
    src = (ctypes.c_void_p * n_src)(*([P] * n_src))
    hole = (ctypes.c_void_p * n_src)(*([P] * (n_src - 1) + [None]))
    front_hole = (ctypes.c_void_p * _lib.HGF_FRONT_SRC)(*([P] * 15 + [None]))
    adr = ctypes.addressof
    pack = lib.e3dge_hgf_pack_weights_t
    assert pack(None, adr(src), n_src, None, 4, 2, S) == bad and "null" in _last(lib)
    assert pack(P, None, n_src, None, 4, 2, S) == bad
    assert pack(P, adr(src), n_src - 1, None, 4, 2, S) == bad and "n_filter_src" in _last(lib)
    assert pack(P, adr(hole), n_src, None, 4, 2, S) == bad and "null" in _last(lib)
    assert pack(P, adr(src), n_src, adr(front_hole), 4, 2, S) == bad and "front" in _last(lib)
    assert pack(P, adr(src), n_src, None, 4, 7, S) == bad
    ws, saved, bws, br = (q(*ok) for q in (lib.e3dge_hgf_ws_bytes, lib.e3dge_hgf_saved_bytes, lib.e3dge_hgf_bwd_ws_bytes, lib.e3dge_hgf_branch_bytes))

    def fwd(**over):
        f = dict(packed=P, input=P, n=1, height=64, width=64, num_stack=4, num_hourglass=2, tmpx=P, normx=P, ws=P, ws_bytes=ws)
        f.update(over)
        a = _lib.HgfArgs(**f)
        for i in range(4):
            a.outputs[i] = P
        return a
    assert lib.e3dge_hgf_forward_saving(ctypes.byref(fwd()), None, saved, S) == bad and "null" in _last(lib)
    assert lib.e3dge_hgf_forward_saving(None, P, saved, S) == bad
    assert lib.e3dge_hgf_forward_saving(ctypes.byref(fwd()), P, saved - 1, S) == bad and "saved state" in _last(lib)
    for over, word in [(dict(packed=None), "null"), (dict(n=0), "n="), (dict(height=60), "height"), (dict(num_stack=9), "num_stack"),
                       (dict(ws_bytes=ws - 1), "workspace")]:
        assert lib.e3dge_hgf_forward_saving(ctypes.byref(fwd(**over)), P, saved, S) == bad and word in _last(lib), (over, _last(lib))
    front = lambda **o: lib.e3dge_hgf_front_saving(*[{**dict(packed=P, image=P, depth=P, out=P, n=1, h=64, w=64, s=4, d=2, ws=P, ws_bytes=ws, saved=P,
                                                            saved_bytes=saved), **o}[k]
                                                     for k in ("packed", "image", "depth", "out", "n", "h", "w", "s", "d", "ws", "ws_bytes", "saved", "saved_bytes")], S)
    for over in [dict(packed=None), dict(image=None), dict(depth=None), dict(out=None), dict(ws=None), dict(saved=None), dict(n=0), dict(h=72), dict(w=0),
                 dict(s=0), dict(d=9), dict(ws_bytes=3 * 32 * 64 * 64 * 4), dict(saved_bytes=saved - 1)]:
        assert front(**over) == bad, over

    def bwd(**over):
        f = dict(packed=P, packed_t=P, saved=P, saved_bytes=saved, tmpx=P, normx=P, n=1, height=64, width=64, num_stack=4, num_hourglass=2, g_normx=P,
                 g_input=P, ws=P, ws_bytes=bws)
        f.update(over)
        a = _lib.HgfBwdArgs(**f)
        a.g_outputs[3] = P
        return a
    assert lib.e3dge_hgf_backward(None, S) == bad
    for over, word in [(dict(packed=None), "null"), (dict(packed_t=None), "null"), (dict(saved=None), "null"), (dict(tmpx=None), "null"),
                       (dict(normx=None), "null"), (dict(g_input=None), "null"), (dict(ws=None), "null"), (dict(n=0), "n="), (dict(height=60), "height"),
                       (dict(width=40), "width"), (dict(num_stack=9), "num_stack"), (dict(num_hourglass=0), "num_hourglass"),
                       (dict(ws_bytes=bws - 1), "workspace"), (dict(saved_bytes=saved - 1), "saved state"), (dict(branch=P, branch_bytes=16), "branch")]:
        assert lib.e3dge_hgf_backward(ctypes.byref(bwd(**over)), S) == bad and word in _last(lib), (over, _last(lib))
    a = bwd(g_normx=None)
    a.g_outputs[3] = None
    assert lib.e3dge_hgf_backward(ctypes.byref(a), S) == bad and "no upstream gradient" in _last(lib)
    fb = lambda **o: lib.e3dge_hgf_front_backward(*[{**dict(packed=P, packed_t=P, saved=P, saved_bytes=saved, g=P, gi=P, gd=P, n=1, h=64, w=64, s=4, d=2, ws=P,
                                                           ws_bytes=bws, branch=None, branch_bytes=0, grads=None, image=None, depth=None), **o}[k]
                                                    for k in ("packed", "packed_t", "saved", "saved_bytes", "g", "gi", "gd", "n", "h", "w", "s", "d", "ws", "ws_bytes",
                                                              "branch", "branch_bytes", "grads", "image", "depth")], S)
    for over in [dict(packed=None), dict(packed_t=None), dict(saved=None), dict(g=None), dict(gi=None, gd=None), dict(ws=None), dict(n=0), dict(h=72), dict(w=0),
                 dict(s=0), dict(d=9), dict(ws_bytes=3 * 32 * 64 * 64 * 4), dict(saved_bytes=saved - 1), dict(branch=P, branch_bytes=br - 1), dict(grads=P), dict(grads=P, image=P)]:
        assert fb(**over) == bad, over
    assert lib.e3dge_hgf_grad_floats(0, 2) == -1 and lib.e3dge_hgf_grad_floats(4, 5) == -1
    m = ResidualImageFilter(syn.pifu_opt())                          # one gradient per source, in the sources' own shapes
    front_numel = sum(p.numel() for net in (m.residual_conv, m.depth_conv) for p in net.parameters())
    assert lib.e3dge_hgf_grad_floats(4, 2) == sum(t.numel() for t in m.image_filter.sources()) + front_numel
    a = bwd(grads=P)                                                 # the parameter gradients need the forward's input and outputs
    assert lib.e3dge_hgf_backward(ctypes.byref(a), S) == bad and "input" in _last(lib)
    a = bwd(grads=P, input=P)
    assert lib.e3dge_hgf_backward(ctypes.byref(a), S) == bad and "output 0" in _last(lib)
    wg = lambda **o: lib.e3dge_hgf_conv_wgrad(*[{**dict(dw=P, db=None, g=P, x=P, ab=None, n=1, cin=8, cout=32, h=8, wd=8, ks=3, st=1, reflect=0, gc=32, g0=0, ws=P,
                                                       wsf=lib.e3dge_hgf_wgrad_ws_floats(1, 8, 32, 8, 8, 3, 1)), **o}[k]
                                                for k in ("dw", "db", "g", "x", "ab", "n", "cin", "cout", "h", "wd", "ks", "st", "reflect", "gc", "g0", "ws", "wsf")], S)
    assert lib.e3dge_hgf_wgrad_ws_floats(1, 8, 32, 8, 8, 3, 1) > 0 and lib.e3dge_hgf_wgrad_ws_floats(1, 8, 24, 8, 8, 3, 1) == -1
    for over in [dict(dw=None), dict(g=None), dict(x=None), dict(ws=None), dict(n=0), dict(cin=0), dict(cout=24), dict(h=0), dict(wd=5000), dict(ks=5),
                 dict(ks=7, st=1), dict(ks=1, reflect=1), dict(reflect=1, h=1), dict(gc=16), dict(g0=8), dict(db=P, gc=64), dict(wsf=100)]:
        assert wg(**over) == bad, over
    dg = lambda **o: lib.e3dge_hgf_conv_dgrad(*[{**dict(out=P, g=P, w=P, wt=P, x=None, ab=None, add=None, n=1, cin=8, cout=32, h=8, wd=8, ks=3, st=1, reflect=0,
                                                       gc=32, g0=0), **o}[k]
                                                for k in ("out", "g", "w", "wt", "x", "ab", "add", "n", "cin", "cout", "h", "wd", "ks", "st", "reflect", "gc", "g0")], S)
    for over in [dict(out=None), dict(g=None), dict(w=None), dict(wt=None), dict(x=P), dict(ab=P), dict(n=0), dict(cin=0), dict(cout=24), dict(h=0), dict(wd=5000),
                 dict(ks=5), dict(ks=7, st=1), dict(ks=3, st=2), dict(ks=1, reflect=1), dict(reflect=1, h=1), dict(gc=16), dict(g0=8), dict(g0=-1)]:
        assert dg(**over) == bad, over
    nb = lambda **o: lib.e3dge_hgf_norm_bwd(*[{**dict(gx=P, gy=P, x=P, gamma=P, mask=None, add0=None, a0c=0, a00=0, add1=None, coef=P, dg=None, db=None, n=1, ct=64, c0=0,
                                                     c=64, groups=32, h=4, w=4), **o}[k]
                                              for k in ("gx", "gy", "x", "gamma", "mask", "add0", "a0c", "a00", "add1", "coef", "dg", "db", "n", "ct", "c0", "c", "groups",
                                                        "h", "w")], S)
    for over in [dict(gx=None), dict(gy=None), dict(x=None), dict(gamma=None), dict(coef=None), dict(n=0), dict(c=0), dict(c0=1), dict(groups=0), dict(groups=48),
                 dict(h=0), dict(c=1024, ct=1024, groups=2), dict(add0=P, a0c=32), dict(add0=P, a0c=64, a00=1), dict(dg=P), dict(db=P)]:
        assert nb(**over) == bad, over
    for args in [(None, P, None, 1, 4, 4), (P, None, None, 1, 4, 4), (P, P, None, 0, 4, 4), (P, P, None, 1, 3, 4), (P, P, None, 1, 4, 0), (P, P, None, 1, 4, 8192)]:
        assert lib.e3dge_hgf_pool_bwd(*args, S) == bad, args
    for args in [(None, P, 1, 4, 4), (P, None, 1, 4, 4), (P, P, 0, 4, 4), (P, P, 1, 0, 4), (P, P, 1, 4, 4096)]:
        assert lib.e3dge_hgf_up_bwd(*args, S) == bad, args


def test_differentiable_on_the_cpu_takes_the_torch_composition(monkeypatch):
    called = []
    monkeypatch.setattr(_lib, "launch", lambda name, *a: called.append(name))
    m = ResidualImageFilter(syn.pifu_opt(num_stack=1, num_hourglass=1), differentiable=True)
    for p in m.parameters():
        p.requires_grad_(False)
    assert m.differentiable and m.image_filter.differentiable
    image, depth = torch.zeros(1, 3, 16, 16, requires_grad=True), torch.zeros(1, 1, 16, 16)
    assert not m._runs_hip_grad(image, depth) and not m.image_filter._runs_hip_grad(torch.zeros(1, 64, 16, 16, requires_grad=True))
    outs, _, _ = m.filter_maps(image, depth)
    outs[-1].sum().backward()
    assert not called and image.grad is not None
    assert not HGFilter(syn.pifu_opt()).differentiable and not ResidualImageFilter(syn.pifu_opt()).differentiable


# ---- the recording ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BWD_CASES))
def test_cpu_autograd_reproduces_the_recording_bit_for_bit(name):
    """The module's torch composition under float32 autograd against the reference's own autograd (tools/gen_golden_hgfilter_grads.py): the
    same ATen backward kernels in the same order, so every sampled value and every float64 sum is equal bit for bit."""
    gold = load_golden("hgfilter_grads")
    inputs, ups = bwd_inputs(name)
    m = bwd_module(name)
    grads, _ = pinned_run(m, name, list(inputs), ups, None)
    keys = input_names(name) + [k for k, _ in used_parameters(m, name)]
    assert len(grads) == len(keys) and sum(k.startswith(name + "__") for k in gold.keys()) == 2 * len(keys)
    for key, g in zip(keys, grads):
        flat = g.reshape(-1)
        assert g.dtype == torch.float32
        assert np.array_equal(flat[grad_samples(flat.numel(), key in input_names(name))].numpy(), gold[f"{name}__{key}"]), (name, key)
        assert float(g.double().sum()) == float(gold[f"{name}__{key}__sum"]), (name, key)


# ---- a dead backward would pass every parity test ---------------------------------------------------------------------------------------
# floors: a tenth of what the float64 truth gives (case A: image 3.46, depth 6.25; case B: input 0.362), stated here so that a change
# of the synthetic weights that kills the gradient is seen
STD_FLOOR = {"A": (0.35, 0.62), "B": (0.036,)}


@pytest.mark.parametrize("name", sorted(BWD_CASES))
def test_the_float64_gradient_is_alive(name):
    inputs, ups = bwd_inputs(name)
    m64 = bwd_module(name, torch.float64)
    grads, _ = pinned_run(m64, name, [t.double() for t in inputs], ups, None)
    params, grads = grads[len(inputs):], grads[:len(inputs)]
    print(name, [float(g.std()) for g in grads])
    assert len(params) == len(used_parameters(m64, name)) and all(g is not None and float(g.abs().max()) > 0 for g in params)
    if name == "A":                                                  # the three routes into `previous`: through the second hourglass, `+ previous`, bl / al
        by_key = {k: g for (k, _), g in zip(used_parameters(m64, name), params)}
        for key in ("image_filter.m1.b1_2.conv1.weight", "image_filter.bl0.weight", "image_filter.al0.weight", "image_filter.conv4.conv1.weight"):
            assert float(by_key[key].abs().max()) > 5e-5 * max(float(g.abs().max()) for g in params), key
    for g, floor in zip(grads, STD_FLOOR[name]):
        assert bool(torch.isfinite(g).all()) and float(g.std()) > floor, (name, float(g.std()))
    # every route carries a gradient: each upstream tensor alone reaches the inputs
    for i, g in enumerate(ups):
        if g is None:
            continue
        alone, _ = pinned_run(m64, name, [t.double() for t in inputs], [u if j == i else None for j, u in enumerate(ups)], None)
        assert all(float(a.abs().max()) > 5e-5 * float(t.abs().max()) for a, t in zip(alone, grads)), (name, i)      # (zip: the inputs' only)
    # in every hourglass level the gradient arriving through the up-sampled branch is at least 0.1 of the one through up1
    hg, probe = m64.image_filter, []
    x = (inputs[0].double() if not BWD_CASES[name][4] else
         torch.cat((m64.residual_conv(inputs[0].double()), m64.depth_conv(inputs[1].double())), 1)).detach().requires_grad_(True)
    level_in, hooks = {}, []
    for i in range(hg.num_modules):
        for d in range(1, hg.num_hourglass + 1):
            hooks.append(hg._modules[f'm{i}']._modules[f'b1_{d}'].register_forward_pre_hook(lambda mod, inp, key=(i, d): level_in.__setitem__(key, inp[0])))
    outs, _, _ = hg.forward_torch(x, probe)
    for h in hooks:
        h.remove()
    for _, _, up1, up2 in probe:
        up1.retain_grad()
        up2.retain_grad()
    torch.autograd.backward(list(outs), [g.double() for g in ups[:len(outs)]], retain_graph=True)
    assert len(probe) == hg.num_modules * hg.num_hourglass == len(level_in)
    for i, d, up1, up2 in probe:
        through_up1, = torch.autograd.grad(up1, level_in[(i, d)], up1.grad, retain_graph=True)
        through_up2, = torch.autograd.grad(up2, level_in[(i, d)], up2.grad, retain_graph=True)
        ratio = float(through_up2.abs().max()) / float(through_up1.abs().max())
        print(name, i, d, ratio)
        assert ratio >= 0.1, (name, i, d, ratio)
    assert float(x.grad.abs().max()) > 0
