"""GPU: the decoder's FIR buffers -- asymmetric ones, and ones that differ per level -- against float64.

Every Blur and Upsample of a Decoder is built from [1, 3, 3, 1] and so equals its own 180-degree flip: a dropped flip or a transposed tap
index in a kernel that reads those buffers changes nothing the other decoder tests look at.  Here the buffers are overwritten (on a copy
of the shared decoder of tests/test_gpu_decoder_bwd_shapes.py; the copy is never handed back) with the asymmetric 4x4 FIR of
tests/test_fir_host.py, times 4 as both modules scale theirs:

  planar path      an asymmetric Blur kernel in every up-sampling layer and an asymmetric (different) Upsample kernel in every ToRGB:
                   _dec2_ok is False (the packed up-sampling kernel applies the blur as two symmetric 1-D passes), and every layer of the
                   layer-by-layer forward -- e3dge_blur_noise_bias_act, e3dge_torgb with their own buffers -- is compared ONE LAYER DEEP with
                   oracle/decoder_ref.decoder_stage in float64 on the layer's own input, by the bound of tests/test_gpu_decoder_fwd_shapes.py
                   (3 chain + 1e-6, chain the float32 oracle stage's distance; store = 0: the activations are fp32), the image at 1e-4.
  packed path      the symmetric Blur kept, the asymmetric FIR in every ToRGB's Upsample (the same at every level): the packed forward's
                   skip images (pk_torgb_kernel and, case d, both fused ToRGB forms: the rgb_fir reads of csrc/decoder2.hip) against the
                   forced float64 stage with E3DGE_DEC2_FUSE_RGB on and off, and the packed backward's feature gradient
                   (pk_drgb_down_kernel, the adjoint of that up-sampler) against decoder_pinned_backward in float64 with the bounds of the
                   backward file (1e-4 per sample, the float32 chain within 1e-5).
  per-level        the Blur or the Upsample kernel of level 1 differs from level 0's: the packed plan hands level 0's taps to every level,
                   so such a decoder has to take the planar path, which applies each layer's own: not _dec2_ok, no plan built, and the
                   image against the float64 chain with the per-level kernels."""
import copy

import pytest
import torch

from conftest import record
from oracle import decoder_ref

import e3dge_amd  # noqa: F401
from e3dge_amd import stylesdf_model as sm

from test_fir_host import asym_fir
from test_gpu_decoder_bwd_shapes import DEV, FIT_TOL, GRAD_TOL, IMG_ATOL, _per_sample, _setup
from test_gpu_decoder_fwd_shapes import STORE_PACKED, _Log, _conv_stage, _rgb_stage, _run

ENV = ("E3DGE_DEC2_FUSE_RGB", "E3DGE_DEC2_FUSE_RGB_MID", "E3DGE_DEC2_S1", "E3DGE_DEC2_UPBLUR_SHAPE")


def _fresh_decoder(s):
    """A private copy of the case's decoder on the GPU (the shared one is never modified), frozen, with no cached plan."""
    dec = copy.deepcopy(s["g"].decoder).to(DEV).eval().requires_grad_(False)
    assert sm._DEC2_STATES.get(dec) is None
    return dec


def _write(buf, k):
    with torch.no_grad():
        buf.copy_(k.to(buf.device, buf.dtype))


def _firs(dec):
    """(per-level Blur kernels, per-level Upsample kernels) as the modules hold them (fp32), on the CPU in float64."""
    n = len(dec.to_rgbs)
    return ([dec.convs[2 * u].conv.blur.kernel.detach().cpu().double() for u in range(n)],
            [dec.to_rgbs[u].upsample.kernel.detach().cpu().double() for u in range(n)])


def _inputs(s):
    return s["feats"].to(DEV), s["wd"].to(DEV), [n.to(DEV) for n in s["noises"]]


def _planar_stages(dec, s):
    """One forward of the layer path under no_grad with a hook on every layer: (image, [(input activation, output)] in the order of
    decoder_ref.decoder_stages), on the CPU."""
    feats, wd, noises = _inputs(s)
    layers = [dec.conv1, dec.to_rgb1]
    for u in range(len(dec.to_rgbs)):
        layers += [dec.convs[2 * u], dec.convs[2 * u + 1], dec.to_rgbs[u]]
    seen = {}
    hooks = [m.register_forward_hook(lambda mod, args, out, j=j: seen.__setitem__(j, (args[0].detach().cpu(), out.detach().cpu())))
             for j, m in enumerate(layers)]
    try:
        with torch.no_grad():
            img, _ = dec(feats, [wd], input_is_latent=True, noise=noises)
    finally:
        for h in hooks:
            h.remove()
    assert sorted(seen) == list(range(len(layers)))
    return img.cpu(), [seen[j] for j in range(len(layers))]


def _compare_planar(log, s, stages_io, blur_firs, up_firs, tag):
    """Every layer of a planar forward against the float64 stage on the layer's own input (and the previous skip image)."""
    stages = decoder_ref.decoder_stages(s["sd"])
    assert len(stages) == len(stages_io)
    skip, n_conv = None, 0
    for st, (x, out) in zip(stages, stages_io):
        kind, p, row, upsample = st
        if kind == "conv":
            other = s["noises"][n_conv]
            level = (n_conv - 1) // 2
            fir = blur_firs[level] if upsample else None
            n_conv += 1
        else:
            other = skip
            fir = up_firs[(n_conv - 2) // 2] if upsample else None
        t64, y32 = (decoder_ref.decoder_stage(s["sd"], st, x, s["wd"][:, row], other, dtype=dt, fir=fir) for dt in (torch.float64, torch.float32))
        log.add(f"{tag}.{p[8:-1]}", out, t64, y32, 0.0)
        if kind == "rgb":
            skip = out


@pytest.mark.gpu
def test_planar_path_with_asymmetric_blur_and_upsample_kernels(monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    s = _setup("c")
    dec = _fresh_decoder(s)
    feats, wd, noises = _inputs(s)
    assert dec._dec2_ok(feats, wd, noises, None)                      # as built: the packed pipeline
    k_blur, k_up = asym_fir(4.0), asym_fir(4.0).t().contiguous()
    for u in range(len(dec.to_rgbs)):
        _write(dec.convs[2 * u].conv.blur.kernel, k_blur)
        _write(dec.to_rgbs[u].upsample.kernel, k_up)
    assert not dec._dec2_ok(feats, wd, noises, None)
    img, io = _planar_stages(dec, s)
    assert sm._DEC2_STATES.get(dec) is None
    blur_firs, up_firs = _firs(dec)
    log = _Log()
    _compare_planar(log, s, io, blur_firs, up_firs, "planar_asym")
    t64, t32 = (decoder_ref.decoder_forward(s["sd"], s["feats"], s["wd"], noises=s["noises"], dtype=dt, blur_firs=blur_firs, up_firs=up_firs)
                for dt in (torch.float64, torch.float32))
    e, c = float((img.double() - t64).abs().max()), float((t32.double() - t64).abs().max())
    moved = float((t64 - s["own64"]["img"]).abs().max())             # what the asymmetric kernels change in the truth
    log.record("dec_fir_planar_asym", img=e, chain_img=c, truth_moved_by=moved)
    assert len(log.rows) == 3 * s["n_up"] + 2
    assert moved > 1000 * IMG_ATOL and e <= IMG_ATOL, (e, c, moved)
    log.check()


def _compare_packed(log, s, run, up_fir, tag):
    """Every stored activation and every skip image of a packed run against its forced float64 stage, the ToRGB stages with `up_fir`."""
    stages = decoder_ref.decoder_stages(s["sd"])
    acts, skips = run["acts"], run["skips"]
    for k in range(1, len(acts)):
        if acts[k] is None or acts[k - 1] is None:
            continue
        st = _conv_stage(stages, k)
        t64, y32 = (decoder_ref.decoder_stage(s["sd"], st, acts[k - 1], s["wd"][:, st[2]], s["noises"][k - 1], dtype=dt) for dt in (torch.float64, torch.float32))
        log.add(f"{tag}.act{k}", acts[k], t64, y32, STORE_PACKED)
    n = 0
    for j in range(len(skips)):
        x = acts[1 + 2 * j]
        if x is None:
            continue
        st = _rgb_stage(stages, j)
        t64, y32 = (decoder_ref.decoder_stage(s["sd"], st, x, s["wd"][:, st[2]], skips[j - 1] if j else None, dtype=dt, fir=up_fir if j else None)
                    for dt in (torch.float64, torch.float32))
        log.add(f"{tag}.rgb{j}" + (".fused" if j and run["fused"][j - 1] else ""), skips[j], t64, y32, 0.0)
        n += 1
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["c", "d"])
def test_packed_path_with_an_asymmetric_upsample_kernel(cid, monkeypatch):
    """Case c: the smallest decoder (stand-alone pk_torgb_kernel at both levels); case d: 64 and 32 channels at the last two levels, where
    the stride-1 convolution carries the fused ToRGB (both forms), and with E3DGE_DEC2_FUSE_RGB=0 the stand-alone kernel everywhere."""
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    s = _setup(cid)
    dec = _fresh_decoder(s)
    k_up = asym_fir(4.0)
    for tr in dec.to_rgbs:
        _write(tr.upsample.kernel, k_up)
    up_fir = _firs(dec)[1][0]
    feats, wd, noises = _inputs(s)
    assert dec._dec2_ok(feats, wd, noises, None)                      # one kernel at every level, symmetric blur: the packed pipeline
    runs = {"save": _run(dec, s, save=True), "nosave": _run(dec, s)}
    monkeypatch.setenv("E3DGE_DEC2_FUSE_RGB", "0")
    runs["nofuse"] = _run(dec, s, env={"E3DGE_DEC2_FUSE_RGB": "0"})
    monkeypatch.delenv("E3DGE_DEC2_FUSE_RGB")
    assert not any(runs["nofuse"]["fused"]) and runs["save"]["fused"] == ([False, True, True] if cid == "d" else [False, False])
    log, rgbs = _Log(), 0
    for tag, run in runs.items():
        rgbs += _compare_packed(log, s, run, up_fir, tag)
    n_up = [up_fir] * s["n_up"]
    t64, t32 = (decoder_ref.decoder_forward(s["sd"], s["feats"], s["wd"], noises=s["noises"], dtype=dt, up_firs=n_up) for dt in (torch.float64, torch.float32))
    imgs = {tag: float((run["skips"][-1].double() - t64).abs().max()) for tag, run in runs.items()}
    moved = float((t64 - s["own64"]["img"]).abs().max())
    # the backward: d features through pk_drgb_down_kernel, branches pinned to the packed forward's own
    f = feats.clone().requires_grad_(True)
    img, _ = dec(f, [wd], input_is_latent=True, noise=noises)
    assert "PackedDecoderFn" in type(img.grad_fn).__name__
    d_f, = torch.autograd.grad(img, f, s["gy"].to(DEV))
    masks = [(dec.dec2_unpack(i, feats.shape) > 0).cpu() for i in range(1, dec.num_layers + 1)]
    p64, p32 = (decoder_ref.decoder_pinned_backward(s["sd"], s["feats"], s["wd"], s["noises"], s["gy"], masks=masks, dtype=dt, up_firs=n_up)
                for dt in (torch.float64, torch.float32))
    sym64 = decoder_ref.decoder_pinned_backward(s["sd"], s["feats"], s["wd"], s["noises"], s["gy"], masks=masks, dtype=torch.float64)
    (e_max, e_l2), (c_max, c_l2) = _per_sample(d_f.cpu(), p64["d_features"]), _per_sample(p32["d_features"], p64["d_features"])
    g_moved = float(_per_sample(sym64["d_features"], p64["d_features"])[0].min())
    log.record(f"dec_fir_packed_asym_up_{cid}", **{"img_" + k: v for k, v in imgs.items()}, chain_img=float((t32.double() - t64).abs().max()),
               truth_moved_by=moved, d_features_max=e_max.tolist(), d_features_l2=e_l2.tolist(), chain_d_features_max=c_max.tolist(),
               chain_d_features_l2=c_l2.tolist(), d_features_truth_moved_by=g_moved, fused_levels=runs["save"]["fused"])
    assert rgbs == 3 * (s["n_up"] + 1) - sum(r["acts"][-1] is None for r in runs.values())
    assert moved > 1000 * IMG_ATOL and g_moved > 1000 * GRAD_TOL, (moved, g_moved)      # the asymmetric kernel is felt in both directions
    assert all(v <= IMG_ATOL for v in imgs.values()), imgs
    assert float(c_max.max()) <= FIT_TOL and float(c_l2.max()) <= FIT_TOL
    assert float(e_max.max()) <= GRAD_TOL and float(e_l2.max()) <= GRAD_TOL, (e_max.tolist(), e_l2.tolist())
    log.check()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["blur", "up"])
def test_fir_buffers_that_differ_per_level_take_the_planar_path(which, monkeypatch):
    """Level 1's kernel is make_kernel([1, 2, 2, 1]) * 4 (as valid for the packed pipeline as level 0's, on its own) or, for the
    Upsample, the asymmetric FIR: the packed plan would apply level 0's taps at level 1."""
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    s = _setup("c")
    dec = _fresh_decoder(s)
    feats, wd, noises = _inputs(s)
    assert dec._dec2_ok(feats, wd, noises, None) and s["n_up"] == 2
    if which == "blur":
        k1 = sm.make_kernel([1, 2, 2, 1]) * 4
        assert sm.blur_factor(k1) is not None
        _write(dec.convs[2].conv.blur.kernel, k1)
    else:
        _write(dec.to_rgbs[1].upsample.kernel, asym_fir(4.0))
    ok = dec._dec2_ok(feats, wd, noises, None)
    img, io = _planar_stages(dec, s) if not ok else (None, None)
    built = sm._DEC2_STATES.get(dec) is not None
    blur_firs, up_firs = _firs(dec)
    t64, t32 = (decoder_ref.decoder_forward(s["sd"], s["feats"], s["wd"], noises=s["noises"], dtype=dt, blur_firs=blur_firs, up_firs=up_firs)
                for dt in (torch.float64, torch.float32))
    moved = float((t64 - s["own64"]["img"]).abs().max())
    e = None if img is None else float((img.double() - t64).abs().max())
    record(f"dec_fir_per_level_{which}", dec2_ok=ok, plan_built=built, img=e, chain_img=float((t32.double() - t64).abs().max()), truth_moved_by=moved)
    assert not ok and not built
    assert moved > 1000 * IMG_ATOL and e <= IMG_ATOL, (e, moved)
    log = _Log()
    _compare_planar(log, s, io, blur_firs, up_firs, f"per_level_{which}")
    log.record(f"dec_fir_per_level_{which}_stages")
    log.check()
    # putting level 0's kernel back gives the packed pipeline back
    _write(dec.convs[2].conv.blur.kernel, dec.convs[0].conv.blur.kernel)
    _write(dec.to_rgbs[1].upsample.kernel, dec.to_rgbs[0].upsample.kernel)
    assert dec._dec2_ok(feats, wd, noises, None)
