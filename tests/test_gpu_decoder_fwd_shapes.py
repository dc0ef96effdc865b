"""The forward of the packed decoder pipeline (csrc/decoder2.hip, e3dge_dec2_forward) against float64, STAGE BY STAGE, at the shapes of
tests/test_gpu_decoder_bwd_shapes.py (cases a - f: feature maps of 16^2, 12^2, 4^2 and 10^2, batch 1 - 3, shared and per-sample noise,
unit-variance latents, case f's small styles, channel counts 512 .. 32: every `gs` of pk_torgb_kernel and both fused ToRGB forms).

Truth: oracle/decoder_ref.decoder_stage in float64 applied to the packed forward's OWN input to that stage -- dec.dec2_unpack(k - 1) for
convolution k, the same activation and the workspace's previous skip image for a ToRGB -- so every comparison is one layer deep: a stage
cannot hide behind its predecessor or be blamed for it.  Yardstick: the same call in float32.  No branch pinning: a leaky relu whose branch
differs changes the output by at most 0.8 sqrt 2 times the pre-activation's own error.  The style table (e3dge_decoder_styles: s, demod,
s_amax) is compared with decoder_ref.decoder_modulations of the latent.

Measures (per sample, test_gpu_decoder_bwd_shapes._per_sample): max-abs error / the sample's maximum, and relative L2.

Bound, for every stage, sample and measure -- nothing in it is measured on the code under test:
    err <= 3 chain + 1e-6 + store
  chain          the float32 oracle stage's distance from float64 on the same inputs (measured per sample, on the oracle);
  3 chain + 1e-6 the project's bound for e3dge_modconv3x3 (tests/test_gpu_modconv.py);
  store          2^-20 for a packed activation, the rounding test_pack_unpack_roundtrip (tests/test_gpu_decoder2.py) holds the packed
                 format to; 0 for the fp32 skip images / the image, the style table and anything else that is stored as fp32.
Precondition, asserted for EVERY sample of EVERY stage (none is left out of a comparison): chain <= 2e-6, twice the largest value the
oracle's own chain shows on the CPU (test_reference_stages_are_fit_for_the_comparison).
The whole-chain image keeps IMG_ATOL = 1e-4 absolute against the float64 chain of the bwd file's _setup (the project's image gate, DESIGN.md
2, as every decoder test has it: the stages are what this file tightens); case f's ratio bound 1e-6 is the one _setup builds the styles to.

The fused ToRGB forms (case d: 64 channels at 40^2 -- convolution + store + ToRGB; 32 channels at 80^2, the last level -- convolution +
ToRGB, the activation stored only when a backward will need it) reduce the convolution's fp32 accumulators, not the stored activation; the
truth reads the stored one.  The two differ by the packed rounding (<= 2^-20 of the maximum per element), which the 1 x 1 reduction
averages far below the 1e-6 term.  Where the top activation is not stored (fused last level without save_for_backward) the forced input
of the last ToRGB is the top activation of the run WITH it, after asserting that both runs fed the convolution the same bits.

Tile forms: E3DGE_DEC2_UPBLUR_SHAPE = 0 .. 4 (the up-sampling stages) and E3DGE_DEC2_S1 = 0 .. 4 (the stride-1 stages that do not carry a
fused ToRGB: conv_s1 ignores the switch for those) on cases b (planes 12, 24, 48) and d (10, 20, 40, 80): every plane is narrower than
the 14 / 30 / 32 / 64-wide tiles or ends in a ragged one.

Measured on the MI355X (the `dec2_fwd_shapes_*` lines that conftest.record appends to the parity report; every figure per sample), largest
error per quantity, the float32 oracle stage's own distance for the same sample, and their ratio:
    conv1 (stride 1, 256 -> C)     1.3e-6 max / maximum (case f; chain 3.1e-7, 4.3 x; largest ratio 4.8, case a), 5.5e-7 relative L2 (case e)
    stride-1 stages                2.5e-6 max / maximum (case a, activation 3: 512 -> 512 at 32^2, sample 1; chain 3.0e-7, 8.2 x, the largest
                                   ratio; bound 2.85e-6, the smallest margin of the file: 1.16), 7.5e-7 relative L2 (case b, 2.8 x)
    up-sampling stages             9.3e-7 max / maximum (case a, activation 2; chain 2.6e-7, 3.6 x), 4.0e-7 relative L2 (case b, 1.6 x)
    skip images, stand-alone ToRGB 3.4e-7 max / maximum (case c, level 1; chain 7.2e-7), 1.7e-7 relative L2; never above the chain (ratio <= 1.0)
    skip images, fused ToRGB       1.9e-7 max / maximum (case d, 64 channels at 40^2; chain 1.9e-7), largest ratio 1.25 (32 channels at 80^2)
    the float32 stages themselves  <= 8.6e-7 max / maximum, <= 4.9e-7 relative L2 (precondition: 2e-6)
    image, whole chain             2.6e-6 .. 4.8e-6 absolute (cases a .. f; the float32 chain 1.5e-6 .. 3.0e-6, ratio 1.4 .. 2.2), the same in
                                   every form of a case
    style table                    s 1.6e-7 (case f; chain 2.1e-7), demod 1.4e-7 (case b; chain 1.2e-7, 1.2 x); s_amax the bit-exact maximum
                                   in every 3x3 layer; case f's small styles 2.9e-8 and 3.5e-8 of the sample's maximum; zero styles 0.0
    forced tile forms              up-sampling 9.1e-7 (case b, 48^2), 4.6e-7 (case d), stride-1 1.8e-6 (case b, 5.1 x), conv1 1.1e-6: the
                                   five forms of a kernel give the same figures (an output sums its channels and taps in the same order
                                   whatever the tile around it)
No committed kernel missed the bound, so no term was added to it.
Sensitivity, shown once on a scratch build: with the horizontal FIR tap g1 of pkconv_upblur2_kernel scaled by 1 + 2^-17 the older gates still
pass (test_every_stage_against_the_planar_kernels at 2e-5, the 1e-4 image gates of tests/test_gpu_decoder2.py), while every up-sampling
stage here fails (5.8e-6 .. 6.7e-6 of the maximum against bounds of 2.6e-6 .. 2.9e-6): 16 of the 26 GPU stage tests, the stride-1 forms
untouched.  (At 1 + 2^-16 the older gates fail as well: 2.1e-5 at activation 5, where the errors of two levels have added up.)"""
import functools

import pytest
import torch

from conftest import full_state_dict, record
from oracle import decoder_ref

import e3dge_amd  # noqa: F401
from e3dge_amd import synthetic as syn

from test_gpu_decoder_bwd_shapes import CASES, DEV, IMG_ATOL, SMALL_STYLE_RATIO, _decoder, _latents, _per_sample, _setup

STORE_PACKED = 2.0 ** -20      # test_pack_unpack_roundtrip's bound on the packed format
CHAIN_TOL = 2e-6               # the float32 oracle stage's own distance from float64: above it, it would not be a yardstick


def _bound(chain, store):
    return 3.0 * chain + 1e-6 + store


def _conv_stage(stages, k):
    """Entry of decoder_stages for the convolution that writes packed activation k (1: conv1, 2 + 2u: up-sampling, 3 + 2u: stride 1)."""
    return stages[0] if k == 1 else stages[(2 if k % 2 == 0 else 3) + 3 * ((k - 2) // 2)]


def _rgb_stage(stages, j):
    """Entry of decoder_stages for ToRGB j (0: to_rgb1, 1 + u: level u)."""
    return stages[1] if j == 0 else stages[4 + 3 * (j - 1)]


_FORCED = {}


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


def _forced(cid, s, what, stage, x, other):
    """(float64 truth, float32 yardstick) of one oracle stage on the fp32 CPU inputs x / other (noise or previous skip image).  Kept per
    (case, stage) and reused while the inputs are the same bits: the runs of one case mostly feed a stage the same activation."""
    hit = _FORCED.get((cid, what))
    if hit is not None and torch.equal(hit[0], x) and _same(hit[1], other):
        return hit[2], hit[3]
    lat = s["wd"][:, stage[2]]
    t64, y32 = (decoder_ref.decoder_stage(s["sd"], stage, x, lat, other, dtype=dt) for dt in (torch.float64, torch.float32))
    _FORCED[(cid, what)] = (x, other, t64, y32)
    return t64, y32


class _Log:
    """Every comparison of a test: measured first, recorded in one line of the parity report, asserted last."""

    def __init__(self):
        self.rows = []

    def add(self, what, got, t64, y32, store):
        assert tuple(got.shape) == tuple(t64.shape), (what, tuple(got.shape), tuple(t64.shape))
        (e_max, e_l2), (c_max, c_l2) = _per_sample(got, t64), _per_sample(y32, t64)
        self.rows.append(dict(what=what, store=store, finite=bool(torch.isfinite(got).all()), err_max=e_max.tolist(), err_l2=e_l2.tolist(),
                              chain_max=c_max.tolist(), chain_l2=c_l2.tolist()))

    def record(self, name, **extra):
        worst = {}
        for m in ("max", "l2"):
            flat = [(e, c, r["what"]) for r in self.rows for e, c in zip(r["err_" + m], r["chain_" + m])]
            e, c, w = max(flat, key=lambda t: t[0])
            worst.update({f"largest_err_{m}": e, f"largest_err_{m}_chain": c, f"largest_err_{m}_at": w,
                          f"largest_chain_{m}": max(t[1] for t in flat), f"largest_ratio_{m}": max(t[0] / max(t[1], 2.0 ** -53) for t in flat),
                          f"smallest_margin_{m}": min(_bound(t[1], r["store"]) / max(t[0], 2.0 ** -53) for r in self.rows
                                                      for t in zip(r["err_" + m], r["chain_" + m]))})
        record(name, comparisons=len(self.rows), **worst, **extra, stages=self.rows)

    def check(self):
        assert self.rows
        for r in self.rows:
            assert r["finite"], r["what"]
            for m in ("max", "l2"):
                for b, (e, c) in enumerate(zip(r["err_" + m], r["chain_" + m])):
                    assert c <= CHAIN_TOL, ("the float32 oracle stage is no yardstick here", r["what"], m, b, c)
                    assert e <= _bound(c, r["store"]), (r["what"], m, "sample", b, "err", e, "chain", c, "bound", _bound(c, r["store"]))


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def _chain(s, dtype, forced=False):
    """The oracle's stages chained over a case's inputs: (activations 0 .. num_layers, skip images).  forced: every stage's inputs are
    rounded to float32 first (what a stage of the packed forward is handed) -- the float64 chain the precondition is shown on."""
    stages = decoder_ref.decoder_stages(s["sd"])
    rnd = (lambda t: t.float()) if forced else (lambda t: t)
    n_conv = sum(st[0] == "conv" for st in stages)
    acts, skips = [s["feats"].to(dtype)], []
    for k in range(1, n_conv + 1):
        st = _conv_stage(stages, k)
        acts.append(decoder_ref.decoder_stage(s["sd"], st, rnd(acts[-1]), s["wd"][:, st[2]], s["noises"][k - 1], dtype=dtype))
        if k % 2 == 1:
            st = _rgb_stage(stages, k // 2)
            skips.append(decoder_ref.decoder_stage(s["sd"], st, rnd(acts[-1]), s["wd"][:, st[2]], rnd(skips[-1]) if skips else None, dtype=dtype))
    return acts, skips


@pytest.mark.parametrize("cid", ["c", "d"])
def test_chained_stages_are_the_decoder_forward(cid):
    """decoder_stage chained over decoder_stages IS decoder_forward: float64 difference 0, float32 bit-identical (case c: the smallest;
    case d: four levels, per-sample noise)."""
    s = _setup(cid)
    for dt in (torch.float64, torch.float32):
        acts, skips = _chain(s, dt)
        ref = decoder_ref.decoder_forward(s["sd"], s["feats"], s["wd"], noises=s["noises"], dtype=dt)
        assert skips[-1].dtype == dt and torch.equal(skips[-1], ref), (cid, dt, float((skips[-1] - ref).abs().max()))
        assert len(acts) == 2 * s["n_up"] + 2 and len(skips) == s["n_up"] + 1
    mods = decoder_ref.decoder_modulations(s["sd"], s["wd"], dtype=torch.float64)
    assert len(mods) == 3 * s["n_up"] + 2 and [d is None for _, d in mods] == [st[0] == "rgb" for st in decoder_ref.decoder_stages(s["sd"])]
    for (sty, _), own in zip([m for m in mods if m[1] is not None], s["own64"]["styles"]):      # the styles the backward file's truth used
        assert torch.equal(sty, own)
    # demod is what modulated_weights applies: (scale W s) demod has unit norm over (Ci, k, k) (up to the 1e-8 under the root)
    sty, dm = mods[0]
    w = decoder_ref.modulated_weights(s["sd"]["decoder.conv1.conv.weight"].double(), sty, demodulate=False)
    assert float(((w * dm.reshape(*dm.shape, 1, 1, 1)).pow(2).sum([2, 3, 4]) - 1).abs().max()) <= 1e-6


@pytest.mark.parametrize("cid", list(CASES))
def test_reference_stages_are_fit_for_the_comparison(cid):
    """CPU: the precondition on the oracle's own chain -- every stage of the float64 chain (inputs rounded to float32, as a stage of the
    packed forward receives them) against the float32 stage on the same inputs: chain <= 2e-6 per sample, in both measures, for every
    activation, skip image, style vector and demodulation factor."""
    s = _setup(cid)
    stages = decoder_ref.decoder_stages(s["sd"])
    acts, skips = _chain(s, torch.float64, forced=True)
    worst = 0.0
    for k in range(1, len(acts)):
        st = _conv_stage(stages, k)
        y32 = decoder_ref.decoder_stage(s["sd"], st, acts[k - 1].float(), s["wd"][:, st[2]], s["noises"][k - 1], dtype=torch.float32)
        for v in _per_sample(y32, acts[k]):
            assert torch.isfinite(v).all() and float(v.max()) <= CHAIN_TOL, (cid, "act", k, v.tolist())
            worst = max(worst, float(v.max()))
    for j in range(len(skips)):
        st = _rgb_stage(stages, j)
        y32 = decoder_ref.decoder_stage(s["sd"], st, acts[1 + 2 * j].float(), s["wd"][:, st[2]], skips[j - 1].float() if j else None, dtype=torch.float32)
        for v in _per_sample(y32, skips[j]):
            assert torch.isfinite(v).all() and float(v.max()) <= CHAIN_TOL, (cid, "rgb", j, v.tolist())
            worst = max(worst, float(v.max()))
    m64, m32 = (decoder_ref.decoder_modulations(s["sd"], s["wd"], dtype=dt) for dt in (torch.float64, torch.float32))
    for j, ((s64, d64), (s32, d32)) in enumerate(zip(m64, m32)):
        for a, b in ((s32, s64),) + (((d32, d64),) if d64 is not None else ()):
            for v in _per_sample(a, b):
                assert torch.isfinite(v).all() and float(v.max()) <= CHAIN_TOL, (cid, "style table", j, v.tolist())
    assert 0.0 < worst <= CHAIN_TOL


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def _fused_levels(dec, env):
    """Which levels' stride-1 convolution carries the fused ToRGB (s1_can_fuse_rgb and its caller in csrc/decoder2.hip)."""
    n_up = len(dec.to_rgbs)
    out = []
    for u in range(n_up):
        m = dec.convs[2 * u + 1].conv
        can = env.get("E3DGE_DEC2_FUSE_RGB", "1") != "0" and m.out_channel in (32, 64) and m.in_channel >= 32
        out.append(can and (u == n_up - 1 or env.get("E3DGE_DEC2_FUSE_RGB_MID", "1") != "0"))
    return out


def _run(dec, s, save=False, env=None):
    """One packed forward through Decoder.forward -- under no_grad, or (save) with the features requiring grad, which makes the forward
    keep its top activation for a backward (plan.save_for_backward) -- and what it left behind, on the CPU: activations 0 .. num_layers
    (None for a top activation this run did not store), the per-level skip images with the returned image last, and the fused levels."""
    feats, wd = s["feats"].to(DEV), s["wd"].to(DEV)
    noises = [n.to(DEV) for n in s["noises"]]
    B, res = feats.shape[0], feats.shape[2]
    assert dec._dec2_ok(feats, wd, noises, None)                                      # the packed pipeline, not the layer path
    if save:
        f = feats.clone().requires_grad_(True)
        img, _ = dec(f, [wd], input_is_latent=True, noise=noises)
        assert "PackedDecoderFn" in type(img.grad_fn).__name__, type(img.grad_fn).__name__
        img = img.detach()
    else:
        with torch.no_grad():
            img, _ = dec(feats, [wd], input_is_latent=True, noise=noises)
        assert img.grad_fn is None
    with torch.no_grad():
        st = dec._dec2_state(B, res, DEV)
        assert bool(st["plan"].save_for_backward) == save
        fused = _fused_levels(dec, env or {})
        acts = [dec.dec2_unpack(i, feats.shape).cpu() for i in range(dec.num_layers + 1)]
        if fused and fused[-1] and not save:
            acts[-1] = None                                                          # not written by this run: whatever an earlier one left
        skips = [t.cpu() for t in st["outs"][:-1]] + [img.cpu()]
    top = res << len(dec.to_rgbs)
    # guard: Decoder._forward_packed allocates the image itself (a test cannot place it inside a guard band), so: exact shapes, no NaN / inf
    assert tuple(skips[-1].shape) == (B, 3, top, top) and skips[-1].dtype == torch.float32 and skips[-1].is_contiguous()
    for j, t in enumerate(skips):
        assert tuple(t.shape) == (B, 3, res << j, res << j) and bool(torch.isfinite(t).all()), j
    return dict(acts=acts, skips=skips, fused=fused)


def _compare(log, cid, s, run, tag, conv_ks=None, rgbs=True, top_from=None):
    """Add every (or the given) stage of a run to the log: activation k against the forced stage on activation k - 1, skip image j against
    the forced ToRGB on its activation and the previous skip image."""
    stages = decoder_ref.decoder_stages(s["sd"])
    acts, skips = run["acts"], run["skips"]
    for k in (range(1, len(acts)) if conv_ks is None else conv_ks):
        if acts[k] is None:
            continue
        t64, y32 = _forced(cid, s, f"act{k}", _conv_stage(stages, k), acts[k - 1], s["noises"][k - 1])
        log.add(f"{tag}.act{k}", acts[k], t64, y32, STORE_PACKED)
    for j in (range(len(skips)) if rgbs else ()):
        x = acts[1 + 2 * j]
        if x is None:                              # fused last level, top activation not stored: the run that stored it, on the same input bits
            assert top_from is not None and torch.equal(top_from["acts"][2 * j], acts[2 * j])
            x = top_from["acts"][1 + 2 * j]
        t64, y32 = _forced(cid, s, f"rgb{j}", _rgb_stage(stages, j), x, skips[j - 1] if j else None)
        log.add(f"{tag}.rgb{j}" + (".fused" if j and run["fused"][j - 1] else ""), skips[j], t64, y32, 0.0)


def _image(s, run):
    """(absolute error of the image against the float64 chain, the float32 chain's, their ratio)."""
    e = float((run["skips"][-1].double() - s["own64"]["img"]).abs().max())
    c = float((s["own32"]["img"].double() - s["own64"]["img"]).abs().max())
    return dict(img=e, chain_img=c, ratio_img=e / c)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_every_stage_against_float64(cid, monkeypatch):
    """Every activation 1 .. num_layers, every skip image and the image of the packed forward against its forced float64 stage: with the
    top activation kept for a backward and without (both settings of rgb_store on a fused last level), with E3DGE_DEC2_FUSE_RGB=0 (the
    stand-alone pk_torgb_kernel at every level; the top activation is stored whatever the channel count) and, where a middle level
    fuses (case d), with E3DGE_DEC2_FUSE_RGB_MID=0."""
    s = _setup(cid)
    dec = _decoder(s, cid)
    for v in ("E3DGE_DEC2_FUSE_RGB", "E3DGE_DEC2_FUSE_RGB_MID", "E3DGE_DEC2_S1", "E3DGE_DEC2_UPBLUR_SHAPE"):
        monkeypatch.delenv(v, raising=False)
    runs = {"save": _run(dec, s, save=True), "nosave": _run(dec, s)}
    monkeypatch.setenv("E3DGE_DEC2_FUSE_RGB", "0")
    runs["nofuse"] = _run(dec, s, env={"E3DGE_DEC2_FUSE_RGB": "0"})
    monkeypatch.delenv("E3DGE_DEC2_FUSE_RGB")
    if any(runs["save"]["fused"][:-1]):
        monkeypatch.setenv("E3DGE_DEC2_FUSE_RGB_MID", "0")
        runs["nofuse_mid"] = _run(dec, s, env={"E3DGE_DEC2_FUSE_RGB_MID": "0"})
        monkeypatch.delenv("E3DGE_DEC2_FUSE_RGB_MID")
    assert all(a is not None for a in runs["save"]["acts"]) and all(a is not None for a in runs["nofuse"]["acts"])
    assert not any(runs["nofuse"]["fused"]) and (cid != "d" or (runs["save"]["fused"] == [False, True, True] and "nofuse_mid" in runs
                                                                and runs["nofuse_mid"]["fused"] == [False, False, True]))
    log, imgs = _Log(), {}
    for tag, run in runs.items():
        _compare(log, cid, s, run, tag, top_from=runs["save"])
        imgs.update({f"{k}_{tag}": v for k, v in _image(s, run).items()})
    log.record(f"dec2_fwd_shapes_{cid}", **imgs, fused_levels=runs["save"]["fused"])
    # nothing left out: every activation a run stored (all but the top one of a fused last level without save) and every skip image
    assert len(log.rows) == sum(dec.num_layers - (r["acts"][-1] is None) + len(dec.to_rgbs) + 1 for r in runs.values())
    assert [t for t, r in runs.items() if r["acts"][-1] is None] == (["nosave", "nofuse_mid"] if cid == "d" else [])
    for tag in runs:
        assert imgs[f"img_{tag}"] <= IMG_ATOL, (tag, imgs)
    log.check()


@functools.lru_cache(maxsize=None)
def _zero_style_setup():
    """The decoder of case c with styles that are exactly zero in every precision: sample 0 has latent rows 1 - 3 zero and the modulation
    bias of two channels of convs.0 (up-sampling), convs.1 (stride 1) and to_rgbs.0 is zero; sample 1 has the same bias and a non-zero
    latent (as test_styles_that_are_exactly_zero of the backward file builds it)."""
    layers = {"decoder.convs.0.conv.modulation.": (3, 200), "decoder.convs.1.conv.modulation.": (5, 77), "decoder.to_rgbs.0.conv.modulation.": (9, 300)}
    g, sd = full_state_dict(size=32, cm=1, res=8)
    for p, chans in layers.items():
        sd[p + "bias"][list(chans)] = 0.0
    g.load_state_dict(sd)
    g.eval().requires_grad_(False)
    feats, noises, _ = syn.decoder_grad_inputs(2, 32, 8, seed=31)
    wd = _latents(2, g.decoder.n_latent, False, 31).clone()
    wd[0, 1:4] = 0.0
    return dict(case=dict(), g=g, sd=sd, feats=feats, wd=wd, noises=noises, n_up=2, small_ratio={}, zero=dict(zip((2, 3, 4), layers.values())))


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES) + ["zero"])
def test_style_table_against_float64(cid):
    """After a forward: s of every modulated layer (ToRGB included) and demod of every 3x3 layer, per sample, against
    decoder_ref.decoder_modulations of the latent in float64 (bound as above, store = 0: the table is fp32); s_amax is the maximum of the
    |s| the kernel itself wrote, bit for bit.  Case f: the small styles reach the table as small as _setup made them.  `zero`: styles
    that are exactly 0.0 -- the measure is the error over the LAYER's maximum for the sample, so it is an absolute bound there, and the
    table holds 0.0 (0 w + 0 = 0 in any precision)."""
    s = _zero_style_setup() if cid == "zero" else _setup(cid)
    dec = _decoder(s, cid)
    _run(dec, s)
    B = s["feats"].shape[0]
    views = [tuple(None if t is None else t.cpu() for t in v) for v in dec._style_table(B, DEV)[2]]
    m64, m32 = (decoder_ref.decoder_modulations(s["sd"], s["wd"], dtype=dt) for dt in (torch.float64, torch.float32))
    assert len(views) == len(m64) == 3 * s["n_up"] + 2
    log, amax_ok, extra = _Log(), [], {}
    for j, ((sv, dv, av), (s64, d64), (s32, d32)) in enumerate(zip(views, m64, m32)):
        log.add(f"s{j}", sv, s64, s32, 0.0)
        assert (dv is None) == (d64 is None) == (av is None)
        if d64 is not None:
            log.add(f"demod{j}", dv, d64, d32, 0.0)
            amax_ok.append(torch.equal(av, sv.abs().amax(1)))
    for k, chans in s["case"].get("small", {}).items():                # convs.k is modulated layer 2 + 3 (k // 2) + k % 2
        sv = views[2 + 3 * (k // 2) + k % 2][0]
        extra[f"small_style_ratio_convs{k}"] = float(sv[0, list(chans)].abs().max() / sv[0].abs().max())
    for j, chans in s.get("zero", {}).items():
        extra[f"zero_style_layer{j}"] = float(views[j][0][0, list(chans)].abs().max())
        assert float(m64[j][0][0, list(chans)].abs().max()) == 0.0 and float(m64[j][0][1, list(chans)].abs().min()) > 0.0
    log.record(f"dec2_fwd_shapes_styles_{cid}", s_amax_is_the_maximum=amax_ok, **extra)
    assert amax_ok and all(amax_ok), amax_ok
    if cid == "f":
        assert len(extra) == 2 and all(v <= SMALL_STYLE_RATIO for v in extra.values()), extra
    if cid == "zero":
        assert len(extra) == 3 and all(v == 0.0 for v in extra.values()), extra
    log.check()


FORMS = [("E3DGE_DEC2_UPBLUR_SHAPE", str(v)) for v in range(5)] + [("E3DGE_DEC2_S1", str(v)) for v in range(5)]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["b", "d"])
@pytest.mark.parametrize("form", FORMS, ids=[f"{n[11:].lower()}{v}" for n, v in FORMS])
def test_every_forward_tile_form_on_ragged_planes(form, cid, monkeypatch):
    """Every tile form of the up-sampling kernel (pkconv_upblur2_kernel: 14 x 30, 6 x 30, 6 x 30 with four waves, 14 x 14 with four and
    with eight waves) and of the stride-1 kernel (pkconv_s1_kernel: 4 x 32, 4 x 64, 8 x 64 with 64 channels; 8 x 64 with 32 channels,
    with eight and with four waves) on planes that are narrower than the tile or ragged against it, each stage the switch reaches against
    its forced float64 stage.  E3DGE_DEC2_S1 reaches the stride-1 convolutions without a fused ToRGB (conv_s1 takes the fused forms
    before it reads the switch): all three of case b; conv1 and level 0 of case d (256 and 128 channels: every form's channel multiple)."""
    var, value = form
    s = _setup(cid)
    dec = _decoder(s, cid)
    planes = [s["feats"].shape[2] << u for u in range(s["n_up"] + 1)]
    assert planes == ([12, 24, 48] if cid == "b" else [10, 20, 40, 80]) and all(p < t or p % t for p in planes for t in (14, 30, 32, 64))
    for v in ("E3DGE_DEC2_FUSE_RGB", "E3DGE_DEC2_FUSE_RGB_MID", "E3DGE_DEC2_S1", "E3DGE_DEC2_UPBLUR_SHAPE"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv(var, value)
    run = _run(dec, s)
    monkeypatch.delenv(var)
    if var == "E3DGE_DEC2_UPBLUR_SHAPE":
        ks = [2 + 2 * u for u in range(s["n_up"])]
    else:
        ks = [1] + [3 + 2 * u for u in range(s["n_up"]) if not run["fused"][u]]
        assert ks == ([1, 3, 5] if cid == "b" else [1, 3])
    log = _Log()
    _compare(log, cid, s, run, f"{var[11:].lower()}{value}", conv_ks=ks, rgbs=False)
    img = _image(s, run)
    log.record(f"dec2_fwd_shapes_{cid}_{var[11:].lower()}{value}", **img)
    assert len(log.rows) == len(ks)
    assert img["img"] <= IMG_ATOL, img
    log.check()
