"""The backward of the packed decoder pipeline (csrc/decoder2_bwd.h, e3dge_dec2_backward) against float64 at the shapes, batches, noise
forms and styles tests/test_gpu_decoder_bwd.py never reaches: feature maps of 4^2 .. 16^2 (planes narrower than one tile, sizes that are
no power of two, R * R below one 4,096-pixel chunk of pk_dstyle_sums_kernel and a ragged last chunk), batch 3, shared noise
(noise_batch == 1), the 32-channel and 4 x 64 tile forms of conv_s1_bwd, unit-variance latents (|s| from 2e-3 to 4, a fifth of the styles
negative) and styles forced to 1e-6 of the layer's maximum.

Truth: oracle/decoder_ref.decoder_pinned_backward in float64 -- autograd of the oracle's layers with the branch of every leaky relu taken
from the signs of the packed forward's OWN activations (dec.dec2_unpack(idx) > 0), so that the step function lrelu' cannot differ between
the two sides and what is compared is arithmetic.  Yardstick: the same function in float32 with the same masks.  A sample / latent row
enters a comparison only if that float32 chain is itself within 1e-5 of float64 there, and every test asserts that none is left out
(test_inputs_are_fit_for_the_comparison shows it on the CPU, with the masks of the float64 forward).

Bounds: image 1e-4 absolute; every stage gradient and d features 1e-4 in max-abs / maximum and in relative L2, PER SAMPLE; d latent 1e-4
in max-abs / maximum PER (sample, latent row); bound / measured maximum of every packed gradient within [1, 2^12].

Measured on the MI355X (the `dec2_bwd_shapes_*` lines that conftest.record appends to the parity report), largest error per quantity and its ratio to the float32 chain's
own distance from float64 for the same sample / row:
    image                      4.8e-6 absolute (cases e, f; the float32 chain: 2.9e-6)
    stage gradients, per sample 2.1e-6 max / maximum (case e, G of level 0's up-sampling layer), 4.4 x the chain; largest ratio 5.7 (case a)
    d features, per sample     2.3e-6 max / maximum, 1.5e-6 relative L2 (case f), 4.7 x and 3.0 x the chain
    d latent, per row          5.6e-6 (case b, sample 1, row 1), 8.5 x the chain; case f 4.8e-6, 6.2 x
    bound / measured maximum   2^0.69 .. 2^9.56 (case c)
    activation signs that differ from the float64 forward: 0 - 3 of 0.3 - 7.5 million per case
Before pk_dstyle_direct_kernel (csrc/decoder2_bwd.h, "small styles") case f's d latent was 5.6e-2 (row 2) and 1.3e-1 (row 3) of the row's
maximum for sample 0 -- S1 / s at |s| = 1e-6 max|s| -- and case e's worst row 1.5e-5; every other figure above was the same.  The styles
that kernel serves per case (|s| <= 2^-10 of the layer's maximum): a 0, b 8, c 1, d 0, e 5, f 11."""
import functools

import numpy as np
import pytest
import torch

from conftest import full_state_dict, record
from oracle import decoder_ref

import e3dge_amd  # noqa: F401
from e3dge_amd import synthetic as syn

from test_gpu_decoder_bwd import _bound_looseness

DEV = "cuda:0"
IMG_ATOL = 1e-4
GRAD_TOL = 1e-4            # the number test_every_packed_gradient_against_autograd_of_the_oracle holds pinned packed gradients to
FIT_TOL = 1e-5             # the float32 pinned chain's own distance from float64: a row / sample above it would not be a reference

# id -> decoder (size, res) of full_state_dict(cm = 1), feature-map size, batch, shared noise, unit-variance latents, what it reaches
CASES = {
    # baseline; the phase plane of pk_dblur_kernel at the top level is 33 wide: one column past a 32-wide tile
    "a": dict(size=64, res=16, feat=16, B=2, shared=False, unit=False),
    # 12 -> 24 -> 48: no power of two, odd batch, every plane under one tile of launch_down (4 x 32) / conv_s1_bwd, noise_batch == 1,
    # wide and negative styles
    "b": dict(size=64, res=16, feat=12, B=3, shared=True, unit=True),
    # the smallest input _dec2_ok admits: one tile row, R * R (16, 64, 256) under one chunk at every level
    "c": dict(size=32, res=8, feat=4, B=1, shared=True, unit=True),
    # channels 256 / 128 / 64 / 32: the 32-channel tile form of conv_s1_bwd on the last level, whose 80^2 = 6,400 pixels are one full
    # chunk and a ragged one of 2,304
    "d": dict(size=512, res=64, feat=10, B=2, shared=False, unit=False),
    # 128^2 at the top: the 4 x 64 tile form (64^2 < pixels <= 128^2), four chunks
    "e": dict(size=128, res=16, feat=16, B=1, shared=True, unit=True),
    # as b, and for sample 0 two input channels of the up-sampling layer convs.2 and of the stride-1 layer convs.1 have
    # |s| <= 1e-6 max|s| (modulation.bias edited; the modulation weight rows stay, so these channels' dL/ds reaches d latent)
    "f": dict(size=64, res=16, feat=12, B=2, shared=False, unit=True, small={2: (3, 200), 1: (5, 77)}),
}
SMALL_STYLE_RATIO = 1e-6


def _latents(B, n_latent, unit, seed):
    """(B, n_latent, 512): syn.synthetic_inputs (0.1 N(0,1)) or the decoder half of syn.stress_inputs (N(0,1))."""
    wd = syn.stress_inputs("wide", B, seed=seed)[1] if unit else syn.synthetic_inputs(B, seed=seed)[1]
    return wd[:, :n_latent].contiguous()


def _style_prefix(k):
    return f"decoder.convs.{k}.conv.modulation."


@functools.lru_cache(maxsize=None)
def _setup(cid):
    """Decoder, state dict and seeded CPU inputs of a case, with the float64 chain on its OWN branches (`own64`: the plain float64
    forward / backward of the oracle) and the float32 chain pinned to those (`own32`).  Computed once, shared by every test, never
    modified."""
    c = CASES[cid]
    seed = 100 + ord(cid)
    g, sd = full_state_dict(size=c["size"], cm=1, res=c["res"])
    dec = g.decoder
    n_up = len(dec.to_rgbs)
    feats, noises, gy = syn.decoder_grad_inputs(c["B"], c["feat"] << n_up, c["feat"], seed=seed)
    if c["shared"]:
        noises = [n[:1].contiguous() for n in noises]
    wd = _latents(c["B"], dec.n_latent, c["unit"], seed)
    achieved = {}
    for k, chans in c.get("small", {}).items():           # convs.k reads latent row k + 1
        sd64 = {key: v.double() for key, v in sd.items() if key.startswith(_style_prefix(k))}
        s = decoder_ref.equal_linear(sd64, _style_prefix(k), wd[:, k + 1].double())
        bias = sd[_style_prefix(k) + "bias"]
        for ci in chans:
            bias[ci] = (bias[ci].double() - s[0, ci]).float()
        s = decoder_ref.equal_linear({key: v.double() for key, v in sd.items() if key.startswith(_style_prefix(k))}, _style_prefix(k), wd[:, k + 1].double())
        achieved[k] = float(s[0, list(chans)].abs().max() / s[0].abs().max())
    if achieved:
        g.load_state_dict(sd)
    g.eval().requires_grad_(False)
    own64 = decoder_ref.decoder_pinned_backward(sd, feats, wd, noises, gy, dtype=torch.float64)
    own32 = decoder_ref.decoder_pinned_backward(sd, feats, wd, noises, gy, masks=own64["signs"], dtype=torch.float32)
    return dict(case=c, g=g, sd=sd, feats=feats, wd=wd, noises=noises, gy=gy, n_up=n_up, own64=own64, own32=own32, small_ratio=achieved)


def _per_sample(got, ref):
    """(max-abs error / maximum, relative L2) of every sample, each normalised by ITS OWN maximum / norm of the reference."""
    g, r = got.detach().double().cpu().flatten(1), ref.detach().double().cpu().flatten(1)
    d = g - r
    return d.abs().amax(1) / r.abs().amax(1), d.norm(dim=1) / r.norm(dim=1)


def _per_row(got, ref):
    """max-abs error of every (sample, latent row) over that row's own maximum in the reference: (B, n_latent)."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    return (g - r).abs().amax(2) / r.abs().amax(2)


def _distances(got, truth):
    """Every quantity of a backward (dict with d_pre, d_features, d_latent) against `truth`, by the measures above:
    {name: tensor of per-sample / per-row figures}."""
    out = {}
    for i, (a, b) in enumerate(zip(got["d_pre"], truth["d_pre"]), start=1):
        out[f"g{i}_max"], out[f"g{i}_l2"] = _per_sample(a, b)
    out["d_features_max"], out["d_features_l2"] = _per_sample(got["d_features"], truth["d_features"])
    out["d_latent_row_max"] = _per_row(got["d_latent"], truth["d_latent"])
    return out


def _assert_fit(chain, what):
    """The precondition: the float32 pinned chain within FIT_TOL of float64 for EVERY sample and latent row -- none is left out."""
    for k, v in chain.items():
        assert torch.isfinite(v).all() and float(v.max()) <= FIT_TOL, (what, k, v.tolist())


@pytest.mark.parametrize("cid", list(CASES))
def test_inputs_are_fit_for_the_comparison(cid):
    """CPU: with the masks of the float64 forward, the float32 pinned chain meets the 1e-5 precondition per sample and per latent row
    (every latent row has a gradient: a decoder reads all n_latent of them), and case f's small styles are as small as its line says."""
    s = _setup(cid)
    assert all(float(r) > 0 for r in s["own64"]["d_latent"].abs().amax(2).flatten())
    _assert_fit(_distances(s["own32"], s["own64"]), cid)
    assert float((s["own32"]["img"].double() - s["own64"]["img"]).abs().max()) <= 1e-5
    if "small" in s["case"]:
        assert s["small_ratio"] and all(r <= SMALL_STYLE_RATIO for r in s["small_ratio"].values()), s["small_ratio"]
        for k, chans in s["case"]["small"].items():       # ... in the oracle's own style, and only for sample 0
            st = s["own64"]["styles"][1 + k]
            assert float(st[0, list(chans)].abs().max()) <= SMALL_STYLE_RATIO * float(st[0].abs().max())
            assert float(st[1, list(chans)].abs().min()) > 1e-3 * float(st[1].abs().max())
    if s["case"]["unit"]:                                  # wide and negative styles, as the case's line says
        st = torch.cat([t.flatten() for t in s["own64"]["styles"]])
        assert float(st.abs().max()) > 2.5 and 0.1 < float((st < 0).double().mean()) < 0.3


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
_ON_DEVICE = {}
_PINNED = {}


def _decoder(s, cid):
    if cid not in _ON_DEVICE:
        _ON_DEVICE[cid] = s["g"].decoder.to(DEV)
    return _ON_DEVICE[cid]


def _run_packed(dec, s, noises=None):
    """One forward + backward through Decoder.forward with the features AND the latent requiring grad (the native d latent runs); the
    image, both gradients, every stage gradient and the signs of the packed forward's activations, on the CPU."""
    feats, wd, gy = s["feats"].to(DEV), s["wd"].to(DEV), s["gy"].to(DEV)
    noises = [n.to(DEV) for n in (s["noises"] if noises is None else noises)]
    f, lat = feats.clone().requires_grad_(True), wd.clone().requires_grad_(True)
    img, _ = dec(f, [lat], input_is_latent=True, noise=noises)
    assert "PackedDecoderFn" in type(img.grad_fn).__name__, type(img.grad_fn).__name__     # the packed pipeline, not the library path
    d_f, d_l = torch.autograd.grad(img, [f, lat], gy)
    idx = range(1, dec.num_layers + 1)
    out = dict(img=img.detach().cpu(), d_features=d_f.cpu(), d_latent=d_l.cpu(),
               masks=[(dec.dec2_unpack(i, feats.shape) > 0).cpu() for i in idx],
               d_pre=[dec.dec2_unpack_grad(i, feats.shape).cpu() for i in idx],
               loose=_bound_looseness(dec, feats.shape[0], feats.shape[2]))
    assert tuple(out["img"].shape) == (feats.shape[0], 3, s["gy"].shape[2], s["gy"].shape[2])
    return out


def _pinned(cid, s, masks, sd=None):
    """(float64, float32) pinned chain for the masks of a packed forward; the forward does not depend on what a test varies in the
    backward, so one evaluation serves every run of a case with the same masks."""
    hit = _PINNED.get(cid)
    if sd is None and hit is not None and all(torch.equal(a, b) for a, b in zip(hit[0], masks)):
        return hit[1], hit[2]
    t64, t32 = (decoder_ref.decoder_pinned_backward(sd or s["sd"], s["feats"], s["wd"], s["noises"], s["gy"], masks=masks, dtype=dt)
                for dt in (torch.float64, torch.float32))
    if sd is None:
        _PINNED[cid] = (masks, t64, t32)
    return t64, t32


def _measure(name, s, run, t64, t32, **extra):
    """Record (before any assertion) every error of `run` against float64, the float32 chain's own distance, their ratio and the number
    of activation signs in which the packed forward differs from the float64 forward; return what the assertions need."""
    err, chain = _distances(run, t64), _distances(t32, t64)
    n_flip = sum(int((m != o).sum()) for m, o in zip(run["masks"], s["own64"]["signs"]))
    e = dict(img=float((run["img"].double() - t64["img"]).abs().max()), chain_img=float((t32["img"].double() - t64["img"]).abs().max()),
             activations_whose_sign_differs_from_float64=n_flip, activations=sum(m.numel() for m in run["masks"]),
             bound_over_measured_max_log2_min=float(np.log2(min(run["loose"]))), bound_over_measured_max_log2_max=float(np.log2(max(run["loose"]))))
    for k in err:
        e[k] = float(err[k].max())
        e["chain_" + k] = float(chain[k].max())
        e["ratio_" + k] = float((err[k] / chain[k]).max())
    e["d_latent_rows"] = [[float(v) for v in row] for row in err["d_latent_row_max"]]
    e["chain_d_latent_rows"] = [[float(v) for v in row] for row in chain["d_latent_row_max"]]
    record(name, **extra, **e)
    return err, chain, e


def _assert_bounds(err, chain, e, run):
    _assert_fit(chain, "float32 chain on the packed forward's masks")
    assert min(run["loose"]) >= 1.0 and max(run["loose"]) <= 2.0 ** 12, run["loose"]      # a bound, and not looser than the split tolerates
    assert e["img"] <= IMG_ATOL, e
    for k, v in err.items():
        assert torch.isfinite(v).all() and float(v.max()) <= GRAD_TOL, (k, v.tolist(), e)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_backward_against_float64_with_the_packed_branches(cid):
    s = _setup(cid)
    dec = _decoder(s, cid)
    run = _run_packed(dec, s)
    t64, t32 = _pinned(cid, s, run["masks"])
    # how many (sample, channel) styles of the 3x3 layers pk_dstyle_direct_kernel serves (|s| <= 2^-10 of the layer's maximum for the sample)
    n_small = sum(int((st.abs() <= 2.0 ** -10 * st.abs().amax(1, keepdim=True)).sum()) for st in s["own64"]["styles"])
    err, chain, e = _measure(f"dec2_bwd_shapes_{cid}", s, run, t64, t32, styles_served_by_the_direct_kernel=n_small,
                             **{f"small_style_ratio_convs{k}": v for k, v in s["small_ratio"].items()})
    assert n_small >= 4 or cid != "f"
    _assert_bounds(err, chain, e, run)


@pytest.mark.gpu
def test_every_tile_form_of_the_stride_1_data_gradient(monkeypatch):
    """conv_s1_bwd on case d's decoder: the automatic choice and E3DGE_DEC2_S1_BWD = 0 .. 3 (64 channels x 4 x 32, 4 x 64, 8 x 64;
    32 channels x 8 x 64), each held to the same bounds and each forced form bit-identical over two runs.  Which forms may be forced
    here: the backward's Co is the layer's input channel count -- 256, 128, 128, 64, 64, 32 (conv1, then conv / up per level; the
    up-sampling layers take launch_down, not this switch).  conv_s1_bwd itself sends every Co that is no multiple of 64 (the 32-channel
    layer) to form 3 whatever is forced; for the others forms 0 - 2 need Co % 64 == 0 and form 3 Co % 32 == 0, and launch_s1 REFUSES
    (E3DGE_REQUIRE, an error code) a form whose LDS need exceeds 160 KB -- form 2 needs 158,208 + 16 Co, which holds for Co <= 352.  So
    every forced form is admitted by every layer of this geometry, and none could launch unchecked.  (The forms need not differ in a
    single bit: every output element sums its channels and taps in the same order whatever the tile around it.)"""
    s = _setup("d")
    dec = _decoder(s, "d")
    chans = [dec.conv1.conv.in_channel] + [c.conv.in_channel for c in dec.convs]
    assert chans == [256, 256, 128, 128, 64, 64, 32] and all(c % 64 == 0 and 158208 + 16 * c <= 160 * 1024 for c in chans[:-1])
    runs = {"auto": _run_packed(dec, s)}
    for form in "0123":
        monkeypatch.setenv("E3DGE_DEC2_S1_BWD", form)
        runs[form] = _run_packed(dec, s)
        again = _run_packed(dec, s)
        for k in ("d_features", "d_latent"):
            assert torch.equal(runs[form][k], again[k]), (form, k)
        assert all(torch.equal(a, b) for a, b in zip(runs[form]["d_pre"], again["d_pre"])), form
    monkeypatch.delenv("E3DGE_DEC2_S1_BWD")
    # The switch is read on every call: case a's decoder has 512 input channels at 32^2, where the 8 x 64 form would need
    # 158,208 + 16 * 512 bytes of LDS -- launch_s1 refuses it with an error code, and the next call without the switch is what it was.
    sa = _setup("a")
    dec_a = _decoder(sa, "a")
    before = _run_packed(dec_a, sa)
    monkeypatch.setenv("E3DGE_DEC2_S1_BWD", "2")
    with pytest.raises(RuntimeError, match="LDS budget"):
        _run_packed(dec_a, sa)
    monkeypatch.delenv("E3DGE_DEC2_S1_BWD")
    after = _run_packed(dec_a, sa)
    assert torch.equal(before["d_features"], after["d_features"]) and torch.equal(before["d_latent"], after["d_latent"])
    t64, t32 = _pinned("d", s, runs["auto"]["masks"])
    results = []
    for form, run in runs.items():
        assert all(torch.equal(a, b) for a, b in zip(run["masks"], runs["auto"]["masks"])), form       # the forward does not see the switch
        results.append(_measure(f"dec2_bwd_shapes_d_s1_bwd_{form}", s, run, t64, t32) + (run,))
    for err, chain, e, run in results:
        _assert_bounds(err, chain, e, run)


@pytest.mark.gpu
def test_shared_noise_equals_the_same_image_repeated_per_sample():
    """Case b: one shared noise image against the same image repeated B times as per-sample noise -- the data is the same and only the
    plane selection (noise_batch > 1 ? b : 0) differs, so every gradient is the same bits."""
    s = _setup("b")
    dec = _decoder(s, "b")
    B = s["case"]["B"]
    assert all(n.shape[0] == 1 for n in s["noises"])
    shared = _run_packed(dec, s)
    repeated = _run_packed(dec, s, noises=[n.repeat(B, 1, 1, 1).contiguous() for n in s["noises"]])
    assert torch.equal(shared["img"], repeated["img"])
    for k in ("d_features", "d_latent"):
        assert torch.equal(shared[k], repeated[k]), k
    for i, (a, b) in enumerate(zip(shared["d_pre"], repeated["d_pre"]), start=1):
        assert torch.equal(a, b), i


@pytest.mark.gpu
def test_styles_that_are_exactly_zero():
    """dL/ds[ci] = r1 / s[ci] - s[ci] (...) with r1 = sum_p x dx, and dx is proportional to s[ci]: at s[ci] == 0 the stored dx is exactly
    zero and there is nothing to divide out, while the true derivative, sum_{co, tap} dL/dw'' (scale W) demod, is NOT zero in general.
    s is exactly zero only when the channel's modulation bias is zero AND its latent row is zero (or cancels to the bit): sample 0 here
    has latent rows 1 - 3 zero and the bias of two channels of convs.0 (up-sampling), convs.1 (stride 1) and to_rgbs.0 zero, so these
    styles are 0.0 in every precision; sample 1 has the same bias and a non-zero latent.
    3x3 layers: such a channel is a small style (|s| <= 2^-10 max|s|), whose first term pk_dstyle_direct_kernel takes from its
    definition -- exact at zero too.  Rows 1 and 2 of sample 0 meet the float64 truth to the usual 1e-4 (the branch returned 0 here until
    the small styles got their own kernel: 6e-2 and 1.9e-2 of the rows' maxima were missing).
    ToRGB: pk_dstyle_kernel keeps `|s| <= 1e-30 -> 0`; S3 = sum_p act (ToRGB^T d rgb) is built from the table (scale W) s, which is zero
    with s, and the channel's share sum_c (scale W)[c][ci] sum_p act d rgb[c] is not recovered.  Pinned as what it is: row 3 of sample 0
    equals float64's row with those channels' dL/ds removed (the truth for a decoder whose ToRGB modulation weight rows for them are
    zero: sample 0's forward is the same), and the float64 truth itself is further away by exactly that share."""
    conv_layers = {"decoder.convs.0.conv.modulation.": (3, 200), "decoder.convs.1.conv.modulation.": (5, 77)}
    rgb_layers = {"decoder.to_rgbs.0.conv.modulation.": (9, 300)}
    layers = {**conv_layers, **rgb_layers}
    latent_row = dict(zip(layers, (1, 2, 3)))
    g, sd = full_state_dict(size=32, cm=1, res=8)
    for p, chans in layers.items():
        sd[p + "bias"][list(chans)] = 0.0
    g.load_state_dict(sd)
    dec = g.eval().requires_grad_(False).decoder.to(DEV)
    feats, noises, gy = syn.decoder_grad_inputs(2, 32, 8, seed=31)
    wd = _latents(2, dec.n_latent, False, 31).clone()
    wd[0, 1:4] = 0.0
    s = dict(feats=feats, wd=wd, noises=noises, gy=gy, sd=sd, own64=decoder_ref.decoder_pinned_backward(sd, feats, wd, noises, gy))
    run = _run_packed(dec, s)
    removed = {k: v.clone() for k, v in sd.items()}
    for p, chans in rgb_layers.items():
        removed[p + "weight"][list(chans)] = 0.0
    t64, t32 = _pinned(None, s, run["masks"], sd=s["sd"])
    z64, z32 = _pinned(None, s, run["masks"], sd=removed)
    for p, chans in layers.items():      # exactly zero in the oracle's style for sample 0 only
        st = decoder_ref.equal_linear(sd, p, wd[:, latent_row[p]])
        assert float(st[0, list(chans)].abs().max()) == 0.0 and float(st[1, list(chans)].abs().min()) > 0.0
    assert float((z64["img"][0] - t64["img"][0]).abs().max()) == 0.0
    got, fit = _per_row(run["d_latent"], t64["d_latent"]), _per_row(t32["d_latent"], t64["d_latent"])
    got_z, fit_z = _per_row(run["d_latent"][:1], z64["d_latent"][:1]), _per_row(z32["d_latent"][:1], z64["d_latent"][:1])
    lost = _per_row(z64["d_latent"][:1], t64["d_latent"][:1])
    record("dec2_bwd_shapes_zero_style", sample0_vs_truth=got[0].tolist(), sample0_vs_truth_without_the_zero_torgb_channels=got_z[0].tolist(),
           sample1_vs_truth=got[1].tolist(), share_of_the_zero_torgb_channels=lost[0].tolist(), chain=fit.tolist(), chain_without=fit_z[0].tolist())
    assert float(fit.max()) <= FIT_TOL and float(fit_z.max()) <= FIT_TOL
    assert torch.isfinite(run["d_latent"]).all()
    assert float(got[1].max()) <= GRAD_TOL, got[1].tolist()                              # sample 1: the truth
    assert float(got[0, [0, 1, 2, 4, 5]].max()) <= GRAD_TOL, got[0].tolist()             # sample 0, 3x3 layers' zero styles included: the truth
    assert float(got_z[0].max()) <= GRAD_TOL, got_z.tolist()                             # row 3: the truth without the ToRGB channels' dL/ds
    assert float(lost[0, 3]) > 10 * GRAD_TOL and float(got[0, 3]) > 10 * GRAD_TOL, (lost.tolist(), got.tolist())     # ... whose share is well above the bound
    err_f = _per_sample(run["d_features"], t64["d_features"])
    assert float(err_f[0].max()) <= GRAD_TOL and float(err_f[1].max()) <= GRAD_TOL
