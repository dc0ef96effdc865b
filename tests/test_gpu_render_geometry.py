"""The SIREN render kernels (csrc/siren16.h, siren.hip, siren_bwd.hip, siren16_bwd.h) against the float64 oracle over the ray /
sample geometries and the opacity regimes the other render tests do not reach.

A. GEOMETRY restates the launcher's choice of R (rays per workgroup, pick_rays_per_wg in csrc/siren.hip) and records, per case, what
   follows from it: rays in an image's last workgroup, 128-point sub-tiles per workgroup, points in the last sub-tile.  The restatement
   is checked against the library through e3dge_siren_backbone_bytes (no GPU needed), and a coverage test names every class of case.
B. Forward at every geometry and forward mode against oracle/renderer_ref.py in float64 and float32, with the bounds of
   test_gpu_renderer.check_against_golden: |hip - oracle32| <= ATOL[k], |hip - f64| <= max(3 |oracle32 - f64|, ATOL[k] / 2).
C. Opacity: sigmoid_beta in {0.1, 0.003, 0.001, 1.0} (transparent / half absorbed / absorbed with alpha -> 1 / mask all zero; the
   float64 oracle is asserted to BE in the regime before anything runs on the GPU).  The compositing alone -- volume_integration in
   float64 on the kernel's own per-point values -- and end to end.
D. d(styles) of render losses in every backward mode against float64 autograd of the oracle, at the geometries and regimes above,
   with the bounds of test_gpu_backward.test_render_backward_vs_oracle_autograd: e <= max(5e-5, 2 e32) and e <= 4 e32 + 2e-5, e32
   the fp32 oracle's own relative distance to float64 (required <= 1e-3: a bound that follows a useless oracle is vacuous).

Every render under test runs with torch.empty handing out NaN-filled memory (outputs, saved state with its padded rows, workspaces):
what a kernel leaves unwritten, or reads without having written it, shows up as NaN.

Cost: the float64 / float32 oracle runs on the CPU, once per (case, sigmoid_beta), shared by the modes.  The two large forward
cases (24x24x21 x 3 = 36,288 and 48x48x16 = 36,864 points) take 2-3 s each there; every other case well under a second.  The whole
file: about 10 s on the GPU machine."""
import contextlib
import math

import pytest
import torch

from conftest import contraction_modes, full_state_dict, maxerr, record
from oracle import renderer_ref
from test_gpu_backward import RENDER_KEYS, oracle_render_grads, rel_err, render_loss
from test_gpu_renderer import ATOL, make_renderer

import e3dge_amd  # noqa: F401
from e3dge_amd import synthetic as syn
from e3dge_amd.camera_utils import generate_camera_params
from e3dge_amd.volume_renderer import BWD_MODES

DEV = "cuda:0"
gpu = pytest.mark.gpu

# ----------------------------------------------------------------------------------------------------------------
# A. geometry
# ----------------------------------------------------------------------------------------------------------------
K_RMAX, K_TILE_PTS, K_MIN_SAMPLES = 16, 128, 16      # kRMax, kTilePts, kMinSamples (csrc/siren_common.h)
K16_SLAB_WORDS = 8 * 2 * 64                          # k16SlabWords (csrc/siren16.h): u32x4 per wave slab of the layer-7 record


def pick_rays_per_wg(S, total_rays):
    """csrc/siren.hip, operation by operation (double arithmetic there as here)."""
    best, best_cost = 1, 1e30
    for R in range(1, K_RMAX + 1):
        pts = R * S
        nsub = (pts + K_TILE_PTS - 1) // K_TILE_PTS
        pad = float(nsub * K_TILE_PTS) / pts
        wgs = (total_rays + R - 1) // R
        rounds = (wgs + 255) // 256
        fill = float(rounds * 256) / float(wgs)
        cost = pad * fill * (1.0 + 0.02 / nsub)
        if cost < best_cost - 1e-12:
            best_cost, best = cost, R
    return best


def geometry(res, S, B):
    """(R, rays in the last workgroup of an image, sub-tiles per workgroup, points in a full workgroup's last sub-tile, workgroups per image)."""
    hw = res * res
    R = min(pick_rays_per_wg(S, hw * B), hw)
    tiles = (hw + R - 1) // R
    subs = (R * S + K_TILE_PTS - 1) // K_TILE_PTS
    return R, hw - (tiles - 1) * R, subs, R * S - (subs - 1) * K_TILE_PTS, tiles


# (res, S, B): (R, rays in last wg, sub-tiles, points in last sub-tile, backward too?)
GEOMETRY = {
    (5, 16, 1): (8, 1, 1, 128, True),       # S = kMinSamples; a 16-point slab is one ray exactly; one-ray last workgroup
    (5, 17, 2): (7, 4, 1, 119, True),       # every slab straddles two rays; 425 points per image: saved rows are padded
    (9, 33, 1): (2, 1, 1, 66, True),        # R = 2
    (13, 31, 1): (4, 1, 1, 124, True),      # R = 4, odd S
    (12, 24, 3): (5, 4, 1, 120, True),      # R = 5, B = 3
    (6, 65, 1): (1, 1, 1, 65, True),        # transmittance scan in two 64-lane passes (64 + 1)
    (5, 129, 1): (1, 1, 2, 1, True),        # ray carried across a sub-tile, last sub-tile one point
    (3, 300, 1): (1, 1, 3, 44, True),       # ray over three sub-tiles, five scan passes
    (24, 21, 3): (11, 4, 2, 103, False),    # R = 11
    (48, 16, 1): (13, 3, 2, 80, False),     # R = 13, 178 workgroups
    (7, 21, 2): (6, 1, 1, 126, True),       # the opacity shape: R = 6, one-ray last workgroup, 1029 points per image (padded saved rows)
}
CASES = list(GEOMETRY)
BWD_CASES = [c for c in CASES if GEOMETRY[c][4]]
OPACITY_SHAPES = [(5, 17, 2), (7, 21, 2)]
BETAS = [0.1, 0.003, 0.001, 1.0]
RAGGED_B2 = [(5, 17, 2), (7, 21, 2)]                 # points per image no multiple of 16, B = 2
LOCS = [[0.2, -0.1], [-0.25, 0.1], [0.3, 0.15]]      # off-centre, different per image
STYLE_SEED = 3
FWD_MODES = contraction_modes("f16x3", "f32")
BACKWARD_MODES = contraction_modes(*BWD_MODES)       # every backward mode the loaded library has: a new default cannot be skipped
OUT_KEYS = tuple(ATOL) + ('dists', 'mask')
_id = lambda c: "x".join(str(v) for v in c)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_geometry_table_matches_the_launcher(lib, case):
    res, S, B = case
    R, rays_last, subs, pts_last, tiles = geometry(res, S, B)
    assert (R, rays_last, subs, pts_last) == GEOMETRY[case][:4]
    assert lib.e3dge_siren_backbone_bytes(B, res, res, S) == tiles * B * subs * 8 * K16_SLAB_WORDS * 16


def test_geometry_table_covers_every_class():
    g = {c: geometry(*c) for c in CASES}
    assert {1, 2, 4, 5, 6, 7, 8, 11, 13} <= {v[0] for v in g.values()}, "rays per workgroup"
    assert any(S == K_MIN_SAMPLES for _, S, _ in g), "S = kMinSamples"
    assert any(64 < S <= 128 for _, S, _ in g), "a scan in two passes inside one sub-tile"
    assert any(S > 128 and v[2] >= 3 for (_, S, _), v in g.items()), "a ray over three sub-tiles"
    assert any(v[1] < v[0] for v in g.values()), "a short last workgroup"
    assert any((res * res * S) % 16 and B >= 2 for res, S, B in g), "padded saved rows between two images"
    assert any(v[3] == 1 for v in g.values()), "a last sub-tile of one point"
    for c in ((24, 21, 3), (48, 16, 1)):
        assert c in g and not GEOMETRY[c][4]
    assert set(BWD_CASES) >= set(CASES) - {(24, 21, 3), (48, 16, 1)}
    assert set(OPACITY_SHAPES) <= set(BWD_CASES) and (7, 21, 2) in OPACITY_SHAPES and set(RAGGED_B2) <= set(OPACITY_SHAPES)
    assert {"f16x3", "f32", "f16x3_g2"} <= set(BACKWARD_MODES)


# ----------------------------------------------------------------------------------------------------------------
# inputs and the oracle (CPU; computed once per key, never modified)
# ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd():
    return full_state_dict()[1]


def with_beta(sd, beta):
    out = dict(sd)
    out['renderer.sigmoid_beta'] = torch.full_like(sd['renderer.sigmoid_beta'], beta)
    return out


def inputs(case, image=None):
    """Cameras and styles on the CPU; image = i: that image of the batch alone."""
    res, S, B = case
    cams = generate_camera_params(res, 'cpu', batch=B, locations=torch.tensor(LOCS[:B]))[:4]
    wr = syn.synthetic_inputs(B, seed=STYLE_SEED)[0]
    if image is not None:
        cams, wr = tuple(c[image:image + 1].contiguous() for c in cams), wr[image:image + 1].contiguous()
    return cams, wr


_ORACLE = {}


def oracle(sd, case, beta, image=None):
    """{float64: dict, float32: dict} of renderer_ref.render."""
    key = (case, beta, image)
    if key not in _ORACLE:
        (poses, focal, near, far), wr = inputs(case, image)
        with torch.no_grad():
            _ORACLE[key] = {dt: renderer_ref.render(with_beta(sd, beta), poses, focal, near, far, wr, res=case[0], n_samples=case[1], dtype=dt)
                            for dt in (torch.float64, torch.float32)}
    return _ORACLE[key]


def regime_stats(o64, beta):
    """Of a float64 oracle render: fraction of absorbed rays (forced-background weight < 1e-3), max alpha in front of the forced last
    sample, mean of mask, smallest last weight."""
    sigma = torch.sigmoid(-o64['sdf'][..., 0] / beta) / beta
    alpha = 1 - torch.exp(-sigma * o64['dists'])
    last = o64['hit_prob'][..., -1, 0]
    return dict(absorbed=float((last < 1e-3).double().mean()), max_alpha=float(alpha[..., :-1].max()),
                mask_mean=float(o64['mask'].mean()), min_last_weight=float(last.min()))


def assert_regime(beta, st):
    """Conditions on the inputs, not measurements of the code under test."""
    if beta == 0.003:
        assert 0.2 <= st['absorbed'] <= 0.6 and 0.0 < st['mask_mean'] < 1.0, st
    elif beta == 0.001:
        assert st['absorbed'] >= 0.6 and st['max_alpha'] > 0.999, st
    elif beta == 1.0:
        assert st['mask_mean'] == 0.0 and st['max_alpha'] < 0.05, st
    else:
        assert beta == 0.1 and st['absorbed'] == 0.0, st


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("case", OPACITY_SHAPES, ids=_id)
def test_opacity_inputs_are_in_their_regime(sd, case, beta):
    assert_regime(beta, regime_stats(oracle(sd, case, beta)[torch.float64], beta))


# ----------------------------------------------------------------------------------------------------------------
# helpers of the GPU tests
# ----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def nan_filled_empty():
    """torch.empty (as the package calls it for outputs, saved state and workspaces) returns NaN-filled floating-point memory.
    Yields the list of the shapes it filled; a block that filled none fails (the pre-fill would be checking nothing)."""
    real, filled = torch.empty, []

    def empty(*a, **k):
        t = real(*a, **k)
        if t.is_floating_point():
            filled.append(tuple(t.shape))
            t.fill_(float('nan'))
        return t
    torch.empty = empty
    try:
        yield filled
    finally:
        torch.empty = real
    assert filled, "no allocation went through torch.empty: the NaN pre-fill did not reach the launch"


def on_gpu(cams, wr):
    return tuple(c.to(DEV) for c in cams), wr.to(DEV)


def check_forward(name, out, o, absolute=True, extra=None):
    """The bounds of test_gpu_renderer.check_against_golden against the oracle pair o; one report row per key.  Returns the worst
    ratio of an error to its bound."""
    o64, o32 = o[torch.float64], o[torch.float32]
    worst, failures = 0.0, []
    for k, atol in ATOL.items():
        e32, e64, ref = maxerr(out[k], o32[k]), maxerr(out[k], o64[k]), maxerr(o32[k], o64[k])
        bound = max(3 * ref, 0.5 * atol)
        record(f"{name}:{k}", hip_vs_f64=e64, oracle32_vs_f64=ref, bound=bound, hip_vs_oracle32=e32, **(extra or {}))
        assert math.isfinite(e64) and math.isfinite(e32), (name, k)
        worst = max(worst, e64 / bound, e32 / atol if absolute else 0.0)
        if absolute and e32 > atol:
            failures.append(f"{name}:{k} |hip-oracle32| = {e32:.3e} > {atol:.1e}")
        if e64 > bound:
            failures.append(f"{name}:{k} |hip-f64| = {e64:.3e} > {bound:.3e} (fp32 oracle: {ref:.3e})")
    d, d32 = out['dists'].double().cpu(), o32['dists'].double()
    rel = float(((d - d32).abs() / d32.abs().clamp_min(1e-12)).max())
    record(f"{name}:dists", hip_rel_vs_oracle32=rel, bound=2e-5)
    if not rel <= 2e-5:            # differences of nearby z values: a few ulp of z relative to dz
        failures.append(f"{name}:dists rel = {rel:.3e}")
    m = out['mask'].cpu()
    near_thr = (o32['depth'].reshape(m.shape) - 1.08).abs() < 1e-5
    differs = m != o32['mask']
    record(f"{name}:mask", differs=int(differs.sum()), differs_away_from_threshold=int((differs & ~near_thr).sum()), bound=0,
           mask_mean=float(m.mean()))
    if bool((differs & ~near_thr).any()):
        failures.append(f"{name}:mask")
    assert not failures, failures
    return worst


def check_invariants(name, out):
    for k in OUT_KEYS:
        assert torch.isfinite(out[k]).all(), f"{name}:{k} holds NaN / inf (an element the kernel did not write?)"
    w = out['hit_prob'][..., 0].double()
    assert float((w.sum(-1) - 1).abs().max()) <= 3e-6, name
    assert float(w.min()) >= -1e-6, (name, float(w.min()))      # (the float64 reference itself reaches -1.4e-9 on the forced last sample)
    assert torch.equal(out['mask'][:, 0, :, :, 0], (out['depth'][..., 0, 0] < 1.08).float()), name


# ----------------------------------------------------------------------------------------------------------------
# B. forward at every geometry
# ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", FWD_MODES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_against_float64_at_every_geometry(sd, case, mode):
    res, S, B = case
    name = f"geom_fwd_{_id(case)}_{mode}"
    o = oracle(sd, case, 0.1)
    cams, wr = on_gpu(*inputs(case))
    r = make_renderer(sd, res, S, mfma_mode=mode)
    with torch.no_grad(), nan_filled_empty() as filled:
        out = r(*cams, styles=wr)
    assert tuple(out['hit_prob'].shape) == (B, res, res, S, 1) and tuple(out['features'].shape) == (B, 256, res, res)
    assert {tuple(out[k].shape) for k in OUT_KEYS} <= set(filled), "an output was not pre-filled"
    check_invariants(name, out)
    check_forward(name, out, o)
    # the saving launch (point-major, and slab-major beside the f16x3 forward) returns the same bits
    n16 = (res * res * S + 15) // 16 * 16
    for bwd in [mode] + (["f16x3_g2"] if mode == "f16x3" else []):
        r.siren.bwd_mode = bwd
        with nan_filled_empty() as filled:
            tr = r(*cams, styles=wr.clone().requires_grad_(True))
        assert (B, n16, 9, 256) in filled, "the saved state (rows of an image padded to 16) was not pre-filled"
        for k in OUT_KEYS:
            assert torch.equal(out[k], tr[k].detach()), f"{name}: saving launch ({bwd}) differs in {k}"
        assert tr['features'].requires_grad and not tr['mask'].requires_grad
    # image 1 alone: other R, other sub-tile cuts, so the same bound and no bit-equality
    if B >= 2:
        c1, w1 = on_gpu(*inputs(case, image=1))
        with torch.no_grad(), nan_filled_empty():
            alone = r(*c1, styles=w1)
        check_invariants(name + "_image1", alone)
        check_forward(name + "_image1", alone, oracle(sd, case, 0.1, image=1))


# ----------------------------------------------------------------------------------------------------------------
# C. opacity regimes
# ----------------------------------------------------------------------------------------------------------------
VI_KEYS = dict(hit_prob='weights', depth='depth', xyz='xyz', gen_thumb_imgs='rgb_map', features='feat_map')


def composite_of(out, raw, z, beta, dtype):
    """renderer_ref.volume_integration on the kernel's own per-point values, in the layouts of the render dict."""
    c = lambda t: t.detach().cpu().to(dtype)
    vi = renderer_ref.volume_integration(c(raw), c(z), c(out['rays_d']), c(out['points']), torch.tensor([beta], dtype=dtype))
    res = {k: vi[v] for k, v in VI_KEYS.items()}
    for k in ('xyz', 'gen_thumb_imgs', 'features'):
        res[k] = res[k].permute(0, 3, 1, 2).contiguous()
    res['mask'] = vi['mask'].permute(0, 4, 1, 2, 3).contiguous()
    return res


@gpu
@pytest.mark.parametrize("mode", FWD_MODES)
@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("case", OPACITY_SHAPES, ids=_id)
def test_opacity_regimes_forward(sd, case, beta, mode):
    res, S, B = case
    name = f"opacity_fwd_{_id(case)}_beta{beta:g}_{mode}"
    o = oracle(sd, case, beta)
    stats = regime_stats(o[torch.float64], beta)
    assert_regime(beta, stats)
    cams, wr = on_gpu(*inputs(case))
    r = make_renderer(with_beta(sd, beta), res, S, mfma_mode=mode)
    with torch.no_grad(), nan_filled_empty():
        out = r(*cams, styles=wr)
        raw = r.run_network(out['points'], out['viewdirs'], styles=wr)
    check_invariants(name, out)
    # 1. compositing alone: rgb / features of the point query, the render's own sdf, points, ray directions and z
    sdf_gap = maxerr(raw[..., 3:4], out['sdf'])
    if sdf_gap:
        record(name + ":sdf_render_vs_query", distance=sdf_gap, bound=ATOL['sdf'])
        assert sdf_gap <= ATOL['sdf'], sdf_gap
    raw = torch.cat([raw[..., :3], out['sdf'], raw[..., 4:]], -1)
    near, far = cams[2], cams[3]
    z = (near.reshape(B, 1, 1, 1) * (1 - r.t_vals) + far.reshape(B, 1, 1, 1) * r.t_vals).expand(B, res, res, S)
    assert maxerr(out['points'], out['rays_o'].unsqueeze(3) + out['rays_d'].unsqueeze(3) * z.unsqueeze(-1)) <= 2e-7
    vi64, vi32 = composite_of(out, raw, z, beta, torch.float64), composite_of(out, raw, z, beta, torch.float32)
    failures = []
    for k in VI_KEYS:
        e, ref = maxerr(out[k], vi64[k]), maxerr(vi32[k], vi64[k])
        bound = max(3 * ref, 0.5 * ATOL[k])
        record(f"{name}:composite:{k}", hip_vs_f64=e, oracle32_vs_f64=ref, bound=bound, **stats)
        if not e <= bound:
            failures.append(f"{name}:composite:{k} {e:.3e} > {bound:.3e} (float32 compositing: {ref:.3e})")
    near_thr = (vi32['depth'].reshape(out['mask'].shape) - 1.08).abs() < 1e-5
    differs = out['mask'].cpu() != vi32['mask']
    record(f"{name}:composite:mask", differs=int(differs.sum()), differs_away_from_threshold=int((differs & ~near_thr).sum()), bound=0, **stats)
    if bool((differs & ~near_thr).any()):
        failures.append(f"{name}:composite:mask")
    assert not failures, failures
    # 2. end to end (the absolute ATOL against the fp32 oracle was measured at 0.1: asserted there only)
    check_forward(name, out, o, absolute=(beta == 0.1), extra=stats)


# ----------------------------------------------------------------------------------------------------------------
# D. backward
# ----------------------------------------------------------------------------------------------------------------
_TRUTH = {}


def render_grad_truth(sd, case, beta, keys, image=None):
    """(G, float64 d styles, float32 d styles) of sum_k <out[k], G_k> from autograd of the oracle."""
    key = (case, beta, keys, image)
    if key not in _TRUTH:
        cams, wr = inputs(case, image)
        res, S, B = case
        shapes = dict(gen_thumb_imgs=(3, res, res), features=(256, res, res), xyz=(3, res, res), depth=(res, res, 1, 1),
                      sdf=(res, res, S, 1), hit_prob=(res, res, S, 1))
        gen = torch.Generator().manual_seed(res * 1000 + S + 7 * len(keys))
        G = {k: torch.randn((wr.shape[0],) + shapes[k], generator=gen) for k in keys}
        sdb = with_beta(sd, beta)
        _TRUTH[key] = (G, oracle_render_grads(sdb, cams, wr, G, res, S, torch.float64),
                       oracle_render_grads(sdb, cams, wr, G, res, S, torch.float32))
    return _TRUTH[key]


def check_backward(name, sd, r, case, beta, keys, image=None, extra=None):
    G, truth, ref32 = render_grad_truth(sd, case, beta, keys, image)
    cams, wr = on_gpu(*inputs(case, image))
    styles = wr.clone().requires_grad_(True)
    with nan_filled_empty():
        out = r(*cams, styles=styles)
        render_loss(out, {k: v.to(DEV) for k, v in G.items()}).backward()
    assert torch.isfinite(styles.grad).all(), f"{name}: gradient holds NaN / inf"
    e, e32 = rel_err(styles.grad, truth), rel_err(ref32, truth)
    bound = min(max(5e-5, 2 * e32), 4 * e32 + 2e-5)
    record(name, hip_vs_f64=e, oracle32_vs_f64=e32, bound=bound, **(extra or {}))
    assert e32 <= 1e-3, (name, e32)               # condition on the inputs: the fp32 oracle is a usable yardstick here
    assert e <= max(5e-5, 2 * e32), (name, e, e32)
    assert e <= 4 * e32 + 2e-5, (name, e, e32)
    return e / bound


BWD_PARAMS = [(c, 0.1) for c in BWD_CASES if c not in OPACITY_SHAPES] + [(c, b) for c in OPACITY_SHAPES for b in BETAS]


@gpu
@pytest.mark.parametrize("mode", BACKWARD_MODES)
@pytest.mark.parametrize("case,beta", BWD_PARAMS, ids=[f"{_id(c)}-beta{b:g}" for c, b in BWD_PARAMS])
def test_backward_against_float64_autograd(sd, case, beta, mode):
    res, S, B = case
    name = f"geom_bwd_{_id(case)}_beta{beta:g}_{mode}"
    extra = None
    if case in OPACITY_SHAPES:
        extra = regime_stats(oracle(sd, case, beta)[torch.float64], beta)
        assert_regime(beta, extra)
    r = make_renderer(with_beta(sd, beta), res, S, mfma_mode=mode)
    check_backward(name + ":" + "+".join(RENDER_KEYS), sd, r, case, beta, RENDER_KEYS, extra=extra)
    if case in OPACITY_SHAPES:
        # on their own: next to the network's large shared terms these two would hide
        check_backward(name + ":xyz+depth", sd, r, case, beta, ('xyz', 'depth'), extra=extra)
        check_backward(name + ":hit_prob", sd, r, case, beta, ('hit_prob',), extra=extra)
    if case in RAGGED_B2:
        # image 1 alone: its saved rows start where the batched launch put the padding behind image 0
        check_backward(name + ":image1:" + "+".join(RENDER_KEYS), sd, r, case, beta, RENDER_KEYS, image=1)
