"""GPU: the fused FiLM-SIREN renderer through the C-ABI against (i) the golden vectors recorded from the
reference, (ii) the float64 evaluation of the restatement ("truth") and (iii) the oracle on other inputs.

Stated fp32 tolerance.  The reference's own fp32 result sits this far from the float64 truth on these fixtures
(tests/golden/generation_report.json): rgb 1e-6, depth/xyz 3e-7, weights 7e-7, sdf 3e-6, 256-ch features 6e-5
(eight sine layers at frequency ~30 amplify rounding by ~1.7x per layer).  A different but equally valid fp32
summation order (MFMA k-order instead of MKL's) lands at the same distance, so the bound on |hip - reference| is
about that noise floor (measured on MI355X, round 1: rgb 5e-7, weights 4e-7, sdf 8e-7, features 1.1e-5, geometry
bit-exact); the stated fp32 tolerance leaves ~5-10x margin over the measurement:
    rgb 5e-6 | depth, xyz, weights 4e-6 | sdf 1e-5 | features 1e-4 | geometry (points, rays, dirs) 5e-7.
The distance to the float64 truth is additionally required to stay within 3x the reference's own."""
import numpy as np
import pytest
import torch

from conftest import contraction_modes, full_state_dict, load_golden, maxerr, record
from oracle import renderer_ref

import e3dge_amd  # noqa: F401
from e3dge_amd import synthetic as syn
from e3dge_amd.camera_utils import generate_camera_params
from e3dge_amd.volume_renderer import VolumeFeatureRenderer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.asarray(a)).to(DEV)

ATOL = dict(gen_thumb_imgs=5e-6, depth=4e-6, xyz=4e-6, hit_prob=4e-6, sdf=1e-5, features=1e-4, points=5e-7,
            rays_d=5e-7, viewdirs=5e-7)


@pytest.fixture(scope="module")
def sd():
    return full_state_dict()[1]


MODES = contraction_modes("f16x3", "f32", "f16x3_v1")     # every contraction kernel must meet the same bounds


def make_renderer(sd, res, S, mfma_mode=None, **over):
    r = VolumeFeatureRenderer(syn.rendering_opt(N_samples=S, **over), out_im_res=res, mode='test')
    if mfma_mode is not None:
        # 'f16x3_g2' names the backward-type kernels (8-wave layout, in every build, the default training path): forward stays f16x3
        r.siren.mfma_mode = "f16x3" if mfma_mode == "f16x3_g2" else mfma_mode
        r.siren.bwd_mode = mfma_mode          # the backward-type kernels run in the same mode
    pre = 'network.netGlobal.' if over.get('enable_local_model') else 'network.'
    own = {}
    for k in r.state_dict():
        src = 'renderer.' + (k.replace('network.netGlobal.', 'network.') if pre != 'network.' else k)
        own[k] = sd[src]
    r.load_state_dict(own)
    r.requires_grad_(False)        # frozen generator, as in encoder training (trainer.py:1568): gradients go to the styles
    return r.to(DEV)


def check_against_golden(name, out, g, sub=None):
    errs = {}
    for k, atol in ATOL.items():
        v = out[k]
        if sub and k in ('sdf', 'hit_prob', 'points'):
            v = v[:, ::sub, ::sub]
        if sub and k == 'features':
            v = v[:, :, ::sub, ::sub]
        e_ref = maxerr(v, g['ref_' + k])
        e_f64 = maxerr(v, g['f64_' + k])
        ref_f64 = maxerr(g['ref_' + k], g['f64_' + k])
        errs[k] = (e_ref, e_f64, ref_f64)
    record(name, **{k + '_vs_ref': v[0] for k, v in errs.items()}, **{k + '_vs_f64': v[1] for k, v in errs.items()},
           **{k + '_ref_vs_f64': v[2] for k, v in errs.items()})
    for k, (e_ref, e_f64, ref_f64) in errs.items():
        assert e_ref <= ATOL[k], f"{name}:{k} |hip-ref| = {e_ref:.3e} > {ATOL[k]:.1e}"
        assert e_f64 <= max(3 * ref_f64, 0.5 * ATOL[k]), f"{name}:{k} |hip-f64| = {e_f64:.3e} vs reference's {ref_f64:.3e}"
    # dists: last interval is 1e10 * |d| -> relative bound
    d = out['dists'][:, ::sub, ::sub] if sub else out['dists']
    rel = float(((d.double().cpu() - torch.from_numpy(g['ref_dists']).double()).abs() /
                 torch.from_numpy(g['ref_dists']).double().abs().clamp_min(1e-12)).max())
    assert rel <= 2e-5, rel     # differences of nearby z values: a few ulp of z relative to dz = 0.01
    m = out['mask'].cpu().numpy()
    near_thr = np.abs(g['ref_depth'].reshape(m.shape) - 1.08) < 1e-5
    assert ((m == g['ref_mask']) | near_thr).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,sub", [("renderer_16x24", None), ("renderer_8x48", None), ("renderer_8x18", None),
                                      ("renderer_64x24", 8)])
def test_render_matches_reference_golden(sd, name, sub, mode):
    g = load_golden(name)
    B, res, S = int(g['batch']), int(g['res']), int(g['n_samples'])
    r = make_renderer(sd, res, S, mfma_mode=mode)
    wr, _ = syn.synthetic_inputs(B, seed=int(g['styles_seed']), device=DEV)
    with torch.no_grad():
        out = r(T(g['poses']), T(g['focal']), T(g['near']), T(g['far']), styles=wr)
    # dict surface of VolumeFeatureRenderer.forward
    assert set(out) >= {'rays_o', 'rays_d', 'dists', 'near', 'far', 'hit_prob', 'surface_eikonal_term', 'points', 'sdf',
                        'gen_thumb_imgs', 'features', 'mask', 'xyz', 'eikonal_term', 'depth', 'mesh', 'viewdirs'}
    assert tuple(out['gen_thumb_imgs'].shape) == (B, 3, res, res) and tuple(out['features'].shape) == (B, 256, res, res)
    assert tuple(out['mask'].shape) == (B, 1, res, res, 1) and tuple(out['depth'].shape) == (B, res, res, 1, 1)
    assert tuple(out['sdf'].shape) == (B, res, res, S, 1) and tuple(out['points'].shape) == (B, res, res, S, 3)
    assert tuple(out['near'].shape) == (B, res, res, 1) and tuple(out['rays_o'].shape) == (B, res, res, 3)
    check_against_golden(name + ':' + mode, out, g, sub)


@pytest.mark.parametrize("mode", MODES)
def test_texture_film_pass(sd, mode):
    g = load_golden("renderer_tex_8x24")
    r = make_renderer(sd, 8, 24, mfma_mode=mode, enable_local_model=True)
    wr, _ = syn.synthetic_inputs(1, seed=1, device=DEV)
    tex = syn.synthetic_tex_conditions(1, 8, 24, seed=int(g['tex_seed']), device=DEV)
    with torch.no_grad():
        out = r(T(g['poses']), T(g['focal']), T(g['near']), T(g['far']), styles=wr, local_data_batch={'tex': tex})
    e = {k: maxerr(out[k], g['ref_' + k]) for k in ('gen_thumb_imgs', 'features', 'sdf', 'hit_prob')}
    record("tex_film:" + mode, **e)
    for k, v in e.items():
        assert v <= ATOL[k], (k, v)


@pytest.mark.parametrize("mode", MODES)
def test_film_params_and_point_queries(sd, mode):
    g = load_golden("points")
    r = make_renderer(sd, 64, 24, mfma_mode=mode)
    wr, _ = syn.synthetic_inputs(2, seed=1, device=DEV)
    film = r.siren.film_params(wr)
    e_film = maxerr(film, g['ref_film'])
    record("film_params", vs_ref=e_film, vs_f64=maxerr(film, g['f64_film']), ref_vs_f64=maxerr(g['ref_film'], g['f64_film']))
    assert e_film <= 1e-5          # gamma ~ 30 +- 15*dot(256): a few ulp of 30 (ulp = 2e-6); measured 1.9e-6
    pts, vd = T(g['pts']), T(g['viewdirs'])
    with torch.no_grad():
        raw0 = r.run_network(pts, torch.zeros_like(pts), styles=wr)
        raw1 = r.run_network(pts, vd, styles=wr)
        sdf_only = r.run_network(pts, torch.zeros_like(pts), styles=wr, return_sdf_only=True)
    assert tuple(raw1.shape) == tuple(g['ref_raw_view'].shape)
    for tag, raw, ref in (("zero_view", raw0, g['ref_raw_zero_view']), ("view", raw1, g['ref_raw_view'])):
        e = dict(rgb=maxerr(raw[..., :3], ref[..., :3]), sdf=maxerr(raw[..., 3], ref[..., 3]), feat=maxerr(raw[..., 4:], ref[..., 4:]))
        record("points_" + tag + ":" + mode, **e)
        assert e['rgb'] <= 5e-6 and e['sdf'] <= 1e-5 and e['feat'] <= 1e-4, e
    assert maxerr(sdf_only[..., 0], raw0[..., 3]) == 0.0


@pytest.mark.parametrize("mode", MODES)
def test_full_size_properties_64x64x24(sd, mode):
    """BASELINE.json configs[1] size: invariants that need no oracle."""
    res, S, B = 64, 24, 3
    r = make_renderer(sd, res, S, mfma_mode=mode)
    wr, _ = syn.synthetic_inputs(B, seed=11, device=DEV)
    loc = torch.tensor([[0.0, 0.0], [0.25, -0.1], [-0.3, 0.12]])
    poses, focal, near, far, _ = generate_camera_params(res, DEV, locations=loc.to(DEV))
    with torch.no_grad():
        out = r(poses, focal, near, far, styles=wr)
        again = r(poses, focal, near, far, styles=wr)
        single = r(poses[1:2], focal[1:2], near[1:2], far[1:2], styles=wr[1:2])
    for k in ('gen_thumb_imgs', 'features', 'sdf', 'hit_prob', 'depth', 'xyz'):
        assert torch.isfinite(out[k]).all(), k
        assert torch.equal(out[k], again[k]), f"{k}: two identical launches differ (non-deterministic reduction?)"
        assert torch.equal(out[k][1:2], single[k]), f"{k}: batch element 1 differs from its stand-alone render"
    w = out['hit_prob'][..., 0]
    assert float((w.sum(-1) - 1).abs().max()) <= 2e-6          # force_background: weights of a ray sum to one
    z = near.reshape(B, 1, 1, 1) * (1 - r.t_vals) + far.reshape(B, 1, 1, 1) * r.t_vals
    assert maxerr(out['points'], out['rays_o'].unsqueeze(3) + out['rays_d'].unsqueeze(3) * z.unsqueeze(-1)) <= 2e-7
    assert maxerr(out['depth'][..., 0, 0], (w * z).sum(-1)) <= 1e-6
    assert torch.equal(out['mask'][:, 0, :, :, 0], (out['depth'][..., 0, 0] < 1.08).float())
    assert float(out['gen_thumb_imgs'].abs().max()) <= 1.0 + 1e-6
    # against the oracle (fp32, CPU) on the second image
    cpu = lambda t: t.detach().cpu()
    with torch.no_grad():
        ref = renderer_ref.render(sd, cpu(poses[1:2]), cpu(focal[1:2]), cpu(near[1:2]), cpu(far[1:2]), cpu(wr[1:2]), res=res, n_samples=S)
    e = {k: maxerr(single[k], ref[k]) for k in ATOL}
    record("full_64x64x24_vs_oracle:" + mode, **e)
    for k, v in e.items():
        assert v <= ATOL[k], (k, v)


def test_c4_size_128x128x48_against_oracle(sd):
    """BASELINE.json configs[3]: 128x128 rays x 48 samples (786,432 points, the reference's W==128 sub-batch path)."""
    res, S = 128, 48
    r = make_renderer(sd, res, S)
    wr, _ = syn.synthetic_inputs(1, seed=21, device=DEV)
    poses, focal, near, far, _ = generate_camera_params(res, DEV, locations=torch.tensor([[0.45, 0.0]], device=DEV))
    with torch.no_grad():
        out = r(poses, focal, near, far, styles=wr)
        cpu = lambda t: t.detach().cpu()
        ref = renderer_ref.render(sd, cpu(poses), cpu(focal), cpu(near), cpu(far), cpu(wr), res=res, n_samples=S)
    e = {k: maxerr(out[k], ref[k]) for k in ATOL}
    record("c4_128x128x48_vs_oracle", **e)
    for k, v in e.items():
        assert v <= ATOL[k], (k, v)
    assert float((out['hit_prob'][..., 0].sum(-1) - 1).abs().max()) <= 3e-6


def test_geometry_sample_requery(sd):
    r = make_renderer(sd, 16, 24)
    wr, _ = syn.synthetic_inputs(1, seed=1, device=DEV)
    poses, focal, near, far, _ = generate_camera_params(16, DEV, locations=torch.zeros(1, 2, device=DEV))
    rs = np.random.RandomState(9)
    uni = T((0.12 * rs.uniform(-1, 1, (1, 500, 1, 1, 3))).astype(np.float32))
    with torch.no_grad():
        out = r(poses, focal, near, far, styles=wr, geometry_sample={'uniform_pts': uni, 'xyz': None})
        ref = renderer_ref.query_points(sd, uni.cpu(), None, wr.cpu())[..., 3:4]
    assert tuple(out['uniform_pts_rec'].shape) == (1, 500, 1, 1, 1)
    assert maxerr(out['uniform_pts_rec'], ref) <= 1e-5


def test_ragged_and_tiny_extents(sd):
    """Edge cases: one ray block smaller than a tile, a point count that is not a multiple of 128, a single point."""
    r = make_renderer(sd, 8, 18)       # 64 rays x 18 = 1152 points
    wr, _ = syn.synthetic_inputs(1, seed=3, device=DEV)
    for n in (1, 127, 129, 1000):
        pts = T((0.1 * np.random.RandomState(n).uniform(-1, 1, (1, n, 1, 1, 3))).astype(np.float32))
        with torch.no_grad():
            raw = r.run_network(pts, torch.zeros_like(pts), styles=wr)
            ref = renderer_ref.query_points(sd, pts.cpu(), None, wr.cpu())
        assert maxerr(raw[..., 3], ref[..., 3]) <= 1e-5 and maxerr(raw[..., 4:], ref[..., 4:]) <= 1e-4, n
    empty = r.run_network(torch.empty(1, 0, 1, 1, 3, device=DEV), torch.empty(1, 0, 1, 1, 3, device=DEV), styles=wr)
    assert empty.numel() == 0


def test_f16x3_weight_range_falls_back_to_fp32(sd):
    """The split-f16 weight image holds 128*w as f16: a module whose weights exceed that range is served by the fp32 MFMA
    kernel automatically (one warning), with the same parity."""
    r = make_renderer(sd, 8, 18, mfma_mode="f16x3")
    wr, _ = syn.synthetic_inputs(1, seed=1, device=DEV)
    poses, focal, near, far, _ = generate_camera_params(8, DEV, locations=torch.zeros(1, 2, device=DEV))
    with torch.no_grad():
        r.siren.pts_linears[3].weight[5, 7] = 300.0
        with pytest.warns(UserWarning, match="fp32 MFMA"):
            out = r(poses, focal, near, far, styles=wr)
        r.siren.mfma_mode = "f32"                                         # what it fell back to, asked for explicitly
        out32 = r(poses, focal, near, far, styles=wr)
    assert torch.isfinite(out['features']).all()
    # (a weight of 300 makes the network chaotic, so the comparison is with the fp32 kernel itself, not with the oracle)
    assert torch.equal(out['features'], out32['features']) and torch.equal(out['sdf'], out32['sdf'])


def test_weight_cache_sees_updates_and_invalidate(sd):
    """The packed weight image follows parameter updates: in-place ops on the parameter are detected through its version
    counter; writes through `.data` (the reference's EMA accumulate(), utils/training_utils.py:45) are not, and need
    renderer.invalidate() -- after which the output changes."""
    r = make_renderer(sd, 8, 18)
    wr, _ = syn.synthetic_inputs(1, seed=1, device=DEV)
    poses, focal, near, far, _ = generate_camera_params(8, DEV, locations=torch.zeros(1, 2, device=DEV))
    with torch.no_grad():
        base = r(poses, focal, near, far, styles=wr)['features'].clone()
        r.siren.pts_linears[2].weight.mul_(1.01)                         # versioned in-place update
        v1 = r(poses, focal, near, far, styles=wr)['features'].clone()
        assert not torch.equal(base, v1)
        r.siren.pts_linears[2].weight.data.mul_(1.01)                    # bypasses the version counter
        r.sigmoid_beta.data.mul_(1.5)
        r.invalidate()
        v2 = r(poses, focal, near, far, styles=wr)
        assert not torch.equal(v1, v2['features'])
        sd2 = {k: v.clone() for k, v in sd.items()}
        sd2['renderer.network.pts_linears.2.weight'] *= 1.01 * 1.01
        sd2['renderer.sigmoid_beta'] *= 1.5
        c = lambda t: t.detach().cpu()
        ref = renderer_ref.render(sd2, c(poses), c(focal), c(near), c(far), c(wr), res=8, n_samples=18)
    assert maxerr(v2['features'], ref['features']) <= 1e-4 and maxerr(v2['hit_prob'], ref['hit_prob']) <= 4e-6


def test_grad_to_renderer_weights_is_refused(sd):
    """Under grad mode with trainable SIREN parameters the reference would train them; the HIP backward does not, and says so."""
    r = make_renderer(sd, 8, 18)
    wr, _ = syn.synthetic_inputs(1, seed=1, device=DEV)
    poses, focal, near, far, _ = generate_camera_params(8, DEV, locations=torch.zeros(1, 2, device=DEV))
    for p_ in r.parameters():
        p_.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="frozen"):
        r(poses, focal, near, far, styles=wr.clone().requires_grad_(True))
    for p_ in r.parameters():
        p_.requires_grad_(False)
    out = r(poses, focal, near, far, styles=wr.clone().requires_grad_(True), sample_without_grad=True)
    assert not out['features'].requires_grad                              # :1291-1294: detached outputs


def test_sample_mode_pseudo_ground_truth(sd):
    """sample_mode=True (stage-1 3-D supervision sampling, render_rays :1297-1324 + collate_fn :1976-2043): jittered
    surface points and uniform box points with their sdf, merged into uniform_pts / uniform_points_sdf / valid mask;
    xyz and mask stay channel-last in this mode (:1951-1958).  The random draws are injected to compare with the oracle."""
    res, S, n_grid = 8, 24, 200
    r = make_renderer(sd, res, S, sample_near_surface=True, sample_uniform_grid=True, surface_sampling_stdv=0.03,
                      uniform_grid_sampling_num=n_grid)
    wr, _ = syn.synthetic_inputs(2, seed=4, device=DEV)
    poses, focal, near, far, _ = generate_camera_params(res, DEV, batch=2, locations=torch.tensor([[0.1, 0.0], [-0.2, 0.1]], device=DEV))
    rs = np.random.RandomState(12)
    noise = T(rs.standard_normal((2, res, res, 3)).astype(np.float32))
    uni = T(rs.uniform(size=(2, n_grid, 3)).astype(np.float32))
    with torch.no_grad():
        out = r(poses, focal, near, far, styles=wr, sample_mode=True, surface_noise=noise, grid_uniform=uni)
        plain = r(poses, focal, near, far, styles=wr)
        drawn = r(poses, focal, near, far, styles=wr, sample_mode=True)              # own torch.rand / randn draws
    c = lambda t: t.detach().cpu()
    assert tuple(out['xyz'].shape) == (2, res, res, 3) and tuple(out['mask'].shape) == (2, res, res, 1, 1)
    assert torch.equal(out['xyz'], plain['xyz'].permute(0, 2, 3, 1)) and torch.equal(out['gen_thumb_imgs'], plain['gen_thumb_imgs'])
    n_all = res * res + n_grid
    assert tuple(out['uniform_pts'].shape) == (2, n_all, 1, 1, 3) and tuple(out['uniform_points_sdf'].shape) == (2, n_all, 1, 1, 1)
    assert tuple(out['uniform_points_valid_mask'].shape) == (2, n_all, 1, 1, 1)
    # expected point sets from the same draws
    near_pts = c(out['xyz']) + c(noise) * 0.03
    grid_pts = c(uni) * 0.24 - 0.12
    exp_pts = torch.cat([near_pts.reshape(2, -1, 3), grid_pts], 1)
    assert maxerr(out['uniform_pts'].reshape(2, -1, 3), exp_pts) <= 1e-7
    vd = c(out['viewdirs']).unsqueeze(3)                                             # (B,H,W,1,3)
    with torch.no_grad():
        sdf_near = renderer_ref.query_points(sd, near_pts.unsqueeze(3), vd, c(wr))[..., 3]
        sdf_grid = renderer_ref.query_points(sd, grid_pts.reshape(2, n_grid, 1, 1, 3), None, c(wr))[..., 3]
    exp_sdf = torch.cat([sdf_near.reshape(2, -1), sdf_grid.reshape(2, -1)], 1)
    assert maxerr(out['uniform_points_sdf'].reshape(2, -1), exp_sdf) <= 1e-5
    exp_valid = torch.cat([(near_pts.abs().max(-1)[0] < 0.12).float().reshape(2, -1), torch.ones(2, n_grid)], 1)
    assert torch.equal(c(out['uniform_points_valid_mask']).reshape(2, -1), exp_valid)
    assert tuple(out['points_near_surface'].shape) == (2, res, res, 1, 3) and tuple(out['grid_random_pts'].shape) == (2, n_grid, 3)
    # the unseeded call draws its own noise: same shapes, different points, all inside the box for the grid part
    assert drawn['uniform_pts'].shape == out['uniform_pts'].shape and not torch.equal(drawn['uniform_pts'], out['uniform_pts'])
    assert float(drawn['grid_random_pts'].abs().max()) <= 0.12
