"""The per-point query kernels against float64, driven through the C ABI at small ragged shapes: e3dge_hitprob_points, e3dge_hitprob_composite
(csrc/hitprob.hip), e3dge_local_query, e3dge_local_query_bwd, e3dge_local_query_bwd_sorted and e3dge_pos_encoding (csrc/local_query.hip).

Every case computes the plain torch restatement of the operation twice on the CPU, in float64 (truth) and in float32 (the reference's own
arithmetic, the yardstick), and asserts  err <= max(floor, 3 |f32 - f64|)  with the floors the older tests state: gathers 2e-5, positional
encoding 2e-6, hit probability 5e-6, map gradient 2e-5 and point gradient 1e-4 of the gradient's maximum, projection 2e-6 (x, y) / 1e-6
(depth).  The sample positions q and the interpolation index of e3dge_hitprob_points have no older bound: 3 |f32 - f64| alone, the yardstick
taken over at least 300 points (a case with fewer points takes it from the same generator run with more rays).  Output buffers are
NaN-filled with spare rows and columns: the written slice must be finite, everything else still NaN.  No point is left out of a comparison:
the inputs are built in pixel space, at least 0.05 pixel away from every integer pixel coordinate and from the image border, so that fp32
rounding cannot flip the in-image mask, a corner's validity or the gradient's bilinear cell (asserted on the float64 side); points that sit
EXACTLY on the border have a test of their own with representable coordinates.

A bilinear footprint on a rectangular map has 0, 2, 3 or 4 corners outside the map (never exactly one): the shares asserted are those.
The positional encoding at n_freqs = 10 is 63 columns wide, so its slice [256, 319) gets rows of 321 floats; the narrower ones use 301.

What each construction would catch: S != Sn in every hit-probability case (a swapped stride moves q / sdf rows or the ray index), near / far
differ per ray (near[b * rays] reads another ray's depths: q and idx move by O(0.05)), totals 1, 70, 333, 600 with NaN guard rows (a missing
tail guard writes them), a second image whose own depth has the other sign (a per-batch z sign flips its projection), negative and mixed z
signs in the point gradient (a dropped sign flips d_pts' depth term), totals that leave a partial batch in the last run (a skipped partial
batch loses those points' gradient), ld = 137 / col_off = 69 and ld = 513 / col_off = 257 with NaN-checked neighbours (a vector store there
is misaligned or overwrites a neighbour).

Measured on an MI355X (maxima over all cases of a test; err / float32 yardstick / bound):
  hitprob_points      q   2.08e-07 / 2.08e-07 / 6.23e-07      idx 2.00e-04 / 2.02e-04 / 6.05e-04   (idx reaches 26: 8e-6 relative)
  hitprob_composite   3.17e-06 / 3.17e-06 / 9.51e-06  (24 cases)      the method, S = 7 against Sn = 18: 2.41e-06 / 2.44e-06 / 7.33e-06
  local_query forward gather 9.92e-06 / 9.87e-06 / 2.96e-05   x, y 1.98e-06 / 1.98e-06 / 5.94e-06   depth 1.53e-07 / 1.53e-07 / 1e-06
  local_query forward, points on the border: gather 2.75e-08 / 2.75e-08 / 2e-05, masks equal
  local_query backward (39 cases)  d map 8.61e-07 (sorted 8.61e-07) / 9.35e-07 / 2e-05      d points 5.93e-07 / 1.23e-06 / 1e-04
  column block        d map 5.37e-07 (sorted 5.27e-07) / 5.17e-07 / 2e-05      d points 1.54e-07 / 2.14e-07 / 1e-04
  one pixel           d map 3.16e-07 (sorted 3.78e-07) / 4.87e-07 / 2e-05      d points 2.03e-07 / 2.28e-07 / 1e-04
  pos_encoding        6.66e-08 / 3.58e-08 / 2e-06
"""
import pytest
import torch

from conftest import full_state_dict, record
from oracle import local_ref, renderer_ref

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, synthetic as syn
from e3dge_amd.camera_utils import generate_camera_params

DEV = "cuda:0"
NAN = float("nan")
F64 = torch.float64


def bound(floor, yard):
    return max(floor, 3.0 * yard)


def dist(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    return float((a - b).abs().max()) if a.numel() else 0.0


def nan_buf(*shape):
    return torch.full(shape, NAN, device=DEV, dtype=torch.float32)


def all_nan(t):
    return bool(torch.isnan(t).all())


def launch(name, *args):
    _lib.launch(name, *args)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------------
# hit probability
# ---------------------------------------------------------------------------------------------------------------------------------------
HP_CASES = [(1, 1, 1, 2), (2, 5, 7, 11), (3, 37, 3, 24), (1, 300, 2, 18)]        # (B, rays, S, Sn): totals 1, 70, 333, 600
HP_LOCATIONS = [[-0.15, 0.05], [0.25, -0.05], [0.05, 0.12]]                        # one reference camera per batch entry
HP_SEED = 11


def t_vals_of(Sn):
    return torch.linspace(0., 1. - 1 / Sn, steps=Sn)                                # reference :690-693


def hitprob_inputs(B, rays, S, Sn, seed=HP_SEED):
    """Points along rays of the reference cameras at chosen depths, in four kinds by flat index modulo 4: beyond the last sample
    (lo = hi = Sn-1, w up to 2.5), within 1e-3 of the first sample (either side), exactly at a sample depth, interior."""
    g = torch.Generator().manual_seed(seed + 1000 * Sn + S)
    u = lambda *s: torch.rand(*s, generator=g, dtype=F64)
    cam = generate_camera_params(8, 'cpu', locations=torch.tensor(HP_LOCATIONS[:B]), return_calibs=True)
    poses, extr = cam['poses'][:, :3, :4].contiguous(), cam['extrinsics'][:, :3, :4].contiguous()
    near = (0.88 + 0.05 * u(B, rays)).float()
    far = (near.double() + 0.2 + 0.1 * u(B, rays)).float()
    tv = t_vals_of(Sn)
    d_cam = torch.cat([(u(B, rays, S, 2) - 0.5) * 0.2, -torch.ones(B, rays, S, 1, dtype=F64)], -1)
    wd = torch.einsum('bij,brsj->brsi', poses[:, :, :3].double(), d_cam)
    z0 = near.double() * (1 - tv[0].double()) + far.double() * tv[0].double()
    z1 = near.double() * (1 - tv[1].double()) + far.double() * tv[1].double()
    kind = (torch.arange(B * rays * S) % 4).reshape(B, rays, S)
    target = torch.where(kind == 0, Sn - 1 + 0.3 + 2.2 * u(B, rays, S),
                         torch.where(kind == 1, 2e-3 * (u(B, rays, S) - 0.5),
                                     torch.where(kind == 2, torch.randint(0, Sn, (B, rays, S), generator=g).double(), (Sn - 1) * u(B, rays, S))))
    depth = z0[..., None] + target * (z1 - z0)[..., None]
    pts = (poses[:, :, 3].double()[:, None, None, :] + wd * depth[..., None]).float()
    return dict(pts=pts.contiguous(), poses=poses, extr=extr, near=near, far=far, tv=tv, kind=kind)


def hitprob_points_ref(i, dtype):
    """renderer_ref.query_hitting_probability_fixed_interval up to the interpolation index (reference :1367-1440): q (B,R,S,Sn,3), idx (B,R,S)."""
    p, P, E = i['pts'].to(dtype), i['poses'].to(dtype), i['extr'].to(dtype)
    B, R, S, _ = p.shape
    Sn = i['tv'].numel()
    w2c = torch.cat((E, torch.zeros_like(E[..., 0:1, :])), dim=-2)
    w2c[..., -1, -1] = 1
    homo = torch.cat((p, torch.ones_like(p[..., 0:1])), dim=-1).unsqueeze(-1)
    ref_space = w2c.reshape(B, 1, 1, 4, 4) @ homo
    rays_d_ref = ref_space[..., :3, :] / (-ref_space[..., 2:3, :])
    rays_d_wd = (P.reshape(B, 1, 1, 3, 4)[..., :3] @ rays_d_ref).permute(0, 1, 2, 4, 3)
    rays_o = P[..., 3:4].permute(0, 2, 1).reshape(B, 1, 1, 1, 3)
    t = i['tv'].to(dtype).reshape(1, 1, 1, 1, Sn)
    z = i['near'].to(dtype).reshape(B, R, 1, 1, 1) * (1. - t) + i['far'].to(dtype).reshape(B, R, 1, 1, 1) * t
    interval = (z[..., 1:2] - z[..., 0:1]) * rays_d_wd.norm(dim=-1, keepdim=True).permute(0, 1, 2, 4, 3)
    q = rays_o + rays_d_wd * z.permute(0, 1, 2, 4, 3)
    idx = (p.unsqueeze(-2) - q[..., 0:1, :]).norm(dim=-1, keepdim=True) / interval + 1e-5
    return q, idx.reshape(B, R, S)


def hitprob_yardstick(B, rays, S, Sn):
    """|f32 - f64| of q and idx over at least 300 points of the case's generator."""
    need = -(-300 // (B * S))
    i = hitprob_inputs(B, max(rays, need), S, Sn)
    (q64, x64), (q32, x32) = hitprob_points_ref(i, F64), hitprob_points_ref(i, torch.float32)
    assert x64.numel() >= 300
    return dist(q32, q64), dist(x32, x64)


def run_hitprob_points(i):
    B, R, S, _ = i['pts'].shape
    Sn, total = i['tv'].numel(), B * R * S
    q, aux = nan_buf(total + 2, Sn, 3), nan_buf(total + 2, 4)
    d = {k: i[k].to(DEV).contiguous() for k in ('pts', 'poses', 'extr', 'near', 'far', 'tv')}
    launch("e3dge_hitprob_points", q, aux, d['pts'], d['poses'], d['extr'], d['near'], d['far'], d['tv'], B, R, S, Sn)
    return q, aux, d


@pytest.mark.gpu
@pytest.mark.parametrize("B,rays,S,Sn", HP_CASES)
def test_hitprob_points_against_float64(B, rays, S, Sn):
    i = hitprob_inputs(B, rays, S, Sn)
    total = B * rays * S
    q64, idx64 = hitprob_points_ref(i, F64)
    yq, yi = hitprob_yardstick(B, rays, S, Sn)
    if total >= 8:            # every kind of point is there (float64 side)
        k = i['kind']
        assert (idx64[k == 0] > Sn - 1 + 0.29).all() and (idx64[k == 0] > Sn).any()
        assert (idx64[k == 1] < 1.1e-3).all()
        assert ((idx64[k == 2] - 1e-5 - idx64[k == 2].round()).abs() < 1e-4).all() and (idx64[k == 2] > 0.5).any()
        assert ((idx64[k == 3] > 1.0) & (idx64[k == 3] < Sn - 2.0)).any()
    q, aux, _ = run_hitprob_points(i)
    assert torch.isfinite(q[:total]).all() and torch.isfinite(aux[:total]).all()
    assert all_nan(q[total:]) and all_nan(aux[total:]), "rows past the end were written"
    e = dict(q=dist(q[:total].reshape(B, rays, S, Sn, 3), q64), q_f32=yq, q_bound=bound(0.0, yq),
             idx=dist(aux[:total, 3].reshape(B, rays, S), idx64), idx_f32=yi, idx_bound=bound(0.0, yi))
    record("hitprob_points_f64", B=B, rays=rays, S=S, Sn=Sn, **e)
    print(e)
    # lo, hi, w from the kernel's own index, bit for bit
    a = aux[:total].cpu()
    idx = a[:, 3]
    lo, hi = idx.floor().clamp(0, Sn - 1), idx.ceil().clamp(0, Sn - 1)
    assert torch.equal(a[:, 0], lo) and torch.equal(a[:, 1], hi) and torch.equal(a[:, 2], idx - lo)
    if total >= 8:
        assert ((a[:, 0] == Sn - 1) & (a[:, 1] == Sn - 1) & (a[:, 2] > 1)).any() and (a[:, 0] == 0).any() and (a[:, 0] == a[:, 1]).any()
    assert e['q'] <= e['q_bound'] and e['idx'] <= e['idx_bound'], e


def composite_sdf(B, rays, S, Sn, seed=HP_SEED):
    """A linear ramp through zero at a random depth per point (from before the first sample to behind the last), plus noise."""
    g = torch.Generator().manual_seed(seed + 7 * Sn + S)
    c = torch.rand(B, rays, S, 1, generator=g, dtype=F64) * (Sn + 1) - 1.5
    if B * rays * S == 1:
        c[:] = -0.5                                                 # the one point: the surface lies in front of its first sample
    s = torch.arange(Sn, dtype=F64)
    return (0.02 * (c - s) + 0.004 * torch.randn(B, rays, S, Sn, generator=g, dtype=F64)).float()


def hitprob_composite_ref(sdf, aux, near, far, tv, beta, visibility, dtype):
    """volume_integration(no_force_stop=True) (:826-837, :869-886) and the interpolation (:1480-1495) as renderer_ref states them, from the
    kernel's own (lo, hi, w).  beta is the fp32 value the kernel receives.  Returns (out (B,R,S), per-sample values (B,R,S,Sn))."""
    t = tv.to(dtype)
    z = near.to(dtype)[..., None] * (1. - t) + far.to(dtype)[..., None] * t                   # B R Sn
    d = z[..., 1:] - z[..., :-1]
    d = torch.cat([d, d[..., 0:1]], -1)[:, :, None, :]
    b = torch.tensor(beta, dtype=torch.float32).to(dtype)
    sigma = torch.sigmoid(-sdf.to(dtype) / b) / b
    alpha = 1 - torch.exp(-sigma * d)
    vis = torch.cumprod(torch.cat([torch.ones_like(alpha[..., :1]), 1. - alpha + 1e-10], -1), -1)[..., :-1]
    val = vis if visibility else alpha * vis
    lo, hi, w = aux[..., 0].long(), aux[..., 1].long(), aux[..., 2].to(dtype)
    f = torch.gather(val, -1, lo[..., None])[..., 0]
    c = torch.gather(val, -1, hi[..., None])[..., 0]
    return torch.lerp(f, c, w), val


@pytest.mark.gpu
@pytest.mark.parametrize("B,rays,S,Sn", HP_CASES)
def test_hitprob_composite_against_float64(B, rays, S, Sn):
    i = hitprob_inputs(B, rays, S, Sn)
    total = B * rays * S
    _, aux, d = run_hitprob_points(i)
    sdf = composite_sdf(B, rays, S, Sn)
    sdf_d = sdf.to(DEV).contiguous()
    aux_c = aux[:total].cpu().reshape(B, rays, S, 4)
    fails = []
    for beta in (0.1, 0.01, 0.001):
        for vis in (0, 1):
            out = nan_buf(total + 2)
            launch("e3dge_hitprob_composite", out, sdf_d, aux, d['near'], d['far'], d['tv'], beta, vis, B, rays, S, Sn)
            assert torch.isfinite(out[:total]).all() and all_nan(out[total:])
            o64, v64 = hitprob_composite_ref(sdf, aux_c, i['near'], i['far'], i['tv'], beta, vis, F64)
            o32, _ = hitprob_composite_ref(sdf, aux_c, i['near'], i['far'], i['tv'], beta, vis, torch.float32)
            if beta == 0.001:         # the hard regime is reached (float64 side)
                assert (float(v64.min()) <= 1e-6) if vis else (float(v64.max()) >= 0.9), (vis, float(v64.min()), float(v64.max()))
            e = dict(err=dist(out[:total].reshape(B, rays, S), o64), f32=dist(o32, o64))
            e['bound'] = bound(5e-6, e['f32'])
            record("hitprob_composite_f64", B=B, rays=rays, S=S, Sn=Sn, beta=beta, visibility=vis, **e)
            print(beta, vis, e)
            if e['err'] > e['bound']:
                fails.append((beta, vis, e))
    assert not fails, fails


@pytest.mark.gpu
def test_hit_probability_method_with_per_pixel_near_far_and_few_points():
    """VolumeFeatureRenderer.query_hitting_probability_fixed_interval with S = 7 points per pixel against N_samples = 18 and near / far that
    differ at every pixel, against renderer_ref in float64."""
    from test_gpu_renderer import make_renderer
    B, H, W, S, Sn = 2, 3, 5, 7, 18
    sd = full_state_dict(res=8, n_samples=Sn)[1]
    r = make_renderer(sd, 8, Sn)
    i = hitprob_inputs(B, H * W, S, Sn)
    wr, _ = syn.synthetic_inputs(B, seed=5)
    pts = i['pts'].reshape(B, H, W, S, 3)
    near, far = i['near'].reshape(B, H, W, 1), i['far'].reshape(B, H, W, 1)
    info = dict(global_render_out=dict(near=near.to(DEV), far=far.to(DEV)),
                cam_settings=dict(poses=i['poses'].to(DEV), extrinsics=i['extr'].to(DEV)), pred_latents=[wr.to(DEV)])
    fails = []
    for rt in ('weights', 'visibility'):
        with torch.no_grad():
            out = r.query_hitting_probability_fixed_interval(pts.to(DEV), info, return_type=rt)
            ref = [renderer_ref.query_hitting_probability_fixed_interval(sd, pts, i['poses'], i['extr'], near, far, wr, Sn, return_type=rt, dtype=dt)
                   for dt in (F64, torch.float32)]
        assert tuple(out.shape) == (B, H, W, S, 1) and torch.isfinite(out).all()
        e = dict(err=dist(out, ref[0]), f32=dist(ref[1], ref[0]))
        e['bound'] = bound(5e-6, e['f32'])
        record("hitprob_method_S7_Sn18", return_type=rt, **e)
        print(rt, e)
        if e['err'] > e['bound']:
            fails.append((rt, e))
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------------------------------
# local query
# ---------------------------------------------------------------------------------------------------------------------------------------
CALIBS = [[[2.2, 0.1, 0.0, 0.03], [0.05, 2.1, 0.1, -0.02], [0.0, 0.1, 1.0, 2.0]],
          [[1.9, -0.2, 0.1, 0.0], [0.1, 2.3, 0.0, 0.05], [0.1, 0.0, 1.0, 1.7]],
          [[2.0, 0.15, -0.1, 0.02], [-0.1, 2.2, 0.05, 0.0], [0.05, -0.05, 1.0, 1.9]]]
SIGNS = ('pos', 'neg', 'mixed')


def calibs_for(B, sign):
    """'pos': every image has homo_z > 0.  'neg': the third row negated, homo_z < 0 everywhere (what the real cameras give) -- the same
    projections.  'mixed': images 0 and 2 negative, image 1 positive: the first point of image 0 decides for all, so image 1 is divided
    by -homo_z and its projections are mirrored through the centre."""
    c = torch.tensor(CALIBS, dtype=torch.float32)[:B].clone()
    if sign == 'neg':
        c[:, 2] *= -1
    elif sign == 'mixed':
        assert B >= 2
        c[0::2, 2] *= -1
    return c


def lq_points(B, N, h, w, seed, mode='spread'):
    """World-space points whose projection (calibs_for(B, 'pos')) is chosen in PIXEL space: coordinate = k + frac with frac in
    [.05, .45] or [.55, .95], so no coordinate is within 0.05 pixel of an integer or of the border (border: k + 0.5).  Per axis 55 % inside
    (k in [0, size-2]), 25 % on the rim (k = -1 or size-1: one of the two columns outside), 10 % just outside (k = -2 or size), 10 % far
    outside (3 .. 20 pixels: outside the kernel's `finite` window).  The first point of every image is inside.
    mode 'pixel': every point in the cell (1, 2); mode 'far': every point far outside."""
    g = torch.Generator().manual_seed(seed)
    n = B * N

    def axis(size, cell):
        kind = torch.randint(0, 20, (n,), generator=g)
        frac = 0.05 + 0.4 * torch.rand(n, generator=g, dtype=F64) + 0.5 * torch.randint(0, 2, (n,), generator=g)
        side = torch.randint(0, 2, (n,), generator=g)
        off = torch.randint(3, 21, (n,), generator=g)
        k_in = torch.randint(0, max(size - 1, 1), (n,), generator=g)
        k_rim = torch.where(side == 0, -1, size - 1)
        k_out = torch.where(side == 0, -2, size)
        k_far = torch.where(side == 0, -off, size - 1 + off)
        if mode == 'pixel':
            return cell + frac
        if mode == 'far':
            return k_far + frac
        if size < 2:
            k_in = k_rim
        first = (torch.arange(n) % N) == 0
        kind = torch.where(first, 0, kind)
        k = torch.where(kind < 11, k_in, torch.where(kind < 16, k_rim, torch.where(kind < 18, k_out, k_far)))
        return k + frac
    fx, fy = axis(w, 1), axis(h, 2)
    x, y = (2 * fx + 1) / w - 1, (2 * fy + 1) / h - 1
    z = 1.5 + torch.rand(n, generator=g, dtype=F64)
    homo = torch.stack([x * z, -y * z, z], -1).reshape(B, N, 3)
    c = calibs_for(B, 'pos').double()
    p = torch.linalg.solve(c[:, :, :3], (homo - c[:, None, :, 3]).transpose(1, 2)).transpose(1, 2)
    return p.float().contiguous()


def lq_ref(pts, calibs, fmap, dtype):
    return local_ref.query(pts.to(dtype).permute(0, 2, 1), calibs.to(dtype), None if fmap is None else fmap.to(dtype))


def pixel_stats(q64, h, w):
    """From the float64 projection: per point the number of footprint corners outside the map, whether it is outside the kernel's
    `finite` window, and the smallest distance of a pixel coordinate to an integer / of a coordinate to the border."""
    x, y = q64['proj_xy'][:, 0].reshape(-1), q64['proj_xy'][:, 1].reshape(-1)
    fx, fy = ((x + 1) * w - 1) / 2, ((y + 1) * h - 1) / 2
    x0, y0 = fx.floor(), fy.floor()
    nx = ((x0 >= 0) & (x0 < w)).long() + ((x0 + 1 >= 0) & (x0 + 1 < w)).long()
    ny = ((y0 >= 0) & (y0 < h)).long() + ((y0 + 1 >= 0) & (y0 + 1 < h)).long()
    outside = 4 - nx * ny
    far = ~((fx > -2) & (fx < w + 1) & (fy > -2) & (fy < h + 1))
    cell = float(torch.minimum((fx - fx.round()).abs(), (fy - fy.round()).abs()).min())
    border = float(torch.minimum((x.abs() - 1).abs(), (y.abs() - 1).abs()).min())
    return outside, far, cell, border


def assert_margins(q64, q32, h, w, spread):
    outside, far, cell, border = pixel_stats(q64, h, w)
    assert border >= 1e-5 and cell >= 1e-3, (border, cell)
    assert torch.equal(q64['in_img'], q32['in_img'])
    if spread:
        n = outside.numel()
        share = {k: float((outside == k).sum()) / n for k in range(5)}
        assert share[1] == 0.0                           # a rectangle never loses exactly one corner
        assert share[0] >= 0.15 and share[2] >= 0.10 and share[3] >= 0.02 and share[4] >= 0.15 and float(far.sum()) / n >= 0.05, share
        assert 0.2 <= float(q64['in_img'].double().mean()) <= 0.8


LQ_FWD_CASES = [(1, 1, 4, 1, 1, 4, 0), (3, 37, 8, 5, 7, 8, 0), (2, 301, 68, 3, 9, 137, 69), (2, 130, 256, 32, 32, 513, 257),
                (1, 50, 260, 4, 4, 260, 0), (1, 40000, 4, 16, 16, 4, 0)]                   # (B, N, C, h, w, ld, col_off); the mixed sign needs B >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,C,h,w,ld,col_off,sign", [c + (s,) for c in LQ_FWD_CASES for s in SIGNS if s != 'mixed' or c[0] >= 2])
def test_local_query_forward_against_float64(B, N, C, h, w, ld, col_off, sign):
    total = B * N
    pts = lq_points(B, N, h, w, seed=100 + N)
    calibs = calibs_for(B, sign)
    fmap = torch.randn(B, C, h, w, generator=torch.Generator().manual_seed(200 + N))
    q64, q32 = lq_ref(pts, calibs, fmap, F64), lq_ref(pts, calibs, fmap, torch.float32)
    assert_margins(q64, q32, h, w, spread=total >= 100)
    hz = torch.einsum('bj,bnj->bn', calibs[:, 2, :3].double(), pts.double()) + calibs[:, 2, 3:4].double()
    assert (hz[0, 0] > 0) == (sign == 'pos') and (sign != 'mixed' or (hz[1] > 0).all())
    out, mask, maskw, proj = nan_buf(total + 2, ld), nan_buf(total + 2), nan_buf(total + 2, 5), nan_buf(total + 2, 3)
    pd, cd = pts.to(DEV), calibs.to(DEV)
    fm = fmap.to(DEV).permute(0, 2, 3, 1).contiguous()
    launch("e3dge_local_query", out, ld, col_off, mask, 1, 0, proj, pd, cd, fm, B, N, C, h, w)
    launch("e3dge_local_query", None, 0, 0, maskw, 5, 3, None, pd, cd, None, B, N, 0, 0, 0)     # projection only: the mask into column 3 of 5
    got = out[:total, col_off:col_off + C]
    assert torch.isfinite(got).all() and torch.isfinite(proj[:total]).all()
    assert all_nan(out[total:]) and all_nan(out[:total, :col_off]) and all_nan(out[:total, col_off + C:]), "written outside the slice"
    assert all_nan(mask[total:]) and all_nan(proj[total:]) and all_nan(maskw[total:]) and all_nan(maskw[:total, :3]) and all_nan(maskw[:total, 4:])
    want_mask = q64['in_img'].reshape(-1).float()
    assert torch.equal(mask[:total].cpu(), want_mask) and torch.equal(maskw[:total, 3].cpu(), want_mask)
    f = lambda t: t.permute(0, 2, 1).reshape(total, -1)
    e = dict(gather=dist(got, f(q64['feats'])), gather_f32=dist(q32['feats'], q64['feats']),
             xy=dist(proj[:total, :2], f(q64['proj_xy'])), xy_f32=dist(q32['proj_xy'], q64['proj_xy']),
             depth=dist(proj[:total, 2:], f(q64['depth'])), depth_f32=dist(q32['depth'], q64['depth']))
    e.update(gather_bound=bound(2e-5, e['gather_f32']), xy_bound=bound(2e-6, e['xy_f32']), depth_bound=bound(1e-6, e['depth_f32']))
    record("local_query_forward_f64", B=B, N=N, C=C, h=h, w=w, ld=ld, col_off=col_off, sign=sign, **e)
    print(e)
    assert e['gather'] <= e['gather_bound'] and e['xy'] <= e['xy_bound'] and e['depth'] <= e['depth_bound'], e


@pytest.mark.gpu
def test_local_query_empty_point_set_writes_nothing():
    out, mask, proj = nan_buf(4, 8), nan_buf(4), nan_buf(4, 3)
    pd, cd = torch.zeros(2, 1, 3, device=DEV), calibs_for(2, 'pos').to(DEV)
    fm = torch.randn(2, 3, 3, 8, device=DEV)
    launch("e3dge_local_query", out, 8, 0, mask, 1, 0, proj, pd, cd, fm, 2, 0, 8, 3, 3)
    launch("e3dge_local_query", out, 8, 0, mask, 1, 0, proj, pd, cd, fm, 0, 5, 8, 3, 3)
    assert all_nan(out) and all_nan(mask) and all_nan(proj)
    record("local_query_forward_empty", written=0)


@pytest.mark.gpu
@pytest.mark.parametrize("sign", ('pos', 'neg'))
def test_local_query_points_exactly_on_the_border_are_inside(sign):
    """x = +-1 or y = +-1 exactly in both precisions (calibration diag(2, 2, 1) with depth offset 2, coordinates that are dyadic rationals):
    the mask's comparisons are <= and >=, so these are inside."""
    calib = torch.tensor([[[2.0, 0.0, 0.0, 0.0], [0.0, 2.0, 0.0, 0.0], [0.0, 0.0, 1.0, 2.0]]])
    if sign == 'neg':
        calib[:, 2] *= -1
    pts = torch.tensor([[[0.25, 0.125, 0.0], [1.0, 0.25, 0.0], [-1.0, -0.5, 0.0], [0.5, 1.0, 0.0], [0.25, -1.0, 0.0], [0.5, -0.25, -1.0],
                         [-0.5, 0.5, -1.0], [1.0, 1.0, 0.0], [-0.75, 0.75, -0.5], [1.0078125, 0.0, 0.0], [0.0, -1.0078125, 0.0]]])
    B, N, C, h, w = 1, pts.shape[1], 4, 4, 6
    fmap = torch.randn(B, C, h, w, generator=torch.Generator().manual_seed(3))
    q64, q32 = lq_ref(pts, calib, fmap, F64), lq_ref(pts, calib, fmap, torch.float32)
    want = torch.tensor([1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0], dtype=torch.bool)
    assert torch.equal(q64['in_img'][0], want) and torch.equal(q32['in_img'][0], want)
    assert int(((q64['proj_xy'].abs() == 1).any(1) & q64['in_img']).sum()) == 8 and torch.equal(q64['proj_xy'], q32['proj_xy'].double())
    out, mask = nan_buf(N + 2, C), nan_buf(N + 2)
    launch("e3dge_local_query", out, C, 0, mask, 1, 0, None, pts.to(DEV), calib.to(DEV), fmap.to(DEV).permute(0, 2, 3, 1).contiguous(), B, N, C, h, w)
    assert torch.equal(mask[:N].cpu(), want.float()) and all_nan(mask[N:]) and all_nan(out[N:])
    e = dict(gather=dist(out[:N], q64['feats'][0].T), gather_f32=dist(q32['feats'], q64['feats']))
    e['gather_bound'] = bound(2e-5, e['gather_f32'])
    record("local_query_forward_border", sign=sign, **e)
    assert e['gather'] <= e['gather_bound'], e


# ---- backward -------------------------------------------------------------------------------------------------------------------------
LQ_BWD_SHAPES = [(1, 1), (3, 1), (2, 15), (3, 43), (1, 613)]                       # totals 1, 3, 30, 129, 613
LQ_BWD_MAPS = {4: (5, 7), 68: (3, 9), 256: (8, 8)}                                 # C -> (h, w)


def lq_grads_ref(pts, calibs, fmap, g_out, dtype):
    """float autograd of perspective + grid_sample(bilinear, zeros, align_corners=False): (d map (B,C,h,w), d points (B,N,3))."""
    p = pts.to(dtype).requires_grad_(True)
    f = fmap.to(dtype).requires_grad_(True)
    feats = local_ref.query(p.permute(0, 2, 1), calibs.to(dtype), f)['feats']
    (feats.permute(0, 2, 1) * g_out.to(dtype)).sum().backward()
    return f.grad, p.grad


def run_lq_bwd(sorted_walk, pts, calibs, fmap, d_out, ld, col_off, C):
    """One call with both gradients requested.  d map: zero-filled as the ABI asks, with two NaN guard rows behind it."""
    B, N, _ = pts.shape
    h, w = fmap.shape[2:]
    total = B * N
    d_fm = nan_buf(B * h * w + 2, C)
    d_fm[:B * h * w] = 0
    d_p = nan_buf(total + 2, 3)
    pd, cd = pts.to(DEV).contiguous(), calibs.to(DEV).contiguous()
    fm = fmap.to(DEV).permute(0, 2, 3, 1).contiguous()
    if sorted_walk:
        n_ws = _lib.load().e3dge_local_query_sort_ws_ints(B, N, h, w)
        ws = torch.full((n_ws,), -1, device=DEV, dtype=torch.int32)
        launch("e3dge_local_query_bwd_sorted", d_fm, d_p, d_out, ld, col_off, pd, cd, fm, B, N, C, h, w, ws, n_ws)
        order = ws[total:2 * total].long()
        assert torch.equal(torch.sort(order).values, torch.arange(total, device=DEV)), "order is not a permutation"
    else:
        launch("e3dge_local_query_bwd", d_fm, d_p, d_out, ld, col_off, pd, cd, fm, B, N, C, h, w)
    assert all_nan(d_fm[B * h * w:]) and all_nan(d_p[total:]), "rows past the end were written"
    assert torch.isfinite(d_fm[:B * h * w]).all() and torch.isfinite(d_p[:total]).all()
    return d_fm[:B * h * w].reshape(B, h, w, C).permute(0, 3, 1, 2).cpu(), d_p[:total].reshape(B, N, 3).cpu()


def check_lq_bwd(name, pts, calibs, fmap, d_out_dev, ld, col_off, C, **tags):
    g_out = d_out_dev[..., col_off:col_off + C].cpu()
    (f64, p64), (f32, p32) = lq_grads_ref(pts, calibs, fmap, g_out, F64), lq_grads_ref(pts, calibs, fmap, g_out, torch.float32)
    mf, mp = float(f64.abs().max()), float(p64.abs().max())
    assert mf > 0 and mp > 0
    plain = run_lq_bwd(False, pts, calibs, fmap, d_out_dev, ld, col_off, C)
    sort = run_lq_bwd(True, pts, calibs, fmap, d_out_dev, ld, col_off, C)
    e = dict(d_fmap=dist(plain[0], f64) / mf, d_fmap_sorted=dist(sort[0], f64) / mf, d_fmap_f32=dist(f32, f64) / mf,
             d_pts=dist(plain[1], p64) / mp, d_pts_f32=dist(p32, p64) / mp)
    e.update(d_fmap_bound=bound(2e-5, e['d_fmap_f32']), d_pts_bound=bound(1e-4, e['d_pts_f32']))
    record(name, C=C, ld=ld, col_off=col_off, **tags, **e)
    print(e)
    assert torch.equal(sort[1], plain[1]), "d_pts of the sorted walk differs from the plain walk"
    assert e['d_fmap'] <= e['d_fmap_bound'] and e['d_fmap_sorted'] <= e['d_fmap_bound'] and e['d_pts'] <= e['d_pts_bound'], e
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,C,sign", [(b, n, c, s) for b, n in LQ_BWD_SHAPES for c in sorted(LQ_BWD_MAPS) for s in SIGNS if s != 'mixed' or b >= 2])
def test_local_query_backward_against_float64(B, N, C, sign):
    """Totals 1, 3, 30, 129, 613: runs of 32 points walked in batches of 4, so 30 = 7 batches + 2, 129 = four runs + one point, 613 = 19 runs +
    5 = one batch + 1 -- the partial batch, the clamped index loads and a run shorter than a batch all execute."""
    h, w = LQ_BWD_MAPS[C]
    pts = lq_points(B, N, h, w, seed=300 + 7 * B + N + C)
    calibs = calibs_for(B, sign)
    gen = torch.Generator().manual_seed(400 + N + C)
    fmap = torch.randn(B, C, h, w, generator=gen)
    d_out = torch.randn(B, N, C, generator=gen).to(DEV)
    assert_margins(lq_ref(pts, calibs, None, F64), lq_ref(pts, calibs, None, torch.float32), h, w, spread=B * N >= 100)
    check_lq_bwd("local_query_backward_f64", pts, calibs, fmap, d_out, C, 0, C, B=B, N=N, sign=sign)


@pytest.mark.gpu
def test_local_query_backward_reads_a_column_block_of_wider_rows():
    """d_out = columns [C+1, 2C+1) of (B, N, 2C+1) rows, as the training form hands it over: odd pitch and offset (scalar loads), both
    gradients requested, the caller's buffer untouched."""
    B, N, C = 3, 43, 68
    h, w = LQ_BWD_MAPS[C]
    pts, calibs = lq_points(B, N, h, w, seed=501), calibs_for(B, 'neg')
    gen = torch.Generator().manual_seed(502)
    fmap = torch.randn(B, C, h, w, generator=gen)
    wide = torch.randn(B, N, 2 * C + 1, generator=gen).to(DEV)
    keep = wide.clone()
    check_lq_bwd("local_query_backward_column_block", pts, calibs, fmap, wide, 2 * C + 1, C + 1, C, B=B, N=N, sign='neg')
    assert torch.equal(wide, keep)


@pytest.mark.gpu
def test_local_query_backward_with_one_gradient_requested():
    """d_fmap alone (what the training form asks for) and d_pts alone: bit-identical points gradient, the map gradient within the bound of
    the call that asks for both (atomics in another order)."""
    B, N, C = 2, 15, 68
    h, w = LQ_BWD_MAPS[C]
    pts, calibs = lq_points(B, N, h, w, seed=551), calibs_for(B, 'mixed')
    gen = torch.Generator().manual_seed(552)
    fmap = torch.randn(B, C, h, w, generator=gen)
    d_out = torch.randn(B, N, C, generator=gen).to(DEV)
    f64, _ = lq_grads_ref(pts, calibs, fmap, d_out.cpu(), F64)
    f32, _ = lq_grads_ref(pts, calibs, fmap, d_out.cpu(), torch.float32)
    both = run_lq_bwd(False, pts, calibs, fmap, d_out, C, 0, C)
    pd, cd, fm = pts.to(DEV), calibs.to(DEV), fmap.to(DEV).permute(0, 2, 3, 1).contiguous()
    d_fm, d_p = torch.zeros(B, h, w, C, device=DEV), nan_buf(B * N + 2, 3)
    launch("e3dge_local_query_bwd", d_fm, None, d_out, C, 0, pd, cd, fm, B, N, C, h, w)
    launch("e3dge_local_query_bwd", None, d_p, d_out, C, 0, pd, cd, fm, B, N, C, h, w)
    assert torch.equal(d_p[:B * N].reshape(B, N, 3).cpu(), both[1]) and all_nan(d_p[B * N:])
    mf = float(f64.abs().max())
    e = dict(d_fmap=dist(d_fm.permute(0, 3, 1, 2), f64) / mf, d_fmap_f32=dist(f32, f64) / mf)
    e['d_fmap_bound'] = bound(2e-5, e['d_fmap_f32'])
    record("local_query_backward_one_gradient", **e)
    assert e['d_fmap'] <= e['d_fmap_bound'], e


@pytest.mark.gpu
@pytest.mark.parametrize("C", (4, 68))
def test_local_query_backward_sorted_with_every_point_in_one_pixel(C):
    """200 points in one bilinear cell: one bin of the counting sort, and every 32-point run of the walk ends in the same four addresses."""
    B, N, h, w = 1, 200, 6, 6
    pts, calibs = lq_points(B, N, h, w, seed=601, mode='pixel'), calibs_for(B, 'neg')
    q64 = lq_ref(pts, calibs, None, F64)
    fx, fy = ((q64['proj_xy'][:, 0] + 1) * w - 1) / 2, ((q64['proj_xy'][:, 1] + 1) * h - 1) / 2
    assert (fx.floor() == 1).all() and (fy.floor() == 2).all()
    gen = torch.Generator().manual_seed(602)
    fmap = torch.randn(B, C, h, w, generator=gen)
    d_out = torch.randn(B, N, C, generator=gen).to(DEV)
    check_lq_bwd("local_query_backward_one_pixel", pts, calibs, fmap, d_out, C, 0, C, B=B, N=N, sign='neg')


@pytest.mark.gpu
def test_local_query_backward_with_every_point_far_outside_is_exactly_zero():
    B, N, C, h, w = 2, 100, 8, 5, 7
    pts, calibs = lq_points(B, N, h, w, seed=701, mode='far'), calibs_for(B, 'mixed')
    _, far, _, _ = pixel_stats(lq_ref(pts, calibs, None, F64), h, w)
    assert far.all()
    gen = torch.Generator().manual_seed(702)
    fmap = torch.randn(B, C, h, w, generator=gen)
    d_out = torch.randn(B, N, C, generator=gen).to(DEV)
    for sorted_walk in (False, True):
        d_fm, d_p = run_lq_bwd(sorted_walk, pts, calibs, fmap, d_out, C, 0, C)         # (finite and guard rows checked inside)
        assert float(d_fm.abs().max()) == 0.0 and float(d_p.abs().max()) == 0.0
    record("local_query_backward_all_far", d_fmap=0.0, d_pts=0.0)


@pytest.mark.gpu
def test_local_query_backward_refuses_more_than_256_channels():
    B, N, C, h, w = 1, 8, 260, 3, 3
    lib = _lib.load()
    z = lambda *s: torch.zeros(*s, device=DEV)
    d_fm, d_p, d_out, pts, fm = z(B, h, w, C), nan_buf(B, N, 3), z(B, N, C), z(B, N, 3), z(B, h, w, C)
    cd = calibs_for(B, 'pos').to(DEV)
    rc = lib.e3dge_local_query_bwd(_lib.ptr(d_fm), _lib.ptr(d_p), _lib.ptr(d_out), C, 0, _lib.ptr(pts), _lib.ptr(cd), _lib.ptr(fm), B, N, C, h, w, None)
    assert rc != 0 and "at most 256 channels" in lib.e3dge_last_error().decode()
    n_ws = lib.e3dge_local_query_sort_ws_ints(B, N, h, w)
    ws = torch.zeros(n_ws, device=DEV, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="at most 256 channels"):
        _lib.launch("e3dge_local_query_bwd_sorted", d_fm, d_p, d_out, C, 0, pts, cd, fm, B, N, C, h, w, ws, n_ws)
    torch.cuda.synchronize()
    assert all_nan(d_p) and float(d_fm.abs().max()) == 0.0
    record("local_query_backward_refuses_C260", refused=1)


# ---- positional encoding --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M", (1, 37, 1000))
@pytest.mark.parametrize("n_freqs", (0, 1, 7, 10))
def test_pos_encoding_against_float64(n_freqs, M):
    """[x, sin(2^k x), cos(2^k x)]_k: 2^k x is exact in fp32, so float64 sin / cos of that product isolates the device sinf / cosf."""
    width = 3 * (2 * n_freqs + 1)
    x = (torch.rand(M, 3, generator=torch.Generator().manual_seed(800 + M)) - 0.5) * 1.2

    def ref(dtype):
        cols = [x.to(dtype)]
        for k in range(n_freqs):
            prod = (x * float(2 ** k)).to(dtype)          # the fp32 product, exact
            cols += [torch.sin(prod), torch.cos(prod)]
        return torch.cat(cols, -1)
    r64, r32 = ref(F64), ref(torch.float32)
    ld = max(301, 256 + width + 2)
    own, wide = nan_buf(M + 2, width), nan_buf(M + 2, ld)
    xd = x.to(DEV)
    launch("e3dge_pos_encoding", own, width, 0, xd, M, n_freqs)
    launch("e3dge_pos_encoding", wide, ld, 256, xd, M, n_freqs)
    assert torch.isfinite(own[:M]).all() and all_nan(own[M:])
    assert all_nan(wide[M:]) and all_nan(wide[:M, :256]) and all_nan(wide[:M, 256 + width:])
    assert torch.equal(wide[:M, 256:256 + width], own[:M]) and torch.equal(own[:M, :3].cpu(), x)
    e = dict(err=dist(own[:M], r64), f32=dist(r32, r64))
    e['bound'] = bound(2e-6, e['f32'])
    record("pos_encoding_f64", n_freqs=n_freqs, M=M, **e)
    print(e)
    assert e['err'] <= e['bound'], e
