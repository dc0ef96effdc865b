"""Surface renderings, host side (mesh_utils.MeshCamera, depth_mesh's face order, the C-ABI of csrc/mesh_render.hip) and the numpy
restatement of the contract in include/e3dge_hip.h (e3dge_vertex_normals, e3dge_mesh_render) that tests/test_gpu_mesh_render.py and
tools/gen_golden_mesh_render.py compare the kernels with.  The restatement takes a dtype: float64 is "truth", float32 the yardstick
(the distance of an independent fp32 evaluation from truth).  It is checked against closed forms here."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, mesh_utils
from e3dge_amd.camera_utils import generate_camera_params

INVALID = -1                                                        # E3DGE_ERR_INVALID_ARG
DEFAULT_LIGHTS = dict(light=(-0.5, 1.0, 5.0), ambient=(0.5, 0.5, 0.5), diffuse=(0.3, 0.3, 0.3), specular=(0.2, 0.2, 0.2))
RUNNER_LIGHTS = dict(light=(0.0, 0.0, 5.0), ambient=(0.1, 0.1, 0.1), diffuse=(0.65, 0.65, 0.65), specular=(0.2, 0.2, 0.2))
SURFACE_LIGHTS = dict(RUNNER_LIGHTS, light=(0.0, 3.0, 5.0))


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def restate_normals(verts, faces, dtype=np.float64):
    """Angle-weighted vertex normals: sum over a vertex's faces of corner angle x unit face normal, normalised; zero-area faces add
    nothing, a vertex without faces (or a zero sum) gets 0."""
    T = dtype
    v = np.asarray(verts).astype(T)
    f = np.asarray(faces).astype(np.int64)
    p = v[f]                                                                     # (F, 3 corners, 3)
    e = np.roll(p, -1, axis=1) - p                                               # e[:, k] = corner k -> corner k + 1
    ln = np.sqrt((e * e).sum(-1))
    n = np.cross(e[:, 0], -e[:, 2])
    nl = np.sqrt((n * n).sum(-1))
    ok = (nl > 0) & (ln > 0).all(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        eu = e / ln[..., None]
        nu = n / nl[:, None]
        acc = np.zeros_like(v)
        for k in range(3):
            dot = (eu[:, k] * -eu[:, (k + 2) % 3]).sum(-1)
            ang = np.arccos(np.clip(dot, T(-1), T(1)))
            np.add.at(acc, f[ok, k], (ang[:, None] * nu)[ok])
        l = np.sqrt((acc * acc).sum(-1, keepdims=True))
        return np.where(l > 0, acc / np.where(l > 0, l, T(1)), T(0)).astype(T)


def _seg_d2(qx, qy, ax, ay, bx, by, T):
    ex, ey = bx - ax, by - ay
    l2 = ex * ex + ey * ey
    if l2 <= T(1e-8):
        return (qx - bx) * (qx - bx) + (qy - by) * (qy - by)
    t = np.clip((ex * (qx - ax) + ey * (qy - ay)) / l2, T(0), T(1))
    px, py = ax + t * ex, ay + t * ey
    return (qx - px) * (qx - px) + (qy - py) * (qy - py)


def _unit(x, T):
    return x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), T(1e-6))


def restate_render(verts, faces, normals, camera, S, K, lights=DEFAULT_LIGHTS, colors=None, blur=1e-6, sigma=1e-4, gamma=1e-4,
                   background=(1.0, 1.0, 1.0), dtype=np.float64):
    """e3dge_mesh_render's contract (include/e3dge_hip.h) in numpy, vectorised over the pixels of each face's bounding box, in the
    documented order of operations.  Inputs are the float32 values the kernel gets; `dtype` is the arithmetic.  Returns a dict: image
    (S, S, 4), zbuf (S, S, K), pix_to_face (S, S, K), covered (S, S) and undecided (S, S) -- a pixel is undecided when, for some face
    whose widened box contains it, a screen barycentric lies within 1e-5 of 0 or the pixel lies outside with |sqrt(d2) - sqrt(blur)| <
    1e-5, or when the K-th and (K+1)-th covered fragments are closer than 1e-6 in depth."""
    T = dtype
    f32 = lambda x: np.asarray(x, np.float32).astype(T)
    V, N = f32(verts), f32(normals)
    F = np.asarray(faces).astype(np.int64)
    cam = f32(camera.floats())
    C, xa, ya, za = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    t, znear, zfar = (T(np.float32(x)) for x in (camera.tan_half_fov, camera.znear, camera.zfar))
    blur_t, sigma_t, gamma_t = (T(np.float32(x)) for x in (blur, sigma, gamma))
    d = V - C
    vx = d[:, 0] * xa[0] + d[:, 1] * xa[1] + d[:, 2] * xa[2]
    vy = d[:, 0] * ya[0] + d[:, 1] * ya[1] + d[:, 2] * ya[2]
    vz = d[:, 0] * za[0] + d[:, 1] * za[1] + d[:, 2] * za[2]
    with np.errstate(invalid="ignore", divide="ignore"):
        den = vz * t
        xn, yn = vx / den, vy / den
    X, Y, Z = xn[F], yn[F], vz[F]                                               # (F, 3)
    area = (X[:, 2] - X[:, 0]) * (Y[:, 1] - Y[:, 0]) - (Y[:, 2] - Y[:, 0]) * (X[:, 1] - X[:, 0])
    cand = (np.abs(area) > T(1e-8)) & (Z >= znear * T(0.5)).all(1)
    r = np.sqrt(blur_t)
    bx0, bx1, by0, by1 = X.min(1) - r, X.max(1) + r, Y.min(1) - r, Y.max(1) + r
    pix_of = lambda ndc: ((1.0 - ndc.astype(np.float64)) * S - 1.0) * 0.5
    with np.errstate(invalid="ignore"):
        jlo = np.clip(np.floor(pix_of(bx1)) - 1, 0, S - 1)
        jhi = np.clip(np.ceil(pix_of(bx0)) + 1, 0, S - 1)
        ilo = np.clip(np.floor(pix_of(by1)) - 1, 0, S - 1)
        ihi = np.clip(np.ceil(pix_of(by0)) + 1, 0, S - 1)
    qc = T(1) - (2 * np.arange(S) + 1).astype(T) / T(S)                          # the centre of column j / row i
    undecided = np.zeros((S, S), bool)
    rows = []
    for f in np.nonzero(cand)[0]:
        i0, i1, j0, j1 = int(ilo[f]), int(ihi[f]) + 1, int(jlo[f]), int(jhi[f]) + 1
        qx, qy = np.meshgrid(qc[j0:j1], qc[i0:i1])
        inb = (qx >= bx0[f]) & (qx <= bx1[f]) & (qy >= by0[f]) & (qy <= by1[f])
        if not inb.any():
            continue
        x0, x1, x2, y0, y1, y2 = X[f, 0], X[f, 1], X[f, 2], Y[f, 0], Y[f, 1], Y[f, 2]
        z0, z1, z2 = Z[f]
        w0 = ((qx - x1) * (y2 - y1) - (qy - y1) * (x2 - x1)) / area[f]
        w1 = ((qx - x2) * (y0 - y2) - (qy - y2) * (x0 - x2)) / area[f]
        w2 = ((qx - x0) * (y1 - y0) - (qy - y0) * (x1 - x0)) / area[f]
        inside = (w0 > 0) & (w1 > 0) & (w2 > 0)
        d2 = np.minimum(_seg_d2(qx, qy, x0, y0, x1, y1, T), np.minimum(_seg_d2(qx, qy, x1, y1, x2, y2, T), _seg_d2(qx, qy, x2, y2, x0, y0, T)))
        covered = inb & (inside | (d2 < blur_t))
        near = inb & ((np.abs(w0) < 1e-5) | (np.abs(w1) < 1e-5) | (np.abs(w2) < 1e-5) |
                      (~inside & (np.abs(np.sqrt(d2) - r) < 1e-5)))
        undecided[i0:i1, j0:j1] |= near
        if not covered.any():
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            t0, t1, t2 = w0 / z0, w1 / z1, w2 / z2
            dn = t0 + t1 + t2
            p0, p1, p2 = (np.clip(x / dn, T(0), T(1)) for x in (t0, t1, t2))
            s = np.maximum(p0 + p1 + p2, T(1e-5))
            p0, p1, p2 = p0 / s, p1 / s, p2 / s
            z = p0 * z0 + p1 * z1 + p2 * z2
            sel = covered & (z >= 0)
        ii, jj = np.nonzero(sel)
        if len(ii):
            rows.append(np.stack([((ii + i0) * S + jj + j0).astype(np.float64), np.full(len(ii), float(f)), z[sel].astype(np.float64),
                                  np.where(inside, -d2, d2)[sel].astype(np.float64), p0[sel].astype(np.float64),
                                  p1[sel].astype(np.float64), p2[sel].astype(np.float64)], 1))
    image = np.empty((S * S, 4), T)
    image[:, :3] = f32(background)
    image[:, 3] = 0
    zbuf = np.full((S * S, K), -1, T)
    p2f = np.full((S * S, K), -1, np.int32)
    out = dict(covered=np.zeros((S, S), bool), undecided=undecided)
    if rows:
        fr = np.concatenate(rows)                                                # the float64 container holds T values exactly
        order = np.lexsort((fr[:, 1], fr[:, 2], fr[:, 0]))                       # by pixel, then depth, then face index
        fr = fr[order]
        pix = fr[:, 0].astype(np.int64)
        first = np.r_[True, pix[1:] != pix[:-1]]
        start = np.maximum.accumulate(np.where(first, np.arange(len(pix)), 0))
        rank = np.arange(len(pix)) - start
        nxt = (rank == K)                                                        # the (K+1)-th fragment of its pixel
        close = nxt & (fr[:, 2] - np.r_[0.0, fr[:-1, 2]] <= 1e-6)
        undecided.reshape(-1)[pix[close]] = True
        out["covered"].reshape(-1)[pix] = True
        keep = rank < K
        fr, pix, rank = fr[keep], pix[keep], rank[keep]
        face = fr[:, 1].astype(np.int64)
        zf, df = fr[:, 2].astype(T), fr[:, 3].astype(T)
        b = fr[:, 4:7].astype(T)
        zbuf[pix, rank] = zf
        p2f[pix, rank] = face
        i0, i1, i2 = F[face, 0], F[face, 1], F[face, 2]
        interp = lambda A: b[:, 0:1] * A[i0] + b[:, 1:2] * A[i1] + b[:, 2:3] * A[i2]
        P, Nn = interp(V), _unit(interp(N), T)
        tex = interp(f32(colors)) if colors is not None else np.ones_like(P)
        L = _unit(f32(lights["light"]) - P, T)
        c = (Nn * L).sum(-1)
        Vd = _unit(C - P, T)
        R = T(2) * c[:, None] * Nn - L
        sp = np.where(c > 0, np.maximum((Vd * R).sum(-1), T(0)), T(0))
        for _ in range(6):
            sp = sp * sp
        colour = (f32(lights["ambient"]) + f32(lights["diffuse"]) * np.maximum(c, T(0))[:, None]) * tex + f32(lights["specular"]) * sp[:, None]
        rng = zfar - znear
        zmin = zbuf[pix, 0]
        m_raw = (zfar - zmin) / rng
        clamped = ~(m_raw >= T(1e-10))
        m = np.where(clamped, T(1e-10), m_raw)
        e = np.where(clamped, (zfar - zf) / rng - m, (zmin - zf) / rng)
        with np.errstate(over="ignore", under="ignore"):
            prob = T(1) / (T(1) + np.exp(df / sigma_t))
            w = prob * np.exp(e / gamma_t)
            delta_f = np.maximum(np.exp((T(1e-10) - m) / gamma_t), T(1e-10))
        num, dsum, keepp, delta = np.zeros((S * S, 3), T), np.zeros(S * S, T), np.ones(S * S, T), np.zeros(S * S, T)
        for k in range(K):                                                       # in list order, as the kernel adds them
            q = rank == k
            num[pix[q]] += w[q, None] * colour[q]
            dsum[pix[q]] += w[q]
            keepp[pix[q]] *= T(1) - prob[q]
            if k == 0:
                delta[pix[q]] = delta_f[q]
        got = np.unique(pix)
        image[got, :3] = (num[got] + delta[got, None] * f32(background)) / (dsum[got] + delta[got])[:, None]
        image[got, 3] = T(1) - keepp[got]
    out.update(image=image.reshape(S, S, 4), zbuf=zbuf.reshape(S, S, K), pix_to_face=p2f.reshape(S, S, K))
    return out


# ---- scenes shared with the GPU tests and the fixture generator --------------------------------------------------------------------
def uv_sphere(radius=0.1, n_lat=32, n_lon=64):
    """(verts, faces, normals) of a UV sphere, float32 / int32: poles single vertices, outward winding, analytic normals."""
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.cos(th), np.ones(n_lon)), np.outer(np.sin(th), np.sin(ph))], -1)
    n = np.concatenate([[[0.0, 1.0, 0.0]], ring.reshape(-1, 3), [[0.0, -1.0, 0.0]]])
    idx = lambda a, b: 1 + a * n_lon + (b % n_lon)
    faces = []
    for b in range(n_lon):
        faces.append([0, idx(0, b + 1), idx(0, b)])
        faces.append([len(n) - 1, idx(n_lat - 2, b), idx(n_lat - 2, b + 1)])
        for a in range(n_lat - 2):
            faces.append([idx(a, b), idx(a, b + 1), idx(a + 1, b)])
            faces.append([idx(a + 1, b), idx(a, b + 1), idx(a + 1, b + 1)])
    faces = np.array(faces, np.int32)
    v = (radius * n).astype(np.float32)
    fn = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    assert ((fn * v[faces].mean(1)).sum(-1) > 0).all()
    return v, faces, n.astype(np.float32)


def height_field(n=32, seed=0):
    """An n x n xyz map (1, 3, n, n) float32 on the rays of generate_camera_params at (0, 0): a smooth bump around depth 1."""
    poses, focal, _, _, _ = generate_camera_params(n, "cpu", locations=torch.zeros(1, 2))
    o, dirs = rays(poses, focal, n)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    depth = 1.0 - 0.06 * np.exp(-(((i - n / 2.3) / (0.3 * n)) ** 2 + ((j - n / 1.9) / (0.25 * n)) ** 2)) + 0.01 * np.sin(0.7 * i) * np.cos(0.5 * j)
    pts = o + depth[..., None] * dirs
    return np.ascontiguousarray(pts.transpose(2, 0, 1)[None]).astype(np.float32), depth


def rays(poses, focal, res):
    """get_rays of the volume renderer in float64: origin (3,), directions (res, res, 3) of the pixel centres (+0.5), not normalised --
    a point o + s d has depth s."""
    c2w = poses[0].double().numpy()
    fo = float(focal.reshape(-1)[0])
    i, j = np.meshgrid(np.arange(res) + 0.5, np.arange(res) + 0.5, indexing="ij")           # i: row (y), j: column (x)
    dirs = np.stack([(j - res * 0.5) / fo, -(i - res * 0.5) / fo, -np.ones_like(i)], -1)
    return c2w[:, 3], dirs @ c2w[:, :3].T


# ---- 1. the camera -------------------------------------------------------------------------------------------------------------------
def test_camera_matches_the_volume_renderers_rays():
    rs = np.random.RandomState(3)
    pairs = np.stack([rs.uniform(-0.45, 0.45, 16), rs.uniform(-0.25, 0.25, 16)], 1)
    pairs[0] = 0
    for azim, elev in pairs:
        for res in (8, 64):
            poses, focal, _, _, viewpoint = generate_camera_params(res, "cpu", locations=torch.tensor([[azim, elev]], dtype=torch.float32))
            az, el = viewpoint[0].double().numpy()
            cam = mesh_utils.MeshCamera(np.rad2deg(az), np.rad2deg(el), fov=12.0)
            o, d = rays(poses, focal, res)
            want = np.stack(np.meshgrid(np.arange(res), np.arange(res), indexing="ij"), -1).astype(np.float64)
            for s in (0.88, 1.0, 1.12):
                p = o + s * d
                assert np.abs(cam.pixels(p, res) - want).max() < 1e-4
                assert np.abs(cam.view(p)[..., 2] - s).max() < 2e-6
    c = mesh_utils.MeshCamera(20.0, -10.0, 12.0)
    fl = c.floats()
    assert fl.dtype == np.float32 and fl.shape == (12,)
    R = fl[3:].reshape(3, 3).astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and np.linalg.det(R) > 0.99
    assert np.abs(c.view(np.zeros(3)) - [0, 0, 1]).max() < 1e-12                  # looks at the origin from distance 1


# ---- 2. the face list ----------------------------------------------------------------------------------------------------------------
def face_stats(faces, h, w):
    """(cell index of every face or -1, signed area in (column, row) index space)."""
    f = np.asarray(faces).astype(np.int64)
    r, c = f // w, f % w
    r0, c0 = r.min(1), c.min(1)
    in_cell = ((r.max(1) - r0) == 1) & ((c.max(1) - c0) == 1)
    ux, uy = c[:, 1] - c[:, 0], r[:, 1] - r[:, 0]
    vx, vy = c[:, 2] - c[:, 0], r[:, 2] - r[:, 0]
    return np.where(in_cell, r0 * (w - 1) + c0, -1), 0.5 * (ux * vy - uy * vx)


@pytest.mark.parametrize("n", [8, 128])
def test_depth_mesh_face_order_against_the_references_xyz2mesh(n):
    gold = np.load(os.path.join(GOLDEN, "xyz2mesh_faces.npz"))[f"faces_{n}"]
    ours = mesh_utils.depth_mesh_faces(n, n)
    assert ours.dtype == np.int32 and ours.shape == gold.shape == (2 * (n - 1) ** 2, 3)
    for faces in (ours, gold):
        cell, area = face_stats(faces, n, n)
        assert (cell >= 0).all()
        assert (np.bincount(cell, minlength=(n - 1) ** 2) == 2).all()
        assert (area == -0.5).all()
    # the documented order
    r, c = 3, 5
    k = 2 * (r * (n - 1) + c)
    assert ours[k].tolist() == [r * n + c, (r + 1) * n + c, r * n + c + 1]
    assert ours[k + 1].tolist() == [(r + 1) * n + c, (r + 1) * n + c + 1, r * n + c + 1]


# ---- 3. the restatement against closed forms -------------------------------------------------------------------------------------------
def phong_by_hand(P, N, C, lights, tex=1.0):
    N = N / np.linalg.norm(N)
    L = np.asarray(lights["light"], np.float64) - P
    L /= np.linalg.norm(L)
    c = N @ L
    Vd = (C - P) / np.linalg.norm(C - P)
    R = 2 * c * N - L
    spec = (max(Vd @ R, 0.0) if c > 0 else 0.0) ** 64
    return (np.asarray(lights["ambient"]) + np.asarray(lights["diffuse"]) * max(c, 0.0)) * tex + np.asarray(lights["specular"]) * spec


def blend_by_hand(colours, zs, d2s, zfar=100.0, znear=0.01, sigma=1e-4, gamma=1e-4):
    p = 1 / (1 + np.exp(-np.asarray(d2s) / sigma))                               # inside: d = -d2
    zi = (zfar - np.asarray(zs)) / (zfar - znear)
    m = max(zi.max(), 1e-10)
    w = p * np.exp((zi - m) / gamma)
    delta = max(np.exp((1e-10 - m) / gamma), 1e-10)
    return ((w[:, None] * np.asarray(colours)).sum(0) + delta * np.ones(3)) / (w.sum() + delta), 1 - np.prod(1 - p)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_one_triangle(dtype):
    cam = mesh_utils.MeshCamera(0.0, 0.0, 12.0)
    S, blur = 48, 1e-6
    # in the plane z = 0.1 (view depth 0.9), wound so that (v1 - v0) x (v2 - v0) faces the camera at (0, 0, 1)
    v = np.array([[-0.07, -0.05, 0.1], [0.08, -0.06, 0.1], [0.01, 0.075, 0.1]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (3, 1))
    out = restate_render(v, f, nrm, cam, S, 1, lights=DEFAULT_LIGHTS, blur=blur, dtype=dtype)
    ndc = cam.project(v.astype(np.float64))
    q = 1 - (2 * np.arange(S) + 1) / S
    qx, qy = np.meshgrid(q, q)
    side = []
    dist = []
    for k in range(3):
        a, b = ndc[k, :2], ndc[(k + 1) % 3, :2]
        e = b - a
        side.append(((qx - a[0]) * e[1] - (qy - a[1]) * e[0]) / np.linalg.norm(e))          # signed distance to the edge's line
        tt = np.clip(((qx - a[0]) * e[0] + (qy - a[1]) * e[1]) / (e @ e), 0, 1)
        dist.append(np.hypot(qx - a[0] - tt * e[0], qy - a[1] - tt * e[1]))
    side, dist = np.stack(side), np.stack(dist).min(0)
    sign = np.sign(side[:, S // 2, S // 2].sum())
    inside = (side * sign > 0).all(0)
    clear = (dist > 1e-6) & (np.abs(dist - np.sqrt(blur)) > 1e-6)
    covered = out["pix_to_face"][..., 0] == 0
    assert inside.sum() > 100 and np.array_equal(covered[clear], (inside | (dist < np.sqrt(blur)))[clear])
    assert np.abs(out["zbuf"][..., 0][covered & inside] - 0.9).max() < 1e-6
    assert (out["zbuf"][..., 0][~covered] == -1).all() and (out["image"][~covered] == [1, 1, 1, 0]).all()
    C = cam.position
    # float64: the restatement takes the camera as the kernel does, twelve float32 and a float32 tangent (relative rounding 6e-8; the
    # colour's sensitivity to them is of order 1); float32: a few dozen roundings of 6e-8 on values of order 1
    tol = 2e-7 if dtype == np.float64 else 2e-5
    ii, jj = np.nonzero(inside & (dist > 0.02))
    for n in (0, len(ii) // 2, len(ii) - 1):
        i, j = ii[n], jj[n]
        P = C + (0.9 / 1.0) * np.array([-qx[i, j] * cam.tan_half_fov, qy[i, j] * cam.tan_half_fov, -1.0])   # x_ax = (-1, 0, 0), z_ax = (0, 0, -1)
        assert abs(P[2] - 0.1) < 1e-12
        colour = phong_by_hand(P, np.array([0.0, 0.0, 1.0]), C, DEFAULT_LIGHTS)
        rgb, alpha = blend_by_hand([colour], [0.9], [dist[i, j] ** 2])
        assert np.abs(out["image"][i, j, :3] - rgb).max() < tol and abs(out["image"][i, j, 3] - alpha) < tol


@pytest.mark.parametrize("dz", [1e-3, 1e-2, 1e-1])
def test_restatement_two_parallel_quads(dz):
    cam = mesh_utils.MeshCamera(0.0, 0.0, 12.0)
    S = 16

    def quad(z, half):
        return np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]], np.float32)

    z_near, z_far = np.float32(0.1), np.float32(0.1 - dz)
    v = np.concatenate([quad(z_far, 0.3), quad(z_near, 0.3)])                     # the far quad first: order of the list is irrelevant
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (8, 1))
    col = np.concatenate([np.tile([[1.0, 0.2, 0.2]], (4, 1)), np.tile([[0.2, 0.4, 1.0]], (4, 1))]).astype(np.float32)
    out = restate_render(v, f, nrm, cam, S, 2, lights=RUNNER_LIGHTS, colors=col, dtype=np.float64)
    i, j = 5, 9                                                                  # off the diagonals of both quads
    assert sorted(out["pix_to_face"][i, j].tolist())[0] in (0, 1) and out["pix_to_face"][i, j, 0] in (2, 3)
    z1, z2 = 1.0 - float(z_near), 1.0 - float(z_far)
    assert np.abs(out["zbuf"][i, j] - [z1, z2]).max() < 1e-9
    q = 1 - (2 * np.arange(S) + 1) / S
    C = cam.position
    cols, d2s = [], []
    for z, tex, (lo, hi) in ((z1, col[4], (4, 8)), (z2, col[0], (0, 4))):
        P = C + z * np.array([-q[j] * cam.tan_half_fov, q[i] * cam.tan_half_fov, -1.0])
        cols.append(phong_by_hand(P, np.array([0.0, 0.0, 1.0]), C, RUNNER_LIGHTS, tex.astype(np.float64)))
        ndc = cam.project(v[lo:hi].astype(np.float64))[:, :2]
        face = out["pix_to_face"][i, j, 0 if lo == 4 else 1] - (2 if lo == 4 else 0)
        tri = ndc[[0, 1, 2]] if face == 0 else ndc[[0, 2, 3]]
        dd = []
        for k in range(3):
            a, e = tri[k], tri[(k + 1) % 3] - tri[k]
            tt = np.clip(((q[j] - a[0]) * e[0] + (q[i] - a[1]) * e[1]) / (e @ e), 0, 1)
            dd.append((q[j] - a[0] - tt * e[0]) ** 2 + (q[i] - a[1] - tt * e[1]) ** 2)
        d2s.append(min(dd))
    rgb, alpha = blend_by_hand(cols, [z1, z2], d2s)
    assert np.abs(out["image"][i, j, :3] - rgb).max() < 1e-7 and abs(out["image"][i, j, 3] - alpha) < 1e-9


def test_restated_normals_on_a_sphere_and_degenerate_faces():
    v, f, n = uv_sphere(0.1, 16, 32)
    got = restate_normals(v, f)
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-12
    assert (got * n).sum(-1).min() > np.cos(np.deg2rad(3.0))
    f2 = np.concatenate([f, [[0, 0, 5], [3, 3, 3]]]).astype(np.int32)             # zero-area faces add nothing
    v2 = np.concatenate([v, [[1.0, 2.0, 3.0]]]).astype(np.float32)                # a vertex without faces
    got2 = restate_normals(v2, f2)
    assert np.array_equal(got2[:-1], got) and (got2[-1] == 0).all()
    # one right triangle: the normal everywhere, whatever the angles
    tri = restate_normals(np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32), np.array([[0, 1, 2]]))
    assert np.abs(tri - [0, 0, 1]).max() < 1e-15


# ---- 4. the ABI ------------------------------------------------------------------------------------------------------------------------
def good_args(keep):
    """Arguments that pass every host-side check (the pointers are never followed: each case below breaks one check)."""
    a = _lib.MeshRenderArgs()
    buf = (ctypes.c_char * 64)()
    keep.append(buf)
    p = ctypes.addressof(buf)
    a.verts = a.faces = a.normals = a.image = a.zbuf = a.pix_to_face = a.status = a.ws = p
    a.n_verts, a.n_faces = 3, 1
    a.camera[:] = mesh_utils.MeshCamera(0, 0, 12).floats().tolist()
    a.tan_half_fov, a.znear, a.zfar = 0.1, 0.01, 100.0
    a.blur_radius, a.sigma, a.gamma = 1e-6, 1e-4, 1e-4
    a.image_size, a.faces_per_pixel = 64, 5
    a.bin_capacity = 16
    a.ws_bytes = 0                                                               # too small: a "good" call stops here, before any launch
    return a


def test_bad_arguments_are_refused_without_a_gpu(lib):
    keep = []
    render = lambda a: lib.e3dge_mesh_render(ctypes.byref(a), None)
    a = good_args(keep)
    assert render(a) == INVALID and b"workspace" in lib.e3dge_last_error()       # everything but the workspace is fine
    for field, value, word in [("faces_per_pixel", 0, b"faces_per_pixel"), ("faces_per_pixel", 9, b"faces_per_pixel"),
                               ("image_size", 0, b"image_size"), ("n_verts", -1, b"vertices"), ("n_faces", -1, b"faces"),
                               ("bin_capacity", -1, b"capacity"), ("image", None, b"null"), ("zbuf", None, b"null"),
                               ("pix_to_face", None, b"null"), ("status", None, b"null"), ("ws", None, b"null"), ("verts", None, b"null"),
                               ("faces", None, b"null"), ("normals", None, b"null"), ("sigma", 0.0, b"sigma")]:
        a = good_args(keep)
        a.ws_bytes = 1 << 40
        setattr(a, field, value)
        assert render(a) == INVALID, field
        assert word in lib.e3dge_last_error(), (field, lib.e3dge_last_error())
    assert lib.e3dge_mesh_render(None, None) == INVALID
    # 32-bit overflow of faces x tiles
    assert lib.e3dge_mesh_render_ws_bytes(10, 1 << 21, 512, 16) == -1 and b"32-bit" in lib.e3dge_last_error()
    assert lib.e3dge_mesh_render_ws_bytes(10, (1 << 21) - 1, 512, 16) > 0
    a = good_args(keep)
    a.n_faces, a.image_size, a.ws_bytes = 1 << 21, 512, 1 << 40
    assert render(a) == INVALID and b"32-bit" in lib.e3dge_last_error()
    assert lib.e3dge_mesh_render_ws_bytes(-1, 1, 64, 16) == -1 and lib.e3dge_mesh_render_ws_bytes(3, 1, 0, 16) == -1
    # depth mesh and normals
    p = ctypes.addressof(keep[0])
    assert lib.e3dge_depth_mesh(p, p, p, 0, 4, None) == INVALID and lib.e3dge_depth_mesh(None, p, p, 4, 4, None) == INVALID
    assert lib.e3dge_depth_mesh(p, None, p, 4, 4, None) == INVALID and lib.e3dge_depth_mesh(p, p, None, 4, 4, None) == INVALID
    assert lib.e3dge_vertex_normals_ws_bytes(-1) == -1 and lib.e3dge_vertex_normals_ws_bytes(10) >= 240
    assert lib.e3dge_vertex_normals(p, p, p, -1, 1, p, 1 << 20, None) == INVALID
    assert lib.e3dge_vertex_normals(p, p, p, 4, -1, p, 1 << 20, None) == INVALID
    assert lib.e3dge_vertex_normals(None, p, p, 4, 1, p, 1 << 20, None) == INVALID
    assert lib.e3dge_vertex_normals(p, p, p, 4, 1, p, 95, None) == INVALID and b"workspace" in lib.e3dge_last_error()


def test_python_surface_refuses_cpu_tensors_and_bad_settings():
    cam = mesh_utils.MeshCamera(0, 0, 12)
    with pytest.raises(ValueError, match="faces_per_pixel"):
        mesh_utils.create_depth_mesh_renderer(cam, faces_per_pixel=17)
    with pytest.raises(ValueError, match="faces_per_pixel"):
        mesh_utils.create_mesh_renderer(cam, faces_per_pixel=0)
    with pytest.raises(TypeError):
        mesh_utils.create_mesh_renderer(None)
    r = mesh_utils.create_mesh_renderer(cam, specular_color=((0.1, 0.2, 0.3),))
    assert r.image_size == 256 and r.faces_per_pixel == 5 and r.blur_radius == 1e-6
    assert r.ambient_color.tolist() == [0.5] * 3 and np.allclose(r.specular_color, [0.1, 0.2, 0.3]) and np.allclose(r.light_location, [-0.5, 1, 5])
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    for call in (lambda: mesh_utils.depth_mesh(torch.zeros(1, 3, 4, 4)), lambda: mesh_utils.vertex_normals(v, f), lambda: r(v, f),
                 lambda: mesh_utils.render_depth_mesh(torch.zeros(1, 3, 4, 4), torch.zeros(2)),
                 lambda: mesh_utils.render_surface_mesh(v, f, torch.zeros(2))):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
