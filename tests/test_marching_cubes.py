"""Marching cubes in HIP (e3dge_marching_cubes_*, mesh_utils.marching_cubes): the case tables, a numpy restatement of the
kernels (same tables, same output order) against the reference's own output (skimage.measure.marching_cubes through
_extract_mesh_with_marching_cubes, volume_renderer.py:1733-1758; fixtures recorded by tools/gen_golden_marching_cubes.py), and the
HIP output against the restatement, bit for bit."""
import hashlib
import io
import json
import os

import numpy as np
import pytest
import torch

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, mesh_utils
from e3dge_amd import synthetic as syn

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REPORT = json.load(open(os.path.join(GOLD, "marching_cubes_report.json")))
CASES = list(REPORT["cases"])
CLOSED = ["blob", "torus", "twoblobs", "quantised", "noise"]
DEV = "cuda:0"
INVALID = -1                                                        # E3DGE_ERR_INVALID_ARG


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def edge_geometry():
    """(12, 4): axis and owner-corner offsets (dx, dy, dz) of edge e = 4 * axis + j (include/e3dge_hip.h)."""
    out = []
    for e in range(12):
        axis, j = e >> 2, e & 3
        o = [0, 0, 0]
        others = [a for a in range(3) if a != axis]
        o[others[0]], o[others[1]] = j & 1, j >> 1
        out.append([axis] + o)
    return np.array(out, np.int64)


def scene_transform(v, shape):
    """The reference's transform (volume_renderer.py:1747-1755) in fp32, in its order."""
    v = v.copy()
    for a in range(3):
        v[:, a] = (v[:, a] / np.float32(shape[a]) - np.float32(0.5)) * np.float32(0.24)
    v[:, 2] *= -1
    v[:, 1] *= -1
    return v


def restate(vol, tables, scene=True):
    """vol (nx, ny, nz) float32 in skimage's axes -> (verts, faces) in the kernels' order: vertices by point then +x, +y, +z edge,
    faces by cell then table order."""
    n_tris, tri = tables
    nx, ny, nz = vol.shape
    pos = vol > 0
    cross = np.zeros(vol.shape + (3,), bool)
    cross[:-1, :, :, 0] = pos[:-1] != pos[1:]
    cross[:, :-1, :, 1] = pos[:, :-1] != pos[:, 1:]
    cross[:, :, :-1, 2] = pos[:, :, :-1] != pos[:, :, 1:]
    flat = cross.reshape(-1, 3)
    voff = np.concatenate([[0], np.cumsum(flat.sum(1))[:-1]]).astype(np.int64)
    mask = flat[:, 0] + 2 * flat[:, 1] + 4 * flat[:, 2]
    p, ax = np.nonzero(flat)
    idx = np.stack(np.unravel_index(p, vol.shape), 1)
    step = np.array([ny * nz, nz, 1])
    a = vol.reshape(-1)[p].astype(np.float64)
    b = vol.reshape(-1)[p + step[ax]].astype(np.float64)
    rows = np.arange(len(p))
    verts = idx.astype(np.float32)
    verts[rows, ax] = (idx[rows, ax] + (0.0 - a) / (b - a)).astype(np.float32)
    if scene:
        verts = scene_transform(verts, vol.shape)
    cas = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for k in range(8):
        dx, dy, dz = k & 1, (k >> 1) & 1, (k >> 2) & 1
        cas |= pos[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << k
    cx, cy, cz = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing="ij")
    cp = ((cx * ny + cy) * nz + cz).reshape(-1)
    c = cas.reshape(-1)
    cell, t = np.nonzero(np.arange(tri.shape[1])[None, :] < n_tris[c][:, None])
    e = tri[c[cell], t]
    geo = edge_geometry()
    owner = cp[cell][:, None] + geo[e, 1] * ny * nz + geo[e, 2] * nz + geo[e, 3]
    below = mask[owner] & ((1 << geo[e, 0]) - 1)
    faces = voff[owner] + (below & 1) + ((below >> 1) & 1)
    return verts, faces.astype(np.int32)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables():
    return mesh_utils.marching_cubes_tables()


def gold(name):
    return np.load(os.path.join(GOLD, f"marching_cubes_{name}.npz"))


def aligned_of(name):
    """(1, h, w, d, 1) float32 input of the case; analytic volumes are rebuilt and checked against the recorded sha256."""
    if name == "render":
        vol = gold(name)["aligned_sdf"]
    else:
        vol = syn.mc_volume(name).reshape(1, *syn.MC_VOLUMES[name], 1)
    assert hashlib.sha256(np.ascontiguousarray(vol).tobytes()).hexdigest() == REPORT["cases"][name]["sha256"]
    return vol


def skimage_view(aligned):
    return np.ascontiguousarray(aligned[0, ..., 0].transpose(1, 0, 2))      # sdf[0, ..., 0].permute(1, 0, 2)


def rows_sorted(v):
    """Rows as raw bits, sorted: a multiset of vertices compared bit for bit."""
    b = np.ascontiguousarray(v.astype(np.float32)).view(np.int32).reshape(-1, 3)
    return b[np.lexsort(b.T[::-1])]


def directed_edges(f):
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_watertight(f):
    d = directed_edges(f.astype(np.int64))
    key = d[:, 0] * (1 << 32) + d[:, 1]
    u = np.sort(d, 1)
    ukey = u[:, 0] * (1 << 32) + u[:, 1]
    _, dcount = np.unique(key, return_counts=True)
    _, ucount = np.unique(ukey, return_counts=True)
    return bool((dcount == 1).all() and (ucount == 2).all())


def euler(v, f):
    u = np.sort(directed_edges(f.astype(np.int64)), 1)
    n_edges = len(np.unique(u[:, 0] * (1 << 32) + u[:, 1]))
    return len(v) - n_edges + len(f)


def signed_volume(v, f):
    v = v.astype(np.float64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6)


def area(v, f):
    v = v.astype(np.float64)
    return float(np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1).sum() / 2)


def normal_dot_gradient(v, f, vol):
    """Area-weighted sum of (face normal . volume gradient at the nearest grid point of the centroid), in index space."""
    v = v.astype(np.float64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    g = np.stack(np.gradient(vol.astype(np.float64)), -1)
    c = np.clip(np.rint(v[f].mean(1)).astype(np.int64), 0, np.array(vol.shape) - 1)
    return np.einsum("ij,ij->i", n, g[c[:, 0], c[:, 1], c[:, 2]])


def check_against_skimage(name, verts_idx, faces, vol, g):
    """The checks of the contract against skimage's own mesh: verts_idx in index space (skimage's frame)."""
    sk_v, sk_f, ref_v = g["sk_verts"], g["sk_faces"], g["ref_verts"]
    on_edge = (sk_v == np.floor(sk_v)).sum(1) >= 2
    # one vertex per crossing edge, bit-identical to the reference's (transformed) edge vertices
    assert len(verts_idx) == int(on_edge.sum()) == REPORT["cases"][name]["n_edge_verts"]
    assert np.array_equal(rows_sorted(scene_transform(verts_idx, vol.shape)), rows_sorted(ref_v[on_edge]))
    assert np.array_equal(rows_sorted(verts_idx), rows_sorted(sk_v[on_edge]))
    assert faces.dtype == np.int32 and faces.min() >= 0 and faces.max() < len(verts_idx)
    if name in ("blob", "torus"):
        assert len(faces) == len(sk_f)
        assert euler(verts_idx, faces) == {"blob": 2, "torus": 0}[name] == euler(sk_v, sk_f)
    if name in CLOSED:
        assert is_watertight(faces)
        vo, vs = signed_volume(verts_idx, faces), signed_volume(sk_v, sk_f)
        assert np.sign(vo) == np.sign(vs) != 0
        if name != "noise":                                            # measured: 0.12 % or less
            assert abs(vo - vs) <= 0.005 * abs(vs)
    ng, ng_sk = normal_dot_gradient(verts_idx, faces, vol), normal_dot_gradient(sk_v, sk_f, vol)
    assert np.sign(ng.sum()) == np.sign(ng_sk.sum()) != 0
    # measured |area - skimage's| / skimage's: 0.04 % or less on blob, torus, quantised and border, 0.6 % on the two blobs, 0.8 % on the
    # noise volume and 4.3 % on the rendered one (synthetic weights: a rough surface with many ambiguous cells, tiled differently)
    tol = {"twoblobs": 0.01, "noise": 0.015, "render": 0.06}.get(name, 0.002)
    a, a_sk = area(verts_idx, faces), area(sk_v, sk_f)
    assert abs(a - a_sk) <= tol * a_sk, (a, a_sk)


# ---- CPU: the tables, the restatement against the reference, the C-ABI's argument checks ---------------------------------------------
def test_marching_cubes_symbols_exported(lib):
    for name in ("e3dge_marching_cubes_ws_bytes", "e3dge_marching_cubes_count", "e3dge_marching_cubes_emit", "e3dge_marching_cubes_tables"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_tables_close_every_loop(tables):
    n_tris, tri = tables
    geo = edge_geometry()
    corner = lambda ax, dx, dy, dz: dx + 2 * dy + 4 * dz
    ends = [(corner(*geo[e]), corner(*geo[e]) + (1 << geo[e, 0])) for e in range(12)]
    assert n_tris[0] == n_tris[255] == 0 and n_tris.max() <= _lib.MC_MAX_TRIS
    for c in range(256):
        t = tri[c, :n_tris[c]]
        assert (tri[c, n_tris[c]:] == -1).all()
        crossing = {e for e in range(12) if ((c >> ends[e][0]) & 1) != ((c >> ends[e][1]) & 1)}
        assert set(t.reshape(-1).tolist()) == crossing, c              # no triangle uses a non-crossing edge; every crossing edge is used
        # loop segments = directed triangle edges whose reverse is not there (the fan's diagonals come in both directions)
        d = [tuple(x) for x in directed_edges(t).tolist()]
        seg = [s for s in d if (s[1], s[0]) not in d]
        assert len(seg) == len(set(seg))
        for e in crossing:
            assert sum(s[0] == e for s in seg) == 1 and sum(s[1] == e for s in seg) == 1, c
        faces_of = lambda e: {(ax, int(geo[e, 1 + ax])) for ax in range(3) if ax != geo[e, 0]}   # (axis, side) of its two faces
        for a, b in seg:                                                   # a segment lies on one face of the cube
            assert len(faces_of(a) & faces_of(b)) == 1, c


@pytest.mark.parametrize("name", CASES)
def test_restatement_against_the_reference(tables, name):
    aligned = aligned_of(name)
    vol = skimage_view(aligned)
    v_idx, f = restate(vol, tables, scene=False)
    check_against_skimage(name, v_idx, f, vol, gold(name))
    v, f2 = restate(vol, tables)
    assert np.array_equal(f, f2) and np.array_equal(v.view(np.int32), scene_transform(v_idx, vol.shape).view(np.int32))
    if name == "border":
        assert not is_watertight(f)                                        # open where the sphere leaves the box


def test_cases_cover_ambiguous_faces_and_zeros():
    # the two-blob neck and the noise volume have ambiguous faces, the quantised sphere exact zeros
    def ambiguous_faces(vol):
        pos = vol > 0
        n = 0
        for ax in range(3):
            p = np.moveaxis(pos, ax, 0)
            a, b, c, d = p[:, :-1, :-1], p[:, 1:, :-1], p[:, 1:, 1:], p[:, :-1, 1:]
            n += int(((a == c) & (b == d) & (a != b)).sum())
        return n
    assert ambiguous_faces(skimage_view(aligned_of("twoblobs"))) > 0
    assert ambiguous_faces(skimage_view(aligned_of("noise"))) > 100
    assert REPORT["cases"]["quantised"]["n_exact_zeros"] > 100


def test_c_abi_rejects_bad_arguments(lib):
    nb = lib.e3dge_marching_cubes_ws_bytes(4, 5, 6)
    assert nb > 0
    assert lib.e3dge_marching_cubes_ws_bytes(1, 5, 6) == -1 and lib.e3dge_marching_cubes_ws_bytes(4, 5, 0) == -1
    assert lib.e3dge_marching_cubes_ws_bytes(2048, 2048, 2048) == -1                      # 32-bit offsets
    fake = 1 << 20                                                                       # never dereferenced: rejected first
    count = lambda *a: lib.e3dge_marching_cubes_count(*a)
    assert count(None, fake, nb, fake, 4, 5, 6, 30, 6, 1, None) == INVALID
    assert count(fake, None, nb, fake, 4, 5, 6, 30, 6, 1, None) == INVALID
    assert count(fake, fake, nb, None, 4, 5, 6, 30, 6, 1, None) == INVALID
    assert count(fake, fake, nb, fake, 1, 5, 6, 30, 6, 1, None) == INVALID
    assert count(fake, fake, nb - 1, fake, 4, 5, 6, 30, 6, 1, None) == INVALID
    assert count(fake, fake, nb, fake, 2048, 2048, 2048, 30, 6, 1, None) == INVALID
    emit = lambda *a: lib.e3dge_marching_cubes_emit(*a)
    assert emit(None, fake, 3, 1, fake, nb, fake, 4, 5, 6, 30, 6, 1, 1, None) == INVALID
    assert emit(fake, None, 3, 1, fake, nb, fake, 4, 5, 6, 30, 6, 1, 1, None) == INVALID
    assert emit(fake, fake, -1, 1, fake, nb, fake, 4, 5, 6, 30, 6, 1, 1, None) == INVALID
    assert emit(fake, fake, 3, 1, None, nb, fake, 4, 5, 6, 30, 6, 1, 1, None) == INVALID
    assert emit(fake, fake, 3, 1, fake, nb, None, 4, 5, 6, 30, 6, 1, 1, None) == INVALID
    assert emit(fake, fake, 3, 1, fake, nb - 1, fake, 4, 5, 6, 30, 6, 1, 1, None) == INVALID
    assert emit(fake, fake, 3, 1, fake, nb, fake, 4, 1, 6, 30, 6, 1, 1, None) == INVALID
    assert lib.e3dge_marching_cubes_tables(None, fake) == INVALID
    assert "marching_cubes" in lib.e3dge_last_error().decode()


def test_python_errors_without_a_gpu():
    with pytest.raises(ValueError, match=r"^Input array must be at least 2x2x2\.$"):
        mesh_utils.marching_cubes(torch.zeros(1, 2, 1, 2, 1))
    with pytest.raises(RuntimeError, match="GPU"):
        mesh_utils.marching_cubes(torch.zeros(1, 2, 2, 2, 1))                           # no CPU path
    assert issubclass(mesh_utils.NoSurfaceError, RuntimeError)


def test_surface_mesh_obj_round_trip(tables):
    v, f = restate(skimage_view(aligned_of("torus")), tables)
    m = mesh_utils.SurfaceMesh(torch.from_numpy(v), torch.from_numpy(f))
    assert m.vertices.dtype == np.float32 and m.faces.dtype == np.int32
    for sink in (io.StringIO(), io.BytesIO()):
        m.export(sink, file_type='obj')
        text = sink.getvalue()
        v2, f2 = parse_obj(text.decode() if isinstance(text, bytes) else text)
        assert np.array_equal(v2.view(np.int32), v.view(np.int32)) and np.array_equal(f2, f)
    with pytest.raises(ValueError):
        m.export(io.StringIO(), file_type='ply')


def parse_obj(text):
    v, f = [], []
    for line in text.splitlines():
        parts = line.split()
        if parts and parts[0] == "v":
            v.append([float(x) for x in parts[1:4]])
        elif parts and parts[0] == "f":
            f.append([int(x.split("/")[0]) - 1 for x in parts[1:4]])
    return np.array(v, np.float32).reshape(-1, 3), np.array(f, np.int32).reshape(-1, 3)


# ---- GPU: the HIP kernels against the restatement (bit for bit, order included) and the reference ---------------------------------------
def hip(aligned, scene=True):
    t = aligned if isinstance(aligned, torch.Tensor) else torch.from_numpy(aligned)
    v, f = mesh_utils.marching_cubes(t.to(DEV), scene=scene)
    torch.cuda.synchronize()
    return v.cpu().numpy(), f.cpu().numpy()


def assert_same(a, b):
    (va, fa), (vb, fb) = a, b
    assert va.dtype == vb.dtype == np.float32 and fa.dtype == fb.dtype == np.int32
    assert va.shape == vb.shape and fa.shape == fb.shape
    assert np.array_equal(va.view(np.int32), vb.view(np.int32))
    assert np.array_equal(fa, fb)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_equals_restatement_and_matches_the_reference(tables, name):
    aligned = aligned_of(name)
    vol = skimage_view(aligned)
    out = hip(aligned)
    assert_same(out, restate(vol, tables))
    out_idx = hip(aligned, scene=False)
    assert_same(out_idx, restate(vol, tables, scene=False))
    check_against_skimage(name, out_idx[0], out_idx[1], vol, gold(name))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,seed", [((2, 2, 2), 0), ((2, 2, 2), 1), ((17, 33, 20), 2), ((5, 3, 70), 3), ((33, 9, 40), 4),
                                        ((64, 64, 64), 5)])
def test_hip_equals_restatement_on_random_volumes(tables, shape, seed):
    rs = np.random.RandomState(seed)
    for trial in range(4 if shape == (2, 2, 2) else 1):
        vol = rs.uniform(-1, 1, size=(1, *shape, 1)).astype(np.float32)
        if seed == 3:
            vol = np.round(vol * 2).astype(np.float32) / 2                       # exact zeros
        if not ((vol > 0).any() and (vol <= 0).any()):
            continue
        assert_same(hip(vol), restate(skimage_view(vol), tables))


@pytest.mark.gpu
def test_hip_reads_through_strides(tables):
    # channel 0 of a 3-channel, 2-sample volume (a strided view, not copied) and a permuted view
    rs = np.random.RandomState(9)
    base = rs.normal(size=(2, 13, 11, 17, 3)).astype(np.float32)
    ref = restate(skimage_view(base[:1, ..., :1]), tables)
    assert_same(hip(torch.from_numpy(base)), ref)
    t = torch.from_numpy(np.ascontiguousarray(base.transpose(0, 3, 1, 2, 4))).to(DEV).permute(0, 2, 3, 1, 4)   # d-major storage
    v, f = mesh_utils.marching_cubes(t)
    assert_same((v.cpu().numpy(), f.cpu().numpy()), ref)


@pytest.mark.gpu
def test_hip_errors_mirror_skimage():
    with pytest.raises(ValueError, match=r"^Surface level must be within volume data range\.$"):
        mesh_utils.marching_cubes(torch.ones(1, 4, 5, 6, 1, device=DEV))
    with pytest.raises(ValueError, match=r"^Surface level must be within volume data range\.$"):
        mesh_utils.marching_cubes(-torch.ones(1, 4, 5, 6, 1, device=DEV))
    z = -torch.ones(1, 4, 5, 6, 1, device=DEV)
    z[0, 1, 2, 3, 0] = 0                                                         # 0 in range, but a zero is negative: no crossing
    with pytest.raises(mesh_utils.NoSurfaceError, match=r"^No surface found at the given iso value\.$"):
        mesh_utils.marching_cubes(z)
    with pytest.raises(ValueError, match=r"^Input array must be at least 2x2x2\.$"):
        mesh_utils.marching_cubes(torch.zeros(1, 2, 2, 1, 1, device=DEV))
    one = torch.ones(1, 3, 3, 3, 1, device=DEV)
    one[0, 1, 1, 1, 0] = 0                                                       # a zero centre: the same mesh as a negative one
    neg = one.clone()
    neg[0, 1, 1, 1, 0] = -1
    v0, f0 = mesh_utils.marching_cubes(one, scene=False)
    v1, f1 = mesh_utils.marching_cubes(neg, scene=False)
    assert v0.shape == v1.shape == (6, 3) and f0.shape == f1.shape == (8, 3) and torch.equal(f0, f1)


def surface_volume():
    """The 128^3 aligned volume of bench.py's surface leg (128 x 128 rays x 128 samples, synthetic weights) and its renderer."""
    from e3dge_amd.camera_utils import generate_camera_params
    from e3dge_amd.volume_renderer import VolumeFeatureRenderer
    r = VolumeFeatureRenderer(syn.rendering_opt(N_samples=128), out_im_res=128, mode='test')
    syn.load_synthetic(r, prefix='renderer.')
    r = r.to(DEV)
    ws, _ = syn.synthetic_inputs(1, seed=1, device=DEV)
    ps, fs, ns, fas, _ = generate_camera_params(128, DEV, locations=torch.zeros(1, 2, device=DEV))
    with torch.no_grad():
        o = r(ps, fs, ns, fas, styles=ws)
        return mesh_utils.align_volume(o['sdf'])


@pytest.mark.gpu
def test_full_size_surface_volume():
    aligned = surface_volume()
    vol = aligned[0, ..., 0].permute(1, 0, 2)                                    # skimage's (x, y, z), a view
    pos = vol > 0
    n_cross = int((pos[1:] != pos[:-1]).sum() + (pos[:, 1:] != pos[:, :-1]).sum() + (pos[:, :, 1:] != pos[:, :, :-1]).sum())
    v, f = mesh_utils.marching_cubes(aligned, scene=False)
    assert v.shape[0] == n_cross > 1000 and f.shape[0] > n_cross
    # every vertex interpolates to 0 on its edge: vertex k belongs to the k-th crossing edge in (point, axis) order
    flags = torch.zeros(*vol.shape, 3, dtype=torch.bool, device=DEV)
    flags[:-1, :, :, 0] = pos[1:] != pos[:-1]
    flags[:, :-1, :, 1] = pos[:, 1:] != pos[:, :-1]
    flags[:, :, :-1, 2] = pos[:, :, 1:] != pos[:, :, :-1]
    p, ax = flags.reshape(-1, 3).nonzero(as_tuple=True)
    nx, ny, nz = vol.shape
    idx = torch.stack([p // (ny * nz), (p // nz) % ny, p % nz], 1)
    rows = torch.arange(len(p), device=DEV)
    other = torch.ones_like(idx, dtype=torch.bool)
    other[rows, ax] = False
    assert torch.equal(v[other], idx[other].float())                             # on the grid line of its edge
    flat = vol.contiguous().reshape(-1).double()
    a = flat[p]
    b = flat[p + torch.tensor([ny * nz, nz, 1], device=DEV)[ax]]
    i = idx[rows, ax].double()
    t = v[rows, ax].double() - i
    assert ((a > 0) != (b > 0)).all() and bool((t >= 0).all()) and bool((t <= 1).all())
    # float32(i + t) is within half an ulp of i + 1 of the exact root
    assert bool(((a + t * (b - a)).abs() <= (b - a).abs() * (i + 1) * 2.0 ** -23).all())
    # manifold and closed where the volume's border is positive (align_volume puts 1 outside the frustum)
    fn = f.cpu().numpy()
    border = torch.cat([vol[0].flatten(), vol[-1].flatten(), vol[:, 0].flatten(), vol[:, -1].flatten(), vol[:, :, 0].flatten(),
                        vol[:, :, -1].flatten()])
    if bool((border > 0).all()):
        assert is_watertight(fn)
    else:
        u = np.sort(directed_edges(fn.astype(np.int64)), 1)
        _, cnt = np.unique(u[:, 0] * (1 << 32) + u[:, 1], return_counts=True)
        assert cnt.max() <= 2
    # deterministic: two calls give the same bits, scene coordinates too
    v2, f2 = mesh_utils.marching_cubes(aligned, scene=False)
    assert torch.equal(v.view(torch.int32), v2.view(torch.int32)) and torch.equal(f, f2)
    s1, g1 = mesh_utils.marching_cubes(aligned)
    s2, g2 = mesh_utils.marching_cubes(aligned)
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and torch.equal(g1, f) and torch.equal(g2, f)


def generator(res=32):
    from e3dge_amd.stylesdf_model import G_pred_latents
    g = G_pred_latents(syn.model_opt(size=128, channel_multiplier=1, renderer_spatial_output_dim=res),
                       syn.rendering_opt(N_samples=res), full_pipeline=True)
    syn.load_synthetic(g)
    return g.to(DEV).eval()


@pytest.mark.gpu
def test_generator_return_mesh():
    from e3dge_amd.camera_utils import generate_camera_params
    res = 32
    g = generator(res)
    wr, wd = syn.synthetic_inputs(1, seed=1, device=DEV)
    wd = wd[:, :g.decoder.n_latent]
    poses, focal, near, far, _ = generate_camera_params(res, DEV, locations=torch.zeros(1, 2, device=DEV))
    with torch.no_grad():
        out = g([wr, wd], poses, focal, near, far, input_is_latent=True, randomize_noise=False, return_mesh=True)
    mv, mf = out['mesh_verts'], out['mesh_faces']
    assert mv.is_cuda and mf.is_cuda and mv.dtype == torch.float32 and mf.dtype == torch.int32 and len(mf) > 0
    assert 'mesh_error' not in out
    v, f = mesh_utils.marching_cubes(out['aligned_sdf'])
    assert torch.equal(v.view(torch.int32), mv.view(torch.int32)) and torch.equal(f, mf)
    mesh = out['mesh']
    assert mesh is not None and out['shaded_mesh'] is mesh
    if isinstance(mesh, mesh_utils.SurfaceMesh):
        assert np.array_equal(mesh.vertices.view(np.int32), mv.cpu().numpy().view(np.int32))
        assert np.array_equal(mesh.faces, mf.cpu().numpy())
        buf = io.StringIO()
        mesh.export(buf, file_type='obj')
        v2, f2 = parse_obj(buf.getvalue())
        assert np.array_equal(v2.view(np.int32), mesh.vertices.view(np.int32)) and np.array_equal(f2, mesh.faces)
    else:                                                                        # third-party mesh (skimage + trimesh installed)
        assert len(mesh.vertices) > 0 and len(mesh.faces) > 0
    # an all-positive volume: no mesh, skimage's message
    with torch.no_grad():
        g.renderer.network.sigma_linear.bias.add_(1e4)
        out2 = g([wr, wd], poses, focal, near, far, input_is_latent=True, randomize_noise=False, return_mesh=True)
    assert bool((out2['aligned_sdf'] > 0).all())
    assert out2['mesh'] is None and out2['shaded_mesh'] is None
    assert out2['mesh_error'] == "Surface level must be within volume data range."
    assert out2['mesh_verts'].shape == (0, 3) and out2['mesh_faces'].shape == (0, 3)
