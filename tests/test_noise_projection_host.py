"""View-consistent decoder noise, host side: pose_to_viewpoint, the numpy restatement of the subdivision rule in include/e3dge_hip.h
(e3dge_mesh_subdivide), the C-ABI of e3dge_noise_project / e3dge_mesh_subdivide, the OBJ reader and the projecting modules' construction.
The scenes and the restatement of the projection (restate_render of tests/test_mesh_render_host.py at K = 17 with ambient-only lights and
the noise as vertex colour) are shared with tests/test_gpu_noise_projection.py and tools/gen_noise_projection_report.py."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from conftest import REPO

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, mesh_utils
from e3dge_amd import synthetic as syn
from e3dge_amd.camera_utils import generate_camera_params
from test_mesh_render_host import restate_normals, restate_render, uv_sphere

INVALID = -1                                                        # E3DGE_ERR_INVALID_ARG
K_NOISE = 17
VIEWPOINTS = [(0.3, 0.15), (-0.45, 0.0), (0.1, -0.2), (0.0, 0.0)]
NOISE_LIGHTS = dict(light=(0.0, 0.0, 5.0), ambient=(1.0, 1.0, 1.0), diffuse=(0.0, 0.0, 0.0), specular=(0.0, 0.0, 0.0))
NOISE_SCENES = {"sphere_L0_S64": (0, 64), "sphere_L1_S64": (1, 64), "sphere_L1_S128": (1, 128)}        # name -> (level, S)


# ---- shared with the GPU tests and the report generator ------------------------------------------------------------------------------------
def restate_subdivide(verts, faces):
    """One level of the rule of include/e3dge_hip.h (e3dge_mesh_subdivide) in numpy: new vertex V + rank of the key lo V + hi among the
    distinct keys in ascending order, at 0.5f * (v_lo + v_hi) in float32; face f -> 4f .. 4f + 3."""
    v = np.asarray(verts, np.float32)
    f = np.asarray(faces).astype(np.int64)
    V = len(v)
    a, b = f, np.roll(f, -1, axis=1)                                             # sides (a, b), (b, c), (c, a)
    keys = np.minimum(a, b) * V + np.maximum(a, b)
    uniq, rank = np.unique(keys.reshape(-1), return_inverse=True)
    mid = np.float32(0.5) * (v[uniq // V] + v[uniq % V])
    m = V + rank.reshape(-1, 3)                                                  # m_ab, m_bc, m_ca
    out = np.stack([np.stack([f[:, 0], m[:, 0], m[:, 2]], 1), np.stack([m[:, 0], f[:, 1], m[:, 1]], 1),
                    np.stack([m[:, 2], m[:, 1], f[:, 2]], 1), np.stack([m[:, 0], m[:, 1], m[:, 2]], 1)], 1).reshape(-1, 3)
    return np.concatenate([v, mid.astype(np.float32)]), out.astype(np.int32)


def scene_mesh(level):
    """The UV sphere after `level` subdivisions (numpy restatement): (verts, faces)."""
    v, f, _ = uv_sphere()
    for _ in range(level):
        v, f = restate_subdivide(v, f)
    return v, f


def scene_noise(n_verts, seed=0, maps=1):
    """(maps, V) float32 of unit variance."""
    return np.random.RandomState(1000 + seed).standard_normal((maps, n_verts)).astype(np.float32)


def scene_camera(viewpoint=VIEWPOINTS[0]):
    return mesh_utils.MeshCamera(azim=np.rad2deg(viewpoint[0]), elev=np.rad2deg(viewpoint[1]), fov=12.0)


def restate_projection(verts, faces, noise, camera, S, K=K_NOISE, dtype=np.float64):
    """e3dge_noise_project's contract through restate_render: ambient-only lights, the field repeated into three colour channels.
    Returns restate_render's dict plus value (S, S) = channel 0 and valid = covered.  (The normals only enter terms multiplied by 0.)"""
    nrm = restate_normals(verts, faces, np.float64).astype(np.float32)
    col = np.repeat(np.asarray(noise, np.float32).reshape(-1, 1), 3, 1)
    out = restate_render(verts, faces, nrm, camera, S, K, lights=NOISE_LIGHTS, colors=col, dtype=dtype)
    out["value"] = out["image"][..., 0]
    return out


def edge_counts(faces, n_verts):
    f = np.asarray(faces).astype(np.int64)
    a, b = f, np.roll(f, -1, axis=1)
    return np.unique((np.minimum(a, b) * n_verts + np.maximum(a, b)).reshape(-1), return_counts=True)


def area_and_volume(verts, faces):
    p = np.asarray(verts, np.float64)[np.asarray(faces).astype(np.int64)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    return 0.5 * np.sqrt((n * n).sum(-1)).sum(), (p[:, 0] * np.cross(p[:, 1], p[:, 2])).sum() / 6.0


# ---- 1. the viewpoint of a pose ------------------------------------------------------------------------------------------------------------
def test_pose_to_viewpoint_returns_what_generate_camera_params_was_given():
    for azim, elev in VIEWPOINTS:
        poses, _, _, _, viewpoint = generate_camera_params(64, "cpu", locations=torch.tensor([[azim, elev]], dtype=torch.float32))
        got = mesh_utils.pose_to_viewpoint(poses)
        want = viewpoint[0].double().numpy()
        err = np.abs(np.asarray(got) - want).max()
        print(f"pose_to_viewpoint({azim}, {elev}): {got}, |error| = {err:.2e}")
        assert err <= 1e-6
        assert mesh_utils.pose_to_viewpoint(poses[0]) == got                     # (3, 4) as well as (b, 3, 4)
        cam = mesh_utils.noise_camera(poses)
        assert cam.fov == 12.0 and cam.dist == 1.0 and np.abs(cam.position - scene_camera((azim, elev)).position).max() < 2e-6


def test_pose_to_viewpoint_inverts_zyx_euler_angles():
    rs = np.random.RandomState(7)
    for _ in range(32):
        a0, a1, a2 = rs.uniform(-3.0, 3.0), rs.uniform(-1.5, 1.5), rs.uniform(-3.0, 3.0)
        c, s = np.cos, np.sin
        Rz = np.array([[c(a0), -s(a0), 0], [s(a0), c(a0), 0], [0, 0, 1]])
        Ry = np.array([[c(a1), 0, s(a1)], [0, 1, 0], [-s(a1), 0, c(a1)]])
        Rx = np.array([[1, 0, 0], [0, c(a2), -s(a2)], [0, s(a2), c(a2)]])
        pose = np.concatenate([Rz @ Ry @ Rx, rs.uniform(-1, 1, (3, 1))], 1)
        azim, elev = mesh_utils.pose_to_viewpoint(pose)
        assert abs(azim - a1) < 1e-12 and abs(elev + a2) < 1e-12
    with pytest.raises(ValueError):
        mesh_utils.pose_to_viewpoint(np.zeros((4, 4, 4, 4)))


def test_subdivision_levels_mirror_the_reference():
    assert [mesh_utils.subdivision_level(s) for s in (64, 128, 256, 512, 1024)] == [0, 0, 1, 3, 3]      # no size gets level 2


# ---- 2. the subdivision rule ---------------------------------------------------------------------------------------------------------------
def test_subdivision_rule_on_the_sphere():
    v, f, _ = uv_sphere()
    area0, vol0 = area_and_volume(v, f)
    area_bound = vol_bound = 0.0
    for level in (1, 2, 3):
        keys, counts = edge_counts(f, len(v))
        E = len(keys)
        v2, f2 = restate_subdivide(v, f)
        assert v2.dtype == np.float32 and f2.dtype == np.int32
        assert len(v2) == len(v) + E and len(f2) == 4 * len(f)
        assert np.array_equal(v2[:len(v)], v)
        # the documented order: new vertex V + rank, faces 4f .. 4f + 3
        lo, hi = keys // len(v), keys % len(v)
        assert np.array_equal(v2[len(v):], np.float32(0.5) * (v[lo] + v[hi]))
        assert np.array_equal(v2[len(v):], ((v[lo].astype(np.float64) + v[hi].astype(np.float64)) / 2).astype(np.float32))
        a, b, c = (int(x) for x in f[5])
        rank = lambda x, y: len(v) + int(np.searchsorted(keys, min(x, y) * len(v) + max(x, y)))
        assert f2[20:24].tolist() == [[a, rank(a, b), rank(c, a)], [rank(a, b), b, rank(b, c)], [rank(c, a), rank(b, c), c],
                                      [rank(a, b), rank(b, c), rank(c, a)]]
        keys2, counts2 = edge_counts(f2, len(v2))
        assert (counts2 == 2).all()                                              # closed and manifold: every edge in two faces
        assert len(v2) - len(keys2) + len(f2) == 2                               # Euler characteristic of the sphere
        # exact midpoints keep every face's plane: area and volume change only by the midpoints' rounding to float32.  A coordinate of
        # magnitude < 0.125 rounds by at most 2^-28, a vertex moves by d <= sqrt(3) 2^-28; a triangle's area changes by at most
        # perimeter d / 2 and the tetrahedron (0, a, b, c) by at most 3 r^2 d / 6 (r = max |v|): summed over the new faces
        d = np.sqrt(3.0) * 2.0 ** -28
        p = v2.astype(np.float64)[f2.astype(np.int64)]
        perimeter = np.sqrt(((np.roll(p, -1, 1) - p) ** 2).sum(-1)).sum()
        area_bound += perimeter * d / 2
        vol_bound += len(f2) * float(np.abs(v2).max()) ** 2 * 3 * d / 2
        area, vol = area_and_volume(v2, f2)
        print(f"level {level}: V = {len(v2)}, F = {len(f2)}, |area - area0| = {abs(area - area0):.2e} (bound {area_bound:.2e}), "
              f"|volume - volume0| = {abs(vol - vol0):.2e} (bound {vol_bound:.2e})")
        assert abs(area - area0) <= area_bound and abs(vol - vol0) <= vol_bound
        assert np.abs(v2).max() < 0.125
        v, f = v2, f2
    assert vol0 > 0                                                              # outward winding, kept by every level


def test_subdivision_follows_the_rule_on_repeated_indices_and_open_meshes():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    f = np.array([[0, 1, 2], [2, 1, 3], [3, 3, 0]], np.int32)                     # an open strip and a face with a repeated index
    v2, f2 = restate_subdivide(v, f)
    keys = sorted({min(a, b) * 4 + max(a, b) for t in f.tolist() for a, b in zip(t, t[1:] + t[:1])})
    assert len(v2) == 4 + len(keys) == 4 + 7 and len(f2) == 12
    k33 = 4 + keys.index(3 * 4 + 3)
    assert np.array_equal(v2[k33], v[3]) and f2[8].tolist() == [3, k33, 4 + keys.index(0 * 4 + 3)]


# ---- 3. the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_noise_project_args_struct_layout_matches_c():
    names = [n for n, _ in _lib.NoiseProjectArgs._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "e3dge_hip.h"\nint main(void) {\n  printf("%zu %d %d %d", sizeof(E3dgeNoiseProjectArgs), ' \
          'E3DGE_NOISE_PROJECT_FACES_PER_PIXEL, E3DGE_NOISE_PROJECT_MAX_MAPS, E3DGE_MESH_MAX_FACES_PER_PIXEL);\n' + \
          "".join(f'  printf(" %zu", offsetof(E3dgeNoiseProjectArgs, {n}));\n' for n in names) + "  return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        with open(c, "w") as fh:
            fh.write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    A = _lib.NoiseProjectArgs
    assert got == [ctypes.sizeof(A), _lib.NOISE_PROJECT_FACES_PER_PIXEL, _lib.NOISE_PROJECT_MAX_MAPS, 8] + [getattr(A, n).offset for n in names]
    assert _lib.NOISE_PROJECT_FACES_PER_PIXEL == K_NOISE and _lib.MESH_MAX_FACES_PER_PIXEL == 8


def good_args(keep):
    """Arguments that pass every host-side check (the pointers are never followed: each case below breaks one check)."""
    a = _lib.NoiseProjectArgs()
    buf = (ctypes.c_char * 64)()
    keep.append(buf)
    p = ctypes.addressof(buf)
    a.verts = a.faces = a.vert_noise = a.prev = a.out = a.valid = a.status = a.ws = p
    a.n_verts, a.n_faces = 3, 1
    a.camera[:] = mesh_utils.MeshCamera(0, 0, 12).floats().tolist()
    a.tan_half_fov, a.znear, a.zfar = 0.1, 0.01, 100.0
    a.blur_radius, a.sigma, a.gamma = 1e-6, 1e-4, 1e-4
    a.image_size, a.n_maps = 64, 2
    a.bin_capacity = 16
    a.ws_bytes = 0                                                               # too small: a "good" call stops here, before any launch
    return a


def test_bad_arguments_are_refused_without_a_gpu(lib):
    keep = []
    project = lambda a: lib.e3dge_noise_project(ctypes.byref(a), None)
    a = good_args(keep)
    assert project(a) == INVALID and b"workspace" in lib.e3dge_last_error()      # everything but the workspace is fine
    for field, value, word in [("image_size", 0, b"image_size"), ("image_size", -3, b"image_size"), ("n_maps", 0, b"n_maps"),
                               ("n_maps", 5, b"n_maps"), ("n_verts", -1, b"vertices"), ("n_faces", -1, b"faces"),
                               ("bin_capacity", -1, b"capacity"), ("bin_capacity", 2 ** 31 - 1, b"capacity"), ("out", None, b"null"),
                               ("valid", None, b"null"), ("prev", None, b"null"), ("status", None, b"null"), ("ws", None, b"null"),
                               ("verts", None, b"null"), ("faces", None, b"null"), ("vert_noise", None, b"null"), ("gamma", 0.0, b"gamma")]:
        a = good_args(keep)
        a.ws_bytes = 1 << 40
        setattr(a, field, value)
        assert project(a) == INVALID, field
        assert word in lib.e3dge_last_error(), (field, lib.e3dge_last_error())
    assert lib.e3dge_noise_project(None, None) == INVALID
    # 2^25 faces at S = 1024 are accepted (the public rasteriser stops below 2^19 there)
    assert lib.e3dge_noise_project_ws_bytes(1 << 24, 1 << 25, 1024, 1 << 27) > 0
    assert lib.e3dge_mesh_render_ws_bytes(1 << 24, 1 << 25, 1024, 1 << 27) == -1
    a = good_args(keep)
    a.n_verts, a.n_faces, a.image_size, a.bin_capacity = 1 << 24, 1 << 25, 1024, 1 << 27
    assert project(a) == INVALID and b"workspace" in lib.e3dge_last_error()
    assert lib.e3dge_noise_project_ws_bytes(-1, 1, 64, 16) == -1 and lib.e3dge_noise_project_ws_bytes(3, 1, 0, 16) == -1
    # subdivision
    p = ctypes.addressof(keep[0])
    sub = lib.e3dge_mesh_subdivide
    assert sub(p, p, p, p, p, p, -1, 1, 1, None) == INVALID and sub(p, p, p, p, p, p, 3, -1, 1, None) == INVALID
    assert sub(p, p, p, p, p, p, 3, 1, 4, None) == INVALID                        # more edges than face sides
    assert sub(p, p, p, p, p, p, 3, 1 << 29, 3, None) == INVALID                  # 4 F >= 2^31
    assert sub(p, p, p, p, p, p, (1 << 31) - 2, 1, 3, None) == INVALID            # V + E >= 2^31
    for k in range(6):
        args = [p] * 6
        args[k] = None
        assert sub(*args, 3, 1, 3, None) == INVALID and b"null" in lib.e3dge_last_error()


def test_python_surface_refuses_cpu_tensors_and_bad_settings():
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    cam = mesh_utils.MeshCamera(0, 0, 12)
    for call in (lambda: mesh_utils.subdivide(v, f), lambda: mesh_utils.project_vertex_noise(v, f, torch.zeros(1, 3), cam, 64),
                 lambda: mesh_utils.load_mesh((v, f))):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    with pytest.raises(TypeError):
        mesh_utils.load_mesh(3.5)
    with pytest.raises(ValueError, match="faces_per_pixel"):                     # the public rasteriser keeps its limit
        mesh_utils.create_depth_mesh_renderer(cam, faces_per_pixel=17)


# ---- 4. the modules --------------------------------------------------------------------------------------------------------------------------
def test_obj_reader_round_trips_surface_mesh_export(tmp_path):
    v, f = scene_mesh(1)
    v = (v * np.float32(1.2345678) + np.float32(1e-3)).astype(np.float32)          # values that need all nine digits
    path = tmp_path / "mesh.obj"
    mesh_utils.SurfaceMesh(v, f).export(str(path))
    v2, f2 = mesh_utils.read_obj(str(path))
    assert v2.dtype == np.float32 and f2.dtype == np.int32
    assert np.array_equal(v2.view(np.int32), v.view(np.int32)) and np.array_equal(f2, f)


def test_projecting_modules_construct_with_the_same_state_dict():
    from e3dge_amd.stylesdf_model import Decoder, G_pred_latents, NoiseInjection
    m = NoiseInjection(project=True)
    assert m.project and m.vert_noise is None and m.prev_noise is None and m.mesh_fn is None
    assert list(m.state_dict()) == list(NoiseInjection().state_dict()) == ["weight"]
    opt = lambda p: syn.model_opt(size=256, channel_multiplier=1, renderer_spatial_output_dim=64, project_noise=p)
    g1, g0 = (G_pred_latents(opt(p), syn.rendering_opt(N_samples=24), full_pipeline=True) for p in (True, False))
    assert list(g1.state_dict()) == list(g0.state_dict())
    assert all(c.noise.project for c in [g1.decoder.conv1] + list(g1.decoder.convs))
    assert not any(c.noise.project for c in [g0.decoder.conv1] + list(g0.decoder.convs))
    # a projecting decoder given noise names what it misses, before anything touches a device
    dec = g1.decoder
    assert isinstance(dec, Decoder)
    feats, latent = torch.zeros(1, 256, 64, 64), torch.zeros(1, dec.n_latent, dec.style_dim)
    with pytest.raises(ValueError, match="transform"):
        dec(feats, [latent], input_is_latent=True, randomize_noise=False, mesh_path="mesh.obj")
    with pytest.raises(ValueError, match="mesh_path"):
        dec(feats, [latent], input_is_latent=True, randomize_noise=False, transform=torch.eye(4)[None, :3])
    with pytest.raises(AssertionError, match="batch"):
        dec(torch.zeros(2, 256, 64, 64), [latent.repeat(2, 1, 1)], input_is_latent=True, randomize_noise=False,
            transform=torch.eye(4)[None, :3], mesh_path="mesh.obj")
