"""Surface renderings on the GPU (csrc/mesh_render.hip through mesh_utils): depth_mesh, vertex_normals and the rasteriser against the
float64 run of the numpy restatement in tests/test_mesh_render_host.py.  The bounds are 3 x the yardsticks recorded by
tools/gen_golden_mesh_render.py in tests/golden/mesh_render_report.json: the distance of the restatement's own float32 run from its
float64 run on the same scene (the factor for "an independent fp32 implementation").  A pixel is compared when it is
decided in float64 (restate_render's docstring); undecided pixels may be at most 2 % of a scene's covered pixels."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, record

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, mesh_utils
from e3dge_amd import synthetic as syn
from e3dge_amd.camera_utils import generate_camera_params
import test_mesh_render_host as host

DEV = "cuda:0"
RES, N_SAMPLES, STYLE_SEED = 32, 24, 1
RENDER_VIEW = (0.1, -0.05)                                          # (azim, elev) in radians of the depth-mesh scene's xyz map
LOOP_VIEWS = [(0.0, 0.0), (0.25, -0.1), (-0.4, 0.2)]
SCENES, KS, SIZES = ("sphere", "depth", "torus"), (1, 5), (64, 250)
FACTOR = 3.0


def report():
    with open(os.path.join(GOLDEN, "mesh_render_report.json")) as f:
        return json.load(f)


def scene_key(name, K, S):
    return f"{name}_K{K}_S{S}"


def scene_camera(name):
    """(camera, lights) a scene is drawn with."""
    if name == "sphere":
        return mesh_utils.MeshCamera(10.0, 5.0, 12.0), host.DEFAULT_LIGHTS
    if name == "depth":                                             # 7 degrees of azimuth and 3 of elevation away from where it was rendered
        return mesh_utils.MeshCamera(np.rad2deg(RENDER_VIEW[0]) + 7.0, np.rad2deg(RENDER_VIEW[1]) + 3.0, 12.0), host.RUNNER_LIGHTS
    # the torus: the issue's viewpoint (azim 0.3, elev 0.15 rad) leaves 2.5 % (S = 64) and 2.1 % (S = 250) of the covered pixels undecided at
    # K = 1 in float64 alone -- with ~4 faces per pixel at S = 64 the share is set by the mesh's edge density: 1.6-3.3 % over 18 viewpoints
    # and sizes tried.  Replaced, as the issue prescribes, by the viewpoint with the lowest share; the 2 % cap stays.
    return mesh_utils.MeshCamera(np.rad2deg(0.45), np.rad2deg(0.25), 12.0), host.SURFACE_LIGHTS


def max_angle(a, b):
    """Largest angle (radians) between corresponding rows, from the cross product (accurate for small angles); two zero rows: 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = np.linalg.norm(np.cross(a, b), axis=1)
    flipped = (a * b).sum(1) < 0
    zero_mismatch = (np.abs(a).sum(1) == 0) != (np.abs(b).sum(1) == 0)
    return float(np.where(flipped | zero_mismatch, np.pi, np.arcsin(np.minimum(s, 1.0))).max())


@functools.lru_cache(maxsize=None)
def volume_render(view):
    from e3dge_amd.volume_renderer import VolumeFeatureRenderer
    r = VolumeFeatureRenderer(syn.rendering_opt(N_samples=N_SAMPLES), out_im_res=RES, mode='test')
    syn.load_synthetic(r, prefix='renderer.')
    r = r.to(DEV)
    ws, _ = syn.synthetic_inputs(1, seed=STYLE_SEED, device=DEV)
    ps, fs, ns, fas, vp = generate_camera_params(RES, DEV, locations=torch.tensor([view], dtype=torch.float32, device=DEV))
    with torch.no_grad():
        o = r(ps, fs, ns, fas, styles=ws)
    return o['xyz'].contiguous(), o['depth'].reshape(RES, RES), vp[0]


@functools.lru_cache(maxsize=None)
def gpu_scene(name):
    """(verts, faces, normals) device tensors."""
    if name == "sphere":
        return tuple(torch.from_numpy(x).to(DEV) for x in host.uv_sphere())
    if name == "depth":
        v, f = mesh_utils.depth_mesh(volume_render(RENDER_VIEW)[0])
    else:
        vol = torch.from_numpy(syn.mc_volume(name)).view(1, *syn.MC_VOLUMES[name], 1).to(DEV)
        v, f = mesh_utils.marching_cubes(vol)
    return v, f, mesh_utils.vertex_normals(v, f)


def renderer_for(name, K, S):
    cam, li = scene_camera(name)
    return mesh_utils.create_mesh_renderer(cam, image_size=S, faces_per_pixel=K, light_location=(li["light"],), ambient_color=(li["ambient"],),
                                           diffuse_color=(li["diffuse"],), specular_color=(li["specular"],))


@functools.lru_cache(maxsize=None)
def truth(name, K, S):
    v, f, n = (x.cpu().numpy() for x in gpu_scene(name))
    cam, li = scene_camera(name)
    return host.restate_render(v, f, n, cam, S, K, lights=li, dtype=np.float64)


def hip(name, K, S, faces=None):
    v, f, n = gpu_scene(name)
    out = renderer_for(name, K, S).rasterize(v, f if faces is None else faces, n)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


# ---- 5. the depth mesh -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_depth_mesh_of_a_renderer_xyz_map():
    xyz = volume_render(RENDER_VIEW)[0]
    assert xyz.shape == (1, 3, RES, RES) and xyz.is_cuda
    v, f = mesh_utils.depth_mesh(xyz)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda and f.is_cuda
    want = xyz[0].permute(1, 2, 0).reshape(RES * RES, 3).contiguous()
    assert torch.equal(v.view(torch.int32), want.view(torch.int32))
    assert np.array_equal(f.cpu().numpy(), mesh_utils.depth_mesh_faces(RES, RES))
    # a non-square map, and the reference's return type
    x2 = torch.randn(1, 3, 5, 9, device=DEV)
    v2, f2 = mesh_utils.depth_mesh(x2)
    assert torch.equal(v2, x2[0].permute(1, 2, 0).reshape(45, 3)) and np.array_equal(f2.cpu().numpy(), mesh_utils.depth_mesh_faces(5, 9))
    mesh = mesh_utils.xyz2mesh(x2.cpu().numpy())
    assert np.array_equal(np.asarray(mesh.faces), f2.cpu().numpy()) and np.allclose(np.asarray(mesh.vertices), v2.cpu().numpy())
    # capturable in a HIP graph: no host round trip
    vg, fg = torch.empty_like(v), torch.empty_like(f)
    lib = _lib.load()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _lib.check(lib.e3dge_depth_mesh(_lib.ptr(vg), _lib.ptr(fg), _lib.ptr(xyz), RES, RES, s.cuda_stream), "e3dge_depth_mesh")
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(lib.e3dge_depth_mesh(_lib.ptr(vg), _lib.ptr(fg), _lib.ptr(xyz), RES, RES, torch.cuda.current_stream().cuda_stream), "e3dge_depth_mesh")
    vg.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(vg, v) and torch.equal(fg, f)


# ---- 6. vertex normals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["depth", "blob", "torus"])
def test_vertex_normals_against_the_float64_restatement(name):
    v, f, n = gpu_scene(name)
    want = host.restate_normals(v.cpu().numpy(), f.cpu().numpy(), np.float64)
    got = n.cpu().numpy()
    yard = report()["normals"][name]["yard_angle"]
    angle = max_angle(got, want)
    print(f"vertex_normals {name}: V = {len(got)}, F = {len(f)}, max angle HIP vs float64 = {angle:.3e}, yardstick = {yard:.3e}")
    record(f"vertex_normals_{name}", angle=angle, yardstick=yard)
    assert len(got) == report()["normals"][name]["n_verts"]
    assert angle <= FACTOR * yard
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-6
    again = mesh_utils.vertex_normals(v, f)
    assert torch.equal(again.view(torch.int32), n.view(torch.int32))
    # zero-area faces and faceless vertices
    v2 = torch.cat([v, torch.tensor([[1.0, 2.0, 3.0]], device=DEV)])
    f2 = torch.cat([f, torch.tensor([[0, 0, 5], [3, 3, 3]], dtype=torch.int32, device=DEV)])
    n2 = mesh_utils.vertex_normals(v2, f2)
    assert torch.equal(n2[:-1].view(torch.int32), n.view(torch.int32)) and bool((n2[-1] == 0).all())


# ---- 7. the rasteriser -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", SCENES)
def test_rasteriser_against_the_float64_restatement(name, K, S):
    t = truth(name, K, S)
    image, zbuf, p2f = hip(name, K, S)
    rec = report()["scenes"][scene_key(name, K, S)]
    covered = int(t["covered"].sum())
    share = float((t["covered"] & t["undecided"]).sum() / max(covered, 1))
    dec = ~t["undecided"]
    same = (np.sort(p2f[dec], -1) == np.sort(t["pix_to_face"][dec], -1)).all(-1)
    ez = float(np.abs(zbuf[dec][same].astype(np.float64) - t["zbuf"][dec][same]).max())
    ei = float(np.abs(image[dec][same].astype(np.float64) - t["image"][dec][same]).max())
    print(f"mesh_render {scene_key(name, K, S)}: covered {covered}, undecided {share:.4%}, face sets differ on {int((~same).sum())} decided pixels, "
          f"zbuf err {ez:.3e} (yardstick {rec['yard_zbuf']:.3e}), image err {ei:.3e} (yardstick {rec['yard_image']:.3e})")
    record(f"mesh_render_{scene_key(name, K, S)}", covered=covered, undecided_share=share, face_set_mismatches=int((~same).sum()), zbuf_err=ez,
           image_err=ei, yard_zbuf=rec["yard_zbuf"], yard_image=rec["yard_image"])
    assert covered > 0.2 * S * S
    assert share <= 0.02
    assert rec["yard_image"] <= 1e-3                                 # otherwise the scene is ill-conditioned and has to be replaced
    assert same.all()
    assert ez <= FACTOR * rec["yard_zbuf"]
    assert ei <= FACTOR * rec["yard_image"]
    # fragments sorted near to far, empty slots last
    zz = np.where(p2f >= 0, zbuf, np.float32(3e38))
    assert (np.diff(zz, axis=-1) >= 0).all() and ((p2f >= 0) == (zbuf >= 0)).all()


# ---- 8. closed loop with the volume renderer -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("view", LOOP_VIEWS)
def test_closed_loop_with_the_volume_renderer(view):
    xyz, depth, vp = volume_render(view)
    v, f = mesh_utils.depth_mesh(xyz)
    cam = mesh_utils.MeshCamera(np.rad2deg(float(vp[0])), np.rad2deg(float(vp[1])), fov=12.0)
    _, zbuf, p2f = mesh_utils.create_mesh_renderer(cam, image_size=RES, faces_per_pixel=1).rasterize(v, f)
    bound = report()["closed_loop"]["bound"]
    err = float((zbuf[..., 0].double() - depth.double()).abs().max())
    print(f"closed loop {view}: uncovered {int((p2f < 0).sum())}, max |zbuf - depth| = {err:.3e}, bound = {bound:.3e}")
    record(f"mesh_render_closed_loop_{view}", err=err, bound=bound)
    assert bool((p2f >= 0).all())
    assert err <= bound


# ---- 9. independence and determinism ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_face_order_independence_and_determinism(name):
    K, S = 5, 64
    t = truth(name, K, S)
    dec = ~t["undecided"]
    a = hip(name, K, S)
    b = hip(name, K, S)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    v, f, n = gpu_scene(name)
    perm = torch.from_numpy(np.random.RandomState(5).permutation(len(f))).to(DEV)
    image_p, zbuf_p, p2f_p = hip(name, K, S, faces=f[perm].contiguous())
    back = np.where(p2f_p >= 0, perm.cpu().numpy()[np.maximum(p2f_p, 0)], -1)
    assert np.array_equal(np.sort(back[dec], -1), np.sort(a[2][dec], -1))
    assert np.array_equal(zbuf_p[dec].view(np.int32), a[1][dec].view(np.int32))
    if name != "depth":                                              # a closed mesh has a front and a back fragment everywhere
        return
    # K = 5 on a pixel with one covered fragment is K = 1
    one = hip(name, 1, S)
    single = dec & (a[2][..., 0] >= 0) & (a[2][..., 1] < 0) & ~truth(name, 1, S)["undecided"]
    assert single.sum() > 1000
    assert np.abs(a[0][single][:, :3] - one[0][single][:, :3]).max() <= 1e-6
    assert np.array_equal(a[2][single][:, 0], one[2][single][:, 0])


# ---- 10. bin overflow, empty input, the runner's images ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bin_overflow_and_workspace_checks():
    v, f, n = gpu_scene("sphere")
    K, S, tiles, cap = 5, 64, 16, 1000
    r = renderer_for("sphere", K, S)
    image, _, _ = r.rasterize(v, f, n)
    with pytest.raises(RuntimeError, match="tile lists need"):
        r.rasterize(v, f, n, bin_capacity=cap)
    lib = _lib.load()
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = [torch.empty(S, S, 4, device=DEV), torch.empty(S, S, K, device=DEV), torch.empty(S, S, K, dtype=torch.int32, device=DEV)]
    nbytes = lib.e3dge_mesh_render_ws_bytes(len(v), len(f), S, cap)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    a = r._args()
    a.verts, a.faces, a.normals = _lib.ptr(v), _lib.ptr(f), _lib.ptr(n)
    a.n_verts, a.n_faces = len(v), len(f)
    a.image, a.zbuf, a.pix_to_face, a.status = (_lib.ptr(x) for x in out + [status])
    a.ws, a.bin_capacity = _lib.ptr(ws), cap
    a.ws_bytes = nbytes - 1                                          # one byte too small: refused before anything is launched
    assert lib.e3dge_mesh_render(ctypes.byref(a), _lib.stream_of(v)) == -1 and b"workspace" in lib.e3dge_last_error()
    a.ws_bytes = nbytes
    out[0].fill_(-7.0)
    _lib.check(lib.e3dge_mesh_render(ctypes.byref(a), _lib.stream_of(v)), "e3dge_mesh_render")
    need, got_cap = status.tolist()
    assert need > cap == got_cap and need < len(f) * tiles
    assert bool((out[0] == -7.0).all())                              # the lists did not fit: reported, nothing drawn
    image2, _, _ = r.rasterize(v, f, n, bin_capacity=need)           # exactly what the lists need
    assert torch.equal(image2, image)
    r.bin_factor = 0                                                 # the default guess (64 per tile here) is too small: the retry
    image3, _, _ = r.rasterize(v, f, n)
    assert torch.equal(image3, image)


@pytest.mark.gpu
def test_nothing_to_draw_gives_the_background():
    v, f, n = gpu_scene("sphere")
    cam = mesh_utils.MeshCamera(0.0, 0.0, 12.0)
    r = mesh_utils.create_mesh_renderer(cam, image_size=40, faces_per_pixel=3)
    white = torch.tensor([1.0, 1.0, 1.0, 0.0], device=DEV)
    for shift in ([0.0, 0.0, 2.0], [5.0, 0.0, 0.0]):                 # behind the camera (at z = 1); outside the frustum
        image, zbuf, p2f = r.rasterize(v + torch.tensor(shift, device=DEV), f, n)
        assert bool((p2f == -1).all()) and bool((zbuf == -1).all()) and bool((image == white).all())
    image, zbuf, p2f = r.rasterize(v, f[:0], n)                      # no faces at all
    assert bool((p2f == -1).all()) and bool((image == white).all())
    assert r(v, f).shape == (1, 40, 40, 4)
    im, zb = mesh_utils.create_depth_mesh_renderer(cam, image_size=40, faces_per_pixel=8)(v, f, n)
    assert im.shape == (1, 40, 40, 4) and zb.shape == (1, 40, 40, 8) and float(zb.max()) > 0.85


@pytest.mark.gpu
def test_the_runners_geometry_images():
    xyz, _, vp = volume_render(RENDER_VIEW)
    img = mesh_utils.render_depth_mesh(xyz, vp)
    assert img.shape == (512, 512, 3) and img.is_cuda and img.dtype == torch.float32
    assert float(img.min()) >= 0.0 and float(img.max()) <= 255.0 and float(img.std()) > 1.0
    assert bool((img[256, 256] < 254).any())                         # the centre is shaded geometry, not background
    v, f, _ = gpu_scene("torus")
    img2 = mesh_utils.render_surface_mesh(v, f, torch.tensor([0.3, 0.15]))
    assert img2.shape == (512, 512, 3) and float(img2.min()) >= 0.0 and float(img2.max()) <= 255.0
    assert bool((img2 < 254).any()) and bool((img2[0, 0] == 255).all())
