"""View-consistent decoder noise on the GPU: mesh_utils.subdivide (e3dge_mesh_subdivide) against the numpy restatement of its rule,
mesh_utils.project_vertex_noise (e3dge_noise_project) against the float64 run of restate_render at K = 17 with ambient-only lights, and
the projecting modules of stylesdf_model.  The value bound is 3 x the yardstick tools/gen_noise_projection_report.py recorded in
tests/golden/noise_projection_report.json (the restatement's float32 run against its float64 run on the same scene: DESIGN.md 2, the
factor for "an independent fp32 implementation"), on pixels the float64 run decides (restate_render's docstring); undecided pixels may be
at most 2 % of a scene's covered pixels."""
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
import test_noise_projection_host as host

DEV = "cuda:0"
FACTOR = 3.0


def report():
    with open(os.path.join(GOLDEN, "noise_projection_report.json")) as f:
        return json.load(f)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def scene(name, viewpoint=host.VIEWPOINTS[0], K=host.K_NOISE):
    """(verts, faces, noise (V,), camera, S, the float64 restatement)."""
    level, S = host.NOISE_SCENES[name]
    v, f = host.scene_mesh(level)
    noise = host.scene_noise(len(v))[0]
    cam = host.scene_camera(viewpoint)
    return v, f, noise, cam, S, host.restate_projection(v, f, noise, cam, S, K=K, dtype=np.float64)


def prev_map(S, maps=1, seed=5):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((maps, S, S)).astype(np.float32)).to(DEV)


def hip(name, viewpoint=host.VIEWPOINTS[0]):
    v, f, noise, cam, S, _ = scene(name, viewpoint)
    prev = prev_map(S)
    maps, valid = mesh_utils.project_vertex_noise(dev(v), dev(f), dev(noise), cam, S, prev=prev)
    torch.cuda.synchronize()
    assert maps.shape == (1, S, S) and maps.dtype == torch.float32 and valid.shape == (S, S) and valid.dtype == torch.bool
    return maps[0].cpu().numpy(), valid.cpu().numpy(), prev[0].cpu().numpy()


# ---- 1. subdivision --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere", "blob"])
def test_subdivide_is_bit_identical_to_the_restated_rule(name):
    if name == "sphere":
        v, f, _ = host.uv_sphere()
        v, f = dev(v), dev(f)
    else:
        vol = torch.from_numpy(syn.mc_volume(name)).view(1, *syn.MC_VOLUMES[name], 1).to(DEV)
        v, f = mesh_utils.marching_cubes(vol)
    wv, wf = v.cpu().numpy(), f.cpu().numpy()
    for level in (1, 2, 3):
        wv, wf = host.restate_subdivide(wv, wf)
        gv, gf = mesh_utils.subdivide(v, f, levels=level)
        assert gv.dtype == torch.float32 and gf.dtype == torch.int32 and gv.is_cuda and gf.is_cuda
        assert gv.shape == wv.shape and gf.shape == wf.shape
        assert np.array_equal(gv.cpu().numpy().view(np.int32), wv.view(np.int32)), (name, level)
        assert np.array_equal(gf.cpu().numpy(), wf), (name, level)
    one, _ = mesh_utils.subdivide(*mesh_utils.subdivide(v, f, 2), 1)             # levels compose
    assert torch.equal(one, gv)
    same_v, same_f = mesh_utils.subdivide(v, f, levels=0)
    assert torch.equal(same_v, v) and torch.equal(same_f, f)
    cached = mesh_utils.load_mesh((v, f))
    assert cached is mesh_utils.load_mesh((v, f)) and cached.level(3)[0] is cached.level(3)[0]
    assert torch.equal(cached.for_image(512)[1], gf) and torch.equal(cached.for_image(256)[0], mesh_utils.subdivide(v, f, 1)[0])
    assert cached.for_image(64)[0].data_ptr() == v.data_ptr() and sorted(cached.levels) == [0, 1, 2, 3]


# ---- 2. the projection against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(host.NOISE_SCENES))
def test_projection_against_the_float64_restatement(name):
    v, f, noise, cam, S, t = scene(name)
    got, valid, prev = hip(name)
    rec = report()["scenes"][name]
    yard = rec["yard_value"]
    covered = int(t["covered"].sum())
    share = float((t["covered"] & t["undecided"]).sum() / max(covered, 1))
    dec = ~t["undecided"]
    mism = int((valid[dec] != t["covered"][dec]).sum())
    both = dec & t["covered"] & valid
    err = float(np.abs(got[both].astype(np.float64) - t["value"][both]).max())
    print(f"noise_project {name}: V = {len(v)}, F = {len(f)}, covered {covered}, undecided {share:.4%}, valid differs on {mism} decided pixels, "
          f"value err {err:.3e} (yardstick {yard:.3e}, bound {FACTOR * yard:.3e}), most fragments on a pixel {int((t['pix_to_face'] >= 0).sum(-1).max())}")
    record(f"noise_project_{name}", covered=covered, undecided_share=share, valid_mismatches=mism, value_err=err, yardstick=yard)
    assert (len(v), len(f)) == (rec["n_verts"], rec["n_faces"])
    assert covered > 0.2 * S * S
    assert share <= 0.02
    assert mism == 0
    assert err <= FACTOR * yard
    assert np.array_equal(got[~valid].view(np.int32), prev[~valid].view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(host.NOISE_SCENES))
def test_the_seventeenth_fragment_matters(name):
    """Near the silhouette a pixel collects 17 fragments and the blend of the nearest 8 is another value: the kernel has to agree with
    K = 17 there."""
    v, f, noise, cam, S, t = scene(name)
    t8 = scene(name, K=8)[5]
    got, valid, _ = hip(name)
    yard = report()["scenes"][name]["yard_value"]
    dec = t["covered"] & ~t["undecided"] & ~t8["undecided"]
    diff = np.abs(t["value"] - t8["value"])
    far = dec & (diff > 0.1)
    err = float(np.abs(got[far].astype(np.float64) - t["value"][far]).max()) if far.any() else float("nan")
    print(f"noise_project {name}: K = 17 and K = 8 differ by up to {diff[dec].max():.3f} on decided pixels, by > 0.1 on {int(far.sum())}; "
          f"most fragments on a pixel {int((t['pix_to_face'] >= 0).sum(-1).max())}; HIP vs K = 17 there: {err:.3e}")
    record(f"noise_project_k17_{name}", k8_max_difference=float(diff[dec].max()), pixels=int(far.sum()), err=err)
    assert far.any()
    assert int((t["pix_to_face"] >= 0).sum(-1).max()) > _lib.MESH_MAX_FACES_PER_PIXEL      # more fragments than the public rasteriser keeps
    assert valid[far].all() and err <= FACTOR * yard


# ---- 3. properties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_maps_share_a_rasterisation_bit_for_bit_and_runs_repeat():
    v, f, _, cam, S, _ = scene("sphere_L1_S64")
    gv, gf = dev(v), dev(f)
    noise = dev(host.scene_noise(len(v), seed=3, maps=4))
    prev = prev_map(S, maps=4)
    for C in (2, 4):
        both, valid = mesh_utils.project_vertex_noise(gv, gf, noise[:C], cam, S, prev=prev[:C])
        again, valid2 = mesh_utils.project_vertex_noise(gv, gf, noise[:C], cam, S, prev=prev[:C])
        assert torch.equal(both.view(torch.int32), again.view(torch.int32)) and torch.equal(valid, valid2)
        for c in range(C):
            one, valid1 = mesh_utils.project_vertex_noise(gv, gf, noise[c], cam, S, prev=prev[c:c + 1])
            assert torch.equal(one[0].view(torch.int32), both[c].view(torch.int32)) and torch.equal(valid1, valid)
        assert bool(valid.any()) and not bool(valid.all())
        assert torch.equal(both[:, ~valid].view(torch.int32), prev[:C][:, ~valid].view(torch.int32))
    with pytest.raises(RuntimeError, match="vert_noise"):
        mesh_utils.project_vertex_noise(gv, gf, torch.zeros(5, len(v), device=DEV), cam, S)
    with pytest.raises(RuntimeError, match="prev"):
        mesh_utils.project_vertex_noise(gv, gf, noise[:2], cam, S, prev=prev[:1])
    zeros, _ = mesh_utils.project_vertex_noise(gv, gf, noise[:1], cam, S)        # prev=None: zeros
    assert bool((zeros[0][~valid] == 0).all())


@pytest.mark.gpu
def test_nothing_to_project_returns_prev_and_overflow_retries():
    v, f, noise, cam, S, _ = scene("sphere_L0_S64")
    gv, gf, gn = dev(v), dev(f), dev(noise)
    prev = prev_map(S)
    for shift in ([0.0, 0.0, 2.0], [5.0, 0.0, 0.0]):                 # behind the camera of viewpoint (0, 0) at z = 1; outside the frustum
        maps, valid = mesh_utils.project_vertex_noise(gv + torch.tensor(shift, device=DEV), gf, gn, host.scene_camera((0.0, 0.0)), S, prev=prev)
        assert not bool(valid.any()) and torch.equal(maps.view(torch.int32), prev.view(torch.int32))
    maps, valid = mesh_utils.project_vertex_noise(gv, gf[:0], gn, cam, S, prev=prev)          # no faces at all
    assert not bool(valid.any()) and torch.equal(maps, prev)
    # the bin protocol: a fixed capacity that is too small raises, the default retries once with what the status word asks for
    want, want_valid = mesh_utils.project_vertex_noise(gv, gf, gn, cam, S, prev=prev)
    with pytest.raises(RuntimeError, match="tile lists need"):
        mesh_utils.project_vertex_noise(gv, gf, gn, cam, S, prev=prev, bin_capacity=1000)
    import ctypes
    lib = _lib.load()
    a = _lib.NoiseProjectArgs()
    a.camera[:] = cam.floats().tolist()
    a.tan_half_fov, a.znear, a.zfar, a.blur_radius, a.sigma, a.gamma = cam.tan_half_fov, cam.znear, cam.zfar, 1e-6, 1e-4, 1e-4
    a.image_size, a.n_maps, a.n_verts, a.n_faces, a.bin_capacity = S, 1, len(v), len(f), 1000
    out, val = torch.full((1, S, S), -7.0, device=DEV), torch.full((S, S), 9, dtype=torch.uint8, device=DEV)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    nbytes = lib.e3dge_noise_project_ws_bytes(len(v), len(f), S, 1000)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    a.verts, a.faces, a.vert_noise, a.prev, a.out, a.valid, a.status, a.ws = (_lib.ptr(x) for x in (gv, gf, gn, prev, out, val, status, ws))
    a.ws_bytes = nbytes - 1
    assert lib.e3dge_noise_project(ctypes.byref(a), _lib.stream_of(gv)) == -1 and b"workspace" in lib.e3dge_last_error()
    a.ws_bytes = nbytes
    _lib.check(lib.e3dge_noise_project(ctypes.byref(a), _lib.stream_of(gv)), "e3dge_noise_project")
    need, cap = status.tolist()
    assert need > cap == 1000 and need < len(f) * 16
    assert bool((out == -7.0).all()) and bool((val == 9).all())      # the lists did not fit: reported, nothing written
    exact, _ = mesh_utils.project_vertex_noise(gv, gf, gn, cam, S, prev=prev, bin_capacity=need)
    assert torch.equal(exact, want)


@pytest.mark.gpu
@pytest.mark.parametrize("viewpoint", [host.VIEWPOINTS[0], host.VIEWPOINTS[1]])
def test_values_are_convex_combinations_of_the_listed_faces_noise(viewpoint):
    name = "sphere_L1_S64"
    v, f, noise, cam, S, t = scene(name, viewpoint)
    got, valid, _ = hip(name, viewpoint)
    dec = ~t["undecided"] & t["covered"]
    assert np.array_equal(valid[~t["undecided"]], t["covered"][~t["undecided"]])
    p2f = t["pix_to_face"][dec]                                      # (n, 17), -1 where empty
    field = noise[f.astype(np.int64)]                                # (F, 3)
    lo = np.where(p2f >= 0, field.min(1)[np.maximum(p2f, 0)], np.inf).min(1)
    hi = np.where(p2f >= 0, field.max(1)[np.maximum(p2f, 0)], -np.inf).max(1)
    # the background's weight delta = 1e-10 against sum w_k >= 0.49 (a covered fragment's p_k), and float32 rounding: at most 17 fragments
    # x (3 weights, 3 products, 2 sums) < 2^8 roundings of 2^-24 on values up to max |noise|
    tol = 1e-9 * (1 + np.abs(noise).max()) + 2.0 ** -16 * np.abs(noise).max()
    x = got[dec].astype(np.float64)
    print(f"convexity {viewpoint}: {len(x)} pixels, worst excess {max((lo - x).max(), (x - hi).max()):.3e}, tolerance {tol:.3e}")
    assert len(x) > 0.2 * S * S
    assert (x >= lo - tol).all() and (x <= hi + tol).all()


# ---- 4. the modules --------------------------------------------------------------------------------------------------------------------------
RES, N_SAMPLES = 64, 24


def generator(project):
    from e3dge_amd.stylesdf_model import G_pred_latents
    g = G_pred_latents(syn.model_opt(size=256, channel_multiplier=1, renderer_spatial_output_dim=RES, project_noise=project),
                       syn.rendering_opt(N_samples=N_SAMPLES), full_pipeline=True)
    syn.load_synthetic(g)
    return g.to(DEV).eval()


def noise_modules(g):
    return [g.decoder.conv1.noise] + [c.noise for c in g.decoder.convs]


def frame(viewpoint):
    return generate_camera_params(RES, DEV, locations=torch.tensor([viewpoint], dtype=torch.float32, device=DEV))[:4]


def run(g, cam, wr, wd, **kw):
    poses, focal, near, far = cam
    with torch.no_grad():
        out = g([wr, wd], poses, focal, near, far, input_is_latent=True, **kw)
    torch.cuda.synchronize()
    return out["gen_imgs"]


def expected_maps(g, mesh, poses, first_noise):
    """The maps the issue prescribes, one project_vertex_noise call per module with the module's own vert_noise."""
    cam = mesh_utils.noise_camera(poses)
    maps = []
    for m, n in zip(noise_modules(g), first_noise):
        S = n.shape[2]
        v, f = mesh_utils.load_mesh(mesh).for_image(S)
        assert m.vert_noise.shape == (len(v),) and m.vert_noise.device == v.device
        maps.append(mesh_utils.project_vertex_noise(v, f, m.vert_noise, cam, S, prev=n.reshape(1, S, S))[0].reshape(1, 1, S, S))
    return maps


@pytest.mark.gpu
def test_projecting_generator_end_to_end(tmp_path):
    v, f, _ = host.uv_sphere()
    mesh = (dev(v), dev(f))
    g1, g0 = generator(True), generator(False)
    wr, wd = syn.synthetic_inputs(1, seed=1, device=DEV)
    wd = wd[:, :g1.decoder.n_latent]
    buffers = [getattr(g1.decoder.noises, f"noise_{i}") for i in range(g1.decoder.num_layers)]
    assert [b.shape[2] for b in buffers] == [64, 128, 128, 256, 256]
    assert [mesh_utils.subdivision_level(b.shape[2]) for b in buffers] == [0, 0, 0, 1, 1]
    cam_a, cam_b = frame(host.VIEWPOINTS[0]), frame(host.VIEWPOINTS[1])

    # noise=None with random noise: nothing is projected
    run(g1, cam_a, wr, wd, project_noise=True, mesh_path=mesh)
    assert all(m.vert_noise is None and m.prev_noise is None for m in noise_modules(g1))

    torch.manual_seed(11)
    img = run(g1, cam_a, wr, wd, randomize_noise=False, project_noise=True, mesh_path=mesh)
    level1 = mesh_utils.load_mesh(mesh).level(1)[0].shape[0]
    assert [m.vert_noise.shape[0] for m in noise_modules(g1)] == [len(v)] * 3 + [level1] * 2
    assert all(m.prev_noise is b for m, b in zip(noise_modules(g1), buffers))
    maps = expected_maps(g1, mesh, cam_a[0], buffers)
    want = run(g0, cam_a, wr, wd, noise=maps)
    assert torch.equal(img.view(torch.int32), want.view(torch.int32))
    plain = run(g0, cam_a, wr, wd, randomize_noise=False)
    assert not torch.equal(plain, want)                              # the projection changes the image

    # a second frame, another viewpoint and another `noise` list: what the mesh does not cover still comes from the first call's noise
    other = [torch.randn_like(b) for b in buffers]
    kept = [m.vert_noise for m in noise_modules(g1)]
    img_b = run(g1, cam_b, wr, wd, noise=other, project_noise=True, mesh_path=mesh)
    assert all(m.vert_noise is k for m, k in zip(noise_modules(g1), kept)) and all(m.prev_noise is b for m, b in zip(noise_modules(g1), buffers))
    maps_b = expected_maps(g1, mesh, cam_b[0], buffers)
    assert torch.equal(img_b.view(torch.int32), run(g0, cam_b, wr, wd, noise=maps_b).view(torch.int32))
    assert not torch.equal(maps_b[0], expected_maps(g1, mesh, cam_b[0], other)[0])

    # mesh_path as an OBJ path gives the same maps as the tuple
    path = str(tmp_path / "sphere.obj")
    mesh_utils.SurfaceMesh(v, f).export(path)
    g2 = generator(True)
    torch.manual_seed(11)
    img2 = run(g2, cam_a, wr, wd, randomize_noise=False, project_noise=True, mesh_path=path)
    assert all(torch.equal(a.vert_noise, b.vert_noise) for a, b in zip(noise_modules(g1), noise_modules(g2)))
    assert all(m.mesh_fn == path for m in noise_modules(g2))
    for a, b in zip(maps, expected_maps(g2, path, cam_a[0], buffers)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(img2.view(torch.int32), img.view(torch.int32))
    # one module alone, the reference's entry
    m = noise_modules(g2)[3]
    assert torch.equal(m.project_noise(other[3], cam_a[0], path), maps[3])

    # batch 2, missing transform, missing mesh
    wr2, wd2 = torch.cat([wr, wr]), torch.cat([wd, wd])
    locs = torch.tensor([host.VIEWPOINTS[0], host.VIEWPOINTS[1]], dtype=torch.float32, device=DEV)
    with pytest.raises(AssertionError, match="batch"):
        run(g1, generate_camera_params(RES, DEV, locations=locs)[:4], wr2, wd2, randomize_noise=False, project_noise=True, mesh_path=mesh)
    with pytest.raises(ValueError, match="transform"):
        run(g1, cam_a, wr, wd, randomize_noise=False, mesh_path=mesh)
    with pytest.raises(ValueError, match="mesh_path"):
        run(g1, cam_a, wr, wd, randomize_noise=False, project_noise=True)
