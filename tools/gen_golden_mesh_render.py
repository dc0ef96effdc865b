"""Fixtures for the surface renderings (tests/test_mesh_render_host.py, tests/test_gpu_mesh_render.py).  Authoring time only, CPU only;
the tests never run this.

    python tools/gen_golden_mesh_render.py

Writes, under tests/golden/:
    xyz2mesh_faces.npz        faces_8, faces_128: the face lists of the reference's own xyz2mesh (project/utils/mesh_utils.py:107-126; real
                              scipy.spatial.Delaunay, through oracle.ref_harness with a trimesh.Trimesh stand-in that keeps its arguments)
                              on an 8 x 8 and a 128 x 128 map
    mesh_render_report.json   per scene of the GPU tests: the share of undecided pixels in float64 and the yardsticks -- the distance of the
                              float32 run of the numpy restatement (tests/test_mesh_render_host.py) from its float64 run on decided pixels
                              -- for zbuf, image and the vertex normals; the closed-loop bound (3 x (the CPU oracle's depth in float32
                              against float64 + the float32 restatement's |zbuf - depth|)).
The pytorch3d renderer itself is not installed anywhere this project builds or runs: the restatement is the specification, the yardsticks
say how far an independent float32 evaluation of it lands from float64."""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
GOLD = os.path.join(REPO, "tests", "golden")

import e3dge_amd  # noqa: E402,F401
from e3dge_amd import mesh_utils, synthetic as syn  # noqa: E402
from e3dge_amd.camera_utils import generate_camera_params  # noqa: E402
import test_mesh_render_host as host  # noqa: E402
import test_gpu_mesh_render as gpu  # noqa: E402


class TrimeshStandIn:
    def __init__(self, *args, **kw):
        self.args, self.kw = args, kw


def reference_faces():
    tm = types.ModuleType("trimesh")
    tm.Trimesh = TrimeshStandIn
    sys.modules["trimesh"] = tm
    from oracle import ref_harness
    ref_harness.prepare()
    ref = importlib.import_module("project.utils.mesh_utils")
    import scipy
    out = {}
    for n in (8, 128):
        mesh = ref.xyz2mesh(torch.zeros(1, 3, n, n))
        verts, faces = mesh.args
        assert verts.shape == (n * n, 3)
        out[f"faces_{n}"] = np.asarray(faces).astype(np.int32)
    return out, scipy.__version__


def oracle_render(view, res, dtype):
    from oracle import renderer_ref
    from e3dge_amd.volume_renderer import VolumeFeatureRenderer
    r = VolumeFeatureRenderer(syn.rendering_opt(N_samples=gpu.N_SAMPLES), out_im_res=res, mode='test')
    syn.load_synthetic(r, prefix='renderer.')
    sd = {'renderer.' + k: v for k, v in r.state_dict().items()}
    wr, _ = syn.synthetic_inputs(1, seed=gpu.STYLE_SEED)
    poses, focal, near, far, _ = generate_camera_params(res, "cpu", locations=torch.tensor([view], dtype=torch.float32))
    with torch.no_grad():
        return renderer_ref.render(sd, poses, focal, near, far, wr, res=res, n_samples=gpu.N_SAMPLES, dtype=dtype)


def cpu_scene(name):
    """(verts, faces, normals) float32 / int32 of a GPU-test scene, built on the CPU."""
    if name == "sphere":
        return host.uv_sphere()
    if name == "depth":
        xyz = oracle_render(gpu.RENDER_VIEW, gpu.RES, torch.float32)['xyz'].numpy()
        v = np.ascontiguousarray(xyz[0].transpose(1, 2, 0).reshape(-1, 3))
        f = mesh_utils.depth_mesh_faces(gpu.RES, gpu.RES)
    else:
        import test_marching_cubes as mc
        vol = syn.mc_volume(name).reshape(1, *syn.MC_VOLUMES[name], 1)
        v, f = mc.restate(mc.skimage_view(vol), mesh_utils.marching_cubes_tables())
    return v, f, host.restate_normals(v, f).astype(np.float32)


def main():
    faces, scipy_version = reference_faces()
    os.chdir(REPO)
    np.savez_compressed(os.path.join(GOLD, "xyz2mesh_faces.npz"), **faces)
    report = dict(scipy_version=scipy_version, scenes={}, normals={}, closed_loop={})
    for name in ("depth", "blob", "torus"):
        v, f, _ = cpu_scene(name)
        n64, n32 = host.restate_normals(v, f, np.float64), host.restate_normals(v, f, np.float32)
        report["normals"][name] = dict(n_verts=len(v), n_faces=len(f), yard_angle=gpu.max_angle(n32, n64))
        print("normals", name, report["normals"][name], flush=True)
    for name in gpu.SCENES:
        v, f, n = cpu_scene(name)
        cam, lights = gpu.scene_camera(name)
        for K in gpu.KS:
            for S in gpu.SIZES:
                t = host.restate_render(v, f, n, cam, S, K, lights=lights, dtype=np.float64)
                y = host.restate_render(v, f, n, cam, S, K, lights=lights, dtype=np.float32)
                dec = t["covered"] & ~t["undecided"]
                same = np.array_equal(np.sort(t["pix_to_face"][dec], -1), np.sort(y["pix_to_face"][dec], -1))
                rec = dict(n_faces=len(f), covered=int(t["covered"].sum()), undecided_share=float((t["covered"] & t["undecided"]).sum() / max(t["covered"].sum(), 1)),
                           two_fragments_share=float((t["pix_to_face"][..., -1] >= 0).sum() / max(t["covered"].sum(), 1)) if K > 1 else None,
                           float32_same_faces=bool(same),
                           yard_zbuf=float(np.abs(y["zbuf"][dec].astype(np.float64) - t["zbuf"][dec]).max()),
                           yard_image=float(np.abs(y["image"][dec].astype(np.float64) - t["image"][dec]).max()))
                # the test's cap is 2 %; a scene above 1.5 % here is a candidate for another viewpoint or size (the torus stays
                # above it at K = 1 from every viewpoint tried)
                rec["above_1p5_percent"] = bool(rec["undecided_share"] > 0.015)
                assert rec["undecided_share"] <= 0.02 and rec["yard_image"] <= 1e-3, (name, K, S, rec)
                report["scenes"][gpu.scene_key(name, K, S)] = rec
                print(gpu.scene_key(name, K, S), rec, flush=True)
    oracle_err, restated = 0.0, 0.0
    for view in gpu.LOOP_VIEWS:
        o32, o64 = oracle_render(view, gpu.RES, torch.float32), oracle_render(view, gpu.RES, torch.float64)
        oracle_err = max(oracle_err, float((o32['depth'].double() - o64['depth']).abs().max()))
        xyz = o32['xyz'].numpy()
        v = np.ascontiguousarray(xyz[0].transpose(1, 2, 0).reshape(-1, 3))
        f = mesh_utils.depth_mesh_faces(gpu.RES, gpu.RES)
        cam = mesh_utils.MeshCamera(np.rad2deg(np.float32(view[0])), np.rad2deg(np.float32(view[1])), 12.0)
        y = host.restate_render(v, f, host.restate_normals(v, f).astype(np.float32), cam, gpu.RES, 1, lights=host.RUNNER_LIGHTS, dtype=np.float32)
        assert (y["pix_to_face"][..., 0] >= 0).all()
        restated = max(restated, float(np.abs(y["zbuf"][..., 0].astype(np.float64) - o32['depth'][0, ..., 0, 0].double().numpy()).max()))
    report["closed_loop"] = dict(oracle_depth_f32_vs_f64=oracle_err, restated_f32_zbuf_vs_depth=restated, bound=3 * (oracle_err + restated))
    print("closed loop", report["closed_loop"], flush=True)
    with open(os.path.join(GOLD, "mesh_render_report.json"), "w") as fh:
        json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
