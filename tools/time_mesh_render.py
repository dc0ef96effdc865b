"""Times the surface renderings (csrc/mesh_render.hip) next to the 128^3 surface pass that precedes them in a frame of the novel-view demo.

    python tools/time_mesh_render.py

Two meshes, both drawn at 512^2 with 5 faces per pixel: the depth mesh of a 128 x 128 xyz map (depth_mesh + vertex_normals + render, 32 K
faces) and the marching-cubes mesh of synthetic.mc_volume('blob') resampled to 128^3 (vertex_normals + render).  HIP events over 50 calls
after 10 warm-up calls; calls go through mesh_utils, so the workspace allocation and the 8-byte status read-back of every render are in.
Prints one JSON line."""
import json
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import e3dge_amd  # noqa: E402,F401
from e3dge_amd import mesh_utils, synthetic as syn  # noqa: E402
from e3dge_amd.camera_utils import generate_camera_params  # noqa: E402
from e3dge_amd.volume_renderer import VolumeFeatureRenderer  # noqa: E402

DEV = "cuda:0"
CALLS, WARMUP = 50, 10


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(CALLS):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / CALLS


def main():
    res = 128
    r = VolumeFeatureRenderer(syn.rendering_opt(N_samples=res), out_im_res=res, mode='test')
    syn.load_synthetic(r, prefix='renderer.')
    r = r.to(DEV)
    ws, _ = syn.synthetic_inputs(1, seed=1, device=DEV)
    view = torch.tensor([[0.2, -0.1]], device=DEV)
    ps, fs, ns, fas, vp = generate_camera_params(res, DEV, locations=view)
    with torch.no_grad():
        surface_ms = timed(lambda: r(ps, fs, ns, fas, styles=ws))
        xyz = r(ps, fs, ns, fas, styles=ws)['xyz'].contiguous()
    out = dict(surface_pass_128_ms=surface_ms, image_size=512, faces_per_pixel=5, calls=CALLS, warmup=WARMUP)
    v, f = mesh_utils.depth_mesh(xyz)
    n = mesh_utils.vertex_normals(v, f)
    out["depth_mesh"] = dict(n_verts=len(v), n_faces=len(f), total_ms=timed(lambda: mesh_utils.render_depth_mesh(xyz, vp[0])),
                             depth_mesh_ms=timed(lambda: mesh_utils.depth_mesh(xyz)), normals_ms=timed(lambda: mesh_utils.vertex_normals(v, f)),
                             render_ms=timed(lambda: _render(v, f, n, vp[0], (0.0, 0.0, 5.0))))
    vol = torch.from_numpy(syn.mc_volume('blob'))[None, None]
    vol = F.interpolate(vol, size=(res, res, res), mode='trilinear', align_corners=True)[0, 0].to(DEV)
    mv, mf = mesh_utils.marching_cubes(vol.view(1, res, res, res, 1))
    mn = mesh_utils.vertex_normals(mv, mf)
    out["marching_cubes_mesh"] = dict(n_verts=len(mv), n_faces=len(mf), total_ms=timed(lambda: mesh_utils.render_surface_mesh(mv, mf, vp[0])),
                                      normals_ms=timed(lambda: mesh_utils.vertex_normals(mv, mf)),
                                      render_ms=timed(lambda: _render(mv, mf, mn, vp[0], (0.0, 3.0, 5.0))))
    print(json.dumps(out))


def _render(v, f, n, viewpoint, light):
    cam = mesh_utils._viewpoint_camera(viewpoint, 6.0)
    return mesh_utils.create_mesh_renderer(cam, image_size=512, light_location=(light,), **mesh_utils._RUNNER_LIGHTS)(v, f, n)


if __name__ == "__main__":
    main()
