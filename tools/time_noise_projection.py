"""Times the view-consistent decoder noise (mesh_utils.subdivide / project_vertex_noise, csrc/mesh_render.hip) next to what a frame of the
novel-view video already costs: the 128^3 surface pass and the decoder's forward.

    python tools/time_noise_projection.py [--calls 50] [--warmup 10] [--mesh surface|blob|both] [--sizes 64,128,256,512,1024]

Two meshes: the marching-cubes surface of the renderer's own 128^3 volume (the benchmark's surface leg) and synthetic.mc_volume('blob')
resampled to 128^3.  Per mesh: the subdivision levels 1..3 (paid once per mesh: 3 calls after 1), then the per-frame cost of the nine maps
of a 1024 decoder -- five launches, one per size: one map at 64 (level 0), two each at 128 (level 0), 256 (level 1), 512 and 1024 (level
3).  HIP events over `calls` calls after `warmup`; calls go through mesh_utils, so the workspace allocation and the 8-byte status read-back
of every launch are in.  Prints one JSON line.  `--sizes 1024 --mesh surface --calls 5 --warmup 1 --no-yardsticks` is what a rocprofv3
--kernel-trace --stats run of the raster kernel alone wants."""
import argparse
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
from e3dge_amd.stylesdf_model import Decoder  # noqa: E402
from e3dge_amd.volume_renderer import VolumeFeatureRenderer  # noqa: E402

DEV = "cuda:0"
MAPS = {64: 1, 128: 2, 256: 2, 512: 2, 1024: 2}                     # the nine noise maps of a 1024 decoder by size


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--mesh", default="both", choices=("surface", "blob", "both"))
    ap.add_argument("--sizes", default="64,128,256,512,1024")
    ap.add_argument("--no-yardsticks", action="store_true")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    res = 128
    out = dict(calls=args.calls, warmup=args.warmup, sizes=sizes, faces_per_pixel=17)
    r = VolumeFeatureRenderer(syn.rendering_opt(N_samples=res), out_im_res=res, mode='test')
    syn.load_synthetic(r, prefix='renderer.')
    r = r.to(DEV)
    ws, _ = syn.synthetic_inputs(1, seed=1, device=DEV)
    view = torch.tensor([[0.2, -0.1]], device=DEV)
    ps, fs, ns, fas, vp = generate_camera_params(res, DEV, locations=view)
    camera = mesh_utils.noise_camera(ps)
    meshes = {}
    with torch.no_grad():
        if not args.no_yardsticks:
            out["surface_pass_128_ms"] = timed(lambda: r(ps, fs, ns, fas, styles=ws), args.calls, args.warmup)
            dec = Decoder(syn.model_opt()).to(DEV).eval()
            feats = torch.randn(1, 256, 64, 64, device=DEV)
            latent = torch.randn(1, dec.n_latent, dec.style_dim, device=DEV)
            out["decoder_forward_1024_ms"] = timed(lambda: dec(feats, [latent], input_is_latent=True, randomize_noise=False), args.calls, args.warmup)
            del dec, feats
        if args.mesh in ("surface", "both"):
            o = r(ps, fs, ns, fas, styles=ws, return_mesh=True)
            meshes["surface_128"] = (o['mesh_verts'], o['mesh_faces'])
        if args.mesh in ("blob", "both"):
            vol = torch.from_numpy(syn.mc_volume('blob'))[None, None]
            vol = F.interpolate(vol, size=(res, res, res), mode='trilinear', align_corners=True)[0, 0].to(DEV)
            meshes["blob_128"] = mesh_utils.marching_cubes(vol.view(1, res, res, res, 1))
    for name, (v, f) in meshes.items():
        rec = dict(levels={}, launches={})
        lv, lf = v, f
        levels = {0: (v, f)}
        for level in (1, 2, 3):
            ms = timed(lambda: mesh_utils.subdivide(lv, lf, 1), 3, 1)
            lv, lf = mesh_utils.subdivide(lv, lf, 1)
            levels[level] = (lv, lf)
            rec["levels"][str(level)] = dict(n_verts=len(lv), n_faces=len(lf), subdivide_ms=ms)
        rec["levels"]["0"] = dict(n_verts=len(v), n_faces=len(f))
        total = 0.0
        for S in sizes:
            mv, mf = levels[mesh_utils.subdivision_level(S)]
            C = MAPS.get(S, 2)
            noise = torch.randn(C, len(mv), device=DEV)
            prev = torch.randn(C, S, S, device=DEV)
            ms = timed(lambda: mesh_utils.project_vertex_noise(mv, mf, noise, camera, S, prev=prev), args.calls, args.warmup)
            _, valid = mesh_utils.project_vertex_noise(mv, mf, noise, camera, S, prev=prev)
            rec["launches"][str(S)] = dict(maps=C, level=mesh_utils.subdivision_level(S), n_faces=len(mf), ms=ms, valid_share=float(valid.float().mean()))
            total += ms
            del noise, prev
        rec["per_frame_ms"] = total
        out[name] = rec
        del levels, lv, lf
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
