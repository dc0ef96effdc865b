"""Golden vectors for marching cubes (surface extraction after align_volume), recorded from the reference's own
_extract_mesh_with_marching_cubes (project/utils/volume_renderer.py:1733-1758) with the real skimage.measure.marching_cubes.
Authoring time only; the tests never run this.

    python tools/gen_golden_marching_cubes.py --skimage-python PY

PY is an interpreter that has scikit-image (torch is not needed there): skimage is bridged to it through a subprocess, registered
before oracle.ref_harness stubs the reference's third-party imports, together with a trimesh.Trimesh stand-in that keeps its
arguments.  Writes, under tests/golden/:
    marching_cubes_<case>.npz    sk_verts (skimage's index-space vertices), sk_faces, ref_verts (the reference's transformed
                                 vertices); the 'render' case also stores its input volume (aligned_sdf)
    marching_cubes_report.json   skimage version, shapes, sha256 of every input volume, counts (V, F, vertices on grid edges)
The analytic volumes are e3dge_amd.synthetic.mc_volume(name); 'render' is a 48^3 renderer SDF volume of the oracle (synthetic weights),
aligned by oracle.mesh_ref.align_volume."""
import argparse
import hashlib
import importlib
import json
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLD = os.path.join(REPO, "tests", "golden")

import e3dge_amd  # noqa: E402,F401
from e3dge_amd import synthetic as syn  # noqa: E402

_BRIDGE = r"""
import sys, warnings
warnings.simplefilter("ignore")
import numpy as np, skimage
from skimage.measure import marching_cubes
src, dst, level = sys.argv[1], sys.argv[2], float(sys.argv[3])
v, f, n, val = marching_cubes(np.load(src), level)
np.savez(dst, verts=v, faces=f, normals=n, values=val, version=np.array(skimage.__version__))
"""


class Bridge:
    def __init__(self, python):
        self.python = python
        self.version = None

    def marching_cubes(self, volume, level=None, **kw):
        if kw:
            raise NotImplementedError(f"bridge: keyword arguments {sorted(kw)}")
        with tempfile.TemporaryDirectory() as d:
            src, dst = os.path.join(d, "vol.npy"), os.path.join(d, "out.npz")
            np.save(src, np.asarray(volume))
            subprocess.run([self.python, "-c", _BRIDGE, src, dst, repr(float(level))], check=True, stderr=subprocess.DEVNULL)
            z = np.load(dst)
            self.version = str(z["version"])
            self.last = (z["verts"].copy(), z["faces"].copy())
            return z["verts"], z["faces"], z["normals"], z["values"]


class TrimeshStandIn:
    def __init__(self, *args, **kw):
        self.args, self.kw = args, kw


def register(bridge):
    sk = types.ModuleType("skimage")
    skm = types.ModuleType("skimage.measure")
    skm.marching_cubes = bridge.marching_cubes
    sk.measure = skm
    tm = types.ModuleType("trimesh")
    tm.Trimesh = TrimeshStandIn
    tm.base = types.SimpleNamespace(Trimesh=TrimeshStandIn)
    sys.modules.update({"skimage": sk, "skimage.measure": skm, "trimesh": tm})


def render_volume(res=48):
    from e3dge_amd.camera_utils import generate_camera_params
    from e3dge_amd.volume_renderer import VolumeFeatureRenderer
    from oracle import mesh_ref, renderer_ref
    r = VolumeFeatureRenderer(syn.rendering_opt(N_samples=res), out_im_res=res, mode='test')
    syn.load_synthetic(r, prefix='renderer.')
    sd = {'renderer.' + k: v for k, v in r.state_dict().items()}
    wr, _ = syn.synthetic_inputs(1, seed=4)
    poses, focal, near, far, _ = generate_camera_params(res, "cpu", batch=1)
    with torch.no_grad():
        out = renderer_ref.render(sd, poses, focal, near, far, wr, res=res, n_samples=res)
    return mesh_ref.align_volume(out['sdf'].float())


def on_edges(sk_verts):
    return (sk_verts == np.floor(sk_verts)).sum(1) >= 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skimage-python", required=True, help="an interpreter with scikit-image")
    args = ap.parse_args()
    bridge = Bridge(args.skimage_python)
    register(bridge)
    from oracle import ref_harness
    vr = ref_harness.modules()[0]
    extract = vr.VolumeFeatureRenderer._extract_mesh_with_marching_cubes
    volumes = {n: torch.from_numpy(syn.mc_volume(n)).view(1, *syn.MC_VOLUMES[n], 1) for n in syn.MC_VOLUMES}
    volumes['render'] = render_volume()
    report = {}
    for name, aligned in volumes.items():
        mesh, verts, faces = extract(None, aligned.clone())
        sk_verts, sk_faces = bridge.last
        assert mesh.args[0] is verts and mesh.args[1] is faces
        arrays = dict(sk_verts=sk_verts, sk_faces=sk_faces, ref_verts=np.asarray(verts, np.float32))
        if name == 'render':
            arrays['aligned_sdf'] = aligned.numpy()
        np.savez_compressed(os.path.join(GOLD, f"marching_cubes_{name}.npz"), **arrays)
        vol = aligned.numpy()
        report[name] = dict(shape=list(vol.shape), sha256=hashlib.sha256(np.ascontiguousarray(vol).tobytes()).hexdigest(),
                            n_verts=int(len(sk_verts)), n_faces=int(len(sk_faces)), n_edge_verts=int(on_edges(sk_verts).sum()),
                            n_exact_zeros=int((vol == 0).sum()))
        print(name, report[name], flush=True)
    with open(os.path.join(GOLD, "marching_cubes_report.json"), "w") as f:
        json.dump(dict(skimage_version=bridge.version, call="skimage.measure.marching_cubes(sdf[0, ..., 0].permute(1, 0, 2), 0)",
                       cases=report), f, indent=1)


if __name__ == "__main__":
    main()
