"""The yardsticks of the noise-projection GPU tests (tests/test_gpu_noise_projection.py).  Authoring time only, pure numpy on the CPU; the
tests never run this.

    python tools/gen_noise_projection_report.py

Writes tests/golden/noise_projection_report.json: per scene of tests/test_noise_projection_host.py (NOISE_SCENES: the UV sphere after the
numpy restatement of the subdivision rule, unit-variance vertex noise, the viewpoint (0.3, 0.15)) the share of covered pixels the float64
restatement leaves undecided, the yardstick -- the largest distance of the restatement's float32 run from its float64 run on decided
pixels -- and how far the blend of the nearest 8 fragments is from the blend of 17.  pytorch3d is not installed anywhere this project
builds or runs: the restatement is the specification, the yardstick says how far an independent float32 evaluation of it lands."""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import test_noise_projection_host as host  # noqa: E402


def main():
    report = {"viewpoint": list(host.VIEWPOINTS[0]), "faces_per_pixel": host.K_NOISE, "scenes": {}}
    cam = host.scene_camera()
    for name, (level, S) in host.NOISE_SCENES.items():
        v, f = host.scene_mesh(level)
        noise = host.scene_noise(len(v))[0]
        t = host.restate_projection(v, f, noise, cam, S, dtype=np.float64)
        y = host.restate_projection(v, f, noise, cam, S, dtype=np.float32)
        t8 = host.restate_projection(v, f, noise, cam, S, K=8, dtype=np.float64)
        dec = t["covered"] & ~t["undecided"]
        rec = dict(level=level, image_size=S, n_verts=len(v), n_faces=len(f), covered=int(t["covered"].sum()),
                   undecided_share=float((t["covered"] & t["undecided"]).sum() / max(t["covered"].sum(), 1)),
                   float32_same_valid=bool(np.array_equal(t["covered"][dec], y["covered"][dec])),
                   max_fragments=int((t["pix_to_face"] >= 0).sum(-1).max()),
                   yard_value=float(np.abs(y["value"][dec].astype(np.float64) - t["value"][dec]).max()),
                   k8_max_difference=float(np.abs(t8["value"][dec & ~t8["undecided"]] - t["value"][dec & ~t8["undecided"]]).max()))
        assert rec["undecided_share"] <= 0.02, (name, rec)
        report["scenes"][name] = rec
        print(name, rec, flush=True)
    with open(os.path.join(REPO, "tests", "golden", "noise_projection_report.json"), "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
