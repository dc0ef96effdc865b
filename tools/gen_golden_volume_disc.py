"""Fixture for the camera-pose predictor (tests/test_volume_disc_host.py, tests/test_gpu_volume_disc.py).  Authoring time only, CPU only;
the tests never run this.

    python tools/gen_golden_volume_disc.py

Imports the reference's VolumeRenderDiscriminator (project/models/stylesdf_model.py) and generate_camera_params
(project/utils/camera_utils.py), loads the synthetic weights of e3dge_amd.synthetic.load_synthetic_volume_discriminator (both variants) and
writes, under tests/golden/:
    volume_disc_state_dict_keys.json   sorted keys and shapes of the reference's state dict for renderer_spatial_output_dim 64 and 16
    volume_disc.npz                    for every case of test_volume_disc_host.CASES and both weight variants, on the images of
                                       test_discriminator_host.golden_images (a formula: no image and no weight is stored): the logits, the
                                       viewpoints, per tap (the stem's output and every block's) 256 sampled values (at
                                       test_idloss_host.tap_samples) and the float64 sum, and at size 64 the poses of image2camsettings
                                       (is_thumb: the reference's generate_camera_params on the predicted locations)
    volume_disc_report.json            torch version, thread count, file sizes; per case the float32 run's distance from a float64 run of
                                       the same modules (per tap, logits, viewpoints: max |f32 - f64| / max |f64|), and for the batches of
                                       two and more how far the float64 viewpoints of different images lie apart (the smallest max |a - b|
                                       over the pairs) against the bound the GPU test asserts on the viewpoints,
                                       max(2e-6 max |f64|, 4 max |f32 - f64|): the generator refuses a fixture where that is under 1000."""
import importlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
GOLD = os.path.join(REPO, "tests", "golden")

import oracle.cpu_numerics  # noqa: E402,F401  (before any arithmetic)
import e3dge_amd  # noqa: E402,F401
from e3dge_amd import synthetic as syn  # noqa: E402
from e3dge_amd.volume_discriminator import VolumeRenderDiscriminator  # noqa: E402
import test_volume_disc_host as host  # noqa: E402
from test_encoder_host import parity_bound  # noqa: E402
from test_idloss_host import tap_samples  # noqa: E402


def reference_modules():
    from oracle import ref_harness, golden_store
    ref_harness.prepare()
    return importlib.import_module("project.models.stylesdf_model"), importlib.import_module("project.utils.camera_utils"), golden_store


def reference_network(sm, size, variant, dtype=torch.float32):
    opt = syn.model_opt(renderer_spatial_output_dim=size)
    ref = sm.VolumeRenderDiscriminator(opt)
    ours = syn.load_synthetic_volume_discriminator(VolumeRenderDiscriminator(opt), variant=variant)
    ref.load_state_dict(ours.state_dict(), strict=True)
    return ref.to(dtype).eval()


def run(ref, x):
    """dict(logits, viewpoints, taps [the stem's output, every block's]) of the reference module under no_grad."""
    taps = {}
    hooks = [layer.register_forward_hook(lambda m, inp, out, i=i: taps.__setitem__(i, out.detach())) for i, layer in enumerate(ref.convs)]
    with torch.no_grad():
        logits, views = ref(x)
    for h in hooks:
        h.remove()
    return dict(logits=logits, viewpoints=views, taps=[taps[i] for i in range(len(ref.convs))])


def rel(a, b):
    top = float(b.abs().max())
    return float((a.double() - b).abs().max()) / top if top > 0 else 0.0


def main():
    sm, cu, golden_store = reference_modules()
    keys = {}
    for size in (64, 16):
        sd = sm.VolumeRenderDiscriminator(syn.model_opt(renderer_spatial_output_dim=size)).state_dict()
        keys[str(size)] = dict(keys=sorted(sd), shapes={k: list(v.shape) for k, v in sd.items()})
    with open(os.path.join(GOLD, "volume_disc_state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    arrays, cases = {}, {}
    cam = host.CAMERA
    for variant in host.VARIANTS:
        for case in host.CASES:
            size, B = case
            x = host.golden_images(B, size)
            r32 = run(reference_network(sm, size, variant), x)
            r64 = run(reference_network(sm, size, variant, torch.float64), x.double())
            key = host.case_id(case, variant) + "/"
            arrays[key + "logits"] = r32["logits"].numpy()
            arrays[key + "viewpoints"] = r32["viewpoints"].numpy()
            for t, v in enumerate(r32["taps"]):
                arrays[key + "tap_" + host.tap_name(t)] = v.reshape(-1)[tap_samples(v.numel())].numpy()
                arrays[key + "sum_" + host.tap_name(t)] = np.float64(v.double().sum().item())
            if size == 64:
                settings = cu.generate_camera_params(host.RENDER_SIZE, "cpu", B, locations=r32["viewpoints"], uniform=cam.uniform, azim_range=cam.azim,
                                                     elev_range=cam.elev, fov_ang=cam.fov, dist_radius=cam.dist_radius, return_calibs=True)
                arrays[key + "poses"] = settings["poses"].numpy()
            row = dict(logits=rel(r32["logits"], r64["logits"]), viewpoints=rel(r32["viewpoints"], r64["viewpoints"]),
                       taps={host.tap_name(t): rel(v, r64["taps"][t]) for t, v in enumerate(r32["taps"])},
                       tap_std={host.tap_name(t): float(v.std()) for t, v in enumerate(r64["taps"])},
                       max_viewpoint=float(r64["viewpoints"].abs().max()))
            if B >= 2:
                v64 = r64["viewpoints"]
                apart = min(float((v64[i] - v64[j]).abs().max()) for i in range(B) for j in range(i))
                bound = parity_bound(v64, r32["viewpoints"], 4)
                row.update(viewpoints_apart=apart, viewpoints_bound=bound, apart_over_bound=apart / bound)
                assert apart >= 1000 * bound, (key, apart, bound)        # a kernel that ignores the image cannot pass the GPU test
            cases[key[:-1]] = row
            print(key, row, flush=True)
    path = golden_store.save(GOLD, "volume_disc", arrays)
    report = dict(torch=torch.__version__, threads=torch.get_num_threads(), npz_bytes=os.path.getsize(path),
                  keys_bytes=os.path.getsize(os.path.join(GOLD, "volume_disc_state_dict_keys.json")), cases=cases)
    with open(os.path.join(GOLD, "volume_disc_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(dict(npz_bytes=report["npz_bytes"], keys_bytes=report["keys_bytes"]))


if __name__ == "__main__":
    main()
