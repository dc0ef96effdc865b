"""Fixture for the hourglass image filter (tests/test_hgfilter_host.py, tests/test_gpu_hgfilter.py).  Authoring time only, CPU only; the
tests never run this.

    python tools/gen_golden_hgfilter.py

Imports the reference's HGFilter (project/vendor/pifu/lib/model/HGFilters.py; ConvBlock comes with it) and ResidualBlock / conv3x3 / conv1x1 /
conv (project/models/helper_modules/helpers.py), builds residual_conv, depth_conv, downsample_channel_conv and image_filter from them as
HGPIFuNetGANResidualResnetFC does (HGPIFuGANNetResidualInputResnetFC.py:28-45: affine instance norms), loads the synthetic weights of e3dge_amd.synthetic.load_synthetic_hgfilter and writes, under tests/golden/:
    hgfilter_state_dict_keys.json   the sorted keys of that reference module's state dict
    hgfilter.npz                    no weights and no inputs (both are formulas).  For every case of test_hgfilter_host.CASES and every
                                    returned tensor (each stack's map, tmpx, normx): 256 values at test_hgfilter_host.samples and the
                                    float64 sum; for the 'default' case also image 0 of the last stack's map, whole
    hgfilter_report.json            torch version, thread count, file size, per-case seconds"""
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
GOLD = os.path.join(REPO, "tests", "golden")

import oracle.cpu_numerics  # noqa: E402,F401  (before any arithmetic)
import e3dge_amd  # noqa: E402,F401
from e3dge_amd import synthetic as syn  # noqa: E402
import test_hgfilter_host as host  # noqa: E402


def reference_filter(name):
    """The parameterised parts of the reference's netLocal filter in one module, weights from our whole synthetic state dict."""
    from oracle import ref_harness
    ref_harness.prepare()
    hgf = importlib.import_module("project.vendor.pifu.lib.model.HGFilters")
    helpers = importlib.import_module("project.models.helper_modules.helpers")
    inorm = lambda dim: torch.nn.InstanceNorm2d(dim, track_running_stats=False, affine=True)
    front = lambda cin: torch.nn.Sequential(helpers.conv3x3(cin, 32), helpers.ResidualBlock(32, 32, norm_layer=inorm), helpers.conv1x1(32, 32))
    ref = torch.nn.Module()
    ref.image_filter = hgf.HGFilter(syn.pifu_opt(**host.CASES[name][0]))
    ref.downsample_channel_conv = helpers.conv(512, 64, 3, 1, norm='in')
    ref.depth_conv = front(1)
    ref.residual_conv = front(3)
    ref.load_state_dict(host.module_cpu(name).state_dict(), strict=True)
    return ref.eval()


def main():
    from oracle import golden_store
    arrays, seconds, keys = {}, {}, None
    with torch.no_grad():
        for name, (over, n, h, w, through_filter) in sorted(host.CASES.items()):
            ref = reference_filter(name)
            if keys is None and not over:
                keys = sorted(ref.state_dict().keys())
            inputs = host.case_inputs(name)
            t0 = time.time()
            if through_filter:
                feats = torch.cat((ref.residual_conv(inputs[0]), ref.depth_conv(inputs[1])), 1)      # HGPIFuGANNetResidualInputResnetFC.py:60-71
            else:
                feats = inputs[0]
            outs, tmpx, normx = ref.image_filter(feats)
            seconds[name] = round(time.time() - t0, 3)
            names = host.tensor_names(name)
            assert len(names) == len(outs) + 2
            for key, t in zip(names, list(outs) + [tmpx, normx]):
                flat = t.reshape(-1)
                arrays[f"{name}_{key}"] = flat[host.samples(flat.numel())].numpy()
                arrays[f"{name}_{key}_sum"] = np.float64(t.double().sum().item())
            if name == "default":
                arrays["default_last_image0"] = outs[-1][0].numpy()
    with open(os.path.join(GOLD, "hgfilter_state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    path = golden_store.save(GOLD, "hgfilter", arrays)
    report = dict(torch=torch.__version__, threads=torch.get_num_threads(), npz_bytes=os.path.getsize(path), keys=len(keys), seconds=seconds)
    with open(os.path.join(GOLD, "hgfilter_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(report)


if __name__ == "__main__":
    main()
