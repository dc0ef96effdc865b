"""Fixture for the E0 image encoder (tests/test_encoder_host.py, tests/test_gpu_encoder.py).  Authoring time only, CPU only; the tests never
run this.

    python tools/gen_golden_encoder.py

Imports the reference's HybridGradualStyleEncoder_V2 (project/models/encoders/fpn_encoders.py; GradualStyleBlock, bottleneck_IR_SE and
EqualLinear come with it), loads the synthetic weights of e3dge_amd.synthetic.load_synthetic_encoder and writes, under tests/golden/:
    encoder_state_dict_keys.json   the sorted keys of the reference module's state dict, at the scripts' options ("scripts", built on the
                                   meta device) and with single_decoder_layer ("single")
    encoder.npz                    no weights and no inputs (both are formulas).  For the input test_encoder_host.GOLDEN_CASE (256^2, B = 2)
                                   and the options test_encoder_host.options() and every returned tensor (thumb_out, stylegan_out,
                                   feat_maps, p32): 256 values at test_encoder_host.samples and the float64 sum, from the reference's fp32
                                   forward (<name>_f32, <name>_f32_sum) and from its float64 forward (<name>_f64, <name>_f64_sum,
                                   <name>_f64_max = max |f64|, <name>_err = max |f32 - f64| over the whole tensor)
    encoder_report.json            torch version, thread count, file size, seconds, the float64 run's standard deviations"""
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
import test_encoder_host as host  # noqa: E402


def reference_class():
    from oracle import ref_harness
    ref_harness.prepare()
    return importlib.import_module("project.models.encoders.fpn_encoders").HybridGradualStyleEncoder_V2


def main():
    from oracle import golden_store
    cls = reference_class()
    with torch.device("meta"):
        keys = dict(scripts=sorted(cls(50, 'ir_se', 9, syn.encoder_opt()).state_dict()))
    ref = syn.load_synthetic_encoder(cls(50, 'ir_se', 9, host.options())).eval()
    keys["single"] = sorted(ref.state_dict())
    ours = host.module_cpu()
    assert sorted(ours.state_dict()) == keys["single"]
    for k, v in ref.state_dict().items():
        assert torch.equal(v, ours.state_dict()[k]), k                # one recipe, whichever class carries the keys
    n, size, seed = host.GOLDEN_CASE
    x = host.encoder_input(n, size, seed)
    arrays, seconds, stds = {}, {}, {}
    with torch.no_grad():
        t0 = time.time()
        t32 = host.as_tensors(ref(x, return_featmap=True))
        seconds["f32"] = round(time.time() - t0, 3)
        t0 = time.time()
        t64 = host.as_tensors(ref.double()(x.double(), return_featmap=True))
        seconds["f64"] = round(time.time() - t0, 3)
    for key in host.TENSORS:
        a, b = t32[key], t64[key]
        assert a.dtype == torch.float32 and b.dtype == torch.float64
        at = host.samples(a.numel())
        arrays[f"{key}_f32"] = a.reshape(-1)[at].numpy()
        arrays[f"{key}_f32_sum"] = np.float64(a.double().sum().item())
        arrays[f"{key}_f64"] = b.reshape(-1)[at].numpy()
        arrays[f"{key}_f64_sum"] = np.float64(b.sum().item())
        arrays[f"{key}_f64_max"] = np.float64(b.abs().max().item())
        arrays[f"{key}_err"] = np.float64((a.double() - b).abs().max().item())
        stds[key] = float(b.std())
    with open(os.path.join(GOLD, "encoder_state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    path = golden_store.save(GOLD, "encoder", arrays)
    report = dict(torch=torch.__version__, threads=torch.get_num_threads(), npz_bytes=os.path.getsize(path), keys={k: len(v) for k, v in keys.items()},
                  seconds=seconds, f64_std=stds, f32_err={k: float(arrays[f"{k}_err"]) for k in host.TENSORS})
    with open(os.path.join(GOLD, "encoder_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(report)


if __name__ == "__main__":
    main()
