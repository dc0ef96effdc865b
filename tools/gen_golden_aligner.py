"""Fixture for the 2-D residual aligner (tests/test_aligner_host.py, tests/test_gpu_aligner.py).  Authoring time only, CPU only; the tests
never run this.

    python tools/gen_golden_aligner.py

Imports the reference's ResidualAligner (project/models/helper_modules/alignment_old.py; bottleneck_IR and DemodulatedConv2d come with
it), loads the synthetic weights of e3dge_amd.synthetic.load_synthetic_aligner and writes, under tests/golden/:
    aligner_state_dict_keys.json   the sorted keys of the reference module's state dict with aligner_norm_type 'batch' (the scripts'),
                                   'instance', 'none' and with aligner_demodulate
    aligner.npz                    no weights and no inputs (both are formulas).  For the input test_aligner_host.GOLDEN_CASE (256^2, B = 2)
                                   and the output and the seven taps (feat1..4, dfea1..3: every stage's output, taken with forward hooks):
                                   256 values at test_encoder_host.samples and the float64 sum, from the reference's fp32 forward
                                   (<name>_f32, <name>_f32_sum) and from its float64 forward (<name>_f64, <name>_f64_sum,
                                   <name>_f64_max = max |f64|, <name>_err = max |f32 - f64| over the whole tensor)
    aligner_report.json            torch version, thread count, file size, seconds, the float64 run's standard deviations"""
import contextlib
import importlib
import io
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
from e3dge_amd import alignment, synthetic as syn  # noqa: E402
import test_aligner_host as host  # noqa: E402

STAGE_OF_TAP = dict(zip(alignment.TAPS, ("conv_layer1",) + tuple(alignment.STAGES)))


def reference_class():
    from oracle import ref_harness
    ref_harness.prepare()
    return importlib.import_module("project.models.helper_modules.alignment_old").ResidualAligner


def build(cls, **over):
    with contextlib.redirect_stdout(io.StringIO()):                   # (the reference prints its norm type)
        return cls(syn.aligner_opt(**over))


def run_with_taps(ref, x):
    taps, hooks = {}, []
    for name, stage in STAGE_OF_TAP.items():
        hooks.append(getattr(ref, stage).register_forward_hook(lambda mod, inp, out, name=name: taps.__setitem__(name, out)))
    try:
        with torch.no_grad():
            out = ref(x)
    finally:
        for h in hooks:
            h.remove()
    return dict(out=out, **taps)


def main():
    from oracle import golden_store
    cls = reference_class()
    keys = {}
    with torch.device("meta"):
        for name, over in [("instance", dict(aligner_norm_type='instance')), ("none", dict(aligner_norm_type='none')),
                           ("demodulate", dict(aligner_demodulate=True))]:
            keys[name] = sorted(build(cls, **over).state_dict())
    ref = syn.load_synthetic_aligner(build(cls)).eval()
    keys["batch"] = sorted(ref.state_dict())
    ours = host.module_cpu()
    assert sorted(ours.state_dict()) == keys["batch"] and len(keys["batch"]) == 295
    for k, v in ref.state_dict().items():
        assert torch.equal(v, ours.state_dict()[k]), k                # one recipe, whichever class carries the keys
    n, seed = host.GOLDEN_CASE
    x = host.aligner_input(n, seed)
    arrays, seconds, stds = {}, {}, {}
    t0 = time.time()
    t32 = run_with_taps(ref, x)
    seconds["f32"] = round(time.time() - t0, 3)
    t0 = time.time()
    t64 = run_with_taps(ref.double(), x.double())
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
    with open(os.path.join(GOLD, "aligner_state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    path = golden_store.save(GOLD, "aligner", arrays)
    report = dict(torch=torch.__version__, threads=torch.get_num_threads(), npz_bytes=os.path.getsize(path), keys={k: len(v) for k, v in keys.items()},
                  parameters=sum(p.numel() for p in ref.parameters()), seconds=seconds, f64_std=stds,
                  f64_max={k: float(arrays[f"{k}_f64_max"]) for k in host.TENSORS}, f32_err={k: float(arrays[f"{k}_err"]) for k in host.TENSORS})
    with open(os.path.join(GOLD, "aligner_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(report)


if __name__ == "__main__":
    main()
