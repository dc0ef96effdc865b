"""Fixture for the trainable 2-D residual aligner (tests/test_aligner_bwd_host.py, tests/test_gpu_aligner_bwd.py).  Authoring time only, CPU
only; the tests never run this.

    python tools/gen_golden_aligner_grads.py

Imports the reference's ResidualAligner (project/models/helper_modules/alignment_old.py), loads the synthetic weights of
e3dge_amd.synthetic.load_synthetic_aligner, puts it in train() (stage 2.1's form: BatchNorm on batch statistics) and records one step
under autograd -- forward of test_aligner_host.aligner_input(2, 0), backward of sum(out * upstream) with the fixed upstream of
tests (numpy RandomState(77), N(0, 1)) -- in float32 and in float64.  Writes tests/golden/aligner_grads.npz:
    names                         'dx', then the 157 parameter names in named_parameters() order
    samples_f32, samples_f64      (158, 64): every gradient tensor at the first 64 positions of test_encoder_host.samples
    sum_f32, sum_f64              (158,): the float64 sum of every gradient tensor (of the float32 run, of the float64 run)
    max_f64, err                  (158,): max |f64| and max |f32 - f64| over the whole tensor
    buffer_names, buffer_<i>_f32 / _f64   the running_mean and running_var of three BatchNorms after the step
and tests/golden/aligner_grads_report.json (torch version, threads, file size, seconds)."""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")

import oracle.cpu_numerics  # noqa: E402,F401  (before any arithmetic)
import e3dge_amd  # noqa: E402,F401
from e3dge_amd import synthetic as syn  # noqa: E402
import test_aligner_host as host  # noqa: E402
from gen_golden_aligner import build, reference_class  # noqa: E402

CASE = (2, 0)                                                         # batch, input seed
N_SAMPLES = 64
BUFFERS = ("conv_layer1.1", "conv_layer3.1.res_layer.4", "dconv_layer1.0.shortcut_layer.1")


def upstream(n):
    return torch.from_numpy(np.random.RandomState(77).standard_normal((n, 3, 256, 256)).astype(np.float32))


def step(ref, x, g):
    """{'dx' | parameter name: gradient}, {buffer name: value after the step} of one train-form step."""
    ref.train()
    for p in ref.parameters():
        p.requires_grad_(True)
        p.grad = None
    x = x.clone().requires_grad_(True)
    (ref(x) * g).sum().backward()
    grads = dict(dx=x.grad, **{k: p.grad for k, p in ref.named_parameters()})
    state = ref.state_dict()
    return grads, {f"{b}.{s}": state[f"{b}.{s}"].clone() for b in BUFFERS for s in ("running_mean", "running_var")}


def main():
    from oracle import golden_store
    cls = reference_class()
    n, seed = CASE
    x, g = host.aligner_input(n, seed), upstream(n)
    seconds = {}
    t0 = time.time()
    g32, b32 = step(syn.load_synthetic_aligner(build(cls)), x, g)
    seconds["f32"] = round(time.time() - t0, 3)
    t0 = time.time()
    g64, b64 = step(syn.load_synthetic_aligner(build(cls)).double(), x.double(), g.double())
    seconds["f64"] = round(time.time() - t0, 3)
    names = list(g32)
    assert names == list(g64) and len(names) == 158
    rows = {k: [] for k in ("samples_f32", "samples_f64", "sum_f32", "sum_f64", "max_f64", "err")}
    for k in names:
        a, b = g32[k], g64[k]
        assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == b.shape
        at = host.samples(a.numel())[:N_SAMPLES]
        rows["samples_f32"].append(a.reshape(-1)[at].numpy())
        rows["samples_f64"].append(b.reshape(-1)[at].numpy())
        rows["sum_f32"].append(a.double().sum().item())
        rows["sum_f64"].append(b.sum().item())
        rows["max_f64"].append(b.abs().max().item())
        rows["err"].append((a.double() - b).abs().max().item())
    arrays = {k: np.stack(v) if k.startswith("samples") else np.asarray(v, dtype=np.float64) for k, v in rows.items()}
    arrays["names"] = np.asarray(names)
    arrays["buffer_names"] = np.asarray(list(b32))
    for i, k in enumerate(b32):
        arrays[f"buffer_{i}_f32"], arrays[f"buffer_{i}_f64"] = b32[k].numpy(), b64[k].numpy()
    path = golden_store.save(GOLD, "aligner_grads", arrays)
    report = dict(torch=torch.__version__, threads=torch.get_num_threads(), npz_bytes=os.path.getsize(path), seconds=seconds, tensors=len(names),
                  dx_max=float(arrays["max_f64"][0]), dx_err=float(arrays["err"][0]))
    with open(os.path.join(GOLD, "aligner_grads_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(report)


if __name__ == "__main__":
    main()
