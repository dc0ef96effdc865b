"""Fixture for the backward of the hourglass image filter (tests/test_hgfilter_bwd_host.py, tests/test_gpu_hgfilter_bwd.py).  Authoring
time only, CPU only; the tests never run this.

    python tools/gen_golden_hgfilter_grads.py

Builds the reference's filter as tools/gen_golden_hgfilter.py does (its HGFilter, ResidualBlock, conv3x3 / conv1x1 / conv), loads the
synthetic weights and runs the reference's own autograd, in float32, on the two cases of test_gpu_hgfilter_bwd.BWD_CASES with their
inputs (a formula) and upstream gradients (seeded normal tensors).  Writes, under tests/golden/:
    hgfilter_grads.npz            no weights and no inputs.  For the gradient to every input (image and depth map, or the filter's own
                                  input) and to every parameter the forward reads: the values at test_gpu_hgfilter_bwd.grad_samples (256
                                  of an input's, 64 of a parameter's) and the float64 sum
    hgfilter_grads_report.json    torch version, thread count, file size, tensors and seconds per case"""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
GOLD = os.path.join(REPO, "tests", "golden")

import oracle.cpu_numerics  # noqa: E402,F401  (before any arithmetic)
import e3dge_amd  # noqa: E402,F401
import gen_golden_hgfilter as fwd  # noqa: E402
import test_gpu_hgfilter_bwd as bwd  # noqa: E402
import test_hgfilter_host as host  # noqa: E402


def main():
    from oracle import golden_store
    arrays, report = {}, {}
    for name, (over, n, h, w, through, _) in sorted(bwd.BWD_CASES.items()):
        host.CASES["_grads_" + name] = (over, n, h, w, through)      # gen_golden_hgfilter.reference_filter reads its options from there
        try:
            ref = fwd.reference_filter("_grads_" + name)
        finally:
            del host.CASES["_grads_" + name]
        ours = bwd.bwd_module(name)
        ref.load_state_dict(ours.state_dict(), strict=True)
        for p in ref.parameters():
            p.requires_grad_(True)
        inputs, ups = bwd.bwd_inputs(name)
        leaves = [t.clone().requires_grad_(True) for t in inputs]
        t0 = time.time()
        feats = torch.cat((ref.residual_conv(leaves[0]), ref.depth_conv(leaves[1])), 1) if through else leaves[0]
        outs, _, normx = ref.image_filter(feats)
        pairs = [(o, g) for o, g in zip(list(outs) + [normx], ups) if g is not None]
        by_key = dict(ref.named_parameters())
        keys = [k for k, _ in bwd.used_parameters(ours, name)]
        grads = torch.autograd.grad([o for o, _ in pairs], leaves + [by_key[k] for k in keys], [g for _, g in pairs])
        names = bwd.input_names(name) + keys
        for key, g in zip(names, grads):
            flat = g.reshape(-1)
            arrays[f"{name}__{key}"] = flat[bwd.grad_samples(flat.numel(), key in bwd.input_names(name))].numpy()
            arrays[f"{name}__{key}__sum"] = np.float64(g.double().sum().item())
        report[name] = dict(tensors=len(names), seconds=round(time.time() - t0, 3))
    path = golden_store.save(GOLD, "hgfilter_grads", arrays)
    report.update(torch=torch.__version__, threads=torch.get_num_threads(), npz_bytes=os.path.getsize(path))
    with open(os.path.join(GOLD, "hgfilter_grads_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(report)


if __name__ == "__main__":
    main()
