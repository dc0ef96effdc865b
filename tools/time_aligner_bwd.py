#!/usr/bin/env python3
"""Time of forward + backward of the 2-D residual aligner in the train form with every parameter trainable
(ResidualAligner(differentiable=True).train(): csrc/aligner_train.h) against the torch composition of the same module under autograd
(library convolutions and BatchNorm through MIOpen; E3DGE_ALIGNER=torch's path), in the same process on the same GPU.

    python tools/time_aligner_bwd.py [--out profiles/aligner_bwd_times.json] [--steps 5] [--only B4]
    python tools/time_aligner_bwd.py --split [--out profiles/aligner_bwd_split.json]      (a run of its own: nothing is timed in it)

Cases: forward of a (B, 6, 256, 256) input, then the backward of sum(out * fixed upstream), B = 1, 4 and 8 (stage 2.1 runs 8 per GPU).
Each case twice: with the packed weight images cached (`cached`), and with the images rebuilt before every call as after an optimiser
step (`repack`: ResidualAligner.invalidate(); on the torch path nothing is packed).  Protocol of tools/time_hg_filter_bwd.py: both paths
warmed, five alternating blocks between HIP events, the median block per call with the fastest and slowest beside it.  What bounds the
kernels is not established here: no counters are taken.  One JSON line per case."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import e3dge_amd  # noqa: E402,F401
from e3dge_amd import synthetic as syn  # noqa: E402
from e3dge_amd.alignment import ResidualAligner  # noqa: E402
from time_hg_filter import alternating_block_ms, kernel_split  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--split", action="store_true", help="only the per-kernel device times of one HIP forward + backward")
    ap.add_argument("--only", help="one case, e.g. B4")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    m = syn.load_synthetic_aligner(ResidualAligner(syn.aligner_opt(), differentiable=True)).to(dev).train()
    watched = m.dconv_layer1[0].res_layer[1].weight
    lines = []
    for batch in (1, 4, 8):
        if args.only and args.only != f"B{batch}":
            continue
        g = torch.Generator(device=dev).manual_seed(batch)
        x = torch.randn(batch, 6, 256, 256, device=dev, generator=g)
        up = torch.randn(batch, 3, 256, 256, device=dev, generator=g)
        assert m._runs_hip_grad(x)

        def step(repack):
            if repack:
                m.invalidate()
            m.zero_grad(set_to_none=True)
            (m(x) * up).sum().backward()
            return watched.grad

        def on_torch(repack):
            os.environ["E3DGE_ALIGNER"] = "torch"
            try:
                return step(repack)
            finally:
                del os.environ["E3DGE_ALIGNER"]

        if args.split:
            line = dict(case=f"B{batch}_256", split=kernel_split(lambda: step(False)))
            print(json.dumps(line), flush=True)
            lines.append(line)
            continue
        a, b = step(False).clone(), on_torch(False).clone()
        line = dict(case=f"B{batch}_256", form="train, all parameters trainable", watched_grad_rel_diff=float((a - b).abs().max() / b.abs().max()),
                    saved_bytes_per_image=e3dge_amd._lib.query("e3dge_aligner_saved_bytes", 1),
                    bound="not established (no counters taken)",
                    estimator=f"median of 5 blocks of {args.steps} forward + backward per path, the paths' blocks alternating, HIP events")
        for label, repack in (("cached", False), ("repack", True)):
            t_hip, t_ref = alternating_block_ms([lambda: step(repack), lambda: on_torch(repack)], args.steps, warmup=2)
            line.update({f"{label}_hip_ms": t_hip[0], f"{label}_hip_ms_min": t_hip[1], f"{label}_hip_ms_max": t_hip[2], f"{label}_torch_ms": t_ref[0],
                         f"{label}_torch_ms_min": t_ref[1], f"{label}_torch_ms_max": t_ref[2], f"{label}_ratio_torch_over_hip": t_ref[0] / t_hip[0]})
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
