#!/usr/bin/env python3
"""Time of forward + backward of the hourglass image filter with every parameter trainable (ResidualImageFilter(differentiable=True):
csrc/hgfilter.hip's saving forward and csrc/hgfilter_bwd.h) against the torch composition of the same module under autograd (library
convolutions through MIOpen; E3DGE_HGFILTER=torch's path), in the same process on the same GPU.

    python tools/time_hg_filter_bwd.py [--out profiles/hgfilter_bwd_times.json] [--steps 5] [--only B4]
    python tools/time_hg_filter_bwd.py --split [--out profiles/hgfilter_bwd_split.json]      (a run of its own: nothing is timed in it)

Cases: filter() from a (B, 3, 256, 256) residual image and a (B, 1, 256, 256) depth map at the default options, then the backward of
sum(map * fixed upstream), B = 1 and B = 4.  Each case twice: with the packed weight images cached (`cached`), and with the images
rebuilt before every call as after an optimiser step (`repack`: HGFilter.invalidate(); on the torch path nothing is packed).  Protocol
of tools/time_hg_filter.py: both paths warmed, five alternating blocks between HIP events, the median block per call with the fastest
and slowest beside it.  What bounds the kernels is not established here: no counters are taken.  One JSON line per case."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import e3dge_amd  # noqa: E402,F401
from e3dge_amd import synthetic as syn  # noqa: E402
from e3dge_amd.hg_filter import ResidualImageFilter  # noqa: E402
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
    m = syn.load_synthetic_hgfilter(ResidualImageFilter(syn.pifu_opt(), differentiable=True)).to(dev).eval()
    lines = []
    for batch in (1, 4):
        if args.only and args.only != f"B{batch}":
            continue
        g = torch.Generator(device=dev).manual_seed(batch)
        image = torch.rand(batch, 3, 256, 256, device=dev, generator=g) * 2 - 1
        depth = torch.rand(batch, 1, 256, 256, device=dev, generator=g) * 2 - 1
        up = torch.randn(batch, 256, 64, 64, device=dev, generator=g)
        assert m._runs_hip_grad(image, depth)

        def step(repack):
            if repack:
                m.invalidate()
            m.zero_grad(set_to_none=True)
            (m.filter(image, depth, return_feat=True)[0] * up).sum().backward()
            return m.image_filter.conv4.conv1.weight.grad

        def on_torch(repack):
            os.environ["E3DGE_HGFILTER"] = "torch"
            try:
                return step(repack)
            finally:
                del os.environ["E3DGE_HGFILTER"]

        if args.split:
            line = dict(case=f"B{batch}_256", split=kernel_split(lambda: step(False)))
            print(json.dumps(line), flush=True)
            lines.append(line)
            continue
        a, b = step(False).clone(), on_torch(False).clone()
        line = dict(case=f"B{batch}_256", conv4_conv1_grad_rel_diff=float((a - b).abs().max() / b.abs().max()),
                    saved_bytes_per_image=e3dge_amd._lib.query("e3dge_hgf_saved_bytes", 1, 256, 256, 4, 2),
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
