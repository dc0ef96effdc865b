#!/usr/bin/env python3
"""Time of the 2-D residual aligner (e3dge_amd.alignment.ResidualAligner, csrc/aligner.hip) against the torch composition of the same
module (library convolutions through MIOpen; E3DGE_ALIGNER=torch's path), in the same process on the same GPU.

    python tools/time_aligner.py [--out profiles/aligner_times.json] [--steps 10] [--only B4]
    python tools/time_aligner.py --split [--out profiles/aligner_split.json]          (a run of its own: nothing is timed in it)

Cases: forward(x) of a (B, 6, 256, 256) input, B = 1 and B = 4, under no_grad.  Estimator: warm-up of both paths, then five blocks of
`steps` calls per path between two HIP events, the two paths' blocks ALTERNATING so that a drift of the clocks meets both; the median
block per call, with the fastest and slowest beside it.  `--split`: the device time of one HIP call per launch, in launch order (torch
profiler), from a process that times nothing else.  `achieved` is the fraction of the fp32 matrix peak (157.3 TFLOP/s) the HIP path
reaches on the convolutions' 2 x MAC count from the layer table.  What bounds the kernels is not established here: no counters are
taken.  One JSON line per case."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import e3dge_amd  # noqa: E402,F401
from e3dge_amd import alignment, synthetic as syn  # noqa: E402
from e3dge_amd.alignment import ResidualAligner  # noqa: E402
from time_encoder import PEAK_F32_MATRIX, alternating_block_ms  # noqa: E402

STAGE_SIZE = dict(conv_layer2=256, conv_layer3=128, conv_layer4=64, dconv_layer1=64, dconv_layer2=128, dconv_layer3=256)


def macs():
    """MACs of the convolutions of one image, per stage."""
    out = dict(conv_layer1=54 * 16 * 256 * 256)
    for name, units in alignment.STAGES.items():
        s, total = STAGE_SIZE[name], 0
        for cin, depth, stride in units:
            o = s // stride
            total += 9 * cin * depth * s * s + 9 * depth * depth * o * o + (cin * depth * o * o if cin != depth else 0)
            s = o
        out[name] = total
    return out


def launch_split(fn):
    """[[kernel name, device ms]] of one call, in launch order."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    events = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
    events.sort(key=lambda e: e.time_range.start)
    return [[e.name.split("(")[0][:80], round(e.device_time / 1e3, 4)] for e in events]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--split", action="store_true", help="only the per-launch device times of one HIP call")
    ap.add_argument("--only", help="one case, e.g. B4")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    m = syn.load_synthetic_aligner(ResidualAligner(syn.aligner_opt())).to(dev).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    lines = []
    for batch in (1, 4):
        if args.only and args.only != f"B{batch}":
            continue
        g = torch.Generator(device=dev).manual_seed(batch)
        x = torch.randn(batch, 6, 256, 256, device=dev, generator=g)
        assert m._runs_hip(x)

        def run_torch():
            os.environ["E3DGE_ALIGNER"] = "torch"
            try:
                return m(x)
            finally:
                del os.environ["E3DGE_ALIGNER"]

        run_hip = lambda: m(x)
        with torch.no_grad():
            if args.split:
                per_launch = launch_split(run_hip)
                by_name = {}
                for name, ms in per_launch:
                    n, total = by_name.get(name, (0, 0.0))
                    by_name[name] = (n + 1, round(total + ms, 4))
                line = dict(case=f"B{batch}_256", launches=len(per_launch), by_kernel=by_name, per_launch=per_launch)
                print(json.dumps(line), flush=True)
                lines.append(line)
                continue
            a, b = run_hip(), run_torch()
            t_hip, t_ref = alternating_block_ms([run_hip, run_torch], args.steps)
            parts = macs()
            fl = 2 * batch * sum(parts.values())
            line = dict(case=f"B{batch}_256", gflop=fl / 1e9, gmac_per_image={k: round(v / 1e9, 3) for k, v in parts.items()},
                        hip_ms=t_hip[0], hip_ms_min=t_hip[1], hip_ms_max=t_hip[2], torch_ms=t_ref[0], torch_ms_min=t_ref[1], torch_ms_max=t_ref[2],
                        ratio_torch_over_hip=t_ref[0] / t_hip[0], images_per_s=batch / (t_hip[0] * 1e-3),
                        achieved=fl / (t_hip[0] * 1e-3) / PEAK_F32_MATRIX, rel_diff=float((a - b).abs().max() / b.abs().max()),
                        bound="not established (no counters taken)",
                        estimator=f"median of 5 blocks of {args.steps} calls per path, the paths' blocks alternating, HIP events")
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
