#!/usr/bin/env python3
"""Time of the hourglass image filter (e3dge_amd.hg_filter.ResidualImageFilter.filter, csrc/hgfilter.hip) against the torch composition
of the same module (library convolutions through MIOpen; E3DGE_HGFILTER=torch's path), in the same process on the same GPU.

    python tools/time_hg_filter.py [--out profiles/hgfilter_times.json] [--steps 25] [--only B4]
    python tools/time_hg_filter.py --split [--out profiles/hgfilter_split.json]          (a run of its own: nothing is timed in it)

Cases: filter() from a (B, 3, 256, 256) residual image and a (B, 1, 256, 256) depth map at the default options (num_stack 4,
num_hourglass 2), B = 1 and B = 4, under no_grad.  Estimator: warm-up of both paths, then five blocks of `steps` calls per path between
two HIP events (a block is 0.2 to 0.3 s), the two paths' blocks ALTERNATING so that a drift of the clocks meets both; the median block
per call, with the fastest and slowest beside it.  `--split`: the device time of one HIP call per kernel name (torch profiler), largest
first, from a process that times nothing else.  `achieved` is the fraction of the fp32 matrix peak (157.3 TFLOP/s) the HIP path
reaches on the convolutions' 2 x MAC count from the layer table.  What bounds the kernels is not established here: no counters are
taken.  One JSON line per case."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import e3dge_amd  # noqa: E402,F401
from e3dge_amd import synthetic as syn  # noqa: E402
from e3dge_amd.hg_filter import ConvBlock, ResidualImageFilter  # noqa: E402

PEAK_F32_MATRIX = 157.3e12


def flops(m, n_images, height, width):
    """2 x MACs of the convolutions of one filter() call, from the layer table."""
    hg = m.image_filter
    p1, p2, p4 = height * width, height * width // 4, height * width // 16
    block = lambda ci, co: 9 * (ci * co // 2 + co // 2 * co // 4 + co // 4 * co // 4) + (ci * co if ci != co else 0)
    macs = p1 * (9 * 3 * 32 + 9 * 1 * 32 + 2 * (2 * 9 * 32 * 32 + 32 * 32))                     # the two front nets
    macs += p2 * (49 * 64 * 64 + block(64, 128)) + p4 * (block(128, 128) + block(128, 256))
    b256 = block(256, 256)

    def level(d, p):                                                 # b1_d at p pixels; b2_d, b3_d and the inner part at p / 4
        return b256 * p + 2 * b256 * (p // 4) + (level(d - 1, p // 4) if d > 1 else b256 * (p // 4))
    S, D = hg.num_modules, hg.num_hourglass
    macs += S * (level(D, p4) + p4 * (b256 + 2 * 256 * 256)) + (S - 1) * p4 * 2 * 256 * 256
    assert sum(isinstance(q, ConvBlock) for q in hg.modules()) == 3 + S * (3 * D + 2)
    return 2 * n_images * macs


def alternating_block_ms(fns, steps, blocks=5, warmup=3):
    """[(median, fastest, slowest) ms per call] of every function of `fns`: block k of each runs before block k + 1 of any."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(blocks):
        for t, fn in zip(ts, fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) / steps)
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def kernel_split(fn):
    """{kernel name: [launches, device ms]} of one call."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        if str(e.device_type).endswith("CUDA"):
            name = e.name.split("(")[0][:80]
            n, ms = out.get(name, (0, 0.0))
            out[name] = (n + 1, ms + e.device_time / 1e3)
    return dict(sorted(((k, [v[0], round(v[1], 4)]) for k, v in out.items()), key=lambda kv: -kv[1][1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--split", action="store_true", help="only the per-kernel device times of one HIP call")
    ap.add_argument("--only", help="one case, e.g. B4")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    m = syn.load_synthetic_hgfilter(ResidualImageFilter(syn.pifu_opt())).to(dev).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    lines = []
    for batch in (1, 4):
        if args.only and args.only != f"B{batch}":
            continue
        g = torch.Generator(device=dev).manual_seed(batch)
        image = torch.rand(batch, 3, 256, 256, device=dev, generator=g) * 2 - 1
        depth = torch.rand(batch, 1, 256, 256, device=dev, generator=g) * 2 - 1
        assert m._runs_hip(image, depth)

        def run_torch():
            os.environ["E3DGE_HGFILTER"] = "torch"
            try:
                return m.filter(image, depth, return_feat=True)[0]
            finally:
                del os.environ["E3DGE_HGFILTER"]

        run_hip = lambda: m.filter(image, depth, return_feat=True)[0]
        with torch.no_grad():
            if args.split:
                line = dict(case=f"B{batch}_256", split=kernel_split(run_hip))
                print(json.dumps(line), flush=True)
                lines.append(line)
                continue
            a, b = run_hip(), run_torch()
            t_hip, t_ref = alternating_block_ms([run_hip, run_torch], args.steps)
            fl = flops(m, batch, 256, 256)
            line = dict(case=f"B{batch}_256", gflop=fl / 1e9, hip_ms=t_hip[0], hip_ms_min=t_hip[1], hip_ms_max=t_hip[2],
                        torch_ms=t_ref[0], torch_ms_min=t_ref[1], torch_ms_max=t_ref[2], ratio_torch_over_hip=t_ref[0] / t_hip[0],
                        achieved=fl / (t_hip[0] * 1e-3) / PEAK_F32_MATRIX, map_rel_diff=float((a - b).abs().max() / b.abs().max()),
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
