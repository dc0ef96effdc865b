#!/usr/bin/env python3
"""Time of the frozen discriminator (e3dge_amd.discriminator.Discriminator, csrc/disc.hip / disc_bwd.h) against the torch composition of
the same module (library convolutions through MIOpen, the package's stream ops; E3DGE_DISCRIMINATOR=torch's path), in the same process
on the same GPU.

    python tools/time_discriminator.py [--out FILE.json] [--steps 5] [--no-split] [--only B4]

Cases: the shapes of scripts/train/ffhq/stage2.2.sh -- D_init_size 256, channel_multiplier 2, 1024^2 input through pool_256 -- at B = 4 and
B = 1.  For each: the forward under no_grad, and forward + backward of g_nonsaturating_loss to the image, both paths.  Estimator:
warm-up, then five blocks of `steps` calls between two HIP events; the median block per call, with the fastest and slowest beside it.
`split` is the device time of one HIP forward + backward per kernel name (torch profiler), largest first.  `achieved` is the fraction of
the fp32 matrix peak (157.3 TFLOP/s) the HIP path reaches on the convolutions' and the head's 2 x MAC count (the backward counted as
one more forward: data gradients only).  Prints one JSON line per case."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import e3dge_amd  # noqa: E402,F401
from e3dge_amd import synthetic as syn  # noqa: E402
from e3dge_amd.discriminator import Discriminator  # noqa: E402
from e3dge_amd.losses import g_nonsaturating_loss  # noqa: E402

PEAK_F32_MATRIX = 157.3e12


def flops(m, n_images):
    """2 x MACs of one forward, from the layer list."""
    c, size = m.in_channel, m.init_size
    f = 2 * m.input_size * c * size * size
    for block in list(m.convs)[1:]:
        co = block.conv2[1].weight.shape[0]
        f += 2 * 9 * c * c * size * size + (2 * 9 * c * co + 2 * c * co) * (size // 2) ** 2
        c, size = co, size // 2
    return n_images * (f + 2 * 9 * 513 * 512 * 16 + 2 * 8192 * 512 + 2 * 512)


def block_ms(fn, steps, blocks=5, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / steps)
    return statistics.median(ts), min(ts), max(ts)


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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--only", help="one case, e.g. B4")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    m = syn.load_synthetic_discriminator(Discriminator(syn.discriminator_opt(256, 2))).to(dev)
    for p in m.parameters():
        p.requires_grad_(False)
    lines = []
    for batch in (4, 1):
        if args.only and args.only != f"B{batch}":
            continue
        g = torch.Generator(device=dev).manual_seed(batch)
        x = (torch.rand(batch, 3, 1024, 1024, device=dev, generator=g) * 2 - 1).requires_grad_(True)
        assert m.uses_hip(x)

        def step(forward):
            x.grad = None
            g_nonsaturating_loss(forward(x)).backward()
            return x.grad

        hip_fb, ref_fb = lambda: step(m), lambda: step(m.forward_torch)
        with torch.no_grad():
            a, b = m(x), m.forward_torch(x)
            t_hip_f, t_ref_f = block_ms(lambda: m(x), args.steps), block_ms(lambda: m.forward_torch(x), args.steps)
        ga, gb = hip_fb().clone(), ref_fb().clone()
        t_hip, t_ref = block_ms(hip_fb, args.steps), block_ms(ref_fb, args.steps)
        fl = flops(m, batch)
        line = dict(case=f"B{batch}_1024", gflop_forward=fl / 1e9,
                    hip_fwd_ms=t_hip_f[0], hip_fwd_ms_min=t_hip_f[1], hip_fwd_ms_max=t_hip_f[2],
                    torch_fwd_ms=t_ref_f[0], torch_fwd_ms_min=t_ref_f[1], torch_fwd_ms_max=t_ref_f[2],
                    hip_fwd_bwd_ms=t_hip[0], hip_fwd_bwd_ms_min=t_hip[1], hip_fwd_bwd_ms_max=t_hip[2],
                    torch_fwd_bwd_ms=t_ref[0], torch_fwd_bwd_ms_min=t_ref[1], torch_fwd_bwd_ms_max=t_ref[2],
                    ratio_torch_over_hip_fwd=t_ref_f[0] / t_hip_f[0], ratio_torch_over_hip_fwd_bwd=t_ref[0] / t_hip[0],
                    achieved_fwd=fl / (t_hip_f[0] * 1e-3) / PEAK_F32_MATRIX, achieved_fwd_bwd=2 * fl / (t_hip[0] * 1e-3) / PEAK_F32_MATRIX,
                    logits_rel_diff=float((a - b).abs().max() / b.abs().max()), grad_rel_diff=float((ga - gb).abs().max() / gb.abs().max()),
                    estimator=f"median of 5 blocks of {args.steps} calls, HIP events")
        if not args.no_split:
            line["split"] = kernel_split(hip_fb)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
