#!/usr/bin/env python3
"""Time of one LPIPS forward (e3dge_amd.lpips.LPIPS, csrc/lpips.hip) against the library formulation a user runs today: the same
forward as torch ops on GPU tensors (conv2d / max_pool2d through MIOpen), in the same process on the same GPU.

    python tools/time_lpips.py [--out FILE.json] [--steps 20] [--no-launches] [--backward]

Cases: 256^2 with B = 1 and B = 8, 1024^2 with B = 1 (what the C3 leg of bench.py hands to image_metrics).  Estimator: warm-up, then
five blocks of `steps` forwards between two HIP events; the median block, per forward.  `achieved` is the fraction of the fp32
matrix peak (157.3 TFLOP/s) the HIP path reaches on the convolutions' 2 x MAC count.  The device kernels of one forward of each path are
counted with torch.profiler (--no-launches skips that, e.g. under another profiler).  Prints one JSON line per case.

--backward times the training direction instead: forward + backward with the gradient to x only (LPIPS(differentiable=True), csrc/
lpips_bwd.h) against autograd through the same torch ops, at 256^2 with B = 1 and B = 4 (the samples per GPU of a training step) and
1024^2 with B = 1; same estimator; `grad_rel_diff` is max|hip - torch| / max|torch| of the two gradients."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import e3dge_amd  # noqa: E402,F401
from e3dge_amd import synthetic as syn  # noqa: E402
from e3dge_amd.lpips import CONVS, LPIPS, tap_shapes  # noqa: E402

PEAK_F32_MATRIX = 157.3e12


def torch_lpips(sd, x, y):
    """lpips.py:33-39 with networks.py:52-65 and utils.py:6-9 as torch ops."""
    B = x.shape[0]
    z = (torch.cat([x, y]) - sd['net.mean']) / sd['net.std']
    res = []
    for i in range(11):
        if i in CONVS:
            _, _, _, s, p = CONVS[i]
            z = F.relu(F.conv2d(z, sd[f'net.layers.{i}.weight'], sd[f'net.layers.{i}.bias'], stride=s, padding=p))
            t = z / (torch.sqrt(torch.sum(z ** 2, dim=1, keepdim=True) + 1e-8) + 1e-10)
            res.append(F.conv2d((t[:B] - t[B:]) ** 2, sd[f'lin.{len(res)}.1.weight']).mean((2, 3), True))
        elif i in (2, 5):
            z = F.max_pool2d(z, 3, 2)
    return torch.sum(torch.cat(res, 0)) / B


def conv_flops(batch, height, width):
    """2 x MACs of the five convolutions for the 2 B images of a batch of pairs."""
    return sum(2 * 2 * batch * c * h * w * CONVS[i][0] * CONVS[i][2] ** 2 for i, (c, h, w) in zip(CONVS, tap_shapes(height, width)))


def block_ms(fn, steps, blocks=5, warmup=5):
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


def count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-launches", action="store_true")
    ap.add_argument("--backward", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    m = syn.load_synthetic_lpips(LPIPS()).to(dev)
    sd = {k: v for k, v in m.state_dict().items()}
    lines = []
    if args.backward:
        m.differentiable = True
        for batch, size in ((1, 256), (4, 256), (1, 1024)):
            g = torch.Generator(device=dev).manual_seed(size + batch)
            x = (torch.rand(batch, 3, size, size, device=dev, generator=g) * 2 - 1).requires_grad_(True)
            y = (x.detach() + 0.3 * torch.randn(batch, 3, size, size, device=dev, generator=g)).clamp(-1, 1)

            def step(fn):
                x.grad = None
                fn(x, y).backward()
                return x.grad

            hip, lib = lambda: step(m), lambda: step(lambda a, b: torch_lpips(sd, a, b))
            ga, gb = hip().clone(), lib().clone()
            t_hip, t_lib = block_ms(hip, args.steps), block_ms(lib, args.steps)
            line = dict(case=f"B{batch}_{size}", what="forward + backward, gradient to x", hip_ms=t_hip[0], hip_ms_min=t_hip[1],
                        hip_ms_max=t_hip[2], torch_ms=t_lib[0], torch_ms_min=t_lib[1], torch_ms_max=t_lib[2], speedup=t_lib[0] / t_hip[0],
                        grad_rel_diff=float((ga - gb).abs().max() / gb.abs().max()),
                        estimator=f"median of 5 blocks of {args.steps} steps, HIP events")
            if not args.no_launches:
                line["hip_launches"], line["torch_launches"] = count_kernels(hip), count_kernels(lib)
            print(json.dumps(line), flush=True)
            lines.append(line)
    with torch.no_grad():
        for batch, size in () if args.backward else ((1, 256), (8, 256), (1, 1024)):
            g = torch.Generator(device=dev).manual_seed(size + batch)
            x = torch.rand(batch, 3, size, size, device=dev, generator=g) * 2 - 1
            y = (x + 0.3 * torch.randn(batch, 3, size, size, device=dev, generator=g)).clamp(-1, 1)
            hip, lib = lambda: m(x, y), lambda: torch_lpips(sd, x, y)
            a, b = float(hip()), float(lib())
            t_hip, t_lib = block_ms(hip, args.steps), block_ms(lib, args.steps)
            flops = conv_flops(batch, size, size)
            line = dict(case=f"B{batch}_{size}", hip_ms=t_hip[0], hip_ms_min=t_hip[1], hip_ms_max=t_hip[2], torch_ms=t_lib[0],
                        torch_ms_min=t_lib[1], torch_ms_max=t_lib[2], speedup=t_lib[0] / t_hip[0], conv_gflop=flops / 1e9,
                        achieved=flops / (t_hip[0] * 1e-3) / PEAK_F32_MATRIX, value_hip=a, value_torch=b, rel_diff=abs(a - b) / abs(b),
                        estimator=f"median of 5 blocks of {args.steps} forwards, HIP events")
            if not args.no_launches:
                line["hip_launches"], line["torch_launches"] = count_kernels(hip), count_kernels(lib)
            print(json.dumps(line), flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
