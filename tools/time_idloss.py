#!/usr/bin/env python3
"""Time of one identity-term forward (e3dge_amd.id_loss.IDLoss, csrc/idnet.hip) against the library chain: the module's own `facenet`
torch layers on the GPU (conv2d / batch_norm / prelu through MIOpen, the pooling and the dots as torch ops), in the same process on
the same GPU.

    python tools/time_idloss.py [--out FILE.json] [--steps 10] [--no-launches] [--no-graph] [--only B1_256]
    python tools/time_idloss.py --backward [--out profiles/idloss_bwd_times.json] [--steps 10] [--no-launches] [--only B1_256]

Cases: one 256^2 pair (the evaluation shape), B = 4 pairs, one 1024^2 pair (through the 256^2 pooling).  Estimator: warm-up, then
five blocks of `steps` forwards between two HIP events; the median block, per forward.  `graph_ms` is the same forward captured once
with e3dge_amd.graphs.GraphedCall and replayed.  `achieved` is the fraction of the fp32 matrix peak (157.3 TFLOP/s) the HIP path
reaches on the convolutions' and the head's 2 x MAC count.  Prints one JSON line per case.

--backward: forward + backward of the loss with respect to y_hat (one 256^2 pair, B = 4 pairs), IDLoss(differentiable=True) -- the
saving forward (csrc/idnet.hip) and the backward (csrc/idnet_bwd.h) -- against the same torch layers under autograd (y's features
under no_grad, as id_loss.py:36 detaches them), with the plain forward's time and the saved-state and workspace bytes beside it."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import e3dge_amd  # noqa: E402,F401
from e3dge_amd import graphs, synthetic as syn  # noqa: E402
from e3dge_amd.id_loss import CROP, IDLoss, UNITS  # noqa: E402

PEAK_F32_MATRIX = 157.3e12


def torch_chain(m, y_hat, y):
    """id_loss.py:29-55 with x = y on GPU tensors through the torch layers; returns the loss."""
    z = torch.cat([y_hat, y])
    if z.shape[-1] != 256:
        z = m.id_loss_pool(z)
    e = m.facenet(m.face_pool(z[:, :, CROP[0]:CROP[1], CROP[2]:CROP[3]]))
    B = y.shape[0]
    return (1 - (e[:B] * e[B:]).sum(1)).sum() / B


def torch_chain_grad(m, y_hat, y):
    """The loss with a graph to y_hat only, through the torch layers."""
    prep = lambda z: m.face_pool((z if z.shape[-1] == 256 else m.id_loss_pool(z))[:, :, CROP[0]:CROP[1], CROP[2]:CROP[3]])
    with torch.no_grad():
        fy = m.facenet(prep(y))
    fh = m.facenet(prep(y_hat))
    return (1 - (fh * fy).sum(1)).sum() / y.shape[0]


def backward_cases(args, dev):
    from e3dge_amd import _lib
    m = syn.load_synthetic_idloss(IDLoss(differentiable=True)).to(dev)
    lib, lines = _lib.load(), []
    for batch, size in ((1, 256), (4, 256)):
        if args.only and args.only != f"B{batch}_{size}":
            continue
        g = torch.Generator(device=dev).manual_seed(size + batch)
        y = torch.rand(batch, 3, size, size, device=dev, generator=g) * 2 - 1
        y_hat = (y + 0.3 * torch.randn(batch, 3, size, size, device=dev, generator=g)).clamp(-1, 1).requires_grad_(True)

        def step(loss_of):
            y_hat.grad = None
            loss_of().backward()
            return y_hat.grad

        hip, ref = lambda: step(lambda: m.run(y_hat, y)['loss']), lambda: step(lambda: torch_chain_grad(m, y_hat, y))
        with torch.no_grad():
            fwd = lambda: m.run(y_hat, y)['loss']
            t_fwd = block_ms(fwd, args.steps)
        a, b = hip().clone(), ref().clone()
        t_hip, t_ref = block_ms(hip, args.steps), block_ms(ref, args.steps)
        line = dict(case=f"B{batch}_{size}", hip_fwd_bwd_ms=t_hip[0], hip_fwd_bwd_ms_min=t_hip[1], hip_fwd_bwd_ms_max=t_hip[2],
                    torch_fwd_bwd_ms=t_ref[0], torch_fwd_bwd_ms_min=t_ref[1], torch_fwd_bwd_ms_max=t_ref[2],
                    ratio_torch_over_hip=t_ref[0] / t_hip[0], hip_plain_fwd_ms=t_fwd[0], hip_plain_fwd_ms_min=t_fwd[1],
                    hip_plain_fwd_ms_max=t_fwd[2], grad_rel_diff=float((a - b).abs().max() / b.abs().max()),
                    saved_bytes_per_image=lib.e3dge_idnet_saved_bytes(batch) / batch,
                    bwd_ws_bytes_per_image=lib.e3dge_idnet_bwd_ws_bytes(batch, size, size) / batch,
                    estimator=f"median of 5 blocks of {args.steps} forward + backward steps, HIP events")
        if not args.no_launches:
            line["hip_launches"], line["torch_launches"] = count_kernels(hip), count_kernels(ref)
            with torch.no_grad():
                line["hip_plain_fwd_launches"] = count_kernels(fwd)
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


def flops(n_images):
    f, size = 2 * 3 * 9 * 64 * 112 * 112, 112
    for cin, depth, stride in UNITS:
        out = size // stride
        f += 2 * 9 * cin * depth * size * size + 2 * 9 * depth * depth * out * out + (2 * cin * depth * out * out if cin != depth else 0)
        size = out
    return n_images * (f + 2 * 25088 * 512)


def block_ms(fn, steps, blocks=5, warmup=3):
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-launches", action="store_true")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--only", help="one case, e.g. B1_256")
    ap.add_argument("--backward", action="store_true", help="forward + backward of the loss with respect to y_hat")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    lines = backward_cases(args, dev) if args.backward else []
    m = syn.load_synthetic_idloss(IDLoss()).to(dev)
    with torch.no_grad():
        for batch, size in () if args.backward else ((1, 256), (4, 256), (1, 1024)):
            if args.only and args.only != f"B{batch}_{size}":
                continue
            g = torch.Generator(device=dev).manual_seed(size + batch)
            y = torch.rand(batch, 3, size, size, device=dev, generator=g) * 2 - 1
            y_hat = (y + 0.3 * torch.randn(batch, 3, size, size, device=dev, generator=g)).clamp(-1, 1)
            hip, lib = lambda: m.run(y_hat, y)['loss'], lambda: torch_chain(m, y_hat, y)
            a, b = float(hip()), float(lib())
            t_hip, t_lib = block_ms(hip, args.steps), block_ms(lib, args.steps)
            fl = flops(2 * batch)
            line = dict(case=f"B{batch}_{size}", hip_ms=t_hip[0], hip_ms_min=t_hip[1], hip_ms_max=t_hip[2], torch_ms=t_lib[0],
                        torch_ms_min=t_lib[1], torch_ms_max=t_lib[2], ratio_torch_over_hip=t_lib[0] / t_hip[0], gflop=fl / 1e9,
                        achieved=fl / (t_hip[0] * 1e-3) / PEAK_F32_MATRIX, value_hip=a, value_torch=b, abs_diff=abs(a - b),
                        estimator=f"median of 5 blocks of {args.steps} forwards, HIP events")
            if not args.no_graph:
                call = graphs.GraphedCall(lambda p, q: m.run(p, q)['loss'], y_hat.clone(), y.clone())
                t_graph = block_ms(lambda: call(y_hat, y), args.steps)
                line.update(graph_ms=t_graph[0], graph_ms_min=t_graph[1], graph_ms_max=t_graph[2])
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
