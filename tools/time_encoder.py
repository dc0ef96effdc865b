#!/usr/bin/env python3
"""Time of the E0 image encoder (e3dge_amd.encoders.HybridGradualStyleEncoder_V2, csrc/encoder.h) against the torch composition of the
same module (library convolutions through MIOpen; E3DGE_ENCODER=torch's path), in the same process on the same GPU.

    python tools/time_encoder.py [--out profiles/encoder_times.json] [--steps 10] [--only B4]
    python tools/time_encoder.py --split [--out profiles/encoder_split.json]          (a run of its own: nothing is timed in it)

Cases: forward(x, return_featmap=True) of a (B, 3, 256, 256) image at the scripts' options with single_decoder_layer (the unread decoder
heads are not built), B = 1 and B = 4, under no_grad.  Estimator: warm-up of both paths, then five blocks of `steps` calls per path
between two HIP events, the two paths' blocks ALTERNATING so that a drift of the clocks meets both; the median block per call, with the
fastest and slowest beside it.  `--split`: the device time of one HIP call per kernel name (torch profiler), largest first, from a
process that times nothing else.  `achieved` is the fraction of the fp32 matrix peak (157.3 TFLOP/s) the HIP path reaches on the
convolutions' 2 x MAC count from the layer table.  What bounds the kernels is not established here: no counters are taken.  One JSON line
per case."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import e3dge_amd  # noqa: E402,F401
from e3dge_amd import synthetic as syn  # noqa: E402
from e3dge_amd.encoders import HybridGradualStyleEncoder_V2, units  # noqa: E402

PEAK_F32_MATRIX = 157.3e12


def macs(m, size):
    """MACs of the convolutions and linear layers of one image: dict(body, laterals, renderer_heads, decoder_head)."""
    body, s = 27 * 64 * size * size, size
    for cin, depth, stride in units(50):
        o = s // stride
        body += 9 * cin * depth * s * s + 9 * depth * depth * o * o + (cin * depth * o * o if cin != depth else 0) + 2 * depth * depth // 16
        s = o
    lat = 512 * (256 * (size // 8) ** 2 + 128 * (size // 4) ** 2 + (64 * (size // 2) ** 2 if m.enable_decoder else 0))

    def head(h, s):
        total = 0
        for c in h.conv_layers():
            s = (s + 1) // 2
            total += 9 * c.in_channels * c.out_channels * s * s
        return total + h.out_c * h.out_c
    tex = size // 4 if m.opts.fpn_pigan_tex_layer_dim == 64 else size // 8
    pigan = sum(head(h, size // 8 if j < 6 else tex) for j, h in enumerate(m.styles_pigan))
    dec = head(m.styles_stylegan[0], size // 2) if m.enable_decoder else 0
    return dict(body=body, laterals=lat, renderer_heads=pigan, decoder_head=dec)


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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--split", action="store_true", help="only the per-kernel device times of one HIP call")
    ap.add_argument("--only", help="one case, e.g. B4")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    with torch.device("meta"):
        m = HybridGradualStyleEncoder_V2(50, 'ir_se', 9, syn.encoder_opt(single_decoder_layer=True))
    m = syn.load_synthetic_encoder(m.to_empty(device="cpu")).to(dev).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    lines = []
    for batch in (1, 4):
        if args.only and args.only != f"B{batch}":
            continue
        g = torch.Generator(device=dev).manual_seed(batch)
        image = torch.randn(batch, 3, 256, 256, device=dev, generator=g)
        assert m._runs_hip(image)

        def run_torch():
            os.environ["E3DGE_ENCODER"] = "torch"
            try:
                return m(image, return_featmap=True)
            finally:
                del os.environ["E3DGE_ENCODER"]

        run_hip = lambda: m(image, return_featmap=True)
        with torch.no_grad():
            if args.split:
                line = dict(case=f"B{batch}_256", split=kernel_split(run_hip))
                print(json.dumps(line), flush=True)
                lines.append(line)
                continue
            a, b = run_hip(), run_torch()
            t_hip, t_ref = alternating_block_ms([run_hip, run_torch], args.steps)
            parts = macs(m, 256)
            fl = 2 * batch * sum(parts.values())
            rel = lambda p, q: float((p - q).abs().max() / q.abs().max())
            line = dict(case=f"B{batch}_256", gflop=fl / 1e9, gmac_per_image={k: round(v / 1e9, 2) for k, v in parts.items()},
                        hip_ms=t_hip[0], hip_ms_min=t_hip[1], hip_ms_max=t_hip[2], torch_ms=t_ref[0], torch_ms_min=t_ref[1], torch_ms_max=t_ref[2],
                        ratio_torch_over_hip=t_ref[0] / t_hip[0], images_per_s=batch / (t_hip[0] * 1e-3),
                        achieved=fl / (t_hip[0] * 1e-3) / PEAK_F32_MATRIX,
                        rel_diff=dict(thumb_out=rel(a['pred_latents'][0], b['pred_latents'][0]), stylegan_out=rel(a['pred_latents'][1], b['pred_latents'][1]),
                                      feat_maps=rel(a['feat_maps'], b['feat_maps']), p32=rel(a['p32'], b['p32'])),
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
