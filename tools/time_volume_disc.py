#!/usr/bin/env python3
"""Time of the camera-pose predictor (e3dge_amd.volume_discriminator.VolumeRenderDiscriminator, csrc/volume_disc.hip) against the torch
composition of the same module (AddCoords copies, library convolutions through MIOpen, pooling and merge as separate ops;
E3DGE_VOLUME_DISC=torch's path), in the same process on the same GPU.

    python tools/time_volume_disc.py [--out profiles/volume_disc_times.json] [--steps 10] [--only B4]
    python tools/time_volume_disc.py --split [--out profiles/volume_disc_split.json]      (a run of its own: nothing is timed in it)

Cases: forward(x) of a (B, 3, 64, 64) input, B = 1, 4 and 8, under no_grad.  Estimator: warm-up of both paths, then five blocks of `steps`
calls per path between two HIP events, the two paths' blocks ALTERNATING so that a drift of the clocks meets both; the median block per
call, with the fastest and slowest beside it.  `--split`: the device time of one HIP call per launch, in launch order (torch profiler),
from a process that times nothing else.  `achieved` is the fraction of the fp32 matrix peak (157.3 TFLOP/s) the HIP path reaches on the
convolutions' 2 x MAC count from the layer table (the two coordinate channels counted); at one image that peak would take about 0.09 ms.
What bounds the kernels is not established here: no counters are taken.  One JSON line per case."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import e3dge_amd  # noqa: E402,F401
from e3dge_amd import synthetic as syn  # noqa: E402
from e3dge_amd.volume_discriminator import CHANNELS, VolumeRenderDiscriminator  # noqa: E402
from time_aligner import launch_split  # noqa: E402
from time_encoder import PEAK_F32_MATRIX, alternating_block_ms  # noqa: E402

SIZE = 64


def macs(size=SIZE):
    """MACs of one image per launch, in launch order: {name: MACs}."""
    out, cin, res = {"stem": 3 * CHANNELS[size] * size * size}, CHANNELS[size], size
    b = 0
    while res > 2:
        cout = CHANNELS[res // 2]
        if cin != cout:
            out[f"block{b}.skip"] = cin * cout * (res // 2) ** 2
        out[f"block{b}.conv1"] = 9 * (cin + 2) * cout * res * res
        out[f"block{b}.conv2"] = 9 * (cout + 2) * cout * res * res
        cin, res, b = cout, res // 2, b + 1
    out["final"] = 4 * cin * 3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--split", action="store_true", help="only the per-launch device times of one HIP call")
    ap.add_argument("--only", help="one case, e.g. B4")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    m = syn.load_synthetic_volume_discriminator(VolumeRenderDiscriminator(syn.model_opt(renderer_spatial_output_dim=SIZE)), variant='wide').to(dev).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    lines = []
    for batch in (1, 4, 8):
        if args.only and args.only != f"B{batch}":
            continue
        g = torch.Generator(device=dev).manual_seed(batch)
        x = torch.tanh(torch.randn(batch, 3, SIZE, SIZE, device=dev, generator=g))
        assert m.uses_hip(x)

        def run_torch():
            os.environ["E3DGE_VOLUME_DISC"] = "torch"
            try:
                return m(x)
            finally:
                del os.environ["E3DGE_VOLUME_DISC"]

        run_hip = lambda: m(x)
        with torch.no_grad():
            if args.split:
                per_launch = launch_split(run_hip)
                by_name = {}
                for name, ms in per_launch:
                    n, total = by_name.get(name, (0, 0.0))
                    by_name[name] = (n + 1, round(total + ms, 4))
                line = dict(case=f"B{batch}_{SIZE}", launches=len(per_launch), by_kernel=by_name, per_launch=per_launch,
                            gmac_per_launch={k: round(batch * v / 1e9, 4) for k, v in macs().items()})
                print(json.dumps(line), flush=True)
                lines.append(line)
                continue
            a, b = run_hip(), run_torch()
            t_hip, t_ref = alternating_block_ms([run_hip, run_torch], args.steps)
            parts = macs()
            fl = 2 * batch * sum(parts.values())
            line = dict(case=f"B{batch}_{SIZE}", gflop=fl / 1e9, gmac_per_image=round(sum(parts.values()) / 1e9, 3),
                        hip_ms=t_hip[0], hip_ms_min=t_hip[1], hip_ms_max=t_hip[2], torch_ms=t_ref[0], torch_ms_min=t_ref[1], torch_ms_max=t_ref[2],
                        ratio_torch_over_hip=t_ref[0] / t_hip[0], images_per_s=batch / (t_hip[0] * 1e-3),
                        achieved=fl / (t_hip[0] * 1e-3) / PEAK_F32_MATRIX, matrix_peak_floor_ms=fl / PEAK_F32_MATRIX * 1e3,
                        rel_diff=float((a[1] - b[1]).abs().max() / b[1].abs().max()), bound="not established (no counters taken)",
                        estimator=f"median of 5 blocks of {args.steps} calls per path, the paths' blocks alternating, HIP events")
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
