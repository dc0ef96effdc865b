"""Times the training loss's HIP kernels (csrc/losses.hip, e3dge_amd.losses) against the torch operations they replace, on one GPU.

    python tools/time_losses.py                     # needs a GPU; writes profiles/losses_times.json and the resource listing
    python tools/time_losses.py --resources-only    # only profiles/losses_kernel_resources.txt (hipcc, no GPU)

Within one process each leg alternates the two forms block by block: five blocks per form, wall clock between device synchronisations,
the MEDIAN block is the figure and the fastest block stands beside it (bench.py's estimator for its training legs).
    pool_256      AvgPool2d((256, 256)) forward + backward at 1x3x1024^2                       vs torch.nn.AdaptiveAvgPool2d
    shape_terms   the four terms of calc_shape_rec_loss forward + backward at the C5 sizes     vs the torch formulas
                  (eikonal_term (1,64,64,18,3), surface terms (1,64,64,...), 4,096 uniform points)
    stage1_step   bench.py's stage-1 full step (renderer with eikonal terms -> decoder -> 1024^2 -> loss -> backward to the styles) with
                  the loss through LossClass + AvgPool2d                                       vs the same loss as torch operations
                  (both forms use the HIP LPIPS node; identity term off).  Reported, not gated."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PROFILES = os.path.join(REPO, "profiles")


def kernel_resources():
    """Registers, LDS and scratch of every kernel of csrc/losses.hip as the compiler reports them."""
    import e3dge_amd  # noqa: F401
    from e3dge_amd import build
    cmd = [build._hipcc(), *build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, "losses.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"kernel": subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    lines = ["# csrc/losses.hip, " + " ".join(build.FLAGS), f"{'VGPR':>5} {'AGPR':>5} {'SGPR':>5} {'LDS B':>6} {'scratch B':>9} {'waves/SIMD':>10}  kernel"]
    for r in rows:
        lines.append(f"{r.get('VGPRs', 0):>5} {r.get('AGPRs', 0):>5} {r.get('TotalSGPRs', 0):>5} {r.get('LDS Size', 0):>6} {r.get('ScratchSize', 0):>9} "
                     f"{r.get('Occupancy', 0):>10}  {r['kernel'].split('(')[0]}")
    assert rows and all(r.get("ScratchSize", 0) == 0 for r in rows), "a kernel of losses.hip uses scratch"
    os.makedirs(PROFILES, exist_ok=True)
    path = os.path.join(PROFILES, "losses_kernel_resources.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--steps", type=int, default=100, help="steps per block of the two small legs")
    args = ap.parse_args()
    if args.resources_only:
        print(kernel_resources())
        return
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_losses.py needs a GPU")
    import e3dge_amd  # noqa: F401
    from e3dge_amd import losses, synthetic as syn
    from e3dge_amd.camera_utils import generate_camera_params
    from e3dge_amd.lpips import LPIPS
    from e3dge_amd.stylesdf_model import G_pred_latents
    dev = "cuda:0"

    def block_ms(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    def leg(hip, ref, steps, warm=10, blocks=5):
        for _ in range(warm):
            hip()
            ref()
        v = {"hip": [], "torch": []}
        for _ in range(blocks):                       # alternate: both forms see the same clocks
            v["hip"].append(block_ms(hip, steps))
            v["torch"].append(block_ms(ref, steps))
        out = {}
        for k, t in v.items():
            t = sorted(t)
            out[k] = {"median_ms": statistics.median(t), "min_ms": t[0], "max_ms": t[-1], "blocks": blocks, "steps_per_block": steps}
        out["torch_over_hip"] = out["torch"]["median_ms"] / out["hip"]["median_ms"]
        # the gate of the issue: faster by more than the spread of the five blocks of either form
        out["hip_faster_beyond_spread"] = bool(out["hip"]["max_ms"] < out["torch"]["min_ms"])
        return out

    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__}

    # (a) pool_256 forward + backward
    x = r(1, 3, 1024, 1024).requires_grad_(True)
    up = r(1, 3, 256, 256)
    pool_hip, pool_ref = losses.AvgPool2d((256, 256)), torch.nn.AdaptiveAvgPool2d((256, 256))
    assert pool_hip.factor(x) == 4

    def run_pool(pool):
        x.grad = None
        pool(x).backward(up)
    result["pool_256"] = leg(lambda: run_pool(pool_hip), lambda: run_pool(pool_ref), args.steps)
    result["pool_256"]["bytes_moved"] = 2 * (x.numel() + up.numel()) * 4

    # (b) the four shape terms forward + backward at the C5 sizes
    opt = types.SimpleNamespace(l2_lambda=1.0, vgg_lambda=0.8, id_lambda=0.0, uniform_pts_sdf_lambda=1.0, surf_sdf_lambda=0.1,
                                surf_normal_lambda=0.05, eikonal_lambda=0.1)
    lpips = syn.load_synthetic_lpips(LPIPS(differentiable=True)).to(dev)
    lc = losses.LossClass(dev, opt, lpips=lpips, id_loss=object())
    pred = dict(uniform_points_sdf=(1.5 * r(1, 4096, 1)).requires_grad_(True), surface_sdf=r(1, 64, 64, 1).requires_grad_(True),
                surface_eikonal_term=r(1, 64, 64, 1, 3).requires_grad_(True), eikonal_term=r(1, 64, 64, 18, 3).requires_grad_(True))
    gt = dict(uniform_points_sdf=r(1, 4096, 1), surface_eikonal_term=F.normalize(r(1, 64, 64, 1, 3), dim=-1))
    flags = dict(supervise_sdf=True, supervise_surface=True, supervise_surface_normal=True, supervise_eikonal=True)

    def shape_torch(p, gt_):
        t = F.smooth_l1_loss(p['uniform_points_sdf'].squeeze(), gt_['uniform_points_sdf'].squeeze()) * opt.uniform_pts_sdf_lambda
        t = t + F.smooth_l1_loss(p['surface_sdf'], torch.zeros_like(p['surface_sdf'])) * opt.surf_sdf_lambda
        t = t + F.smooth_l1_loss(p['surface_eikonal_term'].squeeze(), gt_['surface_eikonal_term'].squeeze()) * opt.surf_normal_lambda
        return t + ((p['eikonal_term'].norm(dim=-1) - 1) ** 2).mean() * opt.eikonal_lambda

    def run_shape(hip):
        for v in pred.values():
            v.grad = None
        (lc.calc_shape_rec_loss(pred, gt, dev, **flags)[0] if hip else shape_torch(pred, gt)).backward()
    run_shape(True)
    a, b = float(lc.calc_shape_rec_loss(pred, gt, dev, **flags)[0].detach()), float(shape_torch(pred, gt).detach())
    assert abs(a - b) <= 1e-5 * abs(a), (a, b)
    result["shape_terms"] = leg(lambda: run_shape(True), lambda: run_shape(False), args.steps)

    # (c) the stage-1 full step of bench.py (train_step_full) with the loss written both ways
    S5, RES = 18, 64
    g5 = G_pred_latents(syn.model_opt(), syn.rendering_opt(N_samples=S5), full_pipeline=True)
    syn.load_synthetic(g5)
    g5 = g5.to(dev).eval()
    g5.requires_grad_(False)
    w5, d5 = syn.synthetic_inputs(1, seed=1, device=dev)
    p5, f5, n5, fa5, _ = generate_camera_params(RES, dev, locations=torch.zeros(1, 2, device=dev))
    gt_img = torch.tanh(r(1, 3, 256, 256))
    gt_normal = F.normalize(r(1, RES, RES, 1, 3), dim=-1)
    step_flags = dict(supervise_sdf=False, supervise_surface=False, supervise_surface_normal=True, supervise_eikonal=True)
    mse = torch.nn.MSELoss()
    values = {}

    def step(hip):
        s_ = w5.clone().requires_grad_(True)
        o = g5([s_, d5], p5, f5, n5, fa5, input_is_latent=True, randomize_noise=False, return_eikonal=True, return_surface_eikonal=True)
        if hip:
            loss = lc.calc_2d_rec_loss(pool_hip(o['gen_imgs']), gt_img, None, None)[0]
            loss = loss + lc.calc_shape_rec_loss(o, dict(surface_eikonal_term=gt_normal), dev, **step_flags)[0]
        else:
            img = pool_ref(o['gen_imgs'])
            loss = mse(img, gt_img) * opt.l2_lambda + lpips(img, gt_img) * opt.vgg_lambda
            loss = loss + F.smooth_l1_loss(o['surface_eikonal_term'].squeeze(), gt_normal.squeeze()) * opt.surf_normal_lambda
            loss = loss + ((o['eikonal_term'].norm(dim=-1) - 1) ** 2).mean() * opt.eikonal_lambda
        loss.backward()
        values[hip] = (loss.detach(), s_.grad)
    step(True)
    step(False)
    torch.cuda.synchronize()
    rel = float((values[True][1] - values[False][1]).abs().max() / values[False][1].abs().max())
    result["stage1_step"] = leg(lambda: step(True), lambda: step(False), 3, warm=3)
    result["stage1_step"]["loss_hip"], result["stage1_step"]["loss_torch"] = float(values[True][0]), float(values[False][0])
    result["stage1_step"]["styles_grad_rel_diff"] = rel
    result["stage1_step"]["note"] = "reported, not gated; both forms run the HIP LPIPS node, identity term off"

    os.makedirs(PROFILES, exist_ok=True)
    with open(os.path.join(PROFILES, "losses_times.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    print(kernel_resources())


if __name__ == "__main__":
    main()
