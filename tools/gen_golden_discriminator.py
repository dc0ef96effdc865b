"""Fixture for the discriminator (tests/test_discriminator_host.py, tests/test_gpu_discriminator.py).  Authoring time only, CPU only; the
tests never run this.

    python tools/gen_golden_discriminator.py

Imports the reference's Discriminator (project/models/stylesdf_model.py) and its GAN losses (project/losses/gan_loss.py), loads the
synthetic weights of e3dge_amd.synthetic.load_synthetic_discriminator (both variants) and writes, under tests/golden/:
    discriminator_state_dict_keys.json   sorted keys and shapes of the reference's state dict for (D_init_size 256, cm 2) and (16, cm 1)
    discriminator.npz                    for every case of test_discriminator_host.CASES and both weight variants, on the images of
                                         test_discriminator_host.golden_images (a formula: no image and no weight is stored): the logits,
                                         per tap (every ResBlock output, the stddev scalars, final_conv's output) 256 sampled values (at
                                         test_idloss_host.tap_samples) and the float64 sum, g_nonsaturating_loss, d_logistic_loss(flipped
                                         logits, logits), and the reference autograd's gradient of g_nonsaturating_loss to the input, sampled
                                         the same way, with its float64 sum
    discriminator_report.json            torch version, thread count, file sizes; per case the float32 run's distance from a float64 run of
                                         the same modules (per tap, logits, gradient: max |f32 - f64| / max |f64|), how many lrelu
                                         pre-activations of the float64 run lie within 1e-5 and 1e-4 of zero, how many lrelu branches the
                                         float32 run takes differently and the largest |pre64| among those"""
import importlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
GOLD = os.path.join(REPO, "tests", "golden")

import oracle.cpu_numerics  # noqa: E402,F401  (before any arithmetic)
import e3dge_amd  # noqa: E402,F401
from e3dge_amd import synthetic as syn  # noqa: E402
from e3dge_amd.discriminator import Discriminator, TAP_FINAL, TAP_STDDEV  # noqa: E402
import test_discriminator_host as host  # noqa: E402
from test_idloss_host import tap_samples  # noqa: E402

SQRT2 = 2 ** 0.5


def reference_modules():
    from oracle import ref_harness, golden_store
    ref_harness.prepare()
    return (importlib.import_module("project.models.stylesdf_model"), importlib.import_module("project.losses.gan_loss"),
            importlib.import_module("project.models.op.fused_act"), golden_store)


def reference_discriminator(sm, init, cm, variant, dtype=torch.float32):
    opt = syn.discriminator_opt(init, cm)
    ref = sm.Discriminator(opt)
    ours = syn.load_synthetic_discriminator(Discriminator(opt), variant=variant)
    ref.load_state_dict(ours.state_dict(), strict=True)
    return ref.to(dtype)


def run(ref, gan, fused_act, x):
    """One forward and backward of the reference module: dict(logits, taps {index: tensor}, g_loss, d_loss, grad, acts: every lrelu
    output in network order)."""
    taps, acts, hooks = {}, [], []
    blocks = list(ref.convs)[1:]
    for i, b in enumerate(blocks):
        hooks.append(b.register_forward_hook(lambda m, inp, out, i=i: taps.__setitem__(i, out.detach())))
    hooks.append(ref.final_conv.register_forward_hook(lambda m, inp, out: taps.__setitem__(TAP_FINAL, out.detach())))
    hooks.append(ref.final_conv.register_forward_pre_hook(
        lambda m, inp: taps.__setitem__(TAP_STDDEV, inp[0].detach()[:inp[0].shape[0] // host.disc.stddev_group(inp[0].shape[0]), -1, 0, 0].clone())))
    for m in ref.modules():
        if isinstance(m, fused_act.FusedLeakyReLU):
            hooks.append(m.register_forward_hook(lambda m, inp, out: acts.append(out.detach())))
    hooks.append(ref.final_linear[0].register_forward_hook(lambda m, inp, out: acts.append(out.detach())))
    leaf = x.clone().requires_grad_(True)
    logits = ref(leaf)
    g_loss = gan.g_nonsaturating_loss(logits)
    d_loss = gan.d_logistic_loss(logits.detach().flip(0), logits.detach())
    g_loss.backward()
    for h in hooks:
        h.remove()
    return dict(logits=logits.detach(), taps=taps, g_loss=g_loss.detach(), d_loss=d_loss, grad=leaf.grad, acts=acts)


def rel(a, b):
    top = float(b.abs().max())
    return float((a.double() - b).abs().max()) / top if top > 0 else 0.0


def main():
    sm, gan, fused_act, golden_store = reference_modules()
    keys = {}
    for name, (init, cm) in {"256x2": (256, 2), "16x1": (16, 1)}.items():
        sd = sm.Discriminator(syn.discriminator_opt(init, cm)).state_dict()
        keys[name] = dict(keys=sorted(sd), shapes={k: list(v.shape) for k, v in sd.items()})
    with open(os.path.join(GOLD, "discriminator_state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    arrays, cases = {}, {}
    for variant in host.VARIANTS:
        for case in host.CASES:
            init, cm, B, size = case
            x = host.golden_images(B, size)
            r32 = run(reference_discriminator(sm, init, cm, variant), gan, fused_act, x)
            r64 = run(reference_discriminator(sm, init, cm, variant, torch.float64), gan, fused_act, x.double())
            key = host.case_id(case, variant) + "/"
            arrays[key + "logits"] = r32["logits"].numpy()
            for t, v in r32["taps"].items():
                arrays[key + "tap_" + host.tap_name(t)] = v.reshape(-1)[tap_samples(v.numel())].numpy()
                arrays[key + "sum_" + host.tap_name(t)] = np.float64(v.double().sum().item())
            arrays[key + "g_nonsaturating_loss"] = r32["g_loss"].numpy()
            arrays[key + "d_logistic_loss"] = r32["d_loss"].numpy()
            arrays[key + "grad"] = r32["grad"].reshape(-1)[tap_samples(r32["grad"].numel())].numpy()
            arrays[key + "grad_sum"] = np.float64(r32["grad"].double().sum().item())
            near5 = near4 = flips = total = 0
            worst = 0.0
            for a32, a64 in zip(r32["acts"], r64["acts"]):
                pre64 = torch.where(a64 > 0, a64 / SQRT2, a64 / (0.2 * SQRT2)).abs()
                near5 += int((pre64 < 1e-5).sum())
                near4 += int((pre64 < 1e-4).sum())
                diff = (a32 > 0) != (a64 > 0)
                flips += int(diff.sum())
                if diff.any():
                    worst = max(worst, float(pre64[diff].max()))
                total += a64.numel()
            cases[key[:-1]] = dict(logits=rel(r32["logits"], r64["logits"]), grad=rel(r32["grad"], r64["grad"]),
                                   taps={host.tap_name(t): rel(v, r64["taps"][t]) for t, v in r32["taps"].items()},
                                   lrelu_inputs=total, near_1e5=near5, near_1e4=near4, f32_flips=flips, f32_worst_flip=worst,
                                   max_logit=float(r64["logits"].abs().max()), max_grad=float(r64["grad"].abs().max()))
            print(key, cases[key[:-1]], flush=True)
    path = golden_store.save(GOLD, "discriminator", arrays)
    report = dict(torch=torch.__version__, threads=torch.get_num_threads(), npz_bytes=os.path.getsize(path),
                  keys_bytes=os.path.getsize(os.path.join(GOLD, "discriminator_state_dict_keys.json")), cases=cases)
    with open(os.path.join(GOLD, "discriminator_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(dict(npz_bytes=report["npz_bytes"], keys_bytes=report["keys_bytes"]))


if __name__ == "__main__":
    main()
