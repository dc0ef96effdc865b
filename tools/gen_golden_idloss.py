"""Fixture for the identity term (tests/test_idloss_host.py, tests/test_gpu_idloss.py).  Authoring time only, CPU only; the tests never
run this.

    python tools/gen_golden_idloss.py

Imports the reference's Backbone (project/models/encoders/model_irse.py) and IDLoss (project/losses/id_loss.py; the object is built
around the Backbone without running its constructor, which reads a checkpoint file), loads the synthetic weights of
e3dge_amd.synthetic.load_synthetic_idloss and writes, under tests/golden/:
    idloss_state_dict_keys.json   the sorted keys of the reference IDLoss's state dict
    idloss_ir_se50.npz            for the images of test_idloss_host.golden_images (a formula: no image and no weight is stored): the
                                  (3, 512) embeddings of the three 256^2 targets, the head output before the normalisation, the dots / loss /
                                  sim_improvement of IDLoss.forward(pred, gt, gt), the same for one 1024^2 pair through id_loss_pool
                                  (builder.py:157-166), and per tap 256 sampled values (at test_idloss_host.tap_samples) and its float64 sum
    idloss_report.json            torch version, thread count, file sizes"""
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
from e3dge_amd.id_loss import IDLoss, TAP_NAMES, TAP_UNITS  # noqa: E402
import test_idloss_host as host  # noqa: E402


def reference_idloss():
    """The reference's IDLoss around its Backbone(112, 50, 'ir_se', drop_ratio=0.6), weights from our synthetic state dict."""
    from oracle import ref_harness, golden_store
    ref_harness.prepare()
    irse = importlib.import_module("project.models.encoders.model_irse")
    ref_mod = importlib.import_module("project.losses.id_loss")
    obj = ref_mod.IDLoss.__new__(ref_mod.IDLoss)
    torch.nn.Module.__init__(obj)
    obj.facenet = irse.Backbone(input_size=112, num_layers=50, drop_ratio=0.6, mode='ir_se')
    obj.face_pool = torch.nn.AdaptiveAvgPool2d((112, 112))
    obj.facenet.eval()
    ours = syn.load_synthetic_idloss(IDLoss())
    obj.load_state_dict(ours.state_dict(), strict=True)
    return obj, golden_store


def record_taps(ref, images):
    """The eight taps of the reference Backbone for the cropped and pooled `images`."""
    taps, hooks = [], []
    net = ref.facenet
    hooks.append(net.register_forward_pre_hook(lambda m, inp: taps.append(inp[0])))
    grab = lambda m, inp, out: taps.append(out)
    hooks.append(net.input_layer.register_forward_hook(grab))
    for u in TAP_UNITS:
        hooks.append(net.body[u].register_forward_hook(grab))
    hooks.append(net.output_layer.register_forward_hook(grab))
    emb = ref.extract_feats(images)
    for h in hooks:
        h.remove()
    assert len(taps) == len(TAP_NAMES)
    return emb, taps


def main():
    ref, golden_store = reference_idloss()
    keys = sorted(ref.state_dict().keys())
    with open(os.path.join(GOLD, "idloss_state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    arrays = {}
    with torch.no_grad():
        pred, gt = host.golden_images(3, 256)
        emb, taps = record_taps(ref, gt)
        arrays["embeddings"] = emb.numpy()
        arrays["head"] = taps[-1].numpy()
        for name, t in zip(TAP_NAMES, taps):
            arrays["tap_" + name] = t.reshape(-1)[host.tap_samples(t.numel())].numpy()
            arrays["sum_" + name] = np.float64(t.double().sum().item())
        loss, sim, logs = ref(pred, gt, gt)
        arrays["dots"] = np.array([[d["diff_target"], d["diff_input"], d["diff_views"]] for d in logs], dtype=np.float64)
        arrays["loss"], arrays["sim_improvement"] = loss.numpy(), np.float64(sim)
        pool = torch.nn.AdaptiveAvgPool2d((256, 256))                   # builder.py:27
        pred4, gt4 = host.golden_images(1, 1024)
        p4, g4 = pool(pred4), pool(gt4)                                 # builder.py:157-160
        loss4, sim4, logs4 = ref(p4, g4, g4)
        arrays["emb_1024"] = torch.cat([ref.extract_feats(p4), ref.extract_feats(g4)]).numpy()
        arrays["dots_1024"] = np.array([[d["diff_target"], d["diff_input"], d["diff_views"]] for d in logs4], dtype=np.float64)
        arrays["loss_1024"] = loss4.numpy()
    path = golden_store.save(GOLD, "idloss_ir_se50", arrays)
    report = dict(torch=torch.__version__, threads=torch.get_num_threads(), npz_bytes=os.path.getsize(path), keys=len(keys))
    with open(os.path.join(GOLD, "idloss_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(report)


if __name__ == "__main__":
    main()
