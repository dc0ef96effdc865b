"""LPIPS-alex on the HIP kernels (csrc/lpips.hip, e3dge_amd.lpips.LPIPS) against a plain-torch restatement of the reference's
forward (project/losses/lpips/lpips.py:33-39, networks.py:52-65, 80-89, utils.py:6-9) on the CPU: once in float64 (truth), once in
float32 (the reference's own arithmetic, the yardstick of DESIGN section 2).

Bounds:  every normalised tap   max|hip - f64| <= max(2e-6, 3 max|f32 - f64|)        (2e-6: the project's custom-op bound)
         per-layer and total    relative error <= max(2e-5, 3 x the float32 restatement's)   (2e-5: tests/test_gpu_metrics.py's)"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import record

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, graphs, sharded_eval, synthetic as syn
from e3dge_amd.lpips import LPIPS, CONV_SLOTS, CONVS

SHAPES = [(1, 3, 31, 31), (2, 3, 67, 67), (3, 3, 95, 71), (2, 3, 256, 256)]


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------
def restate(sd, x, y, dtype):
    """dict(taps: five (2B, C, H, W) normalised features of cat(x, y), active: fraction of positive pre-normalisation tap values,
    per_layer (B, 5), per_image (B,), total ()) in `dtype` on the device of x."""
    g = lambda k: sd[k].to(device=x.device, dtype=dtype)
    z = torch.cat([x, y]).to(dtype)
    B = x.shape[0]
    z = (z - g('net.mean')) / g('net.std')
    taps, active = [], []
    for i in range(11):
        if i in CONVS:
            _, _, _, s, p = CONVS[i]
            z = F.relu(F.conv2d(z, g(f'net.layers.{i}.weight'), g(f'net.layers.{i}.bias'), stride=s, padding=p))
            active.append(float((z > 0).double().mean()))
            taps.append(z / (torch.sqrt(torch.sum(z ** 2, dim=1, keepdim=True) + 1e-8) + 1e-10))
        elif i in (2, 5):
            z = F.max_pool2d(z, 3, 2)
    per_layer = torch.stack([F.conv2d((t[:B] - t[B:]) ** 2, g(f'lin.{l}.1.weight')).mean((1, 2, 3)) for l, t in enumerate(taps)], 1)
    return dict(taps=taps, active=active, per_layer=per_layer, per_image=per_layer.sum(1), total=per_layer.sum() / B)


def make_pair(shape, seed):
    """gt = tanh(5x5 box-filtered 3 N(0,1)), pred = tanh(1.2 gt + 0.5 N(0,1))."""
    rs = np.random.RandomState(seed)
    n = torch.from_numpy(rs.standard_normal(shape)).float()
    gt = torch.tanh(F.avg_pool2d(F.pad(3.0 * n, [2] * 4, mode='replicate'), 5, 1))
    pred = torch.tanh(1.2 * gt + 0.5 * torch.from_numpy(rs.standard_normal(shape)).float())
    return pred.contiguous(), gt.contiguous()


@functools.lru_cache(maxsize=None)
def module_cpu():
    return syn.load_synthetic_lpips(LPIPS())


@functools.lru_cache(maxsize=None)
def case(shape):
    """(pred, gt, float64 truth, float32 yardstick) on the CPU, computed once per shape and shared; never modified."""
    pred, gt = make_pair(shape, seed=sum(shape))
    sd = module_cpu().state_dict()
    return pred, gt, restate(sd, pred, gt, torch.float64), restate(sd, pred, gt, torch.float32)


def check_network_is_alive(truth):
    """Conditions on the CPU truth without which a dead network would pass for free."""
    for l, a in enumerate(truth['active']):
        assert 0.2 <= a <= 0.8, f"tap {l + 1}: {a:.2f} of the ReLUs active"
    d = truth['per_layer'].sum(0)
    assert float(truth['per_layer'].min()) > 0
    assert float(d.min()) >= 0.01 * float(d.max()), d.tolist()


@functools.lru_cache(maxsize=None)
def module_gpu():
    return syn.load_synthetic_lpips(LPIPS()).to("cuda:0")


def rel(a, b):
    return float(((a.double().cpu() - b.double()).abs() / b.double().abs()).max())


# ---- parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_taps_layers_images_and_scalar_match_the_restatement(shape):
    pred, gt, truth, f32 = case(shape)
    check_network_is_alive(truth)
    m = module_gpu()
    out = m.run(pred.cuda(), gt.cuda(), per_layer=True, taps=True)
    scalar = m(pred.cuda(), gt.cuda())
    torch.cuda.synchronize()
    rec = {}
    for l in range(5):
        assert out['taps'][l].shape == truth['taps'][l].shape
        rec[f'tap{l + 1}_err'] = float((out['taps'][l].double().cpu() - truth['taps'][l]).abs().max())
        rec[f'tap{l + 1}_f32'] = float((f32['taps'][l].double() - truth['taps'][l]).abs().max())
        rec[f'layer{l + 1}_rel'] = rel(out['per_layer'][:, l], truth['per_layer'][:, l])
        rec[f'layer{l + 1}_f32'] = rel(f32['per_layer'][:, l], truth['per_layer'][:, l])
    rec['image_rel'], rec['image_f32'] = rel(out['per_image'], truth['per_image']), rel(f32['per_image'], truth['per_image'])
    rec['total_rel'], rec['total_f32'] = rel(scalar.reshape(1), truth['total'].reshape(1)), rel(f32['total'].reshape(1), truth['total'].reshape(1))
    record("lpips_parity", shape=list(shape), **rec)
    print(shape, {k: f"{v:.2e}" for k, v in rec.items()})
    for l in range(5):
        assert rec[f'tap{l + 1}_err'] <= max(2e-6, 3 * rec[f'tap{l + 1}_f32']), (l, rec)
        assert rec[f'layer{l + 1}_rel'] <= max(2e-5, 3 * rec[f'layer{l + 1}_f32']), (l, rec)
    assert rec['image_rel'] <= max(2e-5, 3 * rec['image_f32']), rec
    assert rec['total_rel'] <= max(2e-5, 3 * rec['total_f32']), rec
    assert scalar.shape == () and torch.equal(out['mean'], scalar)


# ---- exact properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_identity_symmetry_repeatability_and_batch_independence():
    pred, gt, truth, _ = case((3, 3, 95, 71))
    check_network_is_alive(truth)
    m = module_gpu()
    p, g = pred.cuda(), gt.cuda()
    assert float(m(p, p)) == 0.0 and (m(g, g, per_image=True) == 0).all()
    a, b = m.run(p, g, per_layer=True), m.run(g, p, per_layer=True)
    assert float(a['mean']) > 0
    for k in ('per_image', 'mean', 'per_layer'):
        assert torch.equal(a[k], b[k]), k                                            # LPIPS(x, y) == LPIPS(y, x)
    again = m.run(p, g, per_layer=True)
    for k in ('per_image', 'mean', 'per_layer'):
        assert torch.equal(a[k], again[k]), k                                        # two calls
    singles = torch.cat([m(p[i:i + 1], g[i:i + 1], per_image=True) for i in range(3)])
    assert torch.equal(singles, a['per_image'])                                      # a pair's value does not depend on its batch


@pytest.mark.gpu
def test_the_weight_image_follows_the_parameters():
    pred, gt, _, _ = case((1, 3, 67, 67))
    m = syn.load_synthetic_lpips(LPIPS()).to("cuda:0")
    p, g = pred.cuda(), gt.cuda()
    base = float(m(p, g))
    with torch.no_grad():
        m.lin[2][1].weight[0, 5, 0, 0] += 0.5                                        # in place: the version counter moves
    after_lin = float(m(p, g))
    assert after_lin != base
    with torch.no_grad():
        m.net.layers[CONV_SLOTS[1]].weight[3, 2, 1, 1] += 0.25
    after_conv = float(m(p, g))
    assert after_conv != after_lin
    m.net.layers[0].bias.data[7] += 0.5                                              # through .data: no version bump ...
    assert float(m(p, g)) == after_conv
    _lib.invalidate(m)                                                               # ... so the cache has to be told
    assert float(m(p, g)) != after_conv


# ---- the metric row --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 3, 67, 67), (3, 3, 95, 71)], ids=["b1", "b3"])
def test_image_metrics_fills_the_lpips_column_and_leaves_the_others(shape):
    pred, gt, truth, _ = case(shape)
    check_network_is_alive(truth)
    m = module_gpu()
    p, g = pred.cuda(), gt.cuda()
    plain = sharded_eval.image_metrics(p, g)
    row = sharded_eval.image_metrics(p, g, lpips=m, vgg_lambda=0.8)
    lp = m(p, g)
    assert float(plain[2]) == 0.0 and float(plain[3]) == float(plain[0])             # today's row: column 2 is 0, loss = MSE
    assert torch.equal(row[2], lp) and float(lp) > 0
    for c in (0, 1, 4, 5, 6, 7):
        assert torch.equal(row[c], plain[c]), c
    want = np.float32(np.float32(row[0].item()) + np.float32(np.float32(0.8) * np.float32(lp.item())))
    assert abs(np.float32(row[3].item()) - want) <= np.spacing(want)
    assert torch.equal(sharded_eval.image_metrics(p, g, l2_lambda=1.0, lpips=None, vgg_lambda=0.0), plain)


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_replay_equals_eager():
    pred, gt = make_pair((1, 3, 67, 67), seed=5)
    m = module_gpu()
    p, g = pred.cuda(), gt.cuda()
    eager = m.run(p, g)
    eager = (eager['per_image'].clone(), eager['mean'].clone())

    def fn(a, b):
        out = m.run(a, b)
        return out['per_image'], out['mean']

    call = graphs.GraphedCall(fn, torch.zeros_like(p), torch.ones_like(g) * 0.5)
    replay = [t.clone() for t in call(p, g)]
    torch.cuda.synchronize()
    assert float(eager[0]) > 0 and torch.equal(replay[0], eager[0]) and torch.equal(replay[1], eager[1])
