"""The identity term on the HIP kernels (csrc/idnet.hip, e3dge_amd.id_loss.IDLoss) against the module's own torch layers on the CPU --
which reproduce the recording of the reference bit for bit (tests/test_idloss_host.py) --: once in float64 (truth), once in float32 (the
reference's own arithmetic, the yardstick of DESIGN section 2).

Bounds:  a convolution, a tap, the embeddings   max|hip - f64| <= max(2e-6 max|f64|, 3 max|f32 - f64|)   (2e-6: the custom-op bound;
                                                 3: SURVEY 8c)
         loss and the three dots                |hip - f64| <= max(2e-6, 3 |f32 - f64|)"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, record

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, graphs, sharded_eval, synthetic as syn
from e3dge_amd.id_loss import IDLoss, TAP_NAMES
from test_idloss_host import alive_stats, golden_images, module_cpu


@functools.lru_cache(maxsize=None)
def module_f64():
    return syn.load_synthetic_idloss(IDLoss()).double()


@functools.lru_cache(maxsize=None)
def module_gpu():
    return syn.load_synthetic_idloss(IDLoss()).to("cuda:0")


def dist(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


# ---- one convolution at a time ----------------------------------------------------------------------------------------------------
CONV_CASES = [  # n, Cin, Cout, H, W, kernel, stride, input affine, epilogue affine, PReLU, plane sums
    (2, 3, 64, 9, 11, 3, 1, False, True, True, False),
    (3, 64, 64, 13, 13, 3, 2, True, True, False, True),
    (1, 64, 128, 8, 8, 1, 2, False, True, False, False),
    (2, 128, 128, 7, 7, 3, 1, True, False, True, False),
    (1, 256, 512, 14, 14, 3, 1, False, False, False, False),
]


@functools.lru_cache(maxsize=None)
def conv_case(i):
    n, ci, co, H, W, k, s, in_aff, epi_aff, prelu, _ = CONV_CASES[i]
    rs = np.random.RandomState(100 + i)
    t = lambda *shape, scale=1.0, shift=0.0: torch.from_numpy(shift + scale * rs.standard_normal(shape)).float()
    d = dict(x=t(n, ci, H, W), w=t(co, ci, k, k, scale=(2.0 / (ci * k * k)) ** 0.5))
    d['in_ab'] = torch.stack([t(ci, scale=0.2, shift=1.0), t(ci, scale=0.5, shift=0.3)], 1).contiguous() if in_aff else None     # b != 0
    d['epi_ab'] = torch.stack([t(co, scale=0.2, shift=1.0), t(co, scale=0.5)], 1).contiguous() if epi_aff else None
    d['slope'] = t(co, scale=0.05, shift=0.25) if prelu else None

    def ref(dtype):
        x = d['x'].to(dtype)
        if in_aff:
            x = d['in_ab'][:, 0].to(dtype)[None, :, None, None] * x + d['in_ab'][:, 1].to(dtype)[None, :, None, None]
        y = F.conv2d(x, d['w'].to(dtype), stride=s, padding=k // 2)
        if epi_aff:
            y = d['epi_ab'][:, 0].to(dtype)[None, :, None, None] * y + d['epi_ab'][:, 1].to(dtype)[None, :, None, None]
        if prelu:
            y = F.prelu(y, d['slope'].to(dtype))
        return y
    d['f64'], d['f32'] = ref(torch.float64), ref(torch.float32)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CONV_CASES)), ids=lambda i: "x".join(map(str, CONV_CASES[i][:7])))
def test_one_convolution_matches_float64(i):
    n, ci, co, H, W, k, s, in_aff, epi_aff, prelu, plane = CONV_CASES[i]
    d = conv_case(i)
    lib = _lib.load()
    g = lambda t: None if t is None else t.cuda()
    x, w = g(d['x']), g(d['w'])
    out = torch.full(d['f64'].shape, float('nan'), device="cuda:0")
    wfrag = torch.empty(co * ((ci * k * k + 31) // 32 * 32), device="cuda:0")
    tiles = lib.e3dge_idnet_conv_tiles(co, H, W, k, s)
    assert tiles >= 1
    part = torch.full((n, co, tiles), float('nan'), device="cuda:0") if plane else None
    _lib.launch("e3dge_idnet_conv", out, x, w, wfrag, g(d['in_ab']), g(d['epi_ab']), g(d['slope']), part, n, ci, co, H, W, k, s)
    torch.cuda.synchronize()
    err, f32 = dist(out, d['f64']), dist(d['f32'], d['f64'])
    bound = max(2e-6 * float(d['f64'].abs().max()), 3 * f32)
    rec = dict(err=err, f32=f32, bound=bound)
    border = torch.ones(d['f64'].shape[2:], dtype=torch.bool)
    border[1:-1, 1:-1] = False
    rec['border_err'] = dist(out.cpu()[..., border], d['f64'][..., border])
    if plane:
        sums64, sums32 = d['f64'].sum((2, 3)), d['f32'].sum((2, 3))
        rec['plane_err'], rec['plane_f32'] = dist(part.sum(2), sums64), dist(sums32, sums64)
        rec['plane_bound'] = max(2e-6 * float(sums64.abs().max()), 3 * rec['plane_f32'])
    record("idloss_conv", case=list(CONV_CASES[i][:7]), **rec)
    print(CONV_CASES[i], {k_: f"{v:.2e}" for k_, v in rec.items()})
    assert err <= bound, rec
    assert rec['border_err'] <= bound, rec                                           # a BN folded across the padding fails here
    if plane:
        assert rec['plane_err'] <= rec['plane_bound'], rec


# ---- the whole network ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def net_case(n, size):
    """(pred, gt, float64 and float32 CPU results of run(pred, gt, taps=True)), computed once and shared; never modified."""
    pred, gt = golden_images(n, size)
    with torch.no_grad():
        return pred, gt, module_f64().run(pred.double(), gt.double(), taps=True), module_cpu().run(pred, gt, taps=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n,size", [(1, 256), (3, 256), (1, 1024)], ids=["n1", "n3", "pool1024"])
def test_taps_embeddings_dots_and_loss_match_float64(n, size):
    pred, gt, t64, t32 = net_case(n, size)
    out = module_gpu().run(pred.cuda(), gt.cuda(), taps=True)
    torch.cuda.synchronize()
    rec, ok = {}, True
    for name, h, a, b in list(zip(TAP_NAMES, out['taps'], t64['taps'], t32['taps'])) + [("embeddings", out['embeddings'], t64['embeddings'],
                                                                                         t32['embeddings'])]:
        assert h.shape == a.shape, name
        rec[name + '_err'], rec[name + '_f32'] = dist(h, a), dist(b, a)
        rec[name + '_bound'] = max(2e-6 * float(a.abs().max()), 3 * rec[name + '_f32'])
        ok &= rec[name + '_err'] <= rec[name + '_bound']
    for name in ('dots', 'loss'):
        rec[name + '_err'], rec[name + '_f32'] = dist(out[name], t64[name]), dist(t32[name], t64[name])
        ok &= rec[name + '_err'] <= max(2e-6, 3 * rec[name + '_f32'])
    rec['sim_err'] = dist(out['sim_improvement'], torch.as_tensor(t64['sim_improvement']))
    record("idloss_parity", n=n, size=size, **rec)
    print(n, size, {k: f"{v:.2e}" for k, v in rec.items()})
    assert ok, rec
    assert rec['sim_err'] <= max(4e-6, 6 * rec['dots_f32']), rec                      # a difference of two dots
    if size == 256:                                                                  # not a dead or saturated network (host test's range)
        assert 0.2 <= float(t64['dots'][:, 0].min()) and float(t64['dots'][:, 0].max()) <= 0.98


@pytest.mark.gpu
def test_the_recording_of_the_reference_is_within_the_bounds():
    gold = load_golden("idloss_ir_se50")
    pred, gt, t64, t32 = net_case(3, 256)
    assert alive_stats()['target'] >= alive_stats()['unrelated'] + 0.05
    m = module_gpu()
    emb = m.embed(gt.cuda())
    loss = m.run(pred.cuda(), gt.cuda())['loss']
    torch.cuda.synchronize()
    truth = t64['embeddings'][3:]                                                     # run() embeds pred's images first
    want = torch.from_numpy(gold['embeddings'])
    f32 = dist(want, truth)
    rec = dict(emb_vs_recording=dist(emb, want), emb_err=dist(emb, truth), emb_f32=f32, loss_err=dist(loss, t64['loss']),
               loss_f32=dist(torch.from_numpy(gold['loss']), t64['loss']))
    record("idloss_recording", **rec)
    print({k: f"{v:.2e}" for k, v in rec.items()})
    assert rec['emb_err'] <= max(2e-6 * float(truth.abs().max()), 3 * f32), rec
    assert rec['loss_err'] <= max(2e-6, 3 * rec['loss_f32']), rec
    assert rec['emb_vs_recording'] <= max(2e-6, 4 * f32), rec                         # both sit within their bounds of the truth


# ---- exact properties -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_repeatability_batch_independence_and_the_two_set_shortcut():
    pred, gt, _, _ = net_case(3, 256)
    m = module_gpu()
    p, g = pred.cuda(), gt.cuda()
    a, b = m.run(p, g, taps=True), m.run(p, g, taps=True)
    for k in ('embeddings', 'dots', 'loss', 'sim_improvement'):
        assert torch.equal(a[k], b[k]), k                                            # two runs
    for x, y in zip(a['taps'], b['taps']):
        assert torch.equal(x, y)
    alone = m.embed(g[2:3])
    assert torch.equal(alone[0], m.embed(g)[2])                                      # alone and at position 2 of a batch of 3
    assert torch.equal(alone[0], a['embeddings'][5])                                 # as y of run(y_hat, y)
    assert torch.equal(alone[0], m.run(g, p)['embeddings'][2])                       # as y_hat
    c = m.run(p, g, x=g.clone())
    assert c['embeddings'].shape == (9, 512)
    for k in ('dots', 'loss', 'sim_improvement'):
        assert torch.equal(a[k], c[k]), k                                            # the two-set shortcut changes nothing
    assert torch.equal(c['embeddings'][:6], a['embeddings']) and torch.equal(c['embeddings'][6:], c['embeddings'][3:6])
    norms = a['embeddings'].double().norm(dim=1)
    assert float((norms - 1).abs().max()) <= 1e-6
    same = m.run(g, g, g)
    assert float(same['loss']) <= 1e-6 and float(same['dots'].min()) >= 1 - 1e-6
    loss, sim, logs = m(p, g, g)
    assert torch.equal(loss, a['loss']) and len(logs) == 3 and logs[1]['diff_target'] == float(a['dots'][1, 0])
    assert abs(sim - float(a['sim_improvement'])) <= 1e-6


@pytest.mark.gpu
def test_the_weight_image_follows_the_parameters():
    pred, gt = golden_images(1, 256)
    m = syn.load_synthetic_idloss(IDLoss()).to("cuda:0")
    p, g = pred.cuda(), gt.cuda()
    base = float(m.run(p, g)['loss'])
    with torch.no_grad():
        m.facenet.body[5].res_layer[2].weight += 0.2                                 # in place: the version counter moves
    after = float(m.run(p, g)['loss'])
    assert after != base
    m.facenet.output_layer[4].running_mean.data.add_(0.5)                            # through .data: needs invalidate()
    _lib.invalidate(m)
    assert float(m.run(p, g)['loss']) != after


# ---- graph capture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_replay_equals_eager():
    pred, gt = golden_images(1, 256)
    m = module_gpu()
    p, g = pred.cuda(), gt.cuda()
    eager = m.run(p, g)                                                              # (warm: the packed image exists)
    eager = (eager['embeddings'].clone(), eager['dots'].clone(), eager['loss'].clone())

    def fn(a, b):
        out = m.run(a, b)
        return out['embeddings'], out['dots'], out['loss']

    call = graphs.GraphedCall(fn, torch.zeros_like(p), torch.ones_like(g) * 0.5)
    replay = [t.clone() for t in call(p, g)]
    torch.cuda.synchronize()
    assert float(eager[2]) > 0
    for a, b in zip(replay, eager):
        assert torch.equal(a, b)


# ---- the metric row ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_image_metrics_fills_the_identity_columns():
    from e3dge_amd.lpips import LPIPS
    from test_gpu_lpips import restate
    pred, gt, t64, t32 = net_case(1, 256)
    m = module_gpu()
    lp = syn.load_synthetic_lpips(LPIPS()).to("cuda:0")
    lp_sd = syn.load_synthetic_lpips(LPIPS()).state_dict()
    p, g = pred.cuda(), gt.cuda()
    row = sharded_eval.image_metrics(p, g, l2_lambda=1.0, lpips=lp, vgg_lambda=1.0, id_loss=m, id_lambda=10.0)
    want = sharded_eval.image_metrics_torch(pred.double(), gt.double(), 1.0, lambda a, b: restate(lp_sd, a, b, torch.float64)['total'], 1.0,
                                            lambda a, b, c: t64['loss'], 10.0)
    torch.cuda.synchronize()
    id_bound = max(2e-6, 3 * dist(t32['loss'], t64['loss']))
    rec = dict(loss_id_err=dist(row[1], want[1]), id_sim_err=dist(row[7], want[7]), loss_rel=abs(float(row[3]) - float(want[3])) / float(want[3]),
               id_bound=id_bound)
    record("idloss_metric_row", **rec)
    print({k: f"{v:.2e}" for k, v in rec.items()})
    assert float(want[1]) > 0.01
    assert rec['loss_id_err'] <= id_bound and rec['id_sim_err'] <= id_bound, rec
    assert rec['loss_rel'] <= 2e-5, rec
    assert torch.equal(row[1], m.run(p, g)['loss']) and torch.equal(row[2], lp(p, g))
    # without the module the row is the existing entries', bit for bit
    assert torch.equal(sharded_eval.image_metrics(p, g, 1.0, lp, 1.0, id_loss=None, id_lambda=10.0), sharded_eval.image_metrics(p, g, 1.0, lp, 1.0))
    assert torch.equal(sharded_eval.image_metrics(p, g, id_loss=None), sharded_eval.image_metrics(p, g))
    only_id = sharded_eval.image_metrics(p, g, 1.0, None, 0.0, id_loss=m, id_lambda=10.0)
    plain = sharded_eval.image_metrics(p, g)
    assert torch.equal(only_id[1], row[1]) and float(only_id[2]) == 0.0
    for c in (0, 4, 5, 6):
        assert torch.equal(only_id[c], plain[c]) and torch.equal(row[c], plain[c]), c
