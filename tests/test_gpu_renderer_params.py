"""GPU: gradients of the renderer's own parameters (VolumeFeatureRenderer.train_renderer, ABI 16) against torch autograd
of the oracle over a state dict whose tensors require grad.

Tolerance per parameter tensor, as in test_gpu_backward.py: max|d - truth| <= 5e-5 * max|truth| (or 2x the fp32 oracle's own distance
where that is larger) and <= 4 x (fp32 oracle vs truth) + 2e-5 * max|truth|."""
import math

import pytest
import torch
from torch.nn import functional as F

from conftest import full_state_dict
from oracle import decoder_ref, renderer_ref

import e3dge_amd  # noqa: F401
from e3dge_amd import synthetic as syn
from e3dge_amd.camera_utils import generate_camera_params
from e3dge_amd.volume_renderer import lin_buffers, saved_state_buffer, saved_state_point_major, siren_backward, siren_param_grads
from test_gpu_renderer import make_renderer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def sd():
    return full_state_dict()[1]


def trainable(sd, res, S):
    r = make_renderer(sd, res, S)
    r.train_renderer = True
    r.requires_grad_(True)
    return r


def leaf_sd(sd, dtype):
    return {k: (v.detach().to(dtype).clone().requires_grad_(True) if k.startswith('renderer.') and v.is_floating_point() else v)
            for k, v in sd.items()}


def check_grads(r, sd64, sd32, tag):
    worst = 0.0
    n = 0
    for name, p in r.named_parameters():
        key = 'renderer.' + name
        truth, t32 = sd64[key].grad, sd32[key].grad
        if truth is None:                         # (sigmoid_beta does not enter run_network)
            assert p.grad is None or not p.grad.any(), f"{tag}: {name}"
            continue
        assert p.grad is not None, f"{tag}: no gradient for {name}"
        d = p.grad.detach().double().cpu()
        mt = float(truth.abs().max())
        if mt == 0.0:
            assert float(d.abs().max()) == 0.0, f"{tag}: {name}"
            continue
        e = float((d - truth).abs().max()) / mt
        e32 = float((t32.double() - truth).abs().max()) / mt
        assert math.isfinite(e) and e <= max(5e-5, 2 * e32) and e <= 4 * e32 + 2e-5, f"{tag}: {name} rel err {e:.2e} (fp32 oracle {e32:.2e})"
        worst = max(worst, e)
        n += 1
    print(f"[{tag}] {n} parameter tensors, worst rel err {worst:.2e}")
    return n


# (20001, 2): padded rows at the image boundary inside one split-K slab of the big products, several slabs per workgroup of the small kernel
@pytest.mark.parametrize("n_pts,B", [(1, 1), (130, 2), (1000, 1), (4096, 2), (20001, 2)])
def test_run_network_parameter_gradients(sd, n_pts, B):
    r = trainable(sd, 8, 18)
    g = torch.Generator().manual_seed(n_pts + B)
    pts = (torch.rand((B, n_pts, 3), generator=g) * 0.24 - 0.12)
    vd = F.normalize(torch.randn((B, n_pts, 3), generator=g), dim=-1)
    styles = syn.synthetic_inputs(B, seed=3, device="cpu")[0]
    gr = torch.randn((B, n_pts, 260), generator=g)
    raw = r.run_network(pts.to(DEV), vd.to(DEV), styles=styles.to(DEV))
    (raw * gr.to(DEV)).sum().backward()
    sds = {}
    for dt in (torch.float64, torch.float32):
        s = leaf_sd(sd, dt)
        (renderer_ref.query_points(s, pts, vd, styles, dtype=dt) * gr.to(dt)).sum().backward()
        sds[dt] = s
    assert check_grads(r, sds[torch.float64], sds[torch.float32], f"run_network {n_pts}x{B}") == 58


def _cams(res, B):
    locs = torch.tensor([[0.1, -0.05], [-0.2, 0.15]], device=DEV)[:B]
    return generate_camera_params(res, DEV, locations=locs)[:4]


KEYS = ('gen_thumb_imgs', 'features', 'xyz', 'depth', 'sdf', 'hit_prob')


@pytest.mark.parametrize("res,S,B", [(8, 18, 1), (8, 18, 2), (16, 24, 1), (16, 24, 2)])
def test_render_parameter_gradients(sd, res, S, B):
    r = trainable(sd, res, S)
    poses, focal, near, far = _cams(res, B)
    wr = syn.synthetic_inputs(B, seed=5, device=DEV)[0]
    st = wr.clone().requires_grad_(True)
    out = r(poses, focal, near, far, styles=st)
    g = torch.Generator().manual_seed(res * 100 + B)
    G = {k: torch.randn(tuple(out[k].shape), generator=g) for k in KEYS}
    sum(((out[k] * G[k].to(DEV)).sum() for k in KEYS)).backward()
    # the frozen path's d(styles), bit for bit
    rf = make_renderer(sd, res, S)
    sf = wr.clone().requires_grad_(True)
    of = rf(poses, focal, near, far, styles=sf)
    sum(((of[k] * G[k].to(DEV)).sum() for k in KEYS)).backward()
    assert torch.equal(st.grad, sf.grad)
    c = lambda t: t.detach().cpu()
    sds = {}
    for dt in (torch.float64, torch.float32):
        s = leaf_sd(sd, dt)
        ro = renderer_ref.render(s, c(poses), c(focal), c(near), c(far), c(wr), res=res, n_samples=S, dtype=dt)
        sum(((ro[k].reshape(G[k].shape) * G[k].to(dt)).sum() for k in KEYS)).backward()
        sds[dt] = s
    assert check_grads(r, sds[torch.float64], sds[torch.float32], f"render {res}x{res}x{S} B={B}") == 59


def test_two_backwards_are_bit_identical(sd):
    r = trainable(sd, 16, 24)
    poses, focal, near, far = _cams(16, 2)
    wr = syn.synthetic_inputs(2, seed=7, device=DEV)[0]
    grads = []
    for _ in range(2):
        r.zero_grad(set_to_none=True)
        out = r(poses, focal, near, far, styles=wr)
        ((out['gen_thumb_imgs'] ** 2).mean() + (out['features'] ** 2).mean() + out['depth'].mean()).backward()
        grads.append([p.grad.clone() for p in r.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))


def test_padded_rows_with_nan_do_not_leak(sd):
    """n_pts not a multiple of 16; the padded rows of the saved state and of d_lin hold NaN: the outputs are finite and equal the clean run."""
    r = trainable(sd, 8, 18)
    siren = r.siren
    B, N = 2, 130
    g = torch.Generator().manual_seed(11)
    pts = (torch.rand((B, N, 3), generator=g) * 0.24 - 0.12).to(DEV)
    vd = F.normalize(torch.randn((B, N, 3), generator=g), dim=-1).to(DEV)
    styles = syn.synthetic_inputs(B, seed=2, device=DEV)[0]
    d_raw = torch.randn((B, N, 260), generator=g).to(DEV)
    res = []
    for fill in (0.0, float('nan')):
        args = saved_state_buffer(B, N, 9, DEV)
        args._base.fill_(fill)
        film = siren.film_params(styles)
        siren._points_launch(film, pts, vd, r.box_scale, True, None, args)
        lin = lin_buffers(B, N, DEV)
        lin[0]._base.fill_(fill)
        _, dfilm, _, _ = siren_backward(siren, film, args, d_raw[..., 4:], d_raw[..., :3], d_raw[..., 3], lin=lin)
        res.append(siren_param_grads(siren, film, styles, dfilm, args, lin[0], lin[1], d_raw[..., 3], d_raw[..., :3], pts, vd, 1,
                                     r.box_scale))
    for a, b in zip(*res):
        assert torch.isfinite(b).all() and torch.equal(a, b)


def _forward_with_args(sd, pts, vd, styles):
    """The oracle's siren_forward with every pre-sine argument a_l kept (float64), for checking d_lin."""
    pre = 'renderer.network.'
    h = pts * (1 / 0.12)
    args, gammas = [], []
    for l in range(9):
        p = f'{pre}pts_linears.{l}.' if l < 8 else f'{pre}views_linears.'
        if l == 8:
            sdf = F.linear(h, sd[pre + 'sigma_linear.weight'], sd[pre + 'sigma_linear.bias'])
            h = torch.cat([h, vd], -1)
        s = styles[:, l:l + 1]
        gamma = 15 * F.linear(s, sd[p + 'gamma.weight'], sd[p + 'gamma.bias']) + 30
        beta = 0.25 * F.linear(s, sd[p + 'beta.weight'], sd[p + 'beta.bias'])
        a = gamma * F.linear(h, sd[p + 'weight'], sd[p + 'bias']) + beta
        a.retain_grad()
        args.append(a)
        gammas.append(gamma)
        h = torch.sin(a)
    rgb = F.linear(h, sd[pre + 'rgb_linear.weight'], sd[pre + 'rgb_linear.bias'])
    return torch.cat([rgb, sdf, h], -1), args, gammas


def test_d_lin_matches_float64_autograd(sd):
    r = trainable(sd, 8, 18)
    siren = r.siren
    B, N = 1, 37
    g = torch.Generator().manual_seed(5)
    pts = torch.rand((B, N, 3), generator=g) * 0.24 - 0.12
    vd = F.normalize(torch.randn((B, N, 3), generator=g), dim=-1)
    styles = syn.synthetic_inputs(B, seed=4, device="cpu")[0]
    d_raw = torch.randn((B, N, 260), generator=g)
    args = saved_state_buffer(B, N, 9, DEV)
    film = siren.film_params(styles.to(DEV))
    siren._points_launch(film, pts.to(DEV), vd.to(DEV), r.box_scale, True, None, args)
    lin = lin_buffers(B, N, DEV)
    dd = d_raw.to(DEV)
    siren_backward(siren, film, args, dd[..., 4:], dd[..., :3], dd[..., 3], lin=lin)
    got = saved_state_point_major(lin[0], True).double().cpu()
    s64 = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    raw, a_l, gam = _forward_with_args(s64, pts.double().requires_grad_(True), vd.double(), styles.double())
    (raw * d_raw.double()).sum().backward()
    for l in range(9):
        truth = gam[l] * a_l[l].grad
        e = float((got[:, :, l] - truth).abs().max() / truth.abs().max())
        assert e <= 5e-5, f"d_lin layer {l}: rel err {e:.2e}"


def test_refusals(sd):
    r = trainable(sd, 8, 18)
    poses, focal, near, far = _cams(8, 1)
    wr = syn.synthetic_inputs(1, seed=1, device=DEV)[0]
    with pytest.raises(NotImplementedError, match="eikonal"):
        r(poses, focal, near, far, styles=wr, return_eikonal=True)
    with pytest.raises(NotImplementedError, match="texture"):
        z = torch.zeros((1, 8, 8, 18, 256), device=DEV)
        r.render(focal, poses, near, far, wr, tex_conditions=(z, z))
    pts = torch.zeros((1, 20, 3), device=DEV)
    with pytest.raises(NotImplementedError, match="eikonal"):
        r.siren.query_points(pts, pts, wr, r.box_scale, want_eikonal=True)
    r.siren.bwd_mode = "f32"
    with pytest.raises(NotImplementedError, match="f16x3_g2"):
        r.run_network(pts, pts, styles=wr)
    # without the opt-in, trainable weights are refused as before
    r0 = make_renderer(sd, 8, 18)
    r0.requires_grad_(True)
    assert not r0.train_renderer
    with pytest.raises(NotImplementedError, match="frozen"):
        r0(poses, focal, near, far, styles=wr.clone().requires_grad_(True))


def test_adam_steps_refresh_the_weight_image(sd):
    """Three Adam steps on every renderer parameter; the next forward equals the oracle evaluated on the updated state dict."""
    res, S = 16, 24
    r = trainable(sd, res, S)
    poses, focal, near, far = _cams(res, 1)
    wr = syn.synthetic_inputs(1, seed=9, device=DEV)[0]
    opt = torch.optim.Adam(r.parameters(), lr=1e-3)
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        out = r(poses, focal, near, far, styles=wr)
        ((out['gen_thumb_imgs'] ** 2).mean() + 0.1 * (out['features'] ** 2).mean()).backward()
        opt.step()
    new_sd = dict(sd)
    new_sd.update({'renderer.' + k: v.detach().cpu() for k, v in r.state_dict().items()})
    assert not torch.equal(new_sd['renderer.network.pts_linears.3.weight'], sd['renderer.network.pts_linears.3.weight'])
    with torch.no_grad():
        out = r(poses, focal, near, far, styles=wr)
    c = lambda t: t.detach().cpu()
    ref = renderer_ref.render(new_sd, c(poses), c(focal), c(near), c(far), c(wr), res=res, n_samples=S)
    stale = renderer_ref.render(sd, c(poses), c(focal), c(near), c(far), c(wr), res=res, n_samples=S)
    # (the stated forward tolerances x3: three Adam steps at lr 1e-3 move the weights off the fixture's conditioning)
    for k, tol in (('gen_thumb_imgs', 5e-6), ('depth', 4e-6), ('sdf', 1e-5), ('features', 1e-4)):
        e = float((c(out[k]).double() - ref[k].reshape(out[k].shape).double()).abs().max())
        assert e <= 3 * tol, f"{k}: {e:.2e}"
        assert float((stale[k] - ref[k]).abs().max()) > 100 * tol, k      # a stale weight image could not pass


def test_generator_sets_train_renderer():
    from e3dge_amd.stylesdf_model import G_pred_latents
    for freeze in (True, False):
        g = G_pred_latents(syn.model_opt(size=64, channel_multiplier=1, renderer_spatial_output_dim=8, freeze_renderer=freeze),
                           syn.rendering_opt(N_samples=8), full_pipeline=False)
        assert g.renderer.train_renderer == (not freeze)


def test_only_sigmoid_beta_trains(sd):
    """Only sigmoid_beta requires grad: its gradient (the compositing backward alone) against float64 autograd."""
    res, S = 16, 24
    r = make_renderer(sd, res, S)
    r.train_renderer = True
    r.sigmoid_beta.requires_grad_(True)
    poses, focal, near, far = _cams(res, 2)
    wr = syn.synthetic_inputs(2, seed=6, device=DEV)[0]
    out = r(poses, focal, near, far, styles=wr)
    g = torch.Generator().manual_seed(17)
    G = {k: torch.randn(tuple(out[k].shape), generator=g) for k in KEYS}
    sum(((out[k] * G[k].to(DEV)).sum() for k in KEYS)).backward()
    c = lambda t: t.detach().cpu()
    gr = {}
    for dt in (torch.float64, torch.float32):
        s_ = leaf_sd(sd, dt)
        ro = renderer_ref.render(s_, c(poses), c(focal), c(near), c(far), c(wr), res=res, n_samples=S, dtype=dt)
        sum(((ro[k].reshape(G[k].shape) * G[k].to(dt)).sum() for k in KEYS)).backward()
        gr[dt] = s_['renderer.sigmoid_beta'].grad
    truth = gr[torch.float64]
    e = float((c(r.sigmoid_beta.grad).double() - truth).abs().max() / truth.abs().max())
    e32 = float((gr[torch.float32].double() - truth).abs().max() / truth.abs().max())
    assert e <= max(5e-5, 2 * e32) and e <= 4 * e32 + 2e-5, f"sigmoid_beta rel err {e:.2e} (fp32 oracle {e32:.2e})"
    assert all(p.grad is None for n, p in r.named_parameters() if n != 'sigmoid_beta')


def test_pti_shaped_generator_loop(sd):
    """A PTI step (projectors.py:447-640): the whole generator trainable, image loss through the decoder (library path with trainable
    weights).  Step 1's renderer gradients against float64 autograd of renderer_ref.render -> decoder_ref.decoder_forward (noise buffers on
    both sides); after three Adam steps the forward equals the oracle on the updated state dict."""
    from e3dge_amd.stylesdf_model import G_pred_latents
    res, S = 16, 24
    gen = G_pred_latents(syn.model_opt(size=256, channel_multiplier=1, renderer_spatial_output_dim=res, freeze_renderer=False,
                                       is_test=False), syn.rendering_opt(N_samples=S), full_pipeline=True)
    syn.load_synthetic(gen)
    sd0 = {k: v.detach().clone() for k, v in gen.state_dict().items()}
    gen = gen.to(DEV)
    assert gen.renderer.train_renderer
    gen.requires_grad_(True)
    wr, wd = syn.synthetic_inputs(1, seed=1, device=DEV)
    wd = wd[:, :gen.decoder.n_latent]
    poses, focal, near, far = _cams(res, 1)
    loss_of = lambda img, thumb: (F.avg_pool2d(img, 4) ** 2).mean() + 0.1 * (thumb ** 2).mean()
    opt = torch.optim.Adam([p for p in gen.parameters() if p.requires_grad], lr=1e-3)
    c = lambda t: t.detach().cpu()
    for it in range(3):
        opt.zero_grad(set_to_none=True)
        out = gen([wr, wd], poses, focal, near, far, input_is_latent=True, randomize_noise=False)
        loss_of(out['gen_imgs'], out['gen_thumb_imgs']).backward()
        if it == 0:
            sds = {}
            for dt in (torch.float64, torch.float32):
                s_ = leaf_sd(sd0, dt)
                ro = renderer_ref.render(s_, c(poses), c(focal), c(near), c(far), c(wr), res=res, n_samples=S, dtype=dt)
                img = decoder_ref.decoder_forward(s_, ro['features'], c(wd), dtype=dt)
                loss_of(img, ro['gen_thumb_imgs']).backward()
                sds[dt] = s_
            assert check_grads(gen.renderer, sds[torch.float64], sds[torch.float32], "PTI step 1") == 59
        opt.step()
    new_sd = {k: v.detach().cpu() for k, v in gen.state_dict().items()}
    assert not torch.equal(new_sd['renderer.network.pts_linears.3.weight'], sd0['renderer.network.pts_linears.3.weight'])
    with torch.no_grad():
        out = gen([wr, wd], poses, focal, near, far, input_is_latent=True, randomize_noise=False)
        ref = renderer_ref.render(new_sd, c(poses), c(focal), c(near), c(far), c(wr), res=res, n_samples=S)
        ref_img = decoder_ref.decoder_forward(new_sd, ref['features'], c(wd))
    # (smoke()'s forward tolerances x3: three Adam steps move the weights off the fixture's conditioning)
    e_t = float((c(out['gen_thumb_imgs']).double() - ref['gen_thumb_imgs'].double()).abs().max())
    e_i = float((c(out['gen_imgs']).double() - ref_img.double()).abs().max())
    assert e_t <= 1.5e-5 and e_i <= 3e-4, (e_t, e_i)
