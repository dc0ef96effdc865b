"""Times the renderer's training step with and without parameter gradients, 64x64x24, B = 1 and 4:
  frozen      render forward + backward to the styles (the encoder-training step)
  trainable   the same with VolumeFeatureRenderer.train_renderer and every renderer parameter requiring grad, and its parts:
              the network backward with / without the d_lin stores, e3dge_siren_wgrad, the host-side FiLM-parameter einsums
  library     torch autograd of oracle/renderer_ref.py in fp32 on the GPU, all parameters requiring grad
Usage: python tools/time_renderer_params.py [--res 64] [--samples 24] [--iters 10]"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import e3dge_amd  # noqa: E402,F401
from e3dge_amd import _lib, synthetic as syn  # noqa: E402
from e3dge_amd.camera_utils import generate_camera_params  # noqa: E402
from e3dge_amd.volume_renderer import VolumeFeatureRenderer, lin_buffers, siren_param_grads  # noqa: E402
from oracle import renderer_ref  # noqa: E402

DEV = "cuda:0"


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--samples", type=int, default=24)
    ap.add_argument("--iters", type=int, default=10)
    o = ap.parse_args()
    res, S = o.res, o.samples
    for B in (1, 4):
        r = VolumeFeatureRenderer(syn.rendering_opt(N_samples=S), out_im_res=res, mode='test')
        syn.load_synthetic(r, prefix='renderer.')
        r = r.to(DEV)
        sd = {'renderer.' + k: v.detach() for k, v in r.state_dict().items()}
        locs = torch.rand((B, 2), device=DEV) * 0.3 - 0.15
        poses, focal, near, far, _ = generate_camera_params(res, DEV, locations=locs)
        wr = syn.synthetic_inputs(B, seed=1, device=DEV)[0]

        def step(train):
            r.train_renderer = train
            r.requires_grad_(train)
            st = wr.clone().requires_grad_(True)
            out = r(poses, focal, near, far, styles=st)
            ((out['gen_thumb_imgs'] ** 2).mean() + (out['features'] ** 2).mean()).backward()
        t_frozen = timed(lambda: step(False), o.iters)
        t_train = timed(lambda: step(True), o.iters)

        # parts: the network backward of one stored render with and without the d_lin stores, the contraction, the host einsums
        siren = r.siren
        n_pts = res * res * S
        from e3dge_amd.volume_renderer import saved_state_buffer, siren_backward
        film = siren.film_params(wr)
        args = saved_state_buffer(B, n_pts, 9, DEV)
        with torch.no_grad():
            r.render_with_film(film, focal, poses, near, far, None, save_args=args)
        g = torch.Generator(device=DEV).manual_seed(0)
        d_rgb = torch.randn((B, n_pts, 3), device=DEV, generator=g)
        d_sdf = torch.randn((B, n_pts), device=DEV, generator=g)
        d_feat = torch.randn((B, n_pts, 256), device=DEV, generator=g) * 1e-3
        lin = lin_buffers(B, n_pts, DEV)
        t_bwd = timed(lambda: siren_backward(siren, film, args, d_feat, d_rgb, d_sdf), o.iters)
        t_bwd_lin = timed(lambda: siren_backward(siren, film, args, d_feat, d_rgb, d_sdf, lin=lin), o.iters)
        dfilm = siren_backward(siren, film, args, d_feat, d_rgb, d_sdf, lin=lin)[1]
        pts = torch.rand((B, n_pts, 3), device=DEV) * 0.2 - 0.1
        vd = torch.nn.functional.normalize(torch.randn((B, res * res, 3), device=DEV), dim=-1)
        t_all = timed(lambda: siren_param_grads(siren, film, wr, dfilm, args, lin[0], lin[1], d_sdf, d_rgb, pts, vd, S, r.box_scale), o.iters)
        lib = _lib.load()
        n_ws = lib.e3dge_siren_wgrad_ws_floats(B, n_pts)
        ws = torch.empty(n_ws, device=DEV)
        outs = [torch.empty(n, device=DEV) for n in (8 * 256 * 256, 768, 768, 256, 1, 768, 3)]
        a = _lib.SirenWgradArgs(args=_lib.ptr(args), d_lin=_lib.ptr(lin[0]), lin_amax=_lib.ptr(lin[1]), d_sdf=_lib.ptr(d_sdf),
                                d_rgb=_lib.ptr(d_rgb), pts=_lib.ptr(pts), viewdirs=_lib.ptr(vd), d_w=_lib.ptr(outs[0]),
                                d_w_view_dirs=_lib.ptr(outs[1]), d_w_first=_lib.ptr(outs[2]), d_w_sigma=_lib.ptr(outs[3]),
                                d_b_sigma=_lib.ptr(outs[4]), d_w_rgb=_lib.ptr(outs[5]), d_b_rgb=_lib.ptr(outs[6]), ws=_lib.ptr(ws),
                                ws_floats=n_ws, n_pts=n_pts, batch=B, samples=S, precision=_lib.PREC_F16X3_G2, box_scale=float(r.box_scale))
        t_wgrad = timed(lambda: _lib.check(lib.e3dge_siren_wgrad(ctypes.byref(a), _lib.stream_of(args)), "e3dge_siren_wgrad"), o.iters)

        # library figure: fp32 autograd of the oracle on the GPU
        def lib_step():
            s = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
            st = wr.clone().requires_grad_(True)
            ro = renderer_ref.render(s, poses, focal, near, far, st, res=res, n_samples=S)
            ((ro['gen_thumb_imgs'] ** 2).mean() + (ro['features'] ** 2).mean()).backward()
        try:
            t_lib = timed(lib_step, max(2, o.iters // 5), warm=1)
        except RuntimeError as e:          # (out of memory at large B)
            t_lib = float('nan')
            print("library step failed:", str(e).splitlines()[0])
        print(f"B={B} {res}x{res}x{S}: frozen step {t_frozen:.3f} ms | trainable step {t_train:.3f} ms (+{t_train - t_frozen:.3f}) | "
              f"network bwd {t_bwd:.3f} -> {t_bwd_lin:.3f} ms with d_lin stores (+{t_bwd_lin - t_bwd:.3f}) | e3dge_siren_wgrad {t_wgrad:.3f} ms | "
              f"param grads incl. host {t_all:.3f} ms (host parts {t_all - t_wgrad:.3f}) | library fp32 autograd {t_lib:.3f} ms", flush=True)


if __name__ == "__main__":
    main()
