"""Reader of the cycle stamps that instrumented variant builds record (csrc/stamps.h has the selectors and the word layout):

    python cvpr23-e3dge_amd/build.py --variant phase --only siren -DE3DGE_PHASE_TIMING
    E3DGE_LIB_PATH=cvpr23-e3dge_amd/lib/variants/lib_phase.so python tools/kernel_stamps.py phase

    phase    -DE3DGE_PHASE_TIMING (siren)      cycles per phase of the render kernel: the first sub-tiles of workgroup 0
    phase2   -DE3DGE_PHASE_TIMING (siren)      the same for render pass #2, the launch that reads pass #1's layer-7 record
    bwd      -DE3DGE_BWD_TIMING (siren_bwd)    first-generation backward kernel: thread 0's cycles, averaged over the workgroups
    trace16  -DE3DGE_16_TRACE (siren)          k-step timeline of one GEMM tile (hidden layer 3, tile 6, workgroup 7), waves 0 and 4
    rb       -DE3DGE_RB_TRACE=1|2 (resblock)   timeline of the texture head: workgroup 7, wave 0, second sub-tile
    modconv  -DE3DGE_MC_TIMING (modconv)       cycles per phase of a step of e3dge_modconv3x3, per layer of --layers
    dec2     -DE3DGE_PK_TIMING (decoder2)      cycles per phase of a step of the packed decoder's convolutions, per launch

The stamps live in a side buffer, so the workload's outputs are the default build's: --dump PATH saves them (torch.save) before the
stamps are read, also when the loaded library turns out not to be instrumented (the read then raises, naming the -D it needs)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import e3dge_amd  # noqa: F401,E402
from e3dge_amd import _lib, synthetic as syn  # noqa: E402
from e3dge_amd.camera_utils import generate_camera_params  # noqa: E402

DEV = "cuda:0"


def renderer(a, seed=1, centred=False, **opt):
    """Synthetic renderer at --res / --samples, one latent (of `seed`) and one camera (`centred`: the frontal one)."""
    from e3dge_amd.volume_renderer import VolumeFeatureRenderer
    r = VolumeFeatureRenderer(syn.rendering_opt(N_samples=a.samples, **opt), out_im_res=a.res, mode='test')
    syn.load_synthetic(r, prefix='renderer.')
    r = r.to(DEV)
    r.requires_grad_(False)
    wr, _ = syn.synthetic_inputs(1, seed=seed, device=DEV)
    poses, focal, near, far, _ = generate_camera_params(a.res, DEV, **(dict(locations=torch.zeros(1, 2, device=DEV)) if centred else {}))
    return r, wr, (poses, focal, near, far)


def run(fn, times):
    """`times` calls (the stamps of the last one stay), synchronised; the last result."""
    with torch.no_grad():
        for _ in range(times):
            out = fn()
    torch.cuda.synchronize()
    return out


def dump(a, out):
    if a.dump:
        keep = lambda v: v.detach().cpu() if torch.is_tensor(v) else v
        torch.save({k: keep(v) for k, v in out.items()} if isinstance(out, dict) else [keep(v) for v in out], a.dump)


def print_phases(names, f16, over=None):
    s = _lib.read_stamps("siren")
    t = s[0]
    d = [0 if i == 0 else t[i] - t[i - 1] for i in range(18)]      # (entry 6 sub: the gap between two sub-tiles)
    for sub in range(3):
        print(f"sub-tile {sub}: " + ", ".join(f"{names[i]}={d[sub * 6 + i]:.0f}" for i in range(6)))
    if f16:       # 8-wave kernel: thread 0's totals
        print(f"chunk sync totals of wave 0{over or ''}: dma-wait={t[18]:.0f} barrier={t[19]:.0f}")
        if over:
            print("sum", float(sum(d)), " mfma-only per sub-tile would be", 16 * 24 * 128, "per wave,", 2 * 16 * 24 * 128, "per SIMD (two waves)")
        print(f"workgroup 0, thread 0: prologue {t[21] - t[20]:.0f} cycles, sub-tile loop {t[22] - t[21]:.0f}, per-ray output stores {t[23] - t[22]:.0f}")
    else:
        print("chunk_sync totals per wave (cycles over 192 tiles): " + "; ".join(f"w{w}: dma-wait={s[1 + w][0]:.0f} barrier={s[1 + w][1]:.0f} issue=0" for w in range(4)))
        print("sum", float(sum(d)), " mfma-only per sub-tile would be", 8224 * 64)


def cmd_phase(a):
    r, wr, cam = renderer(a, centred=True)
    dump(a, run(lambda: r(*cam, styles=wr), 3))
    print_phases(["(gap)", "geometry+layer0", "layers1-7", "sdf+alpha+scan", "view layer", "rgb+composite+merge"], r.siren.mfma_mode == "f16x3",
                 " (cycles over 384 tiles)")


def cmd_phase2(a):
    from e3dge_amd.volume_renderer import _LazyTex, _fuse_texfilm
    r, wr, (poses, focal, near, far) = renderer(a, centred=True, enable_local_model=True, L_pred_tex_modulations=True)
    g = torch.Generator().manual_seed(3)
    tex = tuple(torch.randn(1, a.res, a.res, a.samples, 256, generator=g).to(DEV) * 0.1 for _ in range(2))
    feats = torch.randn(1, a.res, a.res, a.samples, 301, generator=g).to(DEV)
    if _fuse_texfilm():
        tex = _LazyTex(r.network.netLocal.local_feat_to_tex_modulations_linear, feats)      # what the inversion forward runs
    print('texture FiLM:', 'fused into the record (head + FiLM launch)' if _fuse_texfilm() else '(alpha, beta) from HBM')
    with torch.no_grad():
        film = r.siren.film_params(wr)
        key = r._reuse_key(wr, focal, poses, near, far)

    def both():
        r.render_with_film(film, focal, poses, near, far, reuse_key=key)                              # pass #1 (+ record)
        return r.render_with_film(film, focal, poses, near, far, tex_conditions=tex, reuse_key=key)   # pass #2 on the record
    dump(a, run(both, 3))
    print_phases(["(gap)", "geometry+record read", "layers1-7 (skipped)", "sdf+alpha+scan (skipped)", "view layer", "rgb+composite+merge"], True)


def cmd_bwd(a):
    os.environ.setdefault("E3DGE_BWD_MODE", "f16x3")       # the instrumented kernel is the first-generation one
    from e3dge_amd.volume_renderer import saved_state_buffer, siren_backward
    r, wr, (poses, focal, near, far) = renderer(a, seed=7)
    film = r.siren.film_params(wr)
    n_pts = a.res * a.res * a.samples
    args = saved_state_buffer(1, n_pts, 9, DEV)
    with torch.no_grad():
        r.render_with_film(film, focal, poses, near, far, None, save_args=args)
    g = torch.Generator().manual_seed(5)
    d_rgb, d_sdf, d_feat = (torch.randn(*sh, generator=g).to(DEV) for sh in ((1, n_pts, 3), (1, n_pts), (1, n_pts, 256)))
    dump(a, run(lambda: siren_backward(r.siren, film, args, d_feat, d_rgb, d_sdf), 3))
    rows = [s for s in _lib.read_stamps("siren_bwd") if s[0]]
    if not rows:
        sys.exit(f"no workgroup recorded: backward mode {r.siren.bwd_mode!r} does not run the first-generation kernel")
    v = [sum(s[i] for s in rows) / len(rows) for i in range(7)]
    names = ["total", "prologue(view layer)", "GEMM tiles (incl. sync+fetch)", "epilogues", "layer tails", "  of GEMM: vmcnt wait", "  of GEMM: barrier wait"]
    print(f"{len(rows)} workgroups; cycles per wave (s_memtime units), wave 0 average:")
    for n, x in zip(names, v):
        print(f"  {n:<32} {x:12.0f}  ({100 * x / v[0]:.1f}%)")
    print(f"  pure MFMA time would be {192 * 8192} shader cycles")


def cmd_trace16(a):
    r, wr, cam = renderer(a, seed=7)
    dump(a, run(lambda: r(*cam, styles=wr), 3))
    s = _lib.read_stamps("siren")
    v = s[8] + s[9]
    t0 = min((x for x in v if x), default=0)
    for w in range(2):
        print(f"wave {4 * w}:")
        for g in range(8):
            t, u, c = (v[w * 24 + 3 * g + i] - t0 for i in range(3))
            print(f"   k-step {g}: start {t:6d}   mfma issued {u:6d} (+{u - t:4d})   epilogue done {c:6d} (+{c - u:4d})")


def cmd_rb(a):
    from e3dge_amd.volume_renderer import ResnetBlockFC
    prefix = 'renderer.network.netLocal.local_feat_to_tex_modulations_linear.'
    h = ResnetBlockFC(301, 512)
    h.load_state_dict({k: syn.synthetic_tensor(prefix + k, v.shape) for k, v in h.state_dict().items()})
    h = h.to(DEV)
    feats = syn.synthetic_local_feats(1, a.res, a.samples, device=DEV)
    dump(a, run(lambda: h.tex_modulations(feats), 5))
    names = {100: "chunk wait: enter", 200: "chunk wait: own DMA landed", 300: "chunk wait: barrier passed", 400: "GEMM done",
             500: "epilogue done", 600: "W_s x done", 700: "W_1 r done", 800: "stores issued", 1000: "sub-tile start",
             2000: "x loaded and split", 3000: "phase 2 done", 4000: "phase 3 done"}
    s = _lib.read_stamps("resblock")
    t0 = prev = s[0][1]
    for tag, t in (row[:2] for row in s):
        if t == 0:
            break
        print(f"{t - t0:8d}  (+{t - prev:6d})  {names.get(tag, f'k-step {tag}')}")
        prev = t
    if t0 == 0:
        print("no stamp recorded: workgroup 7 needs a second sub-tile (more than 256 tiles of 128 points)")


def cmd_modconv(a):
    from e3dge_amd.stylesdf_model import StyledConv
    names = ["issue(dma+loads)", "mfma", "epilogue", "convert+lds-store", "vmcnt-wait", "barrier"]
    outs, lines, err = [], [], None
    for spec in a.layers.split(","):
        ci, co, res, up = (list(map(int, spec.split(":"))) + [0])[:4]
        m = StyledConv(ci, co, 3, 512, upsample=bool(up))
        sd = {k: syn.synthetic_tensor('decoder.convs.0.' + k, v.shape, ci) for k, v in m.state_dict().items() if not k.endswith('kernel')}
        m.load_state_dict(sd, strict=False)
        m = m.to(DEV).eval()
        g = torch.Generator().manual_seed(ci + co)
        x, style = torch.randn(1, ci, res, res, generator=g).to(DEV), torch.randn(1, 512, generator=g).to(DEV)
        noise = None if up else torch.randn(1, 1, res, res, generator=g).to(DEV)
        buf = torch.zeros(_lib.AMAX_FLOATS, device=DEV)
        outs += [run(lambda: m.conv.forward_fused(x, style, noise=noise, noise_weight=m.noise.weight, bias=m.activate.bias, act=not up,
                                                  out_amax=buf), 3), buf]
        try:          # (every launch overwrites slot 0: read per layer; an uninstrumented library is reported after the dump)
            d = _lib.read_stamps("modconv")[0]
        except RuntimeError as e:
            err = e
            continue
        tot, steps = d[6], max(d[7], 1)
        lines.append(f"{ci:4d}->{co:4d} @{res:5d}{' up' if up else '   '}: steps {steps:.0f}, cycles/step {tot / steps:8.0f} | " +
                     ", ".join(f"{n} {v / steps:7.0f}" for n, v in zip(names, d[:6])))
    dump(a, outs)
    if err is not None:
        raise err
    print("\n".join(lines))


def cmd_dec2(a):
    from e3dge_amd.stylesdf_model import G_pred_latents
    g = G_pred_latents(syn.model_opt(size=a.size, channel_multiplier=a.cm, renderer_spatial_output_dim=a.res),
                       syn.rendering_opt(N_samples=24), full_pipeline=True)
    syn.load_synthetic(g)
    dec = g.to(DEV).eval().decoder
    _, wd = syn.synthetic_inputs(1, seed=1, device=DEV)
    wd = wd[:, :dec.n_latent].contiguous()
    feats = (0.5 * torch.randn(1, dec.conv1.conv.in_channel, a.res, a.res, generator=torch.Generator().manual_seed(2))).to(DEV).contiguous()
    noise = [getattr(dec.noises, f"noise_{i}") for i in range(dec.num_layers)]
    dump(a, [run(lambda: dec._forward_packed(feats, wd, noise), 2)])
    s = _lib.read_stamps("decoder2")
    rows = {"conv1": 1}
    for u in range(len(dec.to_rgbs)):
        rows[f"L{u}.upblur(per TILE: wait, taps, H pass + LDS + barriers [gen 1: T->LDS], V pass + store [gen 1: blur + store])"] = 3 + 3 * u
        rows[f"L{u}.conv"] = 4 + 3 * u
    for name, r in rows.items():
        for wv, d in (("w0", s[2 * r]), ("wl", s[2 * r + 1])):
            steps = max(d[9], 1)
            print(json.dumps(dict(what="phase_cycles_per_step", layer=name, wave=wv, steps=int(steps), total=round(d[8] / steps),
                                  wait_barrier=round(d[0] / steps), issue=round(d[1] / steps), mfma=round(d[2] / steps), epilogue=round(d[3] / steps))))
        t4 = s[2 * r][4:8]
        print(json.dumps(dict(what="tap_cycles_total(w0)", layer=name, epi_step_tap0=t4[0], epi_step_taps1_8=t4[1], other_step_tap0=t4[2],
                              other_step_taps1_8=t4[3])))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cmd", choices=["phase", "phase2", "bwd", "trace16", "rb", "modconv", "dec2"])
    ap.add_argument("--res", type=int, default=64, help="image side (phase, phase2, bwd, trace16, rb); input side of the decoder (dec2)")
    ap.add_argument("--samples", type=int, default=24, help="samples per ray (phase, phase2, bwd, trace16, rb)")
    ap.add_argument("--layers", default="256:512:64,512:256:64:1,256:256:128,256:128:128:1,128:128:256,128:64:256:1,64:64:512,64:32:512:1,32:32:1024",
                    help="modconv: comma list of ci:co:res[:1 = up-sampling]")
    ap.add_argument("--size", type=int, default=1024, help="dec2: output side of the decoder")
    ap.add_argument("--cm", type=int, default=2, help="dec2: channel multiplier")
    ap.add_argument("--dump", help="torch.save the workload's outputs here")
    a = ap.parse_args()
    torch.manual_seed(0)          # (random camera poses: the same in every process, so that two builds' dumps can be compared)
    globals()["cmd_" + a.cmd](a)


if __name__ == "__main__":
    main()
