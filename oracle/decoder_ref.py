"""CPU restatement of the StyleGAN2 up-sampler of StyleSDF (TEST INFRASTRUCTURE -- see oracle/__init__.py).

Functional PyTorch over a state dict with the reference's key names.
Reference: project/models/stylesdf_model.py -- line numbers cited per function."""
import math

import torch
from torch.nn import functional as F

from .ops_ref import fused_leaky_relu_ref, upfirdn2d_ref_simple


def _w(sd, key, dtype):
    return sd[key].to(dtype)


def fir(taps=(1, 3, 3, 1), gain=1.0, dtype=torch.float32):
    """make_kernel :85-93 (outer product, normalised), times `gain` (Blur :155-156, Upsample :102)."""
    k = torch.tensor(taps, dtype=torch.float32)
    k = k[None, :] * k[:, None]
    return (k / k.sum() * gain).to(dtype)


def equal_linear(sd, prefix, x, lr_mul=1.0, activation=False):
    """EqualLinear.forward :234-244."""
    w = _w(sd, prefix + 'weight', x.dtype)
    b = _w(sd, prefix + 'bias', x.dtype)
    scale = (1 / math.sqrt(w.shape[1])) * lr_mul
    if activation:
        return fused_leaky_relu_ref(F.linear(x, w * scale), b * lr_mul)
    return F.linear(x, w * scale, bias=b * lr_mul)


def mapping_linear(sd, prefix, x):
    """MappingLinear.forward :70-77 with activation: linear without bias, then fused lrelu(scale=1)."""
    return fused_leaky_relu_ref(F.linear(x, _w(sd, prefix + 'weight', x.dtype)), _w(sd, prefix + 'bias', x.dtype), scale=1)


def renderer_mapping(sd, z, prefix='style.'):
    """Generator.style :822-830: three MappingLinear layers."""
    for i in range(3):
        z = mapping_linear(sd, f'{prefix}{i}.', z)
    return z


def decoder_mapping(sd, w, prefix='decoder.style.', lr_mul=0.01):
    """Decoder.style :596-611: PixelNorm + 5 EqualLinear(fused_lrelu)."""
    x = w * torch.rsqrt(torch.mean(w ** 2, dim=1, keepdim=True) + 1e-8)
    for i in range(1, 6):
        x = equal_linear(sd, f'{prefix}{i}.', x, lr_mul, activation=True)
    return x


def modulated_weights(weight, s, demodulate=True):
    """The per-sample kernels of ModulatedConv2d.forward: weight (1, Co, Ci, k, k), modulation s (B, Ci) ->
    (B, Co, Ci, k, k) = scale * weight * s (:321) [* rsqrt(sum over (Ci, k, k) of its square + 1e-8) (:325-326)]."""
    _, Co, Ci, k, _ = weight.shape
    B = s.shape[0]
    w = (1 / math.sqrt(Ci * k * k)) * weight * s.reshape(B, 1, Ci, 1, 1)
    if demodulate:
        w = w * torch.rsqrt(w.pow(2).sum([2, 3, 4]) + 1e-8).reshape(B, Co, 1, 1, 1)
    return w


def modulated_conv(sd, prefix, x, style, demodulate=True, upsample=False, blur_fir=None):
    """ModulatedConv2d.forward :317-362 (no downsample branch on this path).  blur_fir: the 4x4 kernel of the up-sampling layer's Blur
    (its registered buffer, gain included); None: make_kernel([1, 3, 3, 1]) * 4, what the module registers."""
    dt = x.dtype
    weight = _w(sd, prefix + 'weight', dt)                          # (1, Co, Ci, k, k)
    _, Co, Ci, k, _ = weight.shape
    B, _, H, W = x.shape
    s = equal_linear(sd, prefix + 'modulation.', style)             # bias_init 1 lives in the weights
    w = modulated_weights(weight, s, demodulate)
    if upsample:
        wt = w.transpose(1, 2).reshape(B * Ci, Co, k, k)            # :333-338
        out = F.conv_transpose2d(x.reshape(1, B * Ci, H, W), wt, padding=0, stride=2, groups=B)
        out = out.reshape(B, Co, out.shape[2], out.shape[3])
        p = (4 - 2) - (k - 1)                                       # :285-287
        k4 = fir(gain=4.0, dtype=dt) if blur_fir is None else blur_fir.to(dt)
        return upfirdn2d_ref_simple(out, k4, pad=((p + 1) // 2 + 1, p // 2 + 1))
    out = F.conv2d(x.reshape(1, B * Ci, H, W), w.reshape(B * Co, Ci, k, k), padding=k // 2, groups=B)
    return out.reshape(B, Co, out.shape[2], out.shape[3])


def styled_conv(sd, prefix, x, style, noise, upsample=False, blur_fir=None):
    """StyledConv.forward :494-507: mod-conv, + noise.weight * noise (:466), lrelu(x + activate.bias) * sqrt 2."""
    out = modulated_conv(sd, prefix + 'conv.', x, style, True, upsample, blur_fir)
    out = out + _w(sd, prefix + 'noise.weight', x.dtype) * noise.to(x.dtype)
    return fused_leaky_relu_ref(out, _w(sd, prefix + 'activate.bias', x.dtype))


def to_rgb(sd, prefix, x, style, skip=None, upsample=True, up_fir=None):
    """ToRGB.forward :531-541.  up_fir: the 4x4 kernel of its Upsample (the registered buffer, gain included); None:
    make_kernel([1, 3, 3, 1]) * 4."""
    out = modulated_conv(sd, prefix + 'conv.', x, style, demodulate=False) + _w(sd, prefix + 'bias', x.dtype)
    if skip is not None:
        if upsample:
            k4 = fir(gain=4.0, dtype=x.dtype) if up_fir is None else up_fir.to(x.dtype)
            skip = upfirdn2d_ref_simple(skip, k4, up=2, pad=(2, 1))                             # Upsample :96-119
        out = out + skip
    return out


def decoder_forward(sd, features, latent, noises=None, prefix='decoder.', dtype=torch.float32, blur_firs=None, up_firs=None):
    """Decoder.forward :742-797 with input_is_latent=True, randomize_noise=False (noise buffers) unless
    `noises` is given.  features (B,256,r,r), latent (B,n_latent,512).  blur_firs / up_firs: per level, the Blur kernel of the
    up-sampling layer and the Upsample kernel of the ToRGB (None: the default of modulated_conv / to_rgb)."""
    features, latent = features.to(dtype), latent.to(dtype)
    n_up = 0
    while f'{prefix}convs.{2 * n_up}.conv.weight' in sd:
        n_up += 1
    if noises is None:
        noises = [sd[f'{prefix}noises.noise_{i}'] for i in range(2 * n_up + 1)]
    out = styled_conv(sd, prefix + 'conv1.', features, latent[:, 0], noises[0])
    skip = to_rgb(sd, prefix + 'to_rgb1.', out, latent[:, 1], None, upsample=False)
    i = 1
    for u in range(n_up):                                           # :773-792
        out = styled_conv(sd, f'{prefix}convs.{2 * u}.', out, latent[:, i], noises[2 * u + 1], upsample=True,
                          blur_fir=None if blur_firs is None else blur_firs[u])
        out = styled_conv(sd, f'{prefix}convs.{2 * u + 1}.', out, latent[:, i + 1], noises[2 * u + 2])
        skip = to_rgb(sd, f'{prefix}to_rgbs.{u}.', out, latent[:, i + 2], skip, up_fir=None if up_firs is None else up_firs[u])
        i += 2
    return skip


def decoder_stages(sd, prefix='decoder.'):
    """The stages of decoder_forward in execution order: [(kind, layer prefix, latent row, upsample)], kind 'conv' (a styled_conv) or
    'rgb' (a to_rgb; its `upsample` says whether the previous skip image is FIR-up-sampled: not for to_rgb1, which has none)."""
    out = [('conv', prefix + 'conv1.', 0, False), ('rgb', prefix + 'to_rgb1.', 1, False)]
    u = 0
    while f'{prefix}convs.{2 * u}.conv.weight' in sd:
        out += [('conv', f'{prefix}convs.{2 * u}.', 2 * u + 1, True), ('conv', f'{prefix}convs.{2 * u + 1}.', 2 * u + 2, False),
                ('rgb', f'{prefix}to_rgbs.{u}.', 2 * u + 3, True)]
        u += 1
    return out


def decoder_stage(sd, stage, x, style, other, dtype=torch.float32, fir=None):
    """ONE stage of decoder_forward (an entry of decoder_stages) in `dtype` on GIVEN inputs: the input activation x, the stage's latent
    row `style` (B, 512), and `other`: the noise image of a 'conv', the previous skip image (or None) of an 'rgb'.  Chained over
    decoder_stages with its own outputs it is decoder_forward, operation for operation.  fir: the stage's own 4x4 kernel (the Blur of an
    up-sampling 'conv', the Upsample of an 'rgb'); None: the default."""
    kind, p, _, upsample = stage
    x, style = x.to(dtype), style.to(dtype)
    if kind == 'conv':
        return styled_conv(sd, p, x, style, other, upsample=upsample, blur_fir=fir)
    return to_rgb(sd, p, x, style, None if other is None else other.to(dtype), upsample=upsample, up_fir=fir)


def decoder_modulations(sd, latent, prefix='decoder.', dtype=torch.float32):
    """[(s, demod)] of every modulated layer in execution order (decoder_stages): s (B, Ci) = the modulation output (equal_linear of the
    layer's latent row); demod (B, Co) = rsqrt(sum over (Ci, k, k) of (scale W s)^2 + 1e-8) for the 3x3 layers (ModulatedConv2d.forward
    :321-326, as modulated_weights applies it), None for the ToRGB layers (no demodulation)."""
    latent = latent.to(dtype)
    out = []
    for kind, p, row, _ in decoder_stages(sd, prefix):
        s = equal_linear(sd, p + 'conv.modulation.', latent[:, row])
        demod = None
        if kind == 'conv':
            weight = _w(sd, p + 'conv.weight', dtype)
            _, _, Ci, k, _ = weight.shape
            w = (1 / math.sqrt(Ci * k * k)) * weight * s.reshape(s.shape[0], 1, Ci, 1, 1)
            demod = torch.rsqrt(w.pow(2).sum([2, 3, 4]) + 1e-8)
        out.append((s, demod))
    return out


def decoder_pinned_backward(sd, features, latent, noises, d_img, masks=None, prefix='decoder.', dtype=torch.float64, blur_firs=None,
                            up_firs=None):
    """decoder_forward and its autograd with the branch of every leaky relu PINNED: StyledConv i (conv1, then up / conv per level)
    computes pre = modulated_conv + noise.weight * noise + activate.bias and returns where(masks[i], pre, 0.2 pre) * sqrt 2, masks[i] a
    boolean tensor of pre's shape (None: pre > 0, the function's own branch -- then this is decoder_forward).  With the masks of the
    implementation under test the step function lrelu' is the same on both sides of a comparison, and what is left is arithmetic: in
    float64 this is the truth for that implementation's gradients, in float32 the yardstick of what fp32 arithmetic can reach.
    On the CPU, in `dtype`.  Returns img, d_features, d_latent (gradients of sum(img * d_img)), d_pre (one per StyledConv), signs
    (pre > 0 per StyledConv) and styles (the modulation output s (B, Ci) of every StyledConv).  blur_firs / up_firs: as decoder_forward."""
    cpu = lambda t: t.detach().cpu()
    sd = {k: cpu(v) for k, v in sd.items() if k.startswith(prefix)}
    f = cpu(features).to(dtype).requires_grad_(True)
    lat = cpu(latent).to(dtype).requires_grad_(True)
    noises = [cpu(n).to(dtype) for n in noises]
    n_up = 0
    while f'{prefix}convs.{2 * n_up}.conv.weight' in sd:
        n_up += 1
    pres, styles = [], []

    def styled(p, x, style, noise, upsample=False, blur_fir=None):
        pre = modulated_conv(sd, p + 'conv.', x, style, True, upsample, blur_fir)
        pre = pre + _w(sd, p + 'noise.weight', dtype) * noise + _w(sd, p + 'activate.bias', dtype).reshape(1, -1, 1, 1)
        pre.retain_grad()
        m = pre.detach() > 0 if masks is None else cpu(masks[len(pres)])
        assert m.dtype == torch.bool and m.shape == pre.shape, (m.dtype, tuple(m.shape), tuple(pre.shape))
        pres.append(pre)
        styles.append(equal_linear(sd, p + 'conv.modulation.', style.detach()))
        return torch.where(m, pre, 0.2 * pre) * (2 ** 0.5)
    out = styled(prefix + 'conv1.', f, lat[:, 0], noises[0])
    skip = to_rgb(sd, prefix + 'to_rgb1.', out, lat[:, 1], None, upsample=False)
    i = 1
    for u in range(n_up):
        out = styled(f'{prefix}convs.{2 * u}.', out, lat[:, i], noises[2 * u + 1], upsample=True,
                     blur_fir=None if blur_firs is None else blur_firs[u])
        out = styled(f'{prefix}convs.{2 * u + 1}.', out, lat[:, i + 1], noises[2 * u + 2])
        skip = to_rgb(sd, f'{prefix}to_rgbs.{u}.', out, lat[:, i + 2], skip, up_fir=None if up_firs is None else up_firs[u])
        i += 2
    skip.backward(cpu(d_img).to(dtype))
    return dict(img=skip.detach(), d_features=f.grad, d_latent=lat.grad, d_pre=[p.grad for p in pres],
                signs=[p.detach() > 0 for p in pres], styles=styles)
