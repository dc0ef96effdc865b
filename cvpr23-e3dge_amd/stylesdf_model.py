"""StyleSDF generator glue on the gfx950 ops -- host-side mirror of project/models/stylesdf_model.py:30-1172.

Kept from the reference: class names, constructor arguments, parameter / buffer names (so the `g_ema` state
dict loads unchanged: `style.{0,1,2}.*`, `renderer.*`, `decoder.style.*`, `decoder.conv1.{conv.weight,
conv.modulation.*, noise.weight, bias, activate.bias}`, `decoder.convs.{i}.*`, `decoder.to_rgb1/to_rgbs.{i}.*`,
`decoder.noises.noise_{i}`; blur kernels are buffers) and the `G_pred_latents.forward` keyword surface that
`trainer.py:881-897` drives.

What runs where: Decoder.forward without an autograd graph is ONE native call (e3dge_dec2_forward, csrc/decoder2.hip):
activations stay in the split-f16 packed layout of the matrix pipe between the kernels, the 3x3 modulated convolutions,
the blur, ToRGB and the modulation GEMVs are hand-written HIP kernels.  `E3DGE_DECODER=planar` keeps the round-2 path
(fp32 planes between fused kernels, e3dge_modconv3x3 etc.); anything that needs an autograd graph through the decoder
uses weight modulation as a HIP launch (e3dge_modconv_weights) + library convolutions (MIOpen through torch).
The StyleGAN2 `Discriminator` (:1514-1617) lives in e3dge_amd.discriminator and the camera-pose predictor `VolumeRenderDiscriminator` with
its building blocks (:1193-1419) in e3dge_amd.volume_discriminator; its encoder variants `VolumeRenderDiscriminatorEncoder` and
`VolumeStyleEncoder` (:1422-1510) and the legacy encoders (:1620-1765) are out of scope.
"""
import ctypes
import math
import os
import random
import types

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import _lib, mesh_utils
from .op import FusedLeakyReLU, fused_leaky_relu, noise_bias_act, upfirdn2d
from .volume_renderer import VolumeFeatureRenderer, _opt_get


class PixelNorm(nn.Module):
    def forward(self, input):
        return input * torch.rsqrt(torch.mean(input ** 2, dim=1, keepdim=True) + 1e-8)


class MappingLinear(nn.Module):
    """Renderer mapping-network layer (reference :40-82): linear, then fused lrelu with scale=1 (:73)."""

    def __init__(self, in_dim, out_dim, bias=True, activation=None, is_last=False):
        super().__init__()
        std = 0.25 if is_last else 1
        self.weight = nn.Parameter(std * nn.init.kaiming_normal_(torch.empty(out_dim, in_dim), a=0.2, mode='fan_in',
                                                                nonlinearity='leaky_relu'))
        lim = np.sqrt(1 / in_dim)
        self.bias = nn.Parameter(torch.empty(out_dim).uniform_(-lim, lim)) if bias else None
        self.activation = activation

    def forward(self, input):
        if self.activation is not None:
            return fused_leaky_relu(F.linear(input, self.weight), self.bias, scale=1)
        return F.linear(input, self.weight, bias=self.bias)


def make_kernel(k):
    k = torch.tensor(k, dtype=torch.float32)
    if k.ndim == 1:
        k = k[None, :] * k[:, None]
    return k / k.sum()


def _fir_pads(taps, factor, conv_kernel=None, mode='up'):
    """The pad arithmetic of the reference's Upsample / Downsample / ModulatedConv2d blurs (:105-110,
    :131-136, :283-299)."""
    if conv_kernel is None:                       # plain Upsample / Downsample
        p = taps - factor
        return ((p + 1) // 2 + factor - 1, p // 2) if mode == 'up' else ((p + 1) // 2, p // 2)
    if mode == 'up':                              # blur after a stride-2 transposed conv
        p = (taps - factor) - (conv_kernel - 1)
        return ((p + 1) // 2 + factor - 1, p // 2 + 1)
    p = (taps - factor) + (conv_kernel - 1)       # blur before a stride-2 conv
    return ((p + 1) // 2, p // 2)


class Upsample(nn.Module):
    def __init__(self, kernel, factor=2):
        super().__init__()
        self.factor = factor
        self.register_buffer("kernel", make_kernel(kernel) * (factor ** 2))
        self.pad = _fir_pads(self.kernel.shape[0], factor, mode='up')

    def forward(self, input):
        return upfirdn2d(input, self.kernel, up=self.factor, down=1, pad=self.pad)


class Downsample(nn.Module):
    def __init__(self, kernel, factor=2):
        super().__init__()
        self.factor = factor
        self.register_buffer("kernel", make_kernel(kernel))
        self.pad = _fir_pads(self.kernel.shape[0], factor, mode='down')

    def forward(self, input):
        return upfirdn2d(input, self.kernel, up=1, down=self.factor, pad=self.pad)


class Blur(nn.Module):
    def __init__(self, kernel, pad, upsample_factor=1):
        super().__init__()
        kernel = make_kernel(kernel)
        if upsample_factor > 1:
            kernel = kernel * (upsample_factor ** 2)
        self.register_buffer("kernel", kernel)
        self.pad = pad

    def forward(self, input):
        return upfirdn2d(input, self.kernel, pad=self.pad)


class EqualLinear(nn.Module):
    """Reference :210-249 (weight stored / lr_mul, runtime scale 1/sqrt(in) * lr_mul)."""

    def __init__(self, in_dim, out_dim, bias=True, bias_init=0, lr_mul=1, activation=None):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(out_dim, in_dim).div_(lr_mul))
        self.bias = nn.Parameter(torch.zeros(out_dim).fill_(bias_init)) if bias else None
        self.activation = activation
        self.scale = (1 / math.sqrt(in_dim)) * lr_mul
        self.lr_mul = lr_mul

    def forward(self, input):
        if self.activation:
            return fused_leaky_relu(F.linear(input, self.weight * self.scale), self.bias * self.lr_mul)
        return F.linear(input, self.weight * self.scale, bias=self.bias * self.lr_mul)


import weakref

_DEC2_NOISE_AMAX = weakref.WeakKeyDictionary()      # Decoder -> {noise tensor version: amax buffer}
_DEC2_STATES = types.SimpleNamespace(get=lambda dec: _lib.latest(dec, 'dec2_state'))   # (tests ask whether a decoder has built a plan)


def blur_factor(kernel):
    """(g0, g1, g1, g0) when the 4x4 blur kernel is outer(g, g) with a symmetric g up to fp32 round-off (make_kernel([1,3,3,1])
    * 4 is), else None.  The packed decoder's up-sampling kernel applies the blur as these two 1-D passes."""
    k2 = kernel.detach().double().cpu()
    tot = float(k2.sum())
    if tuple(k2.shape) != (4, 4) or not tot > 0:
        return None
    g = k2.sum(1) / tot ** 0.5
    kmax = float(k2.abs().max())
    if not (float((torch.outer(g, g) - k2).abs().max()) <= 1e-6 * kmax and float((k2 - k2.t()).abs().max()) <= 1e-6 * kmax and
            float((g - g.flip(0)).abs().max()) <= 1e-7 * float(g.abs().max())):
        return None
    return tuple(float(v) for v in g)


def decoder_backend():
    """'packed' (default): Decoder.forward without an autograd graph runs as one native call on split-f16 packed activations
    (e3dge_dec2_forward).  E3DGE_DECODER=planar keeps the round-2 chain of fused kernels over fp32 planes."""
    v = os.environ.get("E3DGE_DECODER", "packed")
    if v not in ("packed", "planar"):
        raise RuntimeError(f"E3DGE_DECODER must be 'packed' or 'planar', got {v!r}")
    return v


def decoder_autograd_backend():
    """What Decoder.forward does when an autograd graph is wanted through it (features / latent / parameters require grad):
    'auto' (default): when the feature map and / or the decoder latent need a gradient and no decoder parameter does (generator frozen:
    train_ae.py's stage-1 step, trainer.py:1017-1031, where the encoder predicts both latents, :881-897) the packed forward
    (e3dge_dec2_forward) runs inside an autograd.Function whose backward is the packed pipeline's own e3dge_dec2_backward
    (csrc/decoder2_bwd.h: d features, and d latent from per-channel sums unless E3DGE_DEC2_DLATENT=0); a decoder parameter that
    requires grad takes the library path (weight modulation + MIOpen) for both directions.
    'packed': always the packed forward; the backward is native when eligible, otherwise it recomputes the library path under
    enable_grad and differentiates that (for passes that run with grad enabled but never call backward).
    'library': the library path for both directions (round 4's default; A/B).  The packed node's native backward is first-order only: a
    backward taken with create_graph=True (a second differentiation through the decoder; not something the reference's encoder training
    does) is re-routed by the node itself to the library path, whose custom ops are twice differentiable as the reference's are
    (round 6; it raised before).  Parameter writes through `.data` between a forward and its backward bump no version counter and are
    not seen by either path: call `Decoder.invalidate()` (or `Generator.invalidate()`) and run the forward again."""
    v = os.environ.get("E3DGE_DECODER_AUTOGRAD", "auto")
    if v not in ("auto", "packed", "library"):
        raise RuntimeError(f"E3DGE_DECODER_AUTOGRAD must be 'auto', 'packed' or 'library', got {v!r}")
    return v


class _PackedDecoderFn(torch.autograd.Function):
    """Decoder.forward as one native call (packed pipeline) that stays inside an autograd graph (reference: stylesdf_model.py:317-362,
    741-797).  backward, when only d features / d latent are wanted (generator frozen): e3dge_dec2_backward on the activations the forward
    left in its workspace -- if another forward has used the workspace since, the packed forward is re-run first (0.65 ms at 1024^2).
    Otherwise (parameter gradients, or d latent with E3DGE_DEC2_DLATENT=0): the same forward is re-run on the library path (every op differentiable) with the
    saved inputs and the SAME noise, and `torch.autograd.grad` of that graph gives the gradients.  A backward under create_graph=True takes
    that library route too, with the graph kept (round 6)."""

    @staticmethod
    def forward(ctx, dec, noise, features, latent, *params):
        ctx.dec, ctx.noise, ctx.n_params = dec, noise, len(params)
        ctx.save_for_backward(features, latent)
        need = ctx.needs_input_grad
        ctx.native = dec._dec2_bwd_ok() and not any(need[4:]) and (not need[3] or decoder_dlatent_native())
        with torch.no_grad():
            img = dec._forward_packed(features, latent, noise, save=ctx.native)
        if ctx.native:
            ctx.gen = dec.__dict__['_dec2_gen']
        return img

    @staticmethod
    def backward(ctx, d_img):
        features, latent = ctx.saved_tensors
        dec = ctx.dec
        need = ctx.needs_input_grad
        if torch.is_grad_enabled():
            # create_graph=True: this backward is itself being recorded (a path-length / R1-type penalty through the frozen decoder).  The
            # native chain is first-order only, so the pass is re-routed to the library path, whose custom ops are twice differentiable
            # as the reference's are (op/fused_act.py:19-84, op/upfirdn2d.py:18-142): the forward is recomputed from the ORIGINAL inputs
            # (their graph stays attached) and differentiated with create_graph=True.
            params = [p for p in dec.parameters()]
            img = dec._forward_layers(features, latent, ctx.noise, None)
            wrt_all = [features, latent] + params
            want = [bool(n) and t.requires_grad for n, t in zip(need[2:], wrt_all)]
            wrt = [t for t, w_ in zip(wrt_all, want) if w_]
            grads = list(torch.autograd.grad(img, wrt, d_img, create_graph=True, allow_unused=True)) if wrt else []
            return (None, None) + tuple(grads.pop(0) if w_ else None for w_ in want)
        if ctx.native:
            d_feat = d_lat = None
            if need[2] or need[3]:
                with torch.no_grad():
                    if dec.__dict__.get('_dec2_gen') != ctx.gen:          # somebody else ran a forward on this decoder since
                        dec._forward_packed(features, latent, ctx.noise, save=True)
                    d_feat, d_lat = dec._backward_packed(features, d_img, want_latent=need[3], latent_shape=latent.shape)
            return (None, None, d_feat if need[2] else None, d_lat) + (None,) * ctx.n_params
        params = [p for p in dec.parameters()]
        with torch.enable_grad():
            f_ = features.detach().requires_grad_(need[2])
            l_ = latent.detach().requires_grad_(need[3])
            img = dec._forward_layers(f_, l_, ctx.noise, None)
            wrt = [t for t in (f_, l_) if t.requires_grad] + [p for p, n in zip(params, need[4:]) if n]
            grads = list(torch.autograd.grad(img, wrt, d_img.contiguous(), allow_unused=True)) if wrt else []
        out = [None, None]
        out.append(grads.pop(0) if need[2] else None)
        out.append(grads.pop(0) if need[3] else None)
        for n in need[4:]:
            out.append(grads.pop(0) if n else None)
        return tuple(out)


def decoder_dlatent_native():
    """E3DGE_DEC2_DLATENT=0: a decoder latent that requires grad takes the library path (round 4); default: e3dge_dec2_backward also
    returns d latent (per-channel sums over the tensors its chain leaves behind + modulation^T, csrc/decoder2_bwd.h)."""
    return os.environ.get("E3DGE_DEC2_DLATENT", "1") != "0"


def modconv_backend():
    """'hip' (default): 3x3 modulated convolutions run on the fused implicit-GEMM kernel e3dge_modconv3x3.
    E3DGE_MODCONV=library keeps the previous path (e3dge_modconv_weights + MIOpen convolution through torch)."""
    v = os.environ.get("E3DGE_MODCONV", "hip")
    if v not in ("hip", "library"):
        raise RuntimeError(f"E3DGE_MODCONV must be 'hip' or 'library', got {v!r}")
    return v


class ModulatedConv2d(nn.Module):
    """Reference :263-362.  3x3 layers on the inference path: one fused HIP launch (e3dge_modconv3x3) -- no per-sample
    weights, modulation applied to the staged input, demodulation (+ noise, bias, lrelu for StyledConv) in the epilogue.
    Other cases (1x1 ToRGB, down-sampling, anything under autograd): weight modulation + demodulation as one HIP launch
    (e3dge_modconv_weights) that writes the per-sample weights in the grouped-conv layout, then a library convolution."""

    def __init__(self, in_channel, out_channel, kernel_size, style_dim, demodulate=True, upsample=False,
                 downsample=False, blur_kernel=[1, 3, 3, 1]):
        super().__init__()
        self.eps = 1e-8
        self.kernel_size = kernel_size
        self.in_channel = in_channel
        self.out_channel = out_channel
        self.upsample = upsample
        self.downsample = downsample
        if upsample:
            self.blur = Blur(blur_kernel, pad=_fir_pads(len(blur_kernel), 2, kernel_size, 'up'), upsample_factor=2)
        if downsample:
            self.blur = Blur(blur_kernel, pad=_fir_pads(len(blur_kernel), 2, kernel_size, 'down'))
        self.scale = 1 / math.sqrt(in_channel * kernel_size ** 2)
        self.padding = kernel_size // 2
        self.weight = nn.Parameter(torch.randn(1, out_channel, in_channel, kernel_size, kernel_size))
        self.modulation = EqualLinear(style_dim, in_channel, bias_init=1)
        self.demodulate = demodulate

    def _weights(self, s, transpose):
        """s (B, Ci) -> (B*Co, Ci, k, k) or, transposed, (B*Ci, Co, k, k)."""
        B = s.shape[0]
        Co, Ci, k = self.out_channel, self.in_channel, self.kernel_size
        needs_graph = torch.is_grad_enabled() and (s.requires_grad or self.weight.requires_grad)
        if needs_graph:   # autograd path: same arithmetic as GPU torch ops (training through the decoder)
            w = self.scale * self.weight * s.reshape(B, 1, Ci, 1, 1)
            if self.demodulate:
                w = w * torch.rsqrt(w.pow(2).sum([2, 3, 4]) + 1e-8).reshape(B, Co, 1, 1, 1)
            if transpose:
                return w.transpose(1, 2).reshape(B * Ci, Co, k, k)
            return w.reshape(B * Co, Ci, k, k)
        _lib.require_gpu(s, "style")
        out = torch.empty((B * Ci, Co, k, k) if transpose else (B * Co, Ci, k, k), device=s.device, dtype=torch.float32)
        wt = self.weight.detach().contiguous()
        sc = s.contiguous()
        _lib.launch("e3dge_modconv_weights", out, wt, sc, float(self.scale), int(self.demodulate), int(transpose), B, Co, Ci, k * k)
        return out

    # ---- fused path --------------------------------------------------------------------------------------------
    def fused_ok(self, input, style=None):
        """3x3, no down-sampling, fp32 GPU tensors, channel counts the tiles cover, and no autograd graph needed: the
        fused kernels write into fresh buffers without a grad_fn, so anything that requires grad -- the input, the weights,
        the modulation layer, or the STYLE (latent optimisation with a frozen decoder) -- takes the library path."""
        if self.kernel_size != 3 or self.downsample or modconv_backend() != "hip":
            return False
        if input.device.type != "cuda" or input.dtype != torch.float32:
            return False
        if self.in_channel % 16 or self.out_channel % 32:
            return False
        if torch.is_grad_enabled() and (input.requires_grad or self.weight.requires_grad or
                                        self.modulation.weight.requires_grad or
                                        (self.modulation.bias is not None and self.modulation.bias.requires_grad) or
                                        (style is not None and style.requires_grad)):
            return False
        return True

    def invalidate(self):
        """Drop the packed weight images (needed after writes through `.data`; see SirenGenerator.invalidate)."""
        _lib.invalidate(self)

    def device_wpre_t(self):
        """scale * W in the TRANSPOSED fragment order (rows = input channels, taps flipped for the stride-1 layers): what the
        backward's weights launch streams (e3dge_dec2_prepack_weights_t; the data gradient of :331-361 of the reference)."""
        w = self.weight

        def build():
            Co, Ci = self.out_channel, self.in_channel
            wpre = torch.empty(Co * Ci * 9, device=w.device, dtype=torch.float32)
            wc = w.detach().reshape(Co, Ci, 9).contiguous()
            _lib.launch("e3dge_dec2_prepack_weights_t", wpre, wc, float(self.scale), Co, Ci, 0 if self.upsample else 1)
            return wpre
        return _lib.cached(self, 'wpre_t', (w,), build)

    def device_wpre(self):
        """scale * W re-arranged in MFMA A-fragment element order (fp32): what the per-forward weights launch of the packed
        decoder pipeline streams (e3dge_dec2_prepack_weights)."""
        w = self.weight

        def build():
            Co, Ci = self.out_channel, self.in_channel
            wpre = torch.empty(Co * Ci * 9, device=w.device, dtype=torch.float32)
            wc = w.detach().reshape(Co, Ci, 9).contiguous()
            _lib.launch("e3dge_dec2_prepack_weights", wpre, wc, float(self.scale), Co, Ci)
            return wpre
        return _lib.cached(self, 'wpre', (w,), build)

    def device_image(self):
        """(image, wsq): the MFMA fragment image of scale * W (f16 hi/lo) and the per-(co,ci) squared norms."""
        w = self.weight

        def build():
            lib = _lib.load()
            Co, Ci = self.out_channel, self.in_channel
            img = torch.empty(lib.e3dge_modconv_packed_words(Co, Ci), device=w.device, dtype=torch.int32)
            wsq = torch.empty((Co, Ci), device=w.device, dtype=torch.float32)
            wc = w.detach().reshape(Co, Ci, 9).contiguous()
            _lib.launch("e3dge_modconv_pack_weights", img, wsq, wc, float(self.scale), Co, Ci)
            wmax = float(wc.abs().max().item()) * self.scale
            if wmax >= 400.0:                      # the image stores 128 * scale * w as f16
                raise RuntimeError(f"modulated-conv weights up to {wmax:g} (after the 1/sqrt(fan_in) scale) do not fit the "
                                   "f16 image; set E3DGE_MODCONV=library for this checkpoint")
            return img, wsq
        return _lib.cached(self, 'image', (w,), build)

    def forward_fused(self, input, style, noise=None, noise_weight=None, bias=None, negative_slope=0.2, act_scale=1.0,
                      act=False, in_amax=None, out_amax=None, pre=None):
        """The conv (stride-1: with StyledConv's tail when act=True; up-sampling: the transposed conv, BEFORE the blur).
        in_amax / out_amax: amax buffers (_lib.AMAX_FLOATS floats, include/e3dge_hip.h): max|input| as tracked by the
        producer of `input` (computed here with e3dge_amax when not supplied) / zero-initialised buffer receiving max|output|."""
        B, Ci, H, W = input.shape
        x = _lib.dense(input)
        img, wsq = self.device_image()
        dev = x.device
        if pre is not None:           # (s, demod, s_amax) from Decoder's e3dge_decoder_styles launch
            s, demod, s_amax = pre
        else:
            s = self.modulation(style.contiguous()).contiguous()     # (the library GEMM rounds a transposed operand differently: one layout in)
            demod = torch.empty((B, self.out_channel), device=dev, dtype=torch.float32) if self.demodulate else None
            s_amax = torch.empty(B, device=dev, dtype=torch.float32)
        OH, OW = (2 * H + 1, 2 * W + 1) if self.upsample else (H, W)
        y = torch.empty((B, self.out_channel, OH, OW), device=dev, dtype=torch.float32)
        nz = None
        if noise is not None:
            nz = noise.contiguous()
            if nz.shape[0] not in (1, B) or nz.numel() != nz.shape[0] * OH * OW:
                raise RuntimeError(f"noise must be (1|B, 1, {OH}, {OW}); got {tuple(noise.shape)}")
        if pre is None:
            _lib.launch("e3dge_modconv_demod", demod, s_amax, s, wsq, B, self.out_channel, Ci, int(self.demodulate))
        if in_amax is None:       # the producer of `input` did not track max|input|: one extra pass over it
            in_amax = torch.zeros(_lib.AMAX_FLOATS, device=dev, dtype=torch.float32)
            _lib.launch("e3dge_amax", in_amax, x, x.numel())
        a = _lib.ModconvArgs(x=x, wimg=img, style=s, demod=demod, in_amax=in_amax, s_amax=s_amax, noise=nz,
                             noise_w=noise_weight if nz is not None else None, bias=bias, y=y, out_amax=out_amax,
                             negative_slope=float(negative_slope), act_scale=float(act_scale), act=int(bool(act)),
                             upsample=int(bool(self.upsample)), batch=B, ci=Ci, co=self.out_channel, height=H, width=W,
                             noise_batch=0 if nz is None else nz.shape[0])
        _lib.launch("e3dge_modconv3x3", a)
        return y

    def forward(self, input, style):
        B, Ci, H, W = input.shape
        if self.fused_ok(input, style):
            out = self.forward_fused(input, style)
            return self.blur(out) if self.upsample else out
        s = self.modulation(style.contiguous())
        if self.upsample:
            w = self._weights(s, transpose=True)
            out = F.conv_transpose2d(input.reshape(1, B * Ci, H, W), w, padding=0, stride=2, groups=B)
            out = out.reshape(B, self.out_channel, out.shape[2], out.shape[3])
            return self.blur(out)
        w = self._weights(s, transpose=False)
        if self.downsample:
            input = self.blur(input)
            H, W = input.shape[2:]
            out = F.conv2d(input.reshape(1, B * Ci, H, W), w, padding=0, stride=2, groups=B)
        else:
            out = F.conv2d(input.reshape(1, B * Ci, H, W), w, padding=self.padding, groups=B)
        return out.reshape(B, self.out_channel, out.shape[2], out.shape[3])


class NoiseInjection(nn.Module):
    """Parameter holder (`weight`, zero-initialised, reference :365-370); StyledConv fuses its arithmetic
    into the activation kernel.  `project=True` (reference :375-457): a given noise map is replaced by per-vertex noise of the
    extracted surface seen from the frame's camera, so that the texture noise stays on the surface when the view changes.  The
    projection state -- `vert_noise` (V,) on the mesh's device, drawn once per vertex count on the CPU with torch's global generator;
    `prev_noise`, the first call's map, which fills the pixels the mesh does not cover ever after; `mesh_fn` -- are plain attributes,
    not buffers: the state dict is the reference's."""

    def __init__(self, project=False):
        super().__init__()
        self.project = project
        self.weight = nn.Parameter(torch.zeros(1))
        self.prev_noise = None
        self.mesh_fn = None
        self.vert_noise = None

    def projection_inputs(self, noise, mesh_path):
        """The reference's bookkeeping around the rendering (:383-386, :423-425, :442-452): (verts, faces) of the mesh at the level of
        the map's size, this module's vertex noise (V,) and the map (1, S, S) that fills what the mesh does not cover."""
        if noise.dim() != 4 or noise.shape[1] != 1 or noise.shape[2] != noise.shape[3]:
            raise RuntimeError(f"project_noise expects a (1, 1, S, S) noise map, got {tuple(noise.shape)}")
        if noise.shape[0] != 1:
            raise AssertionError(f"project_noise assumes batch size 1 at inference, got a noise map of batch {noise.shape[0]}")
        self.mesh_fn = mesh_path
        verts, faces = mesh_utils.load_mesh(mesh_path, device=noise.device).for_image(noise.shape[2])
        if self.vert_noise is None or self.vert_noise.shape[0] != verts.shape[0]:
            self.vert_noise = torch.empty(verts.shape[0], 1).normal_()[:, 0].to(verts.device)      # (V, 1) on the CPU, as the reference draws
        if self.prev_noise is None:
            self.prev_noise = noise
        return verts, faces, self.vert_noise, self.prev_noise.reshape(1, noise.shape[2], noise.shape[3])

    def project_noise(self, noise, transform, mesh_path=None):
        """The reference's project_noise (:423-457): (1, 1, S, S)."""
        verts, faces, vert_noise, prev = self.projection_inputs(noise, mesh_path)
        maps, _ = mesh_utils.project_vertex_noise(verts, faces, vert_noise, mesh_utils.noise_camera(transform), noise.shape[2], prev=prev)
        return maps.unsqueeze(0)

    def forward(self, image, noise=None, transform=None, mesh_path=None):
        if noise is None:
            B, _, H, W = image.shape
            noise = image.new_empty(B, 1, H, W).normal_()
        elif self.project:
            noise = self.project_noise(noise, transform, mesh_path=mesh_path)
        return noise_bias_act(image, noise, self.weight, None, negative_slope=1.0, scale=1.0)


class StyledConv(nn.Module):
    """mod-conv -> + noise.weight * noise -> lrelu(x + activate.bias, 0.2) * sqrt(2)  (reference :469-507);
    the last two are ONE pass over the activation (e3dge_noise_bias_act)."""

    def __init__(self, in_channel, out_channel, kernel_size, style_dim, upsample=False, blur_kernel=[1, 3, 3, 1],
                 project_noise=False):
        super().__init__()
        self.conv = ModulatedConv2d(in_channel, out_channel, kernel_size, style_dim, upsample=upsample,
                                    blur_kernel=blur_kernel)
        self.noise = NoiseInjection(project=project_noise)
        self.bias = nn.Parameter(torch.zeros(1, out_channel, 1, 1))   # unused by forward, as in the reference (:491)
        self.activate = FusedLeakyReLU(out_channel)

    def forward(self, input, style, noise=None, transform=None, mesh_path=None, in_amax=None, out_amax=None, pre=None):
        conv = self.conv
        if conv.fused_ok(input, style) and not (torch.is_grad_enabled() and (self.noise.weight.requires_grad or
                                                                             self.activate.bias.requires_grad)):
            B, _, H, W = input.shape
            OH, OW = (2 * H, 2 * W) if conv.upsample else (H, W)
            if noise is None:
                noise = input.new_empty(B, 1, OH, OW).normal_()
            act = self.activate
            if not conv.upsample:     # conv + noise + bias + lrelu: one launch
                return conv.forward_fused(input, style, noise=noise, noise_weight=self.noise.weight, bias=act.bias,
                                          negative_slope=act.negative_slope, act_scale=act.scale, act=True, in_amax=in_amax,
                                          out_amax=out_amax, pre=pre)
            # transposed conv by output phase, then blur + noise + bias + lrelu in one pass
            t = conv.forward_fused(input, style, in_amax=in_amax, pre=pre)
            nz = noise.contiguous()
            if nz.shape[0] not in (1, B) or nz.numel() != nz.shape[0] * OH * OW:
                raise RuntimeError(f"noise must be (1|B, 1, {OH}, {OW}); got {tuple(noise.shape)}")
            y = torch.empty((B, conv.out_channel, OH, OW), device=input.device, dtype=torch.float32)
            k = conv.blur.kernel
            _lib.launch("e3dge_blur_noise_bias_act", y, t, k, nz, self.noise.weight, act.bias, float(act.negative_slope),
                        float(act.scale), B, conv.out_channel, t.shape[2], t.shape[3], int(conv.blur.pad[0]), int(conv.blur.pad[1]),
                        nz.shape[0], out_amax)
            return y
        out = conv(input, style)
        if noise is None:
            B, _, H, W = out.shape
            noise = out.new_empty(B, 1, H, W).normal_()
        out = noise_bias_act(out, noise, self.noise.weight, self.activate.bias, self.activate.negative_slope,
                             self.activate.scale)
        if out_amax is not None and out.device.type == "cuda":   # a fused consumer follows: it needs max|out|
            oc = out.detach().contiguous()
            _lib.launch("e3dge_amax", out_amax, oc, oc.numel())
        return out


class ToRGB(nn.Module):
    """1x1 modulated conv without demodulation + bias + FIR-up-sampled skip (reference :510-541)."""

    def __init__(self, in_channel, style_dim, upsample=True, blur_kernel=[1, 3, 3, 1]):
        super().__init__()
        self.upsample = Upsample(blur_kernel) if upsample else upsample
        self.conv = ModulatedConv2d(in_channel, 3, 1, style_dim, demodulate=False)
        self.bias = nn.Parameter(torch.zeros(1, 3, 1, 1))

    def fused_ok(self, input, skip, style=None):
        if modconv_backend() != "hip" or input.device.type != "cuda" or input.dtype != torch.float32:
            return False
        if input.shape[3] % 4 or self.conv.in_channel > 1024:
            return False
        if skip is not None and (not self.upsample or tuple(skip.shape[2:]) != (input.shape[2] // 2, input.shape[3] // 2)
                                 or input.shape[2] % 2):
            return False
        mod = self.conv.modulation
        if torch.is_grad_enabled() and (input.requires_grad or self.bias.requires_grad or self.conv.weight.requires_grad or
                                        (skip is not None and skip.requires_grad) or mod.weight.requires_grad or
                                        (mod.bias is not None and mod.bias.requires_grad) or
                                        (style is not None and style.requires_grad)):
            return False
        return True

    def forward(self, input, style, skip=None, pre=None):
        if self.fused_ok(input, skip, style):
            # 1x1 modulated conv (no demodulation) + bias + FIR-up-sampled skip: one HBM pass (e3dge_torgb)
            B, Ci, H, W = input.shape
            x = _lib.dense(input)                     # (e3dge_torgb requires 16-byte x / y)
            s = pre[0] if pre is not None else self.conv.modulation(style.contiguous()).contiguous()
            w = self.conv.weight.detach().reshape(3, Ci).contiguous()
            y = torch.empty((B, 3, H, W), device=x.device, dtype=torch.float32)
            sk = None if skip is None else skip.contiguous()
            _lib.launch("e3dge_torgb", y, x, w, s, self.bias.detach().reshape(3).contiguous(), sk,
                        self.upsample.kernel if sk is not None else None, float(self.conv.scale), B, Ci, H, W)
            return y
        out = self.conv(input, style) + self.bias
        if skip is not None:
            if self.upsample:
                skip = self.upsample(skip)
            out = out + skip
        return out


class Decoder(nn.Module):
    """64x64x256 feature map -> size x size RGB (reference :587-797)."""

    def __init__(self, model_opt, blur_kernel=[1, 3, 3, 1]):
        super().__init__()
        self.size = model_opt.size
        self.style_dim = model_opt.style_dim * 2
        in_res = model_opt.renderer_spatial_output_dim
        lr_map = model_opt.lr_mapping
        layers = [PixelNorm(), EqualLinear(self.style_dim // 2, self.style_dim, lr_mul=lr_map, activation="fused_lrelu")]
        layers += [EqualLinear(self.style_dim, self.style_dim, lr_mul=lr_map, activation="fused_lrelu")
                   for _ in range(4)]
        self.style = nn.Sequential(*layers)
        cm = model_opt.channel_multiplier
        self.channels = {4: 512, 8: 512, 16: 512, 32: 512, 64: 256 * cm, 128: 128 * cm, 256: 64 * cm,
                         512: 32 * cm, 1024: 16 * cm}
        self.log_size = int(math.log(self.size, 2))
        self.log_in_size = int(math.log(in_res, 2))
        project_noise = _opt_get(model_opt, 'project_noise', False)
        self.conv1 = StyledConv(model_opt.feature_encoder_in_channels, self.channels[in_res], 3, self.style_dim,
                                blur_kernel=blur_kernel, project_noise=project_noise)
        self.to_rgb1 = ToRGB(self.channels[in_res], self.style_dim, upsample=False)
        self.num_layers = (self.log_size - self.log_in_size) * 2 + 1
        self.convs = nn.ModuleList()
        self.upsamples = nn.ModuleList()
        self.to_rgbs = nn.ModuleList()
        self.noises = nn.Module()
        for layer_idx in range(self.num_layers):
            res = (layer_idx + 2 * self.log_in_size + 1) // 2
            self.noises.register_buffer(f"noise_{layer_idx}", torch.randn(1, 1, 2 ** res, 2 ** res))
        in_channel = self.channels[in_res]
        for i in range(self.log_in_size + 1, self.log_size + 1):
            out_channel = self.channels[2 ** i]
            self.convs.append(StyledConv(in_channel, out_channel, 3, self.style_dim, upsample=True,
                                         blur_kernel=blur_kernel, project_noise=project_noise))
            self.convs.append(StyledConv(out_channel, out_channel, 3, self.style_dim, blur_kernel=blur_kernel,
                                         project_noise=project_noise))
            self.to_rgbs.append(ToRGB(out_channel, self.style_dim))
            in_channel = out_channel
        self.n_latent = (self.log_size - self.log_in_size) * 2 + 2

    def mean_latent(self, renderer_latent):
        return self.style(renderer_latent).mean(0, keepdim=True)

    # ---- all modulation vectors of one forward in two launches (e3dge_decoder_styles) ----------------------------------
    def _mod_layers(self):
        """[(ModulatedConv2d, latent index)] in execution order (conv1, to_rgb1, then per level up_conv, conv, to_rgb)."""
        out = [(self.conv1.conv, 0), (self.to_rgb1.conv, 1)]
        i = 1
        for u in range(len(self.to_rgbs)):
            out += [(self.convs[2 * u].conv, i), (self.convs[2 * u + 1].conv, i + 1), (self.to_rgbs[u].conv, i + 2)]
            i += 2
        return out

    def _style_table(self, B, device):
        layers = self._mod_layers()
        wsqs = [m.device_image()[1] if m.kernel_size == 3 else None for m, _ in layers]
        # the table stores the pointers of every modulation layer's parameters and of the squared-norm tables: all are its sources
        sources = [t for (m, _), w in zip(layers, wsqs) for t in (m.modulation.weight, m.modulation.bias, w) if t is not None]

        def build():
            pad4 = lambda n: (n + 3) // 4 * 4
            total = sum(pad4(B * m.in_channel) + (pad4(B * m.out_channel) + pad4(B) if w is not None else 0) for (m, _), w in zip(layers, wsqs))
            buf = torch.empty(total, device=device, dtype=torch.float32)
            rows = (_lib.ModLayer * len(layers))()
            views, off, row_start, co_start = [], 0, 0, 0
            for j, ((m, li), w) in enumerate(zip(layers, wsqs)):
                s_v = buf[off:off + B * m.in_channel].view(B, m.in_channel); off += pad4(B * m.in_channel)
                d_v = a_v = None
                if w is not None:
                    d_v = buf[off:off + B * m.out_channel].view(B, m.out_channel); off += pad4(B * m.out_channel)
                    a_v = buf[off:off + B]; off += pad4(B)
                views.append((s_v, d_v, a_v))
                mod = m.modulation
                rows[j] = _lib.ModLayer(mod_weight=mod.weight, mod_bias=mod.bias, wsq=w, style_out=s_v,
                                        demod_out=d_v if (w is not None and m.demodulate) else None,
                                        s_amax_out=a_v, ci=m.in_channel, co=m.out_channel if w is not None else 0,
                                        latent_index=li, row_start=row_start, co_start=co_start, lin_scale=float(mod.scale),
                                        lr_mul=float(mod.lr_mul))
                row_start += m.in_channel
                co_start += m.out_channel if w is not None else 0
            raw = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).to(device)
            return raw, buf, views, len(layers), row_start, co_start
        # one table (and one output buffer) per stream: two forwards in flight on different streams must not share it.  Eight are kept,
        # the oldest evicted first: a captured graph may still replay the others
        return _lib.cached(self, 'style_table', sources, build, (B, str(device), torch.cuda.current_stream(device).cuda_stream), limit=8)

    def _all_modulations(self, latent):
        """[(s, demod, s_amax)] per modulated conv of the forward, or None when the fused path is not taken."""
        if latent.device.type != "cuda" or modconv_backend() != "hip" or torch.is_grad_enabled() or latent.dtype != torch.float32:
            return None
        if any(m.kernel_size == 3 and (m.in_channel % 16 or m.out_channel % 32) for m, _ in self._mod_layers()):
            return None
        B = latent.shape[0]
        raw, buf, views, n, rows, cos = self._style_table(B, latent.device)
        self.__dict__['_dec2_gen'] = self.__dict__.get('_dec2_gen', 0) + 1      # (the packed backward reads these buffers)
        lat = latent.contiguous()
        _lib.launch("e3dge_decoder_styles", raw, n, rows, cos, lat, lat.shape[1], lat.shape[2], B)
        return views

    # ---- packed pipeline: the whole forward as one native call (e3dge_dec2_forward, csrc/decoder2.hip) -----------------
    def _dec2_ok(self, features, latent, noise, rgbd_in):
        """fp32 GPU tensors, no autograd graph through the decoder, channel counts the MFMA tiles cover."""
        if decoder_backend() != "packed" or modconv_backend() != "hip" or rgbd_in is not None:
            return False
        if features.device.type != "cuda" or features.dtype != torch.float32 or latent.dtype != torch.float32:
            return False
        if latent.device != features.device:
            return False
        if features.ndim != 4 or features.shape[2] != features.shape[3] or features.shape[2] < 4 or features.shape[2] % 2:
            return False
        if len(self.to_rgbs) > _lib.DEC2_MAX_UP or features.shape[0] < 1:
            return False
        if self._needs_graph(features, latent):
            mode = decoder_autograd_backend()
            if mode == "library" or any(n is not None and n.requires_grad for n in noise):
                return False
            if mode == "auto" and not (self._dec2_bwd_ok() and (not latent.requires_grad or decoder_dlatent_native()) and
                                       not any(p.requires_grad for p in _lib.params_of(self))):
                return False
        for m, _ in self._mod_layers():
            if m.kernel_size == 3 and (m.in_channel % 16 or m.out_channel % 32 or not m.demodulate or m.in_channel > 1024):
                return False
        if features.shape[1] != self.conv1.conv.in_channel:
            return False
        if self.to_rgbs and self._blur_factor() is None:     # the planar path applies any 4x4 blur kernel, and each level's own, as it is
            return False
        B, res = features.shape[0], features.shape[2]
        # 32-bit byte offsets inside one packed tensor
        top = res << len(self.to_rgbs)
        if B * max(self.channels.get(top, 16), 16) * (top + 4) * (top + 4) * 4 >= 2 ** 31:
            return False
        return all(n is None or (n.device == features.device and n.dtype == torch.float32) for n in noise)

    def _blur_factor(self):
        """blur_factor of the first up-sampling layer's Blur kernel (the plan hands it, and the first ToRGB's up-sampling kernel, to
        every level), or None when another level's Blur or Upsample buffer differs from the first level's: the planar path applies
        each layer's own.  Cached on every FIR buffer: _dec2_ok asks on every forward, and the kernels are device buffers."""
        blurs = [self.convs[2 * u].conv.blur.kernel for u in range(len(self.to_rgbs))]
        ups = [tr.upsample.kernel for tr in self.to_rgbs]

        def build():
            if any(k.shape != ks[0].shape or not torch.equal(k, ks[0]) for ks in (blurs, ups) for k in ks[1:]):
                return None
            return blur_factor(blurs[0])
        return _lib.cached(self, 'blur_factor', blurs + ups, build)

    def invalidate(self):
        """Drop every packed weight image, style table and plan of the decoder and its layers (needed after writes through `.data`;
        see SirenGenerator.invalidate)."""
        _lib.invalidate(self)

    def _dec2_bwd_ok(self):
        """Can the packed pipeline differentiate itself (e3dge_dec2_backward)?  Every 3x3 layer needs 32-channel multiples on both
        sides (the transposed weight images swap the roles), the up-sampling ones 64 input channels (one workgroup of the stride-2
        data-gradient kernel owns 64); E3DGE_DEC2_BWD=library keeps round 4's recomputing backward (A/B)."""
        if os.environ.get("E3DGE_DEC2_BWD", "native") == "library":
            return False
        return all(m.kernel_size != 3 or (m.in_channel % (64 if m.upsample else 32) == 0 and m.out_channel % 32 == 0) for m, _ in self._mod_layers())

    def _needs_graph(self, features, latent):
        return torch.is_grad_enabled() and (features.requires_grad or latent.requires_grad or
                                            any(p.requires_grad for p in _lib.params_of(self)))

    def _noise_amax(self, nz):
        """amax buffer with max|noise| (the packed producers need it for their operand-scale bound).  Cached only for the
        module's own registered `noises.noise_i` buffers, and the entry keeps the tensor it was measured on: a (data_ptr,
        version) key alone is recycled by the caching allocator (every fresh `normal_()` tensor has version 1 and lands on
        the block the previous call freed), which would hand a caller-supplied noise the maximum of an older tensor -- and
        with it an operand-scale bound that is too small.  Ad-hoc / random noise is measured on every call (one launch)."""
        own = any(nz is b for b in self.noises.buffers())
        cache = _DEC2_NOISE_AMAX.setdefault(self, {})
        key = (nz.data_ptr(), tuple(nz.shape), str(nz.device))
        if own:
            hit = cache.get(key)
            if hit is not None and hit[0] is nz and hit[1] == nz._version:
                return hit[2]
        am = torch.zeros(_lib.AMAX_FLOATS, device=nz.device, dtype=torch.float32)
        _lib.launch("e3dge_amax", am, nz, nz.numel())
        if own:
            if len(cache) >= 64:
                cache.pop(next(iter(cache)))
            cache[key] = (nz, nz._version, am)
        return am

    def _dec2_state(self, B, res, device):
        """Workspace + plan of the packed pipeline for one (batch, input resolution, device, stream): packed activation
        buffers (zero-filled ONCE: their borders are the convolutions' zero padding and no kernel writes them),
        per-sample weight images, ToRGB tables, amax / meta blocks, and the E3dgeDec2Plan struct with every static pointer
        filled in.  Its sources: every parameter, the style table and the pre-packed weights it points into.  Four are kept, the oldest
        evicted first (a captured graph may still replay the others)."""
        tab = self._style_table(B, device)                 # has its own cache; rebuilt when a modulation layer / wsq changes
        wpres = {sc: sc.conv.device_wpre() for sc in [self.conv1] + list(self.convs)}
        return _lib.cached(self, 'dec2_state', _lib.params_of(self) + [tab[0]] + list(wpres.values()),
                           lambda: self._build_dec2_state(B, res, device, tab, wpres),
                           (B, res, str(device), torch.cuda.current_stream(device).cuda_stream), limit=4)

    def _build_dec2_state(self, B, res, device, tab, wpres):
        lib = _lib.load()
        n_up = len(self.to_rgbs)
        raw, buf, views, n_mod, rows, cos = tab
        f32 = dict(device=device, dtype=torch.float32)
        keep = [raw, buf, *wpres.values()]                 # every tensor whose pointer the plan stores
        plan = _lib.Dec2Plan()
        plan.batch, plan.n_up, plan.in_res, plan.in_ch = B, n_up, res, self.conv1.conv.in_channel
        plan.mod_table = raw
        plan.n_mod, plan.mod_rows, plan.mod_co = n_mod, rows, cos
        plan.n_latent, plan.style_dim = self.n_latent, self.style_dim
        plan.negative_slope, plan.act_scale = float(self.conv1.activate.negative_slope), float(self.conv1.activate.scale)

        def fill_conv(dst, sc, view):
            m = sc.conv
            wimg = torch.empty(B * lib.e3dge_modconv_packed_words(m.out_channel, m.in_channel), device=device, dtype=torch.int32)
            bias = sc.activate.bias.detach()
            keep.extend([wimg, bias])
            dst.wpre, dst.style, dst.demod, dst.wimg = wpres[sc], view[0], view[1], wimg
            dst.noise_w, dst.bias = sc.noise.weight, bias
            dst.bias_amax = float(bias.abs().max().item())
            dst.ci, dst.co = m.in_channel, m.out_channel

        def fill_rgb(dst, tr, view, r):
            m = tr.conv
            w = m.weight.detach().reshape(3, m.in_channel)
            wm = torch.empty((B, 3, m.in_channel), **f32)
            out = torch.empty((B, 3, r, r), **f32)
            bias = tr.bias.detach().reshape(3)
            keep.extend([w, wm, out, bias])
            dst.weight, dst.style, dst.bias, dst.wm, dst.out = w, view[0], bias, wm, out
            dst.scale, dst.ci = float(m.scale), m.in_channel
            return out

        def packed(ch, r):
            t = torch.zeros(lib.e3dge_dec2_act_words(B, ch, r), device=device, dtype=torch.int32)
            keep.append(t)
            return t
        acts = [packed(self.conv1.conv.in_channel, res), packed(self.conv1.conv.out_channel, res)]
        fill_conv(plan.conv1, self.conv1, views[0])
        outs = [fill_rgb(plan.rgb1, self.to_rgb1, views[1], res)]
        r = res
        for u in range(n_up):
            up_c, cv, tr = self.convs[2 * u], self.convs[2 * u + 1], self.to_rgbs[u]
            fill_conv(plan.up[u], up_c, views[2 + 3 * u])
            fill_conv(plan.conv[u], cv, views[3 + 3 * u])
            r *= 2
            acts += [packed(up_c.conv.out_channel, r), packed(cv.conv.out_channel, r)]
            outs.append(fill_rgb(plan.rgb[u], tr, views[4 + 3 * u], r))
        for i, t in enumerate(acts):
            plan.act[i] = t.data_ptr()
        amax = torch.zeros((3 * n_up + 2, _lib.AMAX_FLOATS), **f32)
        meta = torch.zeros(2 * n_up + 2, device=device, dtype=torch.int32)
        fir_blur = (self.convs[0].conv.blur.kernel if n_up else self.conv1.conv.weight.new_zeros(4, 4)).detach().contiguous()
        fir_up = (self.to_rgbs[0].upsample.kernel if n_up else fir_blur).detach().contiguous()
        keep += [amax, meta, fir_blur, fir_up]
        plan.amax, plan.meta, plan.fir_blur, plan.fir_up = amax, meta, fir_blur, fir_up
        g = self._blur_factor() if n_up else None        # (None: e3dge_dec2_forward refuses the plan; _dec2_ok keeps such decoders off it)
        if g is not None:
            for i in range(4):
                plan.fir_blur_1d[i] = g[i]
            plan.fir_blur_separable = 1
        return dict(plan=plan, keep=keep, acts=acts, outs=outs, meta=meta, amax=amax, n_launch=lib.e3dge_dec2_num_launches(n_up))

    def _forward_packed(self, features, latent, noise, kernel_ms=None, save=False):
        """Decoder.forward body on the packed pipeline; `kernel_ms` (list) receives the HIP-event time of every launch
        (synchronous; for bench.py / tools).  The returned image is a fresh tensor; skip images live in the workspace."""
        B, res = features.shape[0], features.shape[2]
        dev = features.device
        st = self._dec2_state(B, res, dev)
        plan = st['plan']
        x = _lib.dense(features)
        lat = latent.contiguous()
        convs3 = [self.conv1] + list(self.convs)
        hold = [x, lat]
        r = res
        for i, sc in enumerate(convs3):
            if i >= 1 and i % 2 == 1:
                r *= 2
            nz = noise[i]
            if nz is None:                                   # NoiseInjection's own noise (reference :371-373)
                nz = torch.empty((B, 1, r, r), device=dev, dtype=torch.float32).normal_()
            nz = _lib.dense(nz)
            if nz.shape[0] not in (1, B) or nz.numel() != nz.shape[0] * r * r:
                raise RuntimeError(f"noise[{i}] must be (1|B, 1, {r}, {r}); got {tuple(nz.shape)}")
            dst = plan.conv1 if i == 0 else (plan.up[(i - 1) // 2] if i % 2 == 1 else plan.conv[(i - 1) // 2])
            am = self._noise_amax(nz)
            dst.noise, dst.noise_amax, dst.noise_batch = nz, am, nz.shape[0]
            hold += [nz, am]
        out = torch.empty_like(st['outs'][-1])
        last = plan.rgb[len(self.to_rgbs) - 1] if len(self.to_rgbs) else plan.rgb1
        last.out = out
        plan.features, plan.latent = x, lat
        plan.save_for_backward = int(bool(save))         # keep the top activation too: the backward reads every activation's signs
        self.__dict__['_dec2_gen'] = self.__dict__.get('_dec2_gen', 0) + 1      # (a backward checks that its forward was the last one)
        ms = None
        if kernel_ms is not None:
            ms = (ctypes.c_float * st['n_launch'])()
            plan.kernel_ms, plan.n_kernel_ms = ctypes.cast(ms, ctypes.POINTER(ctypes.c_float)), st['n_launch']
        else:
            plan.kernel_ms, plan.n_kernel_ms = None, 0
        _lib.launch("e3dge_dec2_forward", plan)
        if ms is not None:
            kernel_ms[:] = list(ms)
        st['hold'] = hold            # inputs of the launches just queued stay alive until the next call on this stream
        return out

    # ---- backward of the packed pipeline: d image -> d features (e3dge_dec2_backward, csrc/decoder2_bwd.h) -----------------------
    def _dec2_bwd_state(self, st, B, res, device):
        """Workspace + E3dgeDec2BwdPlan next to a forward state: packed gradient buffers (zero-filled once, shapes of the
        activations), the phase-plane buffer of Blur^T, d rgb images, transposed per-sample weight images, amax / meta / norms."""
        bw = st.get('bwd')
        if bw is not None:
            return bw
        lib = _lib.load()
        n_up = len(self.to_rgbs)
        f32 = dict(device=device, dtype=torch.float32)
        keep = []
        q = _lib.Dec2BwdPlan()

        def fill(dst, sc):
            m = sc.conv
            wimg = torch.empty(B * lib.e3dge_modconv_packed_words(m.in_channel, m.out_channel), device=device, dtype=torch.int32)
            wcol = m.device_image()[1].sum(0).contiguous()     # (ci): column sums of the squared-norm table, for the operator-norm bound
            wpt = m.device_wpre_t()
            keep.extend([wimg, wcol, wpt])
            dst.wpre_t, dst.wcol, dst.wimg_t = wpt, wcol, wimg
        fill(q.conv1, self.conv1)
        gacts = [None, torch.zeros_like(st['acts'][1])]
        r, pwords = res, 0
        for u in range(n_up):
            fill(q.up[u], self.convs[2 * u])
            fill(q.conv[u], self.convs[2 * u + 1])
            d = torch.empty((B, 3, r, r), **f32)
            keep.append(d)
            q.drgb[u] = d.data_ptr()
            r *= 2
            gacts += [torch.zeros_like(st['acts'][2 + 2 * u]), torch.zeros_like(st['acts'][3 + 2 * u])]
            pwords = max(pwords, lib.e3dge_dec2_pbuf_words(B, self.convs[2 * u].conv.out_channel, r))
        for i, t in enumerate(gacts):
            if t is not None:
                q.gact[i] = t.data_ptr()
        pbuf = torch.empty(max(pwords, 4), device=device, dtype=torch.int32)
        amax = torch.zeros((4 * n_up + 2, _lib.AMAX_FLOATS), **f32)
        meta = torch.zeros(3 * n_up + 1, device=device, dtype=torch.int32)
        bounds = torch.zeros(3 * n_up + 2, **f32)
        keep += [gacts, pbuf, amax, meta, bounds]
        q.pbuf, q.amax, q.meta, q.bounds = pbuf, amax, meta, bounds
        bw = dict(plan=q, keep=keep, gacts=gacts, meta=meta, amax=amax, bounds=bounds, n_launch=lib.e3dge_dec2_bwd_num_launches(n_up))
        st['bwd'] = bw
        return bw

    def _backward_packed(self, features, d_img, kernel_ms=None, want_latent=False, latent_shape=None):
        """(d features, d latent or None) for the LAST packed forward of this (batch, resolution, stream) -- it must have run with
        save=True.  d latent (B, n_latent, style_dim): 2 n_up + 7 more launches inside the same native call."""
        B, res = features.shape[0], features.shape[2]
        dev = features.device
        st = self._dec2_state(B, res, dev)
        if not st['plan'].save_for_backward:
            raise RuntimeError("Decoder._backward_packed: the last packed forward of this workspace did not keep its activations")
        bw = self._dec2_bwd_state(st, B, res, dev)
        q = bw['plan']
        g = _lib.dense(d_img)                             # (`img.sum().backward()` delivers a stride-0 gradient)
        if g.dtype != torch.float32 or g.shape != st['outs'][-1].shape:
            raise RuntimeError(f"d image must be float32 {tuple(st['outs'][-1].shape)}; got {g.dtype} {tuple(g.shape)}")
        d_feat = torch.empty((B, self.conv1.conv.in_channel, res, res), device=dev, dtype=torch.float32)
        q.d_img, q.d_features = g, d_feat
        d_lat = None
        if want_latent:
            if 'ds_part' not in bw:
                n = _lib.load().e3dge_dec2_dlatent_ws_floats(st['plan'])      # (ctypes passes the struct by reference: POINTER argtype)
                bw['ds_part'] = torch.empty(max(int(n), 1), device=dev, dtype=torch.float32)
            d_lat = torch.empty((B, self.n_latent, self.style_dim), device=dev, dtype=torch.float32)
            q.d_latent, q.ds_part, q.ds_part_floats = d_lat, bw['ds_part'], bw['ds_part'].numel()
        else:
            q.d_latent, q.ds_part, q.ds_part_floats = None, None, 0
        ms = None
        if kernel_ms is not None:
            ms = (ctypes.c_float * bw['n_launch'])()
            q.kernel_ms, q.n_kernel_ms = ctypes.cast(ms, ctypes.POINTER(ctypes.c_float)), bw['n_launch']
        else:
            q.kernel_ms, q.n_kernel_ms = None, 0
        _lib.launch("e3dge_dec2_backward", st['plan'], q)
        if ms is not None:
            kernel_ms[:] = list(ms)
        bw['hold'] = [g]
        if d_lat is not None and latent_shape is not None and tuple(latent_shape) != tuple(d_lat.shape):
            d_lat = d_lat.reshape(latent_shape)
        return d_feat, d_lat

    def dec2_bwd_launch_names(self):
        """Labels of the launches of one packed backward, in the order of `kernel_ms`."""
        names = ["norms", "weights^T", "amax(d_img)", "to_rgb^T+mask(top)"]
        for u in reversed(range(len(self.to_rgbs))):
            names += [f"L{u}.d_rgb", f"L{u}.conv^T", f"L{u}.blur^T", f"L{u}.convT^T"]
        return names + ["conv1^T"]

    def dec2_unpack_grad(self, index, features_shape):
        """Debug / test view of a packed GRADIENT of the last packed backward (same indices as dec2_unpack; 0 is not a packed tensor)."""
        B, res = features_shape[0], features_shape[2]
        dev = next(self.parameters()).device
        st = self._dec2_state(B, res, dev)
        bw = st['bwd']
        n_up = len(self.to_rgbs)
        chans, ress, r = [None, self.conv1.conv.out_channel], [None, res], res
        for u in range(n_up):
            r *= 2
            chans += [self.convs[2 * u].conv.out_channel, self.convs[2 * u + 1].conv.out_channel]
            ress += [r, r]
        # meta: G2 of level u at [u + 1] (activation index 3 + 2u; conv1's output: u = -1), G1 of level u at [n_up + 1 + u] (index 2 + 2u)
        mi = (index - 3) // 2 + 1 if index % 2 == 1 else n_up + 1 + (index - 2) // 2
        out = torch.empty((B, chans[index], ress[index], ress[index]), device=dev, dtype=torch.float32)
        _lib.launch("e3dge_dec2_unpack", out, bw['gacts'][index], bw['meta'][mi:], B, chans[index], ress[index])
        return out

    def dec2_launch_names(self):
        """Labels of the launches of one packed forward, in the order of `kernel_ms`."""
        names = ["styles", "amax(features)", "pack(features)", "weights", "conv1", "to_rgb1"]
        for u in range(len(self.to_rgbs)):
            names += [f"L{u}.convT", f"L{u}.blur", f"L{u}.conv", f"L{u}.to_rgb"]
        return names

    def dec2_unpack(self, index, features_shape):
        """Debug / test view of a packed activation of the LAST packed forward with this batch and resolution:
        index 0 = packed features, 1 = conv1 output, 2 + 2u = blur output of level u, 3 + 2u = conv output of level u."""
        B, res = features_shape[0], features_shape[2]
        dev = next(self.parameters()).device
        st = self._dec2_state(B, res, dev)
        chans = [self.conv1.conv.in_channel, self.conv1.conv.out_channel]
        ress = [res, res]
        r = res
        for u in range(len(self.to_rgbs)):
            r *= 2
            chans += [self.convs[2 * u].conv.out_channel, self.convs[2 * u + 1].conv.out_channel]
            ress += [r, r]
        out = torch.empty((B, chans[index], ress[index], ress[index]), device=dev, dtype=torch.float32)
        _lib.launch("e3dge_dec2_unpack", out, st['acts'][index], st['meta'][index:], B, chans[index], ress[index])
        return out

    def get_latent(self, input):
        return self.style(input)

    def styles_and_noise_forward(self, styles, noise, inject_index=None, truncation=1, truncation_latent=None,
                                 input_is_latent=False, randomize_noise=True):
        if not input_is_latent:
            styles = [self.style(s) for s in styles]
        if noise is None:
            noise = [None] * self.num_layers if randomize_noise else \
                [getattr(self.noises, f"noise_{i}") for i in range(self.num_layers)]
        if truncation < 1:
            styles = [truncation_latent[1] + truncation * (s - truncation_latent[1]) for s in styles]
        if len(styles) < 2:
            inject_index = self.n_latent
            latent = styles[0] if styles[0].ndim >= 3 else styles[0].unsqueeze(1).repeat(1, inject_index, 1)
        else:
            if inject_index is None:
                inject_index = random.randint(1, self.n_latent - 1)
            latent = torch.cat([styles[0].unsqueeze(1).repeat(1, inject_index, 1),
                                styles[1].unsqueeze(1).repeat(1, self.n_latent - inject_index, 1)], 1)
        return latent, noise

    def forward(self, features, styles, rgbd_in=None, transform=None, return_latents=False, inject_index=None,
                truncation=1, truncation_latent=None, input_is_latent=False, noise=None, randomize_noise=True,
                mesh_path=None, conditions=None):
        assert isinstance(styles, list), 'wrap latent code with list'
        latent, noise = self.styles_and_noise_forward(styles, noise, inject_index, truncation, truncation_latent,
                                                      input_is_latent, randomize_noise)
        if self.conv1.noise.project and any(n is not None for n in noise):
            noise = self._project_noises(features, noise, transform, mesh_path)
        if self._dec2_ok(features, latent, noise, rgbd_in):
            if not self._needs_graph(features, latent):
                return self._forward_packed(features, latent, noise), (latent if return_latents else None)
            # a graph is wanted and E3DGE_DECODER_AUTOGRAD=packed: packed forward, library backward on recomputed activations.
            # NoiseInjection's own noise is drawn HERE so that the backward's recomputation sees the same values.
            r, nz = features.shape[2], []
            for i, n in enumerate(noise):
                if i >= 1 and i % 2 == 1:
                    r *= 2
                nz.append(n if n is not None else torch.empty((features.shape[0], 1, r, r), device=features.device, dtype=torch.float32).normal_())
            img = _PackedDecoderFn.apply(self, nz, features, latent, *self.parameters())
            return img, (latent if return_latents else None)
        return self._forward_layers(features, latent, noise, rgbd_in), (latent if return_latents else None)

    def _project_noises(self, features, noise, transform, mesh_path):
        """What the reference's NoiseInjection.forward does layer by layer for `project_noise` (:459-466), done first: every given map is
        replaced by its module's projection (NoiseInjection.project_noise).  The maps of one size share one rasterisation
        (e3dge_noise_project takes up to four vertex fields): one launch per size, five for the nine maps of a 1024 decoder.  The
        packed and the layer paths then take the list as any other `noise`."""
        for value, name in ((transform, "transform"), (mesh_path, "mesh_path")):
            if value is None:
                raise ValueError(f"a project_noise decoder called with noise needs `{name}` (the frame's camera poses / the surface mesh); "
                                 f"got {name}=None")
        if features.shape[0] != 1:
            raise AssertionError(f"project_noise assumes batch size 1 at inference, got batch {features.shape[0]}")
        modules = [self.conv1.noise] + [c.noise for c in self.convs]
        camera = mesh_utils.noise_camera(transform)
        groups = {}                                                              # size -> [(index, verts, faces, vert_noise, prev)]
        for i, (m, n) in enumerate(zip(modules, noise)):                         # in layer order: the order the reference draws in
            if n is not None:
                groups.setdefault(n.shape[2], []).append((i,) + m.projection_inputs(n, mesh_path))
        out = list(noise)
        for size, members in groups.items():
            for c0 in range(0, len(members), _lib.NOISE_PROJECT_MAX_MAPS):
                part = members[c0:c0 + _lib.NOISE_PROJECT_MAX_MAPS]
                _, verts, faces, _, _ = part[0]
                if any(p[3].shape != part[0][3].shape for p in part):             # a module that kept the noise of another mesh
                    raise RuntimeError("project_noise: the modules of one size hold vertex noise of different meshes")
                maps, _ = mesh_utils.project_vertex_noise(verts, faces, torch.stack([p[3] for p in part]), camera, size,
                                                          prev=torch.cat([p[4] for p in part]))
                for k, p in enumerate(part):
                    out[p[0]] = maps[k].reshape(1, 1, size, size)
        return out

    def _forward_layers(self, features, latent, noise, rgbd_in):
        """The layer-by-layer forward (reference :764-792): fused planar kernels without a graph, weight modulation + library
        convolutions (differentiable) with one."""
        # amax buffers (one row per activation): every fused layer leaves max|output| for the next one's operand scaling
        track = features.device.type == "cuda" and modconv_backend() == "hip" and not torch.is_grad_enabled()
        amax = torch.zeros((self.num_layers + 1, _lib.AMAX_FLOATS), device=features.device, dtype=torch.float32) if track else None
        am = (lambda j: amax[j]) if track else (lambda j: None)
        mods = self._all_modulations(latent) if track else None
        pre = (lambda j: mods[j]) if mods is not None else (lambda j: None)
        out = self.conv1(features, latent[:, 0], noise=noise[0], out_amax=am(1), pre=pre(0))
        skip = self.to_rgb1(out, latent[:, 1], skip=rgbd_in, pre=pre(1))
        i, j = 1, 2
        for up_conv, conv, n_up, n_conv, to_rgb in zip(self.convs[::2], self.convs[1::2], noise[1::2], noise[2::2],
                                                       self.to_rgbs):
            out = up_conv(out, latent[:, i], noise=n_up, in_amax=am(i), out_amax=am(i + 1), pre=pre(j))
            out = conv(out, latent[:, i + 1], noise=n_conv, in_amax=am(i + 1), out_amax=am(i + 2), pre=pre(j + 1))
            skip = to_rgb(out, latent[:, i + 2], skip=skip, pre=pre(j + 2))
            i += 2
            j += 3
        return skip


class Generator(nn.Module):
    """mapping network + volume renderer + decoder (reference :800-1020)."""

    def __init__(self, model_opt, renderer_opt, blur_kernel=[1, 3, 3, 1], ema=False, full_pipeline=True):
        super().__init__()
        self.size = model_opt.size
        self.style_dim = model_opt.style_dim
        self.num_layers = 1
        self.train_renderer = not model_opt.freeze_renderer
        self.full_pipeline = full_pipeline
        model_opt.feature_encoder_in_channels = _opt_get(renderer_opt, 'width', 256)
        self.is_train = not (ema or model_opt.is_test)
        self.style = nn.Sequential(*[MappingLinear(self.style_dim, self.style_dim, activation="fused_lrelu")
                                     for _ in range(3)])
        # the reference builds the renderer in its default mode='train' and relies on perturb=0 from the option
        # overrides (base_setup.py:53-56); same here.
        self.renderer = VolumeFeatureRenderer(renderer_opt, style_dim=self.style_dim,
                                              out_im_res=model_opt.renderer_spatial_output_dim)
        # the reference decides the same way whether the renderer's weights get gradients (:812, :959); off = the frozen fast path
        self.renderer.train_renderer = self.train_renderer
        self.renderer_n_latent = _opt_get(renderer_opt, 'depth', 8) + 1
        if self.full_pipeline:
            self.decoder = Decoder(model_opt)
            self.stylegan_n_latent = 10

    def mean_latent(self, n_latent, device):
        latent_in = torch.randn(n_latent, self.style_dim, device=device)
        renderer_latent = self.style(latent_in)
        renderer_latent_mean = renderer_latent.mean(0, keepdim=True)
        decoder_latent_mean = None
        if self.full_pipeline:
            decoder_latent_mean = self.decoder.mean_latent(renderer_latent)
            self.decoder_latent_mean = decoder_latent_mean.to(device)
        return [renderer_latent_mean, decoder_latent_mean]

    def get_latent(self, input):
        return self.style(input)

    def invalidate(self):
        """Drop everything derived from the parameters anywhere in the generator: the renderer's records and host copies
        (VolumeFeatureRenderer.invalidate) and every packed weight image, table and plan of the renderer, the decoder and any other
        sub-module.  Needed after writes through `.data` (the reference's EMA accumulate()); see SirenGenerator.invalidate."""
        self.renderer.invalidate()
        _lib.invalidate(self)

    def styles_and_noise_forward(self, styles, inject_index=None, truncation=1, truncation_latent=None,
                                 input_is_latent=False):
        if not input_is_latent:
            styles = [self.style(s) for s in styles]
        if truncation < 1:
            assert isinstance(truncation_latent, list)
            styles = [truncation_latent[0] + truncation * (s - truncation_latent[0]) for s in styles]
        return styles


    def init_forward(self, *a, **k):
        raise NotImplementedError("sphere-initialisation pre-training (mlp_init_pass, reference :923-932) is outside this build")

    def data_sample_forward(self, *a, **k):
        raise NotImplementedError("sdf_sample_pass (reference :905-921) is outside this build")

    def forward(self, styles, cam_poses, focals, near=0.88, far=1.12, return_latents=False, inject_index=None,
                truncation=1, truncation_latent=None, input_is_latent=False, noise=None, randomize_noise=True,
                return_sdf=False, return_xyz=False, return_eikonal=False, project_noise=False, return_mesh=False,
                mesh_with_shading=True, mesh_path=None, pred_decoder_latents=None, sample_mode=False,
                diable_decoder_inference=False):
        """The base class entry (reference :934-1020) -- what the surface-extraction generator `surface_g_ema` is called
        through (train_setup.py:112-126): tuple (rgb or None, thumb [, xyz] [, sdf] [, eikonal_term] [, mask]).
        [`diable_decoder_inference` is the reference's spelling.]"""
        # as the reference: no renderer graph when its weights are frozen
        with torch.set_grad_enabled(torch.is_grad_enabled() and self.is_train and self.train_renderer):
            latent = self.styles_and_noise_forward(styles, inject_index, truncation, truncation_latent, input_is_latent)
            sample_batch = self.renderer(cam_poses, focals, near, far, styles=latent[0], return_eikonal=return_eikonal,
                                         sample_mode=sample_mode, return_mesh=return_mesh, mesh_with_shading=mesh_with_shading)
            if sample_mode:
                return sample_batch
        rgb = decoder_latent = None
        if self.full_pipeline and not diable_decoder_inference:
            decoder_latent = latent if pred_decoder_latents is None else pred_decoder_latents
            rgb, decoder_latent = self.decoder(sample_batch['features'], decoder_latent, transform=cam_poses if project_noise else None,
                                               return_latents=return_latents, inject_index=inject_index, truncation=truncation,
                                               truncation_latent=truncation_latent, noise=noise,
                                               input_is_latent=input_is_latent, randomize_noise=randomize_noise,
                                               mesh_path=mesh_path)
        if return_latents:
            return rgb, decoder_latent
        out = (rgb, sample_batch['gen_thumb_imgs'])
        if return_xyz:
            out += (sample_batch['xyz'],)
        if return_sdf:
            out += (sample_batch['sdf'],)
        if return_eikonal:
            out += (sample_batch['eikonal_term'],)
        if return_xyz:
            out += (sample_batch['mask'],)
        return out


class G_pred_latents(Generator):
    """The generator entry the runners call (reference :1023-1172, call site trainer.py:881-897):
    `generator([w_renderer, w_decoder], cam_poses, focals, near, far, input_is_latent=True, ...) -> dict`."""

    def forward(self, styles, cam_poses, focals, near=0.88, far=1.12, return_latents=False, inject_index=None,
                truncation=1, truncation_latent=None, input_is_latent=False, noise=None, randomize_noise=True,
                return_sdf=False, return_xyz=False, return_eikonal=False, project_noise=False, return_mesh=False,
                mesh_with_shading=True, mesh_path=None, conditions=None, sample_mode=False, geometry_sample=None,
                sample_with_decoder=False, sample_with_renderer=False, return_surface_eikonal=False,
                renderer_only=False, inference_mode=False, sample_without_grad=False, **kwargs):
        if self.full_pipeline:
            assert type(styles) in [list, tuple], 'reformat latent to list/tuple'
            if not input_is_latent:
                encoder_latent, decoder_latent = styles[0], None
            else:
                encoder_latent, decoder_latent = styles
        else:
            decoder_latent = None
            encoder_latent = styles[0]
        renderer_latent = self.styles_and_noise_forward([encoder_latent], inject_index, truncation,
                                                        truncation_latent, input_is_latent)
        will_decode = (not renderer_only) and (self.full_pipeline or sample_with_decoder) and not sample_with_renderer
        # the stage-1 step (trainer.py:881-897 with return_eikonal): the eikonal chains of the renderer do not feed the decoder, so they may run
        # beside its forward / backward on a side stream (volume_renderer.begin_deferred / finish_deferred)
        deferred = will_decode and return_eikonal and torch.is_grad_enabled() and not sample_without_grad and \
            hasattr(self.renderer, 'begin_deferred') and self.renderer.begin_deferred()
        try:
            render_out = self.renderer(cam_poses, focals, near, far, styles=renderer_latent[0],
                                       return_eikonal=return_eikonal, return_mesh=return_mesh,
                                       mesh_with_shading=mesh_with_shading, sample_mode=sample_mode,
                                       geometry_sample=geometry_sample, return_surface_eikonal=return_surface_eikonal,
                                       sample_without_grad=sample_without_grad, **kwargs)
            render_out['styles'] = renderer_latent[0]
            if renderer_only:
                return render_out
            if will_decode:
                if decoder_latent is None:
                    decoder_latent = renderer_latent
                elif not isinstance(decoder_latent, list):
                    decoder_latent = [decoder_latent]
                gen_imgs, decoder_latent = self.decoder(
                    render_out['features'], decoder_latent, transform=cam_poses if project_noise else None, return_latents=return_latents,
                    inject_index=inject_index, truncation=truncation, truncation_latent=truncation_latent, noise=noise,
                    input_is_latent=input_is_latent, randomize_noise=randomize_noise, mesh_path=mesh_path,
                    conditions=conditions)
                render_out['gen_imgs'] = gen_imgs
                render_out['decoder_latent'] = decoder_latent
        finally:
            if deferred:
                self.renderer.finish_deferred(render_out if 'render_out' in locals() else {})
        return render_out
