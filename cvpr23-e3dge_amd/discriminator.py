"""StyleGAN2 discriminator on the HIP kernels of csrc/disc.hip / csrc/disc_bwd.h: the adversarial term of the stage-2.2 objective,
`g_nonsaturating_loss(discriminator(render_out['gen_imgs']))` with the discriminator frozen (project/trainer.py:1212, :1233-1244).

`Discriminator(opt, blur_kernel=[1, 3, 3, 1])` has the reference's constructor, call surface and sub-module arrangement
(project/models/stylesdf_model.py:1514-1617, ConvLayer :544-584, EqualConv2d :168-207), so a state dict saved from the reference loads
with strict=True, `Blur.kernel` buffers included:

    convs.0.{0.weight, 1.bias}, convs.N.conv1.{0.weight, 1.bias}, convs.N.conv2.{0.kernel, 1.weight, 2.bias},
    convs.N.skip.{0.kernel, 1.weight}, final_conv.{0.weight, 1.bias}, final_linear.{0,1}.{weight, bias}

Two paths compute `forward(input)` -> (B, 1) logits:

  torch  the composition of plain torch layers and the package's own op.upfirdn2d / op.fused_leaky_relu / EqualLinear.  It is the
         computation itself for CPU tensors, for any dtype other than float32, whenever a discriminator parameter requires grad (the
         D-step, with d_r1_loss's double backward: differentiable stream ops and library convolutions on the GPU), for a pool_256 ratio
         the HIP pool does not cover, and when E3DGE_DISCRIMINATOR=torch (A/B timing).
  HIP    GPU float32 input with every parameter frozen.  Under no_grad, or for an input that wants no gradient, one C-ABI call
         (e3dge_disc_forward).  Under grad with an input that requires grad, one autograd Function whose forward is the state-saving
         form of the same launches (bit-identical logits) and whose backward (e3dge_disc_backward) returns the gradient to the input
         image only; it is once-differentiable: a double backward raises, as in IDLoss.

Weight images go through _lib.cached (drop them with `invalidate()` after writes through `.data`).  Out of scope, as before:
StyleGANEncoder, DEncoder and the VolumeRenderDiscriminator* family (stylesdf_model.py:1193-1510, :1620-1765); of that family
`VolumeRenderDiscriminator` itself now lives in e3dge_amd.volume_discriminator."""
import math
import os

import torch
from torch import nn
from torch.nn import functional as F

from . import _lib
from .losses import AvgPool2d
from .op import FusedLeakyReLU
from .stylesdf_model import Blur, EqualLinear
from .volume_renderer import _opt_get

TAP_STDDEV, TAP_FINAL, TAP_STEM = _lib.DISC_TAP_STDDEV, _lib.DISC_TAP_FINAL, _lib.DISC_TAP_STEM


def backend():
    """'hip' (default) or 'torch' (E3DGE_DISCRIMINATOR=torch forces the torch composition everywhere)."""
    v = os.environ.get("E3DGE_DISCRIMINATOR", "hip")
    if v not in ("hip", "torch"):
        raise ValueError(f"E3DGE_DISCRIMINATOR={v!r}: 'hip' or 'torch'")
    return v


def stddev_group(batch, stddev_group=4):
    """The minibatch-stddev group of stylesdf_model.py:1600-1602; raises for a batch the reference's reshape rejects."""
    group = min(batch, stddev_group)
    if batch % group != 0:
        group = 3 if batch % 3 == 0 else 2
    if batch % group != 0:
        raise ValueError(f"Discriminator: a batch of {batch} has no minibatch-stddev group (the reference's reshape({group}, -1, ...) rejects it)")
    return group


class EqualConv2d(nn.Module):
    """Reference :168-207."""

    def __init__(self, in_channel, out_channel, kernel_size, stride=1, padding=0, bias=True):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(out_channel, in_channel, kernel_size, kernel_size))
        self.scale = 1 / math.sqrt(in_channel * kernel_size ** 2)
        self.stride = stride
        self.padding = padding
        self.bias = nn.Parameter(torch.zeros(out_channel)) if bias else None

    def forward(self, input):
        return F.conv2d(input, self.weight * self.scale, bias=self.bias, stride=self.stride, padding=self.padding)

    def __repr__(self):
        return (f"{self.__class__.__name__}({self.weight.shape[1]}, {self.weight.shape[0]}, {self.weight.shape[2]}, "
                f"stride={self.stride}, padding={self.padding})")


class ConvLayer(nn.Sequential):
    """Reference :544-584: [Blur,] EqualConv2d [, FusedLeakyReLU]."""

    def __init__(self, in_channel, out_channel, kernel_size, downsample=False, blur_kernel=[1, 3, 3, 1], bias=True, activate=True):
        layers = []
        if downsample:
            factor = 2
            p = (len(blur_kernel) - factor) + (kernel_size - 1)
            layers.append(Blur(blur_kernel, pad=((p + 1) // 2, p // 2)))
            stride = 2
            self.padding = 0
        else:
            stride = 1
            self.padding = kernel_size // 2
        layers.append(EqualConv2d(in_channel, out_channel, kernel_size, padding=self.padding, stride=stride, bias=bias and not activate))
        if activate:
            layers.append(FusedLeakyReLU(out_channel, bias=bias))
        super().__init__(*layers)


class ResBlock(nn.Module):
    """Reference :1514-1538 (its blur_kernel argument is accepted and, as there, not passed on)."""

    def __init__(self, in_channel, out_channel, blur_kernel=[1, 3, 3, 1], merge=False):
        super().__init__()
        self.conv1 = ConvLayer(2 * in_channel if merge else in_channel, in_channel, 3)
        self.conv2 = ConvLayer(in_channel, out_channel, 3, downsample=True)
        self.skip = ConvLayer(2 * in_channel if merge else in_channel, out_channel, 1, downsample=True, activate=False, bias=False)

    def forward(self, input):
        out = self.conv1(input)
        out = self.conv2(out)
        return (out + self.skip(input)) / math.sqrt(2)


class Discriminator(nn.Module):
    """`Discriminator(opt)(images)` -> (B, 1) logits.  opt: D_init_size (1024), D_input_size (3), channel_multiplier (2)."""

    def __init__(self, opt, blur_kernel=[1, 3, 3, 1]):
        super().__init__()
        init_size = _opt_get(opt, "D_init_size", 1024)
        input_size = _opt_get(opt, "D_input_size", 3)
        cm = _opt_get(opt, "channel_multiplier", 2)
        self.init_size, self.input_size, self.channel_multiplier = init_size, input_size, cm
        self.pool_256 = AvgPool2d((256, 256))                        # AdaptiveAvgPool2d; HIP at integer ratios
        channels = {4: 512, 8: 512, 16: 512, 32: 512, 64: 256 * cm, 128: 128 * cm, 256: 64 * cm, 512: 32 * cm, 1024: 16 * cm}
        convs = [ConvLayer(input_size, channels[init_size], 1)]
        log_size = int(math.log(init_size, 2))
        in_channel = channels[init_size]
        self.in_channel = in_channel
        for i in range(log_size, 2, -1):
            out_channel = channels[2 ** (i - 1)]
            convs.append(ResBlock(in_channel, out_channel, blur_kernel))
            in_channel = out_channel
        self.convs = nn.Sequential(*convs)
        self.stddev_group = 4
        self.stddev_feat = 1
        in_channel += 1
        self.final_conv = ConvLayer(in_channel, channels[4], 3)
        self.final_linear = nn.Sequential(EqualLinear(channels[4] * 4 * 4, channels[4], activation="fused_lrelu"),
                                          EqualLinear(channels[4], 1))

    def invalidate(self):
        """Drop the packed weight image (needed only after writes through `.data`)."""
        _lib.invalidate(self)

    # ---- the torch composition --------------------------------------------------------------------------------------------------
    def forward_torch(self, input, taps=None):
        """The reference's forward, operation for operation.  taps: a list that receives every ResBlock output, the stddev scalars
        and final_conv's output."""
        if self.init_size == 256:
            input = self.pool_256(input)
        out = input
        for i, layer in enumerate(self.convs):
            out = layer(out)
            if taps is not None and i > 0:
                taps.append(out)
        batch, channel, height, width = out.shape
        group = stddev_group(batch, self.stddev_group)
        stddev = out.reshape(group, -1, self.stddev_feat, channel // self.stddev_feat, height, width)
        stddev = torch.sqrt(stddev.var(0, unbiased=False) + 1e-8)
        stddev = stddev.mean([2, 3, 4], keepdims=True).squeeze(2)
        if taps is not None:
            taps.append(stddev.reshape(-1))
        stddev = stddev.repeat(group, 1, height, width)
        final_out = torch.cat([out, stddev], 1)
        final_out = self.final_conv(final_out)
        if taps is not None:
            taps.append(final_out)
        final_out = final_out.reshape(batch, -1)
        final_out = self.final_linear(final_out)
        return final_out[:, :1]

    # ---- the HIP path -----------------------------------------------------------------------------------------------------------
    def _key(self):
        return self.init_size, self.channel_multiplier, self.input_size

    def _pool_factor(self, input):
        """1 (no pooling), the integer pool_256 ratio of the HIP pool, or None (not a shape of the HIP path)."""
        if input.ndim != 4 or input.shape[1] != self.input_size or input.shape[2] != input.shape[3] or input.shape[0] < 1:
            return None
        size = input.shape[2]
        if size == self.init_size:
            return 1
        if self.init_size == 256 and size in (512, 1024, 2048, 4096):
            return size // 256
        return None

    def uses_hip(self, input):
        """Does forward(input) take the HIP kernels?"""
        if backend() != "hip" or input.device.type != "cuda" or input.dtype != torch.float32:
            return False
        if any(p.requires_grad for p in _lib.params_of(self)):
            return False
        return self._pool_factor(input) is not None

    def _sources(self):
        blocks = list(self.convs)[1:]
        first_blur = blocks[0].conv2[0].kernel
        return dict(stem=[self.convs[0][0].weight, self.convs[0][1].bias],
                    conv1_w=[b.conv1[0].weight for b in blocks], conv1_b=[b.conv1[1].bias for b in blocks],
                    conv2_w=[b.conv2[1].weight for b in blocks], conv2_b=[b.conv2[2].bias for b in blocks],
                    skip_w=[b.skip[1].weight for b in blocks],
                    final=[self.final_conv[0].weight, self.final_conv[1].bias],
                    lin=[self.final_linear[0].weight, self.final_linear[0].bias, self.final_linear[1].weight, self.final_linear[1].bias],
                    blur=[first_blur] + [k for b in blocks for k in (b.conv2[0].kernel, b.skip[0].kernel)])

    def _packed(self, device):
        groups = self._sources()
        src = [t for g in groups.values() for t in g]

        def build():
            with torch.no_grad():
                blurs = groups["blur"]
                if any(k.shape != (4, 4) for k in blurs) or not all(torch.equal(k, blurs[0]) for k in blurs[1:]):
                    raise NotImplementedError("Discriminator HIP path: one 4 x 4 blur kernel for every Blur (set E3DGE_DISCRIMINATOR=torch)")
                keep = {k: [t.detach().contiguous() for t in g] for k, g in groups.items()}
                s = _lib.DiscPackSrc(init_size=self.init_size, channel_multiplier=self.channel_multiplier, in_channels=self.input_size)
                s.stem_w, s.stem_b = keep["stem"]
                for name in ("conv1_w", "conv1_b", "conv2_w", "conv2_b", "skip_w"):
                    for i, t in enumerate(keep[name]):
                        getattr(s, name)[i] = t.data_ptr()
                s.final_w, s.final_b = keep["final"]
                s.lin1_w, s.lin1_b, s.lin2_w, s.lin2_b = keep["lin"]
                s.blur = keep["blur"][0]
                packed = torch.empty(_lib.query("e3dge_disc_packed_floats", *self._key()), device=device, dtype=torch.float32)
                _lib.launch("e3dge_disc_pack_weights", packed, s)
                return packed

        return _lib.weight_image(self, "disc_packed", src, device, "Discriminator", build)

    def tap_shapes(self, batch):
        """{tap index: shape} of the tensors e3dge_disc_forward can write beside the logits."""
        out, c, size = {}, self.in_channel, self.init_size
        for i, block in enumerate(list(self.convs)[1:]):
            size //= 2
            c = block.conv2[1].weight.shape[0]
            out[i] = (batch, c, size, size)
        out[TAP_STDDEV] = (batch // stddev_group(batch, self.stddev_group),)
        out[TAP_FINAL] = (batch, 512, 4, 4)
        return out

    def _launch_forward(self, input, taps=False, save=False):
        """(logits, {tap: tensor} or None, saved state or None) of one e3dge_disc_forward; no autograd."""
        _lib.require_gpu(input, "Discriminator input")
        B, _, H, W = input.shape
        stddev_group(B, self.stddev_group)
        dev = input.device
        x = input.detach().contiguous()
        ws_bytes = _lib.query("e3dge_disc_ws_bytes", B, H, W, *self._key(), 0, exc=ValueError)
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        logits = torch.empty((B, 1), device=dev, dtype=torch.float32)
        a = _lib.DiscArgs(packed=self._packed(dev), images=x, n=B, height=H, width=W, init_size=self.init_size,
                          channel_multiplier=self.channel_multiplier, in_channels=self.input_size, logits=logits, ws=ws, ws_bytes=ws_bytes)
        tl = saved = None
        if taps:
            tl = {t: torch.empty(s, device=dev, dtype=torch.float32) for t, s in self.tap_shapes(B).items()}
            for t, v in tl.items():
                a.taps[t] = v.data_ptr()
        if save:
            saved_bytes = _lib.query("e3dge_disc_saved_bytes", B, *self._key(), exc=ValueError)
            saved = torch.empty(saved_bytes, device=dev, dtype=torch.uint8)
            a.saved, a.saved_bytes = saved, saved_bytes
        _lib.launch("e3dge_disc_forward", a)
        return logits, tl, saved

    def _launch_backward(self, saved, shape, grad_logits, stages=False):
        """(grad_images, {tap: gradient} or None) from the state a saving forward of an input of `shape` left behind."""
        B, _, H, W = shape
        dev = saved.device
        ws_bytes = _lib.query("e3dge_disc_ws_bytes", B, H, W, *self._key(), 1, exc=ValueError)
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        grad = torch.empty(shape, device=dev, dtype=torch.float32)
        g = grad_logits.detach().to(torch.float32).reshape(B, 1).contiguous()
        a = _lib.DiscBwdArgs(packed=self._packed(dev), saved=saved, saved_bytes=saved.numel(), n=B, height=H, width=W, init_size=self.init_size,
                             channel_multiplier=self.channel_multiplier, in_channels=self.input_size, grad_logits=g, grad_images=grad, ws=ws,
                             ws_bytes=ws_bytes)
        gs = None
        if stages:
            shapes = self.tap_shapes(B)
            del shapes[TAP_STDDEV]
            shapes[TAP_STEM] = (B, self.in_channel, self.init_size, self.init_size)
            gs = {t: torch.empty(s, device=dev, dtype=torch.float32) for t, s in shapes.items()}
            for t, v in gs.items():
                a.gstage[t] = v.data_ptr()
        _lib.launch("e3dge_disc_backward", a)
        return grad, gs

    def run(self, input, taps=False):
        """Debug entry of the HIP path, no autograd and no synchronisation: dict(logits, taps: {tap index: tensor} or None)."""
        with torch.no_grad():
            logits, tl, _ = self._launch_forward(input, taps)
        return dict(logits=logits, taps=tl)

    def run_backward(self, input, grad_logits, stages=False):
        """Debug entry, no autograd: the saving forward of `input`, then the backward for grad_logits (B, 1).  Returns dict(logits,
        grad, stages: {tap index: gradient} or None, saved: the saved state as a float32 tensor, saved_layout: see saved_layout())."""
        with torch.no_grad():
            logits, _, saved = self._launch_forward(input, save=True)
            grad, gs = self._launch_backward(saved, tuple(input.shape), grad_logits, stages)
        return dict(logits=logits, grad=grad, stages=gs, saved=saved.view(torch.float32))

    def saved_layout(self, batch):
        """[(name, offset in floats, shape)] of the lrelu outputs in the saved state (DcSaved, csrc/disc.hip): 'stem', 'conv1.i',
        'conv2.i' per ResBlock, 'last' (the last block's output), 'final', 'hidden'."""
        out, off = [], 0

        def take(name, shape):
            nonlocal off
            out.append((name, off, shape))
            off += (math.prod(shape) + 63) // 64 * 64

        c, size = self.in_channel, self.init_size
        take("stem", (batch, c, size, size))
        for i, block in enumerate(list(self.convs)[1:]):
            co = block.conv2[1].weight.shape[0]
            take(f"conv1.{i}", (batch, c, size, size))
            size //= 2
            take(f"conv2.{i}", (batch, co, size, size))
            c = co
        take("last", (batch, 512, 4, 4))
        take("final", (batch, 512, 4, 4))
        take("hidden", (batch, 512))
        return out

    def forward(self, input):
        if not self.uses_hip(input):
            return self.forward_torch(input)
        if torch.is_grad_enabled() and input.requires_grad:
            return _DiscriminatorFunction.apply(self, input)
        return self._launch_forward(input)[0]


class _DiscriminatorFunction(torch.autograd.Function):
    """The logits of one saving forward; the graph leads to the input image only."""

    @staticmethod
    def forward(ctx, module, input):
        logits, _, saved = module._launch_forward(input, save=True)
        ctx.module, ctx.saved, ctx.shape = module, saved, tuple(input.shape)
        ctx.set_materialize_grads(False)
        return logits

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_logits):
        if g_logits is None or not ctx.needs_input_grad[1]:
            return None, None
        return None, ctx.module._launch_backward(ctx.saved, ctx.shape, g_logits)[0]
