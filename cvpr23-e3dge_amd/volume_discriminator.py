"""The camera-pose predictor (`VolumeRenderDiscriminator`) on the HIP kernel of csrc/volume_disc.hip: a (B, 3, S, S) image in, the GAN
logit (B, 1) and the two predicted camera angles (B, 2) out -- what `image2camsettings` hands to `generate_camera_params(locations=...)`
so that `encode_ref_images` (e3dge_full_runner.py:77-183) gets a camera for an image whose camera is not known.

`VolumeRenderDiscConv2d`, `AddCoords`, `CoordConv2d`, `CoordConvLayer`, `VolumeRenderResBlock` and `VolumeRenderDiscriminator(opt)` have
the reference's constructors, sub-module names, state-dict keys and initialisation ranges (project/models/stylesdf_model.py:1193-1419), so
the `['d']` entry of a reference checkpoint loads with strict=True.  The modules are plain torch.nn layers in that arrangement.  Forward
only, frozen, eval form -- the reference calls the network under no_grad everywhere in E3DGE (train_setup.py:108-109, trainer.py:944): a GPU
float32 (B, 3, S, S) input with S == renderer_spatial_output_dim in {16, 32, 64, 128} runs the HIP kernel when the module is in eval mode,
no gradient is wanted (grad mode off, or neither the input nor a parameter requires grad) and E3DGE_VOLUME_DISC is not `torch`.  Everything
else -- CPU tensors, other dtypes and sizes, train(), gradients -- runs the module's own torch layers in the reference's order; on the CPU
they reproduce the reference bit for bit (tests/test_volume_disc_host.py against tools/gen_golden_volume_disc.py's recording).  The
encoder variants `VolumeRenderDiscriminatorEncoder` and `VolumeStyleEncoder` (:1422-1510) are not covered."""
import ctypes
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .camera_utils import generate_camera_params
from .losses import AvgPool2d
from .op import FusedLeakyReLU

CHANNELS = {2: 400, 4: 400, 8: 400, 16: 400, 32: 256, 64: 128, 128: 64}      # stylesdf_model.py:1377-1385
NATIVE_SIZES = (16, 32, 64, 128)
TAPS = _lib.VDISC_TAPS                                                       # the stem's output, then every block's


def backend():
    """'hip' or 'torch' (E3DGE_VOLUME_DISC=torch: the module's own torch layers on every input)."""
    v = os.environ.get("E3DGE_VOLUME_DISC", "") or "hip"
    if v not in ("hip", "torch"):
        raise ValueError(f"E3DGE_VOLUME_DISC={v!r}: 'hip' or 'torch'")
    return v


class VolumeRenderDiscConv2d(nn.Module):
    """stylesdf_model.py:1193-1235: Conv2d, then FusedLeakyReLU(scale=1) carrying the bias when `activate`."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, activate=False):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, bias=bias and not activate)
        self.activate = activate
        if self.activate:
            self.activation = FusedLeakyReLU(out_channels, bias=bias, scale=1)
            bias_init_coef = np.sqrt(1 / (in_channels * kernel_size * kernel_size))
            nn.init.uniform_(self.activation.bias, a=-bias_init_coef, b=bias_init_coef)

    def init_offset(self):
        self.conv.weight.data.zero_()
        self.conv.bias.data.zero_()

    def forward(self, input):
        out = self.conv(input)
        if self.activate:
            out = self.activation(out)
        return out


class AddCoords(nn.Module):
    """stylesdf_model.py:1238-1268: cat(input, yy, xx) with yy / xx = arange / (d - 1) * 2 - 1 along the rows / the columns."""

    def forward(self, input_tensor):
        batch_size_shape, channel_in_shape, dim_y, dim_x = input_tensor.shape
        xx_channel = torch.arange(dim_x, dtype=torch.float32, device=input_tensor.device).repeat(1, 1, dim_y, 1)
        yy_channel = torch.arange(dim_y, dtype=torch.float32, device=input_tensor.device).repeat(1, 1, dim_x, 1).transpose(2, 3)
        xx_channel = xx_channel / (dim_x - 1)
        yy_channel = yy_channel / (dim_y - 1)
        xx_channel = xx_channel * 2 - 1
        yy_channel = yy_channel * 2 - 1
        xx_channel = xx_channel.repeat(batch_size_shape, 1, 1, 1)
        yy_channel = yy_channel.repeat(batch_size_shape, 1, 1, 1)
        return torch.cat([input_tensor, yy_channel, xx_channel], dim=1)


class CoordConv2d(nn.Module):
    """stylesdf_model.py:1271-1299."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True):
        super().__init__()
        self.addcoords = AddCoords()
        self.conv = nn.Conv2d(in_channels + 2, out_channels, kernel_size, stride=stride, padding=padding, bias=bias)

    def forward(self, input_tensor):
        return self.conv(self.addcoords(input_tensor))


class CoordConvLayer(nn.Module):
    """stylesdf_model.py:1302-1336 (like the reference, the bias initialiser needs `activate`)."""

    def __init__(self, in_channel, out_channel, kernel_size, bias=True, activate=True):
        super().__init__()
        self.activate = activate
        self.padding = kernel_size // 2 if kernel_size > 2 else 0
        self.conv = CoordConv2d(in_channel, out_channel, kernel_size, padding=self.padding, stride=1, bias=bias and not activate)
        if activate:
            self.activation = FusedLeakyReLU(out_channel, bias=bias, scale=1)
        bias_init_coef = np.sqrt(1 / (in_channel * kernel_size * kernel_size))
        nn.init.uniform_(self.activation.bias, a=-bias_init_coef, b=bias_init_coef)

    def forward(self, input):
        out = self.conv(input)
        if self.activate:
            out = self.activation(out)
        return out


class VolumeRenderResBlock(nn.Module):
    """stylesdf_model.py:1339-1366."""

    def __init__(self, in_channel, out_channel):
        super().__init__()
        self.conv1 = CoordConvLayer(in_channel, out_channel, 3)
        self.conv2 = CoordConvLayer(out_channel, out_channel, 3)
        self.pooling = nn.AvgPool2d(2)
        self.downsample = nn.AvgPool2d(2)
        if out_channel != in_channel:
            self.skip = VolumeRenderDiscConv2d(in_channel, out_channel, 1)
        else:
            self.skip = None

    def forward(self, input):
        out = self.conv1(input)
        out = self.conv2(out)
        out = self.pooling(out)
        downsample_in = self.downsample(input)
        if self.skip is not None:
            skip_in = self.skip(downsample_in)
        else:
            skip_in = downsample_in
        out = (out + skip_in) / math.sqrt(2)
        return out


class VolumeRenderDiscriminator(nn.Module):
    """`VolumeRenderDiscriminator(opt)(input)`: (gan_preds (B, 1), viewpoints_preds (B, 2)), as the reference (stylesdf_model.py:1369-1419).
    `opt` needs renderer_spatial_output_dim (synthetic.model_opt has the scripts' value, 64)."""

    def __init__(self, opt):
        super().__init__()
        init_size = opt.renderer_spatial_output_dim
        self.init_size = init_size
        self.viewpoint_loss = True
        final_out_channel = 3 if self.viewpoint_loss else 1
        channels = CHANNELS
        convs = [VolumeRenderDiscConv2d(3, channels[init_size], 1, activate=True)]
        log_size = int(math.log(init_size, 2))
        in_channel = channels[init_size]
        for i in range(log_size - 1, 0, -1):
            out_channel = channels[2 ** i]
            convs.append(VolumeRenderResBlock(in_channel, out_channel))
            in_channel = out_channel
        self.convs = nn.Sequential(*convs)
        self.final_conv = VolumeRenderDiscConv2d(in_channel, final_out_channel, 2)
        self.in_channel = in_channel

    # ---- the torch composition, in the reference's order ----------------------------------------------------------------------------
    def forward_torch(self, input, taps=None):
        """The reference's forward; `taps`: a list that receives the stem's output and every block's."""
        out = input
        for layer in self.convs:
            out = layer(out)
            if taps is not None:
                taps.append(out)
        out = self.final_conv(out)
        gan_preds = out[:, 0:1]
        gan_preds = gan_preds.reshape(-1, 1)
        if self.viewpoint_loss:
            viewpoints_preds = out[:, 1:]
            viewpoints_preds = viewpoints_preds.reshape(-1, 2)
        else:
            viewpoints_preds = None
        return gan_preds, viewpoints_preds

    # ---- dispatch ---------------------------------------------------------------------------------------------------------------------
    def uses_hip(self, x):
        """Does forward(x) run the HIP kernel?"""
        if backend() == "torch" or self.training or self.init_size not in NATIVE_SIZES:
            return False
        if not (hasattr(x, "shape") and x.device.type == "cuda" and x.dtype == torch.float32 and x.ndim == 4):
            return False
        if not (1 <= x.shape[0] <= 256 and tuple(x.shape[1:]) == (3, self.init_size, self.init_size)):
            return False
        return not (torch.is_grad_enabled() and (getattr(x, "requires_grad", False) or any(p.requires_grad for p in _lib.params_of(self))))

    # ---- launch plumbing --------------------------------------------------------------------------------------------------------------
    def sources(self):
        """The source tensors in the order of e3dge_vdisc_pack_weights (include/e3dge_hip.h): the state dict's."""
        out = [self.convs[0].conv.weight, self.convs[0].activation.bias]
        for block in list(self.convs)[1:]:
            out += [block.conv1.conv.conv.weight, block.conv1.activation.bias, block.conv2.conv.conv.weight, block.conv2.activation.bias]
            if block.skip is not None:
                out += [block.skip.conv.weight, block.skip.conv.bias]
        return out + [self.final_conv.conv.weight, self.final_conv.conv.bias]

    def packed(self, device):
        """The packed weight image on `device`."""
        src = self.sources()

        def build():
            with torch.no_grad():
                keep = [t.detach().contiguous() for t in src]
                ptrs = (ctypes.c_void_p * len(keep))(*[t.data_ptr() for t in keep])
                image = torch.empty(_lib.query("e3dge_vdisc_packed_floats", self.init_size), device=device, dtype=torch.float32)
                _lib.launch("e3dge_vdisc_pack_weights", image, ctypes.addressof(ptrs), len(keep), self.init_size)
                return image

        return _lib.weight_image(self, "vdisc_packed", src, device, "VolumeRenderDiscriminator", build)

    def invalidate(self):
        """Drop the packed weight image (needed only after writes through `.data`)."""
        _lib.invalidate(self)

    def tap_shapes(self, n):
        """Shapes of the taps for n images: the stem's output, then every block's."""
        S = self.init_size
        shapes = [(n, CHANNELS[S], S, S)]
        for b in range(len(self.convs) - 1):
            r = S >> (b + 1)
            shapes.append((n, CHANNELS[r], r, r))
        return shapes

    def forward_hip(self, x, taps=False):
        """(gan_preds (B, 1), viewpoints_preds (B, 2), taps or None) of a GPU float32 (B, 3, S, S) input; no synchronisation."""
        _lib.require_gpu(x, "volume discriminator input")
        n, S, dev = x.shape[0], self.init_size, x.device
        image = self.packed(dev)
        x = _lib.dense(x.detach())                                   # contiguous, and realigned when a view starts off a 16-byte boundary
        ws_bytes = _lib.query("e3dge_vdisc_ws_bytes", n, S)
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        new = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
        logits, views = new(n, 1), new(n, 2)
        a = _lib.VdiscArgs(packed=image, images=x, n=n, size=S, logits=logits, viewpoints=views, ws=ws, ws_bytes=ws_bytes)
        kept = None
        if taps:
            kept = [new(*s) for s in self.tap_shapes(n)]
            for i, t in enumerate(kept):
                a.taps[i] = t.data_ptr()
        _lib.launch("e3dge_vdisc_forward", a)
        return logits, views, kept

    def run(self, x, taps=False):
        """forward(); with taps=True a third value: the list of the stem's output and every block's."""
        if self.uses_hip(x):
            logits, views, kept = self.forward_hip(x, taps)
        else:
            kept = [] if taps else None
            logits, views = self.forward_torch(x, kept)
        return (logits, views, kept) if taps else (logits, views)

    def forward(self, input):
        return self.run(input)


_pool_64 = AvgPool2d((64, 64))


def image2camsettings(volume_discriminator, images, camera_opt, renderer_output_size, is_thumb=False):
    """trainer.py:935-948 with :971-987: pool the images to 64 x 64 (unless is_thumb), predict the two camera angles under no_grad, and
    return generate_camera_params(renderer_output_size, ..., locations=pred, return_calibs=True): the dict `G_pred_latents` and
    `netLocal.query` take.  camera_opt: uniform, azim, elev, fov, dist_radius (synthetic.rendering_opt().camera)."""
    thumb_img = images if is_thumb else _pool_64(images)
    assert thumb_img.shape[-1] == 64, 'check volume_discriminator input img dim'
    with torch.no_grad():
        _, pred_locations = volume_discriminator(thumb_img)
    return generate_camera_params(renderer_output_size, images.device, images.shape[0], locations=pred_locations, uniform=camera_opt.uniform,
                                  azim_range=camera_opt.azim, elev_range=camera_opt.elev, fov_ang=camera_opt.fov,
                                  dist_radius=camera_opt.dist_radius, return_calibs=True)
