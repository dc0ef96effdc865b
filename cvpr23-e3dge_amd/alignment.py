"""The 2-D residual aligner (ADA) on the HIP kernels of csrc/aligner.hip: cat(res_gt, up(thumb)) (B, 6, 256, 256) in, the `aligned_res`
image (B, 3, 256, 256) that the second `netLocal.filter` of the novel-view forward consumes out
(project/trainers/E3DGE/e3dge_full_runner.py:138, :255-264).

`ResidualAligner` has the reference's constructor, sub-module names and state-dict keys
(project/models/helper_modules/alignment_old.py:316-398, helpers.py:14-80, :161-201), so the `grid_align` entry of the reference's
checkpoint loads with strict=True.  The module is built from plain torch.nn layers in that arrangement.  Forward only, eval form: a GPU
float32 (B, 6, 256, 256) input runs the HIP kernels when the module is in eval mode (BatchNorm on its running statistics), the options
are aligner_norm_type 'batch' without demodulation and no gradient is wanted (grad mode off, or neither the input nor a parameter
requires grad).  Everything else -- CPU tensors, other dtypes, train(), gradients, 'instance' / 'none' / demodulation, other sizes (which
raise in torch.cat as the reference does), E3DGE_ALIGNER=torch -- runs the module's own torch layers in the reference's order; on the CPU
they reproduce the reference bit for bit (tests/test_aligner_host.py against tools/gen_golden_aligner.py's recording)."""
import ctypes
import functools
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

SIZE, IN_CHANNELS = 256, 6
STAGES = {                                                         # (in, depth, stride) of every bottleneck_IR unit (alignment_old.py:345-375)
    "conv_layer2": ((16, 32, 2), (32, 32, 1), (32, 32, 1)),
    "conv_layer3": ((32, 48, 2), (48, 48, 1), (48, 48, 1)),
    "conv_layer4": ((48, 64, 2), (64, 64, 1), (64, 64, 1)),
    "dconv_layer1": ((112, 64, 1), (64, 32, 1), (32, 32, 1)),
    "dconv_layer2": ((64, 32, 1), (32, 16, 1), (16, 16, 1)),
    "dconv_layer3": ((32, 16, 1), (16, 3, 1), (3, 3, 1)),
}
TAPS = ("feat1", "feat2", "feat3", "feat4", "dfea1", "dfea2", "dfea3")       # every stage's output, before its up-sampling
TAP_SHAPES = ((16, 256), (32, 128), (48, 64), (64, 32), (32, 64), (16, 128), (3, 256))


class DemodulatedConv2d(nn.Module):
    """helpers.py:14-80: a convolution whose filters are scaled to unit norm.  The weight keeps the reference's shape (1, out, in, kh, kw);
    the reference repeats the scaled filters per sample and runs one grouped convolution over the batch, which is this convolution."""

    def __init__(self, in_channel, out_channel, kernel_size=3, stride=1, padding=0, bias=False, dilation=1):
        super().__init__()
        ks = kernel_size if isinstance(kernel_size, tuple) else (kernel_size, kernel_size)
        self.weight = nn.Parameter(torch.randn(1, out_channel, in_channel, *ks))
        self.bias = nn.Parameter(torch.randn(out_channel)) if bias else None
        self.stride, self.padding, self.dilation, self.eps = stride, padding, dilation, 1e-8

    def forward(self, x):
        w = self.weight[0]
        w = w * torch.rsqrt(w.pow(2).sum([1, 2, 3], keepdim=True) + self.eps)
        return F.conv2d(x, w, self.bias, self.stride, self.padding, self.dilation)


def get_norm_layer(norm_type='instance'):
    """alignment_old.py:16-40: batch (affine, running statistics) | instance (neither) | none."""
    if norm_type == 'batch':
        return functools.partial(nn.BatchNorm2d, affine=True, track_running_stats=True)
    if norm_type == 'instance':
        return functools.partial(nn.InstanceNorm2d, affine=False, track_running_stats=False)
    if norm_type == 'none':
        return lambda channels: nn.Identity()
    raise NotImplementedError('normalization layer [%s] is not found' % norm_type)


class _Unit(nn.Module):
    """helpers.py:161-201: bottleneck_IR with a choice of normalisation and convolution (encoders._Unit(se=False) for 'batch')."""

    def __init__(self, cin, depth, stride, norm_layer, demodulate):
        super().__init__()
        conv2d = DemodulatedConv2d if demodulate else nn.Conv2d
        if cin == depth:
            self.shortcut_layer = nn.MaxPool2d(1, stride)
        else:
            self.shortcut_layer = nn.Sequential(conv2d(cin, depth, (1, 1), stride, bias=False), norm_layer(depth))
        self.res_layer = nn.Sequential(norm_layer(cin), conv2d(cin, depth, (3, 3), (1, 1), 1, bias=False), nn.PReLU(depth),
                                       conv2d(depth, depth, (3, 3), stride, 1, bias=False), norm_layer(depth))

    def forward(self, x):
        shortcut = self.shortcut_layer(x)
        res = self.res_layer(x)
        return res + shortcut


def up2_bilinear(x):
    """F.interpolate(x, size=(2 H, 2 W), mode='bilinear') (align_corners=False) restated: ATen's source index 0.5 (dst + 0.5) - 0.5
    clamped at 0 gives the taps 0.25 / 0.75 with clamped edges.  The weights are exact; what differs between ATen's CPU kernels is the
    order of the roundings, by shape (found on torch 2.x with ATen's non-vectorised kernels; tests/test_aligner_host.py pins it):
        output plane above 4096 elements   hy (hx a + lx b) + ly (hx c + lx d)                 the separable form; aln_up2_kernel's, at every size
        up to 4096, fewer than 8 channels   ((hy hx) a + (hy lx) b) + (ly hx) c) + (ly lx) d
        up to 4096, 8 channels or more      ((ly hx) c + (ly lx) d) + (hy lx) b) + (hy hx) a
    with a, b the upper and c, d the lower pair of neighbours.  The forms differ by an ulp or two of the result."""
    H, W = x.shape[-2:]

    def taps(n):
        src = (0.5 * (torch.arange(2 * n, dtype=x.dtype, device=x.device) + 0.5) - 0.5).clamp(min=0)
        i0 = src.floor().long().clamp(max=n - 1)
        i1 = i0 + (i0 < n - 1).long()
        l1 = (src - i0.to(x.dtype)).clamp(0, 1)
        return i0, i1, 1 - l1, l1
    y0, y1, hy, ly = taps(H)
    x0, x1, hx, lx = taps(W)
    hy, ly = hy[:, None], ly[:, None]
    upper, lower = x[..., y0, :], x[..., y1, :]
    a, b, c, d = upper[..., x0], upper[..., x1], lower[..., x0], lower[..., x1]
    if 4 * H * W > 4096:
        return hy * (hx * a + lx * b) + ly * (hx * c + lx * d)
    if x.shape[-3] < 8:
        return (((hy * hx) * a + (hy * lx) * b) + (ly * hx) * c) + (ly * lx) * d
    return (((ly * hx) * c + (ly * lx) * d) + (hy * lx) * b) + (hy * hx) * a


class ResidualAligner(nn.Module):
    """`ResidualAligner(opt_training)(x)`: x (B, 6, 256, 256) = cat(res_gt, thumb at 256^2) -> (B, 3, 256, 256).  `opt_training` needs
    aligner_demodulate and aligner_norm_type (synthetic.aligner_opt has the scripts' values)."""

    def __init__(self, opt_training=None):
        super().__init__()
        self.demodulate = bool(opt_training.aligner_demodulate)
        self.norm_type = 'none' if self.demodulate else opt_training.aligner_norm_type
        norm_layer = get_norm_layer(self.norm_type)
        conv2d = DemodulatedConv2d if self.demodulate else nn.Conv2d
        self.conv_layer1 = nn.Sequential(conv2d(IN_CHANNELS, 16, (3, 3), 1, 1, bias=False), norm_layer(16), nn.PReLU(16))
        for name, units in STAGES.items():
            setattr(self, name, nn.Sequential(*[_Unit(*u, norm_layer=norm_layer, demodulate=self.demodulate) for u in units]))

    # ---- the torch composition, in the reference's order ----------------------------------------------------------------------------
    def forward_torch(self, x, taps=None):
        """alignment_old.py:377-398.  `taps`: a dict that receives the tensors of TAPS."""
        feat1 = self.conv_layer1(x)
        feat2 = self.conv_layer2(feat1)
        feat3 = self.conv_layer3(feat2)
        feat4 = self.conv_layer4(feat3)
        up4 = F.interpolate(feat4, size=(64, 64), mode='bilinear')
        dfea1 = self.dconv_layer1(torch.cat((up4, feat3), 1))
        up1 = F.interpolate(dfea1, size=(128, 128), mode='bilinear')
        dfea2 = self.dconv_layer2(torch.cat((up1, feat2), 1))
        up2 = F.interpolate(dfea2, size=(256, 256), mode='bilinear')
        dfea3 = self.dconv_layer3(torch.cat((up2, feat1), 1))
        if taps is not None:
            taps.update(zip(TAPS, (feat1, feat2, feat3, feat4, dfea1, dfea2, dfea3)))
        return dfea3

    # ---- dispatch ---------------------------------------------------------------------------------------------------------------------
    def native_options(self):
        """Do the kernels cover this module's options?"""
        return self.norm_type == 'batch' and not self.demodulate

    def _runs_hip(self, *inputs):
        """inputs: the 6-channel tensor, or (res_gt, thumb) with 3 channels each and a 64^2 or 256^2 thumb."""
        if os.environ.get("E3DGE_ALIGNER", "") == "torch" or self.training or not self.native_options():
            return False
        channels = 0
        for i, t in enumerate(inputs):
            if not (torch.is_tensor(t) and t.device.type == "cuda" and t.dtype == torch.float32 and t.ndim == 4):
                return False
            if t.device != inputs[0].device or t.shape[0] != inputs[0].shape[0] or t.shape[0] < 1 or t.shape[0] > 256:
                return False
            sizes = ((SIZE, SIZE), (SIZE // 4, SIZE // 4)) if i == 1 else ((SIZE, SIZE),)
            if tuple(t.shape[-2:]) not in sizes:
                return False
            channels += t.shape[1]
        if channels != IN_CHANNELS:
            return False
        return not (torch.is_grad_enabled() and (any(t.requires_grad for t in inputs) or any(p.requires_grad for p in _lib.params_of(self))))

    # ---- launch plumbing --------------------------------------------------------------------------------------------------------------
    def sources(self):
        """The source tensors in the order of e3dge_aligner_pack (include/e3dge_hip.h)."""
        bn = lambda m: [m.weight, m.bias, m.running_mean, m.running_var]
        out = [self.conv_layer1[0].weight] + bn(self.conv_layer1[1]) + [self.conv_layer1[2].weight]
        for name in STAGES:
            for u in getattr(self, name):
                r = u.res_layer
                out += bn(r[0]) + [r[1].weight, r[2].weight, r[3].weight] + bn(r[4])
                if isinstance(u.shortcut_layer, nn.Sequential):
                    out += [u.shortcut_layer[0].weight] + bn(u.shortcut_layer[1])
        return out

    def packed(self, device):
        """The packed weight image on `device`, from the shared weight-image cache."""
        src = self.sources()

        def build():
            with torch.no_grad():
                keep = [t.detach().contiguous() for t in src]
                ptrs = (ctypes.c_void_p * len(keep))(*[t.data_ptr() for t in keep])
                image = torch.empty(_lib.query("e3dge_aligner_packed_floats"), device=device, dtype=torch.float32)
                _lib.launch("e3dge_aligner_pack", image, image.numel(), ctypes.addressof(ptrs), len(keep))
                return image

        return _lib.weight_image(self, "aligner_packed", src, device, "ResidualAligner", build)

    def invalidate(self):
        """Drop the packed weight image (needed only after writes through `.data`)."""
        _lib.invalidate(self)

    def forward_hip(self, res_gt, thumb=None, taps=None):
        """The output of the GPU float32 inputs: res_gt (B, 6, 256, 256) alone, or res_gt (B, c, 256, 256) with thumb (B, 6 - c, 256, 256) or
        (B, 6 - c, 64, 64) (read at nearest x4); no concatenation, no synchronisation.  `taps`: a dict that receives the tensors of TAPS."""
        _lib.require_gpu(res_gt, "aligner input")
        n, dev = res_gt.shape[0], res_gt.device
        image = self.packed(dev)
        res_gt = res_gt.detach().contiguous()
        up4 = 0
        if thumb is not None:
            _lib.require_gpu(thumb, "aligner thumb")
            thumb = thumb.detach().contiguous()
            up4 = int(thumb.shape[-1] != SIZE)
        ws_bytes = _lib.query("e3dge_aligner_workspace_bytes", n)
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        out = torch.empty((n, 3, SIZE, SIZE), device=dev, dtype=torch.float32)
        a = _lib.AlignerArgs(packed=image, packed_floats=image.numel(), res_gt=res_gt, thumb=thumb, n=n, size=SIZE, split=res_gt.shape[1],
                             thumb_up4=up4, out=out, ws=ws, ws_bytes=ws_bytes)
        if taps is not None:
            for i, (name, (c, s)) in enumerate(zip(TAPS[:-1], TAP_SHAPES)):
                taps[name] = torch.empty((n, c, s, s), device=dev, dtype=torch.float32)
                a.taps[i] = taps[name].data_ptr()
            taps[TAPS[-1]] = out
        _lib.launch("e3dge_aligner_forward", a)
        return out

    def forward(self, x):
        if not self._runs_hip(x):
            return self.forward_torch(x)
        return self.forward_hip(x)

    def align(self, res_gt, thumb):
        """The call site's composition forward(cat(res_gt, F.interpolate(thumb, (256, 256)))) (e3dge_full_runner.py:255-259, nearest), bit
        for bit.  On the native path with a 64^2 or 256^2 thumb neither the up-sampled thumb nor the 6-channel tensor is materialised."""
        if self._runs_hip(res_gt, thumb):
            return self.forward_hip(res_gt, thumb)
        return self.forward(torch.cat((res_gt, F.interpolate(thumb, (SIZE, SIZE))), dim=1))
