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
they reproduce the reference bit for bit (tests/test_aligner_host.py against tools/gen_golden_aligner.py's recording).

Trainable form, opt-in: `ResidualAligner(opt_training, differentiable=True)` (also an attribute, or `differentiable_aligner` in the
options; off by default, and with it off nothing above changes).  With it on, a call with grad mode on and a wanted gradient -- an input
or a tensor of sources() requires grad -- is one autograd node (_AlignerNode) on csrc/aligner_train.h, in the form of `self.training`: the
eval form, or the train form with BatchNorm on batch statistics and nn.BatchNorm2d's update of the running buffers.  Its backward returns
the gradient to the input(s) and to every parameter that requires grad, once (a second differentiation raises).  DESIGN.md 4.17b."""
import ctypes
import functools
import os

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

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


def _walk():
    """One walk of STAGES with the sizes it implies (a dconv stage runs on the up-sampled map): the (channels, size) of every tap, and of
    every BatchNorm in the order of ResidualAligner.sources() a getter from the module and the H W of its input."""
    taps, size = [(16, SIZE)], SIZE
    norms = [(lambda m: m.conv_layer1[1], size * size)]
    for name, units in STAGES.items():
        size *= 2 if name.startswith("dconv") else 1
        for i, (cin, depth, stride) in enumerate(units):
            out = size // stride
            norms += [(lambda m, name=name, i=i: getattr(m, name)[i].res_layer[0], size * size),
                      (lambda m, name=name, i=i: getattr(m, name)[i].res_layer[4], out * out)]
            if cin != depth:
                norms.append((lambda m, name=name, i=i: getattr(m, name)[i].shortcut_layer[1], out * out))
            size = out
        taps.append((units[-1][1], size))
    return tuple(taps), tuple(norms)


TAP_SHAPES, _NORMS = _walk()


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

    def __init__(self, opt_training=None, differentiable=None):
        super().__init__()
        if differentiable is None:                                   # from the options; off by default
            differentiable = getattr(opt_training, 'differentiable_aligner', False)
        self.differentiable = bool(differentiable)
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
        if os.environ.get("E3DGE_ALIGNER", "") == "torch" or self.training or not self.native_options() or not self._covers(*inputs):
            return False
        return not (torch.is_grad_enabled() and (any(t.requires_grad for t in inputs) or any(p.requires_grad for p in _lib.params_of(self))))

    def _covers(self, *inputs):
        """The device, dtype, shape and batch checks on the one-tensor or (res_gt, thumb) form."""
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
        return channels == IN_CHANNELS

    def _runs_hip_grad(self, *inputs):
        """Does this call run as one autograd node on the kernels (csrc/aligner_train.h)?  Opt-in (`differentiable`), grad mode on, the
        kernels' options and inputs, a wanted gradient (an input or a source tensor requires grad) and, in train(), a numeric momentum on
        every BatchNorm (momentum=None, the cumulative average, stays on the torch layers)."""
        if not (self.differentiable and torch.is_grad_enabled() and self.native_options()) or os.environ.get("E3DGE_ALIGNER", "") == "torch":
            return False
        if not self._covers(*inputs):
            return False
        if not (any(t.requires_grad for t in inputs) or any(t.requires_grad for t in self.sources())):
            return False
        return not self.training or all(m.momentum is not None for m in self.batch_norms())

    # ---- launch plumbing --------------------------------------------------------------------------------------------------------------
    def sources(self):
        """The source tensors in the order of e3dge_aligner_pack (include/e3dge_hip.h).  The (dict, key) slots are listed once per module
        and looked up per call, so a replaced Parameter is still seen; invalidate() drops the listing (after a sub-module was replaced)."""
        return [d[k] for d, k in self._slots()]

    def _slots(self):
        slots = self.__dict__.get("_source_slots")
        if slots is None:
            slots = []
            bn = lambda m: [(m._parameters, "weight"), (m._parameters, "bias"), (m._buffers, "running_mean"), (m._buffers, "running_var")]
            w = lambda m: [(m._parameters, "weight")]
            slots += w(self.conv_layer1[0]) + bn(self.conv_layer1[1]) + w(self.conv_layer1[2])
            for name in STAGES:
                for u in getattr(self, name):
                    r = u.res_layer
                    slots += bn(r[0]) + w(r[1]) + w(r[2]) + w(r[3]) + bn(r[4])
                    if isinstance(u.shortcut_layer, nn.Sequential):
                        slots += w(u.shortcut_layer[0]) + bn(u.shortcut_layer[1])
            self.__dict__["_source_slots"] = slots
        return slots

    def running_statistic_slots(self):
        """The positions of the running buffers in sources(): the slots that point into a module's _buffers; listed once."""
        out = self.__dict__.get("_statistic_slots")
        if out is None:
            buffers = {id(m._buffers) for m in self.modules()}
            out = self.__dict__["_statistic_slots"] = frozenset(i for i, (d, _) in enumerate(self._slots()) if id(d) in buffers)
        return out

    def batch_norms(self):
        """The BatchNorms in the order of sources() (the order of the statistics buffer of e3dge_aligner_forward_saving); listed once."""
        out = self.__dict__.get("_batch_norms")
        if out is None:
            out = self.__dict__["_batch_norms"] = [get(self) for get, _ in _NORMS]
        return out

    def packed(self, device):
        """The packed weight image on `device`, from the shared weight-image cache."""
        return self._image(device, "aligner_packed", "e3dge_aligner_packed_floats", "e3dge_aligner_pack", self.sources())

    def packed_train(self, device):
        """The same image for the train form, which reads no running statistics from it: keyed on the parameters alone, so that the
        buffer update of every train-form forward does not rebuild it (an optimiser step does).  The buffers are still packed, so they
        are checked like the parameters."""
        return self._image(device, "aligner_packed_train", "e3dge_aligner_packed_floats", "e3dge_aligner_pack", list(_lib.params_of(self)))

    def packed_t(self, device):
        """The transposed, tap-flipped images of the convolutions beside it: the data gradients' operand."""
        return self._image(device, "aligner_packed_t", "e3dge_aligner_packed_t_floats", "e3dge_aligner_pack_t", [t for t in self.sources() if t.ndim == 4])

    def _image(self, device, slot, size_entry, pack_entry, keyed):
        src = self.sources()

        def build():
            with torch.no_grad():
                keep = [t.detach().contiguous() for t in src]
                ptrs = (ctypes.c_void_p * len(keep))(*[t.data_ptr() for t in keep])
                image = torch.empty(_lib.query(size_entry), device=device, dtype=torch.float32)
                _lib.launch(pack_entry, image, image.numel(), ctypes.addressof(ptrs), len(keep))
                return image

        for t in src:                                                # (weight_image checks what it is keyed on; the pack kernels read all of these)
            if t.device != device or t.dtype != torch.float32:
                raise RuntimeError(f"ResidualAligner weights must be float32 on the inputs' device {device} (got {t.dtype} on {t.device})")
        return _lib.weight_image(self, slot, keyed, device, "ResidualAligner", build)

    def invalidate(self):
        """Drop the packed weight images (needed only after writes through `.data`) and the listings of sources() and batch_norms()."""
        for listing in ("_source_slots", "_statistic_slots", "_batch_norms"):
            self.__dict__.pop(listing, None)
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

    def _node(self, res_gt, thumb):
        """The call as one autograd node; in train() the running buffers are then updated, once, from the statistics it computed."""
        train = bool(self.training)
        out, stats = _AlignerNode.apply(self, train, res_gt, thumb, *self.sources())
        if train:
            _update_running_buffers(self.batch_norms(), stats, res_gt.shape[0])
        return out

    def forward(self, x):
        if self._runs_hip_grad(x):
            return self._node(x, None)
        if not self._runs_hip(x):
            return self.forward_torch(x)
        return self.forward_hip(x)

    def align(self, res_gt, thumb):
        """The call site's composition forward(cat(res_gt, F.interpolate(thumb, (256, 256)))) (e3dge_full_runner.py:255-259, nearest), bit
        for bit.  On the native path with a 64^2 or 256^2 thumb neither the up-sampled thumb nor the 6-channel tensor is materialised."""
        if self._runs_hip_grad(res_gt, thumb):
            return self._node(res_gt, thumb)
        if self._runs_hip(res_gt, thumb):
            return self.forward_hip(res_gt, thumb)
        return self.forward(torch.cat((res_gt, F.interpolate(thumb, (SIZE, SIZE))), dim=1))


class _AlignerNode(torch.autograd.Function):
    """(output, batch statistics) of ResidualAligner on the kernels as one autograd node, from the 6-channel tensor (thumb None) or from
    (res_gt, thumb).  params: ResidualAligner.sources(), so that autograd asks for their gradients (the running buffers among them get
    None).  Forward: e3dge_aligner_forward_saving in the form `train` -- on running statistics the plain forward's output bit for bit, the
    statistics empty; on batch statistics the (channels, 2) float64 (mean, biased variance) pairs, not differentiable, from which the
    caller updates the running buffers (the node itself writes to none of its inputs).  Backward: e3dge_aligner_backward, once (a second
    differentiation raises); each gradient only where autograd asks for it.  Every tensor the backward reads again -- the inputs, gamma,
    the slopes and, in the eval form, the running statistics -- is saved with save_for_backward: an in-place change between forward and
    backward raises, as under torch.  Inputs, upstream gradient and source tensors are handed over dense (_lib.dense)."""
    branches = None                                                  # debug: a list that receives every forward's e3dge_aligner_branch_bytes buffer
    taps = None                                                      # debug: a dict that receives the tensors of TAPS of every forward

    @staticmethod
    def forward(ctx, module, train, res_gt, thumb, *params):
        n, dev = res_gt.shape[0], res_gt.device
        image, image_t = (module.packed_train(dev) if train else module.packed(dev)), module.packed_t(dev)
        res_gt = _lib.dense(res_gt.detach())
        thumb = None if thumb is None else _lib.dense(thumb.detach())
        up4 = int(thumb is not None and thumb.shape[-1] != SIZE)
        saved = torch.empty(_lib.query("e3dge_aligner_saved_bytes", n), device=dev, dtype=torch.uint8)
        out = torch.empty((n, 3, SIZE, SIZE), device=dev, dtype=torch.float32)
        stats = torch.empty((_sizes(module)[0] if train else 0, 2), device=dev, dtype=torch.float64)
        keep = [_lib.dense(p.detach(), align=4) for p in params]     # (the kernels read gamma, beta and the slopes one float at a time)
        ptrs = (ctypes.c_void_p * len(keep))(*[p.data_ptr() for p in keep])
        a = _lib.AlignerSaveArgs(packed=image, packed_floats=image.numel(), src=ctypes.addressof(ptrs), n_src=len(keep), train=int(train), res_gt=res_gt,
                                 thumb=thumb, n=n, size=SIZE, split=res_gt.shape[1], thumb_up4=up4, out=out, saved=saved, saved_bytes=saved.numel(),
                                 stats=stats if train else None, stats_doubles=stats.numel())
        if _AlignerNode.taps is not None:
            for i, (name, (c, s)) in enumerate(zip(TAPS, TAP_SHAPES)):
                _AlignerNode.taps[name] = torch.empty((n, c, s, s), device=dev, dtype=torch.float32)
                a.taps[i] = _AlignerNode.taps[name].data_ptr()
        _lib.launch("e3dge_aligner_forward_saving", a)
        if _AlignerNode.branches is not None:
            branch = torch.empty(_lib.query("e3dge_aligner_branch_count", n), device=dev, dtype=torch.uint8)
            _lib.launch("e3dge_aligner_branch_bytes", branch, branch.numel(), image, image.numel(), saved, saved.numel(), n, int(train))
            _AlignerNode.branches.append(branch)
        # what the backward reads again of the source tensors: everything but, in the train form, the running statistics (the caller
        # updates those right after this forward; the train form's backward reads the batch statistics instead)
        read_again = [i for i in range(len(params)) if not (train and i in module.running_statistic_slots())]
        ctx.read_again, ctx.offsets = read_again, _sizes(module)[1]
        ctx.save_for_backward(saved, image, image_t, stats, res_gt, *([] if thumb is None else [thumb]), *[params[i] for i in read_again])
        ctx.form = (n, bool(train), thumb is not None, up4, len(params))
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, _g_stats):
        n, train, two, up4, n_src = ctx.form
        saved, image, image_t, stats, res_gt, *rest = ctx.saved_tensors
        thumb = rest.pop(0) if two else None
        dev = saved.device
        params = [None] * n_src
        for i, p in zip(ctx.read_again, rest):
            params[i] = p
        nothing = (None,) * (4 + n_src)
        if g_out is None:
            return nothing
        g_out = _lib.dense(g_out.to(torch.float32))
        want = [bool(w) for w in ctx.needs_input_grad[4:]]
        want_input = bool(ctx.needs_input_grad[2] or (two and ctx.needs_input_grad[3]))
        ws_bytes = _lib.query("e3dge_aligner_bwd_workspace_bytes", n)
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        offsets = ctx.offsets
        grads = torch.empty(offsets[-1], device=dev, dtype=torch.float32) if any(want) else None
        d_res_gt = torch.empty_like(res_gt) if want_input else None
        d_thumb = torch.empty_like(thumb) if want_input and two else None
        keep = [image if p is None else _lib.dense(p.detach(), align=4) for p in params]   # (a slot the train form never reads: any valid address)
        ptrs = (ctypes.c_void_p * n_src)(*[p.data_ptr() for p in keep])
        flags = (ctypes.c_uint8 * n_src)(*[int(w) for w in want])
        a = _lib.AlignerBwdArgs(packed=image, packed_floats=image.numel(), packed_t=image_t, packed_t_floats=image_t.numel(), src=ctypes.addressof(ptrs),
                                want=ctypes.addressof(flags), n_src=n_src, train=int(train), res_gt=res_gt, thumb=thumb, g_out=g_out, n=n, size=SIZE,
                                split=res_gt.shape[1], thumb_up4=up4, want_input=int(want_input), saved=saved, saved_bytes=saved.numel(),
                                stats=stats if train else None, d_res_gt=d_res_gt, d_thumb=d_thumb, grads=grads,
                                grad_floats=0 if grads is None else grads.numel(), ws=ws, ws_bytes=ws_bytes)
        _lib.launch("e3dge_aligner_backward", a)
        out = [grads[offsets[i]:offsets[i + 1]].view(p.shape) if w else None for i, (p, w) in enumerate(zip(params, want))]
        return (None, None, d_res_gt if ctx.needs_input_grad[2] else None, d_thumb if two and ctx.needs_input_grad[3] else None, *out)


def _sizes(module):
    """(BatchNorm channels in all, the slot of every source tensor in the gradient buffer with the buffer's size last): asked of the
    library once per module, kept with its weight images."""
    def build():
        return (_lib.query("e3dge_aligner_stats_channels"), tuple(_lib.query("e3dge_aligner_grad_offset", i) for i in range(_lib.ALIGNER_SOURCES + 1)))
    return _lib.cached(module, "aligner_sizes", (), build)


_TABLES = {}                                                         # (device, momenta, batch) -> the per-channel float64 factors of the buffer update


def _update_running_buffers(bns, stats, n):
    """nn.BatchNorm2d's buffer update of every BatchNorm from the (mean, biased variance) float64 pairs of one forward, in a handful of
    launches whatever the number of BatchNorms: running <- (1 - m) running + m stat, the variance through M / (M - 1).  The per-channel
    factors are built once per (device, momenta, batch)."""
    with torch.no_grad():
        sizes = [m.num_features for m in bns]
        momenta = tuple(float(m.momentum) for m in bns)
        key = (stats.device, momenta, n)
        if key not in _TABLES:
            momentum = torch.tensor([v for v, c in zip(momenta, sizes) for _ in range(c)], dtype=torch.float64)
            count = torch.tensor([float(p * n) for p, c in zip(_bn_planes(len(bns)), sizes) for _ in range(c)], dtype=torch.float64)
            _TABLES[key] = torch.stack((momentum, momentum * count / (count - 1)), 1).to(stats.device)
        scaled = (stats * _TABLES[key]).float()
        mean, var = scaled[:, 0].split(sizes), scaled[:, 1].split(sizes)
        keep = [1.0 - v for v in momenta]
        torch._foreach_mul_([m.running_mean for m in bns], keep)
        torch._foreach_add_([m.running_mean for m in bns], list(mean))
        torch._foreach_mul_([m.running_var for m in bns], keep)
        torch._foreach_add_([m.running_var for m in bns], list(var))
        torch._foreach_add_([m.num_batches_tracked for m in bns], 1)


def _bn_planes(count):
    """H W of every BatchNorm's input, in the order of ResidualAligner.batch_norms()."""
    assert len(_NORMS) == count
    return [plane for _, plane in _NORMS]
