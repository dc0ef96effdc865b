"""The hourglass image filter of the local branch: what PRODUCES local_data_batch['feature_maps'] = {'ref', 'que'}, each a
(B, 256, H / 4, W / 4) map, from a residual image and a depth map (trainers/E3DGE/e3dge_full_runner.py:166-171, 264-269).

    feats = cat(residual_conv(residual_images), depth_conv(depth_feat))        3 -> 32 and 1 -> 32 channels, reflect padding, instance norm
    outputs, tmpx, normx = image_filter(feats)                                 HGFilter: 7x7 stride-2 stem, three ConvBlocks, num_stack HourGlasses

The classes have the reference's constructor arguments, attribute names and state-dict keys (vendor/pifu/lib/model/HGFilters.py,
vendor/pifu/lib/net_util.py:399-453, vendor/pifu/lib/model/HGPIFuGANNetResidualInputResnetFC.py:19-76; `conv` of
models/helper_modules/helpers.py:432-455), so that class's `netLocal` state dict loads with strict=True; the code is
this package's own.  A GPU float32 input runs csrc/hgfilter.hip when no gradient is wanted (grad mode off, or neither the input nor a
parameter requires grad) and the options are norm='group', hg_down='ave_pool', hg_input_channel=64, hourglass_dim=256.  With
`differentiable=True` (opt-in; the constructors' keyword, an attribute, or `differentiable_filter` in the options) a wanted gradient --
to the residual image, the depth map or HGFilter's own 64-channel input, or to any parameter the forward reads -- runs there too: one
autograd node whose forward is the state-saving form of the same launches and whose backward is csrc/hgfilter_bwd.h, once
differentiable (a second differentiation raises).  With trainable weights the packed images are rebuilt after every optimiser step
(_lib.weight_image).  Everything else -- CPU tensors, other dtypes and options, E3DGE_HGFILTER=torch, `differentiable` off -- runs the
torch composition below under plain autograd: F.conv2d, F.group_norm, F.interpolate and the rest in the reference's order."""
import ctypes
import os

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib

FEATURE_CHANNELS = 256


def _opt(opt, name, default=None):
    v = opt.get(name, None) if hasattr(opt, 'get') else getattr(opt, name, None)
    return default if v is None else v


def _norm(kind, channels):
    if kind == 'batch':
        return nn.BatchNorm2d(channels)
    if kind == 'group':
        return nn.GroupNorm(32, channels)
    raise NotImplementedError(f"norm={kind!r}: 'batch' or 'group'")


def _conv3x3(cin, cout):
    return nn.Conv2d(cin, cout, 3, 1, 1, bias=False)


class ConvBlock(nn.Module):
    """out = cat(o1, o2, o3) + residual with o_i = conv_i(relu(bn_i(o_{i-1}))), o_0 = x; the residual is x, or
    conv1x1(relu(bn4(x))) where the channel count changes.  bn4 always exists and is also `downsample.0`."""

    def __init__(self, in_planes, out_planes, norm='batch'):
        super().__init__()
        half, quarter = int(out_planes / 2), int(out_planes / 4)
        self.conv1, self.conv2, self.conv3 = _conv3x3(in_planes, half), _conv3x3(half, quarter), _conv3x3(quarter, quarter)
        self.bn1, self.bn2, self.bn3, self.bn4 = _norm(norm, in_planes), _norm(norm, half), _norm(norm, quarter), _norm(norm, in_planes)
        if in_planes != out_planes:
            self.downsample = nn.Sequential(self.bn4, nn.ReLU(True), nn.Conv2d(in_planes, out_planes, 1, 1, bias=False))
        else:
            self.downsample = None

    def forward(self, x):
        o1 = self.conv1(F.relu(self.bn1(x), True))
        o2 = self.conv2(F.relu(self.bn2(o1), True))
        o3 = self.conv3(F.relu(self.bn3(o2), True))
        out = torch.cat((o1, o2, o3), 1)
        out += x if self.downsample is None else self.downsample(x)
        return out


class HourGlass(nn.Module):
    """level(d, x) = b1_d(x) + bicubic_x2(b3_d(inner(b2_d(avg_pool(x))))), inner = level(d - 1) or b2_plus_1."""

    def __init__(self, num_modules, depth, num_features, norm='batch'):
        super().__init__()
        self.num_modules, self.depth, self.features, self.norm = num_modules, depth, num_features, norm
        self._make(depth)

    def _make(self, level):
        block = lambda: ConvBlock(self.features, self.features, norm=self.norm)
        self.add_module(f'b1_{level}', block())
        self.add_module(f'b2_{level}', block())
        if level > 1:
            self._make(level - 1)
        else:
            self.add_module(f'b2_plus_{level}', block())
        self.add_module(f'b3_{level}', block())

    def _level(self, level, x, probe=None):
        up1 = self._modules[f'b1_{level}'](x)
        low = self._modules[f'b2_{level}'](F.avg_pool2d(x, 2, stride=2))
        low = self._level(level - 1, low, probe) if level > 1 else self._modules[f'b2_plus_{level}'](low)
        low = self._modules[f'b3_{level}'](low)
        up2 = F.interpolate(low, scale_factor=2, mode='bicubic', align_corners=True)
        if probe is not None:
            probe.append((level, up1, up2))
        return up1 + up2

    def forward(self, x, probe=None):
        return self._level(self.depth, x, probe)


def _block_sources(b):
    out = [b.bn1.weight, b.bn1.bias, b.conv1.weight, b.bn2.weight, b.bn2.bias, b.conv2.weight, b.bn3.weight, b.bn3.bias, b.conv3.weight]
    if b.downsample is not None:
        out += [b.bn4.weight, b.bn4.bias, b.downsample[2].weight]
    return out


def _level_sources(hg, level):
    m = hg._modules
    inner = _level_sources(hg, level - 1) if level > 1 else _block_sources(m[f'b2_plus_{level}'])
    return _block_sources(m[f'b1_{level}']) + _block_sources(m[f'b2_{level}']) + inner + _block_sources(m[f'b3_{level}'])


class HGFilter(nn.Module):
    """`HGFilter(opt)(x)` = (outputs: one (B, hourglass_dim, H / 4, W / 4) map per stack, tmpx: the stem's activation, detached,
    normx: the pooled first ConvBlock) for x (B, opt.hg_input_channel, H, W)."""

    def __init__(self, opt, differentiable=False):
        super().__init__()
        self.opt = opt
        self.differentiable = bool(differentiable)
        self.num_modules = int(_opt(opt, 'num_stack'))
        self.num_hourglass = int(_opt(opt, 'num_hourglass'))
        self.front_nets = None      # (residual_conv, depth_conv) of the ResidualImageFilter that owns this filter: packed into the same image
        norm, down, dim = _opt(opt, 'norm'), _opt(opt, 'hg_down'), int(_opt(opt, 'hourglass_dim'))
        self.conv1 = nn.Conv2d(int(_opt(opt, 'hg_input_channel')), 64, 7, 2, 3)
        self.bn1 = _norm(norm, 64)
        if down == 'conv64':
            self.conv2 = ConvBlock(64, 64, norm)
            self.down_conv2 = nn.Conv2d(64, 128, 3, 2, 1)
        elif down == 'conv128':
            self.conv2 = ConvBlock(64, 128, norm)
            self.down_conv2 = nn.Conv2d(128, 128, 3, 2, 1)
        elif down == 'ave_pool':
            self.conv2 = ConvBlock(64, 128, norm)
        else:
            raise NameError('Unknown Fan Filter setting!')
        self.conv3 = ConvBlock(128, 128, norm)
        self.conv4 = ConvBlock(128, 256, norm)
        for i in range(self.num_modules):
            self.add_module(f'm{i}', HourGlass(1, self.num_hourglass, 256, norm))
            self.add_module(f'top_m_{i}', ConvBlock(256, 256, norm))
            self.add_module(f'conv_last{i}', nn.Conv2d(256, 256, 1))
            self.add_module(f'bn_end{i}', _norm(norm, 256))
            self.add_module(f'l{i}', nn.Conv2d(256, dim, 1))
            if i < self.num_modules - 1:
                self.add_module(f'bl{i}', nn.Conv2d(256, 256, 1))
                self.add_module(f'al{i}', nn.Conv2d(dim, 256, 1))

    # ---- which path ---------------------------------------------------------------------------------------------------------------
    def hip_options(self):
        """The options csrc/hgfilter.hip covers."""
        o = self.opt
        return (_opt(o, 'norm') == 'group' and _opt(o, 'hg_down') == 'ave_pool' and int(_opt(o, 'hourglass_dim')) == FEATURE_CHANNELS and
                int(_opt(o, 'hg_input_channel')) == 64 and 1 <= self.num_modules <= _lib.HGF_MAX_STACK and 1 <= self.num_hourglass <= 4)

    def hip_shape(self, n, height, width):
        m = 4 << self.num_hourglass
        return 1 <= n <= 4096 and m <= height <= 4096 and m <= width <= 4096 and height % m == 0 and width % m == 0

    def _covers(self, x):
        if os.environ.get("E3DGE_HGFILTER", "hip") == "torch" or not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32):
            return False
        return x.ndim == 4 and x.shape[1] == 64 and self.hip_options() and self.hip_shape(x.shape[0], x.shape[2], x.shape[3])

    def _runs_hip(self, x):
        if not self._covers(x):
            return False
        return not (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in _lib.params_of(self))))

    def _runs_hip_grad(self, x):
        """The autograd node on the kernels: opted in, and a gradient is wanted: to the input or to a parameter the forward reads."""
        return (self.differentiable and torch.is_grad_enabled() and self._covers(x) and
                (x.requires_grad or any(p.requires_grad for p in self.sources())))

    # ---- launch plumbing ------------------------------------------------------------------------------------------------------------
    def sources(self):
        """The filter's source tensors in the order of e3dge_hgf_pack_weights (include/e3dge_hip.h)."""
        m = self._modules
        out = [self.conv1.weight, self.conv1.bias, self.bn1.weight, self.bn1.bias]
        out += _block_sources(self.conv2) + _block_sources(self.conv3) + _block_sources(self.conv4)
        for i in range(self.num_modules):
            out += _level_sources(m[f'm{i}'], self.num_hourglass) + _block_sources(m[f'top_m_{i}'])
            out += [m[f'conv_last{i}'].weight, m[f'conv_last{i}'].bias, m[f'bn_end{i}'].weight, m[f'bn_end{i}'].bias, m[f'l{i}'].weight, m[f'l{i}'].bias]
            if i < self.num_modules - 1:
                out += [m[f'bl{i}'].weight, m[f'bl{i}'].bias, m[f'al{i}'].weight, m[f'al{i}'].bias]
        return out

    def packed(self, device):
        """The packed weight image on `device`: one per filter.  The front nets' part of it is written when the filter belongs to a
        ResidualImageFilter (`front_nets`) and stays unwritten, and unread, otherwise."""
        return self._image(device, "hgf_packed", "e3dge_hgf_packed_floats", "e3dge_hgf_pack_weights")

    def packed_t(self, device):
        """The transposed image beside it: every convolution's data-gradient image, for the backward."""
        return self._image(device, "hgf_packed_t", "e3dge_hgf_packed_t_floats", "e3dge_hgf_pack_weights_t")

    def _image(self, device, slot, size_entry, pack_entry):
        front = [t for net in self.front_nets for t in _front_sources(net)] if self.front_nets else None
        src = self.sources() + list(front or ())
        S, D = self.num_modules, self.num_hourglass

        def build():
            with torch.no_grad():
                keep = [t.detach().contiguous() for t in src]
                n = len(keep) - (len(front) if front else 0)
                filt = (ctypes.c_void_p * n)(*[t.data_ptr() for t in keep[:n]])
                fr = (ctypes.c_void_p * len(front))(*[t.data_ptr() for t in keep[n:]]) if front else None
                image = torch.empty(_lib.query(size_entry, S, D), device=device, dtype=torch.float32)
                _lib.launch(pack_entry, image, ctypes.addressof(filt), n, ctypes.addressof(fr) if front else None, S, D)
                return image

        return _lib.weight_image(self, slot, src, device, "HGFilter", build)

    def invalidate(self):
        """Drop the packed weight images (needed only after writes through `.data`)."""
        _lib.invalidate(self)

    def forward_hip(self, x, ws=None, saved=None):
        """The forward on csrc/hgfilter.hip, no synchronisation; x (B, 64, H, W) float32 on the GPU.  ws: a workspace of
        e3dge_hgf_ws_bytes that the caller already holds (filter_maps: the front nets' and the filter's are one).  saved: a buffer of
        e3dge_hgf_saved_bytes: the state-saving form of the same launches, for the backward."""
        _lib.require_gpu(x, "HGFilter input")
        n, c, H, W = x.shape
        if c != 64 or not self.hip_options() or not self.hip_shape(n, H, W):
            raise ValueError(f"HGFilter on HIP takes (B, 64, H, W) with H, W multiples of {4 << self.num_hourglass} and the options norm='group', "
                             f"hg_down='ave_pool', hg_input_channel=64, hourglass_dim=256 (got {tuple(x.shape)})")
        dev, S, D = x.device, self.num_modules, self.num_hourglass
        x = x.detach().contiguous()
        image = self.packed(dev)
        ws_bytes = _lib.query("e3dge_hgf_ws_bytes", n, H, W, S, D)
        if ws is None:
            ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        new = lambda ch, h, w: torch.empty((n, ch, h, w), device=dev, dtype=torch.float32)
        outs, tmpx, normx = [new(FEATURE_CHANNELS, H // 4, W // 4) for _ in range(S)], new(64, H // 2, W // 2), new(128, H // 4, W // 4)
        a = _lib.HgfArgs(packed=image, input=x, n=n, height=H, width=W, num_stack=S, num_hourglass=D, tmpx=tmpx, normx=normx, ws=ws, ws_bytes=ws_bytes)
        for i, t in enumerate(outs):
            a.outputs[i] = t.data_ptr()
        if saved is None:
            _lib.launch("e3dge_hgf_forward", a)
        else:
            _lib.launch("e3dge_hgf_forward_saving", a, saved, saved.numel())
        return outs, tmpx, normx

    def forward_torch(self, x, probe=None):
        """The torch composition, in the reference's order.  probe: a list that receives (stack, level, up1, up2) of every HourGlass level."""
        m = self._modules
        x = F.relu(self.bn1(self.conv1(x)), True)
        tmpx = x
        down = _opt(self.opt, 'hg_down')
        if down == 'ave_pool':
            x = F.avg_pool2d(self.conv2(x), 2, stride=2)
        elif down in ('conv64', 'conv128'):
            x = self.down_conv2(self.conv2(x))
        else:
            raise NameError('Unknown Fan Filter setting!')
        normx = x
        previous = self.conv4(self.conv3(x))
        outputs = []
        for i in range(self.num_modules):
            levels = [] if probe is not None else None
            ll = m[f'top_m_{i}'](m[f'm{i}'](previous, levels))
            if probe is not None:
                probe += [(i,) + lv for lv in levels]
            ll = F.relu(m[f'bn_end{i}'](m[f'conv_last{i}'](ll)), True)
            out = m[f'l{i}'](ll)
            outputs.append(out)
            if i < self.num_modules - 1:
                previous = previous + m[f'bl{i}'](ll) + m[f'al{i}'](out)
        return outputs, tmpx.detach(), normx

    def forward(self, x):
        if self._runs_hip_grad(x):
            *outs, tmpx, normx = _FilterNode.apply(self, x, None, *self.sources())
            return list(outs), tmpx, normx
        return self.forward_hip(x) if self._runs_hip(x) else self.forward_torch(x)


class _FilterNode(torch.autograd.Function):
    """(*outputs, tmpx, normx) of HGFilter on the kernels from its 64-channel input (depth None), or from the residual image and the depth
    map through the front nets.  params: HGFilter.sources() and, with a depth map, the front nets' sixteen tensors, so that autograd asks
    for their gradients.  Forward: the state-saving form of the plain forward's launches, bit-identical results.  Backward:
    csrc/hgfilter_bwd.h, once; absent upstream gradients are skipped, tmpx has none, and each gradient is computed only where autograd
    asks for it (the parameter gradients as a whole: one buffer in the order of the sources)."""
    branches = None                                                  # debug: a list that receives every backward's e3dge_hgf_branch_bytes buffer

    @staticmethod
    def forward(ctx, hg, x, depth, *params):
        ctx.set_materialize_grads(False)
        n, _, H, W = x.shape
        dev, S, D = x.device, hg.num_modules, hg.num_hourglass
        saved = torch.empty(_lib.query("e3dge_hgf_saved_bytes", n, H, W, S, D), device=dev, dtype=torch.uint8)
        image = hg.packed(dev)
        ws, first, second = None, x.detach().contiguous(), None
        x = first                                                    # (what the stem's weight gradient reads again must be dense too)
        if depth is not None:
            ws_bytes = _lib.query("e3dge_hgf_ws_bytes", n, H, W, S, D)
            ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
            feats = torch.empty((n, 64, H, W), device=dev, dtype=torch.float32)
            second = depth.detach().contiguous()
            _lib.launch("e3dge_hgf_front_saving", image, first, second, feats, n, H, W, S, D, ws, ws_bytes, saved, saved.numel())
            x = feats
        outs, tmpx, normx = hg.forward_hip(x, ws, saved)
        ctx.mark_non_differentiable(tmpx)
        wants = any(ctx.needs_input_grad[3:])
        keep = [x.detach(), first, second] + list(outs) if wants else []                 # what the weight gradients read beside the saved state
        ctx.save_for_backward(tmpx, normx, saved, image, hg.packed_t(dev), *[t for t in keep if t is not None])
        ctx.shape = (n, H, W, S, D, depth is not None)
        ctx.numels = [p.numel() for p in params]
        ctx.shapes = [tuple(p.shape) for p in params]
        return (*outs, tmpx, normx)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        n, H, W, S, D, front = ctx.shape
        g_outs, g_normx = grads[:S], grads[S + 1]
        nothing = (None,) * (3 + len(ctx.numels))
        if g_normx is None and all(g is None for g in g_outs):
            return nothing
        tmpx, normx, saved, image, image_t, *kept = ctx.saved_tensors
        dev = tmpx.device
        dense = lambda g: None if g is None else g.to(torch.float32).contiguous()
        g_outs, g_normx = [dense(g) for g in g_outs], dense(g_normx)
        ws_bytes = _lib.query("e3dge_hgf_bwd_ws_bytes", n, H, W, S, D)
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        g_input = torch.empty((n, 64, H, W), device=dev, dtype=torch.float32)
        branch = None
        if _FilterNode.branches is not None:                         # debug: the ReLU branches of this run (tests: a branch-pinned truth)
            branch = torch.zeros(_lib.query("e3dge_hgf_branch_bytes", n, H, W, S, D), device=dev, dtype=torch.uint8)
            _FilterNode.branches.append(branch)
        wants = any(ctx.needs_input_grad[3:])
        buf = torch.zeros(_lib.query("e3dge_hgf_grad_floats", S, D), device=dev, dtype=torch.float32) if wants else None
        a = _lib.HgfBwdArgs(packed=image, packed_t=image_t, saved=saved, saved_bytes=saved.numel(), tmpx=tmpx, normx=normx, n=n, height=H, width=W,
                            num_stack=S, num_hourglass=D, g_normx=g_normx, g_input=g_input, ws=ws, ws_bytes=ws_bytes, branch=branch,
                            branch_bytes=0 if branch is None else branch.numel(), grads=buf)
        for i, g in enumerate(g_outs):
            a.g_outputs[i] = None if g is None else g.data_ptr()
        first = second = None
        if wants:
            a.input, first = kept[0], kept[1]
            second = kept[2] if front else None
            for i, t in enumerate(kept[3 if front else 2:]):
                a.outputs[i] = t.data_ptr()
        _lib.launch("e3dge_hgf_backward", a)
        g_first, g_second = g_input if ctx.needs_input_grad[1] else None, None
        if front:
            g_first = torch.empty((n, 3, H, W), device=dev, dtype=torch.float32) if ctx.needs_input_grad[1] else None
            g_second = torch.empty((n, 1, H, W), device=dev, dtype=torch.float32) if ctx.needs_input_grad[2] else None
            if g_first is not None or g_second is not None or wants:
                _lib.launch("e3dge_hgf_front_backward", image, image_t, saved, saved.numel(), g_input, g_first, g_second, n, H, W, S, D, ws, ws_bytes, branch,
                            0 if branch is None else branch.numel(), buf, first if wants else None, second if wants else None)
        if not wants:
            return (None, g_first, g_second) + nothing[3:]
        # which sources an upstream gradient reaches: without a stack's gradient only the stem and conv2 (through normx); otherwise
        # everything up to the last stack with a gradient, without that stack's bl / al; the front nets always
        s_max = max([i for i, g in enumerate(g_outs) if g is not None], default=-1)
        per_stack = (3 * D + 2) * 9 + 6
        reached = 16 if s_max < 0 else 37 + (s_max + 1) * per_stack + 4 * s_max
        n_filter = 37 + S * per_stack + 4 * (S - 1)
        out, off = [], 0
        for i, (numel, shape) in enumerate(zip(ctx.numels, ctx.shapes)):
            live = ctx.needs_input_grad[3 + i] and (i < reached or i >= n_filter)
            out.append(buf[off:off + numel].view(shape) if live else None)
            off += numel
        return (None, g_first, g_second, *out)


class _FrontResidual(nn.Module):
    """x + conv3x3(relu(IN(conv3x3(relu(IN(x)))))) with reflect padding and affine instance norms: keys conv.{0,2,3,5}.*"""

    def __init__(self, dim):
        super().__init__()
        inorm = lambda: nn.InstanceNorm2d(dim, track_running_stats=False, affine=True)
        conv = lambda: nn.Conv2d(dim, dim, 3, 1, 1, bias=False, padding_mode='reflect')
        self.conv = nn.Sequential(inorm(), nn.ReLU(True), conv(), inorm(), nn.ReLU(True), conv())
        self.short_cut = None

    def forward(self, x):
        return self.conv(x) + x


def _front_net(cin, dim=32):
    return nn.Sequential(nn.Conv2d(cin, dim, 3, 1, 1, bias=False, padding_mode='reflect'), _FrontResidual(dim),
                         nn.Conv2d(dim, dim, 1, 1, bias=False, padding_mode='reflect'))


def _front_sources(net):
    c = net[1].conv
    return [net[0].weight, c[0].weight, c[0].bias, c[2].weight, c[3].weight, c[3].bias, c[5].weight, net[2].weight]


class _ChannelConv(nn.Module):
    """elu(IN(conv(x))), reflect padding, a convolution with bias and an affine instance norm: keys conv.{weight,bias}, bn.{weight,bias}"""

    def __init__(self, cin, cout, kernel_size, stride):
        super().__init__()
        self.kernel_size = kernel_size
        self.conv = nn.Conv2d(cin, cout, kernel_size, stride, (kernel_size - 1) // 2, padding_mode='reflect')
        self.bn = nn.InstanceNorm2d(cout, track_running_stats=False, affine=True)

    def forward(self, x):
        return F.elu(self.bn(self.conv(x)), inplace=True)


class ResidualImageFilter(nn.Module):
    """The image-filter half of the reference's `netLocal` (HGPIFuNetGANResidualResnetFC): residual_conv, depth_conv,
    downsample_channel_conv (512 -> 64; parameters only: the reference raises where it would be used) and
    image_filter = HGFilter(local_options).  filter() keeps
    im_feat_dict[feat_key] = [the last stack's map], tmpx and normx, as the reference does."""

    def __init__(self, local_options, differentiable=None):
        super().__init__()
        self.local_options = local_options
        if differentiable is None:                                   # LocalFilterHead / SirenLocalGlobal: from the options; off by default
            differentiable = bool(_opt(local_options, 'differentiable_filter', False))
        self.image_filter = HGFilter(local_options, differentiable)
        self.downsample_channel_conv = _ChannelConv(512, 64, 3, 1)
        self.depth_conv = _front_net(1)
        self.residual_conv = _front_net(3)
        self.image_filter.front_nets = (self.residual_conv, self.depth_conv)
        self.im_feat_dict = {}
        self.tmpx = self.normx = None

    def invalidate(self):
        _lib.invalidate(self)

    @property
    def differentiable(self):
        return self.image_filter.differentiable

    @differentiable.setter
    def differentiable(self, value):
        self.image_filter.differentiable = bool(value)

    def _covers(self, image, depth):
        hg = self.image_filter
        if depth is None or os.environ.get("E3DGE_HGFILTER", "hip") == "torch":
            return False
        for t, ch in ((image, 3), (depth, 1)):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.ndim == 4 and t.shape[1] == ch):
                return False
        if depth.device != image.device or depth.shape[0] != image.shape[0] or depth.shape[2:] != image.shape[2:]:
            return False
        return hg.hip_options() and hg.hip_shape(image.shape[0], image.shape[2], image.shape[3])

    def _trainable(self):
        return any(p.requires_grad for mod in (self.residual_conv, self.depth_conv, self.image_filter) for p in _lib.params_of(mod))

    def _runs_hip(self, image, depth):
        if not self._covers(image, depth):
            return False
        if not torch.is_grad_enabled():
            return True
        return not (image.requires_grad or depth.requires_grad or self._trainable())

    def _runs_hip_grad(self, image, depth):
        if not (self.differentiable and torch.is_grad_enabled() and self._covers(image, depth)):
            return False
        used = self.image_filter.sources() + _front_sources(self.residual_conv) + _front_sources(self.depth_conv)
        return image.requires_grad or depth.requires_grad or any(p.requires_grad for p in used)

    def filter_maps(self, residual_images, depth_feat=None):
        """(outputs, tmpx, normx) of the image filter for the residual image and the depth map."""
        if self._runs_hip_grad(residual_images, depth_feat):
            params = self.image_filter.sources() + _front_sources(self.residual_conv) + _front_sources(self.depth_conv)
            *outs, tmpx, normx = _FilterNode.apply(self.image_filter, residual_images, depth_feat, *params)
            return list(outs), tmpx, normx
        if self._runs_hip(residual_images, depth_feat):
            hg = self.image_filter
            n, _, H, W = residual_images.shape
            dev, S, D = residual_images.device, hg.num_modules, hg.num_hourglass
            image = hg.packed(dev)
            ws_bytes = _lib.query("e3dge_hgf_ws_bytes", n, H, W, S, D)
            ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
            feats = torch.empty((n, 64, H, W), device=dev, dtype=torch.float32)
            _lib.launch("e3dge_hgf_front", image, residual_images.detach().contiguous(), depth_feat.detach().contiguous(), feats, n, H, W, S, D, ws,
                        ws_bytes)
            return hg.forward_hip(feats, ws)
        feats = self.residual_conv(residual_images)
        if depth_feat is not None:
            feats = torch.cat((feats, self.depth_conv(depth_feat)), 1)
        return self.image_filter(feats)

    def filter(self, residual_images, depth_feat=None, ref_feats=None, feat_key='ref_view', return_feat=False):
        if ref_feats is not None:
            raise DeprecationWarning('deprecated in editing version model.')
        outputs, self.tmpx, self.normx = self.filter_maps(residual_images, depth_feat)
        self.im_feat_dict[feat_key] = [outputs[-1]]
        if return_feat:
            return self.im_feat_dict[feat_key]
