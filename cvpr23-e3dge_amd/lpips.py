"""LPIPS (AlexNet) perceptual distance on the HIP kernels of csrc/lpips.hip.

The module has the reference's call surface and state-dict keys (project/losses/lpips/lpips.py:8-39, networks.py:23-89), so a
state dict saved from the reference's `LPIPS` loads with strict=True:

    net.mean, net.std, net.layers.{0,3,6,8,10}.{weight,bias}, lin.{0..4}.1.weight

Unlike the reference it never downloads anything: a fresh module holds zeros, and `load_pretrained(alexnet_file, lin_file)` reads two
LOCAL files (a torchvision AlexNet state dict and richzhang's alex.pth).

The gradient with respect to the two images (csrc/lpips_bwd.h; the weights stay frozen, as the reference freezes them) is opt-in:
`LPIPS(..., differentiable=True)` or `module.differentiable = True`.  Then, with grad enabled and an input that requires grad, the
call goes through one autograd Function whose forward is the same launch (bit-identical values) and keeps its workspace -- the five
activations and two pooled maps -- for the backward; the backward is once-differentiable.  With the switch off (the default) inputs
that require grad raise NotImplementedError, as before."""
import ctypes

import torch
import torch.nn as nn

from . import _lib

CHANNELS = (64, 192, 384, 256, 256)
# torchvision's AlexNet `features`: index -> (C_in, C_out, kernel, stride, padding); the other slots are ReLU / MaxPool2d(3, 2)
CONVS = {0: (3, 64, 11, 4, 2), 3: (64, 192, 5, 1, 2), 6: (192, 384, 3, 1, 1), 8: (384, 256, 3, 1, 1), 10: (256, 256, 3, 1, 1)}
CONV_SLOTS = tuple(CONVS)
MIN_SIZE = 31                     # the smallest height / width for which every layer has an output


def tap_shapes(height, width):
    """[(C, H, W)] of the five taps for an input of that size (floor-mode pooling)."""
    h1, w1 = (height + 4 - 11) // 4 + 1, (width + 4 - 11) // 4 + 1
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    h3, w3 = (h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1
    return [(64, h1, w1), (192, h2, w2), (384, h3, w3), (256, h3, w3), (256, h3, w3)]


class _AlexFeatures(nn.Module):
    """Holder of the reference's `net.*` keys (networks.py:35-47, 80-89).  `layers` has torchvision's thirteen slots so that the conv
    indices are 0, 3, 6, 8, 10; only the parameters are used, the arithmetic is csrc/lpips.hip."""

    def __init__(self):
        super().__init__()
        self.register_buffer('mean', torch.tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer('std', torch.tensor([.458, .448, .450])[None, :, None, None])
        slots = []
        for i in range(13):
            if i in CONVS:
                ci, co, k, s, p = CONVS[i]
                conv = nn.Conv2d(ci, co, k, s, p)
                nn.init.zeros_(conv.weight)
                nn.init.zeros_(conv.bias)
                slots.append(conv)
            else:
                slots.append(nn.MaxPool2d(3, 2) if i in (2, 5, 12) else nn.ReLU(inplace=True))
        self.layers = nn.Sequential(*slots)
        self.target_layers = [2, 5, 8, 10, 12]
        self.n_channels_list = list(CHANNELS)
        for p in self.parameters():
            p.requires_grad = False


class _LinLayers(nn.ModuleList):
    """networks.py:23-32: Sequential(Identity, Conv2d(C, 1, 1, bias=False)) per tap, frozen."""

    def __init__(self, n_channels_list):
        super().__init__([nn.Sequential(nn.Identity(), nn.Conv2d(nc, 1, 1, 1, 0, bias=False)) for nc in n_channels_list])
        for p in self.parameters():
            nn.init.zeros_(p)
            p.requires_grad = False


class LPIPS(nn.Module):
    """`LPIPS(device)(x, y)`: the scalar of lpips.py:39 for x, y (B, 3, H, W) float32 on the GPU, H, W >= 31.
    `forward(x, y, per_image=True)` returns the (B,) distances whose mean that scalar is."""

    def __init__(self, device=None, net_type='alex', version='0.1', differentiable=False):
        assert version in ['0.1'], 'v0.1 is only supported now'
        if net_type in ('vgg', 'squeeze'):
            raise NotImplementedError(f"LPIPS net_type '{net_type}': only the AlexNet backbone has HIP kernels")
        if net_type != 'alex':
            raise NotImplementedError('choose net_type from [alex, squeeze, vgg].')
        super().__init__()
        self.net = _AlexFeatures()
        self.lin = _LinLayers(self.net.n_channels_list)
        self.differentiable = bool(differentiable)
        if device is not None:
            self.to(device)

    def load_pretrained(self, alexnet_file, lin_file):
        """Weights from two local files: a torchvision AlexNet state dict (`features.N.weight / bias`; classifier entries are ignored)
        and richzhang's LPIPS v0.1 alex.pth (`linN.model.1.weight`, renamed as the reference does, utils.py:31-37)."""
        alex = torch.load(alexnet_file, map_location='cpu')
        lin = torch.load(lin_file, map_location='cpu')
        sd = {}
        for k, v in alex.items():
            if k.startswith('features.'):
                sd['net.layers.' + k[len('features.'):]] = v
        for k, v in lin.items():
            sd['lin.' + k.replace('lin', '').replace('model.', '')] = v
        missing, unexpected = self.load_state_dict(sd, strict=False)
        if unexpected or [m for m in missing if m not in ('net.mean', 'net.std')]:
            raise RuntimeError(f"load_pretrained: missing {missing}, unexpected {unexpected}")
        return self

    # ---- launch plumbing --------------------------------------------------------------------------------------------------------
    def _sources(self):
        convs = [self.net.layers[i] for i in CONV_SLOTS]
        return [c.weight for c in convs] + [c.bias for c in convs] + [l[1].weight for l in self.lin]

    def _packed(self, device):
        src = self._sources()

        def build():
            with torch.no_grad():
                keep = [t.detach().contiguous() for t in src]
                packed = torch.empty(_lib.query("e3dge_lpips_packed_floats"), device=device, dtype=torch.float32)
                ptrs = [(ctypes.c_void_p * 5)(*[t.data_ptr() for t in keep[5 * i:5 * i + 5]]) for i in range(3)]
                _lib.launch("e3dge_lpips_pack_weights", packed, *ptrs)
                return packed

        return _lib.weight_image(self, "lpips_packed", src, device, "LPIPS", build)

    def _packed_t(self, device):
        """The transposed weight image of the backward, on the same sources as the forward image."""
        src = self._sources()

        def build():
            with torch.no_grad():
                keep = [t.detach().contiguous() for t in src[:5]]
                packed_t = torch.empty(_lib.query("e3dge_lpips_packed_t_floats"), device=device, dtype=torch.float32)
                _lib.launch("e3dge_lpips_pack_weights_t", packed_t, (ctypes.c_void_p * 5)(*[t.data_ptr() for t in keep]))
                return packed_t

        return _lib.weight_image(self, "lpips_packed_t", src, device, "LPIPS", build)

    def _norm(self):
        """net.mean / net.std as host floats (read back once per buffer update, not per call)."""
        src = [self.net.mean, self.net.std]
        return _lib.cached(self, "lpips_norm", src, lambda: ([float(v) for v in src[0].reshape(-1).tolist()],
                                                             [float(v) for v in src[1].reshape(-1).tolist()]))

    def _check(self, x, y):
        if not (torch.is_tensor(x) and torch.is_tensor(y)):
            raise TypeError("LPIPS takes two tensors")
        if x.ndim != 4 or x.shape[1] != 3 or x.shape != y.shape:
            raise ValueError(f"LPIPS takes two (B, 3, H, W) tensors of one shape (got {tuple(x.shape)} and {tuple(y.shape)})")
        B, _, H, W = x.shape
        if B < 1 or H < MIN_SIZE or W < MIN_SIZE:
            raise ValueError(f"LPIPS needs B >= 1 and H, W >= {MIN_SIZE} (got {tuple(x.shape)})")

    def _launch_forward(self, x, y, per_layer=False, taps=False):
        """(result dict of run(), workspace tensor): the one forward launch sequence, for detached GPU inputs."""
        _lib.require_gpu(x, "LPIPS x")
        _lib.require_gpu(y, "LPIPS y")
        dev = x.device
        if y.device != dev:
            raise RuntimeError(f"LPIPS x is on {dev}, y on {y.device}")
        B, _, H, W = x.shape
        packed = self._packed(dev)
        mean, std = self._norm()
        x, y = x.detach().contiguous(), y.detach().contiguous()
        ws_bytes = _lib.query("e3dge_lpips_ws_bytes", B, H, W)
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        out = torch.empty(B + 1, device=dev, dtype=torch.float32)
        a = _lib.LpipsArgs(packed=packed, x=x, y=y, batch=B, height=H, width=W, per_image=out, mean_out=out.data_ptr() + 4 * B,
                           ws=ws, ws_bytes=ws_bytes)
        a.mean[:] = mean
        a.std[:] = std
        res = dict(per_image=out[:B], mean=out[B], per_layer=None, taps=None)
        if per_layer:
            res['per_layer'] = torch.empty((B, 5), device=dev, dtype=torch.float32)
            a.per_layer = res['per_layer']
        if taps:
            res['taps'] = [torch.empty((2 * B, c, h, w), device=dev, dtype=torch.float32) for c, h, w in tap_shapes(H, W)]
            for i, t in enumerate(res['taps']):
                a.taps[i] = t.data_ptr()
        _lib.launch("e3dge_lpips_forward", a)
        return res, ws

    def _launch_backward(self, ws, shape, upstream, want_x, want_y, gpre=False):
        """(grad_x or None, grad_y or None, the five G_l or None) from the workspace `ws` a forward of inputs of `shape` left behind;
        upstream (B,) = dL / d per_image."""
        B, _, H, W = shape
        dev = ws.device
        both = bool(want_x and want_y)
        ws_bytes = _lib.query("e3dge_lpips_bwd_ws_bytes", B, H, W, int(both))
        bws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        gx = torch.empty(shape, device=dev, dtype=torch.float32) if want_x else None
        gy = torch.empty(shape, device=dev, dtype=torch.float32) if want_y else None
        a = _lib.LpipsBwdArgs(packed=self._packed(dev), packed_t=self._packed_t(dev), fwd_ws=ws, fwd_ws_bytes=ws.numel(), batch=B, height=H,
                              width=W, upstream=upstream, grad_x=gx, grad_y=gy, ws=bws, ws_bytes=ws_bytes)
        a.std[:] = self._norm()[1]
        g = None
        if gpre:
            g = [torch.empty(((2 if both else 1) * B, c, h, w), device=dev, dtype=torch.float32) for c, h, w in tap_shapes(H, W)]
            for i, t in enumerate(g):
                a.gpre[i] = t.data_ptr()
        _lib.launch("e3dge_lpips_backward", a)
        return gx, gy, g

    def run(self, x, y, per_layer=False, taps=False):
        """The forward with its side outputs: dict(per_image (B,), mean (), per_layer (B, 5) or None, taps: five (2B, C, H, W) tensors
        of the normalised features (x's images first) or None).  With `differentiable` set, grad enabled and an input that requires
        grad, per_image and mean carry the graph (per_layer and taps never do)."""
        self._check(x, y)
        if torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
            if not self.differentiable:
                raise NotImplementedError("LPIPS backward is off for this module: set `differentiable = True` (or construct it with "
                                          "differentiable=True), call under torch.no_grad(), or detach the inputs")
            _lib.require_gpu(x, "LPIPS x")
            _lib.require_gpu(y, "LPIPS y")
            side = {}
            per_image, mean = _LpipsFunction.apply(self, side, bool(per_layer), bool(taps), x, y)
            return dict(per_image=per_image, mean=mean, per_layer=side['per_layer'], taps=side['taps'])
        return self._launch_forward(x, y, per_layer, taps)[0]

    def run_backward(self, x, y, upstream, want_x=True, want_y=False, gpre=False):
        """Debug entry: the forward, then the backward for upstream (B,) = dL / d per_image.  Returns (grad_x or None, grad_y or None,
        the five gradients G_l at the conv pre-activations -- (n, C_l, H_l, W_l) of the images that get a gradient, x's first -- or
        None).  Needs no autograd and records none."""
        self._check(x, y)
        if not (want_x or want_y):
            raise ValueError("LPIPS.run_backward: neither gradient is wanted")
        _lib.require_gpu(upstream, "LPIPS upstream")
        if upstream.shape != (x.shape[0],):
            raise ValueError(f"LPIPS upstream must be ({x.shape[0]},) (got {tuple(upstream.shape)})")
        with torch.no_grad():
            _, ws = self._launch_forward(x, y)
            return self._launch_backward(ws, tuple(x.shape), upstream.detach().contiguous(), want_x, want_y, gpre)

    def forward(self, x, y, per_image=False):
        res = self.run(x, y)
        return res['per_image'] if per_image else res['mean']


class _LpipsFunction(torch.autograd.Function):
    """(per_image, mean) of one forward launch; the backward reads the workspace that launch left behind."""

    @staticmethod
    def forward(ctx, module, side, per_layer, taps, x, y):
        res, ws = module._launch_forward(x, y, per_layer, taps)
        side['per_layer'], side['taps'] = res['per_layer'], res['taps']
        ctx.module, ctx.ws, ctx.shape = module, ws, tuple(x.shape)
        ctx.set_materialize_grads(False)
        # two tensors of their own storage would cost a copy: the two views of one buffer are returned as they are
        return res['per_image'], res['mean']

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_per_image, g_mean):
        want_x, want_y = ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        if (g_per_image is None and g_mean is None) or not (want_x or want_y):
            return None, None, None, None, None, None
        B = ctx.shape[0]
        if g_mean is None:
            u = g_per_image
        else:
            u = (g_mean / B).expand(B)
            if g_per_image is not None:
                u = g_per_image + u
        u = u.to(torch.float32).contiguous()
        gx, gy, _ = ctx.module._launch_backward(ctx.ws, ctx.shape, u, want_x, want_y)
        return None, None, None, None, gx, gy
