"""LPIPS (AlexNet) perceptual distance on the HIP kernels of csrc/lpips.hip.

The module has the reference's call surface and state-dict keys (project/losses/lpips/lpips.py:8-39, networks.py:23-89), so a
state dict saved from the reference's `LPIPS` loads with strict=True:

    net.mean, net.std, net.layers.{0,3,6,8,10}.{weight,bias}, lin.{0..4}.1.weight

Unlike the reference it never downloads anything: a fresh module holds zeros, and `load_pretrained(alexnet_file, lin_file)` reads two
LOCAL files (a torchvision AlexNet state dict and richzhang's alex.pth).  Only the forward exists; inputs that require grad raise."""
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

    def __init__(self, device=None, net_type='alex', version='0.1'):
        assert version in ['0.1'], 'v0.1 is only supported now'
        if net_type in ('vgg', 'squeeze'):
            raise NotImplementedError(f"LPIPS net_type '{net_type}': only the AlexNet backbone has HIP kernels")
        if net_type != 'alex':
            raise NotImplementedError('choose net_type from [alex, squeeze, vgg].')
        super().__init__()
        self.net = _AlexFeatures()
        self.lin = _LinLayers(self.net.n_channels_list)
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
        for t in src:
            if t.device != device or t.dtype != torch.float32:
                raise RuntimeError(f"LPIPS weights must be float32 on the inputs' device {device} (got {t.dtype} on {t.device})")

        def build():
            with torch.no_grad():
                keep = [t.detach().contiguous() for t in src]
                packed = torch.empty(_lib.load().e3dge_lpips_packed_floats(), device=device, dtype=torch.float32)
                ptrs = [(ctypes.c_void_p * 5)(*[t.data_ptr() for t in keep[5 * i:5 * i + 5]]) for i in range(3)]
                _lib.launch("e3dge_lpips_pack_weights", packed, *ptrs)
                return packed

        return _lib.cached(self, "lpips_packed", src, build)

    def _norm(self):
        """net.mean / net.std as host floats (read back once per buffer update, not per call)."""
        src = [self.net.mean, self.net.std]
        return _lib.cached(self, "lpips_norm", src, lambda: ([float(v) for v in src[0].reshape(-1).tolist()],
                                                             [float(v) for v in src[1].reshape(-1).tolist()]))

    def run(self, x, y, per_layer=False, taps=False):
        """The forward with its side outputs: dict(per_image (B,), mean (), per_layer (B, 5) or None, taps: five (2B, C, H, W) tensors
        of the normalised features (x's images first) or None)."""
        if not (torch.is_tensor(x) and torch.is_tensor(y)):
            raise TypeError("LPIPS takes two tensors")
        if x.ndim != 4 or x.shape[1] != 3 or x.shape != y.shape:
            raise ValueError(f"LPIPS takes two (B, 3, H, W) tensors of one shape (got {tuple(x.shape)} and {tuple(y.shape)})")
        B, _, H, W = x.shape
        if B < 1 or H < MIN_SIZE or W < MIN_SIZE:
            raise ValueError(f"LPIPS needs B >= 1 and H, W >= {MIN_SIZE} (got {tuple(x.shape)})")
        if torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
            raise NotImplementedError("LPIPS backward is not implemented: call under torch.no_grad() or detach the inputs")
        _lib.require_gpu(x, "LPIPS x")
        _lib.require_gpu(y, "LPIPS y")
        dev = x.device
        if y.device != dev:
            raise RuntimeError(f"LPIPS x is on {dev}, y on {y.device}")
        packed = self._packed(dev)
        mean, std = self._norm()
        x, y = x.detach().contiguous(), y.detach().contiguous()
        ws_bytes = _lib.load().e3dge_lpips_ws_bytes(B, H, W)
        if ws_bytes < 0:
            raise RuntimeError(f"e3dge_lpips_ws_bytes: {_lib.load().e3dge_last_error().decode(errors='replace')}")
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
        return res

    def forward(self, x, y, per_image=False):
        res = self.run(x, y)
        return res['per_image'] if per_image else res['mean']
