"""The E0 image encoder (IR-SE50 body, feature pyramid, style heads) on the HIP kernels of csrc/encoder.h: image in, the (B, 9, 256)
renderer latent and the (B, 10, 512) decoder latent out -- what `G_pred_latents` takes as `styles` once the mean latents are added
(`image2latents`) -- and, with return_featmap, the p64 map that --local_append_E_feature_map hands to the local branch.

`HybridGradualStyleEncoder_V2` has the reference's constructor, sub-module names and state-dict keys
(project/models/encoders/fpn_encoders.py:266-433, models/helper_modules/helpers.py:83-224, :472-497), so the `encoder` entry of the
reference's checkpoint loads with strict=True.  The module is built from plain torch.nn layers in that arrangement.  Forward only, eval
form: a GPU float32 input runs the HIP kernels when the module is in eval mode (BatchNorm on its running statistics), no gradient is
wanted (grad mode off, or neither the input nor a parameter requires grad) and the options are the ones the kernels cover
(num_layers 50, mode 'ir_se', input_nc 3, fpn_pigan_geo_layer_dim and fpn_pigan_tex_layer_dim in {32, 64, 128}).  Everything else -- CPU
tensors, other dtypes and options, train(), gradients, E3DGE_ENCODER=torch -- runs the module's own torch layers in the reference's order;
on the CPU they reproduce the reference bit for bit (tests/test_encoder_host.py against tools/gen_golden_encoder.py's recording)."""
import ctypes
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .id_loss import _SE
from .losses import AvgPool2d
from .stylesdf_model import EqualLinear

BLOCKS = {50: (3, 4, 14, 3), 100: (3, 13, 30, 3), 152: (3, 8, 36, 3)}      # helpers.py:104-130
KEEP_UNITS = (2, 6, 20, 23)                                                # c128, c64, c32, c16 (fpn_encoders.py:384-391)
N_PIGAN, N_STYLEGAN, LATENT, STYLE = 9, 10, 512, 256
NATIVE_DIMS = (32, 64, 128)


def units(num_layers):
    """(in, depth, stride) of every bottleneck unit (helpers.py:99-130)."""
    out, cin = [], 64
    for depth, count in zip((64, 128, 256, 512), BLOCKS[num_layers]):
        out += [(cin, depth, 2)] + [(depth, depth, 1)] * (count - 1)
        cin = depth
    return out


class _Unit(nn.Module):
    """helpers.py:161-223: bottleneck_IR (se=False) and bottleneck_IR_SE."""

    def __init__(self, cin, depth, stride, se):
        super().__init__()
        if cin == depth:
            self.shortcut_layer = nn.MaxPool2d(1, stride)
        else:
            self.shortcut_layer = nn.Sequential(nn.Conv2d(cin, depth, (1, 1), stride, bias=False), nn.BatchNorm2d(depth))
        layers = [nn.BatchNorm2d(cin), nn.Conv2d(cin, depth, (3, 3), (1, 1), 1, bias=False), nn.PReLU(depth),
                  nn.Conv2d(depth, depth, (3, 3), stride, 1, bias=False), nn.BatchNorm2d(depth)]
        self.res_layer = nn.Sequential(*layers, *([_SE(depth, 16)] if se else []))

    def forward(self, x):
        shortcut = self.shortcut_layer(x)
        res = self.res_layer(x)
        return res + shortcut


class GradualStyleBlock(nn.Module):
    """helpers.py:472-497: log2(spatial) x [conv3x3 stride 2, LeakyReLU], EqualLinear."""

    def __init__(self, in_c, out_c, spatial):
        super().__init__()
        self.out_c = out_c
        self.spatial = spatial
        num_pools = int(math.log2(spatial))
        modules = [nn.Conv2d(in_c, out_c, kernel_size=3, stride=2, padding=1), nn.LeakyReLU()]
        for _ in range(num_pools - 1):
            modules += [nn.Conv2d(out_c, out_c, kernel_size=3, stride=2, padding=1), nn.LeakyReLU()]
        self.convs = nn.Sequential(*modules)
        self.linear = EqualLinear(out_c, out_c, lr_mul=1)

    def forward(self, x):
        x = self.convs(x)
        x = x.reshape(-1, self.out_c)
        return self.linear(x)

    def conv_layers(self):
        return [m for m in self.convs if isinstance(m, nn.Conv2d)]


class HybridGradualStyleEncoder_V2(nn.Module):
    """`HybridGradualStyleEncoder_V2(50, 'ir_se', n_styles, opts)(x, return_featmap=False)`: [thumb_out (B, 9, 256), stylegan_out
    (B, 10, 512) or None], or with return_featmap and the decoder head on dict(pred_latents=[...], feat_maps=p64, p32=p32), as the
    reference.  `opts` needs input_nc, full_pipeline, disable_decoder_fpn, single_decoder_layer, fpn_pigan_geo_layer_dim and
    fpn_pigan_tex_layer_dim (synthetic.encoder_opt has the scripts' values)."""

    def __init__(self, num_layers, mode, n_styles=None, opts=None):
        super().__init__()
        assert num_layers in [50, 100, 152], 'num_layers should be 50,100, or 152'
        assert mode in ['ir', 'ir_se'], 'mode should be ir or ir_se'
        self.opts = opts
        self.num_layers, self.mode = num_layers, mode
        self.input_layer = nn.Sequential(nn.Conv2d(opts.input_nc, 64, (3, 3), 1, 1, bias=False), nn.BatchNorm2d(64), nn.PReLU(64))
        self.full_pipeline = opts.full_pipeline
        self.body = nn.Sequential(*[_Unit(*u, se=mode == 'ir_se') for u in units(num_layers)])
        self.styles_pigan = nn.ModuleList()
        self.pigan_geo_layer = 6
        self.pigan_tex_layer = 9
        for i in range(N_PIGAN):
            dim = opts.fpn_pigan_geo_layer_dim if i < self.pigan_geo_layer else opts.fpn_pigan_tex_layer_dim
            self.styles_pigan.append(GradualStyleBlock(LATENT, STYLE, dim))
        self.enable_decoder = bool(self.full_pipeline and not opts.disable_decoder_fpn)
        if self.enable_decoder:
            self.styles_stylegan = nn.ModuleList()
            self.stylegan_style_count = N_STYLEGAN
            if not opts.single_decoder_layer:
                self.stylegan_coarse_ind = 0
                self.stylegan_middle_ind = 3
                for i in range(self.stylegan_style_count):           # only head 0 is ever read (fpn_encoders.py:417-419)
                    self.styles_stylegan.append(GradualStyleBlock(LATENT, LATENT, 128 if i < self.stylegan_middle_ind else 256))
            else:
                self.styles_stylegan.append(GradualStyleBlock(LATENT, LATENT, 128))
        self.latlayer64 = nn.Conv2d(64, LATENT, kernel_size=1, stride=1, padding=0)
        self.latlayer128 = nn.Conv2d(128, LATENT, kernel_size=1, stride=1, padding=0)
        self.latlayer256 = nn.Conv2d(256, LATENT, kernel_size=1, stride=1, padding=0)
        self.gt_pool = AvgPool2d((256, 256))                          # utils/transform.py:4; no parameters, no keys

    # ---- the torch composition, in the reference's order ----------------------------------------------------------------------------
    def _upsample_add(self, x, y):
        _, _, H, W = y.size()
        return F.interpolate(x, size=(H, W), mode='bilinear', align_corners=True) + y

    def forward_torch(self, x, return_featmap=False):
        x = self.input_layer(x)
        for i, unit in enumerate(self.body):
            x = unit(x)
            if i == 2:
                c128 = x
            elif i == 6:
                c64 = x
            elif i == 20:
                c32 = x
            elif i == 23:
                c16 = x
        p32 = self._upsample_add(c16, self.latlayer256(c32))
        p64 = self._upsample_add(p32, self.latlayer128(c64))
        latents = [self.styles_pigan[j](p32) for j in range(self.pigan_geo_layer)]
        for j in range(self.pigan_geo_layer, self.pigan_tex_layer):
            latents.append(self.styles_pigan[j](p64 if self.opts.fpn_pigan_tex_layer_dim == 64 else p32))
        thumb_out = torch.stack(latents, dim=1)
        if self.enable_decoder:
            p128 = self._upsample_add(p64, self.latlayer64(c128))
            stylegan_out = self.styles_stylegan[0](p128).unsqueeze(1).repeat(1, self.stylegan_style_count, 1)
            if return_featmap:
                return {'pred_latents': [thumb_out, stylegan_out], 'feat_maps': p64, 'p32': p32}
        else:
            stylegan_out = None
        return [thumb_out, stylegan_out]

    # ---- dispatch ---------------------------------------------------------------------------------------------------------------------
    def native_options(self):
        """Do the kernels cover this module's options?"""
        o = self.opts
        return (self.num_layers == 50 and self.mode == 'ir_se' and o.input_nc == 3 and o.fpn_pigan_geo_layer_dim in NATIVE_DIMS and
                o.fpn_pigan_tex_layer_dim in NATIVE_DIMS)

    def _runs_hip(self, x):
        if os.environ.get("E3DGE_ENCODER", "") == "torch" or self.training or not self.native_options():
            return False
        if not (torch.is_tensor(x) and x.device.type == "cuda" and x.dtype == torch.float32 and x.ndim == 4 and x.shape[1] == 3):
            return False
        S = x.shape[-1]
        if x.shape[0] < 1 or x.shape[0] > 256 or x.shape[-2] != S or S % 16 or S < 32 or S > 256:
            return False
        return not (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in _lib.params_of(self))))

    # ---- launch plumbing --------------------------------------------------------------------------------------------------------------
    def sources(self):
        """The source tensors in the order of e3dge_enc_pack_weights (include/e3dge_hip.h)."""
        bn = lambda m: [m.weight, m.bias, m.running_mean, m.running_var]
        out = [self.input_layer[0].weight] + bn(self.input_layer[1]) + [self.input_layer[2].weight]
        for u in self.body:
            r = u.res_layer
            out += bn(r[0]) + [r[1].weight, r[2].weight, r[3].weight] + bn(r[4]) + [r[5].fc1.weight, r[5].fc2.weight]
            if isinstance(u.shortcut_layer, nn.Sequential):
                out += [u.shortcut_layer[0].weight] + bn(u.shortcut_layer[1])
        for lat in (self.latlayer256, self.latlayer128, self.latlayer64):
            out += [lat.weight, lat.bias]
        for head in list(self.styles_pigan) + ([self.styles_stylegan[0]] if self.enable_decoder else []):
            for c in head.conv_layers():
                out += [c.weight, c.bias]
            out += [head.linear.weight, head.linear.bias]
        return out

    def _config(self, S):
        return (S, self.opts.fpn_pigan_geo_layer_dim, self.opts.fpn_pigan_tex_layer_dim, int(self.enable_decoder))

    def packed(self, device, S):
        """The packed weight image for inputs of size S on `device` (the heads' tails hold live taps only, so it depends on S)."""
        src = self.sources()
        cfg = self._config(S)

        def build():
            with torch.no_grad():
                keep = [t.detach().contiguous() for t in src]
                ptrs = (ctypes.c_void_p * len(keep))(*[t.data_ptr() for t in keep])
                image = torch.empty(_lib.query("e3dge_enc_packed_floats", *cfg), device=device, dtype=torch.float32)
                _lib.launch("e3dge_enc_pack_weights", image, ctypes.addressof(ptrs), len(keep), *cfg)
                return image

        return _lib.weight_image(self, f"enc_packed_{S}", src, device, "HybridGradualStyleEncoder_V2", build)

    def invalidate(self):
        """Drop the packed weight images (needed only after writes through `.data`)."""
        _lib.invalidate(self)

    def forward_hip(self, x):
        """(thumb_out (B, 9, 256), head 0 of the decoder latent (B, 512) or None, p32, p64) of a GPU float32 (B, 3, S, S) input; no
        synchronisation."""
        _lib.require_gpu(x, "encoder input")
        n, _, _, S = x.shape
        dev, cfg = x.device, self._config(S)
        image = self.packed(dev, S)
        x = x.detach().contiguous()
        ws_bytes = _lib.query("e3dge_enc_ws_bytes", n, *cfg)
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        new = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
        thumb, sg = new(n, N_PIGAN, STYLE), new(n, LATENT) if self.enable_decoder else None
        p32, p64 = new(n, LATENT, S // 8, S // 8), new(n, LATENT, S // 4, S // 4)
        a = _lib.EncArgs(packed=image, images=x, n=n, size=S, geo_dim=cfg[1], tex_dim=cfg[2], enable_decoder=cfg[3], thumb_out=thumb, stylegan_out=sg,
                         p32=p32, p64=p64, ws=ws, ws_bytes=ws_bytes)
        _lib.launch("e3dge_enc_forward", a)
        return thumb, sg, p32, p64

    def run(self, x, return_featmap=False, pool=True):
        """forward(); with pool=False the input is not pooled to 256 x 256 first and may be any square size that is a multiple of 16 and at
        least 32 (the heads need their maps to end at 1 x 1: at most 256)."""
        if pool and x.shape[-1] != 256:
            x = self.gt_pool(x)                                       # fpn_encoders.py:372-373
        if not self._runs_hip(x):
            return self.forward_torch(x, return_featmap)
        thumb_out, sg, p32, p64 = self.forward_hip(x)
        if self.enable_decoder:
            stylegan_out = sg.unsqueeze(1).repeat(1, self.stylegan_style_count, 1)
            if return_featmap:
                return {'pred_latents': [thumb_out, stylegan_out], 'feat_maps': p64, 'p32': p32}
        else:
            stylegan_out = None
        return [thumb_out, stylegan_out]

    def forward(self, x, return_featmap=False):
        return self.run(x, return_featmap)


def add_offset2latent(pred_offsets, mean_latent):
    """trainer.py:989-1015, the W+ branch: pred_offsets[i] <- mean_latent[i] repeated over the batch + pred_offsets[i], in place in the list."""
    for i in range(2):
        if pred_offsets[i] is not None:
            repeat_latent = mean_latent[i].repeat(pred_offsets[0].shape[0], 1, 1).to(pred_offsets[i].device)
            assert repeat_latent.shape == pred_offsets[i].shape
            pred_offsets[i] = repeat_latent + pred_offsets[i]
    return pred_offsets


_pool_256 = AvgPool2d((256, 256))


def image2latents(encoder, images, mean_latent, **kwargs):
    """trainer.py:950-969: pool_256, the encoder, the mean latents added.  Returns what `G_pred_latents` takes as `styles` (a list), or with
    return_featmap=True the encoder's dict with 'pred_latents' replaced by it.  mean_latent: [(1, 9, 256) or (9, 256), (1, 10, 512) or
    (10, 512)] (the second may be None when the decoder head is off)."""
    encoder_out = encoder(_pool_256(images), **kwargs)
    if isinstance(encoder_out, dict):
        encoder_out['pred_latents'] = add_offset2latent(encoder_out['pred_latents'], mean_latent)
        return encoder_out
    return add_offset2latent(encoder_out, mean_latent)
