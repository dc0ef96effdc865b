"""ArcFace identity term (IR-SE50 backbone) on the HIP kernels of csrc/idnet.hip: the loss_id / ID_SIM columns of the evaluated image
and the `id_lambda` term of the reference's 2-D reconstruction loss.

The gradient with respect to y_hat (csrc/idnet_bwd.h; the network stays frozen, as the reference freezes it, and y and x never get
one: id_loss.py:36 detaches y's features and x's enter only the logs) is opt-in: `IDLoss(..., differentiable=True)` or
`module.differentiable = True`.  Then, with grad enabled and a y_hat that requires grad, the call goes through one autograd Function
whose forward is the state-saving form of the same launches (bit-identical values) and whose backward is once-differentiable.  With the
switch off (the default) inputs that require grad raise NotImplementedError, as before.

The module has the reference's call surface and state-dict keys (project/losses/id_loss.py, models/encoders/model_irse.py,
models/helper_modules/helpers.py:83-224), so a state dict saved from the reference's `IDLoss` loads with strict=True:

    facenet.input_layer.{0,1,2}.*, facenet.body.N.{shortcut_layer,res_layer}.*, facenet.output_layer.{0,3,4}.*

`facenet` is built from plain torch.nn layers in that arrangement; on the GPU only its parameters are used (the arithmetic is
csrc/idnet.hip), on the CPU it is the computation itself.  Nothing is ever downloaded: a fresh module holds its constructor's values
and `load_pretrained(file)` reads one LOCAL file."""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

UNITS = [(64, 64, 2)] + [(64, 64, 1)] * 2 + [(64, 128, 2)] + [(128, 128, 1)] * 3 + [(128, 256, 2)] + [(256, 256, 1)] * 13 + \
        [(256, 512, 2)] + [(512, 512, 1)] * 2                          # (in, depth, stride) of the 24 bottleneck_IR_SE units
TAP_UNITS = (0, 3, 7, 21, 23)
TAP_NAMES = ("net_input", "input_layer") + tuple(f"unit{u}" for u in TAP_UNITS) + ("head",)
EMBED = 512
CROP = (35, 223, 32, 220)                                            # id_loss.py:24


def mask_shapes(n):
    """Shapes of the 25 PReLU inputs for n images: the input layer's, then each unit's (its first 3x3 has stride 1)."""
    out, size = [(n, 64, 112, 112)], 112
    for _, depth, stride in UNITS:
        out.append((n, depth, size, size))
        size //= stride
    return out


def tap_shapes(n):
    """Shapes of the eight taps of E3dgeIdnetArgs for n images."""
    out, size = [(n, 3, 112, 112), (n, 64, 112, 112)], 112
    for u, (_, depth, stride) in enumerate(UNITS):
        size //= stride
        if u in TAP_UNITS:
            out.append((n, depth, size, size))
    return out + [(n, EMBED)]


class _SE(nn.Module):
    """helpers.py:133-158: the squeeze-and-excitation gate."""

    def __init__(self, channels, reduction):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(channels, channels // reduction, 1, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.fc2 = nn.Conv2d(channels // reduction, channels, 1, bias=False)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        return x * self.sigmoid(self.fc2(self.relu(self.fc1(self.avg_pool(x)))))


class _Unit(nn.Module):
    """helpers.py:204-223: res_layer = BN, conv3x3, PReLU, conv3x3 (stride), BN, SE; shortcut = strided pick or conv1x1 + BN."""

    def __init__(self, cin, depth, stride):
        super().__init__()
        if cin == depth:
            self.shortcut_layer = nn.MaxPool2d(1, stride)
        else:
            self.shortcut_layer = nn.Sequential(nn.Conv2d(cin, depth, 1, stride, bias=False), nn.BatchNorm2d(depth))
        self.res_layer = nn.Sequential(nn.BatchNorm2d(cin), nn.Conv2d(cin, depth, 3, 1, 1, bias=False), nn.PReLU(depth),
                                       nn.Conv2d(depth, depth, 3, stride, 1, bias=False), nn.BatchNorm2d(depth), _SE(depth, 16))

    def forward(self, x):
        return self.res_layer(x) + self.shortcut_layer(x)


class _Backbone(nn.Module):
    """model_irse.py:8-51 for (112, 50, 'ir_se'), eval form."""

    def __init__(self):
        super().__init__()
        self.input_layer = nn.Sequential(nn.Conv2d(3, 64, 3, 1, 1, bias=False), nn.BatchNorm2d(64), nn.PReLU(64))
        self.output_layer = nn.Sequential(nn.BatchNorm2d(512), nn.Dropout(0.6), nn.Flatten(), nn.Linear(512 * 7 * 7, EMBED),
                                          nn.BatchNorm1d(EMBED))
        self.body = nn.Sequential(*[_Unit(*u) for u in UNITS])

    def forward(self, x, taps=None):
        x = self.input_layer(x)
        if taps is not None:
            taps.append(x)
        for u, unit in enumerate(self.body):
            x = unit(x)
            if taps is not None and u in TAP_UNITS:
                taps.append(x)
        x = self.output_layer(x)
        if taps is not None:
            taps.append(x)
        return x / torch.norm(x, 2, 1, True)


class IDLoss(nn.Module):
    """`IDLoss(device)(y_hat, y, x)`: (loss, sim_improvement, id_logs) of id_loss.py:29-55 for three (B, 3, S, S) tensors in [-1, 1].
    GPU float32 tensors run the HIP kernels, CPU tensors the torch layers of `facenet` (under autograd when `differentiable`)."""

    def __init__(self, device=None, differentiable=False):
        super().__init__()
        self.differentiable = bool(differentiable)
        self.facenet = _Backbone()
        self.face_pool = nn.AdaptiveAvgPool2d((112, 112))
        self.id_loss_pool = nn.AdaptiveAvgPool2d((256, 256))          # builder.py:27
        for p in self.parameters():
            p.requires_grad = False
        self.eval()
        if device is not None:
            self.to(device)

    def train(self, mode=True):
        return super().train(False)                                   # the arithmetic is always the eval form (id_loss.py:21)

    def load_pretrained(self, ir_se50_file):
        """Weights from one local file: the state dict of the reference's Backbone (the ir_se50 checkpoint)."""
        sd = torch.load(ir_se50_file, map_location='cpu')
        missing, unexpected = self.facenet.load_state_dict(sd, strict=False)
        if missing or unexpected:
            raise RuntimeError(f"load_pretrained: missing {missing}, unexpected {unexpected}")
        return self

    # ---- launch plumbing --------------------------------------------------------------------------------------------------------
    def _sources(self):
        """The tensors of E3dgeIdnetPackSrc in its order (include/e3dge_hip.h): dict of lists."""
        f = self.facenet
        units = list(f.body)
        short = [u for u in units if isinstance(u.shortcut_layer, nn.Sequential)]
        convs = [f.input_layer[0]] + [c for u in units for c in (u.res_layer[1], u.res_layer[3])] + [u.shortcut_layer[0] for u in short]
        bns = [f.input_layer[1]] + [b for u in units for b in (u.res_layer[0], u.res_layer[4])] + [u.shortcut_layer[1] for u in short] + \
              [f.output_layer[0], f.output_layer[4]]
        return dict(conv_w=[c.weight for c in convs], bn_weight=[b.weight for b in bns], bn_bias=[b.bias for b in bns],
                    bn_mean=[b.running_mean for b in bns], bn_var=[b.running_var for b in bns],
                    prelu=[f.input_layer[2].weight] + [u.res_layer[2].weight for u in units],
                    se_fc1=[u.res_layer[5].fc1.weight for u in units], se_fc2=[u.res_layer[5].fc2.weight for u in units],
                    head_w=[f.output_layer[3].weight], head_b=[f.output_layer[3].bias])

    def _packed(self, device):
        groups = self._sources()
        src = [t for g in groups.values() for t in g]

        def build():
            with torch.no_grad():
                keep = {k: [t.detach().contiguous() for t in g] for k, g in groups.items()}
                s = _lib.IdnetPackSrc()
                for k, g in keep.items():
                    if k in ("head_w", "head_b"):
                        setattr(s, k, g[0].data_ptr())
                    else:
                        getattr(s, k)[:] = [t.data_ptr() for t in g]
                packed = torch.empty(_lib.query("e3dge_idnet_packed_floats"), device=device, dtype=torch.float32)
                _lib.launch("e3dge_idnet_pack_weights", packed, ctypes.addressof(s))
                return packed

        return _lib.weight_image(self, "idnet_packed", src, device, "IDLoss", build)

    def _packed_t(self, device):
        """The transposed weight image of the backward, on the same sources as the forward image."""
        groups = self._sources()
        src = [t for g in groups.values() for t in g]

        def build():
            with torch.no_grad():
                keep = [t.detach().contiguous() for t in groups["conv_w"]]
                s = _lib.IdnetPackSrc()
                s.conv_w[:] = [t.data_ptr() for t in keep]
                packed_t = torch.empty(_lib.query("e3dge_idnet_packed_t_floats"), device=device, dtype=torch.float32)
                _lib.launch("e3dge_idnet_pack_weights_t", packed_t, ctypes.addressof(s))
                return packed_t

        return _lib.weight_image(self, "idnet_packed_t", src, device, "IDLoss", build)

    def _check(self, sets):
        self._check_shapes(sets)
        for t in sets:
            if torch.is_grad_enabled() and t.requires_grad and not self.differentiable:
                raise NotImplementedError("IDLoss backward is not in this build: call under torch.no_grad() or detach the inputs")

    @staticmethod
    def _check_shapes(sets):
        first = sets[0]
        for t in sets:
            if not torch.is_tensor(t):
                raise TypeError("IDLoss takes tensors")
            if t.ndim != 4 or t.shape[1] != 3 or t.shape[0] < 1 or t.shape[2] != t.shape[3] or t.shape != first.shape:
                raise ValueError(f"IDLoss takes (B, 3, S, S) tensors of one shape, B >= 1 (got {[tuple(q.shape) for q in sets]})")
            if t.device != first.device or t.dtype != first.dtype:
                raise RuntimeError("IDLoss inputs must share one device and dtype")

    def _wants_grad(self, y_hat):
        return self.differentiable and torch.is_grad_enabled() and y_hat.requires_grad

    def _embed_sets(self, sets, taps=False, n_saved=0, grad_first=False):
        """(embeddings (len(sets) * B, 512), taps or None) of up to three image sets of one shape, set after set.  GPU, n_saved > 0: the
        state-saving forward; the saved state of the leading n_saved images is returned as a third value.  CPU, grad_first: the first
        set's embeddings carry the graph (the reference's own path); taps never do."""
        dev, B, S = sets[0].device, sets[0].shape[0], sets[0].shape[2]
        n = B * len(sets)
        if dev.type != "cuda":
            embs, per_set = [], []
            for i, z in enumerate(sets):                              # set by set, as id_loss.py:33-35 calls extract_feats
                with torch.enable_grad() if grad_first and i == 0 else torch.no_grad():
                    z = z.to(self.facenet.input_layer[0].weight.dtype)
                    if S != 256:
                        z = self.id_loss_pool(z)                      # builder.py:157-160
                    z = self.face_pool(z[:, :, CROP[0]:CROP[1], CROP[2]:CROP[3]])
                    tl = [z] if taps else None
                    embs.append(self.facenet(z, tl))
                    per_set.append([t.detach() for t in tl] if taps else None)
            return torch.cat(embs), ([torch.cat(t) for t in zip(*per_set)] if taps else None)
        for i, t in enumerate(sets):
            _lib.require_gpu(t, f"IDLoss input {i}")
        packed = self._packed(dev)
        keep = [t.detach().contiguous() for t in sets]
        ws_bytes = _lib.query("e3dge_idnet_ws_bytes", n)
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        emb = torch.empty((n, EMBED), device=dev, dtype=torch.float32)
        a = _lib.IdnetArgs(packed=packed, n_per_set=B, n_sets=len(sets), height=S, width=S, embeddings=emb, ws=ws, ws_bytes=ws_bytes)
        for i, t in enumerate(keep):
            a.images[i] = t.data_ptr()
        tl = None
        if taps:
            tl = [torch.empty(s, device=dev, dtype=torch.float32) for s in tap_shapes(n)]
            for i, t in enumerate(tl):
                a.taps[i] = t.data_ptr()
        a._note(dev)
        if n_saved:
            saved_bytes = _lib.query("e3dge_idnet_saved_bytes", n_saved)
            saved = torch.empty(saved_bytes, device=dev, dtype=torch.uint8)
            sa = _lib.IdnetSaveArgs(net=a, saved=saved, saved_bytes=saved_bytes, n_saved=n_saved)
            _lib.launch("e3dge_idnet_embed_save", sa)
            return emb, tl, saved
        _lib.launch("e3dge_idnet_embed", a)
        return emb, tl

    def _launch_backward(self, saved, shape, grad_emb, stages=False, masks=False):
        """(grad_y_hat, the eight stage gradients or None, the 25 masks or None) from the state `saved` a saving forward of inputs of
        `shape` left behind; grad_emb (B, 512) = dL / d f_hat."""
        B, _, S, _ = shape
        dev = saved.device
        ws_bytes = _lib.query("e3dge_idnet_bwd_ws_bytes", B, S, S)
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        grad = torch.empty(shape, device=dev, dtype=torch.float32)
        a = _lib.IdnetBwdArgs(packed=self._packed(dev), packed_t=self._packed_t(dev), saved=saved, saved_bytes=saved.numel(), n=B, height=S,
                              width=S, grad_embeddings=grad_emb, grad_images=grad, ws=ws, ws_bytes=ws_bytes)
        gs = ms = None
        if stages:
            gs = [torch.empty(s, device=dev, dtype=torch.float32) for s in tap_shapes(B)]
            for i, t in enumerate(gs):
                a.gstage[i] = t.data_ptr()
        if masks:
            ms = [torch.empty(s, device=dev, dtype=torch.uint8) for s in mask_shapes(B)]
            for i, t in enumerate(ms):
                a.masks[i] = t.data_ptr()
        _lib.launch("e3dge_idnet_backward", a)
        return grad, gs, ms

    def run_backward(self, y_hat, y, upstream, stages=False, masks=False):
        """Debug entry, no synchronisation: the saving forward of (y_hat, y), then the backward for upstream (B,) = dL / d(1 - dot_b)
        (1 / B for the loss).  Returns (grad_y_hat, the gradients at the eight tensors of TAP_NAMES or None -- the head's is the
        gradient at v, before the normalisation --, the 25 PReLU branch masks (uint8, shaped like the PReLU inputs of y_hat's images, 1 =
        positive branch) or None).  Needs no autograd and records none."""
        self._check_shapes([y_hat, y])
        _lib.require_gpu(upstream, "IDLoss upstream")
        B = y_hat.shape[0]
        if upstream.shape != (B,):
            raise ValueError(f"IDLoss upstream must be ({B},) (got {tuple(upstream.shape)})")
        with torch.no_grad():
            emb, _, saved = self._embed_sets([y_hat, y], n_saved=B)
            g_f = -upstream.detach().to(torch.float32)[:, None] * emb[B:2 * B]       # dL / d f_hat[b] = -u_b f_y[b]
            return self._launch_backward(saved, tuple(y_hat.shape), g_f, stages, masks)

    def embed(self, images):
        """(n, 512) unit-norm embeddings of (n, 3, S, S) images."""
        self._check([images])
        if torch.is_grad_enabled() and images.requires_grad:
            raise NotImplementedError("IDLoss backward is not in this build for embed(): the gradient exists for the loss of run() / forward()")
        return self._embed_sets([images])[0]

    def run(self, y_hat, y, x=None, taps=False):
        """The forward with its side outputs, no synchronisation: dict(embeddings (sets * B, 512) -- y_hat's, y's, then x's when x is
        a third set --, diff_target / diff_input / diff_views (B,), loss (), sim_improvement (), taps: list of TAP_NAMES tensors or
        None).  `x is y` or `x is None` (builder.py:165 passes the same object): two sets are embedded and x's features are y's."""
        two = x is None or x is y
        sets = [y_hat, y] if two else [y_hat, y, x]
        self._check(sets)
        B = y_hat.shape[0]
        want = self._wants_grad(y_hat)
        if want and y_hat.device.type == "cuda":
            side = {}
            loss = _IdLossFunction.apply(self, side, bool(taps), y_hat, y.detach(), None if two else x.detach())
            return dict(side, loss=loss)
        emb, tl = self._embed_sets(sets, taps, grad_first=want)
        return self._finish(emb, tl, B, two)

    def _finish(self, emb, tl, B, two):
        """The dot products, the loss and the result dict of run() from the embeddings."""
        fh, fy = emb[:B], emb[B:2 * B]
        fx = fy if two else emb[2 * B:]
        if emb.device.type != "cuda":
            dots = torch.empty((B, 3), dtype=emb.dtype)
            for b in range(B):                                       # the reference's own dot products, sample by sample
                dots[b, 0], dots[b, 1], dots[b, 2] = fh[b].dot(fy[b]), fh[b].dot(fx[b]), fy[b].dot(fx[b])
            loss, sim = 0, 0
            for b in range(B):
                loss = loss + (1 - dots[b, 0])
                sim += float(dots[b, 0].detach()) - float(dots[b, 2].detach())
            loss, sim = loss / B, torch.tensor(sim / B, dtype=dots.dtype)
        else:
            out = torch.empty(3 * B + 2, device=emb.device, dtype=torch.float32)
            a = _lib.IdLossArgs(y_hat=fh, y=fy, x=fx, batch=B, dots=out, loss=out.data_ptr() + 12 * B, sim_improvement=out.data_ptr() + 12 * B + 4)
            _lib.launch("e3dge_id_loss", a)
            dots, loss, sim = out[:3 * B].view(B, 3), out[3 * B], out[3 * B + 1]
        return dict(embeddings=emb.detach(), dots=dots.detach(), diff_target=dots[:, 0].detach(), diff_input=dots[:, 1].detach(),
                    diff_views=dots[:, 2].detach(), loss=loss, sim_improvement=sim, taps=tl)

    def forward(self, y_hat, y, x):
        res = self.run(y_hat, y, x)
        rows = res['dots'].tolist()                                   # the one device-to-host copy
        logs = [dict(diff_target=r[0], diff_input=r[1], diff_views=r[2]) for r in rows]
        B = len(rows)
        sim = sum(r[0] - r[2] for r in rows) / B                      # Python floats, as id_loss.py:51-55
        return res['loss'], sim, logs


class _IdLossFunction(torch.autograd.Function):
    """The loss of one saving forward (its side outputs go to `side`); the graph leads to y_hat only."""

    @staticmethod
    def forward(ctx, module, side, taps, y_hat, y, x=None):
        sets = [y_hat, y] if x is None else [y_hat, y, x]
        B = y_hat.shape[0]
        emb, tl, saved = module._embed_sets(sets, taps, n_saved=B)
        res = module._finish(emb, tl, B, x is None)
        side.update(res)
        ctx.module, ctx.saved, ctx.shape, ctx.f_y = module, saved, tuple(y_hat.shape), emb[B:2 * B]
        ctx.set_materialize_grads(False)
        return res['loss']

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        if g_loss is None or not ctx.needs_input_grad[3]:
            return (None,) * 6
        B = ctx.shape[0]
        u = (g_loss.to(torch.float32) / B).expand(B)
        g_f = -u[:, None] * ctx.f_y                                    # dL / d f_hat[b] = -u_b f_y[b]
        return None, None, None, ctx.module._launch_backward(ctx.saved, ctx.shape, g_f)[0], None, None
