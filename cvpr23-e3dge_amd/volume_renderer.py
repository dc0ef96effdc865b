"""VolumeFeatureRenderer on the fused gfx950 kernel -- host-side mirror of project/utils/volume_renderer.py.

What is kept identical to the reference (so that `train_setup.py:98-100` can swap the import):
  * constructor signatures `VolumeFeatureRenderer(opt, style_dim=256, out_im_res=64, mode='train')`,
    `SirenGenerator(opt, D, W, style_dim, ...)`, `FiLMSiren`, `LinearLayer` and their parameter names, hence
    the checkpoint keys `renderer.sigmoid_beta`, `renderer.network[.netGlobal].pts_linears.{i}.{weight,bias,
    gamma.weight,gamma.bias,beta.weight,beta.bias}`, `...views_linears.*`, `...rgb_linear.*`,
    `...sigma_linear.*`;
  * `forward(cam_poses, focal, near, far, styles, ...)` keyword list (:1865-1881) and the keys / shapes /
    layouts of the returned dict (:1270-1287, :1695-1701, :1957-1968);
  * `run_network(inputs, viewdirs, styles=...)` on arbitrary (B, ..., 3) point sets (:1052-1128).

What differs: nothing is evaluated in PyTorch.  One `e3dge_film_params` launch turns the W+ codes into the 9
(gamma, beta) pairs, one `e3dge_siren_render_fwd` launch does rays -> samples -> MLP -> composite; the eikonal terms,
`sample_mode` and the training direction (gradient to the styles, to the second pass's texture FiLM and to query
points) are further HIP launches.  Options the kernels do not cover (stratified perturbation, density
mode, mesh extraction) raise NotImplementedError instead of silently taking another path.

Renderer parameters: with `VolumeFeatureRenderer.train_renderer = True` (Generator sets it from
`not freeze_renderer`, as the reference's `train_renderer` does) the first-order backward of `render` and `run_network` also
returns the gradients of every SIREN parameter and of `sigmoid_beta`: the training backward stores g_l = gamma_l * dL/da_l, the
contraction e3dge_siren_wgrad turns it into the weight gradients, the FiLM biases and style linears follow from d(film) on the host
side.  Precision f16x3_g2 only; the eikonal term and the texture-FiLM pass with trainable weights are refused.  Off (the default),
trainable SIREN parameters under a backward raise NotImplementedError, as before.
"""
import os
import weakref
import warnings

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from .hg_filter import ResidualImageFilter


MFMA_MODES = {"f32": _lib.PREC_F32, "f16x3": _lib.PREC_F16X3, "f16x3_v1": _lib.PREC_F16X3_V1}
_SIDE_STREAM = os.environ.get("E3DGE_SIDE_STREAM", "1") != "0"     # surface-normal query beside the sdf chain (forward())
def _fuse_texfilm():                                                   # texture head writes the FiLM-ed layer-7 record itself
    return os.environ.get("E3DGE_FUSE_TEXFILM", "1") != "0"


class _LazyTex:
    """The texture FiLM of a second pass, not yet evaluated: the head and its (B,H,W,S,C) input.  When the pass starts from the
    first pass's layer-7 record, head + FiLM run as ONE launch that writes the FiLM-ed record (e3dge_tex_film_fwd: (alpha, beta)
    never reach HBM); otherwise `materialize()` gives the (alpha, beta) pair every other path consumes."""
    __slots__ = ('head', 'feats', '_ab')

    def __init__(self, head, feats):
        self.head, self.feats, self._ab = head, feats, None

    def materialize(self):
        if self._ab is None:
            self._ab = self.head.tex_modulations(self.feats)
        return self._ab


def _reuse_backbone():                                                 # second pass of an image reads the first pass's layer-7 output
    return os.environ.get("E3DGE_REUSE_BACKBONE", "1") != "0"


class _ReuseKey:
    """Key of a backbone record: strong references to the tensors + their version counters + plain scalars."""
    __slots__ = ('tensors', 'sig', 'scalars')

    def __init__(self, tensors, scalars):
        self.tensors = tuple(tensors)
        self.sig = tuple((t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride())) if torch.is_tensor(t) else t
                         for t in self.tensors)
        self.scalars = tuple(scalars)

    def extended(self, *more):
        k = _ReuseKey.__new__(_ReuseKey)
        k.tensors, k.sig, k.scalars = self.tensors, self.sig, self.scalars + tuple(more)
        return k

    def matches(self, rec_key):
        """`self` describes the current call, `rec_key` the recorded one (whose tensors are alive by construction)."""
        if rec_key is None or self.scalars != rec_key.scalars or self.sig != rec_key.sig:
            return False
        # the packed weight image is compared by identity (it is rebuilt, not edited); the recorded tensors must not have
        # been edited in place since (their version is part of sig: re-read it from the LIVE recorded tensors)
        if self.tensors[-1] is not rec_key.tensors[-1]:
            return False
        return all((t._version == s[1]) for t, s in zip(rec_key.tensors, rec_key.sig) if torch.is_tensor(t))


# renderer -> {(kind, stream, bytes, device): [buffer, pinned, last use]}: the raw storage of the layer-7 records ('bb': written by a first
# pass, 'film': the FiLM-ed copy e3dge_tex_film_fwd writes).  One buffer per STREAM and size -- two streams rendering with one renderer do
# not share storage -- and a buffer that a HIP-graph capture has seen is PINNED: the graph holds its raw pointer, so it is never replaced
# or dropped by a render or by invalidate() (round-4 advisor finding); `release_record_buffers(renderer)` drops the pinned ones once the
# graphs that captured them are gone.  Unpinned buffers: the two most recently used sizes per (kind, stream) stay (alternating batch sizes
# do not re-allocate and re-zero ~100 MB per switch), older ones are released.  A zero-filled buffer ('film': zeroed ONCE, the launches
# only ever write the rows they own) must exist BEFORE a capture: the fill would be captured and re-run on every replay, and the storage
# would live in the graph's private pool while eager renders use it too -- a first-seen key mid-capture raises (graphs.GraphedCall warms
# up on its capture stream, which creates it).
_RECORD_BUFS = weakref.WeakKeyDictionary()
_RECORD_KEEP = 2
_record_clock = [0]


def _record_buffer(renderer, kind, n_bytes, dev, stream, capturing, zero):
    pool = _RECORD_BUFS.setdefault(renderer, {})
    key = (kind, stream, int(n_bytes), str(dev))
    ent = pool.get(key)
    _record_clock[0] += 1
    if ent is None:
        if capturing and zero:
            raise RuntimeError(f"renderer record buffer '{kind}' ({int(n_bytes)} bytes) would be allocated and zero-filled inside a HIP-graph "
                               "capture: run the same call once eagerly on the capture stream first (graphs.GraphedCall does)")
        loose = sorted((k for k, e in pool.items() if k[0] == kind and k[1] == stream and not e[1]), key=lambda k: pool[k][2])
        for k in loose[:max(0, len(loose) - (_RECORD_KEEP - 1))]:
            pool.pop(k)
        buf = (torch.zeros if zero else torch.empty)(int(n_bytes), device=dev, dtype=torch.uint8)
        ent = pool[key] = [buf, False, 0]
    ent[2] = _record_clock[0]
    if capturing:
        ent[1] = True
    return ent[0]


def release_record_buffers(renderer, pinned_only=False):
    """Drop the renderer's record buffers, INCLUDING the ones a HIP-graph capture pinned: call it after the graphs that captured this
    renderer's second pass have been destroyed (their replays write through the raw pointers)."""
    pool = _RECORD_BUFS.get(renderer)
    if pool:
        for k in [k for k, e in pool.items() if e[1] or not pinned_only]:
            pool.pop(k)


_BACKBONE = weakref.WeakKeyDictionary()                                # renderer -> {key, buf (record), out (first pass's tensors)}
_SIDE_STREAMS = {}                                                     # per device (module level: modules stay deep-copyable)


def _side_stream(dev, idx=0):
    key = (str(dev), idx)
    st = _SIDE_STREAMS.get(key)
    if st is None:
        st = _SIDE_STREAMS[key] = torch.cuda.Stream(device=dev)
    return st


# Round 5: when the generator runs the decoder behind the renderer under grad (train_ae.py's stage-1 step, --full_pipeline), the ray
# samples' sdf chain (forward) and their tangent pass (backward) do not feed the decoder: they go to a second side stream and run BESIDE
# the decoder's forward / backward, and the launch stream waits for them only when the generator hands its outputs over / when the
# render node's backward needs the tangent.  E3DGE_OVERLAP_DECODER=0 keeps everything on the launch stream.
def _overlap_decoder():
    return os.environ.get("E3DGE_OVERLAP_DECODER", "1") != "0"


# backward-type launches additionally know the 8-wave x 16-point layout (E3DGE_PREC_F16X3_G2, csrc/siren16_bwd.h)
BWD_MODES = dict(MFMA_MODES, f16x3_g2=_lib.PREC_F16X3_G2)


def default_mfma_mode():
    """How the 256-wide contractions run (see include/e3dge_hip.h): 'f16x3' (split-f16 on the f16 matrix pipe, fp32
    accumulate -- same parity bounds, ~4x faster) unless E3DGE_MFMA_MODE=f32 asks for the fp32 MFMA kernel."""
    mode = os.environ.get("E3DGE_MFMA_MODE", "f16x3")
    if mode not in MFMA_MODES:
        raise RuntimeError(f"E3DGE_MFMA_MODE must be one of {sorted(MFMA_MODES)}, got {mode!r}")
    return mode


def default_bwd_mode():
    """The same choice for the backward-type kernels (E3DGE_BWD_MODE).  Default: 'f16x3_g2' beside the f16x3 forward -- the 8-wave
    kernels of csrc/siren16_bwd.h (block-scaled split-f16 like 'f16x3', saved state slab-major, second-order inputs as the products
    ta r; round 6) --, 'f32' beside the f32 forward.  'f16x3' = the first-generation 4-wave kernels."""
    fwd = default_mfma_mode()
    mode = os.environ.get("E3DGE_BWD_MODE", "f16x3_g2" if fwd == "f16x3" else fwd)
    if mode not in BWD_MODES:
        raise RuntimeError(f"E3DGE_BWD_MODE must be one of {sorted(BWD_MODES)}, got {mode!r}")
    return mode


def saved_state_buffer(B, N, L, device, W=256):
    """Uninitialised (B, N, L, W) fp32 scratch for the saved state of a training launch (pre-sine arguments: L = 9; r_l / ta_l r_l:
    L = 8).  The rows of an image are padded to a multiple of 16 -- the slab-major layout of the f16x3_g2 kernels (siren_common.h)
    addresses whole 16-row slabs -- and the tensor returned is the (B, N, ..) view of it: only its data pointer is ever used."""
    n16 = (int(N) + 15) // 16 * 16
    return torch.empty((int(B), n16, int(L), int(W)), device=device, dtype=torch.float32)[:, :int(N)]


def saved_state_point_major(t, slab_major):
    """Debug / test view of a saved-state tensor made by saved_state_buffer: (B, N, L, W) indexed [image, point, layer, feature] whatever
    the storage layout -- slab-major (siren_common.h: [slab of 16 rows][layer][tile of 16 features][q][row & 15][4]) is re-ordered."""
    if not slab_major:
        return t
    B, N, L, W = t.shape
    n16 = (N + 15) // 16 * 16
    v = torch.as_strided(t, (B, n16 // 16, L, W // 16, 4, 16, 4), (n16 * L * W, 16 * L * W, 16 * W, 256, 64, 4, 1))   # [b, slab, layer, tile, q, n, j]
    return v.permute(0, 1, 5, 2, 3, 4, 6).reshape(B, n16, L, W)[:, :N]


def _opt_get(opt, name, default=None):
    if opt is None:
        return default
    if isinstance(opt, dict):
        return opt.get(name, default)
    return getattr(opt, name, default)


class UniformBoxWarp(nn.Module):
    """Reference :23-30."""

    def __init__(self, sidelength):
        super().__init__()
        self.scale_factor = 2 / sidelength

    def forward(self, coordinates):
        return coordinates * self.scale_factor


class LinearLayer(nn.Module):
    """Parameter holder + initialiser of the reference's LinearLayer (:42-80).
    out = std_init * (W x + b) + bias_init.  On the render path these are evaluated inside the HIP kernels
    (gamma/beta in e3dge_film_params, the sdf/rgb heads in the fused renderer); `forward` exists for callers
    that apply one directly and runs as a GPU torch op."""

    def __init__(self, in_dim, out_dim, bias=True, bias_init=0, std_init=1, freq_init=False, is_first=False):
        super().__init__()
        if is_first:
            w = torch.empty(out_dim, in_dim).uniform_(-1 / in_dim, 1 / in_dim)
        elif freq_init:
            lim = np.sqrt(6 / in_dim) / 25
            w = torch.empty(out_dim, in_dim).uniform_(-lim, lim)
        else:
            w = 0.25 * nn.init.kaiming_normal_(torch.randn(out_dim, in_dim), a=0.2, mode='fan_in',
                                               nonlinearity='leaky_relu')
        self.weight = nn.Parameter(w)
        lim = np.sqrt(1 / in_dim)
        self.bias = nn.Parameter(torch.empty(out_dim).uniform_(-lim, lim))
        self.bias_init = bias_init
        self.std_init = std_init

    def forward(self, input):
        return self.std_init * torch.nn.functional.linear(input, self.weight, bias=self.bias) + self.bias_init


class FiLMSiren(nn.Module):
    """sin(gamma(style) * (W x + b) + beta(style)) -- parameter holder for reference :84-132."""

    def __init__(self, in_channel, out_channel, style_dim, is_first=False):
        super().__init__()
        self.in_channel = in_channel
        self.out_channel = out_channel
        if is_first:
            w = torch.empty(out_channel, in_channel).uniform_(-1 / 3, 1 / 3)
        else:
            lim = np.sqrt(6 / in_channel) / 25
            w = torch.empty(out_channel, in_channel).uniform_(-lim, lim)
        self.weight = nn.Parameter(w)
        lim = np.sqrt(1 / in_channel)
        self.bias = nn.Parameter(torch.empty(out_channel).uniform_(-lim, lim))
        self.gamma = LinearLayer(style_dim, out_channel, bias_init=30, std_init=15)
        self.beta = LinearLayer(style_dim, out_channel, bias_init=0, std_init=0.25)


class SirenGenerator(nn.Module):
    """The StyleSDF MLP (reference :136-264) as a parameter container plus the two device-side caches the
    kernels consume: the MFMA fragment-major weight image and the stacked gamma/beta matrices."""

    def __init__(self, opt=None, D=8, W=256, style_dim=256, input_ch=3, input_ch_views=3, output_ch=4,
                 output_features=True, scene_scale=0.12, **kwargs):
        super().__init__()
        if D != 8 or W != 256 or style_dim != 256 or input_ch != 3 or input_ch_views != 3:
            raise NotImplementedError(
                f"the gfx950 kernels are specialised for D=8, W=256, style_dim=256, 3+3 inputs "
                f"(got D={D}, W={W}, style_dim={style_dim}, input_ch={input_ch}, views={input_ch_views})")
        self.opt = opt
        self.D, self.W = D, W
        self.input_ch, self.input_ch_views = input_ch, input_ch_views
        self.style_dim = style_dim
        self.output_features = output_features
        self.pts_linears = nn.ModuleList(
            [FiLMSiren(3, W, style_dim=style_dim, is_first=True)] +
            [FiLMSiren(W, W, style_dim=style_dim) for _ in range(D - 1)])
        self.views_linears = FiLMSiren(input_ch_views + W, W, style_dim=style_dim)
        self.rgb_linear = LinearLayer(W, 3, freq_init=True)
        self.sigma_linear = LinearLayer(W, 1, freq_init=True)
        self.mfma_mode = default_mfma_mode()
        self.bwd_mode = default_bwd_mode()
        self.train_params = False          # set through VolumeFeatureRenderer.train_renderer

    def trainable_params(self, what, eikonal=False, tex=False):
        """() when the renderer is not trained (train_params off) or no parameter requires grad; else siren_trainable_params(self) --
        after refusing what the parameter gradients do not cover."""
        if not self.train_params or not any(p.requires_grad for p in _lib.params_of(self)):
            return ()
        if eikonal:
            raise NotImplementedError(f"{what}: trainable renderer parameters together with the eikonal term (second-order parameter "
                                      "gradients) are not covered")
        if tex:
            raise NotImplementedError(f"{what}: trainable renderer parameters on the texture-FiLM pass are not covered")
        _require_param_mode(self, what)
        return tuple(siren_trainable_params(self))

    # -- device caches -------------------------------------------------------------------------------
    def _film_layers(self):
        return list(self.pts_linears) + [self.views_linears]

    def invalidate(self):
        """Drop the packed weight image.  The cache (_lib.cached) follows every parameter's identity, data pointer and version, which
        catches optimizer steps, `load_state_dict`, `.to()`, a replaced Parameter and in-place ops on the parameter itself -- but NOT
        writes through `.data` (`p.data.mul_()`, the reference's EMA `accumulate()` in utils/training_utils.py:45 and ranger.py:178 do
        that; they leave the version untouched).  Call this after such an update, or set E3DGE_STRICT_WEIGHT_CACHE=1 to
        have every call compare a device-side fingerprint of the weights (extra reductions + a host sync per call)."""
        _lib.invalidate(self)

    def _apply(self, fn, *a, **k):
        _lib.forget_params(self)
        return super()._apply(fn, *a, **k)

    def device_image(self):
        """(packed, wg, bg, wb, bb): rebuilt only when a parameter changed (or moved); see invalidate()."""
        return _lib.cached(self, 'image', _lib.params_of(self), self._build_image)[0]

    def _build_image(self):
        """[device_image(), max |w| of the 256-wide layers, has check_mode warned about it]."""
        w0 = self.pts_linears[0].weight
        _lib.require_gpu(w0, "SirenGenerator parameters")
        lib = _lib.load()
        with torch.no_grad():
            dev = w0.device
            f32 = dict(device=dev, dtype=torch.float32)
            w_first = self.pts_linears[0].weight.detach().contiguous()
            b_first = self.pts_linears[0].bias.detach().contiguous()
            w_hidden = torch.stack([l.weight.detach() for l in self.pts_linears[1:]]).contiguous()
            b_hidden = torch.stack([l.bias.detach() for l in self.pts_linears[1:]]).contiguous()
            w_view = self.views_linears.weight.detach().contiguous()
            b_view = self.views_linears.bias.detach().contiguous()
            w_rgb = self.rgb_linear.weight.detach().contiguous()
            b_rgb = self.rgb_linear.bias.detach().contiguous()
            w_sig = self.sigma_linear.weight.detach().contiguous()
            b_sig = self.sigma_linear.bias.detach().contiguous()
            if self.rgb_linear.std_init != 1 or self.rgb_linear.bias_init != 0 or \
                    self.sigma_linear.std_init != 1 or self.sigma_linear.bias_init != 0:
                raise NotImplementedError("head LinearLayers with std_init != 1 / bias_init != 0")
            packed = torch.empty(lib.e3dge_siren_packed_floats(), **f32)
            _lib.launch("e3dge_siren_pack_weights", packed, w_first, b_first, w_hidden, b_hidden, w_view, b_view, w_rgb, b_rgb,
                        w_sig, b_sig)
            # The f16x3 images carry the weights times 128 as f16 (max 65504): a checkpoint with |w| >= 256 in the
            # 256-wide layers (trained ones are ~0.01) cannot use them; check_mode() then selects the fp32 MFMA kernels.
            wmax = float(torch.maximum(w_hidden.abs().max(), w_view.abs().max()).item())
            layers = self._film_layers()
            wg = torch.stack([l.gamma.weight.detach() for l in layers]).contiguous()
            bg = torch.stack([l.gamma.bias.detach() for l in layers]).contiguous()
            wb = torch.stack([l.beta.weight.detach() for l in layers]).contiguous()
            bb = torch.stack([l.beta.bias.detach() for l in layers]).contiguous()
        return [(packed, wg, bg, wb, bb), wmax, False]

    def check_mode(self, mode):
        """Precision selector for a launch.  Weights outside the f16x3 image's range (|w| >= 256, see device_image) fall
        back to the fp32 MFMA kernels for this module, with one warning."""
        built = _lib.latest(self, 'image')
        if mode != "f32" and built is not None and built[1] >= 256.0:
            if not built[2]:
                warnings.warn(f"SIREN weights up to {built[1]:g} do not fit the f16x3 weight image (|w| < 256); "
                              "this module uses the fp32 MFMA kernels instead")
                built[2] = True
            mode = "f32"
        return BWD_MODES[mode]

    def saved_state_is_slab_major(self):
        """Layout in which the training launches of this module save their state (see saved_state_point_major)."""
        return self.check_mode(self.bwd_mode) == _lib.PREC_F16X3_G2

    def save_precision(self, mfma_mode=None):
        """Precision code of a forward launch that saves its pre-sine arguments: the forward's own, or E3DGE_PREC_F16X3_G2 (= the
        f16x3 forward writing the slab-major layout) when the backward-type kernels run in mode f16x3_g2."""
        fwd = self.check_mode(mfma_mode or self.mfma_mode)
        if self.check_mode(self.bwd_mode) == _lib.PREC_F16X3_G2:
            if fwd != _lib.PREC_F16X3:
                raise RuntimeError("backward mode 'f16x3_g2' reads the saved arguments slab-major, which only the 'f16x3' forward writes "
                                   f"(forward mode {mfma_mode or self.mfma_mode!r})")
            return _lib.PREC_F16X3_G2
        return fwd

    def require_frozen(self, what):
        """The HIP backward returns gradients for the styles (and, where stated, points / texture FiLM) only; the
        reference can also train the renderer (Generator.train_renderer = not freeze_renderer).  Make the frozen
        generator an explicit precondition instead of a silent no-op."""
        if not any(p.requires_grad for p in _lib.params_of(self)):       # (the cheap check first: named_parameters() walks the tree, 120 us)
            return
        hot = [n for n, p in self.named_parameters() if p.requires_grad]
        if hot:
            raise NotImplementedError(
                f"{what}: SIREN parameters require grad ({hot[0]}, ... {len(hot)} in all) but the HIP backward only "
                "differentiates w.r.t. the styles (frozen generator, trainer.py:1568); call requires_grad_(False) on the "
                "renderer or run under torch.no_grad()")

    def film_params(self, styles):
        """styles (B,9,256) [W+] or (B,256) [W, shared by all layers, reference :189-191] -> (B,9,2,256)."""
        _lib.require_gpu(styles, "styles")
        if styles.ndim == 2:
            styles = styles.unsqueeze(1).expand(-1, 9, -1)
        if styles.ndim != 3 or styles.shape[1] != 9 or styles.shape[2] != self.style_dim:
            raise RuntimeError(f"styles must be (B, 9, {self.style_dim}) or (B, {self.style_dim}); got {tuple(styles.shape)}")
        styles = _lib.dense(styles)                 # (stride-0 `latent.unsqueeze(1).expand(...)` styles; e3dge_film_params requires 16-byte pointers)
        _, wg, bg, wb, bb = self.device_image()
        B = styles.shape[0]
        film = torch.empty((B, 9, 2, self.W), device=styles.device, dtype=torch.float32)
        _lib.launch("e3dge_film_params", film, styles, wg, bg, wb, bb, B)
        return film

    def query_points(self, pts, viewdirs, styles, box_scale, want_raw=True, mfma_mode=None, save_args=None,
                     want_eikonal=False):
        """pts (B, N, 3) world-space, viewdirs (B, N, 3) or None -> (sdf (B,N), raw (B,N,260) or None)
        [, eikonal term d sdf / d pts (B,N,3) with want_eikonal].
        Under grad mode the call is differentiable w.r.t. `styles` and w.r.t. `pts` (whichever requires grad): HIP
        backward e3dge_siren_bwd, the eikonal term included -- d(eikonal)/d(pts) is the Hessian-vector product the
        reference gets by keeping the surface point in the graph (:921-930).  View directions get no gradient."""
        _lib.require_gpu(pts, "pts")
        live = pts.shape[0] and pts.shape[1]
        params = self.trainable_params("query_points", want_eikonal) if torch.is_grad_enabled() and live else ()
        if torch.is_grad_enabled() and (styles.requires_grad or pts.requires_grad or params) and live:
            if not params:
                self.require_frozen("query_points")
            sdf, raw, eik = _PointsQuery.apply(styles, self, pts, None if viewdirs is None else viewdirs.detach(),
                                               box_scale, mfma_mode, bool(want_eikonal), *params)
            raw = raw if want_raw else None
            return (sdf, raw, eik) if want_eikonal else (sdf, raw)
        film = self.film_params(styles)
        if not want_eikonal:
            return self._points_launch(film, pts, viewdirs, box_scale, want_raw, mfma_mode, save_args)
        B, N = pts.shape[0], pts.shape[1]
        args = save_args if save_args is not None else saved_state_buffer(B, N, 9, pts.device, self.W)
        sdf, raw = self._points_launch(film, pts, viewdirs, box_scale, want_raw, mfma_mode, args)
        eik = sdf_gradient(self, film, args, box_scale)[0] if live else torch.empty((B, N, 3), device=pts.device)
        return sdf, raw, eik

    def _points_launch(self, film, pts, viewdirs, box_scale, want_raw, mfma_mode, save_args):
        packed = self.device_image()[0]
        pts = pts.contiguous()
        vd = None if viewdirs is None else viewdirs.contiguous()
        B, N, _ = pts.shape
        sdf = torch.empty((B, N), device=pts.device, dtype=torch.float32)
        raw = torch.empty((B, N, 260), device=pts.device, dtype=torch.float32) if want_raw else None
        if B == 0 or N == 0:
            return sdf, raw
        prec = self.save_precision(mfma_mode) if save_args is not None else self.check_mode(mfma_mode or self.mfma_mode)
        _lib.launch("e3dge_siren_points_fwd", packed, film, pts, vd, float(box_scale), B, N, sdf, raw, save_args, prec)
        return sdf, raw

    def forward(self, net_inputs, styles, residuals=None):
        """(B, ..., 6) = [box-warped xyz, viewdir] -> (B, ..., 260) = [rgb3, sdf1, feat256] (reference :240-264).
        The points are already warped here, so the kernel's box scale is 1."""
        lead = net_inputs.shape[:-1]
        B = net_inputs.shape[0]
        flat = net_inputs.reshape(B, -1, 6)
        _, raw = self.query_points(flat[..., :3], flat[..., 3:], styles, 1.0, want_raw=True)
        return raw.reshape(*lead, 260)


def sdf_gradient(siren, film, args, box_scale):
    """Eikonal term e = d sdf / d x (B,N,3) from the saved arguments (e3dge_siren_sdf_grad, reference :796-802), plus
    the per-layer r_l = d sdf / d h_l (B,N,8,256) a loss on e needs for its backward."""
    packed = siren.device_image()[0]
    B, N = args.shape[0], args.shape[1]
    rsave = saved_state_buffer(B, N, 8, args.device, siren.W)
    eik = torch.empty((B, N, 3), device=args.device, dtype=torch.float32)
    _lib.launch("e3dge_siren_sdf_grad", packed, film, args, None, float(box_scale), B, N, rsave, eik, siren.check_mode(siren.bwd_mode))
    return eik, rsave


def tangent_arguments(siren, film, args, v, box_scale, images=None, rsave=None, out=None):
    """Tangent arguments (B,N,8,256) along v = dL/de (B,N,3) (e3dge_siren_tangent).  `images`: siren.device_image() as the forward
    of the same autograd node saw it (a backward differentiates the weights its saved arguments were computed with, and skipping the
    cache-key check keeps ~20 us of host time out of the gap in front of the launch).
    Returns (tang, rs) as e3dge_siren_bwd / e3dge_siren_render_bwd take them: in the 8-wave backward mode (`f16x3_g2`) with `rsave`
    given, `tang` holds the PRODUCTS ta_l r_l (e3dge_siren_tangent_tr: the only form in which the two ever enter the second-order
    backward) and rs is None; otherwise (ta_l, rsave).  `out`: a saved_state_buffer(B, N, 8, ...) to write into (a caller that launches on a side
    stream allocates it on ITS stream: GB-sized blocks that change streams are what the caching allocator handles worst)."""
    packed = (images if images is not None else siren.device_image())[0]
    B, N = args.shape[0], args.shape[1]
    v = v.reshape(B, N, 3).contiguous().float()
    tang = out if out is not None else saved_state_buffer(B, N, 8, args.device, siren.W)
    prec = siren.check_mode(siren.bwd_mode)
    if prec == _lib.PREC_F16X3_G2 and rsave is not None:
        _lib.launch("e3dge_siren_tangent_tr", packed, film, args, v, rsave, float(box_scale), B, N, tang, prec)
        rsave = None
    else:
        _lib.launch("e3dge_siren_tangent", packed, film, args, v, float(box_scale), B, N, tang, prec)
    return tang, rsave


def siren_backward(siren, film, args, d_feat, d_rgb, d_sdf, tang=None, rsave=None, want_d_pts=False, box_scale=1.0,
                   tex_alpha=None, images=None, lin=None):
    """dL/d(styles) (B,9,256) and dL/d(film) (B,9,2,256) from the per-point output gradients (e3dge_siren_bwd).
    args (B,N,9,256) are the forward launch's saved pre-sine arguments; any of d_feat (B,N,256), d_rgb (B,N,3),
    d_sdf (B,N) may be None.  tang + rsave add the gradient of a loss on the eikonal term.  Returns
    (dstyles, dfilm, d_pts or None, (d_alpha, d_beta) or None)."""
    packed, wg, _, wb, _ = images if images is not None else siren.device_image()
    B, N = args.shape[0], args.shape[1]
    dev = args.device
    lib = _lib.load()
    d_feat = None if d_feat is None else _lib.dense(d_feat.float())          # (16-byte loads: siren_bwd.hip:1142 guards it)
    d_rgb, d_sdf = [None if t is None else t.contiguous().float() for t in (d_rgb, d_sdf)]
    n_part = lib.e3dge_siren_bwd_partial_floats(B, N)
    partials = torch.empty(max(n_part, 1), device=dev, dtype=torch.float32)
    dfilm = torch.empty((B, 9, 2, siren.W), device=dev, dtype=torch.float32)
    dstyles = torch.empty((B, 9, siren.W), device=dev, dtype=torch.float32)
    d_pts = torch.empty((B, N, 3), device=dev, dtype=torch.float32) if want_d_pts else None
    d_ta = d_tb = None
    if tex_alpha is not None:
        d_ta = torch.empty((B, N, siren.W), device=dev, dtype=torch.float32)
        d_tb = torch.empty((B, N, siren.W), device=dev, dtype=torch.float32)
    a = _lib.SirenBwdArgs(
        packed=packed, film=film, args=args, d_feat=d_feat, d_rgb=d_rgb, d_sdf=d_sdf, tang=tang, rsave=rsave, wg=wg, wb=wb,
        tex_alpha=tex_alpha, batch=B, precision=siren.check_mode(siren.bwd_mode), n_pts=N, box_scale=float(box_scale),
        partials=partials, dfilm=dfilm, dstyles=dstyles, d_pts=d_pts, d_tex_alpha=d_ta, d_tex_beta=d_tb)
    if lin is not None:                            # (d_lin, lin_amax) of lin_buffers(): the renderer's parameter gradients follow
        a.d_lin, a.lin_amax = lin
    _lib.launch("e3dge_siren_bwd", a)
    return dstyles, dfilm, d_pts, (None if d_ta is None else (d_ta, d_tb))


# ---- renderer parameter gradients (ABI 16) ----------------------------------------------------------------------
def siren_trainable_params(siren):
    """The SIREN's parameters in a fixed order (pts_linears.0..7, views_linears: weight, bias, gamma.weight, gamma.bias, beta.weight,
    beta.bias; then rgb_linear, sigma_linear: weight, bias) -- the extra autograd inputs of _RenderQuery / _PointsQuery."""
    out = []
    for l in siren._film_layers():
        out += [l.weight, l.bias, l.gamma.weight, l.gamma.bias, l.beta.weight, l.beta.bias]
    return out + [siren.rgb_linear.weight, siren.rgb_linear.bias, siren.sigma_linear.weight, siren.sigma_linear.bias]


def _require_param_mode(siren, what):
    siren.device_image()                                   # (check_mode reads the weight range the image build records)
    if siren.check_mode(siren.bwd_mode) != _lib.PREC_F16X3_G2:
        raise NotImplementedError(f"{what}: gradients of the renderer's parameters exist for backward mode 'f16x3_g2' only "
                                  f"(mode {siren.bwd_mode!r}, or the fp32 fallback for weights with |w| >= 256)")


def lin_buffers(B, N, device):
    """(d_lin, lin_amax): the backward's parameter-gradient outputs -- g_l of the nine layers, laid out like the saved arguments, and
    nine zeroed amax buffers."""
    return (saved_state_buffer(B, N, 9, device), torch.zeros(9 * _lib.AMAX_FLOATS, device=device, dtype=torch.float32))


def siren_param_grads(siren, film, styles, dfilm, args, d_lin, lin_amax, d_sdf, d_rgb, pts, viewdirs, samples, box_scale):
    """Gradients of siren_trainable_params(siren), in that order, from one training backward: e3dge_siren_wgrad for the weights and
    heads, d(film) and the styles for the FiLM biases and the gamma / beta style linears (LinearLayer: out = std_init (W s + b) + bias_init)."""
    B, N = args.shape[0], args.shape[1]
    dev = args.device
    W = siren.W
    lib = _lib.load()
    f32 = dict(device=dev, dtype=torch.float32)
    d_w = torch.empty((8, W, W), **f32)
    d_wv, d_w0 = torch.empty((W, 3), **f32), torch.empty((W, 3), **f32)
    d_ws, d_bs = torch.empty((1, W), **f32), torch.empty(1, **f32)
    d_wr, d_br = torch.empty((3, W), **f32), torch.empty(3, **f32)
    n_ws = lib.e3dge_siren_wgrad_ws_floats(B, N)
    ws = torch.empty(max(n_ws, 1), **f32)
    c = lambda t: None if t is None else t.contiguous().float()
    d_sdf, d_rgb, pts, viewdirs = c(d_sdf), c(d_rgb), c(pts), c(viewdirs)
    a = _lib.SirenWgradArgs(
        args=args, d_lin=d_lin, lin_amax=lin_amax, d_sdf=d_sdf, d_rgb=d_rgb, pts=pts, viewdirs=viewdirs, d_w=d_w, d_w_view_dirs=d_wv,
        d_w_first=d_w0, d_w_sigma=d_ws, d_b_sigma=d_bs, d_w_rgb=d_wr, d_b_rgb=d_br, ws=ws,
        ws_floats=n_ws, n_pts=N, batch=B, samples=int(samples), precision=siren.check_mode(siren.bwd_mode), box_scale=float(box_scale))
    _lib.launch("e3dge_siren_wgrad", a)
    st = styles.detach().float()
    st = st.unsqueeze(1).expand(-1, 9, -1) if st.ndim == 2 else st            # (B, 9, 256)
    dg, db = dfilm[:, :, 0], dfilm[:, :, 1]                                    # (B, 9, 256)
    d_bias = (film[:, :, 0] * db).sum(0)                                       # d b_l = sum_b gamma_l[b] d beta_l[b]
    d_gw = 15.0 * torch.einsum('bln,blk->lnk', dg, st)
    d_gb = 15.0 * dg.sum(0)
    d_bw = 0.25 * torch.einsum('bln,blk->lnk', db, st)
    d_bb = 0.25 * db.sum(0)
    weights = [d_w0] + [d_w[i] for i in range(7)] + [torch.cat([d_w[7], d_wv], 1)]
    out = []
    for l in range(9):
        out += [weights[l], d_bias[l], d_gw[l], d_gb[l], d_bw[l], d_bb[l]]
    return out + [d_wr, d_br, d_ws, d_bs]


class _PointsQuery(torch.autograd.Function):
    """run_network with a gradient path to the styles (the encoder's output) and to the query points: forward saves the
    pre-sine arguments, backward is the fused HIP chain.  With want_eik the eikonal term d sdf / d x is a third,
    differentiable output (the reference builds it with autograd.grad(create_graph=True), :796-802).  View directions
    get no gradient (they are fixed samples).  The backward is not itself differentiable (once_differentiable)."""

    @staticmethod
    def forward(ctx, styles, siren, pts, viewdirs, box_scale, mfma_mode, want_eik, *params):
        B, N = pts.shape[0], pts.shape[1]
        ctx.n_params = len(params)                     # trainable renderer: siren_trainable_params(siren), gradients returned in order
        ctx.set_materialize_grads(False)               # (unused outputs arrive as None in backward, not as zero tensors: a fill each)
        args = saved_state_buffer(B, N, 9, pts.device, siren.W)
        film = siren.film_params(styles)
        sdf, raw = siren._points_launch(film, pts, viewdirs, box_scale, True, mfma_mode, args)
        ctx.siren, ctx.styles_ndim, ctx.box_scale = siren, styles.ndim, float(box_scale)
        ctx.images = siren.device_image()
        if want_eik:
            eik, rsave = sdf_gradient(siren, film, args, box_scale)
        else:
            eik, rsave = torch.empty(0, device=pts.device), torch.empty(0, device=pts.device)
        ctx.want_eik = want_eik
        extra = (styles.detach(), pts.detach(), viewdirs if viewdirs is not None else torch.empty(0, device=pts.device)) if params else ()
        ctx.save_for_backward(film, args, rsave, *extra)
        return sdf, raw, eik

    @staticmethod
    @once_differentiable
    def backward(ctx, d_sdf, d_raw, d_eik):
        film, args, rsave = ctx.saved_tensors[:3]
        d_rgb = d_feat = None
        ds = d_sdf
        if d_raw is not None:
            d_rgb, d_feat = d_raw[..., :3], d_raw[..., 4:]
            ds = d_raw[..., 3] if ds is None else ds + d_raw[..., 3]
        tang = rs = None
        if ctx.want_eik and d_eik is not None:
            tang, rs = tangent_arguments(ctx.siren, film, args, d_eik, ctx.box_scale, ctx.images, rsave)
        lin = lin_buffers(args.shape[0], args.shape[1], args.device) if ctx.n_params else None
        dstyles, dfilm, d_pts, _ = siren_backward(ctx.siren, film, args, d_feat, d_rgb, ds, tang, rs,
                                                  want_d_pts=ctx.needs_input_grad[2], box_scale=ctx.box_scale, images=ctx.images, lin=lin)
        pgrads = ()
        if ctx.n_params:
            styles, pts, vd = ctx.saved_tensors[3:]
            pgrads = tuple(siren_param_grads(ctx.siren, film, styles, dfilm, args, lin[0], lin[1], ds, d_rgb, pts,
                                             vd if vd.numel() else None, 1, ctx.box_scale))
        if ctx.styles_ndim == 2:                   # one W shared by the nine layers (reference :189-191)
            dstyles = dstyles.sum(1)
        return ((dstyles if ctx.needs_input_grad[0] else None), None, d_pts, None, None, None, None) + pgrads


_DIFF_KEYS = ('gen_thumb_imgs', 'features', 'xyz', 'depth', 'sdf', 'hit_prob', 'eikonal_term')
_AUX_KEYS = ('mask', 'points', 'rays_d', 'viewdirs', 'dists')


class _EikShared:
    """What the eikonal tap below and _RenderQuery.backward share: the tangent arguments of the incoming d(eikonal term)."""
    __slots__ = ("siren", "film", "args", "box_scale", "tang", "d_eik", "images", "side", "tang_stream", "rsave", "rs")

    def __init__(self):
        self.siren = self.film = self.args = self.box_scale = self.tang = self.d_eik = self.images = self.rsave = self.rs = None
        self.side = self.tang_stream = None          # (deferred mode: the stream the chain ran on / the tangent runs on)


class _EikTap(torch.autograd.Function):
    """Identity on the eikonal term whose backward launches the tangent kernel (e3dge_siren_tangent) as soon as
    d(eikonal term) exists.  _RenderQuery.backward also needs d(xyz), which arrives from the surface-normal query's backward
    on the side stream; started from here, the 7-GEMM tangent pass of the ray samples runs beside that instead of after it."""

    @staticmethod
    def forward(ctx, eik, shared):
        ctx.shared = shared
        return eik.view_as(eik)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_eik):
        sh = ctx.shared
        if d_eik is not None and sh.args is not None:
            sh.d_eik = d_eik
            side = sh.side
            if side is None and _SIDE_STREAM and d_eik.is_cuda and os.environ.get("E3DGE_OVERLAP_COMPOSITE", "0") == "1":
                # round 6, measured and left OFF: with the tangent pass on a side stream, what _RenderQuery.backward launches before it needs
                # the tangent (the row copies of the incoming gradients, the backward of the compositing: e3dge_siren_render_bwd phase 1) runs
                # beside it -- 1.81 / 1.87 / 1.88 ms per step against 1.80 / 1.85 / 1.84 without on one box: the 60 us it hides come back as
                # a slower tangent pass and the extra stream hand-over
                side = _side_stream(d_eik.device, 1)
            if side is not None:
                # deferred mode: this node was created AFTER the decoder's, so its backward runs BEFORE the decoder's; the tangent goes to the
                # side stream and the decoder's backward launches that follow on this stream run beside it
                cur = torch.cuda.current_stream(d_eik.device)
                # (the output is allocated HERE, on the stream that consumes and frees it: allocated on the side stream and handed over with
                # record_stream, its 0.6 GB per sample came back too late for the next step and every step paid a fresh hipMalloc --
                # 2.0 instead of 1.57 ms per sample at four samples per GPU)
                buf = saved_state_buffer(sh.args.shape[0], sh.args.shape[1], 8, sh.args.device, sh.siren.W)
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    sh.tang, sh.rs = tangent_arguments(sh.siren, sh.film, sh.args, d_eik, sh.box_scale, sh.images, sh.rsave, out=buf)
                d_eik.record_stream(side)
                sh.tang_stream = side
            else:
                sh.tang, sh.rs = tangent_arguments(sh.siren, sh.film, sh.args, d_eik, sh.box_scale, sh.images, sh.rsave)
        return d_eik, None


class _RenderQuery(torch.autograd.Function):
    """VolumeFeatureRenderer.render with a gradient path from (rgb, features, xyz, depth, sdf, hit_prob, eikonal term) to
    the styles and -- on the second pass -- to the per-point texture FiLM (alpha, beta): e3dge_siren_render_fwd with saved
    pre-sine arguments, e3dge_siren_render_bwd for the way back.  Cameras, near / far get no gradient."""

    @staticmethod
    def differentiable(renderer, styles, focal, c2w, near, far, want_eik=False, tex_conditions=None, params=()):
        ta, tb = tex_conditions if tex_conditions is not None else (None, None)
        shared = _EikShared() if want_eik else None
        vals = _RenderQuery.apply(styles, renderer, focal, c2w, near, far, bool(want_eik), ta, tb, shared, *params)
        out = dict(zip(_DIFF_KEYS + _AUX_KEYS, vals))
        if not want_eik:
            out['eikonal_term'] = None
        elif out['eikonal_term'].requires_grad:
            if shared.side is not None:
                renderer._deferred_tap = shared          # finish_deferred() applies the tap behind the decoder's forward
            else:
                out['eikonal_term'] = _EikTap.apply(out['eikonal_term'], shared)
        return renderer._render_dict(out, c2w, near, far)

    @staticmethod
    def forward(ctx, styles, renderer, focal, c2w, near, far, want_eik, tex_alpha, tex_beta, shared=None, *params):
        # params (trainable renderer): siren_trainable_params(renderer.siren) + [sigmoid_beta], or [sigmoid_beta] alone; gradients in that order
        B, H, S = c2w.shape[0], renderer.out_im_res, renderer.N_samples
        ctx.n_params = len(params)
        # seven differentiable outputs, a stage-1 loss touches three: without this autograd hands backward a zero tensor for each of the
        # others (a fill + a transposing copy per output, and the kernels then read and add the zeros)
        ctx.set_materialize_grads(False)
        film = renderer.siren.film_params(styles)
        args = saved_state_buffer(B, H * H * S, 9, c2w.device, renderer.siren.W)
        tex = None if tex_alpha is None else (tex_alpha.detach(), tex_beta.detach())
        out = renderer.render_with_film(film, focal, c2w, near, far, tex, save_args=args)
        # marks "xyz is ready" on the launch stream: the surface-normal query that follows in forward() depends on this launch
        # only, not on the sdf chain below, and runs beside it on a side stream
        renderer._render_done = torch.cuda.Event()
        renderer._render_done.record(torch.cuda.current_stream(c2w.device))
        if want_eik and shared is not None and getattr(renderer, '_defer_sync', False) and B > 0:
            # the sdf chain beside whatever the caller launches next on this stream (the decoder's forward): second side stream
            cur = torch.cuda.current_stream(c2w.device)
            side2 = _side_stream(c2w.device, 1)
            side2.wait_event(renderer._render_done)
            with torch.cuda.stream(side2):
                eik, rsave = sdf_gradient(renderer.siren, film, args, renderer.box_scale)
            args.record_stream(side2); film.record_stream(side2)
            eik.record_stream(cur); rsave.record_stream(cur)
            shared.side = side2
            renderer._pending_sync.append(side2)
            out['eikonal_term'] = eik.reshape(B, H, H, S, 3)
        elif want_eik:
            eik, rsave = sdf_gradient(renderer.siren, film, args, renderer.box_scale)
            out['eikonal_term'] = eik.reshape(B, H, H, S, 3)
        else:
            out['eikonal_term'], rsave = torch.empty(0, device=c2w.device), torch.empty(0, device=c2w.device)
        ctx.renderer, ctx.styles_ndim, ctx.want_eik = renderer, styles.ndim, want_eik
        ctx.images = renderer.siren.device_image()
        ctx.sigmoid_beta = renderer._sigmoid_beta_value()
        ctx.has_tex = tex is not None
        ctx.shared = shared
        if shared is not None:
            shared.siren, shared.film, shared.args, shared.box_scale = renderer.siren, film, args, renderer.box_scale
            shared.images = renderer.siren.device_image()
            shared.rsave = rsave if want_eik else None
        ta = _lib.dense(tex[0]) if tex is not None else torch.empty(0, device=c2w.device)
        extra = (styles.detach(), out['viewdirs']) if len(params) > 1 else ()
        ctx.save_for_backward(film, args, out['sdf'], out['dists'], out['points'], out['hit_prob'],
                              near.reshape(B).contiguous().float(), far.reshape(B).contiguous().float(), rsave, ta, *extra)
        aux = tuple(out[k] for k in _AUX_KEYS)
        ctx.mark_non_differentiable(*aux)
        return tuple(out[k] for k in _DIFF_KEYS) + aux

    @staticmethod
    @once_differentiable
    def backward(ctx, d_rgb, d_feat, d_xyz, d_depth, d_sdf, d_hit, d_eik, *unused):
        film, args, sdf, dists, points, weights, near, far, rsave, ta = ctx.saved_tensors[:10]
        r = ctx.renderer
        siren = r.siren
        B, H, S = film.shape[0], r.out_im_res, r.N_samples
        dev = film.device
        rows = lambda t, c: None if t is None else t.reshape(B, c, H * H).transpose(1, 2).contiguous().float()
        d_rgb_map, d_feat_map, d_xyz_map = rows(d_rgb, 3), rows(d_feat, siren.W), rows(d_xyz, 3)
        d_depth_map = None if d_depth is None else d_depth.reshape(B, H * H).contiguous().float()
        d_sdf_in = None if d_sdf is None else d_sdf.reshape(B, H * H * S).contiguous().float()
        d_w_in = None if d_hit is None else d_hit.reshape(B, H * H * S).contiguous().float()
        packed, wg, _, wb, _ = ctx.images
        lib = _lib.load()
        n_pts = H * H * S
        partials = torch.empty(max(lib.e3dge_siren_bwd_partial_floats(B, n_pts), 1), device=dev, dtype=torch.float32)
        d_rgb_pts = torch.empty((B, n_pts, 3), device=dev, dtype=torch.float32)
        d_sdf_pts = torch.empty((B, n_pts), device=dev, dtype=torch.float32)
        dfilm = torch.empty((B, 9, 2, siren.W), device=dev, dtype=torch.float32)
        dstyles = torch.empty((B, 9, siren.W), device=dev, dtype=torch.float32)
        tang = rs = None
        wait_for = None
        if ctx.want_eik and d_eik is not None:
            sh = ctx.shared
            if (sh is not None and sh.tang is not None and sh.d_eik.data_ptr() == d_eik.data_ptr()
                    and sh.d_eik.shape == d_eik.shape):                     # launched early by _EikTap.backward
                tang, rs = sh.tang, sh.rs
                wait_for = sh.tang_stream                                   # (it ran on a side stream: waited for between the two launches below)
            else:
                tang, rs = tangent_arguments(siren, film, args, d_eik, r.box_scale, ctx.images, rsave)
            if sh is not None:
                sh.tang = sh.d_eik = sh.args = sh.film = sh.images = sh.tang_stream = sh.rsave = sh.rs = None
        d_ta = d_tb = tex_a = None
        if ctx.has_tex:
            tex_a = ta
            d_ta = torch.empty((B, H, H, S, siren.W), device=dev, dtype=torch.float32)
            d_tb = torch.empty((B, H, H, S, siren.W), device=dev, dtype=torch.float32)
        a = _lib.RenderBwdArgs(
            packed=packed, film=film, args=args, sdf=sdf, dists=dists, points=points, weights=weights, t_vals=r.t_vals, near=near,
            far=far, wg=wg, wb=wb, d_rgb_map=d_rgb_map, d_feat_map=d_feat_map, d_xyz_map=d_xyz_map, d_depth_map=d_depth_map,
            d_sdf=d_sdf_in, tang=tang, rsave=rs, d_weights=d_w_in, tex_alpha=tex_a, sigmoid_beta=ctx.sigmoid_beta, batch=B,
            height=H, width=H, n_samples=S, force_background=int(bool(r.force_background)),
            precision=siren.check_mode(siren.bwd_mode), d_rgb_pts=d_rgb_pts, d_sdf_pts=d_sdf_pts, partials=partials, dfilm=dfilm,
            dstyles=dstyles, d_tex_alpha=d_ta, d_tex_beta=d_tb)
        lin = d_beta = None
        if ctx.n_params:                                                     # trainable renderer (eikonal / tex passes were refused)
            d_beta = torch.empty(B * H * H, device=dev, dtype=torch.float32)
            a.d_sigmoid_beta = d_beta
        if ctx.n_params > 1:                                                 # (1 = sigmoid_beta alone: no d_lin, no contraction)
            lin = lin_buffers(B, n_pts, dev)
            a.d_lin, a.lin_amax = lin
        if wait_for is None:
            _lib.launch("e3dge_siren_render_bwd", a)
        else:
            a.phase = 1                                                      # the backward of the compositing does not read the tangent
            _lib.launch("e3dge_siren_render_bwd", a)
            torch.cuda.current_stream(dev).wait_stream(wait_for)
            a.phase = 2
            _lib.launch("e3dge_siren_render_bwd", a)
        pgrads = ()
        if ctx.n_params > 1:
            styles, viewdirs = ctx.saved_tensors[10:]
            pgrads = tuple(siren_param_grads(siren, film, styles, dfilm, args, lin[0], lin[1], d_sdf_pts, d_rgb_pts, points, viewdirs,
                                             S, r.box_scale))
        if ctx.n_params:
            pgrads += (d_beta.sum().reshape(1),)
        if ctx.styles_ndim == 2:
            dstyles = dstyles.sum(1)
        return ((dstyles if ctx.needs_input_grad[0] else None), None, None, None, None, None, None, d_ta, d_tb, None) + pgrads


def _resblock_backward_torch(x, w0, b0, w1, ws, dy):
    """Backward of out = Ws x + W1 relu(W0 relu(x) + b0) + b1 on the GPU with library GEMMs (rocBLAS through torch): the
    hidden activations are recomputed, nothing was saved by the fused forward.  Returns dx, dW0, db0, dW1, db1, dWs."""
    r0 = torch.relu(x)
    net = torch.addmm(b0, r0, w0.t())
    r1 = torch.relu(net)
    dnet = (dy @ w1) * (net > 0)
    dx = dy @ ws + (dnet @ w0) * (x > 0)
    return dx, dnet.t() @ r0, dnet.sum(0), dy.t() @ r1, dy.sum(0), dy.t() @ x


def tex_head_backward_backend():
    """E3DGE_TEXHEAD_BWD = hip (default: e3dge_tex_modulations_bwd, one launch) | library (round 4's GEMM chain with recomputation)."""
    v = os.environ.get("E3DGE_TEXHEAD_BWD", "hip").lower()
    if v not in ("hip", "library"):
        raise ValueError(f"E3DGE_TEXHEAD_BWD={v!r}: expected hip or library")
    return v


class _TexHead(torch.autograd.Function):
    """The fused texture head with a backward (stage-2 training differentiates the second pass,
    e3dge_full_runner.py:185-317): forward = e3dge_tex_modulations_fwd; backward = e3dge_tex_modulations_bwd for the data gradient (round 5:
    one launch, net recomputed inside, d net left in the workspace) + library GEMMs on (d net, relu(x), relu(net), d out, x) for whichever
    parameter gradients are wanted.  E3DGE_TEXHEAD_BWD=library restores round 4's chain of library GEMMs."""

    @staticmethod
    def forward(ctx, feats2d, block, w0, b0, w1, b1, ws):
        ctx.save_for_backward(feats2d, w0, b0, w1, ws)
        ctx.block = block
        return block._launch(feats2d)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_alpha, d_beta):
        x, w0, b0, w1, ws = ctx.saved_tensors
        if d_alpha is None:
            d_alpha = torch.zeros_like(d_beta)
        if d_beta is None:
            d_beta = torch.zeros_like(d_alpha)
        need = ctx.needs_input_grad
        if tex_head_backward_backend() == "library" or x.shape[0] == 0:
            dy = torch.cat([d_alpha, d_beta], -1).contiguous()
            dx, dw0, db0, dw1, db1, dws = _resblock_backward_torch(x, w0, b0, w1, ws, dy)
            return (dx if need[0] else None, None, dw0 if need[2] else None, db0 if need[3] else None,
                    dw1 if need[4] else None, db1 if need[5] else None, dws if need[6] else None)
        from .wgrad import amax_of, wgrad
        d_alpha, d_beta = _lib.dense(d_alpha.float()), _lib.dense(d_beta.float())
        trainable = any(need[2:])
        r_ = ctx.block._launch_bwd(x, d_alpha, d_beta, want_net=need[4], want_amax=trainable)      # (n, 320) rows, columns >= cin zero
        dx, dnet_p, net_p = r_[:3]
        dw0 = db0 = dw1 = db1 = dws = None
        cin = x.shape[1]
        dnet = dnet_p[:, :cin]
        # (round 6: the operand scales of the five weight gradients come out of the backward launch itself -- max |x|, max |[d alpha | d beta]|
        # (one bound for both halves), max |d net|, max |net|: five e3dge_amax passes over 100-MB tensors less)
        am4 = r_[3] if trainable else None
        am_x = am4[0] if trainable else None
        am_a = am_b = am4[1] if trainable else None
        # (round 6: the bias gradients -- column sums of d net / d out -- come from the weight gradient's pass over the same rows)
        if need[2]:
            r = wgrad(dnet, x, relu_b=True, amax_a=am4[2], amax_b=am_x, colsum=need[3])     # d net^T relu(x)
            dw0, db0 = r if need[3] else (r, None)
        elif need[3]:
            db0 = dnet_p.sum(0)[:cin]                                             # (the contiguous rows: a strided view reduces 25x slower)
        db1a = db1b = None
        if need[4]:                                                               # d out^T relu(net), net as the backward kernel recomputed it
            dw1 = torch.empty((512, cin), device=x.device, dtype=torch.float32)
            am_n, net = am4[3], net_p[:, :cin]
            ra = wgrad(d_alpha, net, relu_b=True, amax_a=am_a, amax_b=am_n, out=dw1[:256], colsum=need[5])
            rb = wgrad(d_beta, net, relu_b=True, amax_a=am_b, amax_b=am_n, out=dw1[256:], colsum=need[5])
            if need[5]:
                db1a, db1b = ra[1], rb[1]
        if need[6]:
            dws = torch.empty((512, cin), device=x.device, dtype=torch.float32)
            ra = wgrad(d_alpha, x, amax_a=am_a, amax_b=am_x, out=dws[:256], colsum=need[5] and db1a is None)
            rb = wgrad(d_beta, x, amax_a=am_b, amax_b=am_x, out=dws[256:], colsum=need[5] and db1a is None)
            if need[5] and db1a is None:
                db1a, db1b = ra[1], rb[1]
        if need[5]:
            db1 = torch.cat([db1a, db1b], 0) if db1a is not None else torch.cat([d_alpha.sum(0), d_beta.sum(0)], 0)
        return (dx if need[0] else None, None, dw0, db0, dw1, db1, dws)


class ResnetBlockFC(nn.Module):
    """The local branch's texture head (reference project/models/helper_modules/resnetfc.py:7-58 as built at
    vendor/pifu/lib/model/HGPIFuGANNetResidualInputResnetFC.py:84-93): x (.., size_in) ->
    shortcut(x) + fc_1(relu(fc_0(relu(x)))), one fused HIP launch (e3dge_tex_modulations_fwd).  Same parameter names
    (fc_0, fc_1, shortcut) and the reference's zero initialisation, so checkpoints load unchanged."""

    def __init__(self, size_in, size_out=512):
        super().__init__()
        if size_in > 320 or size_out != 512:
            raise NotImplementedError(f"ResnetBlockFC({size_in}, {size_out}): the kernel covers size_in <= 320, size_out = 512")
        self.size_in, self.size_h, self.size_out = size_in, min(size_in, size_out), size_out
        self.fc_0 = nn.Linear(size_in, self.size_h)
        self.fc_1 = nn.Linear(self.size_h, size_out)
        self.shortcut = nn.Linear(size_in, size_out, bias=False)
        for t in (self.fc_0.bias, self.fc_0.weight, self.fc_1.bias, self.fc_1.weight, self.shortcut.weight):
            nn.init.zeros_(t)                                        # :88-93 (and resnetfc.py:36)

    def invalidate(self):
        """Drop the packed weight images (needed after writes through `.data`; see SirenGenerator.invalidate)."""
        _lib.invalidate(self)

    def device_image(self):
        ps = [self.fc_0.weight, self.fc_0.bias, self.fc_1.weight, self.fc_1.bias, self.shortcut.weight]

        def build():
            dev = ps[0].device
            _lib.require_gpu(ps[0], "ResnetBlockFC weights")
            lib = _lib.load()
            packed = torch.empty(lib.e3dge_resblock_packed_floats(), device=dev, dtype=torch.float32)
            c = [p.detach().contiguous().float() for p in ps]
            _lib.launch("e3dge_resblock_pack_weights", packed, *c, self.size_in)
            wmax = max(float(t.abs().max().item()) for t in (c[0], c[2], c[4]))
            if wmax >= 500.0:              # the image stores 128 * w as f16
                raise RuntimeError(f"texture-head weights up to {wmax:g} do not fit the f16x3 weight image (|w| < 500)")
            return packed
        return _lib.cached(self, 'image', ps, build)

    def device_image_bwd(self):
        """The backward's weight image (W_0, W_1^T, W_s^T, W_0^T chunks + b_0), rebuilt when a parameter changes."""
        ps = [self.fc_0.weight, self.fc_0.bias, self.fc_1.weight, self.shortcut.weight]

        def build():
            dev = ps[0].device
            _lib.require_gpu(ps[0], "ResnetBlockFC weights")
            lib = _lib.load()
            packed = torch.empty(lib.e3dge_resblock_bwd_packed_floats(), device=dev, dtype=torch.float32)
            c = [p.detach().contiguous().float() for p in ps]
            _lib.launch("e3dge_resblock_bwd_pack_weights", packed, *c, self.size_in)
            # Range check of the f16x3 image (|w| < 500) without stalling the launch queue: a training head rebuilds this image every
            # step, and three blocking .item() reads per rebuild sat in front of every backward (round-5 advisor finding).  The first
            # image is checked synchronously; after that the maximum is reduced on the device, copied to pinned host memory without
            # blocking, and examined at the NEXT rebuild (by then the copy has long finished) -- weights drift, they do not jump.
            st = _lib.cached(self, 'wmax_check', (), dict)  # (pinned host scalar + event; no sources: it outlives the images)
            self._check_pending_wmax(st)
            wmax_dev = torch.stack([t.abs().max() for t in (c[0], c[2], c[3])]).max()
            if "host" not in st:
                self._raise_if_out_of_range(float(wmax_dev.item()))
                st["host"] = torch.zeros(1, dtype=torch.float32).pin_memory()
            else:
                st["host"].copy_(wmax_dev.reshape(1), non_blocking=True)
                st["event"] = torch.cuda.Event()
                st["event"].record(torch.cuda.current_stream(dev))
            return packed
        return _lib.cached(self, 'image_bwd', ps, build)

    @staticmethod
    def _raise_if_out_of_range(wmax):
        if not wmax < 500.0:
            raise RuntimeError(f"texture-head weights up to {wmax:g} do not fit the f16x3 weight image (|w| < 500)")

    def _check_pending_wmax(self, st):
        ev = st.get("event")
        if ev is not None and ev.query():
            st["event"] = None
            self._raise_if_out_of_range(float(st["host"][0]))

    def _launch_bwd(self, x, d_alpha, d_beta, want_net=False, want_amax=False):
        """x (n, size_in), d_alpha / d_beta (n, 256), contiguous fp32 on the GPU -> (d x (n, size_in), d net as (n, 320) rows of the workspace
        (columns >= size_in are zero), net likewise or None[, amax buffers (4, AMAX_FLOATS) of x, d out, d net, net from the same launch])."""
        _lib.require_gpu(x, "feats")
        n = x.shape[0]
        lib = _lib.load()
        packed = self.device_image_bwd()
        x = x.contiguous()
        dx = torch.empty_like(x)
        ws = torch.empty(lib.e3dge_tex_modulations_bwd_ws_floats(n), device=x.device, dtype=torch.float32)
        net = torch.empty((n, 320), device=x.device, dtype=torch.float32) if want_net else None
        am = torch.zeros((4, _lib.AMAX_FLOATS), device=x.device, dtype=torch.float32) if want_amax else None
        _lib.launch("e3dge_tex_modulations_bwd", packed, x, self.size_in, n, d_alpha, d_beta, dx, ws, net, am)
        if want_amax:
            return dx, ws[:n * 320].view(n, 320), net, am
        return dx, ws[:n * 320].view(n, 320), net

    def forward(self, x):
        """(.., size_in) -> (.., 512) like the reference module."""
        a, b = self.tex_modulations(x)
        return torch.cat([a, b], -1)

    def _launch(self, f):
        """f (n, size_in) contiguous fp32 on the GPU -> (alpha, beta), each (n, 256): one fused launch."""
        n = f.shape[0]
        alpha = torch.empty((n, 256), device=f.device, dtype=torch.float32)
        beta = torch.empty((n, 256), device=f.device, dtype=torch.float32)
        packed = self.device_image()
        _lib.launch("e3dge_tex_modulations_fwd", packed, f, self.size_in, n, alpha, beta)
        return alpha, beta

    def tex_film(self, feats, record_in, record_out, B, H, W, S):
        """feats (B,H,W,S,size_in) + the first render pass's layer-7 record -> `record_out` = the record of (alpha + 1) h8 + beta,
        in one launch (inference only; bit-identical to tex_modulations + the FiLM step inside the render kernel)."""
        _lib.require_gpu(feats, "feats")
        f = feats.reshape(-1, self.size_in).contiguous()
        if f.shape[0] != B * H * W * S:
            raise RuntimeError(f"local features {tuple(feats.shape)} do not match the render ({B},{H},{W},{S},{self.size_in})")
        packed = self.device_image()
        _lib.launch("e3dge_tex_film_fwd", packed, f, self.size_in, B, H, W, S, record_in, record_out)
        return record_out

    def tex_modulations(self, feats):
        """feats (.., size_in) -> (alpha, beta), each (.., 256): the split the renderer's second pass consumes.
        Differentiable (features and the five parameters) when anything requires grad: the backward recomputes the hidden
        activations and uses library GEMMs (stage-2 training, e3dge_full_runner.py:185-317)."""
        _lib.require_gpu(feats, "feats")
        if feats.shape[-1] != self.size_in:
            raise RuntimeError(f"local features must have {self.size_in} channels, got {tuple(feats.shape)}")
        lead = feats.shape[:-1]
        f = feats.reshape(-1, self.size_in).contiguous().float()
        ps = (self.fc_0.weight, self.fc_0.bias, self.fc_1.weight, self.fc_1.bias, self.shortcut.weight)
        if torch.is_grad_enabled() and (f.requires_grad or any(p.requires_grad for p in ps)) and f.shape[0]:
            alpha, beta = _TexHead.apply(f, self, *ps)
        else:
            alpha, beta = self._launch(f)
        return alpha.reshape(*lead, 256), beta.reshape(*lead, 256)


class LocalTexHead(nn.Module):
    """`netLocal` without PIFu options: only the texture-modulation head (state-dict key
    `netLocal.local_feat_to_tex_modulations_linear.*`).  The local features come in through `local_data_batch['feats']` (B,H,W,S,C)
    or are queried from `local_data_batch['feature_maps']` (local_query.py); the hourglass image filter that produces those maps is
    LocalFilterHead's, below."""

    def __init__(self, feats_dim):
        super().__init__()
        self.local_feat_to_tex_modulations_linear = ResnetBlockFC(feats_dim, 512)

    def tex_modulations_from_maps(self, renderer, cam_poses, focal, near, far, local_data_batch, lazy=False):
        from .local_query import tex_modulations_from_maps
        return tex_modulations_from_maps(self, renderer, cam_poses, focal, near, far, local_data_batch, lazy=lazy)


class LocalFilterHead(ResidualImageFilter):
    """`netLocal` with PIFu-style `local_options`: the texture-modulation head of LocalTexHead and, beside it, the hourglass image
    filter (hg_filter.py: residual_conv, depth_conv, downsample_channel_conv, image_filter and `filter()`), whose maps are what
    `local_data_batch['feature_maps']` takes."""

    def __init__(self, feats_dim, local_options):
        super().__init__(local_options)
        self.local_feat_to_tex_modulations_linear = ResnetBlockFC(feats_dim, 512)

    tex_modulations_from_maps = LocalTexHead.tex_modulations_from_maps


class SirenLocalGlobal(nn.Module):
    """Keeps the `network.netGlobal.*` / `network.netLocal.local_feat_to_tex_modulations_linear.*` checkpoint keys of
    the reference's local+global wrapper (:267-558).  Second-pass inputs (`local_data_batch`): either the local features
    'feats' (B,H,W,S,C) -- the texture FiLM (alpha, beta) is then computed by the fused head above (:327-336) -- or
    'tex' = (alpha, beta) directly; both are applied inside the fused render kernel (:217-220).  With PIFu-style `local_options`
    netLocal also carries the hourglass image filter (LocalFilterHead); with None it and every state dict are as without."""

    def __init__(self, D=8, W=256, style_dim=256, input_ch=3, input_ch_views=3, output_ch=4,
                 output_features=True, scene_scale=0.12, local_options=None, opt=None):
        super().__init__()
        self.opt = opt
        self.netGlobal = SirenGenerator(opt, D, W, style_dim, input_ch, input_ch_views, output_ch,
                                        output_features, scene_scale)
        if _opt_get(opt, 'L_pred_tex_modulations', False):
            feats_dim = int(_opt_get(opt, 'residual_local_feats_dim', 301))
            self.netLocal = LocalTexHead(feats_dim) if local_options is None else LocalFilterHead(feats_dim, local_options)
        else:
            self.netLocal = None


class VolumeFeatureRenderer(nn.Module):
    """Drop-in for the reference class (:636-2043) on the inference configuration."""

    def __init__(self, opt, style_dim=256, out_im_res=64, mode='train'):
        super().__init__()
        self.test = mode != 'train'
        self.opt = opt
        self.perturb = _opt_get(opt, 'perturb', 0)
        self.offset_sampling = not _opt_get(opt, 'no_offset_sampling', False)
        self.N_samples = int(_opt_get(opt, 'N_samples', 24))
        self.raw_noise_std = _opt_get(opt, 'raw_noise_std', 0.)
        self.return_xyz = _opt_get(opt, 'return_xyz', True)
        self.return_sdf = True                                   # hard-wired in the reference (:648)
        self.static_viewdirs = _opt_get(opt, 'static_viewdirs', True)
        self.z_normalize = not _opt_get(opt, 'no_z_normalize', False)
        self.out_im_res = out_im_res
        self.spatial_ss = _opt_get(opt, 'spatial_super_sampling_factor', 1)
        self.force_background = _opt_get(opt, 'force_background', True)
        self.with_sdf = not _opt_get(opt, 'no_sdf', False)
        self.add_fg_mask = _opt_get(opt, 'add_fg_mask', False)
        keys = opt.keys() if hasattr(opt, 'keys') else ()
        self.output_features = 'no_features_output' not in keys
        if self.with_sdf:
            self.sigmoid_beta = nn.Parameter(0.1 * torch.ones(1))
        # pixel-centre grids (:666-674); kept as buffers for callers that read them, the kernel regenerates them
        lin = torch.linspace(0.5, out_im_res - 0.5, out_im_res * self.spatial_ss)
        i, j = torch.meshgrid(lin, lin, indexing='ij')
        self.register_buffer('i', i.t().unsqueeze(0), persistent=False)
        self.register_buffer('j', j.t().unsqueeze(0), persistent=False)
        if self.offset_sampling:
            t_vals = torch.linspace(0., 1. - 1 / self.N_samples, steps=self.N_samples).reshape(1, 1, 1, -1)
        else:
            t_vals = torch.linspace(0., 1., steps=self.N_samples).reshape(1, 1, 1, -1)
        self.register_buffer('t_vals', t_vals, persistent=False)
        self.register_buffer('inf', torch.Tensor([1e10]), persistent=False)
        if self.test:
            self.perturb = False
            self.raw_noise_std = 0.
        self.channel_dim = -1
        self.samples_dim = 3
        self.input_ch = 3
        self.input_ch_views = 3
        self.feature_out_size = _opt_get(opt, 'width', 256)
        camera = _opt_get(opt, 'camera', None)
        self.dist_radius = float(_opt_get(camera, 'dist_radius', 0.12))
        self.grid_warper = UniformBoxWarp(self.dist_radius * 2)
        self.grid_un_warper = UniformBoxWarp(1 / self.dist_radius * 2)
        self.enable_local_model = bool(_opt_get(opt, 'enable_local_model', False))
        net_kwargs = dict(opt=opt, D=_opt_get(opt, 'depth', 8), W=_opt_get(opt, 'width', 256), style_dim=style_dim,
                          input_ch=self.input_ch, output_ch=4, input_ch_views=self.input_ch_views,
                          output_features=self.output_features)
        if self.enable_local_model:
            self.network = SirenLocalGlobal(local_options=_opt_get(opt, 'pifu', None), **net_kwargs)
        else:
            self.network = SirenGenerator(**net_kwargs)
        self.register_buffer('B_MAX', torch.Tensor([self.dist_radius] * 3), persistent=False)
        self.register_buffer('B_MIN', -torch.Tensor([self.dist_radius] * 3), persistent=False)
        self.local_batch = None
        self.sample_mode = False
        self._render_done = None
        self.mask_depth_thresh = 1.08                            # :910
        self._check_supported()

    # -------------------------------------------------------------------------------------------------
    def _check_supported(self):
        bad = []
        if not self.with_sdf: bad.append("no_sdf (density mode)")
        if not self.offset_sampling: bad.append("no_offset_sampling")
        if not self.static_viewdirs: bad.append("static_viewdirs=False")
        if not self.z_normalize: bad.append("no_z_normalize")
        if self.spatial_ss != 1: bad.append("spatial_super_sampling_factor != 1")
        if not self.output_features: bad.append("no_features_output")
        if not self.return_xyz: bad.append("return_xyz=False")
        if _opt_get(self.opt, 'return_feats', False): bad.append("return_feats")
        if bad:
            raise NotImplementedError("VolumeFeatureRenderer (gfx950): unsupported options: " + ", ".join(bad))

    @property
    def siren(self):
        return self.network.netGlobal if self.enable_local_model else self.network

    @property
    def box_scale(self):
        return self.grid_warper.scale_factor

    # -------------------------------------------------------------------------------------------------
    def run_network(self, inputs, viewdirs, normalize=True, styles=None, global_only=False,
                    return_sdf_only=False, **kwargs):
        """Un-composited network query on arbitrary points (reference :1052-1128).
        inputs (B, ..., 3) world-space; viewdirs broadcastable to it."""
        if viewdirs.shape != inputs.shape:
            if viewdirs.ndim != inputs.ndim:
                viewdirs = viewdirs.unsqueeze(self.samples_dim)
            viewdirs = viewdirs.expand(inputs.shape)
        lead = inputs.shape[:-1]
        B = inputs.shape[0]
        sdf, raw = self.siren.query_points(inputs.reshape(B, -1, 3), viewdirs.reshape(B, -1, 3), styles,
                                           self.box_scale, want_raw=not return_sdf_only)
        if return_sdf_only:
            return sdf.reshape(*lead, 1)
        return raw.reshape(*lead, 260)

    # -------------------------------------------------------------------------------------------------
    def render(self, focal, c2w, near, far, styles, tex_conditions=None, return_eikonal=False):
        """Fused rays -> samples -> MLP -> composite.  Returns the dict of render_rays + render
        (:1270-1287, :1695-1701), before forward()'s permutes (already applied here for free: the kernel
        writes channel-first directly)."""
        for name, t in (("cam_poses", c2w), ("focal", focal), ("near", near), ("far", far)):
            _lib.require_gpu(t, name)
        if not self.test and (self.perturb or self.raw_noise_std):
            raise NotImplementedError("stratified perturbation / raw noise (train-mode sampling) is not covered by "
                                      "the fused kernel; construct with mode='test' or perturb=0")
        if isinstance(tex_conditions, _LazyTex) and (torch.is_grad_enabled() or return_eikonal or not self._reuse_enabled(None)):
            tex_conditions = tex_conditions.materialize()          # (only the record path can use the fused head + FiLM launch)
        tex_grad = tex_conditions is not None and not isinstance(tex_conditions, _LazyTex) and (tex_conditions[0].requires_grad or tex_conditions[1].requires_grad)
        params = self._trainable_params(tex_conditions is not None, return_eikonal) if torch.is_grad_enabled() and c2w.shape[0] else ()
        if params:
            return _RenderQuery.differentiable(self, styles, focal, c2w, near, far, False, None, params)
        if torch.is_grad_enabled() and (styles.requires_grad or tex_grad) and c2w.shape[0]:
            self.siren.require_frozen("VolumeFeatureRenderer.render")
            if self.sigmoid_beta.requires_grad:
                raise NotImplementedError("renderer.sigmoid_beta requires grad, but the HIP backward treats it as frozen "
                                          "(trainer.py:1568); call requires_grad_(False) on the renderer")
            if tex_conditions is not None and return_eikonal:
                raise NotImplementedError("eikonal term together with the tex-FiLM pass")
            return _RenderQuery.differentiable(self, styles, focal, c2w, near, far, return_eikonal, tex_conditions)
        if not return_eikonal:
            key = self._reuse_key(styles, focal, c2w, near, far) if self._reuse_enabled(None) else None
            film = None
            if key is not None and tex_conditions is not None and c2w.shape[0]:
                # second pass on a first pass's record: same styles (the key says so), so the same FiLM parameters -- the record
                # keeps them (one launch less per evaluated image)
                rec = _BACKBONE.get(self)
                if rec is not None and rec.get('film') is not None and \
                        key.extended(_lib.load().e3dge_stream_capture_id(_lib.stream_of(c2w))).matches(rec['key']):
                    film = rec['film']
            if film is None:
                film = self.siren.film_params(styles)
            return self.render_with_film(film, focal, c2w, near, far, tex_conditions, reuse_key=key)
        film = self.siren.film_params(styles)
        if tex_conditions is not None:
            raise NotImplementedError("eikonal term together with the tex-FiLM pass")
        B, H, S = c2w.shape[0], self.out_im_res, self.N_samples
        args = saved_state_buffer(B, H * H * S, 9, c2w.device, self.siren.W)
        out = self.render_with_film(film, focal, c2w, near, far, None, save_args=args)
        if B:
            out['eikonal_term'] = sdf_gradient(self.siren, film, args, self.box_scale)[0].reshape(B, H, H, S, 3)
        return out

    @property
    def train_renderer(self):
        """Opt-in (default False): backward passes also return the gradients of the SIREN parameters and of sigmoid_beta (whichever
        require grad).  Off, trainable renderer parameters under a backward raise NotImplementedError."""
        return self.__dict__.get('_train_renderer', False)

    @train_renderer.setter
    def train_renderer(self, on):
        self.__dict__['_train_renderer'] = bool(on)
        self.siren.train_params = bool(on)

    def _trainable_params(self, tex, eikonal):
        """() unless train_renderer is on and a renderer parameter requires grad; then the SIREN's parameters and sigmoid_beta, or
        sigmoid_beta alone when no SIREN parameter requires grad (its gradient comes from the compositing backward, in any precision)."""
        if not self.train_renderer:
            return ()
        sb = self.sigmoid_beta
        ps = self.siren.trainable_params("VolumeFeatureRenderer.render", eikonal, tex)
        if not ps and not sb.requires_grad:
            return ()
        if not ps:                                           # only sigmoid_beta trains: the compositing backward alone
            if eikonal or tex:
                raise NotImplementedError("VolumeFeatureRenderer.render: a trainable sigmoid_beta together with the eikonal term or the "
                                          "texture-FiLM pass is not covered")
            return (sb,)
        return ps + (sb,)

    # ---- backbone hand-over between the two renders of an evaluated image -------------------------------------------------
    def _reuse_key(self, styles, focal, c2w, near, far):
        """Identity of everything layers 0..7, the sdf head and the scan depend on.  The key HOLDS the tensors it names (and
        the packed weight image): as long as a record exists their storage cannot be freed and handed to another tensor, so
        equal (data_ptr, shape, stride, version) means the same live memory with the same autograd-visible contents -- a
        freed latent and a new one the caching allocator places at the same address can no longer alias (round-3 ABA).
        Edits through `.data` / graph replays into the same buffers still need invalidate(), as for the weights."""
        dev = c2w.device
        return _ReuseKey((styles, focal, c2w, near, far, self.sigmoid_beta, self.siren.device_image()[0]),
                         (self.N_samples, self.out_im_res, str(dev), torch.cuda.current_stream(dev).cuda_stream,
                          self.siren.mfma_mode, bool(self.force_background), float(self.box_scale)))

    def _lazy_tex_ok(self, feats, head):
        """May the texture head be deferred into the record path (no autograd graph wanted anywhere near it)?"""
        return (not torch.is_grad_enabled() and self._reuse_enabled(None) and _fuse_texfilm() and torch.is_tensor(feats)
                and feats.ndim == 5 and feats.shape[-1] == head.size_in and feats.dtype == torch.float32 and feats.device.type == "cuda")

    def _reuse_enabled(self, save_args):
        return (_reuse_backbone() and save_args is None and not torch.is_grad_enabled() and self.enable_local_model
                and self.siren.check_mode(self.siren.mfma_mode) == _lib.PREC_F16X3)

    def render_with_film(self, film, focal, c2w, near, far, tex_conditions=None, save_args=None, reuse_key=None):
        """The single fused launch (e3dge_siren_render_fwd) given precomputed FiLM parameters (B,9,2,256).
        `reuse_key` (render(): inference with a local branch): a launch WITHOUT texture conditions also writes its layer-7
        output, and a following launch WITH texture conditions and the same key -- the second pass of que_render_given_ref,
        e3dge_full_runner.py:185-317 -- reads it back instead of recomputing layers 0..7, the sdf head and the transmittance
        scan (they do not see the texture FiLM; the result is bit-identical).  E3DGE_REUSE_BACKBONE=0 turns this off."""
        B = c2w.shape[0]
        H = Wd = self.out_im_res
        S = self.N_samples
        dev = c2w.device
        packed = self.siren.device_image()[0]
        c2w_c = c2w[:, :3, :4].contiguous()
        focal_c = focal.reshape(B).contiguous()
        near_c = near.reshape(B).contiguous()
        far_c = far.reshape(B).contiguous()
        lazy = tex_conditions if isinstance(tex_conditions, _LazyTex) else None
        ab = tex_conditions if lazy is None else None       # (alpha, beta) given, or materialised below when the record path is closed
        f32 = dict(device=dev, dtype=torch.float32)
        use = bb_out = None
        if reuse_key is not None and B > 0 and self._reuse_enabled(save_args):
            # producer and consumer of a record must be both eager or both inside the same graph capture (a graph holding only the
            # second pass would replay against whatever the record held at capture time)
            cap_id = _lib.load().e3dge_stream_capture_id(_lib.stream_of(c2w))
            reuse_key = reuse_key.extended(cap_id)
            rec = _BACKBONE.get(self)
            if tex_conditions is None:                       # first pass: leave a record behind
                n_bytes = _lib.load().e3dge_siren_backbone_bytes(B, H, Wd, S)
                bb_out = _record_buffer(self, 'bb', n_bytes, dev, _lib.stream_of(c2w), cap_id != 0, zero=False)
                _BACKBONE[self] = None                        # (not valid until the launch below is queued)
            elif rec is not None and reuse_key.matches(rec['key']) and \
                    all(t._version == v for t, v in zip(rec['out'].values(), rec['out_versions'])):
                use = rec                                     # (a first-pass output edited in place since is a miss, not a stale read)
        elif tex_conditions is None:
            _BACKBONE.pop(self, None)                         # a plain render that leaves no record must not leave an older one valid
        bb_in = use['buf'] if use is not None else None
        if lazy is not None:
            n_rec = use['buf'].numel() if use is not None else 0
            if (use is not None and _fuse_texfilm() and lazy.feats.dtype == torch.float32 and lazy.feats.device == dev
                    and tuple(lazy.feats.shape[:4]) == (B, H, Wd, S) and 0 < n_rec < 2 ** 32 and B * H * Wd * S < 2 ** 31):
                # the FiLM-ed record outlives the layer-7 records it is computed from (one buffer per stream and size, zero-filled ONCE:
                # padding slabs are never written): allocating it per record put a 100-MB fill into every captured forward
                tb_ = _record_buffer(self, 'film', n_rec, dev, _lib.stream_of(c2w),
                                     _lib.load().e3dge_stream_capture_id(_lib.stream_of(c2w)) != 0, zero=True)
                use['tex_buf'] = tb_
                bb_in = lazy.head.tex_film(lazy.feats, use['buf'], tb_, B, H, Wd, S)
            else:
                ab = lazy.materialize()
        ta = tb = None
        if ab is not None:
            ta, tb = ab
            _lib.require_gpu(ta, "tex alpha"); _lib.require_gpu(tb, "tex beta")
            if tuple(ta.shape) != (B, H, Wd, S, 256) or tuple(tb.shape) != (B, H, Wd, S, 256):
                raise RuntimeError(f"tex conditions must be (B,H,W,S,256) = {(B, H, Wd, S, 256)}; got {tuple(ta.shape)}")
            ta, tb = _lib.dense(ta), _lib.dense(tb)
        if use is not None:
            o1 = use['out']
            out = dict(o1, rgb=torch.empty((B, 3, H, Wd), **f32), features=torch.empty((B, 256, H, Wd), **f32))
            own = ('rgb', 'features')
        else:
            out = dict(
                rgb=torch.empty((B, 3, H, Wd), **f32), features=torch.empty((B, 256, H, Wd), **f32),
                xyz=torch.empty((B, 3, H, Wd), **f32), depth=torch.empty((B, H, Wd, 1, 1), **f32),
                mask=torch.empty((B, 1, H, Wd, 1), **f32), sdf=torch.empty((B, H, Wd, S, 1), **f32),
                weights=torch.empty((B, H, Wd, S, 1), **f32), points=torch.empty((B, H, Wd, S, 3), **f32),
                rays_d=torch.empty((B, H, Wd, 3), **f32), viewdirs=torch.empty((B, H, Wd, 3), **f32),
                dists=torch.empty((B, H, Wd, S), **f32))
            own = tuple(out)
        op = {k: (out[k] if k in own else None) for k in out}
        args = _lib.RenderArgs(
            packed=packed, film=film, c2w=c2w_c, focal=focal_c, near=near_c, far=far_c, t_vals=self.t_vals,
            tex_alpha=ta, tex_beta=tb,
            sigmoid_beta=self._sigmoid_beta_value(),
            box_scale=float(self.box_scale), mask_depth_thresh=float(self.mask_depth_thresh),
            batch=B, height=H, width=Wd, n_samples=S, res=int(self.out_im_res),
            force_background=int(bool(self.force_background)),
            precision=self.siren.save_precision() if save_args is not None else self.siren.check_mode(self.siren.mfma_mode),
            rgb=op['rgb'], features=op['features'], xyz=op['xyz'], depth=op['depth'], mask=op['mask'], sdf=op['sdf'],
            weights=op['weights'], points=op['points'], rays_d=op['rays_d'], viewdirs=op['viewdirs'], dists=op['dists'],
            save_args=save_args, backbone_out=bb_out, backbone_in=bb_in if use is not None else None,
            weights_in=use['out']['weights'] if use is not None else None)
        _lib.launch("e3dge_siren_render_fwd", args)
        if bb_out is not None:
            # the record keeps the geometry tensors a second pass returns (a few MB), not the first pass's rgb / features
            geo = {k: v for k, v in out.items() if k not in ('rgb', 'features')}
            _BACKBONE[self] = dict(key=reuse_key, buf=bb_out, out=geo, out_versions=[t._version for t in geo.values()], film=film)
        return self._render_dict({'rays_d': out['rays_d'], 'dists': out['dists'], 'hit_prob': out['weights'],
                                  'points': out['points'], 'sdf': out['sdf'], 'gen_thumb_imgs': out['rgb'],
                                  'features': out['features'], 'mask': out['mask'], 'xyz': out['xyz'],
                                  'depth': out['depth'], 'viewdirs': out['viewdirs']}, c2w, near, far)

    def _render_dict(self, tensors, c2w, near, far):
        """The dict of render_rays + render (:1270-1287, :1695-1701) around the kernel's output tensors."""
        B, H = c2w.shape[0], self.out_im_res
        d = {'rays_o': c2w[:, None, None, :3, -1].expand(B, H, H, 3),
             'near': near.reshape(B, 1, 1, 1).expand(B, H, H, 1), 'far': far.reshape(B, 1, 1, 1).expand(B, H, H, 1),
             'surface_eikonal_term': None, 'eikonal_term': None, 'mesh': None, 'shading_mesh': None, 'debug_mesh': None}
        d.update(tensors)
        return d

    def _sigmoid_beta_value(self):
        """Host copy of the learned sigmoid_beta, refreshed only when the parameter changes (a `.item()` per
        call would put a device synchronisation in front of every render).  Writes through `.data` need invalidate()."""
        p = self.sigmoid_beta
        return _lib.cached(self, 'sigmoid_beta', (p,), lambda: float(p.detach().item()))

    def invalidate(self):
        """Forget every host / device copy derived from the parameters (packed SIREN image, texture-head image,
        sigmoid_beta).  Needed only after updates that bypass autograd's version counter (`p.data.mul_()`, the reference's
        EMA accumulate(), utils/training_utils.py:45); optimizer steps, load_state_dict, .to() and train()/eval() are
        detected without it."""
        _lib.invalidate(self)                                 # (this module's and every sub-module's: SIREN, texture head)
        _BACKBONE.pop(self, None)                             # (the first pass's layer-7 record was computed from the old values)
        pool = _RECORD_BUFS.get(self)
        if pool:                                              # storage a captured graph points into stays; the rest is released
            for k in [k for k, e in pool.items() if not e[1]]:
                pool.pop(k)

    # ---- deferred synchronisation (the generator runs the decoder between begin_deferred() and finish_deferred()) ------------------------
    def begin_deferred(self):
        """The next forward may leave its side-stream work (sdf chain of the ray samples, surface-normal query) un-joined: the caller
        promises to call finish_deferred(render_out) before anybody reads 'eikonal_term' / 'surface_eikonal_term'."""
        self._defer_sync = bool(_overlap_decoder() and _SIDE_STREAM)
        self._pending_sync = []
        self._deferred_tap = None
        return self._defer_sync

    def finish_deferred(self, render_out):
        """Join the side streams on the current stream and put the tangent tap on the eikonal term (created HERE, behind the decoder's
        node, so that autograd runs it before the decoder's backward)."""
        pend, tap = getattr(self, '_pending_sync', None) or [], getattr(self, '_deferred_tap', None)
        self._defer_sync, self._pending_sync, self._deferred_tap = False, [], None
        if pend:
            cur = torch.cuda.current_stream(pend[0].device)
            for st in pend:
                cur.wait_stream(st)
        if tap is not None and render_out.get('eikonal_term', None) is not None:
            render_out['eikonal_term'] = _EikTap.apply(render_out['eikonal_term'], tap)
        return render_out

    # -------------------------------------------------------------------------------------------------
    def forward(self, cam_poses, focal, near, far, styles=None, return_eikonal=False, geometry_sample=None,
                return_surface_eikonal=False, local_data_batch=None, sample_mode=False, return_mesh=False,
                mesh_with_shading=True, return_sdf_only=False, sample_without_grad=False, **kwargs):
        if sample_without_grad and torch.is_grad_enabled():
            # the reference detaches every output in this mode (:1291-1294); running the whole query without a graph is
            # the same result without saving 9.2 KB of pre-sine arguments per point
            with torch.no_grad():
                return self.forward(cam_poses, focal, near, far, styles=styles, return_eikonal=return_eikonal,
                                    geometry_sample=geometry_sample, return_surface_eikonal=return_surface_eikonal,
                                    local_data_batch=local_data_batch, sample_mode=sample_mode, return_mesh=return_mesh,
                                    mesh_with_shading=mesh_with_shading, return_sdf_only=return_sdf_only, **kwargs)
        self.sample_mode = bool(sample_mode)
        self._render_done = None          # (an event left by an earlier grad-mode render that nobody consumed must not order THIS call)
        tex = None
        if self.enable_local_model and local_data_batch is not None:
            if 'tex' in local_data_batch:
                tex = local_data_batch['tex']
            elif local_data_batch.get('feats', None) is not None and self.network.netLocal is not None:
                # already-queried local features (forward_local :434-437) -> texture FiLM (:327-336), fused head
                head = self.network.netLocal.local_feat_to_tex_modulations_linear
                tex = _LazyTex(head, local_data_batch['feats']) if self._lazy_tex_ok(local_data_batch['feats'], head) \
                    else head.tex_modulations(local_data_batch['feats'])
            elif local_data_batch.get('feature_maps', None) is not None and self.network.netLocal is not None:
                # feature maps of the local branch: the per-point query (projection + bilinear gather + positional
                # encoding, e3dge_full_runner.py:185-317) runs in HIP and feeds the texture head directly
                tex = self.network.netLocal.tex_modulations_from_maps(self, cam_poses, focal, near, far, local_data_batch, lazy=True)
                if isinstance(tex, _LazyTex) and not self._lazy_tex_ok(tex.feats, tex.head):
                    tex = tex.materialize()
            else:
                raise NotImplementedError(
                    "local_data_batch must carry the local features 'feats' (B,H,W,S,C) [with L_pred_tex_modulations], the "
                    "local branch's 'feature_maps' or the texture FiLM conditions 'tex' = (alpha, beta); the hourglass image "
                    "filters of the PIFu branch are outside this build (SURVEY.md 8f-2)")
            self.local_batch = local_data_batch
        else:
            self.local_batch = None

        render_out = self.render(focal, cam_poses, near, far, styles, tex_conditions=tex, return_eikonal=return_eikonal)
        if return_mesh:
            # surface extraction (:1703-1731): the rendered SDF volume onto the regular grid and marching cubes, both in HIP
            # ('aligned_sdf', 'mesh_verts', 'mesh_faces').  'mesh' is the reference's skimage / trimesh mesh when those are installed,
            # otherwise built from the HIP arrays
            from . import mesh_utils
            aligned = render_out['aligned_sdf'] = mesh_utils.align_volume(render_out['sdf'].detach())
            try:
                mverts, mfaces = mesh_utils.marching_cubes(aligned)
            except (ValueError, mesh_utils.NoSurfaceError) as e:   # no zero crossing (the reference prints and goes on)
                render_out['mesh_verts'] = torch.empty(0, 3, dtype=torch.float32, device=aligned.device)
                render_out['mesh_faces'] = torch.empty(0, 3, dtype=torch.int32, device=aligned.device)
                render_out['mesh'] = render_out['shaded_mesh'] = None
                render_out['mesh_error'] = str(e)
            else:
                render_out['mesh_verts'], render_out['mesh_faces'] = mverts, mfaces
                if mesh_utils.third_party_available():
                    mesh = mesh_utils.marching_cubes_mesh(aligned)[0]
                else:
                    mesh = mesh_utils.mesh_from_hip(mverts, mfaces)
                render_out['mesh'], render_out['shaded_mesh'] = mesh, mesh
        if return_surface_eikonal:
            # normal at the integrated surface point (:921-930).  As in the reference the point stays in the graph: the
            # term's gradient reaches the styles through the network AND through d xyz / d styles (the Hessian-vector
            # product e3dge_siren_bwd returns as d_pts, chained into the compositing backward as d_xyz).
            B = cam_poses.shape[0]
            dev = cam_poses.device
            ev = getattr(self, '_render_done', None)
            self._render_done = None
            if ev is not None and return_eikonal and _SIDE_STREAM:
                # 4,096 surface points are 32 workgroups; the sdf chain of the ray samples, still running on the launch stream,
                # leaves a quarter of the CUs free at S = 18: the two overlap.  autograd runs this query's backward on the side
                # stream as well and orders it against the consumers of its gradients.
                cur = torch.cuda.current_stream(dev)
                side = _side_stream(dev)
                side.wait_event(ev)
                with torch.cuda.stream(side):
                    surf = render_out['xyz'].permute(0, 2, 3, 1).reshape(B, -1, 3)
                    _, _, se = self.siren.query_points(surf, None, styles, self.box_scale, want_raw=False, want_eikonal=True)
                    se = se.reshape(B, self.out_im_res, self.out_im_res, 1, 3)
                render_out['xyz'].record_stream(side)
                if torch.is_tensor(styles):
                    styles.record_stream(side)
                if getattr(self, '_defer_sync', False):
                    self._pending_sync.append(side)          # (finish_deferred() waits, behind the decoder's forward)
                else:
                    cur.wait_stream(side)
                se.record_stream(cur)
                render_out['surface_eikonal_term'] = se
            else:
                surf = render_out['xyz'].permute(0, 2, 3, 1).reshape(B, -1, 3)
                _, _, se = self.siren.query_points(surf, None, styles, self.box_scale, want_raw=False, want_eikonal=True)
                render_out['surface_eikonal_term'] = se.reshape(B, self.out_im_res, self.out_im_res, 1, 3)

        if geometry_sample:   # 3-D supervision re-queries (:1916-1949)
            corpus = ['uniform_pts'] + (['xyz'] if geometry_sample.get('xyz', None) is not None else [])
            for k in corpus:
                if k not in geometry_sample:
                    continue
                samples = geometry_sample[k]
                if samples.ndim == 4:
                    samples = samples.unsqueeze(self.samples_dim)
                if return_surface_eikonal and k == 'xyz':      # normals of the surface samples (:1944-1949)
                    Bq = samples.shape[0]
                    sdf_q, _, eik_q = self.siren.query_points(samples.reshape(Bq, -1, 3), None, styles, self.box_scale,
                                                              want_raw=False, want_eikonal=True)
                    render_out[f'{k}_rec'] = sdf_q.reshape(*samples.shape[:-1], 1)
                    render_out[f'{k}_rec_eikonal_term'] = eik_q.reshape(samples.shape)
                    continue
                render_out[f'{k}_rec'] = self.run_network(samples, torch.zeros_like(samples), styles=styles,
                                                          return_sdf_only=True)
        if self.sample_mode:
            # pseudo ground truth for the 3-D supervision of stage 1 (render_rays :1297-1324, then collate_fn :1976-2043):
            # sdf at jittered surface points and at uniform points of the scene box; xyz / mask keep the channel-last
            # layout in this mode (:1951-1958)
            B = cam_poses.shape[0]
            xyz_cl = render_out['xyz'].permute(0, 2, 3, 1).contiguous()
            if _opt_get(self.opt, 'sample_near_surface', False):
                pts, sdf_s, valid = self.sample_near_surface_grid(
                    xyz_cl, render_out['viewdirs'], float(_opt_get(self.opt, 'surface_sampling_stdv', 0.03)), styles,
                    noise=kwargs.get('surface_noise', None))
                render_out.update(points_near_surface=pts, points_near_surface_sdf=sdf_s, points_near_surface_valid_mask=valid)
            if _opt_get(self.opt, 'sample_uniform_grid', False):
                gp, gs, gm = self.sample_uniform_grid(B, int(_opt_get(self.opt, 'uniform_grid_sampling_num', 2048)),
                                                      cam_poses.device, styles, uniform=kwargs.get('grid_uniform', None))
                render_out.update(grid_random_pts=gp, grid_random_pts_sdf=gs, grid_sample_valid_mask=gm)
            render_out['xyz'] = xyz_cl
            render_out['mask'] = render_out['mask'].permute(0, 2, 3, 4, 1).contiguous()      # back to (B,H,W,1,1)
            render_out = self.collate_fn(render_out)
            self.sample_mode = False
        return render_out

    # -------------------------------------------------------------------------------------------------
    def query_hitting_probability_fixed_interval(self, wd_space_pts, ref_img_info, return_type='weights'):
        """Hit probability (or visibility) of world-space points as seen from a reference view (reference :1326-1495, caller
        cycle_runner.py:139-158): for every point the ray from the reference camera through it is re-sampled at the
        renderer's S fixed depths, the SDF network is queried there (fused point kernel, sdf only), the samples are
        composited WITHOUT the far-plane stop (`no_force_stop`: last interval = first interval, no background weight,
        :826-837, :884), and the per-sample value is linearly interpolated at the point's position along its ray.
        wd_space_pts (B,H,W,S,3) -> (B,H,W,S,1).  Everything runs on the GPU; no gradient is provided."""
        if return_type not in ('weights', 'visibility'):
            raise ValueError("return_type must be 'weights' or 'visibility'")
        if wd_space_pts.ndim != 5:
            raise RuntimeError("wd_space_pts must be (B, H, W, S, 3)")
        if not self.static_viewdirs:
            raise NotImplementedError("static_viewdirs=False")
        _lib.require_gpu(wd_space_pts, "wd_space_pts")
        B, H, W, S = wd_space_pts.shape[:4]
        Sn = self.N_samples
        ro = ref_img_info['global_render_out']
        poses = ref_img_info['cam_settings']['poses']                       # (B,3,4) c2w
        extr = ref_img_info['cam_settings']['extrinsics']                   # (B,3,4) w2c
        styles = ref_img_info['pred_latents'][0]
        dev = wd_space_pts.device
        for name, t in (("cam_settings.poses", poses), ("cam_settings.extrinsics", extr), ("global_render_out.near", ro['near']),
                        ("global_render_out.far", ro['far']), ("pred_latents[0]", styles)):
            if not torch.is_tensor(t) or t.device != dev:      # raw pointers go to the kernels: a CPU / other-device tensor must raise here
                raise RuntimeError(f"query_hitting_probability_fixed_interval: {name} must be a tensor on {dev} "
                                   f"(got {getattr(t, 'device', type(t))})")
        with torch.no_grad():
            N = H * W
            near = ro['near'].reshape(B, N).contiguous().float()
            far = ro['far'].reshape(B, N).contiguous().float()
            pts = wd_space_pts.reshape(B, N, S, 3).contiguous().float()
            pc, ec, tv = poses[:, :3, :4].contiguous().float(), extr[:, :3, :4].contiguous().float(), self.t_vals.contiguous()
            q = torch.empty((B, N * S * Sn, 3), device=dev, dtype=torch.float32)
            aux = torch.empty((B, N, S, 4), device=dev, dtype=torch.float32)
            out = torch.empty((B, N, S), device=dev, dtype=torch.float32)
            # launch 1: the Sn samples of the reference camera's ray through every point + where the point sits between them
            _lib.launch("e3dge_hitprob_points", q, aux, pts, pc, ec, near, far, tv, B, N, S, Sn)
            # launch 2: sdf of all B*HW*S*Sn samples (view directions do not enter the sdf head)
            sdf = self.siren.query_points(q, None, styles, self.box_scale, want_raw=False)[0]
            # launch 3: alpha, transmittance scan without the far-plane stop, interpolation
            _lib.launch("e3dge_hitprob_composite", out, sdf.contiguous(), aux, near, far, tv, float(self._sigmoid_beta_value()),
                        int(return_type == 'visibility'), B, N, S, Sn)
        return out.reshape(B, H, W, S, 1)

    # -------------------------------------------------------------------------------------------------
    def sample_uniform_grid(self, batch_size, num_sample_inout, device, styles, uniform=None):
        """Uniform points of the scene box and their sdf (:945-963).  `uniform` (B,N,3) in [0,1) replaces the torch.rand
        draw (tests)."""
        u = torch.rand(batch_size, num_sample_inout, 3, device=device) if uniform is None else uniform
        pts = (u * (self.B_MAX - self.B_MIN) + self.B_MIN).reshape(batch_size, num_sample_inout, 1, 1, 3)
        sdf = self.run_network(pts, torch.zeros_like(pts), styles=styles, return_sdf_only=True)[..., 0]
        pts = pts.reshape(batch_size, -1, 3)
        sdf = sdf.reshape(batch_size, -1, 1)
        return pts, sdf, torch.ones_like(sdf)

    def sample_near_surface_grid(self, surface_points, viewdirs, normal_stdv, styles, multiplier=1, noise=None):
        """Surface points (B,H,W,3) jittered by N(0, stdv^2) and their sdf (:965-1003).  `noise` replaces the
        torch.randn_like draw (tests)."""
        n = torch.randn_like(surface_points) if noise is None else noise
        pts = (surface_points + n * normal_stdv).unsqueeze(-2)                           # (B,H,W,1,3)
        valid = (pts.abs().max(dim=-1)[0] < self.dist_radius).int()                       # (B,H,W,1)
        sdf = self.run_network(pts, viewdirs, styles=styles, return_sdf_only=True)[..., 0]   # (B,H,W,1)
        return pts, sdf, valid

    def collate_fn(self, render_out, match_inference_dim=True):
        """Merge the sampled point sets into `uniform_pts`, `uniform_points_sdf`, `uniform_points_valid_mask`
        (:1976-2043)."""
        B = render_out['gen_thumb_imgs'].shape[0]
        dev = render_out['gen_thumb_imgs'].device
        P = [torch.empty(B, 0, 3, device=dev)]
        S = [torch.empty(B, 0, 1, device=dev)]
        M = [torch.empty(B, 0, 1, device=dev)]
        if _opt_get(self.opt, 'sample_near_surface', False):
            P.append(render_out['points_near_surface'].reshape(B, -1, 3))
            S.append(render_out['points_near_surface_sdf'].reshape(B, -1, 1))
            M.append(render_out['points_near_surface_valid_mask'].reshape(B, -1, 1).float())
        if _opt_get(self.opt, 'sample_uniform_grid', False):
            P.append(render_out['grid_random_pts'].reshape(B, -1, 3))
            S.append(render_out['grid_random_pts_sdf'].reshape(B, -1, 1))
            M.append(render_out['grid_sample_valid_mask'].reshape(B, -1, 1))
        pts, sdf, msk = torch.cat(P, 1), torch.cat(S, 1), torch.cat(M, 1)
        if match_inference_dim:
            pts, sdf, msk = pts.reshape(B, -1, 1, 1, 3), sdf.reshape(B, -1, 1, 1, 1), msk.reshape(B, -1, 1, 1, 1)
        render_out.update(uniform_pts=pts, uniform_points_sdf=sdf, uniform_points_valid_mask=msk)
        return render_out
