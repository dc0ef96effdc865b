"""Strided, offset and expanded tensors through the module entries (DESIGN.md 'What a kernel may be handed').

Every row of ROWS is one public entry at its smallest case.  A row's inputs come from the builders of the existing parity tests wherever
one exists, so the dense run here is the run those tests bound against float64; this file restates no reference.  Per row:

    * one input at a time takes each layout of tests/layout_variants.py that applies to its shape, and once all inputs take one together;
    * every returned tensor must have the bits of the dense run's (NaN included), the input view and the sentinels around it must be
      unchanged, and no output may live in an input's buffer;
    * upstream gradients are inputs like any other, restricted to the layouts autograd delivers: `expanded` (out.sum().backward()),
      `offset4` and `pitch`;
    * the dense case runs once more on a side stream and must give the same bits.

The gate (an autouse fixture, nothing in conftest.py) wraps `_lib.launch`, `_lib.query` and the pointer fields of `_lib._Args` for every
test of this file.  Before the real call it asserts that each tensor is contiguous (or listed in TAKES_STRIDES, with its pitch argument
equal to its stride) and 16-byte aligned (or listed in FOUR_BYTE_OK, with the kernel access that allows it): a violation is an
AssertionError on the host and nothing is launched, so no test here can hand a kernel a layout it does not expect.  The gate also
records the entry names, for the native-path check of every case and for the coverage test at the end of the file.

One exception to bit equality, by construction of the kernel and not of this test: `d_fmap` of the local-query gather (and the two map
gradients of the training form of local_features_from_maps) is a sum of fp32 atomic adds in arbitrary order (tests/test_local_query.py);
it is compared at that test's standing bound, 2e-5 of the maximum: ATOMIC_OUTPUTS."""
import functools
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib, losses, mesh_utils, synthetic as syn
from e3dge_amd.camera_utils import generate_camera_params

import layout_variants as lv
from test_layouts_host import launched_entry_names

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UPSTREAM_KINDS = ("expanded", "offset4", "pitch")

# ---------------------------------------------------------------------------------------------------------------------------- the lists
# (entry, index of the argument) or (argument struct, field) -> where the kernels read it with nothing wider than 4 bytes, or branch.
FOUR_BYTE_OK = {
    **{(f"e3dge_fused_bias_act{s}", i): "stream_ops.hip:138 launch_bias_act takes the vector kernel only when x, y and ref are 16-byte aligned"
       for s in ("", "_f16", "_f64") for i in (0, 1, 2, 3)},
    **{(f"e3dge_upfirdn2d{s}", 1): "upfirdn2d.hip:98 the planes are staged into LDS one element at a time (:352, :381 the generic kernels)"
       for s in ("", "_f16", "_f64")},
    **{(f"e3dge_upfirdn2d{s}", 2): "upfirdn2d.hip:240 the FIR taps one at a time (:352 the generic kernels)" for s in ("", "_f16", "_f64")},
    ("e3dge_blur_noise_bias_act", 3): "upfirdn2d.hip:154 the 16-byte noise load only when the plane is aligned (:282 the 4x4 form)",
    ("e3dge_avgpool_fwd", 0): "losses.hip:319 vector form only when out and in are aligned",
    ("e3dge_avgpool_fwd", 1): "losses.hip:319 vector form only when out and in are aligned",
    ("e3dge_avgpool_bwd", 0): "losses.hip:343 vector store only when d_in is aligned",
    ("e3dge_avgpool_bwd", 1): "losses.hip:77 and losses.hip:90 d_out is read one float at a time in both kernels",
    ("e3dge_sqerr_bwd", 0): "losses.hip:369 vec only when d_pred, pred and gt are aligned",
    ("e3dge_sqerr_bwd", 1): "losses.hip:369",
    ("e3dge_sqerr_bwd", 2): "losses.hip:369",
    ("e3dge_sqerr_bwd", 4): "losses.hip:97 one float",
    ("ShapeLossSegment", "pred"): "losses.hip:274 o.vec only when pred, gt and d_pred are aligned",
    ("ShapeLossSegment", "gt"): "losses.hip:274",
    ("ShapeLossSegment", "d_pred"): "losses.hip:274",
    ("ShapeLossArgs", "upstream"): "losses.hip:225 one float",
    ("e3dge_image_metrics", 2): "metrics.hip:44 pred one float at a time",
    ("e3dge_image_metrics", 3): "metrics.hip:45 gt one float at a time",
    ("e3dge_image_metric_row", 1): "metrics.hip:127 the per-image sums",
    ("e3dge_image_metric_row", 2): "metrics.hip:128 lp[b]",
    ("e3dge_image_metric_row", 3): "metrics.hip:130 id[0] (element 3 B of the id-loss result buffer)",
    ("e3dge_local_query", 7): "local_query.hip:52 p[0], p[1], p[2]",
    ("e3dge_local_query", 8): "local_query.hip:58 calibs one float at a time",
    ("e3dge_local_query_bwd", 5): "local_query.hip:185 p[0..2]",
    ("e3dge_local_query_bwd", 6): "local_query.hip:211 calibs one float at a time",
    ("e3dge_local_query_bwd_sorted", 5): "local_query.hip:185 the same kernel (the sort key reads the same way)",
    ("e3dge_local_query_bwd_sorted", 6): "local_query.hip:211 the same kernel (the sort key reads the same way)",
    ("e3dge_pos_encoding", 3): "local_query.hip:355 pts[m * 3 + ax]",
    ("e3dge_hitprob_points", 2): "hitprob.hip:31 pts",
    ("e3dge_hitprob_points", 3): "hitprob.hip:37 the pose rows",
    ("e3dge_hitprob_points", 4): "hitprob.hip:33 the extrinsics rows",
    ("e3dge_hitprob_points", 5): "hitprob.hip:38 near",
    ("e3dge_hitprob_points", 6): "hitprob.hip:38 far",
    ("e3dge_hitprob_points", 7): "hitprob.hip:39 t_vals",
    ("e3dge_hitprob_composite", 1): "hitprob.hip:79 sd[s]",
    ("e3dge_hitprob_composite", 2): "hitprob.hip:70 aux",
    ("e3dge_hitprob_composite", 3): "hitprob.hip:69 near",
    ("e3dge_hitprob_composite", 4): "hitprob.hip:69 far",
    ("e3dge_hitprob_composite", 5): "hitprob.hip:73 t_vals",
    ("Wgrad", "a"): "wgrad.hip:43 WgU4 is packed, aligned(4): rows of any pitch",
    ("Wgrad", "b"): "wgrad.hip:43",
    ("Wgrad", "c"): "wgrad.hip:43",
    # the convolution networks gather a caller's image one float at a time (the implicit-GEMM B operand, conv_igemm.h); every 8- and
    # 16-byte cast of these files goes to a weight image, an (a, b) table or an activation of the workspace
    ("LpipsArgs", "x"): "lpips.hip:90",
    ("LpipsArgs", "y"): "lpips.hip:90",
    ("LpipsBwdArgs", "upstream"): "lpips_bwd.h:98",
    ("DiscArgs", "images"): "disc.hip:143 (a larger image is pooled first: losses.hip:319 branches)",
    ("DiscBwdArgs", "grad_logits"): "disc_bwd.h:30",
    ("EncArgs", "images"): "idnet.hip:160 (id_conv, the stem of encoder.h:339)",
    ("AlignerArgs", "res_gt"): "aligner.hip:122",
    ("AlignerArgs", "thumb"): "aligner.hip:122",
    ("HgfArgs", "input"): "hgfilter.hip:72",
    **{(e, i): "hgfilter.hip:72 (the front nets are the same conv kernel)" for e in ("e3dge_hgf_front", "e3dge_hgf_front_saving") for i in (1, 2)},
    ("HgfBwdArgs", "g_normx"): "hgfilter_bwd.h:78 the data-gradient gather (hgfilter_bwd.h:70 reflect padding)",
    ("HgfBwdArgs", "input"): "hgfilter_bwd.h:363 the weight-gradient gather",
    ("e3dge_hgf_front_backward", 17): "hgfilter_bwd.h:363",
    ("e3dge_hgf_front_backward", 18): "hgfilter_bwd.h:363",
    ("e3dge_depth_mesh", 2): "mesh_render.hip:37",
    ("e3dge_vertex_normals", 1): "mesh_render.hip:73",
    ("e3dge_vertex_normals", 2): "mesh_render.hip:69",
    ("e3dge_mesh_subdivide", 2): "mesh_render.hip:543",
    ("e3dge_mesh_subdivide", 3): "mesh_render.hip:551",
    **{(st, "verts"): "mesh_render.hip:158" for st in ("MeshRenderArgs", "NoiseProjectArgs")},
    **{(st, "faces"): "mesh_render.hip:181" for st in ("MeshRenderArgs", "NoiseProjectArgs")},
    ("MeshRenderArgs", "normals"): "mesh_render.hip:434",
    ("MeshRenderArgs", "colors"): "mesh_render.hip:435",
    ("NoiseProjectArgs", "vert_noise"): "mesh_render.hip:522",
    ("NoiseProjectArgs", "prev"): "mesh_render.hip:533",
    # the renderer: points, view directions, cameras and the narrow upstream gradients; styles, tex (alpha, beta), d_feat and d_feat_map
    # are read 16 bytes at a time and guarded (siren.hip:1013, :1029, siren_bwd.hip:1142, :1230): the wrappers realign those
    ("e3dge_siren_points_fwd", 2): "siren16.h:481 (siren.hip:206 the f32 kernel)",
    ("e3dge_siren_points_fwd", 3): "siren16.h:482 (siren.hip:207)",
    **{("RenderArgs", f): "siren16.h:359" if f == "c2w" else "siren16.h:360" for f in ("c2w", "focal", "near", "far")},
    ("RenderBwdArgs", "near"): "siren_bwd.hip:892", ("RenderBwdArgs", "far"): "siren_bwd.hip:892",
    ("RenderBwdArgs", "d_rgb_map"): "siren_bwd.hip:896", ("RenderBwdArgs", "d_xyz_map"): "siren_bwd.hip:897",
    ("RenderBwdArgs", "d_depth_map"): "siren_bwd.hip:898", ("RenderBwdArgs", "d_weights"): "siren_bwd.hip:910",
    ("RenderBwdArgs", "d_sdf"): "siren_bwd.hip:990",
    ("SirenBwdArgs", "d_sdf"): "siren16_bwd.h:250 (siren_bwd.hip:222)", ("SirenBwdArgs", "d_rgb"): "siren16_bwd.h:253 (siren_bwd.hip:224)",
    ("e3dge_siren_tangent", 3): "siren_bwd.hip:694 v one float at a time", ("e3dge_siren_tangent_tr", 3): "siren_bwd.hip:694",
    **{(e, 1): "resblock.hip:319 F4u is packed, aligned(4): rows of 301 floats (resblock.hip:211)" for e in ("e3dge_tex_modulations_fwd", "e3dge_tex_film_fwd")},
    ("e3dge_tex_modulations_bwd", 1): "resblock_bwd.h:200 F4u",
    # the decoder: features, d_img and the noise images go through e3dge_amax (16-byte loads, modconv.hip:424, guarded :611) and are realigned
    ("e3dge_decoder_styles", 4): "modconv.hip:464 x[k]",
    ("Dec2Plan", "latent"): "modconv.hip:464 (the forward plan launches the same style kernel)",
    ("ModconvArgs", "noise"): "modconv.hip:298",
    ("e3dge_torgb", 5): "stream_ops.hip:517 sp[iy * w + ix]",
}
# tensors that may be strided: (entry, index) -> index of the pitch argument, (struct, field) -> pitch field.  Unit last stride always.
# ROWS16: a workspace of volume_renderer.saved_state_buffer, the (B, N, L, W) view of a dense (B, ceil16(N), L, W) block -- the kernels
# address whole 16-row slabs of it (siren_common.h) and take no pitch: the gate checks the strides against that padding instead.
ROWS16 = "rows padded to a multiple of 16"
TAKES_STRIDES = {
    ("e3dge_amax_rows", 1): 4,
    ("Wgrad", "a"): "lda",
    ("Wgrad", "b"): "ldb",
    ("Wgrad", "c"): "ldc",
    **{("WsLinear", f): "ld_" + f for f in ("x", "m", "r1", "r2", "y", "xmul")},          # column blocks of the 301- / 513-wide row buffers
    **{k: ROWS16 for k in [("e3dge_siren_points_fwd", 9), ("e3dge_siren_sdf_grad", 2), ("e3dge_siren_sdf_grad", 7), ("e3dge_siren_tangent", 2),
                           ("e3dge_siren_tangent", 7), ("e3dge_siren_tangent_tr", 2), ("e3dge_siren_tangent_tr", 4), ("e3dge_siren_tangent_tr", 8),
                           ("RenderArgs", "save_args"), ("SirenWgradArgs", "args"), ("SirenWgradArgs", "d_lin")]
       + [(st, f) for st in ("SirenBwdArgs", "RenderBwdArgs") for f in ("args", "tang", "rsave", "d_lin")]},
}
# (row, input, kind) that the module answers with torch, on purpose, and the reason.
FALLS_BACK = {("avgpool", "x", k): "AvgPool2d takes F.adaptive_avg_pool2d for strided inputs (losses.AvgPool2d.factor)"
              for k in ("pitch", "channels_last", "wide", "expanded")}
# outputs that are views of an input by the reference's own definition (volume_renderer.py:788 rays_o = c2w[..., :3, -1].expand(...); near and
# far are handed back expanded): compared like any other output, exempt from the aliasing check
PASS_THROUGH = {"rays_o": "poses", "near": "near", "far": "far"}
# outputs that cannot be bit-compared, with the standing bound of the module's own test (fraction of the maximum)
ATOMIC_OUTPUTS = {("local_query_bwd", "d_fmap"): 2e-5, ("local_features_training", "d_ref"): 2e-5, ("local_features_training", "d_que"): 2e-5}


def _bits_equal(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous(), b.contiguous()
    if a.is_floating_point():
        as_int = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        a, b = a.view(as_int), b.view(as_int)
    return torch.equal(a, b)


# --------------------------------------------------------------------------------------------------------------------------------- gate
class Gate:
    def __init__(self):
        self.names = []
        self.pending = {}                         # id(struct) -> [(field, pitch field, stride)]

    def tensor(self, where, key, t, pitch_of=None):
        spec = TAKES_STRIDES.get(key)
        if t.is_contiguous() and spec is not None and spec is not ROWS16 and t.dim() == 2 and t.shape[0] > 1:
            pitch_of(spec, t.stride(0))                      # (a dense buffer handed over with the wrong pitch is as wrong as a strided one)
        if not t.is_contiguous():
            assert spec is not None, f"{where}: a non-contiguous tensor (shape {tuple(t.shape)}, strides {t.stride()}) and {key} is not in TAKES_STRIDES"
            if spec is ROWS16:
                B, N, L, W = t.shape
                assert t.stride() == ((N + 15) // 16 * 16 * L * W, L * W, W, 1), f"{where}: not a saved-state buffer: {tuple(t.shape)}, {t.stride()}"
                return self.aligned(where, key, t)
            assert t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1), f"{where}: {key} takes rows of unit column stride, got {t.stride()}"
            if t.shape[0] > 1:
                pitch_of(spec, t.stride(0))
        self.aligned(where, key, t)

    @staticmethod
    def aligned(where, key, t):
        if t.numel() and t.data_ptr() % 16:
            assert key in FOUR_BYTE_OK, f"{where}: pointer is {t.data_ptr() % 16} mod 16 and {key} is not in FOUR_BYTE_OK"
            assert t.data_ptr() % t.element_size() == 0, where

    def launch(self, name, args):
        self.names.append(name)
        for i, a in enumerate(args):
            if hasattr(a, "data_ptr") and a.__class__ is not int:
                def pitch_of(spec, stride, i=i):
                    assert args[spec] == stride, f"{name}: argument {i} has row stride {stride} but pitch argument {spec} is {args[spec]}"
                self.tensor(f"{name} argument {i}", (name, i), a, pitch_of)
            elif isinstance(a, _lib._Args):
                for field, pitch, stride in self.pending.pop(id(a), ()):
                    assert getattr(a, pitch) == stride, f"{name}: {type(a).__name__}.{field} has row stride {stride} but .{pitch} is {getattr(a, pitch)}"

    def field(self, struct, field, t):
        root = struct
        while root._b_base_ is not None:
            root = root._b_base_
        key = (type(struct).__name__, field)

        def pitch_of(spec, stride):
            self.pending.setdefault(id(root), []).append((field, spec, stride))
        self.tensor(f"{key[0]}.{field}", key, t, pitch_of)


RECORDED = set()             # every entry name the gate saw in this module, for the coverage test


@pytest.fixture(autouse=True)
def gate(monkeypatch):
    g = Gate()
    real_launch, real_query, real_init, real_set = _lib.launch, _lib.query, _lib._Args.__init__, _lib._Args.__setattr__
    is_tensor = lambda v: v is not None and v.__class__ not in (int, float) and hasattr(v, "data_ptr")

    def launch(name, *args):
        g.launch(name, args)
        return real_launch(name, *args)

    def query(name, *args, **kw):
        g.names.append(name)
        return real_query(name, *args, **kw)

    def init(self, *values, **fields):
        if values:
            fields = dict(zip((f[0] for f in self._fields_), values), **fields)
        for k, v in fields.items():
            if is_tensor(v):
                g.field(self, k, v)
        real_init(self, **fields)

    def setattr_(self, k, v):
        if is_tensor(v):
            g.field(self, k, v)
        real_set(self, k, v)

    monkeypatch.setattr(_lib, "launch", launch)
    monkeypatch.setattr(_lib, "query", query)
    monkeypatch.setattr(_lib._Args, "__init__", init)
    monkeypatch.setattr(_lib._Args, "__setattr__", setattr_)
    yield g
    RECORDED.update(g.names)


# --------------------------------------------------------------------------------------------------------------------------------- rows
class Row:
    """name; inputs() -> {name: CPU tensor} (cheap: it runs at collection); state() -> whatever run needs on the GPU (built once);
    run(state, {name: GPU tensor}) -> {name: tensor}; native: entries every run must launch; upstream: inputs that are upstream
    gradients; extra: {input: more kinds}; fixed: inputs that are not varied."""

    def __init__(self, name, inputs, run, native, state=lambda: None, upstream=(), extra=None, fixed=()):
        self.name, self.run, self.native, self.upstream, self.extra, self.fixed = name, run, set(native), set(upstream), extra or {}, set(fixed)
        self.inputs, self.state = functools.lru_cache(maxsize=None)(inputs), functools.lru_cache(maxsize=None)(state)

    def kinds(self, k):
        x = self.inputs()[k]
        if k in self.fixed:
            return []
        own = [q for q in lv.kinds_for(x) if k not in self.upstream or q in UPSTREAM_KINDS]
        return own + [q for q in self.extra.get(k, ()) if lv.applies(x, q)]


def _rand(seed, *shape, scale=1.0):
    return torch.from_numpy((scale * np.random.RandomState(seed).standard_normal(shape)).astype(np.float32))


def _leaf(t):
    return t.detach().requires_grad_(True)


# ---- op.fused_leaky_relu, op.upfirdn2d -----------------------------------------------------------------------------------------------
def _flrelu_inputs(shape):
    return lambda: dict(x=_rand(1, *shape), bias=_rand(2, shape[1]), gy=_rand(3, *shape))


def _flrelu_run(_, t):
    from e3dge_amd.op import fused_leaky_relu
    x, b = _leaf(t["x"]), _leaf(t["bias"])
    y = fused_leaky_relu(x, b)
    gx, gb = torch.autograd.grad(y, [x, b], t["gy"])
    return dict(y=y.detach(), gx=gx, gb=gb)


def _flrelu_module_run(m, t):
    x = _leaf(t["x"])
    y = m(x)
    gx, gb = torch.autograd.grad(y, [x, m.bias], t["gy"])
    return dict(y=y.detach(), gx=gx, gb=gb)


def _flrelu_module_state():
    from e3dge_amd.op import FusedLeakyReLU
    m = FusedLeakyReLU(5)
    with torch.no_grad():
        m.bias.copy_(_rand(2, 5))
    return m.to(DEV)


def _upfirdn_inputs(up, down, pad):
    def inputs():
        from e3dge_amd.op import upfirdn2d
        x, k = _rand(4, 2, 3, 9, 11), _rand(5, 4, 4)
        return dict(x=x, kernel=k, gy=_rand(6, *upfirdn2d(x, k, up=up, down=down, pad=pad).shape))        # (the CPU branch: the shape)
    return inputs


def _upfirdn_run(up, down, pad):
    def run(_, t):
        from e3dge_amd.op import upfirdn2d
        x = _leaf(t["x"])
        y = upfirdn2d(x, t["kernel"], up=up, down=down, pad=pad)
        gx, = torch.autograd.grad(y, [x], t["gy"])
        return dict(y=y.detach(), gx=gx)
    return run


# ---- losses ------------------------------------------------------------------------------------------------------------------------
def _pool_run(_, t):
    x = _leaf(t["x"])
    y = losses.AvgPool2d((8, 8))(x)
    gx, = torch.autograd.grad(y, [x], t["gy"])
    return dict(y=y.detach(), gx=gx)


def _pool_fallback_check(t, out):
    """A listed fallback: torch on the same values, under the module's standing bound (tests/test_gpu_losses.check)."""
    from test_gpu_losses import check
    x, gy = t["x"].detach(), t["gy"].detach()
    check("layout_pool_fwd", out["y"], F.adaptive_avg_pool2d(x.double(), (8, 8)), F.adaptive_avg_pool2d(x.contiguous(), (8, 8)))
    g64 = (gy.double() / 16).repeat_interleave(4, -2).repeat_interleave(4, -1)
    check("layout_pool_bwd", out["gx"], g64, g64.float())


def _shape_inputs():
    from conftest import load_golden
    from test_losses_host import shape_inputs
    pred, gt = shape_inputs(load_golden("losses_shape"))
    return dict(**{"pred_" + k: v.detach() for k, v in pred.items()}, **{"gt_" + k: v for k, v in gt.items()})


def _shape_run(_, t):
    from test_losses_host import ALL_ON, LAMBDAS_A, PRED_KEYS, opt_of
    pred = {k: _leaf(t["pred_" + k]) for k in PRED_KEYS}
    gt = {k[3:]: v for k, v in t.items() if k.startswith("gt_")}
    lc = losses.LossClass(DEV, opt_of(**LAMBDAS_A), lpips=object(), id_loss=object())
    total, d = lc.calc_shape_rec_loss(pred, gt, DEV, **ALL_ON)
    grads = torch.autograd.grad(total * 0.75, [pred[k] for k in PRED_KEYS], allow_unused=True)
    out = dict(total=total.detach(), **{"term_" + k: v.detach() for k, v in d.items() if torch.is_tensor(v)})
    out.update({"grad_" + k: g for k, g in zip(PRED_KEYS, grads) if g is not None})
    return out


def _rec2d_inputs():
    from test_gpu_losses import pair
    pred, gt = pair(64)
    return dict(pred=pred, gt=gt)


def _rec2d_run(lc, t):
    p = _leaf(t["pred"])
    loss, rec, lp, lid = lc.calc_2d_rec_loss(p, t["gt"], t["gt"], None)[:4]
    grad, = torch.autograd.grad(loss, p)
    return dict(loss=loss.detach(), rec=rec.detach(), lp=lp.detach(), lid=lid.detach(), grad=grad)


def _rec2d_state():
    from test_gpu_losses import loss_class
    return loss_class(1.0, 0.8, 0.1)


def _metrics_inputs():
    from test_gpu_lpips import make_pair
    pred, gt = make_pair((2, 3, 50, 70), seed=7)
    return dict(pred=pred, gt=gt)


def _metrics_run(_, t):
    from e3dge_amd.sharded_eval import image_metrics
    with torch.no_grad():
        return dict(row=image_metrics(t["pred"], t["gt"]))


# ---- LPIPS, identity, discriminator ------------------------------------------------------------------------------------------------------
def _lpips_inputs():
    from test_gpu_lpips import make_pair
    x, y = make_pair((2, 3, 31, 31), seed=31)                        # (batch 2: `expanded` applies to x, y and the upstream gradient)
    return dict(x=x, y=y, upstream=_rand(8, 2))


def _lpips_state():
    from test_gpu_losses import lpips_gpu
    return lpips_gpu()


def _lpips_run(m, t):
    with torch.no_grad():
        r = m.run(t["x"], t["y"], per_layer=True, taps=True)
    out = dict(per_image=r["per_image"], mean=r["mean"], per_layer=r["per_layer"], **{f"tap{i}": v for i, v in enumerate(r["taps"])})
    gx, gy, _ = m.run_backward(t["x"], t["y"], t["upstream"], want_x=True, want_y=True)
    return dict(out, gx=gx, gy=gy)


def _lpips_diff_run(m, t):
    x = _leaf(t["x"])
    r = m.run(x, t["y"])
    gx, = torch.autograd.grad(r["per_image"], [x], t["upstream"])
    return dict(per_image=r["per_image"].detach(), gx=gx)


def _id_inputs():
    from test_idloss_host import make_pair
    y_hat, y = make_pair((1, 3, 256, 256), seed=3)
    return dict(y_hat=y_hat, y=y, upstream=_rand(9, 1))


def _id_state():
    from test_gpu_losses import idloss_gpu
    return idloss_gpu()


def _id_run(m, t):
    with torch.no_grad():
        r = m.run(t["y_hat"], t["y"])
    grad = m.run_backward(t["y_hat"], t["y"], t["upstream"])[0]
    yh = _leaf(t["y_hat"])
    loss = m.run(yh, t["y"])["loss"]
    g2, = torch.autograd.grad(loss, [yh])
    return dict(embeddings=r["embeddings"], dots=r["dots"], loss=r["loss"], grad=grad, loss_diff=loss.detach(), grad_diff=g2)


def _disc_case():
    from test_discriminator_host import CASES
    return CASES[0]


def _disc_inputs():
    from test_discriminator_host import golden_images
    _, _, b, size = _disc_case()
    return dict(x=golden_images(b, size), g=_rand(10, b, 1))


def _disc_state():
    from test_gpu_discriminator import module_gpu
    init, cm, _, _ = _disc_case()
    return module_gpu(init, cm)


def _disc_run(m, t):
    r = m.run(t["x"], taps=True)
    b = m.run_backward(t["x"], t["g"])
    x = _leaf(t["x"])
    gx, = torch.autograd.grad(m(x), [x], t["g"])
    return dict(logits=r["logits"], grad=b["grad"], grad_autograd=gx, **{f"tap{k}": v for k, v in r["taps"].items()})


# ---- encoder, aligner, image filter -------------------------------------------------------------------------------------------------------
def _enc_inputs():
    import test_encoder_host as host
    _, n, size = host.CASES["s48"]
    return dict(x=host.encoder_input(n, size, sorted(host.CASES).index("s48") + 1))


def _enc_state():
    import test_encoder_host as host
    from test_gpu_encoder import module_gpu
    return module_gpu(**host.CASES["s48"][0])


def _enc_run(m, t):
    import test_encoder_host as host
    with torch.no_grad():
        return host.as_tensors(m.run(t["x"], return_featmap=True, pool=False))


def _aln_inputs():
    from test_aligner_host import aligner_input
    x = aligner_input(1, 5)
    return dict(x=x, res_gt=x[:, :3].contiguous(), thumb=x[:, 3:, ::4, ::4].contiguous())


def _aln_state():
    from test_gpu_aligner import module_gpu
    return module_gpu()


def _aln_forward_run(m, t):
    with torch.no_grad():
        return dict(out=m(t["x"]))


def _aln_align_run(m, t):
    with torch.no_grad():
        return dict(out=m.align(t["res_gt"], t["thumb"]))


def _aln_slice_run(m, t):
    """The call site's own view: res_gt is x[:, :3] of the 6-channel tensor, whatever layout that tensor has."""
    with torch.no_grad():
        return dict(out=m.align(t["x"][:, :3], t["thumb"]))


def _hgf64_inputs():
    from test_hgfilter_host import case_inputs
    return dict(x=case_inputs("default")[0])


def _hgf64_state():
    from test_gpu_hgfilter import module_gpu
    return module_gpu("default")


def _hgf64_run(m, t):
    """HGFilter.forward on its own 64-channel input (no front nets)."""
    with torch.no_grad():
        outs, tmpx, normx = m.image_filter(t["x"])
    return dict(tmpx=tmpx, normx=normx, **{f"out{i}": o for i, o in enumerate(outs)})


def _hgf_inputs():
    from test_hgfilter_host import case_inputs
    image, depth = case_inputs("filter")
    n, _, h, w = image.shape
    return dict(image=image, depth=depth, g_out=_rand(11, n, 256, h // 4, w // 4, scale=0.1), g_normx=_rand(12, n, 128, h // 4, w // 4, scale=0.1))


def _hgf_state():
    from test_gpu_hgfilter import module_gpu
    from test_hgfilter_host import CASES
    from e3dge_amd.hg_filter import ResidualImageFilter
    plain = module_gpu("filter")
    diff = ResidualImageFilter(syn.pifu_opt(**CASES["filter"][0]), differentiable=True)
    diff.load_state_dict(plain.state_dict())
    return plain, diff.to(DEV).eval()


def _hgf_run(state, t):
    plain, _ = state
    with torch.no_grad():
        outs, tmpx, normx = plain.filter_maps(t["image"], t["depth"])
    return dict(tmpx=tmpx, normx=normx, **{f"out{i}": o for i, o in enumerate(outs)})


def _hgf_diff_run(state, t):
    _, diff = state
    image, depth = _leaf(t["image"]), _leaf(t["depth"])
    params = [p for p in diff.parameters() if p.requires_grad]
    outs, tmpx, normx = diff.filter_maps(image, depth)
    grads = torch.autograd.grad([outs[-1], normx], [image, depth] + params, [t["g_out"], t["g_normx"]], allow_unused=True)
    out = dict(out=outs[-1].detach(), normx=normx.detach(), g_image=grads[0], g_depth=grads[1])
    out.update({f"g_param{i}": g for i, g in enumerate(grads[2:]) if g is not None})
    return out


# ---- mesh utilities ------------------------------------------------------------------------------------------------------------------
def _sphere():
    from test_mesh_render_host import uv_sphere
    return tuple(torch.from_numpy(a) for a in uv_sphere())


def _depth_mesh_inputs():
    from test_mesh_render_host import height_field
    return dict(xyz=torch.from_numpy(height_field(8)[0]))


def _depth_mesh_run(_, t):
    v, f = mesh_utils.depth_mesh(t["xyz"])
    return dict(verts=v, faces=f)


def _normals_run(_, t):
    return dict(normals=mesh_utils.vertex_normals(t["verts"], t["faces"]))


def _render_run(_, t):
    from test_gpu_mesh_render import renderer_for
    image, zbuf, pix = renderer_for("sphere", 1, 64).rasterize(t["verts"], t["faces"], t["normals"])
    return dict(image=image, zbuf=zbuf, pix=pix)


def _subdivide_run(_, t):
    v, f = mesh_utils.subdivide(t["verts"], t["faces"], levels=1)
    return dict(verts=v, faces=f)


def _noise_inputs():
    import test_noise_projection_host as host
    v, f = host.scene_mesh(0)
    return dict(verts=torch.from_numpy(v), faces=torch.from_numpy(f), noise=torch.from_numpy(host.scene_noise(len(v))[0]), prev=_rand(5, 1, 64, 64))


def _noise_run(_, t):
    import test_noise_projection_host as host
    maps, valid = mesh_utils.project_vertex_noise(t["verts"], t["faces"], t["noise"], host.scene_camera(), 64, prev=t["prev"])
    return dict(maps=maps, valid=valid)


# ---- point queries -----------------------------------------------------------------------------------------------------------------
def _points(seed, scale):
    pts = (torch.rand(2, 125, 3, generator=torch.Generator().manual_seed(seed)) - 0.5) * scale
    return pts


def _lq_inputs():
    pts = _points(5, 0.5)
    pts[:, :125 // 8] *= 6.0                                         # some project outside the image plane (tests/test_local_query.py)
    calib = torch.tensor([[[2.2, 0.1, 0.0, 0.03], [0.05, 2.1, 0.1, -0.02], [0.0, 0.1, 1.0, 2.0]],
                          [[1.9, -0.2, 0.1, 0.0], [0.1, 2.3, 0.0, 0.05], [0.1, 0.0, 1.0, 1.7]]])
    return dict(pts=pts, calibs=calib, fmap=_rand(13, 2, 8, 5, 7), g_out=_rand(14, 2, 125, 8))


def _lq_run(_, t):
    from e3dge_amd.local_query import pos_encoding, query_feature_map
    with torch.no_grad():
        feats, mask, proj = query_feature_map(t["pts"], t["calibs"], t["fmap"], want_proj=True)
        enc = pos_encoding(t["pts"])
    return dict(feats=feats, mask=mask, proj=proj, enc=enc)


def _lq_bwd_run(_, t):
    from e3dge_amd.local_query import query_feature_map
    p, fm = _leaf(t["pts"]), _leaf(t["fmap"])
    feats, mask, _ = query_feature_map(p, t["calibs"], fm)
    d_p, d_fm = torch.autograd.grad(feats, [p, fm], t["g_out"])
    return dict(feats=feats.detach(), mask=mask, d_pts=d_p, d_fmap=d_fm)


@functools.lru_cache(maxsize=None)
def _renderer(res, S, mode=None):
    from test_gpu_renderer import make_renderer
    return make_renderer(_renderer_sd(), res, S, mfma_mode=mode)


@functools.lru_cache(maxsize=None)
def _renderer_sd():
    from conftest import full_state_dict
    return full_state_dict()[1]            # (the renderer's weights do not depend on the resolution; the generator's decoder wants a power of two)


def _qp_inputs():
    return dict(pts=_points(21, 0.2), viewdirs=F.normalize(_points(22, 1.0), dim=-1), styles=syn.synthetic_inputs(2, seed=1)[0],
                g_sdf=_rand(15, 2, 125), g_raw=_rand(16, 2, 125, 260, scale=0.1), g_eik=_rand(17, 2, 125, 3, scale=0.1))


def _qp_run(r, t):
    with torch.no_grad():
        sdf, raw = r.siren.query_points(t["pts"], t["viewdirs"], t["styles"], r.box_scale)
        sdf2, _, eik = r.siren.query_points(t["pts"], t["viewdirs"], t["styles"], r.box_scale, want_eikonal=True)
    return dict(sdf=sdf, raw=raw, sdf_eik=sdf2, eik=eik)


def _qp_bwd_run(r, t):
    st, p = _leaf(t["styles"]), _leaf(t["pts"])
    sdf, raw, eik = r.siren.query_points(p, t["viewdirs"], st, r.box_scale, want_eikonal=True)
    d_st, d_p = torch.autograd.grad([sdf, raw, eik], [st, p], [t["g_sdf"], t["g_raw"], t["g_eik"]])
    return dict(sdf=sdf.detach(), raw=raw.detach(), eik=eik.detach(), d_styles=d_st, d_pts=d_p)


def _render_inputs(wide_styles):
    def inputs():
        poses, focal, near, far, _ = generate_camera_params(5, "cpu", locations=torch.tensor([[0.1, -0.05], [-0.2, 0.1]]))
        wr = syn.synthetic_inputs(2, seed=1)[0]
        return dict(poses=poses, focal=focal, near=near, far=far, styles=wr if wide_styles else wr[:, 0].contiguous(),
                    g_rgb=_rand(18, 2, 3, 5, 5), g_feat=_rand(19, 2, 256, 5, 5, scale=0.1), g_eik=_rand(20, 2, 5, 5, 17, 3, scale=0.1))
    return inputs


def _render_fwd_run(r, t):
    with torch.no_grad():
        out = r(t["poses"], t["focal"], t["near"], t["far"], styles=t["styles"])
    return {k: v for k, v in out.items() if torch.is_tensor(v)}


def _render_bwd_run(r, t):
    st = _leaf(t["styles"])
    o = r(t["poses"], t["focal"], t["near"], t["far"], styles=st, return_eikonal=True)
    assert o["eikonal_term"].shape == t["g_eik"].shape, tuple(o["eikonal_term"].shape)
    d_st, = torch.autograd.grad([o["gen_thumb_imgs"], o["features"], o["eikonal_term"]], [st], [t["g_rgb"], t["g_feat"], t["g_eik"]])
    return dict(rgb=o["gen_thumb_imgs"].detach(), features=o["features"].detach(), eik=o["eikonal_term"].detach(), d_styles=d_st)


def _hitprob_inputs():
    from conftest import load_golden
    return dict(points=torch.from_numpy(load_golden("hitprob_8x18")["points"]))


def _hitprob_state():
    from conftest import load_golden
    g = load_golden("hitprob_8x18")
    r = _renderer(8, 18)
    wr, _ = syn.synthetic_inputs(2, seed=int(g["styles_seed"]), device=DEV)
    T = lambda k: torch.from_numpy(g[k]).to(DEV)
    with torch.no_grad():
        ref_out = r(T("ref_poses"), T("ref_focal"), T("ref_near"), T("ref_far"), styles=wr)
    return r, dict(global_render_out=ref_out, cam_settings=dict(poses=T("ref_poses"), extrinsics=T("ref_extrinsics")), pred_latents=[wr])


def _hitprob_run(state, t):
    r, info = state
    with torch.no_grad():
        return {rt: r.query_hitting_probability_fixed_interval(t["points"], info, return_type=rt) for rt in ("weights", "visibility")}


# ---- texture head ---------------------------------------------------------------------------------------------------------------------
def _tex_inputs():
    rs = np.random.RandomState(301 + 200)
    feats = torch.from_numpy((rs.standard_normal((200, 301)) * (0.1 + 2 * rs.uniform(size=(1, 301)))).astype(np.float32))
    return dict(feats=feats, g_alpha=_rand(23, 200, 256, scale=0.1), g_beta=_rand(24, 200, 256, scale=0.1))


def _tex_state():
    from test_gpu_texhead import make_head
    return make_head(301)[0]


def _tex_run(h, t):
    with torch.no_grad():
        a, b = h.tex_modulations(t["feats"])
    f = _leaf(t["feats"])
    params = list(h.parameters())
    a2, b2 = h.tex_modulations(f)
    grads = torch.autograd.grad([a2, b2], [f] + params, [t["g_alpha"], t["g_beta"]])
    return dict(alpha=a, beta=b, alpha_grad_mode=a2.detach(), d_feats=grads[0], **{f"d_param{i}": g for i, g in enumerate(grads[1:])})


# ---- decoder --------------------------------------------------------------------------------------------------------------------------
DEC_CASE = "c"               # the smallest input _dec2_ok admits (tests/test_gpu_decoder_bwd_shapes.CASES)


def _dec_inputs():
    from test_gpu_decoder_bwd_shapes import CASES, _latents
    c = CASES[DEC_CASE]
    n_up = int(np.log2(c["size"] // c["res"]))
    feats, noises, gy = syn.decoder_grad_inputs(c["B"], c["feat"] << n_up, c["feat"], seed=100 + ord(DEC_CASE))
    if c["shared"]:
        noises = [n[:1].contiguous() for n in noises]
    n_latent = 2 * n_up + 2
    return dict(feats=feats, wd=_latents(c["B"], n_latent, c["unit"], 100 + ord(DEC_CASE)), gy=gy, **{f"noise{i}": n for i, n in enumerate(noises)})


def _dec_state():
    from conftest import full_state_dict
    from test_gpu_decoder_bwd_shapes import CASES
    c = CASES[DEC_CASE]
    g, _ = full_state_dict(size=c["size"], cm=1, res=c["res"])
    g.eval().requires_grad_(False)
    return g.decoder.to(DEV)


def _dec_noises(t):
    return [t[f"noise{i}"] for i in range(sum(k.startswith("noise") for k in t))]


def _dec_run(dec, t):
    assert t["wd"].shape[1] == dec.n_latent, (tuple(t["wd"].shape), dec.n_latent)
    with torch.no_grad():
        img, _ = dec(t["feats"], [t["wd"]], input_is_latent=True, noise=_dec_noises(t))
    f, lat = _leaf(t["feats"]), _leaf(t["wd"])
    img2, _ = dec(f, [lat], input_is_latent=True, noise=_dec_noises(t))
    assert "PackedDecoderFn" in type(img2.grad_fn).__name__, type(img2.grad_fn).__name__
    d_f, d_l = torch.autograd.grad(img2, [f, lat], t["gy"])
    return dict(img=img, img_grad_mode=img2.detach(), d_features=d_f, d_latent=d_l)


# ---- the decoder's layers on their own (the path a decoder takes when the packed pipeline does not cover its shape) ---------------------------
def _layer_inputs(ci, H, W, up):
    def inputs():
        rs = np.random.RandomState(3)
        r = lambda *shape: torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
        OH, OW = (2 * H, 2 * W) if up else (H, W)
        return dict(x=r(2, ci, H, W), style=r(2, 512), noise=r(2, 1, OH, OW))
    return inputs


def _layer_state(ci, co, up):
    def state():
        from e3dge_amd.stylesdf_model import StyledConv
        from test_gpu_modconv import make_layer
        return make_layer(StyledConv, ci, co, up, seed=7)[0]
    return state


def _layer_run(m, t):
    with torch.no_grad():
        return dict(y=m(t["x"], t["style"], noise=t["noise"]))


def _torgb_inputs():
    rs = np.random.RandomState(4)
    r = lambda *shape: torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
    return dict(x=r(2, 16, 4, 4), style=r(2, 512), skip=r(2, 3, 2, 2))          # (the smallest shape fused_ok admits, tests/test_gpu_modconv.py)


def _torgb_state():
    from e3dge_amd.stylesdf_model import ToRGB
    m = ToRGB(16, 512, upsample=True)
    m.load_state_dict({k: syn.synthetic_tensor("decoder.to_rgbs.0." + k, v.shape, 16) for k, v in m.state_dict().items() if not k.endswith("kernel")},
                      strict=False)
    return m.to(DEV).eval()


def _torgb_run(m, t):
    with torch.no_grad():
        assert m.fused_ok(t["x"], t["skip"])
        return dict(y=m(t["x"], t["style"], skip=t["skip"]))


# ---- the local branch: gathers + Fuse_sft_MLP, inference and training form ------------------------------------------------------------------
def _lf_inputs():
    g = torch.Generator().manual_seed(3)
    calib = torch.tensor([[[2.0, 0.0, 0.0, 0.0], [0.0, 2.0, 0.0, 0.0], [0.0, 0.0, 1.0, 2.0]]])
    return dict(ref=_rand(30, 1, 256, 16, 16), que=_rand(31, 1, 256, 16, 16), points=torch.rand(1, 8, 8, 6, 3, generator=g) - 0.5,
                xyz=torch.rand(1, 3, 8, 8, generator=g) - 0.5, ref_calibs=calib, que_calibs=calib.clone(), g=_rand(32, 1, 8, 8, 6, 301, scale=0.1))


def _lf_state():
    from e3dge_amd.local_query import Fuse_sft_MLP
    fuse = Fuse_sft_MLP(257, 256)
    with torch.no_grad():
        for i, p in enumerate(fuse.parameters()):
            p.copy_(_rand(100 + i, *p.shape, scale=0.05))
    return fuse.to(DEV)


def _lf_batch(fuse, t, ref, que):
    return dict(feature_maps=dict(ref=ref, que=que), ref_calibs=t["ref_calibs"], que_calibs=t["que_calibs"], points=t["points"], xyz=t["xyz"],
                fuse_sft_block=fuse)


def _lf_run(fuse, t):
    from e3dge_amd.local_query import local_features_from_maps
    with torch.no_grad():
        feats, mask = local_features_from_maps(_lf_batch(fuse, t, t["ref"], t["que"]))
    return dict(feats=feats, mask=mask)


def _lf_train_run(fuse, t):
    from e3dge_amd.local_query import local_features_from_maps
    ref, que = _leaf(t["ref"]), _leaf(t["que"])
    params = list(fuse.parameters())
    feats, _ = local_features_from_maps(_lf_batch(fuse, t, ref, que))
    grads = torch.autograd.grad(feats, [ref, que] + params, t["g"], allow_unused=True)
    out = dict(feats=feats.detach(), d_ref=grads[0], d_que=grads[1])
    out.update({f"d_param{i}": g for i, g in enumerate(grads[2:]) if g is not None})
    return out


def _fuse_inputs():
    return dict(enc_in=_rand(40, 200, 513), g=_rand(41, 200, 256, scale=0.1))


def _fuse_run(fuse, t):
    with torch.no_grad():
        y = fuse.fuse(t["enc_in"], t["enc_in"][..., 257:])
    x = _leaf(t["enc_in"])
    params = list(fuse.parameters())
    y2 = fuse.fuse(x, x[..., 257:])
    assert "FuseFn" in type(y2.grad_fn).__name__, type(y2.grad_fn).__name__
    grads = torch.autograd.grad(y2, [x] + params, t["g"])
    return dict(y=y, y_grad_mode=y2.detach(), d_enc_in=grads[0], **{f"d_param{i}": g for i, g in enumerate(grads[1:])})


def _nba_inputs():
    return dict(x=_rand(42, 2, 5, 6, 4), noise=_rand(43, 2, 1, 6, 4), weight=_rand(44, 1), bias=_rand(45, 5), gy=_rand(46, 2, 5, 6, 4))


def _nba_run(_, t):
    from e3dge_amd.op.fused_act import noise_bias_act
    x, w, b = _leaf(t["x"]), _leaf(t["weight"]), _leaf(t["bias"])
    y = noise_bias_act(x, t["noise"], w, b)
    gx, gw, gb = torch.autograd.grad(y, [x, w, b], t["gy"])
    return dict(y=y.detach(), gx=gx, gw=gw, gb=gb)


# ---- the renderer's second pass and its parameter gradients ---------------------------------------------------------------------------------
def _second_pass_inputs():
    d = _render_inputs(True)()
    return dict({k: d[k] for k in ("poses", "focal", "near", "far", "styles")}, feats=syn.synthetic_local_feats(2, 5, 17))


def _second_pass_state():
    from test_gpu_texhead import _local_renderer
    return _local_renderer(5, 17)


def _second_pass_run(r, t):
    with torch.no_grad():                # (the first pass leaves the layer-7 record that the head + FiLM launch of the second pass reads)
        first = r(t["poses"], t["focal"], t["near"], t["far"], styles=t["styles"])
        out = r(t["poses"], t["focal"], t["near"], t["far"], styles=t["styles"], local_data_batch={"feats": t["feats"]})
    return dict({k: v for k, v in out.items() if torch.is_tensor(v)}, first_features=first["features"])


def _params_state():
    from test_gpu_renderer_params import trainable
    return trainable(_renderer_sd(), 5, 17)


def _params_run(r, t):
    st = _leaf(t["styles"])
    params = [p for p in r.parameters() if p.requires_grad]
    o = r(t["poses"], t["focal"], t["near"], t["far"], styles=st)
    grads = torch.autograd.grad([o["gen_thumb_imgs"], o["features"]], [st] + params, [t["g_rgb"], t["g_feat"]], allow_unused=True)
    out = dict(rgb=o["gen_thumb_imgs"].detach(), d_styles=grads[0])
    out.update({f"d_param{i}": g for i, g in enumerate(grads[1:]) if g is not None})
    return out


def _dec_planar_run(dec, t):
    """The chain of fused layer kernels over fp32 planes (E3DGE_DECODER=planar): the styles come from e3dge_decoder_styles."""
    import os
    old = os.environ.get("E3DGE_DECODER")
    os.environ["E3DGE_DECODER"] = "planar"
    try:
        with torch.no_grad():
            img, _ = dec(t["feats"], [t["wd"]], input_is_latent=True, noise=_dec_noises(t))
    finally:
        if old is None:
            del os.environ["E3DGE_DECODER"]
        else:
            os.environ["E3DGE_DECODER"] = old
    return dict(img=img)


_SPHERE_INPUTS = lambda: dict(zip(("verts", "faces", "normals"), _sphere()))

ROWS = [
    Row("fused_leaky_relu_rows", _flrelu_inputs((2, 5, 6, 4)), _flrelu_run, {"e3dge_fused_bias_act"}, upstream={"gy"}),
    Row("fused_leaky_relu_elements", _flrelu_inputs((2, 5, 3, 3)), _flrelu_run, {"e3dge_fused_bias_act"}, upstream={"gy"}),
    Row("fused_leaky_relu_module", lambda: dict(x=_rand(1, 2, 5, 6, 4), gy=_rand(3, 2, 5, 6, 4)), _flrelu_module_run, {"e3dge_fused_bias_act"},
        _flrelu_module_state, upstream={"gy"}),
    Row("upfirdn2d_up2", _upfirdn_inputs(2, 1, (2, 1)), _upfirdn_run(2, 1, (2, 1)), {"e3dge_upfirdn2d"}, upstream={"gy"}),
    Row("upfirdn2d_down2", _upfirdn_inputs(1, 2, (1, 1)), _upfirdn_run(1, 2, (1, 1)), {"e3dge_upfirdn2d"}, upstream={"gy"}),
    Row("avgpool", lambda: dict(x=_rand(7, 2, 3, 32, 32), gy=_rand(8, 2, 3, 8, 8)), _pool_run, {"e3dge_avgpool_fwd", "e3dge_avgpool_bwd"}, upstream={"gy"}),
    Row("shape_loss", _shape_inputs, _shape_run, {"e3dge_shape_loss_fwd", "e3dge_shape_loss_bwd"}),
    Row("rec_loss_2d", _rec2d_inputs, _rec2d_run, {"e3dge_image_metrics", "e3dge_image_metric_row", "e3dge_sqerr_bwd", "e3dge_lpips_forward",
                                                    "e3dge_lpips_backward", "e3dge_idnet_embed_save", "e3dge_idnet_backward", "e3dge_id_loss"}, _rec2d_state),
    Row("image_metrics", _metrics_inputs, _metrics_run, {"e3dge_image_metrics", "e3dge_image_metric_row"}),
    Row("lpips", _lpips_inputs, _lpips_run, {"e3dge_lpips_forward", "e3dge_lpips_backward"}, _lpips_state, upstream={"upstream"}),
    Row("lpips_differentiable", _lpips_inputs, _lpips_diff_run, {"e3dge_lpips_forward", "e3dge_lpips_backward"}, _lpips_state, upstream={"upstream"}),
    Row("idloss", _id_inputs, _id_run, {"e3dge_idnet_embed", "e3dge_idnet_embed_save", "e3dge_idnet_backward", "e3dge_id_loss"}, _id_state,
        upstream={"upstream"}),
    Row("discriminator", _disc_inputs, _disc_run, {"e3dge_disc_forward", "e3dge_disc_backward"}, _disc_state, upstream={"g"}),
    Row("encoder", _enc_inputs, _enc_run, {"e3dge_enc_forward"}, _enc_state),
    Row("aligner_forward", _aln_inputs, _aln_forward_run, {"e3dge_aligner_forward"}, _aln_state, fixed={"res_gt", "thumb"}),
    Row("aligner_align", _aln_inputs, _aln_align_run, {"e3dge_aligner_forward"}, _aln_state, fixed={"x"}),
    Row("aligner_align_slice", _aln_inputs, _aln_slice_run, {"e3dge_aligner_forward"}, _aln_state, fixed={"res_gt"}),
    Row("hg_filter", _hgf64_inputs, _hgf64_run, {"e3dge_hgf_forward"}, _hgf64_state),
    Row("image_filter", _hgf_inputs, _hgf_run, {"e3dge_hgf_front", "e3dge_hgf_forward"}, _hgf_state, fixed={"g_out", "g_normx"}),
    Row("image_filter_differentiable", _hgf_inputs, _hgf_diff_run, {"e3dge_hgf_front_saving", "e3dge_hgf_forward_saving", "e3dge_hgf_backward",
                                                                    "e3dge_hgf_front_backward"}, _hgf_state, upstream={"g_out", "g_normx"}),
    Row("depth_mesh", _depth_mesh_inputs, _depth_mesh_run, {"e3dge_depth_mesh"}),
    Row("vertex_normals", lambda: dict(zip(("verts", "faces"), _sphere()[:2])), _normals_run, {"e3dge_vertex_normals"}),
    Row("mesh_render", _SPHERE_INPUTS, _render_run, {"e3dge_mesh_render"}),
    Row("mesh_subdivide", lambda: dict(zip(("verts", "faces"), _sphere()[:2])), _subdivide_run, {"e3dge_mesh_subdivide"}),
    Row("noise_project", _noise_inputs, _noise_run, {"e3dge_noise_project"}),
    Row("local_query", _lq_inputs, _lq_run, {"e3dge_local_query", "e3dge_pos_encoding"}, fixed={"g_out"}),
    Row("local_query_bwd", _lq_inputs, _lq_bwd_run, {"e3dge_local_query", "e3dge_local_query_bwd"}, upstream={"g_out"}),
    Row("query_points", _qp_inputs, _qp_run, {"e3dge_film_params", "e3dge_siren_points_fwd", "e3dge_siren_sdf_grad"}, lambda: _renderer(8, 18),
        extra={"styles": ["expanded1"]}, fixed={"g_sdf", "g_raw", "g_eik"}),
    Row("query_points_bwd", _qp_inputs, _qp_bwd_run, {"e3dge_film_params", "e3dge_siren_points_fwd", "e3dge_siren_bwd"}, lambda: _renderer(8, 18),
        upstream={"g_sdf", "g_raw", "g_eik"}, extra={"styles": ["expanded1"]}),
    Row("render", _render_inputs(True), _render_fwd_run, {"e3dge_film_params", "e3dge_siren_render_fwd"}, lambda: _renderer(5, 17),
        extra={"styles": ["expanded1"]}, fixed={"g_rgb", "g_feat", "g_eik"}),
    Row("render_one_style", _render_inputs(False), _render_fwd_run, {"e3dge_film_params", "e3dge_siren_render_fwd"}, lambda: _renderer(5, 17),
        fixed={"g_rgb", "g_feat", "g_eik"}),
    Row("render_bwd", _render_inputs(True), _render_bwd_run, {"e3dge_film_params", "e3dge_siren_render_fwd", "e3dge_siren_render_bwd"},
        lambda: _renderer(5, 17), upstream={"g_rgb", "g_feat", "g_eik"}, extra={"styles": ["expanded1"]}, fixed={"poses", "focal", "near", "far"}),
    Row("hitprob", _hitprob_inputs, _hitprob_run, {"e3dge_hitprob_points", "e3dge_hitprob_composite"}, _hitprob_state),
    Row("texture_head", _tex_inputs, _tex_run, {"e3dge_tex_modulations_fwd", "e3dge_tex_modulations_bwd"}, _tex_state, upstream={"g_alpha", "g_beta"}),
    Row("decoder", _dec_inputs, _dec_run, {"e3dge_dec2_forward", "e3dge_dec2_backward"}, _dec_state, upstream={"gy"},
        extra={"wd": ["expanded1"]}),
    Row("decoder_planar", _dec_inputs, _dec_planar_run, {"e3dge_decoder_styles", "e3dge_modconv3x3", "e3dge_torgb"}, _dec_state, extra={"wd": ["expanded1"]},
        fixed={"gy"}),
    Row("styled_conv", _layer_inputs(32, 24, 40, False), _layer_run, {"e3dge_modconv3x3", "e3dge_modconv_demod", "e3dge_amax"}, _layer_state(32, 32, False)),
    Row("styled_conv_up", _layer_inputs(64, 24, 40, True), _layer_run, {"e3dge_modconv3x3", "e3dge_modconv_demod", "e3dge_blur_noise_bias_act"},
        _layer_state(64, 32, True)),
    Row("styled_conv_library", _layer_inputs(24, 6, 6, False), _layer_run, {"e3dge_modconv_weights", "e3dge_noise_bias_act"}, _layer_state(24, 40, False)),
    Row("noise_bias_act", _nba_inputs, _nba_run, {"e3dge_noise_bias_act", "e3dge_fused_bias_act"}, upstream={"gy"}),
    Row("fuse_sft_mlp", _fuse_inputs, _fuse_run, {"e3dge_ws_linear", "e3dge_amax", "e3dge_ws_rowdot2"}, _lf_state, upstream={"g"}),
    Row("query_points_bwd_f32", _qp_inputs, _qp_bwd_run, {"e3dge_film_params", "e3dge_siren_points_fwd", "e3dge_siren_bwd", "e3dge_siren_tangent"},
        lambda: _renderer(8, 18, "f32"), upstream={"g_sdf", "g_raw", "g_eik"}, fixed={"viewdirs"}),
    Row("to_rgb", _torgb_inputs, _torgb_run, {"e3dge_torgb"}, _torgb_state),
    Row("local_features", _lf_inputs, _lf_run, {"e3dge_local_query", "e3dge_pos_encoding", "e3dge_ws_linear"}, _lf_state, fixed={"g"}),
    Row("local_features_training", _lf_inputs, _lf_train_run, {"e3dge_local_query", "e3dge_local_query_bwd"}, _lf_state, upstream={"g"}),
    Row("render_second_pass", _second_pass_inputs, _second_pass_run, {"e3dge_siren_render_fwd"}, _second_pass_state, extra={"styles": ["expanded1"]}),
    Row("render_parameter_gradients", _render_inputs(True), _params_run, {"e3dge_siren_render_fwd", "e3dge_siren_render_bwd", "e3dge_siren_wgrad"},
        _params_state, upstream={"g_rgb", "g_feat"}, fixed={"poses", "focal", "near", "far", "g_eik"}),
]
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)

# Entries the table does not reach, each with its reason; the coverage test holds the table and this list to the package's source.
_OWN_VIEW_TESTS = "reached with strided views by its own test"
NOT_REACHED = {
    "e3dge_dec2_unpack": "debug reader of the packed activations and their gradients (Decoder.dec2_unpack, dec2_unpack_grad): tests call it",
    "e3dge_hgf_branch_bytes": "debug: sizes the ReLU-branch record that exists only while a test sets _FilterNode.branches",
    "e3dge_marching_cubes_count": _OWN_VIEW_TESTS + " (tests/test_marching_cubes.py)",
    "e3dge_marching_cubes_emit": _OWN_VIEW_TESTS + " (tests/test_marching_cubes.py)",
    "e3dge_align_volume": _OWN_VIEW_TESTS + " (tests/test_mesh_utils.py)",
}


# ------------------------------------------------------------------------------------------------------------------------------- engine
@functools.lru_cache(maxsize=None)
def _device_inputs(name):
    return {k: v.to(DEV).contiguous() for k, v in BY_NAME[name].inputs().items()}


def _run(row, t):
    out = row.run(row.state(), t)
    torch.cuda.synchronize()
    return out


_REFERENCE = {}


def _reference(row, twins=()):
    """The dense run (computed once per row and per set of replaced inputs, never modified): `twins` = ((input, kind), ...) for the
    inputs whose dense twin is not the input itself (the expanded kinds)."""
    key = (row.name, tuple(sorted(twins)))
    if key not in _REFERENCE:
        t = dict(_device_inputs(row.name))
        for k, kind in twins:
            t[k] = lv.dense_twin(t[k], kind)
        _REFERENCE[key] = _run(row, t)
    return _REFERENCE[key]


def _check_case(row, gate, choice):
    """choice: {input: kind}."""
    dense = _device_inputs(row.name)
    twins = tuple((k, kind) for k, kind in choice.items() if kind.startswith("expanded"))
    want = _reference(row, twins)
    variants = {k: lv.Variant(dense[k], kind) for k, kind in choice.items()}
    t = dict(dense, **{k: v.tensor for k, v in variants.items()})
    for k, v in variants.items():
        assert torch.equal(v.tensor, lv.dense_twin(dense[k], v.kind)), (k, v.kind)
    RECORDED.update(gate.names)                                      # (the dense run's, packing launches included)
    del gate.names[:]
    got = _run(row, t)
    fallback = [FALLS_BACK[(row.name, k, kind)] for k, kind in choice.items() if (row.name, k, kind) in FALLS_BACK]
    if fallback:
        assert not (row.native & set(gate.names)), ("listed as a fallback, but it launched", row.native & set(gate.names))
        _pool_fallback_check(t, got)
    else:
        missing = row.native - {re.sub(r"_f(16|64)$", "", n) for n in gate.names}
        assert not missing, f"{row.name} {choice}: not launched: {sorted(missing)} (an unlisted fallback)"
        assert got.keys() == want.keys(), (sorted(got), sorted(want))
        for k in want:
            if (row.name, k) in ATOMIC_OUTPUTS:
                err = float((got[k].double() - want[k].double()).abs().max() / want[k].double().abs().max())
                assert err <= ATOMIC_OUTPUTS[(row.name, k)], (k, err)
            else:
                assert _bits_equal(got[k], want[k]), f"{row.name} {choice}: output {k} differs from the dense run"
    for k, v in variants.items():
        v.check_untouched()
        mine = v.buffer.untyped_storage().data_ptr()
        for name, o in got.items():
            if row.name.startswith("render") and PASS_THROUGH.get(name) == k:
                assert not o.is_contiguous() or o.numel() == 1          # (still the expanded view, not something a kernel wrote)
                continue
            assert o.untyped_storage().data_ptr() != mine, f"{row.name}: output {name} lives in the buffer of input {k}"


SINGLE = [(r.name, k, kind) for r in ROWS for k in r.inputs() for kind in r.kinds(k)]


@pytest.mark.parametrize("name,key,kind", SINGLE, ids=lambda v: str(v))
def test_one_input_in_another_layout(name, key, kind, gate):
    _check_case(BY_NAME[name], gate, {key: kind})


@pytest.mark.parametrize("name", list(BY_NAME))
def test_all_inputs_in_other_layouts_together(name, gate):
    row = BY_NAME[name]
    choice = {}
    for i, k in enumerate(row.inputs()):
        kinds = [q for q in row.kinds(k) if (name, k, q) not in FALLS_BACK]
        if kinds:
            choice[k] = kinds[i % len(kinds)]
    assert choice
    _check_case(row, gate, choice)


@pytest.mark.parametrize("name", list(BY_NAME))
def test_dense_case_on_a_side_stream(name, gate):
    row = BY_NAME[name]
    want = _reference(row)
    side, main = torch.cuda.Stream(device=DEV), torch.cuda.current_stream(DEV)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        got = row.run(row.state(), dict(_device_inputs(name)))
    main.wait_stream(side)
    torch.cuda.synchronize()
    for k in want:
        if (name, k) in ATOMIC_OUTPUTS:
            err = float((got[k].double() - want[k].double()).abs().max() / want[k].double().abs().max())
            assert err <= ATOMIC_OUTPUTS[(name, k)], (k, err)
        else:
            assert _bits_equal(got[k], want[k]), f"{name}: output {k} differs on a side stream"


def _modules(state):
    if isinstance(state, torch.nn.Module):
        yield state
    elif isinstance(state, (tuple, list)):
        for q in state:
            yield from _modules(q)


def test_every_launched_entry_has_a_row_or_a_reason(gate):
    """The names in the package source = what the gate saw over the table + NOT_REACHED, nothing on both sides."""
    broken = []
    for row in ROWS:
        # every row's dense run goes through THIS gate, with the weight images dropped first: a module that an earlier test file of the
        # session already packed (the builders are shared) would otherwise not launch its packing entries again
        try:
            for m in _modules(row.state()):
                _lib.invalidate(m)
            _run(row, dict(_device_inputs(row.name)))
        except AssertionError as e:                                  # (the gate's refusal: nothing was launched; the sets are still worth reading)
            broken.append(f"{row.name}: {str(e)[:200]}")
        except RuntimeError as e:
            if not re.search(r"^e3dge_\w+ failed \(code -?\d+\)", str(e)):   # (an entry's own refusal, _lib.check; anything else -- a HIP error -- ends the test)
                raise
            broken.append(f"{row.name}: {str(e)[:200]}")
    names, families = launched_entry_names()
    seen = {re.sub(r"_f(16|64)$", "", n) if re.sub(r"_f(16|64)$", "", n) in families else n for n in RECORDED | set(gate.names)}
    both = sorted(seen & set(NOT_REACHED))
    assert not both, f"listed as not reached, but launched: {both}"
    unknown = sorted(set(NOT_REACHED) - names - families)
    assert not unknown, f"NOT_REACHED names that the package does not launch: {unknown}"
    missing = sorted((names | families) - seen - set(NOT_REACHED))
    assert not missing and not broken, f"launched by the package, but by no layout row: {missing}; rows whose dense run failed: {broken}"
