"""ctypes binding of libe3dge_hip.so (the C-ABI declared in include/e3dge_hip.h).

The library is built in-tree by `build.py` (hipcc --offload-arch=gfx950) and shipped next to this file; it is
loaded lazily on first use.  Nothing here falls back to another implementation: a missing library or a
failing call raises RuntimeError."""
import ctypes
import operator
import os
import threading
import weakref

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("E3DGE_LIB_PATH") or os.path.join(_HERE, "lib", "libe3dge_hip.so")   # override: kernel A/B variants
ABI_VERSION = 17
PREC_F32, PREC_F16X3, PREC_F16X3_V1, PREC_F16X3_G2 = 0, 1, 2, 3
AMAX_FLOATS = 64 * 32           # E3DGE_AMAX_FLOATS: one amax buffer (include/e3dge_hip.h)
MC_MAX_TRIS = 16                # E3DGE_MC_MAX_TRIS: triangles per case in e3dge_marching_cubes_tables (include/e3dge_hip.h)

_c_float_p = ctypes.c_void_p     # device pointers travel as integers
_i32, _i64, _f32, _vp = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p


class _Args(ctypes.Structure):
    """Base of the argument-struct mirrors: a pointer field takes a tensor (its data_ptr() is stored) as well as an address or None, in
    the constructor and on later assignment.  The struct remembers the distinct devices of the tensors it was given (`devices`; a
    nested struct such as `plan.up[i]` reports to the outermost one), so that launch() can take the launch device from it and refuse a
    struct that mixes devices.  The tensors themselves are not kept alive, exactly as with data_ptr()."""

    def __init__(self, *values, **fields):
        if values:                                  # positional, in field order, as ctypes.Structure takes them
            fields = dict(zip((f[0] for f in self._fields_), values), **fields)
        seen = None
        for name, value in fields.items():          # (one loop here, not one __setattr__ call per field: a launch wrapper's host time)
            kind = value.__class__
            if kind is not int and kind is not float and value is not None and hasattr(value, "data_ptr"):
                if value.device != seen:
                    seen = self._note(value.device)
                value = value.data_ptr()
            _set_field(self, name, value)

    def __setattr__(self, name, value):
        kind = value.__class__
        if kind is not int and kind is not float and value is not None and hasattr(value, "data_ptr"):
            self._note(value.device)
            value = value.data_ptr()
        _set_field(self, name, value)

    def _note(self, dev):
        root = self
        while root._b_base_ is not None:
            root = root._b_base_
        seen = root.__dict__.setdefault("devices", [])
        if dev not in seen:
            seen.append(dev)
        return dev


_set_field = ctypes.Structure.__setattr__


class RenderArgs(_Args):
    """Mirror of struct E3dgeRenderArgs (include/e3dge_hip.h)."""
    _fields_ = [
        ("packed", _vp), ("film", _vp), ("c2w", _vp), ("focal", _vp), ("near", _vp), ("far", _vp),
        ("t_vals", _vp), ("tex_alpha", _vp), ("tex_beta", _vp),
        ("sigmoid_beta", _f32), ("box_scale", _f32), ("mask_depth_thresh", _f32),
        ("batch", _i32), ("height", _i32), ("width", _i32), ("n_samples", _i32),
        ("res", _i32), ("force_background", _i32), ("precision", _i32),
        ("rgb", _vp), ("features", _vp), ("xyz", _vp), ("depth", _vp), ("mask", _vp), ("sdf", _vp),
        ("weights", _vp), ("points", _vp), ("rays_d", _vp), ("viewdirs", _vp), ("dists", _vp), ("save_args", _vp),
        ("backbone_out", _vp), ("backbone_in", _vp), ("weights_in", _vp),
    ]


class RenderBwdArgs(_Args):
    """Mirror of struct E3dgeRenderBwdArgs (include/e3dge_hip.h)."""
    _fields_ = [(n, _vp) for n in ("packed", "film", "args", "sdf", "dists", "points", "weights", "t_vals", "near", "far",
                                   "wg", "wb", "d_rgb_map", "d_feat_map", "d_xyz_map", "d_depth_map", "d_sdf", "tang", "rsave",
                                   "d_weights", "tex_alpha")] + [
        ("sigmoid_beta", _f32), ("batch", _i32), ("height", _i32), ("width", _i32), ("n_samples", _i32),
        ("force_background", _i32), ("precision", _i32)] + [(n, _vp) for n in ("d_rgb_pts", "d_sdf_pts", "partials", "dfilm", "dstyles",
                                                                                "d_tex_alpha", "d_tex_beta")] + [("phase", _i32)] + [
        (n, _vp) for n in ("d_lin", "lin_amax", "d_sigmoid_beta")]


class SirenBwdArgs(_Args):
    """Mirror of struct E3dgeSirenBwdArgs (include/e3dge_hip.h)."""
    _fields_ = [(n, _vp) for n in ("packed", "film", "args", "d_feat", "d_rgb", "d_sdf", "tang", "rsave", "wg", "wb", "tex_alpha")] + [
        ("batch", _i32), ("precision", _i32), ("n_pts", _i64), ("box_scale", _f32)] + [
        (n, _vp) for n in ("partials", "dfilm", "dstyles", "d_pts", "d_tex_alpha", "d_tex_beta", "d_lin", "lin_amax")]


class SirenWgradArgs(_Args):
    """Mirror of struct E3dgeSirenWgradArgs (include/e3dge_hip.h, ABI 16)."""
    _fields_ = [(n, _vp) for n in ("args", "d_lin", "lin_amax", "d_sdf", "d_rgb", "pts", "viewdirs", "d_w", "d_w_view_dirs", "d_w_first",
                                   "d_w_sigma", "d_b_sigma", "d_w_rgb", "d_b_rgb", "ws")] + [
        ("ws_floats", _i64), ("n_pts", _i64), ("batch", _i32), ("samples", _i32), ("precision", _i32), ("box_scale", _f32)]


class ModconvArgs(_Args):
    """Mirror of struct E3dgeModconvArgs (include/e3dge_hip.h)."""
    _fields_ = [(n, _vp) for n in ("x", "wimg", "style", "demod", "in_amax", "s_amax", "noise", "noise_w", "bias", "y", "out_amax")] + [
        ("negative_slope", _f32), ("act_scale", _f32)] + [(n, _i32) for n in ("act", "upsample", "batch", "ci", "co", "height", "width",
                                                                                "noise_batch")]


class ModLayer(_Args):
    """Mirror of struct E3dgeModLayer (include/e3dge_hip.h)."""
    _fields_ = [(n, _vp) for n in ("mod_weight", "mod_bias", "wsq", "style_out", "demod_out", "s_amax_out")] + [
        (n, _i32) for n in ("ci", "co", "latent_index", "row_start", "co_start")] + [("lin_scale", _f32), ("lr_mul", _f32)]


DEC2_MAX_UP = 6                 # E3DGE_DEC2_MAX_UP


class Dec2Conv(_Args):
    """Mirror of struct E3dgeDec2Conv (include/e3dge_hip.h)."""
    _fields_ = [(n, _vp) for n in ("wpre", "style", "demod", "wimg", "noise", "noise_w", "noise_amax", "bias")] + [
        ("bias_amax", _f32), ("ci", _i32), ("co", _i32), ("noise_batch", _i32)]


class Dec2Rgb(_Args):
    """Mirror of struct E3dgeDec2Rgb (include/e3dge_hip.h)."""
    _fields_ = [(n, _vp) for n in ("weight", "style", "bias", "wm", "out")] + [("scale", _f32), ("ci", _i32)]


class Dec2Plan(_Args):
    """Mirror of struct E3dgeDec2Plan (include/e3dge_hip.h)."""
    _fields_ = [("batch", _i32), ("n_up", _i32), ("in_res", _i32), ("in_ch", _i32),
                ("features", _vp), ("skip_in", _vp), ("mod_table", _vp), ("latent", _vp),
                ("n_mod", _i32), ("mod_rows", _i32), ("mod_co", _i32), ("n_latent", _i32), ("style_dim", _i32), ("reserved0", _i32),
                ("conv1", Dec2Conv), ("rgb1", Dec2Rgb),
                ("up", Dec2Conv * DEC2_MAX_UP), ("conv", Dec2Conv * DEC2_MAX_UP), ("rgb", Dec2Rgb * DEC2_MAX_UP),
                ("act", _vp * (2 * DEC2_MAX_UP + 2)), ("amax", _vp), ("meta", _vp),
                ("fir_blur", _vp), ("fir_up", _vp), ("negative_slope", _f32), ("act_scale", _f32),
                ("kernel_ms", ctypes.POINTER(ctypes.c_float)), ("n_kernel_ms", _i32), ("reserved1", _i32),
                ("fir_blur_1d", _f32 * 4), ("fir_blur_separable", _i32), ("save_for_backward", _i32)]


class Dec2BwdConv(_Args):
    """Mirror of struct E3dgeDec2BwdConv (include/e3dge_hip.h)."""
    _fields_ = [(n, _vp) for n in ("wpre_t", "wcol", "wimg_t")]


class Dec2BwdPlan(_Args):
    """Mirror of struct E3dgeDec2BwdPlan (include/e3dge_hip.h)."""
    _fields_ = [("d_img", _vp), ("d_features", _vp), ("conv1", Dec2BwdConv), ("up", Dec2BwdConv * DEC2_MAX_UP),
                ("conv", Dec2BwdConv * DEC2_MAX_UP), ("gact", _vp * (2 * DEC2_MAX_UP + 2)), ("pbuf", _vp),
                ("drgb", _vp * DEC2_MAX_UP), ("amax", _vp), ("meta", _vp), ("bounds", _vp),
                ("kernel_ms", ctypes.POINTER(ctypes.c_float)), ("n_kernel_ms", _i32), ("reserved", _i32),
                ("d_latent", _vp), ("ds_part", _vp), ("ds_part_floats", _i64)]


class WsLinear(_Args):
    """Mirror of struct E3dgeWsLinear (include/e3dge_hip.h)."""
    _fields_ = [(n, _vp) for n in ("wimg", "x", "amax_in", "bias", "colw", "m", "r1", "r2", "y", "amax_out")] + [("n_rows", _i64)] + [
        (n, _i32) for n in ("ld_x", "off_x", "ld_m", "off_m", "ld_r1", "off_r1", "ld_r2", "off_r2", "ld_y", "off_y", "pre_relu", "post")] + [
        ("slope", _f32), ("w_fuse", _f32), ("xmul", _vp), ("amax_xmul", _vp), ("ld_xmul", _i32), ("off_xmul", _i32), ("x_scale", _f32),
        ("reserved", _i32)]


class Wgrad(_Args):
    """Mirror of struct E3dgeWgrad (include/e3dge_hip.h)."""
    _fields_ = [(n, _vp) for n in ("a", "amax_a", "b", "amax_b", "c", "ws")] + [("ws_floats", _i64), ("n_rows", _i64)] + [
        (n, _i32) for n in ("lda", "off_a", "m", "ldb", "off_b", "n", "ldc", "relu_b")] + [(n, _vp) for n in ("xcol", "colsum", "ccol")] + [
        (n, _i32) for n in ("ld_xcol", "ld_ccol", "b_gap_at", "b_gap")]


MESH_MAX_FACES_PER_PIXEL = 8    # E3DGE_MESH_MAX_FACES_PER_PIXEL


class MeshRenderArgs(_Args):
    """Mirror of struct E3dgeMeshRenderArgs (include/e3dge_hip.h)."""
    _fields_ = [(n, _vp) for n in ("verts", "faces", "normals", "colors")] + [("n_verts", _i64), ("n_faces", _i64), ("camera", _f32 * 12),
               ("tan_half_fov", _f32), ("znear", _f32), ("zfar", _f32)] + [
        (n, _f32 * 3) for n in ("light_location", "ambient_color", "diffuse_color", "specular_color", "background_color")] + [
        ("blur_radius", _f32), ("sigma", _f32), ("gamma", _f32), ("image_size", _i32), ("faces_per_pixel", _i32)] + [
        (n, _vp) for n in ("image", "zbuf", "pix_to_face", "status", "ws")] + [("ws_bytes", _i64), ("bin_capacity", _i64)]


NOISE_PROJECT_FACES_PER_PIXEL, NOISE_PROJECT_MAX_MAPS = 17, 4    # E3DGE_NOISE_PROJECT_FACES_PER_PIXEL, E3DGE_NOISE_PROJECT_MAX_MAPS


class NoiseProjectArgs(_Args):
    """Mirror of struct E3dgeNoiseProjectArgs (include/e3dge_hip.h)."""
    _fields_ = [(n, _vp) for n in ("verts", "faces", "vert_noise", "prev")] + [("n_verts", _i64), ("n_faces", _i64), ("camera", _f32 * 12)] + [
        (n, _f32) for n in ("tan_half_fov", "znear", "zfar", "blur_radius", "sigma", "gamma")] + [("image_size", _i32), ("n_maps", _i32)] + [
        (n, _vp) for n in ("out", "valid", "status", "ws")] + [("ws_bytes", _i64), ("bin_capacity", _i64)]


LPIPS_LAYERS = 5


class LpipsArgs(_Args):
    """Mirror of struct E3dgeLpipsArgs (include/e3dge_hip.h)."""
    _fields_ = [(n, _vp) for n in ("packed", "x", "y")] + [(n, _i32) for n in ("batch", "height", "width", "reserved")] + [
        ("mean", _f32 * 3), ("std", _f32 * 3)] + [(n, _vp) for n in ("per_image", "per_layer", "mean_out")] + [
        ("taps", _vp * LPIPS_LAYERS), ("ws", _vp), ("ws_bytes", _i64)]


class LpipsBwdArgs(_Args):
    """Mirror of struct E3dgeLpipsBwdArgs (include/e3dge_hip.h)."""
    _fields_ = [("packed", _vp), ("packed_t", _vp), ("fwd_ws", _vp), ("fwd_ws_bytes", _i64)] + [
        (n, _i32) for n in ("batch", "height", "width")] + [("std", _f32 * 3)] + [(n, _vp) for n in ("upstream", "grad_x", "grad_y")] + [
        ("gpre", _vp * LPIPS_LAYERS), ("ws", _vp), ("ws_bytes", _i64)]


IDNET_CONVS, IDNET_BNS, IDNET_UNITS, IDNET_TAPS = 52, 54, 24, 8     # E3DGE_IDNET_* (include/e3dge_hip.h)


class IdnetPackSrc(_Args):
    """Mirror of struct E3dgeIdnetPackSrc (include/e3dge_hip.h)."""
    _fields_ = [("conv_w", _vp * IDNET_CONVS)] + [(n, _vp * IDNET_BNS) for n in ("bn_weight", "bn_bias", "bn_mean", "bn_var")] + [
        ("prelu", _vp * (IDNET_UNITS + 1)), ("se_fc1", _vp * IDNET_UNITS), ("se_fc2", _vp * IDNET_UNITS), ("head_w", _vp), ("head_b", _vp)]


class IdnetArgs(_Args):
    """Mirror of struct E3dgeIdnetArgs (include/e3dge_hip.h)."""
    _fields_ = [("packed", _vp), ("images", _vp * 3)] + [(n, _i32) for n in ("n_per_set", "n_sets", "height", "width")] + [
        ("embeddings", _vp), ("taps", _vp * IDNET_TAPS), ("ws", _vp), ("ws_bytes", _i64)]


IDNET_PRELUS = IDNET_UNITS + 1                                      # E3DGE_IDNET_PRELUS


class IdnetSaveArgs(_Args):
    """Mirror of struct E3dgeIdnetSaveArgs (include/e3dge_hip.h)."""
    _fields_ = [("net", IdnetArgs), ("saved", _vp), ("saved_bytes", _i64), ("n_saved", _i32), ("reserved", _i32)]


class IdnetBwdArgs(_Args):
    """Mirror of struct E3dgeIdnetBwdArgs (include/e3dge_hip.h)."""
    _fields_ = [("packed", _vp), ("packed_t", _vp), ("saved", _vp), ("saved_bytes", _i64)] + [
        (n, _i32) for n in ("n", "height", "width", "reserved")] + [("grad_embeddings", _vp), ("grad_images", _vp), ("gstage", _vp * IDNET_TAPS),
                                                                    ("masks", _vp * IDNET_PRELUS), ("ws", _vp), ("ws_bytes", _i64)]


class IdLossArgs(_Args):
    """Mirror of struct E3dgeIdLossArgs (include/e3dge_hip.h)."""
    _fields_ = [(n, _vp) for n in ("y_hat", "y", "x")] + [("batch", _i32), ("reserved", _i32)] + [(n, _vp) for n in ("dots", "loss", "sim_improvement")]


SHAPE_LOSS_SEGMENTS, SHAPE_SMOOTH_L1, SHAPE_EIKONAL = 4, 0, 1      # E3DGE_SHAPE_LOSS_SEGMENTS, E3DGE_SHAPE_* (include/e3dge_hip.h)


class ShapeLossSegment(_Args):
    """Mirror of struct E3dgeShapeLossSegment (include/e3dge_hip.h)."""
    _fields_ = [("pred", _vp), ("gt", _vp), ("d_pred", _vp), ("n", _i64), ("lambda_", _f32), ("kind", _i32)]


class ShapeLossArgs(_Args):
    """Mirror of struct E3dgeShapeLossArgs (include/e3dge_hip.h)."""
    _fields_ = [("seg", ShapeLossSegment * SHAPE_LOSS_SEGMENTS), ("terms", _vp), ("total", _vp), ("partial", _vp), ("partial_floats", _i64),
                ("upstream", _vp)]


DISC_MAX_BLOCKS, DISC_TAP_STDDEV, DISC_TAP_FINAL, DISC_TAP_STEM, DISC_TAPS = 8, 8, 9, 10, 11     # E3DGE_DISC_* (include/e3dge_hip.h)


class DiscPackSrc(_Args):
    """Mirror of struct E3dgeDiscPackSrc (include/e3dge_hip.h)."""
    _fields_ = [(n, _i32) for n in ("init_size", "channel_multiplier", "in_channels", "reserved")] + [("stem_w", _vp), ("stem_b", _vp)] + [
        (n, _vp * DISC_MAX_BLOCKS) for n in ("conv1_w", "conv1_b", "conv2_w", "conv2_b", "skip_w")] + [
        (n, _vp) for n in ("final_w", "final_b", "lin1_w", "lin1_b", "lin2_w", "lin2_b", "blur")]


class DiscArgs(_Args):
    """Mirror of struct E3dgeDiscArgs (include/e3dge_hip.h)."""
    _fields_ = [("packed", _vp), ("images", _vp)] + [(n, _i32) for n in ("n", "height", "width", "init_size", "channel_multiplier", "in_channels")] + [
        ("logits", _vp), ("taps", _vp * DISC_TAPS), ("ws", _vp), ("ws_bytes", _i64), ("saved", _vp), ("saved_bytes", _i64)]


class DiscBwdArgs(_Args):
    """Mirror of struct E3dgeDiscBwdArgs (include/e3dge_hip.h)."""
    _fields_ = [("packed", _vp), ("saved", _vp), ("saved_bytes", _i64)] + [
        (n, _i32) for n in ("n", "height", "width", "init_size", "channel_multiplier", "in_channels")] + [
        ("grad_logits", _vp), ("grad_images", _vp), ("gstage", _vp * DISC_TAPS), ("ws", _vp), ("ws_bytes", _i64)]


HGF_MAX_STACK, HGF_FRONT_SRC = 8, 16                               # E3DGE_HGF_* (include/e3dge_hip.h)


class HgfArgs(_Args):
    """Mirror of struct E3dgeHgfArgs (include/e3dge_hip.h)."""
    _fields_ = [("packed", _vp), ("input", _vp)] + [(n, _i32) for n in ("n", "height", "width", "num_stack", "num_hourglass", "reserved")] + [
        ("outputs", _vp * HGF_MAX_STACK), ("tmpx", _vp), ("normx", _vp), ("ws", _vp), ("ws_bytes", _i64)]


class HgfBwdArgs(_Args):
    """Mirror of struct E3dgeHgfBwdArgs (include/e3dge_hip.h)."""
    _fields_ = [("packed", _vp), ("packed_t", _vp), ("saved", _vp), ("saved_bytes", _i64), ("tmpx", _vp), ("normx", _vp)] + [
        (n, _i32) for n in ("n", "height", "width", "num_stack", "num_hourglass", "reserved")] + [
        ("g_outputs", _vp * HGF_MAX_STACK), ("g_normx", _vp), ("g_input", _vp), ("ws", _vp), ("ws_bytes", _i64), ("branch", _vp), ("branch_bytes", _i64), ("grads", _vp), ("input", _vp), ("outputs", _vp * HGF_MAX_STACK)]


ENC_HEADS, ENC_MAX_HEAD_CONVS = 9, 8                               # E3DGE_ENC_* (include/e3dge_hip.h)


class EncArgs(_Args):
    """Mirror of struct E3dgeEncArgs (include/e3dge_hip.h)."""
    _fields_ = [("packed", _vp), ("images", _vp)] + [(n, _i32) for n in ("n", "size", "geo_dim", "tex_dim", "enable_decoder", "reserved")] + [
        (n, _vp) for n in ("thumb_out", "stylegan_out", "p32", "p64", "ws")] + [("ws_bytes", _i64)]


ALIGNER_TAPS, ALIGNER_SOURCES = 7, 249                            # E3DGE_ALIGNER_* (include/e3dge_hip.h)


class AlignerArgs(_Args):
    """Mirror of struct E3dgeAlignerArgs (include/e3dge_hip.h)."""
    _fields_ = [("packed", _vp), ("packed_floats", _i64), ("res_gt", _vp), ("thumb", _vp)] + [(n, _i32) for n in ("n", "size", "split", "thumb_up4")] + [
        ("out", _vp), ("taps", _vp * ALIGNER_TAPS), ("ws", _vp), ("ws_bytes", _i64)]


class AlignerSaveArgs(_Args):
    """Mirror of struct E3dgeAlignerSaveArgs (include/e3dge_hip.h)."""
    _fields_ = [("packed", _vp), ("packed_floats", _i64), ("src", _vp), ("n_src", _i32), ("train", _i32), ("res_gt", _vp), ("thumb", _vp)] + [
        (n, _i32) for n in ("n", "size", "split", "thumb_up4")] + [("out", _vp), ("taps", _vp * ALIGNER_TAPS), ("saved", _vp), ("saved_bytes", _i64),
                                                                   ("stats", _vp), ("stats_doubles", _i64)]


class AlignerBwdArgs(_Args):
    """Mirror of struct E3dgeAlignerBwdArgs (include/e3dge_hip.h)."""
    _fields_ = [("packed", _vp), ("packed_floats", _i64), ("packed_t", _vp), ("packed_t_floats", _i64), ("src", _vp), ("want", _vp), ("n_src", _i32),
                ("train", _i32), ("res_gt", _vp), ("thumb", _vp), ("g_out", _vp)] + [
        (n, _i32) for n in ("n", "size", "split", "thumb_up4", "want_input", "reserved")] + [
        ("saved", _vp), ("saved_bytes", _i64), ("stats", _vp), ("d_res_gt", _vp), ("d_thumb", _vp), ("grads", _vp), ("grad_floats", _i64), ("ws", _vp),
        ("ws_bytes", _i64)]


VDISC_MAX_BLOCKS, VDISC_TAPS = 6, 7                                # E3DGE_VDISC_* (include/e3dge_hip.h)
VDISC_FORM_STEM, VDISC_FORM_CONV, VDISC_FORM_CONV_POOL, VDISC_FORM_SKIP, VDISC_FORM_FINAL = 0, 1, 2, 3, 4
VDISC_SKIP_READ, VDISC_SKIP_POOL = 1, 2


class VdiscArgs(_Args):
    """Mirror of struct E3dgeVdiscArgs (include/e3dge_hip.h)."""
    _fields_ = [("packed", _vp), ("images", _vp), ("n", _i32), ("size", _i32), ("logits", _vp), ("viewpoints", _vp), ("taps", _vp * VDISC_TAPS),
                ("ws", _vp), ("ws_bytes", _i64)]


def has_experimental():
    """Was the loaded library built with -DE3DGE_EXPERIMENTAL (include/e3dge_hip_experimental.h, tools/build_variant.sh: one more
    precision mode, f16x3_v1, and no extra symbols; f16x3_g2 is in every build)?"""
    return bool(load().e3dge_build_flags() & 1)


# name -> (restype, argtypes); every symbol include/e3dge_hip.h declares.
SIGNATURES = {
    "e3dge_abi_version": (_i32, []),
    "e3dge_build_flags": (_i32, []),
    "e3dge_last_error": (ctypes.c_char_p, []),
    "e3dge_stream_capture_id": (_i64, [_vp]),
    "e3dge_fused_bias_act": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _f32, _f32, _i64, _i64, _i64, _vp]),
    "e3dge_fused_bias_act_f16": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _f32, _f32, _i64, _i64, _i64, _vp]),
    "e3dge_upfirdn2d_f16": (_i32, [_vp, _vp, _vp, _i64] + [_i32] * 12 + [_vp]),
    "e3dge_fused_bias_act_f64": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _f32, _f32, _i64, _i64, _i64, _vp]),
    "e3dge_upfirdn2d_f64": (_i32, [_vp, _vp, _vp, _i64] + [_i32] * 12 + [_vp]),
    "e3dge_noise_bias_act": (_i32, [_vp, _vp, _vp, _vp, _vp, _f32, _f32, _i64, _i64, _i64, _i64, _vp]),
    "e3dge_upfirdn2d": (_i32, [_vp, _vp, _vp, _i64] + [_i32] * 12 + [_vp]),
    "e3dge_upfirdn2d_out_size": (_i32, [_i32] * 6),
    "e3dge_modconv_weights": (_i32, [_vp, _vp, _vp, _f32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "e3dge_blur_noise_bias_act": (_i32, [_vp] * 6 + [_f32, _f32, _i64, _i64, _i32, _i32, _i32, _i32, _i64, _vp, _vp]),
    "e3dge_torgb": (_i32, [_vp] * 7 + [_f32, _i32, _i32, _i32, _i32, _vp]),
    "e3dge_decoder_styles": (_i32, [_vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _vp]),
    "e3dge_modconv_packed_words": (_i64, [_i32, _i32]),
    "e3dge_modconv_pack_weights": (_i32, [_vp, _vp, _vp, _f32, _i32, _i32, _vp]),
    "e3dge_modconv_demod": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "e3dge_amax": (_i32, [_vp, _vp, _i64, _vp]),
    "e3dge_amax_rows": (_i32, [_vp, _vp, _i64, _i32, _i64, _vp]),
    "e3dge_modconv3x3": (_i32, [ctypes.POINTER(ModconvArgs), _vp]),
    "e3dge_dec2_act_words": (_i64, [_i32, _i32, _i32]),
    "e3dge_dec2_prepack_weights": (_i32, [_vp, _vp, _f32, _i32, _i32, _vp]),
    "e3dge_dec2_num_launches": (_i32, [_i32]),
    "e3dge_dec2_forward": (_i32, [ctypes.POINTER(Dec2Plan), _vp]),
    "e3dge_dec2_prepack_weights_t": (_i32, [_vp, _vp, _f32, _i32, _i32, _i32, _vp]),
    "e3dge_dec2_pbuf_words": (_i64, [_i32, _i32, _i32]),
    "e3dge_dec2_bwd_num_launches": (_i32, [_i32]),
    "e3dge_dec2_backward": (_i32, [ctypes.POINTER(Dec2Plan), ctypes.POINTER(Dec2BwdPlan), _vp]),
    "e3dge_dec2_dlatent_ws_floats": (_i64, [ctypes.POINTER(Dec2Plan)]),
    "e3dge_dec2_pack": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "e3dge_dec2_unpack": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "e3dge_siren_packed_floats": (_i64, []),
    "e3dge_siren_pack_weights": (_i32, [_vp] * 11 + [_vp]),
    "e3dge_film_params": (_i32, [_vp] * 6 + [_i32, _vp]),
    "e3dge_siren_render_fwd": (_i32, [ctypes.POINTER(RenderArgs), _vp]),
    "e3dge_siren_backbone_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "e3dge_siren_points_fwd": (_i32, [_vp, _vp, _vp, _vp, _f32, _i32, _i64, _vp, _vp, _vp, _i32, _vp]),
    "e3dge_siren_bwd_partial_floats": (_i64, [_i32, _i64]),
    "e3dge_siren_bwd": (_i32, [ctypes.POINTER(SirenBwdArgs), _vp]),
    "e3dge_siren_sdf_grad": (_i32, [_vp, _vp, _vp, _vp, _f32, _i32, _i64, _vp, _vp, _i32, _vp]),
    "e3dge_siren_tangent": (_i32, [_vp, _vp, _vp, _vp, _f32, _i32, _i64, _vp, _i32, _vp]),
    "e3dge_siren_tangent_tr": (_i32, [_vp, _vp, _vp, _vp, _vp, _f32, _i32, _i64, _vp, _i32, _vp]),
    "e3dge_siren_render_bwd": (_i32, [ctypes.POINTER(RenderBwdArgs), _vp]),
    "e3dge_resblock_packed_floats": (_i64, []),
    "e3dge_resblock_pack_weights": (_i32, [_vp] * 6 + [_i32, _vp]),
    "e3dge_tex_modulations_fwd": (_i32, [_vp, _vp, _i32, _i64, _vp, _vp, _vp]),
    "e3dge_tex_film_fwd": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "e3dge_resblock_bwd_packed_floats": (_i64, []),
    "e3dge_resblock_bwd_pack_weights": (_i32, [_vp] * 5 + [_i32, _vp]),
    "e3dge_tex_modulations_bwd_ws_floats": (_i64, [_i64]),
    "e3dge_tex_modulations_bwd": (_i32, [_vp, _vp, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "e3dge_wgrad_ws_floats": (_i64, [_i32, _i32, _i64]),
    "e3dge_wgrad": (_i32, [_vp, _vp]),
    "e3dge_siren_wgrad_ws_floats": (_i64, [_i32, _i64]),
    "e3dge_siren_wgrad": (_i32, [ctypes.POINTER(SirenWgradArgs), _vp]),
    "e3dge_local_query": (_i32, [_vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _i32, _vp]),
    "e3dge_local_query_bwd": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _i32, _vp]),
    "e3dge_local_query_sort_ws_ints": (_i64, [_i32, _i64, _i32, _i32]),
    "e3dge_local_query_bwd_sorted": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _i32, _vp, _i64, _vp]),
    "e3dge_pos_encoding": (_i32, [_vp, _i32, _i32, _vp, _i64, _i32, _vp]),
    "e3dge_image_metrics_scratch_floats": (_i64, [_i32, _i32, _i32, _i32]),
    "e3dge_image_metrics": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp]),
    "e3dge_image_metric_row": (_i32, [_vp, _vp, _vp, _vp, _i32, _f32, _f32, _f32, _vp]),
    "e3dge_lpips_packed_floats": (_i64, []),
    "e3dge_lpips_pack_weights": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "e3dge_lpips_ws_bytes": (_i64, [_i32, _i32, _i32]),
    "e3dge_lpips_forward": (_i32, [ctypes.POINTER(LpipsArgs), _vp]),
    "e3dge_lpips_packed_t_floats": (_i64, []),
    "e3dge_lpips_pack_weights_t": (_i32, [_vp, _vp, _vp]),
    "e3dge_lpips_bwd_ws_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "e3dge_lpips_backward": (_i32, [ctypes.POINTER(LpipsBwdArgs), _vp]),
    "e3dge_idnet_packed_floats": (_i64, []),
    "e3dge_idnet_pack_weights": (_i32, [_vp, _vp, _vp]),
    "e3dge_idnet_ws_bytes": (_i64, [_i32]),
    "e3dge_idnet_embed": (_i32, [ctypes.POINTER(IdnetArgs), _vp]),
    "e3dge_id_loss": (_i32, [ctypes.POINTER(IdLossArgs), _vp]),
    "e3dge_idnet_conv_tiles": (_i32, [_i32] * 5),
    "e3dge_idnet_conv": (_i32, [_vp] * 8 + [_i32] * 7 + [_vp]),
    "e3dge_idnet_packed_t_floats": (_i64, []),
    "e3dge_idnet_pack_weights_t": (_i32, [_vp, _vp, _vp]),
    "e3dge_idnet_saved_bytes": (_i64, [_i32]),
    "e3dge_idnet_embed_save": (_i32, [ctypes.POINTER(IdnetSaveArgs), _vp]),
    "e3dge_idnet_bwd_ws_bytes": (_i64, [_i32, _i32, _i32]),
    "e3dge_idnet_backward": (_i32, [ctypes.POINTER(IdnetBwdArgs), _vp]),
    "e3dge_idnet_conv_bwd": (_i32, [_vp] * 9 + [_i32] * 7 + [_vp]),
    "e3dge_idnet_prep_bwd": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "e3dge_hitprob_points": (_i32, [_vp] * 8 + [_i32, _i64, _i32, _i32, _vp]),
    "e3dge_hitprob_composite": (_i32, [_vp] * 6 + [_f32, _i32, _i32, _i64, _i32, _i32, _vp]),
    "e3dge_align_volume": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "e3dge_marching_cubes_ws_bytes": (_i64, [_i32, _i32, _i32]),
    "e3dge_marching_cubes_count": (_i32, [_vp, _vp, _i64, _vp, _i32, _i32, _i32, _i64, _i64, _i64, _vp]),
    "e3dge_marching_cubes_emit": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _i32, _i32, _i32, _i64, _i64, _i64, _i32, _vp]),
    "e3dge_marching_cubes_tables": (_i32, [_vp, _vp]),
    "e3dge_depth_mesh": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp]),
    "e3dge_vertex_normals_ws_bytes": (_i64, [_i64]),
    "e3dge_vertex_normals": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _vp]),
    "e3dge_mesh_render_ws_bytes": (_i64, [_i64, _i64, _i32, _i64]),
    "e3dge_mesh_render": (_i32, [ctypes.POINTER(MeshRenderArgs), _vp]),
    "e3dge_mesh_subdivide": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp]),
    "e3dge_noise_project_ws_bytes": (_i64, [_i64, _i64, _i32, _i64]),
    "e3dge_noise_project": (_i32, [ctypes.POINTER(NoiseProjectArgs), _vp]),
    "e3dge_selftest_mfma": (_i32, [_vp, _vp, _vp, _i32, _vp]),
    "e3dge_selftest_mfma16": (_i32, [_vp, _vp, _vp, _i32, _vp]),
    "e3dge_selftest_mfma16x16": (_i32, [_vp, _vp, _vp, _i32, _vp]),
    "e3dge_ws_image_bytes": (_i64, [_i32]),
    "e3dge_ws_pack": (_i32, [_vp, _vp, _i32, _vp]),
    "e3dge_ws_linear": (_i32, [ctypes.POINTER(WsLinear), _vp]),
    "e3dge_ws_rowdot2": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i64, _vp]),
    "e3dge_selftest_sin": (_i32, [_vp, _vp, _i32, _vp]),
    "e3dge_selftest_sin_poly": (_i32, [_vp, _vp, _i32, _vp]),
    "e3dge_avgpool_fwd": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "e3dge_avgpool_bwd": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "e3dge_sqerr_bwd": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "e3dge_shape_loss_partial_floats": (_i64, [ctypes.POINTER(ShapeLossArgs)]),
    "e3dge_shape_loss_fwd": (_i32, [ctypes.POINTER(ShapeLossArgs), _vp]),
    "e3dge_shape_loss_bwd": (_i32, [ctypes.POINTER(ShapeLossArgs), _vp]),
    "e3dge_disc_packed_floats": (_i64, [_i32] * 3),
    "e3dge_disc_pack_weights": (_i32, [_vp, _vp, _vp]),
    "e3dge_disc_ws_bytes": (_i64, [_i32] * 7),
    "e3dge_disc_saved_bytes": (_i64, [_i32] * 4),
    "e3dge_disc_forward": (_i32, [ctypes.POINTER(DiscArgs), _vp]),
    "e3dge_disc_backward": (_i32, [ctypes.POINTER(DiscBwdArgs), _vp]),
    "e3dge_disc_conv": (_i32, [_vp] * 6 + [_i32] * 9 + [_f32, _vp]),
    "e3dge_disc_conv_dgrad": (_i32, [_vp] * 5 + [_f32, _f32, _vp] + [_i32] * 7 + [_f32, _vp]),
    "e3dge_disc_stddev": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "e3dge_hgf_packed_floats": (_i64, [_i32, _i32]),
    "e3dge_hgf_pack_weights": (_i32, [_vp, _vp, _i32, _vp, _i32, _i32, _vp]),
    "e3dge_hgf_ws_bytes": (_i64, [_i32] * 5),
    "e3dge_hgf_forward": (_i32, [ctypes.POINTER(HgfArgs), _vp]),
    "e3dge_hgf_front": (_i32, [_vp] * 4 + [_i32] * 5 + [_vp, _i64, _vp]),
    "e3dge_hgf_conv": (_i32, [_vp] * 8 + [_i32] * 12 + [_vp]),
    "e3dge_hgf_norm": (_i32, [_vp] * 4 + [_i32] * 7 + [_vp]),
    "e3dge_hgf_pool": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp]),
    "e3dge_hgf_up_add": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "e3dge_hgf_saved_bytes": (_i64, [_i32] * 5),
    "e3dge_hgf_forward_saving": (_i32, [ctypes.POINTER(HgfArgs), _vp, _i64, _vp]),
    "e3dge_hgf_front_saving": (_i32, [_vp] * 4 + [_i32] * 5 + [_vp, _i64, _vp, _i64, _vp]),
    "e3dge_hgf_packed_t_floats": (_i64, [_i32, _i32]),
    "e3dge_hgf_pack_weights_t": (_i32, [_vp, _vp, _i32, _vp, _i32, _i32, _vp]),
    "e3dge_hgf_bwd_ws_bytes": (_i64, [_i32] * 5),
    "e3dge_hgf_backward": (_i32, [ctypes.POINTER(HgfBwdArgs), _vp]),
    "e3dge_hgf_front_backward": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _vp] + [_i32] * 5 + [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "e3dge_hgf_branch_bytes": (_i64, [_i32] * 5),
    "e3dge_hgf_conv_dgrad": (_i32, [_vp] * 7 + [_i32] * 10 + [_vp]),
    "e3dge_hgf_norm_bwd": (_i32, [_vp] * 6 + [_i32, _i32, _vp, _vp, _vp, _vp] + [_i32] * 7 + [_vp]),
    "e3dge_hgf_grad_floats": (_i64, [_i32, _i32]),
    "e3dge_hgf_wgrad_ws_floats": (_i64, [_i32] * 7),
    "e3dge_hgf_conv_wgrad": (_i32, [_vp] * 5 + [_i32] * 10 + [_vp, _i64, _vp]),
    "e3dge_hgf_pool_bwd": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "e3dge_hgf_up_bwd": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp]),
    "e3dge_enc_packed_floats": (_i64, [_i32] * 4),
    "e3dge_enc_pack_weights": (_i32, [_vp, _vp] + [_i32] * 5 + [_vp]),
    "e3dge_enc_ws_bytes": (_i64, [_i32] * 5),
    "e3dge_enc_forward": (_i32, [ctypes.POINTER(EncArgs), _vp]),
    "e3dge_enc_lateral": (_i32, [_vp] * 6 + [_i32] * 7 + [_vp]),
    "e3dge_enc_head_conv": (_i32, [_vp] * 5 + [_i32] * 7 + [_vp]),
    "e3dge_enc_head_tail": (_i32, [_vp] * 7 + [_i64] + [_i32] * 5 + [_vp]),
    "e3dge_aligner_packed_floats": (_i64, []),
    "e3dge_aligner_pack": (_i32, [_vp, _i64, _vp, _i32, _vp]),
    "e3dge_aligner_workspace_bytes": (_i64, [_i32]),
    "e3dge_aligner_forward": (_i32, [ctypes.POINTER(AlignerArgs), _vp]),
    "e3dge_aln_conv": (_i32, [_vp] * 9 + [_i64] + [_i32] * 10 + [_vp]),
    "e3dge_aln_up2": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp]),
    "e3dge_aln_norm_ws_bytes": (_i64, [_i32] * 4),
    "e3dge_aln_bn_stats": (_i32, [_vp] * 7 + [_i64] + [_i32] * 5 + [_vp]),
    "e3dge_aln_bn_apply": (_i32, [_vp] * 6 + [_i32] * 8 + [_vp]),
    "e3dge_aln_norm_bwd": (_i32, [_vp] * 12 + [_i64] + [_i32] * 6 + [_vp]),
    "e3dge_aln_prelu_bwd": (_i32, [_vp] * 6 + [_i64] + [_i32] * 4 + [_vp]),
    "e3dge_aln_up2_bwd": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp]),
    "e3dge_aln_pick_bwd": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "e3dge_aln_conv_dgrad": (_i32, [_vp] * 6 + [_i64] + [_i32] * 7 + [_vp]),
    "e3dge_aln_wgrad_ws_floats": (_i64, [_i32] * 7),
    "e3dge_aln_conv_wgrad": (_i32, [_vp] * 6 + [_i64] + [_i32] * 9 + [_vp]),
    "e3dge_aligner_saved_bytes": (_i64, [_i32]),
    "e3dge_aligner_bwd_workspace_bytes": (_i64, [_i32]),
    "e3dge_aligner_grad_floats": (_i64, []),
    "e3dge_aligner_grad_offset": (_i64, [_i32]),
    "e3dge_aligner_stats_channels": (_i64, []),
    "e3dge_aligner_packed_t_floats": (_i64, []),
    "e3dge_aligner_branch_count": (_i64, [_i32]),
    "e3dge_aligner_pack_t": (_i32, [_vp, _i64, _vp, _i32, _vp]),
    "e3dge_aligner_forward_saving": (_i32, [ctypes.POINTER(AlignerSaveArgs), _vp]),
    "e3dge_aligner_backward": (_i32, [ctypes.POINTER(AlignerBwdArgs), _vp]),
    "e3dge_aligner_branch_bytes": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _vp]),
    "e3dge_vdisc_packed_floats": (_i64, [_i32]),
    "e3dge_vdisc_pack_weights": (_i32, [_vp, _vp, _i32, _i32, _vp]),
    "e3dge_vdisc_ws_bytes": (_i64, [_i32, _i32]),
    "e3dge_vdisc_forward": (_i32, [ctypes.POINTER(VdiscArgs), _vp]),
    "e3dge_vdisc_conv": (_i32, [_vp] * 6 + [_i64] + [_i32] * 7 + [_vp]),
}

_lib = None
_lock = threading.Lock()


def _adopt_torch_hip_runtime():
    """libe3dge_hip.so needs libamdhip64.so.7.  PyTorch-ROCm wheels ship their own copy; a process must not
    hold two HIP runtimes (streams and device pointers would not be interchangeable and the second runtime
    does not even find the device).  Importing torch first and pinning ITS libamdhip64 globally makes our
    NEEDED entry resolve to the copy torch uses, whatever the import order of the caller."""
    try:
        import torch
    except ImportError:          # plain C-ABI use without torch: the system ROCm runtime is the only one
        return
    cand = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)


def load():
    """Load (once) and return the ctypes handle; raises if the library is absent or has the wrong ABI."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no fallback implementation.")
        _adopt_torch_hip_runtime()
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)     # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        got = lib.e3dge_abi_version()
        if got != ABI_VERSION:
            raise RuntimeError(f"libe3dge_hip.so ABI {got} != expected {ABI_VERSION}; rebuild")
        _lib = lib
    return _lib


def check(rc, what):
    if rc != 0:
        msg = load().e3dge_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def query(name, *args, exc=RuntimeError):
    """The value of the size entry `name` (a *_bytes / *_floats query: a plain call, no stream); a negative one raises `exc` with the
    entry's name and the library's message."""
    lib = load()
    v = getattr(lib, name)(*args)
    if v < 0:
        raise exc(f"{name}: {lib.e3dge_last_error().decode(errors='replace')}")
    return v


STAMP_UNITS = ("siren", "siren_bwd", "resblock", "modconv", "decoder2")      # kStampUnit* (csrc/stamps.h), in order
STAMP_SLOTS, STAMP_WORDS = 320, 24                                           # kStampSlots, kStampWords


def _stamps_call(unit, out, n_words):
    lib = load()
    fn = lib.e3dge_debug_stamps          # (not in include/e3dge_hip.h: bound here, on first use)
    fn.restype, fn.argtypes = _i32, [_i32, ctypes.POINTER(ctypes.c_ulonglong), _i64]
    check(fn(STAMP_UNITS.index(unit), out, n_words), f"stamps({unit})")


def read_stamps(unit):
    """The cycle stamps the kernels of translation unit `unit` (STAMP_UNITS) left in their side buffer, as STAMP_SLOTS lists of
    STAMP_WORDS ints (csrc/stamps.h says which word is what; tools/kernel_stamps.py prints them).  Synchronises with the device.
    Raises RuntimeError naming the -D the unit needs when the loaded library (E3DGE_LIB_PATH) is not instrumented for it."""
    buf = (ctypes.c_ulonglong * (STAMP_SLOTS * STAMP_WORDS))()
    _stamps_call(unit, buf, len(buf))
    return [list(buf[s * STAMP_WORDS:(s + 1) * STAMP_WORDS]) for s in range(STAMP_SLOTS)]


def clear_stamps(unit):
    """Zero the unit's stamp buffer (same errors as read_stamps)."""
    _stamps_call(unit, None, 0)


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def dense(t, align=16):
    """`t` itself when a kernel may take it as it is -- contiguous, base pointer a multiple of `align` bytes -- and a fresh contiguous
    copy otherwise (a strided, expanded or permuted view; a contiguous slice such as `pts[1:]` of (B, 125, 3) floats, whose pointer
    is 12 mod 16).  None stays None.  DESIGN.md 'What a kernel may be handed' lists the entries that take 4-byte alignment (pass
    align=4 there); every other pointer of a caller's tensor goes through this with the default."""
    if t is None:
        return None
    if t.is_contiguous() and t.data_ptr() % align == 0:
        return t
    import torch
    return t.clone(memory_format=torch.contiguous_format)      # (the allocators align a fresh block far beyond 16 bytes)


def stream_of(t):
    """The current HIP stream of the tensor's device (or of a device), as the void* the C-ABI wants."""
    import torch
    return torch.cuda.current_stream(getattr(t, "device", t)).cuda_stream


def launch(name, *args):
    """Queue the C-ABI entry point `name`: the one way the package launches a kernel.  A tensor argument goes as its data_ptr(), None
    as NULL, an argument struct (_Args) by reference, numbers as they are (host addresses and `data_ptr() + offset` are plain ints).  The
    launch device is that of the first tensor -- an argument, or a field of an argument struct --; every other tensor must live there too
    (a pointer from another GPU would fault inside the kernel, so it raises here, before anything is queued).  The call runs under
    on_device(dev) with dev's current stream appended as the last argument, and a non-zero return raises with `name` and the library's
    message.  Entry points that take no stream (size queries, tables, e3dge_last_error) are plain calls on load()."""
    fn = getattr(load(), name)
    dev, out = None, []
    for a in args:
        kind = a.__class__
        if kind is int or kind is float or a is None:
            out.append(a)
            continue
        if hasattr(a, "data_ptr"):
            devices = (a.device,)
            out.append(a.data_ptr())
        elif isinstance(a, _Args):
            devices = a.__dict__.get("devices", ())
            out.append(ctypes.byref(a))
        else:                    # bool, numpy scalars, ctypes arrays: ctypes converts them by the declared argtypes
            out.append(a)
            continue
        for d in devices:
            if dev is None:
                dev = d
            elif d != dev:
                raise RuntimeError(f"{name}: arguments live on {dev} and on {d}; every tensor of a launch must be on the launch device")
    if dev is None:
        raise RuntimeError(f"{name}: no tensor argument to take the launch device from")
    with on_device(dev):
        rc = fn(*out, stream_of(dev))
    if rc != 0:
        check(rc, name)


def params_of(module):
    """The module's parameters as `module.parameters()` yields them, without walking the module tree on every call: the
    (sub-module, name) slots are listed once and looked up per call, so a replaced Parameter object is still seen.  The listing is
    re-validated cheaply on every call -- the number of entries of every sub-module's `_parameters` / `_modules` dict it was built from
    -- so a parameter or sub-module ADDED or REMOVED later (weight_norm, parametrize, add_module) rebuilds it instead of leaving the
    weight-image caches and requires_grad checks looking at detached parameters (round-4 advisor finding).  `module.parameters()`
    costs ~1.3 us per parameter -- 77 us for the SIREN, called by every launch wrapper to key its weight-image cache: ~0.7 ms of host
    time per training step, which the GPU spent idle between launches (rocprofv3 kernel trace, round 4); the check is ~2 us."""
    cached = module.__dict__.get('_e3dge_param_slots')
    if cached is not None and cached[2] == id(module):      # (a shallow copy -- DataParallel's replicas -- carries the master's listing)
        slots, checks, _ = cached
        if all(len(d) == n for d, n in checks):
            try:
                out = [d[n] for d, n in slots]
                if all(q is not None for q in out):
                    return out
            except KeyError:
                pass
    seen, slots, checks = set(), [], []
    for m in module.modules():
        checks.append((m._parameters, len(m._parameters)))
        checks.append((m._modules, len(m._modules)))
        for n, q in m._parameters.items():
            if q is not None and id(q) not in seen:
                seen.add(id(q))
                slots.append((m._parameters, n))
    module.__dict__['_e3dge_param_slots'] = (slots, checks, id(module))
    return [d[n] for d, n in slots]


def forget_params(module):
    module.__dict__.pop('_e3dge_param_slots', None)


STRICT_WEIGHT_CACHE = os.environ.get("E3DGE_STRICT_WEIGHT_CACHE", "0") not in ("", "0")
_WEIGHT_CACHE = weakref.WeakKeyDictionary()      # module -> {slot name: [(sources, signature, extra, fingerprint, value), ...], oldest first}


def _fingerprint(sources):
    """Norm and sum of every floating-point source: what E3DGE_STRICT_WEIGHT_CACHE=1 compares on every hit to catch writes through
    `.data` (device reductions and a host synchronisation per lookup)."""
    import torch
    with torch.no_grad():
        flat = [t.detach().reshape(-1) for t in sources if t.is_floating_point()]
        return torch.stack(list(torch._foreach_norm(flat)) + [t.sum() for t in flat]) if flat else torch.zeros(0)


def cached(module, slot, sources, build, extra=(), limit=1):
    """The value `build()` made from the tensors `sources` (parameters, buffers, or other cached values this one was derived from --
    every tensor whose contents or pointer the value carries), kept for `module` under the name `slot`; the one cache of every packed
    weight image, table and plan.  Entries live in a module-level weak map, never on the module: deepcopy, state_dict and pickling do not
    see them.  A hit needs the SAME tensor objects (the entry holds them, so their storage cannot be freed and handed to another tensor:
    (data_ptr, _version) alone is recycled by the caching allocator) with unchanged data_ptr (`Module._apply` swaps `.data` under the same
    Parameter) and _version (optimizer steps, load_state_dict, in-place ops), and an equal `extra` tuple (device, batch, resolution,
    stream).  Writes through `.data` bump no version: call invalidate(), or run with E3DGE_STRICT_WEIGHT_CACHE=1.  `limit` > 1 keeps that
    many entries of different `extra`, evicting the oldest first -- a captured graph may still replay the older ones."""
    try:
        entries = _WEIGHT_CACHE[module][slot]
    except KeyError:
        entries = _WEIGHT_CACHE.setdefault(module, {}).setdefault(slot, [])
    sig = [(t.data_ptr(), t._version) for t in sources]
    for e in entries:
        if e[1] == sig and e[2] == extra and all(map(operator.is_, e[0], sources)):
            if not STRICT_WEIGHT_CACHE or (e[3] is not None and e[3].equal(_fingerprint(sources))):
                return e[4]
    value = build()
    keep = [e for e in entries if e[2] != extra]              # (an entry of the same `extra` is replaced)
    entries[:] = keep[max(0, len(keep) - (limit - 1)):]
    entries.append((list(sources), sig, extra, _fingerprint(sources) if STRICT_WEIGHT_CACHE else None, value))
    return value


def weight_image(module, slot, sources, device, who, build):
    """cached(module, slot, sources, build) for a packed weight image that a launch on `device` will read: every source must be float32
    and live there (a pointer from elsewhere would fault inside the pack kernel), or it raises RuntimeError naming `who`."""
    import torch
    for t in sources:
        if t.device != device or t.dtype != torch.float32:
            raise RuntimeError(f"{who} weights must be float32 on the inputs' device {device} (got {t.dtype} on {t.device})")
    return cached(module, slot, sources, build)


def latest(module, slot):
    """The newest value cached for (module, slot), or None: for what a build records beside the image (the SIREN's weight range)."""
    entries = _WEIGHT_CACHE.get(module, {}).get(slot)
    return entries[-1][4] if entries else None


def invalidate(module):
    """Drop every cached value of `module` and of all its sub-modules (needed only after writes through `.data`)."""
    for m in module.modules():
        _WEIGHT_CACHE.pop(m, None)


class on_device:
    """`with on_device(dev):` = torch.cuda.device(dev) when `dev` is not already the current device, nothing otherwise (the context
    manager costs ~10 us of host time per launch wrapper; a single-GPU process never needs it)."""
    __slots__ = ("ctx",)

    def __init__(self, dev):
        import torch
        idx = dev.index if hasattr(dev, "index") else dev
        self.ctx = None if idx is None or torch.cuda.current_device() == idx else torch.cuda.device(dev)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            return self.ctx.__exit__(*exc)
        return False


def require_gpu(t, name, half_ok=False):
    """`half_ok`: the two stream ops (fused_bias_act, upfirdn2d) also take float16 and float64, as the reference's do
    (AT_DISPATCH_FLOATING_TYPES_AND_HALF)."""
    import torch
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"{name} must be a GPU (HIP) tensor; this build has no CPU path "
                           f"(got {getattr(t, 'device', type(t))})")
    if t.dtype != torch.float32 and not (half_ok and t.dtype in (torch.float16, torch.float64)):
        raise RuntimeError(f"{name} must be float32{', float16 or float64' if half_ok else ''} (got {t.dtype})")
