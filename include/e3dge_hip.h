/*
 * e3dge_hip.h -- C-ABI of libe3dge_hip.so: the MI355X (gfx950) volume-rendering hot path of E3DGE.
 *
 * Every entry point is `extern "C"`, takes plain device pointers + sizes + a HIP stream, allocates
 * nothing, never synchronises, and returns 0 on success or a negative E3DGE_ERR_* code (the message is
 * available from e3dge_last_error()).  All tensors are fp32, contiguous, resident in HBM.
 *
 * Each function names the reference interface it replaces (paths relative to the reference checkout).
 * The Python host side (cvpr23-e3dge_amd/_lib.py) binds these with ctypes; INTEGRATION.md shows the
 * stub a reference maintainer would add.
 */
#ifndef E3DGE_HIP_H
#define E3DGE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* e3dge_stream_t; /* a hipStream_t (NULL = the legacy default stream) */

enum {
    E3DGE_OK = 0,
    E3DGE_ERR_INVALID_ARG = -1, /* bad size / unsupported configuration / null pointer */
    E3DGE_ERR_LAUNCH = -2,      /* hipLaunchKernel / hipFuncSetAttribute failed          */
    E3DGE_ERR_UNSUPPORTED = -3  /* valid for the reference but outside this build's coverage */
};

/* ABI version; bumped whenever a signature below changes. */
int e3dge_abi_version(void);
/* bit 0: built with -DE3DGE_EXPERIMENTAL (the A/B-only precisions of include/e3dge_hip_experimental.h exist) */
int e3dge_build_flags(void);
/* 0 when `stream` is not being captured into a HIP graph, otherwise a positive id unique to the capture session (-1: query failed).
 * Host-side caches that hand device buffers from one launch to a later one (the backbone record of E3dgeRenderArgs) use it to
 * keep producer and consumer inside the same capture -- a graph that holds only the consumer would replay against a stale buffer. */
int64_t e3dge_stream_capture_id(e3dge_stream_t stream);
/* Thread-local message of the most recent failing call on this thread ("" if none). */
const char* e3dge_last_error(void);

/* --------------------------------------------------------------------------------------------
 * StyleGAN2 custom ops (reference: project/models/op/)
 * ------------------------------------------------------------------------------------------ */

/*
 * Replaces fused_bias_act_op / fused_bias_act_kernel
 * (project/models/op/fused_bias_act_kernel.cu:19-98, binding fused_bias_act.cpp:11-20).
 *   y[i] = act(x[i] + bias[(i / step_b) % size_b]) * scale
 *   act*10+grad: 10/11 linear, 12 -> 0, 30 lrelu(x>0 ? x : alpha x), 31 lrelu-grad gated by sign of
 *   ref[i] (the saved forward OUTPUT), 32 -> 0.
 * bias may be NULL (size_b == 0), ref may be NULL (treated as 0, as the reference does).
 * n < 2^31 (the reference indexes with int32, :66).
 */
int e3dge_fused_bias_act(float* y, const float* x, const float* bias, const float* ref, int act,
                         int grad, float alpha, float scale, int64_t n, int64_t step_b,
                         int64_t size_b, e3dge_stream_t stream);

/*
 * StyledConv tail fused into one pass: NoiseInjection + FusedLeakyReLU
 * (project/models/stylesdf_model.py:459-466 and :500-507 followed by fused_act.py:55-118):
 *   y[b,c,h,w] = lrelu(x[b,c,h,w] + noise_weight[0] * noise[b % noise_batch, 0, h, w] + bias[c], alpha) * scale
 * x,y: (batch, channels, hw) ; noise: (noise_batch, hw) with noise_batch in {1, batch};
 * noise_weight: device pointer to the 1-element NoiseInjection.weight.
 */
int e3dge_noise_bias_act(float* y, const float* x, const float* noise, const float* noise_weight,
                         const float* bias, float alpha, float scale, int64_t batch,
                         int64_t channels, int64_t hw, int64_t noise_batch,
                         e3dge_stream_t stream);

/*
 * Replaces upfirdn2d_op / upfirdn2d_kernel{,_large}
 * (project/models/op/upfirdn2d_kernel.cu:49-369, binding upfirdn2d.cpp:12-23) for minor_dim == 1,
 * which is the only way the Python wrappers call it (upfirdn2d.py:27,78,96).
 * x: (major, in_h, in_w); k: (kh, kw) FIR, correlated FLIPPED (upfirdn2d_kernel.cu:137);
 * y: (major, out_h, out_w) with out = (in*up + pad0 + pad1 - k + down) / down (:237-240).
 * Negative pads crop.  kh, kw <= 32.
 */
int e3dge_upfirdn2d(float* y, const float* x, const float* k, int64_t major, int in_h, int in_w,
                    int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0,
                    int pad_x1, int pad_y0, int pad_y1, e3dge_stream_t stream);
/* Half-precision forms of the two ops (ABI 11; the reference dispatches AT_DISPATCH_FLOATING_TYPES_AND_HALF:
 * fused_bias_act_kernel.cu:79, upfirdn2d_kernel.cu:311).  x, y, bias, ref are IEEE fp16 tensors; the FIR taps stay fp32.  Arithmetic
 * is fp32 with ONE rounding (RNE) on store -- at least as accurate as the reference's scalar_t = half arithmetic, which rounds after
 * every operation; parity is stated against the fp32 op on the widened inputs, rounded to fp16 (tests/test_gpu_selftest_and_ops.py).
 * What the half forms are FOR: e3dge_fused_bias_act_f16 is a stream-rate kernel (half the bytes, 0.8 of HBM like the fp32 form).
 * e3dge_upfirdn2d_f16 exists for DISPATCH PARITY with upfirdn2d_kernel.cu:311 only: it stages the same fp32 LDS patch as the fp32 form
 * and is bound by that stage, so a half Blur takes the wall time of the fp32 Blur (0.31 of HBM on half the bytes, bench `stream_ops`);
 * the decoder itself never calls it -- its blurs are fused into the packed fp32-accurate convolutions (e3dge_dec2_forward). */
int e3dge_fused_bias_act_f16(void* y, const void* x, const void* bias, const void* ref, int act, int grad, float alpha, float scale,
                             int64_t n, int64_t step_b, int64_t size_b, e3dge_stream_t stream);
int e3dge_upfirdn2d_f16(void* y, const void* x, const float* k, int64_t major, int in_h, int in_w, int kh, int kw, int up_x, int up_y,
                        int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1, e3dge_stream_t stream);
/* Double-precision forms of the two ops (ABI 12): the reference's AT_DISPATCH_FLOATING_TYPES_AND_HALF (fused_bias_act_kernel.cu:79,
 * upfirdn2d_kernel.cu:311) includes double, which is what torch.autograd.gradcheck / gradgradcheck feed an op.  Arithmetic is double
 * throughout (scalar_t = double in the reference); alpha / scale are widened from float as fused_bias_act.cpp:11-20 passes them; the FIR
 * taps are double (the reference reads kernel.data_ptr<scalar_t>()).  Plain element kernels: correctness tools, not stream-rate code. */
int e3dge_fused_bias_act_f64(double* y, const double* x, const double* bias, const double* ref, int act, int grad, float alpha, float scale,
                             int64_t n, int64_t step_b, int64_t size_b, e3dge_stream_t stream);
int e3dge_upfirdn2d_f64(double* y, const double* x, const double* k, int64_t major, int in_h, int in_w, int kh, int kw, int up_x, int up_y,
                        int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1, e3dge_stream_t stream);
/* Output extent helper (same formula as above); returns <0 if the result would be empty. */
int e3dge_upfirdn2d_out_size(int in, int up, int down, int pad0, int pad1, int k);

/*
 * ModulatedConv2d weight preparation (project/models/stylesdf_model.py:317-338) in one pass:
 *   w'[b,o,i,:] = scale * weight[o,i,:] * style[b,i];  if demod: w' *= rsqrt(sum_{i,k} w'^2 + 1e-8)
 * weight: (co, ci, kk) ; style: (batch, ci) (already through `modulation`) ;
 * transpose == 0 -> out (batch*co, ci, kk)   [F.conv2d, groups=batch]
 * transpose == 1 -> out (batch*ci, co, kk)   [F.conv_transpose2d, groups=batch]
 */
int e3dge_modconv_weights(float* out, const float* weight, const float* style, float scale,
                          int demodulate, int transpose, int batch, int co, int ci, int kk,
                          e3dge_stream_t stream);

/*
 * Fused modulated 3x3 convolution.  Replaces ModulatedConv2d.forward for kernel_size 3
 * (project/models/stylesdf_model.py:317-362: weight modulation + demodulation + F.conv2d(padding=1, groups=B) or
 * F.conv_transpose2d(stride=2, groups=B)) and, for the stride-1 layers, StyledConv's NoiseInjection + FusedLeakyReLU
 * tail (:459-466, :500-507) in the epilogue.  No per-sample weight tensor exists: the style scales the input patch
 * while it is staged, demod[b,co] scales the accumulators; the contraction runs as split-f16 (hi+lo, 3 products, fp32
 * accumulate) MFMAs against a weight image packed once per layer.
 *   e3dge_modconv_packed_words(co, ci): 32-bit words of the image.
 *   e3dge_modconv_pack_weights: weight (co, ci, 3, 3) [ModulatedConv2d.weight[0]], scale = 1/sqrt(ci*9) (:302) ->
 *       image, and wsq (co, ci) = sum_k (scale w)^2 for the demodulation.
 *   e3dge_modconv_demod: style (batch, ci) [= modulation(style), :319] -> demod (batch, co) = rsqrt(sum_ci s^2 wsq + 1e-8)
 *       (:323-324; skipped when demodulate == 0) and s_amax (batch) = max_ci |s|.
 *   amax buffers: max|tensor| tracked by the producer of an activation, so the next conv can choose its operand scale
 *       without re-reading the data: E3DGE_AMAX_FLOATS floats, zero-initialised by the caller; producers atomically max
 *       into one of E3DGE_AMAX_SLOTS slots (E3DGE_AMAX_STRIDE floats apart), the consumer takes the maximum over the slots.
 *   e3dge_amax: max|x| of a tensor into such a buffer (for inputs whose producer did not track it).
 *   e3dge_modconv3x3: x (batch, ci, H, W) -> y (batch, co, H, W), or with upsample (batch, co, 2H+1, 2W+1) = the
 *       transposed convolution BEFORE the FIR blur.  in_amax: amax buffer with max over slots >= max|x| (operand scaling;
 *       any upper bound works, a tight one keeps full precision).  act != 0 (stride-1 only):
 *       y = lrelu(conv * demod + noise_w[0] * noise[b % noise_batch] + bias[co], negative_slope) * act_scale.
 *       out_amax (optional amax buffer) receives max|y|.  ci %% 16 == 0, co %% 32 == 0.
 */
#define E3DGE_AMAX_SLOTS 64
#define E3DGE_AMAX_STRIDE 32
#define E3DGE_AMAX_FLOATS (E3DGE_AMAX_SLOTS * E3DGE_AMAX_STRIDE)
typedef struct E3dgeModconvArgs {
    const float* x; const uint32_t* wimg; const float* style; const float* demod; const float* in_amax;
    const float* s_amax; const float* noise; const float* noise_w; const float* bias;
    float* y; float* out_amax;
    float negative_slope, act_scale;
    int act, upsample, batch, ci, co, height, width, noise_batch;
} E3dgeModconvArgs;
/* One row of the decoder's modulation table (device-resident array) for e3dge_decoder_styles: all layers' modulation
 * vectors s = conv.modulation(latent[:, latent_index]) (EqualLinear, stylesdf_model.py:234-244 as used at :319), their
 * demodulation factors and max|s| in two launches instead of ~4 tiny kernels per layer.  row_start / co_start are the prefix
 * sums of ci / co over the table (co counts 0 for rows without demod_out). */
typedef struct E3dgeModLayer {
    const float* mod_weight;   /* (ci, style_dim)  conv.modulation.weight                                  */
    const float* mod_bias;     /* (ci)             conv.modulation.bias                                    */
    const float* wsq;          /* (co, ci) from e3dge_modconv_pack_weights, or NULL                         */
    float* style_out;          /* (batch, ci) out                                                          */
    float* demod_out;          /* (batch, co) out, or NULL (ToRGB: no demodulation)                         */
    float* s_amax_out;         /* (batch) out, or NULL                                                     */
    int ci, co, latent_index, row_start, co_start;
    float lin_scale, lr_mul;   /* EqualLinear.scale = lr_mul / sqrt(style_dim), lr_mul                      */
} E3dgeModLayer;
int e3dge_decoder_styles(const E3dgeModLayer* table, int n_layers, int total_rows, int total_co, const float* latent,
                         int n_latent, int style_dim, int batch, e3dge_stream_t stream);
int64_t e3dge_modconv_packed_words(int co, int ci);
int e3dge_modconv_pack_weights(uint32_t* image, float* wsq, const float* weight, float scale, int co, int ci,
                               e3dge_stream_t stream);
int e3dge_modconv_demod(float* demod, float* s_amax, const float* style, const float* wsq, int batch, int co, int ci,
                        int demodulate, e3dge_stream_t stream);
int e3dge_amax(float* out, const float* x, int64_t n, e3dge_stream_t stream);
/* ABI 14: the same over the first `width` columns of `n_rows` rows of pitch `ld` floats (4-byte aligned): a column block of a wider row tensor,
 * e.g. the first 256 of the 301 gradient columns torch.cat's backward hands to Fuse_sft_MLP (sft.py:84-110 behind e3dge_full_runner.py:185-317). */
int e3dge_amax_rows(float* out, const float* x, int64_t n_rows, int width, int64_t ld, e3dge_stream_t stream);
int e3dge_modconv3x3(const E3dgeModconvArgs* args, e3dge_stream_t stream);

/*
 * Blur + StyledConv tail of the up-sampling layers in one pass: y = lrelu(upfirdn2d(x, k, pad=(pad0,pad1)) +
 * noise_weight[0] * noise + bias[c], alpha) * scale  (stylesdf_model.py:346 then :459-466, :500-507), k a 4x4 FIR.
 * x (batch, channels, in_h, in_w) -> y (batch, channels, in_h+pad0+pad1-3, ...); noise (noise_batch, out_h*out_w) or NULL;
 * out_amax: optional amax buffer (see e3dge_modconv3x3) receiving max|y|.
 */
int e3dge_blur_noise_bias_act(float* y, const float* x, const float* k, const float* noise, const float* noise_weight,
                              const float* bias, float alpha, float scale, int64_t batch, int64_t channels, int in_h,
                              int in_w, int pad0, int pad1, int64_t noise_batch, float* out_amax, e3dge_stream_t stream);

/*
 * ToRGB.forward (stylesdf_model.py:531-541) in one pass: 1x1 modulated conv without demodulation (weight (3, ci) =
 * conv.weight[0,:,:,0,0], style (batch, ci) = conv.modulation(style), scale = 1/sqrt(ci)) + bias (3) + the skip image
 * (batch, 3, H/2, W/2) up-sampled with upfirdn2d(up=2, pad=(2,1)) by the 4x4 FIR `fir` (Upsample.kernel), or NULL.
 * x (batch, ci, H, W) -> y (batch, 3, H, W).  W %% 4 == 0.
 */
int e3dge_torgb(float* y, const float* x, const float* weight, const float* style, const float* bias, const float* skip,
                const float* fir, float scale, int batch, int ci, int height, int width, e3dge_stream_t stream);

/*
 * ---- Packed decoder pipeline ("dec2"): Decoder.forward (project/models/stylesdf_model.py:741-797) as ONE native call ----
 *
 * The up-sampler's activations never exist as fp32 planes between its kernels.  Every producer writes its output already
 * split for the f16 matrix pipe, in the layout the next convolution's LDS-DMA consumes verbatim:
 *
 *   packed tensor (batch, C/8, 2, H+2, W+2) of 16-byte entries:  entry (b, g, hl, y, x) = the eight f16 values
 *       hl = 0: hi = f16_rtz(v * 2^(141 - eb)),   hl = 1: lo = f16(v * 2^(141 - eb) - hi)       of channels 8g .. 8g+7
 *   at pixel (y-1, x-1); the one-entry border is zero (= the convolutions' zero padding) and is never written by a
 *   producer, so the caller zero-fills a packed buffer ONCE (workspace) and reuses it.  eb (one int per tensor, in
 *   `meta`) is the biased exponent of an a-priori bound on max|v| that the producer computes before its first store:
 *   stride-1 conv: act_scale * (amax_in * sqrt(9 ci) + |noise_w| amax_noise + max|bias|) (Cauchy-Schwarz: demodulated
 *   filters have unit norm); blur: act_scale * (amax_T + ...).  The bound may be 2^12 loose before the representation
 *   (22 bits relative to the tensor's maximum) degrades to fp32's 24.
 *
 * Weights: per sample, w'' = ((scale W) s) demod exactly as the reference rounds them (:319-326), times 128, split into
 * f16 hi/lo MFMA A-fragments (e3dge_modconv_packed_words words per sample), rebuilt by one launch per forward from the
 * pre-arranged fp32 image `wpre` (e3dge_dec2_prepack_weights, once per weight update).
 *
 * Kernels of one forward, all launched by e3dge_dec2_forward on `stream` (nothing else, no allocation, no sync unless
 * kernel_ms is given): styles (2), amax + pack of the features, per-sample weights, conv1, ToRGB, then per level: transposed
 * conv by output phase -> fp32 T, blur + noise + bias + lrelu -> packed, stride-1 conv (+ noise + bias + lrelu) -> packed,
 * ToRGB (+ FIR-up-sampled skip).  The convolutions stage BOTH operands by LDS-DMA (no VGPR staging, no conversion).
 */
#define E3DGE_DEC2_MAX_UP 6
typedef struct E3dgeDec2Conv {
    const float* wpre;        /* e3dge_dec2_prepack_weights image of ModulatedConv2d.weight (co*ci*9 floats)            */
    const float* style;       /* (batch, ci)  conv.modulation(latent) -- written by the styles launch of this call       */
    const float* demod;       /* (batch, co)  demodulation factors    -- idem                                            */
    uint32_t* wimg;           /* workspace: batch * e3dge_modconv_packed_words(co, ci) words                              */
    const float* noise;       /* (noise_batch, 1, OH, OW) or NULL                                                        */
    const float* noise_w;     /* NoiseInjection.weight (device scalar), required with noise                              */
    const float* noise_amax;  /* amax buffer holding max|noise| (e3dge_amax), required with noise                        */
    const float* bias;        /* (co) FusedLeakyReLU.bias                                                                */
    float bias_amax;          /* max|bias| (host value, computed when the weights are packed)                            */
    int32_t ci, co, noise_batch;
} E3dgeDec2Conv;
typedef struct E3dgeDec2Rgb {
    const float* weight;      /* (3, ci) ToRGB.conv.weight                                                               */
    const float* style;       /* (batch, ci)                                                                             */
    const float* bias;        /* (3)                                                                                     */
    float* wm;                /* workspace (batch, 3, ci): (scale W) s                                                   */
    float* out;               /* (batch, 3, res, res): this level's image (the last one is Decoder.forward's result)     */
    float scale;              /* 1 / sqrt(ci)                                                                            */
    int32_t ci;
} E3dgeDec2Rgb;
typedef struct E3dgeDec2Plan {
    int32_t batch, n_up, in_res, in_ch;
    const float* features;                         /* (batch, in_ch, in_res, in_res) fp32                                 */
    const float* skip_in;                          /* rgbd_in of Decoder.forward (batch, 3, in_res, in_res) or NULL        */
    const E3dgeModLayer* mod_table;                /* device table for the styles launch (see e3dge_decoder_styles)        */
    const float* latent;                           /* (batch, n_latent, style_dim)                                        */
    int32_t n_mod, mod_rows, mod_co, n_latent, style_dim, reserved0;
    E3dgeDec2Conv conv1;
    E3dgeDec2Rgb rgb1;
    E3dgeDec2Conv up[E3DGE_DEC2_MAX_UP];           /* up-sampling StyledConv of level u (convs[2u])                        */
    E3dgeDec2Conv conv[E3DGE_DEC2_MAX_UP];         /* stride-1 StyledConv of level u (convs[2u+1])                         */
    E3dgeDec2Rgb rgb[E3DGE_DEC2_MAX_UP];
    uint32_t* act[2 * E3DGE_DEC2_MAX_UP + 2];      /* packed workspaces: [0] features, [1] conv1 out, [2+2u] blur out, [3+2u] conv out */
    float* amax;                                   /* (3 n_up + 2) amax buffers (zeroed by the call): [0] features, [1] conv1 out, [2+3u] not written, [3+3u] blur out, [4+3u] conv out */
    int32_t* meta;                                 /* (2 n_up + 2) ints: eb of act[i]                                      */
    const float* fir_blur;                         /* 4x4 taps of the up-sampling convs' Blur (make_kernel * 4)            */
    const float* fir_up;                           /* 4x4 taps of ToRGB's Upsample                                        */
    float negative_slope, act_scale;
    float* kernel_ms;                              /* host array, n_kernel_ms floats, or NULL: HIP-event time of every launch (makes the call synchronous) */
    int32_t n_kernel_ms, reserved1;
    /* ABI 11: when the blur kernel is rank one with a SYMMETRIC factor (make_kernel([1,3,3,1]) is), fir_blur = outer(fir_blur_1d,
     * fir_blur_1d), fir_blur_1d = (g0, g1, g1, g0) and fir_blur_separable != 0: the fused up-sampling kernel applies the two 1-D passes (horizontal in registers,
     * vertical through LDS).  ABI 15: with n_up > 0, fir_blur_separable == 0 is rejected (E3DGE_ERR_INVALID_ARG); such a decoder takes the planar path. */
    float fir_blur_1d[4];
    int32_t fir_blur_separable;
    /* ABI 12: != 0 keeps the packed activation of the LAST convolution too (normally it only exists inside the fused ToRGB epilogue):
     * e3dge_dec2_backward reads the sign of every stored activation for lrelu'. */
    int32_t save_for_backward;
} E3dgeDec2Plan;
/* 32-bit words of a packed tensor */
int64_t e3dge_dec2_act_words(int batch, int channels, int res);
/* weight (co, ci, 3, 3) -> wpre[t][c][tap][lane][j] = scale * weight[32t + (lane & 31)][16c + 8 (lane >> 5) + j][tap] */
int e3dge_dec2_prepack_weights(float* wpre, const float* weight, float scale, int co, int ci, e3dge_stream_t stream);
/* launches per forward with n_up levels (= number of kernel_ms entries written): 6 + 4 n_up */
int e3dge_dec2_num_launches(int n_up);
int e3dge_dec2_forward(const E3dgeDec2Plan* plan, e3dge_stream_t stream);
/*
 * ---- Backward of the packed pipeline (ABI 12): d image -> d features, generator frozen ----------------------------------------------
 * The data gradient of Decoder.forward (project/models/stylesdf_model.py:742-797; ModulatedConv2d :317-362, StyledConv :469-507, ToRGB
 * :531-541, Blur / Upsample -> op/upfirdn2d.py:18-142, FusedLeakyReLU -> op/fused_act.py:19-84) that train_ae.py's stage-1 step takes
 * through the pixel loss on pool_256(gen_imgs) (trainers/trainer.py:1017-1031, :728) -- in the reference: autograd through F.conv2d /
 * F.conv_transpose2d on the modulated weights and the two custom ops' backward classes.  Here: the same MFMA convolutions on TRANSPOSED
 * per-sample weight images, gradients packed like the activations, lrelu' from the sign of the stored packed activations (csrc/
 * decoder2_bwd.h).  Call it after e3dge_dec2_forward(plan) ran with plan->save_for_backward != 0 on the same workspace and BEFORE
 * anything else overwrites that workspace (act[], style / demod / wm buffers).  d latent and parameter gradients are NOT produced.
 * Launches: norms (+ clearing the amax block), transposed weights, amax(d img), ToRGB^T + mask at the top, then per level
 * Upsample^T of d rgb, conv^T, Blur^T + phase split, convT^T (+ ToRGB^T of the level below), and conv1^T: 5 + 4 n_up.
 */
typedef struct E3dgeDec2BwdConv {
    const float* wpre_t;      /* e3dge_dec2_prepack_weights_t image of ModulatedConv2d.weight (co*ci*9 floats)                        */
    const float* wcol;        /* (ci) column sums over co of the (co, ci) table sum_taps (scale W)^2 that e3dge_modconv_pack_weights writes */
    uint32_t* wimg_t;         /* workspace: batch * e3dge_modconv_packed_words(ci, co) words                                          */
} E3dgeDec2BwdConv;
typedef struct E3dgeDec2BwdPlan {
    const float* d_img;                            /* (batch, 3, R, R), R = in_res << n_up: gradient of Decoder.forward's image       */
    float* d_features;                             /* (batch, in_ch, in_res, in_res): result                                          */
    E3dgeDec2BwdConv conv1;
    E3dgeDec2BwdConv up[E3DGE_DEC2_MAX_UP];
    E3dgeDec2BwdConv conv[E3DGE_DEC2_MAX_UP];
    uint32_t* gact[2 * E3DGE_DEC2_MAX_UP + 2];     /* packed gradient workspaces, shapes of plan->act[i], zero-filled ONCE; [0] unused */
    uint32_t* pbuf;                                /* phase planes of Blur^T: e3dge_dec2_pbuf_words(batch, co, res) of the largest up level */
    float* drgb[E3DGE_DEC2_MAX_UP];                /* [i]: (batch, 3, r, r) gradient of the ToRGB image of level i - 1 (r = in_res << i) */
    float* amax;                                   /* (4 n_up + 2) amax buffers (cleared by the call)                                 */
    int32_t* meta;                                 /* (3 n_up + 1) ints                                                               */
    float* bounds;                                 /* (3 n_up + 2) floats: operator norms of the transposed images / ToRGB tables     */
    float* kernel_ms;                              /* host array or NULL: HIP-event time of every launch of the d-features chain (makes the call synchronous) */
    int32_t n_kernel_ms, reserved;
    /* optional: the gradient to the decoder's W+ latent, (batch, n_latent, style_dim), or NULL.  Formed from per-channel dot products of
     * the tensors the chain leaves in its workspace -- dL/ds[ci] = (1/s) sum_p x dx - s sum_co demod^2 wsq sum_p g y (3x3 layers),
     * (1/s) sum_p act (ToRGB^T d rgb) (ToRGB), then modulation^T -- no weight-gradient contraction (csrc/decoder2_bwd.h), except for the
     * channels of a 3x3 layer whose |s| is at most 2^-10 of the layer's maximum: their first term is contracted directly, without the
     * division.  2 n_up + 7 more launches.  Needs plan->features / mod_table as the forward had them and ds_part = e3dge_dec2_dlatent_ws_floats(plan) floats. */
    float* d_latent;
    float* ds_part;
    int64_t ds_part_floats;
} E3dgeDec2BwdPlan;
/* weight (co, ci, 3, 3) -> wpre_t[t][c][tap][lane][j] = scale * weight[16c + 8 (lane >> 5) + j][32t + (lane & 31)][flip ? 8 - tap : tap];
 * flip = 1 for the stride-1 convolutions, 0 for the up-sampling (transposed-stride) ones.  ci %% 32 == 0, co %% 16 == 0. */
int e3dge_dec2_prepack_weights_t(float* wpre_t, const float* weight, float scale, int co, int ci, int flip, e3dge_stream_t stream);
int64_t e3dge_dec2_pbuf_words(int batch, int channels, int res);
int e3dge_dec2_bwd_num_launches(int n_up);
int64_t e3dge_dec2_dlatent_ws_floats(const E3dgeDec2Plan* plan);
int e3dge_dec2_backward(const E3dgeDec2Plan* plan, const E3dgeDec2BwdPlan* bwd, e3dge_stream_t stream);
/* stand-alone pieces (tests, tools): fp32 (batch, c, res, res) <-> packed; both use meta[0] / amax as e3dge_dec2_forward does */
int e3dge_dec2_pack(uint32_t* packed, int32_t* meta, const float* x, const float* amax, int batch, int channels, int res,
                    e3dge_stream_t stream);
int e3dge_dec2_unpack(float* x, const uint32_t* packed, const int32_t* meta, int batch, int channels, int res,
                      e3dge_stream_t stream);

/*
 * Reference-view hit probability (VolumeFeatureRenderer.query_hitting_probability_fixed_interval,
 * project/utils/volume_renderer.py:1326-1495; compositing with no_force_stop :826-837, :884).
 *   e3dge_hitprob_points: pts (batch, rays, s_pts, 3) world-space points of the query view, poses / extrinsics (batch, 3, 4) of the
 *       reference view (c2w / w2c), near / far (batch, rays), t_vals (n_samples) -> q (batch, rays, s_pts, n_samples, 3): the samples
 *       of the reference camera's ray through every point, and aux (batch, rays, s_pts, 4) = (lo, hi, frac, index) of the interpolation.
 *   e3dge_hitprob_composite: sdf (batch, rays, s_pts, n_samples) at q [e3dge_siren_points_fwd] -> out (batch, rays, s_pts): the
 *       compositing weight (visibility == 0) or transmittance (visibility != 0) interpolated at the point.
 */
int e3dge_hitprob_points(float* q, float* aux, const float* pts, const float* poses, const float* extrinsics, const float* near,
                         const float* far, const float* t_vals, int batch, int64_t rays, int s_pts, int n_samples, e3dge_stream_t stream);
int e3dge_hitprob_composite(float* out, const float* sdf, const float* aux, const float* near, const float* far, const float* t_vals,
                            float sigmoid_beta, int visibility, int batch, int64_t rays, int s_pts, int n_samples, e3dge_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * FiLM-SIREN volume renderer (reference: project/utils/volume_renderer.py)
 * ------------------------------------------------------------------------------------------ */

#define E3DGE_SIREN_WIDTH 256     /* W (options.py:841-844); the kernels are specialised for 256 */
#define E3DGE_SIREN_DEPTH 8       /* D backbone layers (options.py:837-840)                       */
#define E3DGE_SIREN_NLAYERS 9     /* D + views_linears                                           */

/* How the 256-wide contractions are evaluated.  Both accumulate in fp32 and meet the same parity bounds. */
#define E3DGE_PREC_F32 0          /* v_mfma_f32_32x32x2_f32 on fp32 operands                                     */
#define E3DGE_PREC_F16X3 1        /* operands split as f16 hi+lo, 3 f16 MFMA products per fp32 product, fp32 accumulate.  Forward
                                     launches: 8 waves x 16 points on v_mfma_f32_16x16x32_f16; backward-type launches: 4 waves x 32
                                     points on v_mfma_f32_32x32x16_f16 with per-point block scaling */
#define E3DGE_PREC_F16X3_V1 2     /* forward launches: the first-generation split-f16 kernel (4 waves x 32 points,
                                     v_mfma_f32_32x32x16_f16), kept for A/B measurements; backward-type launches: same as
                                     E3DGE_PREC_F16X3 */
#define E3DGE_PREC_F16X3_G2 3     /* The training configuration of E3DGE_PREC_F16X3 (round 6, csrc/siren16_bwd.h):
                                     * backward-type launches (e3dge_siren_bwd / _render_bwd / _sdf_grad / _tangent / _tangent_tr): the 8-wave x
                                       16-point layout of the forward kernel, saved-state streams by LDS-DMA through a per-wave ring.  Same
                                       block-scaled split-f16 arithmetic as E3DGE_PREC_F16X3; the second-order inputs come as the products
                                       ta_l r_l (e3dge_siren_tangent_tr);
                                     * forward launches (e3dge_siren_render_fwd / _points_fwd): the E3DGE_PREC_F16X3 kernel; `save_args` is
                                       written SLAB-MAJOR, which is what the launches above read (and write: rsave, tang): 16 consecutive
                                       rows of an image form a slab [L layers][16 tiles][lane 16 q + (row & 15)][4 floats] (feature =
                                       16 tile + 4 q + j; L = 9 for save_args, 8 for rsave / tang), so that a wave's tile is one contiguous
                                       KiB.  Rows per image are padded to a multiple of 16: every saved-state buffer of this precision
                                       holds batch * ceil16(n_pts) * L * 256 floats.  Point-major (batch, n_pts, L, 256) everywhere else. */

/* Number of floats of the packed weight image produced by e3dge_siren_pack_weights. */
int64_t e3dge_siren_packed_floats(void);

/*
 * Re-lays the SirenGenerator parameters (volume_renderer.py:158-166; FiLMSiren.weight/bias :91-104,
 * rgb_linear / sigma_linear :165-166) into the MFMA fragment-major image the render kernels stream
 * through LDS.  Call once per weight update.  All inputs row-major (out, in) as in the state dict:
 *   w_first (256,3)  b_first (256)            pts_linears.0
 *   w_hidden (7,256,256)  b_hidden (7,256)    pts_linears.1..7
 *   w_view (256,259)  b_view (256)            views_linears  (input = [features(256), viewdir(3)])
 *   w_rgb (3,256) b_rgb (3) ; w_sigma (1,256) b_sigma (1)
 * packed: e3dge_siren_packed_floats() floats.
 */
int e3dge_siren_pack_weights(float* packed, const float* w_first, const float* b_first,
                             const float* w_hidden, const float* b_hidden, const float* w_view,
                             const float* b_view, const float* w_rgb, const float* b_rgb,
                             const float* w_sigma, const float* b_sigma, e3dge_stream_t stream);

/*
 * FiLM parameters of all 9 layers for a batch of W+ codes
 * (FiLMSiren.gamma / .beta = LinearLayer(std_init=15,bias_init=30) / (std_init=0.25),
 *  volume_renderer.py:76-80,107-120):
 *   film[b,l,0,:] = 15  * (Wg_l styles[b,l] + bg_l) + 30
 *   film[b,l,1,:] = 0.25 * (Wb_l styles[b,l] + bb_l)
 * styles (batch, 9, 256); wg, wb (9,256,256); bg, bb (9,256); film (batch, 9, 2, 256).
 */
int e3dge_film_params(float* film, const float* styles, const float* wg, const float* bg,
                      const float* wb, const float* bb, int batch, e3dge_stream_t stream);

/* Inputs/outputs of one fused render launch; unused outputs may be NULL. */
typedef struct E3dgeRenderArgs {
    /* ---- inputs ---- */
    const float* packed;   /* from e3dge_siren_pack_weights                                      */
    const float* film;     /* (batch, 9, 2, 256) from e3dge_film_params                           */
    const float* c2w;      /* (batch, 3, 4) camera-to-world (cam_poses)                            */
    const float* focal;    /* (batch)                                                              */
    const float* near;     /* (batch)                                                              */
    const float* far;      /* (batch)                                                              */
    const float* t_vals;   /* (n_samples) -- VolumeFeatureRenderer.t_vals (:690-698)                */
    const float* tex_alpha;/* optional (batch,H,W,S,256) per-point texture FiLM alpha (:217-220)     */
    const float* tex_beta; /* optional, same shape                                                  */
    float sigmoid_beta;    /* renderer.sigmoid_beta (:663)                                         */
    float box_scale;       /* grid_warper scale = 2 / (2*dist_radius) (:720)                        */
    float mask_depth_thresh; /* 1.08 (:910)                                                        */
    int batch, height, width, n_samples;
    int res;               /* out_im_res used for the pixel-centre offset (:773-774)                */
    int force_background;  /* (:884-886)                                                           */
    int precision;         /* E3DGE_PREC_F32 or E3DGE_PREC_F16X3                                      */
    /* ---- outputs ---- */
    float* rgb;            /* (batch, 3, H, W)    gen_thumb_imgs (:888-890, permuted :1964)          */
    float* features;       /* (batch, 256, H, W)  (:894, :1967)                                     */
    float* xyz;            /* (batch, 3, H, W)    (:905, :1958)                                     */
    float* depth;          /* (batch, H, W)       (:907)                                            */
    float* mask;           /* (batch, H, W)       (:910)                                            */
    float* sdf;            /* (batch, H, W, S)    (:880)                                            */
    float* weights;        /* (batch, H, W, S)    hit_prob (:877,:885)                              */
    float* points;         /* (batch, H, W, S, 3) (:1231)                                           */
    float* rays_d;         /* (batch, H, W, 3)    (:782)                                            */
    float* viewdirs;       /* (batch, H, W, 3)    normalised (:1679)                                */
    float* dists;          /* (batch, H, W, S)    (:826-837)                                        */
    float* save_args;      /* training only, else NULL: (batch, H, W, S, 9, 256) pre-sine arguments of the 9 FiLM
                              layers, consumed by e3dge_siren_bwd                                        */
    /* ---- backbone hand-over between the two renders of one evaluated image (precision f16x3, inference; all NULL otherwise) ----
     * que_render_given_ref (e3dge_full_runner.py:185-317) renders the same rays twice: without and with the texture FiLM, which
     * enters behind the sdf head (volume_renderer.py:217-220).  Layers 0..7, the sdf head, alpha and the transmittance scan are
     * identical in both.  backbone_out: the first launch also writes its layer-7 output (e3dge_siren_backbone_bytes bytes).
     * backbone_in + weights_in (that launch's `weights` output): the second launch, same sizes / poses / film, reads them and
     * runs only texture FiLM -> view layer -> compositing; it produces rgb and features (+ ray geometry): sdf, weights, xyz,
     * depth, mask must be NULL there (the first launch's are the values).  Results are bit-identical to a full launch. */
    void* backbone_out;
    const void* backbone_in;
    const float* weights_in;
} E3dgeRenderArgs;

/*
 * Replaces VolumeFeatureRenderer.render -> render_rays -> run_network -> SirenGenerator.forward ->
 * volume_integration (volume_renderer.py:1666-1701, 1183-1287, 1052-1128, 168-264, 809-943) for the
 * inference configuration (offset_sampling, static_viewdirs, perturb=0, with_sdf, return_xyz):
 * ray generation, sample placement, the 9 FiLM-SIREN layers, both heads, SDF->alpha, transmittance
 * scan and all composites in ONE kernel; the (B,H,W,S,260) raw tensor never exists.
 * Requires n_samples >= 16 (or use e3dge_siren_points_fwd for un-composited queries).
 */
int e3dge_siren_render_fwd(const E3dgeRenderArgs* args, e3dge_stream_t stream);
/* bytes of the backbone record of a render launch with these sizes (0 if the sizes are not renderable) */
int64_t e3dge_siren_backbone_bytes(int batch, int height, int width, int n_samples);

/*
 * Replaces VolumeFeatureRenderer.run_network on an arbitrary point set
 * (volume_renderer.py:1052-1128; callers :925-930, :1916-1949, sample_uniform_grid :945-).
 * pts (batch, n_pts, 3) world-space (box warp applied inside); viewdirs (batch, n_pts, 3) or NULL (= 0).
 * Outputs (any may be NULL): sdf (batch, n_pts); raw (batch, n_pts, 260) = [rgb3, sdf1, feat256]
 * exactly as SirenGenerator.forward concatenates them (:259-261); save_args (batch, n_pts, 9, 256) as in
 * E3dgeRenderArgs (training only).
 */
int e3dge_siren_points_fwd(const float* packed, const float* film, const float* pts,
                           const float* viewdirs, float box_scale, int batch, int64_t n_pts,
                           float* sdf, float* raw, float* save_args, int precision, e3dge_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Training direction: gradient of a loss w.r.t. the renderer's styles (W+ latents), generator weights frozen.
 * Replaces autograd through SirenGenerator.forward (project/utils/volume_renderer.py:168-264) as the encoder
 * trainer drives it (project/trainer.py:728 loss.backward(); the generator is frozen at :1568).
 *
 *   args     (batch, n_pts, 9, 256)  pre-sine arguments saved by the forward launch (save_args)
 *   d_feat   (batch, n_pts, 256)     dL/d(view-layer features) per point, or NULL (= 0)
 *   d_rgb    (batch, n_pts, 3)       dL/d(rgb head output, pre-sigmoid), or NULL
 *   d_sdf    (batch, n_pts)          dL/d(sdf head output), or NULL
 *   wg, wb   (9, 256, 256)           the gamma / beta style-linear weights as given to e3dge_film_params
 *   partials  e3dge_siren_bwd_partial_floats(batch, n_pts) floats of scratch (need not be initialised)
 *   dfilm    (batch, 9, 2, 256) out  dL/d(gamma, beta)
 *   dstyles  (batch, 9, 256)    out  dL/d(styles)
 * precision: E3DGE_PREC_F32 (fp32 MFMA) or E3DGE_PREC_F16X3: every gradient operand is scaled per point by a power of
 * two into [1, 2), split into f16 hi + lo, three f16 MFMA products accumulated in fp32 -- same error as fp32.
 * Optional outputs / inputs (NULL = absent):
 *   d_pts (batch, n_pts, 3) out: dL/d(query points) = box_scale * W_0^T (gamma_0 * adj(a_0)) -- with tang/rsave this is
 *     the Hessian-vector product the reference obtains by keeping xyz in the graph of the surface normals
 *     (volume_renderer.py:921-930); box_scale as given to the forward launch.
 *   tex_alpha (batch, n_pts, 256): the forward pass applied the texture FiLM h8' = (alpha+1) h8 + beta (:217-220);
 *     d_tex_alpha, d_tex_beta (batch, n_pts, 256) out receive dL/dalpha, dL/dbeta (stage-2 training differentiates the
 *     second pass, e3dge_full_runner.py:185-317).  Not combinable with tang/rsave.
 * ---------------------------------------------------------------------------------------------------------------- */
int64_t e3dge_siren_bwd_partial_floats(int batch, int64_t n_pts);
typedef struct E3dgeSirenBwdArgs {
    const float* packed; const float* film; const float* args;
    const float* d_feat; const float* d_rgb; const float* d_sdf;
    const float* tang; const float* rsave;
    const float* wg; const float* wb;
    const float* tex_alpha;
    int batch; int precision;
    int64_t n_pts;
    float box_scale;
    float* partials; float* dfilm; float* dstyles;
    float* d_pts; float* d_tex_alpha; float* d_tex_beta;
    /* ABI 16 (renderer parameter gradients, see e3dge_siren_wgrad below; NULL = off): */
    float* d_lin;      /* (batch, n_pts, 9, 256) out, laid out like `args` (E3DGE_PREC_F16X3_G2: slab-major): g_l = gamma_l * dL/d a_l of
                          every layer and point.  Rows of padded points are not written. */
    float* lin_amax;   /* 9 amax buffers (9 * E3DGE_AMAX_FLOATS floats, zeroed by the caller): max |g_l| per layer */
} E3dgeSirenBwdArgs;
int e3dge_siren_bwd(const E3dgeSirenBwdArgs* args, e3dge_stream_t stream);

/* Eikonal term e = d sdf / d x (get_eikonal_term, volume_renderer.py:796-802) and its double backward.
 *   e3dge_siren_sdf_grad : from the saved arguments, e (batch, n_pts, 3) [world-space x: includes box_scale] and
 *                          rsave (batch, n_pts, 8, 256) = d sdf / d h_l, needed again if a loss on e is differentiated.
 *                          seed (batch, n_pts) scales r_7 per point, NULL = 1 (grad_outputs = ones, :799).
 *   e3dge_siren_tangent  : given v = dL/de (batch, n_pts, 3), the tangent arguments tang (batch, n_pts, 8, 256).
 * Passing tang + rsave to e3dge_siren_bwd / E3dgeRenderBwdArgs adds dL/d(styles) of the loss on e (the reference's
 * create_graph=True path) to the first-order gradient; NULL, NULL = no such loss. */
int e3dge_siren_sdf_grad(const float* packed, const float* film, const float* args, const float* seed,
                         float box_scale, int batch, int64_t n_pts, float* rsave, float* eik, int precision,
                         e3dge_stream_t stream);
int e3dge_siren_tangent(const float* packed, const float* film, const float* args, const float* v,
                        float box_scale, int batch, int64_t n_pts, float* tang, int precision, e3dge_stream_t stream);
/* ABI 13, precision E3DGE_PREC_F16X3_G2 only: the tangent pass in product form.  ta_l and r_l enter the second-order backward only as
 * ta_l * r_l (adj(a_l) -= sin(a_l) ta_l r_l, adj(gamma_l) += ta_l r_l cos(a_l) / gamma_l), so this launch reads rsave (the sdf
 * chain's r_l) beside the arguments and stores tr (batch, n_pts, 8, 256) = ta_l r_l; e3dge_siren_bwd / e3dge_siren_render_bwd in the
 * same precision take it as `tang` with `rsave` = NULL -- one 8-KB-per-point stream less in the longest kernel of the training step. */
int e3dge_siren_tangent_tr(const float* packed, const float* film, const float* args, const float* v, const float* rsave,
                           float box_scale, int batch, int64_t n_pts, float* tr, int precision, e3dge_stream_t stream);

/* Backward of e3dge_siren_render_fwd: volume_integration (volume_renderer.py:809-943) back to the per-point outputs
 * (one wave per ray), then the MLP chain above.  Gradient maps are ROW-MAJOR PER RAY (ray = (b*H + y)*W + x):
 *   d_rgb_map (rays,3)  d_feat_map (rays,256)  d_xyz_map (rays,3)  d_depth_map (rays)  d_sdf (rays,S); any may be NULL.
 * args/sdf/dists/points/weights are the forward launch's outputs (save_args, sdf, dists, points, weights).
 * d_rgb_pts (rays,S,3) and d_sdf_pts (rays,S) are scratch the caller provides; partials as for e3dge_siren_bwd with
 * n_pts = H*W*S.  sigmoid_beta and the generator weights get no gradient (frozen in encoder training).
 * d_weights (rays,S): gradient arriving at the compositing weights (`hit_prob`, read by cycle_runner.py:134), or NULL.
 * tex_alpha / d_tex_alpha / d_tex_beta (rays,S,256): as in E3dgeSirenBwdArgs, for the second (texture-FiLM) pass. */
typedef struct E3dgeRenderBwdArgs {
    const float* packed; const float* film; const float* args; const float* sdf; const float* dists;
    const float* points; const float* weights; const float* t_vals; const float* near; const float* far;
    const float* wg; const float* wb;
    const float* d_rgb_map; const float* d_feat_map; const float* d_xyz_map; const float* d_depth_map; const float* d_sdf;
    const float* tang; const float* rsave;
    const float* d_weights; const float* tex_alpha;
    float sigmoid_beta;
    int batch, height, width, n_samples, force_background;
    int precision;           /* E3DGE_PREC_F32 or E3DGE_PREC_F16X3 (block-scaled split-f16 GEMMs, fp32 accumulate) */
    float* d_rgb_pts; float* d_sdf_pts; float* partials;
    float* dfilm; float* dstyles;
    float* d_tex_alpha; float* d_tex_beta;
    int phase;               /* ABI 14: 0 = both launches; 1 = only the backward of the compositing (reads the d_*_map / d_sdf / d_weights inputs, writes
                                d_rgb_pts / d_sdf_pts; needs neither tang nor rsave); 2 = only the network backward on what phase 1 left in those buffers.
                                Lets a caller run phase 1 beside e3dge_siren_tangent(_tr) on another stream and wait for the tangent before phase 2. */
    /* ABI 16 (NULL = off): d_lin, lin_amax as in E3dgeSirenBwdArgs (phase 0 / 2), with n_pts = H*W*S;
     * d_sigmoid_beta (rays) out (phase 0 / 1): each ray's share of dL/d sigmoid_beta -- sum them for the gradient. */
    float* d_lin; float* lin_amax; float* d_sigmoid_beta;
} E3dgeRenderBwdArgs;
int e3dge_siren_render_bwd(const E3dgeRenderBwdArgs* args, e3dge_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * ABI 16: gradients of the SIREN renderer's own weights (the reference trains them: Generator.train_renderer =
 * not freeze_renderer, stylesdf_model.py:812; PTI fine-tunes the whole generator, projectors.py:447-640).
 * Precision E3DGE_PREC_F16X3_G2 only: the backward launches above return E3DGE_ERR_INVALID_ARG for any other precision when
 * d_lin is set.  First order only (no tang / rsave, no texture FiLM pass).
 * Inputs: `args` (the forward's saved arguments) and `d_lin` / `lin_amax` (the backward's new outputs), both (batch, n_pts, 9, 256)
 * slab-major; d_sdf (batch, n_pts) and d_rgb (batch, n_pts, 3): the gradients at the head outputs (d_sdf_pts / d_rgb_pts of a
 * render backward, the caller's d_sdf / d_rgb of e3dge_siren_bwd; NULL = 0); pts (batch, n_pts, 3) the un-warped points and
 * box_scale as given to the forward; viewdirs: (batch, n_pts / samples, 3) per ray (samples = S of a render), per point
 * (samples = 1), or NULL (= 0, run_network without view directions).
 * Outputs (all written, never accumulated into):
 *   d_w[8]        (8, 256, 256)  dL/d W_l of pts_linears.1..7 and, last, the first 256 columns of views_linears.weight
 *   d_w_view_dirs (256, 3)       dL/d views_linears.weight[:, 256:259]
 *   d_w_first     (256, 3)       dL/d pts_linears.0.weight
 *   d_w_sigma (256), d_b_sigma (1), d_w_rgb (3, 256), d_b_rgb (3)   the two heads
 * The FiLM layers' own biases and the gamma / beta style-linear parameters follow from dfilm on the host side.
 * ws: e3dge_siren_wgrad_ws_floats(batch, n_pts) floats of scratch, 16-B aligned (args and d_lin too).  Fixed-order split-K folds: bit-reproducible. */
typedef struct E3dgeSirenWgradArgs {
    const float* args; const float* d_lin; const float* lin_amax;
    const float* d_sdf; const float* d_rgb; const float* pts; const float* viewdirs;
    float* d_w; float* d_w_view_dirs; float* d_w_first; float* d_w_sigma; float* d_b_sigma; float* d_w_rgb; float* d_b_rgb;
    float* ws;
    int64_t ws_floats, n_pts;
    int batch, samples, precision;
    float box_scale;
} E3dgeSirenWgradArgs;
int64_t e3dge_siren_wgrad_ws_floats(int batch, int64_t n_pts);
int e3dge_siren_wgrad(const E3dgeSirenWgradArgs* args, e3dge_stream_t stream);



/* ------------------------------------------------------------------------------------------------------------------
 * Local-feature -> texture-FiLM head (second renderer pass): out = W_s x + W_1 relu(W_0 relu(x) + b_0) + b_1,
 * (alpha, beta) = split(out, 256).  Replaces ResnetBlockFC.forward (project/models/helper_modules/resnetfc.py:49-58) as
 * netLocal.local_feat_to_tex_modulations_linear (vendor/pifu/lib/model/HGPIFuGANNetResidualInputResnetFC.py:84-93), called
 * in SirenLocalGlobal.forward_backbone (project/utils/volume_renderer.py:327-336).
 *   w0 (cin, cin), b0 (cin)   fc_0        w1 (512, cin), b1 (512)   fc_1        ws (512, cin)   shortcut (no bias)
 *   feats (n_pts, cin) row-major, cin <= 320        alpha, beta (n_pts, 256) out -- the tex_alpha / tex_beta inputs of
 *   e3dge_siren_render_fwd.  Split-f16 contraction with per-point block scaling, fp32 accumulate.
 * ---------------------------------------------------------------------------------------------------------------- */
int64_t e3dge_resblock_packed_floats(void);
int e3dge_resblock_pack_weights(float* packed, const float* w0, const float* b0, const float* w1, const float* b1,
                                const float* ws, int cin, e3dge_stream_t stream);
int e3dge_tex_modulations_fwd(const float* packed, const float* feats, int cin, int64_t n_pts,
                              float* alpha, float* beta, e3dge_stream_t stream);
/* Data gradient of the head (round 5): d feats = W_s^T d out + (W_0^T ((W_1^T d out) [net > 0])) [x > 0], d out = [d alpha | d beta] -- what
 * autograd runs through ResnetBlockFC (helper_modules/resnetfc.py:49-58) for the stage-2 losses (e3dge_full_runner.py:185-317); the reference
 * has no hand-written backward.  One launch, split-f16 contractions like the forward; net is recomputed (signs only).
 *   packed_bwd   e3dge_resblock_bwd_packed_floats() floats from e3dge_resblock_bwd_pack_weights (W_0, W_1^T, W_s^T, W_0^T images + b_0)
 *   d_alpha, d_beta (n_pts, 256), 16-byte aligned     d_feats (n_pts, cin) out
 *   ws           e3dge_tex_modulations_bwd_ws_floats(n_pts) floats, 16-byte aligned; on return ws[0 .. n_pts * 320) holds d net = d L / d (fc_0
 *                output) as (n_pts, 320) rows (columns >= cin are zero) -- the operand of the parameter gradients (e3dge_wgrad)
 *   net_out      NULL, or (n_pts, 320) rows receiving net = fc_0(relu(x)) as recomputed (the input of fc_1's parameter gradient, before its relu)
 *   amax4        (ABI 14) NULL, or 4 x E3DGE_AMAX_FLOATS floats, zeroed by the caller: amax buffers of feats, [d alpha | d beta], d net and net (the
 *                last only with net_out) -- the operand scales e3dge_wgrad needs, from values this launch holds anyway */
int64_t e3dge_resblock_bwd_packed_floats(void);
int e3dge_resblock_bwd_pack_weights(float* packed_bwd, const float* w0, const float* b0, const float* w1, const float* ws, int cin,
                                    e3dge_stream_t stream);
int64_t e3dge_tex_modulations_bwd_ws_floats(int64_t n_pts);
int e3dge_tex_modulations_bwd(const float* packed_bwd, const float* feats, int cin, int64_t n_pts, const float* d_alpha, const float* d_beta,
                              float* d_feats, float* ws, float* net_out, float* amax4, e3dge_stream_t stream);
/* The head INSIDE the second render pass's data flow (ABI 11; SURVEY.md 8 f1 as specified: (alpha, beta) never materialise):
 * feats (batch, height, width, n_samples, cin) -> h' = (alpha + 1) h8 + beta, where h8 is the layer-7 output that render
 * pass #1 left in `backbone_in` (e3dge_siren_render_fwd backbone_out, e3dge_siren_backbone_bytes bytes) -- the FiLM step of
 * volume_renderer.py:217-220 in siren16_kernel's operation order, bit-identical to applying tex_alpha / tex_beta there.
 * `backbone_out` (same size and layout, zero-filled once by the caller: padding slabs are never written) is what pass #2 then
 * takes as its backbone_in, WITHOUT tex_alpha / tex_beta.  Records are limited to 4 GiB (32-bit offsets). */
int e3dge_tex_film_fwd(const float* packed, const float* feats, int cin, int batch, int height, int width, int n_samples,
                       const void* backbone_in, void* backbone_out, e3dge_stream_t stream);


/* ------------------------------------------------------------------------------------------------------------------
 * Per-point query of the local branch's feature maps (project/trainers/E3DGE/e3dge_full_runner.py:185-317).
 *   e3dge_local_query: replaces HGPIFuNetGAN.query(return_feat_only / return_projection_only / im_feat=...)
 *       (vendor/pifu/lib/model/HGPIFuGANNet.py:85-151) = perspective projection (vendor/pifu/lib/geometry.py:101-129; the
 *       sign of the depth is decided by the first point of the first sample, as there) + y flip + in-image mask + bilinear
 *       gather index() (geometry.py:64-80: grid_sample, zeros padding, align_corners=False).
 *       pts (batch, n_pts, 3) world space; calibs (batch, 3, 4); fmap_nhwc (batch, fh, fw, channels) CHANNEL-LAST, or NULL
 *       for projection / mask only.  Features go to out[(b*n_pts + n) * ld + col_off + c]; in_img (1.0 / 0.0) to
 *       in_img[(b*n_pts + n) * mask_ld + mask_off] (NULL = not wanted; may point into the same rows as `out`);
 *       proj (batch, n_pts, 3) = (x, flipped y, depth) or NULL.  channels %% 4 == 0.
 *   e3dge_pos_encoding: PosEncoding.forward (project/utils/misc_utils.py:148-185, logscale): pts (n_pts, 3) ->
 *       out[n * ld + col_off + ...] = [x, sin(2^0 x), cos(2^0 x), ..., sin(2^(F-1) x), cos(2^(F-1) x)], 3 (2F+1) columns.
 * ---------------------------------------------------------------------------------------------------------------- */
int e3dge_local_query(float* out, int ld, int col_off, float* in_img, int mask_ld, int mask_off, float* proj,
                      const float* pts, const float* calibs, const float* fmap_nhwc, int batch, int64_t n_pts, int channels,
                      int fh, int fw, e3dge_stream_t stream);
/* Backward of the gather (ABI 11; reference: project/models/op/grid_sample_gradfix.py:52-89 behind HGPIFuNetGAN.query's index()):
 * d_fmap_nhwc (batch, fh, fw, channels), ZERO-FILLED by the caller, receives the bilinear scatter of d_out[..., col_off:col_off+C]
 * (atomic adds); d_pts (batch, n_pts, 3) the gradient through the sampling position (projection included).  Either may be NULL. */
int e3dge_local_query_bwd(float* d_fmap_nhwc, float* d_pts, const float* d_out, int ld, int col_off, const float* pts,
                          const float* calibs, const float* fmap_nhwc, int batch, int64_t n_pts, int channels, int fh, int fw,
                          e3dge_stream_t stream);
/* ABI 14 (round 6): the same with the points walked in the order of a counting sort by (image, pixel of the top-left corner) -- for gathers
 * whose consecutive points do NOT share pixels (another view's rays: every sample of the reference-view gather lands on its own pixel, and the
 * scatter is then one device-scope atomic instruction per corner, channel group and point).  ws: e3dge_local_query_sort_ws_ints(...) ints of
 * scratch (keys, order, ranks, bin counters); five launches (zero, key + count + rank, scan, scatter, the gather's backward on `order`).  Sums within a pixel
 * arrive in an order that varies from run to run, like the atomics' of the unsorted form. */
int64_t e3dge_local_query_sort_ws_ints(int batch, int64_t n_pts, int fh, int fw);
int e3dge_local_query_bwd_sorted(float* d_fmap_nhwc, float* d_pts, const float* d_out, int ld, int col_off, const float* pts,
                                 const float* calibs, const float* fmap_nhwc, int batch, int64_t n_pts, int channels, int fh, int fw,
                                 int32_t* ws, int64_t ws_ints, e3dge_stream_t stream);
int e3dge_pos_encoding(float* out, int ld, int col_off, const float* pts, int64_t n_pts, int n_freqs, e3dge_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Per-image reconstruction metrics in one pass (the scalars the sharded evaluation all-gathers):
 * replaces the MSE / L1 / PSNR / SSIM part of Loss.calc_2d_rec_loss (project/losses/builder.py:130-184; SSIM = kornia
 * ssim_loss with a 5x5 Gaussian window, sigma 1.5, reflect padding, max_val as given -- the reference passes its [-1,1]
 * images with max_val = 1).  pred, gt (batch, channels, H, W); scratch e3dge_image_metrics_scratch_floats() floats;
 * sums (batch, 4) = [sum (p-g)^2, sum |p-g|, sum clamp((1-ssim)/2, 0, 1), element count] per image.
 * ---------------------------------------------------------------------------------------------------------------- */
int64_t e3dge_image_metrics_scratch_floats(int batch, int channels, int height, int width);
int e3dge_image_metrics(float* sums, float* scratch, const float* pred, const float* gt, int batch, int channels,
                        int height, int width, float max_val, e3dge_stream_t stream);
/* The eight columns builder.py:174-184 reports, from those sums (means over the whole batch tensor, as the reference's
 * losses are), in one launch: row (8) = [loss_l2 = MSE, loss_id, loss_lpips, loss, mae, PSNR of the images rescaled to
 * [0,1], SSIM = 1 - ssim_loss, ID_SIM = 1 - loss_id].  lpips_per_image: NULL or (batch), e3dge_lpips_forward's per_image;
 * loss_lpips = (sum_b lpips_per_image[b]) / batch, the same fp32 sum as its mean_out.  id_loss: NULL or a device scalar,
 * e3dge_id_loss's loss.  A NULL pointer reports its column as the reference does with that lambda at 0 (:145, :158-163:
 * loss_lpips = 0; loss_id = 0, ID_SIM = 1) and adds no term to loss, whatever the lambda (an infinite one included).
 * loss = fl(l2_lambda MSE), + fl(vgg_lambda loss_lpips) when lpips_per_image is given, + fl(id_lambda loss_id) when id_loss
 * is given, in that fp32 order (builder.py:168).
 * ABI 17: this one entry replaces e3dge_image_metric_row(row, sums, batch, l2_lambda), e3dge_image_metric_row_lpips and
 * e3dge_image_metric_row_full; it reproduces the first two bit for bit and the third wherever that one added an exact zero. */
int e3dge_image_metric_row(float* row, const float* sums, const float* lpips_per_image, const float* id_loss, int batch,
                           float l2_lambda, float vgg_lambda, float id_lambda, e3dge_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * LPIPS-alex perceptual distance (csrc/lpips.hip).  Additions to ABI 16.  No allocation, no synchronisation.  Replaces
 * LPIPS.forward (project/losses/lpips/lpips.py:33-39) with BaseNet.z_score / forward and AlexNet (networks.py:52-65, 80-89)
 * and normalize_activation (utils.py:6-9), as calc_2d_rec_loss calls it (project/losses/builder.py:143, 168, 176):
 *   z = (x - mean) / std per channel (zero padding applies to z);
 *   conv 3->64 k11 s4 p2, relu [tap 1], maxpool 3 s2 (floor), conv 64->192 k5 p2, relu [tap 2], maxpool 3 s2, conv 192->384 k3 p1,
 *   relu [tap 3], conv 384->256 k3 p1, relu [tap 4], conv 256->256 k3 p1, relu [tap 5];
 *   f^ = f / (sqrt(sum_c f^2 + 1e-8) + 1e-10);  d_l[b] = mean_{h,w} sum_c lin_l[c] (x^_c - y^_c)^2;  per_image[b] = sum_l d_l[b].
 * fp32 throughout (v_mfma_f32_16x16x4_f32); every sum is folded in a fixed order: bit-reproducible, and an image pair's value does
 * not depend on the batch it is in.
 *
 * e3dge_lpips_packed_floats  floats of the packed weight image: the five conv weights in MFMA A-fragment order (K padded to a
 *                            multiple of 32 with zeros), the five biases, the five lin rows.
 * e3dge_lpips_pack_weights   w, b, lin: HOST arrays of five device pointers -- w[l] (C_out, C_in, k, k) contiguous as torchvision's
 *                            features.{0,3,6,8,10}.weight, b[l] (C_out), lin[l] (C_out of layer l) the 1x1 weight of lin layer l
 *                            (the renamed keys of utils.py:31-37).  Fifteen small launches (conv_igemm.h's packers); call once per weight update.
 * e3dge_lpips_ws_bytes       workspace bytes of a forward (-1: batch < 1 or height / width < 31, the smallest image for which every
 *                            layer has an output).
 * e3dge_lpips_forward        x, y (batch, 3, height, width) fp32 contiguous.  per_image (batch); per_layer NULL or (batch, 5) = d_l[b];
 *                            mean_out NULL or (1) = (sum_b per_image[b]) / batch, summed in ascending b in fp32 -- the scalar
 *                            lpips.py:39 returns; taps[l] NULL or (2 batch, C_l, H_l, W_l): the normalised features of x (images
 *                            0..batch-1) and y (batch..2 batch-1).  Nine launches.  Fails before any launch on a null required pointer,
 *                            batch < 1, height or width < 31, ws_bytes below e3dge_lpips_ws_bytes().
 * per_image is what e3dge_image_metric_row takes as lpips_per_image.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct E3dgeLpipsArgs {
    const float* packed; const float* x; const float* y;
    int32_t batch, height, width, reserved;
    float mean[3], std[3];            /* net.mean, net.std of the reference module (networks.py:41-46) */
    float* per_image; float* per_layer; float* mean_out;
    float* taps[5];
    void* ws;
    int64_t ws_bytes;
} E3dgeLpipsArgs;
int64_t e3dge_lpips_packed_floats(void);
int e3dge_lpips_pack_weights(float* packed, const float* const* w, const float* const* b, const float* const* lin, e3dge_stream_t stream);
int64_t e3dge_lpips_ws_bytes(int batch, int height, int width);
int e3dge_lpips_forward(const E3dgeLpipsArgs* args, e3dge_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * LPIPS backward (csrc/lpips_bwd.h): the gradient of per_image[b] with respect to x, y or both; the AlexNet and lin weights
 * are frozen, as the reference freezes them.  Additions to ABI 16.  No allocation, no synchronisation, no atomics: eight
 * launches whatever the batch, bit-reproducible, and an image's gradient does not depend on the batch it is in.
 *
 * The workspace of e3dge_lpips_forward is therefore also an OUTPUT of the forward: after the call it holds the five post-ReLU
 * conv outputs and the two pooled maps of the 2 batch images, and a caller that wants the gradient keeps it untouched until
 * e3dge_lpips_backward has run (fwd_ws, fwd_ws_bytes; same batch, height and width).  Nothing of the forward is recomputed
 * but the channel norms.
 *
 * e3dge_lpips_packed_t_floats floats of the transposed weight image: W_l^T with flipped taps for conv 2..5 (M = C_in, K = (co, r, s)
 *                            padded to a multiple of 32) in MFMA A-fragment order, then conv 1 as (3, 64, 11, 11).  A buffer of
 *                            its own; the forward image is unchanged.
 * e3dge_lpips_pack_weights_t w: HOST array of the five device pointers e3dge_lpips_pack_weights takes.  Five launches per weight update.
 * e3dge_lpips_bwd_ws_bytes   workspace bytes of a backward for `batch` gradient images (both = 0) or 2 batch (both != 0); -1 as
 *                            e3dge_lpips_ws_bytes.
 * e3dge_lpips_backward       upstream (batch) = dL / d per_image[b] (for the scalar mean: dL / d mean / batch).  grad_x, grad_y: NULL
 *                            or (batch, 3, height, width), at least one; every element is written.  gpre[l]: NULL or (n, C_l, H_l,
 *                            W_l), the gradient at conv l + 1's pre-activation of the images that get a gradient, x's first
 *                            (n = batch or 2 batch).  std as in the forward.  Fails before any launch on a null required pointer
 *                            ("null"), both gradients NULL, batch < 1 ("batch"), height or width < 31, a zero std, or either
 *                            workspace too small ("workspace").
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct E3dgeLpipsBwdArgs {
    const float* packed;              /* the forward image (its lin rows are read) */
    const float* packed_t;            /* e3dge_lpips_pack_weights_t */
    const void* fwd_ws;               /* what a completed e3dge_lpips_forward of the same batch / height / width left behind */
    int64_t fwd_ws_bytes;
    int32_t batch, height, width;
    float std[3];
    const float* upstream;
    float* grad_x; float* grad_y;
    float* gpre[5];
    void* ws;
    int64_t ws_bytes;
} E3dgeLpipsBwdArgs;
int64_t e3dge_lpips_packed_t_floats(void);
int e3dge_lpips_pack_weights_t(float* packed_t, const float* const* w, e3dge_stream_t stream);
int64_t e3dge_lpips_bwd_ws_bytes(int batch, int height, int width, int both);
int e3dge_lpips_backward(const E3dgeLpipsBwdArgs* args, e3dge_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * ArcFace identity term, forward (csrc/idnet.hip).  Additions to ABI 16.  No allocation, no synchronisation, no atomics;
 * bit-reproducible, and an image's embedding does not depend on its position in the batch or on the batch size.  Replaces
 * IDLoss.forward (project/losses/id_loss.py:23-55) with Backbone(112, 50, 'ir_se') in eval form (models/encoders/
 * model_irse.py:8-51, models/helper_modules/helpers.py:83-224) and the pooling of builder.py:157-160.
 *
 * Order of the pointer arrays of E3dgeIdnetPackSrc (unit = one of the 24 bottleneck_IR_SE, in body order):
 *   conv_w    [0] input_layer.0; [1 + 2u], [2 + 2u] unit u's res_layer.1 and res_layer.3; [49..51] shortcut_layer.0 of units 3, 7, 21 (unit 0 is
 *             64 -> 64: its shortcut is the strided pick)
 *   bn_*      [0] input_layer.1; [1 + 2u], [2 + 2u] unit u's res_layer.0 and res_layer.4; [49..51] shortcut_layer.1 of those units;
 *             [52] output_layer.0 (BatchNorm2d); [53] output_layer.4 (BatchNorm1d).  weight = gamma, bias = beta, running mean / var
 *   prelu     [0] input_layer.2; [1 + u] unit u's res_layer.2
 *   se_fc1/2  unit u's res_layer.5.fc1 (C / 16, C) and fc2 (C, C / 16);  head_w (512, 25088), head_b (512): output_layer.3
 *
 * e3dge_idnet_packed_floats  floats of the packed image: the 52 conv weights in MFMA A-fragment order (K = (ci, r, s) padded to a
 *                            multiple of 32), every BatchNorm as per-channel pairs (a, b) with a = gamma / sqrt(var + 1e-5),
 *                            b = beta - mean a, PReLU slopes, SE matrices, the head's matrix and bias.
 * e3dge_idnet_pack_weights   src: HOST struct of device pointers.  Re-run after a weight update.
 * e3dge_idnet_ws_bytes       workspace bytes of an embed of n_images (-1: n_images < 1 or too large).
 * e3dge_idnet_embed          images[s] (n_per_set, 3, height, width) fp32 contiguous, s < n_sets (1..3); image s * n_per_set + i of
 *                            the batch is images[s][i].  height = width = 256: crop [35:223, 32:220], adaptive average to 112 x 112;
 *                            any other size: the 256 x 256 adaptive average first, each value rounded to fp32.  embeddings
 *                            (n, 512), unit L2 norm.  taps[t] NULL or: the network input (n, 3, 112, 112), the input layer's output,
 *                            the outputs of units 0, 3, 7, 21, 23, the head's output before the normalisation (n, 512).  103
 *                            launches without taps.  Fails before any launch on a null required pointer ("null"),
 *                            n_per_set < 1 or n_sets outside 1..3 ("n_"), height or width < 1, ws_bytes too small ("workspace").
 * e3dge_id_loss              y_hat, y, x (batch, 512) embeddings.  dots (batch, 3) = [y_hat.y, y_hat.x, y.x] per sample; loss =
 *                            (sum_b 1 - dots[b][0]) / batch in fp32, sim_improvement = (sum_b dots[b][0] - dots[b][2]) / batch in
 *                            double, both in sample order (NULL: not written).  One launch.
 * e3dge_idnet_conv_tiles     pixel tiles per (image, channel) plane of e3dge_idnet_conv's plane sums (-1: bad sizes).
 * e3dge_idnet_conv           debug entry: one convolution of the family.  in (n, cin, height, width), w (cout, cin, ksize, ksize)
 *                            with ksize 1 (pad 0) or 3 (pad 1), stride 1 or 2, cout a multiple of 64.  wfrag: scratch of
 *                            cout * roundup(cin ksize^2, 32) floats for the A-fragment image.  in_ab NULL or (cin, 2): x <- a x + b
 *                            on in-image elements (padding stays 0); epi_ab NULL or (cout, 2); slope NULL or (cout): PReLU after
 *                            the affine; plane NULL or (n, cout, tiles) partial sums of the stored plane.  Two launches.
 * e3dge_id_loss's loss is what e3dge_image_metric_row takes as id_loss.
 * ---------------------------------------------------------------------------------------------------------------- */
#define E3DGE_IDNET_CONVS 52
#define E3DGE_IDNET_BNS 54
#define E3DGE_IDNET_UNITS 24
#define E3DGE_IDNET_TAPS 8
typedef struct E3dgeIdnetPackSrc {
    const float* conv_w[E3DGE_IDNET_CONVS];
    const float* bn_weight[E3DGE_IDNET_BNS]; const float* bn_bias[E3DGE_IDNET_BNS];
    const float* bn_mean[E3DGE_IDNET_BNS]; const float* bn_var[E3DGE_IDNET_BNS];
    const float* prelu[E3DGE_IDNET_UNITS + 1];
    const float* se_fc1[E3DGE_IDNET_UNITS]; const float* se_fc2[E3DGE_IDNET_UNITS];
    const float* head_w; const float* head_b;
} E3dgeIdnetPackSrc;
typedef struct E3dgeIdnetArgs {
    const float* packed;
    const float* images[3];
    int32_t n_per_set, n_sets, height, width;
    float* embeddings;
    float* taps[E3DGE_IDNET_TAPS];
    void* ws;
    int64_t ws_bytes;
} E3dgeIdnetArgs;
typedef struct E3dgeIdLossArgs {
    const float* y_hat; const float* y; const float* x;
    int32_t batch, reserved;
    float* dots; float* loss; float* sim_improvement;
} E3dgeIdLossArgs;
int64_t e3dge_idnet_packed_floats(void);
int e3dge_idnet_pack_weights(float* packed, const E3dgeIdnetPackSrc* src, e3dge_stream_t stream);
int64_t e3dge_idnet_ws_bytes(int n_images);
int e3dge_idnet_embed(const E3dgeIdnetArgs* args, e3dge_stream_t stream);
int e3dge_id_loss(const E3dgeIdLossArgs* args, e3dge_stream_t stream);
int e3dge_idnet_conv_tiles(int cout, int height, int width, int ksize, int stride);
int e3dge_idnet_conv(float* out, const float* in, const float* w, float* wfrag, const float* in_ab, const float* epi_ab,
                     const float* slope, float* plane, int n, int cin, int cout, int height, int width, int ksize, int stride,
                     e3dge_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * ArcFace identity term, backward (csrc/idnet_bwd.h): the gradient of the loss with respect to the y_hat images; the network is
 * frozen, as the reference freezes it.  Additions to ABI 16.  No allocation, no synchronisation, no atomics; bit-reproducible,
 * and an image's gradient does not depend on the batch it is in or on its position in it.
 *
 * e3dge_idnet_packed_t_floats floats of the transposed weight image: for each of the 52 convolutions W^T with flipped taps
 *                            (M = C_in padded to 16, K = (co, r, s) padded to a multiple of 32) in MFMA A-fragment order.  A
 *                            buffer of its own; the forward image is unchanged.
 * e3dge_idnet_pack_weights_t src: the struct e3dge_idnet_pack_weights takes (only conv_w is read).  Re-run after a weight update.
 * e3dge_idnet_saved_bytes    bytes of the state the saving forward keeps for n_saved images (-1: n_saved outside 1..4096): per
 *                            image the 25 PReLU branches as bytes (3,713,024), the 24 `res` tensors (BN2 output before the
 *                            gate; 1,781,248 floats), the gates, the SE hidden activations, and the head's v, f and |v|.
 * e3dge_idnet_embed_save     e3dge_idnet_embed (net: same fields, same launches, bit-identical embeddings and taps) that also
 *                            fills `saved` for the leading n_saved images of the batch (set 0 first).  1 <= n_saved <=
 *                            n_per_set * n_sets.  Fails like e3dge_idnet_embed, and on a null or too small `saved` ("saved").
 * e3dge_idnet_bwd_ws_bytes   workspace bytes of a backward of n images of height x width (-1: bad n or size).
 * e3dge_idnet_backward       saved: what e3dge_idnet_embed_save left for n_saved = n images of the same height and width.
 *                            grad_embeddings (n, 512) = dL / d f (for the loss term: -u_b f_y[b], u_b = dL / d(1 - dot_b)).
 *                            grad_images (n, 3, height, width): every element is written (exact zeros outside the crop's
 *                            pre-image).  gstage[t]: NULL or the gradient at tap t of E3dgeIdnetArgs (the head's is the
 *                            gradient at v, before the normalisation).  masks[i]: NULL or bytes shaped like PReLU i's input
 *                            ([0] input layer, [1 + u] unit u) that receive 1 where the saved branch is the positive one.
 *                            104 launches without gstage and masks.  Fails before any launch on a null required pointer
 *                            ("null"), n < 1 ("n="), height or width < 1, saved_bytes too small ("saved") or ws_bytes too
 *                            small ("workspace").
 * e3dge_idnet_conv_bwd       debug entry: one data gradient of the family.  g (n, cout, OH, OW) with OH = (height - 1) / stride
 *                            + 1, w (cout, cin, ksize, ksize), ksize 1 (pad 0) or 3 (pad 1), stride 1 or 2; out (n, cin,
 *                            height, width) = (conv^T g) * factor + addend.  wfrag_t: scratch of roundup(cin, 16) * roundup(cout
 *                            ksize^2, 32) floats.  in_ab NULL or (n, cout, 2): g <- a g + b per (image, channel) on in-image
 *                            elements.  factor: mask (n, cin, height, width bytes) with slope (cin): 1 where the byte is set,
 *                            slope[c] elsewhere; or scale (cin): scale[c]; both NULL: 1.  addend NULL or (n, cin, height,
 *                            width).  Two launches.
 * e3dge_idnet_prep_bwd       debug entry: the adjoint of the crop and the adaptive averages.  grad_net_in (n, 3, 112, 112) ->
 *                            grad_images (n, 3, height, width), every element written.  One launch.
 * ---------------------------------------------------------------------------------------------------------------- */
#define E3DGE_IDNET_PRELUS 25
typedef struct E3dgeIdnetSaveArgs {
    E3dgeIdnetArgs net;
    void* saved;
    int64_t saved_bytes;
    int32_t n_saved, reserved;
} E3dgeIdnetSaveArgs;
typedef struct E3dgeIdnetBwdArgs {
    const float* packed;              /* the forward image (BN pairs, slopes and SE matrices are read) */
    const float* packed_t;            /* e3dge_idnet_pack_weights_t */
    const void* saved;                /* e3dge_idnet_embed_save with n_saved = n */
    int64_t saved_bytes;
    int32_t n, height, width, reserved;
    const float* grad_embeddings;
    float* grad_images;
    float* gstage[E3DGE_IDNET_TAPS];
    unsigned char* masks[E3DGE_IDNET_PRELUS];
    void* ws;
    int64_t ws_bytes;
} E3dgeIdnetBwdArgs;
int64_t e3dge_idnet_packed_t_floats(void);
int e3dge_idnet_pack_weights_t(float* packed_t, const E3dgeIdnetPackSrc* src, e3dge_stream_t stream);
int64_t e3dge_idnet_saved_bytes(int n_saved);
int e3dge_idnet_embed_save(const E3dgeIdnetSaveArgs* args, e3dge_stream_t stream);
int64_t e3dge_idnet_bwd_ws_bytes(int n, int height, int width);
int e3dge_idnet_backward(const E3dgeIdnetBwdArgs* args, e3dge_stream_t stream);
int e3dge_idnet_conv_bwd(float* out, const float* g, const float* w, float* wfrag_t, const float* in_ab, const unsigned char* mask,
                         const float* slope, const float* scale, const float* addend, int n, int cin, int cout, int height, int width,
                         int ksize, int stride, e3dge_stream_t stream);
int e3dge_idnet_prep_bwd(float* grad_images, const float* grad_net_in, int n, int height, int width, e3dge_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Surface extraction, device half: replaces align_volume (project/utils/mesh_utils.py:17-44; called on the rendered
 * 128^3 SDF volume at volume_renderer.py:1706, before the CPU marching cubes).  volume, out (batch, height, width, depth,
 * channels), not aliased; xs (width), ys (height), zs (depth) = linspace(-1, 1, n) and coef (depth) = linspace(far / near,
 * 1, depth) as the caller's torch.linspace produced them.  out[b, y, x, z] = trilinear border-clamped lookup
 * (grid_sample, align_corners) at (xs[x] coef[z], ys[y] coef[z], zs[z]), or 1 where that point leaves [-1, 1]^3.
 * ---------------------------------------------------------------------------------------------------------------- */
int e3dge_align_volume(float* out, const float* volume, const float* xs, const float* ys, const float* zs, const float* coef,
                       int batch, int height, int width, int depth, int channels, e3dge_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Surface extraction, marching cubes: replaces the CPU step after align_volume, the reference's
 * _extract_mesh_with_marching_cubes (project/utils/volume_renderer.py:1733-1758, the same code as project/utils/mesh_utils.py:48-70):
 *     verts, faces = skimage.measure.marching_cubes(sdf[0, ..., 0].permute(1, 0, 2), 0)
 *     verts[:, a] = (verts[:, a] / n_a - 0.5) * 0.24,  n = (w, h, d);  verts[:, 2] *= -1;  verts[:, 1] *= -1
 * The volume is read through strides in skimage's axes (x, y, z) = the (w, h, d) axes of aligned_sdf (b, h, w, d, c): value (x, y, z) at
 * sdf[x * sx + y * sy + z * sz] (strides in floats); nx, ny, nz >= 2 and nx * ny * nz <= 2^31 / E3DGE_MC_MAX_TRIS - 1.
 *   vertices  exactly one per grid edge whose end points straddle 0 (a value > 0 is positive, 0 counts as negative); on the edge from
 *             the lower corner a at index i to b the coordinate is float32(i + t), t = (0 - a) / (b - a) in double (skimage's own
 *             values; Lewiner's extra cell-interior vertices are not made).  scene != 0: then the transform above in fp32, in that order.
 *             Order: by point p = (x * ny + y) * nz + z, then the point's +x, +y, +z edge.
 *   faces     int32 vertex indices, wound as skimage's default gradient_direction='descent' (the right-hand normal points to the positive
 *             side); watertight and consistently oriented, degenerate triangles kept.  Order: by cell (numbered by its lowest point p),
 *             then the triangle order of the case table (e3dge_marching_cubes_tables).  On an ambiguous face the positive corners are
 *             separated, so tilings differ from Lewiner's there.
 * Three calls, no allocation, no synchronisation:
 *   e3dge_marching_cubes_ws_bytes   workspace bytes for the grid (-1: bad sizes)
 *   e3dge_marching_cubes_count      totals (2 ints, device) = {V, F}; {-1, -1} when 0 lies outside [min, max] of the volume (skimage's
 *                                   "Surface level must be within volume data range."); V = 0 otherwise means no surface
 *   e3dge_marching_cubes_emit       on the same stream, with the same workspace, volume and sizes: verts (n_verts, 3) float32, faces
 *                                   (n_faces, 3) int32; the caller passes the totals it read back, nothing is written past them
 *   e3dge_marching_cubes_tables     host only: n_tris (256), tri_edges (256, E3DGE_MC_MAX_TRIS, 3) (-1 past n_tris[c]).  Case c has bit k
 *                                   set iff corner k = (k & 1, (k >> 1) & 1, (k >> 2) & 1) is positive; edge e = 4 * axis + j runs along
 *                                   axis (0 x, 1 y, 2 z) from its lower corner, whose offsets on the other two axes are (j & 1, j >> 1)
 *                                   in increasing axis order; the lower corner's point owns the edge's vertex.
 * ---------------------------------------------------------------------------------------------------------------- */
#define E3DGE_MC_MAX_TRIS 16
int64_t e3dge_marching_cubes_ws_bytes(int nx, int ny, int nz);
int e3dge_marching_cubes_count(int* totals, void* ws, int64_t ws_bytes, const float* sdf, int nx, int ny, int nz, int64_t sx, int64_t sy,
                               int64_t sz, e3dge_stream_t stream);
int e3dge_marching_cubes_emit(float* verts, int* faces, int64_t n_verts, int64_t n_faces, const void* ws, int64_t ws_bytes, const float* sdf,
                              int nx, int ny, int nz, int64_t sx, int64_t sy, int64_t sz, int scene, e3dge_stream_t stream);
int e3dge_marching_cubes_tables(int* n_tris, int* tri_edges);

/* ----------------------------------------------------------------------------------------------------------------
 * Surface renderings (csrc/mesh_render.hip): the depth mesh of an xyz map, vertex normals, and a mesh rasteriser with Phong shading --
 * what the reference gets from xyz2mesh (project/utils/mesh_utils.py:107-126), trimesh's vertex_normals and pytorch3d's MeshRasterizer +
 * SoftPhongShader (create_mesh_renderer, mesh_utils.py:145-173).  Additions to ABI 16.  No allocation, no synchronisation.
 *
 * e3dge_depth_mesh      xyz (3, h, w) float32 -> verts (h w, 3): vertex r w + c = xyz[:, r, c]; faces (2 (h-1)(w-1), 3) int32: cell (r, c),
 *                       cells in row-major order, gives (r w + c, (r+1) w + c, r w + c + 1) then ((r+1) w + c, (r+1) w + c + 1, r w + c + 1):
 *                       one fixed diagonal; every face has signed area -1/2 in (column, row) index space, the winding the reference's
 *                       faces have after its column swap (its diagonal is Qhull's choice per cell).
 * e3dge_vertex_normals  normals (V, 3) float32 = normalise( sum over the vertex's faces of corner angle x unit face normal ), the normal
 *                       (v1 - v0) x (v2 - v0); faces of zero area (or with an index outside [0, V)) add nothing; a vertex without faces or
 *                       with a zero sum gets (0, 0, 0).  The terms are computed in float64 and summed as 2^40 fixed-point integers:
 *                       bit-reproducible.  ws: e3dge_vertex_normals_ws_bytes(V) bytes.
 * e3dge_mesh_render     one mesh, one camera, one point light, material all ones with shininess 64.  camera = C (3), x_ax (3), y_ax (3),
 *                       z_ax (3): view coordinates p_v = ((p - C).x_ax, (p - C).y_ax, (p - C).z_ax), +x left, +y up, +z into the scene; NDC
 *                       x_n = p_v.x / (p_v.z t), y_n = p_v.y / (p_v.z t), t = tan_half_fov; the centre of pixel (row i, column j) is
 *                       q = (1 - (2 j + 1) / S, 1 - (2 i + 1) / S).  Per pixel, for every face with |area| > 1e-8 (area = (x2 - x0)(y1 - y0) -
 *                       (y2 - y0)(x1 - x0) in NDC) and all three p_v.z >= znear / 2:
 *                         b0 = ((qx - x1)(y2 - y1) - (qy - y1)(x2 - x1)) / area, b1, b2 cyclically; inside = all b > 0;
 *                         d2 = min over the three edges of the squared distance from q to the segment (an edge shorter than 1e-4: to its end
 *                         point); covered = inside or d2 < blur_radius; d = inside ? -d2 : d2;
 *                         b'_k = (b_k / z_k) / sum_m (b_m / z_m), clamped to [0, 1], divided by max(their sum, 1e-5); z = sum b'_k z_k
 *                         (the NDC coordinates, b, b' and z are evaluated in float64 from the float32 vertices and camera: a face on the
 *                         silhouette is 1e-4 NDC wide with a depth range that is not small, and float32 coordinates and edge functions lose
 *                         its depth to rounding and cancellation; z_k, d2 and everything after the fragment's depth are float32);
 *                       the K = faces_per_pixel covered fragments with the smallest z >= 0 are kept, equal z: the lower face index first.
 *                       Each is shaded at P = sum b'_k vertex_k, N = normalise(sum b'_k normal_k) (normalise: x / max(|x|, 1e-6)):
 *                         L = normalise(light - P), c = N.L, V = normalise(C - P), R = 2 c N - L,
 *                         colour = (ambient + diffuse max(c, 0)) texel + specular (c > 0 ? max(V.R, 0) : 0)^64, texel = sum b'_k colour_k
 *                         (colors NULL: 1);
 *                       and blended:  p_k = 1 / (1 + exp(d_k / sigma)),  m = max((zfar - z_min) / (zfar - znear), 1e-10) with z_min the
 *                         nearest kept z,  w_k = p_k exp(((z_min - z_k) / (zfar - znear)) / gamma)  -- the exponent is formed from the view-space
 *                         depths, not as the difference of two rounded (zfar - z) / (zfar - znear) (only when m is the clamp 1e-10 is it
 *                         (zfar - z_k) / (zfar - znear) - 1e-10) --  delta = max(exp((1e-10 - m) / gamma), 1e-10),
 *                         rgb = (sum w_k colour_k + delta background) / (sum w_k + delta),  alpha = 1 - prod (1 - p_k).
 *                       image (S, S, 4) float32; zbuf (S, S, K) float32, near to far, -1 where empty; pix_to_face (S, S, K) int32, -1 where
 *                       empty; a pixel without fragments is (background, 0).
 *                       Faces are binned by 16 x 16-pixel tile into lists of bin_capacity entries in all.  status (2 ints, device) =
 *                       {entries needed, bin_capacity}: when the first exceeds the second the outputs are NOT written -- the caller reads
 *                       status and calls again with a larger capacity and workspace.  ws: e3dge_mesh_render_ws_bytes(V, F, S, bin_capacity)
 *                       bytes (-1: bad sizes; F x tiles must stay below 2^31).
 * ---------------------------------------------------------------------------------------------------------------- */
#define E3DGE_MESH_MAX_FACES_PER_PIXEL 8
typedef struct E3dgeMeshRenderArgs {
    const float* verts; const int32_t* faces; const float* normals; const float* colors;
    int64_t n_verts, n_faces;
    float camera[12];
    float tan_half_fov, znear, zfar;
    float light_location[3], ambient_color[3], diffuse_color[3], specular_color[3], background_color[3];
    float blur_radius, sigma, gamma;
    int32_t image_size, faces_per_pixel;
    float* image; float* zbuf; int32_t* pix_to_face;
    int32_t* status;
    void* ws;
    int64_t ws_bytes, bin_capacity;
} E3dgeMeshRenderArgs;
int e3dge_depth_mesh(float* verts, int32_t* faces, const float* xyz, int h, int w, e3dge_stream_t stream);
int64_t e3dge_vertex_normals_ws_bytes(int64_t n_verts);
int e3dge_vertex_normals(float* normals, const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, void* ws, int64_t ws_bytes,
                         e3dge_stream_t stream);
int64_t e3dge_mesh_render_ws_bytes(int64_t n_verts, int64_t n_faces, int image_size, int64_t bin_capacity);
int e3dge_mesh_render(const E3dgeMeshRenderArgs* args, e3dge_stream_t stream);

/* ----------------------------------------------------------------------------------------------------------------
 * View-consistent decoder noise (csrc/mesh_render.hip): midpoint subdivision of a triangle mesh and the projection of per-vertex noise
 * into the decoder's noise maps -- what the reference's NoiseInjection.project_noise (project/models/stylesdf_model.py:365-466) gets from
 * trimesh.remesh.subdivide and from pytorch3d through create_depth_mesh_renderer (mesh_utils.py:130-219: faces_per_pixel = 17, blur_radius
 * 1e-6, ambient 1, no diffuse or specular term, BlendParams defaults).  Additions to ABI 16.  No allocation, no synchronisation.
 *
 * e3dge_mesh_subdivide  one level.  An edge is the unordered pair (lo, hi) of a face side; the E distinct edges are ranked by their key
 *                       lo V + hi (int64) in ascending order.  edge_keys (E) int64: the distinct keys, ascending; side_rank (F, 3) int32:
 *                       the rank of the key of side (a, b), (b, c), (c, a) of face (a, b, c) -- ranking 3 F keys is the caller's (a sort).
 *                       out_verts (V + E, 3): vertex i < V is copied; vertex V + rank is 0.5f * (v_lo + v_hi) in float32 (the float64 mean
 *                       rounded to float32).  out_faces (4 F, 3) int32: face f = (a, b, c) becomes 4f = (a, m_ab, m_ca), 4f + 1 = (m_ab, b,
 *                       m_bc), 4f + 2 = (m_ca, m_bc, c), 4f + 3 = (m_ab, m_bc, m_ca), m_xy = V + rank of side (x, y): the winding is kept.
 *                       No special cases: a face with a repeated index follows the same rule (its side (a, a) is an edge with a "midpoint"
 *                       at v_a).  Face indices must lie in [0, V) (they are copied, not followed; a key that is no vertex pair gives a
 *                       vertex at the origin).  V + E and 4 F must stay below 2^31.  Vertex order differs from trimesh's, which numbers the
 *                       edges in the order numpy's unique of the sorted pairs returns them -- the same ascending (lo, hi) order -- but
 *                       nothing here depends on it.
 * e3dge_noise_project   vert_noise (n_maps, V) float32, 1 <= n_maps <= 4: scalar fields over the vertices (the maps of one size share one
 *                       rasterisation).  Camera, pixel centres, the candidate test, coverage with the blur rule, float64 NDC / barycentrics /
 *                       depth, the K-list ordered by (z, face index) and the blend with m, w_k, delta are e3dge_mesh_render's, word for word,
 *                       with K = E3DGE_NOISE_PROJECT_FACES_PER_PIXEL, colour_k = sum b'_k noise_k and background 1:
 *                         value = (sum w_k colour_k + delta) / (sum w_k + delta).
 *                       valid (S, S) uint8 = 1 where the largest kept z is > 0 (the reference's zbuf.max(-1) > 0: some fragment was kept);
 *                       out (n_maps, S, S) = value where valid, prev (n_maps, S, S) elsewhere (out may not alias prev).
 *                       Binning, status and the overflow protocol are e3dge_mesh_render's (outputs NOT written when status[0] >
 *                       status[1]); faces x tiles is not bounded here -- the scan carries 64 bits and `entries needed` saturates at
 *                       2^31 - 1, above every accepted bin_capacity (< 2^31 - 1).  ws: e3dge_noise_project_ws_bytes(V, F, S, bin_capacity)
 *                       bytes (-1: bad sizes).
 * ---------------------------------------------------------------------------------------------------------------- */
#define E3DGE_NOISE_PROJECT_FACES_PER_PIXEL 17
#define E3DGE_NOISE_PROJECT_MAX_MAPS 4
typedef struct E3dgeNoiseProjectArgs {
    const float* verts; const int32_t* faces; const float* vert_noise; const float* prev;
    int64_t n_verts, n_faces;
    float camera[12];
    float tan_half_fov, znear, zfar;
    float blur_radius, sigma, gamma;
    int32_t image_size, n_maps;
    float* out; uint8_t* valid;
    int32_t* status;
    void* ws;
    int64_t ws_bytes, bin_capacity;
} E3dgeNoiseProjectArgs;
int e3dge_mesh_subdivide(float* out_verts, int32_t* out_faces, const float* verts, const int32_t* faces, const int64_t* edge_keys,
                         const int32_t* side_rank, int64_t n_verts, int64_t n_faces, int64_t n_edges, e3dge_stream_t stream);
int64_t e3dge_noise_project_ws_bytes(int64_t n_verts, int64_t n_faces, int image_size, int64_t bin_capacity);
int e3dge_noise_project(const E3dgeNoiseProjectArgs* args, e3dge_stream_t stream);

/* Layout self-test: runs a 32x32xK fp32-MFMA product with the fragment conventions the render kernel
 * relies on and writes it to c (32*32 floats, row-major) for the caller to compare with a @ b^T.
 * a: (32, k) row-major, b: (32, k) row-major, k multiple of 8, k <= 256. */
int e3dge_selftest_mfma(float* c, const float* a, const float* b, int k, e3dge_stream_t stream);
/* The same with one f16 MFMA (v_mfma_f32_32x32x16_f16) per 16 k on the hi halves of a, b; k multiple of 16. */
int e3dge_selftest_mfma16(float* c, const float* a, const float* b, int k, e3dge_stream_t stream);
/* The same for v_mfma_f32_16x16x32_f16 (c: 16x16, a, b: (16, k) row-major, k multiple of 32). */
int e3dge_selftest_mfma16x16(float* c, const float* a, const float* b, int k, e3dge_stream_t stream);
/* Weight-stationary split-f16 layers (csrc/siren_ws.hip): the weights of a 256 x 256 layer live in registers, activations in LDS.
 *   wimg   : e3dge_ws_image_bytes(n_layers) bytes, written by e3dge_ws_pack from fp32 weights (n_layers, 256, 256) [out][in]
 * (The round-3 study chain e3dge_ws_chain -- DESIGN.md 4.1d -- was removed in round 5.) */
int64_t e3dge_ws_image_bytes(int n_layers);
int e3dge_ws_pack(void* wimg, const float* weights, int n_layers, e3dge_stream_t stream);
/* One 256 x 256 linear layer over the rows of a matrix, weight-stationary split-f16 (the layers of Fuse_sft_MLP,
 * project/models/helper_modules/sft.py:84-109 and resnetfc.py:49-58 -- local_query.py chains nine of these):
 *   y[row, off_y + f] = post( sum_k W[f][k] pre(x[row, off_x + k]) + bias[f] + colw[f] pre(m[row, off_m]) + r1[row, off_r1 + f] + r2[row, off_r2 + f] )
 * pre = relu (pre_relu != 0) or identity; post: 0 identity, 1 leaky relu (slope), 2 the SFT fuse  D + w_fuse (D S + v)  with
 * D = r1, S = r2 and v the bracket without r1, r2.  wimg = e3dge_ws_pack(W, 1).  amax_in: amax buffer (E3DGE_AMAX_FLOATS) holding
 * max |x| over the tensor x comes from (operand scale; NULL: values of order 1), amax_out: NULL or the buffer that receives max |y|
 * (zero it first).  Pointers other than wimg, x, y may be NULL (colw and m together); row pitches in floats, any alignment.
 * ABI 12 -- what the BACKWARD of those layers needs (d input = d output @ W is the same layer on the image of W^T):
 *   input side:  x <- x (.) xmul[row, off_xmul + k] * x_scale  (xmul NULL: x * x_scale; x_scale 0 = unset = 1; amax_xmul = amax buffer of xmul)
 *   post 3:      y = v * (r1 > 0 ? 1 : slope) + r2     the backward through lrelu (slope) / relu (slope 0) whose output / input is r1
 *   post 4:      y = v + r1 (1 + w_fuse r2)            d dec of the SFT fuse: v + g (1 + w scale)
 * y may alias r2 (posts 0, 1, 3) -- every element is read by the thread that writes it. */
typedef struct E3dgeWsLinear {
    const void* wimg; const float* x; const float* amax_in; const float* bias; const float* colw; const float* m;
    const float* r1; const float* r2; float* y; float* amax_out;
    int64_t n_rows;
    int32_t ld_x, off_x, ld_m, off_m, ld_r1, off_r1, ld_r2, off_r2, ld_y, off_y;
    int32_t pre_relu, post;
    float slope, w_fuse;
    const float* xmul; const float* amax_xmul;
    int32_t ld_xmul, off_xmul;
    float x_scale;
    int32_t reserved;
} E3dgeWsLinear;
int e3dge_ws_linear(const E3dgeWsLinear* args, e3dge_stream_t stream);
/* out[row * ld_out + off_out] = a[row, :] . u + [gate[row * ld_gate + off_gate] > 0] (b[row, :] . v)   (gate NULL: 1); a, b (n_rows, 256), u, v (256).
 * The data gradient of ONE extra input column shared by two 256-wide layers -- the visibility-mask column of Fuse_sft_MLP's 513-wide input
 * (sft.py:103-109 / resnetfc.py:49-58: d x[:, 256] = de Ws[:, 256] + (dnet W0[:, 256]) [x[:, 256] > 0]). */
int e3dge_ws_rowdot2(float* out, int ld_out, int off_out, const float* a, const float* u, const float* b, const float* v, const float* gate,
                     int ld_gate, int off_gate, int64_t n_rows, e3dge_stream_t stream);
/* Parameter gradient of a fully connected layer of the local branch (round 5):  c (m, n) = sum over rows p of a[p, off_a : off_a + m]^T f(b[p, off_b : off_b + n]),
 * f = relu when relu_b != 0 -- autograd's `grad_output.t() @ input` for the nn.Linear layers of ResnetBlockFC (helper_modules/resnetfc.py:49-58)
 * and Fuse_sft_MLP (helper_modules/sft.py:84-110) in the stage-2 step (e3dge_full_runner.py:185-317), with the relu of the layer's input folded in.
 * a, b: fp32 rows of lda / ldb floats (4-byte aligned; any row pitch), amax_a / amax_b: amax buffers (e3dge_amax) bounding |a| / |b|;
 * ws: e3dge_wgrad_ws_floats(m, n, n_rows) floats (split-K partial blocks, folded in fixed order: bit-reproducible).  Split-f16 x 3, fp32 accumulate.
 * ABI 14 (round 6) -- what rides with the same pass over the rows (all optional, NULL / 0 = off):
 *   colsum (m):          sum_p a[p, off_a + i]                       autograd's `grad_output.sum(0)`, the layer's bias gradient
 *   xcol, ccol:          ccol[i * ld_ccol] = sum_p a[p, off_a + i] f(xcol[p * ld_xcol])   one more column of b that the block grid leaves out
 *   b_gap_at, b_gap:     columns [b_gap_at, b_gap_at + b_gap) of b's rows (and of c's) are skipped: c[:, j] for j >= b_gap_at comes from
 *                        b[:, off_b + j + b_gap] and lands in c[:, j + b_gap]; n counts the columns that ARE contracted.  b_gap_at: a
 *                        multiple of 256.  (Fuse_sft_MLP's 513-wide input: 256 features | visibility mask | 256 features -- n = 512,
 *                        b_gap_at = 256, b_gap = 1, xcol = b + off_b + 256, ccol = c + 256.) */
typedef struct E3dgeWgrad {
    const float* a; const float* amax_a; const float* b; const float* amax_b;
    float* c; float* ws;
    int64_t ws_floats, n_rows;
    int32_t lda, off_a, m, ldb, off_b, n, ldc, relu_b;
    const float* xcol; float* colsum; float* ccol;
    int32_t ld_xcol, ld_ccol, b_gap_at, b_gap;
} E3dgeWgrad;
int64_t e3dge_wgrad_ws_floats(int m, int n, int64_t n_rows);
int e3dge_wgrad(const E3dgeWgrad* args, e3dge_stream_t stream);
/* Accuracy self-test of the kernel's sine: y[i] = sin(x[i]) with the device routine the SIREN layers use. */
int e3dge_selftest_sin(float* y, const float* x, int n, e3dge_stream_t stream);
/* The alternative 13-op polynomial sine (kernels built with -DE3DGE_POLY_SINE use it). */
int e3dge_selftest_sin_poly(float* y, const float* x, int n, e3dge_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The training loss's own kernels (csrc/losses.hip).  Additions to ABI 16.  No allocation, no synchronisation, no atomics:
 * results are bit-identical from run to run.  Replaces what LossClass (project/losses/builder.py) and its callers run as
 * framework kernels: the trainers' pool_256 / pool_64 (trainer.py:1023-1025), the backward of criterionImg (builder.py:142)
 * and the four terms of calc_shape_rec_loss (builder.py:76-104) with eikonal_loss (gan_loss.py:14-25).
 *
 * e3dge_avgpool_fwd   out (planes, in_h / f, in_w / f) = mean over the f x f blocks of in (planes, in_h, in_w); f in {1, 2, 4, 8, 16}
 *                     dividing in_h and in_w -- AdaptiveAvgPool2d at an integer ratio.  Summed row-major inside the block, then one
 *                     division by f^2.
 * e3dge_avgpool_bwd   d_in[p, y, x] = d_out[p, y / f, x / f] / f^2 (every element of d_in is written).
 * e3dge_sqerr_bwd     d_pred[i] = (*scale_ptr) * (pred[i] - gt[i]), i < n: the backward of mean((pred - gt)^2) with the caller's
 *                     (upstream * 2 * l2_lambda / n) read from device memory.  The forward is e3dge_image_metrics' sums.
 * planes == 0 / n == 0: nothing is launched, E3DGE_OK.
 * ---------------------------------------------------------------------------------------------------------------- */
int e3dge_avgpool_fwd(float* out, const float* in, int64_t planes, int in_h, int in_w, int f, e3dge_stream_t stream);
int e3dge_avgpool_bwd(float* d_in, const float* d_out, int64_t planes, int in_h, int in_w, int f, e3dge_stream_t stream);
int e3dge_sqerr_bwd(float* d_pred, const float* pred, const float* gt, int64_t n, const float* scale_ptr, e3dge_stream_t stream);
/* The shape terms.  seg[0..3] are, in the reference's order of summation, sdf_rec_loss, surf_rec_loss, surface_norm_rec_loss and
 * eikonal_term; a segment with n == 0 is off (its term is 0 and is not added).  kind:
 *   E3DGE_SHAPE_SMOOTH_L1  mean over n elements of smooth_l1(pred - gt), beta 1: 0.5 d^2 if |d| < 1, else |d| - 0.5; gt NULL = zeros
 *   E3DGE_SHAPE_EIKONAL    mean over n 3-vectors of (|pred| - 1)^2; gt must be NULL
 * forward:  terms[s] = lambda_s * mean_s, *total = the enabled terms added in slot order; one tile launch over all segments and
 *           one single-workgroup fold in double.  partial: e3dge_shape_loss_partial_floats(args) floats of workspace.
 * backward: one launch; d_pred_s = (*upstream) * lambda_s / n_s * clamp(pred - gt, -1, 1)  (Smooth-L1)
 *                                  (*upstream) * lambda_s / n_s * 2 (|e| - 1) e / |e|, exactly 0 where e = 0  (eikonal).
 *           Reads pred, gt, d_pred, n, lambda, kind and upstream; a segment whose gradient is not wanted has n = 0.
 * Every segment off: nothing is launched (terms and total are left as they are), E3DGE_OK. */
#define E3DGE_SHAPE_LOSS_SEGMENTS 4
#define E3DGE_SHAPE_SMOOTH_L1 0
#define E3DGE_SHAPE_EIKONAL 1
typedef struct E3dgeShapeLossSegment {
    const float* pred; const float* gt; float* d_pred;
    int64_t n;
    float lambda;
    int32_t kind;
} E3dgeShapeLossSegment;
typedef struct E3dgeShapeLossArgs {
    E3dgeShapeLossSegment seg[E3DGE_SHAPE_LOSS_SEGMENTS];
    float* terms; float* total; float* partial;
    int64_t partial_floats;
    const float* upstream;
} E3dgeShapeLossArgs;
int64_t e3dge_shape_loss_partial_floats(const E3dgeShapeLossArgs* args);
int e3dge_shape_loss_fwd(const E3dgeShapeLossArgs* args, e3dge_stream_t stream);
int e3dge_shape_loss_bwd(const E3dgeShapeLossArgs* args, e3dge_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * StyleGAN2 discriminator with frozen weights (csrc/disc.hip, csrc/disc_bwd.h): the logits and their gradient with respect
 * to the input images -- the adversarial term of the stage-2.2 encoder step.  Additions to ABI 16.  No allocation, no
 * synchronisation, no atomics: results are bit-identical from run to run, and everything up to the minibatch-stddev channel
 * does not depend on the batch an image is in.  Replaces Discriminator.forward (project/models/stylesdf_model.py:1541-1617)
 * and its autograd for a frozen network.  A network is named by (init_size, channel_multiplier, in_channels): init_size a power
 * of two in 8..1024, channel_multiplier 1..4, in_channels 1..16 (D_input_size).
 *
 * e3dge_disc_packed_floats   floats of the packed image (-1: no such network): per convolution `weight * scale` (rounded once, as
 *                            EqualConv2d rounds it on every call) in MFMA A-fragment order and once more transposed with flipped taps
 *                            for the data gradient, the biases, both EqualLinear matrices scaled, the blur FIR and its flip.
 * e3dge_disc_pack_weights    src: HOST struct of device pointers (blocks beyond the network's are not read).  Re-run after a weight
 *                            update.
 * e3dge_disc_ws_bytes        workspace bytes of a forward (backward = 0) or a backward (backward != 0) of n images of
 *                            height x width (-1: bad sizes, or a batch the reference's minibatch-stddev reshape rejects).
 *                            height = width = init_size, or, for init_size 256, 256 f with f in {2, 4, 8, 16} (pool_256).
 * e3dge_disc_saved_bytes     bytes of the state the saving forward keeps for n images: the output of every lrelu and the last
 *                            block's output.
 * e3dge_disc_forward         images (n, in_channels, height, width) fp32 contiguous -> logits (n, 1).  taps[t] NULL or: t <
 *                            E3DGE_DISC_MAX_BLOCKS the output of ResBlock t, E3DGE_DISC_TAP_STDDEV the n / group stddev scalars,
 *                            E3DGE_DISC_TAP_FINAL final_conv's output (n, 512, 4, 4), E3DGE_DISC_TAP_STEM unused.  saved != NULL:
 *                            the state-saving forward, the same launches with the activations written to `saved` (bit-identical
 *                            logits and taps).  Fails with the field named: "null", "n=", "height", "init_size", "workspace", "saved".
 * e3dge_disc_backward        saved: what e3dge_disc_forward left for the same n, sizes and network.  grad_logits (n, 1) ->
 *                            grad_images (n, in_channels, height, width), every element written.  gstage[t] NULL or the gradient
 *                            at tap t (E3DGE_DISC_TAP_STEM: at the stem's output; E3DGE_DISC_TAP_STDDEV unused).
 * e3dge_disc_conv            debug entry: one convolution of the family.  in (n, cin, height, width), w (cout, cin, ksize, ksize)
 *                            -> out (n, cout, OH, OW): stride 1 pads ksize / 2 (OH = height), stride 2 pads nothing (OH = (height -
 *                            ksize) / 2 + 1).  v = conv(in, fl(w * scale)) [+ bias[c]] [lrelu 0.2, * sqrt 2 when act]
 *                            [+ addend, / sqrt 2 when merge].  wfrag: scratch of ceil16(cout) * ceil32(cin ksize^2) floats.
 * e3dge_disc_conv_dgrad      debug entry: its data gradient.  g (n, cout, OH, OW) -> out (n, cin, height, width) = conv^T(g m)
 *                            [+ addend], m = s_pos where sign > 0 else s_neg (sign NULL: m = s_pos), sign shaped like g.
 *                            wfrag_t: scratch of ceil16(cin) * ceil32(cout ksize^2) floats.
 * e3dge_disc_stddev          debug entry: feat (n, channels, hw) -> cat (n, channels + 1, hw) with the minibatch-stddev channel;
 *                            scalars NULL or (n / group,).
 * ---------------------------------------------------------------------------------------------------------------- */
#define E3DGE_DISC_MAX_BLOCKS 8
#define E3DGE_DISC_TAP_STDDEV 8
#define E3DGE_DISC_TAP_FINAL 9
#define E3DGE_DISC_TAP_STEM 10
#define E3DGE_DISC_TAPS 11
typedef struct E3dgeDiscPackSrc {
    int32_t init_size, channel_multiplier, in_channels, reserved;
    const float* stem_w; const float* stem_b;                              /* convs.0.0.weight, convs.0.1.bias */
    const float* conv1_w[E3DGE_DISC_MAX_BLOCKS]; const float* conv1_b[E3DGE_DISC_MAX_BLOCKS];
    const float* conv2_w[E3DGE_DISC_MAX_BLOCKS]; const float* conv2_b[E3DGE_DISC_MAX_BLOCKS];
    const float* skip_w[E3DGE_DISC_MAX_BLOCKS];
    const float* final_w; const float* final_b;
    const float* lin1_w; const float* lin1_b; const float* lin2_w; const float* lin2_b;
    const float* blur;                                                     /* the 4 x 4 Blur.kernel */
} E3dgeDiscPackSrc;
typedef struct E3dgeDiscArgs {
    const float* packed; const float* images;
    int32_t n, height, width, init_size, channel_multiplier, in_channels;
    float* logits;
    float* taps[E3DGE_DISC_TAPS];
    void* ws; int64_t ws_bytes;
    void* saved; int64_t saved_bytes;
} E3dgeDiscArgs;
typedef struct E3dgeDiscBwdArgs {
    const float* packed; const void* saved; int64_t saved_bytes;
    int32_t n, height, width, init_size, channel_multiplier, in_channels;
    const float* grad_logits; float* grad_images;
    float* gstage[E3DGE_DISC_TAPS];
    void* ws; int64_t ws_bytes;
} E3dgeDiscBwdArgs;
int64_t e3dge_disc_packed_floats(int init_size, int channel_multiplier, int in_channels);
int e3dge_disc_pack_weights(float* packed, const E3dgeDiscPackSrc* src, e3dge_stream_t stream);
int64_t e3dge_disc_ws_bytes(int n, int height, int width, int init_size, int channel_multiplier, int in_channels, int backward);
int64_t e3dge_disc_saved_bytes(int n, int init_size, int channel_multiplier, int in_channels);
int e3dge_disc_forward(const E3dgeDiscArgs* args, e3dge_stream_t stream);
int e3dge_disc_backward(const E3dgeDiscBwdArgs* args, e3dge_stream_t stream);
int e3dge_disc_conv(float* out, const float* in, const float* w, float* wfrag, const float* bias, const float* addend, int n, int cin, int cout,
                    int height, int width, int ksize, int stride, int act, int merge, float scale, e3dge_stream_t stream);
int e3dge_disc_conv_dgrad(float* out, const float* g, const float* w, float* wfrag_t, const float* sign, float s_pos, float s_neg,
                          const float* addend, int n, int cin, int cout, int height, int width, int ksize, int stride, float scale,
                          e3dge_stream_t stream);
int e3dge_disc_stddev(float* cat, float* scalars, const float* feat, int n, int channels, int hw, e3dge_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Hourglass image filter of the local branch, forward (csrc/hgfilter.hip; the backward is the next section).  Additions to
 * ABI 17.  No allocation, no synchronisation, no atomics; bit-reproducible, and an image's maps do not depend on its position in the batch or on the batch
 * size.  Replaces HGPIFuNetGANResidualResnetFC.filter (vendor/pifu/lib/model/HGPIFuGANNetResidualInputResnetFC.py:33-76): residual_conv and
 * depth_conv (reflect padding, InstanceNorm2d(affine)), the concatenation and HGFilter (vendor/pifu/lib/model/HGFilters.py) with
 * norm='group', hg_down='ave_pool', hg_input_channel=64, hourglass_dim=256.  fp32; the entries of this section are the forward.
 *
 * Source tensors of the filter, in this order (ConvBlock(cin, cout) = bn1.weight, bn1.bias, conv1.weight, bn2.weight, bn2.bias,
 * conv2.weight, bn3.weight, bn3.bias, conv3.weight and, where cin != cout, bn4.weight, bn4.bias, downsample.2.weight;
 * level(d) = b1_d, b2_d, level(d - 1) or b2_plus_1 for d = 1, b3_d):
 *   conv1.weight, conv1.bias, bn1.weight, bn1.bias, ConvBlock conv2, conv3, conv4; then per stack i: level(num_hourglass) of m<i>,
 *   ConvBlock top_m_<i>, conv_last<i>.weight, .bias, bn_end<i>.weight, .bias, l<i>.weight, .bias and, for all but the last stack,
 *   bl<i>.weight, .bias, al<i>.weight, .bias.
 * Source tensors of the two front nets (E3DGE_HGF_FRONT_SRC = 16), residual_conv's eight then depth_conv's: 0.weight,
 *   1.conv.0.weight, 1.conv.0.bias, 1.conv.2.weight, 1.conv.3.weight, 1.conv.3.bias, 1.conv.5.weight, 2.weight.
 *
 * e3dge_hgf_packed_floats   floats of the packed image of (num_stack 1..8, num_hourglass 1..4), front nets included (-1: outside).
 * e3dge_hgf_pack_weights    filter_src, front_src: HOST arrays of device pointers; front_src NULL: the front nets' part of the
 *                           image stays unwritten and e3dge_hgf_front must not be called with it.  Re-run after a weight update.
 * e3dge_hgf_ws_bytes        workspace bytes of e3dge_hgf_forward and e3dge_hgf_front for n images of height x width (the INPUT
 *                           size of the filter: the image size) (-1: bad sizes).
 * e3dge_hgf_forward         input (n, 64, height, width) -> outputs[i] (n, 256, height / 4, width / 4) for every stack i < num_stack,
 *                           tmpx (n, 64, height / 2, width / 2), normx (n, 128, height / 4, width / 4).  252 launches at the default
 *                           (4, 2).  Fails before any launch on a null pointer ("null"), n outside 1..4096, num_stack or
 *                           num_hourglass out of range, height or width not a multiple of 4 * 2^num_hourglass or above 4096, and a
 *                           workspace that is too small ("workspace").
 * e3dge_hgf_front           image (n, 3, height, width), depth (n, 1, height, width) -> out (n, 64, height, width): residual_conv
 *                           into channels 0..31, depth_conv into 32..63.  12 launches.  Same refusals.
 * e3dge_hgf_conv            debug entry: one convolution of the family.  in (n, cin, height, width), w (cout, cin, ksize, ksize) with
 *                           (ksize, stride) = (7, 2), (3, 1) or (1, 1), padding ksize / 2, zeros or (reflect != 0, ksize 3) mirrored;
 *                           cout a multiple of 16.  wfrag: scratch of cout * roundup(cin ksize^2, 32) floats.  in_ab NULL or
 *                           (n, cin, 2): x <- relu(a x + b) on in-image elements.  bias NULL or (cout).  raw NULL or (n, cout, OH, OW):
 *                           the result before the residual.  res NULL or (n, res_channels, OH, OW), added from channel res_c0 on.
 *                           out (n, out_channels, OH, OW), written from channel out_c0 on.  Two launches.
 * e3dge_hgf_norm            debug entry: ab (n, channels, 2) = (gamma rstd, beta - mean gamma rstd) of GroupNorm(groups, channels),
 *                           eps 1e-5, over the channels [c0, c0 + channels) of x (n, channels_total, height, width); moments in
 *                           float64.  groups = channels is InstanceNorm2d(affine).  One launch.
 * e3dge_hgf_pool            debug entry: out (planes, height / 2, width / 2) = avg_pool2d(in, 2, 2); height and width even.
 * e3dge_hgf_up_add          debug entry: out (planes, 2 height, 2 width) = up1 + bicubic x2 of low (planes, height, width),
 *                           align_corners, A = -0.75, source indices clamped at the border.
 * ---------------------------------------------------------------------------------------------------------------- */
#define E3DGE_HGF_MAX_STACK 8
#define E3DGE_HGF_FRONT_SRC 16
typedef struct E3dgeHgfArgs {
    const float* packed;              /* e3dge_hgf_pack_weights */
    const float* input;
    int32_t n, height, width, num_stack, num_hourglass, reserved;
    float* outputs[E3DGE_HGF_MAX_STACK];
    float* tmpx; float* normx;
    void* ws;
    int64_t ws_bytes;
} E3dgeHgfArgs;
int64_t e3dge_hgf_packed_floats(int num_stack, int num_hourglass);
int e3dge_hgf_pack_weights(float* packed, const float* const* filter_src, int n_filter_src, const float* const* front_src, int num_stack,
                           int num_hourglass, e3dge_stream_t stream);
int64_t e3dge_hgf_ws_bytes(int n, int height, int width, int num_stack, int num_hourglass);
int e3dge_hgf_forward(const E3dgeHgfArgs* args, e3dge_stream_t stream);
int e3dge_hgf_front(const float* packed, const float* image, const float* depth, float* out, int n, int height, int width, int num_stack,
                    int num_hourglass, void* ws, int64_t ws_bytes, e3dge_stream_t stream);
int e3dge_hgf_conv(float* out, float* raw, const float* in, const float* w, float* wfrag, const float* in_ab, const float* bias,
                   const float* res, int n, int cin, int cout, int height, int width, int ksize, int stride, int reflect, int out_channels,
                   int out_c0, int res_channels, int res_c0, e3dge_stream_t stream);
int e3dge_hgf_norm(float* ab, const float* x, const float* gamma, const float* beta, int n, int channels_total, int c0, int channels,
                   int groups, int height, int width, e3dge_stream_t stream);
int e3dge_hgf_pool(float* out, const float* in, int64_t planes, int height, int width, e3dge_stream_t stream);
int e3dge_hgf_up_add(float* out, const float* up1, const float* low, int64_t planes, int height, int width, e3dge_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Hourglass image filter of the local branch, backward (csrc/hgfilter_bwd.h).  Additions to ABI 17.  The gradient to the filter's
 * input and, through the front nets, to the residual image and the depth map, and (grads != NULL) to every parameter the forward
 * reads; once differentiable, fp32.
 * No allocation, no synchronisation, no atomics; two runs are bit-identical and an image's gradient does not depend on the batch.
 * Every entry refuses null pointers, sizes and configurations outside the forward's, a workspace that is too small ("workspace") and
 * a saved state that is too small ("saved state") before any launch.
 *
 * e3dge_hgf_saved_bytes     bytes of the saved state of n images of height x width, the front nets' part included (-1: bad sizes):
 *                           every convolution's pre-norm input and every norm's (a, b), each in a buffer of its own.  No masks: a
 *                           ReLU's branch is recomputed as fmaf(a, x, b) > 0; no mean or rstd: the moments are summed again.
 * e3dge_hgf_forward_saving  e3dge_hgf_forward with the same launches and bit-identical results, the state kept in `saved`.
 * e3dge_hgf_front_saving    e3dge_hgf_front likewise, into the same `saved` buffer.
 * e3dge_hgf_packed_t_floats floats of the transposed image: the data gradient's A-fragment image of every convolution (-1: outside).
 * e3dge_hgf_pack_weights_t  as e3dge_hgf_pack_weights; norm weights are read from the forward image.  Re-run after a weight update.
 * e3dge_hgf_bwd_ws_bytes    workspace bytes of e3dge_hgf_backward and e3dge_hgf_front_backward (-1: bad sizes).
 * e3dge_hgf_backward        g_outputs[i] (n, 256, height / 4, width / 4) or NULL (absent: skipped, not zeros), g_normx likewise, at
 *                           least one of them; tmpx, normx: the forward's results -> g_input (n, 64, height, width).
 * e3dge_hgf_front_backward  g_feats (n, 64, height, width) -> g_image (n, 3, height, width), g_depth (n, 1, height, width); either
 *                           may be NULL (not wanted).  grads: NULL, or the same buffer as e3dge_hgf_backward's: the front nets'
 *                           sixteen gradients are written behind the filter's; then image and depth are the forward's inputs.
 * e3dge_hgf_grad_floats     floats of `grads`: one gradient per source tensor of e3dge_hgf_pack_weights, filter_src then front_src,
 *                           in that order and in the sources' own shapes, back to back (-1: outside).  Gradients of layers that no
 *                           upstream gradient reaches (stacks above the last one with a gradient) are left unwritten.
 * e3dge_hgf_branch_bytes    bytes of the optional debug buffer `branch` of the two entries above (one buffer for both): one byte per
 *                           element of every norm's input, 1 where this run's ReLU passed -- what a branch-pinned float64 truth
 *                           takes its ReLU derivatives from.  Order: the stem's norm; bn1, bn2, bn3 and, where the block has a
 *                           downsample, bn4 of every ConvBlock in the order of the source tensors; bn_end of every stack; the two
 *                           norms of residual_conv, then of depth_conv.  Every buffer starts at a multiple of 256 bytes.
 * e3dge_hgf_conv_dgrad      debug entry: out (n, cin, height, width) = addend + [fmaf(a, x, b) > 0] * the data gradient of the
 *                           convolution of e3dge_hgf_conv from g = the channels [g_c0, g_c0 + cout) of (n, g_channels, OH, OW);
 *                           (a, b) = x_ab (n, cin, 2), x (n, cin, height, width), both or neither; addend optional; wfrag_t:
 *                           ig_mpad(cin) * ig_kpad(cout ksize^2) floats, written here.  Two launches.
 * e3dge_hgf_norm_bwd        debug entry: gx (n, channels, height, width) = add1 + (add0 + d norm / d x applied to gy) for the norm
 *                           of e3dge_hgf_norm; add0 the channels [add0_c0, ..) of (n, add0_channels, height, width), add1 dense,
 *                           both optional; mask_ab (n, channels, 2) optional: gy is first multiplied by fmaf(a, x, b) > 0; coef:
 *                           n * channels * 5 float64 of scratch.  dgamma, dbeta (channels) optional, together: the norm's
 *                           parameter gradients, summed over the images in ascending order in float64.  Two or three launches.
 * e3dge_hgf_pool_bwd        debug entry: gin (planes, height, width) = addend + the adjoint of avg_pool2d(2, 2) applied to gout.
 * e3dge_hgf_conv_wgrad      debug entry: dw (cout, cin, ksize, ksize) = the weight gradient of the convolution of e3dge_hgf_conv from g
 *                           (as e3dge_hgf_conv_dgrad's) and its input x (n, cin, height, width), activated by relu(a x + b) where
 *                           x_ab is given; dbias (cout) optional, from a dense g.  ws: e3dge_hgf_wgrad_ws_floats floats.  Split K
 *                           over images and 2048-pixel segments, partials folded in float64 in ascending order: no atomics.
 * e3dge_hgf_up_bwd          debug entry: glow (planes, height, width) = the adjoint of e3dge_hgf_up_add's bicubic x2 applied to g
 *                           (planes, 2 height, 2 width).
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct E3dgeHgfBwdArgs {
    const float* packed;              /* e3dge_hgf_pack_weights */
    const float* packed_t;            /* e3dge_hgf_pack_weights_t */
    const float* saved;               /* e3dge_hgf_forward_saving */
    int64_t saved_bytes;
    const float* tmpx; const float* normx;
    int32_t n, height, width, num_stack, num_hourglass, reserved;
    const float* g_outputs[E3DGE_HGF_MAX_STACK];
    const float* g_normx;
    float* g_input;
    void* ws;
    int64_t ws_bytes;
    unsigned char* branch;            /* debug, or NULL: e3dge_hgf_branch_bytes */
    int64_t branch_bytes;
    float* grads;                     /* NULL (frozen), or e3dge_hgf_grad_floats floats: the parameter gradients */
    const float* input;               /* with grads: the forward's input and its outputs below the last one with a gradient */
    const float* outputs[E3DGE_HGF_MAX_STACK];
} E3dgeHgfBwdArgs;
int64_t e3dge_hgf_saved_bytes(int n, int height, int width, int num_stack, int num_hourglass);
int e3dge_hgf_forward_saving(const E3dgeHgfArgs* args, void* saved, int64_t saved_bytes, e3dge_stream_t stream);
int e3dge_hgf_front_saving(const float* packed, const float* image, const float* depth, float* out, int n, int height, int width,
                           int num_stack, int num_hourglass, void* ws, int64_t ws_bytes, void* saved, int64_t saved_bytes,
                           e3dge_stream_t stream);
int64_t e3dge_hgf_packed_t_floats(int num_stack, int num_hourglass);
int e3dge_hgf_pack_weights_t(float* packed_t, const float* const* filter_src, int n_filter_src, const float* const* front_src,
                             int num_stack, int num_hourglass, e3dge_stream_t stream);
int64_t e3dge_hgf_bwd_ws_bytes(int n, int height, int width, int num_stack, int num_hourglass);
int64_t e3dge_hgf_branch_bytes(int n, int height, int width, int num_stack, int num_hourglass);
int e3dge_hgf_backward(const E3dgeHgfBwdArgs* args, e3dge_stream_t stream);
int e3dge_hgf_front_backward(const float* packed, const float* packed_t, const void* saved, int64_t saved_bytes, const float* g_feats,
                             float* g_image, float* g_depth, int n, int height, int width, int num_stack, int num_hourglass, void* ws,
                             int64_t ws_bytes, unsigned char* branch, int64_t branch_bytes, float* grads, const float* image,
                             const float* depth, e3dge_stream_t stream);
int e3dge_hgf_conv_dgrad(float* out, const float* g, const float* w, float* wfrag_t, const float* x, const float* x_ab, const float* addend,
                         int n, int cin, int cout, int height, int width, int ksize, int stride, int reflect, int g_channels, int g_c0,
                         e3dge_stream_t stream);
int e3dge_hgf_norm_bwd(float* gx, const float* gy, const float* x, const float* gamma, const float* mask_ab, const float* add0,
                       int add0_channels, int add0_c0, const float* add1, double* coef, float* dgamma, float* dbeta, int n, int channels_total, int c0,
                       int channels, int groups, int height, int width, e3dge_stream_t stream);
int e3dge_hgf_pool_bwd(float* gin, const float* gout, const float* addend, int64_t planes, int height, int width, e3dge_stream_t stream);
int e3dge_hgf_up_bwd(float* glow, const float* g, int64_t planes, int height, int width, e3dge_stream_t stream);
int64_t e3dge_hgf_grad_floats(int num_stack, int num_hourglass);
int64_t e3dge_hgf_wgrad_ws_floats(int n, int cin, int cout, int height, int width, int ksize, int stride);
int e3dge_hgf_conv_wgrad(float* dw, float* dbias, const float* g, const float* x, const float* x_ab, int n, int cin, int cout, int height,
                         int width, int ksize, int stride, int reflect, int g_channels, int g_c0, float* ws, int64_t ws_floats,
                         e3dge_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The E0 image encoder, forward, eval form (csrc/encoder.h, compiled with csrc/idnet.hip).  Additions to ABI 17.  No allocation, no
 * synchronisation, no atomics; bit-reproducible, and an image's results do not depend on its position in the batch or on the batch
 * size.  Replaces HybridGradualStyleEncoder_V2.forward (project/models/encoders/fpn_encoders.py:266-433) for num_layers 50, mode
 * 'ir_se', input_nc 3, BatchNorm on its running statistics: input_layer and the 24 bottleneck_IR_SE units, the three lateral layers of
 * the pyramid and the style heads (GradualStyleBlock, helpers.py:472-497).  fp32.  No backward.
 *
 * Configuration: size (the square input: a multiple of 16 in 32..256), geo_dim and tex_dim (fpn_pigan_geo_layer_dim,
 * fpn_pigan_tex_layer_dim: 32, 64 or 128; a head has log2(dim) convolutions; the three texture heads read p64 when tex_dim is 64 and
 * p32 otherwise), enable_decoder (0 / 1: the decoder head styles_stylegan.0 on p128).  A head layer whose input map is larger than
 * 2 x 2 is a convolution; from the 2 x 2 (or 1 x 1) map on the packed image holds the taps that see the map and nothing else, so the
 * image depends on the size.
 *
 * Source tensors, in this order (BN = weight, bias, running_mean, running_var):
 *   input_layer.0.weight, BN input_layer.1, input_layer.2.weight; per unit body.<u>: BN res_layer.0, res_layer.1.weight,
 *   res_layer.2.weight, res_layer.3.weight, BN res_layer.4, res_layer.5.fc1.weight, res_layer.5.fc2.weight and, for units 3, 7 and 21,
 *   shortcut_layer.0.weight, BN shortcut_layer.1; latlayer256, latlayer128, latlayer64 (.weight, .bias each); per head
 *   styles_pigan.0 .. 8 and then, with enable_decoder, styles_stylegan.0: convs.0.weight, convs.0.bias, convs.2.weight, ... (every
 *   convolution), linear.weight, linear.bias.  styles_stylegan.1-9 are never read by the reference's forward and are not sources.
 *
 * e3dge_enc_packed_floats   floats of the packed image (-1: outside the configurations above).
 * e3dge_enc_pack_weights    src: HOST array of n_src device pointers.  Re-run after a weight update.
 * e3dge_enc_ws_bytes        workspace bytes of e3dge_enc_forward for n images (1..256) (-1: bad sizes).
 * e3dge_enc_forward         images (n, 3, size, size) -> thumb_out (n, 9, 256), stylegan_out (n, 512) (head 0 of the decoder latent; may
 *                           be NULL without enable_decoder, when no p128 work is done), p32 (n, 512, size / 8, size / 8), p64
 *                           (n, 512, size / 4, size / 4).  Fails before any launch on a null pointer ("null"), n, size or dims out of range
 *                           and a workspace that is too small ("workspace").
 * e3dge_enc_lateral         debug entry: out (n, cout, height, width) = bilinear(coarse (n, cout, coarse_height, coarse_width) -> height
 *                           x width, align_corners) + (conv1x1(in (n, cin, height, width), w (cout, cin)) + bias).  cout a multiple of
 *                           64; wfrag: scratch of cout * roundup(cin, 32) floats.  Two launches.
 * e3dge_enc_head_conv       debug entry: out (heads, n, cout, ceil(height / 2), ceil(width / 2)) = LeakyReLU_0.01(conv3x3 stride 2 pad 1
 *                           + bias) per head; in (n, cin, height, width) with shared = 1, (heads, n, cin, height, width) with 0;
 *                           w (heads, cout, cin, 3, 3), bias (heads, cout).  wfrag: heads * cout * roundup(9 cin, 32) floats.
 * e3dge_enc_head_tail       debug entry: a head group's tail from a start x start map (start 1 or 2): in (heads, n, channels, start,
 *                           start) -> n_convs stride-2 layers (the first one sees the start x start map, the rest 1 x 1 maps;
 *                           conv_w (heads, n_convs, channels, channels, 3, 3) whose dead taps are never read, conv_b (heads, n_convs,
 *                           channels)) -> EqualLinear (lin_w (heads, channels, channels) times 1 / sqrt(channels), lin_b (heads,
 *                           channels)) -> out (n, heads, channels).  scratch: at least heads * channels * (channels * (n_convs + 4) +
 *                           n_convs + 1 + 2 n) floats.
 * ---------------------------------------------------------------------------------------------------------------- */
#define E3DGE_ENC_HEADS 9
#define E3DGE_ENC_MAX_HEAD_CONVS 8
typedef struct E3dgeEncArgs {
    const float* packed;              /* e3dge_enc_pack_weights, for the same size and dims */
    const float* images;
    int32_t n, size, geo_dim, tex_dim, enable_decoder, reserved;
    float* thumb_out; float* stylegan_out; float* p32; float* p64;
    void* ws;
    int64_t ws_bytes;
} E3dgeEncArgs;
int64_t e3dge_enc_packed_floats(int size, int geo_dim, int tex_dim, int enable_decoder);
int e3dge_enc_pack_weights(float* packed, const float* const* src, int n_src, int size, int geo_dim, int tex_dim, int enable_decoder,
                           e3dge_stream_t stream);
int64_t e3dge_enc_ws_bytes(int n, int size, int geo_dim, int tex_dim, int enable_decoder);
int e3dge_enc_forward(const E3dgeEncArgs* args, e3dge_stream_t stream);
int e3dge_enc_lateral(float* out, const float* coarse, const float* in, const float* w, const float* bias, float* wfrag, int n, int cin,
                      int cout, int coarse_height, int coarse_width, int height, int width, e3dge_stream_t stream);
int e3dge_enc_head_conv(float* out, const float* in, const float* w, const float* bias, float* wfrag, int n, int heads, int shared, int cin,
                        int cout, int height, int width, e3dge_stream_t stream);
int e3dge_enc_head_tail(float* out, const float* in, const float* conv_w, const float* conv_b, const float* lin_w, const float* lin_b,
                        float* scratch, int64_t scratch_floats, int n, int heads, int channels, int start, int n_convs,
                        e3dge_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The 2-D residual aligner (ADA), forward, eval form (csrc/aligner.hip).  Additions to ABI 17.  No allocation, no synchronisation, no
 * atomics; bit-reproducible, and an image's results do not depend on its position in the batch or on the batch size.  Replaces
 * ResidualAligner.forward (project/models/helper_modules/alignment_old.py:316-398) with aligner_norm_type 'batch' (BatchNorm on its
 * running statistics, eps 1e-5) and no demodulation: conv_layer1, the 18 bottleneck_IR units of conv_layer2-4 and dconv_layer1-3 and
 * the three bilinear x2 up-samplings.  fp32.  The backward and the train form: the two blocks below.  The up-sampling sizes are fixed: 256 x 256.
 *
 * Source tensors, in this order (BN = weight, bias, running_mean, running_var): conv_layer1.0.weight, BN conv_layer1.1,
 * conv_layer1.2.weight; per unit of conv_layer2, 3, 4, dconv_layer1, 2, 3 (three each): BN res_layer.0, res_layer.1.weight,
 * res_layer.2.weight, res_layer.3.weight, BN res_layer.4 and, where the unit changes the channel count (the first of every stage and
 * dconv_layer1.1, dconv_layer2.1, dconv_layer3.1), shortcut_layer.0.weight, BN shortcut_layer.1.  E3DGE_ALIGNER_SOURCES in all.
 *
 * e3dge_aligner_packed_floats    floats of the packed image: A-fragment images of the convolutions, every BatchNorm folded to (a, b)
 *                                pairs, the PReLU slopes.
 * e3dge_aligner_pack             src: HOST array of n_src device pointers.  Re-run after a weight update.
 * e3dge_aligner_workspace_bytes  workspace bytes of e3dge_aligner_forward for n images (1..256) (-1: bad n).
 * e3dge_aligner_forward          the six input channels are the `split` channels of res_gt (n, split, 256, 256) followed by those of
 *                                thumb (n, 6 - split, 256, 256), or (n, 6 - split, 64, 64) read at nearest x4 with thumb_up4: split 6
 *                                is the module's forward on one tensor, split 3 the call site's cat(res_gt, interpolate(thumb)) with no
 *                                concatenated copy.  out (n, 3, 256, 256).  taps: feat1 (n, 16, 256, 256), feat2 (n, 32, 128, 128),
 *                                feat3 (n, 48, 64, 64), feat4 (n, 64, 32, 32), dfea1 (n, 32, 64, 64), dfea2 (n, 16, 128, 128) -- each
 *                                stage's output before its up-sampling -- and dfea3 (= out); any may be NULL.  Fails before any launch on
 *                                a null pointer ("null"), n out of range, a size other than 256, a split outside 0..6, a packed buffer
 *                                ("packed") or workspace ("workspace") that is too small.  49 launches (50 with the dfea3 tap).
 * e3dge_aln_conv                 debug entry for aln_conv_kernel: out (n, cout, oh, ow) = conv ksize x ksize (1 pad 0, or 3 pad 1), stride
 *                                1 or 2, of the cin input channels: `split` from in0 (n, split, height, width), the rest from in1
 *                                (n, cin - split, height, width), or (n, cin - split, height / 4, width / 4) read at nearest x4 with up4.
 *                                w (cout, cin, ksize, ksize), cout 1..64.  in_ab (cin, 2): a x + b on in-image elements (NULL: none);
 *                                epi_ab (cout, 2) and slope (cout): the affine and the PReLU after the sum (NULL: none); shortcut_mode 0:
 *                                none, 1: + shortcut[:, :, ::stride, ::stride] of a (n, cout, height, width) tensor, 2: + a
 *                                (n, cout, oh, ow) tensor.  wfrag: scratch of roundup(cout, 16) * roundup(cin ksize^2, 32) floats.  Two
 *                                launches.
 * e3dge_aln_up2                  debug entry for aln_up2_kernel: out (planes, 2 height, 2 width) = bilinear x2 of in (planes, height,
 *                                width), align_corners = False.
 * ---------------------------------------------------------------------------------------------------------------- */
#define E3DGE_ALIGNER_TAPS 7
#define E3DGE_ALIGNER_SOURCES 249
typedef struct E3dgeAlignerArgs {
    const float* packed;              /* e3dge_aligner_pack */
    int64_t packed_floats;
    const float* res_gt; const float* thumb;
    int32_t n, size, split, thumb_up4;
    float* out;
    float* taps[E3DGE_ALIGNER_TAPS];
    void* ws;
    int64_t ws_bytes;
} E3dgeAlignerArgs;
int64_t e3dge_aligner_packed_floats(void);
int e3dge_aligner_pack(float* packed, int64_t packed_floats, const float* const* src, int n_src, e3dge_stream_t stream);
int64_t e3dge_aligner_workspace_bytes(int n);
int e3dge_aligner_forward(const E3dgeAlignerArgs* args, e3dge_stream_t stream);
int e3dge_aln_conv(float* out, const float* in0, const float* in1, const float* w, const float* in_ab, const float* epi_ab, const float* slope,
                   const float* shortcut, float* wfrag, int64_t wfrag_floats, int n, int cin, int split, int up4, int cout, int height,
                   int width, int ksize, int stride, int shortcut_mode, e3dge_stream_t stream);
int e3dge_aln_up2(float* out, const float* in, int64_t planes, int height, int width, e3dge_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The 2-D residual aligner, trainable form: its kernels (csrc/aligner_bwd.h), each through a debug entry at run-time shapes.
 * Additions to ABI 17.  The network's forward with saved state and its backward (next block) are composed of them.  fp32 tensors; every per-channel sum in float64, partial sums
 * per (image, segment of 4096 pixels) folded in ascending order: no atomics, bit-reproducible.  n 1..256, channels 1..4096, height and
 * width 1..1024, at most 2^31 elements per tensor.  Every entry fails before any launch on a null pointer ("null"), a value out of
 * range or a workspace that is too small ("workspace").
 *
 * e3dge_aln_norm_ws_bytes   workspace bytes of e3dge_aln_bn_stats, e3dge_aln_norm_bwd and e3dge_aln_prelu_bwd for (n, channels, height,
 *                           width) tensors (-1: a value out of range).
 * e3dge_aln_bn_stats        BatchNorm2d's batch statistics of the `channels` channels of which `split` come from in0 (n, split, height,
 *                           width) and the rest from in1 (n, channels - split, height, width): stats (channels, 2) float64 = (mean,
 *                           biased variance); ab (channels, 2) = (gamma rstd, beta - mean gamma rstd) with rstd = 1 / sqrt(var + 1e-5),
 *                           computed in float64 and rounded once -- the in_ab / epi_ab pair of e3dge_aln_conv and the ab of
 *                           e3dge_aln_bn_apply.  Either output may be NULL (ab needs gamma and beta).  n height width >= 2.  Two launches.
 * e3dge_aln_bn_apply        out = ab[c].a in + ab[c].b, then PReLU (slope (channels), NULL: none), then the shortcut, added after that
 *                           rounding: shortcut_mode 0 none, 1 + shortcut[:, :, ::stride, ::stride] of a (n, channels, shortcut_height,
 *                           shortcut_width) tensor, 2 + a tensor of the output's shape, 3 + shortcut_ab[c].a shortcut + shortcut_ab[c].b
 *                           (the raw 1x1 branch under its own BatchNorm).  The arithmetic of e3dge_aln_conv's epilogue.  One launch.
 * e3dge_aln_norm_bwd        BatchNorm2d's backward at the input x (the two sources as above) and the incoming gy (n, channels, height,
 *                           width): dbeta = P = sum gy, dgamma = Q = sum gy xhat with xhat = (x - mean) rstd, gx = A gy + B x + C + add
 *                           in float64, rounded once (add: a tensor of gx's shape, NULL: none).  train 1: batch statistics from `stats`
 *                           (e3dge_aln_bn_stats), A = gamma rstd, B = -A Q rstd / M, C = -A P / M - B mean, M = n height width.  train
 *                           0: running_mean / running_var, B = C = 0.  gx, dgamma, dbeta: each may be NULL (not all); with train 0 and
 *                           neither parameter gradient wanted the sums are not launched and x is not read.  At most three launches.
 * e3dge_aln_prelu_bwd       gx = pre > 0 ? gy : slope[c] gy, dslope[c] = sum of gy pre over pre <= 0 (float64), from the saved
 *                           pre-activation `pre`.  gx or dslope may be NULL; ws is needed for dslope.  One or two launches.
 * e3dge_aln_up2_bwd         the adjoint of e3dge_aln_up2: gx (planes, height, width) from gy (planes, 2 height, 2 width), a gather with the
 *                           forward's own weights, float64 sum, one rounding.
 * e3dge_aln_pick_bwd        the adjoint of x[:, :, ::stride, ::stride]: gx (planes, height, width) = add + (gy at (y / stride, x / stride)
 *                           where both are multiples of stride, else 0), gy (planes, (height - 1) / stride + 1, (width - 1) / stride + 1);
 *                           add may be NULL.
 * e3dge_aln_conv_dgrad      the data gradient of e3dge_aln_conv's convolution: gx (n, cin, height, width) from gy (n, cout, oh, ow) and
 *                           w (cout, cin, ksize, ksize), cout 1..64; aln_conv_kernel's GEMM on the transposed, tap-flipped image with
 *                           M = cin (four channel tiles per launch: cin 112 takes two), stride 2 as a parity predicate of the gather.
 *                           gx = sum + add0 + add1, in that order: add0 / add1 fan-in addends of gx's shape; each may be NULL.  wfrag:
 *                           scratch of roundup(cin, 16) * roundup(cout ksize^2, 32) floats.
 * e3dge_aln_wgrad_ws_floats workspace floats of e3dge_aln_conv_wgrad: one (cout, cin ksize^2) partial per image and segment of 1024
 *                           output pixels (-1: a value out of range).
 * e3dge_aln_conv_wgrad      the weight gradient of that convolution: dw (cout, cin, ksize, ksize) = sum over images and output pixels
 *                           of gy times the forward's own gather of (in0 | in1) (zero padding, in_ab on in-image elements only, the x4
 *                           read with up4); fp32 MFMA partials per image and segment, folded in float64, images then segments ascending.
 *                           Two launches.
 * ---------------------------------------------------------------------------------------------------------------- */
int64_t e3dge_aln_norm_ws_bytes(int n, int channels, int height, int width);
int e3dge_aln_bn_stats(float* ab, double* stats, const float* in0, const float* in1, const float* gamma, const float* beta, void* ws,
                       int64_t ws_bytes, int n, int channels, int split, int height, int width, e3dge_stream_t stream);
int e3dge_aln_bn_apply(float* out, const float* in, const float* ab, const float* slope, const float* shortcut, const float* shortcut_ab, int n,
                       int channels, int height, int width, int shortcut_height, int shortcut_width, int stride, int shortcut_mode,
                       e3dge_stream_t stream);
int e3dge_aln_norm_bwd(float* gx, float* dgamma, float* dbeta, const float* gy, const float* in0, const float* in1, const float* gamma,
                       const double* stats, const float* running_mean, const float* running_var, const float* add, void* ws, int64_t ws_bytes,
                       int n, int channels, int split, int height, int width, int train, e3dge_stream_t stream);
int e3dge_aln_prelu_bwd(float* gx, float* dslope, const float* gy, const float* pre, const float* slope, void* ws, int64_t ws_bytes, int n,
                        int channels, int height, int width, e3dge_stream_t stream);
int e3dge_aln_up2_bwd(float* gx, const float* gy, int64_t planes, int height, int width, e3dge_stream_t stream);
int e3dge_aln_pick_bwd(float* gx, const float* gy, const float* add, int64_t planes, int height, int width, int stride, e3dge_stream_t stream);
int e3dge_aln_conv_dgrad(float* gx, const float* gy, const float* w, const float* add0, const float* add1, float* wfrag,
                         int64_t wfrag_floats, int n, int cin, int cout, int height, int width, int ksize, int stride, e3dge_stream_t stream);
int64_t e3dge_aln_wgrad_ws_floats(int n, int cin, int cout, int height, int width, int ksize, int stride);
int e3dge_aln_conv_wgrad(float* dw, const float* gy, const float* in0, const float* in1, const float* in_ab, float* ws, int64_t ws_floats, int n,
                         int cin, int split, int up4, int cout, int height, int width, int ksize, int stride, e3dge_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The 2-D residual aligner, trainable form: the network (csrc/aligner_train.h).  Additions to ABI 17.  One forward that keeps what the
 * backward needs, and the backward, on HIP launches only; the eval form (BatchNorm on its running statistics) and the train form (batch
 * statistics).  No allocation, no synchronisation, no atomics; bit-reproducible.  Source tensors and their order: e3dge_aligner_pack.
 *
 * e3dge_aligner_saved_bytes          bytes of the saved state for n images (-1: bad n): every convolution's raw sums, the PReLU outputs, the
 *                                    unit outputs and the three up-sampled maps, plus per call the (a, b) pairs of the batch statistics.
 * e3dge_aligner_bwd_workspace_bytes  workspace bytes of e3dge_aligner_backward for n images (-1: bad n).
 * e3dge_aligner_grad_floats          floats of the gradient buffer: one slot per source tensor in the source order, each of the tensor's
 *                                    size and shape.  The slots of running_mean / running_var are never written.
 * e3dge_aligner_grad_offset          offset of source tensor `source` (0..E3DGE_ALIGNER_SOURCES: the total) in that buffer (-1: out of range).
 * e3dge_aligner_stats_channels       BatchNorm channels in all: the statistics buffer holds (mean, biased variance) float64 pairs per
 *                                    channel, BatchNorms in source order.
 * e3dge_aligner_packed_t_floats, e3dge_aligner_pack_t   the transposed, tap-flipped A-fragment images of every convolution (the data
 *                                    gradients' operand); re-run after a weight update, like e3dge_aligner_pack.
 * e3dge_aligner_branch_count         PReLU input elements of n images: the 19 PReLUs in launch order (-1: bad n).
 * e3dge_aligner_forward_saving       e3dge_aligner_forward's arguments and results (out and taps bit for bit in the eval form) plus the saved
 *                                    state.  Every convolution writes its raw sums and an apply launch does the epilogue's arithmetic; with
 *                                    train 1 a statistics launch pair runs between them and `stats` (2 * stats_channels float64) receives
 *                                    every BatchNorm's batch mean and biased variance (src is read for gamma and beta: needed with train 1).
 *                                    Running buffers are not touched: the caller updates them from `stats`.
 * e3dge_aligner_backward             from g_out (n, 3, 256, 256), the saved state, the inputs and (train 1) `stats` of that forward:
 *                                    d_res_gt / d_thumb in the inputs' shapes with want_input (a 64^2 thumb read at nearest x4 gets the
 *                                    float64 sum of its 4 x 4 block, rows then columns ascending), and the gradient of every source tensor i
 *                                    with want[i] != 0 (HOST array of n_src bytes) at its slot of `grads`.  The weight gradient, slope and
 *                                    (eval form) BatchNorm sum launches of unwanted tensors do not run, nor the stem's data gradient without
 *                                    want_input; the data gradient chain above the stem always runs.
 * e3dge_aligner_branch_bytes         debug: one byte per PReLU input element of the saved state (1: positive), the 19 PReLUs in launch order
 *                                    (conv_layer1, then every unit's), each (n, channels, h, w).
 * Each entry fails before any launch on a null pointer ("null"), n out of range, a size other than 256, a bad split or flag, and a packed
 * ("packed"), saved ("saved"), statistics ("stats"), gradient ("gradient") or workspace ("workspace") buffer that is too small.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct E3dgeAlignerSaveArgs {
    const float* packed;              /* e3dge_aligner_pack */
    int64_t packed_floats;
    const float* const* src;          /* HOST array of n_src device pointers (train 1) */
    int32_t n_src, train;
    const float* res_gt; const float* thumb;
    int32_t n, size, split, thumb_up4;
    float* out;
    float* taps[E3DGE_ALIGNER_TAPS];
    void* saved;
    int64_t saved_bytes;
    double* stats;
    int64_t stats_doubles;
} E3dgeAlignerSaveArgs;
typedef struct E3dgeAlignerBwdArgs {
    const float* packed;              /* e3dge_aligner_pack */
    int64_t packed_floats;
    const float* packed_t;            /* e3dge_aligner_pack_t */
    int64_t packed_t_floats;
    const float* const* src;          /* HOST array of n_src device pointers */
    const uint8_t* want;              /* HOST array of n_src flags */
    int32_t n_src, train;
    const float* res_gt; const float* thumb; const float* g_out;
    int32_t n, size, split, thumb_up4, want_input, reserved;
    const void* saved;
    int64_t saved_bytes;
    const double* stats;
    float* d_res_gt; float* d_thumb;
    float* grads;
    int64_t grad_floats;
    void* ws;
    int64_t ws_bytes;
} E3dgeAlignerBwdArgs;
int64_t e3dge_aligner_saved_bytes(int n);
int64_t e3dge_aligner_bwd_workspace_bytes(int n);
int64_t e3dge_aligner_grad_floats(void);
int64_t e3dge_aligner_grad_offset(int source);
int64_t e3dge_aligner_stats_channels(void);
int64_t e3dge_aligner_packed_t_floats(void);
int64_t e3dge_aligner_branch_count(int n);
int e3dge_aligner_pack_t(float* packed_t, int64_t packed_t_floats, const float* const* src, int n_src, e3dge_stream_t stream);
int e3dge_aligner_forward_saving(const E3dgeAlignerSaveArgs* args, e3dge_stream_t stream);
int e3dge_aligner_backward(const E3dgeAlignerBwdArgs* args, e3dge_stream_t stream);
int e3dge_aligner_branch_bytes(uint8_t* out, int64_t out_bytes, const float* packed, int64_t packed_floats, const void* saved, int64_t saved_bytes,
                               int n, int train, e3dge_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The camera-pose predictor, forward, eval form (csrc/volume_disc.hip).  Additions to ABI 17.  No allocation, no synchronisation, no
 * atomics; bit-reproducible, and an image's results do not depend on its position in the batch or on the batch size.  Replaces
 * VolumeRenderDiscriminator.forward (project/models/stylesdf_model.py:1369-1419): the 1x1 stem, log2(size) - 1 VolumeRenderResBlocks
 * of two 3x3 CoordConv layers with AvgPool2d(2) and the (out + skip) / sqrt(2) merge, and the 2x2 final layer.  fp32.  `size` is
 * renderer_spatial_output_dim: 16, 32, 64 or 128.
 *
 * Source tensors, in state-dict order: convs.0.conv.weight, convs.0.activation.bias; per block i = 1 ..: convs.i.conv1.conv.conv.weight,
 * convs.i.conv1.activation.bias, convs.i.conv2.conv.conv.weight, convs.i.conv2.activation.bias and, where the block changes the channel
 * count, convs.i.skip.conv.weight, convs.i.skip.conv.bias; final_conv.conv.weight, final_conv.conv.bias.
 *
 * e3dge_vdisc_packed_floats   floats of the packed image at `size`: per layer its A-fragment image, roundup(cout, 16) * roundup(K, 32)
 *                             floats with K = cin (stem, skip) or 9 (cin + 2) (CoordConv, the reference's channel order), then its cout
 *                             bias floats; the final layer's weight as it is, 3 * 4 cin floats, and its 3 bias floats (-1: unsupported
 *                             size).
 * e3dge_vdisc_pack_weights    ptrs: HOST array of n device pointers, n as the list above gives it at `size`.  Re-run after a weight update.
 * e3dge_vdisc_ws_bytes        workspace bytes of e3dge_vdisc_forward for n images (1..256): two block inputs / outputs, one conv1 output
 *                             and one skip output of the largest layer each; neither a concatenated nor a pre-pool tensor (-1: bad n or size).
 * e3dge_vdisc_forward         images (n, 3, size, size) -> logits (n, 1), viewpoints (n, 2).  taps[0]: the stem's output (n, c0, size,
 *                             size); taps[1 + b]: block b's output (n, cout, size >> (b + 1), size >> (b + 1)); any may be NULL.  Fails
 *                             before any launch on a null pointer, an unsupported size, n outside 1..256 or a workspace that is too
 *                             small.  8 / 11 / 14 / 17 launches at size 16 / 32 / 64 / 128.
 * e3dge_vdisc_conv            debug entry: one launch of vdisc_conv_kernel (_FINAL: of vdisc_final_kernel) after packing w into wfrag, on in
 *                             (n, cin, height, width).
 *                             form E3DGE_VDISC_FORM_STEM: out (n, cout, height, width) = lrelu(conv1x1 + bias), w (cout, cin, 1, 1);
 *                             _CONV: lrelu(conv3x3 pad 1 of cat(in, yy, xx) + bias), w (cout, cin + 2, 3, 3), height, width >= 2;
 *                             _CONV_POOL: out (n, cout, height / 2, width / 2) = (avgpool2(that) + s) / sqrt(2) with s = skip
 *                             (n, cout, height / 2, width / 2) (skip_mode E3DGE_VDISC_SKIP_READ) or avgpool2(skip (n, cout, height,
 *                             width)) (_SKIP_POOL); _SKIP: out (n, cout, height / 2, width / 2) = conv1x1(avgpool2(in)) + bias;
 *                             _FINAL: out (n, cout, 1, 1) = conv2x2 + bias of the 2 x 2 map (height = width = 2, cout 1..64), w
 *                             (cout, cin, 2, 2), summed in float64.  lrelu: slope 0.2, scale 1.  The pooled forms refuse odd planes.
 *                             wfrag: scratch of roundup(cout, 16) * roundup(K, 32) floats (_FINAL: cout * 4 cin).  Two launches.
 * ---------------------------------------------------------------------------------------------------------------- */
#define E3DGE_VDISC_MAX_BLOCKS 6
#define E3DGE_VDISC_TAPS 7
#define E3DGE_VDISC_FORM_STEM 0
#define E3DGE_VDISC_FORM_CONV 1
#define E3DGE_VDISC_FORM_CONV_POOL 2
#define E3DGE_VDISC_FORM_SKIP 3
#define E3DGE_VDISC_FORM_FINAL 4
#define E3DGE_VDISC_SKIP_READ 1
#define E3DGE_VDISC_SKIP_POOL 2
typedef struct E3dgeVdiscArgs {
    const float* packed;              /* e3dge_vdisc_pack_weights */
    const float* images;
    int32_t n, size;
    float* logits; float* viewpoints;
    float* taps[E3DGE_VDISC_TAPS];
    void* ws;
    int64_t ws_bytes;
} E3dgeVdiscArgs;
int64_t e3dge_vdisc_packed_floats(int size);
int e3dge_vdisc_pack_weights(float* image, const float* const* ptrs, int n, int size, e3dge_stream_t stream);
int64_t e3dge_vdisc_ws_bytes(int n, int size);
int e3dge_vdisc_forward(const E3dgeVdiscArgs* args, e3dge_stream_t stream);
int e3dge_vdisc_conv(float* out, const float* in, const float* w, const float* bias, const float* skip, float* wfrag, int64_t wfrag_floats,
                     int n, int cin, int cout, int height, int width, int form, int skip_mode, e3dge_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* E3DGE_HIP_H */
