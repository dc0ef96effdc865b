// ArcFace identity term, forward: the loss_id / ID_SIM columns of the evaluated image and the `id_lambda` term of the reference's 2-D
// reconstruction loss.
//
// Reference: IDLoss.forward / extract_feats (project/losses/id_loss.py:23-55), Backbone(112, 50, 'ir_se') in eval form
// (models/encoders/model_irse.py:8-51), bottleneck_IR_SE / SEModule / l2_norm (models/helper_modules/helpers.py:83-224), called from
// Loss.calc_2d_rec_loss (project/losses/builder.py:156-168, 175, 182).
//
//   x[:, :, 35:223, 32:220] -> adaptive average 112^2 -> conv 3->64, BN, PReLU -> 24 units -> BN2d, flatten, Linear 25088->512, BN1d, x / |x|
//   unit(in, depth, stride):  res = SE(BN(conv3x3_stride(PReLU(conv3x3(BN(x))))));  out = res + (in == depth ? x[::stride] : BN(conv1x1_stride(x)))
//
// Kernels (103 launches for one embed, whatever the batch; one more for the dot products):
//   prep_kernel   crop and both adaptive averages in one launch (the 256^2 average only where the crop needs it, each value rounded
//                 to fp32 as the reference's separate pool would).
//   conv_kernel   the implicit GEMM of conv_igemm.h (M = output channels, K = (ci, r, s), weights from the packed A-fragment image) with
//                 N = the output pixels of ONE image per workgroup column.  Gather: zero padding, and an optional per-input-channel
//                 affine on in-image elements (the leading BN: padding stays 0, so it cannot be folded into the weights).  Epilogue:
//                 the sum of the two accumulators, an optional per-output-channel affine (trailing BN) and an optional PReLU.  With
//                 `plane` it also writes one partial plane sum per (image, channel, pixel tile): the tile's columns in ascending order
//                 per lane, then a fixed butterfly over the 16 lanes.  Tiles never straddle images and the tile width depends on the
//                 layer alone, so an image's values and partials do not depend on the batch.
//   se_kernel     one workgroup per image: the partials in tile order, / HW, C -> C/16 ReLU, C/16 -> C sigmoid.
//   merge_kernel  out = res * gate + shortcut (two roundings, as the reference), the shortcut picked with the stride or read.
//   head_kernel   BN2d while loading, then 4 output rows x 1/7 of K per workgroup for up to 8 images at once (the 51 MB matrix is
//                 read once per 8 images); head_fold_kernel adds the seven slices in order, bias, BN1d, L2 normalisation.
//   dot_kernel    the three dot products per sample and the two batch means in sample order.
// The backward (the gradient to the y_hat images, 104 launches) is idnet_bwd.h; the conv, se, merge and head fold kernels have a SAVE
// instantiation that keeps what it needs.
// Measured times, the per-kernel split and what bounds each kernel: DESIGN.md 4.11d.
// The E0 image encoder (encoder.h, included at the end) runs the same units at a run-time size with a driver of its own.
#include "conv_igemm.h"

namespace e3dge {

constexpr int kIdUnits = E3DGE_IDNET_UNITS, kIdConvs = E3DGE_IDNET_CONVS, kIdBns = E3DGE_IDNET_BNS;
constexpr int kIdNet = 112, kIdEmbed = 512, kIdHeadK = 512 * 7 * 7;
constexpr int kIdHeadSlices = 7, kIdHeadSliceK = kIdHeadK / kIdHeadSlices, kIdHeadRows = 4, kIdHeadImgs = 8;
static_assert(kIdHeadSliceK * kIdHeadSlices == kIdHeadK && kIdHeadSliceK % 4 == 0, "head slices");

struct IdUnit { int cin, depth, stride, shortcut; };            // shortcut: index of the 1x1 branch (0..2) or -1
static IdUnit id_unit(int u) {
    if (u == 0) return {64, 64, 2, -1};
    if (u < 3) return {64, 64, 1, -1};
    if (u == 3) return {64, 128, 2, 0};
    if (u < 7) return {128, 128, 1, -1};
    if (u == 7) return {128, 256, 2, 1};
    if (u < 21) return {256, 256, 1, -1};
    if (u == 21) return {256, 512, 2, 2};
    return {512, 512, 1, -1};
}
static int id_tap_of_unit(int u) { return u == 0 ? 2 : u == 3 ? 3 : u == 7 ? 4 : u == 21 ? 5 : u == 23 ? 6 : -1; }

// offsets (floats) into the packed image
struct IdLayout {
    int cin[kIdConvs], cout[kIdConvs], ks[kIdConvs];
    int64_t w_off[kIdConvs];
    int bn_c[kIdBns];
    int64_t bn_off[kIdBns];                       // (a, b) pairs
    int prelu_c[kIdUnits + 1];
    int64_t prelu_off[kIdUnits + 1], fc1_off[kIdUnits], fc2_off[kIdUnits], head_w_off, head_b_off, total;
};

static const IdLayout& id_layout() {
    static const IdLayout lay = [] {
        IdLayout l{};
        int64_t off = 0;
        auto take = [&](int64_t floats) { const int64_t at = off; off += (floats + 63) / 64 * 64; return at; };
        auto conv = [&](int i, int ci, int co, int ks) { l.cin[i] = ci; l.cout[i] = co; l.ks[i] = ks; l.w_off[i] = take((int64_t)co * ig_kpad(ci * ks * ks)); };
        auto bn = [&](int i, int c) { l.bn_c[i] = c; l.bn_off[i] = take(2 * (int64_t)c); };
        conv(0, 3, 64, 3); bn(0, 64);
        l.prelu_c[0] = 64; l.prelu_off[0] = take(64);
        for (int u = 0; u < kIdUnits; ++u) {
            const IdUnit q = id_unit(u);
            conv(1 + 2 * u, q.cin, q.depth, 3); conv(2 + 2 * u, q.depth, q.depth, 3);
            bn(1 + 2 * u, q.cin); bn(2 + 2 * u, q.depth);
            l.prelu_c[1 + u] = q.depth; l.prelu_off[1 + u] = take(q.depth);
            l.fc1_off[u] = take((int64_t)q.depth * (q.depth / 16)); l.fc2_off[u] = take((int64_t)q.depth * (q.depth / 16));
            if (q.shortcut >= 0) { conv(49 + q.shortcut, q.cin, q.depth, 1); bn(49 + q.shortcut, q.depth); }
        }
        bn(52, 512); bn(53, kIdEmbed);
        l.head_w_off = take((int64_t)kIdEmbed * kIdHeadK); l.head_b_off = take(kIdEmbed);
        l.total = off;
        return l;
    }();
    return lay;
}

// ---- packing ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) idnet_pack_bn_kernel(float* __restrict__ dst, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ mean, const float* __restrict__ var, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float a = __fdiv_rn(gamma[c], __fsqrt_rn(__fadd_rn(var[c], 1e-5f)));
    dst[2 * c] = a;
    dst[2 * c + 1] = __fsub_rn(beta[c], __fmul_rn(mean[c], a));
}

// ---- crop and pool ------------------------------------------------------------------------------------------------------------
struct IdPrepArgs { float* out; const float* set[3]; int n_per_set, n, H, W; };

__global__ void __launch_bounds__(256) idnet_prep_kernel(IdPrepArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)a.n * 3 * kIdNet * kIdNet) return;
    const int ox = (int)(i % kIdNet), oy = (int)((i / kIdNet) % kIdNet);
    const int64_t plane = i / (kIdNet * kIdNet);                    // img * 3 + c
    const int img = (int)(plane / 3), c = (int)(plane - (int64_t)img * 3);
    const int s = img / a.n_per_set, j = img - s * a.n_per_set;
    const float* base = s == 0 ? a.set[0] : s == 1 ? a.set[1] : a.set[2];
    const float* __restrict__ src = base + ((int64_t)j * 3 + c) * a.H * a.W;
    // PyTorch's adaptive windows: [floor(i in / out), ceil((i + 1) in / out))
    const int ys = oy * 188 / kIdNet, ye = ((oy + 1) * 188 + kIdNet - 1) / kIdNet;
    const int xs = ox * 188 / kIdNet, xe = ((ox + 1) * 188 + kIdNet - 1) / kIdNet;
    float sum = 0.0f;
    for (int y = ys; y < ye; ++y)
        for (int x = xs; x < xe; ++x) {
            const int Y = 35 + y, X = 32 + x;                        // id_loss.py:24, on the 256 x 256 grid
            const int hs = (int)((int64_t)Y * a.H / 256), he = (int)((((int64_t)Y + 1) * a.H + 255) / 256);
            const int ws = (int)((int64_t)X * a.W / 256), we = (int)((((int64_t)X + 1) * a.W + 255) / 256);
            float v = 0.0f;
            for (int h = hs; h < he; ++h)
                for (int w = ws; w < we; ++w) v = __fadd_rn(v, src[(int64_t)h * a.W + w]);
            v = __fdiv_rn(__fdiv_rn(v, (float)(he - hs)), (float)(we - ws));
            sum = __fadd_rn(sum, v);
        }
    a.out[i] = __fdiv_rn(__fdiv_rn(sum, (float)(ye - ys)), (float)(xe - xs));
}

// ---- convolution --------------------------------------------------------------------------------------------------------------
struct IdConvArgs {
    float* out; const float* in; const float* wfrag;
    const float2* in_ab; const float2* epi_ab; const float* slope; float* plane;
    int Cin, IH, IW, Cout, OH, OW, K, KS4, tiles;
    unsigned char* mask; int n_mask;                // SAVE only: the PReLU branch of the leading n_mask images
};

// SAVE (here and in the se, merge and head fold kernels): the state-saving form for the backward (idnet_bwd.h).  It is a template
// parameter and not a null check so that the plain forward runs the instructions it ran before the backward existed.
template <int KS_, int STRIDE, int NT, bool SAVE = false>
__global__ void __launch_bounds__(256) idnet_conv_kernel(IdConvArgs a) {
    constexpr int BN = IgTile<NT>::BN, ROWS = IgTile<NT>::ROWS, PER = IgTile<NT>::PER;
    constexpr int PAD = KS_ == 3 ? 1 : 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mt = blockIdx.y * (kIgBM / 16) + wave;
    const int OHW = a.OH * a.OW, IH = a.IH, IW = a.IW, K = a.K;
    const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
    const int sn = tid % BN, srow = tid / BN;
    const int spix = tile * BN + sn;
    const bool n_ok = spix < OHW;
    const int soy = spix / a.OW, sox = spix - soy * a.OW;
    const int iy0 = soy * STRIDE - PAD, ix0 = sox * STRIDE - PAD;
    const float* __restrict__ src = a.in + (int64_t)img * a.Cin * IH * IW;
    const float2* __restrict__ in_ab = a.in_ab;
    auto fetch = [&](int k0, float (&v)[PER]) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = k0 + srow + i * ROWS;
            const auto [ci, r, s] = ig_decode<KS_>(k);
            const int iy = iy0 + r, ix = ix0 + s;
            float x = 0.0f;
            if (n_ok && k < K && iy >= 0 && iy < IH && ix >= 0 && ix < IW) {
                x = src[((int64_t)ci * IH + iy) * IW + ix];
                if (in_ab) { const float2 ab = in_ab[ci]; x = __fmaf_rn(ab.x, x, ab.y); }   // the leading BN; padding stays 0
            }
            v[i] = x;
        }
    };
    f32x4 acc[NT][2];
    ig_k_loop<NT, 2, false>(acc, a.wfrag + (int64_t)mt * a.KS4 * 64 + lane, a.KS4 / (kIgKC / 4), true, fetch, [](int, bool) {});
    // C/D fragment: lane l, register r holds D[4 (l >> 4) + r][l & 15]
    float psum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int row0 = mt * 16 + 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int pix = tile * BN + t * 16 + (lane & 15);
        const bool ok = pix < OHW;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + r;
            float v = __fadd_rn(acc[t][0][r], acc[t][1][r]);
            if (a.epi_ab) { const float2 e = a.epi_ab[row]; v = __fmaf_rn(e.x, v, e.y); }
            if (a.slope) {
                if (SAVE && ok && img < a.n_mask) a.mask[((int64_t)img * a.Cout + row) * OHW + pix] = v > 0.0f;
                v = v > 0.0f ? v : __fmul_rn(a.slope[row], v);
            }
            if (ok) {
                a.out[((int64_t)img * a.Cout + row) * OHW + pix] = v;
                psum[r] = __fadd_rn(psum[r], v);
            }
        }
    }
    if (a.plane) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float s = psum[r];
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) s = __fadd_rn(s, __shfl_xor(s, off, kWave));
            if ((lane & 15) == 0) a.plane[((int64_t)img * a.Cout + row0 + r) * a.tiles + tile] = s;
        }
    }
}

// ---- SE gate ------------------------------------------------------------------------------------------------------------------
template <bool SAVE>
__global__ void __launch_bounds__(256) idnet_se_kernel(float* __restrict__ gate, const float* __restrict__ plane, const float* __restrict__ fc1,
                                                       const float* __restrict__ fc2, int C, int tiles, int HW, float* __restrict__ gate_save,
                                                       float* __restrict__ hid_save, int n_saved) {
    __shared__ float mean[512];
    __shared__ float hid[32];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, Ch = C / 16;
    for (int c = tid; c < C; c += 256) {
        const float* p = plane + ((int64_t)img * C + c) * tiles;
        float s = 0.0f;
        for (int t = 0; t < tiles; ++t) s = __fadd_rn(s, p[t]);
        mean[c] = __fdiv_rn(s, (float)HW);
    }
    __syncthreads();
    for (int j = wave; j < Ch; j += 4) {
        float s = 0.0f;
        for (int c = lane; c < C; c += 64) s = __fmaf_rn(fc1[j * C + c], mean[c], s);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s = __fadd_rn(s, __shfl_xor(s, off, kWave));
        if (lane == 0) {
            hid[j] = fmaxf(s, 0.0f);
            if (SAVE && img < n_saved) hid_save[(int64_t)img * Ch + j] = hid[j];
        }
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        float s = 0.0f;
        for (int j = 0; j < Ch; ++j) s = __fmaf_rn(fc2[c * Ch + j], hid[j], s);
        const float g = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-s)));
        gate[(int64_t)img * C + c] = g;
        if (SAVE && img < n_saved) gate_save[(int64_t)img * C + c] = g;
    }
}

// ---- unit merge ---------------------------------------------------------------------------------------------------------------
template <bool SAVE>
__global__ void __launch_bounds__(256) idnet_merge_kernel(float* __restrict__ out, const float* __restrict__ res, const float* __restrict__ gate,
                                                          const float* __restrict__ sc, const float* __restrict__ xin, int OH, int OW, int IH,
                                                          int IW, int stride, int64_t total, float* __restrict__ res_save,
                                                          int64_t saved_total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int OHW = OH * OW;
    const int64_t plane = i / OHW;                                   // img * C + c
    const int pix = (int)(i - plane * OHW), oy = pix / OW, ox = pix - oy * OW;
    const float s = sc ? sc[i] : xin[(plane * IH + (int64_t)oy * stride) * IW + ox * stride];
    const float r = res[i];
    if (SAVE && i < saved_total) res_save[i] = r;                    // the leading images are the ones that get a gradient
    out[i] = __fadd_rn(__fmul_rn(r, gate[plane]), s);                // helpers.py:158, :223
}

// ---- head ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) idnet_head_kernel(float* __restrict__ part, const float* __restrict__ x, const float* __restrict__ w,
                                                         const float2* __restrict__ ab, int n) {
    __shared__ float red[4][kIdHeadRows * kIdHeadImgs];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int o0 = blockIdx.x * kIdHeadRows, k0 = blockIdx.y * kIdHeadSliceK;
    for (int i0 = 0; i0 < n; i0 += kIdHeadImgs) {
        const int cnt = n - i0 < kIdHeadImgs ? n - i0 : kIdHeadImgs;
        float acc[kIdHeadRows][kIdHeadImgs];
#pragma unroll
        for (int r = 0; r < kIdHeadRows; ++r)
#pragma unroll
            for (int i = 0; i < kIdHeadImgs; ++i) acc[r][i] = 0.0f;
        for (int k4 = tid; k4 < kIdHeadSliceK / 4; k4 += 256) {
            const int k = k0 + k4 * 4;
            float4 wv[kIdHeadRows];
#pragma unroll
            for (int r = 0; r < kIdHeadRows; ++r) wv[r] = *reinterpret_cast<const float4*>(w + (int64_t)(o0 + r) * kIdHeadK + k);
            const float2 e0 = ab[k / 49], e1 = ab[(k + 1) / 49], e2 = ab[(k + 2) / 49], e3 = ab[(k + 3) / 49];
#pragma unroll
            for (int i = 0; i < kIdHeadImgs; ++i) {
                if (i < cnt) {
                    float4 xv = *reinterpret_cast<const float4*>(x + (int64_t)(i0 + i) * kIdHeadK + k);
                    xv.x = __fmaf_rn(e0.x, xv.x, e0.y); xv.y = __fmaf_rn(e1.x, xv.y, e1.y);
                    xv.z = __fmaf_rn(e2.x, xv.z, e2.y); xv.w = __fmaf_rn(e3.x, xv.w, e3.y);
#pragma unroll
                    for (int r = 0; r < kIdHeadRows; ++r) {
                        float s = acc[r][i];
                        s = __fmaf_rn(wv[r].x, xv.x, s); s = __fmaf_rn(wv[r].y, xv.y, s);
                        s = __fmaf_rn(wv[r].z, xv.z, s); s = __fmaf_rn(wv[r].w, xv.w, s);
                        acc[r][i] = s;
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kIdHeadRows; ++r)
#pragma unroll
            for (int i = 0; i < kIdHeadImgs; ++i) {
                float s = acc[r][i];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) s = __fadd_rn(s, __shfl_xor(s, off, kWave));
                if (lane == 0) red[wave][r * kIdHeadImgs + i] = s;
            }
        __syncthreads();
        if (tid < kIdHeadRows * kIdHeadImgs) {
            const int i = tid % kIdHeadImgs, r = tid / kIdHeadImgs;
            if (i < cnt)
                part[((int64_t)blockIdx.y * n + i0 + i) * kIdEmbed + o0 + r] =
                    __fadd_rn(__fadd_rn(__fadd_rn(red[0][tid], red[1][tid]), red[2][tid]), red[3][tid]);
        }
        __syncthreads();
    }
}

template <bool SAVE>
__global__ void __launch_bounds__(kIdEmbed) idnet_head_fold_kernel(float* __restrict__ emb, float* __restrict__ tap, const float* __restrict__ part,
                                                                   const float* __restrict__ bias, const float2* __restrict__ ab, int n,
                                                                   float* __restrict__ save_v, float* __restrict__ save_f,
                                                                   float* __restrict__ save_norm, int n_saved) {
    __shared__ float sq[kIdEmbed];
    const int img = blockIdx.x, o = threadIdx.x;
    float v = 0.0f;
#pragma unroll
    for (int s = 0; s < kIdHeadSlices; ++s) v = __fadd_rn(v, part[((int64_t)s * n + img) * kIdEmbed + o]);
    v = __fadd_rn(v, bias[o]);
    const float2 e = ab[o];
    v = __fmaf_rn(e.x, v, e.y);
    if (tap) tap[(int64_t)img * kIdEmbed + o] = v;
    sq[o] = __fmul_rn(v, v);
    __syncthreads();
    for (int off = kIdEmbed / 2; off > 0; off >>= 1) {
        if (o < off) sq[o] = __fadd_rn(sq[o], sq[o + off]);
        __syncthreads();
    }
    const float norm = __fsqrt_rn(sq[0]), f = __fdiv_rn(v, norm);
    emb[(int64_t)img * kIdEmbed + o] = f;                                       // helpers.py:89-92
    if (SAVE && img < n_saved) {
        save_v[(int64_t)img * kIdEmbed + o] = v;
        save_f[(int64_t)img * kIdEmbed + o] = f;
        if (o == 0) save_norm[img] = norm;
    }
}

// ---- dot products -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(192) idnet_dot_kernel(float* __restrict__ dots, float* __restrict__ loss_out, float* __restrict__ sim_out,
                                                        const float* __restrict__ fh, const float* __restrict__ fy, const float* __restrict__ fx,
                                                        int batch) {
    __shared__ float d[3];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* p = w == 2 ? fy : fh;                               // id_loss.py:42-44
    const float* q = w == 0 ? fy : fx;
    float loss = 0.0f;
    double sim = 0.0;
    for (int b = 0; b < batch; ++b) {
        float s = 0.0f;
        for (int c = lane; c < kIdEmbed; c += 64) s = __fmaf_rn(p[(int64_t)b * kIdEmbed + c], q[(int64_t)b * kIdEmbed + c], s);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s = __fadd_rn(s, __shfl_xor(s, off, kWave));
        if (lane == 0) { d[w] = s; dots[b * 3 + w] = s; }
        __syncthreads();
        if (threadIdx.x == 0) { loss = __fadd_rn(loss, __fsub_rn(1.0f, d[0])); sim += (double)d[0] - (double)d[2]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (loss_out) loss_out[0] = __fdiv_rn(loss, (float)batch);
        if (sim_out) sim_out[0] = (float)(sim / (double)batch);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
static int id_out_size(int in, int stride) { return (in - 1) / stride + 1; }     // 3x3 pad 1 and 1x1 pad 0 alike

// the tile width comes from the layer alone (two images counted), so that the partial plane sums of an image do not depend on the batch
static int id_tile_width(int OHW, int Cout) { return ig_tile_width(OHW, 2, Cout / kIgBM); }
static int id_tiles(int OHW, int Cout) { const int bn = 16 * id_tile_width(OHW, Cout); return (OHW + bn - 1) / bn; }

static int id_conv(float* out, const float* in, const float* wfrag, const float* in_ab, const float* epi_ab, const float* slope, float* plane,
                   int n, int Cin, int Cout, int IH, int IW, int ks, int stride, hipStream_t st, unsigned char* mask = nullptr, int n_mask = 0) {
    IdConvArgs a;
    a.mask = mask; a.n_mask = n_mask;
    a.out = out; a.in = in; a.wfrag = wfrag;
    a.in_ab = reinterpret_cast<const float2*>(in_ab); a.epi_ab = reinterpret_cast<const float2*>(epi_ab); a.slope = slope; a.plane = plane;
    a.Cin = Cin; a.IH = IH; a.IW = IW; a.Cout = Cout; a.OH = id_out_size(IH, stride); a.OW = id_out_size(IW, stride);
    a.K = Cin * ks * ks; a.KS4 = ig_kpad(a.K) / 4;
    const int OHW = a.OH * a.OW, nt = id_tile_width(OHW, Cout);
    a.tiles = id_tiles(OHW, Cout);
    const dim3 grid((unsigned)((int64_t)n * a.tiles), (unsigned)(Cout / kIgBM));
    ig_dispatch_nt(nt, [&](auto nt_c) {
        constexpr int NT = decltype(nt_c)::value;
        if (mask && ks == 3 && stride == 1) idnet_conv_kernel<3, 1, NT, true><<<grid, dim3(256), 0, st>>>(a);   // every PReLU follows a 3x3 of stride 1
        else if (ks == 3 && stride == 1) idnet_conv_kernel<3, 1, NT><<<grid, dim3(256), 0, st>>>(a);
        else if (ks == 3) idnet_conv_kernel<3, 2, NT><<<grid, dim3(256), 0, st>>>(a);
        else if (stride == 1) idnet_conv_kernel<1, 1, NT><<<grid, dim3(256), 0, st>>>(a);
        else idnet_conv_kernel<1, 2, NT><<<grid, dim3(256), 0, st>>>(a);
    });
    return check_launch("idnet(conv)");
}

struct IdWs { int64_t net_in, buf[3], res, sc, plane, gate, part, total_bytes; int64_t plane_per_img; };

static bool id_ws(int64_t n, IdWs* d) {
    if (n < 1 || n > 4096) return false;
    int64_t off = 0;
    auto take = [&](int64_t floats) { const int64_t at = off; off += (floats + 63) / 64 * 64; return at; };
    d->net_in = take(n * 3 * kIdNet * kIdNet);
    for (int q = 0; q < 3; ++q) d->buf[q] = take(n * 64 * kIdNet * kIdNet);            // unit input, unit output, first 3x3's output
    d->res = take(n * 64 * 56 * 56);                                                   // the largest strided output: unit 0
    d->sc = take(n * 128 * 28 * 28);                                                   // the largest 1x1 branch: unit 3
    int64_t per = 0;
    int size = kIdNet;
    for (int u = 0; u < kIdUnits; ++u) {
        const IdUnit q = id_unit(u);
        size = id_out_size(size, q.stride);
        const int64_t p = (int64_t)q.depth * id_tiles(size * size, q.depth);
        if (p > per) per = p;
    }
    d->plane_per_img = per;
    d->plane = take(n * per);
    d->gate = take(n * 512);
    d->part = take((int64_t)kIdHeadSlices * n * kIdEmbed);
    d->total_bytes = off * (int64_t)sizeof(float);
    return true;
}

// what the saving forward keeps for the backward (idnet_bwd.h), tensor after tensor, each for all n_saved images: offsets in bytes
struct IdSaved {
    int64_t res[kIdUnits], gate[kIdUnits], hid[kIdUnits], v, f, norm, mask[kIdUnits + 1], total_bytes;
    int mask_c[kIdUnits + 1], mask_size[kIdUnits + 1];
};

static bool id_saved(int64_t n, IdSaved* d) {
    if (n < 1 || n > 4096) return false;
    int64_t off = 0;
    auto take = [&](int64_t bytes) { const int64_t at = off; off += (bytes + 255) / 256 * 256; return at; };
    int size = kIdNet;
    d->mask_c[0] = 64; d->mask_size[0] = kIdNet;
    for (int u = 0; u < kIdUnits; ++u) {
        const IdUnit q = id_unit(u);
        d->mask_c[1 + u] = q.depth; d->mask_size[1 + u] = size;       // the first 3x3 has stride 1
        size = id_out_size(size, q.stride);
        d->res[u] = take(n * q.depth * size * size * (int64_t)sizeof(float));
        d->gate[u] = take(n * q.depth * (int64_t)sizeof(float));
        d->hid[u] = take(n * (q.depth / 16) * (int64_t)sizeof(float));
    }
    d->v = take(n * kIdEmbed * (int64_t)sizeof(float));
    d->f = take(n * kIdEmbed * (int64_t)sizeof(float));
    d->norm = take(n * (int64_t)sizeof(float));
    for (int i = 0; i <= kIdUnits; ++i) d->mask[i] = take(n * d->mask_c[i] * d->mask_size[i] * d->mask_size[i]);
    d->total_bytes = off;
    return true;
}

}  // namespace e3dge

using namespace e3dge;

extern "C" int64_t e3dge_idnet_packed_floats(void) { return id_layout().total; }

extern "C" int e3dge_idnet_pack_weights(float* packed, const E3dgeIdnetPackSrc* src, e3dge_stream_t stream) {
    E3DGE_REQUIRE(packed && src, "idnet_pack_weights: null pointer");
    const E3dgeIdnetPackSrc& s = *src;
    for (int i = 0; i < kIdConvs; ++i) E3DGE_REQUIRE(s.conv_w[i], "idnet_pack_weights: null pointer (conv %d)", i);
    for (int i = 0; i < kIdBns; ++i)
        E3DGE_REQUIRE(s.bn_weight[i] && s.bn_bias[i] && s.bn_mean[i] && s.bn_var[i], "idnet_pack_weights: null pointer (bn %d)", i);
    for (int i = 0; i <= kIdUnits; ++i) E3DGE_REQUIRE(s.prelu[i], "idnet_pack_weights: null pointer (prelu %d)", i);
    for (int i = 0; i < kIdUnits; ++i) E3DGE_REQUIRE(s.se_fc1[i] && s.se_fc2[i], "idnet_pack_weights: null pointer (se %d)", i);
    E3DGE_REQUIRE(s.head_w && s.head_b, "idnet_pack_weights: null pointer (head)");
    const IdLayout& l = id_layout();
    hipStream_t st = as_stream(stream);
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    auto copy = [&](int64_t off, const float* from, int64_t n) { ig_copy(packed + off, from, n, 1.0f, 0, st); };
    for (int i = 0; i < kIdConvs; ++i) ig_pack(packed + l.w_off[i], s.conv_w[i], l.cin[i], l.cout[i], l.ks[i], 1.0f, st);
    for (int i = 0; i < kIdBns; ++i)
        idnet_pack_bn_kernel<<<blocks(l.bn_c[i]), dim3(256), 0, st>>>(packed + l.bn_off[i], s.bn_weight[i], s.bn_bias[i], s.bn_mean[i], s.bn_var[i],
                                                                     l.bn_c[i]);
    for (int i = 0; i <= kIdUnits; ++i) copy(l.prelu_off[i], s.prelu[i], l.prelu_c[i]);
    for (int u = 0; u < kIdUnits; ++u) {
        const int64_t m = (int64_t)id_unit(u).depth * (id_unit(u).depth / 16);
        copy(l.fc1_off[u], s.se_fc1[u], m);
        copy(l.fc2_off[u], s.se_fc2[u], m);
    }
    copy(l.head_w_off, s.head_w, (int64_t)kIdEmbed * kIdHeadK);
    copy(l.head_b_off, s.head_b, kIdEmbed);
    return check_launch("idnet_pack_weights");
}

extern "C" int64_t e3dge_idnet_ws_bytes(int n_images) {
    IdWs d;
    if (!id_ws(n_images, &d)) {
        fail(E3DGE_ERR_INVALID_ARG, "idnet_ws_bytes: n_images=%d (1..4096)", n_images);
        return -1;
    }
    return d.total_bytes;
}

// e3dge_idnet_embed, and with `saved` the saving forward: the same launches, which also fill `saved` for the leading n_saved images
static int id_embed(const E3dgeIdnetArgs& a, void* saved, int64_t saved_bytes, int n_saved, bool saving, e3dge_stream_t stream) {
    E3DGE_REQUIRE(a.n_sets >= 1 && a.n_sets <= 3, "idnet_embed: n_sets=%d (1..3)", a.n_sets);
    E3DGE_REQUIRE(a.n_per_set >= 1 && a.n_per_set <= 4096 / a.n_sets, "idnet_embed: n_per_set=%d (n_sets * n_per_set in 1..4096)", a.n_per_set);
    E3DGE_REQUIRE(a.packed && a.embeddings && a.ws, "idnet_embed: null pointer");
    for (int s = 0; s < a.n_sets; ++s) E3DGE_REQUIRE(a.images[s], "idnet_embed: null pointer (image set %d)", s);
    E3DGE_REQUIRE(a.height >= 1 && a.width >= 1 && a.height <= 32768 && a.width <= 32768, "idnet_embed: height=%d width=%d (1..32768)", a.height,
                  a.width);
    const int n = a.n_per_set * a.n_sets;
    IdWs d;
    E3DGE_REQUIRE(id_ws(n, &d), "idnet_embed: n_images=%d", n);
    E3DGE_REQUIRE(a.ws_bytes >= d.total_bytes, "idnet_embed: workspace of %lld bytes, %lld needed", (long long)a.ws_bytes, (long long)d.total_bytes);
    IdSaved sv{};
    if (saving) {
        E3DGE_REQUIRE(n_saved >= 1 && n_saved <= n, "idnet_embed_save: n_saved=%d (1..%d)", n_saved, n);
        E3DGE_REQUIRE(saved, "idnet_embed_save: null pointer (saved)");
        E3DGE_REQUIRE(id_saved(n_saved, &sv) && saved_bytes >= sv.total_bytes, "idnet_embed_save: saved state of %lld bytes, %lld needed",
                      (long long)saved_bytes, (long long)sv.total_bytes);
    } else {
        n_saved = 0;
    }
    char* const S = static_cast<char*>(saved);
    auto sv_f = [&](int64_t off) { return saving ? reinterpret_cast<float*>(S + off) : nullptr; };
    auto sv_m = [&](int i) { return saving ? reinterpret_cast<unsigned char*>(S + sv.mask[i]) : nullptr; };
    const IdLayout& l = id_layout();
    hipStream_t st = as_stream(stream);
    float* ws = static_cast<float*>(a.ws);
    const float* P = a.packed;
    int rc;
    auto tap = [&](int t, const float* from, int64_t floats) {
        if (a.taps[t]) (void)hipMemcpyAsync(a.taps[t], from, floats * sizeof(float), hipMemcpyDeviceToDevice, st);
    };
    float* net_in = ws + d.net_in;
    IdPrepArgs p;
    p.out = net_in; p.n_per_set = a.n_per_set; p.n = n; p.H = a.height; p.W = a.width;
    for (int s = 0; s < 3; ++s) p.set[s] = s < a.n_sets ? a.images[s] : a.images[0];
    const int64_t in_floats = (int64_t)n * 3 * kIdNet * kIdNet;
    idnet_prep_kernel<<<dim3((unsigned)((in_floats + 255) / 256)), dim3(256), 0, st>>>(p);
    if ((rc = check_launch("idnet_embed(prep)"))) return rc;
    tap(0, net_in, in_floats);
    float* x = ws + d.buf[0];
    float* y = ws + d.buf[1];
    float* t1 = ws + d.buf[2];
    float* res = ws + d.res;
    float* sc = ws + d.sc;
    float* plane = ws + d.plane;
    float* gate = ws + d.gate;
    if ((rc = id_conv(x, net_in, P + l.w_off[0], nullptr, P + l.bn_off[0], P + l.prelu_off[0], nullptr, n, 3, 64, kIdNet, kIdNet, 3, 1, st, sv_m(0),
                      n_saved)))
        return rc;
    tap(1, x, (int64_t)n * 64 * kIdNet * kIdNet);
    int size = kIdNet;
    for (int u = 0; u < kIdUnits; ++u) {
        const IdUnit q = id_unit(u);
        const int osize = id_out_size(size, q.stride), c1 = 1 + 2 * u, c2 = 2 + 2 * u;
        if ((rc = id_conv(t1, x, P + l.w_off[c1], P + l.bn_off[c1], nullptr, P + l.prelu_off[1 + u], nullptr, n, q.cin, q.depth, size, size, 3, 1, st,
                          sv_m(1 + u), n_saved)))
            return rc;
        if ((rc = id_conv(res, t1, P + l.w_off[c2], nullptr, P + l.bn_off[c2], nullptr, plane, n, q.depth, q.depth, size, size, 3, q.stride, st)))
            return rc;
        if (q.shortcut >= 0) {
            const int cs = 49 + q.shortcut;
            if ((rc = id_conv(sc, x, P + l.w_off[cs], nullptr, P + l.bn_off[cs], nullptr, nullptr, n, q.cin, q.depth, size, size, 1, q.stride, st)))
                return rc;
        }
        if (saving)
            idnet_se_kernel<true><<<dim3((unsigned)n), dim3(256), 0, st>>>(gate, plane, P + l.fc1_off[u], P + l.fc2_off[u], q.depth,
                                                                           id_tiles(osize * osize, q.depth), osize * osize, sv_f(sv.gate[u]),
                                                                           sv_f(sv.hid[u]), n_saved);
        else
            idnet_se_kernel<false><<<dim3((unsigned)n), dim3(256), 0, st>>>(gate, plane, P + l.fc1_off[u], P + l.fc2_off[u], q.depth,
                                                                            id_tiles(osize * osize, q.depth), osize * osize, nullptr, nullptr, 0);
        if ((rc = check_launch("idnet_embed(se)"))) return rc;
        const int64_t total = (int64_t)n * q.depth * osize * osize;
        if (saving)
            idnet_merge_kernel<true><<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(y, res, gate, q.shortcut >= 0 ? sc : nullptr, x, osize,
                                                                                                 osize, size, size, q.stride, total, sv_f(sv.res[u]),
                                                                                                 (int64_t)n_saved * q.depth * osize * osize);
        else
            idnet_merge_kernel<false><<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(y, res, gate, q.shortcut >= 0 ? sc : nullptr, x,
                                                                                                   osize, osize, size, size, q.stride, total, nullptr, 0);
        if ((rc = check_launch("idnet_embed(merge)"))) return rc;
        const int t = id_tap_of_unit(u);
        if (t >= 0) tap(t, y, total);
        float* swap = x; x = y; y = swap;
        size = osize;
    }
    float* part = ws + d.part;
    idnet_head_kernel<<<dim3(kIdEmbed / kIdHeadRows, kIdHeadSlices), dim3(256), 0, st>>>(part, x, P + l.head_w_off,
                                                                                         reinterpret_cast<const float2*>(P + l.bn_off[52]), n);
    if ((rc = check_launch("idnet_embed(head)"))) return rc;
    if (saving)
        idnet_head_fold_kernel<true><<<dim3((unsigned)n), dim3(kIdEmbed), 0, st>>>(a.embeddings, a.taps[7], part, P + l.head_b_off,
                                                                                  reinterpret_cast<const float2*>(P + l.bn_off[53]), n, sv_f(sv.v),
                                                                                  sv_f(sv.f), sv_f(sv.norm), n_saved);
    else
        idnet_head_fold_kernel<false><<<dim3((unsigned)n), dim3(kIdEmbed), 0, st>>>(a.embeddings, a.taps[7], part, P + l.head_b_off,
                                                                                    reinterpret_cast<const float2*>(P + l.bn_off[53]), n, nullptr,
                                                                                    nullptr, nullptr, 0);
    return check_launch("idnet_embed(head fold)");
}

extern "C" int e3dge_idnet_embed(const E3dgeIdnetArgs* args, e3dge_stream_t stream) {
    E3DGE_REQUIRE(args, "idnet_embed: null argument struct");
    return id_embed(*args, nullptr, 0, 0, false, stream);
}

extern "C" int e3dge_id_loss(const E3dgeIdLossArgs* args, e3dge_stream_t stream) {
    E3DGE_REQUIRE(args, "id_loss: null argument struct");
    const E3dgeIdLossArgs& a = *args;
    E3DGE_REQUIRE(a.y_hat && a.y && a.x && a.dots, "id_loss: null pointer");
    E3DGE_REQUIRE(a.batch >= 1, "id_loss: batch=%d", a.batch);
    idnet_dot_kernel<<<dim3(1), dim3(192), 0, as_stream(stream)>>>(a.dots, a.loss, a.sim_improvement, a.y_hat, a.y, a.x, a.batch);
    return check_launch("id_loss");
}

static bool id_conv_sizes_ok(int cout, int height, int width, int ksize, int stride) {
    return cout >= kIgBM && cout % kIgBM == 0 && cout <= 65535 * kIgBM && height >= 1 && width >= 1 && height <= 4096 && width <= 4096 &&
           (ksize == 1 || ksize == 3) && (stride == 1 || stride == 2);
}

extern "C" int e3dge_idnet_conv_tiles(int cout, int height, int width, int ksize, int stride) {
    if (!id_conv_sizes_ok(cout, height, width, ksize, stride)) {
        fail(E3DGE_ERR_INVALID_ARG, "idnet_conv_tiles: cout=%d height=%d width=%d ksize=%d stride=%d", cout, height, width, ksize, stride);
        return -1;
    }
    return id_tiles(id_out_size(height, stride) * id_out_size(width, stride), cout);
}

extern "C" int e3dge_idnet_conv(float* out, const float* in, const float* w, float* wfrag, const float* in_ab, const float* epi_ab,
                                const float* slope, float* plane, int n, int cin, int cout, int height, int width, int ksize, int stride,
                                e3dge_stream_t stream) {
    E3DGE_REQUIRE(out && in && w && wfrag, "idnet_conv: null pointer");
    E3DGE_REQUIRE(n >= 1 && n <= 4096 && cin >= 1 && cin <= 4096, "idnet_conv: n=%d cin=%d (1..4096)", n, cin);
    E3DGE_REQUIRE(id_conv_sizes_ok(cout, height, width, ksize, stride),
                  "idnet_conv: cout=%d height=%d width=%d ksize=%d stride=%d (cout a multiple of 64, sizes 1..4096, ksize 1 or 3, stride 1 or 2)",
                  cout, height, width, ksize, stride);
    E3DGE_REQUIRE((int64_t)cin * height * width < ((int64_t)1 << 31), "idnet_conv: image too large");
    hipStream_t st = as_stream(stream);
    ig_pack(wfrag, w, cin, cout, ksize, 1.0f, st);
    int rc;
    if ((rc = check_launch("idnet_conv(pack)"))) return rc;
    return id_conv(out, in, wfrag, in_ab, epi_ab, slope, plane, n, cin, cout, height, width, ksize, stride, st);
}

#include "idnet_bwd.h"
#include "encoder.h"
