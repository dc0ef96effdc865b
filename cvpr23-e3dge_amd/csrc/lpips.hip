// LPIPS (AlexNet) perceptual distance of image pairs: the loss_lpips column of the evaluated image and the `vgg_lambda` term of the
// reference's 2-D reconstruction loss.
//
// Reference: LPIPS.forward (project/losses/lpips/lpips.py:33-39), BaseNet.z_score / forward and AlexNet (networks.py:52-65, 80-89: the
// torchvision `features` stack, taps after ReLU 2, 5, 8, 10, 12 counted from 1, the last max-pool never runs), normalize_activation
// (utils.py:6-9), called from Loss.calc_2d_rec_loss (project/losses/builder.py:143, 168, 176).
//
//   z = (x - mean) / std                                   (zero padding applies to z: the mean is NOT folded into conv1's bias)
//   conv 3->64 k11 s4 p2, relu [tap 1], maxpool 3 s2, conv 64->192 k5 p2, relu [tap 2], maxpool 3 s2,
//   conv 192->384 k3 p1, relu [tap 3], conv 384->256 k3 p1, relu [tap 4], conv 256->256 k3 p1, relu [tap 5]
//   f^ = f / (sqrt(sum_c f^2 + 1e-8) + 1e-10);   d_l[b] = mean_{h,w} sum_c lin_l[c] (x^_c - y^_c)^2;   per_image[b] = sum_l d_l[b]
//
// The backward (the gradient with respect to x and y, eight launches) is lpips_bwd.h.
//
// Kernels (nine launches for one forward, whatever the batch):
//   conv_kernel      the implicit GEMM of conv_igemm.h.  M = output channels, N = the output pixels of all 2B images (x then y)
//                    flattened, K = (ci, r, s); NT = 1, 2, 4 by the size of N, so that the 15^2 maps still spread over the chip.
//                    Gather: zero padding (a staged element outside the image, past N or past K is 0 and is never loaded), conv 1
//                    z-scores while staging.  Epilogue: the sum of the two accumulators, + bias, ReLU (the backward's two epilogues:
//                    lpips_bwd.h).  A pixel's value does not depend on its position in the batch, on the batch size or on which of
//                    the two images it belongs to.
//   pool_kernel      the two 3x3 stride-2 floor-mode max-pools.
//   tap_kernel       all five taps in one launch: 16 pixels x 16 channel groups per workgroup, both images of the pair; channel norms,
//                    then sum_c lin_c (x^_c - y^_c)^2 with the same fp32 operations as the reference (true divisions), folded in a
//                    fixed order to one partial per workgroup.
//   fold_kernel      one workgroup: the partials of every (image, layer) in a fixed order (double accumulation), the spatial mean,
//                    per_layer, per_image and their batch mean.  Bit-reproducible.
// Measured times, the per-kernel split and what bounds each kernel: DESIGN.md 4.11b.
#include "conv_igemm.h"

namespace e3dge {

constexpr int kLpLayers = 5;
__host__ __device__ constexpr int lp_cin(int l) { return l == 0 ? 3 : l == 1 ? 64 : l == 2 ? 192 : l == 3 ? 384 : 256; }
__host__ __device__ constexpr int lp_cout(int l) { return l == 0 ? 64 : l == 1 ? 192 : l == 2 ? 384 : 256; }
__host__ __device__ constexpr int lp_ks(int l) { return l == 0 ? 11 : l == 1 ? 5 : 3; }
constexpr int kLpTapPix = 16, kLpTapGroups = 16;

__host__ __device__ constexpr int lp_k(int l) { return lp_cin(l) * lp_ks(l) * lp_ks(l); }
__host__ __device__ constexpr int lp_kpad(int l) { return ig_kpad(lp_k(l)); }
__host__ __device__ constexpr int64_t lp_w_floats(int l) { return (int64_t)lp_cout(l) * lp_kpad(l); }
__host__ __device__ constexpr int64_t lp_w_off(int l) { int64_t o = 0; for (int q = 0; q < l; ++q) o += lp_w_floats(q); return o; }
__host__ __device__ constexpr int64_t lp_c_off(int l) { int64_t o = 0; for (int q = 0; q < l; ++q) o += lp_cout(q); return o; }   // bias / lin rows
constexpr int64_t kLpBiasOff = lp_w_off(kLpLayers - 1) + lp_w_floats(kLpLayers - 1);
constexpr int64_t kLpChannels = lp_c_off(kLpLayers - 1) + lp_cout(kLpLayers - 1);                                    // 1152
constexpr int64_t kLpLinOff = kLpBiasOff + kLpChannels;
constexpr int64_t kLpPackedFloats = kLpLinOff + kLpChannels;

// The packed image: at lp_w_off(l) conv_igemm.h's forward image of W_l (ig_pack; every C_out is a multiple of 16, so no rows are added),
// then the five biases at kLpBiasOff + lp_c_off(l) and the five lin rows at kLpLinOff + lp_c_off(l), as they are.
static_assert(lp_cout(0) % 16 == 0 && lp_cout(1) % 16 == 0 && lp_cout(2) % 16 == 0 && lp_cout(3) % 16 == 0, "lp_w_floats has no padded rows");

struct LpNorm { float mean[3], std[3]; };

// The epilogue of conv_kernel.  kLpEpiRelu: the forward's, relu(acc + bias).  The other two make the same kernel a stride-1 data-gradient
// convolution on the transposed weight image (lpips_bwd.h): kLpEpiStore writes the sum (the gradient of a pooled map), kLpEpiMask
// writes (acc + out) * [f > 0] in place over the masked tap gradient that out already holds (`bias` is then f, the forward's
// post-ReLU activation of this layer, image `f_first` onwards).
enum { kLpEpiRelu = 0, kLpEpiStore = 1, kLpEpiMask = 2 };

template <int KS_, int STRIDE, int PAD, int NT, bool FIRST, int EPI = kLpEpiRelu>
__global__ void __launch_bounds__(256)
lpips_conv_kernel(float* __restrict__ out, const float* __restrict__ in0, const float* __restrict__ in1, int n_first,
                  const float* __restrict__ wfrag, const float* __restrict__ bias, int Cin, int IH, int IW, int Cout, int OH, int OW,
                  int64_t N, int K, int KS4, LpNorm nrm, int f_first = 0) {
    constexpr int BN = IgTile<NT>::BN, ROWS = IgTile<NT>::ROWS, PER = IgTile<NT>::PER;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mt = blockIdx.y * (kIgBM / 16) + wave;
    const int OHW = OH * OW;
    // the pixel this thread stages
    const int sn = tid % BN, srow = tid / BN;
    const int64_t n_glob = (int64_t)blockIdx.x * BN + sn;
    const bool n_ok = n_glob < N;
    int iy0 = 0, ix0 = 0;
    const float* src = in0;
    if (n_ok) {
        const int img = (int)(n_glob / OHW), pix = (int)(n_glob - (int64_t)img * OHW);
        const int oy = pix / OW, ox = pix - oy * OW;
        iy0 = oy * STRIDE - PAD; ix0 = ox * STRIDE - PAD;
        src = img < n_first ? in0 + (int64_t)img * Cin * IH * IW : in1 + (int64_t)(img - n_first) * Cin * IH * IW;
    }
    auto fetch = [&](int k0, float (&v)[PER]) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = k0 + srow + i * ROWS;
            const auto [ci, r, s] = ig_decode<KS_>(k);
            const int iy = iy0 + r, ix = ix0 + s;
            float x = 0.0f;
            if (n_ok && k < K && iy >= 0 && iy < IH && ix >= 0 && ix < IW) {
                x = src[((int64_t)ci * IH + iy) * IW + ix];
                if (FIRST) {
                    const float m = ci == 0 ? nrm.mean[0] : ci == 1 ? nrm.mean[1] : nrm.mean[2];
                    const float sd = ci == 0 ? nrm.std[0] : ci == 1 ? nrm.std[1] : nrm.std[2];
                    x = __fdiv_rn(__fsub_rn(x, m), sd);                               // networks.py:52-53
                }
            }
            v[i] = x;
        }
    };
    f32x4 acc[NT][2];
    ig_k_loop<NT, 2, false>(acc, wfrag + (int64_t)mt * KS4 * 64 + lane, KS4 / (kIgKC / 4), true, fetch, [](int, bool) {});
    // C/D fragment: lane l, register r holds D[4 (l >> 4) + r][l & 15]
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int64_t n = (int64_t)blockIdx.x * BN + t * 16 + (lane & 15);
        if (n >= N) continue;
        const int img = (int)(n / OHW), pix = (int)(n - (int64_t)img * OHW);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = mt * 16 + 4 * (lane >> 4) + r;
            const int64_t at = ((int64_t)img * Cout + row) * OHW + pix;
            if (EPI == kLpEpiRelu) {
                const float v = __fadd_rn(__fadd_rn(acc[t][0][r], acc[t][1][r]), bias[row]);
                out[at] = fmaxf(v, 0.0f);
            } else if (EPI == kLpEpiStore) {
                out[at] = __fadd_rn(acc[t][0][r], acc[t][1][r]);
            } else {
                const float f = bias[((int64_t)(img + f_first) * Cout + row) * OHW + pix];
                out[at] = f > 0.0f ? __fadd_rn(__fadd_rn(acc[t][0][r], acc[t][1][r]), out[at]) : 0.0f;
            }
        }
    }
}

// 3x3 stride-2 max-pool, floor mode: every window lies inside the map
__global__ void __launch_bounds__(256)
lpips_pool_kernel(float* __restrict__ out, const float* __restrict__ in, int64_t planes, int IH, int IW, int OH, int OW) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= planes * OH * OW) return;
    const int64_t plane = i / (OH * OW);
    const int pix = (int)(i - plane * (OH * OW)), oy = pix / OW, ox = pix - oy * OW;
    const float* p = in + (plane * IH + 2 * oy) * IW + 2 * ox;
    float m = p[0];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) m = fmaxf(m, p[r * IW + s]);
    out[i] = m;
}

struct LpTapArgs {
    const float* feat[kLpLayers];      // (2B, C_l, HW_l): images 0..B-1 are x, B..2B-1 are y
    float* taps[kLpLayers];            // NULL or (2B, C_l, HW_l): the normalised features
    int hw[kLpLayers];
    int blk_off[kLpLayers + 1];        // per image: first workgroup of every layer, [5] = workgroups per image
    const float* lin;                  // packed + kLpLinOff
    float* partial;                    // (B, blk_off[5])
    int batch;
};

__global__ void __launch_bounds__(256) lpips_tap_kernel(LpTapArgs a) {
    __shared__ float red[2][kLpTapGroups][kLpTapPix];
    __shared__ float nrm[2][kLpTapPix];
    const int per_img = a.blk_off[kLpLayers];
    const int b = blockIdx.x / per_img, wb = blockIdx.x - b * per_img;
    int l = 0;
#pragma unroll
    for (int q = 1; q < kLpLayers; ++q) if (wb >= a.blk_off[q]) l = q;
    int C = lp_cout(0), HW = a.hw[0], first = a.blk_off[0]; int64_t coff = 0;
    const float* feat = a.feat[0]; float* taps = a.taps[0];
#pragma unroll
    for (int q = 1; q < kLpLayers; ++q)
        if (l == q) { C = lp_cout(q); coff = lp_c_off(q); HW = a.hw[q]; first = a.blk_off[q]; feat = a.feat[q]; taps = a.taps[q]; }
    const int p = threadIdx.x & (kLpTapPix - 1), g = threadIdx.x >> 4;
    const int pix = (wb - first) * kLpTapPix + p;
    const bool ok = pix < HW;
    const float* __restrict__ fx = feat + (int64_t)b * C * HW + pix;
    const float* __restrict__ fy = feat + (int64_t)(b + a.batch) * C * HW + pix;
    float sx = 0.0f, sy = 0.0f;
    if (ok)
        for (int c = g; c < C; c += kLpTapGroups) {
            const float x = fx[(int64_t)c * HW], y = fy[(int64_t)c * HW];
            sx = fmaf(x, x, sx); sy = fmaf(y, y, sy);
        }
    red[0][g][p] = sx; red[1][g][p] = sy;
    __syncthreads();
    if (threadIdx.x < 2 * kLpTapPix) {
        const int w = threadIdx.x >> 4;
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < kLpTapGroups; ++q) s += red[w][q][p];
        nrm[w][p] = __fadd_rn(__fsqrt_rn(__fadd_rn(s, 1e-8f)), 1e-10f);          // utils.py:8-9
    }
    __syncthreads();
    const float nx = nrm[0][p], ny = nrm[1][p];
    const float* __restrict__ lin = a.lin + coff;
    float* tx = taps ? taps + (int64_t)b * C * HW + pix : nullptr;
    float* ty = taps ? taps + (int64_t)(b + a.batch) * C * HW + pix : nullptr;
    float d = 0.0f;
    if (ok)
        for (int c = g; c < C; c += kLpTapGroups) {
            const float x = __fdiv_rn(fx[(int64_t)c * HW], nx), y = __fdiv_rn(fy[(int64_t)c * HW], ny);
            if (tx) { tx[(int64_t)c * HW] = x; ty[(int64_t)c * HW] = y; }
            const float e = __fsub_rn(x, y);
            d = fmaf(lin[c], __fmul_rn(e, e), d);
        }
    __syncthreads();
    red[0][g][p] = d;
    __syncthreads();
    if (threadIdx.x < kLpTapPix) {                                 // a pixel's 16 channel groups in ascending order, ...
        float t = 0.0f;
#pragma unroll
        for (int q = 0; q < kLpTapGroups; ++q) t += red[0][q][p];
        nrm[0][p] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                        // ... then the 16 pixels in ascending order
        float s = 0.0f;
#pragma unroll
        for (int pp = 0; pp < kLpTapPix; ++pp) s += nrm[0][pp];
        a.partial[blockIdx.x] = s;
    }
}

struct LpFoldArgs {
    const float* partial; float* per_image; float* per_layer; float* mean;
    int hw[kLpLayers]; int blk_off[kLpLayers + 1]; int batch;
};

// one workgroup of five waves, wave l = layer l: lane-strided double sums, then a fixed butterfly
__global__ void __launch_bounds__(64 * kLpLayers) lpips_fold_kernel(LpFoldArgs a) {
    __shared__ double dl[kLpLayers];
    const int l = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int first = a.blk_off[0], last = a.blk_off[1], hw = a.hw[0];
#pragma unroll
    for (int q = 1; q < kLpLayers; ++q) if (l == q) { first = a.blk_off[q]; last = a.blk_off[q + 1]; hw = a.hw[q]; }
    const int per_img = a.blk_off[kLpLayers], n = last - first;
    float total = 0.0f;
    for (int b = 0; b < a.batch; ++b) {
        const float* pr = a.partial + (int64_t)b * per_img + first;
        double s = 0.0;
        for (int i = lane; i < n; i += 64) s += (double)pr[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
        const double d = s / (double)hw;
        if (lane == 0) {
            dl[l] = d;
            if (a.per_layer) a.per_layer[b * kLpLayers + l] = (float)d;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const float v = (float)((((dl[0] + dl[1]) + dl[2]) + dl[3]) + dl[4]);
            a.per_image[b] = v;
            total += v;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && a.mean) a.mean[0] = total / (float)a.batch;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
struct LpDims {
    int h[kLpLayers], w[kLpLayers];            // the five conv outputs (= taps)
    int ph[2], pw[2];                          // the two pooled maps
    int blk_off[kLpLayers + 1];
    int64_t act_off[kLpLayers], pool_off[2], partial_off, total_bytes;
};

static bool lp_dims(int batch, int height, int width, LpDims* d) {
    if (batch < 1 || height < 31 || width < 31) return false;
    d->h[0] = (height + 4 - 11) / 4 + 1; d->w[0] = (width + 4 - 11) / 4 + 1;
    d->ph[0] = (d->h[0] - 3) / 2 + 1; d->pw[0] = (d->w[0] - 3) / 2 + 1;
    d->h[1] = d->ph[0]; d->w[1] = d->pw[0];
    d->ph[1] = (d->h[1] - 3) / 2 + 1; d->pw[1] = (d->w[1] - 3) / 2 + 1;
    for (int l = 2; l < kLpLayers; ++l) { d->h[l] = d->ph[1]; d->w[l] = d->pw[1]; }
    const int64_t n_img = 2 * (int64_t)batch;
    int64_t off = 0;
    auto take = [&](int64_t floats) { const int64_t at = off; off += (floats + 63) / 64 * 64; return at; };
    d->blk_off[0] = 0;
    for (int l = 0; l < kLpLayers; ++l) {
        const int64_t hw = (int64_t)d->h[l] * d->w[l];
        if (n_img * hw * lp_cout(l) >= ((int64_t)1 << 40)) return false;
        d->act_off[l] = take(n_img * lp_cout(l) * hw);
        const int64_t blocks = (hw + kLpTapPix - 1) / kLpTapPix;
        if (d->blk_off[l] + blocks >= ((int64_t)1 << 30)) return false;
        d->blk_off[l + 1] = d->blk_off[l] + (int)blocks;
    }
    for (int q = 0; q < 2; ++q) d->pool_off[q] = take(n_img * lp_cout(q) * d->ph[q] * d->pw[q]);
    if ((int64_t)batch * d->blk_off[kLpLayers] >= ((int64_t)1 << 31)) return false;
    d->partial_off = take((int64_t)batch * d->blk_off[kLpLayers]);
    d->total_bytes = off * (int64_t)sizeof(float);
    return true;
}

template <int KS_, int STRIDE, int PAD, bool FIRST>
static int lp_conv(float* out, const float* in0, const float* in1, int n_first, const float* packed, int l, int IH, int IW, int OH, int OW,
                   int n_img, const LpNorm& nrm, hipStream_t st) {
    const int64_t N = (int64_t)n_img * OH * OW;
    const int Cout = lp_cout(l), gy = Cout / kIgBM;
    const float* wf = packed + lp_w_off(l);
    const float* bias = packed + kLpBiasOff + lp_c_off(l);
    const int K = lp_k(l), KS4 = lp_kpad(l) / 4;
    auto blocks = [&](int bn) { return (N + bn - 1) / bn; };
    E3DGE_REQUIRE(blocks(16) < ((int64_t)1 << 31), "lpips_forward: grid too large");
    ig_dispatch_nt(ig_tile_width(N, 1, gy), [&](auto nt_c) {
        constexpr int NT = decltype(nt_c)::value;
        lpips_conv_kernel<KS_, STRIDE, PAD, NT, FIRST><<<dim3((unsigned)blocks(16 * NT), gy), dim3(256), 0, st>>>(
            out, in0, in1, n_first, wf, bias, lp_cin(l), IH, IW, Cout, OH, OW, N, K, KS4, nrm);
    });
    return check_launch("lpips_forward(conv)");
}

static int lp_pool(float* out, const float* in, int64_t planes, int IH, int IW, int OH, int OW, hipStream_t st) {
    const int64_t n = planes * OH * OW;
    lpips_pool_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(out, in, planes, IH, IW, OH, OW);
    return check_launch("lpips_forward(pool)");
}

#include "lpips_bwd.h"

}  // namespace e3dge

using namespace e3dge;

extern "C" int64_t e3dge_lpips_packed_floats(void) { return kLpPackedFloats; }

extern "C" int e3dge_lpips_pack_weights(float* packed, const float* const* w, const float* const* b, const float* const* lin,
                                        e3dge_stream_t stream) {
    E3DGE_REQUIRE(packed && w && b && lin, "lpips_pack_weights: null pointer");
    for (int l = 0; l < kLpLayers; ++l) E3DGE_REQUIRE(w[l] && b[l] && lin[l], "lpips_pack_weights: null pointer (layer %d)", l);
    hipStream_t st = as_stream(stream);
    for (int l = 0; l < kLpLayers; ++l) {
        ig_pack(packed + lp_w_off(l), w[l], lp_cin(l), lp_cout(l), lp_ks(l), 1.0f, st);
        ig_copy(packed + kLpBiasOff + lp_c_off(l), b[l], lp_cout(l), 1.0f, 0, st);
        ig_copy(packed + kLpLinOff + lp_c_off(l), lin[l], lp_cout(l), 1.0f, 0, st);
    }
    return check_launch("lpips_pack_weights");
}

extern "C" int64_t e3dge_lpips_ws_bytes(int batch, int height, int width) {
    LpDims d;
    if (!lp_dims(batch, height, width, &d)) {
        fail(E3DGE_ERR_INVALID_ARG, "lpips_ws_bytes: batch=%d height=%d width=%d (batch >= 1, height and width >= 31)", batch, height, width);
        return -1;
    }
    return d.total_bytes;
}

extern "C" int e3dge_lpips_forward(const E3dgeLpipsArgs* args, e3dge_stream_t stream) {
    E3DGE_REQUIRE(args, "lpips_forward: null argument struct");
    const E3dgeLpipsArgs& a = *args;
    E3DGE_REQUIRE(a.packed && a.x && a.y && a.per_image && a.ws, "lpips_forward: null pointer");
    E3DGE_REQUIRE(a.batch >= 1, "lpips_forward: batch=%d", a.batch);
    E3DGE_REQUIRE(a.height >= 31 && a.width >= 31, "lpips_forward: height=%d width=%d (the smallest image with an output at every layer is 31 x 31)",
                  a.height, a.width);
    E3DGE_REQUIRE(a.std[0] != 0.0f && a.std[1] != 0.0f && a.std[2] != 0.0f, "lpips_forward: a channel's std is 0");
    LpDims d;
    E3DGE_REQUIRE(lp_dims(a.batch, a.height, a.width, &d), "lpips_forward: sizes too large");
    E3DGE_REQUIRE(a.ws_bytes >= d.total_bytes, "lpips_forward: workspace of %lld bytes, %lld needed", (long long)a.ws_bytes, (long long)d.total_bytes);
    hipStream_t st = as_stream(stream);
    float* ws = static_cast<float*>(a.ws);
    const int B = a.batch, n_img = 2 * B;
    LpNorm nrm;
    for (int c = 0; c < 3; ++c) { nrm.mean[c] = a.mean[c]; nrm.std[c] = a.std[c]; }
    float* act[kLpLayers];
    for (int l = 0; l < kLpLayers; ++l) act[l] = ws + d.act_off[l];
    float* p0 = ws + d.pool_off[0];
    float* p1 = ws + d.pool_off[1];
    int rc;
    if ((rc = lp_conv<11, 4, 2, true>(act[0], a.x, a.y, B, a.packed, 0, a.height, a.width, d.h[0], d.w[0], n_img, nrm, st))) return rc;
    if ((rc = lp_pool(p0, act[0], (int64_t)n_img * lp_cout(0), d.h[0], d.w[0], d.ph[0], d.pw[0], st))) return rc;
    if ((rc = lp_conv<5, 1, 2, false>(act[1], p0, p0, n_img, a.packed, 1, d.ph[0], d.pw[0], d.h[1], d.w[1], n_img, nrm, st))) return rc;
    if ((rc = lp_pool(p1, act[1], (int64_t)n_img * lp_cout(1), d.h[1], d.w[1], d.ph[1], d.pw[1], st))) return rc;
    if ((rc = lp_conv<3, 1, 1, false>(act[2], p1, p1, n_img, a.packed, 2, d.ph[1], d.pw[1], d.h[2], d.w[2], n_img, nrm, st))) return rc;
    if ((rc = lp_conv<3, 1, 1, false>(act[3], act[2], act[2], n_img, a.packed, 3, d.h[2], d.w[2], d.h[3], d.w[3], n_img, nrm, st))) return rc;
    if ((rc = lp_conv<3, 1, 1, false>(act[4], act[3], act[3], n_img, a.packed, 4, d.h[3], d.w[3], d.h[4], d.w[4], n_img, nrm, st))) return rc;
    LpTapArgs t;
    LpFoldArgs f;
    for (int l = 0; l < kLpLayers; ++l) {
        t.feat[l] = act[l]; t.taps[l] = a.taps[l]; t.hw[l] = f.hw[l] = d.h[l] * d.w[l];
    }
    for (int l = 0; l <= kLpLayers; ++l) t.blk_off[l] = f.blk_off[l] = d.blk_off[l];
    t.lin = a.packed + kLpLinOff; t.partial = ws + d.partial_off; t.batch = B;
    lpips_tap_kernel<<<dim3((unsigned)(B * d.blk_off[kLpLayers])), dim3(256), 0, st>>>(t);
    if ((rc = check_launch("lpips_forward(taps)"))) return rc;
    f.partial = t.partial; f.per_image = a.per_image; f.per_layer = a.per_layer; f.mean = a.mean_out; f.batch = B;
    lpips_fold_kernel<<<dim3(1), dim3(64 * kLpLayers), 0, st>>>(f);
    return check_launch("lpips_forward(fold)");
}

extern "C" int64_t e3dge_lpips_packed_t_floats(void) { return kLpPackedTFloats; }

extern "C" int e3dge_lpips_pack_weights_t(float* packed_t, const float* const* w, e3dge_stream_t stream) {
    E3DGE_REQUIRE(packed_t && w, "lpips_pack_weights_t: null pointer");
    for (int l = 0; l < kLpLayers; ++l) E3DGE_REQUIRE(w[l], "lpips_pack_weights_t: null pointer (layer %d)", l);
    hipStream_t st = as_stream(stream);
    for (int l = 1; l < kLpLayers; ++l) ig_pack_t(packed_t + lp_wt_off(l), w[l], lp_cin(l), lp_cout(l), lp_ks(l), 1.0f, st);
    lpips_pack_w1t_kernel<<<dim3((unsigned)((kLpW1tFloats + 255) / 256)), dim3(256), 0, st>>>(packed_t + kLpW1tOff, w[0]);
    return check_launch("lpips_pack_weights_t");
}

extern "C" int64_t e3dge_lpips_bwd_ws_bytes(int batch, int height, int width, int both) {
    LpDims d;
    if (!lp_dims(batch, height, width, &d) || batch >= 32768) {
        fail(E3DGE_ERR_INVALID_ARG, "lpips_bwd_ws_bytes: batch=%d height=%d width=%d (batch >= 1, height and width >= 31)", batch, height, width);
        return -1;
    }
    LpBwdDims bd;
    lp_bwd_dims(d, both ? 2 * batch : batch, &bd);
    return bd.total_bytes;
}

extern "C" int e3dge_lpips_backward(const E3dgeLpipsBwdArgs* args, e3dge_stream_t stream) {
    E3DGE_REQUIRE(args, "lpips_backward: null argument struct");
    return lp_backward(*args, as_stream(stream));
}
