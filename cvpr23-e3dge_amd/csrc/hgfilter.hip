// Hourglass image filter of the local branch, forward: the (B, 256, H/4, W/4) feature maps that the second renderer pass and the
// stage-2 step consume as local_data_batch['feature_maps'].
//
// Reference: HGPIFuNetGANResidualResnetFC.filter (vendor/pifu/lib/model/HGPIFuGANNetResidualInputResnetFC.py:33-76) = residual_conv / depth_conv
// (conv3x3, ResidualBlock, conv1x1 of models/helper_modules/helpers.py:250-370, reflect padding, instance norm), concatenation, and
// HGFilter (vendor/pifu/lib/model/HGFilters.py) with norm='group', hg_down='ave_pool', hourglass_dim=256; ConvBlock is
// vendor/pifu/lib/net_util.py:399-453.
//
//   front net    f0 = conv3x3(x);  f2 = f0 + conv3x3(relu(IN(conv3x3(relu(IN(f0))))));  out[:, slice] = conv1x1(f2)
//   HGFilter     x = relu(GN(conv7x7/2(in))) = tmpx;  normx = pool(ConvBlock(64, 128)(x));  ConvBlock(128, 128), ConvBlock(128, 256);
//                per stack: HourGlass, ConvBlock, relu(GN(conv1x1)), l = conv1x1 -> output;  previous += bl(ll) + al(output)
//   ConvBlock    out = cat(o1, o2, o3) + residual, o_i = conv3x3(relu(GN(o_{i-1}))), residual = x or conv1x1(relu(GN(x)))
//   HourGlass    level(d, x) = ConvBlock(x) + bicubic_x2(ConvBlock(inner(ConvBlock(pool(x))))), inner = level(d - 1) or a ConvBlock
//
// Kernels (no atomics, bit-reproducible; an image's values do not depend on the batch):
//   hgf_conv_kernel    the implicit GEMM of conv_igemm.h, N = the output pixels of ONE image per workgroup column.  Gather: zero padding
//                      or the mirrored index (reflect), and an optional relu(a x + b) with (a, b) per (image, channel) on in-image
//                      elements: the leading norm and ReLU; a zero-padded tap stays 0.  Epilogue: the sum of the two accumulator chains
//                      (each in ascending k whatever the tile width), an optional bias, an optional plain store (`raw`: what the next
//                      norm of the block reads), an optional residual from a channel slice of a second tensor, and the store into a
//                      channel slice of a wider output: ConvBlock's cat(...) + residual without a concatenation copy.  Layers of 32
//                      output channels run with two idle waves (IDLE).
//   hgf_norm_kernel    one workgroup per (image, group): sum and sum of squares in float64, each thread a fixed stride of the group, then
//                      a fixed tree; (a, b) = (gamma rstd, beta - mean gamma rstd) rounded once.  The order of the sums depends on the
//                      group's shape alone.  InstanceNorm2d(affine) is the case groups = channels.
//   hgf_act_kernel     relu(a x + b): tmpx, the one activated tensor the filter returns.
//   hgf_pool_kernel    avg_pool2d(2, 2).      hgf_up_add_kernel    up1 + bicubic x2 (align_corners, A = -0.75, clamped indices).
// Launch count and measured times: DESIGN.md 4.15.  The backward (hgfilter_bwd.h) is included at the end; its saving
// forward is the same launches with every tensor the backward reads again kept in a buffer of its own (HgfSaved below).
#include "conv_igemm.h"

namespace e3dge {

constexpr int kHgfMaxStack = E3DGE_HGF_MAX_STACK, kHgfMaxDepth = 4, kHgfFrontSrc = E3DGE_HGF_FRONT_SRC;
constexpr float kHgfEps = 1e-5f;

// ---- convolution --------------------------------------------------------------------------------------------------------------
struct HgfConvArgs {
    float* out; float* raw; const float* in; const float* wfrag; const float2* in_ab; const float* bias; const float* res;
    int Cin, IH, IW, Cout, OH, OW, K, KS4, tiles;
    int out_C, out_c0, res_C, res_c0;
};

template <int KS_, int STRIDE, int NT, bool REFLECT, bool IDLE>
__global__ void __launch_bounds__(256) hgf_conv_kernel(HgfConvArgs a) {
    constexpr int BN = IgTile<NT>::BN, ROWS = IgTile<NT>::ROWS, PER = IgTile<NT>::PER;
    constexpr int PAD = KS_ / 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mt = blockIdx.y * (kIgBM / 16) + wave;
    const bool live = mt * 16 < a.Cout;
    const int OHW = a.OH * a.OW, IH = a.IH, IW = a.IW, K = a.K;
    const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
    const int sn = tid % BN, srow = tid / BN;
    const int spix = tile * BN + sn;
    const bool n_ok = spix < OHW;
    const int soy = spix / a.OW, sox = spix - soy * a.OW;
    const int iy0 = soy * STRIDE - PAD, ix0 = sox * STRIDE - PAD;
    const float* __restrict__ src = a.in + (int64_t)img * a.Cin * IH * IW;
    const float2* __restrict__ in_ab = a.in_ab ? a.in_ab + (int64_t)img * a.Cin : nullptr;
    auto fetch = [&](int k0, float (&v)[PER]) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = k0 + srow + i * ROWS;
            const auto [ci, r, s] = ig_decode<KS_>(k);
            int iy = iy0 + r, ix = ix0 + s;
            if (REFLECT) {                                           // PAD < IH, IW (checked on the host): one mirror is enough
                iy = iy < 0 ? -iy : iy >= IH ? 2 * IH - 2 - iy : iy;
                ix = ix < 0 ? -ix : ix >= IW ? 2 * IW - 2 - ix : ix;
            }
            float x = 0.0f;
            if (n_ok && k < K && iy >= 0 && iy < IH && ix >= 0 && ix < IW) {
                x = src[((int64_t)ci * IH + iy) * IW + ix];
                if (in_ab) { const float2 ab = in_ab[ci]; x = fmaxf(__fmaf_rn(ab.x, x, ab.y), 0.0f); }   // a zero-padded tap stays 0
            }
            v[i] = x;
        }
    };
    f32x4 acc[NT][2];
    ig_k_loop<NT, 2, IDLE>(acc, a.wfrag + (int64_t)mt * a.KS4 * 64 + lane, a.KS4 / (kIgKC / 4), live, fetch, [](int, bool) {});
    if (IDLE && !live) return;
    // C/D fragment: lane l, register r holds D[4 (l >> 4) + r][l & 15]
    const int row0 = mt * 16 + 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int pix = tile * BN + t * 16 + (lane & 15);
        if (pix >= OHW) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + r;
            float v = __fadd_rn(acc[t][0][r], acc[t][1][r]);
            if (a.bias) v = __fadd_rn(v, a.bias[row]);
            if (a.raw) a.raw[((int64_t)img * a.Cout + row) * OHW + pix] = v;
            if (a.res) v = __fadd_rn(v, a.res[((int64_t)img * a.res_C + a.res_c0 + row) * OHW + pix]);
            a.out[((int64_t)img * a.out_C + a.out_c0 + row) * OHW + pix] = v;
        }
    }
}

// ---- group statistics -----------------------------------------------------------------------------------------------------------
// ab[(img * C + c)] = (a, b) for the C channels [c0, c0 + C) of x (n, C_total, HW); one workgroup per (image, group)
constexpr int kHgfNormThreads = 512, kHgfNormUnroll = 4;
__global__ void __launch_bounds__(kHgfNormThreads) hgf_norm_kernel(float2* __restrict__ ab, const float* __restrict__ x, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, int C_total, int c0, int C, int groups, int HW) {
    __shared__ double s1[kHgfNormThreads], s2[kHgfNormThreads];
    const int tid = threadIdx.x, img = blockIdx.x / groups, g = blockIdx.x - img * groups;
    const int cpg = C / groups;
    const int64_t count = (int64_t)cpg * HW;                          // the group's channels are contiguous
    const float* __restrict__ p = x + ((int64_t)img * C_total + c0 + (int64_t)g * cpg) * HW;
    double a1 = 0.0, a2 = 0.0;
    for (int64_t i0 = tid; i0 < count; i0 += kHgfNormThreads * kHgfNormUnroll) {
        float v[kHgfNormUnroll];
#pragma unroll
        for (int u = 0; u < kHgfNormUnroll; ++u) {                    // the loads of one step are in flight together; 0 adds nothing
            const int64_t i = i0 + (int64_t)u * kHgfNormThreads;
            v[u] = i < count ? p[i] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kHgfNormUnroll; ++u) {
            a1 += (double)v[u];
            a2 = fma((double)v[u], (double)v[u], a2);
        }
    }
    s1[tid] = a1; s2[tid] = a2;
    __syncthreads();
    for (int off = kHgfNormThreads / 2; off > 0; off >>= 1) {
        if (tid < off) { s1[tid] += s1[tid + off]; s2[tid] += s2[tid + off]; }
        __syncthreads();
    }
    const double mean = s1[0] / (double)count;
    double var = s2[0] / (double)count - mean * mean;
    var = var > 0.0 ? var : 0.0;
    const double rstd = 1.0 / sqrt(var + (double)kHgfEps);
    if (tid < cpg) {
        const int c = g * cpg + tid;
        const double sa = (double)gamma[c] * rstd;
        ab[(int64_t)img * C + c] = make_float2((float)sa, (float)((double)beta[c] - mean * sa));
    }
}

// y = relu(a x + b), ab per (image, channel) = per plane
__global__ void __launch_bounds__(256) hgf_act_kernel(float* __restrict__ y, const float* __restrict__ x, const float2* __restrict__ ab, int HW,
                                                      int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const float2 e = ab[i / HW];
    y[i] = fmaxf(__fmaf_rn(e.x, x[i], e.y), 0.0f);
}

// ---- pooling and up-sampling ------------------------------------------------------------------------------------------------------
// out (planes, H / 2, W / 2) = avg_pool2d(in (planes, H, W), 2, 2)
__global__ void __launch_bounds__(256) hgf_pool_kernel(float* __restrict__ out, const float* __restrict__ in, int H, int W, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int OW = W / 2, OH = H / 2;
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
    const int64_t plane = i / ((int64_t)OW * OH);
    const float* __restrict__ p = in + (plane * H + 2 * oy) * W + 2 * ox;
    const float s = __fadd_rn(__fadd_rn(__fadd_rn(p[0], p[1]), p[W]), p[W + 1]);
    out[i] = __fmul_rn(s, 0.25f);
}

__device__ __forceinline__ void hgf_cubic(float t, float (&w)[4]) {
    constexpr float A = -0.75f;
    auto c1 = [](float x) { return __fmaf_rn(__fmul_rn(__fmaf_rn(A + 2.0f, x, -(A + 3.0f)), x), x, 1.0f); };
    auto c2 = [](float x) { return __fmaf_rn(__fmaf_rn(__fmaf_rn(A, x, -5.0f * A), x, 8.0f * A), x, -4.0f * A); };
    w[0] = c2(__fadd_rn(t, 1.0f)); w[1] = c1(t); w[2] = c1(__fsub_rn(1.0f, t)); w[3] = c2(__fsub_rn(2.0f, t));
}

// out (planes, 2 H, 2 W) = up1 + bicubic_x2(low (planes, H, W)), align_corners = True
__global__ void __launch_bounds__(256) hgf_up_add_kernel(float* __restrict__ out, const float* __restrict__ up1, const float* __restrict__ low, int H,
                                                         int W, float scale_y, float scale_x, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int OW = 2 * W, OH = 2 * H;
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
    const int64_t plane = i / ((int64_t)OW * OH);
    const float ry = __fmul_rn(scale_y, (float)oy), rx = __fmul_rn(scale_x, (float)ox);
    int y0 = (int)floorf(ry), x0 = (int)floorf(rx);
    y0 = y0 < H - 1 ? y0 : H - 1; x0 = x0 < W - 1 ? x0 : W - 1;
    const float ty = fminf(fmaxf(__fsub_rn(ry, (float)y0), 0.0f), 1.0f), tx = fminf(fmaxf(__fsub_rn(rx, (float)x0), 0.0f), 1.0f);
    float wy[4], wx[4];
    hgf_cubic(ty, wy);
    hgf_cubic(tx, wx);
    const float* __restrict__ p = low + plane * H * W;
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int yy = y0 - 1 + j;
        yy = yy < 0 ? 0 : yy > H - 1 ? H - 1 : yy;
        float row = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int xx = x0 - 1 + k;
            xx = xx < 0 ? 0 : xx > W - 1 ? W - 1 : xx;
            row = __fmaf_rn(wx[k], p[(int64_t)yy * W + xx], row);
        }
        acc = __fmaf_rn(wy[j], row, acc);
    }
    out[i] = __fadd_rn(up1[i], acc);
}

// ---- host side: single layers -------------------------------------------------------------------------------------------------
static int hgf_pad(int ks) { return ks / 2; }
static int hgf_out_size(int in, int ks, int stride) { return (in + 2 * hgf_pad(ks) - ks) / stride + 1; }
static bool hgf_geometry_ok(int ks, int stride) { return (ks == 7 && stride == 2) || ((ks == 3 || ks == 1) && stride == 1); }
static int64_t hgf_gy(int Cout) { return (Cout + kIgBM - 1) / kIgBM; }
// the tile width comes from the layer alone (two images counted): an image's values do not depend on the batch
static int hgf_tile_width(int OHW, int Cout) { return ig_tile_width(OHW, 2, hgf_gy(Cout)); }

struct HgfConvCall {
    float* out; float* raw; const float* in; const float* wfrag; const float* in_ab; const float* bias; const float* res;
    int n, Cin, Cout, IH, IW, ks, stride, reflect, out_C, out_c0, res_C, res_c0;
};

static int hgf_conv(const HgfConvCall& c, hipStream_t st) {
    HgfConvArgs a;
    a.out = c.out; a.raw = c.raw; a.in = c.in; a.wfrag = c.wfrag; a.in_ab = reinterpret_cast<const float2*>(c.in_ab); a.bias = c.bias; a.res = c.res;
    a.Cin = c.Cin; a.IH = c.IH; a.IW = c.IW; a.Cout = c.Cout;
    a.OH = hgf_out_size(c.IH, c.ks, c.stride); a.OW = hgf_out_size(c.IW, c.ks, c.stride);
    a.K = c.Cin * c.ks * c.ks; a.KS4 = ig_kpad(a.K) / 4;
    a.out_C = c.out_C; a.out_c0 = c.out_c0; a.res_C = c.res_C; a.res_c0 = c.res_c0;
    const int OHW = a.OH * a.OW, nt = hgf_tile_width(OHW, c.Cout), bn = 16 * nt;
    a.tiles = (OHW + bn - 1) / bn;
    const dim3 grid((unsigned)((int64_t)c.n * a.tiles), (unsigned)hgf_gy(c.Cout));
    const bool idle = c.Cout % kIgBM != 0;
    ig_dispatch_nt(nt, [&](auto nt_c) {
        constexpr int NT = decltype(nt_c)::value;
        auto go = [&](auto idle_c) {
            constexpr bool ID = decltype(idle_c)::value;
            if (c.ks == 7) hgf_conv_kernel<7, 2, NT, false, ID><<<grid, dim3(256), 0, st>>>(a);
            else if (c.ks == 3 && c.reflect) hgf_conv_kernel<3, 1, NT, true, ID><<<grid, dim3(256), 0, st>>>(a);
            else if (c.ks == 3) hgf_conv_kernel<3, 1, NT, false, ID><<<grid, dim3(256), 0, st>>>(a);
            else hgf_conv_kernel<1, 1, NT, false, ID><<<grid, dim3(256), 0, st>>>(a);
        };
        if (idle) go(std::true_type{}); else go(std::false_type{});
    });
    return check_launch("hgf(conv)");
}

static int hgf_norm(float* ab, const float* x, const float* gamma, const float* beta, int n, int C_total, int c0, int C, int groups, int HW,
                    hipStream_t st) {
    hgf_norm_kernel<<<dim3((unsigned)(n * groups)), dim3(kHgfNormThreads), 0, st>>>(reinterpret_cast<float2*>(ab), x, gamma, beta, C_total, c0, C, groups, HW);
    return check_launch("hgf(norm)");
}

static int hgf_pool(float* out, const float* in, int64_t planes, int H, int W, hipStream_t st) {
    const int64_t total = planes * (H / 2) * (W / 2);
    hgf_pool_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(out, in, H, W, total);
    return check_launch("hgf(pool)");
}

static int hgf_up_add(float* out, const float* up1, const float* low, int64_t planes, int H, int W, hipStream_t st) {
    const int64_t total = planes * 4 * H * W;
    const float sy = H > 1 ? (float)(H - 1) / (float)(2 * H - 1) : 0.0f, sx = W > 1 ? (float)(W - 1) / (float)(2 * W - 1) : 0.0f;
    hgf_up_add_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(out, up1, low, H, W, sy, sx, total);
    return check_launch("hgf(up_add)");
}

// ---- host side: the packed image ------------------------------------------------------------------------------------------------
// One entry per source tensor, in the order of the source array: a convolution weight (packed as an A-fragment image) or a vector
// (bias, norm weight, norm bias: copied).
struct HgfEntry { int64_t off; int cin, cout, ks; int64_t len; };            // ks == 0: a vector of len floats
struct HgfBlock { int cin, cout, bn[4], w[4]; bool down; };                  // entry indices: bn[i] = gamma (beta = bn[i] + 1)
struct HgfStack { int first_block, top, last_w, bn_end, l_w, bl_w, al_w; };  // *_w: weight entry (bias = + 1)
struct HgfFront { int w0, n1, w1, n2, w2, w3; };

// the most a configuration can hold (8 stacks at depth 4): 3 + S (3 D + 2) blocks; the stem's 4 entries, conv2 to conv4's 12 + 9 + 12, per
// stack 9 per block and 6, 4 more for all but the last, 16 of the front nets
constexpr int kHgfMaxBlocks = 3 + kHgfMaxStack * (3 * kHgfMaxDepth + 2);
constexpr int kHgfMaxEntries = 4 + 33 + kHgfMaxStack * ((3 * kHgfMaxDepth + 2) * 9 + 6) + (kHgfMaxStack - 1) * 4 + kHgfFrontSrc;

struct HgfLayout {                                                           // fixed size: nothing is allocated, on the host either
    HgfEntry e[kHgfMaxEntries];
    HgfBlock blocks[kHgfMaxBlocks];
    int n_entries, n_blocks;
    HgfStack stack[kHgfMaxStack];
    HgfFront front[2];
    int stem_w, stem_bn, conv2, conv3, conv4, n_filter_src, n_src;
    int64_t total;
};

// S and D within hgf_config_ok, so the counts stay within the arrays
static void hgf_layout(int S, int D, HgfLayout* out) {
    HgfLayout& l = *out;
    l.n_entries = l.n_blocks = 0;
    int64_t off = 0;
    auto take = [&](int64_t floats) { const int64_t at = off; off += (floats + 63) / 64 * 64; return at; };
    auto conv = [&](int ci, int co, int ks) { l.e[l.n_entries] = {take((int64_t)ig_mpad(co) * ig_kpad(ci * ks * ks)), ci, co, ks, 0}; return l.n_entries++; };
    auto vec = [&](int len) { l.e[l.n_entries] = {take(len), 0, 0, 0, len}; return l.n_entries++; };
    auto norm = [&](int c) { const int g = vec(c); vec(c); return g; };
    auto block = [&](int ci, int co) {
        HgfBlock b{};
        b.cin = ci; b.cout = co; b.down = ci != co;
        b.bn[0] = norm(ci); b.w[0] = conv(ci, co / 2, 3);
        b.bn[1] = norm(co / 2); b.w[1] = conv(co / 2, co / 4, 3);
        b.bn[2] = norm(co / 4); b.w[2] = conv(co / 4, co / 4, 3);
        if (b.down) { b.bn[3] = norm(ci); b.w[3] = conv(ci, co, 1); }
        l.blocks[l.n_blocks] = b;
        return l.n_blocks++;
    };
    l.stem_w = conv(64, 64, 7); vec(64);
    l.stem_bn = norm(64);
    l.conv2 = block(64, 128); l.conv3 = block(128, 128); l.conv4 = block(128, 256);
    for (int s = 0; s < S; ++s) {
        HgfStack& k = l.stack[s];
        k.first_block = l.n_blocks;
        auto level = [&](auto&& self, int d) -> void {
            block(256, 256); block(256, 256);                        // b1_d, b2_d
            if (d > 1) self(self, d - 1); else block(256, 256);      // b2_plus_1
            block(256, 256);                                         // b3_d
        };
        level(level, D);
        k.top = block(256, 256);
        k.last_w = conv(256, 256, 1); vec(256);
        k.bn_end = norm(256);
        k.l_w = conv(256, 256, 1); vec(256);
        k.bl_w = k.al_w = -1;
        if (s + 1 < S) { k.bl_w = conv(256, 256, 1); vec(256); k.al_w = conv(256, 256, 1); vec(256); }
    }
    l.n_filter_src = l.n_entries;
    for (int f = 0; f < 2; ++f) {                                     // residual_conv (3 channels in), depth_conv (1 channel in)
        HgfFront& q = l.front[f];
        q.w0 = conv(f == 0 ? 3 : 1, 32, 3);
        q.n1 = norm(32); q.w1 = conv(32, 32, 3);
        q.n2 = norm(32); q.w2 = conv(32, 32, 3);
        q.w3 = conv(32, 32, 1);
    }
    l.n_src = l.n_entries;
    l.total = off;
}

static bool hgf_config_ok(int S, int D) { return S >= 1 && S <= kHgfMaxStack && D >= 1 && D <= kHgfMaxDepth; }
static bool hgf_sizes_ok(int n, int H, int W, int D) {
    const int m = 4 << D;
    return n >= 1 && n <= 4096 && H >= m && W >= m && H <= 4096 && W <= 4096 && H % m == 0 && W % m == 0;
}

// ---- host side: workspaces ------------------------------------------------------------------------------------------------------
struct HgfWs {
    int64_t ab[4], stem, c2, c3, prev[2], t1, t2, hg, top, last;
    int64_t up1[kHgfMaxDepth + 1], pooled[kHgfMaxDepth + 1], low1[kHgfMaxDepth + 1], low2[kHgfMaxDepth + 1], low3[kHgfMaxDepth + 1];
    int64_t f[3], fab, filter_floats, front_floats;
};

static HgfWs hgf_ws(int64_t n, int64_t H, int64_t W, int D) {
    HgfWs d{};
    int64_t off = 0;
    auto take = [&](int64_t floats) { const int64_t at = off; off += (floats + 63) / 64 * 64; return at; };
    const int64_t p2 = (H / 2) * (W / 2), p4 = (H / 4) * (W / 4);
    for (int i = 0; i < 4; ++i) d.ab[i] = take(n * 256 * 2);
    d.stem = take(n * 64 * p2);
    d.c2 = take(n * 128 * p2);
    d.c3 = take(n * 128 * p4);
    d.prev[0] = take(n * 256 * p4); d.prev[1] = take(n * 256 * p4);
    d.t1 = take(n * 64 * p2); d.t2 = take(n * 32 * p2);               // the widest ConvBlock halves: conv2's, = 256 and 128 channels at p4
    d.hg = take(n * 256 * p4); d.top = take(n * 256 * p4); d.last = take(n * 256 * p4);
    int64_t p = p4;
    for (int lv = D; lv >= 1; --lv, p /= 4) {
        d.up1[lv] = take(n * 256 * p);
        d.pooled[lv] = take(n * 256 * (p / 4)); d.low1[lv] = take(n * 256 * (p / 4));
        d.low2[lv] = take(n * 256 * (p / 4)); d.low3[lv] = take(n * 256 * (p / 4));
    }
    d.filter_floats = off;
    off = 0;
    d.fab = take(n * 32 * 2);
    for (int i = 0; i < 3; ++i) d.f[i] = take(n * 32 * H * W);
    d.front_floats = off;
    return d;
}

// ---- host side: the saved state of the saving forward -----------------------------------------------------------------------------
// What the backward reads again, each in a buffer of its own: every convolution's pre-norm input and every norm's (a, b).  The plain
// forward reuses t1, t2, ab[], hg, top, last and the level buffers across blocks and stacks; the saving forward takes them from here.
struct HgfBlockBuf { int64_t t1, t2, ab[4]; };
struct HgfSaved {
    HgfBlockBuf blk[kHgfMaxBlocks];
    HgfWs stack[kHgfMaxStack];                                        // up1 .. low3 of every level, hg, top, last; ab[0]: bn_end's
    int64_t stem, ab_stem, c2, c3, prev[kHgfMaxStack];
    int64_t f0[2], f1[2], f2[2], fab[2][2];                           // the front nets: the three later convolutions' inputs and the norms' (a, b)
    int64_t filter_floats, floats;
};

static void hgf_saved(int64_t n, int64_t H, int64_t W, int S, int D, const HgfLayout& l, HgfSaved* out) {
    HgfSaved& v = *out;
    int64_t off = 0;
    auto take = [&](int64_t floats) { const int64_t at = off; off += (floats + 63) / 64 * 64; return at; };
    const int64_t p2 = (H / 2) * (W / 2), p4 = (H / 4) * (W / 4);
    auto block = [&](int bi, int64_t HW) {
        const HgfBlock& b = l.blocks[bi];
        HgfBlockBuf& k = v.blk[bi];
        k.t1 = take(n * (b.cout / 2) * HW); k.t2 = take(n * (b.cout / 4) * HW);
        k.ab[0] = take(n * b.cin * 2); k.ab[1] = take(n * (b.cout / 2) * 2); k.ab[2] = take(n * (b.cout / 4) * 2); k.ab[3] = take(n * b.cin * 2);
    };
    v.stem = take(n * 64 * p2); v.ab_stem = take(n * 64 * 2);
    v.c2 = take(n * 128 * p2); v.c3 = take(n * 128 * p4);
    block(l.conv2, p2); block(l.conv3, p4); block(l.conv4, p4);
    for (int s = 0; s < S; ++s) {
        v.prev[s] = take(n * 256 * p4);
        HgfWs& w = v.stack[s];
        w = HgfWs{};
        int bi = l.stack[s].first_block;
        int64_t p = p4;
        for (int lv = D; lv >= 1; --lv, p /= 4) {                     // the layout's order: b1_d, b2_d, the inner level, b3_d
            w.up1[lv] = take(n * 256 * p);
            w.pooled[lv] = take(n * 256 * (p / 4)); w.low1[lv] = take(n * 256 * (p / 4));
            w.low2[lv] = take(n * 256 * (p / 4)); w.low3[lv] = take(n * 256 * (p / 4));
            block(bi++, p); block(bi++, p / 4);
        }
        p *= 4;
        block(bi++, p / 4);                                           // b2_plus_1
        for (int lv = 1; lv <= D; ++lv, p *= 4) block(bi++, p / 4);   // b3_1 .. b3_D
        block(l.stack[s].top, p4);
        w.hg = take(n * 256 * p4); w.top = take(n * 256 * p4); w.last = take(n * 256 * p4);
        w.ab[0] = take(n * 256 * 2);
    }
    v.filter_floats = off;
    for (int f = 0; f < 2; ++f) {
        v.f0[f] = take(n * 32 * H * W); v.f1[f] = take(n * 32 * H * W); v.f2[f] = take(n * 32 * H * W);
        v.fab[f][0] = take(n * 32 * 2); v.fab[f][1] = take(n * 32 * 2);
    }
    v.floats = off;
}

struct HgfRun {
    const float* P; const HgfLayout* lay; const HgfWs* w; float* ws; hipStream_t st; int n;
    const HgfBlockBuf* bb; float* sv;                                 // the saving forward: per-block buffers in sv; null otherwise
    const float* at(int entry) const { return P + lay->e[entry].off; }
};

// out (n, cout, H, W) = ConvBlock(x (n, cin, H, W)); out must not be x
static int hgf_block(const HgfRun& r, const HgfBlock& b, const float* x, float* out, int H, int W) {
    int rc;
    const int HW = H * W, co = b.cout;
    const HgfBlockBuf* k = r.bb ? r.bb + (&b - r.lay->blocks) : nullptr;
    float* ab[4];
    for (int i = 0; i < 4; ++i) ab[i] = k ? r.sv + k->ab[i] : r.ws + r.w->ab[i];
    float* t1 = k ? r.sv + k->t1 : r.ws + r.w->t1;
    float* t2 = k ? r.sv + k->t2 : r.ws + r.w->t2;
    const float* res = x;
    if (b.down) {                                                     // the residual goes into `out` first; the three slices add to it in place
        if ((rc = hgf_norm(ab[3], x, r.at(b.bn[3]), r.at(b.bn[3] + 1), r.n, b.cin, 0, b.cin, 32, HW, r.st))) return rc;
        if ((rc = hgf_conv({out, nullptr, x, r.at(b.w[3]), ab[3], nullptr, nullptr, r.n, b.cin, co, H, W, 1, 1, 0, co, 0, 0, 0}, r.st))) return rc;
        res = out;
    }
    if ((rc = hgf_norm(ab[0], x, r.at(b.bn[0]), r.at(b.bn[0] + 1), r.n, b.cin, 0, b.cin, 32, HW, r.st))) return rc;
    if ((rc = hgf_conv({out, t1, x, r.at(b.w[0]), ab[0], nullptr, res, r.n, b.cin, co / 2, H, W, 3, 1, 0, co, 0, co, 0}, r.st))) return rc;
    if ((rc = hgf_norm(ab[1], t1, r.at(b.bn[1]), r.at(b.bn[1] + 1), r.n, co / 2, 0, co / 2, 32, HW, r.st))) return rc;
    if ((rc = hgf_conv({out, t2, t1, r.at(b.w[1]), ab[1], nullptr, res, r.n, co / 2, co / 4, H, W, 3, 1, 0, co, co / 2, co, co / 2}, r.st))) return rc;
    if ((rc = hgf_norm(ab[2], t2, r.at(b.bn[2]), r.at(b.bn[2] + 1), r.n, co / 4, 0, co / 4, 32, HW, r.st))) return rc;
    return hgf_conv({out, nullptr, t2, r.at(b.w[2]), ab[2], nullptr, res, r.n, co / 4, co / 4, H, W, 3, 1, 0, co, 3 * co / 4, co, 3 * co / 4}, r.st);
}

// out = HourGlass level d of inp, both (n, 256, H, W); bi: the next block of the layout, advanced in the layout's order
static int hgf_level(const HgfRun& r, int d, int& bi, const float* inp, float* out, int H, int W) {
    int rc;
    const HgfWs& w = *r.w;
    float* up1 = r.ws + w.up1[d];
    float* pooled = r.ws + w.pooled[d];
    float* low1 = r.ws + w.low1[d];
    float* low2 = r.ws + w.low2[d];
    float* low3 = r.ws + w.low3[d];
    if ((rc = hgf_block(r, r.lay->blocks[bi++], inp, up1, H, W))) return rc;                       // b1_d
    if ((rc = hgf_pool(pooled, inp, (int64_t)r.n * 256, H, W, r.st))) return rc;
    if ((rc = hgf_block(r, r.lay->blocks[bi++], pooled, low1, H / 2, W / 2))) return rc;           // b2_d
    if (d > 1) rc = hgf_level(r, d - 1, bi, low1, low2, H / 2, W / 2);
    else rc = hgf_block(r, r.lay->blocks[bi++], low1, low2, H / 2, W / 2);                         // b2_plus_1
    if (rc) return rc;
    if ((rc = hgf_block(r, r.lay->blocks[bi++], low2, low3, H / 2, W / 2))) return rc;             // b3_d
    return hgf_up_add(out, up1, low3, (int64_t)r.n * 256, H / 2, W / 2, r.st);
}

}  // namespace e3dge

using namespace e3dge;

extern "C" int64_t e3dge_hgf_packed_floats(int num_stack, int num_hourglass) {
    if (!hgf_config_ok(num_stack, num_hourglass)) {
        fail(E3DGE_ERR_INVALID_ARG, "hgf_packed_floats: num_stack=%d (1..%d) num_hourglass=%d (1..%d)", num_stack, kHgfMaxStack, num_hourglass, kHgfMaxDepth);
        return -1;
    }
    HgfLayout l;
    hgf_layout(num_stack, num_hourglass, &l);
    return l.total;
}

extern "C" int e3dge_hgf_pack_weights(float* packed, const float* const* filter_src, int n_filter_src, const float* const* front_src,
                                      int num_stack, int num_hourglass, e3dge_stream_t stream) {
    E3DGE_REQUIRE(packed && filter_src, "hgf_pack_weights: null pointer");
    E3DGE_REQUIRE(hgf_config_ok(num_stack, num_hourglass), "hgf_pack_weights: num_stack=%d (1..%d) num_hourglass=%d (1..%d)", num_stack, kHgfMaxStack,
                  num_hourglass, kHgfMaxDepth);
    HgfLayout l;
    hgf_layout(num_stack, num_hourglass, &l);
    E3DGE_REQUIRE(n_filter_src == l.n_filter_src, "hgf_pack_weights: n_filter_src=%d, %d expected", n_filter_src, l.n_filter_src);
    for (int i = 0; i < l.n_filter_src; ++i) E3DGE_REQUIRE(filter_src[i], "hgf_pack_weights: null pointer (filter source %d)", i);
    if (front_src)
        for (int i = 0; i < kHgfFrontSrc; ++i) E3DGE_REQUIRE(front_src[i], "hgf_pack_weights: null pointer (front source %d)", i);
    hipStream_t st = as_stream(stream);
    const int n = front_src ? l.n_src : l.n_filter_src;
    for (int i = 0; i < n; ++i) {
        const HgfEntry& e = l.e[i];
        const float* from = i < l.n_filter_src ? filter_src[i] : front_src[i - l.n_filter_src];
        if (e.ks) ig_pack(packed + e.off, from, e.cin, e.cout, e.ks, 1.0f, st);
        else ig_copy(packed + e.off, from, e.len, 1.0f, 0, st);
    }
    return check_launch("hgf_pack_weights");
}

extern "C" int64_t e3dge_hgf_ws_bytes(int n, int height, int width, int num_stack, int num_hourglass) {
    if (!hgf_config_ok(num_stack, num_hourglass) || !hgf_sizes_ok(n, height, width, num_hourglass)) {
        fail(E3DGE_ERR_INVALID_ARG, "hgf_ws_bytes: n=%d height=%d width=%d num_stack=%d num_hourglass=%d (sizes multiples of 4 * 2^num_hourglass)", n,
             height, width, num_stack, num_hourglass);
        return -1;
    }
    const HgfWs d = hgf_ws(n, height, width, num_hourglass);
    return (d.filter_floats > d.front_floats ? d.filter_floats : d.front_floats) * (int64_t)sizeof(float);
}

// saved == null: the plain forward.  Otherwise the same launches with the buffers of HgfSaved in place of the reused ones.
static int hgf_forward_impl(const E3dgeHgfArgs* args, float* saved, int64_t saved_bytes, e3dge_stream_t stream) {
    E3DGE_REQUIRE(args, "hgf_forward: null argument struct");
    const E3dgeHgfArgs& a = *args;
    const int S = a.num_stack, D = a.num_hourglass, n = a.n, H = a.height, W = a.width;
    E3DGE_REQUIRE(hgf_config_ok(S, D), "hgf_forward: num_stack=%d (1..%d) num_hourglass=%d (1..%d)", S, kHgfMaxStack, D, kHgfMaxDepth);
    E3DGE_REQUIRE(hgf_sizes_ok(n, H, W, D), "hgf_forward: n=%d height=%d width=%d (n 1..4096, sizes multiples of %d up to 4096)", n, H, W, 4 << D);
    E3DGE_REQUIRE(a.packed && a.input && a.tmpx && a.normx && a.ws, "hgf_forward: null pointer");
    for (int s = 0; s < S; ++s) E3DGE_REQUIRE(a.outputs[s], "hgf_forward: null pointer (output %d)", s);
    const HgfWs w = hgf_ws(n, H, W, D);
    E3DGE_REQUIRE(a.ws_bytes >= w.filter_floats * (int64_t)sizeof(float), "hgf_forward: workspace of %lld bytes, %lld needed", (long long)a.ws_bytes,
                  (long long)(w.filter_floats * (int64_t)sizeof(float)));
    HgfLayout l;
    hgf_layout(S, D, &l);
    HgfSaved sv;
    if (saved) {
        hgf_saved(n, H, W, S, D, l, &sv);
        E3DGE_REQUIRE(saved_bytes >= sv.floats * (int64_t)sizeof(float), "hgf_forward: saved state of %lld bytes, %lld needed", (long long)saved_bytes,
                      (long long)(sv.floats * (int64_t)sizeof(float)));
    }
    hipStream_t st = as_stream(stream);
    float* ws = static_cast<float*>(a.ws);
    const HgfRun r{a.packed, &l, &w, ws, st, n, saved ? sv.blk : nullptr, saved};
    const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4;
    int rc;
    float* stem = saved ? saved + sv.stem : ws + w.stem;
    float* ab0 = saved ? saved + sv.ab_stem : ws + w.ab[0];
    if ((rc = hgf_conv({stem, nullptr, a.input, r.at(l.stem_w), nullptr, r.at(l.stem_w + 1), nullptr, n, 64, 64, H, W, 7, 2, 0, 64, 0, 0, 0}, st))) return rc;
    if ((rc = hgf_norm(ab0, stem, r.at(l.stem_bn), r.at(l.stem_bn + 1), n, 64, 0, 64, 32, H2 * W2, st))) return rc;
    const int64_t stem_total = (int64_t)n * 64 * H2 * W2;
    hgf_act_kernel<<<dim3((unsigned)((stem_total + 255) / 256)), dim3(256), 0, st>>>(a.tmpx, stem, reinterpret_cast<const float2*>(ab0), H2 * W2, stem_total);
    if ((rc = check_launch("hgf_forward(act)"))) return rc;
    float* c2 = saved ? saved + sv.c2 : ws + w.c2;
    float* c3 = saved ? saved + sv.c3 : ws + w.c3;
    float* prev = saved ? saved + sv.prev[0] : ws + w.prev[0];
    float* next = ws + w.prev[1];
    if ((rc = hgf_block(r, l.blocks[l.conv2], a.tmpx, c2, H2, W2))) return rc;
    if ((rc = hgf_pool(a.normx, c2, (int64_t)n * 128, H2, W2, st))) return rc;
    if ((rc = hgf_block(r, l.blocks[l.conv3], a.normx, c3, H4, W4))) return rc;
    if ((rc = hgf_block(r, l.blocks[l.conv4], c3, prev, H4, W4))) return rc;
    float* hg = ws + w.hg;
    float* top = ws + w.top;
    float* last = ws + w.last;
    HgfRun rs = r;                                                    // the stack's level buffers
    for (int s = 0; s < S; ++s) {
        const HgfStack& k = l.stack[s];
        int bi = k.first_block;
        if (saved) {
            rs.w = &sv.stack[s]; rs.ws = saved;
            hg = saved + rs.w->hg; top = saved + rs.w->top; last = saved + rs.w->last; ab0 = saved + rs.w->ab[0];
            if (s + 1 < S) next = saved + sv.prev[s + 1];
        }
        if ((rc = hgf_level(rs, D, bi, prev, hg, H4, W4))) return rc;
        if ((rc = hgf_block(r, l.blocks[k.top], hg, top, H4, W4))) return rc;
        if ((rc = hgf_conv({last, nullptr, top, r.at(k.last_w), nullptr, r.at(k.last_w + 1), nullptr, n, 256, 256, H4, W4, 1, 1, 0, 256, 0, 0, 0}, st))) return rc;
        if ((rc = hgf_norm(ab0, last, r.at(k.bn_end), r.at(k.bn_end + 1), n, 256, 0, 256, 32, H4 * W4, st))) return rc;
        if ((rc = hgf_conv({a.outputs[s], nullptr, last, r.at(k.l_w), ab0, r.at(k.l_w + 1), nullptr, n, 256, 256, H4, W4, 1, 1, 0, 256, 0, 0, 0}, st))) return rc;
        if (s + 1 < S) {                                              // previous = (previous + bl(ll)) + al(output)
            if ((rc = hgf_conv({next, nullptr, last, r.at(k.bl_w), ab0, r.at(k.bl_w + 1), prev, n, 256, 256, H4, W4, 1, 1, 0, 256, 0, 256, 0}, st))) return rc;
            if ((rc = hgf_conv({next, nullptr, a.outputs[s], r.at(k.al_w), nullptr, r.at(k.al_w + 1), next, n, 256, 256, H4, W4, 1, 1, 0, 256, 0, 256, 0}, st)))
                return rc;
            float* swap = prev; prev = next; next = swap;
        }
    }
    return E3DGE_OK;
}

extern "C" int e3dge_hgf_forward(const E3dgeHgfArgs* args, e3dge_stream_t stream) { return hgf_forward_impl(args, nullptr, 0, stream); }

static int hgf_front_impl(const float* packed, const float* image, const float* depth, float* out, int n, int height, int width, int num_stack,
                          int num_hourglass, void* ws, int64_t ws_bytes, float* saved, int64_t saved_bytes, e3dge_stream_t stream);

extern "C" int e3dge_hgf_front(const float* packed, const float* image, const float* depth, float* out, int n, int height, int width,
                               int num_stack, int num_hourglass, void* ws, int64_t ws_bytes, e3dge_stream_t stream) {
    return hgf_front_impl(packed, image, depth, out, n, height, width, num_stack, num_hourglass, ws, ws_bytes, nullptr, 0, stream);
}

static int hgf_front_impl(const float* packed, const float* image, const float* depth, float* out, int n, int height, int width,
                          int num_stack, int num_hourglass, void* ws, int64_t ws_bytes, float* saved, int64_t saved_bytes, e3dge_stream_t stream) {
    E3DGE_REQUIRE(packed && image && depth && out && ws, "hgf_front: null pointer");
    E3DGE_REQUIRE(hgf_config_ok(num_stack, num_hourglass), "hgf_front: num_stack=%d (1..%d) num_hourglass=%d (1..%d)", num_stack, kHgfMaxStack,
                  num_hourglass, kHgfMaxDepth);
    E3DGE_REQUIRE(hgf_sizes_ok(n, height, width, num_hourglass), "hgf_front: n=%d height=%d width=%d (n 1..4096, sizes multiples of %d up to 4096)", n,
                  height, width, 4 << num_hourglass);
    const HgfWs w = hgf_ws(n, height, width, num_hourglass);
    E3DGE_REQUIRE(ws_bytes >= w.front_floats * (int64_t)sizeof(float), "hgf_front: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
                  (long long)(w.front_floats * (int64_t)sizeof(float)));
    HgfLayout l;
    hgf_layout(num_stack, num_hourglass, &l);
    HgfSaved sv;
    if (saved) {
        hgf_saved(n, height, width, num_stack, num_hourglass, l, &sv);
        E3DGE_REQUIRE(saved_bytes >= sv.floats * (int64_t)sizeof(float), "hgf_front: saved state of %lld bytes, %lld needed", (long long)saved_bytes,
                      (long long)(sv.floats * (int64_t)sizeof(float)));
    }
    hipStream_t st = as_stream(stream);
    float* base = static_cast<float*>(ws);
    float* ab = base + w.fab;
    float* ab2 = ab;
    float* f0 = base + w.f[0];
    float* f1 = base + w.f[1];
    float* f2 = base + w.f[2];
    auto at = [&](int entry) { return packed + l.e[entry].off; };
    const int HW = height * width;
    int rc;
    for (int f = 0; f < 2; ++f) {
        const HgfFront& q = l.front[f];
        const float* x = f == 0 ? image : depth;
        const int cin = f == 0 ? 3 : 1;
        if (saved) { f0 = saved + sv.f0[f]; f1 = saved + sv.f1[f]; f2 = saved + sv.f2[f]; ab = saved + sv.fab[f][0]; ab2 = saved + sv.fab[f][1]; }
        if ((rc = hgf_conv({f0, nullptr, x, at(q.w0), nullptr, nullptr, nullptr, n, cin, 32, height, width, 3, 1, 1, 32, 0, 0, 0}, st))) return rc;
        if ((rc = hgf_norm(ab, f0, at(q.n1), at(q.n1 + 1), n, 32, 0, 32, 32, HW, st))) return rc;
        if ((rc = hgf_conv({f1, nullptr, f0, at(q.w1), ab, nullptr, nullptr, n, 32, 32, height, width, 3, 1, 1, 32, 0, 0, 0}, st))) return rc;
        if ((rc = hgf_norm(ab2, f1, at(q.n2), at(q.n2 + 1), n, 32, 0, 32, 32, HW, st))) return rc;
        if ((rc = hgf_conv({f2, nullptr, f1, at(q.w2), ab2, nullptr, f0, n, 32, 32, height, width, 3, 1, 1, 32, 0, 32, 0}, st))) return rc;
        if ((rc = hgf_conv({out, nullptr, f2, at(q.w3), nullptr, nullptr, nullptr, n, 32, 32, height, width, 1, 1, 0, 64, 32 * f, 0, 0}, st))) return rc;
    }
    return E3DGE_OK;
}

// ---- debug entries ----------------------------------------------------------------------------------------------------------------
extern "C" int e3dge_hgf_conv(float* out, float* raw, const float* in, const float* w, float* wfrag, const float* in_ab, const float* bias,
                              const float* res, int n, int cin, int cout, int height, int width, int ksize, int stride, int reflect,
                              int out_channels, int out_c0, int res_channels, int res_c0, e3dge_stream_t stream) {
    E3DGE_REQUIRE(out && in && w && wfrag, "hgf_conv: null pointer");
    E3DGE_REQUIRE(n >= 1 && n <= 4096 && cin >= 1 && cin <= 4096, "hgf_conv: n=%d cin=%d (1..4096)", n, cin);
    E3DGE_REQUIRE(cout >= 16 && cout % 16 == 0 && cout <= 4096, "hgf_conv: cout=%d (a multiple of 16 up to 4096)", cout);
    E3DGE_REQUIRE(hgf_geometry_ok(ksize, stride), "hgf_conv: ksize=%d stride=%d (7 with 2, 3 with 1, 1 with 1)", ksize, stride);
    E3DGE_REQUIRE(height >= 1 && width >= 1 && height <= 4096 && width <= 4096, "hgf_conv: height=%d width=%d (1..4096)", height, width);
    E3DGE_REQUIRE(!reflect || (ksize == 3 && height >= 2 && width >= 2), "hgf_conv: reflect padding needs ksize 3 and sizes >= 2");
    E3DGE_REQUIRE((int64_t)cin * height * width < ((int64_t)1 << 31), "hgf_conv: image too large");
    E3DGE_REQUIRE(out_c0 >= 0 && out_channels >= 1 && out_c0 + cout <= out_channels, "hgf_conv: output slice [%d, %d) of %d channels", out_c0, out_c0 + cout,
                  out_channels);
    E3DGE_REQUIRE(!res || (res_c0 >= 0 && res_channels >= 1 && res_c0 + cout <= res_channels), "hgf_conv: residual slice [%d, %d) of %d channels", res_c0,
                  res_c0 + cout, res_channels);
    E3DGE_REQUIRE((int64_t)out_channels * height * width < ((int64_t)1 << 31) && (int64_t)res_channels * height * width < ((int64_t)1 << 31),
                  "hgf_conv: image too large");
    hipStream_t st = as_stream(stream);
    ig_pack(wfrag, w, cin, cout, ksize, 1.0f, st);
    int rc;
    if ((rc = check_launch("hgf_conv(pack)"))) return rc;
    return hgf_conv({out, raw, in, wfrag, in_ab, bias, res, n, cin, cout, height, width, ksize, stride, reflect != 0, out_channels, out_c0, res_channels, res_c0},
                    st);
}

extern "C" int e3dge_hgf_norm(float* ab, const float* x, const float* gamma, const float* beta, int n, int channels_total, int c0, int channels,
                              int groups, int height, int width, e3dge_stream_t stream) {
    E3DGE_REQUIRE(ab && x && gamma && beta, "hgf_norm: null pointer");
    E3DGE_REQUIRE(n >= 1 && n <= 4096 && channels >= 1 && channels <= 4096 && channels_total <= 4096, "hgf_norm: n=%d channels=%d of %d (1..4096)", n, channels,
                  channels_total);
    E3DGE_REQUIRE(c0 >= 0 && c0 + channels <= channels_total, "hgf_norm: channel slice [%d, %d) of %d", c0, c0 + channels, channels_total);
    E3DGE_REQUIRE(groups >= 1 && channels % groups == 0 && channels / groups <= 256, "hgf_norm: groups=%d for %d channels (a divisor, at most 256 channels per group)",
                  groups, channels);
    E3DGE_REQUIRE(height >= 1 && width >= 1 && height <= 4096 && width <= 4096, "hgf_norm: height=%d width=%d (1..4096)", height, width);
    return hgf_norm(ab, x, gamma, beta, n, channels_total, c0, channels, groups, height * width, as_stream(stream));
}

extern "C" int e3dge_hgf_pool(float* out, const float* in, int64_t planes, int height, int width, e3dge_stream_t stream) {
    E3DGE_REQUIRE(out && in, "hgf_pool: null pointer");
    E3DGE_REQUIRE(planes >= 1 && planes <= ((int64_t)1 << 24), "hgf_pool: planes=%lld (1..2^24)", (long long)planes);
    E3DGE_REQUIRE(height >= 2 && width >= 2 && height <= 4096 && width <= 4096 && height % 2 == 0 && width % 2 == 0,
                  "hgf_pool: height=%d width=%d (even, 2..4096)", height, width);
    E3DGE_REQUIRE(planes * (height / 2) * (width / 2) < ((int64_t)1 << 38), "hgf_pool: tensor too large");
    return hgf_pool(out, in, planes, height, width, as_stream(stream));
}

extern "C" int e3dge_hgf_up_add(float* out, const float* up1, const float* low, int64_t planes, int height, int width, e3dge_stream_t stream) {
    E3DGE_REQUIRE(out && up1 && low, "hgf_up_add: null pointer");
    E3DGE_REQUIRE(planes >= 1 && planes <= ((int64_t)1 << 24), "hgf_up_add: planes=%lld (1..2^24)", (long long)planes);
    E3DGE_REQUIRE(height >= 1 && width >= 1 && height <= 2048 && width <= 2048, "hgf_up_add: height=%d width=%d (1..2048)", height, width);
    E3DGE_REQUIRE(planes * 4 * height * width < ((int64_t)1 << 38), "hgf_up_add: tensor too large");
    return hgf_up_add(out, up1, low, planes, height, width, as_stream(stream));
}

#include "hgfilter_bwd.h"
