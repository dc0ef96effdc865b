// The 2-D residual aligner (ADA), forward, eval form: cat(res_gt, up(thumb)) (B, 6, 256, 256) -> aligned_res (B, 3, 256, 256).
//
// Reference: ResidualAligner (project/models/helper_modules/alignment_old.py:316-398) on bottleneck_IR (helpers.py:161-201) with
// aligner_norm_type 'batch' (BatchNorm on its running statistics) and no demodulation; called as self.grid_align
// (project/trainers/E3DGE/e3dge_full_runner.py:138, :257).
//
//   unit(in, depth, stride):  res = BN(conv3x3_stride(PReLU(conv3x3(BN(x)))));  out = res + (in == depth ? x[::stride] : BN(conv1x1_stride(x)))
//   feat1 = PReLU(BN(conv3x3 6->16))                                                  256^2
//   feat2 = units (16,32,2) (32,32,1) (32,32,1)       feat3 = (32,48,2) (48,48,1) x2       feat4 = (48,64,2) (64,64,1) x2      128^2, 64^2, 32^2
//   dfea1 = units (112,64,1) (64,32,1) (32,32,1) of cat(up2(feat4), feat3)            64^2
//   dfea2 = units (64,32,1) (32,16,1) (16,16,1) of cat(up2(dfea1), feat2)             128^2
//   dfea3 = units (32,16,1) (16,3,1) (3,3,1) of cat(up2(dfea2), feat1)                256^2, the output
//
// Kernels (49 launches for one forward, whatever the batch):
//   aln_conv_kernel  the narrow-layer form of the fp32 implicit GEMM of conv_igemm.h: the same v_mfma_f32_16x16x4_f32 steps, the same packed
//                    A-fragment image (ig_pack), K staged through LDS in tiles of kIgKC with the next tile's loads in flight during the
//                    matrix steps, two accumulator chains per output element (even / odd groups of four k), each in ascending k.  The
//                    network's layers have 3 to 64 output channels, so here the four waves split the PIXELS: a workgroup is 64 NT pixels of
//                    ONE image, every wave owns 16 NT of them and all MT = ceil(Cout / 16) channel tiles, and a B fragment read from LDS
//                    feeds MT matrix steps.  No wave idles below 64 channels.  Cout = 3 runs on a zero-padded 16-row tile.
//                    Gather: zero padding; an optional per-input-channel affine on in-image elements (the leading BN: a padded tap stays
//                    0); input channels from up to two tensors split at a run-time channel (the three cats and the call site's
//                    cat(res_gt, thumb), no concatenated copy), the second one optionally read at nearest x4 (src = dst >> 2).
//                    Epilogue: the sum of the two chains, an optional per-output-channel affine (trailing BN), an optional PReLU, an optional
//                    shortcut added after that rounding: a strided pick from a tensor of the input's size (MaxPool2d(1, stride)) or a
//                    read of a tensor of the output's size (the 1x1 branch, a launch of its own).
//   aln_up2_kernel   bilinear x2, align_corners = False, in the separable form of ATen's upsample_bilinear2d:
//                    hy (hx a + lx b) + ly (hx c + lx d), every product and sum rounded on its own.
// No atomics, a fixed summation order, tiles that never straddle images and a tile width from the layer alone (aln_tile_width): results
// are bit-reproducible and an image's values do not depend on the batch.
// Measured errors and times: DESIGN.md 4.17.
#include "conv_igemm.h"

namespace e3dge {

constexpr int kAlnSize = 256, kAlnUnits = 18, kAlnTaps = E3DGE_ALIGNER_TAPS, kAlnSources = E3DGE_ALIGNER_SOURCES, kAlnIn = 6, kAlnStem = 16;
constexpr int kAlnMaxCout = 64;

struct AlnUnit { int cin, depth, stride; };                          // the only statement of the units on this side; aln_net() derives the rest
constexpr AlnUnit kAlnUnit[kAlnUnits] = {{16, 32, 2}, {32, 32, 1}, {32, 32, 1}, {32, 48, 2}, {48, 48, 1}, {48, 48, 1}, {48, 64, 2}, {64, 64, 1}, {64, 64, 1},
                                         {112, 64, 1}, {64, 32, 1}, {32, 32, 1}, {64, 32, 1}, {32, 16, 1}, {16, 16, 1}, {32, 16, 1}, {16, 3, 1}, {3, 3, 1}};

enum { kAlnScNone = 0, kAlnScPick = 1, kAlnScRead = 2 };

template <int NT>
struct AlnTile {
    static constexpr int BN = 64 * NT;                               // pixels per workgroup: 16 NT per wave
    static constexpr int BNP = BN + 16;                              // LDS row pitch: the four k rows of one read land in four bank groups
    static constexpr int ROWS = 256 / BN, PER = kIgKC / ROWS;        // k rows staged per pass, staged elements per thread and tile
};

// The k loop of one workgroup, beside ig_k_loop (conv_igemm.h): the same staging and the same order of the matrix steps per output element
// (step j adds into chain j & 1), with the waves side by side along the pixels.  acc[m][t]: channel tile m, pixel tile t of this wave.
// wa: this lane's dword of the first A fragment of channel tile 0; channel tile m starts m * KS4 fragments later.
template <int MT, int NT, typename Fetch>
__device__ __forceinline__ void aln_k_loop(f32x4 (&acc)[MT][NT][2], const float* wa, int KS4, int n_tiles, Fetch&& fetch) {
    constexpr int BN = AlnTile<NT>::BN, BNP = AlnTile<NT>::BNP, ROWS = AlnTile<NT>::ROWS, PER = AlnTile<NT>::PER;
    __shared__ float bs[kIgKC * BNP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sn = tid % BN, srow = tid / BN;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[m][t][0] = acc[m][t][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float stage[PER];
    fetch(0, stage);
    const float* bw = bs + (lane >> 4) * BNP + wave * 16 * NT + (lane & 15);
#pragma unroll 1
    for (int kt = 0; kt < n_tiles; ++kt) {
        __syncthreads();                                            // the previous tile's reads are done
#pragma unroll
        for (int i = 0; i < PER; ++i) bs[(srow + i * ROWS) * BNP + sn] = stage[i];
        __syncthreads();
        float af[MT][kIgKC / 4];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int j = 0; j < kIgKC / 4; ++j) af[m][j] = wa[((int64_t)m * KS4 + kt * (kIgKC / 4) + j) * 64];
        if (kt + 1 < n_tiles) fetch((kt + 1) * kIgKC, stage);      // in flight during the MFMAs
#pragma unroll
        for (int j = 0; j < kIgKC / 4; ++j) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float b = bw[j * 4 * BNP + t * 16];
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m][t][j & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[m][j], b, acc[m][t][j & 1], 0, 0, 0);
            }
        }
    }
}

struct AlnConvArgs {
    float* out; const float* in0; const float* in1; const float* wfrag;
    const float2* in_ab; const float2* epi_ab; const float* slope; const float* sc;
    int C0, C1, IH, IW, Cout, OH, OW, K, KS4, tiles, stride, up4, sc_mode;
};

template <int KS_, int MT, int NT>
__global__ void __launch_bounds__(256) aln_conv_kernel(AlnConvArgs a) {
    constexpr int BN = AlnTile<NT>::BN, ROWS = AlnTile<NT>::ROWS, PER = AlnTile<NT>::PER;
    constexpr int PAD = KS_ == 3 ? 1 : 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int OHW = a.OH * a.OW, IH = a.IH, IW = a.IW, K = a.K, C0 = a.C0;
    const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
    const int sn = tid % BN, srow = tid / BN;
    const int spix = tile * BN + sn;
    const bool n_ok = spix < OHW;
    const int soy = spix / a.OW, sox = spix - soy * a.OW;
    const int iy0 = soy * a.stride - PAD, ix0 = sox * a.stride - PAD;
    const int H1 = a.up4 ? IH >> 2 : IH, W1 = a.up4 ? IW >> 2 : IW, sh1 = a.up4 ? 2 : 0;
    const float* __restrict__ src0 = a.in0 + (int64_t)img * C0 * IH * IW;
    const float* __restrict__ src1 = a.in1 + (int64_t)img * a.C1 * H1 * W1;          // (never read when C1 == 0)
    const float2* __restrict__ in_ab = a.in_ab;
    auto fetch = [&](int k0, float (&v)[PER]) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = k0 + srow + i * ROWS;
            const auto [ci, r, s] = ig_decode<KS_>(k);
            const int iy = iy0 + r, ix = ix0 + s;
            float x = 0.0f;
            if (n_ok && k < K && iy >= 0 && iy < IH && ix >= 0 && ix < IW) {
                x = ci < C0 ? src0[((int64_t)ci * IH + iy) * IW + ix] : src1[((int64_t)(ci - C0) * H1 + (iy >> sh1)) * W1 + (ix >> sh1)];
                if (in_ab) { const float2 ab = in_ab[ci]; x = __fmaf_rn(ab.x, x, ab.y); }   // the leading BN; padding stays 0
            }
            v[i] = x;
        }
    };
    f32x4 acc[MT][NT][2];
    aln_k_loop<MT, NT>(acc, a.wfrag + lane, a.KS4, a.KS4 / (kIgKC / 4), fetch);
    // C/D fragment: lane l, register r holds D[4 (l >> 4) + r][l & 15]
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int pix = tile * BN + wave * 16 * NT + t * 16 + (lane & 15);
        if (pix >= OHW) continue;
        const int oy = pix / a.OW, ox = pix - oy * a.OW;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m * 16 + 4 * (lane >> 4) + r;
                if (row >= a.Cout) continue;                          // the zero-padded rows of a partial channel tile
                float v = __fadd_rn(acc[m][t][0][r], acc[m][t][1][r]);
                if (a.epi_ab) { const float2 e = a.epi_ab[row]; v = __fmaf_rn(e.x, v, e.y); }
                if (a.slope) v = v > 0.0f ? v : __fmul_rn(a.slope[row], v);
                const int64_t plane = (int64_t)img * a.Cout + row;
                if (a.sc_mode == kAlnScPick) v = __fadd_rn(v, a.sc[(plane * IH + (int64_t)oy * a.stride) * IW + ox * a.stride]);
                else if (a.sc_mode == kAlnScRead) v = __fadd_rn(v, a.sc[plane * OHW + pix]);
                a.out[plane * OHW + pix] = v;                         // helpers.py:198-201: res + shortcut
            }
        }
    }
}

constexpr int aln_out_size(int in, int ks, int stride) { return (in + (ks == 3 ? 2 : 0) - ks) / stride + 1; }

// Pixel tiles per wave: two where 128-pixel workgroups of two images (the evaluation shape) still give every CU one, from the layer alone.
static int aln_tile_width(int64_t pixels) { return (pixels + 127) / 128 * 2 >= kIgCUs ? 2 : 1; }

struct AlnConv {
    float* out; const float* in0; const float* in1; const float* wfrag; const float* in_ab; const float* epi_ab; const float* slope; const float* sc;
    int n, cin, split, up4, cout, h, w, ks, stride, sc_mode;
};

static int aln_conv(const AlnConv& c, hipStream_t st) {
    AlnConvArgs a;
    a.out = c.out; a.in0 = c.in0; a.in1 = c.in1; a.wfrag = c.wfrag; a.slope = c.slope; a.sc = c.sc;
    a.in_ab = reinterpret_cast<const float2*>(c.in_ab); a.epi_ab = reinterpret_cast<const float2*>(c.epi_ab);
    a.C0 = c.split; a.C1 = c.cin - c.split; a.IH = c.h; a.IW = c.w; a.Cout = c.cout;
    a.OH = aln_out_size(c.h, c.ks, c.stride); a.OW = aln_out_size(c.w, c.ks, c.stride);
    a.K = c.cin * c.ks * c.ks; a.KS4 = ig_kpad(a.K) / 4; a.stride = c.stride; a.up4 = c.up4; a.sc_mode = c.sc_mode;
    const int OHW = a.OH * a.OW, nt = aln_tile_width(OHW), bn = 64 * nt, mt = ig_mpad(c.cout) / 16;
    a.tiles = (OHW + bn - 1) / bn;
    const dim3 grid((unsigned)((int64_t)c.n * a.tiles));
    auto with_mt = [&](auto ks_c, auto nt_c) {
        constexpr int KS_ = decltype(ks_c)::value, NT = decltype(nt_c)::value;
        if (mt == 1) aln_conv_kernel<KS_, 1, NT><<<grid, dim3(256), 0, st>>>(a);
        else if (mt == 2) aln_conv_kernel<KS_, 2, NT><<<grid, dim3(256), 0, st>>>(a);
        else if (mt == 3) aln_conv_kernel<KS_, 3, NT><<<grid, dim3(256), 0, st>>>(a);
        else aln_conv_kernel<KS_, 4, NT><<<grid, dim3(256), 0, st>>>(a);
    };
    auto with_nt = [&](auto ks_c) {
        if (nt == 2) with_mt(ks_c, std::integral_constant<int, 2>{});
        else with_mt(ks_c, std::integral_constant<int, 1>{});
    };
    if (c.ks == 3) with_nt(std::integral_constant<int, 3>{});
    else with_nt(std::integral_constant<int, 1>{});
    return check_launch("aln(conv)");
}

// ---- bilinear x2, align_corners = False ---------------------------------------------------------------------------------------------
// ATen's source index: src = 0.5 (dst + 0.5) - 0.5 clamped at 0, i0 = trunc(src), i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1: taps
// 0.25 / 0.75 with the edges clamped; all of it exact in fp32.
__device__ __forceinline__ void aln_up2_tap(int o, int in, int& i0, int& i1, float& l0, float& l1) {
    const float src = fmaxf(__fsub_rn(__fmul_rn(0.5f, __fadd_rn((float)o, 0.5f)), 0.5f), 0.0f);
    i0 = min((int)src, in - 1);
    i1 = i0 + (i0 < in - 1);
    l1 = fminf(fmaxf(__fsub_rn(src, (float)i0), 0.0f), 1.0f);
    l0 = __fsub_rn(1.0f, l1);
}

__global__ void __launch_bounds__(256) aln_up2_kernel(float* __restrict__ out, const float* __restrict__ in, int H, int W, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int OW = 2 * W, OHW = 4 * H * W;
    const int64_t plane = i / OHW;
    const int pix = (int)(i - plane * OHW), oy = pix / OW, ox = pix - oy * OW;
    int y0, y1, x0, x1;
    float hy, ly, hx, lx;
    aln_up2_tap(oy, H, y0, y1, hy, ly);
    aln_up2_tap(ox, W, x0, x1, hx, lx);
    const float* __restrict__ p = in + plane * H * W;
    const float top = __fadd_rn(__fmul_rn(hx, p[y0 * W + x0]), __fmul_rn(lx, p[y0 * W + x1]));
    const float bot = __fadd_rn(__fmul_rn(hx, p[y1 * W + x0]), __fmul_rn(lx, p[y1 * W + x1]));
    out[i] = __fadd_rn(__fmul_rn(hy, top), __fmul_rn(ly, bot));
}

static int aln_up2(float* out, const float* in, int64_t planes, int H, int W, hipStream_t st) {
    const int64_t total = planes * 4 * H * W;
    aln_up2_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(out, in, H, W, total);
    return check_launch("aln(up2)");
}

}  // namespace e3dge

// The kernels around the convolutions (BatchNorm on batch statistics, every backward) with their launch helpers: aligner_bwd.h.  The network
// -- its table, its layouts, the forward walk in both forms and the backward walk: aligner_train.h.  DESIGN.md 4.17, 4.17b.
#include "aligner_bwd.h"

namespace e3dge {

// BatchNorm on its running statistics as the pair (a, b) = (gamma / sqrt(var + 1e-5), beta - mean a)
__global__ void __launch_bounds__(256) aln_pack_bn_kernel(float* __restrict__ dst, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const float* __restrict__ mean, const float* __restrict__ var, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float a = __fdiv_rn(gamma[c], __fsqrt_rn(__fadd_rn(var[c], 1e-5f)));
    dst[2 * c] = a;
    dst[2 * c + 1] = __fsub_rn(beta[c], __fmul_rn(mean[c], a));
}

}  // namespace e3dge

#include "aligner_train.h"

using namespace e3dge;

// ---- argument ranges, each stated once --------------------------------------------------------------------------------------------------
static bool aln_plane_ok(int n, int channels, int height, int width) {
    return n >= 1 && n <= 256 && channels >= 1 && channels <= 4096 && height >= 1 && width >= 1 && height <= 1024 && width <= 1024;
}
#define ALN_REQUIRE_PLANE(who)                                                                                                                  \
    E3DGE_REQUIRE(aln_plane_ok(n, channels, height, width) && (int64_t)n * channels * height * width <= ((int64_t)1 << 31),                     \
                  who ": n=%d (1..256) channels=%d (1..4096) height=%d width=%d (1..1024), at most 2^31 elements", n, channels, height, width)

static bool aln_planes_ok(int64_t planes, int height, int width, int log2_elements) {
    return planes >= 1 && planes <= (1 << 20) && height >= 1 && width >= 1 && height <= 1024 && width <= 1024 &&
           planes * height * width <= ((int64_t)1 << log2_elements);
}

// 0, or the first clause of a convolution's shape that does not hold
static int aln_conv_bad(int n, int cin, int cout, int height, int width, int ksize, int stride) {
    if (!(n >= 1 && n <= 256 && cin >= 1 && cin <= 4096)) return 1;
    if (!(cout >= 1 && cout <= kAlnMaxCout)) return 2;
    if (!((ksize == 1 || ksize == 3) && (stride == 1 || stride == 2))) return 3;
    if (!(height >= 1 && width >= 1 && height <= 1024 && width <= 1024)) return 4;
    return 0;
}
#define ALN_REQUIRE_CONV(who)                                                                                                                   \
    switch (aln_conv_bad(n, cin, cout, height, width, ksize, stride)) {                                                                         \
        case 1: return fail(E3DGE_ERR_INVALID_ARG, who ": n=%d (1..256) cin=%d (1..4096)", n, cin);                                             \
        case 2: return fail(E3DGE_ERR_INVALID_ARG, who ": cout=%d (1..64: the wide layers are the core's)", cout);                              \
        case 3: return fail(E3DGE_ERR_INVALID_ARG, who ": ksize=%d (1 or 3) stride=%d (1 or 2)", ksize, stride);                                \
        case 4: return fail(E3DGE_ERR_INVALID_ARG, who ": height=%d width=%d (1..1024)", height, width);                                        \
    }
#define ALN_REQUIRE_SOURCES(who, channels)                                                                                                      \
    E3DGE_REQUIRE(split >= 0 && split <= channels, who ": split=%d outside [0, " #channels "=%d]", split, channels);                            \
    E3DGE_REQUIRE((split == 0 || in0) && (split == channels || in1), who ": null pointer (a source with channels)")

// What the three network entries check alike, under the entry's name
static int aln_check_call(const char* who, int n, int size, int split, int thumb_up4, const void* res_gt, const void* thumb, const void* packed) {
    E3DGE_REQUIRE(n >= 1 && n <= 256, "%s: n=%d (1..256)", who, n);
    E3DGE_REQUIRE(size == kAlnSize, "%s: size=%d (the network's up-samplings are fixed: 256)", who, size);
    E3DGE_REQUIRE(split >= 0 && split <= kAlnIn, "%s: split=%d (0..6)", who, split);
    E3DGE_REQUIRE(thumb_up4 == 0 || thumb_up4 == 1, "%s: thumb_up4=%d (0 or 1)", who, thumb_up4);
    E3DGE_REQUIRE(packed && (split == 0 || res_gt) && (split == kAlnIn || thumb), "%s: null pointer", who);
    return E3DGE_OK;
}
static int aln_check_sources(const char* who, const float* const* src, int n_src) {
    E3DGE_REQUIRE(n_src == kAlnSources, "%s: n_src=%d, %d source tensors expected", who, n_src, kAlnSources);
    for (int i = 0; i < n_src; ++i) E3DGE_REQUIRE(src[i], "%s: null pointer (source %d)", who, i);
    return E3DGE_OK;
}
#define ALN_REQUIRE_FLOATS(who, what, have, need)                                                                                               \
    E3DGE_REQUIRE((have) >= (need), who ": " what " of %lld floats, %lld needed", (long long)(have), (long long)(need))
#define ALN_REQUIRE_BYTES(who, what, have, need)                                                                                                \
    E3DGE_REQUIRE((have) >= (need), who ": " what " of %lld bytes, %lld needed", (long long)(have), (long long)(need))

template <typename Layout>
static int64_t aln_layout_bytes(const char* who, bool (*layout)(int64_t, Layout*), int n) {
    Layout d;
    if (!layout(n, &d)) {
        fail(E3DGE_ERR_INVALID_ARG, "%s: n=%d (1..256)", who, n);
        return -1;
    }
    return d.total_bytes;
}

// ---- the network ------------------------------------------------------------------------------------------------------------------------------
extern "C" int64_t e3dge_aligner_packed_floats(void) { return aln_net().packed_total; }
extern "C" int64_t e3dge_aligner_packed_t_floats(void) { return aln_net().packed_t_total; }
extern "C" int64_t e3dge_aligner_stats_channels(void) { return aln_net().channels; }
extern "C" int64_t e3dge_aligner_grad_floats(void) { return aln_net().goff[kAlnSources]; }
extern "C" int64_t e3dge_aligner_grad_offset(int source) {
    if (source < 0 || source > kAlnSources) {
        fail(E3DGE_ERR_INVALID_ARG, "aligner_grad_offset: source=%d (0..%d)", source, kAlnSources);
        return -1;
    }
    return aln_net().goff[source];
}
extern "C" int64_t e3dge_aligner_workspace_bytes(int n) { return aln_layout_bytes("aligner_workspace_bytes", aln_ws, n); }
extern "C" int64_t e3dge_aligner_saved_bytes(int n) { return aln_layout_bytes("aligner_saved_bytes", aln_saved, n); }
extern "C" int64_t e3dge_aligner_bwd_workspace_bytes(int n) { return aln_layout_bytes("aligner_bwd_workspace_bytes", aln_bwd_ws, n); }

extern "C" int e3dge_aligner_pack(float* packed, int64_t packed_floats, const float* const* src, int n_src, e3dge_stream_t stream) {
    E3DGE_REQUIRE(packed && src, "aligner_pack: null pointer");
    const AlnNet& net = aln_net();
    ALN_REQUIRE_FLOATS("aligner_pack", "packed buffer", packed_floats, net.packed_total);
    int rc;
    if ((rc = aln_check_sources("aligner_pack", src, n_src))) return rc;
    hipStream_t st = as_stream(stream);
    auto conv = [&](const AlnWeight& w, int ci, int co, int ks) { ig_pack(packed + w.packed, src[w.src], ci, co, ks, 1.0f, st); };
    auto copy = [&](const AlnSlope& p, int ch) { ig_copy(packed + p.packed, src[p.src], ch, 1.0f, 0, st); };
    auto bn = [&](const AlnBn& b) {
        aln_pack_bn_kernel<<<dim3((unsigned)((b.ch + 255) / 256)), dim3(256), 0, st>>>(packed + b.packed, src[b.src], src[b.src + 1], src[b.src + 2],
                                                                                        src[b.src + 3], b.ch);
    };
    conv(net.stem_w, kAlnIn, kAlnStem, 3); bn(net.stem_bn); copy(net.stem_prelu, kAlnStem);
    for (const AlnUnitRow& q : net.u) {                               // res_layer.0 .. 4, then the shortcut
        bn(q.bn0); conv(q.w1, q.cin, q.depth, 3); copy(q.prelu, q.depth); conv(q.w2, q.depth, q.depth, 3); bn(q.bn4);
        if (q.conv_sc) { conv(q.wsc, q.cin, q.depth, 1); bn(q.bnsc); }
    }
    return check_launch("aligner_pack");
}

extern "C" int e3dge_aligner_pack_t(float* packed_t, int64_t packed_t_floats, const float* const* src, int n_src, e3dge_stream_t stream) {
    E3DGE_REQUIRE(packed_t && src, "aligner_pack_t: null pointer");
    const AlnNet& net = aln_net();
    ALN_REQUIRE_FLOATS("aligner_pack_t", "packed buffer", packed_t_floats, net.packed_t_total);
    int rc;
    if ((rc = aln_check_sources("aligner_pack_t", src, n_src))) return rc;
    hipStream_t st = as_stream(stream);
    auto conv = [&](const AlnWeight& w, int ci, int co, int ks) { ig_pack_t(packed_t + w.packed_t, src[w.src], ci, co, ks, 1.0f, st); };
    conv(net.stem_w, kAlnIn, kAlnStem, 3);
    for (const AlnUnitRow& q : net.u) {
        conv(q.w1, q.cin, q.depth, 3); conv(q.w2, q.depth, q.depth, 3);
        if (q.conv_sc) conv(q.wsc, q.cin, q.depth, 1);
    }
    return check_launch("aligner_pack_t");
}

extern "C" int e3dge_aligner_forward(const E3dgeAlignerArgs* args, e3dge_stream_t stream) {
    E3DGE_REQUIRE(args, "aligner_forward: null argument struct");
    const E3dgeAlignerArgs& a = *args;
    int rc;
    if ((rc = aln_check_call("aligner_forward", a.n, a.size, a.split, a.thumb_up4, a.res_gt, a.thumb, a.packed))) return rc;
    E3DGE_REQUIRE(a.out && a.ws, "aligner_forward: null pointer");
    ALN_REQUIRE_FLOATS("aligner_forward", "packed buffer", a.packed_floats, aln_net().packed_total);
    AlnFwd r;
    aln_ws(a.n, &r.ws);
    ALN_REQUIRE_BYTES("aligner_forward", "workspace", a.ws_bytes, r.ws.total_bytes);
    r.n = a.n; r.train = 0; r.P = a.packed; r.src = nullptr; r.stats = nullptr; r.st = as_stream(stream); r.S = nullptr; r.W = static_cast<float*>(a.ws);
    for (int t = 0; t < kAlnTaps - 1; ++t) r.feature[t] = a.taps[t] ? a.taps[t] : r.W + r.ws.feature[t];   // a wanted tap is written in place
    r.feature[kAlnTaps - 1] = a.out;
    return aln_forward(r, a.res_gt, a.thumb, a.split, a.thumb_up4, a.taps, "aligner_forward(tap)");
}

extern "C" int e3dge_aligner_forward_saving(const E3dgeAlignerSaveArgs* args, e3dge_stream_t stream) {
    E3DGE_REQUIRE(args, "aligner_forward_saving: null argument struct");
    const E3dgeAlignerSaveArgs& a = *args;
    int rc;
    if ((rc = aln_check_call("aligner_forward_saving", a.n, a.size, a.split, a.thumb_up4, a.res_gt, a.thumb, a.packed))) return rc;
    E3DGE_REQUIRE(a.train == 0 || a.train == 1, "aligner_forward_saving: train=%d (0 or 1)", a.train);
    E3DGE_REQUIRE(a.out && a.saved && (!a.train || (a.stats && a.src)), "aligner_forward_saving: null pointer");
    if (a.train && (rc = aln_check_sources("aligner_forward_saving", a.src, a.n_src))) return rc;
    const AlnNet& net = aln_net();
    ALN_REQUIRE_FLOATS("aligner_forward_saving", "packed buffer", a.packed_floats, net.packed_total);
    E3DGE_REQUIRE(!a.train || a.stats_doubles >= 2 * (int64_t)net.channels, "aligner_forward_saving: stats of %lld doubles, %lld needed",
                  (long long)a.stats_doubles, (long long)(2 * net.channels));
    AlnFwd r;
    aln_saved(a.n, &r.lay);
    ALN_REQUIRE_BYTES("aligner_forward_saving", "saved state", a.saved_bytes, r.lay.total_bytes);
    r.n = a.n; r.train = a.train; r.P = a.packed; r.src = a.src; r.stats = a.stats; r.st = as_stream(stream); r.S = static_cast<float*>(a.saved); r.W = nullptr;
    for (int t = 0; t < kAlnTaps - 1; ++t) r.feature[t] = r.S + r.lay.feature(t);
    r.feature[kAlnTaps - 1] = a.out;
    return aln_forward(r, a.res_gt, a.thumb, a.split, a.thumb_up4, a.taps, "aligner_forward_saving(tap)");
}

extern "C" int e3dge_aligner_backward(const E3dgeAlignerBwdArgs* args, e3dge_stream_t stream) {
    E3DGE_REQUIRE(args, "aligner_backward: null argument struct");
    const E3dgeAlignerBwdArgs& a = *args;
    int rc;
    if ((rc = aln_check_call("aligner_backward", a.n, a.size, a.split, a.thumb_up4, a.res_gt, a.thumb, a.packed))) return rc;
    E3DGE_REQUIRE(a.train == 0 || a.train == 1, "aligner_backward: train=%d (0 or 1)", a.train);
    E3DGE_REQUIRE(a.want_input == 0 || a.want_input == 1, "aligner_backward: want_input=%d (0 or 1)", a.want_input);
    E3DGE_REQUIRE(a.packed_t && a.src && a.want && a.g_out && a.saved && a.ws && (!a.train || a.stats), "aligner_backward: null pointer");
    E3DGE_REQUIRE(!a.want_input || ((a.split == 0 || a.d_res_gt) && (a.split == kAlnIn || a.d_thumb)), "aligner_backward: null pointer (an input gradient)");
    if ((rc = aln_check_sources("aligner_backward", a.src, a.n_src))) return rc;
    const AlnNet& net = aln_net();
    bool any = false;
    for (int i = 0; i < a.n_src; ++i) any = any || a.want[i];
    E3DGE_REQUIRE(!any || a.grads, "aligner_backward: null pointer (the gradient buffer)");
    E3DGE_REQUIRE(!any || a.grad_floats >= net.goff[kAlnSources], "aligner_backward: gradient buffer of %lld floats, %lld needed", (long long)a.grad_floats,
                  (long long)net.goff[kAlnSources]);
    E3DGE_REQUIRE(a.packed_floats >= net.packed_total && a.packed_t_floats >= net.packed_t_total,
                  "aligner_backward: packed buffers of %lld and %lld floats, %lld and %lld needed", (long long)a.packed_floats, (long long)a.packed_t_floats,
                  (long long)net.packed_total, (long long)net.packed_t_total);
    AlnBwdRun r;
    aln_saved(a.n, &r.lay);
    aln_bwd_ws(a.n, &r.ws);
    ALN_REQUIRE_BYTES("aligner_backward", "saved state", a.saved_bytes, r.lay.total_bytes);
    ALN_REQUIRE_BYTES("aligner_backward", "workspace", a.ws_bytes, r.ws.total_bytes);
    r.n = a.n; r.train = a.train; r.want_input = a.want_input; r.P = a.packed; r.T = a.packed_t; r.src = a.src; r.want = a.want;
    r.S = static_cast<const float*>(a.saved); r.stats = a.stats; r.W = static_cast<float*>(a.ws); r.grads = a.grads; r.st = as_stream(stream);
    if ((rc = aln_stages_bwd(r, a.g_out))) return rc;
    // conv_layer1: PReLU (in place; its pre-activation is the BatchNorm's output), BatchNorm, convolution
    const int n = a.n, S = kAlnSize;
    const float* c0 = r.S + r.lay.c0;
    float* gstage = r.W + r.ws.gstage;
    float* gc0 = r.W + r.ws.gc2;
    if ((rc = aln_prelu_bwd(gstage, r.grad(net.stem_prelu.src), gstage, c0, r.ab(net.stem_bn), a.src[net.stem_prelu.src], r.norm_ws(), n, kAlnStem, S * S, r.st)))
        return rc;
    if ((rc = r.norm_bwd(net.stem_bn, gc0, nullptr, 0, gstage, c0, nullptr, kAlnStem, nullptr, nullptr, S * S))) return rc;
    if (a.want[net.stem_w.src] &&
        (rc = aln_wgrad({r.grad(net.stem_w.src), gc0, a.res_gt, a.thumb, nullptr, r.W + r.ws.wg, n, kAlnIn, a.split, a.thumb_up4, kAlnStem, S, S, 3, 1}, r.st)))
        return rc;
    if (a.want_input) {
        AlnDgrad d{a.d_res_gt, gc0, r.T + net.stem_w.packed_t, nullptr, nullptr, n, kAlnIn, kAlnStem, S, S, 3, 1};
        float* second = a.thumb_up4 ? r.W + r.ws.d256 : a.d_thumb;
        if (a.split == 0) d.gx = second;
        else if (a.split < kAlnIn) { d.gx1 = second; d.gsplit = a.split; }
        if ((rc = aln_dgrad(d, r.st))) return rc;
        if (a.thumb_up4 && a.split < kAlnIn) {
            const int64_t total = (int64_t)n * (kAlnIn - a.split) * (S / 4) * (S / 4);
            aln_down4_kernel<<<dim3(aln_blocks(total)), dim3(256), 0, r.st>>>(a.d_thumb, second, S / 4, S / 4, total);
            if ((rc = check_launch("aln(down4)"))) return rc;
        }
    }
    return E3DGE_OK;
}

// The sign of every PReLU's input of one forward, from its saved state: the stem's, then every unit's
extern "C" int64_t e3dge_aligner_branch_count(int n) {
    if (n < 1 || n > 256) {
        fail(E3DGE_ERR_INVALID_ARG, "aligner_branch_count: n=%d (1..256)", n);
        return -1;
    }
    int64_t per = aln_feature_floats(0);
    for (const AlnUnitRow& q : aln_net().u) per += (int64_t)q.depth * q.size * q.size;
    return n * per;
}

extern "C" int e3dge_aligner_branch_bytes(uint8_t* out, int64_t out_bytes, const float* packed, int64_t packed_floats, const void* saved,
                                          int64_t saved_bytes, int n, int train, e3dge_stream_t stream) {
    E3DGE_REQUIRE(out && packed && saved, "aligner_branch_bytes: null pointer");
    E3DGE_REQUIRE(n >= 1 && n <= 256 && (train == 0 || train == 1), "aligner_branch_bytes: n=%d (1..256) train=%d (0 or 1)", n, train);
    const AlnNet& net = aln_net();
    AlnSaved lay;
    aln_saved(n, &lay);
    ALN_REQUIRE_FLOATS("aligner_branch_bytes", "packed buffer", packed_floats, net.packed_total);
    ALN_REQUIRE_BYTES("aligner_branch_bytes", "saved state", saved_bytes, lay.total_bytes);
    ALN_REQUIRE_BYTES("aligner_branch_bytes", "out", out_bytes, e3dge_aligner_branch_count(n));
    hipStream_t st = as_stream(stream);
    const float* S = static_cast<const float*>(saved);
    int64_t at = 0;
    auto signs = [&](int64_t from, const float* ab, int ch, int size) {
        const int64_t total = (int64_t)n * ch * size * size;
        aln_branch_kernel<<<dim3(aln_blocks(total)), dim3(256), 0, st>>>(out + at, S + from, reinterpret_cast<const float2*>(ab), ch, size * size, total);
        at += total;
    };
    signs(lay.c0, train ? S + lay.ab + 2 * net.stem_bn.chan : packed + net.stem_bn.packed, kAlnStem, kAlnSize);
    for (int u = 0; u < kAlnUnits; ++u) signs(lay.c1[u], nullptr, net.u[u].depth, net.u[u].size);
    return check_launch("aligner_branch_bytes");
}

// ---- every kernel at run-time shapes: the checks, then the helper the network calls -------------------------------------------------------
extern "C" int e3dge_aln_conv(float* out, const float* in0, const float* in1, const float* w, const float* in_ab, const float* epi_ab,
                              const float* slope, const float* shortcut, float* wfrag, int64_t wfrag_floats, int n, int cin, int split, int up4,
                              int cout, int height, int width, int ksize, int stride, int shortcut_mode, e3dge_stream_t stream) {
    E3DGE_REQUIRE(out && w && wfrag, "aln_conv: null pointer");
    ALN_REQUIRE_CONV("aln_conv");
    ALN_REQUIRE_SOURCES("aln_conv", cin);
    E3DGE_REQUIRE(up4 == 0 || (up4 == 1 && height % 4 == 0 && width % 4 == 0), "aln_conv: up4=%d at %d x %d (0, or 1 at multiples of 4)", up4, height, width);
    E3DGE_REQUIRE(shortcut_mode >= kAlnScNone && shortcut_mode <= kAlnScRead && (shortcut_mode == kAlnScNone || shortcut),
                  "aln_conv: shortcut_mode=%d (0 none, 1 strided pick, 2 read) needs its tensor", shortcut_mode);
    ALN_REQUIRE_FLOATS("aln_conv", "wfrag", wfrag_floats, aln_image_floats(cin, cout, ksize));
    hipStream_t st = as_stream(stream);
    ig_pack(wfrag, w, cin, cout, ksize, 1.0f, st);
    int rc;
    if ((rc = check_launch("aln_conv(pack)"))) return rc;
    return aln_conv({out, in0, in1, wfrag, in_ab, epi_ab, slope, shortcut, n, cin, split, up4, cout, height, width, ksize, stride, shortcut_mode}, st);
}

extern "C" int e3dge_aln_up2(float* out, const float* in, int64_t planes, int height, int width, e3dge_stream_t stream) {
    E3DGE_REQUIRE(out && in, "aln_up2: null pointer");
    E3DGE_REQUIRE(aln_planes_ok(planes, height, width, 62 /* no bound on the elements */), "aln_up2: planes=%lld (1..2^20) height=%d width=%d (1..1024)", (long long)planes, height, width);
    return aln_up2(out, in, planes, height, width, as_stream(stream));
}

extern "C" int64_t e3dge_aln_norm_ws_bytes(int n, int channels, int height, int width) {
    if (!aln_plane_ok(n, channels, height, width)) {
        fail(E3DGE_ERR_INVALID_ARG, "aln_norm_ws_bytes: n=%d (1..256) channels=%d (1..4096) height=%d width=%d (1..1024)", n, channels, height, width);
        return -1;
    }
    return aln_norm_ws_bytes(n, channels, height * width);
}

extern "C" int e3dge_aln_bn_stats(float* ab, double* stats, const float* in0, const float* in1, const float* gamma, const float* beta, void* ws,
                                  int64_t ws_bytes, int n, int channels, int split, int height, int width, e3dge_stream_t stream) {
    E3DGE_REQUIRE((ab || stats) && ws && (!ab || (gamma && beta)), "aln_bn_stats: null pointer");
    ALN_REQUIRE_PLANE("aln_bn_stats");
    ALN_REQUIRE_SOURCES("aln_bn_stats", channels);
    const int hw = height * width;
    E3DGE_REQUIRE((int64_t)n * hw >= 2, "aln_bn_stats: %lld values per channel (batch statistics need 2)", (long long)n * hw);
    ALN_REQUIRE_BYTES("aln_bn_stats", "workspace", ws_bytes, aln_norm_ws_bytes(n, channels, hw));
    return aln_stats(ab, stats, static_cast<double*>(ws), in0, in1, gamma, beta, n, channels, split, hw, as_stream(stream));
}

extern "C" int e3dge_aln_bn_apply(float* out, const float* in, const float* ab, const float* slope, const float* shortcut, const float* shortcut_ab,
                                  int n, int channels, int height, int width, int shortcut_height, int shortcut_width, int stride, int shortcut_mode,
                                  e3dge_stream_t stream) {
    E3DGE_REQUIRE(out && in && ab, "aln_bn_apply: null pointer");
    ALN_REQUIRE_PLANE("aln_bn_apply");
    E3DGE_REQUIRE(shortcut_mode >= kAlnScNone && shortcut_mode <= kAlnScAffine && (shortcut_mode == kAlnScNone || shortcut) &&
                      (shortcut_mode != kAlnScAffine || shortcut_ab),
                  "aln_bn_apply: shortcut_mode=%d (0 none, 1 strided pick, 2 read, 3 read under its own affine) needs its tensors", shortcut_mode);
    if (shortcut_mode == kAlnScPick) {
        E3DGE_REQUIRE(stride == 1 || stride == 2, "aln_bn_apply: stride=%d (1 or 2)", stride);
        E3DGE_REQUIRE(shortcut_height >= 1 && shortcut_width >= 1 && shortcut_height <= 1024 && shortcut_width <= 1024 &&
                          (shortcut_height - 1) / stride + 1 == height && (shortcut_width - 1) / stride + 1 == width,
                      "aln_bn_apply: a %d x %d shortcut picked at stride %d is not %d x %d", shortcut_height, shortcut_width, stride, height, width);
    }
    return aln_apply(out, in, ab, slope, shortcut, shortcut_ab, n, channels, height, width, shortcut_height, shortcut_width, stride, shortcut_mode,
                     as_stream(stream));
}

extern "C" int e3dge_aln_norm_bwd(float* gx, float* dgamma, float* dbeta, const float* gy, const float* in0, const float* in1, const float* gamma,
                                  const double* stats, const float* running_mean, const float* running_var, const float* add, void* ws,
                                  int64_t ws_bytes, int n, int channels, int split, int height, int width, int train, e3dge_stream_t stream) {
    E3DGE_REQUIRE((gx || dgamma || dbeta) && gy && gamma && ws, "aln_norm_bwd: null pointer");
    E3DGE_REQUIRE(train == 0 || train == 1, "aln_norm_bwd: train=%d (0 or 1)", train);
    E3DGE_REQUIRE(train ? stats != nullptr : (running_mean && running_var), "aln_norm_bwd: null pointer (the statistics of this form)");
    ALN_REQUIRE_PLANE("aln_norm_bwd");
    E3DGE_REQUIRE(split >= 0 && split <= channels, "aln_norm_bwd: split=%d outside [0, channels=%d]", split, channels);
    const bool reads_x = train || dgamma || dbeta;                    // on running statistics g_x = A g reads no x
    E3DGE_REQUIRE(!reads_x || ((split == 0 || in0) && (split == channels || in1)), "aln_norm_bwd: null pointer (a source with channels)");
    const int hw = height * width;
    ALN_REQUIRE_BYTES("aln_norm_bwd", "workspace", ws_bytes, aln_norm_ws_bytes(n, channels, hw));
    return aln_norm_bwd(gx, nullptr, 0, dgamma, dbeta, gy, in0, in1, split, gamma, stats, running_mean, running_var, add, nullptr, static_cast<double*>(ws), n,
                        channels, hw, train, as_stream(stream));
}

extern "C" int e3dge_aln_prelu_bwd(float* gx, float* dslope, const float* gy, const float* pre, const float* slope, void* ws, int64_t ws_bytes, int n,
                                   int channels, int height, int width, e3dge_stream_t stream) {
    E3DGE_REQUIRE((gx || dslope) && gy && pre && slope && (!dslope || ws), "aln_prelu_bwd: null pointer");
    ALN_REQUIRE_PLANE("aln_prelu_bwd");
    const int hw = height * width;
    E3DGE_REQUIRE(!dslope || ws_bytes >= aln_norm_ws_bytes(n, channels, hw), "aln_prelu_bwd: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
                  (long long)aln_norm_ws_bytes(n, channels, hw));
    return aln_prelu_bwd(gx, dslope, gy, pre, nullptr, slope, static_cast<double*>(ws), n, channels, hw, as_stream(stream));
}

extern "C" int e3dge_aln_up2_bwd(float* gx, const float* gy, int64_t planes, int height, int width, e3dge_stream_t stream) {
    E3DGE_REQUIRE(gx && gy, "aln_up2_bwd: null pointer");
    E3DGE_REQUIRE(aln_planes_ok(planes, height, width, 29), "aln_up2_bwd: planes=%lld (1..2^20) height=%d width=%d (1..1024), at most 2^29 elements",
                  (long long)planes, height, width);
    return aln_up2_bwd(gx, gy, planes, height, width, as_stream(stream));
}

extern "C" int e3dge_aln_pick_bwd(float* gx, const float* gy, const float* add, int64_t planes, int height, int width, int stride,
                                  e3dge_stream_t stream) {
    E3DGE_REQUIRE(gx && gy, "aln_pick_bwd: null pointer");
    E3DGE_REQUIRE(aln_planes_ok(planes, height, width, 31), "aln_pick_bwd: planes=%lld (1..2^20) height=%d width=%d (1..1024), at most 2^31 elements",
                  (long long)planes, height, width);
    E3DGE_REQUIRE(stride == 1 || stride == 2, "aln_pick_bwd: stride=%d (1 or 2)", stride);
    return aln_pick_bwd(gx, gy, add, planes, height, width, stride, as_stream(stream));
}

extern "C" int e3dge_aln_conv_dgrad(float* gx, const float* gy, const float* w, const float* add0, const float* add1, float* wfrag,
                                    int64_t wfrag_floats, int n, int cin, int cout, int height, int width, int ksize, int stride, e3dge_stream_t stream) {
    E3DGE_REQUIRE(gx && gy && w && wfrag, "aln_conv_dgrad: null pointer");
    ALN_REQUIRE_CONV("aln_conv_dgrad");
    ALN_REQUIRE_FLOATS("aln_conv_dgrad", "wfrag", wfrag_floats, aln_image_t_floats(cin, cout, ksize));
    hipStream_t st = as_stream(stream);
    ig_pack_t(wfrag, w, cin, cout, ksize, 1.0f, st);
    int rc;
    if ((rc = check_launch("aln_conv_dgrad(pack)"))) return rc;
    return aln_dgrad({gx, gy, wfrag, add0, add1, n, cin, cout, height, width, ksize, stride}, st);
}

extern "C" int64_t e3dge_aln_wgrad_ws_floats(int n, int cin, int cout, int height, int width, int ksize, int stride) {
    if (aln_conv_bad(n, cin, cout, height, width, ksize, stride)) {
        fail(E3DGE_ERR_INVALID_ARG, "aln_wgrad_ws_floats: n=%d (1..256) cin=%d (1..4096) cout=%d (1..64) height=%d width=%d (1..1024) ksize=%d (1 or 3) "
             "stride=%d (1 or 2)", n, cin, cout, height, width, ksize, stride);
        return -1;
    }
    return aln_wgrad_ws_floats(n, cin, cout, height, width, ksize, stride);
}

extern "C" int e3dge_aln_conv_wgrad(float* dw, const float* gy, const float* in0, const float* in1, const float* in_ab, float* ws, int64_t ws_floats,
                                    int n, int cin, int split, int up4, int cout, int height, int width, int ksize, int stride,
                                    e3dge_stream_t stream) {
    E3DGE_REQUIRE(dw && gy && ws, "aln_conv_wgrad: null pointer");
    ALN_REQUIRE_CONV("aln_conv_wgrad");
    ALN_REQUIRE_SOURCES("aln_conv_wgrad", cin);
    E3DGE_REQUIRE(up4 == 0 || (up4 == 1 && height % 4 == 0 && width % 4 == 0), "aln_conv_wgrad: up4=%d at %d x %d (0, or 1 at multiples of 4)", up4, height,
                  width);
    ALN_REQUIRE_FLOATS("aln_conv_wgrad", "workspace", ws_floats, aln_wgrad_ws_floats(n, cin, cout, height, width, ksize, stride));
    return aln_wgrad({dw, gy, in0, in1, in_ab, ws, n, cin, split, up4, cout, height, width, ksize, stride}, as_stream(stream));
}
