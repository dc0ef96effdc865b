// The fp32 implicit-GEMM core of the LPIPS, identity-term and discriminator convolutions (lpips.hip, idnet.hip, disc.hip and their
// backward headers): everything the four kernels lpips_conv_kernel, idnet_conv_kernel, idnet_dgrad_kernel and disc_gemm_kernel share.
// Each of them keeps its own gather (what a staged element is) and its own epilogue; the rest is here, once.
//
//   GEMM        D[M][N] = A[M][K] B[K][N] on v_mfma_f32_16x16x4_f32, fp32 throughout.  M = output channels, K = (channel, r, s), N = output
//               pixels.  A workgroup is 4 waves = kIgBM = 64 channels x 16 NT pixels (NT = 1, 2, 4); every wave owns one 16-channel tile.
//   A operand   read from a packed weight image in fragment order, one coalesced dword per lane and matrix step, no LDS:
//               image[(mt * KS4 + ks) * 64 + lane] = A[mt * 16 + (lane & 15)][ks * 4 + (lane >> 4)], 0 past M or K, K padded to kIgKC
//               (ig_kpad) and M to 16 (ig_mpad).  conv_pack_kernel writes it from W[M][K], conv_pack_t_kernel writes the transposed,
//               tap-flipped image of a data gradient; both round `w * scale` once (scale 1 is exact).  conv_copy_kernel moves what
//               is not a fragment image (biases, linear layers, FIRs) into the same packed buffer, with the same rounding.
//   B operand   the im2col tile of kIgKC = 32 k x 16 NT pixels, staged in LDS by the kernel's gather with the NEXT tile's loads in
//               flight during the matrix steps.  Row pitch BN + 16: the four k rows of one read land in four bank groups.
//   k loop      ig_k_loop: per staged tile eight A fragments and eight matrix steps per pixel tile; step j adds into accumulator
//               j % NACC, so every output element is the sum of NACC chains (NACC = 2: even / odd groups of four k), each in ascending
//               k, whatever the tile shape.  A per-tile hook lets the discriminator fold its four chains into fp64 every kDcFlush tiles.
//   tile width  ig_tile_width: the widest tile that still gives every CU a workgroup, from the layer alone.
#pragma once
#include <type_traits>

#include "common.h"

namespace e3dge {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kIgKC = 32;                       // k per staged tile (8 MFMA steps)
constexpr int kIgBM = 64;                       // channels per workgroup (4 waves x 16)
constexpr int kIgCUs = 256;                     // compute units of the MI355X: the tile width is chosen to give each a workgroup

__host__ __device__ constexpr int ig_kpad(int K) { return (K + kIgKC - 1) / kIgKC * kIgKC; }
__host__ __device__ constexpr int ig_mpad(int M) { return (M + 15) / 16 * 16; }

template <int NT>
struct IgTile {
    static constexpr int BN = 16 * NT;                              // pixels per workgroup
    static constexpr int BNP = NT == 1 ? 16 : BN + 16;              // LDS row pitch
    static constexpr int ROWS = 256 / BN, PER = kIgKC / ROWS;       // k rows staged per pass, staged elements per thread and tile
};

// k = (c * KS + r) * KS + s
struct IgTap { int c, r, s; };
template <int KS>
__device__ __forceinline__ IgTap ig_decode(int k) {
    constexpr int KK = KS * KS;
    const int c = k / KK, rs = k - c * KK, r = rs / KS;
    return {c, r, rs - r * KS};
}

// The whole k loop of one workgroup.  acc: zeroed here, NACC chains per pixel tile.  wa: this lane's dword of the wave's first A fragment.
// fetch(k0, v): the PER elements (k0 + tid / BN + i ROWS, pixel tid % BN) of this thread.  hook(kt, last): after tile kt's matrix steps.
// IDLE: waves past M exist (live == false); they stage and synchronise but load no A and run no matrix step.  Without IDLE no test of
// `live` is compiled.
template <int NT, int NACC, bool IDLE, typename Fetch, typename Hook>
__device__ __forceinline__ void ig_k_loop(f32x4 (&acc)[NT][NACC], const float* wa, int n_tiles, bool live, Fetch&& fetch,
                                          Hook&& hook) {
    constexpr int BN = IgTile<NT>::BN, BNP = IgTile<NT>::BNP, ROWS = IgTile<NT>::ROWS, PER = IgTile<NT>::PER;
    static_assert((NACC & (NACC - 1)) == 0 && NACC <= kIgKC / 4, "accumulator count");
    __shared__ float bs[kIgKC * BNP];
    const int tid = threadIdx.x, lane = tid & 63;
    const int sn = tid % BN, srow = tid / BN;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int h = 0; h < NACC; ++h) acc[t][h] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float stage[PER];
    fetch(0, stage);
#pragma unroll 1                                                    // rolled and unpeeled: a peeled first tile costs disc_gemm_kernel 12 to 48 registers
    for (int kt = 0; kt < n_tiles; ++kt) {
        __syncthreads();                                            // the previous tile's reads are done
#pragma unroll
        for (int i = 0; i < PER; ++i) bs[(srow + i * ROWS) * BNP + sn] = stage[i];
        __syncthreads();
        float af[kIgKC / 4];
        if (!IDLE || live) {
#pragma unroll
            for (int j = 0; j < kIgKC / 4; ++j) af[j] = wa[(int64_t)(kt * (kIgKC / 4) + j) * 64];
        }
        if (kt + 1 < n_tiles) fetch((kt + 1) * kIgKC, stage);      // in flight during the MFMAs
        if (!IDLE || live) {
#pragma unroll
            for (int j = 0; j < kIgKC / 4; ++j) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float b = bs[(j * 4 + (lane >> 4)) * BNP + t * 16 + (lane & 15)];
                    acc[t][j & (NACC - 1)] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j], b, acc[t][j & (NACC - 1)], 0, 0, 0);
                }
            }
            hook(kt, kt + 1 == n_tiles);
        }
    }
}

// ---- packing ------------------------------------------------------------------------------------------------------------------
// dst = the A-fragment image of fl(W[M][K] * scale)
static __global__ void __launch_bounds__(256) conv_pack_kernel(float* __restrict__ dst, const float* __restrict__ w, int M, int K, int KS4, float scale,
                                                               int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int lane = (int)(i & 63);
    const int64_t t = i >> 6;
    const int ks = (int)(t % KS4), mt = (int)(t / KS4);
    const int row = mt * 16 + (lane & 15), k = ks * 4 + (lane >> 4);
    dst[i] = (row < M && k < K) ? __fmul_rn(w[(int64_t)row * K + k], scale) : 0.0f;
}

// dst = the A-fragment image of Wt[ci][(co, r, s)] = fl(W[co][ci][KS - 1 - r][KS - 1 - s] * scale)
static __global__ void __launch_bounds__(256) conv_pack_t_kernel(float* __restrict__ dst, const float* __restrict__ w, int Cin, int Cout, int KS,
                                                                 int KS4, float scale, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int lane = (int)(i & 63), KK = KS * KS;
    const int64_t t = i >> 6;
    const int ks = (int)(t % KS4), mt = (int)(t / KS4);
    const int ci = mt * 16 + (lane & 15), k = ks * 4 + (lane >> 4);
    float v = 0.0f;
    if (ci < Cin && k < Cout * KK) {
        const int co = k / KK, rs = k - co * KK, r = rs / KS, s = rs - r * KS;
        v = __fmul_rn(w[(((int64_t)co * Cin + ci) * KS + (KS - 1 - r)) * KS + (KS - 1 - s)], scale);
    }
    dst[i] = v;
}

// dst[i] = fl(src[i] * scale); flip: src is read back to front.  Everything of a packed image that is not an A-fragment image: biases,
// the linear layers, the FIR of a blur (flipped: its adjoint's).
static __global__ void __launch_bounds__(256) conv_copy_kernel(float* __restrict__ dst, const float* __restrict__ src, float scale, int flip,
                                                               int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) dst[i] = __fmul_rn(src[flip ? total - 1 - i : i], scale);
}

static inline void ig_copy(float* dst, const float* src, int64_t total, float scale, int flip, hipStream_t st) {
    conv_copy_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(dst, src, scale, flip, total);
}

// W (cout, cin, ks, ks) -> the forward image: ig_mpad(cout) * ig_kpad(cin ks ks) floats
static inline void ig_pack(float* dst, const float* w, int cin, int cout, int ks, float scale, hipStream_t st) {
    const int K = cin * ks * ks, kpad = ig_kpad(K);
    const int64_t total = (int64_t)ig_mpad(cout) * kpad;
    conv_pack_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(dst, w, cout, K, kpad / 4, scale, total);
}

// W (cout, cin, ks, ks) -> the data gradient's image: ig_mpad(cin) * ig_kpad(cout ks ks) floats
static inline void ig_pack_t(float* dst, const float* w, int cin, int cout, int ks, float scale, hipStream_t st) {
    const int kpad = ig_kpad(cout * ks * ks);
    const int64_t total = (int64_t)ig_mpad(cin) * kpad;
    conv_pack_t_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(dst, w, cin, cout, ks, kpad / 4, scale, total);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
// Pixels per workgroup / 16: the widest tile that still gives every CU a workgroup when `images` images of `pixels` pixels run with gy
// channel blocks.  LPIPS passes its flattened N once; the other two pass ONE image's pixels and count two images (the evaluation
// shape), so that an image's tiles, and with them its partial sums, do not depend on the batch.
inline int ig_tile_width(int64_t pixels, int images, int64_t gy) {
    auto blocks = [&](int bn) { return (pixels + bn - 1) / bn; };
    return blocks(64) * images * gy >= kIgCUs ? 4 : blocks(32) * images * gy >= kIgCUs ? 2 : 1;
}

// f(std::integral_constant<int, NT>) for the run-time nt: the one place a tile width becomes a template argument
template <typename F>
inline void ig_dispatch_nt(int nt, F&& f) {
    if (nt == 4) f(std::integral_constant<int, 4>{});
    else if (nt == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 1>{});
}

}  // namespace e3dge
