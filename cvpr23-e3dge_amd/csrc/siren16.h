// The split-f16 ("f16x3") fused renderer, second generation: 8 waves per workgroup (two per SIMD), 16 points per wave,
// v_mfma_f32_16x16x32_f16.  Included by siren.hip (shares its launch code); see siren.hip for the reference lines of every
// phase and DESIGN.md 4.1c for the numbers.
//
// Why: the first f16x3 kernel (one wave per SIMD, 32 points per wave, 32x32x16 MFMAs) keeps the matrix pipe 41 % busy -- with a
// single wave on a SIMD every weight-fragment ds_read, every epilogue VALU op and every thin phase between the layers comes
// straight out of the MFMA stream.  Halving the points per wave halves the register-resident state (64 + 64 registers of
// packed f16 hi/lo activations instead of 128 + 128), so two waves fit on a SIMD and one wave's LDS reads / epilogue run
// under the other's MFMAs.  Price: every wave still reads the whole weight chunk for its (now 16) points, so LDS read
// traffic per point doubles (to ~60 % of the 256 B/clk ds_read_b128 rate) -- affordable, because the LDS itself was never
// the bottleneck, the single wave's issue stream was.
//
// Fragment conventions (validated on the GPU by e3dge_selftest_mfma16x16): lane l, n = l & 15, q = l >> 4
//   A (16 x 32): row n, k = 8q + j          B (32 x 16): column n, k = 8q + j          C/D (16 x 16): column n, rows 4q + r
// Standard layers: A = weights (16 out features x 32 k), B = activations (32 k x 16 points): D[feature 16t + 4q + r][point n].
// A lane's C/D registers of the tiles 2g, 2g+1 (features 32g + 16e + 4q + r) are its 8 k-slots of k-step g of the next layer
// -- the weight image (kOffBig16b) is packed in that k order, so activations never leave the registers.
// View layer: the same registers as the A operand, weights as B: D[point 4q + r][feature n] (features on lanes).
#pragma once
#include "siren_common.h"

namespace e3dge {

typedef float f32x4v __attribute__((ext_vector_type(4)));

constexpr int k16Threads = 512;
constexpr int k16Tiles = 16;                     // 16-feature output tiles per layer
constexpr int k16Steps = 8;                      // k-steps of 32 per tile
constexpr int k16ChunkFloats = 16 * kWidth;      // one tile x K = 256: 16 KiB
constexpr int k16Chunks = kBigLayers * k16Tiles; // 128 chunks per 128-point sub-tile
// One workgroup barrier per tile.  (Per two tiles with a fifth LDS buffer measured the same, 0.3140 vs 0.3145 ms: the wait at
// the barrier is where the two waves of a SIMD queue for the matrix pipe, not a cost of the barrier -- removed)
constexpr int k16NBuf = 4;                       // LDS weight buffers
constexpr int k16Slots = 2;                      // rays a 16-point slab can touch when S >= 16
// k-steps of (hi, lo) fragments held in registers (must divide 8).  2, 4 and 8 measured the same (0.320 / 0.320 / 0.323 ms):
// the fragment reads are not latency-exposed
constexpr int k16Ring = 2;

// ---- LDS carve (floats) ----
// The small tables come first: everything the tile streams read from them lies below 64 KiB, inside the 16-bit offset field of a
// ds_read, so a FiLM row or a view record is one base register + an immediate (behind the weight buffers, at 0x14000 and up, every
// tile rebuilt two addresses in the VALU).
constexpr int k16LdsFilm = 0;                                         // [9][2][256]
constexpr int k16LdsHead = k16LdsFilm + 9 * 2 * kWidth;               // w_sigma[256], w_rgb[3][256], b_sigma, b_rgb[3]
constexpr int k16LdsW0 = k16LdsHead + kHeadFloats;                    // [3][256] first-layer weights, column-major
// [2][256][4] per-feature record of the view layer, one ds_read_b128 per half: (gamma, beta, w_r, w_g), (w_b, view-direction
// columns x, y, z x128) -- gamma / beta as in the FiLM block (bias folded in, 1/128 divided out), w_rgb a copy of the head's
constexpr int k16LdsVrec = k16LdsW0 + 3 * kWidth;
constexpr int k16LdsW = k16LdsVrec + 2 * 4 * kWidth;                  // [k16NBuf] weight chunks
constexpr int k16LdsFeat = k16LdsW + k16NBuf * k16ChunkFloats;        // [kRMax][kFPitch]
constexpr int k16LdsPart = k16LdsFeat + kRMax * kFPitch;              // [8 waves][2 slots][256]
constexpr int k16LdsAlpha = ((k16LdsPart + 8 * k16Slots * kWidth + 3) / 4) * 4;
constexpr int k16LdsWgt = k16LdsAlpha + kTilePts;
constexpr int k16LdsZ = k16LdsWgt + kTilePts;
constexpr int k16LdsPts = k16LdsZ + kTilePts;                         // [128][3]
constexpr int k16LdsRgb = k16LdsPts + kTilePts * 3;                   // [128][3]
constexpr int k16LdsState = k16LdsRgb + kTilePts * 3;                 // [kRMax][12]
constexpr int k16LdsWq = ((k16LdsState + kRMax * kStateStride + 3) / 4) * 4;   // [8 waves][2 slots][16 rows]
constexpr int k16LdsVd = k16LdsWq + 8 * k16Slots * 16;                // [8 waves][16 points][4]: view direction (padded)
constexpr int k16LdsFloats = k16LdsVd + 8 * 16 * 4;
constexpr int k16LdsBytes = k16LdsFloats * 4;
static_assert(k16LdsBytes <= 160 * 1024, "LDS budget");
static_assert((k16LdsFilm % 4) == 0 && (k16LdsHead % 4) == 0 && (k16LdsW0 % 4) == 0 && (k16LdsVrec % 4) == 0 && (k16LdsW % 4) == 0, "alignment");
static_assert(k16LdsW * 4 <= 64 * 1024, "the tables stay inside the ds_read offset field");

// one 16-byte store of saved state: non-temporal (against plain stores an A/B of round 6)
__device__ __forceinline__ void save_st4(float* p, const f32x4v& v) {
    __builtin_nontemporal_store(v, reinterpret_cast<f32x4v*>(p));
}
__device__ __forceinline__ f32x4v mfma16x16(u32x4 a, u32x4 b, f32x4v c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, a), __builtin_bit_cast(half8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4v zero4() { return f32x4v{0.f, 0.f, 0.f, 0.f}; }
// acc + w * (f16 half `HI` of the packed word p), one instruction
template <int HI> __device__ __forceinline__ float fma_mix_h(unsigned p, float w, float acc) {
    float r;
    if (HI) asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(p), "v"(w), "v"(acc));
    else asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(p), "v"(w), "v"(acc));
    return r;
}
// value r (0..3) of 16-feature tile t from the packed (hi, lo) activations
__device__ __forceinline__ float act16_get(const u32x4 (&aH)[k16Steps], const u32x4 (&aL)[k16Steps], int t, int r) {
    const int g = t >> 1, w = 2 * (t & 1) + (r >> 1);
    return (r & 1) ? f16hi(aH[g][w]) + f16hi(aL[g][w]) : f16lo(aH[g][w]) + f16lo(aL[g][w]);
}
// sum over the 16 lanes of a row (every lane of the row gets the total)
__device__ __forceinline__ float row_sum16(float x) {
    x += dpp_f32<0x128>(x);    // row_ror:8
    x += dpp_f32<0x124>(x);    // row_ror:4
    x += dpp_f32<0x122>(x);    // row_ror:2
    x += dpp_f32<0x121>(x);    // row_ror:1
    return x;
}

// x[l] + x[l ^ 16] + x[l ^ 32] + x[l ^ 48] in every lane (the sum over the four 16-lane groups q), in the VALU: v_permlane16_swap
// exchanges the odd rows of its first operand with the even rows of the second, v_permlane32_swap the upper half of the first
// with the lower half of the second -- fed the same register twice, the two results add up to the pairwise sums.  (The same
// tree as two __shfl_xor steps, without their ds_bpermute round trips through the LDS crossbar.)
__device__ __forceinline__ float sum_over_q(float x) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    const float y = __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
    const unsigned v = __builtin_bit_cast(unsigned, y);
    const auto t = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return __builtin_bit_cast(float, (unsigned)t[0]) + __builtin_bit_cast(float, (unsigned)t[1]);
}

// Wave-wide inclusive scans in the VALU (dpp_or, gfx950_prims.h): four shifted steps inside every 16-lane row, then lane 15 of rows
// 0 / 2 into rows 1 / 3 and lane 31 into rows 2 and 3.  Lanes a step does not reach combine with the identity.  Lane 63 ends up
// with the reduction over the wave.
__device__ __forceinline__ float wave_incl_prod(float x) {
    x = __fmul_rn(x, dpp_or<0x111, 0xf>(1.0f, x));
    x = __fmul_rn(x, dpp_or<0x112, 0xf>(1.0f, x));
    x = __fmul_rn(x, dpp_or<0x114, 0xf>(1.0f, x));
    x = __fmul_rn(x, dpp_or<0x118, 0xf>(1.0f, x));
    x = __fmul_rn(x, dpp_or<0x142, 0xa>(1.0f, x));
    x = __fmul_rn(x, dpp_or<0x143, 0xc>(1.0f, x));
    return x;
}
__device__ __forceinline__ float wave_sum_last(float x) {      // the sum over the wave, valid in lane 63 (broadcast below)
    x = __fadd_rn(x, dpp_or<0x111, 0xf>(0.0f, x));
    x = __fadd_rn(x, dpp_or<0x112, 0xf>(0.0f, x));
    x = __fadd_rn(x, dpp_or<0x114, 0xf>(0.0f, x));
    x = __fadd_rn(x, dpp_or<0x118, 0xf>(0.0f, x));
    x = __fadd_rn(x, dpp_or<0x142, 0xa>(0.0f, x));
    x = __fadd_rn(x, dpp_or<0x143, 0xc>(0.0f, x));
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}

// 16-KiB weight chunks through k16NBuf LDS buffers; every wave moves a 2-KiB slice (two LDS-DMA pieces) of each chunk.
//   tile g: sync() -> wait for everything but the chunk issued one tile ago, barrier (publishes chunk g+2, proves tile g-1 is
//   finished) -> issue chunk g+3 into the buffer tile g-1 used: two tile times to arrive.
// The chunk may be issued anywhere in tile g behind that barrier, as long as its two pieces stay in this order and in this tile
// (the counted wait is about the youngest two operations): the inference renders issue them two and three k-steps behind the
// barrier, one piece per k-step (issue_piece), everything else right behind it (issue_chunk).
struct ChunkPipe16 {
    const char* img;
    uint32_t voff, lds_base;
    int idx, buf, use_buf, count;
    float* wbuf;
    const float* wcur;
    const float* wnxt;
    // `image` = first chunk of the cycle, `count_` chunks per 128-point sub-tile (the cycle then starts over)
    __device__ __forceinline__ void init(float* wbuf_, const float* image, int wave, int lane, int count_ = k16Chunks) {
        const int wave_u = __builtin_amdgcn_readfirstlane(wave);
        wbuf = wbuf_;
        count = count_;
        img = reinterpret_cast<const char*>(image) + wave_u * 2048;
        voff = (uint32_t)lane * 16u;
        lds_base = lds_addr(wbuf_) + (uint32_t)wave_u * 2048u;
        idx = 0; buf = 0; use_buf = 0;
        wcur = wbuf_; wnxt = wbuf_ + k16ChunkFloats;
    }
    __device__ __forceinline__ void issue_chunk() {
        const char* s = img + (size_t)idx * (k16ChunkFloats * 4);
        const uint32_t d = lds_base + (uint32_t)buf * (k16ChunkFloats * 4);
        glds16_saddr<0>(s, voff, d);
        glds16_saddr<1024>(s, voff, d);
        idx = (idx + 1 == count) ? 0 : idx + 1;
        buf = (buf + 1 == k16NBuf) ? 0 : buf + 1;
    }
    template <int PIECE> __device__ __forceinline__ void issue_piece() {      // issue_chunk() as two calls: PIECE 0, then PIECE 1
        const char* s = img + (size_t)idx * (k16ChunkFloats * 4);
        const uint32_t d = lds_base + (uint32_t)buf * (k16ChunkFloats * 4);
        if (PIECE == 0) {
            glds16_saddr<0>(s, voff, d);
        } else {
            glds16_saddr<1024>(s, voff, d);
            idx = (idx + 1 == count) ? 0 : idx + 1;
            buf = (buf + 1 == k16NBuf) ? 0 : buf + 1;
        }
    }
    __device__ __forceinline__ void prime() {
        issue_chunk(); issue_chunk(); issue_chunk();
    }
    IF_PHASE_TIMING(stamp_t t_wait[2] = {0, 0};)              // cycles in sync(): [0] the vmcnt wait, [1] the barrier
    template <bool STRICT> __device__ __forceinline__ void sync() {
        IF_PHASE_TIMING(stamp_t tc[2]; stamp_mark(tc, 0);)
        // STRICT (training: the epilogue's argument stores share vmcnt): wait for everything
        if (STRICT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        IF_PHASE_TIMING(stamp_mark(tc, 1);)
        __syncthreads();
        IF_PHASE_TIMING(t_wait[0] += tc[1] - tc[0]; stamp_add(t_wait, 1, tc[1]);)
    }
    __device__ __forceinline__ void advance() {
        use_buf = (use_buf + 1 == k16NBuf) ? 0 : use_buf + 1;
        wcur = wnxt;
        wnxt = wbuf + ((use_buf + 1 == k16NBuf) ? 0 : use_buf + 1) * k16ChunkFloats;
    }
};

// -DE3DGE_16_TRACE: s_memtime at the start of every k-step, after its MFMAs and after its epilogue slice, for one tile of two
// partner waves (stamps.h).  Inline asm, so no s_waitcnt is placed behind the stamps; they are collected after the tile.
#define TRACE16_STAMP(i) IF_16_TRACE(if (trace) STAMP_MEMTIME(tstamp[i]);)

// K = 256 contraction of one 16-feature tile: 8 k-steps x (hi*hi, lo*hi, hi*lo) on two alternating accumulators.
// On entry the ring holds k-steps 0..2 of this chunk; on exit k-steps 0..2 of the next one.
// `hook()` runs once, after k-step 1: the chunk wait + workgroup barrier + next DMA issue (and whatever else has to sit there;
// the inference renders issue the DMA from `epi`, in k-steps kDmaStep and kDmaStep + 1 -- see siren16_kernel).
template <bool TRANSPOSED, int RING = k16Ring, class Epi, class Hook>
__device__ __forceinline__ void tile16(ChunkPipe16& pipe, int lane, const u32x4 (&aH)[k16Steps], const u32x4 (&aL)[k16Steps],
                                       f32x4v& acc, f32x4v& accb, u32x4 (&ringH)[RING], u32x4 (&ringL)[RING], Epi&& epi,
                                       Hook&& hook, int sbuf = -1, [[maybe_unused]] int trace = 0) {
    IF_16_TRACE(stamp_t tstamp[24];)
    // sbuf >= 0: the caller knows the buffer index statically (tile index mod k16NBuf in a fully unrolled layer): the fragment
    // reads then are one base register + immediates instead of per-buffer address registers
    const u32x4* __restrict__ wp = reinterpret_cast<const u32x4*>(sbuf >= 0 ? pipe.wbuf + sbuf * k16ChunkFloats : pipe.wcur) + lane;
    const u32x4* __restrict__ wn = reinterpret_cast<const u32x4*>(sbuf >= 0 ? pipe.wbuf + ((sbuf + 1) % k16NBuf) * k16ChunkFloats : pipe.wnxt) + lane;
#pragma unroll
    for (int g = 0; g < k16Steps; ++g) {
        const int ga = g + RING - 1;
        TRACE16_STAMP(3 * g);
        ringH[ga % RING] = (ga < k16Steps) ? wp[(ga * 2 + 0) * 64] : wn[((ga - k16Steps) * 2 + 0) * 64];
        ringL[ga % RING] = (ga < k16Steps) ? wp[(ga * 2 + 1) * 64] : wn[((ga - k16Steps) * 2 + 1) * 64];
        __builtin_amdgcn_sched_barrier(0);
        const u32x4 wh = ringH[g % RING], wl = ringL[g % RING];
        f32x4v& x0 = (g & 1) ? accb : acc;
        f32x4v& x1 = (g & 1) ? acc : accb;
        if (!TRANSPOSED) {
            x0 = mfma16x16(wh, aH[g], x0);
            x1 = mfma16x16(wl, aH[g], x1);
            x0 = mfma16x16(wh, aL[g], x0);
        } else {
            x0 = mfma16x16(aH[g], wh, x0);
            x1 = mfma16x16(aH[g], wl, x1);
            x0 = mfma16x16(aL[g], wh, x0);
        }
        TRACE16_STAMP(3 * g + 1);
        if (g == 1) hook();
        epi(g);
        TRACE16_STAMP(3 * g + 2);
    }
    IF_16_TRACE(if (trace) stamps_flush<kStampWaitLgkm>((threadIdx.x & 63) == 0, 8 + trace - 1, tstamp, 24);)
}

#ifndef E3DGE_16_HELPERS_ONLY
// -DE3DGE_PHASE_TIMING: thread 0 of workgroup 0 marks the phase boundaries of its first three sub-tiles (stamps.h)
#define PHASE16(i) IF_PHASE_TIMING(if (MODE == 0 && blockIdx.x == 0 && tid == 0 && sub < 3) stamp_mark(tstamp, sub * 6 + (i));)

// CACHE (render mode without SAVE only): 1 = also write the backbone output (layer 7, packed hi / lo) to a.bb_out, one 16-KiB
// record per wave slab in register order; 2 = read it (and the composite weights a.weights_in) back instead of running layers
// 0..7, the sdf head, alpha and the transmittance scan: the second pass of an evaluated image differs from the first only
// behind the sdf head (texture FiLM -> view layer -> colour / feature compositing).  Geometry, launch shape and the point ->
// (workgroup, sub-tile, wave, lane) mapping are those of the launch that wrote the record.
constexpr int64_t k16SlabWords = 8 * 2 * 64;      // u32x4 per slab record: [g][hi | lo][lane]

template <int MODE, bool SAVE, int CACHE = 0>
__global__ void __launch_bounds__(k16Threads) siren16_kernel(const SirenK a) {
    static_assert(CACHE == 0 || (MODE == 0 && !SAVE), "the backbone hand-over exists for inference renders only");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const wbuf = smem + k16LdsW;
    float* const film_s = smem + k16LdsFilm;
    float* const head_s = smem + k16LdsHead;
    float* const w0_s = smem + k16LdsW0;
    float* const vrec_s = smem + k16LdsVrec;
    float* const feat_acc = smem + k16LdsFeat;
    float* const part = smem + k16LdsPart;
    float* const alpha_s = smem + k16LdsAlpha;
    float* const wgt_s = smem + k16LdsWgt;
    float* const z_s = smem + k16LdsZ;
    float* const pts_s = smem + k16LdsPts;
    float* const rgb_s = smem + k16LdsRgb;
    float* const state = smem + k16LdsState;

    const int tid_k = threadIdx.x;
    IF_PHASE_TIMING(stamp_t tstamp[24]; stamp_mark(tstamp, 20);)
    // ---- work assignment (as siren_kernel) ----
    int b, npts, n_sub;
    int pix0 = 0, nrays = 0;
    long long pt0 = 0;
    const int S = (MODE == 0) ? a.S : 1;
    if (MODE == 0) {
        b = blockIdx.x / a.tiles_per_img;
        const int tile = blockIdx.x - b * a.tiles_per_img;
        const int HW = a.H * a.Wd;
        pix0 = tile * a.R;
        nrays = min(a.R, HW - pix0);
        npts = nrays * S;
    } else {
        b = blockIdx.x / a.wgs_per_img;
        const int wg = blockIdx.x - b * a.wgs_per_img;
        pt0 = (long long)wg * a.subtiles_per_wg * kTilePts;
        const long long rem = a.n_pts - pt0;
        npts = (int)(rem < (long long)a.subtiles_per_wg * kTilePts ? rem : (long long)a.subtiles_per_wg * kTilePts);
    }
    n_sub = (npts + kTilePts - 1) / kTilePts;

    const float* __restrict__ packed = a.packed;
    const float* __restrict__ film_g = a.film + (int64_t)b * 9 * 2 * kWidth;
    // first weight chunks on their way (L2 -> LDS by DMA) while the tables below are built
    ChunkPipe16 pipe;
    if (CACHE == 2) pipe.init(wbuf, packed + kOffBig16b + (int64_t)(kBigLayers - 1) * k16Tiles * k16ChunkFloats, tid_k >> 6, tid_k & 63, k16Tiles);
    else pipe.init(wbuf, packed + kOffBig16b, tid_k >> 6, tid_k & 63);
    pipe.prime();
    // The tables: this thread's share of every global read is issued first, into registers, and only then written to the LDS --
    // one L2 round trip for the whole prologue instead of one per loop iteration (film_g was just written by another kernel,
    // possibly on another XCD).
    constexpr int kFilmIt = (9 * kWidth + k16Threads - 1) / k16Threads;
    constexpr int kHeadIt = (kHeadFloats + k16Threads - 1) / k16Threads;
    constexpr int kColIt = (3 * kWidth + k16Threads - 1) / k16Threads;
    float ld_gm[kFilmIt], ld_bt[kFilmIt], ld_bias[kFilmIt], ld_head[kHeadIt], ld_w0[kColIt], ld_vt[kColIt];
#pragma unroll
    for (int j = 0; j < kFilmIt; ++j) {
        const int i = tid_k + j * k16Threads, l = i >> 8, n = i & 255;
        ld_gm[j] = ld_bt[j] = ld_bias[j] = 0.0f;
        if (i < 9 * kWidth) {
            ld_gm[j] = film_g[(l * 2 + 0) * kWidth + n];
            ld_bt[j] = film_g[(l * 2 + 1) * kWidth + n];
            ld_bias[j] = packed[kOffBias + l * kWidth + n];
        }
    }
#pragma unroll
    for (int j = 0; j < kHeadIt; ++j) {
        const int i = tid_k + j * k16Threads;
        ld_head[j] = (i < kHeadFloats) ? packed[kOffWSigma + i] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < kColIt; ++j) {
        const int i = tid_k + j * k16Threads, c = i >> 8, n = i & 255;   // fragment images of layer 0 / the view tail: [t][m][lane], k = 2m + half
        const int src = ((n >> 5) * 2 + (c >> 1)) * 64 + (c & 1) * 32 + (n & 31);
        ld_w0[j] = ld_vt[j] = 0.0f;
        if (i < 3 * kWidth) { ld_w0[j] = packed[kOffFirst + src]; ld_vt[j] = packed[kOffVTail + src]; }
    }
    // FiLM block with the layer bias folded into the offset and the weights' factor 128 divided out of gamma (layers >= 1); the
    // view layer's (l = 8) values also go to its record
#pragma unroll
    for (int j = 0; j < kFilmIt; ++j) {
        const int i = tid_k + j * k16Threads, l = i >> 8, n = i & 255;
        if (i < 9 * kWidth) {
            const float gm = ld_gm[j], bt = ld_bt[j];
            const float g_s = (l >= 1) ? gm * (1.0f / kW16Scale) : gm;
            const float b_s = __fadd_rn(__fmul_rn(gm, ld_bias[j]), bt);
            film_s[(l * 2 + 0) * kWidth + n] = g_s;
            film_s[(l * 2 + 1) * kWidth + n] = b_s;
            if (l == 8) { vrec_s[4 * n + 0] = g_s; vrec_s[4 * n + 1] = b_s; }
        }
    }
#pragma unroll
    for (int j = 0; j < kHeadIt; ++j) {
        const int i = tid_k + j * k16Threads;
        if (i < kHeadFloats) {
            head_s[i] = ld_head[j];
            const int c = (i >> 8) - 1, n = i & 255;     // w_rgb[c][n] (head floats 256 .. 1023)
            if (c >= 0 && c < 3) vrec_s[(c == 2 ? 4 * kWidth : 0) + 4 * n + (c == 2 ? 0 : 2 + c)] = ld_head[j];
        }
    }
#pragma unroll
    for (int j = 0; j < kColIt; ++j) {
        const int i = tid_k + j * k16Threads, c = i >> 8, n = i & 255;
        if (i < 3 * kWidth) {
            w0_s[i] = ld_w0[j];
            vrec_s[4 * kWidth + 4 * n + 1 + c] = ld_vt[j] * kW16Scale;
        }
    }
    float cw[12] = {0}, focal = 1.f, nearv = 0.f, farv = 0.f;
    if (MODE == 0) {
#pragma unroll
        for (int i = 0; i < 12; ++i) cw[i] = a.c2w[b * 12 + i];
        focal = a.focal[b]; nearv = a.near[b]; farv = a.far[b];
        for (int i = tid_k; i < kRMax * kStateStride; i += k16Threads) state[i] = 0.0f;
        for (int i = tid_k; i < kRMax * kFPitch; i += k16Threads) feat_acc[i] = 0.0f;
    }
    const float* __restrict__ film = film_s;

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    u32x4 ringH[k16Ring], ringL[k16Ring];
    {
        const int lane0 = tid_k & 63;
#pragma unroll
        for (int g = 0; g < k16Ring - 1; ++g) {
            ringH[g] = reinterpret_cast<const u32x4*>(pipe.wcur)[(g * 2 + 0) * 64 + lane0];
            ringL[g] = reinterpret_cast<const u32x4*>(pipe.wcur)[(g * 2 + 1) * 64 + lane0];
        }
    }

    auto trace_sel = [&]([[maybe_unused]] int L, [[maybe_unused]] int t) {      // 1 / 2: tile16 records this tile for wave 0 / 4
        IF_16_TRACE(const int w = __builtin_amdgcn_readfirstlane(tid_k >> 6);
                    if (MODE == 0 && blockIdx.x == 7 && L == 3 && t == 6 && (w == 0 || w == 4)) return 1 + (w >> 2);)
        return 0;
    };
    // SAVE: the argument stores share the in-order memory queue with the weight DMA.  Until round 6 this hook drained the queue
    // (s_waitcnt vmcnt(0), and __syncthreads() adds the same for the compiler's own stores): every tile of the saving forward waited for
    // its previous tile's stores to reach L2 -- +40 % over the plain forward.  Now a counted wait (the chunk of tile t+1 was issued at
    // hook t-2; younger than it: `younger` guaranteed operations) and a barrier in asm, as in siren16_bwd.h.
    // Inference renders (MODE 0, no SAVE, every CACHE): the hook only waits; the two DMA pieces of the next chunk go out in k-steps
    // kDmaStep and kDmaStep + 1 of the same tile, one each.  Right behind the barrier all eight waves issued theirs at the same moment,
    // each in front of its own k-step-1 epilogue slice and with its partner's MFMAs waiting for the pipe.  Same chunks, same order, same
    // counted wait (the youngest two operations at a hook are still the previous tile's pieces).  Kernel time -2.6 % against the parent
    // (medians 0.28992 -> 0.28240 ms, profiles/r9_ab.txt visit 4); the other placements measured are in DESIGN.md 4.1c, round 9.  The
    // saving forward and the point query keep issue_chunk() in the hook: their hand-counted waits depend on where the pieces sit
    // between the argument stores.
    constexpr bool kSeamless = MODE == 0 && !SAVE;      // (also: the hidden layers run without a seam, below)
    constexpr bool kDmaInTile = kSeamless;              // every tile of these renders has an epilogue lambda, which calls dma_step()
    constexpr int kDmaStep = 3;
    auto dma_step = [&](int g) {
        if (kDmaInTile && g == kDmaStep) pipe.template issue_piece<0>();
        if (kDmaInTile && g == kDmaStep + 1) pipe.template issue_piece<1>();
    };
    auto fwd_hook = [&](int younger) {          // younger: compile-time constant at every call site; ignored without SAVE
        if (SAVE) {
            switch (younger) {
                case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
                case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
                default: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        } else {
            pipe.template sync<false>();
        }
        if (!kDmaInTile) pipe.issue_chunk();
    };
    // packed f16 (hi, lo) activations of this wave's 16 points: word 2e + (r >> 1), half r & 1 of in?[g] = feature 32g + 16e + 4q + r
    u32x4 inH[k16Steps], inL[k16Steps], outH[k16Steps], outL[k16Steps];
    // Inference renders (kSeamless, above) run the hidden layers without a seam: the layers alternate between the two arrays (no `in := out` copies) and
    // the last tile's epilogue of a layer runs inside the first tile of the next one, so the backbone output ends up in `out` when the
    // number of hidden layers is odd.  The saving forward and the point query keep the seam (epilogue behind the layer, copy back):
    // their counted waits depend on where the argument stores sit, and they are at the register limit when unrolled further.
    constexpr bool kFinalOut = kSeamless && ((E3DGE_SIREN_DEPTH - 1) & 1) != 0;
    u32x4 (&hH)[k16Steps] = kFinalOut ? outH : inH;       // layer 7's output: sdf head, layer-7 record, texture FiLM, view layer
    u32x4 (&hL)[k16Steps] = kFinalOut ? outL : inL;
    IF_PHASE_TIMING(for (int i = 0; i < 18; ++i) tstamp[i] = 0;
                    stamp_mark(tstamp, 21);)
    for (int sub = 0; sub < n_sub; ++sub) {
        int tid_o = tid_k;
        asm volatile("" : "+v"(tid_o));                    // opaque: address math stays inside the sub-tile (no hoisted registers)
        const int tid = tid_o, lane = tid & 63, wave = tid >> 6, q = lane >> 4, col = lane & 15;
        PHASE16(0);
        // =====================================================================================
        // 1. this lane's point (replicated over the four lane groups q)
        // =====================================================================================
        const int p_sub = 16 * wave + col;
        const int p = sub * kTilePts + p_sub;
        const bool valid = p < npts;
        const int pc = valid ? p : (npts - 1);
        float px = 0.f, py = 0.f, pz = 0.f, vx = 0.f, vy = 0.f, vz = 0.f, zval = 0.f, dist = 0.f;
        int ray_l = 0, s_idx = 0;
        int64_t gpt;
        if (MODE == 0) {
            ray_l = pc / S;
            s_idx = pc - ray_l * S;
            const int pix = pix0 + ray_l;
            const int iy = pix / a.Wd, ix = pix - iy * a.Wd;
            gpt = ((int64_t)b * a.H * a.Wd + pix) * S + s_idx;
            const float hres = (float)a.res * 0.5f;
            const float d0 = __fdiv_rn(((float)ix + 0.5f) - hres, focal);
            const float d1 = -__fdiv_rn(((float)iy + 0.5f) - hres, focal);
            const float d2 = -1.0f;
            float rd[3];
#pragma unroll
            for (int m = 0; m < 3; ++m)
                rd[m] = __fadd_rn(__fadd_rn(__fmul_rn(d0, cw[4 * m + 0]), __fmul_rn(d1, cw[4 * m + 1])), __fmul_rn(d2, cw[4 * m + 2]));
            const float dn = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2)));
            vx = __fdiv_rn(d0, dn); vy = __fdiv_rn(d1, dn); vz = __fdiv_rn(d2, dn);
            const float tv = a.t_vals[s_idx];
            zval = __fadd_rn(__fmul_rn(nearv, __fsub_rn(1.0f, tv)), __fmul_rn(farv, tv));
            px = __fadd_rn(cw[3], __fmul_rn(rd[0], zval));
            py = __fadd_rn(cw[7], __fmul_rn(rd[1], zval));
            pz = __fadd_rn(cw[11], __fmul_rn(rd[2], zval));
            const float rdn = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(rd[0], rd[0]), __fmul_rn(rd[1], rd[1])), __fmul_rn(rd[2], rd[2])));
            if (s_idx + 1 < S) {
                const float tn = a.t_vals[s_idx + 1];
                const float zn = __fadd_rn(__fmul_rn(nearv, __fsub_rn(1.0f, tn)), __fmul_rn(farv, tn));
                dist = __fmul_rn(__fsub_rn(zn, zval), rdn);
            } else {
                dist = __fmul_rn(1e10f, rdn);
            }
            if (valid && q == 0) {
                if (a.points) { float* o = a.points + gpt * 3; o[0] = px; o[1] = py; o[2] = pz; }
                if (a.dists) a.dists[gpt] = dist;
                if (s_idx == 0) {
                    const int64_t gr = (int64_t)b * a.H * a.Wd + pix;
                    if (a.rays_d) { float* o = a.rays_d + gr * 3; o[0] = rd[0]; o[1] = rd[1]; o[2] = rd[2]; }
                    if (a.viewdirs) { float* o = a.viewdirs + gr * 3; o[0] = vx; o[1] = vy; o[2] = vz; }
                }
            }
        } else {
            gpt = (int64_t)b * a.n_pts + pt0 + pc;
            const float* pp = a.pts + gpt * 3;
            px = pp[0]; py = pp[1]; pz = pp[2];
            if (a.vdirs) { const float* vv = a.vdirs + gpt * 3; vx = vv[0]; vy = vv[1]; vz = vv[2]; }
        }
        const int64_t gpt_block = (MODE == 0) ? ((int64_t)b * a.H * a.Wd + pix0) * S : (int64_t)b * a.n_pts + pt0;
        // Saved arguments: every lane stores -- rows beyond the tensor are exact clones of the last valid point (same position, same
        // arithmetic, the same values to the same address), so the store count per tile does not depend on the data (counted waits).
        const bool sblk = SAVE && a.save_blocked != 0;
        const int64_t img_n = (MODE == 0) ? (int64_t)a.H * a.Wd * S : (int64_t)a.n_pts;
        const int64_t srow_block = (int64_t)b * saved_rows_per_image(sblk, img_n) + ((MODE == 0) ? (int64_t)pix0 * S : pt0);    // padded row of the block's first point
        float* const sv = SAVE ? a.save_args + saved_row_floats(sblk, srow_block + pc, q, 9) : nullptr;
        const int sv_ls = sblk ? kSlabLayerF : kWidth, sv_ts = sblk ? kSlabTileF : 16;
        // the view layer (features on lanes) needs the directions of the points 4q + r: through LDS
        float* const vd_s = smem + k16LdsVd + wave * 64;
        if (q == 0) { vd_s[col * 4 + 0] = vx; vd_s[col * 4 + 1] = vy; vd_s[col * 4 + 2] = vz; }

        // =====================================================================================
        // 2. layer 0 (3 -> 256) in the VALU: every lane its 4 features of each tile
        // =====================================================================================
        f32x4v prev = zero4();        // a tile's four accumulator sums, until its epilogue has run (seamless: also over a layer boundary)
        if (CACHE != 2) {
            const float xs = __fmul_rn(px, a.box_scale), ys = __fmul_rn(py, a.box_scale), zs = __fmul_rn(pz, a.box_scale);
#pragma unroll
            for (int t = 0; t < k16Tiles; ++t) {
                const int o = 16 * t + 4 * q;
                const f32x4v wx = *reinterpret_cast<const f32x4v*>(w0_s + o), wy = *reinterpret_cast<const f32x4v*>(w0_s + kWidth + o),
                             wz = *reinterpret_cast<const f32x4v*>(w0_s + 2 * kWidth + o);
                f32x4v lin;
#pragma unroll
                for (int r = 0; r < 4; ++r) lin[r] = fmaf(wz[r], zs, fmaf(wy[r], ys, wx[r] * xs));
                if (kSeamless && t == k16Tiles - 1) {      // the last tile's FiLM + sine run inside layer 1's first tile, like every layer's
                    prev = lin;
                } else {
                    const f32x4v g4 = *reinterpret_cast<const f32x4v*>(film + o), b4 = *reinterpret_cast<const f32x4v*>(film + kWidth + o);
                    f32x4v arg, v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        arg[r] = fmaf(g4[r], lin[r], b4[r]);
                        v[r] = sin_f32(arg[r]);
                    }
                    if (SAVE) save_st4(sv + t * sv_ts, arg);
                    SPLIT2_TO(v[0], v[1], inH[t >> 1][2 * (t & 1)], inL[t >> 1][2 * (t & 1)]);
                    SPLIT2_TO(v[2], v[3], inH[t >> 1][2 * (t & 1) + 1], inL[t >> 1][2 * (t & 1) + 1]);
                }
            }
        }

        PHASE16(1);
        // =====================================================================================
        // 3. layers 1..7: 112 tiles; the FiLM + sine epilogue of tile t-1 issues inside tile t's MFMA stream
        // =====================================================================================
        // (A role split of the two waves of a SIMD -- GEMM segment / epilogue segment in opposite phases, two barriers per tile -- was
        // built and measured 5 % slower; the code is in the history at da20f64.)
        // whole epilogue of tile tp of layer L at once, FiLM row `fl` (where no following tile is there to carry it)
        auto finish = [&](const float* __restrict__ fl, int L, int tp, const f32x4v& pv, auto& dH, auto& dL) {
            const int o = 16 * tp + 4 * q;
            const f32x4v g4 = *reinterpret_cast<const f32x4v*>(fl + o), b4 = *reinterpret_cast<const f32x4v*>(fl + kWidth + o);
            f32x4v arg, v;
#pragma unroll
            for (int r = 0; r < 4; ++r) { arg[r] = fmaf(g4[r], pv[r], b4[r]); v[r] = sin_f32(arg[r]); }
            if (SAVE) save_st4(sv + L * sv_ls + tp * sv_ts, arg);
            SPLIT2_TO(v[0], v[1], dH[tp >> 1][2 * (tp & 1)], dL[tp >> 1][2 * (tp & 1)]);
            SPLIT2_TO(v[2], v[3], dH[tp >> 1][2 * (tp & 1) + 1], dL[tp >> 1][2 * (tp & 1) + 1]);
        };
        // Layer L from (sH, sL) into (dH, dL).  Seamless: tile 0 carries the epilogue of the PREVIOUS layer's last tile -- `prev` and the
        // FiLM row of layer L-1, into words 2, 3 of s?[7], which only k-step 7 reads and stage 4 has written by then -- and the layer
        // leaves its own last tile in `prev`.  One base register for both FiLM rows: the reads are ds_read_b128 base offset:imm.
        auto hidden_layer = [&](int L, auto& sH, auto& sL, auto& dH, auto& dL) {
            const float* __restrict__ film_p = film + (L - 1) * 2 * kWidth;
#pragma unroll
            for (int t = 0; t < k16Tiles; ++t) {
                f32x4v acc = zero4(), accb = zero4();
                static_assert(!kDmaInTile || kSeamless, "a tile without an epilogue lambda issues its chunk in the hook only");
                if (t == 0 && !kSeamless) {
                    tile16<false>(pipe, lane, sH, sL, acc, accb, ringH, ringL, [](int) {}, [&]() { fwd_hook(2); }, t % k16NBuf);
                } else {
                    const int tp = (t == 0) ? k16Tiles - 1 : t - 1;
                    const int o = ((t == 0) ? 0 : 2 * kWidth) + 16 * tp + 4 * q;
                    auto& eH = (t == 0) ? sH : dH;
                    auto& eL = (t == 0) ? sL : dL;
                    f32x4v g4 = zero4(), b4 = zero4(), arg4 = zero4(), kf4 = zero4(), x4 = zero4();
                    tile16<false>(pipe, lane, sH, sL, acc, accb, ringH, ringL, [&](int g) {
                        // the FiLM + sine + split of tile tp's four values, staged over the k-steps with the four values side by
                        // side: every slice is four independent instructions deep instead of one dependent chain (a lone chain
                        // leaves the wave -- in order -- waiting on VALU latency with nothing else to issue)
                        dma_step(g);
                        if (g == 0) {
                            g4 = *reinterpret_cast<const f32x4v*>(film_p + o);
                            b4 = *reinterpret_cast<const f32x4v*>(film_p + kWidth + o);
                        } else if (g == 1) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) arg4[r] = fmaf(g4[r], prev[r], b4[r]);
#ifndef E3DGE_POLY_SINE      // sin_hw_f32 (siren_common.h) in stages: period index, reduced argument in revolutions, v_sin
#pragma unroll
                            for (int r = 0; r < 4; ++r) kf4[r] = rintf(arg4[r] * 0.15915494f);
                        } else if (g == 2) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) kf4[r] = fmaf(arg4[r], 6.4206382e-09f, fmaf(arg4[r], 0.15915494f, -kf4[r]));
#endif
                        } else if (g == 3) {
#pragma unroll
#ifndef E3DGE_POLY_SINE
                            for (int r = 0; r < 4; ++r) x4[r] = __builtin_amdgcn_sinf(kf4[r]);
#else
                            for (int r = 0; r < 4; ++r) x4[r] = sin_poly_f32(arg4[r]);
#endif
                            if (SAVE) save_st4(sv + L * sv_ls + tp * sv_ts, arg4);
                        } else if (g == 4) {
                            SPLIT2_TO(x4[0], x4[1], eH[tp >> 1][2 * (tp & 1)], eL[tp >> 1][2 * (tp & 1)]);
                            SPLIT2_TO(x4[2], x4[3], eH[tp >> 1][2 * (tp & 1) + 1], eL[tp >> 1][2 * (tp & 1) + 1]);
                        }
                    // (guaranteed operations younger than chunk t+1: the two pieces of hook t-1 and the stores of tiles t-3, t-2 -- none
                    // guaranteed in front of a layer's first tiles: the view layer's stores are predicated)
                    }, [&]() { fwd_hook(t < 2 ? 2 : (t == 2 ? 3 : 4)); }, t % k16NBuf, trace_sel(L, t));
                }
                pipe.advance();
                prev = acc + accb;
            }
        };
        if constexpr (kSeamless) {
            if (CACHE != 2) {
                // two layer bodies, in -> out and out -> in, in one loop (not one body per layer: the pair is the hot set of the
                // instruction cache)
#pragma unroll 1
                for (int L = 1; L < E3DGE_SIREN_DEPTH; L += 2) {
                    hidden_layer(L, inH, inL, outH, outL);
                    if (L + 1 >= E3DGE_SIREN_DEPTH) break;
                    hidden_layer(L + 1, outH, outL, inH, inL);
                }
                // the sdf head needs all of layer 7: its last tile's epilogue stays exposed, once per sub-tile
                finish(film + (E3DGE_SIREN_DEPTH - 1) * 2 * kWidth, E3DGE_SIREN_DEPTH - 1, k16Tiles - 1, prev, hH, hL);
            }
        } else {
#pragma unroll 1
            for (int L = 1; L < E3DGE_SIREN_DEPTH; ++L) {
                hidden_layer(L, inH, inL, outH, outL);
                finish(film + L * 2 * kWidth, L, k16Tiles - 1, prev, outH, outL);
#pragma unroll
                for (int g = 0; g < k16Steps; ++g) { inH[g] = outH[g]; inL[g] = outL[g]; }
            }
        }

        if (CACHE != 0) {
            const int64_t rec = (((int64_t)blockIdx.x * a.bb_subs + sub) * 8 + wave) * k16SlabWords + lane;
            if (CACHE == 1) {
                u32x4* __restrict__ dst = reinterpret_cast<u32x4*>(a.bb_out) + rec;
#pragma unroll
                for (int g = 0; g < k16Steps; ++g) { dst[(g * 2 + 0) * 64] = hH[g]; dst[(g * 2 + 1) * 64] = hL[g]; }
            } else {
                const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(a.bb_in) + rec;
#pragma unroll
                for (int g = 0; g < k16Steps; ++g) { hH[g] = src[(g * 2 + 0) * 64]; hL[g] = src[(g * 2 + 1) * 64]; }
            }
        }

        PHASE16(2);
        // =====================================================================================
        // 4. sdf head on the backbone output (features on registers): 64 features per lane, then over the 4 lane groups
        // =====================================================================================
        float sdf = 0.0f;
        if (CACHE == 2) {
            if (q == 0) wgt_s[p_sub] = valid ? a.weights_in[gpt] : 0.0f;      // (read back by this wave's own lanes and, after the
        } else {                                                                //  barrier behind rgb_s, by the compositing threads)
            float acc = 0.0f;
#pragma unroll
            for (int t = 0; t < k16Tiles; ++t) {
                const f32x4v w4 = *reinterpret_cast<const f32x4v*>(head_s + 16 * t + 4 * q);
                const int g = t >> 1, w0i = 2 * (t & 1);
                acc = fma_mix_h<0>(hH[g][w0i], w4[0], acc); acc = fma_mix_h<0>(hL[g][w0i], w4[0], acc);
                acc = fma_mix_h<1>(hH[g][w0i], w4[1], acc); acc = fma_mix_h<1>(hL[g][w0i], w4[1], acc);
                acc = fma_mix_h<0>(hH[g][w0i + 1], w4[2], acc); acc = fma_mix_h<0>(hL[g][w0i + 1], w4[2], acc);
                acc = fma_mix_h<1>(hH[g][w0i + 1], w4[3], acc); acc = fma_mix_h<1>(hL[g][w0i + 1], w4[3], acc);
            }
            sdf = sum_over_q(acc) + head_s[4 * kWidth];
        }

        if (MODE == 0 && CACHE != 2) {
            const float sg = __fdiv_rn(sigmoid_f32(__fdiv_rn(-sdf, a.sigmoid_beta)), a.sigmoid_beta);
            const float alpha = __fsub_rn(1.0f, expf(-__fmul_rn(sg, dist)));
            if (q == 0) {
                alpha_s[p_sub] = valid ? alpha : 0.0f;
                z_s[p_sub] = zval;
                pts_s[p_sub * 3 + 0] = px; pts_s[p_sub * 3 + 1] = py; pts_s[p_sub * 3 + 2] = pz;
                if (valid && a.sdf) a.sdf[gpt] = sdf;
            }
            __syncthreads();
            // transmittance scan (:869-886) as a wavefront prefix product: a wave per ray touching this sub-tile, a lane per sample
            // (64 at a time, front to back): T_s = T_in * prod_{j < s} (1 - alpha_j + 1e-10) from one inclusive DPP scan shifted by a
            // lane, the weight sum in front of the last sample and the weighted depth / position sums as DPP reductions.
            // (Same terms as the reference's cumprod / sum; the association order is the scan tree's.)
            const int sub_lo = sub * kTilePts;
            const int sub_hi = min(sub_lo + kTilePts, npts);
            const int r_first = sub_lo / S, r_last = (sub_hi - 1) / S;
            for (int i = __builtin_amdgcn_readfirstlane(wave); i <= r_last - r_first; i += 8) {
                const int rl = r_first + i;
                const int s_lo = max(0, sub_lo - rl * S), s_hi = min(S, sub_hi - rl * S);
                float* st = state + rl * kStateStride;
                float T_in = (s_lo == 0) ? 1.0f : st[0];
                float wsum = (s_lo == 0) ? 0.0f : st[1];
                float dep = 0.0f, x0 = 0.0f, x1 = 0.0f, x2 = 0.0f;
                for (int c0 = s_lo; c0 < s_hi; c0 += 64) {
                    const int s = c0 + lane;
                    const bool act = s < s_hi;
                    const int ps = rl * S + min(s, s_hi - 1) - sub_lo;
                    const float al = act ? alpha_s[ps] : 0.0f;
                    const float zz = z_s[ps], p0 = pts_s[ps * 3 + 0], p1 = pts_s[ps * 3 + 1], p2 = pts_s[ps * 3 + 2];
                    const float incl = wave_incl_prod(act ? __fadd_rn(__fsub_rn(1.0f, al), 1e-10f) : 1.0f);
                    const float T = __fmul_rn(T_in, dpp_or<0x138, 0xf>(1.0f, incl));
                    float w = __fmul_rn(al, T);
                    const bool last = a.force_bg && act && s == S - 1;
                    const float wfront = wave_sum_last(last ? 0.0f : w);
                    if (last) w = __fsub_rn(1.0f, __fadd_rn(wsum, wfront));
                    wsum = __fadd_rn(wsum, wfront);
                    if (act) wgt_s[ps] = w;
                    dep = __fadd_rn(dep, wave_sum_last(__fmul_rn(w, zz)));
                    x0 = __fadd_rn(x0, wave_sum_last(__fmul_rn(w, p0)));
                    x1 = __fadd_rn(x1, wave_sum_last(__fmul_rn(w, p1)));
                    x2 = __fadd_rn(x2, wave_sum_last(__fmul_rn(w, p2)));
                    T_in = __fmul_rn(T_in, __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, incl), 63)));
                }
                if (lane == 0) {
                    st[0] = T_in; st[1] = wsum;
                    st[2] = __fadd_rn(st[2], dep); st[3] = __fadd_rn(st[3], x0); st[4] = __fadd_rn(st[4], x1); st[5] = __fadd_rn(st[5], x2);
                }
            }
            __syncthreads();
            if (valid && q == 0 && a.weights) a.weights[gpt] = wgt_s[p_sub];
        }

        // optional per-point texture FiLM (:217-220), after the sdf head read h
        if (MODE == 0 && a.tex_alpha) {
            const float* __restrict__ ta = a.tex_alpha + gpt * kWidth;
            const float* __restrict__ tb = a.tex_beta + gpt * kWidth;
#pragma unroll
            for (int t = 0; t < k16Tiles; ++t) {
                const f32x4v a4 = *reinterpret_cast<const f32x4v*>(ta + 16 * t + 4 * q);
                const f32x4v b4 = *reinterpret_cast<const f32x4v*>(tb + 16 * t + 4 * q);
                float y[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = __fadd_rn(__fmul_rn(__fadd_rn(a4[r], 1.0f), act16_get(hH, hL, t, r)), b4[r]);
                SPLIT2_TO(y[0], y[1], hH[t >> 1][2 * (t & 1)], hL[t >> 1][2 * (t & 1)]);
                SPLIT2_TO(y[2], y[3], hH[t >> 1][2 * (t & 1) + 1], hL[t >> 1][2 * (t & 1) + 1]);
            }
        }

        PHASE16(3);
        // =====================================================================================
        // 5. view layer (259 -> 256), TRANSPOSED: D[point 4q + r][feature 16t + col]
        // =====================================================================================
        float* const wq_s = smem + k16LdsWq + wave * (k16Slots * 16);
        int slab_first_ray = 0, slab_nslots = 0;
        const int slab_p0 = sub * kTilePts + 16 * wave;
        if (MODE == 0) {
            const int slab_hi = min(slab_p0 + 16, npts);
            if (slab_hi > slab_p0) {
                slab_first_ray = slab_p0 / S;
                slab_nslots = (slab_hi - 1) / S - slab_first_ray + 1;
            }
            const int b1 = (slab_first_ray + 1) * S - slab_p0;
            if (lane < 16) {                               // row = lane: composite weight of that point, by the ray it belongs to
                const float w = (slab_p0 + lane < npts) ? wgt_s[16 * wave + lane] : 0.0f;
                wq_s[lane] = (lane < b1) ? w : 0.0f;
                wq_s[16 + lane] = (lane >= b1) ? w : 0.0f;
            }
        }
        // (vd_s and wq_s were written by this wave's own lanes: no workgroup barrier needed, only the LDS ordering of a wave)
        const f32x4v q0 = (MODE == 0) ? *reinterpret_cast<const f32x4v*>(wq_s + 4 * q) : zero4();
        const f32x4v q1 = (MODE == 0) ? *reinterpret_cast<const f32x4v*>(wq_s + 16 + 4 * q) : zero4();
        float dvx[4], dvy[4], dvz[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { dvx[r] = vd_s[(4 * q + r) * 4 + 0]; dvy[r] = vd_s[(4 * q + r) * 4 + 1]; dvz[r] = vd_s[(4 * q + r) * 4 + 2]; }
        float prgb[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) prgb[c][r] = 0.0f;
        {
            // The 16 tiles unrolled (static LDS buffer t % k16NBuf, as in layers 1..7).  Tile t's epilogue -- view-direction columns,
            // FiLM, sine, rgb / feature partials -- runs staged over the k-steps of tile t+1, the four values of a lane side by side;
            // every operation, and the order of every accumulation, is that of the one-value-at-a-time form.
            const f32x4v* __restrict__ vra = reinterpret_cast<const f32x4v*>(vrec_s) + col;               // (gamma, beta, w_r, w_g)
            const f32x4v* __restrict__ vrb = reinterpret_cast<const f32x4v*>(vrec_s + 4 * kWidth) + col;  // (w_b, columns x, y, z)
            f32x4v ra = zero4(), rb = zero4(), pacc = zero4(), paccb = zero4(), pv = zero4(), varg = zero4(), kf = zero4(), hv = zero4();
            float fa0 = 0.f, fa1 = 0.f;
            auto epi = [&](int tp, int g) {          // stage g of tile tp's epilogue (record of tile tp in ra / rb)
                const int e_n = 16 * tp + col;
                if (g == 0) {
                    const f32x4v s4 = pacc + paccb;
                    // view-direction columns (fp32, already x128 like the streamed weights)
#pragma unroll
                    for (int r = 0; r < 4; ++r) pv[r] = fmaf(rb[3], dvz[r], fmaf(rb[2], dvy[r], fmaf(rb[1], dvx[r], s4[r])));
                } else if (g == 1) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) varg[r] = fmaf(ra[0], pv[r], ra[1]);
#ifndef E3DGE_POLY_SINE      // sin_hw_f32 in stages, as in layers 1..7
#pragma unroll
                    for (int r = 0; r < 4; ++r) kf[r] = rintf(varg[r] * 0.15915494f);
                } else if (g == 2) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) kf[r] = fmaf(varg[r], 6.4206382e-09f, fmaf(varg[r], 0.15915494f, -kf[r]));
#pragma unroll
                    for (int r = 0; r < 4; ++r) hv[r] = __builtin_amdgcn_sinf(kf[r]);
#else
                } else if (g == 2) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) hv[r] = sin_poly_f32(varg[r]);
#endif
                } else if (g == 3) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int pr = slab_p0 + 4 * q + r;
                        if (SAVE && pr < npts) a.save_args[saved_elem_floats(sblk, srow_block + pr, 8, e_n, 9)] = varg[r];
                        if (MODE != 0 && a.raw && pr < npts) a.raw[((int64_t)b * a.n_pts + pt0 + pr) * 260 + 4 + e_n] = hv[r];
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        prgb[0][r] = fmaf(ra[2], hv[r], prgb[0][r]);
                        prgb[1][r] = fmaf(ra[3], hv[r], prgb[1][r]);
                        prgb[2][r] = fmaf(rb[0], hv[r], prgb[2][r]);
                    }
                } else if (g == 4) {
                    if (MODE == 0) {
                        fa0 = fa1 = 0.f;
#pragma unroll
                        for (int r = 0; r < 4; ++r) { fa0 = fmaf(q0[r], hv[r], fa0); fa1 = fmaf(q1[r], hv[r], fa1); }
                    }
                } else if (g == 5) {
                    if (MODE == 0) {
                        fa0 = sum_over_q(fa0);
                        fa1 = sum_over_q(fa1);
                        if (q == 0) {
                            float* pp = part + (wave * k16Slots) * kWidth + e_n;
                            if (slab_nslots > 0) pp[0] = fa0;
                            if (slab_nslots > 1) pp[kWidth] = fa1;
                        }
                    }
                }
            };
            auto load_rec = [&](int t) { ra = vra[16 * t]; rb = vrb[16 * t]; };     // after stage 3: the last use of the previous record
            auto view_tile = [&](int t, int sbuf) {
                f32x4v acc = zero4(), accb = zero4();
                tile16<true>(pipe, lane, hH, hL, acc, accb, ringH, ringL, [&](int g) {
                    if (t > 0 && g <= 5) epi(t - 1, g);
                    if (g == 4) load_rec(t);
                    dma_step(g);
                }, [&]() { fwd_hook(2); }, sbuf);
                pipe.advance();
                pacc = acc; paccb = accb;
            };
            if constexpr (MODE == 0 && !SAVE) {
#pragma unroll
                for (int t = 0; t < k16Tiles; ++t) view_tile(t, t % k16NBuf);
            } else {      // (unrolled, the per-tile store addresses of the saved arguments / raw outputs push these past 256 VGPRs)
#pragma unroll 1
                for (int t = 0; t < k16Tiles; ++t) view_tile(t, -1);
            }
#pragma unroll
            for (int g = 0; g <= 5; ++g) epi(k16Tiles - 1, g);
        }

        PHASE16(4);
        // =====================================================================================
        // 6. rgb head: sum the per-lane partials over the 16 feature lanes of each lane group (DPP row rotations)
        // =====================================================================================
        float rgbv[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) rgbv[c][r] = row_sum16(prgb[c][r]) + head_s[4 * kWidth + 1 + c];
        if (MODE == 0) {
            if (col == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ps = 16 * wave + 4 * q + r;
                    rgb_s[ps * 3 + 0] = sigmoid_f32(rgbv[0][r]);
                    rgb_s[ps * 3 + 1] = sigmoid_f32(rgbv[1][r]);
                    rgb_s[ps * 3 + 2] = sigmoid_f32(rgbv[2][r]);
                }
            }
            __syncthreads();
            const int sub_lo = sub * kTilePts;
            const int sub_hi = min(sub_lo + kTilePts, npts);
            const int r_first = sub_lo / S, r_last = (sub_hi - 1) / S;
            for (int i = __builtin_amdgcn_readfirstlane(wave); i <= r_last - r_first; i += 8) {   // a wave per ray, a lane per sample
                const int rl = r_first + i;
                const int s_lo = max(0, sub_lo - rl * S), s_hi = min(S, sub_hi - rl * S);
                float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
                for (int b0 = s_lo; b0 < s_hi; b0 += 64) {
                    const int s = b0 + lane;
                    const int ps = rl * S + min(s, s_hi - 1) - sub_lo;
                    const float ww = (s < s_hi) ? wgt_s[ps] : 0.0f;
                    c0 = __fadd_rn(c0, wave_sum_last(__fmul_rn(ww, rgb_s[ps * 3 + 0])));
                    c1 = __fadd_rn(c1, wave_sum_last(__fmul_rn(ww, rgb_s[ps * 3 + 1])));
                    c2 = __fadd_rn(c2, wave_sum_last(__fmul_rn(ww, rgb_s[ps * 3 + 2])));
                }
                if (lane == 0) {
                    float* st = state + rl * kStateStride;
                    st[6] = __fadd_rn(st[6], c0); st[7] = __fadd_rn(st[7], c1); st[8] = __fadd_rn(st[8], c2);
                }
            }
            if (tid < kWidth) {   // ordered merge of the feature partials: slab by slab, ray slot by ray slot
                const int n = tid;
                float pv[8 * k16Slots];                      // (all sixteen loads in flight at once; unused slots are never added)
#pragma unroll
                for (int j = 0; j < 8 * k16Slots; ++j) pv[j] = part[j * kWidth + n];
                int cur = -1;
                float run = 0.0f;
#pragma unroll
                for (int wv = 0; wv < 8; ++wv) {
                    const int slab_lo = sub_lo + 16 * wv;
                    const int slab_hi2 = min(slab_lo + 16, npts);
                    if (slab_hi2 > slab_lo) {
                        const int fr = slab_lo / S;
                        const int ns = (slab_hi2 - 1) / S - fr + 1;
#pragma unroll
                        for (int sl = 0; sl < k16Slots; ++sl)
                            if (sl < ns) {
                                if (fr + sl != cur) {
                                    if (cur >= 0) feat_acc[cur * kFPitch + n] += run;
                                    cur = fr + sl;
                                    run = 0.0f;
                                }
                                run += pv[wv * k16Slots + sl];
                            }
                    }
                }
                if (cur >= 0) feat_acc[cur * kFPitch + n] += run;
            }
            __syncthreads();
        } else {
            if (a.raw && col == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int pr = sub * kTilePts + 16 * wave + 4 * q + r;
                    if (pr < npts) {
                        float* o = a.raw + ((int64_t)b * a.n_pts + pt0 + pr) * 260;
                        o[0] = rgbv[0][r]; o[1] = rgbv[1][r]; o[2] = rgbv[2][r];
                    }
                }
            }
            if (valid && q == 0) {
                if (a.sdf) a.sdf[gpt] = sdf;
                if (a.raw) a.raw[gpt * 260 + 3] = sdf;
            }
        }
        PHASE16(5);
    }  // sub-tiles

    IF_PHASE_TIMING(stamp_mark(tstamp, 22);)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // no LDS-DMA in flight when the workgroup retires
    if (MODE == 0) {
        // 7. per-ray outputs, channel-first like VolumeFeatureRenderer.forward returns them (:1957-1968)
        const int tid = tid_k;
        const int HW = a.H * a.Wd;
        if (a.features) {
            float* fo = a.features + (int64_t)b * kWidth * HW + pix0;
            for (int e = tid; e < nrays * kWidth; e += k16Threads) {
                const int n = e / nrays, rl = e - n * nrays;
                fo[(int64_t)n * HW + rl] = feat_acc[rl * kFPitch + n];
            }
        }
        for (int rl = tid; rl < nrays; rl += k16Threads) {
            const float* st = state + rl * kStateStride;
            const int pix = pix0 + rl;
            if (a.rgb) {
                float* o = a.rgb + (int64_t)b * 3 * HW + pix;
                o[0] = __fadd_rn(-1.0f, __fmul_rn(2.0f, st[6]));
                o[HW] = __fadd_rn(-1.0f, __fmul_rn(2.0f, st[7]));
                o[2 * HW] = __fadd_rn(-1.0f, __fmul_rn(2.0f, st[8]));
            }
            if (a.xyz) {
                float* o = a.xyz + (int64_t)b * 3 * HW + pix;
                o[0] = st[3]; o[HW] = st[4]; o[2 * HW] = st[5];
            }
            if (a.depth) a.depth[(int64_t)b * HW + pix] = st[2];
            if (a.mask) a.mask[(int64_t)b * HW + pix] = (st[2] < a.mask_thresh) ? 1.0f : 0.0f;
        }
        IF_PHASE_TIMING(tstamp[18] = pipe.t_wait[0]; tstamp[19] = pipe.t_wait[1];
                        __syncthreads();
                        stamp_mark(tstamp, 23);                 // per-ray outputs: up to this thread's last store
                        stamps_flush(blockIdx.x == 0 && tid == 0, 0, tstamp, 24);)
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Layout self-test of v_mfma_f32_16x16x32_f16 with the conventions above: c (16x16, row-major) = hi(a) hi(b)^T
__global__ void __launch_bounds__(64)
selftest_mfma16x16_kernel(float* __restrict__ cmat, const float* __restrict__ amat, const float* __restrict__ bmat, int k) {
    const int lane = threadIdx.x, q = lane >> 4, n = lane & 15;
    f32x4v acc = zero4();
    for (int kb = 0; kb < k; kb += 32) {
        u32x4 a4, b4, dummy;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            SPLIT2_TO(amat[n * k + kb + 8 * q + 2 * w], amat[n * k + kb + 8 * q + 2 * w + 1], a4[w], dummy[w]);
            SPLIT2_TO(bmat[n * k + kb + 8 * q + 2 * w], bmat[n * k + kb + 8 * q + 2 * w + 1], b4[w], dummy[w]);
        }
        acc = mfma16x16(a4, b4, acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) cmat[(4 * q + r) * 16 + n] = acc[r];
}

#endif  // E3DGE_16_HELPERS_ONLY

}  // namespace e3dge
