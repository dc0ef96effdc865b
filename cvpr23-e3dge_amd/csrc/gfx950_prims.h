// gfx950 building blocks that no kernel owns: LDS addresses and LDS-DMA pieces, the weight-chunk pipeline, the per-point power-of-two
// block scale, wave reductions and DPP moves, the XCD-contiguous tile order.  One form of each; nothing here knows about a network.
#pragma once
#include "common.h"
#include "stamps.h"

namespace e3dge {

// LDS byte address of a pointer into (dynamic) shared memory
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return (uint32_t)(size_t)(__attribute__((address_space(3))) const unsigned char*)p;
}

// LDS-DMA (global_load_lds_dwordx4: 16 B per lane straight into LDS, wave-uniform LDS base in M0).  The instruction's
// immediate offset is added to BOTH the global and the LDS address (validated on gfx950), so with the chunk image laid
// out identically on both sides the pieces of a chunk differ only in that immediate.
// Addressing: scalar 64-bit base + per-lane 32-bit byte offset + immediate.  hipcc never selects this mode for
// __builtin_amdgcn_global_load_lds (it builds a 64-bit VGPR address per piece: ~10 instructions and two VGPRs each
// time); written out, a piece is s_mov m0 / s_nop / global_load_lds.  No other code in these kernels uses M0.  The
// compiler does not count these in vmcnt; every consumer waits with an explicit s_waitcnt vmcnt.
template <int OFF_BYTES>
__device__ __forceinline__ void glds16_saddr(const void* sbase, uint32_t voff, uint32_t lds_dst) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 offset:%3"
                 :: "v"(voff), "s"(sbase), "s"(lds_dst), "n"(OFF_BYTES) : "memory");
}
__device__ __forceinline__ const void* uniform_ptr(const void* p) {       // make wave-uniformity explicit for an SGPR operand
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    return reinterpret_cast<const void*>(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
                                         (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v));
}
// one LDS-DMA piece (64 lanes x 16 B -> 1 KiB of LDS at lds_dst), global address = wave-uniform base + per-lane byte offset
__device__ __forceinline__ void dma_piece(const void* sbase, uint32_t voff, uint32_t lds_dst) {
    glds16_saddr<0>(uniform_ptr(sbase), voff, (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_dst));
}

// The weight-chunk pipeline of the 4-wave kernels: chunks of CHUNK_FLOATS floats of a fragment image stream L2 -> LDS through NBUF
// buffers; chunk c lives in buffer c % NBUF, wave w copies bytes [w, w + 1) * PIECES KiB of it in PIECES 1-KiB LDS-DMA pieces
// (16 B per lane), handed out one at a time inside the tile that runs NBUF - 1 chunks ahead of the chunk's first read.
// sync() runs early in the tile of chunk c.  Every wave waits until ITS pieces of chunk c+1 have landed: completion is in order
// and the chunks younger than c+1 that have been issued are c+2 .. c+NBUF-2, so the wait is vmcnt(WAIT) with WAIT = PIECES *
// (NBUF - 3) pieces that may stay outstanding (NBUF = 3: nothing younger exists, WAIT = 0).  A count is a lower bound of the
// operations younger than the awaited one: loads or stores a kernel puts into the queue besides the pieces only make the wait
// stricter, never laxer.  The barrier then publishes chunk c+1 and proves that everybody has left chunk c-1, whose buffer the DMA
// of chunk c + NBUF - 1 may now overwrite.  Chunk indices wrap inside [first, first + count): the chunks fetched past the end of
// the work land in buffers nobody reads (kernels end with vmcnt(0)).
//   siren.hip / siren_bwd.hip: 32-KiB chunks (one 32-row output tile x K = 256), 8 pieces, 3 buffers, vmcnt(0);
//   resblock.hip (one wave per SIMD: nothing else covers a chunk that has not landed): 20-KiB chunks, 5 pieces, 5 buffers, vmcnt(10).
template <int CHUNK_FLOATS, int PIECES, int NBUF, int WAIT>
struct ChunkPipeT {
    static constexpr int kSliceBytes = PIECES * 1024, kChunkBytes = CHUNK_FLOATS * 4, kWait = WAIT;
    static_assert(kChunkBytes == 4 * kSliceBytes, "four waves x PIECES pieces of 1 KiB");
    static_assert(NBUF >= 3 && WAIT == PIECES * (NBUF - 3), "the pieces of chunks c+2 .. c+NBUF-2 may stay outstanding");
    const char* img;          // image + this wave's slice (wave-uniform)
    const char* src;          // chunk being issued
    uint32_t voff;            // lane * 16
    uint32_t lds_base;        // LDS byte address of wbuf + this wave's slice
    uint32_t lds_dst;         // ... of the buffer being filled
    int idx, first, count, buf, use_buf;
    float* wbuf;
    const float* wcur;
    const float* wnxt;
    IF_PIPE_TIMING(stamp_t t_wait[2];)             // cycles in sync(): [0] the vmcnt wait, [1] the barrier
    __device__ __forceinline__ void init(float* wbuf_, const float* image, int wave, int lane, int first_, int count_) {
        const int wave_u = __builtin_amdgcn_readfirstlane(wave);
        wbuf = wbuf_;
        img = reinterpret_cast<const char*>(image) + wave_u * kSliceBytes;
        voff = (uint32_t)lane * 16u;
        lds_base = lds_addr(wbuf_) + (uint32_t)wave_u * kSliceBytes;
        first = first_; count = count_;
        idx = first_; buf = 0; use_buf = 0;
        src = img + (size_t)idx * kChunkBytes;
        lds_dst = lds_base;
        wcur = wbuf_; wnxt = wbuf_ + CHUNK_FLOATS;
        IF_PIPE_TIMING(t_wait[0] = 0; t_wait[1] = 0;)
    }
    __device__ __forceinline__ void issue_piece(int i) {     // i is a compile-time constant at every call site
        const char* s = src + (i >> 2) * 4096;                // the immediate is 13-bit signed: 4 KiB steps go into the bases
        const uint32_t d = lds_dst + (uint32_t)(i >> 2) * 4096u;
        switch (i & 3) {
            case 0: glds16_saddr<0>(s, voff, d); break;
            case 1: glds16_saddr<1024>(s, voff, d); break;
            case 2: glds16_saddr<2048>(s, voff, d); break;
            default: glds16_saddr<3072>(s, voff, d); break;
        }
        if (i == PIECES - 1) {
            idx = (idx + 1 == first + count) ? first : idx + 1;
            src = img + (size_t)idx * kChunkBytes;
            buf = (buf + 1 == NBUF) ? 0 : buf + 1;
            lds_dst = lds_base + (uint32_t)buf * kChunkBytes;
        }
    }
    __device__ __forceinline__ void prime() {
        for (int c = 0; c < NBUF - 1; ++c)
#pragma unroll
            for (int i = 0; i < PIECES; ++i) issue_piece(i);
    }
    __device__ __forceinline__ void sync() {
        IF_PIPE_TIMING(stamp_t tc[2]; stamp_mark(tc, 0);)
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(WAIT) : "memory");
        IF_PIPE_TIMING(stamp_mark(tc, 1);)
        __syncthreads();
        IF_PIPE_TIMING(t_wait[0] += tc[1] - tc[0]; stamp_add(t_wait, 1, tc[1]);)
    }
    __device__ __forceinline__ void advance() {
        use_buf = (use_buf + 1 == NBUF) ? 0 : use_buf + 1;
        wcur = wnxt;
        wnxt = wbuf + ((use_buf + 1 == NBUF) ? 0 : use_buf + 1) * CHUNK_FLOATS;
    }
};

// Power-of-two block scale of a point (a column of a split-f16 B operand) whose largest magnitude is m: value * sc lies in [1, 2)
// before the (hi, lo) split, and accumulator * inv is the unscaled sum -- inv = 1 / (128 * sc), the weight images carry kW16Scale
// = 128.  The GEMM is linear per column, so this is exact.
__device__ __forceinline__ void block_scale(float m, float& sc, float& inv) {
    const unsigned e = min((__float_as_uint(m) >> 23) & 255u, 254u);    // m in [2^(e-127), 2^(e-126)); inf/nan: scale 0 -> NaN out
    sc = __uint_as_float((254u - e) << 23);                             // m * sc in [1, 2)   (m == 0: sc = 2^127, harmless)
    inv = __uint_as_float((e > 8u ? e - 7u : 1u) << 23);                // 1 / (128 * sc) = 2^(e-134)
}

// maximum over the wavefront, in every lane.  By reference on purpose: a by-value parameter is `noundef` to the compiler, and for a value
// that comes straight from a load (amax_read) that changed the register allocation and one s_waitcnt of two decoder kernels against the
// loop written in place.  The amax epilogues of upfirdn2d.hip (two), ws_linear_kernel, modconv_kernel and pkconv_down_kernel still write
// the loop in place: called under their `if (out_amax)`, the helper flips the polarity of a handful of scalar branches there.
__device__ __forceinline__ float wave_max(const float& v) {
    float m = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, kWave));
    return m;
}

// DPP moves (gfx9 controls: quad_perm:[a,b,c,d] = a | b << 2 | c << 4 | d << 6, row_shr:n = 0x110 + n, row_ror:n = 0x120 + n, wave_shl:1 = 0x130, wave_shr:1 = 0x138, row_bcast:15 = 0x142,
// row_bcast:31 = 0x143).  dpp_f32: lanes the control does not reach read 0.  dpp_or: those lanes, and the rows outside ROW_MASK, get `ident`.
template <int CTRL> __device__ __forceinline__ float dpp_f32(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}
template <int CTRL, int ROW_MASK> __device__ __forceinline__ float dpp_or(float ident, float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, ident), __builtin_bit_cast(int, x), CTRL, ROW_MASK, 0xf, false));
}
// value of the lane one below / one above in the wavefront (the end lanes read 0)
__device__ __forceinline__ float dpp_wave_shr1(float v) { return dpp_f32<0x138>(v); }
__device__ __forceinline__ float dpp_wave_shl1(float v) { return dpp_f32<0x130>(v); }
// value of lane 4 q + I of the lane's quad (quad_perm:[I,I,I,I]), and ((v0 + v1) + v2) + v3 over the quad's lanes in that order, in every
// lane of the quad.  Whole quads must be active.
template <int I> __device__ __forceinline__ float dpp_quad_bcast(float v) { return dpp_f32<I * 0x55>(v); }
__device__ __forceinline__ float quad_sum(float v) {
    return __fadd_rn(__fadd_rn(__fadd_rn(dpp_quad_bcast<0>(v), dpp_quad_bcast<1>(v)), dpp_quad_bcast<2>(v)), dpp_quad_bcast<3>(v));
}

// XCD-aware tile order (block b runs on XCD b % 8, each XCD has its own L2): workgroup-tile t -> logical tile id such that every
// XCD walks one CONTIGUOUS range of logical ids, so tiles with neighbouring ids (they share operands) share an L2.
__device__ __forceinline__ int xcd_logical(int t, int n_tiles) {
    const int nq = n_tiles >> 3, nr = n_tiles & 7, xcd = t & 7, slot = t >> 3;
    return (xcd < nr ? xcd * (nq + 1) : nr * (nq + 1) + (xcd - nr) * nq) + slot;
}

}  // namespace e3dge
