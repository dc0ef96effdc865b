// Cycle stamps of the instrumented variant builds (build.py --variant NAME --only STEM -D<selector>): the one place that knows
// how they are stored and read.  Kernels keep their stamps in a small per-thread array and leave them, once, in a side buffer of
// their own translation unit -- never in an argument buffer, so an instrumented build returns the default build's outputs.  The
// host copies the buffer out with e3dge_debug_stamps (tools/kernel_stamps.py prints it).  With no selector set every macro below
// expands to nothing and no buffer exists: the default library's device code does not know about any of this.
//
// Selectors (one per kernel; instrumenting one leaves the others alone) and the words of a slot, all raw 64-bit counts:
//   siren      E3DGE_PHASE_TIMING  slot 0, thread 0 of workgroup 0 (render launches): word 6 sub + i = cycle counter at boundary i of
//                                  sub-tile sub (0 loop top, 1 geometry + layer 0, 2 layers 1-7, 3 sdf + alpha + scan, 4 view layer,
//                                  5 rgb + composite + merge); 8-wave kernel (sub < 3): 18 chunk-wait vmcnt sum, 19 barrier sum,
//                                  20 kernel entry, 21 loop start, 22 loop end, 23 after the per-ray stores.  First generation
//                                  (sub < 4): slot 1 + w, words 0 / 1 = the vmcnt / barrier sums of wave w.
//              E3DGE_16_TRACE      slots 8 / 9 = waves 0 / 4 of workgroup 7, hidden layer 3, tile 6: s_memtime at 3 g + (0 start,
//                                  1 MFMAs issued, 2 epilogue slice done) of k-step g.
//   siren_bwd  E3DGE_BWD_TIMING    slot = workgroup, thread 0 (first-generation kernel): 0 total, 1 prologue, 2 GEMM tiles, 3 epilogues,
//                                  4 layer tails, 5 / 6 the vmcnt / barrier sums inside the tiles.
//   resblock   E3DGE_RB_TRACE      slot i = the i-th stamp of wave 0, workgroup 7, sub-tile 1: word 0 tag, word 1 s_memtime.  =1: the
//                                  four phase boundaries (tags 1000..4000), held in SGPRs until the sub-tile ends; =2: also every
//                                  k-step and chunk wait of tiles E3DGE_RB_TRACE_T2 / _T3 (the stamp code spills: structure only).
//   modconv    E3DGE_MC_TIMING     slot 0, thread 0 of workgroup 0: 0 issue, 1 mfma, 2 epilogue, 3 convert + LDS store, 4 vmcnt wait,
//                                  5 barrier (sums over the steps), 6 total, 7 steps.
//   decoder2   E3DGE_PK_TIMING     slots 2 r / 2 r + 1 = waves 0 / NW-1 of workgroup 0 of the forward launch whose output amax buffer is
//                                  r (conv1: 1, level u: up-sampling 3 + 3 u, conv 4 + 3 u; r = 0: every other launch): 0 wait +
//                                  barrier, 1 issue, 2 MFMAs, 3 epilogue (sums over the steps), 4 / 5 tap 0 / taps 1-8 of the steps
//                                  with an epilogue, 6 / 7 of the other steps, 8 total, 9 steps.
#pragma once
#include "common.h"

#ifdef E3DGE_PHASE_TIMING
#define IF_PHASE_TIMING(...) __VA_ARGS__
#else
#define IF_PHASE_TIMING(...)
#endif
#if defined(E3DGE_PHASE_TIMING) || defined(E3DGE_BWD_TIMING)      // ChunkPipeT (gfx950_prims.h) as ChunkPipe serves both kernels
#define IF_PIPE_TIMING(...) __VA_ARGS__
#else
#define IF_PIPE_TIMING(...)
#endif
#ifdef E3DGE_BWD_TIMING
#define IF_BWD_TIMING(...) __VA_ARGS__
#else
#define IF_BWD_TIMING(...)
#endif
#ifdef E3DGE_16_TRACE
#define IF_16_TRACE(...) __VA_ARGS__
#else
#define IF_16_TRACE(...)
#endif
#ifdef E3DGE_RB_TRACE
#define IF_RB_TRACE(...) __VA_ARGS__
#else
#define IF_RB_TRACE(...)
#endif
#if defined(E3DGE_RB_TRACE) && E3DGE_RB_TRACE > 1      // level 1 only / level 2 only
#define IF_RB_TRACE1(...)
#define IF_RB_TRACE2(...) __VA_ARGS__
#else
#define IF_RB_TRACE1(...) IF_RB_TRACE(__VA_ARGS__)
#define IF_RB_TRACE2(...)
#endif
#ifdef E3DGE_MC_TIMING
#define IF_MC_TIMING(...) __VA_ARGS__
#else
#define IF_MC_TIMING(...)
#endif
#ifdef E3DGE_PK_TIMING
#define IF_PK_TIMING(...) __VA_ARGS__
#else
#define IF_PK_TIMING(...)
#endif

namespace e3dge {

constexpr int kStampSlots = 320, kStampWords = 24;      // 320 stamps of E3DGE_RB_TRACE=2; 256 workgroups of the backward at 64 x 64 x 24
enum { kStampUnitSiren, kStampUnitSirenBwd, kStampUnitResblock, kStampUnitModconv, kStampUnitDecoder2, kStampUnits };

#if defined(E3DGE_PHASE_TIMING) || defined(E3DGE_BWD_TIMING) || defined(E3DGE_16_TRACE) || defined(E3DGE_RB_TRACE) || \
    defined(E3DGE_MC_TIMING) || defined(E3DGE_PK_TIMING)
typedef unsigned long long stamp_t;
// The library is built without relocatable device code: every translation unit has its own copy.
static __device__ stamp_t g_stamps[kStampSlots * kStampWords];

// Two clocks, as each site chose them: s_memtime into an SGPR (with or without its wait: a site that collects later waits once,
// in stamps_flush<kStampWaitLgkm>), and the cycle counter.
#define STAMP_MEMTIME(dst) asm volatile("s_memtime %0" : "=s"(dst))
#define STAMP_MEMTIME_WAIT(dst) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(dst))
__device__ __forceinline__ stamp_t stamp_now() { return __builtin_readcyclecounter(); }
__device__ __forceinline__ void stamp_mark(stamp_t* v, int i) { v[i] = stamp_now(); }
__device__ __forceinline__ void stamp_add(stamp_t* v, int i, stamp_t& last) {        // v[i] += time since the last mark
    const stamp_t now = stamp_now();
    v[i] += now - last;
    last = now;
}

// Leave v[0..n) in words word0.. of `slot`: every thread calls it (WAIT = the workgroup barrier or the scalar-memory wait the site
// needs in front of its stores), `writer` stores.  Writers beyond the last slot are dropped.
enum { kStampNoWait, kStampBarrier, kStampWaitLgkm };
template <int WAIT = kStampNoWait>
__device__ __forceinline__ void stamps_flush(bool writer, int slot, const stamp_t* v, int n, int word0 = 0) {
    if (WAIT == kStampBarrier) __syncthreads();
    if (WAIT == kStampWaitLgkm) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (writer && slot < kStampSlots)
        for (int i = 0; i < n; ++i) g_stamps[slot * kStampWords + word0 + i] = v[i];
}

// out != NULL: copy the buffer out; NULL: zero it.  `on`: is this unit's selector set (another unit's may be)?
#define E3DGE_STAMPS_UNIT(unit, on, need)                                                                                         \
    int stamps_##unit(unsigned long long* out, int64_t n_words) {                                                                 \
        if (!(on)) return fail(E3DGE_ERR_UNSUPPORTED, "stamps: " #unit " is not instrumented in this build (needs " need ")");    \
        static const stamp_t zero[kStampSlots * kStampWords] = {};                                                                \
        const hipError_t e = out ? hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(stamp_t) * n_words)                       \
                                 : hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), zero, sizeof(zero));                                   \
        return e == hipSuccess ? E3DGE_OK : fail(E3DGE_ERR_LAUNCH, "stamps(" #unit "): %s", hipGetErrorString(e));                \
    }
#else
#define E3DGE_STAMPS_UNIT(unit, on, need)                                                                                         \
    int stamps_##unit(unsigned long long*, int64_t) {                                                                             \
        return fail(E3DGE_ERR_UNSUPPORTED, "stamps: " #unit " is not instrumented in this build (needs " need ")");               \
    }
#endif

// one per instrumented translation unit (E3DGE_STAMPS_UNIT); the dispatcher below them lives in stream_ops.hip
int stamps_siren(unsigned long long*, int64_t);
int stamps_siren_bwd(unsigned long long*, int64_t);
int stamps_resblock(unsigned long long*, int64_t);
int stamps_modconv(unsigned long long*, int64_t);
int stamps_decoder2(unsigned long long*, int64_t);

}  // namespace e3dge

// Debug entry points, deliberately not part of include/e3dge_hip.h.  `unit`: kStampUnit*; n_words <= kStampSlots * kStampWords.
// Both synchronise with the device (they are plain symbol copies); both fail with the selector's name on a unit that has none set.
extern "C" int e3dge_debug_stamps(int unit, unsigned long long* out, int64_t n_words);
extern "C" int e3dge_debug_stamps_clear(int unit);
