// The training loss's own kernels: what joins the renderer, decoder, LPIPS and identity nodes into one scalar
// (project/losses/builder.py: LossClass).
//
//   avgpool fwd / bwd   the trainers' pool_256 / pool_64 (AdaptiveAvgPool2d at an integer ratio f): block mean over f x f, summed
//                       row-major inside the block, one multiplication by 1/f^2 (a power of two: the division, exactly).
//                       Bound: HBM, 4 B read per input element + 4 B / f^2 written (forward), the mirror image backward.
//   sqerr bwd           d_pred = (*scale) * (pred - gt): the MSE node's backward; the forward is e3dge_image_metrics' sums.
//   shape loss fwd/bwd  up to four terms of calc_shape_rec_loss (builder.py:76-104) in one tile launch + one fold launch
//                       (forward) and one launch (backward).  Bound: launch latency -- the C5 sizes are < 1 MB in all.
//
// Every kernel is a plain stream: 16-byte accesses where the row width and the pointers allow (a scalar form otherwise), wave
// shuffles, LDS, one partial per workgroup; the fold is one workgroup that adds the partials in a fixed order in double, as
// metrics.hip does.  No atomics: results are bit-identical from run to run.
#include "common.h"

namespace e3dge {

constexpr int kLsThreads = 256;

__host__ __device__ inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---------------------------------------------------------------------------------------------------------------- pool
// one thread = four consecutive outputs of one output row (one 16-byte store) from F rows of F 16-byte loads
template <int F>
__global__ void __launch_bounds__(kLsThreads)
avgpool_fwd_vec_kernel(float* __restrict__ out, const float* __restrict__ in, int64_t groups, int out_h, int out_w4, int in_w) {
    const int64_t gid = (int64_t)blockIdx.x * kLsThreads + threadIdx.x;
    if (gid >= groups) return;
    const int x4 = (int)(gid % out_w4);
    const int64_t row = gid / out_w4;                       // plane * out_h + oy
    const int oy = (int)(row % out_h);
    const int64_t plane = row / out_h;
    const float* __restrict__ src = in + ((plane * out_h + oy) * (int64_t)F) * in_w + (int64_t)x4 * 4 * F;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < F; ++r) {
        const float4* __restrict__ line = reinterpret_cast<const float4*>(src + (int64_t)r * in_w);
#pragma unroll
        for (int k = 0; k < F; ++k) {
            const float4 v = line[k];
            acc[(4 * k + 0) / F] += v.x;
            acc[(4 * k + 1) / F] += v.y;
            acc[(4 * k + 2) / F] += v.z;
            acc[(4 * k + 3) / F] += v.w;
        }
    }
    constexpr float inv = 1.0f / (float)(F * F);
    reinterpret_cast<float4*>(out)[gid] = make_float4(acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv);
}

// any width / alignment: one thread = one output
__global__ void __launch_bounds__(kLsThreads)
avgpool_fwd_scalar_kernel(float* __restrict__ out, const float* __restrict__ in, int64_t n_out, int out_h, int out_w, int in_w, int f) {
    const int64_t gid = (int64_t)blockIdx.x * kLsThreads + threadIdx.x;
    if (gid >= n_out) return;
    const int ox = (int)(gid % out_w);
    const int64_t row = gid / out_w;
    const float* __restrict__ src = in + (row * f) * in_w + (int64_t)ox * f;   // row = plane * out_h + oy; in_h = f * out_h
    float acc = 0.f;
    for (int r = 0; r < f; ++r)
        for (int c = 0; c < f; ++c) acc += src[(int64_t)r * in_w + c];
    out[gid] = acc * (1.0f / (float)(f * f));
}

// one thread = four consecutive elements of one input row (one 16-byte store)
template <int F>
__global__ void __launch_bounds__(kLsThreads)
avgpool_bwd_vec_kernel(float* __restrict__ d_in, const float* __restrict__ d_out, int64_t groups, int in_w4, int out_w) {
    const int64_t gid = (int64_t)blockIdx.x * kLsThreads + threadIdx.x;
    if (gid >= groups) return;
    const int x4 = (int)(gid % in_w4);
    const int64_t row = gid / in_w4;                        // plane * in_h + y, and in_h = F * out_h: the output row is row / F
    const float* __restrict__ src = d_out + (row / F) * out_w;
    constexpr float inv = 1.0f / (float)(F * F);
    const int x = x4 * 4;
    float4 v;
    if (F >= 4) {
        v.x = v.y = v.z = v.w = src[x / F] * inv;
    } else {
        v.x = src[(x + 0) / F] * inv; v.y = src[(x + 1) / F] * inv; v.z = src[(x + 2) / F] * inv; v.w = src[(x + 3) / F] * inv;
    }
    reinterpret_cast<float4*>(d_in)[gid] = v;
}

__global__ void __launch_bounds__(kLsThreads)
avgpool_bwd_scalar_kernel(float* __restrict__ d_in, const float* __restrict__ d_out, int64_t n_in, int in_w, int out_w, int f) {
    const int64_t gid = (int64_t)blockIdx.x * kLsThreads + threadIdx.x;
    if (gid >= n_in) return;
    const int x = (int)(gid % in_w);
    const int64_t row = gid / in_w;
    d_in[gid] = d_out[(row / f) * out_w + x / f] * (1.0f / (float)(f * f));
}

// --------------------------------------------------------------------------------------------------------------- sqerr
__global__ void __launch_bounds__(kLsThreads)
sqerr_bwd_kernel(float* __restrict__ d_pred, const float* __restrict__ pred, const float* __restrict__ gt, int64_t n, int vec,
                 const float* __restrict__ scale_ptr) {
    const float s = *scale_ptr;
    const int64_t gid = (int64_t)blockIdx.x * kLsThreads + threadIdx.x;
    const int64_t e0 = gid * 4;
    if (e0 >= n) return;
    if (vec && e0 + 4 <= n) {
        const float4 p = reinterpret_cast<const float4*>(pred)[gid], g = reinterpret_cast<const float4*>(gt)[gid];
        reinterpret_cast<float4*>(d_pred)[gid] = make_float4(s * (p.x - g.x), s * (p.y - g.y), s * (p.z - g.z), s * (p.w - g.w));
    } else {
        for (int64_t e = e0; e < n && e < e0 + 4; ++e) d_pred[e] = s * (pred[e] - gt[e]);
    }
}

// ---------------------------------------------------------------------------------------------------------- shape terms
// An item is one element (Smooth-L1) or one 3-vector (eikonal).  A thread takes groups of four items -- one 16-byte load per
// operand, three for the vectors --, a workgroup kShapeItems of them; segment s owns the workgroups [first[s], first[s + 1]).
constexpr int kShapeSeg = E3DGE_SHAPE_LOSS_SEGMENTS;
constexpr int kShapeGroupsPerThread = 2;
constexpr int kShapeItems = kLsThreads * 4 * kShapeGroupsPerThread;      // 2048

struct ShapeSeg {
    const float* pred;
    const float* gt;
    float* d_pred;
    int64_t n;
    float lambda;
    int kind, vec;
};
struct ShapeLaunch {
    ShapeSeg seg[kShapeSeg];
    int first[kShapeSeg + 1];
};

__device__ __forceinline__ float smooth_l1(float d) {
    const float a = fabsf(d);
    return a < 1.0f ? 0.5f * d * d : a - 0.5f;
}
__device__ __forceinline__ float eik_sq(float x, float y, float z) {
    const float r = sqrtf(x * x + y * y + z * z) - 1.0f;
    return r * r;
}
__device__ __forceinline__ float clamp1(float d) { return fminf(fmaxf(d, -1.0f), 1.0f); }
// d/de of (|e| - 1)^2 times c; torch's sub-gradient of norm() at the zero vector is 0
__device__ __forceinline__ void eik_grad(float c, float x, float y, float z, float& gx, float& gy, float& gz) {
    const float nrm = sqrtf(x * x + y * y + z * z);
    const float k = nrm > 0.0f ? c * 2.0f * (nrm - 1.0f) / nrm : 0.0f;
    gx = k * x; gy = k * y; gz = k * z;
}

__device__ __forceinline__ int shape_segment_of(const ShapeLaunch& L, int block) {
    int s = 0;
#pragma unroll
    for (int i = 1; i < kShapeSeg; ++i) s += block >= L.first[i] ? 1 : 0;
    return s;
}

__global__ void __launch_bounds__(kLsThreads)
shape_loss_tile_kernel(float* __restrict__ partial, const ShapeLaunch L) {
    __shared__ float red[kLsThreads / kWave];
    const int s = shape_segment_of(L, blockIdx.x);
    const float* __restrict__ p = L.seg[s].pred;
    const float* __restrict__ g = L.seg[s].gt;
    const int64_t n = L.seg[s].n;
    const int kind = L.seg[s].kind, vec = L.seg[s].vec;
    const int64_t base = (int64_t)(blockIdx.x - L.first[s]) * kShapeItems;
    float acc = 0.0f;
#pragma unroll
    for (int it = 0; it < kShapeGroupsPerThread; ++it) {
        const int64_t i0 = base + ((int64_t)it * kLsThreads + threadIdx.x) * 4;      // first item of this thread's group
        if (i0 >= n) continue;
        const bool whole = vec && i0 + 4 <= n;
        if (kind == E3DGE_SHAPE_SMOOTH_L1) {
            if (whole) {
                const float4 a = *reinterpret_cast<const float4*>(p + i0);
                float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
                if (g) b = *reinterpret_cast<const float4*>(g + i0);
                acc += smooth_l1(a.x - b.x); acc += smooth_l1(a.y - b.y); acc += smooth_l1(a.z - b.z); acc += smooth_l1(a.w - b.w);
            } else {
                for (int64_t i = i0; i < n && i < i0 + 4; ++i) acc += smooth_l1(p[i] - (g ? g[i] : 0.0f));
            }
        } else {
            if (whole) {
                const float4* q = reinterpret_cast<const float4*>(p + i0 * 3);
                const float4 a = q[0], b = q[1], c = q[2];
                acc += eik_sq(a.x, a.y, a.z); acc += eik_sq(a.w, b.x, b.y); acc += eik_sq(b.z, b.w, c.x); acc += eik_sq(c.y, c.z, c.w);
            } else {
                for (int64_t i = i0; i < n && i < i0 + 4; ++i) acc += eik_sq(p[i * 3], p[i * 3 + 1], p[i * 3 + 2]);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, kWave);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one workgroup: per segment the partials in a fixed order (double), mean, times lambda; total in the reference's order
__global__ void __launch_bounds__(kLsThreads)
shape_loss_fold_kernel(float* __restrict__ terms, float* __restrict__ total, const float* __restrict__ partial, const ShapeLaunch L) {
    __shared__ double acc[kLsThreads];
    __shared__ float term[kShapeSeg];
    for (int s = 0; s < kShapeSeg; ++s) {
        double t = 0.0;
        for (int i = L.first[s] + threadIdx.x; i < L.first[s + 1]; i += kLsThreads) t += (double)partial[i];
        acc[threadIdx.x] = t;
        __syncthreads();
        if (threadIdx.x == 0) {
            double sum = 0.0;
            for (int i = 0; i < kLsThreads; ++i) sum += acc[i];
            term[s] = L.seg[s].n > 0 ? (float)(sum / (double)L.seg[s].n) * L.seg[s].lambda : 0.0f;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float sum = 0.0f;
        for (int s = 0; s < kShapeSeg; ++s) { terms[s] = term[s]; if (L.seg[s].n > 0) sum += term[s]; }
        *total = sum;
    }
}

__global__ void __launch_bounds__(kLsThreads)
shape_loss_bwd_kernel(const float* __restrict__ upstream, const ShapeLaunch L) {
    const int s = shape_segment_of(L, blockIdx.x);
    const float* __restrict__ p = L.seg[s].pred;
    const float* __restrict__ g = L.seg[s].gt;
    float* __restrict__ d = L.seg[s].d_pred;
    const int64_t n = L.seg[s].n;
    const int kind = L.seg[s].kind, vec = L.seg[s].vec;
    const float c = *upstream * L.seg[s].lambda / (float)n;
    const int64_t base = (int64_t)(blockIdx.x - L.first[s]) * kShapeItems;
#pragma unroll
    for (int it = 0; it < kShapeGroupsPerThread; ++it) {
        const int64_t i0 = base + ((int64_t)it * kLsThreads + threadIdx.x) * 4;
        if (i0 >= n) continue;
        const bool whole = vec && i0 + 4 <= n;
        if (kind == E3DGE_SHAPE_SMOOTH_L1) {
            if (whole) {
                const float4 a = *reinterpret_cast<const float4*>(p + i0);
                float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
                if (g) b = *reinterpret_cast<const float4*>(g + i0);
                *reinterpret_cast<float4*>(d + i0) =
                    make_float4(c * clamp1(a.x - b.x), c * clamp1(a.y - b.y), c * clamp1(a.z - b.z), c * clamp1(a.w - b.w));
            } else {
                for (int64_t i = i0; i < n && i < i0 + 4; ++i) d[i] = c * clamp1(p[i] - (g ? g[i] : 0.0f));
            }
        } else {
            if (whole) {
                const float4* q = reinterpret_cast<const float4*>(p + i0 * 3);
                const float4 a = q[0], b = q[1], e = q[2];
                float4 oa, ob, oe;
                eik_grad(c, a.x, a.y, a.z, oa.x, oa.y, oa.z);
                eik_grad(c, a.w, b.x, b.y, oa.w, ob.x, ob.y);
                eik_grad(c, b.z, b.w, e.x, ob.z, ob.w, oe.x);
                eik_grad(c, e.y, e.z, e.w, oe.y, oe.z, oe.w);
                float4* o = reinterpret_cast<float4*>(d + i0 * 3);
                o[0] = oa; o[1] = ob; o[2] = oe;
            } else {
                for (int64_t i = i0; i < n && i < i0 + 4; ++i) {
                    float gx, gy, gz;
                    eik_grad(c, p[i * 3], p[i * 3 + 1], p[i * 3 + 2], gx, gy, gz);
                    d[i * 3] = gx; d[i * 3 + 1] = gy; d[i * 3 + 2] = gz;
                }
            }
        }
    }
}

// validates `a` and lays the segments out over workgroups; `backward`: d_pred is required where the forward needs none
static int shape_plan(ShapeLaunch& L, const E3dgeShapeLossArgs* a, const char* who, bool backward) {
    E3DGE_REQUIRE(a != nullptr, "%s: args is null", who);
    int64_t blocks = 0;
    for (int s = 0; s < kShapeSeg; ++s) {
        const E3dgeShapeLossSegment& in = a->seg[s];
        E3DGE_REQUIRE(in.n >= 0, "%s: seg[%d].n=%lld is negative", who, s, (long long)in.n);
        L.first[s] = (int)blocks;
        ShapeSeg& o = L.seg[s];
        o.pred = in.pred; o.gt = in.gt; o.d_pred = in.d_pred; o.n = in.n; o.lambda = in.lambda; o.kind = in.kind;
        o.vec = aligned16(in.pred) && aligned16(in.gt) && (!backward || aligned16(in.d_pred));
        if (in.n == 0) continue;
        E3DGE_REQUIRE(in.kind == E3DGE_SHAPE_SMOOTH_L1 || in.kind == E3DGE_SHAPE_EIKONAL, "%s: seg[%d].kind=%d", who, s, in.kind);
        E3DGE_REQUIRE(in.pred != nullptr, "%s: seg[%d].pred is null", who, s);
        E3DGE_REQUIRE(in.kind != E3DGE_SHAPE_EIKONAL || in.gt == nullptr, "%s: seg[%d].gt must be null for the eikonal kind", who, s);
        E3DGE_REQUIRE(!backward || in.d_pred != nullptr, "%s: seg[%d].d_pred is null", who, s);
        blocks += (in.n + kShapeItems - 1) / kShapeItems;
        E3DGE_REQUIRE(blocks < ((int64_t)1 << 30), "%s: seg[%d].n=%lld: grid too large", who, s, (long long)in.n);
    }
    L.first[kShapeSeg] = (int)blocks;
    return E3DGE_OK;
}

template <int F>
static void pool_fwd_launch(float* out, const float* in, int64_t groups, int out_h, int out_w4, int in_w, hipStream_t st) {
    avgpool_fwd_vec_kernel<F><<<dim3((unsigned)((groups + kLsThreads - 1) / kLsThreads)), dim3(kLsThreads), 0, st>>>(out, in, groups, out_h,
                                                                                                                 out_w4, in_w);
}
template <int F>
static void pool_bwd_launch(float* d_in, const float* d_out, int64_t groups, int in_w4, int out_w, hipStream_t st) {
    avgpool_bwd_vec_kernel<F><<<dim3((unsigned)((groups + kLsThreads - 1) / kLsThreads)), dim3(kLsThreads), 0, st>>>(d_in, d_out, groups,
                                                                                                                 in_w4, out_w);
}

static int pool_check(const char* who, int64_t planes, int in_h, int in_w, int f) {
    E3DGE_REQUIRE(planes >= 0, "%s: planes=%lld is negative", who, (long long)planes);
    E3DGE_REQUIRE(in_h >= 1 && in_w >= 1, "%s: in_h=%d in_w=%d", who, in_h, in_w);
    E3DGE_REQUIRE(f == 1 || f == 2 || f == 4 || f == 8 || f == 16, "%s: f=%d (1, 2, 4, 8 or 16)", who, f);
    E3DGE_REQUIRE(in_h % f == 0 && in_w % f == 0, "%s: in_h=%d in_w=%d are not multiples of f=%d", who, in_h, in_w, f);
    E3DGE_REQUIRE(planes * in_h * (int64_t)in_w < ((int64_t)1 << 38), "%s: planes=%lld: grid too large", who, (long long)planes);
    return E3DGE_OK;
}

}  // namespace e3dge

using namespace e3dge;

extern "C" int e3dge_avgpool_fwd(float* out, const float* in, int64_t planes, int in_h, int in_w, int f, e3dge_stream_t stream) {
    if (int rc = pool_check("avgpool_fwd", planes, in_h, in_w, f)) return rc;
    if (planes == 0) return E3DGE_OK;
    E3DGE_REQUIRE(out != nullptr, "avgpool_fwd: out is null");
    E3DGE_REQUIRE(in != nullptr, "avgpool_fwd: in is null");
    const int out_h = in_h / f, out_w = in_w / f;
    const int64_t n_out = planes * out_h * out_w;
    hipStream_t st = as_stream(stream);
    if (out_w % 4 == 0 && aligned16(out) && aligned16(in)) {
        const int64_t groups = n_out / 4;
        switch (f) {
            case 1: pool_fwd_launch<1>(out, in, groups, out_h, out_w / 4, in_w, st); break;
            case 2: pool_fwd_launch<2>(out, in, groups, out_h, out_w / 4, in_w, st); break;
            case 4: pool_fwd_launch<4>(out, in, groups, out_h, out_w / 4, in_w, st); break;
            case 8: pool_fwd_launch<8>(out, in, groups, out_h, out_w / 4, in_w, st); break;
            default: pool_fwd_launch<16>(out, in, groups, out_h, out_w / 4, in_w, st); break;
        }
    } else {
        avgpool_fwd_scalar_kernel<<<dim3((unsigned)((n_out + kLsThreads - 1) / kLsThreads)), dim3(kLsThreads), 0, st>>>(out, in, n_out, out_h,
                                                                                                                     out_w, in_w, f);
    }
    return check_launch("avgpool_fwd");
}

extern "C" int e3dge_avgpool_bwd(float* d_in, const float* d_out, int64_t planes, int in_h, int in_w, int f, e3dge_stream_t stream) {
    if (int rc = pool_check("avgpool_bwd", planes, in_h, in_w, f)) return rc;
    if (planes == 0) return E3DGE_OK;
    E3DGE_REQUIRE(d_in != nullptr, "avgpool_bwd: d_in is null");
    E3DGE_REQUIRE(d_out != nullptr, "avgpool_bwd: d_out is null");
    const int out_w = in_w / f;
    const int64_t n_in = planes * in_h * in_w;
    hipStream_t st = as_stream(stream);
    if (in_w % 4 == 0 && aligned16(d_in)) {
        const int64_t groups = n_in / 4;
        switch (f) {
            case 1: pool_bwd_launch<1>(d_in, d_out, groups, in_w / 4, out_w, st); break;
            case 2: pool_bwd_launch<2>(d_in, d_out, groups, in_w / 4, out_w, st); break;
            case 4: pool_bwd_launch<4>(d_in, d_out, groups, in_w / 4, out_w, st); break;
            case 8: pool_bwd_launch<8>(d_in, d_out, groups, in_w / 4, out_w, st); break;
            default: pool_bwd_launch<16>(d_in, d_out, groups, in_w / 4, out_w, st); break;
        }
    } else {
        avgpool_bwd_scalar_kernel<<<dim3((unsigned)((n_in + kLsThreads - 1) / kLsThreads)), dim3(kLsThreads), 0, st>>>(d_in, d_out, n_in, in_w,
                                                                                                                    out_w, f);
    }
    return check_launch("avgpool_bwd");
}

extern "C" int e3dge_sqerr_bwd(float* d_pred, const float* pred, const float* gt, int64_t n, const float* scale_ptr,
                               e3dge_stream_t stream) {
    E3DGE_REQUIRE(n >= 0, "sqerr_bwd: n=%lld is negative", (long long)n);
    if (n == 0) return E3DGE_OK;
    E3DGE_REQUIRE(d_pred != nullptr, "sqerr_bwd: d_pred is null");
    E3DGE_REQUIRE(pred != nullptr, "sqerr_bwd: pred is null");
    E3DGE_REQUIRE(gt != nullptr, "sqerr_bwd: gt is null");
    E3DGE_REQUIRE(scale_ptr != nullptr, "sqerr_bwd: scale_ptr is null");
    const int64_t groups = (n + 3) / 4, blocks = (groups + kLsThreads - 1) / kLsThreads;
    E3DGE_REQUIRE(blocks < ((int64_t)1 << 31), "sqerr_bwd: n=%lld: grid too large", (long long)n);
    const int vec = aligned16(d_pred) && aligned16(pred) && aligned16(gt);
    sqerr_bwd_kernel<<<dim3((unsigned)blocks), dim3(kLsThreads), 0, as_stream(stream)>>>(d_pred, pred, gt, n, vec, scale_ptr);
    return check_launch("sqerr_bwd");
}

extern "C" int64_t e3dge_shape_loss_partial_floats(const E3dgeShapeLossArgs* args) {
    if (!args) return 0;
    int64_t blocks = 0;
    for (int s = 0; s < kShapeSeg; ++s)
        if (args->seg[s].n > 0) blocks += (args->seg[s].n + kShapeItems - 1) / kShapeItems;
    return blocks;
}

extern "C" int e3dge_shape_loss_fwd(const E3dgeShapeLossArgs* args, e3dge_stream_t stream) {
    ShapeLaunch L;
    if (int rc = shape_plan(L, args, "shape_loss_fwd", false)) return rc;
    const int blocks = L.first[kShapeSeg];
    if (blocks == 0) return E3DGE_OK;
    E3DGE_REQUIRE(args->terms != nullptr, "shape_loss_fwd: terms is null");
    E3DGE_REQUIRE(args->total != nullptr, "shape_loss_fwd: total is null");
    E3DGE_REQUIRE(args->partial != nullptr, "shape_loss_fwd: partial is null");
    E3DGE_REQUIRE(args->partial_floats >= blocks, "shape_loss_fwd: partial_floats=%lld, %d needed", (long long)args->partial_floats, blocks);
    hipStream_t st = as_stream(stream);
    shape_loss_tile_kernel<<<dim3((unsigned)blocks), dim3(kLsThreads), 0, st>>>(args->partial, L);
    if (int rc = check_launch("shape_loss_fwd(tiles)")) return rc;
    shape_loss_fold_kernel<<<dim3(1), dim3(kLsThreads), 0, st>>>(args->terms, args->total, args->partial, L);
    return check_launch("shape_loss_fwd(fold)");
}

extern "C" int e3dge_shape_loss_bwd(const E3dgeShapeLossArgs* args, e3dge_stream_t stream) {
    ShapeLaunch L;
    if (int rc = shape_plan(L, args, "shape_loss_bwd", true)) return rc;
    const int blocks = L.first[kShapeSeg];
    if (blocks == 0) return E3DGE_OK;
    E3DGE_REQUIRE(args->upstream != nullptr, "shape_loss_bwd: upstream is null");
    shape_loss_bwd_kernel<<<dim3((unsigned)blocks), dim3(kLsThreads), 0, as_stream(stream)>>>(args->upstream, L);
    return check_launch("shape_loss_bwd");
}
