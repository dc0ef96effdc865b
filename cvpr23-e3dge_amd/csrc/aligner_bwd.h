// The 2-D residual aligner (ADA), trainable form: the kernels around the convolutions -- BatchNorm on batch statistics (forward and
// backward), the PReLU backward with its slope gradient, and the adjoints of aln_up2_kernel and of MaxPool2d(1, stride).  Included by
// aligner.hip (after aln_up2_tap and the kAlnSc* modes); below them the data and the weight gradient of a convolution.  Every kernel is
// followed by its launch helper, which the network (aligner_train.h) and the run-time-shape entry of aligner.hip both call.  Measured errors and times: DESIGN.md 4.17b.
//
// Every per-channel sum runs in float64 in a fixed order: a workgroup sums one (channel, image, pixel segment) -- 256 strided partial
// sums, then a fixed tree through LDS -- and one thread per channel folds the partials, images then segments ascending.  The segment
// length (kAlnSeg pixels) comes from the plane alone.  No atomics, no scratch: results are bit-reproducible.
//
//   aln_bn_stats_kernel / _fold   S = sum x, SS = sum x^2 per channel over (n, h, w), x from up to two tensors split at a run-time channel
//                                 (the leading BatchNorm of dconv_layer*.0 sees cat(up, feat)); mean = S / M, var = SS / M - mean^2
//                                 (biased), both kept in float64; (a, b) = (gamma rstd, beta - mean a), rounded once -- the pair the
//                                 convolution's gather (in_ab) or aln_bn_apply_kernel reads.
//   aln_bn_apply_kernel           y = a v + b, an optional PReLU, an optional shortcut added after that rounding: the strided pick, a read,
//                                 or the raw 1x1 branch under its own (a, b).  The arithmetic of aln_conv_kernel's epilogue.
//   aln_norm_sums_kernel / _fold  P = sum g, Q = sum g xhat, xhat = (x - mean) rstd in float64; d beta = P, d gamma = Q; the factors of
//   aln_norm_bwd_kernel           g_x = A g + B x + C (+ a fan-in addend), summed in float64 and rounded once.  Batch statistics:
//                                 A = gamma rstd, B = -A Q rstd / M, C = -A P / M - B mean.  Running statistics: B = C = 0.
//   aln_prelu_bwd_kernel / _fold  g_x = pre > 0 ? g : slope g (the branch from the saved pre-activation's sign); d slope = sum g pre over
//                                 the non-positive branch.
//   aln_up2_bwd_kernel            the adjoint of aln_up2_kernel as a gather over the low-resolution pixel: the up to 5 x 5 output pixels
//                                 around it in ascending order, each with the forward's own aln_up2_tap weights; float64 sum, one rounding.
//   aln_pick_bwd_kernel           the adjoint of x[:, :, ::stride, ::stride]: a predicated read of g (+ a fan-in addend), not a scatter.
#pragma once

namespace e3dge {

constexpr int kAlnSeg = 4096;                                        // pixels of one partial sum
constexpr double kAlnEps = 1e-5;                                     // nn.BatchNorm2d's eps
enum { kAlnScAffine = 3 };                                           // aln_bn_apply: + sc_ab.x sc + sc_ab.y (beside kAlnScNone / Pick / Read)

static int aln_segments(int hw) { return (hw + kAlnSeg - 1) / kAlnSeg; }
static unsigned aln_blocks(int64_t total) { return (unsigned)((total + 255) / 256); }
// workspace of the per-channel sums: the partials (two float64 per channel, image and segment), then three float64 per channel
static int64_t aln_norm_ws_bytes(int64_t n, int64_t c, int hw) { return (2 * c * n * aln_segments(hw) + 3 * c) * (int64_t)sizeof(double); }

struct AlnSrc2 { const float* p0; const float* p1; int c0, c1; };   // channels [0, c0) of p0 (n, c0, h, w), then c1 of p1 (n, c1, h, w)

__device__ __forceinline__ const float* aln_plane(const AlnSrc2& s, int img, int c, int hw) {
    return c < s.c0 ? s.p0 + ((int64_t)img * s.c0 + c) * hw : s.p1 + ((int64_t)img * s.c1 + (c - s.c0)) * hw;
}

// The two sums of a workgroup of 256: thread t's values at red[.][t], folded by halves -- the same order at every launch.
__device__ __forceinline__ void aln_block_sum2(double s0, double s1, double* part) {
    __shared__ double red[2][256];
    const int tid = threadIdx.x;
    red[0][tid] = s0; red[1][tid] = s1;
    __syncthreads();
#pragma unroll
    for (int step = 128; step >= 1; step >>= 1) {
        if (tid < step) { red[0][tid] += red[0][tid + step]; red[1][tid] += red[1][tid + step]; }
        __syncthreads();
    }
    if (tid == 0) { part[0] = red[0][0]; part[1] = red[1][0]; }
}

// grid (segments, n, channels); partials at ((c n + img) segments + seg) * 2
__device__ __forceinline__ double* aln_partial(double* part) {
    return part + (((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 2;
}

__device__ __forceinline__ void aln_fold(const double* part, int c, int count, double& s0, double& s1) {
    const double* p = part + (int64_t)c * count * 2;
    s0 = s1 = 0.0;
    for (int i = 0; i < count; ++i) { s0 += p[2 * i]; s1 += p[2 * i + 1]; }
}

// ---- batch statistics -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) aln_bn_stats_kernel(double* __restrict__ part, AlnSrc2 src, int hw) {
    const float* __restrict__ x = aln_plane(src, blockIdx.y, blockIdx.z, hw);
    const int end = min(hw, (int)(blockIdx.x + 1) * kAlnSeg);
    double s = 0.0, ss = 0.0;
    for (int i = blockIdx.x * kAlnSeg + threadIdx.x; i < end; i += 256) {
        const double v = x[i];
        s += v;
        ss = fma(v, v, ss);                                           // v^2 is exact in float64
    }
    aln_block_sum2(s, ss, aln_partial(part));
}

__global__ void __launch_bounds__(64) aln_bn_stats_fold_kernel(float2* __restrict__ ab, double* __restrict__ stats, const double* __restrict__ part,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta, int C, int count,
                                                               double M) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double s, ss;
    aln_fold(part, c, count, s, ss);
    const double mean = s / M, var = fmax(ss / M - mean * mean, 0.0);
    if (stats) { stats[2 * c] = mean; stats[2 * c + 1] = var; }
    if (ab) {
        const double a = (double)gamma[c] / sqrt(var + kAlnEps);
        ab[c] = make_float2((float)a, (float)((double)beta[c] - mean * a));
    }
}

static int aln_stats(float* ab, double* stats, double* part, const float* in0, const float* in1, const float* gamma, const float* beta, int n, int c,
                     int split, int hw, hipStream_t st) {
    const int segs = aln_segments(hw);
    aln_bn_stats_kernel<<<dim3(segs, n, c), dim3(256), 0, st>>>(part, AlnSrc2{in0, in1, split, c - split}, hw);
    aln_bn_stats_fold_kernel<<<dim3((c + 63) / 64), dim3(64), 0, st>>>(reinterpret_cast<float2*>(ab), stats, part, gamma, beta, c, n * segs, (double)n * hw);
    return check_launch("aln(stats)");
}

// ---- a v + b, PReLU, shortcut -----------------------------------------------------------------------------------------------------------
struct AlnApplyArgs {
    float* out; const float* in; const float2* ab; const float* slope; const float* sc; const float2* sc_ab;
    int C, OH, OW, SH, SW, stride, sc_mode; int64_t total;
};

__global__ void __launch_bounds__(256) aln_bn_apply_kernel(AlnApplyArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.total) return;
    const int OHW = a.OH * a.OW;
    const int64_t plane = i / OHW;
    const int pix = (int)(i - plane * OHW), c = (int)(plane % a.C);
    float v = a.in[i];
    if (a.ab) { const float2 e = a.ab[c]; v = __fmaf_rn(e.x, v, e.y); }
    if (a.slope) v = v > 0.0f ? v : __fmul_rn(a.slope[c], v);
    if (a.sc_mode == kAlnScPick) {
        const int oy = pix / a.OW, ox = pix - oy * a.OW;
        v = __fadd_rn(v, a.sc[(plane * a.SH + (int64_t)oy * a.stride) * a.SW + ox * a.stride]);
    } else if (a.sc_mode == kAlnScRead) {
        v = __fadd_rn(v, a.sc[i]);
    } else if (a.sc_mode == kAlnScAffine) {
        const float2 s = a.sc_ab[c];
        v = __fadd_rn(v, __fmaf_rn(s.x, a.sc[i], s.y));
    }
    a.out[i] = v;
}

static int aln_apply(float* out, const float* in, const float* ab, const float* slope, const float* sc, const float* sc_ab, int n, int c, int oh, int ow,
                     int sh, int sw, int stride, int mode, hipStream_t st) {
    AlnApplyArgs a;
    a.out = out; a.in = in; a.ab = reinterpret_cast<const float2*>(ab); a.slope = slope; a.sc = sc; a.sc_ab = reinterpret_cast<const float2*>(sc_ab);
    a.C = c; a.OH = oh; a.OW = ow; a.SH = sh; a.SW = sw; a.stride = stride; a.sc_mode = mode; a.total = (int64_t)n * c * oh * ow;
    aln_bn_apply_kernel<<<dim3(aln_blocks(a.total)), dim3(256), 0, st>>>(a);
    return check_launch("aln(apply)");
}

// ---- BatchNorm backward -----------------------------------------------------------------------------------------------------------------
struct AlnNormStat { const double* stats; const float* rmean; const float* rvar; };   // batch statistics (mean, var), or the running ones

__device__ __forceinline__ void aln_norm_stat(const AlnNormStat& s, int c, double& mean, double& rstd) {
    const double var = s.stats ? s.stats[2 * c + 1] : (double)s.rvar[c];
    mean = s.stats ? s.stats[2 * c] : (double)s.rmean[c];
    rstd = 1.0 / sqrt(var + kAlnEps);
}

__global__ void __launch_bounds__(256) aln_norm_sums_kernel(double* __restrict__ part, const float* __restrict__ gy, AlnSrc2 src, AlnNormStat st,
                                                            int C, int hw) {
    const int c = blockIdx.z, img = blockIdx.y;
    const float* __restrict__ x = aln_plane(src, img, c, hw);
    const float* __restrict__ g = gy + ((int64_t)img * C + c) * hw;
    double mean, rstd;
    aln_norm_stat(st, c, mean, rstd);
    const int end = min(hw, (int)(blockIdx.x + 1) * kAlnSeg);
    double p = 0.0, q = 0.0;
    for (int i = blockIdx.x * kAlnSeg + threadIdx.x; i < end; i += 256) {
        const double gv = g[i];
        p += gv;
        q = fma(gv, ((double)x[i] - mean) * rstd, q);
    }
    aln_block_sum2(p, q, aln_partial(part));
}

// coef: (A, B, C) per channel
__global__ void __launch_bounds__(64) aln_norm_fold_kernel(double* __restrict__ coef, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           const double* __restrict__ part, const float* __restrict__ gamma, AlnNormStat st, int C,
                                                           int count, double M, int train) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double mean, rstd, P = 0.0, Q = 0.0;
    aln_norm_stat(st, c, mean, rstd);
    if (part) aln_fold(part, c, count, P, Q);
    if (dgamma) dgamma[c] = (float)Q;
    if (dbeta) dbeta[c] = (float)P;
    const double A = (double)gamma[c] * rstd;
    const double B = train ? -A * Q * rstd / M : 0.0;
    coef[3 * c] = A; coef[3 * c + 1] = B; coef[3 * c + 2] = train ? -A * P / M - B * mean : 0.0;
}

struct AlnDst2 { float* p0; float* p1; int c0, c1; };                 // the destination split like a source: channels [0, c0) to p0, the rest to p1

__device__ __forceinline__ float* aln_plane(const AlnDst2& d, int img, int c, int hw) {
    return c < d.c0 ? d.p0 + ((int64_t)img * d.c0 + c) * hw : d.p1 + ((int64_t)img * d.c1 + (c - d.c0)) * hw;
}

__global__ void __launch_bounds__(256) aln_norm_bwd_kernel(AlnDst2 gx, const float* __restrict__ gy, AlnSrc2 src, const float* __restrict__ add,
                                                           const float* __restrict__ add1, const double* __restrict__ coef, int C, int hw,
                                                           int64_t total, int train) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t plane = i / hw;
    const int pix = (int)(i - plane * hw), c = (int)(plane % C), img = (int)(plane / C);
    double v = coef[3 * c] * (double)gy[i];
    if (train) v += fma(coef[3 * c + 1], (double)aln_plane(src, img, c, hw)[pix], coef[3 * c + 2]);
    if (add) v += (double)add[i];
    if (add1) v += (double)add1[i];
    aln_plane(gx, img, c, hw)[pix] = (float)v;
}

// gx split at gsplit (gx1 NULL: one tensor; gx0 NULL: the parameter gradients alone); dgamma / dbeta NULL: not wanted; ws: aln_norm_ws_bytes
static int aln_norm_bwd(float* gx0, float* gx1, int gsplit, float* dgamma, float* dbeta, const float* gy, const float* in0, const float* in1, int split,
                        const float* gamma, const double* stats, const float* rmean, const float* rvar, const float* add0, const float* add1, double* ws,
                        int n, int c, int hw, int train, hipStream_t st) {
    const int segs = aln_segments(hw);
    double* coef = ws + (int64_t)2 * c * n * segs;
    const AlnSrc2 src{in0, in1, split, c - split};
    const AlnNormStat ns{train ? stats : nullptr, rmean, rvar};
    const bool sums = train || dgamma || dbeta;                       // on running statistics g_x = A g needs no sum
    if (sums) aln_norm_sums_kernel<<<dim3(segs, n, c), dim3(256), 0, st>>>(ws, gy, src, ns, c, hw);
    aln_norm_fold_kernel<<<dim3((c + 63) / 64), dim3(64), 0, st>>>(coef, dgamma, dbeta, sums ? ws : nullptr, gamma, ns, c, n * segs, (double)n * hw, train);
    if (gx0) {
        const int64_t total = (int64_t)n * c * hw;
        aln_norm_bwd_kernel<<<dim3(aln_blocks(total)), dim3(256), 0, st>>>(AlnDst2{gx0, gx1, gx1 ? gsplit : c, gx1 ? c - gsplit : 0}, gy, src, add0, add1, coef,
                                                                           c, hw, total, train);
    }
    return check_launch("aln(norm_bwd)");
}

// ---- PReLU backward -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) aln_prelu_bwd_kernel(float* __restrict__ gx, double* __restrict__ part, const float* __restrict__ gy,
                                                            const float* __restrict__ pre, const float2* __restrict__ pre_ab, const float* __restrict__ slope, int C,
                                                            int hw) {
    const int c = blockIdx.z;
    const float2 e = pre_ab ? pre_ab[c] : make_float2(1.0f, 0.0f);     // the stem's PReLU follows its BatchNorm: the forward's own a v + b
    const int64_t base = ((int64_t)blockIdx.y * C + c) * hw;
    const float sl = slope[c];
    const int end = min(hw, (int)(blockIdx.x + 1) * kAlnSeg);
    double s = 0.0;
    for (int i = blockIdx.x * kAlnSeg + threadIdx.x; i < end; i += 256) {
        const float g = gy[base + i], v = pre_ab ? __fmaf_rn(e.x, pre[base + i], e.y) : pre[base + i];
        if (gx) gx[base + i] = v > 0.0f ? g : __fmul_rn(sl, g);
        if (!(v > 0.0f)) s = fma((double)g, (double)v, s);
    }
    if (part) aln_block_sum2(s, 0.0, aln_partial(part));
}

__global__ void __launch_bounds__(64) aln_prelu_fold_kernel(float* __restrict__ dslope, const double* __restrict__ part, int C, int count) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double s, unused;
    aln_fold(part, c, count, s, unused);
    dslope[c] = (float)s;
}

// pre_ab: the affine under which `pre` was the PReLU's input (NULL: pre itself); ws (aln_norm_ws_bytes) is read only with dslope
static int aln_prelu_bwd(float* gx, float* dslope, const float* gy, const float* pre, const float* pre_ab, const float* slope, double* ws, int n, int c,
                         int hw, hipStream_t st) {
    const int segs = aln_segments(hw);
    aln_prelu_bwd_kernel<<<dim3(segs, n, c), dim3(256), 0, st>>>(gx, dslope ? ws : nullptr, gy, pre, reinterpret_cast<const float2*>(pre_ab), slope, c, hw);
    if (dslope) aln_prelu_fold_kernel<<<dim3((c + 63) / 64), dim3(64), 0, st>>>(dslope, ws, c, n * segs);
    return check_launch("aln(prelu_bwd)");
}

// ---- adjoint of aln_up2_kernel --------------------------------------------------------------------------------------------------------------
// The weight output row / column o puts on input index i: l0 where its first tap is i, plus l1 where its second is (both at a clamped edge).
__device__ __forceinline__ double aln_up2_weight(int o, int in, int i) {
    int i0, i1;
    float l0, l1;
    aln_up2_tap(o, in, i0, i1, l0, l1);
    return (i0 == i ? (double)l0 : 0.0) + (i1 == i ? (double)l1 : 0.0);
}

__global__ void __launch_bounds__(256) aln_up2_bwd_kernel(float* __restrict__ gx, const float* __restrict__ gy, int H, int W, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int HW = H * W, OW = 2 * W;
    const int64_t plane = i / HW;
    const int pix = (int)(i - plane * HW), y = pix / W, x = pix - y * W;
    const float* __restrict__ g = gy + plane * 4 * HW;
    const int oy0 = max(2 * y - 2, 0), oy1 = min(2 * y + 2, 2 * H - 1), ox0 = max(2 * x - 2, 0), ox1 = min(2 * x + 2, OW - 1);
    double sum = 0.0;
    for (int oy = oy0; oy <= oy1; ++oy) {
        const double wy = aln_up2_weight(oy, H, y);
        if (wy == 0.0) continue;
        double row = 0.0;
        for (int ox = ox0; ox <= ox1; ++ox) row = fma(aln_up2_weight(ox, W, x), (double)g[oy * OW + ox], row);
        sum = fma(wy, row, sum);
    }
    gx[i] = (float)sum;
}

static int aln_up2_bwd(float* gx, const float* gy, int64_t planes, int h, int w, hipStream_t st) {   // h, w: gx's plane
    const int64_t total = planes * h * w;
    aln_up2_bwd_kernel<<<dim3(aln_blocks(total)), dim3(256), 0, st>>>(gx, gy, h, w, total);
    return check_launch("aln(up2_bwd)");
}

// ---- adjoint of the strided pick ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) aln_pick_bwd_kernel(float* __restrict__ gx, const float* __restrict__ gy, const float* __restrict__ add,
                                                           int H, int W, int OH, int OW, int stride, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int HW = H * W;
    const int64_t plane = i / HW;
    const int pix = (int)(i - plane * HW), y = pix / W, x = pix - y * W;
    float v = 0.0f;
    if (y % stride == 0 && x % stride == 0) v = gy[(plane * OH + y / stride) * OW + x / stride];
    gx[i] = add ? __fadd_rn(add[i], v) : v;
}

static int aln_pick_bwd(float* gx, const float* gy, const float* add, int64_t planes, int h, int w, int stride, hipStream_t st) {   // h, w: gx's plane
    const int64_t total = planes * h * w;
    aln_pick_bwd_kernel<<<dim3(aln_blocks(total)), dim3(256), 0, st>>>(gx, gy, add, h, w, (h - 1) / stride + 1, (w - 1) / stride + 1, stride, total);
    return check_launch("aln(pick_bwd)");
}

// ---- data gradient of a convolution -----------------------------------------------------------------------------------------------------------
// gx[ci][y][x] = sum over (co, r, s) of W[co][ci][r][s] g[co][(y + PAD - r) / stride][(x + PAD - s) / stride]: aln_conv_kernel's GEMM (aln_k_loop,
// the waves side by side along the pixels) on the transposed, tap-flipped image (ig_pack_t), M = Cin, K = (co, r', s') with r' = KS - 1 - r,
// N = the pixels of the convolution's INPUT.  The gather reads g at (y - PAD + r', x - PAD + s') / stride; stride 2 is a parity predicate on
// that position.  A launch covers up to four channel tiles from tile m0 on (Cin = 112 has seven: two launches, 4 + 3).  Epilogue: the sum of
// the two chains plus up to two fan-in addends in that order (the leading BatchNorm's factor is aln_norm_bwd_kernel's, in both forms).
struct AlnDgradArgs {
    float* gx; float* gx1; const float* g; const float* wfrag; const float* add0; const float* add1;
    int Cin, IH, IW, Cout, OH, OW, K, KS4, tiles, stride, m0, gsplit;   // gx1: channels from gsplit on go to a second tensor (NULL: gsplit = Cin)
};

template <int KS_, int MT, int NT>
__global__ void __launch_bounds__(256) aln_dgrad_kernel(AlnDgradArgs a) {
    constexpr int BN = AlnTile<NT>::BN, ROWS = AlnTile<NT>::ROWS, PER = AlnTile<NT>::PER;
    constexpr int PAD = KS_ == 3 ? 1 : 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int IHW = a.IH * a.IW, OH = a.OH, OW = a.OW, K = a.K, par = a.stride - 1;     // stride 1 or 2: a shift and a mask
    const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
    const int sn = tid % BN, srow = tid / BN;
    const int spix = tile * BN + sn;
    const bool n_ok = spix < IHW;
    const int sy = spix / a.IW, sx = spix - sy * a.IW;
    const float* __restrict__ src = a.g + (int64_t)img * a.Cout * OH * OW;
    auto fetch = [&](int k0, float (&v)[PER]) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = k0 + srow + i * ROWS;
            const auto [co, r, s] = ig_decode<KS_>(k);
            const int ty = sy - PAD + r, tx = sx - PAD + s;
            float x = 0.0f;
            if (n_ok && k < K && ty >= 0 && tx >= 0 && ((ty | tx) & par) == 0) {
                const int oy = ty >> par, ox = tx >> par;
                if (oy < OH && ox < OW) x = src[((int64_t)co * OH + oy) * OW + ox];
            }
            v[i] = x;
        }
    };
    f32x4 acc[MT][NT][2];
    aln_k_loop<MT, NT>(acc, a.wfrag + (int64_t)a.m0 * a.KS4 * 64 + lane, a.KS4, a.KS4 / (kIgKC / 4), fetch);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int pix = tile * BN + wave * 16 * NT + t * 16 + (lane & 15);
        if (pix >= IHW) continue;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = (a.m0 + m) * 16 + 4 * (lane >> 4) + r;
                if (row >= a.Cin) continue;
                float v = __fadd_rn(acc[m][t][0][r], acc[m][t][1][r]);
                const int64_t at = ((int64_t)img * a.Cin + row) * IHW + pix;
                if (a.add0) v = __fadd_rn(v, a.add0[at]);
                if (a.add1) v = __fadd_rn(v, a.add1[at]);
                if (row < a.gsplit) a.gx[((int64_t)img * a.gsplit + row) * IHW + pix] = v;
                else a.gx1[((int64_t)img * (a.Cin - a.gsplit) + (row - a.gsplit)) * IHW + pix] = v;
            }
        }
    }
}

struct AlnDgrad {
    float* gx; const float* g; const float* wfrag_t; const float* add0; const float* add1;
    int n, cin, cout, h, w, ks, stride;                              // h, w: the convolution's input, gx's plane
    float* gx1 = nullptr; int gsplit = 0;                            // a split destination (the stem's d res_gt | d thumb)
};

static int aln_dgrad(const AlnDgrad& c, hipStream_t st) {
    AlnDgradArgs a;
    a.gx = c.gx; a.gx1 = c.gx1; a.gsplit = c.gx1 ? c.gsplit : c.cin; a.g = c.g; a.wfrag = c.wfrag_t; a.add0 = c.add0; a.add1 = c.add1;
    a.Cin = c.cin; a.IH = c.h; a.IW = c.w; a.Cout = c.cout; a.OH = aln_out_size(c.h, c.ks, c.stride); a.OW = aln_out_size(c.w, c.ks, c.stride);
    a.K = c.cout * c.ks * c.ks; a.KS4 = ig_kpad(a.K) / 4; a.stride = c.stride;
    const int IHW = c.h * c.w, nt = aln_tile_width(IHW), bn = 64 * nt, tiles_m = ig_mpad(c.cin) / 16;
    a.tiles = (IHW + bn - 1) / bn;
    const dim3 grid((unsigned)((int64_t)c.n * a.tiles));
    for (int m0 = 0; m0 < tiles_m; m0 += 4) {
        a.m0 = m0;
        const int mt = tiles_m - m0 < 4 ? tiles_m - m0 : 4;
        auto with_mt = [&](auto ks_c, auto nt_c) {
            constexpr int KS_ = decltype(ks_c)::value, NT = decltype(nt_c)::value;
            if (mt == 1) aln_dgrad_kernel<KS_, 1, NT><<<grid, dim3(256), 0, st>>>(a);
            else if (mt == 2) aln_dgrad_kernel<KS_, 2, NT><<<grid, dim3(256), 0, st>>>(a);
            else if (mt == 3) aln_dgrad_kernel<KS_, 3, NT><<<grid, dim3(256), 0, st>>>(a);
            else aln_dgrad_kernel<KS_, 4, NT><<<grid, dim3(256), 0, st>>>(a);
        };
        auto with_nt = [&](auto ks_c) {
            if (nt == 2) with_mt(ks_c, std::integral_constant<int, 2>{});
            else with_mt(ks_c, std::integral_constant<int, 1>{});
        };
        if (c.ks == 3) with_nt(std::integral_constant<int, 3>{});
        else with_nt(std::integral_constant<int, 1>{});
    }
    return check_launch("aln(dgrad)");
}

// ---- weight gradient of a convolution -----------------------------------------------------------------------------------------------------------
// dW[co][k] = sum over images and output pixels of g[co][pix] B[k][pix], k = (ci, r, s), B the forward's own gather (zero padding, a x + b on
// in-image elements only, both sources, the x4 read).  GEMM on v_mfma_f32_16x16x4_f32 with M = Cout, N = the k columns, and the pixels as the
// reduction: a workgroup owns one (image, segment of kAlnWgSeg pixels), 64 k columns (16 per wave) and all MT channel tiles; it stages 32
// pixels of g (A) and of the gather (B) per pass in LDS, the next pass's loads in flight during the matrix steps, two accumulator chains per
// element (even / odd groups of four pixels), each ascending.  The partials (float32, one per image and segment) are folded in float64,
// images then segments ascending, into the parameter's own shape by aln_wgrad_fold_kernel.  The split comes from the layer's shape alone.
constexpr int kAlnWgSeg = 1024, kAlnWgCols = 64, kAlnWgAP = kIgKC + 1, kAlnWgBP = kAlnWgCols + 1;

static int aln_wgrad_segments(int ohw) { return (ohw + kAlnWgSeg - 1) / kAlnWgSeg; }

struct AlnWgradArgs {
    float* part; const float* g; const float* in0; const float* in1; const float2* in_ab;
    int C0, C1, IH, IW, Cout, OH, OW, K, stride, up4;
};

template <int KS_, int MT>
__global__ void __launch_bounds__(256) aln_wgrad_kernel(AlnWgradArgs a) {
    constexpr int PAD = KS_ == 3 ? 1 : 0, AROWS = 2 * MT, BCOLS = kAlnWgCols / 8;       // staged elements per thread and pass: rows of g, columns of B
    __shared__ float as[MT * 16 * kAlnWgAP];
    __shared__ float bs[kIgKC * kAlnWgBP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int OHW = a.OH * a.OW, IH = a.IH, IW = a.IW, C0 = a.C0, K = a.K;
    const int col0 = blockIdx.x * kAlnWgCols, seg = blockIdx.y, img = blockIdx.z;
    const int p_begin = seg * kAlnWgSeg, p_end = min(OHW, p_begin + kAlnWgSeg);
    const int sp = tid & 31, sr = tid >> 5;                          // this thread's pixel of a pass, and its first row / column
    const int H1 = a.up4 ? IH >> 2 : IH, W1 = a.up4 ? IW >> 2 : IW, sh1 = a.up4 ? 2 : 0;
    const float* __restrict__ g = a.g + (int64_t)img * a.Cout * OHW;
    const float* __restrict__ src0 = a.in0 + (int64_t)img * C0 * IH * IW;
    const float* __restrict__ src1 = a.in1 + (int64_t)img * a.C1 * H1 * W1;          // (never read when C1 == 0)
    const float2* __restrict__ in_ab = a.in_ab;
    float ga[AROWS], xb[BCOLS];
    auto fetch = [&](int p0) {
        const int pix = p0 + sp;
        const bool ok = pix < p_end;
        const int oy = pix / a.OW, ox = pix - oy * a.OW;
        const int iy0 = oy * a.stride - PAD, ix0 = ox * a.stride - PAD;
#pragma unroll
        for (int i = 0; i < AROWS; ++i) {
            const int co = sr + 8 * i;
            ga[i] = ok && co < a.Cout ? g[(int64_t)co * OHW + pix] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < BCOLS; ++i) {
            const int k = col0 + sr + 8 * i;
            const auto [ci, r, s] = ig_decode<KS_>(k);
            const int iy = iy0 + r, ix = ix0 + s;
            float x = 0.0f;
            if (ok && k < K && iy >= 0 && iy < IH && ix >= 0 && ix < IW) {
                x = ci < C0 ? src0[((int64_t)ci * IH + iy) * IW + ix] : src1[((int64_t)(ci - C0) * H1 + (iy >> sh1)) * W1 + (ix >> sh1)];
                if (in_ab) { const float2 ab = in_ab[ci]; x = __fmaf_rn(ab.x, x, ab.y); }   // the leading BN; padding stays 0
            }
            xb[i] = x;
        }
    };
    f32x4 acc[MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m][0] = acc[m][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    fetch(p_begin);
#pragma unroll 1
    for (int p0 = p_begin; p0 < p_end; p0 += kIgKC) {
        __syncthreads();                                            // the previous pass's reads are done
#pragma unroll
        for (int i = 0; i < AROWS; ++i) as[(sr + 8 * i) * kAlnWgAP + sp] = ga[i];
#pragma unroll
        for (int i = 0; i < BCOLS; ++i) bs[sp * kAlnWgBP + sr + 8 * i] = xb[i];
        __syncthreads();
        if (p0 + kIgKC < p_end) fetch(p0 + kIgKC);                  // in flight during the MFMAs
#pragma unroll
        for (int j = 0; j < kIgKC / 4; ++j) {
            const float b = bs[(j * 4 + (lane >> 4)) * kAlnWgBP + wave * 16 + (lane & 15)];
#pragma unroll
            for (int m = 0; m < MT; ++m)
                acc[m][j & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[(m * 16 + (lane & 15)) * kAlnWgAP + j * 4 + (lane >> 4)], b, acc[m][j & 1], 0, 0, 0);
        }
    }
    // C/D fragment: lane l, register r holds D[4 (l >> 4) + r][l & 15]
    const int k = col0 + wave * 16 + (lane & 15);
    if (k >= K) return;
    float* __restrict__ part = a.part + ((int64_t)img * gridDim.y + seg) * a.Cout * K;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = m * 16 + 4 * (lane >> 4) + r;
            if (co < a.Cout) part[(int64_t)co * K + k] = __fadd_rn(acc[m][0][r], acc[m][1][r]);
        }
}

__global__ void __launch_bounds__(256) aln_wgrad_fold_kernel(float* __restrict__ dw, const float* __restrict__ part, int count, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    double s = 0.0;
#pragma unroll 8                                                    // the loads of eight partials in flight; the additions stay in order
    for (int p = 0; p < count; ++p) s += (double)part[(int64_t)p * total + i];
    dw[i] = (float)s;
}

struct AlnWgrad {
    float* dw; const float* g; const float* in0; const float* in1; const float* in_ab; float* ws;
    int n, cin, split, up4, cout, h, w, ks, stride;
};

static int64_t aln_wgrad_ws_floats(int64_t n, int cin, int cout, int h, int w, int ks, int stride) {
    return n * aln_wgrad_segments(aln_out_size(h, ks, stride) * aln_out_size(w, ks, stride)) * cout * cin * ks * ks;
}

static int aln_wgrad(const AlnWgrad& c, hipStream_t st) {
    AlnWgradArgs a;
    a.part = c.ws; a.g = c.g; a.in0 = c.in0; a.in1 = c.in1; a.in_ab = reinterpret_cast<const float2*>(c.in_ab);
    a.C0 = c.split; a.C1 = c.cin - c.split; a.IH = c.h; a.IW = c.w; a.Cout = c.cout;
    a.OH = aln_out_size(c.h, c.ks, c.stride); a.OW = aln_out_size(c.w, c.ks, c.stride);
    a.K = c.cin * c.ks * c.ks; a.stride = c.stride; a.up4 = c.up4;
    const int segs = aln_wgrad_segments(a.OH * a.OW), mt = ig_mpad(c.cout) / 16;
    const dim3 grid((a.K + kAlnWgCols - 1) / kAlnWgCols, segs, c.n);
    auto with_mt = [&](auto ks_c) {
        constexpr int KS_ = decltype(ks_c)::value;
        if (mt == 1) aln_wgrad_kernel<KS_, 1><<<grid, dim3(256), 0, st>>>(a);
        else if (mt == 2) aln_wgrad_kernel<KS_, 2><<<grid, dim3(256), 0, st>>>(a);
        else if (mt == 3) aln_wgrad_kernel<KS_, 3><<<grid, dim3(256), 0, st>>>(a);
        else aln_wgrad_kernel<KS_, 4><<<grid, dim3(256), 0, st>>>(a);
    };
    if (c.ks == 3) with_mt(std::integral_constant<int, 3>{});
    else with_mt(std::integral_constant<int, 1>{});
    const int total = c.cout * a.K;
    aln_wgrad_fold_kernel<<<dim3((total + 255) / 256), dim3(256), 0, st>>>(c.dw, c.ws, c.n * segs, total);
    return check_launch("aln(wgrad)");
}

}  // namespace e3dge
