// Hourglass image filter of the local branch, backward (included at the end of hgfilter.hip): d outputs, d normx -> d input of HGFilter and,
// through the two front nets, d residual image and d depth map; with a gradient buffer also d of every parameter the forward reads.  Once
// differentiable, fp32.  Launch count, saved bytes, measured times and errors: DESIGN.md 4.15b.
//
// Kernels (no atomics, bit-reproducible; an image's gradient does not depend on the batch):
//   hgf_dgrad_kernel           data gradient of one convolution on ig_k_loop with the transposed, tap-flipped image (ig_pack_t): M = C_in,
//                              K = (c_out, r, s), waves past M idle.  g is read from a channel slice of a wider tensor (cat(o1, o2, o3) is
//                              never materialised).  Stride 2 (the stem) is a predicate on the parity of the tap's position.  Reflect
//                              padding's adjoint is extra mirrored taps in the gather: row 1 also receives what row 0 sent to row -1, row
//                              H - 2 what row H - 1 sent to row H; columns alike, corners from both.  Epilogue: the two chains' sum, times the
//                              ReLU branch of the leading norm recomputed as fmaf(a, x, b) > 0 (the forward gather's expression), plus an
//                              optional addend.
//   hgf_norm_bwd_stats_kernel  per (image, group), hgf_norm_kernel's fixed-stride, fixed-tree order: the moments again, then per channel
//                              P = sum g_y and Q = sum g_y xhat in float64; S1 = sum_c gamma_c P_c, S2 = sum_c gamma_c Q_c in ascending c.
//                              Writes per (image, channel) the float64 coefficients of  g_x = A g_y + B x + C,  A = gamma rstd,
//                              B = -rstd^2 S2 / m, C = -rstd (S1 - rstd mean S2) / m.  mean and rstd are never recovered from (a, b).
//   hgf_norm_bwd_apply_kernel  g_x = add1 + (add0 + fl(A g_y + B x + C)), the norm term in float64 and rounded once; add0 is a channel slice
//                              (the direct path through the concatenation or the residual), add1 a whole tensor (a second consumer).
//   hgf_pool_bwd_kernel        adjoint of avg_pool2d(2, 2), with an optional addend.
//   hgf_up_bwd_kernel          adjoint of the bicubic x2 as a gather over the low-resolution pixel: every up-sampled position whose taps,
//                              after clamping, name it, rows then columns ascending, the forward's own weights.
//   hgf_wgrad_kernel           weight gradient of one convolution: the same implicit GEMM turned on its side, M = c_out, N = (c_in, r, s),
//                              K = the pixels of ONE image.  A = g of that image in fragment order (hgf_pack_g_kernel: conv_pack_kernel's
//                              layout from the channel slice), B = the forward's own gather (zero padding or the mirror, the stem's stride
//                              on the pixel index, relu(a x + b) on in-image elements only).  K is split over images and segments of
//                              kHgfWgradSegTiles k tiles, from the layer's shape alone; the partials go to the workspace and
//                              hgf_wgrad_fold_kernel sums them in float64, images then segments ascending, and rounds once.
//   hgf_bias_grad_kernel       d bias = the plane sums of g, images ascending, float64, a fixed tree.
//   hgf_norm_param_kernel      d gamma = sum_img Q, d beta = sum_img P of the norm backward's statistics, images ascending, float64.
// Fan-in, every sum in this order:  ConvBlock input = (incoming + residual slice + bn1's term) + bn4's term;  o1, o2 = own slice + the next
// norm's term;  level input = b1_d's gradient + the pool's;  previous = through the hourglass + (`+ previous`, bl, al of the stack above:
// what the buffer held);  ll = l's + bl's;  stack output = the caller's + al's.
#pragma once

namespace e3dge {

struct HgfDgradArgs {
    float* out; const float* g; const float* wfrag; const float* x; const float2* ab; const float* addend; unsigned char* branch;
    int Cg_total, g_c0, Cg, GH, GW, M, H, W, K, KS4, tiles;
};

template <int KS_, int STRIDE, int NT, bool REFLECT>
__global__ void __launch_bounds__(256) hgf_dgrad_kernel(HgfDgradArgs a) {
    constexpr int BN = IgTile<NT>::BN, ROWS = IgTile<NT>::ROWS, PER = IgTile<NT>::PER;
    constexpr int PAD = KS_ / 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mt = blockIdx.y * (kIgBM / 16) + wave;
    const bool live = mt * 16 < a.M;                                 // wave-uniform: the 32 -> 3 and 32 -> 1 gradients have one live wave
    const int HW = a.H * a.W, GH = a.GH, GW = a.GW, K = a.K;
    const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
    const int sn = tid % BN, srow = tid / BN;
    const int spix = tile * BN + sn;
    const bool n_ok = spix < HW;
    const int sy = spix / a.W, sx = spix - sy * a.W;
    const int y0 = sy - PAD, x0 = sx - PAD;
    const float* __restrict__ src = a.g + ((int64_t)img * a.Cg_total + a.g_c0) * GH * GW;
    auto fetch = [&](int k0, float (&v)[PER]) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = k0 + srow + i * ROWS;
            const auto [co, r, s] = ig_decode<KS_>(k);
            const int ny = y0 + r, nx = x0 + s;
            float x = 0.0f;
            if (n_ok && k < K) {
                const float* __restrict__ p = src + (int64_t)co * GH * GW;
                if (REFLECT) {                                       // stride 1, pad 1: GH = H, GW = W >= 2
                    const int ya = ny >= 0 && ny < GH ? ny : -1, xa = nx >= 0 && nx < GW ? nx : -1;
                    const int yb = sy == 1 && r == 2 ? 0 : sy == GH - 2 && r == 0 ? GH - 1 : -1;
                    const int xb = sx == 1 && s == 2 ? 0 : sx == GW - 2 && s == 0 ? GW - 1 : -1;
                    if (ya >= 0 && xa >= 0) x = p[ya * GW + xa];
                    if (ya >= 0 && xb >= 0) x = __fadd_rn(x, p[ya * GW + xb]);
                    if (yb >= 0 && xa >= 0) x = __fadd_rn(x, p[yb * GW + xa]);
                    if (yb >= 0 && xb >= 0) x = __fadd_rn(x, p[yb * GW + xb]);
                } else {
                    bool ok = ny >= 0 && nx >= 0;
                    int gy = ny, gx = nx;
                    if (STRIDE == 2) { ok = ok && !((ny | nx) & 1); gy = ny >> 1; gx = nx >> 1; }
                    if (ok && gy < GH && gx < GW) x = p[gy * GW + gx];
                }
            }
            v[i] = x;
        }
    };
    f32x4 acc[NT][2];
    ig_k_loop<NT, 2, true>(acc, a.wfrag + (int64_t)(live ? mt : 0) * a.KS4 * 64 + lane, a.KS4 / (kIgKC / 4), live, fetch, [](int, bool) {});
    if (!live) return;
    const int row0 = mt * 16 + 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int pix = tile * BN + t * 16 + (lane & 15);
        if (pix >= HW) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + r;
            if (row >= a.M) continue;
            const int64_t at = ((int64_t)img * a.M + row) * HW + pix;
            float v = __fadd_rn(acc[t][0][r], acc[t][1][r]);
            if (a.x) {
                const float2 e = a.ab[(int64_t)img * a.M + row];
                const bool pass = __fmaf_rn(e.x, a.x[at], e.y) > 0.0f;
                if (!pass) v = 0.0f;
                if (a.branch) a.branch[at] = pass;                   // debug: the branch this run took, for a branch-pinned truth
            }
            if (a.addend) v = __fadd_rn(a.addend[at], v);
            a.out[at] = v;
        }
    }
}

// ---- norm backward ------------------------------------------------------------------------------------------------------------------
// coef[(img * C + c) * 3 + {0, 1, 2}] = (A, B, C) of g_x = A g_y + B x + C; g_y (n, C, HW) dense, x the channels [c0, c0 + C) of
// (n, C_total, HW).  mask_ab: g_y is first multiplied by the ReLU branch fmaf(a, x, b) > 0 (the stem's norm, whose activation tmpx is a
// tensor of its own and no convolution's gather).
__global__ void __launch_bounds__(kHgfNormThreads) hgf_norm_bwd_stats_kernel(double* __restrict__ coef, double* __restrict__ pq, const float* __restrict__ gy,
                                                                            const float* __restrict__ x,
                                                                            const float* __restrict__ gamma, const float2* __restrict__ mask_ab, int C_total,
                                                                            int c0, int C, int groups, int HW) {
    __shared__ double s1[kHgfNormThreads], s2[kHgfNormThreads];
    __shared__ double sp[256], sq[256];
    const int tid = threadIdx.x, img = blockIdx.x / groups, g = blockIdx.x - img * groups;
    const int cpg = C / groups;
    const int64_t count = (int64_t)cpg * HW;
    const float* __restrict__ p = x + ((int64_t)img * C_total + c0 + (int64_t)g * cpg) * HW;
    double a1 = 0.0, a2 = 0.0;
    for (int64_t i0 = tid; i0 < count; i0 += kHgfNormThreads * kHgfNormUnroll) {      // the forward's moments, in the forward's order
        float v[kHgfNormUnroll];
#pragma unroll
        for (int u = 0; u < kHgfNormUnroll; ++u) {
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
    __syncthreads();
    for (int j = 0; j < cpg; ++j) {                                   // P and Q of channel j of the group
        const int c = g * cpg + j;
        const float* __restrict__ px = p + (int64_t)j * HW;
        const float* __restrict__ pg = gy + ((int64_t)img * C + c) * HW;
        float2 e = make_float2(0.0f, 0.0f);
        if (mask_ab) e = mask_ab[(int64_t)img * C + c];
        a1 = a2 = 0.0;
        for (int i = tid; i < HW; i += kHgfNormThreads) {
            const float xv = px[i];
            float gv = pg[i];
            if (mask_ab && !(__fmaf_rn(e.x, xv, e.y) > 0.0f)) gv = 0.0f;
            a1 += (double)gv;
            a2 = fma((double)gv, ((double)xv - mean) * rstd, a2);
        }
        s1[tid] = a1; s2[tid] = a2;
        __syncthreads();
        for (int off = kHgfNormThreads / 2; off > 0; off >>= 1) {
            if (tid < off) { s1[tid] += s1[tid + off]; s2[tid] += s2[tid + off]; }
            __syncthreads();
        }
        if (tid == 0) { sp[j] = s1[0]; sq[j] = s2[0]; }
        __syncthreads();
    }
    if (tid < cpg) {
        double S1 = 0.0, S2 = 0.0;
        for (int j = 0; j < cpg; ++j) {
            const double gm = (double)gamma[g * cpg + j];
            S1 = fma(gm, sp[j], S1);
            S2 = fma(gm, sq[j], S2);
        }
        const int c = g * cpg + tid;
        double* __restrict__ o = coef + ((int64_t)img * C + c) * 3;
        const double m = (double)count;
        o[0] = (double)gamma[c] * rstd;
        o[1] = -rstd * rstd * S2 / m;
        o[2] = -rstd * (S1 - rstd * mean * S2) / m;
        if (pq) { pq[((int64_t)img * C + c) * 2] = sp[tid]; pq[((int64_t)img * C + c) * 2 + 1] = sq[tid]; }
    }
}

// gx may be gy or add1
__global__ void __launch_bounds__(256) hgf_norm_bwd_apply_kernel(float* gx, const float* gy, const float* __restrict__ x, const double* __restrict__ coef,
                                                                const float2* __restrict__ mask_ab, const float* __restrict__ add0, int add0_C, int add0_c0,
                                                                const float* add1, unsigned char* __restrict__ branch, int C_total, int c0, int C, int HW,
                                                                int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t plane = i / HW;
    const int pix = (int)(i - plane * HW);
    const int64_t img = plane / C;
    const int c = (int)(plane - img * C);
    const float xv = x[((int64_t)img * C_total + c0 + c) * HW + pix];
    float gv = gy[i];
    if (mask_ab) {
        const float2 e = mask_ab[plane];
        const bool pass = __fmaf_rn(e.x, xv, e.y) > 0.0f;
        if (!pass) gv = 0.0f;
        if (branch) branch[i] = pass;
    }
    const double* __restrict__ k = coef + plane * 3;
    float v = (float)fma(k[0], (double)gv, fma(k[1], (double)xv, k[2]));
    if (add0) v = __fadd_rn(add0[((int64_t)img * add0_C + add0_c0 + c) * HW + pix], v);
    if (add1) v = __fadd_rn(add1[i], v);
    gx[i] = v;
}

// ---- pooling and up-sampling, adjoints ------------------------------------------------------------------------------------------------
// gin (planes, H, W) = addend + 0.25 gout (planes, H / 2, W / 2)[y / 2][x / 2]; gin may be addend
__global__ void __launch_bounds__(256) hgf_pool_bwd_kernel(float* gin, const float* __restrict__ gout, const float* addend, int H, int W, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const int64_t plane = i / ((int64_t)W * H);
    float v = __fmul_rn(gout[(plane * (H / 2) + (y >> 1)) * (W / 2) + (x >> 1)], 0.25f);
    if (addend) v = __fadd_rn(addend[i], v);
    gin[i] = v;
}

// the weight with which low-resolution index `want` enters up-sampled index o (hgf_up_add_kernel's own expressions); false: it does not
__device__ __forceinline__ bool hgf_up_weight(int o, int want, int L, float scale, float& wsum) {
    const float rp = __fmul_rn(scale, (float)o);
    int i0 = (int)floorf(rp);
    i0 = i0 < L - 1 ? i0 : L - 1;
    const float t = fminf(fmaxf(__fsub_rn(rp, (float)i0), 0.0f), 1.0f);
    float w[4];
    hgf_cubic(t, w);
    bool any = false;
    wsum = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int ii = i0 - 1 + j;
        ii = ii < 0 ? 0 : ii > L - 1 ? L - 1 : ii;
        if (ii == want) { wsum = any ? __fadd_rn(wsum, w[j]) : w[j]; any = true; }
    }
    return any;
}

// the up-sampled indices that can name low-resolution index i: those whose first tap index floor(scale o) lies in [i - 2, i + 2], widened by 2
__device__ __forceinline__ void hgf_up_range(int i, int L, float scale, int& lo, int& hi) {
    lo = 0; hi = 2 * L - 1;
    if (scale > 0.0f) {
        const int a = (int)floorf((float)(i - 2) / scale) - 2, b = (int)ceilf((float)(i + 2) / scale) + 2;
        lo = a > lo ? a : lo; hi = b < hi ? b : hi;
    }
}

// glow (planes, H, W) = adjoint of bicubic_x2 applied to g (planes, 2 H, 2 W)
__global__ void __launch_bounds__(256) hgf_up_bwd_kernel(float* __restrict__ glow, const float* __restrict__ g, int H, int W, float scale_y, float scale_x,
                                                         int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int lx = (int)(i % W), ly = (int)((i / W) % H);
    const int64_t plane = i / ((int64_t)W * H);
    const float* __restrict__ p = g + plane * 4 * H * W;
    int ylo, yhi, xlo, xhi;
    hgf_up_range(ly, H, scale_y, ylo, yhi);
    hgf_up_range(lx, W, scale_x, xlo, xhi);
    float acc = 0.0f;
    for (int oy = ylo; oy <= yhi; ++oy) {
        float wy;
        if (!hgf_up_weight(oy, ly, H, scale_y, wy)) continue;
        float row = 0.0f;
        for (int ox = xlo; ox <= xhi; ++ox) {
            float wx;
            if (hgf_up_weight(ox, lx, W, scale_x, wx)) row = __fmaf_rn(wx, p[(int64_t)oy * 2 * W + ox], row);
        }
        acc = __fmaf_rn(wy, row, acc);
    }
    glow[i] = acc;
}

// ---- parameter gradients ----------------------------------------------------------------------------------------------------------------
// dgamma[c] = sum_img Q, dbeta[c] = sum_img P; pq (n, C, 2) float64
__global__ void __launch_bounds__(256) hgf_norm_param_kernel(float* __restrict__ dgamma, float* __restrict__ dbeta, const double* __restrict__ pq, int n, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double P = 0.0, Q = 0.0;
    for (int img = 0; img < n; ++img) { P += pq[((int64_t)img * C + c) * 2]; Q += pq[((int64_t)img * C + c) * 2 + 1]; }
    dgamma[c] = (float)Q;
    dbeta[c] = (float)P;
}

// db[c] = sum over images and pixels of g (n, C, HW); one workgroup per channel
__global__ void __launch_bounds__(256) hgf_bias_grad_kernel(float* __restrict__ db, const float* __restrict__ g, int n, int C, int HW) {
    __shared__ double sm[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    double a = 0.0;
    for (int img = 0; img < n; ++img) {
        const float* __restrict__ p = g + ((int64_t)img * C + c) * HW;
        for (int i = tid; i < HW; i += 256) a += (double)p[i];
    }
    sm[tid] = a;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) sm[tid] += sm[tid + off];
        __syncthreads();
    }
    if (tid == 0) db[c] = (float)sm[0];
}

// gfrag[img] = the A-fragment image (conv_igemm.h) of G[M][K] = g[img, g_c0 + m, k], K = the pixels, padded with zeros
__global__ void __launch_bounds__(256) hgf_pack_g_kernel(float* __restrict__ gfrag, const float* __restrict__ g, int Cg_total, int g_c0, int M, int K, int KS4,
                                                         int64_t per_img, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t img = i / per_img, j = i - img * per_img;
    const int lane = (int)(j & 63);
    const int64_t t = j >> 6;
    const int ks = (int)(t % KS4), mt = (int)(t / KS4);
    const int row = mt * 16 + (lane & 15), k = ks * 4 + (lane >> 4);
    gfrag[i] = (row < M && k < K) ? g[((int64_t)img * Cg_total + g_c0 + row) * K + k] : 0.0f;
}

constexpr int kHgfWgradNT = 4;                                       // 64 columns (c_in, r, s) per workgroup
constexpr int kHgfWgradSegTiles = 64;                                // k tiles (2048 pixels) per segment

struct HgfWgradArgs {
    float* part; const float* gfrag; const float* x; const float2* ab;
    int Cin, IH, IW, Cout, OW, OHW, N, KS4, tilesN, segs, k_tiles;
    int64_t per_img;
};

// part[(img * segs + seg)][c_out][(c_in, r, s)] = sum over the segment's pixels of g[c_out, pix] * act(x)[c_in, pix + tap]
template <int KS_, int STRIDE, bool REFLECT>
__global__ void __launch_bounds__(256) hgf_wgrad_kernel(HgfWgradArgs a) {
    constexpr int NT = kHgfWgradNT, BN = IgTile<NT>::BN, ROWS = IgTile<NT>::ROWS, PER = IgTile<NT>::PER;
    constexpr int PAD = KS_ / 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mt = blockIdx.y * (kIgBM / 16) + wave;
    const bool live = mt * 16 < a.Cout;
    const int IH = a.IH, IW = a.IW, OHW = a.OHW;
    const int tile = blockIdx.x % a.tilesN, is = blockIdx.x / a.tilesN, img = is / a.segs, seg = is - img * a.segs;
    const int sn = tid % BN, srow = tid / BN;
    const int col = tile * BN + sn;
    const bool n_ok = col < a.N;
    const IgTap tap = ig_decode<KS_>(col);
    const int ci = tap.c, tr = tap.r, ts = tap.s;
    const float* __restrict__ src = a.x + ((int64_t)img * a.Cin + ci) * IH * IW;
    float2 e = make_float2(0.0f, 0.0f);
    if (a.ab && n_ok) e = a.ab[(int64_t)img * a.Cin + ci];
    const int kbase = seg * kHgfWgradSegTiles * kIgKC;
    const int left = a.k_tiles - seg * kHgfWgradSegTiles, n_tiles = left < kHgfWgradSegTiles ? left : kHgfWgradSegTiles;
    auto fetch = [&](int k0, float (&v)[PER]) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = kbase + k0 + srow + i * ROWS;
            const int oy = k / a.OW, ox = k - oy * a.OW;
            int iy = oy * STRIDE - PAD + tr, ix = ox * STRIDE - PAD + ts;
            if (REFLECT) {
                iy = iy < 0 ? -iy : iy >= IH ? 2 * IH - 2 - iy : iy;
                ix = ix < 0 ? -ix : ix >= IW ? 2 * IW - 2 - ix : ix;
            }
            float x = 0.0f;
            if (n_ok && k < OHW && iy >= 0 && iy < IH && ix >= 0 && ix < IW) {
                x = src[(int64_t)iy * IW + ix];
                if (a.ab) x = fmaxf(__fmaf_rn(e.x, x, e.y), 0.0f);   // the forward's gather: a zero-padded tap stays 0
            }
            v[i] = x;
        }
    };
    f32x4 acc[NT][2];
    const float* wa = a.gfrag + (int64_t)img * a.per_img + ((int64_t)(live ? mt : 0) * a.KS4 + (int64_t)seg * kHgfWgradSegTiles * (kIgKC / 4)) * 64 + lane;
    ig_k_loop<NT, 2, true>(acc, wa, n_tiles, live, fetch, [](int, bool) {});
    if (!live) return;
    const int row0 = mt * 16 + 4 * (lane >> 4);
    float* __restrict__ out = a.part + (int64_t)is * a.Cout * a.N;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = tile * BN + t * 16 + (lane & 15);
        if (c >= a.N) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + r;
            if (row < a.Cout) out[(int64_t)row * a.N + c] = __fadd_rn(acc[t][0][r], acc[t][1][r]);
        }
    }
}

// dw[i] = the sum of the `parts` partials of element i, in ascending (image, segment) order, float64, rounded once
__global__ void __launch_bounds__(256) hgf_wgrad_fold_kernel(float* __restrict__ dw, const float* __restrict__ part, int parts, int64_t MN) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= MN) return;
    double s = 0.0;
    for (int p = 0; p < parts; ++p) s += (double)part[(int64_t)p * MN + i];
    dw[i] = (float)s;
}

// ---- host side: single steps ----------------------------------------------------------------------------------------------------------
// d in (n, cin, H, W) of a convolution (cin -> cout, ks, stride) from g = the channels [g_c0, g_c0 + cout) of (n, Cg_total, GH, GW)
struct HgfDgradCall {
    float* out; const float* g; const float* wfrag; const float* x; const float* ab; const float* addend;
    int n, cin, cout, Cg_total, g_c0, H, W, ks, stride, reflect;
    unsigned char* branch;
};

static int hgf_dgrad(const HgfDgradCall& c, hipStream_t st) {
    HgfDgradArgs a;
    a.out = c.out; a.g = c.g; a.wfrag = c.wfrag; a.x = c.x; a.ab = reinterpret_cast<const float2*>(c.ab); a.addend = c.addend; a.branch = c.x ? c.branch : nullptr;
    a.Cg_total = c.Cg_total; a.g_c0 = c.g_c0; a.Cg = c.cout; a.M = c.cin; a.H = c.H; a.W = c.W;
    a.GH = hgf_out_size(c.H, c.ks, c.stride); a.GW = hgf_out_size(c.W, c.ks, c.stride);
    a.K = c.cout * c.ks * c.ks; a.KS4 = ig_kpad(a.K) / 4;
    const int HW = c.H * c.W, nt = hgf_tile_width(HW, c.cin), bn = 16 * nt;
    a.tiles = (HW + bn - 1) / bn;
    const dim3 grid((unsigned)((int64_t)c.n * a.tiles), (unsigned)hgf_gy(c.cin));
    ig_dispatch_nt(nt, [&](auto nt_c) {
        constexpr int NT = decltype(nt_c)::value;
        if (c.ks == 7) hgf_dgrad_kernel<7, 2, NT, false><<<grid, dim3(256), 0, st>>>(a);
        else if (c.ks == 3 && c.reflect) hgf_dgrad_kernel<3, 1, NT, true><<<grid, dim3(256), 0, st>>>(a);
        else if (c.ks == 3) hgf_dgrad_kernel<3, 1, NT, false><<<grid, dim3(256), 0, st>>>(a);
        else hgf_dgrad_kernel<1, 1, NT, false><<<grid, dim3(256), 0, st>>>(a);
    });
    return check_launch("hgf(dgrad)");
}

static int hgf_norm_bwd(float* gx, const float* gy, const float* x, const float* gamma, const float* mask_ab, const float* add0, int add0_C, int add0_c0,
                        const float* add1, double* coef, int n, int C_total, int c0, int C, int groups, int HW, hipStream_t st,
                        unsigned char* branch = nullptr, float* dgamma = nullptr, float* dbeta = nullptr) {
    const float2* m = reinterpret_cast<const float2*>(mask_ab);
    double* pq = dgamma ? coef + (int64_t)n * C * 3 : nullptr;       // the coefficient buffer holds n * C * 5 float64
    hgf_norm_bwd_stats_kernel<<<dim3((unsigned)(n * groups)), dim3(kHgfNormThreads), 0, st>>>(coef, pq, gy, x, gamma, m, C_total, c0, C, groups, HW);
    int rc;
    if ((rc = check_launch("hgf(norm_bwd stats)"))) return rc;
    if (dgamma) {
        hgf_norm_param_kernel<<<dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st>>>(dgamma, dbeta, pq, n, C);
        if ((rc = check_launch("hgf(norm_bwd parameters)"))) return rc;
    }
    const int64_t total = (int64_t)n * C * HW;
    hgf_norm_bwd_apply_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(gx, gy, x, coef, m, add0, add0_C, add0_c0, add1, branch, C_total, c0, C,
                                                                                         HW, total);
    return check_launch("hgf(norm_bwd apply)");
}

// dw (cout, cin, ks, ks) of the convolution of hgf_conv from g = the channels [g_c0, g_c0 + cout) of (n, Cg_total, OH, OW) and its input x
struct HgfWgradCall {
    float* dw; const float* g; const float* x; const float* ab;
    int n, cin, cout, Cg_total, g_c0, H, W, ks, stride, reflect;
};
static int hgf_wgrad_segs(int OHW) { return (ig_kpad(OHW) / kIgKC + kHgfWgradSegTiles - 1) / kHgfWgradSegTiles; }
static int64_t hgf_wgrad_gfrag_floats(int64_t n, int cout, int OHW) { return n * ig_mpad(cout) * ig_kpad(OHW); }
static int64_t hgf_wgrad_part_floats(int64_t n, int cin, int cout, int ks, int OHW) { return n * hgf_wgrad_segs(OHW) * cout * cin * ks * ks; }

static int hgf_wgrad(const HgfWgradCall& c, float* gfrag, float* part, hipStream_t st) {
    HgfWgradArgs a;
    a.part = part; a.gfrag = gfrag; a.x = c.x; a.ab = reinterpret_cast<const float2*>(c.ab);
    a.Cin = c.cin; a.IH = c.H; a.IW = c.W; a.Cout = c.cout;
    const int OH = hgf_out_size(c.H, c.ks, c.stride);
    a.OW = hgf_out_size(c.W, c.ks, c.stride); a.OHW = OH * a.OW;
    a.N = c.cin * c.ks * c.ks; a.KS4 = ig_kpad(a.OHW) / 4; a.k_tiles = ig_kpad(a.OHW) / kIgKC;
    a.tilesN = (a.N + 16 * kHgfWgradNT - 1) / (16 * kHgfWgradNT); a.segs = hgf_wgrad_segs(a.OHW);
    a.per_img = (int64_t)ig_mpad(c.cout) * ig_kpad(a.OHW);
    int rc;
    const int64_t total = a.per_img * c.n;
    hgf_pack_g_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(gfrag, c.g, c.Cg_total, c.g_c0, c.cout, a.OHW, a.KS4, a.per_img, total);
    if ((rc = check_launch("hgf(wgrad pack)"))) return rc;
    const dim3 grid((unsigned)((int64_t)c.n * a.segs * a.tilesN), (unsigned)hgf_gy(c.cout));
    if (c.ks == 7) hgf_wgrad_kernel<7, 2, false><<<grid, dim3(256), 0, st>>>(a);
    else if (c.ks == 3 && c.reflect) hgf_wgrad_kernel<3, 1, true><<<grid, dim3(256), 0, st>>>(a);
    else if (c.ks == 3) hgf_wgrad_kernel<3, 1, false><<<grid, dim3(256), 0, st>>>(a);
    else hgf_wgrad_kernel<1, 1, false><<<grid, dim3(256), 0, st>>>(a);
    if ((rc = check_launch("hgf(wgrad)"))) return rc;
    const int64_t MN = (int64_t)c.cout * a.N;
    hgf_wgrad_fold_kernel<<<dim3((unsigned)((MN + 255) / 256)), dim3(256), 0, st>>>(c.dw, part, c.n * a.segs, MN);
    return check_launch("hgf(wgrad fold)");
}

static int hgf_bias_grad(float* db, const float* g, int n, int C, int HW, hipStream_t st) {
    hgf_bias_grad_kernel<<<dim3((unsigned)C), dim3(256), 0, st>>>(db, g, n, C, HW);
    return check_launch("hgf(bias grad)");
}

static int hgf_pool_bwd(float* gin, const float* gout, const float* addend, int64_t planes, int H, int W, hipStream_t st) {
    const int64_t total = planes * H * W;
    hgf_pool_bwd_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(gin, gout, addend, H, W, total);
    return check_launch("hgf(pool_bwd)");
}

// glow (planes, H, W) from g (planes, 2 H, 2 W)
static int hgf_up_bwd(float* glow, const float* g, int64_t planes, int H, int W, hipStream_t st) {
    const int64_t total = planes * H * W;
    const float sy = H > 1 ? (float)(H - 1) / (float)(2 * H - 1) : 0.0f, sx = W > 1 ? (float)(W - 1) / (float)(2 * W - 1) : 0.0f;
    hgf_up_bwd_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(glow, g, H, W, sy, sx, total);
    return check_launch("hgf(up_bwd)");
}

// ---- host side: the transposed image --------------------------------------------------------------------------------------------------
// ig_pack_t of every convolution of the layout, in the layout's entry order
struct HgfLayoutT { int64_t off[kHgfMaxEntries]; int64_t total; };

static void hgf_layout_t(const HgfLayout& l, HgfLayoutT* out) {
    int64_t off = 0;
    for (int i = 0; i < l.n_src; ++i) {
        const HgfEntry& e = l.e[i];
        out->off[i] = off;
        if (e.ks) off += ((int64_t)ig_mpad(e.cin) * ig_kpad(e.cout * e.ks * e.ks) + 63) / 64 * 64;
    }
    out->total = off;
}

// ---- host side: the gradient buffer ----------------------------------------------------------------------------------------------------
// One gradient per source tensor, in the order and the shapes of the source arrays, back to back
struct HgfGradLayout { int64_t off[kHgfMaxEntries]; int64_t filter_total, total; };

static void hgf_grad_layout(const HgfLayout& l, HgfGradLayout* out) {
    int64_t off = 0;
    for (int i = 0; i < l.n_src; ++i) {
        const HgfEntry& e = l.e[i];
        if (i == l.n_filter_src) out->filter_total = off;
        out->off[i] = off;
        off += e.ks ? (int64_t)e.cout * e.cin * e.ks * e.ks : e.len;
    }
    out->total = off;
}

// the pixels of every ConvBlock's planes, in the layout's order (see hgf_saved)
static void hgf_block_pixels(const HgfLayout& l, int S, int D, int64_t p2, int64_t p4, int64_t* hw) {
    hw[l.conv2] = p2; hw[l.conv3] = p4; hw[l.conv4] = p4;
    for (int s = 0; s < S; ++s) {
        int bi = l.stack[s].first_block;
        int64_t p = p4;
        for (int lv = D; lv >= 1; --lv, p /= 4) { hw[bi++] = p; hw[bi++] = p / 4; }
        p *= 4;
        hw[bi++] = p / 4;
        for (int lv = 1; lv <= D; ++lv, p *= 4) hw[bi++] = p / 4;
        hw[l.stack[s].top] = p4;
    }
}

// ---- host side: the debug branch bytes -------------------------------------------------------------------------------------------------
// One byte per element of every norm's input, 1 where this run's ReLU passed: the stem's norm, then bn1, bn2, bn3 (and bn4 where the
// block has a downsample) of every ConvBlock in the layout's order, then bn_end of every stack, then the two norms of either front net.
struct HgfBranch { int64_t stem, blk[kHgfMaxBlocks][4], end[kHgfMaxStack], front[2][2], filter_bytes, bytes; };

static void hgf_branch(int64_t n, int64_t H, int64_t W, int S, int D, const HgfLayout& l, HgfBranch* out) {
    HgfBranch& v = *out;
    int64_t off = 0;
    auto take = [&](int64_t bytes) { const int64_t at = off; off += (bytes + 255) / 256 * 256; return at; };
    const int64_t p2 = (H / 2) * (W / 2), p4 = (H / 4) * (W / 4);
    int64_t hw[kHgfMaxBlocks];
    hgf_block_pixels(l, S, D, p2, p4, hw);
    v.stem = take(n * 64 * p2);
    for (int bi = 0; bi < l.n_blocks; ++bi) {
        const HgfBlock& b = l.blocks[bi];
        v.blk[bi][0] = take(n * b.cin * hw[bi]); v.blk[bi][1] = take(n * (b.cout / 2) * hw[bi]); v.blk[bi][2] = take(n * (b.cout / 4) * hw[bi]);
        v.blk[bi][3] = b.down ? take(n * b.cin * hw[bi]) : -1;
    }
    for (int s = 0; s < S; ++s) v.end[s] = take(n * 256 * p4);
    v.filter_bytes = off;
    for (int f = 0; f < 2; ++f) { v.front[f][0] = take(n * 32 * H * W); v.front[f][1] = take(n * 32 * H * W); }
    v.bytes = off;
}

// ---- host side: the backward's workspace ----------------------------------------------------------------------------------------------
struct HgfBwdWs {
    int64_t coef, gy, gt1, gt2, g_prev, g_o, g_last, g_top, g_hg, g_c3, g_normx, g_c2, g_tmpx, g_stem, lv_a[kHgfMaxDepth + 1], lv_b[kHgfMaxDepth + 1];
    int64_t gfrag, part, f_gfrag, f_part;                             // the weight gradients': g in fragment order, the split-K partials
    int64_t f_coef, f_gy, f_g2, f_g1, filter_floats, front_floats;
};

static HgfBwdWs hgf_bwd_ws(int64_t n, int64_t H, int64_t W, int S, int D) {
    HgfBwdWs d{};
    int64_t off = 0;
    auto take = [&](int64_t floats) { const int64_t at = off; off += (floats + 63) / 64 * 64; return at; };
    const int64_t p2 = (H / 2) * (W / 2), p4 = (H / 4) * (W / 4), q = n * 256 * p4;
    d.coef = take(n * 256 * 5 * 2);                                   // float64: the (A, B, C) triples, then the (P, Q) pairs
    d.gy = take(q); d.gt1 = take(q); d.gt2 = take(q);                 // the widest: conv2's 64 channels at p2
    d.g_prev = take(q); d.g_o = take(q); d.g_last = take(q); d.g_top = take(q); d.g_hg = take(q);
    d.g_c3 = take(n * 128 * p4); d.g_normx = take(n * 128 * p4); d.g_c2 = take(n * 128 * p2); d.g_tmpx = take(n * 64 * p2); d.g_stem = take(n * 64 * p2);
    int64_t p = p4;
    for (int lv = D; lv >= 1; --lv, p /= 4) { d.lv_a[lv] = take(n * 256 * (p / 4)); d.lv_b[lv] = take(n * 256 * (p / 4)); }
    {                                                                 // the widest g image and the most partials of any convolution
        HgfLayout l;
        hgf_layout(S, D, &l);
        int64_t hw[kHgfMaxBlocks], gf = hgf_wgrad_gfrag_floats(n, 64, (int)p2), pt = hgf_wgrad_part_floats(n, 64, 64, 7, (int)p2);      // the stem
        hgf_block_pixels(l, S, D, p2, p4, hw);
        auto more = [&](int ci, int co, int ks, int64_t px) {
            const int64_t a = hgf_wgrad_gfrag_floats(n, co, (int)px), b = hgf_wgrad_part_floats(n, ci, co, ks, (int)px);
            gf = a > gf ? a : gf; pt = b > pt ? b : pt;
        };
        for (int bi = 0; bi < l.n_blocks; ++bi) {
            const HgfBlock& b = l.blocks[bi];
            more(b.cin, b.cout / 2, 3, hw[bi]); more(b.cout / 2, b.cout / 4, 3, hw[bi]); more(b.cout / 4, b.cout / 4, 3, hw[bi]);
            if (b.down) more(b.cin, b.cout, 1, hw[bi]);
        }
        more(256, 256, 1, p4);
        d.gfrag = take(gf); d.part = take(pt);
    }
    d.filter_floats = off;
    off = 0;
    d.f_coef = take(n * 32 * 5 * 2);
    d.f_gy = take(n * 32 * H * W); d.f_g2 = take(n * 32 * H * W); d.f_g1 = take(n * 32 * H * W);
    d.f_gfrag = take(hgf_wgrad_gfrag_floats(n, 32, (int)(H * W))); d.f_part = take(hgf_wgrad_part_floats(n, 32, 32, 3, (int)(H * W)));
    d.front_floats = off;
    return d;
}

struct HgfBwdRun {
    const float* P; const float* PT; const HgfLayout* lay; const HgfLayoutT* lt; const HgfSaved* sv; const float* saved; const HgfBwdWs* w; float* ws;
    hipStream_t st; int n;
    unsigned char* branch; const HgfBranch* bl;                       // debug: null, or where every norm's ReLU branches go
    float* grads; const HgfGradLayout* gl;                            // null (frozen), or the parameter gradients
    float* gr(int entry) const { return grads ? grads + gl->off[entry] : nullptr; }
    // the weight gradient beside a data gradient: the same g, the convolution's own input
    int wgrad(int entry, const float* g, const float* x, const float* ab, int cin, int cout, int Cg_total, int g_c0, int H, int W, int ks, int stride) const {
        if (!grads) return E3DGE_OK;
        return hgf_wgrad({grads + gl->off[entry], g, x, ab, n, cin, cout, Cg_total, g_c0, H, W, ks, stride, 0}, ws + w->gfrag, ws + w->part, st);
    }
    unsigned char* br(int64_t off) const { return branch && off >= 0 ? branch + off : nullptr; }
    const float* at(int entry) const { return P + lay->e[entry].off; }
    const float* wt(int entry) const { return PT + lt->off[entry]; }
    double* coef() const { return reinterpret_cast<double*>(ws + w->coef); }
};

// g_x (n, cin, H, W) = acc + d ConvBlock / d x applied to g_out (n, cout, H, W); acc: null, or what g_x receives from elsewhere (may be g_x)
static int hgf_block_bwd(const HgfBwdRun& r, int bi, const float* x, const float* g_out, float* g_x, const float* acc, int H, int W) {
    int rc;
    const HgfBlock& b = r.lay->blocks[bi];
    const HgfBlockBuf& k = r.sv->blk[bi];
    const int HW = H * W, co = b.cout, ci = b.cin, n = r.n;
    const float* t1 = r.saved + k.t1;
    const float* t2 = r.saved + k.t2;
    const float* ab[4] = {r.saved + k.ab[0], r.saved + k.ab[1], r.saved + k.ab[2], r.saved + k.ab[3]};
    float* gy = r.ws + r.w->gy;
    float* gt1 = r.ws + r.w->gt1;
    float* gt2 = r.ws + r.w->gt2;
    const int64_t* q = r.bl ? r.bl->blk[bi] : nullptr;
    unsigned char* br[4];
    for (int i = 0; i < 4; ++i) br[i] = q ? r.br(q[i]) : nullptr;
    if ((rc = hgf_dgrad({gy, g_out, r.wt(b.w[2]), t2, ab[2], nullptr, n, co / 4, co / 4, co, 3 * co / 4, H, W, 3, 1, 0, br[2]}, r.st))) return rc;
    if ((rc = r.wgrad(b.w[2], g_out, t2, ab[2], co / 4, co / 4, co, 3 * co / 4, H, W, 3, 1))) return rc;
    if ((rc = hgf_norm_bwd(gt2, gy, t2, r.at(b.bn[2]), nullptr, g_out, co, co / 2, nullptr, r.coef(), n, co / 4, 0, co / 4, 32, HW, r.st, nullptr, r.gr(b.bn[2]),
                           r.gr(b.bn[2] + 1))))
        return rc;
    if ((rc = r.wgrad(b.w[1], gt2, t1, ab[1], co / 2, co / 4, co / 4, 0, H, W, 3, 1))) return rc;
    if ((rc = hgf_dgrad({gy, gt2, r.wt(b.w[1]), t1, ab[1], nullptr, n, co / 2, co / 4, co / 4, 0, H, W, 3, 1, 0, br[1]}, r.st))) return rc;
    if ((rc = hgf_norm_bwd(gt1, gy, t1, r.at(b.bn[1]), nullptr, g_out, co, 0, nullptr, r.coef(), n, co / 2, 0, co / 2, 32, HW, r.st, nullptr, r.gr(b.bn[1]),
                           r.gr(b.bn[1] + 1))))
        return rc;
    if ((rc = r.wgrad(b.w[0], gt1, x, ab[0], ci, co / 2, co / 2, 0, H, W, 3, 1))) return rc;
    if ((rc = hgf_dgrad({gy, gt1, r.wt(b.w[0]), x, ab[0], nullptr, n, ci, co / 2, co / 2, 0, H, W, 3, 1, 0, br[0]}, r.st))) return rc;
    if ((rc = hgf_norm_bwd(g_x, gy, x, r.at(b.bn[0]), nullptr, b.down ? nullptr : g_out, co, 0, acc, r.coef(), n, ci, 0, ci, 32, HW, r.st, nullptr, r.gr(b.bn[0]),
                           r.gr(b.bn[0] + 1))))
        return rc;
    if (!b.down) return E3DGE_OK;
    if ((rc = r.wgrad(b.w[3], g_out, x, ab[3], ci, co, co, 0, H, W, 1, 1))) return rc;
    if ((rc = hgf_dgrad({gy, g_out, r.wt(b.w[3]), x, ab[3], nullptr, n, ci, co, co, 0, H, W, 1, 1, 0, br[3]}, r.st))) return rc;
    return hgf_norm_bwd(g_x, gy, x, r.at(b.bn[3]), nullptr, nullptr, 0, 0, g_x, r.coef(), n, ci, 0, ci, 32, HW, r.st, nullptr, r.gr(b.bn[3]), r.gr(b.bn[3] + 1));
}

static int hgf_level_blocks(int d) { return d > 1 ? 3 + hgf_level_blocks(d - 1) : 4; }

// g_inp = acc + d level / d inp applied to g_out, both (n, 256, H, W); w: the stack's saved buffers; first: the level's first block
static int hgf_level_bwd(const HgfBwdRun& r, const HgfWs& w, int d, int first, const float* inp, const float* g_out, float* g_inp, const float* acc,
                         int H, int W) {
    int rc;
    const float* pooled = r.saved + w.pooled[d];
    const float* low1 = r.saved + w.low1[d];
    const float* low2 = r.saved + w.low2[d];
    float* A = r.ws + r.w->lv_a[d];
    float* B = r.ws + r.w->lv_b[d];
    const int inner = d > 1 ? hgf_level_blocks(d - 1) : 1, b3 = first + 2 + inner, h = H / 2, v = W / 2;
    if ((rc = hgf_up_bwd(A, g_out, (int64_t)r.n * 256, h, v, r.st))) return rc;                        // d low3; d up1 is g_out itself
    if ((rc = hgf_block_bwd(r, b3, low2, A, B, nullptr, h, v))) return rc;                             // d low2
    if (d > 1) rc = hgf_level_bwd(r, w, d - 1, first + 2, low1, B, A, nullptr, h, v);
    else rc = hgf_block_bwd(r, first + 2, low1, B, A, nullptr, h, v);                                  // d low1
    if (rc) return rc;
    if ((rc = hgf_block_bwd(r, first + 1, pooled, A, B, nullptr, h, v))) return rc;                    // d pooled
    if ((rc = hgf_block_bwd(r, first, inp, g_out, g_inp, acc, H, W))) return rc;                       // through b1_d
    return hgf_pool_bwd(g_inp, B, g_inp, (int64_t)r.n * 256, H, W, r.st);
}

}  // namespace e3dge

using namespace e3dge;

extern "C" int64_t e3dge_hgf_saved_bytes(int n, int height, int width, int num_stack, int num_hourglass) {
    if (!hgf_config_ok(num_stack, num_hourglass) || !hgf_sizes_ok(n, height, width, num_hourglass)) {
        fail(E3DGE_ERR_INVALID_ARG, "hgf_saved_bytes: n=%d height=%d width=%d num_stack=%d num_hourglass=%d (sizes multiples of 4 * 2^num_hourglass)", n,
             height, width, num_stack, num_hourglass);
        return -1;
    }
    HgfLayout l;
    hgf_layout(num_stack, num_hourglass, &l);
    HgfSaved sv;
    hgf_saved(n, height, width, num_stack, num_hourglass, l, &sv);
    return sv.floats * (int64_t)sizeof(float);
}

extern "C" int e3dge_hgf_forward_saving(const E3dgeHgfArgs* args, void* saved, int64_t saved_bytes, e3dge_stream_t stream) {
    E3DGE_REQUIRE(saved, "hgf_forward_saving: null pointer (saved state)");
    return hgf_forward_impl(args, static_cast<float*>(saved), saved_bytes, stream);
}

extern "C" int e3dge_hgf_front_saving(const float* packed, const float* image, const float* depth, float* out, int n, int height, int width,
                                      int num_stack, int num_hourglass, void* ws, int64_t ws_bytes, void* saved, int64_t saved_bytes,
                                      e3dge_stream_t stream) {
    E3DGE_REQUIRE(saved, "hgf_front_saving: null pointer (saved state)");
    return hgf_front_impl(packed, image, depth, out, n, height, width, num_stack, num_hourglass, ws, ws_bytes, static_cast<float*>(saved), saved_bytes, stream);
}

extern "C" int64_t e3dge_hgf_packed_t_floats(int num_stack, int num_hourglass) {
    if (!hgf_config_ok(num_stack, num_hourglass)) {
        fail(E3DGE_ERR_INVALID_ARG, "hgf_packed_t_floats: num_stack=%d (1..%d) num_hourglass=%d (1..%d)", num_stack, kHgfMaxStack, num_hourglass, kHgfMaxDepth);
        return -1;
    }
    HgfLayout l;
    hgf_layout(num_stack, num_hourglass, &l);
    HgfLayoutT t;
    hgf_layout_t(l, &t);
    return t.total;
}

extern "C" int e3dge_hgf_pack_weights_t(float* packed_t, const float* const* filter_src, int n_filter_src, const float* const* front_src,
                                        int num_stack, int num_hourglass, e3dge_stream_t stream) {
    E3DGE_REQUIRE(packed_t && filter_src, "hgf_pack_weights_t: null pointer");
    E3DGE_REQUIRE(hgf_config_ok(num_stack, num_hourglass), "hgf_pack_weights_t: num_stack=%d (1..%d) num_hourglass=%d (1..%d)", num_stack, kHgfMaxStack,
                  num_hourglass, kHgfMaxDepth);
    HgfLayout l;
    hgf_layout(num_stack, num_hourglass, &l);
    HgfLayoutT t;
    hgf_layout_t(l, &t);
    E3DGE_REQUIRE(n_filter_src == l.n_filter_src, "hgf_pack_weights_t: n_filter_src=%d, %d expected", n_filter_src, l.n_filter_src);
    for (int i = 0; i < l.n_filter_src; ++i) E3DGE_REQUIRE(filter_src[i], "hgf_pack_weights_t: null pointer (filter source %d)", i);
    if (front_src)
        for (int i = 0; i < kHgfFrontSrc; ++i) E3DGE_REQUIRE(front_src[i], "hgf_pack_weights_t: null pointer (front source %d)", i);
    hipStream_t st = as_stream(stream);
    const int n = front_src ? l.n_src : l.n_filter_src;
    for (int i = 0; i < n; ++i) {
        const HgfEntry& e = l.e[i];
        if (e.ks) ig_pack_t(packed_t + t.off[i], i < l.n_filter_src ? filter_src[i] : front_src[i - l.n_filter_src], e.cin, e.cout, e.ks, 1.0f, st);
    }
    return check_launch("hgf_pack_weights_t");
}

extern "C" int64_t e3dge_hgf_branch_bytes(int n, int height, int width, int num_stack, int num_hourglass) {
    if (!hgf_config_ok(num_stack, num_hourglass) || !hgf_sizes_ok(n, height, width, num_hourglass)) {
        fail(E3DGE_ERR_INVALID_ARG, "hgf_branch_bytes: n=%d height=%d width=%d num_stack=%d num_hourglass=%d (sizes multiples of 4 * 2^num_hourglass)", n,
             height, width, num_stack, num_hourglass);
        return -1;
    }
    HgfLayout l;
    hgf_layout(num_stack, num_hourglass, &l);
    HgfBranch b;
    hgf_branch(n, height, width, num_stack, num_hourglass, l, &b);
    return b.bytes;
}

extern "C" int64_t e3dge_hgf_bwd_ws_bytes(int n, int height, int width, int num_stack, int num_hourglass) {
    if (!hgf_config_ok(num_stack, num_hourglass) || !hgf_sizes_ok(n, height, width, num_hourglass)) {
        fail(E3DGE_ERR_INVALID_ARG, "hgf_bwd_ws_bytes: n=%d height=%d width=%d num_stack=%d num_hourglass=%d (sizes multiples of 4 * 2^num_hourglass)", n,
             height, width, num_stack, num_hourglass);
        return -1;
    }
    const HgfBwdWs d = hgf_bwd_ws(n, height, width, num_stack, num_hourglass);
    return (d.filter_floats > d.front_floats ? d.filter_floats : d.front_floats) * (int64_t)sizeof(float);
}

extern "C" int e3dge_hgf_backward(const E3dgeHgfBwdArgs* args, e3dge_stream_t stream) {
    E3DGE_REQUIRE(args, "hgf_backward: null argument struct");
    const E3dgeHgfBwdArgs& a = *args;
    const int S = a.num_stack, D = a.num_hourglass, n = a.n, H = a.height, W = a.width;
    E3DGE_REQUIRE(hgf_config_ok(S, D), "hgf_backward: num_stack=%d (1..%d) num_hourglass=%d (1..%d)", S, kHgfMaxStack, D, kHgfMaxDepth);
    E3DGE_REQUIRE(hgf_sizes_ok(n, H, W, D), "hgf_backward: n=%d height=%d width=%d (n 1..4096, sizes multiples of %d up to 4096)", n, H, W, 4 << D);
    E3DGE_REQUIRE(a.packed && a.packed_t && a.saved && a.tmpx && a.normx && a.g_input && a.ws, "hgf_backward: null pointer");
    int s_max = -1;
    for (int s = 0; s < S; ++s)
        if (a.g_outputs[s]) s_max = s;
    E3DGE_REQUIRE(s_max >= 0 || a.g_normx, "hgf_backward: null pointer (no upstream gradient at all)");
    if (a.grads) {
        E3DGE_REQUIRE(a.input, "hgf_backward: null pointer (the parameter gradients need the filter's input)");
        for (int s = 0; s < s_max; ++s) E3DGE_REQUIRE(a.outputs[s], "hgf_backward: null pointer (the parameter gradients need output %d)", s);
    }
    const HgfBwdWs w = hgf_bwd_ws(n, H, W, S, D);
    E3DGE_REQUIRE(a.ws_bytes >= w.filter_floats * (int64_t)sizeof(float), "hgf_backward: workspace of %lld bytes, %lld needed", (long long)a.ws_bytes,
                  (long long)(w.filter_floats * (int64_t)sizeof(float)));
    HgfLayout l;
    hgf_layout(S, D, &l);
    HgfLayoutT lt;
    hgf_layout_t(l, &lt);
    HgfSaved sv;
    hgf_saved(n, H, W, S, D, l, &sv);
    E3DGE_REQUIRE(a.saved_bytes >= sv.floats * (int64_t)sizeof(float), "hgf_backward: saved state of %lld bytes, %lld needed", (long long)a.saved_bytes,
                  (long long)(sv.floats * (int64_t)sizeof(float)));
    HgfBranch bl;
    if (a.branch) {
        hgf_branch(n, H, W, S, D, l, &bl);
        E3DGE_REQUIRE(a.branch_bytes >= bl.filter_bytes, "hgf_backward: branch buffer of %lld bytes, %lld needed", (long long)a.branch_bytes,
                      (long long)bl.filter_bytes);
    }
    hipStream_t st = as_stream(stream);
    float* ws = static_cast<float*>(a.ws);
    const float* saved = a.saved;
    const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4;
    HgfGradLayout gl;
    hgf_grad_layout(l, &gl);
    const HgfBwdRun r{a.packed, a.packed_t, &l, &lt, &sv, saved, &w, ws, st, n, a.branch, a.branch ? &bl : nullptr, a.grads, &gl};
    const int P4 = H4 * W4;
    int rc;
    float* gy = ws + w.gy;
    float* g_prev = ws + w.g_prev;
    float* g_o = ws + w.g_o;
    float* g_last = ws + w.g_last;
    float* g_top = ws + w.g_top;
    float* g_hg = ws + w.g_hg;
    for (int s = s_max; s >= 0; --s) {                                // stacks above the last one with a gradient receive none
        const HgfStack& k = l.stack[s];
        const HgfWs& v = sv.stack[s];
        const float* last = saved + v.last;
        const float* ab_end = saved + v.ab[0];
        const bool above = s < s_max;                                 // g_prev holds d previous of stack s + 1
        const float* go = a.g_outputs[s];
        if (above) {                                                  // d output = the caller's + al's
            if ((rc = hgf_dgrad({g_o, g_prev, r.wt(k.al_w), nullptr, nullptr, go, n, 256, 256, 256, 0, H4, W4, 1, 1, 0}, st))) return rc;
            go = g_o;
            if (a.grads) {                                            // al and bl: g is d previous of the stack above
                if ((rc = r.wgrad(k.al_w, g_prev, a.outputs[s], nullptr, 256, 256, 256, 0, H4, W4, 1, 1))) return rc;
                if ((rc = r.wgrad(k.bl_w, g_prev, last, ab_end, 256, 256, 256, 0, H4, W4, 1, 1))) return rc;
                if ((rc = hgf_bias_grad(r.gr(k.al_w + 1), g_prev, n, 256, P4, st))) return rc;
                if ((rc = hgf_bias_grad(r.gr(k.bl_w + 1), g_prev, n, 256, P4, st))) return rc;
            }
        }
        if (a.grads) {
            if ((rc = r.wgrad(k.l_w, go, last, ab_end, 256, 256, 256, 0, H4, W4, 1, 1))) return rc;
            if ((rc = hgf_bias_grad(r.gr(k.l_w + 1), go, n, 256, P4, st))) return rc;
        }
        if ((rc = hgf_dgrad({gy, go, r.wt(k.l_w), last, ab_end, nullptr, n, 256, 256, 256, 0, H4, W4, 1, 1, 0, a.branch ? r.br(bl.end[s]) : nullptr}, st))) return rc;     // d ll = l's + bl's
        if (above && (rc = hgf_dgrad({gy, g_prev, r.wt(k.bl_w), last, ab_end, gy, n, 256, 256, 256, 0, H4, W4, 1, 1, 0}, st))) return rc;
        if ((rc = hgf_norm_bwd(g_last, gy, last, r.at(k.bn_end), nullptr, nullptr, 0, 0, nullptr, r.coef(), n, 256, 0, 256, 32, P4, st, nullptr, r.gr(k.bn_end),
                               r.gr(k.bn_end + 1))))
            return rc;
        if (a.grads) {
            if ((rc = r.wgrad(k.last_w, g_last, saved + v.top, nullptr, 256, 256, 256, 0, H4, W4, 1, 1))) return rc;
            if ((rc = hgf_bias_grad(r.gr(k.last_w + 1), g_last, n, 256, P4, st))) return rc;
        }
        if ((rc = hgf_dgrad({g_top, g_last, r.wt(k.last_w), nullptr, nullptr, nullptr, n, 256, 256, 256, 0, H4, W4, 1, 1, 0}, st))) return rc;
        if ((rc = hgf_block_bwd(r, k.top, saved + v.hg, g_top, g_hg, nullptr, H4, W4))) return rc;
        if ((rc = hgf_level_bwd(r, v, D, k.first_block, saved + sv.prev[s], g_hg, g_prev, above ? g_prev : nullptr, H4, W4))) return rc;
    }
    const float* g_normx = a.g_normx;
    if (s_max >= 0) {
        float* g_c3 = ws + w.g_c3;
        float* g_n = ws + w.g_normx;
        if ((rc = hgf_block_bwd(r, l.conv4, saved + sv.c3, g_prev, g_c3, nullptr, H4, W4))) return rc;
        if ((rc = hgf_block_bwd(r, l.conv3, a.normx, g_c3, g_n, a.g_normx, H4, W4))) return rc;
        g_normx = g_n;
    }
    float* g_c2 = ws + w.g_c2;
    float* g_tmpx = ws + w.g_tmpx;
    float* g_stem = ws + w.g_stem;
    if ((rc = hgf_pool_bwd(g_c2, g_normx, nullptr, (int64_t)n * 128, H2, W2, st))) return rc;
    if ((rc = hgf_block_bwd(r, l.conv2, a.tmpx, g_c2, g_tmpx, nullptr, H2, W2))) return rc;
    if ((rc = hgf_norm_bwd(g_stem, g_tmpx, saved + sv.stem, r.at(l.stem_bn), saved + sv.ab_stem, nullptr, 0, 0, nullptr, r.coef(), n, 64, 0, 64, 32, H2 * W2, st,
                           a.branch ? r.br(bl.stem) : nullptr, r.gr(l.stem_bn), r.gr(l.stem_bn + 1))))
        return rc;
    if (a.grads) {
        if ((rc = r.wgrad(l.stem_w, g_stem, a.input, nullptr, 64, 64, 64, 0, H, W, 7, 2))) return rc;
        if ((rc = hgf_bias_grad(r.gr(l.stem_w + 1), g_stem, n, 64, H2 * W2, st))) return rc;
    }
    return hgf_dgrad({a.g_input, g_stem, r.wt(l.stem_w), nullptr, nullptr, nullptr, n, 64, 64, 64, 0, H, W, 7, 2, 0}, st);
}

extern "C" int e3dge_hgf_front_backward(const float* packed, const float* packed_t, const void* saved, int64_t saved_bytes, const float* g_feats,
                                        float* g_image, float* g_depth, int n, int height, int width, int num_stack, int num_hourglass, void* ws,
                                        int64_t ws_bytes, unsigned char* branch, int64_t branch_bytes, float* grads, const float* image,
                                        const float* depth, e3dge_stream_t stream) {
    E3DGE_REQUIRE(packed && packed_t && saved && g_feats && ws, "hgf_front_backward: null pointer");
    E3DGE_REQUIRE(g_image || g_depth || grads, "hgf_front_backward: null pointer (no gradient is wanted)");
    E3DGE_REQUIRE(!grads || (image && depth), "hgf_front_backward: null pointer (the parameter gradients need the image and the depth map)");
    E3DGE_REQUIRE(hgf_config_ok(num_stack, num_hourglass), "hgf_front_backward: num_stack=%d (1..%d) num_hourglass=%d (1..%d)", num_stack, kHgfMaxStack,
                  num_hourglass, kHgfMaxDepth);
    E3DGE_REQUIRE(hgf_sizes_ok(n, height, width, num_hourglass), "hgf_front_backward: n=%d height=%d width=%d (n 1..4096, sizes multiples of %d up to 4096)",
                  n, height, width, 4 << num_hourglass);
    const HgfBwdWs w = hgf_bwd_ws(n, height, width, num_stack, num_hourglass);
    E3DGE_REQUIRE(ws_bytes >= w.front_floats * (int64_t)sizeof(float), "hgf_front_backward: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
                  (long long)(w.front_floats * (int64_t)sizeof(float)));
    HgfLayout l;
    hgf_layout(num_stack, num_hourglass, &l);
    HgfLayoutT lt;
    hgf_layout_t(l, &lt);
    HgfSaved sv;
    hgf_saved(n, height, width, num_stack, num_hourglass, l, &sv);
    E3DGE_REQUIRE(saved_bytes >= sv.floats * (int64_t)sizeof(float), "hgf_front_backward: saved state of %lld bytes, %lld needed", (long long)saved_bytes,
                  (long long)(sv.floats * (int64_t)sizeof(float)));
    HgfBranch bl;
    if (branch) {
        hgf_branch(n, height, width, num_stack, num_hourglass, l, &bl);
        E3DGE_REQUIRE(branch_bytes >= bl.bytes, "hgf_front_backward: branch buffer of %lld bytes, %lld needed", (long long)branch_bytes, (long long)bl.bytes);
    }
    hipStream_t st = as_stream(stream);
    float* base = static_cast<float*>(ws);
    const float* keep = static_cast<const float*>(saved);
    double* coef = reinterpret_cast<double*>(base + w.f_coef);
    float* gy = base + w.f_gy;
    float* g2 = base + w.f_g2;
    float* g1 = base + w.f_g1;
    const int HW = height * width;
    int rc;
    HgfGradLayout gl;
    hgf_grad_layout(l, &gl);
    float* gfrag = base + w.f_gfrag;
    float* part = base + w.f_part;
    for (int f = 0; f < 2; ++f) {
        float* g_x = f == 0 ? g_image : g_depth;
        if (!g_x && !grads) continue;
        const HgfFront& q = l.front[f];
        auto gr = [&](int entry) { return grads ? grads + gl.off[entry] : nullptr; };
        auto wgrad = [&](int entry, const float* g, const float* x, const float* ab, int ci, int Cg_total, int g_c0, int ks, int reflect) {
            return grads ? hgf_wgrad({gr(entry), g, x, ab, n, ci, 32, Cg_total, g_c0, height, width, ks, 1, reflect}, gfrag, part, st) : (int)E3DGE_OK;
        };
        const int cin = f == 0 ? 3 : 1;
        const float* f0 = keep + sv.f0[f];
        const float* f1 = keep + sv.f1[f];
        auto wt = [&](int entry) { return packed_t + lt.off[entry]; };
        auto at = [&](int entry) { return packed + l.e[entry].off; };
        if ((rc = hgf_dgrad({g2, g_feats, wt(q.w3), nullptr, nullptr, nullptr, n, 32, 32, 64, 32 * f, height, width, 1, 1, 0}, st))) return rc;         // d f2
        if ((rc = hgf_dgrad({gy, g2, wt(q.w2), f1, keep + sv.fab[f][1], nullptr, n, 32, 32, 32, 0, height, width, 3, 1, 1, branch ? branch + bl.front[f][1] : nullptr}, st))) return rc;
        if ((rc = wgrad(q.w3, g_feats, keep + sv.f2[f], nullptr, 32, 64, 32 * f, 1, 0))) return rc;
        if ((rc = wgrad(q.w2, g2, f1, keep + sv.fab[f][1], 32, 32, 0, 3, 1))) return rc;
        if ((rc = hgf_norm_bwd(g1, gy, f1, at(q.n2), nullptr, nullptr, 0, 0, nullptr, coef, n, 32, 0, 32, 32, HW, st, nullptr, gr(q.n2), gr(q.n2 + 1)))) return rc;   // d f1
        if ((rc = wgrad(q.w1, g1, f0, keep + sv.fab[f][0], 32, 32, 0, 3, 1))) return rc;
        if ((rc = hgf_dgrad({gy, g1, wt(q.w1), f0, keep + sv.fab[f][0], nullptr, n, 32, 32, 32, 0, height, width, 3, 1, 1, branch ? branch + bl.front[f][0] : nullptr}, st))) return rc;
        if ((rc = hgf_norm_bwd(g1, gy, f0, at(q.n1), nullptr, nullptr, 0, 0, g2, coef, n, 32, 0, 32, 32, HW, st, nullptr, gr(q.n1), gr(q.n1 + 1)))) return rc;       // d f0 = d f2 + IN1's
        if ((rc = wgrad(q.w0, g1, f == 0 ? image : depth, nullptr, cin, 32, 0, 3, 1))) return rc;
        if (g_x && (rc = hgf_dgrad({g_x, g1, wt(q.w0), nullptr, nullptr, nullptr, n, cin, 32, 32, 0, height, width, 3, 1, 1}, st)))
            return rc;
    }
    return E3DGE_OK;
}

// ---- debug entries ----------------------------------------------------------------------------------------------------------------------
extern "C" int e3dge_hgf_conv_dgrad(float* out, const float* g, const float* w, float* wfrag_t, const float* x, const float* x_ab, const float* addend,
                                    int n, int cin, int cout, int height, int width, int ksize, int stride, int reflect, int g_channels, int g_c0,
                                    e3dge_stream_t stream) {
    E3DGE_REQUIRE(out && g && w && wfrag_t, "hgf_conv_dgrad: null pointer");
    E3DGE_REQUIRE(!x == !x_ab, "hgf_conv_dgrad: null pointer (x and x_ab go together)");
    E3DGE_REQUIRE(n >= 1 && n <= 4096 && cin >= 1 && cin <= 4096, "hgf_conv_dgrad: n=%d cin=%d (1..4096)", n, cin);
    E3DGE_REQUIRE(cout >= 16 && cout % 16 == 0 && cout <= 4096, "hgf_conv_dgrad: cout=%d (a multiple of 16 up to 4096)", cout);
    E3DGE_REQUIRE(hgf_geometry_ok(ksize, stride), "hgf_conv_dgrad: ksize=%d stride=%d (7 with 2, 3 with 1, 1 with 1)", ksize, stride);
    E3DGE_REQUIRE(height >= 1 && width >= 1 && height <= 4096 && width <= 4096, "hgf_conv_dgrad: height=%d width=%d (1..4096)", height, width);
    E3DGE_REQUIRE(!reflect || (ksize == 3 && height >= 2 && width >= 2), "hgf_conv_dgrad: reflect padding needs ksize 3 and sizes >= 2");
    E3DGE_REQUIRE(g_c0 >= 0 && g_channels >= 1 && g_channels <= 4096 && g_c0 + cout <= g_channels, "hgf_conv_dgrad: gradient slice [%d, %d) of %d channels",
                  g_c0, g_c0 + cout, g_channels);
    E3DGE_REQUIRE((int64_t)cin * height * width < ((int64_t)1 << 31) && (int64_t)g_channels * height * width < ((int64_t)1 << 31),
                  "hgf_conv_dgrad: image too large");
    hipStream_t st = as_stream(stream);
    ig_pack_t(wfrag_t, w, cin, cout, ksize, 1.0f, st);
    int rc;
    if ((rc = check_launch("hgf_conv_dgrad(pack)"))) return rc;
    return hgf_dgrad({out, g, wfrag_t, x, x_ab, addend, n, cin, cout, g_channels, g_c0, height, width, ksize, stride, reflect != 0}, st);
}

extern "C" int e3dge_hgf_norm_bwd(float* gx, const float* gy, const float* x, const float* gamma, const float* mask_ab, const float* add0, int add0_channels,
                                  int add0_c0, const float* add1, double* coef, float* dgamma, float* dbeta, int n, int channels_total, int c0, int channels,
                                  int groups, int height, int width, e3dge_stream_t stream) {
    E3DGE_REQUIRE(gx && gy && x && gamma && coef, "hgf_norm_bwd: null pointer");
    E3DGE_REQUIRE(!dgamma == !dbeta, "hgf_norm_bwd: null pointer (dgamma and dbeta go together)");
    E3DGE_REQUIRE(n >= 1 && n <= 4096 && channels >= 1 && channels <= 4096 && channels_total <= 4096, "hgf_norm_bwd: n=%d channels=%d of %d (1..4096)", n,
                  channels, channels_total);
    E3DGE_REQUIRE(c0 >= 0 && c0 + channels <= channels_total, "hgf_norm_bwd: channel slice [%d, %d) of %d", c0, c0 + channels, channels_total);
    E3DGE_REQUIRE(groups >= 1 && channels % groups == 0 && channels / groups <= 256,
                  "hgf_norm_bwd: groups=%d for %d channels (a divisor, at most 256 channels per group)", groups, channels);
    E3DGE_REQUIRE(height >= 1 && width >= 1 && height <= 4096 && width <= 4096, "hgf_norm_bwd: height=%d width=%d (1..4096)", height, width);
    E3DGE_REQUIRE(!add0 || (add0_c0 >= 0 && add0_channels <= 4096 && add0_c0 + channels <= add0_channels), "hgf_norm_bwd: addend slice [%d, %d) of %d channels",
                  add0_c0, add0_c0 + channels, add0_channels);
    return hgf_norm_bwd(gx, gy, x, gamma, mask_ab, add0, add0_channels, add0_c0, add1, coef, n, channels_total, c0, channels, groups, height * width,
                        as_stream(stream), nullptr, dgamma, dbeta);
}

extern "C" int e3dge_hgf_pool_bwd(float* gin, const float* gout, const float* addend, int64_t planes, int height, int width, e3dge_stream_t stream) {
    E3DGE_REQUIRE(gin && gout, "hgf_pool_bwd: null pointer");
    E3DGE_REQUIRE(planes >= 1 && planes <= ((int64_t)1 << 24), "hgf_pool_bwd: planes=%lld (1..2^24)", (long long)planes);
    E3DGE_REQUIRE(height >= 2 && width >= 2 && height <= 4096 && width <= 4096 && height % 2 == 0 && width % 2 == 0,
                  "hgf_pool_bwd: height=%d width=%d (even, 2..4096)", height, width);
    E3DGE_REQUIRE(planes * height * width < ((int64_t)1 << 38), "hgf_pool_bwd: tensor too large");
    return hgf_pool_bwd(gin, gout, addend, planes, height, width, as_stream(stream));
}

extern "C" int e3dge_hgf_up_bwd(float* glow, const float* g, int64_t planes, int height, int width, e3dge_stream_t stream) {
    E3DGE_REQUIRE(glow && g, "hgf_up_bwd: null pointer");
    E3DGE_REQUIRE(planes >= 1 && planes <= ((int64_t)1 << 24), "hgf_up_bwd: planes=%lld (1..2^24)", (long long)planes);
    E3DGE_REQUIRE(height >= 1 && width >= 1 && height <= 2048 && width <= 2048, "hgf_up_bwd: height=%d width=%d (1..2048)", height, width);
    E3DGE_REQUIRE(planes * 4 * height * width < ((int64_t)1 << 38), "hgf_up_bwd: tensor too large");
    return hgf_up_bwd(glow, g, planes, height, width, as_stream(stream));
}

extern "C" int64_t e3dge_hgf_grad_floats(int num_stack, int num_hourglass) {
    if (!hgf_config_ok(num_stack, num_hourglass)) {
        fail(E3DGE_ERR_INVALID_ARG, "hgf_grad_floats: num_stack=%d (1..%d) num_hourglass=%d (1..%d)", num_stack, kHgfMaxStack, num_hourglass, kHgfMaxDepth);
        return -1;
    }
    HgfLayout l;
    hgf_layout(num_stack, num_hourglass, &l);
    HgfGradLayout g;
    hgf_grad_layout(l, &g);
    return g.total;
}

extern "C" int64_t e3dge_hgf_wgrad_ws_floats(int n, int cin, int cout, int height, int width, int ksize, int stride) {
    if (!(n >= 1 && n <= 4096 && cin >= 1 && cin <= 4096 && cout >= 16 && cout % 16 == 0 && cout <= 4096 && hgf_geometry_ok(ksize, stride) && height >= 1 &&
          width >= 1 && height <= 4096 && width <= 4096)) {
        fail(E3DGE_ERR_INVALID_ARG, "hgf_wgrad_ws_floats: n=%d cin=%d cout=%d height=%d width=%d ksize=%d stride=%d", n, cin, cout, height, width, ksize, stride);
        return -1;
    }
    const int OHW = hgf_out_size(height, ksize, stride) * hgf_out_size(width, ksize, stride);
    return (hgf_wgrad_gfrag_floats(n, cout, OHW) + 63) / 64 * 64 + hgf_wgrad_part_floats(n, cin, cout, ksize, OHW);
}

extern "C" int e3dge_hgf_conv_wgrad(float* dw, float* dbias, const float* g, const float* x, const float* x_ab, int n, int cin, int cout, int height, int width,
                                    int ksize, int stride, int reflect, int g_channels, int g_c0, float* ws, int64_t ws_floats, e3dge_stream_t stream) {
    E3DGE_REQUIRE(dw && g && x && ws, "hgf_conv_wgrad: null pointer");
    E3DGE_REQUIRE(n >= 1 && n <= 4096 && cin >= 1 && cin <= 4096, "hgf_conv_wgrad: n=%d cin=%d (1..4096)", n, cin);
    E3DGE_REQUIRE(cout >= 16 && cout % 16 == 0 && cout <= 4096, "hgf_conv_wgrad: cout=%d (a multiple of 16 up to 4096)", cout);
    E3DGE_REQUIRE(hgf_geometry_ok(ksize, stride), "hgf_conv_wgrad: ksize=%d stride=%d (7 with 2, 3 with 1, 1 with 1)", ksize, stride);
    E3DGE_REQUIRE(height >= 1 && width >= 1 && height <= 4096 && width <= 4096, "hgf_conv_wgrad: height=%d width=%d (1..4096)", height, width);
    E3DGE_REQUIRE(!reflect || (ksize == 3 && height >= 2 && width >= 2), "hgf_conv_wgrad: reflect padding needs ksize 3 and sizes >= 2");
    E3DGE_REQUIRE(g_c0 >= 0 && g_channels >= 1 && g_channels <= 4096 && g_c0 + cout <= g_channels, "hgf_conv_wgrad: gradient slice [%d, %d) of %d channels", g_c0,
                  g_c0 + cout, g_channels);
    E3DGE_REQUIRE(!dbias || g_channels == cout, "hgf_conv_wgrad: the bias gradient takes a dense g");
    E3DGE_REQUIRE((int64_t)cin * height * width < ((int64_t)1 << 31) && (int64_t)g_channels * height * width < ((int64_t)1 << 31),
                  "hgf_conv_wgrad: image too large");
    const int OH = hgf_out_size(height, ksize, stride), OW = hgf_out_size(width, ksize, stride);
    const int64_t gf = (hgf_wgrad_gfrag_floats(n, cout, OH * OW) + 63) / 64 * 64, need = gf + hgf_wgrad_part_floats(n, cin, cout, ksize, OH * OW);
    E3DGE_REQUIRE(ws_floats >= need, "hgf_conv_wgrad: workspace of %lld floats, %lld needed", (long long)ws_floats, (long long)need);
    hipStream_t st = as_stream(stream);
    int rc;
    if ((rc = hgf_wgrad({dw, g, x, x_ab, n, cin, cout, g_channels, g_c0, height, width, ksize, stride, reflect != 0}, ws, ws + gf, st))) return rc;
    return dbias ? hgf_bias_grad(dbias, g, n, cout, OH * OW, st) : (int)E3DGE_OK;
}
