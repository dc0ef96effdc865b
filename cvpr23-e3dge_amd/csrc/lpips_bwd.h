// LPIPS backward: the gradient of per_image[b] with respect to x, y or both (included by lpips.hip, inside namespace e3dge).  The
// AlexNet and lin weights are frozen, as the reference freezes them (networks.py:47, 30-31); the forward's workspace supplies the five
// post-ReLU activations f_l and nothing is recomputed but the channel norms.
//
//   n = sqrt(sum_c f_c^2 + 1e-8) + 1e-10,  f^ = f / n,  u[b] = dL / d per_image[b]
//   dx^_c = 2 lin_c (x^_c - y^_c) u[b] / HW_l  (dy^ = -dx^),   dtap_c = dx^_c / n - f_c (sum_c' dx^_c' f_c') / (n^2 sqrt(sum f^2 + 1e-8))
//   G_5 = dtap_5 [f_5 > 0],  G_l = (D_{l+1} + dtap_l) [f_l > 0],  D_{l+1} = conv l+1's data gradient of G_{l+1} (through the max-pool's
//   backward for l = 1, 2),  dx = D_1 / std
//
// Kernels (eight launches for one backward, whatever the batch; no atomics, every sum in a fixed order):
//   tap_bwd_kernel    the tap kernel's geometry, all five layers in one launch: channel norms of both images of the pair, then
//                     dtap_l [f_l > 0] of the images that get a gradient, into the G_l buffers (for layer 5 that is G_5).
//   conv_kernel       the forward's kernel (the implicit GEMM of conv_igemm.h, the forward's gather) on the transposed, tap-flipped
//                     weight image: M = C_in(l), K = (co, r, s), N = the pixels of the gradient images.  3x3 / p1 and 5x5 / p2 are
//                     their own adjoints' geometry.  Epilogue kLpEpiMask (data gradients of conv 5 and 4: (acc + dtap) [f > 0] in
//                     place, G_4 and G_3) or kLpEpiStore (conv 3 and 2: the gradients of the two pooled maps).  The forward's order of
//                     sums holds, so a pixel's gradient does not depend on the batch or the tile width.
//   pool_bwd_kernel   a gather: an element sums the gradients of the at most four windows whose FIRST maximum in row-major order it
//                     is (torch's rule), then + dtap_l and the ReLU mask: G_2 and G_1.
//   conv1_bwd_kernel  64 -> 3 channels, k 11, stride 4, pad 2, phase-decomposed on the VALU: a thread owns the 4 x 4 input pixels
//                     (iy + 2, ix + 2) = 4 (by, bx) + (py, px) of one channel; tap (r, s) then always meets output pixel
//                     (by - r / 4, bx - s / 4) and phase (r % 4, s % 4), so per output channel the thread reads a 3 x 3 patch of G_1
//                     and runs 121 FMAs whose weight operand is uniform over the wave (scalar loads, no LDS for weights or patch).  The
//                     64 output channels are split over the eight waves of a workgroup -- one wave per pixel block left the chip
//                     waiting on the scalar loads -- and folded through LDS in a fixed order; / std in the store.
// Measured times and what bounds each kernel: DESIGN.md 4.11c.

// ---- the transposed weight image ------------------------------------------------------------------------------------------------------
// layer l = 1..4 (conv 2..5): Wt_l[ci][(co, r, s)] = W_l[co][ci][ks - 1 - r][ks - 1 - s] in A-fragment order as the forward image holds
// W_l, M = lp_cin(l); then conv 1 as [c][co][11 x 11], the order conv1_bwd_kernel reads.
__host__ __device__ constexpr int lp_kt(int l) { return lp_cout(l) * lp_ks(l) * lp_ks(l); }
__host__ __device__ constexpr int lp_ktpad(int l) { return ig_kpad(lp_kt(l)); }
__host__ __device__ constexpr int64_t lp_wt_floats(int l) { return (int64_t)lp_cin(l) * lp_ktpad(l); }
__host__ __device__ constexpr int64_t lp_wt_off(int l) { int64_t o = 0; for (int q = 1; q < l; ++q) o += lp_wt_floats(q); return o; }
constexpr int64_t kLpW1tOff = lp_wt_off(kLpLayers);
constexpr int64_t kLpW1tFloats = (int64_t)lp_cin(0) * lp_cout(0) * lp_ks(0) * lp_ks(0);
constexpr int64_t kLpPackedTFloats = kLpW1tOff + kLpW1tFloats;
static_assert(lp_cin(1) % kIgBM == 0 && lp_cin(2) % kIgBM == 0 && lp_cin(3) % kIgBM == 0 && lp_cin(4) % kIgBM == 0, "whole channel tiles");

// conv 1's block, the one layout conv_igemm.h does not know: w1t[c][co][rs] = W_1[co][c][rs]
__global__ void __launch_bounds__(256) lpips_pack_w1t_kernel(float* __restrict__ w1t, const float* __restrict__ w) {
    constexpr int KK = lp_ks(0) * lp_ks(0);
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= kLpW1tFloats) return;
    const int c = e / (lp_cout(0) * KK), rest = e - c * (lp_cout(0) * KK), co = rest / KK, rs = rest - co * KK;
    w1t[e] = w[(co * lp_cin(0) + c) * KK + rs];
}

// ---- tap backward ---------------------------------------------------------------------------------------------------------------------
struct LpTapBwdArgs {
    const float* feat[kLpLayers];      // the forward's activations (2B, C_l, HW_l)
    float* g[kLpLayers];               // (n, C_l, HW_l): dtap_l [f_l > 0] of the images that get a gradient, x's first
    int hw[kLpLayers];
    int blk_off[kLpLayers + 1];
    const float* lin;
    const float* upstream;             // (B)
    int batch, want_x, want_y;
};

__global__ void __launch_bounds__(256) lpips_tap_bwd_kernel(LpTapBwdArgs a) {
    __shared__ float red[2][kLpTapGroups][kLpTapPix];
    __shared__ float nrm[2][kLpTapPix], coef[2][kLpTapPix];
    const int per_img = a.blk_off[kLpLayers];
    const int b = blockIdx.x / per_img, wb = blockIdx.x - b * per_img;
    int l = 0;
#pragma unroll
    for (int q = 1; q < kLpLayers; ++q) if (wb >= a.blk_off[q]) l = q;
    int C = lp_cout(0), HW = a.hw[0], first = a.blk_off[0]; int64_t coff = 0;
    const float* feat = a.feat[0]; float* gout = a.g[0];
#pragma unroll
    for (int q = 1; q < kLpLayers; ++q)
        if (l == q) { C = lp_cout(q); coff = lp_c_off(q); HW = a.hw[q]; first = a.blk_off[q]; feat = a.feat[q]; gout = a.g[q]; }
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
        const float rt = __fsqrt_rn(__fadd_rn(s, 1e-8f)), n = __fadd_rn(rt, 1e-10f);
        nrm[w][p] = n;
        coef[w][p] = __fmul_rn(__fmul_rn(n, n), rt);                 // n^2 sqrt(sum f^2 + 1e-8)
    }
    __syncthreads();
    const float nx = nrm[0][p], ny = nrm[1][p];
    const float* __restrict__ lin = a.lin + coff;
    const float scale = __fdiv_rn(__fmul_rn(2.0f, a.upstream[b]), (float)HW);
    // t_c = dx^_c = -dy^_c; the two dot products sum_c t_c f_c
    float dx = 0.0f, dy = 0.0f;
    if (ok)
        for (int c = g; c < C; c += kLpTapGroups) {
            const float vx = fx[(int64_t)c * HW], vy = fy[(int64_t)c * HW];
            const float t = __fmul_rn(__fmul_rn(lin[c], __fsub_rn(__fdiv_rn(vx, nx), __fdiv_rn(vy, ny))), scale);
            dx = fmaf(t, vx, dx); dy = fmaf(t, vy, dy);
        }
    __syncthreads();
    red[0][g][p] = dx; red[1][g][p] = dy;
    __syncthreads();
    if (threadIdx.x < 2 * kLpTapPix) {
        const int w = threadIdx.x >> 4;
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < kLpTapGroups; ++q) s += red[w][q][p];
        coef[w][p] = __fdiv_rn(s, coef[w][p]);
    }
    __syncthreads();
    if (!ok) return;
    const float kx = coef[0][p], ky = coef[1][p];
    float* gx = a.want_x ? gout + (int64_t)b * C * HW + pix : nullptr;
    float* gy = a.want_y ? gout + (int64_t)(b + (a.want_x ? a.batch : 0)) * C * HW + pix : nullptr;
    for (int c = g; c < C; c += kLpTapGroups) {
        const float vx = fx[(int64_t)c * HW], vy = fy[(int64_t)c * HW];
        const float t = __fmul_rn(__fmul_rn(lin[c], __fsub_rn(__fdiv_rn(vx, nx), __fdiv_rn(vy, ny))), scale);
        if (gx) gx[(int64_t)c * HW] = vx > 0.0f ? __fsub_rn(__fdiv_rn(t, nx), __fmul_rn(vx, kx)) : 0.0f;
        if (gy) gy[(int64_t)c * HW] = vy > 0.0f ? -__fsub_rn(__fdiv_rn(t, ny), __fmul_rn(vy, ky)) : 0.0f;
    }
}

// ---- max-pool backward, + dtap, ReLU mask ---------------------------------------------------------------------------------------------
// g (planes, IH, IW) holds dtap [f > 0] and becomes G; dpool (planes, OH, OW); f: the forward's activation of the same planes
__global__ void __launch_bounds__(256)
lpips_pool_bwd_kernel(float* __restrict__ g, const float* __restrict__ dpool, const float* __restrict__ f, int64_t planes, int IH, int IW,
                      int OH, int OW) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= planes * IH * IW) return;
    const int64_t plane = i / (IH * IW);
    const int pix = (int)(i - plane * (IH * IW)), iy = pix / IW, ix = pix - iy * IW;
    const float* fp = f + plane * IH * IW;
    if (!(fp[pix] > 0.0f)) { g[i] = 0.0f; return; }                   // relu'(0) = 0
    const float* dp = dpool + plane * OH * OW;
    const int oy0 = iy > 1 ? (iy - 1) >> 1 : 0, oy1 = min(OH - 1, iy >> 1);
    const int ox0 = ix > 1 ? (ix - 1) >> 1 : 0, ox1 = min(OW - 1, ix >> 1);
    float sum = 0.0f;
    for (int oy = oy0; oy <= oy1; ++oy)
        for (int ox = ox0; ox <= ox1; ++ox) {
            const float* w = fp + (2 * oy) * IW + 2 * ox;
            float best = w[0];
            int at = 0;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const float v = w[r * IW + s];
                    if (v > best) { best = v; at = r * 3 + s; }          // strict: the first maximum in row-major order
                }
            if (2 * oy + at / 3 == iy && 2 * ox + at % 3 == ix) sum = __fadd_rn(sum, dp[oy * OW + ox]);
        }
    g[i] = __fadd_rn(sum, g[i]);
}

// ---- conv 1's data gradient -----------------------------------------------------------------------------------------------------------
// grid (blocks of 64 (by, bx), 3 channels, n images); wave w of the eight owns output channels 8 w .. 8 w + 7 (the weight operand stays
// uniform over a wave), the eight partial sums are folded through LDS in ascending w.  out: image z < n_x goes to gx, the others to gy.
constexpr int kLpC1Waves = 8, kLpC1Co = lp_cout(0) / kLpC1Waves;

__global__ void __launch_bounds__(64 * kLpC1Waves)
lpips_conv1_bwd_kernel(float* __restrict__ gx, float* __restrict__ gy, int n_x, const float* __restrict__ g1, const float* __restrict__ wt,
                       int H, int W, int OH, int OW, int BH, int BW, LpNorm nrm) {
    constexpr int KS = lp_ks(0), CO = lp_cout(0);
    __shared__ float red[kLpC1Waves][16][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (uniform: scalar weight loads)
    const int t = blockIdx.x * 64 + lane;
    const bool valid = t < BH * BW;
    const int by = t / BW, bx = t - by * BW;
    const int c = blockIdx.y, img = blockIdx.z;
    float acc[4][4];
#pragma unroll
    for (int py = 0; py < 4; ++py)
#pragma unroll
        for (int px = 0; px < 4; ++px) acc[py][px] = 0.0f;
    const float* __restrict__ gimg = g1 + ((int64_t)img * CO + wave * kLpC1Co) * OH * OW;
    const float* __restrict__ w = wt + ((int64_t)c * CO + wave * kLpC1Co) * KS * KS;
    bool in[3][3];
    int off[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int oy = by - j, ox = bx - i;
            in[j][i] = valid && oy >= 0 && oy < OH && ox >= 0 && ox < OW;
            off[j][i] = in[j][i] ? oy * OW + ox : 0;
        }
    for (int co = 0; co < kLpC1Co; ++co) {
        float gv[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i) gv[j][i] = in[j][i] ? gimg[(int64_t)co * OH * OW + off[j][i]] : 0.0f;
#pragma unroll
        for (int r = 0; r < KS; ++r)
#pragma unroll
            for (int s = 0; s < KS; ++s) acc[r & 3][s & 3] = fmaf(w[(co * KS + r) * KS + s], gv[r >> 2][s >> 2], acc[r & 3][s & 3]);
    }
#pragma unroll
    for (int py = 0; py < 4; ++py)
#pragma unroll
        for (int px = 0; px < 4; ++px) red[wave][py * 4 + px][lane] = acc[py][px];
    __syncthreads();
    if (!valid) return;
    const float sd = c == 0 ? nrm.std[0] : c == 1 ? nrm.std[1] : nrm.std[2];
    float* out = img < n_x ? gx + (int64_t)img * 3 * H * W : gy + (int64_t)(img - n_x) * 3 * H * W;
#pragma unroll
    for (int q = 0; q < 16 / kLpC1Waves; ++q) {                     // wave w stores phases 2 w and 2 w + 1 of its lane's pixel block
        const int k = wave * (16 / kLpC1Waves) + q, py = k >> 2, px = k & 3;
        float v = red[0][k][lane];
#pragma unroll
        for (int g = 1; g < kLpC1Waves; ++g) v = __fadd_rn(v, red[g][k][lane]);
        const int iy = 4 * by + py - 2, ix = 4 * bx + px - 2;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) out[((int64_t)c * H + iy) * W + ix] = __fdiv_rn(v, sd);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
struct LpBwdDims { int64_t g_off[kLpLayers], dpool_off[2], total_bytes; };

static bool lp_bwd_dims(const LpDims& d, int n_img, LpBwdDims* o) {
    int64_t off = 0;
    auto take = [&](int64_t floats) { const int64_t at = off; off += (floats + 63) / 64 * 64; return at; };
    for (int l = 0; l < kLpLayers; ++l) o->g_off[l] = take((int64_t)n_img * lp_cout(l) * d.h[l] * d.w[l]);
    for (int q = 0; q < 2; ++q) o->dpool_off[q] = take((int64_t)n_img * lp_cout(q) * d.ph[q] * d.pw[q]);
    o->total_bytes = off * (int64_t)sizeof(float);
    return true;
}

// data gradient of conv l (1..4) of the n images g (n, C_out(l), H, W) -> out (n, C_in(l), H, W); f, f_first: kLpEpiMask's activation
template <int KS_, int PAD, int EPI>
static int lp_dgrad(float* out, const float* g, const float* packed_t, int l, int H, int W, int n_img, const float* f, int f_first,
                    hipStream_t st) {
    const int64_t N = (int64_t)n_img * H * W;
    const int M = lp_cin(l), gy = M / kIgBM;
    const float* wf = packed_t + lp_wt_off(l);
    const int K = lp_kt(l), KS4 = lp_ktpad(l) / 4;
    auto blocks = [&](int bn) { return (N + bn - 1) / bn; };
    E3DGE_REQUIRE(blocks(16) < ((int64_t)1 << 31), "lpips_backward: grid too large");
    const LpNorm nrm{};
    ig_dispatch_nt(ig_tile_width(N, 1, gy), [&](auto nt_c) {           // the forward's rule
        constexpr int NT = decltype(nt_c)::value;
        lpips_conv_kernel<KS_, 1, PAD, NT, false, EPI><<<dim3((unsigned)blocks(16 * NT), gy), dim3(256), 0, st>>>(
            out, g, g, n_img, wf, f, lp_cout(l), H, W, M, H, W, N, K, KS4, nrm, f_first);
    });
    return check_launch("lpips_backward(dgrad)");
}

static int lp_backward(const E3dgeLpipsBwdArgs& a, hipStream_t st) {
    E3DGE_REQUIRE(a.packed && a.packed_t && a.fwd_ws && a.upstream && a.ws, "lpips_backward: null pointer");
    E3DGE_REQUIRE(a.grad_x || a.grad_y, "lpips_backward: grad_x and grad_y are both null");
    E3DGE_REQUIRE(a.batch >= 1 && a.batch < 32768, "lpips_backward: batch=%d", a.batch);
    E3DGE_REQUIRE(a.height >= 31 && a.width >= 31, "lpips_backward: height=%d width=%d (the smallest image with an output at every layer is 31 x 31)",
                  a.height, a.width);
    E3DGE_REQUIRE(a.std[0] != 0.0f && a.std[1] != 0.0f && a.std[2] != 0.0f, "lpips_backward: a channel's std is 0");
    LpDims d;
    E3DGE_REQUIRE(lp_dims(a.batch, a.height, a.width, &d), "lpips_backward: sizes too large");
    const int B = a.batch, n = (a.grad_x ? B : 0) + (a.grad_y ? B : 0), f_first = a.grad_x ? 0 : B;
    LpBwdDims bd;
    lp_bwd_dims(d, n, &bd);
    E3DGE_REQUIRE(a.fwd_ws_bytes >= d.total_bytes, "lpips_backward: forward workspace of %lld bytes, %lld needed", (long long)a.fwd_ws_bytes,
                  (long long)d.total_bytes);
    E3DGE_REQUIRE(a.ws_bytes >= bd.total_bytes, "lpips_backward: workspace of %lld bytes, %lld needed", (long long)a.ws_bytes,
                  (long long)bd.total_bytes);
    const float* fws = static_cast<const float*>(a.fwd_ws);
    float* ws = static_cast<float*>(a.ws);
    const float* act[kLpLayers];
    float* G[kLpLayers];
    for (int l = 0; l < kLpLayers; ++l) { act[l] = fws + d.act_off[l]; G[l] = a.gpre[l] ? a.gpre[l] : ws + bd.g_off[l]; }
    float* dp0 = ws + bd.dpool_off[0];
    float* dp1 = ws + bd.dpool_off[1];
    auto f_of = [&](int l) { return act[l] + (int64_t)f_first * lp_cout(l) * d.h[l] * d.w[l]; };
    LpTapBwdArgs t;
    for (int l = 0; l < kLpLayers; ++l) { t.feat[l] = act[l]; t.g[l] = G[l]; t.hw[l] = d.h[l] * d.w[l]; }
    for (int l = 0; l <= kLpLayers; ++l) t.blk_off[l] = d.blk_off[l];
    t.lin = a.packed + kLpLinOff; t.upstream = a.upstream; t.batch = B; t.want_x = a.grad_x != nullptr; t.want_y = a.grad_y != nullptr;
    lpips_tap_bwd_kernel<<<dim3((unsigned)(B * d.blk_off[kLpLayers])), dim3(256), 0, st>>>(t);
    int rc;
    if ((rc = check_launch("lpips_backward(taps)"))) return rc;
    if ((rc = lp_dgrad<3, 1, kLpEpiMask>(G[3], G[4], a.packed_t, 4, d.h[4], d.w[4], n, act[3], f_first, st))) return rc;
    if ((rc = lp_dgrad<3, 1, kLpEpiMask>(G[2], G[3], a.packed_t, 3, d.h[3], d.w[3], n, act[2], f_first, st))) return rc;
    if ((rc = lp_dgrad<3, 1, kLpEpiStore>(dp1, G[2], a.packed_t, 2, d.h[2], d.w[2], n, nullptr, 0, st))) return rc;
    auto pool_bwd = [&](float* g, const float* dpool, int l) {
        const int64_t planes = (int64_t)n * lp_cout(l), total = planes * d.h[l] * d.w[l];
        lpips_pool_bwd_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(g, dpool, f_of(l), planes, d.h[l], d.w[l], d.ph[l],
                                                                                        d.pw[l]);
        return check_launch("lpips_backward(pool)");
    };
    if ((rc = pool_bwd(G[1], dp1, 1))) return rc;
    if ((rc = lp_dgrad<5, 2, kLpEpiStore>(dp0, G[1], a.packed_t, 1, d.h[1], d.w[1], n, nullptr, 0, st))) return rc;
    if ((rc = pool_bwd(G[0], dp0, 0))) return rc;
    LpNorm nrm;
    for (int c = 0; c < 3; ++c) { nrm.mean[c] = 0.0f; nrm.std[c] = a.std[c]; }
    const int BH = (a.height + 1) / 4 + 1, BW = (a.width + 1) / 4 + 1;
    lpips_conv1_bwd_kernel<<<dim3((unsigned)((BH * BW + 63) / 64), 3, (unsigned)n), dim3(64 * kLpC1Waves), 0, st>>>(
        a.grad_x ? a.grad_x : a.grad_y, a.grad_y, a.grad_x ? B : 0, G[0], a.packed_t + kLpW1tOff, a.height, a.width, d.h[0], d.w[0], BH, BW, nrm);
    return check_launch("lpips_backward(conv1)");
}
