// StyleGAN2 discriminator, forward: the frozen network behind the adversarial term of the stage-2.2 objective,
// g_nonsaturating_loss(D(gen_imgs)) (project/trainer.py:1233-1244 with requires_grad(discriminator, False)).
//
// Reference: Discriminator / ResBlock / ConvLayer / EqualConv2d / Blur / EqualLinear (project/models/stylesdf_model.py:148-249, :544-584,
// :1514-1617), FusedLeakyReLU (models/op/fused_act.py).
//
//   pool_256 (init_size 256) -> conv1x1 in->C0, lrelu -> ResBlocks down to 4^2 -> minibatch stddev channel -> conv3x3 (C+1)->512, lrelu
//   -> flatten -> linear 8192->512, lrelu -> linear 512->1
//   ResBlock(in, out):  t = lrelu(conv3x3(x) + b1);  a = lrelu(conv3x3_stride2(blur_pad2(t)) + b2);  out = (a + conv1x1_stride2(blur_pad1(x))) / sqrt 2
//   lrelu(v) = (v > 0 ? v : 0.2 v) * sqrt 2   (FusedLeakyReLU)
//
// Kernels:
//   gemm_kernel    the implicit GEMM of conv_igemm.h (M = output channels, K = (ci, r, s), N = the output pixels of ONE image per workgroup
//                  column; waves past M idle) on a packed A-fragment image that already carries EqualConv2d's scale.  Four fp32
//                  accumulators (the groups of four k, modulo 4) run in ascending k and are folded every 128 k into an fp64 total,
//                  (0 + 1) + (2 + 3), which is rounded to fp32 once: chains of eight matrix steps, so a K = 4608 sum is about as accurate
//                  as a blocked library GEMM's instead of carrying 288 sequential roundings.  The tile width depends on the layer alone,
//                  and tiles never straddle images, so an image's convolution outputs do not depend on the batch.  Gather, three modes:
//                  stride 1 with padding, stride 2 without (on a blurred plane), and the transposed stride 2 of the backward; an optional
//                  factor chosen by the sign of a second tensor (the backward's lrelu derivative from the saved activations).  Epilogue:
//                  optional bias and lrelu, optional addend, merged as (v + addend) / sqrt 2 or added.
//   blur           e3dge_upfirdn2d (csrc/upfirdn2d.hip): every blurred value is rounded to fp32 as the reference's separate op rounds it.
//   stddev_kernel  one workgroup per sub-batch: per element the group's mean and variance (two passes), sqrt(var + 1e-8) in fp32, summed in
//                  fp64 per thread in ascending order, then a fixed tree; writes the concatenated (C + 1)-channel tensor.
//   head_kernel    two rows of the 8192 -> 512 matrix per workgroup, held in registers for every image of the launch (the 16 MB matrix is
//                  read once per launch), fp64 sums rounded to fp32 once, bias and lrelu fused; head_out_kernel: the 512 -> 1 dot
//                  product, one workgroup per image.
// The state-saving forward is the same launches writing the activations into the caller's `saved` buffer instead of the workspace, so
// its logits are bit-identical.  No atomics, no allocation, no synchronisation.  The backward is disc_bwd.h.
// Measured times: DESIGN.md 4.11g.
#include "conv_igemm.h"

namespace e3dge {

constexpr int kDcFlush = 4;                     // k tiles between two folds of the fp32 accumulators into the fp64 totals (a power of two)
constexpr int kDcMaxBlocks = E3DGE_DISC_MAX_BLOCKS;
constexpr int kDcHeadK = 512 * 16, kDcHid = 512, kDcHeadRows = 2, kDcHeadImgs = 4;
constexpr float kDcSqrt2 = 1.41421356237309515f, kDcSlope = 0.2f;

// ---- network description --------------------------------------------------------------------------------------------------------
struct DcNet {
    int init, cm, cin, n_blocks;
    int c[kDcMaxBlocks + 1];                      // c[0]: the stem's width; c[i + 1]: block i's output width
    int size[kDcMaxBlocks + 1];                   // size[0] = init; size[i + 1] = size[i] / 2
};

static int dc_channels(int size, int cm) {
    switch (size) {
        case 4: case 8: case 16: case 32: return 512;
        case 64: return 256 * cm;
        case 128: return 128 * cm;
        case 256: return 64 * cm;
        case 512: return 32 * cm;
        case 1024: return 16 * cm;
    }
    return 0;
}

static bool dc_net(int init, int cm, int cin, DcNet* d) {
    if (init < 8 || init > 1024 || (init & (init - 1)) || cm < 1 || cm > 4 || cin < 1 || cin > 16) return false;
    d->init = init; d->cm = cm; d->cin = cin;
    int lg = 0;
    while ((1 << lg) < init) ++lg;
    d->n_blocks = lg - 2;
    d->c[0] = dc_channels(init, cm); d->size[0] = init;
    for (int i = 0; i < d->n_blocks; ++i) { d->size[i + 1] = d->size[i] / 2; d->c[i + 1] = dc_channels(d->size[i + 1], cm); }
    return d->c[d->n_blocks] == 512;                                // (narrower layers leave waves of a workgroup idle: 16 cm channels at 1024^2)
}

// offsets (floats) into the packed image: forward and transposed A fragments of every convolution, the biases, the head
struct DcLayout {
    int64_t stem_w, stem_wt, stem_b;
    int64_t c1_w[kDcMaxBlocks], c1_wt[kDcMaxBlocks], c1_b[kDcMaxBlocks];
    int64_t c2_w[kDcMaxBlocks], c2_wt[kDcMaxBlocks], c2_b[kDcMaxBlocks];
    int64_t sk_w[kDcMaxBlocks], sk_wt[kDcMaxBlocks];
    int64_t fin_w, fin_wt, fin_b, lin1_w, lin1_b, lin2_w, lin2_b, blur, blur_flip, total;
};

static void dc_layout(const DcNet& n, DcLayout* l) {
    int64_t off = 0;
    auto take = [&](int64_t floats) { const int64_t at = off; off += (floats + 63) / 64 * 64; return at; };
    auto fw = [&](int ci, int co, int ks) { return take((int64_t)ig_mpad(co) * ig_kpad(ci * ks * ks)); };
    auto tw = [&](int ci, int co, int ks) { return take((int64_t)ig_mpad(ci) * ig_kpad(co * ks * ks)); };
    l->stem_w = fw(n.cin, n.c[0], 1); l->stem_wt = tw(n.cin, n.c[0], 1); l->stem_b = take(n.c[0]);
    for (int i = 0; i < n.n_blocks; ++i) {
        const int ci = n.c[i], co = n.c[i + 1];
        l->c1_w[i] = fw(ci, ci, 3); l->c1_wt[i] = tw(ci, ci, 3); l->c1_b[i] = take(ci);
        l->c2_w[i] = fw(ci, co, 3); l->c2_wt[i] = tw(ci, co, 3); l->c2_b[i] = take(co);
        l->sk_w[i] = fw(ci, co, 1); l->sk_wt[i] = tw(ci, co, 1);
    }
    l->fin_w = fw(513, 512, 3); l->fin_wt = tw(513, 512, 3); l->fin_b = take(512);
    l->lin1_w = take((int64_t)kDcHid * kDcHeadK); l->lin1_b = take(kDcHid);
    l->lin2_w = take(kDcHid); l->lin2_b = take(64);
    l->blur = take(16); l->blur_flip = take(16);
    l->total = off;
}

// ---- packing ----------------------------------------------------------------------------------------------------------------------
// The A-fragment images come from conv_igemm.h's packers with EqualConv2d's scale: the product is rounded once, as `weight * scale` is on
// every call of the reference.  Biases, the two linear layers and the FIR (flipped: the blur's adjoint's) go through ig_copy.

// ---- convolution ----------------------------------------------------------------------------------------------------------------
struct DcGemmArgs {
    float* out; const float* in; const float* wfrag;
    const float* sign; float s_pos, s_neg; int scaled;   // staging: x *= sign ? (sign[at] > 0 ? s_pos : s_neg) : s_pos, when `scaled`
    const float* bias; int act;                          // v += bias[row]; act: v = (v > 0 ? v : 0.2 v) * sqrt 2
    const float* addend; int merge;                      // v = merge ? (addend + v) / sqrt 2 : v + addend
    int Cin, IH, IW, M, OH, OW, K, KS4, tiles, pad;
};

// MODE 0: input (oy - pad + r, ox - pad + s).  MODE 1: input (2 oy + r, 2 ox + s) (stride 2, no padding).  MODE 2: the transposed
// stride 2: tap (r, s) of output (oy, ox) exists where oy - pad + r and ox - pad + s are even, at half those coordinates.
template <int KS_, int MODE, int NT>
__global__ void __launch_bounds__(256) disc_gemm_kernel(DcGemmArgs a) {
    constexpr int BN = IgTile<NT>::BN, ROWS = IgTile<NT>::ROWS, PER = IgTile<NT>::PER;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mt = blockIdx.y * (kIgBM / 16) + wave;
    const bool live = mt * 16 < a.M;                                // wave-uniform
    const int OHW = a.OH * a.OW, IH = a.IH, IW = a.IW, K = a.K;
    const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
    const int sn = tid % BN, srow = tid / BN;
    const int spix = tile * BN + sn;
    const bool n_ok = spix < OHW;
    const int soy = spix / a.OW, sox = spix - soy * a.OW;
    const int iy0 = MODE == 1 ? 2 * soy : soy - a.pad, ix0 = MODE == 1 ? 2 * sox : sox - a.pad;
    const int64_t img_off = (int64_t)img * a.Cin * IH * IW;
    const float* __restrict__ src = a.in + img_off;
    const float* __restrict__ sgn = a.sign ? a.sign + img_off : nullptr;
    const bool scaled = a.scaled != 0;
    const float s_pos = a.s_pos, s_neg = a.s_neg;
    auto fetch = [&](int k0, float (&v)[PER]) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = k0 + srow + i * ROWS;
            const auto [ci, r, s] = ig_decode<KS_>(k);
            int iy = iy0 + r, ix = ix0 + s;
            bool ok = n_ok && k < K && iy >= 0 && ix >= 0;
            if (MODE == 2) { ok = ok && !((iy | ix) & 1); iy >>= 1; ix >>= 1; }
            ok = ok && iy < IH && ix < IW;
            float x = 0.0f;
            if (ok) {
                const int64_t at = ((int64_t)ci * IH + iy) * IW + ix;
                x = src[at];
                if (scaled) x = __fmul_rn(x, sgn ? (sgn[at] > 0.0f ? s_pos : s_neg) : s_pos);
            }
            v[i] = x;
        }
    };
    f32x4 acc[NT][4];
    double tot[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) tot[t][r] = 0.0;
    auto fold = [&](int kt, bool last) {
        if ((kt & (kDcFlush - 1)) == kDcFlush - 1 || last) {        // every 128 k: fold the fp32 chains into the fp64 totals
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    tot[t][r] += ((double)acc[t][0][r] + (double)acc[t][1][r]) + ((double)acc[t][2][r] + (double)acc[t][3][r]);
#pragma unroll
                    for (int h = 0; h < 4; ++h) acc[t][h][r] = 0.0f;
                }
        }
    };
    ig_k_loop<NT, 4, true>(acc, a.wfrag + (int64_t)(live ? mt : 0) * a.KS4 * 64 + lane, a.KS4 / (kIgKC / 4), live, fetch, fold);
    if (!live) return;
    // C/D fragment: lane l, register r holds D[4 (l >> 4) + r][l & 15]
    const int row0 = mt * 16 + 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int pix = tile * BN + t * 16 + (lane & 15);
        if (pix >= OHW) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + r;
            if (row >= a.M) continue;
            const int64_t at = ((int64_t)img * a.M + row) * OHW + pix;
            float v = (float)tot[t][r];                              // one rounding of the whole sum
            if (a.bias) v = __fadd_rn(v, a.bias[row]);
            if (a.act) v = __fmul_rn(v > 0.0f ? v : __fmul_rn(v, kDcSlope), kDcSqrt2);
            if (a.addend) {
                v = __fadd_rn(a.addend[at], v);
                if (a.merge) v = __fdiv_rn(v, kDcSqrt2);
            }
            a.out[at] = v;
        }
    }
}

// mode: 0 stride 1 (pad given), 1 stride 2 forward, 2 transposed stride 2 (pad = ks - 1); a.Cin, IH, IW, M, OH, OW, pad are set
static int dc_gemm(DcGemmArgs a, int n, int ks, int mode, hipStream_t st) {
    a.K = a.Cin * ks * ks; a.KS4 = ig_kpad(a.K) / 4;
    const int OHW = a.OH * a.OW, gy = (a.M + kIgBM - 1) / kIgBM, nt = ig_tile_width(OHW, 2, gy), bn = 16 * nt;   // two images counted, whatever n
    a.tiles = (OHW + bn - 1) / bn;
    const dim3 grid((unsigned)((int64_t)n * a.tiles), (unsigned)gy);
    ig_dispatch_nt(nt, [&](auto nt_c) {
        constexpr int NT = decltype(nt_c)::value;
        if (ks == 3 && mode == 0) disc_gemm_kernel<3, 0, NT><<<grid, dim3(256), 0, st>>>(a);
        else if (ks == 3 && mode == 1) disc_gemm_kernel<3, 1, NT><<<grid, dim3(256), 0, st>>>(a);
        else if (ks == 3) disc_gemm_kernel<3, 2, NT><<<grid, dim3(256), 0, st>>>(a);
        else if (mode == 0) disc_gemm_kernel<1, 0, NT><<<grid, dim3(256), 0, st>>>(a);
        else if (mode == 1) disc_gemm_kernel<1, 1, NT><<<grid, dim3(256), 0, st>>>(a);
        else disc_gemm_kernel<1, 2, NT><<<grid, dim3(256), 0, st>>>(a);
    });
    return check_launch("disc(conv)");
}

// the forward convolution of the family: in (n, cin, IH, IW) -> out (n, cout, OH, OW)
static int dc_conv(float* out, const float* in, const float* wfrag, const float* bias, int act, const float* addend, int merge, int n, int cin,
                   int cout, int IH, int IW, int ks, int stride, hipStream_t st) {
    DcGemmArgs a{};
    a.out = out; a.in = in; a.wfrag = wfrag; a.bias = bias; a.act = act; a.addend = addend; a.merge = merge;
    a.Cin = cin; a.IH = IH; a.IW = IW; a.M = cout;
    a.OH = stride == 1 ? IH : (IH - ks) / 2 + 1; a.OW = stride == 1 ? IW : (IW - ks) / 2 + 1;
    a.pad = stride == 1 ? ks / 2 : 0;
    return dc_gemm(a, n, ks, stride == 1 ? 0 : 1, st);
}

static int dc_blur(float* out, const float* in, const float* fir, int64_t planes, int size, int pad0, int pad1, hipStream_t st) {
    return e3dge_upfirdn2d(out, in, fir, planes, size, size, 4, 4, 1, 1, 1, 1, pad0, pad1, pad0, pad1, reinterpret_cast<e3dge_stream_t>(st));
}

// ---- minibatch standard deviation -----------------------------------------------------------------------------------------------
// stylesdf_model.py:1598-1609 with stddev_feat 1
static int dc_group(int B) {
    int g = B < 4 ? B : 4;
    if (B % g) g = B % 3 == 0 ? 3 : 2;
    return B % g ? 0 : g;                                           // 0: the reference's reshape rejects this batch
}

__global__ void __launch_bounds__(256) disc_stddev_kernel(float* __restrict__ cat, float* __restrict__ scalars, const float* __restrict__ feat, int B,
                                                          int group, int C, int HW) {
    __shared__ double red[256];
    const int j = blockIdx.x, n_sub = B / group, tid = threadIdx.x;
    const int64_t N = (int64_t)C * HW;
    double sum = 0.0;
    for (int64_t e = tid; e < N; e += 256) {
        float m = 0.0f;
        for (int g = 0; g < group; ++g) m = __fadd_rn(m, feat[(int64_t)(g * n_sub + j) * N + e]);
        m = __fdiv_rn(m, (float)group);
        float var = 0.0f;
        for (int g = 0; g < group; ++g) {
            const float x = feat[(int64_t)(g * n_sub + j) * N + e];
            const float d = __fsub_rn(x, m);
            var = __fmaf_rn(d, d, var);
            cat[(int64_t)(g * n_sub + j) * (N + HW) + e] = x;
        }
        var = __fdiv_rn(var, (float)group);
        sum += (double)__fsqrt_rn(__fadd_rn(var, 1e-8f));
    }
    red[tid] = sum;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    const float s = (float)(red[0] / (double)N);
    if (tid == 0 && scalars) scalars[j] = s;
    for (int i = tid; i < group * HW; i += 256) {
        const int g = i / HW, p = i - g * HW;
        cat[(int64_t)(g * n_sub + j) * (N + HW) + N + p] = s;
    }
}

static int dc_stddev(float* cat, float* scalars, const float* feat, int B, int C, int HW, hipStream_t st) {
    const int group = dc_group(B);
    disc_stddev_kernel<<<dim3((unsigned)(B / group)), dim3(256), 0, st>>>(cat, scalars, feat, B, group, C, HW);
    return check_launch("disc(stddev)");
}

// ---- head -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) disc_head_kernel(float* __restrict__ hid, const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, int n) {
    constexpr int PER = kDcHeadK / 4 / 256;                        // float4 per thread and row: 8
    __shared__ double red[4][kDcHeadRows * kDcHeadImgs];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int o0 = blockIdx.x * kDcHeadRows;
    float4 wv[kDcHeadRows][PER];
#pragma unroll
    for (int r = 0; r < kDcHeadRows; ++r)
#pragma unroll
        for (int j = 0; j < PER; ++j) wv[r][j] = *reinterpret_cast<const float4*>(w + (int64_t)(o0 + r) * kDcHeadK + (j * 256 + tid) * 4);
    for (int i0 = 0; i0 < n; i0 += kDcHeadImgs) {
        const int cnt = n - i0 < kDcHeadImgs ? n - i0 : kDcHeadImgs;
        double acc[kDcHeadRows][kDcHeadImgs];                      // fp64: the 8192-term sums are rounded to fp32 once
#pragma unroll
        for (int r = 0; r < kDcHeadRows; ++r)
#pragma unroll
            for (int i = 0; i < kDcHeadImgs; ++i) acc[r][i] = 0.0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
#pragma unroll
            for (int i = 0; i < kDcHeadImgs; ++i) {
                if (i < cnt) {
                    const float4 xv = *reinterpret_cast<const float4*>(x + (int64_t)(i0 + i) * kDcHeadK + (j * 256 + tid) * 4);
#pragma unroll
                    for (int r = 0; r < kDcHeadRows; ++r) {
                        double s = acc[r][i];
                        s = fma((double)wv[r][j].x, (double)xv.x, s); s = fma((double)wv[r][j].y, (double)xv.y, s);
                        s = fma((double)wv[r][j].z, (double)xv.z, s); s = fma((double)wv[r][j].w, (double)xv.w, s);
                        acc[r][i] = s;
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kDcHeadRows; ++r)
#pragma unroll
            for (int i = 0; i < kDcHeadImgs; ++i) {
                double s = acc[r][i];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
                if (lane == 0) red[wave][r * kDcHeadImgs + i] = s;
            }
        __syncthreads();
        if (tid < kDcHeadRows * kDcHeadImgs) {
            const int i = tid % kDcHeadImgs, r = tid / kDcHeadImgs;
            if (i < cnt) {
                float v = (float)(((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid]);
                v = __fadd_rn(v, bias[o0 + r]);
                hid[(int64_t)(i0 + i) * kDcHid + o0 + r] = __fmul_rn(v > 0.0f ? v : __fmul_rn(v, kDcSlope), kDcSqrt2);
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kDcHid) disc_head_out_kernel(float* __restrict__ logits, const float* __restrict__ hid, const float* __restrict__ w2,
                                                               const float* __restrict__ b2) {
    __shared__ double red[kDcHid];
    const int img = blockIdx.x, o = threadIdx.x;
    red[o] = (double)hid[(int64_t)img * kDcHid + o] * (double)w2[o];
    __syncthreads();
    for (int off = kDcHid / 2; off > 0; off >>= 1) {
        if (o < off) red[o] += red[o + off];
        __syncthreads();
    }
    if (o == 0) logits[img] = __fadd_rn((float)red[0], b2[0]);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static int dc_pool_factor(const DcNet& n, int height, int width) {
    if (height != width) return 0;
    if (height == n.init) return 1;
    if (n.init != 256) return 0;                                    // pool_256 exists for init_size 256 only
    for (int f = 2; f <= 16; f *= 2)
        if (height == 256 * f) return f;
    return 0;
}

// the forward's (and, from `g0` on, the backward's) workspace, offsets in floats
struct DcWs { int64_t pooled, x[2], t1, blur, act2, cat, hid, stdv, fwd_floats; int64_t g[2], gt[3], gcat, ghid, gpool, total_floats; };

static void dc_ws(const DcNet& net, int64_t n, int f, bool backward, DcWs* d) {
    int64_t off = 0;
    auto take = [&](int64_t floats) { const int64_t at = off; off += (floats + 63) / 64 * 64; return at; };
    const int64_t S = net.init;
    int64_t act = n * net.c[0] * S * S, blur = 64, half = 64;
    for (int i = 0; i < net.n_blocks; ++i) {
        const int64_t s = net.size[i];
        const int64_t b = n * net.c[i] * (s + 1) * (s + 1), h = n * net.c[i + 1] * (s / 2) * (s / 2);
        if (b > blur) blur = b;
        if (h > half) half = h;
    }
    d->pooled = take(f > 1 ? n * net.cin * S * S : 0);
    d->x[0] = take(act); d->x[1] = take(act); d->t1 = take(act);
    d->blur = take(blur); d->act2 = take(half);
    d->cat = take(n * 513 * 16); d->hid = take(n * kDcHid); d->stdv = take(n);
    d->fwd_floats = off;
    if (backward) {
        off = 0;
        d->g[0] = take(act); d->g[1] = take(act);
        d->gt[0] = take(blur); d->gt[1] = take(act); d->gt[2] = take(act);
        d->gcat = take(n * 513 * 16); d->ghid = take(n * kDcHid);
        d->gpool = take(f > 1 ? n * net.cin * S * S : 0);
    }
    d->total_floats = off;
}

// what the saving forward keeps, offsets in floats: every lrelu's output (the backward reads its sign), the last block's output (the
// stddev channel's adjoint) and the stddev scalars
struct DcSaved { int64_t stem, t1[kDcMaxBlocks], act2[kDcMaxBlocks], last, fin, hid, total_floats; };

static void dc_saved(const DcNet& net, int64_t n, DcSaved* d) {
    int64_t off = 0;
    auto take = [&](int64_t floats) { const int64_t at = off; off += (floats + 63) / 64 * 64; return at; };
    d->stem = take(n * net.c[0] * net.init * net.init);
    for (int i = 0; i < net.n_blocks; ++i) {
        const int64_t s = net.size[i];
        d->t1[i] = take(n * net.c[i] * s * s);
        d->act2[i] = take(n * net.c[i + 1] * (s / 2) * (s / 2));
    }
    d->last = take(n * 512 * 16); d->fin = take(n * 512 * 16); d->hid = take(n * kDcHid);
    d->total_floats = off;
}

static bool dc_batch_ok(int n) { return n >= 1 && n <= 1024; }

}  // namespace e3dge

using namespace e3dge;

extern "C" int64_t e3dge_disc_packed_floats(int init_size, int channel_multiplier, int in_channels) {
    DcNet net;
    if (!dc_net(init_size, channel_multiplier, in_channels, &net)) {
        fail(E3DGE_ERR_INVALID_ARG, "disc_packed_floats: init_size=%d channel_multiplier=%d in_channels=%d (a power of two 8..1024, 1..4, 1..16)",
             init_size, channel_multiplier, in_channels);
        return -1;
    }
    DcLayout l;
    dc_layout(net, &l);
    return l.total;
}

extern "C" int e3dge_disc_pack_weights(float* packed, const E3dgeDiscPackSrc* src, e3dge_stream_t stream) {
    E3DGE_REQUIRE(packed && src, "disc_pack_weights: null pointer");
    const E3dgeDiscPackSrc& s = *src;
    DcNet net;
    E3DGE_REQUIRE(dc_net(s.init_size, s.channel_multiplier, s.in_channels, &net),
                  "disc_pack_weights: init_size=%d channel_multiplier=%d in_channels=%d (a power of two 8..1024, 1..4, 1..16)", s.init_size,
                  s.channel_multiplier, s.in_channels);
    E3DGE_REQUIRE(s.stem_w && s.stem_b, "disc_pack_weights: null pointer (stem)");
    for (int i = 0; i < net.n_blocks; ++i)
        E3DGE_REQUIRE(s.conv1_w[i] && s.conv1_b[i] && s.conv2_w[i] && s.conv2_b[i] && s.skip_w[i], "disc_pack_weights: null pointer (block %d)", i);
    E3DGE_REQUIRE(s.final_w && s.final_b, "disc_pack_weights: null pointer (final_conv)");
    E3DGE_REQUIRE(s.lin1_w && s.lin1_b && s.lin2_w && s.lin2_b, "disc_pack_weights: null pointer (final_linear)");
    E3DGE_REQUIRE(s.blur, "disc_pack_weights: null pointer (blur)");
    DcLayout l;
    dc_layout(net, &l);
    hipStream_t st = as_stream(stream);
    auto eq_scale = [](int fan_in) { return (float)(1.0 / sqrt((double)fan_in)); };
    auto conv = [&](int64_t fw, int64_t tw, const float* w, int ci, int co, int ks) {
        const float scale = eq_scale(ci * ks * ks);
        ig_pack(packed + fw, w, ci, co, ks, scale, st);
        ig_pack_t(packed + tw, w, ci, co, ks, scale, st);
    };
    auto copy = [&](int64_t off, const float* from, int64_t n, float scale, int flip) { ig_copy(packed + off, from, n, scale, flip, st); };
    conv(l.stem_w, l.stem_wt, s.stem_w, net.cin, net.c[0], 1);
    copy(l.stem_b, s.stem_b, net.c[0], 1.0f, 0);
    for (int i = 0; i < net.n_blocks; ++i) {
        const int ci = net.c[i], co = net.c[i + 1];
        conv(l.c1_w[i], l.c1_wt[i], s.conv1_w[i], ci, ci, 3); copy(l.c1_b[i], s.conv1_b[i], ci, 1.0f, 0);
        conv(l.c2_w[i], l.c2_wt[i], s.conv2_w[i], ci, co, 3); copy(l.c2_b[i], s.conv2_b[i], co, 1.0f, 0);
        conv(l.sk_w[i], l.sk_wt[i], s.skip_w[i], ci, co, 1);
    }
    conv(l.fin_w, l.fin_wt, s.final_w, 513, 512, 3);
    copy(l.fin_b, s.final_b, 512, 1.0f, 0);
    copy(l.lin1_w, s.lin1_w, (int64_t)kDcHid * kDcHeadK, eq_scale(kDcHeadK), 0); copy(l.lin1_b, s.lin1_b, kDcHid, 1.0f, 0);
    copy(l.lin2_w, s.lin2_w, kDcHid, eq_scale(kDcHid), 0); copy(l.lin2_b, s.lin2_b, 1, 1.0f, 0);
    copy(l.blur, s.blur, 16, 1.0f, 0); copy(l.blur_flip, s.blur, 16, 1.0f, 1);
    return check_launch("disc_pack_weights");
}

// shared validation of the network description and the image size of a forward or backward: 0, or the pool factor
static int dc_shape(const char* who, int n, int height, int width, int init, int cm, int cin, DcNet* net) {
    if (!dc_net(init, cm, cin, net)) {
        fail(E3DGE_ERR_INVALID_ARG, "%s: init_size=%d channel_multiplier=%d in_channels=%d (a power of two 8..1024, 1..4, 1..16)", who, init, cm, cin);
        return 0;
    }
    if (!dc_batch_ok(n)) { fail(E3DGE_ERR_INVALID_ARG, "%s: n=%d (1..1024)", who, n); return 0; }
    if (!dc_group(n)) { fail(E3DGE_ERR_INVALID_ARG, "%s: n=%d has no minibatch-stddev group (the batch must be a multiple of 4, 3 or 2, or below 4)", who, n); return 0; }
    const int f = dc_pool_factor(*net, height, width);
    if (!f) fail(E3DGE_ERR_INVALID_ARG, "%s: height=%d width=%d (init_size %d, or 256 times 2, 4, 8 or 16 for init_size 256)", who, height, width, init);
    return f;
}

extern "C" int64_t e3dge_disc_ws_bytes(int n, int height, int width, int init_size, int channel_multiplier, int in_channels, int backward) {
    DcNet net;
    const int f = dc_shape("disc_ws_bytes", n, height, width, init_size, channel_multiplier, in_channels, &net);
    if (!f) return -1;
    DcWs d;
    dc_ws(net, n, f, backward != 0, &d);
    return d.total_floats * (int64_t)sizeof(float);
}

extern "C" int64_t e3dge_disc_saved_bytes(int n, int init_size, int channel_multiplier, int in_channels) {
    DcNet net;
    if (!dc_shape("disc_saved_bytes", n, init_size, init_size, init_size, channel_multiplier, in_channels, &net)) return -1;
    DcSaved d;
    dc_saved(net, n, &d);
    return d.total_floats * (int64_t)sizeof(float);
}

extern "C" int e3dge_disc_forward(const E3dgeDiscArgs* args, e3dge_stream_t stream) {
    E3DGE_REQUIRE(args, "disc_forward: null argument struct");
    const E3dgeDiscArgs& a = *args;
    DcNet net;
    const int f = dc_shape("disc_forward", a.n, a.height, a.width, a.init_size, a.channel_multiplier, a.in_channels, &net);
    if (!f) return E3DGE_ERR_INVALID_ARG;
    E3DGE_REQUIRE(a.packed && a.images && a.logits && a.ws, "disc_forward: null pointer");
    const int n = a.n;
    DcWs d;
    dc_ws(net, n, f, false, &d);
    E3DGE_REQUIRE(a.ws_bytes >= d.total_floats * (int64_t)sizeof(float), "disc_forward: workspace of %lld bytes, %lld needed", (long long)a.ws_bytes,
                  (long long)(d.total_floats * (int64_t)sizeof(float)));
    DcSaved sv{};
    const bool saving = a.saved != nullptr;
    if (saving) {
        dc_saved(net, n, &sv);
        E3DGE_REQUIRE(a.saved_bytes >= sv.total_floats * (int64_t)sizeof(float), "disc_forward: saved state of %lld bytes, %lld needed",
                      (long long)a.saved_bytes, (long long)(sv.total_floats * (int64_t)sizeof(float)));
    }
    DcLayout l;
    dc_layout(net, &l);
    hipStream_t st = as_stream(stream);
    float* ws = static_cast<float*>(a.ws);
    float* S = static_cast<float*>(a.saved);
    const float* P = a.packed;
    int rc;
    auto tap = [&](int t, const float* from, int64_t floats) {
        if (a.taps[t]) (void)hipMemcpyAsync(a.taps[t], from, floats * sizeof(float), hipMemcpyDeviceToDevice, st);
    };
    const float* img = a.images;
    if (f > 1) {
        if ((rc = e3dge_avgpool_fwd(ws + d.pooled, a.images, (int64_t)n * net.cin, a.height, a.width, f, stream))) return rc;
        img = ws + d.pooled;
    }
    float* x = saving ? S + sv.stem : ws + d.x[0];                  // block i reads x[i & 1] (block 0: the stem's output) and writes x[(i + 1) & 1]
    if ((rc = dc_conv(x, img, P + l.stem_w, P + l.stem_b, 1, nullptr, 0, n, net.cin, net.c[0], net.init, net.init, 1, 1, st))) return rc;
    for (int i = 0; i < net.n_blocks; ++i) {
        const int ci = net.c[i], co = net.c[i + 1], s = net.size[i], h = s / 2;
        float* t1 = saving ? S + sv.t1[i] : ws + d.t1;
        float* act2 = saving ? S + sv.act2[i] : ws + d.act2;
        float* out = (saving && i == net.n_blocks - 1) ? S + sv.last : ws + d.x[(i + 1) & 1];
        float* blur = ws + d.blur;
        if ((rc = dc_conv(t1, x, P + l.c1_w[i], P + l.c1_b[i], 1, nullptr, 0, n, ci, ci, s, s, 3, 1, st))) return rc;
        if ((rc = dc_blur(blur, t1, P + l.blur, (int64_t)n * ci, s, 2, 2, st))) return rc;
        if ((rc = dc_conv(act2, blur, P + l.c2_w[i], P + l.c2_b[i], 1, nullptr, 0, n, ci, co, s + 1, s + 1, 3, 2, st))) return rc;
        if ((rc = dc_blur(blur, x, P + l.blur, (int64_t)n * ci, s, 1, 1, st))) return rc;
        if ((rc = dc_conv(out, blur, P + l.sk_w[i], nullptr, 0, act2, 1, n, ci, co, s - 1, s - 1, 1, 2, st))) return rc;
        tap(i, out, (int64_t)n * co * h * h);
        x = out;
    }
    float* cat = ws + d.cat;
    float* stdv = ws + d.stdv;
    if ((rc = dc_stddev(cat, stdv, x, n, 512, 16, st))) return rc;
    tap(E3DGE_DISC_TAP_STDDEV, stdv, n / dc_group(n));
    float* fin = saving ? S + sv.fin : ws + d.t1;                    // (t1 is free: the blocks are done)
    if ((rc = dc_conv(fin, cat, P + l.fin_w, P + l.fin_b, 1, nullptr, 0, n, 513, 512, 4, 4, 3, 1, st))) return rc;
    tap(E3DGE_DISC_TAP_FINAL, fin, (int64_t)n * 512 * 16);
    float* hid = saving ? S + sv.hid : ws + d.hid;
    disc_head_kernel<<<dim3(kDcHid / kDcHeadRows), dim3(256), 0, st>>>(hid, fin, P + l.lin1_w, P + l.lin1_b, n);
    if ((rc = check_launch("disc_forward(head)"))) return rc;
    disc_head_out_kernel<<<dim3((unsigned)n), dim3(kDcHid), 0, st>>>(a.logits, hid, P + l.lin2_w, P + l.lin2_b);
    return check_launch("disc_forward(head out)");
}

static bool dc_conv_sizes_ok(int n, int cin, int cout, int height, int width, int ksize, int stride) {
    return n >= 1 && n <= 4096 && cin >= 1 && cin <= 4096 && cout >= 1 && cout <= 4096 && height >= ksize && width >= ksize && height <= 4096 &&
           width <= 4096 && (ksize == 1 || ksize == 3) && (stride == 1 || stride == 2) &&
           (int64_t)(cin > cout ? cin : cout) * height * width < ((int64_t)1 << 31);
}

extern "C" int e3dge_disc_conv(float* out, const float* in, const float* w, float* wfrag, const float* bias, const float* addend, int n, int cin,
                               int cout, int height, int width, int ksize, int stride, int act, int merge, float scale, e3dge_stream_t stream) {
    E3DGE_REQUIRE(out && in && w && wfrag, "disc_conv: null pointer");
    E3DGE_REQUIRE(dc_conv_sizes_ok(n, cin, cout, height, width, ksize, stride),
                  "disc_conv: n=%d cin=%d cout=%d height=%d width=%d ksize=%d stride=%d (n, channels 1..4096, sizes ksize..4096, ksize 1 or 3, stride 1 or 2)",
                  n, cin, cout, height, width, ksize, stride);
    E3DGE_REQUIRE(!merge || addend, "disc_conv: merge without an addend");
    hipStream_t st = as_stream(stream);
    ig_pack(wfrag, w, cin, cout, ksize, scale, st);
    int rc;
    if ((rc = check_launch("disc_conv(pack)"))) return rc;
    return dc_conv(out, in, wfrag, bias, act != 0, addend, merge != 0, n, cin, cout, height, width, ksize, stride, st);
}

extern "C" int e3dge_disc_stddev(float* cat, float* scalars, const float* feat, int n, int channels, int hw, e3dge_stream_t stream) {
    E3DGE_REQUIRE(cat && feat, "disc_stddev: null pointer");
    E3DGE_REQUIRE(dc_batch_ok(n), "disc_stddev: n=%d (1..1024)", n);
    E3DGE_REQUIRE(dc_group(n), "disc_stddev: n=%d has no minibatch-stddev group (the batch must be a multiple of 4, 3 or 2, or below 4)", n);
    E3DGE_REQUIRE(channels >= 1 && channels <= 65536 && hw >= 1 && hw <= 65536, "disc_stddev: channels=%d hw=%d (1..65536)", channels, hw);
    return dc_stddev(cat, scalars, feat, n, channels, hw, as_stream(stream));
}

#include "disc_bwd.h"
