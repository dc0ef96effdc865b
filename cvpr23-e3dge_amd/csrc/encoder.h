// The E0 image encoder, forward, eval form: image -> the (B, 9, 256) renderer latent and the (B, 512) decoder latent, with the p32 / p64 pyramid maps.
// Included at the end of idnet.hip: the body is the identity network's 24 bottleneck_IR_SE units on idnet_conv_kernel / idnet_se_kernel /
// idnet_merge_kernel, at a run-time square input size.
//
// Reference: HybridGradualStyleEncoder_V2 (project/models/encoders/fpn_encoders.py:266-433), GradualStyleBlock (helpers.py:472-497), EqualLinear
// (stylesdf_model.py:210-249), BatchNorm with its running statistics.
//
//   x -> input_layer -> 24 units, keeping units 2, 6, 20, 23 (c128, c64, c32, c16)
//   p32 = up2(c16) + latlayer256(c32);  p64 = up2(p32) + latlayer128(c64);  p128 = up2(p64) + latlayer64(c128)      (bilinear, align_corners)
//   head(map): log2(dim) x [conv3x3 stride 2 pad 1, bias, LeakyReLU(0.01)] down to 1x1, then EqualLinear
//
// Kernels beside the body's:
//   enc_lateral_kernel    implicit GEMM of conv_igemm.h with K = the lateral's input channels, M = 512, N = the fine map's pixels of one
//                         image.  Epilogue: (sum + bias) rounded, then added to the bilinear sample of the coarse map (rounded on its own):
//                         the reference's two ops.
//   enc_head_conv_kernel  the same GEMM for 3x3 stride 2 pad 1, bias and LeakyReLU, for G heads in one launch: grid (pixel tile x image,
//                         channel block, head).  `shared`: every head reads the same input (a head's first layer on a pyramid map).
//   enc_tail_kernel       from the 2x2 (or 1x1) map on a layer is a matrix-vector product per image: a 2x2 -> 1x1 layer has four live taps
//                         of nine, a 1x1 -> 1x1 layer one, and the packed image holds the live taps alone (enc_pack_live_kernel).  One
//                         wave per output channel and head, k ascending per lane, a fixed butterfly over the lanes; up to 8 images per
//                         pass over the weights.  EqualLinear is the same kernel without the activation, its weight times 1 / sqrt(in)
//                         rounded once at packing.
// Every sum runs in a fixed order and no kernel uses atomics; tiles never straddle images and their width comes from the layer alone
// (ig_tile_width), so results are bit-reproducible and an image's values do not depend on the batch.
// Launch counts, measured times and what bounds each kernel: DESIGN.md 4.16.
#pragma once

namespace e3dge {

constexpr int kEncHeads = E3DGE_ENC_HEADS, kEncMaxConvs = E3DGE_ENC_MAX_HEAD_CONVS, kEncLat = 512, kEncStyle = 256;
constexpr int kEncBodyConvs = 52, kEncBodyBns = 52, kEncBodySrc = 6 + kIdUnits * 13 + 3 * 5, kEncKeepUnits[4] = {2, 6, 20, 23};
constexpr int kEncTailImgs = 8;
constexpr float kEncSlope = 0.01f;                                  // nn.LeakyReLU()

// ---- lateral: fine = up2(coarse) + (conv1x1(in) + bias) ----------------------------------------------------------------------------
struct EncLatArgs {
    float* out; const float* coarse; const float* in; const float* wfrag; const float* bias;
    int Cin, H, W, CH, CW, Cout, KS4, tiles;
    float sy, sx;                                                   // (CH - 1) / (H - 1), (CW - 1) / (W - 1) in fp32; 0 when the fine size is 1
};

template <int NT>
__global__ void __launch_bounds__(256) enc_lateral_kernel(EncLatArgs a) {
    constexpr int BN = IgTile<NT>::BN, ROWS = IgTile<NT>::ROWS, PER = IgTile<NT>::PER;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mt = blockIdx.y * (kIgBM / 16) + wave;
    const int HW = a.H * a.W, K = a.Cin;
    const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
    const int sn = tid % BN, srow = tid / BN;
    const int spix = tile * BN + sn;
    const bool n_ok = spix < HW;
    const float* __restrict__ src = a.in + (int64_t)img * a.Cin * HW;
    auto fetch = [&](int k0, float (&v)[PER]) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = k0 + srow + i * ROWS;
            v[i] = (n_ok && k < K) ? src[(int64_t)k * HW + spix] : 0.0f;
        }
    };
    f32x4 acc[NT][2];
    ig_k_loop<NT, 2, false>(acc, a.wfrag + (int64_t)mt * a.KS4 * 64 + lane, a.KS4 / (kIgKC / 4), true, fetch, [](int, bool) {});
    const int row0 = mt * 16 + 4 * (lane >> 4);
    const int CHW = a.CH * a.CW;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int pix = tile * BN + t * 16 + (lane & 15);
        if (pix >= HW) continue;
        const int oy = pix / a.W, ox = pix - oy * a.W;
        // PyTorch's align_corners source index: scale * dst, index0 = trunc, index1 = index0 + (index0 < in - 1), lambda1 = src - index0
        const float fy = __fmul_rn(a.sy, (float)oy), fx = __fmul_rn(a.sx, (float)ox);
        const int y0 = min((int)fy, a.CH - 1), x0 = min((int)fx, a.CW - 1);       // (never past the map, whatever the rounding of the scale)
        const int y1 = y0 + (y0 < a.CH - 1), x1 = x0 + (x0 < a.CW - 1);
        const float ly = fminf(fmaxf(__fsub_rn(fy, (float)y0), 0.0f), 1.0f), lx = fminf(fmaxf(__fsub_rn(fx, (float)x0), 0.0f), 1.0f);
        const float hy = __fsub_rn(1.0f, ly), hx = __fsub_rn(1.0f, lx);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + r;
            const float* __restrict__ c = a.coarse + ((int64_t)img * a.Cout + row) * CHW;
            const float top = __fadd_rn(__fmul_rn(hx, c[y0 * a.CW + x0]), __fmul_rn(lx, c[y0 * a.CW + x1]));
            const float bot = __fadd_rn(__fmul_rn(hx, c[y1 * a.CW + x0]), __fmul_rn(lx, c[y1 * a.CW + x1]));
            const float up = __fadd_rn(__fmul_rn(hy, top), __fmul_rn(ly, bot));
            const float v = __fadd_rn(__fadd_rn(acc[t][0][r], acc[t][1][r]), a.bias[row]);
            a.out[((int64_t)img * a.Cout + row) * HW + pix] = __fadd_rn(up, v);            // fpn_encoders.py:366-369
        }
    }
}

static int enc_lateral(float* out, const float* coarse, const float* in, const float* wfrag, const float* bias, int n, int Cin, int Cout, int CH,
                       int CW, int H, int W, hipStream_t st) {
    EncLatArgs a;
    a.out = out; a.coarse = coarse; a.in = in; a.wfrag = wfrag; a.bias = bias;
    a.Cin = Cin; a.H = H; a.W = W; a.CH = CH; a.CW = CW; a.Cout = Cout; a.KS4 = ig_kpad(Cin) / 4;
    a.sy = H > 1 ? (float)(CH - 1) / (float)(H - 1) : 0.0f;
    a.sx = W > 1 ? (float)(CW - 1) / (float)(W - 1) : 0.0f;
    const int HW = H * W, nt = ig_tile_width(HW, 2, Cout / kIgBM), bn = 16 * nt;
    a.tiles = (HW + bn - 1) / bn;
    const dim3 grid((unsigned)((int64_t)n * a.tiles), (unsigned)(Cout / kIgBM));
    ig_dispatch_nt(nt, [&](auto nt_c) { enc_lateral_kernel<decltype(nt_c)::value><<<grid, dim3(256), 0, st>>>(a); });
    return check_launch("enc(lateral)");
}

// ---- grouped head convolution: 3x3, stride 2, pad 1, bias, LeakyReLU -------------------------------------------------------------
struct EncHeadArgs {
    float* out; const float* in; const float* wfrag; const float* bias;
    int Cin, IH, IW, Cout, OH, OW, K, KS4, tiles, n, shared;
};

template <int NT>
__global__ void __launch_bounds__(256) enc_head_conv_kernel(EncHeadArgs a) {
    constexpr int BN = IgTile<NT>::BN, ROWS = IgTile<NT>::ROWS, PER = IgTile<NT>::PER;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mt = blockIdx.y * (kIgBM / 16) + wave, g = blockIdx.z;
    const int OHW = a.OH * a.OW, IH = a.IH, IW = a.IW, K = a.K;
    const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
    const int sn = tid % BN, srow = tid / BN;
    const int spix = tile * BN + sn;
    const bool n_ok = spix < OHW;
    const int soy = spix / a.OW, sox = spix - soy * a.OW;
    const int iy0 = soy * 2 - 1, ix0 = sox * 2 - 1;
    const float* __restrict__ src = a.in + ((int64_t)(a.shared ? 0 : g * a.n) + img) * a.Cin * IH * IW;
    auto fetch = [&](int k0, float (&v)[PER]) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = k0 + srow + i * ROWS;
            const auto [ci, r, s] = ig_decode<3>(k);
            const int iy = iy0 + r, ix = ix0 + s;
            float x = 0.0f;
            if (n_ok && k < K && iy >= 0 && iy < IH && ix >= 0 && ix < IW) x = src[((int64_t)ci * IH + iy) * IW + ix];
            v[i] = x;
        }
    };
    f32x4 acc[NT][2];
    ig_k_loop<NT, 2, false>(acc, a.wfrag + ((int64_t)g * (a.Cout / 16) + mt) * a.KS4 * 64 + lane, a.KS4 / (kIgKC / 4), true, fetch, [](int, bool) {});
    const int row0 = mt * 16 + 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int pix = tile * BN + t * 16 + (lane & 15);
        if (pix >= OHW) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + r;
            float v = __fadd_rn(__fadd_rn(acc[t][0][r], acc[t][1][r]), a.bias[g * a.Cout + row]);
            v = v > 0.0f ? v : __fmul_rn(v, kEncSlope);
            a.out[(((int64_t)g * a.n + img) * a.Cout + row) * OHW + pix] = v;
        }
    }
}

static int enc_head_out(int in) { return (in + 1) / 2; }             // 3x3, stride 2, pad 1

static int enc_head_conv(float* out, const float* in, const float* wfrag, const float* bias, int n, int G, int shared, int Cin, int Cout, int IH,
                         int IW, hipStream_t st) {
    EncHeadArgs a;
    a.out = out; a.in = in; a.wfrag = wfrag; a.bias = bias;
    a.Cin = Cin; a.IH = IH; a.IW = IW; a.Cout = Cout; a.OH = enc_head_out(IH); a.OW = enc_head_out(IW);
    a.K = Cin * 9; a.KS4 = ig_kpad(a.K) / 4; a.n = n; a.shared = shared;
    const int OHW = a.OH * a.OW, nt = ig_tile_width(OHW, 2, (int64_t)(Cout / kIgBM) * G), bn = 16 * nt;
    a.tiles = (OHW + bn - 1) / bn;
    const dim3 grid((unsigned)((int64_t)n * a.tiles), (unsigned)(Cout / kIgBM), (unsigned)G);
    ig_dispatch_nt(nt, [&](auto nt_c) { enc_head_conv_kernel<decltype(nt_c)::value><<<grid, dim3(256), 0, st>>>(a); });
    return check_launch("enc(head conv)");
}

// ---- head tail ---------------------------------------------------------------------------------------------------------------------
// dst[co][ci * T + t] = w[co][ci][1 + t / 2][1 + t % 2]: the taps of a 3x3 stride-2 pad-1 layer that see a 2x2 (T = 4) or 1x1 (T = 1) input
static __global__ void __launch_bounds__(256) enc_pack_live_kernel(float* __restrict__ dst, const float* __restrict__ w, int T, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int t = (int)(i % T);
    dst[i] = w[(i / T) * 9 + (1 + t / 2) * 3 + 1 + t % 2];
}

static void enc_pack_live(float* dst, const float* w, int cout, int cin, int T, hipStream_t st) {
    const int64_t total = (int64_t)cout * cin * T;
    enc_pack_live_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(dst, w, T, total);
}

// out[g out_g + img out_img + co] = act(b[g][co] + sum_k w[g][co][k] x[g][img][k]); K a multiple of 4
template <bool ACT>
__global__ void __launch_bounds__(256) enc_tail_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ b, int n, int K, int C, int64_t out_g, int64_t out_img) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int co = blockIdx.x * 4 + wave, g = blockIdx.y;
    const float* __restrict__ wr = w + ((int64_t)g * C + co) * K;
    const float bias = b[g * C + co];
    for (int i0 = 0; i0 < n; i0 += kEncTailImgs) {
        const int cnt = n - i0 < kEncTailImgs ? n - i0 : kEncTailImgs;
        float acc[kEncTailImgs];
#pragma unroll
        for (int i = 0; i < kEncTailImgs; ++i) acc[i] = 0.0f;
        for (int k4 = lane; k4 < K / 4; k4 += 64) {
            const float4 wv = *reinterpret_cast<const float4*>(wr + k4 * 4);
#pragma unroll
            for (int i = 0; i < kEncTailImgs; ++i) {
                if (i < cnt) {
                    const float4 xv = *reinterpret_cast<const float4*>(x + ((int64_t)g * n + i0 + i) * K + k4 * 4);
                    float s = acc[i];
                    s = __fmaf_rn(wv.x, xv.x, s); s = __fmaf_rn(wv.y, xv.y, s);
                    s = __fmaf_rn(wv.z, xv.z, s); s = __fmaf_rn(wv.w, xv.w, s);
                    acc[i] = s;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < kEncTailImgs; ++i) {
            float s = acc[i];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s = __fadd_rn(s, __shfl_xor(s, off, kWave));
            if (lane == 0 && i < cnt) {
                float v = __fadd_rn(s, bias);
                if (ACT) v = v > 0.0f ? v : __fmul_rn(v, kEncSlope);
                out[(int64_t)g * out_g + (int64_t)(i0 + i) * out_img + co] = v;
            }
        }
    }
}

static int enc_tail(float* out, const float* x, const float* w, const float* b, int n, int G, int K, int C, int64_t out_g, int64_t out_img, bool act,
                    hipStream_t st) {
    const dim3 grid((unsigned)(C / 4), (unsigned)G);
    if (act) enc_tail_kernel<true><<<grid, dim3(256), 0, st>>>(out, x, w, b, n, K, C, out_g, out_img);
    else enc_tail_kernel<false><<<grid, dim3(256), 0, st>>>(out, x, w, b, n, K, C, out_g, out_img);
    return check_launch("enc(head tail)");
}

// ---- configuration, packed image, workspace ------------------------------------------------------------------------------------------
struct EncCfg { int size, geo, tex, dec; };

static bool enc_dim_ok(int d) { return d == 32 || d == 64 || d == 128; }
static int enc_log2(int d) { int l = 0; while ((1 << l) < d) ++l; return l; }
static bool enc_cfg_ok(const EncCfg& c) {
    return c.size >= 32 && c.size <= 256 && c.size % 16 == 0 && enc_dim_ok(c.geo) && enc_dim_ok(c.tex) && (c.dec == 0 || c.dec == 1);
}

// heads that run together: the same layer count on the same map
struct EncGroup { int heads, head0, convs, level, cout, size; };     // level: 0 = p32, 1 = p64, 2 = p128; head 9 is the decoder's
struct EncPlan {
    int n_groups;
    EncGroup g[3];
    int in_size[3][kEncMaxConvs];                                    // a layer whose input is larger than 2 is a convolution, the rest are the tail
    int64_t w_off[3][kEncMaxConvs], b_off[3][kEncMaxConvs], lin_w[3], lin_b[3];
    int64_t body_w[kEncBodyConvs], body_bn[kEncBodyBns], prelu[kIdUnits + 1], fc1[kIdUnits], fc2[kIdUnits], lat_w[3], lat_b[3], total;
    int body_cin[kEncBodyConvs], body_cout[kEncBodyConvs], body_ks[kEncBodyConvs], bn_c[kEncBodyBns], prelu_c[kIdUnits + 1];
    int n_src;
};
constexpr int kEncLatCin[3] = {256, 128, 64};                        // latlayer256 (-> p32), latlayer128 (-> p64), latlayer64 (-> p128)

static EncPlan enc_plan(const EncCfg& c) {
    EncPlan p{};
    const int tex_level = c.tex == 64 ? 1 : 0;                       // fpn_encoders.py:406-410
    if (c.geo == c.tex && tex_level == 0) {
        p.g[p.n_groups++] = {9, 0, enc_log2(c.geo), 0, kEncStyle, c.size / 8};
    } else {
        p.g[p.n_groups++] = {6, 0, enc_log2(c.geo), 0, kEncStyle, c.size / 8};
        p.g[p.n_groups++] = {3, 6, enc_log2(c.tex), tex_level, kEncStyle, tex_level ? c.size / 4 : c.size / 8};
    }
    if (c.dec) p.g[p.n_groups++] = {1, 9, 7, 2, kEncLat, c.size / 2};
    int64_t off = 0;
    auto take = [&](int64_t floats) { const int64_t at = off; off += (floats + 63) / 64 * 64; return at; };
    auto conv = [&](int i, int ci, int co, int ks) { p.body_cin[i] = ci; p.body_cout[i] = co; p.body_ks[i] = ks; p.body_w[i] = take((int64_t)co * ig_kpad(ci * ks * ks)); };
    auto bn = [&](int i, int ch) { p.bn_c[i] = ch; p.body_bn[i] = take(2 * (int64_t)ch); };
    conv(0, 3, 64, 3); bn(0, 64);
    p.prelu_c[0] = 64; p.prelu[0] = take(64);
    for (int u = 0; u < kIdUnits; ++u) {
        const IdUnit q = id_unit(u);
        conv(1 + 2 * u, q.cin, q.depth, 3); conv(2 + 2 * u, q.depth, q.depth, 3);
        bn(1 + 2 * u, q.cin); bn(2 + 2 * u, q.depth);
        p.prelu_c[1 + u] = q.depth; p.prelu[1 + u] = take(q.depth);
        p.fc1[u] = take((int64_t)q.depth * (q.depth / 16)); p.fc2[u] = take((int64_t)q.depth * (q.depth / 16));
        if (q.shortcut >= 0) { conv(49 + q.shortcut, q.cin, q.depth, 1); bn(49 + q.shortcut, q.depth); }
    }
    for (int i = 0; i < 3; ++i) { p.lat_w[i] = take((int64_t)kEncLat * ig_kpad(kEncLatCin[i])); p.lat_b[i] = take(kEncLat); }
    p.n_src = kEncBodySrc + 6;
    for (int gi = 0; gi < p.n_groups; ++gi) {
        const EncGroup& g = p.g[gi];
        int s = g.size;
        for (int l = 0; l < g.convs; ++l) {
            const int cin = l == 0 ? kEncLat : g.cout;
            p.in_size[gi][l] = s;
            p.w_off[gi][l] = take(s > 2 ? (int64_t)g.heads * g.cout * ig_kpad(cin * 9) : (int64_t)g.heads * g.cout * cin * s * s);
            p.b_off[gi][l] = take((int64_t)g.heads * g.cout);
            s = enc_head_out(s);
        }
        p.lin_w[gi] = take((int64_t)g.heads * g.cout * g.cout);
        p.lin_b[gi] = take((int64_t)g.heads * g.cout);
        p.n_src += g.heads * (2 * g.convs + 2);
    }
    p.total = off;
    return p;
}

struct EncWs { int64_t buf[3], res, sc, plane, gate, keep[4], p128, act[2], total_bytes; };

static bool enc_ws(int64_t n, const EncCfg& c, const EncPlan& p, EncWs* d) {
    if (n < 1 || n > 256 || !enc_cfg_ok(c)) return false;
    int64_t off = 0;
    auto take = [&](int64_t floats) { const int64_t at = off; off += (floats + 63) / 64 * 64; return at; };
    const int64_t S = c.size;
    for (int q = 0; q < 3; ++q) d->buf[q] = take(n * 64 * S * S);
    d->res = take(n * 64 * (S / 2) * (S / 2));
    d->sc = take(n * 128 * (S / 4) * (S / 4));
    int64_t per = 0;
    int size = c.size;
    for (int u = 0; u < kIdUnits; ++u) {
        const IdUnit q = id_unit(u);
        size = id_out_size(size, q.stride);
        const int64_t pl = (int64_t)q.depth * id_tiles(size * size, q.depth);
        if (pl > per) per = pl;
    }
    d->plane = take(n * per);
    d->gate = take(n * 512);
    d->keep[0] = take(n * 64 * (S / 2) * (S / 2));
    d->keep[1] = take(n * 128 * (S / 4) * (S / 4));
    d->keep[2] = take(n * 256 * (S / 8) * (S / 8));
    d->keep[3] = take(n * 512 * (S / 16) * (S / 16));
    d->p128 = take(c.dec ? n * kEncLat * (S / 2) * (S / 2) : 0);
    int64_t act = 0;
    for (int gi = 0; gi < p.n_groups; ++gi) {
        const int o = enc_head_out(p.g[gi].size);
        const int64_t a = n * p.g[gi].heads * p.g[gi].cout * o * o;
        if (a > act) act = a;
    }
    d->act[0] = take(act); d->act[1] = take(act);
    d->total_bytes = off * (int64_t)sizeof(float);
    return true;
}

// ---- the body at a run-time size ---------------------------------------------------------------------------------------------------
static int enc_body(float* const keep[4], const float* images, const float* P, const EncPlan& l, float* ws, const EncWs& d, int n, int S,
                    hipStream_t st) {
    int rc;
    float* bufs[2] = {ws + d.buf[0], ws + d.buf[1]};
    float* t1 = ws + d.buf[2];
    float* res = ws + d.res;
    float* sc = ws + d.sc;
    float* plane = ws + d.plane;
    float* gate = ws + d.gate;
    float* x = bufs[0];
    if ((rc = id_conv(x, images, P + l.body_w[0], nullptr, P + l.body_bn[0], P + l.prelu[0], nullptr, n, 3, 64, S, S, 3, 1, st))) return rc;
    int size = S, kept = 0;
    for (int u = 0; u < kIdUnits; ++u) {
        const IdUnit q = id_unit(u);
        const int osize = id_out_size(size, q.stride), c1 = 1 + 2 * u, c2 = 2 + 2 * u;
        float* y = (kept < 4 && u == kEncKeepUnits[kept]) ? keep[kept++] : (x == bufs[0] ? bufs[1] : bufs[0]);
        if ((rc = id_conv(t1, x, P + l.body_w[c1], P + l.body_bn[c1], nullptr, P + l.prelu[1 + u], nullptr, n, q.cin, q.depth, size, size, 3, 1, st)))
            return rc;
        if ((rc = id_conv(res, t1, P + l.body_w[c2], nullptr, P + l.body_bn[c2], nullptr, plane, n, q.depth, q.depth, size, size, 3, q.stride, st)))
            return rc;
        if (q.shortcut >= 0) {
            const int cs = 49 + q.shortcut;
            if ((rc = id_conv(sc, x, P + l.body_w[cs], nullptr, P + l.body_bn[cs], nullptr, nullptr, n, q.cin, q.depth, size, size, 1, q.stride, st)))
                return rc;
        }
        idnet_se_kernel<false><<<dim3((unsigned)n), dim3(256), 0, st>>>(gate, plane, P + l.fc1[u], P + l.fc2[u], q.depth,
                                                                        id_tiles(osize * osize, q.depth), osize * osize, nullptr, nullptr, 0);
        if ((rc = check_launch("enc(se)"))) return rc;
        const int64_t total = (int64_t)n * q.depth * osize * osize;
        idnet_merge_kernel<false><<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(y, res, gate, q.shortcut >= 0 ? sc : nullptr, x, osize,
                                                                                               osize, size, size, q.stride, total, nullptr, 0);
        if ((rc = check_launch("enc(merge)"))) return rc;
        x = y;
        size = osize;
    }
    return E3DGE_OK;
}

// one group of heads from its pyramid map to its latents: out[g out_g + img out_img + c]
static int enc_heads(float* out, int64_t out_g, int64_t out_img, const float* map, const float* P, const EncPlan& l, int gi, float* const act[2],
                     int n, hipStream_t st) {
    const EncGroup& g = l.g[gi];
    int rc, pp = 0;
    const float* in = map;
    for (int i = 0; i < g.convs; ++i) {
        const int s = l.in_size[gi][i], cin = i == 0 ? kEncLat : g.cout;
        if (s > 2) rc = enc_head_conv(act[pp], in, P + l.w_off[gi][i], P + l.b_off[gi][i], n, g.heads, i == 0, cin, g.cout, s, s, st);
        else rc = enc_tail(act[pp], in, P + l.w_off[gi][i], P + l.b_off[gi][i], n, g.heads, cin * s * s, g.cout, (int64_t)n * g.cout, g.cout, true, st);
        if (rc) return rc;
        in = act[pp];
        pp ^= 1;
    }
    return enc_tail(out, in, P + l.lin_w[gi], P + l.lin_b[gi], n, g.heads, g.cout, g.cout, out_g, out_img, false, st);
}

}  // namespace e3dge

using namespace e3dge;

extern "C" int64_t e3dge_enc_packed_floats(int size, int geo_dim, int tex_dim, int enable_decoder) {
    const EncCfg c{size, geo_dim, tex_dim, enable_decoder};
    if (!enc_cfg_ok(c)) {
        fail(E3DGE_ERR_INVALID_ARG, "enc_packed_floats: size=%d geo_dim=%d tex_dim=%d enable_decoder=%d (size a multiple of 16 in 32..256, dims 32, 64 or 128)",
             size, geo_dim, tex_dim, enable_decoder);
        return -1;
    }
    return enc_plan(c).total;
}

extern "C" int e3dge_enc_pack_weights(float* packed, const float* const* src, int n_src, int size, int geo_dim, int tex_dim, int enable_decoder,
                                      e3dge_stream_t stream) {
    E3DGE_REQUIRE(packed && src, "enc_pack_weights: null pointer");
    const EncCfg c{size, geo_dim, tex_dim, enable_decoder};
    E3DGE_REQUIRE(enc_cfg_ok(c), "enc_pack_weights: size=%d geo_dim=%d tex_dim=%d enable_decoder=%d", size, geo_dim, tex_dim, enable_decoder);
    const EncPlan l = enc_plan(c);
    E3DGE_REQUIRE(n_src == l.n_src, "enc_pack_weights: n_src=%d, %d source tensors expected", n_src, l.n_src);
    for (int i = 0; i < n_src; ++i) E3DGE_REQUIRE(src[i], "enc_pack_weights: null pointer (source %d)", i);
    hipStream_t st = as_stream(stream);
    int at = 0;
    auto next = [&]() { return src[at++]; };
    auto copy = [&](int64_t off, int64_t cnt) { ig_copy(packed + off, next(), cnt, 1.0f, 0, st); };
    auto conv = [&](int i) { ig_pack(packed + l.body_w[i], next(), l.body_cin[i], l.body_cout[i], l.body_ks[i], 1.0f, st); };
    auto bn = [&](int i) {
        const float* gamma = next(); const float* beta = next(); const float* mean = next(); const float* var = next();
        idnet_pack_bn_kernel<<<dim3((unsigned)((l.bn_c[i] + 255) / 256)), dim3(256), 0, st>>>(packed + l.body_bn[i], gamma, beta, mean, var, l.bn_c[i]);
    };
    conv(0); bn(0); copy(l.prelu[0], 64);
    for (int u = 0; u < kIdUnits; ++u) {                              // res_layer.0 .. 5, then the shortcut
        const IdUnit q = id_unit(u);
        const int64_t m = (int64_t)q.depth * (q.depth / 16);
        bn(1 + 2 * u); conv(1 + 2 * u); copy(l.prelu[1 + u], q.depth); conv(2 + 2 * u); bn(2 + 2 * u);
        copy(l.fc1[u], m); copy(l.fc2[u], m);
        if (q.shortcut >= 0) { conv(49 + q.shortcut); bn(49 + q.shortcut); }
    }
    for (int i = 0; i < 3; ++i) {
        ig_pack(packed + l.lat_w[i], next(), kEncLatCin[i], kEncLat, 1, 1.0f, st);
        copy(l.lat_b[i], kEncLat);
    }
    for (int gi = 0; gi < l.n_groups; ++gi) {
        const EncGroup& g = l.g[gi];
        for (int h = 0; h < g.heads; ++h) {
            for (int i = 0; i < g.convs; ++i) {
                const int s = l.in_size[gi][i], cin = i == 0 ? kEncLat : g.cout;
                if (s > 2) ig_pack(packed + l.w_off[gi][i] + (int64_t)h * g.cout * ig_kpad(cin * 9), next(), cin, g.cout, 3, 1.0f, st);
                else enc_pack_live(packed + l.w_off[gi][i] + (int64_t)h * g.cout * cin * s * s, next(), g.cout, cin, s * s, st);
                ig_copy(packed + l.b_off[gi][i] + (int64_t)h * g.cout, next(), g.cout, 1.0f, 0, st);
            }
            ig_copy(packed + l.lin_w[gi] + (int64_t)h * g.cout * g.cout, next(), (int64_t)g.cout * g.cout, (float)(1.0 / sqrt((double)g.cout)), 0, st);
            ig_copy(packed + l.lin_b[gi] + (int64_t)h * g.cout, next(), g.cout, 1.0f, 0, st);
        }
    }
    return check_launch("enc_pack_weights");
}

extern "C" int64_t e3dge_enc_ws_bytes(int n, int size, int geo_dim, int tex_dim, int enable_decoder) {
    const EncCfg c{size, geo_dim, tex_dim, enable_decoder};
    EncWs d;
    if (!enc_cfg_ok(c) || !enc_ws(n, c, enc_plan(c), &d)) {
        fail(E3DGE_ERR_INVALID_ARG, "enc_ws_bytes: n=%d (1..256) size=%d geo_dim=%d tex_dim=%d enable_decoder=%d", n, size, geo_dim, tex_dim, enable_decoder);
        return -1;
    }
    return d.total_bytes;
}

extern "C" int e3dge_enc_forward(const E3dgeEncArgs* args, e3dge_stream_t stream) {
    E3DGE_REQUIRE(args, "enc_forward: null argument struct");
    const E3dgeEncArgs& a = *args;
    E3DGE_REQUIRE(a.n >= 1 && a.n <= 256, "enc_forward: n=%d (1..256)", a.n);
    const EncCfg c{a.size, a.geo_dim, a.tex_dim, a.enable_decoder};
    E3DGE_REQUIRE(enc_cfg_ok(c), "enc_forward: size=%d geo_dim=%d tex_dim=%d enable_decoder=%d (size a multiple of 16 in 32..256, dims 32, 64 or 128)", a.size,
                  a.geo_dim, a.tex_dim, a.enable_decoder);
    E3DGE_REQUIRE(a.packed && a.images && a.thumb_out && a.p32 && a.p64 && a.ws, "enc_forward: null pointer");
    E3DGE_REQUIRE(!c.dec || a.stylegan_out, "enc_forward: null pointer (stylegan_out with the decoder head on)");
    const EncPlan l = enc_plan(c);
    EncWs d;
    E3DGE_REQUIRE(enc_ws(a.n, c, l, &d), "enc_forward: n=%d size=%d", a.n, a.size);
    E3DGE_REQUIRE(a.ws_bytes >= d.total_bytes, "enc_forward: workspace of %lld bytes, %lld needed", (long long)a.ws_bytes, (long long)d.total_bytes);
    hipStream_t st = as_stream(stream);
    float* ws = static_cast<float*>(a.ws);
    const float* P = a.packed;
    const int n = a.n, S = a.size;
    float* const keep[4] = {ws + d.keep[0], ws + d.keep[1], ws + d.keep[2], ws + d.keep[3]};
    float* const act[2] = {ws + d.act[0], ws + d.act[1]};
    int rc;
    if ((rc = enc_body(keep, a.images, P, l, ws, d, n, S, st))) return rc;
    float* p128 = ws + d.p128;
    if ((rc = enc_lateral(a.p32, keep[3], keep[2], P + l.lat_w[0], P + l.lat_b[0], n, 256, kEncLat, S / 16, S / 16, S / 8, S / 8, st))) return rc;
    if ((rc = enc_lateral(a.p64, a.p32, keep[1], P + l.lat_w[1], P + l.lat_b[1], n, 128, kEncLat, S / 8, S / 8, S / 4, S / 4, st))) return rc;
    if (c.dec && (rc = enc_lateral(p128, a.p64, keep[0], P + l.lat_w[2], P + l.lat_b[2], n, 64, kEncLat, S / 4, S / 4, S / 2, S / 2, st))) return rc;
    for (int gi = 0; gi < l.n_groups; ++gi) {
        const EncGroup& g = l.g[gi];
        const float* map = g.level == 0 ? a.p32 : g.level == 1 ? a.p64 : p128;
        if (g.head0 == 9) rc = enc_heads(a.stylegan_out, 0, kEncLat, map, P, l, gi, act, n, st);
        else rc = enc_heads(a.thumb_out + g.head0 * kEncStyle, kEncStyle, (int64_t)kEncHeads * kEncStyle, map, P, l, gi, act, n, st);
        if (rc) return rc;
    }
    return E3DGE_OK;
}

static bool enc_channels_ok(int c) { return c >= kIgBM && c % kIgBM == 0 && c <= 4096; }

extern "C" int e3dge_enc_lateral(float* out, const float* coarse, const float* in, const float* w, const float* bias, float* wfrag, int n, int cin,
                                 int cout, int coarse_height, int coarse_width, int height, int width, e3dge_stream_t stream) {
    E3DGE_REQUIRE(out && coarse && in && w && bias && wfrag, "enc_lateral: null pointer");
    E3DGE_REQUIRE(n >= 1 && n <= 256 && cin >= 1 && cin <= 4096, "enc_lateral: n=%d (1..256) cin=%d (1..4096)", n, cin);
    E3DGE_REQUIRE(enc_channels_ok(cout), "enc_lateral: cout=%d (a multiple of 64 up to 4096)", cout);
    E3DGE_REQUIRE(height >= 1 && width >= 1 && height <= 1024 && width <= 1024 && coarse_height >= 1 && coarse_width >= 1 && coarse_height <= height &&
                      coarse_width <= width,
                  "enc_lateral: coarse %d x %d, fine %d x %d (1..1024, coarse no larger than fine)", coarse_height, coarse_width, height, width);
    hipStream_t st = as_stream(stream);
    ig_pack(wfrag, w, cin, cout, 1, 1.0f, st);
    int rc;
    if ((rc = check_launch("enc_lateral(pack)"))) return rc;
    return enc_lateral(out, coarse, in, wfrag, bias, n, cin, cout, coarse_height, coarse_width, height, width, st);
}

extern "C" int e3dge_enc_head_conv(float* out, const float* in, const float* w, const float* bias, float* wfrag, int n, int heads, int shared, int cin,
                                   int cout, int height, int width, e3dge_stream_t stream) {
    E3DGE_REQUIRE(out && in && w && bias && wfrag, "enc_head_conv: null pointer");
    E3DGE_REQUIRE(n >= 1 && n <= 256 && heads >= 1 && heads <= 16 && cin >= 1 && cin <= 4096, "enc_head_conv: n=%d (1..256) heads=%d (1..16) cin=%d (1..4096)", n,
                  heads, cin);
    E3DGE_REQUIRE(shared == 0 || shared == 1, "enc_head_conv: shared=%d (0 or 1)", shared);
    E3DGE_REQUIRE(enc_channels_ok(cout), "enc_head_conv: cout=%d (a multiple of 64 up to 4096)", cout);
    E3DGE_REQUIRE(height >= 1 && width >= 1 && height <= 1024 && width <= 1024, "enc_head_conv: height=%d width=%d (1..1024)", height, width);
    hipStream_t st = as_stream(stream);
    const int64_t per = (int64_t)cout * ig_kpad(cin * 9);
    for (int g = 0; g < heads; ++g) ig_pack(wfrag + g * per, w + (int64_t)g * cout * cin * 9, cin, cout, 3, 1.0f, st);
    int rc;
    if ((rc = check_launch("enc_head_conv(pack)"))) return rc;
    return enc_head_conv(out, in, wfrag, bias, n, heads, shared, cin, cout, height, width, st);
}

extern "C" int e3dge_enc_head_tail(float* out, const float* in, const float* conv_w, const float* conv_b, const float* lin_w, const float* lin_b,
                                   float* scratch, int64_t scratch_floats, int n, int heads, int channels, int start, int n_convs,
                                   e3dge_stream_t stream) {
    E3DGE_REQUIRE(out && in && lin_w && lin_b && scratch, "enc_head_tail: null pointer");
    E3DGE_REQUIRE(n >= 1 && n <= 256 && heads >= 1 && heads <= 16, "enc_head_tail: n=%d (1..256) heads=%d (1..16)", n, heads);
    E3DGE_REQUIRE(enc_channels_ok(channels), "enc_head_tail: channels=%d (a multiple of 64 up to 4096)", channels);
    E3DGE_REQUIRE(start == 1 || start == 2, "enc_head_tail: start=%d (a 1x1 or 2x2 map)", start);
    E3DGE_REQUIRE(n_convs >= (start == 2 ? 1 : 0) && n_convs <= kEncMaxConvs, "enc_head_tail: n_convs=%d (a 2x2 start needs one; at most %d)", n_convs,
                  kEncMaxConvs);
    E3DGE_REQUIRE(n_convs == 0 || (conv_w && conv_b), "enc_head_tail: null pointer (conv_w, conv_b)");
    const int64_t C = channels, G = heads;
    int64_t need = 2 * G * n * C + G * C * C + G * C;                 // two activation buffers, the linear layer
    for (int i = 0; i < n_convs; ++i) need += G * C * C * (i == 0 ? start * start : 1) + G * C;
    E3DGE_REQUIRE(scratch_floats >= need, "enc_head_tail: scratch of %lld floats, %lld needed", (long long)scratch_floats, (long long)need);
    hipStream_t st = as_stream(stream);
    float* act[2] = {scratch, scratch + G * n * C};
    float* at = scratch + 2 * G * n * C;
    float* lw = at; at += G * C * C;
    float* lb = at; at += G * C;
    ig_copy(lw, lin_w, G * C * C, (float)(1.0 / sqrt((double)channels)), 0, st);
    ig_copy(lb, lin_b, G * C, 1.0f, 0, st);
    int rc, pp = 0;
    const float* x = in;
    for (int i = 0; i < n_convs; ++i) {
        const int T = i == 0 ? start * start : 1;
        float* w = at; at += G * C * C * T;
        float* b = at; at += G * C;
        for (int g = 0; g < heads; ++g) {
            enc_pack_live(w + g * C * C * T, conv_w + ((int64_t)g * n_convs + i) * C * C * 9, channels, channels, T, st);
            ig_copy(b + g * C, conv_b + ((int64_t)g * n_convs + i) * C, C, 1.0f, 0, st);
        }
        if ((rc = check_launch("enc_head_tail(pack)"))) return rc;
        if ((rc = enc_tail(act[pp], x, w, b, n, heads, channels * T, channels, (int64_t)n * C, C, true, st))) return rc;
        x = act[pp];
        pp ^= 1;
    }
    return enc_tail(out, x, lw, lb, n, heads, channels, channels, C, G * C, false, st);
}
