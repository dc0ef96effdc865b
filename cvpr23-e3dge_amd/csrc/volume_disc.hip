// The camera-pose predictor, forward, eval form: image (B, 3, S, S), S in {16, 32, 64, 128} -> logits (B, 1), viewpoints (B, 2).
//
// Reference: VolumeRenderDiscriminator (project/models/stylesdf_model.py:1369-1419) on VolumeRenderDiscConv2d, AddCoords, CoordConv2d,
// CoordConvLayer and VolumeRenderResBlock (:1193-1366); called under no_grad as self.volume_discriminator (project/trainers/trainer.py:944).
//
//   channels(res) = 400 at res <= 16, 256 at 32, 128 at 64, 64 at 128
//   stem    = lrelu(conv1x1(3 -> channels(S)) + b)                                                          S^2
//   block   = (avgpool2(lrelu(coordconv3x3(lrelu(coordconv3x3(x) + b1)) + b2)) + skip(x)) / sqrt(2)         res -> res / 2, log2(S) - 1 blocks
//             skip(x) = conv1x1(avgpool2(x)) + b where the block changes the channel count, avgpool2(x) where it does not
//             coordconv3x3 = conv3x3 pad 1 of cat(x, yy, xx), yy / xx = 2 i / (d - 1) - 1 along the rows / the columns
//   final   = conv2x2(channels(2) -> 3) + b on the 2 x 2 map; column 0 is the logit, columns 1 and 2 are the two angles
//
// Two kernels (launches at S = 16 / 32 / 64 / 128: 8 / 11 / 14 / 17, whatever the batch; all but the last are the first kernel's):
//   vdisc_conv_kernel  the fp32 implicit GEMM of conv_igemm.h (ig_k_loop: v_mfma_f32_16x16x4_f32, the packed A-fragment image of ig_pack, K
//                      staged through LDS in tiles of kIgKC with the next tile's loads in flight, two accumulator chains per output element,
//                      each in ascending k), a workgroup of 64 channels x 16 NT pixels of ONE image, the IDLE form (400 channels: the
//                      seventh channel block has one live wave).
//                      Gather (KS, POOLIN): 3x3 pad 1 over C + 2 channels, channel C = yy and C + 1 = xx computed in registers from the
//                      tap's row and column exactly as torch does, fl(fl(fl(i) / fl(d - 1)) * 2) - 1, and 0 where the tap falls into the
//                      zero padding -- the concatenated tensor never exists; 1x1 (the stem); 1x1 on the average of the input's 2x2 block
//                      (the skip: pooling first is the reference's own order).
//                      Epilogue: kVdEpiBias (+ bias), kVdEpiAct (+ bias, leaky_relu 0.2, scale 1), kVdEpiPool (kVdEpiAct, then the block's
//                      tail).  In the pooled form the pixels of the GEMM are ordered quad-major: pixel 4 q + 2 dy + dx is element (dy, dx)
//                      of the 2x2 block of pooled pixel q, so a block's four pre-pool values sit in four adjacent lanes of the C/D fragment
//                      and AvgPool2d(2) is a DPP quad_perm reduction ((v0 + v1) + v2) + v3 (ATen's order) times 0.25.  Lane i of a quad
//                      then finishes row i of the fragment's four: + skip (read from the skip launch's output, or the average of the
//                      block input's 2x2 pixels), * fl(1 / fl(sqrt 2)) (torch's GPU form of `/ math.sqrt(2)`), and stores the pooled
//                      tensor only.
//   vdisc_final_kernel the final layer.  A 2x2 convolution without padding on the 2 x 2 map is three dot products of length 4 C over the
//                      image's flattened map, far too little for a matrix tile; and the logit is a sum of 1600 terms that cancel to a few
//                      percent of their magnitude, so it is summed in float64 (products exact, a fixed tree) and rounded once.  One
//                      workgroup per image; it writes the logit and the two angles to their own tensors.
// No atomics, a fixed summation order, tiles that never straddle images and a tile width from the layer alone (ig_tile_width, two images
// counted): results are bit-reproducible and an image's values do not depend on the batch.  Measured errors and times: DESIGN.md 4.18.
#include <algorithm>

#include "conv_igemm.h"
#include "gfx950_prims.h"

namespace e3dge {

constexpr int kVdMaxBlocks = E3DGE_VDISC_MAX_BLOCKS, kVdTaps = E3DGE_VDISC_TAPS;
constexpr int kVdStem = E3DGE_VDISC_FORM_STEM, kVdConv = E3DGE_VDISC_FORM_CONV, kVdConvPool = E3DGE_VDISC_FORM_CONV_POOL,
              kVdSkip = E3DGE_VDISC_FORM_SKIP, kVdFinal = E3DGE_VDISC_FORM_FINAL;
constexpr int kVdSkipRead = E3DGE_VDISC_SKIP_READ, kVdSkipPool = E3DGE_VDISC_SKIP_POOL;
enum { kVdEpiBias = 0, kVdEpiAct = 1, kVdEpiPool = 2 };
constexpr float kVdSlope = 0.2f;
constexpr float kVdInvSqrt2 = 1.0f / 1.41421356237309504880f;    // fl(1 / fl(sqrt 2)): `/ math.sqrt(2)` as torch divides by a scalar on the GPU

struct VdConvArgs {
    float* out; const float* in; const float* wfrag; const float* bias; const float* skip;
    int C, IH, IW, Cout, OH, OW, K, KS4, tiles, skip_mode;
};

// AddCoords (stylesdf_model.py:1249-1262): arange / (d - 1) * 2 - 1, every step rounded to fp32
__device__ __forceinline__ float vd_coord(int i, int d) { return __fsub_rn(__fmul_rn(__fdiv_rn((float)i, (float)(d - 1)), 2.0f), 1.0f); }

// average of the 2x2 block at p (row pitch W) as AvgPool2d(2) sums it
__device__ __forceinline__ float vd_avg4(const float* __restrict__ p, int W) {
    return __fmul_rn(__fadd_rn(__fadd_rn(__fadd_rn(p[0], p[1]), p[W]), p[W + 1]), 0.25f);
}

// GEMM pixel -> (row, column) of the OH x OW plane: raster, or quad-major over the 2x2 blocks (OW even)
template <bool QUAD>
__device__ __forceinline__ void vd_pixel(int pix, int OW, int& oy, int& ox) {
    if (QUAD) {
        const int q = pix >> 2, PW = OW >> 1, py = q / PW, px = q - py * PW;
        oy = 2 * py + ((pix >> 1) & 1);
        ox = 2 * px + (pix & 1);
    } else {
        oy = pix / OW;
        ox = pix - oy * OW;
    }
}

template <int NT, int KS, bool POOLIN, int EPI>
__global__ void __launch_bounds__(256) vdisc_conv_kernel(VdConvArgs a) {
    constexpr int BN = IgTile<NT>::BN, ROWS = IgTile<NT>::ROWS, PER = IgTile<NT>::PER;
    constexpr bool COORD = KS == 3, QUAD = EPI == kVdEpiPool;
    constexpr int PAD = KS == 3 ? 1 : 0;
    static_assert(KS == 3 || KS == 1, "3x3 with the coordinate channels, or 1x1");
    static_assert(!POOLIN || KS == 1, "the pooled gather is the skip's 1x1");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mt = blockIdx.y * (kIgBM / 16) + wave;
    const bool live = mt * 16 < a.Cout;
    const int OHW = a.OH * a.OW, IH = a.IH, IW = a.IW, K = a.K, C = a.C;
    const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
    const int sn = tid % BN, srow = tid / BN;
    const int spix = tile * BN + sn;
    const bool n_ok = spix < OHW;
    int soy, sox;
    vd_pixel<QUAD>(spix, a.OW, soy, sox);
    const int iy0 = soy - PAD, ix0 = sox - PAD;
    const float* __restrict__ src = a.in + (int64_t)img * C * IH * IW;
    auto fetch = [&](int k0, float (&v)[PER]) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = k0 + srow + i * ROWS;
            const auto [ci, r, s] = ig_decode<KS>(k);
            float x = 0.0f;
            if (POOLIN) {                                             // (C, 2 OH, 2 OW): the block is inside the plane
                if (n_ok && k < K) x = vd_avg4(src + ((int64_t)ci * IH + 2 * soy) * IW + 2 * sox, IW);
            } else {
                const int iy = iy0 + r, ix = ix0 + s;
                if (n_ok && k < K && iy >= 0 && iy < IH && ix >= 0 && ix < IW) {    // a tap in the zero padding stays 0, the coordinates too
                    if (COORD && ci >= C) x = ci == C ? vd_coord(iy, IH) : vd_coord(ix, IW);
                    else x = src[((int64_t)ci * IH + iy) * IW + ix];
                }
            }
            v[i] = x;
        }
    };
    f32x4 acc[NT][2];
    ig_k_loop<NT, 2, true>(acc, a.wfrag + (int64_t)(live ? mt : 0) * a.KS4 * 64 + lane, a.KS4 / (kIgKC / 4), live, fetch, [](int, bool) {});
    if (!live) return;                                                // (wave-uniform: the DPP moves below see whole waves)
    // C/D fragment: lane l, register r holds D[4 (l >> 4) + r][l & 15]
    const int row0 = mt * 16 + 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int pix = tile * BN + t * 16 + (lane & 15);
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            v[r] = __fadd_rn(__fadd_rn(acc[t][0][r], acc[t][1][r]), row0 + r < a.Cout ? a.bias[row0 + r] : 0.0f);
            if (EPI != kVdEpiBias) v[r] = v[r] > 0.0f ? v[r] : __fmul_rn(v[r], kVdSlope);
        }
        if (EPI == kVdEpiPool) {
            // every lane takes part in the reduction (a tile holds whole quads, live or past the plane); lane i of a quad keeps row i
            float mine = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __fmul_rn(quad_sum(v[r]), 0.25f);
                mine = (lane & 3) == r ? p : mine;
            }
            const int row = row0 + (lane & 3);
            if (pix >= OHW || row >= a.Cout) continue;
            const int q = pix >> 2, PW = a.OW >> 1, PHW = OHW >> 2;
            const int64_t plane = (int64_t)img * a.Cout + row;
            float sk;
            if (a.skip_mode == kVdSkipRead) {
                sk = a.skip[plane * PHW + q];
            } else {                                                  // the block's input (n, Cout, OH, OW), pooled here
                const int py = q / PW, px = q - py * PW;
                sk = vd_avg4(a.skip + (plane * a.OH + 2 * py) * a.OW + 2 * px, a.OW);
            }
            a.out[plane * PHW + q] = __fmul_rn(__fadd_rn(mine, sk), kVdInvSqrt2);
        } else {
            if (pix >= OHW) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + r;
                if (row >= a.Cout) continue;                          // the zero-padded rows of a partial channel tile
                a.out[((int64_t)img * a.Cout + row) * OHW + pix] = v[r];
            }
        }
    }
}

// out[img][m] = bias[m] + sum_k w[m][k] x[img][k], k over the flattened (C, 2, 2) map: float64 products and sums in a fixed order, one rounding.
// With out2, output 0 goes to out (n, 1) and outputs 1 .. M - 1 to out2 (n, M - 1).
constexpr int kVdFinalThreads = 256;
__global__ void __launch_bounds__(kVdFinalThreads) vdisc_final_kernel(float* __restrict__ out, float* __restrict__ out2, const float* __restrict__ in,
                                                                      const float* __restrict__ w, const float* __restrict__ bias, int K, int M) {
    __shared__ double part[kVdFinalThreads];
    const int tid = threadIdx.x, img = blockIdx.x;
    const float* __restrict__ x = in + (int64_t)img * K;
    for (int m = 0; m < M; ++m) {
        double acc = 0.0;
        for (int k = tid; k < K; k += kVdFinalThreads) acc = fma((double)w[(int64_t)m * K + k], (double)x[k], acc);
        part[tid] = acc;
        __syncthreads();
        for (int off = kVdFinalThreads / 2; off > 0; off >>= 1) {
            if (tid < off) part[tid] += part[tid + off];
            __syncthreads();
        }
        if (tid == 0) {
            const float v = (float)(part[0] + (double)bias[m]);
            if (out2 && m > 0) out2[(int64_t)img * (M - 1) + m - 1] = v;
            else out[out2 ? (int64_t)img : (int64_t)img * M + m] = v;
        }
        __syncthreads();                                              // part[] is free for the next output
    }
}

// ---- host side: one launch ------------------------------------------------------------------------------------------------------------
struct VdConv {
    float* out; float* out2; const float* in; const float* wfrag; const float* bias; const float* skip;
    int n, cin, cout, h, w, form, skip_mode;                          // h, w: the input plane; out2: kVdFinal only
};

static int vd_ksize(int form) { return form == kVdConv || form == kVdConvPool ? 3 : form == kVdFinal ? 2 : 1; }
static int vd_k(int form, int cin) { return form == kVdConv || form == kVdConvPool ? 9 * (cin + 2) : form == kVdFinal ? 4 * cin : cin; }
// floats of a layer's weights in the packed image: the A-fragment image, or for the final layer the weight as it is
static int64_t vd_image_floats(int form, int cin, int cout) {
    return form == kVdFinal ? (int64_t)cout * vd_k(form, cin) : (int64_t)ig_mpad(cout) * ig_kpad(vd_k(form, cin));
}
// the GEMM's plane: the pre-pool plane of kVdConvPool, the pooled plane of kVdSkip
static void vd_plane(int form, int h, int w, int& oh, int& ow) {
    oh = form == kVdSkip ? h / 2 : form == kVdFinal ? h - 1 : h;
    ow = form == kVdSkip ? w / 2 : form == kVdFinal ? w - 1 : w;
}

static int vd_conv(const VdConv& c, hipStream_t st) {
    if (c.form == kVdFinal) {                                         // h == w == 2
        vdisc_final_kernel<<<dim3((unsigned)c.n), dim3(kVdFinalThreads), 0, st>>>(c.out, c.out2, c.in, c.wfrag, c.bias, vd_k(c.form, c.cin), c.cout);
        return check_launch("vdisc(final)");
    }
    VdConvArgs a;
    a.out = c.out; a.in = c.in; a.wfrag = c.wfrag; a.bias = c.bias; a.skip = c.skip;
    a.C = c.cin; a.IH = c.h; a.IW = c.w; a.Cout = c.cout; a.skip_mode = c.skip_mode;
    vd_plane(c.form, c.h, c.w, a.OH, a.OW);
    a.K = vd_k(c.form, c.cin); a.KS4 = ig_kpad(a.K) / 4;
    const int OHW = a.OH * a.OW, gy = (c.cout + kIgBM - 1) / kIgBM, nt = ig_tile_width(OHW, 2, gy), bn = 16 * nt;   // two images counted, whatever n
    a.tiles = (OHW + bn - 1) / bn;
    const dim3 grid((unsigned)((int64_t)c.n * a.tiles), (unsigned)gy);
    ig_dispatch_nt(nt, [&](auto nt_c) {
        constexpr int NT = decltype(nt_c)::value;
        switch (c.form) {
            case kVdStem: vdisc_conv_kernel<NT, 1, false, kVdEpiAct><<<grid, dim3(256), 0, st>>>(a); break;
            case kVdConv: vdisc_conv_kernel<NT, 3, false, kVdEpiAct><<<grid, dim3(256), 0, st>>>(a); break;
            case kVdConvPool: vdisc_conv_kernel<NT, 3, false, kVdEpiPool><<<grid, dim3(256), 0, st>>>(a); break;
            default: vdisc_conv_kernel<NT, 1, true, kVdEpiBias><<<grid, dim3(256), 0, st>>>(a); break;
        }
    });
    return check_launch("vdisc(conv)");
}

// ---- the network: one table for the packed image, the workspace and the walk ------------------------------------------------------------
struct VdLayer { int64_t w, b; };                                     // offsets into the packed image
struct VdNet {
    int size, c0, blocks, n_src;
    int cin[kVdMaxBlocks], cout[kVdMaxBlocks], res[kVdMaxBlocks];     // res: the block's input plane
    VdLayer stem, conv1[kVdMaxBlocks], conv2[kVdMaxBlocks], skip[kVdMaxBlocks], final_;
    int64_t packed_total, max_x, max_t, max_s;                        // floats per image: a block input / output, a conv1 output, a skip output
};

static int vd_channels(int res) { return res <= 16 ? 400 : res == 32 ? 256 : res == 64 ? 128 : 64; }      // stylesdf_model.py:1377-1385

static bool vd_net(int size, VdNet* net) {
    if (size != 16 && size != 32 && size != 64 && size != 128) return false;
    VdNet& d = *net;
    d.size = size; d.c0 = vd_channels(size); d.blocks = 0; d.n_src = 2;
    int64_t at = 0;
    auto layer = [&](int form, int cin, int cout) {
        VdLayer l{at, at + vd_image_floats(form, cin, cout)};
        at = l.b + cout;
        return l;
    };
    d.stem = layer(kVdStem, 3, d.c0);
    d.max_x = (int64_t)d.c0 * size * size; d.max_t = 0; d.max_s = 0;
    int cin = d.c0;
    for (int res = size; res > 2; res /= 2) {
        const int b = d.blocks++, cout = vd_channels(res / 2);
        d.cin[b] = cin; d.cout[b] = cout; d.res[b] = res;
        d.conv1[b] = layer(kVdConv, cin, cout);
        d.conv2[b] = layer(kVdConvPool, cout, cout);
        d.n_src += 4;
        d.max_t = std::max(d.max_t, (int64_t)cout * res * res);
        d.max_x = std::max(d.max_x, (int64_t)cout * (res / 2) * (res / 2));
        if (cin != cout) {
            d.skip[b] = layer(kVdSkip, cin, cout);
            d.n_src += 2;
            d.max_s = std::max(d.max_s, (int64_t)cout * (res / 2) * (res / 2));
        }
        cin = cout;
    }
    d.final_ = layer(kVdFinal, cin, 3);
    d.n_src += 2;
    d.packed_total = at;
    return true;
}

static int64_t vd_ws_floats(const VdNet& d, int64_t n) { return n * (2 * d.max_x + d.max_t + d.max_s); }

}  // namespace e3dge

using namespace e3dge;

extern "C" int64_t e3dge_vdisc_packed_floats(int size) {
    VdNet d;
    if (!vd_net(size, &d)) {
        fail(E3DGE_ERR_INVALID_ARG, "vdisc_packed_floats: size=%d (16, 32, 64 or 128)", size);
        return -1;
    }
    return d.packed_total;
}

extern "C" int64_t e3dge_vdisc_ws_bytes(int n, int size) {
    VdNet d;
    if (!vd_net(size, &d) || n < 1 || n > 256) {
        fail(E3DGE_ERR_INVALID_ARG, "vdisc_ws_bytes: n=%d (1..256) size=%d (16, 32, 64 or 128)", n, size);
        return -1;
    }
    return 4 * vd_ws_floats(d, n);
}

extern "C" int e3dge_vdisc_pack_weights(float* image, const float* const* ptrs, int n, int size, e3dge_stream_t stream) {
    E3DGE_REQUIRE(image && ptrs, "vdisc_pack_weights: null pointer");
    VdNet d;
    E3DGE_REQUIRE(vd_net(size, &d), "vdisc_pack_weights: size=%d (16, 32, 64 or 128)", size);
    E3DGE_REQUIRE(n == d.n_src, "vdisc_pack_weights: n=%d, %d source tensors expected at size %d", n, d.n_src, size);
    for (int i = 0; i < n; ++i) E3DGE_REQUIRE(ptrs[i], "vdisc_pack_weights: null pointer (source %d)", i);
    hipStream_t st = as_stream(stream);
    int at = 0;
    auto layer = [&](const VdLayer& l, int form, int cin, int cout) {  // a weight, then its bias
        const int ks = vd_ksize(form);
        if (form == kVdFinal) ig_copy(image + l.w, ptrs[at], (int64_t)cout * vd_k(form, cin), 1.0f, 0, st);
        else ig_pack(image + l.w, ptrs[at], vd_k(form, cin) / (ks * ks), cout, ks, 1.0f, st);
        ig_copy(image + l.b, ptrs[at + 1], cout, 1.0f, 0, st);
        at += 2;
    };
    layer(d.stem, kVdStem, 3, d.c0);
    for (int b = 0; b < d.blocks; ++b) {
        layer(d.conv1[b], kVdConv, d.cin[b], d.cout[b]);
        layer(d.conv2[b], kVdConvPool, d.cout[b], d.cout[b]);
        if (d.cin[b] != d.cout[b]) layer(d.skip[b], kVdSkip, d.cin[b], d.cout[b]);
    }
    layer(d.final_, kVdFinal, d.cout[d.blocks - 1], 3);
    return check_launch("vdisc_pack_weights");
}

extern "C" int e3dge_vdisc_forward(const E3dgeVdiscArgs* args, e3dge_stream_t stream) {
    E3DGE_REQUIRE(args, "vdisc_forward: null argument struct");
    const E3dgeVdiscArgs& a = *args;
    VdNet d;
    E3DGE_REQUIRE(vd_net(a.size, &d), "vdisc_forward: size=%d (16, 32, 64 or 128)", a.size);
    E3DGE_REQUIRE(a.n >= 1 && a.n <= 256, "vdisc_forward: n=%d (1..256)", a.n);
    E3DGE_REQUIRE(a.packed && a.images && a.logits && a.viewpoints && a.ws, "vdisc_forward: null pointer");
    E3DGE_REQUIRE(a.ws_bytes >= 4 * vd_ws_floats(d, a.n), "vdisc_forward: workspace of %lld bytes, %lld needed", (long long)a.ws_bytes,
                  (long long)(4 * vd_ws_floats(d, a.n)));
    hipStream_t st = as_stream(stream);
    const float* P = a.packed;
    float* W = static_cast<float*>(a.ws);
    float* X[2] = {W, W + a.n * d.max_x};
    float* T = W + 2 * a.n * d.max_x;
    float* S = T + a.n * d.max_t;
    int rc;
    float* x = a.taps[0] ? a.taps[0] : X[0];                          // a wanted tap is written in place
    if ((rc = vd_conv({x, nullptr, a.images, P + d.stem.w, P + d.stem.b, nullptr, a.n, 3, d.c0, d.size, d.size, kVdStem, 0}, st))) return rc;
    for (int b = 0; b < d.blocks; ++b) {
        const int cin = d.cin[b], cout = d.cout[b], res = d.res[b];
        const bool conv_skip = cin != cout;
        if (conv_skip && (rc = vd_conv({S, nullptr, x, P + d.skip[b].w, P + d.skip[b].b, nullptr, a.n, cin, cout, res, res, kVdSkip, 0}, st))) return rc;
        if ((rc = vd_conv({T, nullptr, x, P + d.conv1[b].w, P + d.conv1[b].b, nullptr, a.n, cin, cout, res, res, kVdConv, 0}, st))) return rc;
        float* y = a.taps[b + 1] ? a.taps[b + 1] : X[(b + 1) & 1];
        if ((rc = vd_conv({y, nullptr, T, P + d.conv2[b].w, P + d.conv2[b].b, conv_skip ? S : x, a.n, cout, cout, res, res, kVdConvPool,
                           conv_skip ? kVdSkipRead : kVdSkipPool}, st)))
            return rc;
        x = y;
    }
    return vd_conv({a.logits, a.viewpoints, x, P + d.final_.w, P + d.final_.b, nullptr, a.n, d.cout[d.blocks - 1], 3, 2, 2, kVdFinal, 0}, st);
}

// One launch of vdisc_conv_kernel at run-time shapes (after packing w): what the tests call
extern "C" int e3dge_vdisc_conv(float* out, const float* in, const float* w, const float* bias, const float* skip, float* wfrag, int64_t wfrag_floats,
                                int n, int cin, int cout, int height, int width, int form, int skip_mode, e3dge_stream_t stream) {
    E3DGE_REQUIRE(out && in && w && bias && wfrag, "vdisc_conv: null pointer");
    E3DGE_REQUIRE(form >= kVdStem && form <= kVdFinal, "vdisc_conv: form=%d (0 stem, 1 conv, 2 conv + pool, 3 skip, 4 final)", form);
    E3DGE_REQUIRE(n >= 1 && n <= 256 && cin >= 1 && cin <= 4096 && cout >= 1 && cout <= 4096, "vdisc_conv: n=%d (1..256) cin=%d cout=%d (1..4096)", n, cin, cout);
    E3DGE_REQUIRE(height >= 1 && width >= 1 && height <= 1024 && width <= 1024, "vdisc_conv: height=%d width=%d (1..1024)", height, width);
    E3DGE_REQUIRE(form == kVdStem || (height >= 2 && width >= 2), "vdisc_conv: height=%d width=%d (at least 2: the coordinates divide by d - 1)", height, width);
    E3DGE_REQUIRE(form != kVdFinal || (height == 2 && width == 2 && cout <= 64), "vdisc_conv: height=%d width=%d cout=%d (the final layer takes the 2 x 2 map, cout 1..64)",
                  height, width, cout);
    E3DGE_REQUIRE((form != kVdConvPool && form != kVdSkip) || (height % 2 == 0 && width % 2 == 0), "vdisc_conv: height=%d width=%d (the pooled forms take even planes)",
                  height, width);
    if (form == kVdConvPool)
        E3DGE_REQUIRE(skip && (skip_mode == kVdSkipRead || skip_mode == kVdSkipPool), "vdisc_conv: skip_mode=%d (1 read, 2 pooled read) needs its tensor", skip_mode);
    E3DGE_REQUIRE((int64_t)n * std::max(cin, cout) * height * width <= ((int64_t)1 << 31), "vdisc_conv: at most 2^31 elements per tensor");
    E3DGE_REQUIRE(wfrag_floats >= vd_image_floats(form, cin, cout), "vdisc_conv: wfrag of %lld floats, %lld needed", (long long)wfrag_floats,
                  (long long)vd_image_floats(form, cin, cout));
    hipStream_t st = as_stream(stream);
    const int ks = vd_ksize(form);
    if (form == kVdFinal) ig_copy(wfrag, w, (int64_t)cout * vd_k(form, cin), 1.0f, 0, st);
    else ig_pack(wfrag, w, vd_k(form, cin) / (ks * ks), cout, ks, 1.0f, st);
    int rc;
    if ((rc = check_launch("vdisc_conv(pack)"))) return rc;
    return vd_conv({out, nullptr, in, wfrag, bias, skip, n, cin, cout, height, width, form, skip_mode}, st);
}
