// ArcFace identity term, backward: the gradient of the loss with respect to the y_hat images (included at the end of idnet.hip).  The
// network is frozen, as the reference freezes it (id_loss.py:21), so only data gradients exist.
//
// The saving forward (e3dge_idnet_embed_save: the forward's own launches, bit-identical outputs) keeps for the images that get a gradient
// every PReLU's branch as a byte, each unit's `res` (BN2 output before the gate), the gates, the SE hidden activations and the head's
// v, f = v / |v| and |v| (IdSaved).  In reverse order:
//
//   head_norm_bwd   g_v = (g_f - (g_f . f) f) / |v|, then the BN1d scale.
//   head_bwd        a52[k / 49] * sum_o W[o][k] g[o] for up to 8 images per pass over the 51 MB matrix: a wave owns 64 k and a quarter
//                   of o in ascending order, the four quarters are added in order.
//   per unit        plane_dot     d gate[b, c] = sum_hw g_out res, one wave per plane: lane-strided in ascending order, then a butterfly.
//                   se_bwd        one workgroup per image: gate (1 - gate), fc2^T, the hidden ReLU's mask, fc1^T, / HW; written as the
//                                 pair (gate a2, d mean a2) per (image, channel), the next launch's input affine.
//                   dgrad 3x3     (g_out gate + d mean) a2 while staging (in-image elements only), the transposed strided 3x3, times
//                                 the saved PReLU derivative.
//                   dgrad 3x3     the transposed stride-1 3x3, times BN1's a[ci], plus the shortcut's gradient read in the epilogue:
//                                 g_out itself (identity units; for unit 0 at the even positions only, the adjoint of the strided pick)
//                                 or, for units 3, 7, 21, a transposed 1x1 stride-2 dgrad of a_sc g_out launched before.
//   input layer     PReLU derivative and BN scale in place, then the 64 -> 3 dgrad (wave 0 of a workgroup holds the 3 rows).
//   prep_bwd        the adjoint of the crop and both adaptive averages as a gather per image pixel: every element is written.
//
// dgrad_kernel is the implicit GEMM of conv_igemm.h on the transposed weight image (W^T with flipped taps, M = C_in, K = (co, r, s)):
// idnet_conv_kernel's tile and two accumulators, tile width from the layer alone; waves past M idle (the 64 -> 3 gradient has one live
// wave).  Gather: g with an optional per-image affine or per-channel factor on in-image elements; stride 2 is a predicate: the tap
// (r, s) of output pixel (y, x) exists where y - pad + r and x - pad + s are even and in range, so three quarters of the staged
// elements of a stride-2 dgrad are zeros that still go through the matrix unit (cost: DESIGN.md 4.11e).  Epilogue: the saved PReLU
// branch or a per-channel factor, then an optional addend read with stride 1 or 2.
// 104 launches, no atomics, no allocation, no synchronisation.

namespace e3dge {

constexpr int kIdPrelus = E3DGE_IDNET_PRELUS;
static_assert(kIdPrelus == kIdUnits + 1, "one PReLU per unit and the input layer's");

struct IdLayoutT { int64_t w_off[kIdConvs], total; };

static const IdLayoutT& id_layout_t() {
    static const IdLayoutT lay = [] {
        IdLayoutT t{};
        const IdLayout& l = id_layout();
        int64_t off = 0;
        for (int i = 0; i < kIdConvs; ++i) {
            t.w_off[i] = off;
            off += ((int64_t)ig_mpad(l.cin[i]) * ig_kpad(l.cout[i] * l.ks[i] * l.ks[i]) + 63) / 64 * 64;
        }
        t.total = off;
        return t;
    }();
    return lay;
}

// ---- data gradient of one convolution --------------------------------------------------------------------------------------------
struct IdDgradArgs {
    float* out; const float* g; const float* wfrag;
    const float2* in_ab; int ab_img_stride;          // g <- a g + b with (a, b) = in_ab[img * ab_img_stride + co], in-image elements only
    const float* in_scale; int in_scale_pitch;       // or g <- in_scale[co * pitch] g
    const unsigned char* mask; const float* slope;   // factor: mask ? 1 : slope[row]
    const float* scale; int scale_pitch;             // factor: scale[row * scale_pitch]  (2: the a of a BN's (a, b) pairs)
    const float* addend; int add_stride, AH, AW;     // + addend[img][row][y / add_stride][x / add_stride] where both divide
    int Cg, GH, GW, M, H, W, K, KS4, tiles;
};

template <int KS_, int STRIDE, int NT>
__global__ void __launch_bounds__(256) idnet_dgrad_kernel(IdDgradArgs a) {
    constexpr int BN = IgTile<NT>::BN, ROWS = IgTile<NT>::ROWS, PER = IgTile<NT>::PER;
    constexpr int PAD = KS_ == 3 ? 1 : 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mt = blockIdx.y * (kIgBM / 16) + wave;
    const bool live = mt * 16 < a.M;                                 // wave-uniform: the 64 -> 3 gradient has one live wave
    const int HW = a.H * a.W, GH = a.GH, GW = a.GW, K = a.K;
    const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
    const int sn = tid % BN, srow = tid / BN;
    const int spix = tile * BN + sn;
    const bool n_ok = spix < HW;
    const int sy = spix / a.W, sx = spix - sy * a.W;
    const int y0 = sy - PAD, x0 = sx - PAD;
    const float* __restrict__ src = a.g + (int64_t)img * a.Cg * GH * GW;
    const float2* __restrict__ in_ab = a.in_ab ? a.in_ab + (int64_t)img * a.ab_img_stride : nullptr;
    auto fetch = [&](int k0, float (&v)[PER]) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = k0 + srow + i * ROWS;
            const auto [co, r, s] = ig_decode<KS_>(k);
            const int ny = y0 + r, nx = x0 + s;
            bool ok = n_ok && k < K && ny >= 0 && nx >= 0;
            int gy = ny, gx = nx;
            if (STRIDE == 2) { ok = ok && !((ny | nx) & 1); gy = ny >> 1; gx = nx >> 1; }
            ok = ok && gy < GH && gx < GW;
            float x = 0.0f;
            if (ok) {
                x = src[((int64_t)co * GH + gy) * GW + gx];
                if (in_ab) { const float2 ab = in_ab[co]; x = __fmaf_rn(ab.x, x, ab.y); }
                else if (a.in_scale) x = __fmul_rn(a.in_scale[co * a.in_scale_pitch], x);
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
        const int y = pix / a.W, x = pix - y * a.W;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + r;
            if (row >= a.M) continue;
            const int64_t at = ((int64_t)img * a.M + row) * HW + pix;
            float v = __fadd_rn(acc[t][0][r], acc[t][1][r]);
            if (a.mask) { if (!a.mask[at]) v = __fmul_rn(a.slope[row], v); }
            else if (a.scale) v = __fmul_rn(a.scale[row * a.scale_pitch], v);
            if (a.addend) {
                if (a.add_stride == 1) v = __fadd_rn(v, a.addend[at]);
                else if (!((y | x) & 1)) v = __fadd_rn(v, a.addend[(((int64_t)img * a.M + row) * a.AH + (y >> 1)) * a.AW + (x >> 1)]);
            }
            a.out[at] = v;
        }
    }
}

static int id_dgrad(IdDgradArgs a, int n, int ks, int stride, hipStream_t st) {
    a.K = a.Cg * ks * ks; a.KS4 = ig_kpad(a.K) / 4;
    a.GH = id_out_size(a.H, stride); a.GW = id_out_size(a.W, stride);
    const int HW = a.H * a.W, gy = (a.M + kIgBM - 1) / kIgBM, nt = id_tile_width(HW, gy * kIgBM);
    a.tiles = id_tiles(HW, gy * kIgBM);
    const dim3 grid((unsigned)((int64_t)n * a.tiles), (unsigned)gy);
    ig_dispatch_nt(nt, [&](auto nt_c) {
        constexpr int NT = decltype(nt_c)::value;
        if (ks == 3 && stride == 1) idnet_dgrad_kernel<3, 1, NT><<<grid, dim3(256), 0, st>>>(a);
        else if (ks == 3) idnet_dgrad_kernel<3, 2, NT><<<grid, dim3(256), 0, st>>>(a);
        else if (stride == 1) idnet_dgrad_kernel<1, 1, NT><<<grid, dim3(256), 0, st>>>(a);
        else idnet_dgrad_kernel<1, 2, NT><<<grid, dim3(256), 0, st>>>(a);
    });
    return check_launch("idnet(dgrad)");
}

// ---- SE gate ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) idnet_plane_dot_kernel(float* __restrict__ dgate, const float* __restrict__ g, const float* __restrict__ res,
                                                             int HW) {
    const int64_t base = (int64_t)blockIdx.x * HW;                   // blockIdx.x = img * C + c
    float s = 0.0f;
    for (int i = threadIdx.x; i < HW; i += 64) s = __fmaf_rn(g[base + i], res[base + i], s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s = __fadd_rn(s, __shfl_xor(s, off, kWave));
    if (threadIdx.x == 0) dgate[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256) idnet_se_bwd_kernel(float2* __restrict__ ab, const float* __restrict__ dgate, const float* __restrict__ gate,
                                                           const float* __restrict__ hid, const float* __restrict__ fc1,
                                                           const float* __restrict__ fc2, const float2* __restrict__ bn2, int C, int HW) {
    __shared__ float dz[512];
    __shared__ float dh[32];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, Ch = C / 16;
    for (int c = tid; c < C; c += 256) {
        const float s = gate[(int64_t)img * C + c];
        dz[c] = __fmul_rn(dgate[(int64_t)img * C + c], __fmul_rn(s, __fsub_rn(1.0f, s)));
    }
    __syncthreads();
    for (int j = wave; j < Ch; j += 4) {
        float s = 0.0f;
        for (int c = lane; c < C; c += 64) s = __fmaf_rn(fc2[c * Ch + j], dz[c], s);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s = __fadd_rn(s, __shfl_xor(s, off, kWave));
        if (lane == 0) dh[j] = hid[(int64_t)img * Ch + j] > 0.0f ? s : 0.0f;
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        float s = 0.0f;
        for (int j = 0; j < Ch; ++j) s = __fmaf_rn(fc1[j * C + c], dh[j], s);
        const float a2 = bn2[c].x;
        ab[(int64_t)img * C + c] = make_float2(__fmul_rn(gate[(int64_t)img * C + c], a2), __fmul_rn(__fdiv_rn(s, (float)HW), a2));
    }
}

// ---- head ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kIdEmbed) idnet_head_norm_bwd_kernel(float* __restrict__ gpre, float* __restrict__ gv_out, float* __restrict__ gv_tap,
                                                                       const float* __restrict__ gf, const float* __restrict__ f,
                                                                       const float* __restrict__ norm, const float2* __restrict__ bn) {
    __shared__ float red[kIdEmbed];
    const int img = blockIdx.x, o = threadIdx.x;
    const int64_t at = (int64_t)img * kIdEmbed + o;
    const float g = gf[at], fo = f[at];
    red[o] = __fmul_rn(g, fo);
    __syncthreads();
    for (int off = kIdEmbed / 2; off > 0; off >>= 1) {
        if (o < off) red[o] = __fadd_rn(red[o], red[o + off]);
        __syncthreads();
    }
    const float gv = __fdiv_rn(__fsub_rn(g, __fmul_rn(red[0], fo)), norm[img]);
    gv_out[at] = gv;
    if (gv_tap) gv_tap[at] = gv;
    gpre[at] = __fmul_rn(gv, bn[o].x);
}

__global__ void __launch_bounds__(256) idnet_head_bwd_kernel(float* __restrict__ gx, const float* __restrict__ gpre, const float* __restrict__ w,
                                                             const float2* __restrict__ ab, int n) {
    __shared__ float gs[kIdHeadImgs * kIdEmbed];
    __shared__ float red[4][kIdHeadImgs][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.x * 64 + lane;                            // 25088 = 392 * 64
    constexpr int OQ = kIdEmbed / 4;
    for (int i0 = 0; i0 < n; i0 += kIdHeadImgs) {
        const int cnt = n - i0 < kIdHeadImgs ? n - i0 : kIdHeadImgs;
        for (int i = tid; i < kIdHeadImgs * kIdEmbed; i += 256) gs[i] = i < cnt * kIdEmbed ? gpre[(int64_t)i0 * kIdEmbed + i] : 0.0f;
        __syncthreads();
        float acc[kIdHeadImgs];
#pragma unroll
        for (int i = 0; i < kIdHeadImgs; ++i) acc[i] = 0.0f;
        const float* __restrict__ wp = w + (int64_t)(wave * OQ) * kIdHeadK + k;
#pragma unroll 8
        for (int o = 0; o < OQ; ++o) {
            const float wv = wp[(int64_t)o * kIdHeadK];
#pragma unroll
            for (int i = 0; i < kIdHeadImgs; ++i) acc[i] = __fmaf_rn(wv, gs[i * kIdEmbed + wave * OQ + o], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < kIdHeadImgs; ++i) red[wave][i][lane] = acc[i];
        __syncthreads();
        if (wave == 0) {
            const float a = ab[k / 49].x;
            for (int i = 0; i < cnt; ++i) {
                const float s = __fadd_rn(__fadd_rn(__fadd_rn(red[0][i][lane], red[1][i][lane]), red[2][i][lane]), red[3][i][lane]);
                gx[(int64_t)(i0 + i) * kIdHeadK + k] = __fmul_rn(s, a);
            }
        }
        __syncthreads();
    }
}

// ---- input layer --------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) idnet_prelu_bn_bwd_kernel(float* __restrict__ g, const unsigned char* __restrict__ mask,
                                                                 const float* __restrict__ slope, const float2* __restrict__ bn, int C, int HW,
                                                                 int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)((i / HW) % C);
    float v = g[i];
    if (!mask[i]) v = __fmul_rn(slope[c], v);
    g[i] = __fmul_rn(v, bn[c].x);
}

// ---- crop and pool ------------------------------------------------------------------------------------------------------------
// PyTorch's adaptive window of output o is [floor(o in / out), ceil((o + 1) in / out)); input i lies in the windows of the outputs
// [floor(i out / in), ceil((i + 1) out / in)).
__global__ void __launch_bounds__(256) idnet_prep_bwd_kernel(float* __restrict__ gimg, const float* __restrict__ gnet, int n, int H, int W) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n * 3 * H * W) return;
    const int w = (int)(i % W), h = (int)((i / W) % H);
    const int64_t plane = i / ((int64_t)H * W);
    const float* __restrict__ g = gnet + plane * kIdNet * kIdNet;
    const int Y0 = (int)((int64_t)h * 256 / H), Y1 = (int)((((int64_t)h + 1) * 256 + H - 1) / H);
    const int X0 = (int)((int64_t)w * 256 / W), X1 = (int)((((int64_t)w + 1) * 256 + W - 1) / W);
    float sum = 0.0f;
    for (int Y = Y0; Y < Y1; ++Y) {
        const int y = Y - 35;
        if (y < 0 || y >= 188) continue;
        const int hs = (int)((int64_t)Y * H / 256), he = (int)((((int64_t)Y + 1) * H + 255) / 256);
        const int oy0 = y * kIdNet / 188, oy1 = ((y + 1) * kIdNet + 187) / 188;
        for (int X = X0; X < X1; ++X) {
            const int x = X - 32;
            if (x < 0 || x >= 188) continue;
            const int ws = (int)((int64_t)X * W / 256), we = (int)((((int64_t)X + 1) * W + 255) / 256);
            const int ox0 = x * kIdNet / 188, ox1 = ((x + 1) * kIdNet + 187) / 188;
            float gp = 0.0f;                                         // the gradient at pixel (Y, X) of the 256 x 256 grid
            for (int oy = oy0; oy < oy1; ++oy) {
                const int ny = ((oy + 1) * 188 + kIdNet - 1) / kIdNet - oy * 188 / kIdNet;
                for (int ox = ox0; ox < ox1; ++ox) {
                    const int nx = ((ox + 1) * 188 + kIdNet - 1) / kIdNet - ox * 188 / kIdNet;
                    gp = __fadd_rn(gp, __fdiv_rn(g[oy * kIdNet + ox], (float)(ny * nx)));
                }
            }
            sum = __fadd_rn(sum, __fdiv_rn(gp, (float)((he - hs) * (we - ws))));
        }
    }
    gimg[i] = sum;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct IdBwdWs { int64_t ga, gb, gt, gs, gnet, dgate, ab, gpre, gv, total_bytes; };

static bool id_bwd_ws(int64_t n, IdBwdWs* d) {
    if (n < 1 || n > 4096) return false;
    int64_t off = 0;
    auto take = [&](int64_t floats) { const int64_t at = off; off += (floats + 63) / 64 * 64; return at; };
    d->ga = take(n * 64 * kIdNet * kIdNet);                            // the gradient at a unit's output / input, in turn
    d->gb = take(n * 64 * kIdNet * kIdNet);
    d->gt = take(n * 64 * kIdNet * kIdNet);                            // at the first 3x3's output
    d->gs = take(n * 64 * 56 * 56);                                    // the largest 1x1 branch's input gradient: unit 3
    d->gnet = take(n * 3 * kIdNet * kIdNet);
    d->dgate = take(n * 512);
    d->ab = take(n * 512 * 2);
    d->gpre = take(n * kIdEmbed);
    d->gv = take(n * kIdEmbed);
    d->total_bytes = off * (int64_t)sizeof(float);
    return true;
}

static int id_prep_bwd(float* gimg, const float* gnet, int n, int H, int W, hipStream_t st) {
    const int64_t total = (int64_t)n * 3 * H * W;
    idnet_prep_bwd_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(gimg, gnet, n, H, W);
    return check_launch("idnet(prep bwd)");
}

}  // namespace e3dge

extern "C" int64_t e3dge_idnet_packed_t_floats(void) { return id_layout_t().total; }

extern "C" int e3dge_idnet_pack_weights_t(float* packed_t, const E3dgeIdnetPackSrc* src, e3dge_stream_t stream) {
    E3DGE_REQUIRE(packed_t && src, "idnet_pack_weights_t: null pointer");
    for (int i = 0; i < kIdConvs; ++i) E3DGE_REQUIRE(src->conv_w[i], "idnet_pack_weights_t: null pointer (conv %d)", i);
    const IdLayout& l = id_layout();
    const IdLayoutT& t = id_layout_t();
    hipStream_t st = as_stream(stream);
    for (int i = 0; i < kIdConvs; ++i) ig_pack_t(packed_t + t.w_off[i], src->conv_w[i], l.cin[i], l.cout[i], l.ks[i], 1.0f, st);
    return check_launch("idnet_pack_weights_t");
}

extern "C" int64_t e3dge_idnet_saved_bytes(int n_saved) {
    IdSaved d;
    if (!id_saved(n_saved, &d)) {
        fail(E3DGE_ERR_INVALID_ARG, "idnet_saved_bytes: n_saved=%d (1..4096)", n_saved);
        return -1;
    }
    return d.total_bytes;
}

extern "C" int e3dge_idnet_embed_save(const E3dgeIdnetSaveArgs* args, e3dge_stream_t stream) {
    E3DGE_REQUIRE(args, "idnet_embed_save: null argument struct");
    return id_embed(args->net, args->saved, args->saved_bytes, args->n_saved, true, stream);
}

static bool id_image_size_ok(int n, int height, int width) {
    return height >= 1 && width >= 1 && height <= 32768 && width <= 32768 && (int64_t)n * 3 * height * width < ((int64_t)1 << 40);
}

extern "C" int64_t e3dge_idnet_bwd_ws_bytes(int n, int height, int width) {
    IdBwdWs d;
    if (!id_bwd_ws(n, &d) || !id_image_size_ok(n, height, width)) {
        fail(E3DGE_ERR_INVALID_ARG, "idnet_bwd_ws_bytes: n=%d height=%d width=%d", n, height, width);
        return -1;
    }
    return d.total_bytes;
}

extern "C" int e3dge_idnet_backward(const E3dgeIdnetBwdArgs* args, e3dge_stream_t stream) {
    E3DGE_REQUIRE(args, "idnet_backward: null argument struct");
    const E3dgeIdnetBwdArgs& a = *args;
    E3DGE_REQUIRE(a.n >= 1 && a.n <= 4096, "idnet_backward: n=%d (1..4096)", a.n);
    E3DGE_REQUIRE(a.packed && a.packed_t && a.saved && a.grad_embeddings && a.grad_images && a.ws, "idnet_backward: null pointer");
    E3DGE_REQUIRE(id_image_size_ok(a.n, a.height, a.width), "idnet_backward: height=%d width=%d (1..32768)", a.height, a.width);
    const int n = a.n;
    IdSaved sv;
    IdBwdWs d;
    E3DGE_REQUIRE(id_saved(n, &sv) && id_bwd_ws(n, &d), "idnet_backward: n=%d", n);
    E3DGE_REQUIRE(a.saved_bytes >= sv.total_bytes, "idnet_backward: saved state of %lld bytes, %lld needed", (long long)a.saved_bytes,
                  (long long)sv.total_bytes);
    E3DGE_REQUIRE(a.ws_bytes >= d.total_bytes, "idnet_backward: workspace of %lld bytes, %lld needed", (long long)a.ws_bytes, (long long)d.total_bytes);
    const IdLayout& l = id_layout();
    const IdLayoutT& lt = id_layout_t();
    hipStream_t st = as_stream(stream);
    const float* P = a.packed;
    const float* PT = a.packed_t;
    const char* S = static_cast<const char*>(a.saved);
    auto sf = [&](int64_t off) { return reinterpret_cast<const float*>(S + off); };
    auto sm = [&](int i) { return reinterpret_cast<const unsigned char*>(S + sv.mask[i]); };
    float* ws = static_cast<float*>(a.ws);
    int rc;
    auto tap = [&](int t, const float* from, int64_t floats) {
        if (a.gstage[t]) (void)hipMemcpyAsync(a.gstage[t], from, floats * sizeof(float), hipMemcpyDeviceToDevice, st);
    };
    for (int i = 0; i < kIdPrelus; ++i)
        if (a.masks[i])
            (void)hipMemcpyAsync(a.masks[i], sm(i), (size_t)n * sv.mask_c[i] * sv.mask_size[i] * sv.mask_size[i], hipMemcpyDeviceToDevice, st);
    float* gout = ws + d.ga;
    float* gin = ws + d.gb;
    float* gt = ws + d.gt;
    float* gs = ws + d.gs;
    float* dgate = ws + d.dgate;
    float2* ab = reinterpret_cast<float2*>(ws + d.ab);
    idnet_head_norm_bwd_kernel<<<dim3((unsigned)n), dim3(kIdEmbed), 0, st>>>(ws + d.gpre, ws + d.gv, a.gstage[7], a.grad_embeddings, sf(sv.f),
                                                                             sf(sv.norm), reinterpret_cast<const float2*>(P + l.bn_off[53]));
    if ((rc = check_launch("idnet_backward(head norm)"))) return rc;
    idnet_head_bwd_kernel<<<dim3(kIdHeadK / 64), dim3(256), 0, st>>>(gout, ws + d.gpre, P + l.head_w_off,
                                                                     reinterpret_cast<const float2*>(P + l.bn_off[52]), n);
    if ((rc = check_launch("idnet_backward(head)"))) return rc;
    int sizes[kIdUnits + 1];
    sizes[0] = kIdNet;
    for (int u = 0; u < kIdUnits; ++u) sizes[u + 1] = id_out_size(sizes[u], id_unit(u).stride);
    for (int u = kIdUnits - 1; u >= 0; --u) {
        const IdUnit q = id_unit(u);
        const int size = sizes[u], osize = sizes[u + 1], c1 = 1 + 2 * u, c2 = 2 + 2 * u;
        const int t = id_tap_of_unit(u);
        if (t >= 0) tap(t, gout, (int64_t)n * q.depth * osize * osize);
        idnet_plane_dot_kernel<<<dim3((unsigned)(n * q.depth)), dim3(64), 0, st>>>(dgate, gout, sf(sv.res[u]), osize * osize);
        if ((rc = check_launch("idnet_backward(plane dot)"))) return rc;
        idnet_se_bwd_kernel<<<dim3((unsigned)n), dim3(256), 0, st>>>(ab, dgate, sf(sv.gate[u]), sf(sv.hid[u]), P + l.fc1_off[u], P + l.fc2_off[u],
                                                                     reinterpret_cast<const float2*>(P + l.bn_off[c2]), q.depth, osize * osize);
        if ((rc = check_launch("idnet_backward(se)"))) return rc;
        const float* addend = gout;                                  // identity units: g_out lands on the picked positions
        if (q.shortcut >= 0) {                                       // BN scale, then the transposed 1x1 stride-2
            const int cs = 49 + q.shortcut;
            IdDgradArgs g{};
            g.out = gs; g.g = gout; g.wfrag = PT + lt.w_off[cs];
            g.in_scale = P + l.bn_off[cs]; g.in_scale_pitch = 2;
            g.Cg = q.depth; g.M = q.cin; g.H = size; g.W = size;
            if ((rc = id_dgrad(g, n, 1, q.stride, st))) return rc;
            addend = gs;
        }
        {   // (g_out gate + d mean) a2 -> transposed strided 3x3 -> PReLU derivative
            IdDgradArgs g{};
            g.out = gt; g.g = gout; g.wfrag = PT + lt.w_off[c2];
            g.in_ab = ab; g.ab_img_stride = q.depth;
            g.mask = sm(1 + u); g.slope = P + l.prelu_off[1 + u];
            g.Cg = q.depth; g.M = q.depth; g.H = size; g.W = size;
            if ((rc = id_dgrad(g, n, 3, q.stride, st))) return rc;
        }
        {   // transposed 3x3 -> BN1's a[ci] -> + the shortcut's gradient
            IdDgradArgs g{};
            g.out = gin; g.g = gt; g.wfrag = PT + lt.w_off[c1];
            g.scale = P + l.bn_off[c1]; g.scale_pitch = 2;
            g.addend = addend;
            g.add_stride = q.shortcut >= 0 ? 1 : q.stride; g.AH = q.shortcut >= 0 ? size : osize; g.AW = g.AH;
            g.Cg = q.depth; g.M = q.cin; g.H = size; g.W = size;
            if ((rc = id_dgrad(g, n, 3, 1, st))) return rc;
        }
        float* swap = gout; gout = gin; gin = swap;
    }
    const int64_t l0 = (int64_t)n * 64 * kIdNet * kIdNet;
    tap(1, gout, l0);
    idnet_prelu_bn_bwd_kernel<<<dim3((unsigned)((l0 + 255) / 256)), dim3(256), 0, st>>>(gout, sm(0), P + l.prelu_off[0],
                                                                                        reinterpret_cast<const float2*>(P + l.bn_off[0]), 64,
                                                                                        kIdNet * kIdNet, l0);
    if ((rc = check_launch("idnet_backward(input layer)"))) return rc;
    {
        IdDgradArgs g{};
        g.out = ws + d.gnet; g.g = gout; g.wfrag = PT + lt.w_off[0];
        g.Cg = 64; g.M = 3; g.H = kIdNet; g.W = kIdNet;
        if ((rc = id_dgrad(g, n, 3, 1, st))) return rc;
    }
    tap(0, ws + d.gnet, (int64_t)n * 3 * kIdNet * kIdNet);
    return id_prep_bwd(a.grad_images, ws + d.gnet, n, a.height, a.width, st);
}

static bool id_dgrad_sizes_ok(int n, int cin, int cout, int height, int width, int ksize, int stride) {
    return n >= 1 && n <= 4096 && cin >= 1 && cin <= 4096 && cout >= 1 && cout <= 4096 && height >= 1 && width >= 1 && height <= 4096 &&
           width <= 4096 && (ksize == 1 || ksize == 3) && (stride == 1 || stride == 2);
}

extern "C" int e3dge_idnet_conv_bwd(float* out, const float* g, const float* w, float* wfrag_t, const float* in_ab, const unsigned char* mask,
                                    const float* slope, const float* scale, const float* addend, int n, int cin, int cout, int height, int width,
                                    int ksize, int stride, e3dge_stream_t stream) {
    E3DGE_REQUIRE(out && g && w && wfrag_t, "idnet_conv_bwd: null pointer");
    E3DGE_REQUIRE(!mask == !slope, "idnet_conv_bwd: null pointer (mask and slope go together)");
    E3DGE_REQUIRE(!(mask && scale), "idnet_conv_bwd: mask and scale are alternatives");
    E3DGE_REQUIRE(id_dgrad_sizes_ok(n, cin, cout, height, width, ksize, stride),
                  "idnet_conv_bwd: n=%d cin=%d cout=%d height=%d width=%d ksize=%d stride=%d (n, channels, sizes 1..4096, ksize 1 or 3, stride 1 or 2)",
                  n, cin, cout, height, width, ksize, stride);
    E3DGE_REQUIRE((int64_t)(cin > cout ? cin : cout) * height * width < ((int64_t)1 << 31), "idnet_conv_bwd: image too large");
    hipStream_t st = as_stream(stream);
    ig_pack_t(wfrag_t, w, cin, cout, ksize, 1.0f, st);
    int rc;
    if ((rc = check_launch("idnet_conv_bwd(pack)"))) return rc;
    IdDgradArgs a{};
    a.out = out; a.g = g; a.wfrag = wfrag_t;
    a.in_ab = reinterpret_cast<const float2*>(in_ab); a.ab_img_stride = cout;
    a.mask = mask; a.slope = slope; a.scale = scale; a.scale_pitch = 1;
    a.addend = addend; a.add_stride = 1; a.AH = height; a.AW = width;
    a.Cg = cout; a.M = cin; a.H = height; a.W = width;
    return id_dgrad(a, n, ksize, stride, st);
}

extern "C" int e3dge_idnet_prep_bwd(float* grad_images, const float* grad_net_in, int n, int height, int width, e3dge_stream_t stream) {
    E3DGE_REQUIRE(grad_images && grad_net_in, "idnet_prep_bwd: null pointer");
    E3DGE_REQUIRE(n >= 1 && n <= 4096, "idnet_prep_bwd: n=%d (1..4096)", n);
    E3DGE_REQUIRE(id_image_size_ok(n, height, width), "idnet_prep_bwd: height=%d width=%d (1..32768)", height, width);
    return id_prep_bwd(grad_images, grad_net_in, n, height, width, as_stream(stream));
}
