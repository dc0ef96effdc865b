// StyleGAN2 discriminator, backward: the gradient of the logits with respect to the input images (included at the end of disc.hip).
// The network is frozen, as the encoder step freezes it (trainer.py:1212), so only data gradients exist.
//
// The saving forward keeps every lrelu's OUTPUT (DcSaved); its sign is the lrelu's branch, as in FusedLeakyReLU's own backward, so no
// mask tensors exist.  In reverse order:
//
//   head_bwd_hid   g_hid = g_logit w2 lrelu'(hid).
//   head_bwd       sum_o W1[o][k] g_hid[o] for up to 8 images per pass over the matrix: a wave owns 64 k and a quarter of o in
//                  ascending order, the four quarters are added in order.
//   dgrad 3x3      the final convolution: lrelu' from the saved activation while staging, the forward kernel on the transposed, flipped
//                  weight image, M = 513.
//   stddev_bwd     g_feat = g_cat[:, :C] + (sum of the stddev channel's gradient over the sub-batch) (x - mean) / (N group sd).
//   per block      skip:  g / sqrt 2 while staging -> transposed 1x1 stride 2 -> Blur^T (e3dge_upfirdn2d in the adjoint geometry)
//                  main:  g lrelu'(a) (the merge's 1 / sqrt 2 and the lrelu's sqrt 2 cancel) -> transposed 3x3 stride 2 -> Blur^T
//                         -> lrelu'(t) while staging -> transposed 3x3 + the skip branch's gradient in the epilogue.
//   stem           lrelu' while staging, the 1x1 C0 -> in_channels gradient (one live wave), then pool_256's adjoint (e3dge_avgpool_bwd).
//
// Every data gradient is disc_gemm_kernel (disc.hip) on the transposed, tap-flipped weight image with its sign-chosen staging factor.
// The transposed stride 2 is a predicate in its gather (three quarters of the staged elements are zeros that still go through the
// matrix unit), as in idnet_bwd.h.  No atomics, no allocation, no synchronisation.

namespace e3dge {

__global__ void __launch_bounds__(256) disc_head_bwd_hid_kernel(float* __restrict__ ghid, const float* __restrict__ glogit, const float* __restrict__ hid,
                                                                const float* __restrict__ w2, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int img = i / kDcHid, o = i - img * kDcHid;
    const float m = hid[i] > 0.0f ? kDcSqrt2 : kDcSlope * kDcSqrt2;
    ghid[i] = __fmul_rn(__fmul_rn(glogit[img], w2[o]), m);
}

__global__ void __launch_bounds__(256) disc_head_bwd_kernel(float* __restrict__ gx, const float* __restrict__ ghid, const float* __restrict__ w, int n) {
    constexpr int IMGS = 8, OQ = kDcHid / 4;
    __shared__ float gs[IMGS * kDcHid];
    __shared__ float red[4][IMGS][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.x * 64 + lane;                            // 8192 = 128 * 64
    for (int i0 = 0; i0 < n; i0 += IMGS) {
        const int cnt = n - i0 < IMGS ? n - i0 : IMGS;
        for (int i = tid; i < IMGS * kDcHid; i += 256) gs[i] = i < cnt * kDcHid ? ghid[(int64_t)i0 * kDcHid + i] : 0.0f;
        __syncthreads();
        float acc[IMGS];
#pragma unroll
        for (int i = 0; i < IMGS; ++i) acc[i] = 0.0f;
        const float* __restrict__ wp = w + (int64_t)(wave * OQ) * kDcHeadK + k;
#pragma unroll 8
        for (int o = 0; o < OQ; ++o) {
            const float wv = wp[(int64_t)o * kDcHeadK];
#pragma unroll
            for (int i = 0; i < IMGS; ++i) acc[i] = __fmaf_rn(wv, gs[i * kDcHid + wave * OQ + o], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < IMGS; ++i) red[wave][i][lane] = acc[i];
        __syncthreads();
        if (wave == 0) {
            for (int i = 0; i < cnt; ++i)
                gx[(int64_t)(i0 + i) * kDcHeadK + k] = __fadd_rn(__fadd_rn(__fadd_rn(red[0][i][lane], red[1][i][lane]), red[2][i][lane]), red[3][i][lane]);
        }
        __syncthreads();
    }
}

// d s_j / d x[b, e] = (x[b, e] - mean_j[e]) / (N group sd_j[e]) for the samples b of sub-batch j; s_j reaches group * HW elements
__global__ void __launch_bounds__(256) disc_stddev_bwd_kernel(float* __restrict__ gfeat, const float* __restrict__ gcat, const float* __restrict__ feat,
                                                              int B, int group, int C, int HW) {
    const int j = blockIdx.x, n_sub = B / group, tid = threadIdx.x;
    const int64_t N = (int64_t)C * HW;
    float G = 0.0f;                                                  // every thread adds the same values in the same order
    for (int g = 0; g < group; ++g)
        for (int p = 0; p < HW; ++p) G = __fadd_rn(G, gcat[(int64_t)(g * n_sub + j) * (N + HW) + N + p]);
    const float coef = __fdiv_rn(G, (float)N * (float)group);
    for (int64_t e = tid; e < N; e += 256) {
        float m = 0.0f;
        for (int g = 0; g < group; ++g) m = __fadd_rn(m, feat[(int64_t)(g * n_sub + j) * N + e]);
        m = __fdiv_rn(m, (float)group);
        float var = 0.0f;
        for (int g = 0; g < group; ++g) {
            const float d = __fsub_rn(feat[(int64_t)(g * n_sub + j) * N + e], m);
            var = __fmaf_rn(d, d, var);
        }
        const float sd = __fsqrt_rn(__fadd_rn(__fdiv_rn(var, (float)group), 1e-8f));
        const float c = __fdiv_rn(coef, sd);
        for (int g = 0; g < group; ++g) {
            const int64_t b = g * n_sub + j;
            const float d = __fsub_rn(feat[b * N + e], m);
            gfeat[b * N + e] = __fmaf_rn(c, d, gcat[b * (N + HW) + e]);
        }
    }
}

// the data gradient of one convolution of the family: g (n, cout, GH, GW) -> out (n, cin, H, W)
static int dc_dgrad(float* out, const float* g, const float* wfrag_t, const float* sign, float s_pos, float s_neg, const float* addend, int n, int cin,
                    int cout, int H, int W, int ks, int stride, hipStream_t st) {
    DcGemmArgs a{};
    a.out = out; a.in = g; a.wfrag = wfrag_t; a.sign = sign; a.s_pos = s_pos; a.s_neg = s_neg; a.scaled = sign != nullptr || s_pos != 1.0f;
    a.addend = addend;
    a.Cin = cout; a.M = cin; a.OH = H; a.OW = W;
    a.IH = stride == 1 ? H : (H - ks) / 2 + 1; a.IW = stride == 1 ? W : (W - ks) / 2 + 1;
    a.pad = stride == 1 ? ks / 2 : ks - 1;
    return dc_gemm(a, n, ks, stride == 1 ? 0 : 2, st);
}

}  // namespace e3dge

extern "C" int e3dge_disc_backward(const E3dgeDiscBwdArgs* args, e3dge_stream_t stream) {
    E3DGE_REQUIRE(args, "disc_backward: null argument struct");
    const E3dgeDiscBwdArgs& a = *args;
    DcNet net;
    const int f = dc_shape("disc_backward", a.n, a.height, a.width, a.init_size, a.channel_multiplier, a.in_channels, &net);
    if (!f) return E3DGE_ERR_INVALID_ARG;
    E3DGE_REQUIRE(a.packed && a.saved && a.grad_logits && a.grad_images && a.ws, "disc_backward: null pointer");
    const int n = a.n;
    DcWs d;
    DcSaved sv;
    dc_ws(net, n, f, true, &d);
    dc_saved(net, n, &sv);
    E3DGE_REQUIRE(a.saved_bytes >= sv.total_floats * (int64_t)sizeof(float), "disc_backward: saved state of %lld bytes, %lld needed",
                  (long long)a.saved_bytes, (long long)(sv.total_floats * (int64_t)sizeof(float)));
    E3DGE_REQUIRE(a.ws_bytes >= d.total_floats * (int64_t)sizeof(float), "disc_backward: workspace of %lld bytes, %lld needed", (long long)a.ws_bytes,
                  (long long)(d.total_floats * (int64_t)sizeof(float)));
    DcLayout l;
    dc_layout(net, &l);
    hipStream_t st = as_stream(stream);
    const float* P = a.packed;
    const float* S = static_cast<const float*>(a.saved);
    float* ws = static_cast<float*>(a.ws);
    int rc;
    auto tap = [&](int t, const float* from, int64_t floats) {
        if (a.gstage[t]) (void)hipMemcpyAsync(a.gstage[t], from, floats * sizeof(float), hipMemcpyDeviceToDevice, st);
    };
    const float up = kDcSqrt2, dn = kDcSlope * kDcSqrt2, inv = 1.0f / kDcSqrt2;
    float* ghid = ws + d.ghid;
    float* gfin = ws + d.gt[1];
    float* gcat = ws + d.gcat;
    disc_head_bwd_hid_kernel<<<dim3((unsigned)((n * kDcHid + 255) / 256)), dim3(256), 0, st>>>(ghid, a.grad_logits, S + sv.hid, P + l.lin2_w, n * kDcHid);
    if ((rc = check_launch("disc_backward(head hidden)"))) return rc;
    disc_head_bwd_kernel<<<dim3(kDcHeadK / 64), dim3(256), 0, st>>>(gfin, ghid, P + l.lin1_w, n);
    if ((rc = check_launch("disc_backward(head)"))) return rc;
    tap(E3DGE_DISC_TAP_FINAL, gfin, (int64_t)n * 512 * 16);
    if ((rc = dc_dgrad(gcat, gfin, P + l.fin_wt, S + sv.fin, up, dn, nullptr, n, 513, 512, 4, 4, 3, 1, st))) return rc;
    int p = 0;
    float* gout = ws + d.g[p];
    disc_stddev_bwd_kernel<<<dim3((unsigned)(n / dc_group(n))), dim3(256), 0, st>>>(gout, gcat, S + sv.last, n, dc_group(n), 512, 16);
    if ((rc = check_launch("disc_backward(stddev)"))) return rc;
    for (int i = net.n_blocks - 1; i >= 0; --i) {
        const int ci = net.c[i], co = net.c[i + 1], s = net.size[i], h = s / 2;
        float* gin = ws + d.g[1 - p];
        float* gb = ws + d.gt[0];
        float* gskip = ws + d.gt[1];
        float* gt1 = ws + d.gt[2];
        tap(i, gout, (int64_t)n * co * h * h);
        if ((rc = dc_dgrad(gb, gout, P + l.sk_wt[i], nullptr, inv, inv, nullptr, n, ci, co, s - 1, s - 1, 1, 2, st))) return rc;
        if ((rc = dc_blur(gskip, gb, P + l.blur_flip, (int64_t)n * ci, s - 1, 2, 2, st))) return rc;      // adjoint of pad (1, 1): k - 1 - 1 = 2
        if ((rc = dc_dgrad(gb, gout, P + l.c2_wt[i], S + sv.act2[i], 1.0f, kDcSlope, nullptr, n, ci, co, s + 1, s + 1, 3, 2, st))) return rc;
        if ((rc = dc_blur(gt1, gb, P + l.blur_flip, (int64_t)n * ci, s + 1, 1, 1, st))) return rc;        // adjoint of pad (2, 2): k - 2 - 1 = 1
        if ((rc = dc_dgrad(gin, gt1, P + l.c1_wt[i], S + sv.t1[i], up, dn, gskip, n, ci, ci, s, s, 3, 1, st))) return rc;
        gout = gin; p = 1 - p;
    }
    tap(E3DGE_DISC_TAP_STEM, gout, (int64_t)n * net.c[0] * net.init * net.init);
    float* gimg = f > 1 ? ws + d.gpool : a.grad_images;
    if ((rc = dc_dgrad(gimg, gout, P + l.stem_wt, S + sv.stem, up, dn, nullptr, n, net.cin, net.c[0], net.init, net.init, 1, 1, st))) return rc;
    if (f > 1) return e3dge_avgpool_bwd(a.grad_images, gimg, (int64_t)n * net.cin, a.height, a.width, f, stream);
    return E3DGE_OK;
}

extern "C" int e3dge_disc_conv_dgrad(float* out, const float* g, const float* w, float* wfrag_t, const float* sign, float s_pos, float s_neg,
                                     const float* addend, int n, int cin, int cout, int height, int width, int ksize, int stride, float scale,
                                     e3dge_stream_t stream) {
    E3DGE_REQUIRE(out && g && w && wfrag_t, "disc_conv_dgrad: null pointer");
    E3DGE_REQUIRE(dc_conv_sizes_ok(n, cin, cout, height, width, ksize, stride),
                  "disc_conv_dgrad: n=%d cin=%d cout=%d height=%d width=%d ksize=%d stride=%d (n, channels 1..4096, sizes ksize..4096, ksize 1 or 3, stride 1 or 2)",
                  n, cin, cout, height, width, ksize, stride);
    hipStream_t st = as_stream(stream);
    ig_pack_t(wfrag_t, w, cin, cout, ksize, scale, st);
    int rc;
    if ((rc = check_launch("disc_conv_dgrad(pack)"))) return rc;
    return dc_dgrad(out, g, wfrag_t, sign, s_pos, s_neg, addend, n, cin, cout, height, width, ksize, stride, st);
}
