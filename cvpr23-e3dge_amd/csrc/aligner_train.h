// The 2-D residual aligner (ADA), trainable form: the network's forward with its saved state and its backward, composed of aln_conv_kernel
// and the kernels of aligner_bwd.h.  Included by aligner.hip after the packed layout.
//
// Forward with saved state, both forms: every convolution runs with no trailing affine and writes its raw sums (c0; per unit c1, c2 and the
// 1x1 branch csc), which are what the backward of the BatchNorms and the PReLU branch need; aln_bn_apply_kernel then does the epilogue's own
// arithmetic (a v + b, PReLU, shortcut), so on running statistics the output is the plain forward's bit for bit.  On batch statistics
// aln_bn_stats_kernel runs between the two and writes the (a, b) pair the apply step (trailing and shortcut BatchNorms, the stem's) or the
// next gather (leading BatchNorm: in_ab, padded taps stay 0) reads.
//
// Backward of a unit, from the gradient gy of its output: the trailing BatchNorm (aln_norm_*), the second convolution's weight and data
// gradient, the PReLU, the first convolution's weight and data gradient, the shortcut (1x1 branch: its BatchNorm, weight and data gradient;
// pick: gy itself -- every such unit has stride 1), and last the leading BatchNorm, whose kernel adds the shortcut's gradient
// and, at a stage's first unit, the skip connection's: every fan-in sum is an addend of that step.  The gradient of a concatenated input is
// written split (AlnDst2): the up-sampled part goes to aln_up2_bwd_kernel, the skip part waits as that addend.
#pragma once

namespace e3dge {

struct AlnBnRef { int src; int ch; int chan; };                      // gamma's index in the source list (beta, mean, var follow); channels; offset
struct AlnNetUnit { AlnBnRef bn0, bn4, bnsc; int w1, prelu, w2, wsc; };
struct AlnNet {
    int stem_w, stem_prelu;
    AlnBnRef stem_bn;
    AlnNetUnit u[kAlnUnits];
    int64_t goff[kAlnSources + 1];                                   // offset of every source tensor's gradient in the gradient buffer
    int channels;                                                    // BatchNorm channels in all
    int64_t t_stem, t_w1[kAlnUnits], t_w2[kAlnUnits], t_wsc[kAlnUnits], t_total;   // the transposed images
};

static int64_t aln_image_t_floats(int cin, int cout, int ks) { return (int64_t)ig_mpad(cin) * ig_kpad(cout * ks * ks); }

static const AlnNet& aln_net() {
    static const AlnNet net = [] {
        AlnNet t{};
        int at = 0, chan = 0;
        int64_t off = 0, toff = 0;
        auto one = [&](int64_t numel) { t.goff[at] = off; off += numel; return at++; };
        auto bn = [&](int ch) { AlnBnRef r{at, ch, chan}; for (int i = 0; i < 4; ++i) one(ch); chan += ch; return r; };
        auto timg = [&](int cin, int cout, int ks) { const int64_t o = toff; toff += (aln_image_t_floats(cin, cout, ks) + 63) / 64 * 64; return o; };
        t.stem_w = one((int64_t)kAlnStem * kAlnIn * 9); t.stem_bn = bn(kAlnStem); t.stem_prelu = one(kAlnStem);
        t.t_stem = timg(kAlnIn, kAlnStem, 3);
        for (int u = 0; u < kAlnUnits; ++u) {
            const AlnUnit q = kAlnUnit[u];
            AlnNetUnit& n = t.u[u];
            n.bn0 = bn(q.cin); n.w1 = one((int64_t)q.depth * q.cin * 9); n.prelu = one(q.depth); n.w2 = one((int64_t)q.depth * q.depth * 9); n.bn4 = bn(q.depth);
            t.t_w1[u] = timg(q.cin, q.depth, 3); t.t_w2[u] = timg(q.depth, q.depth, 3);
            n.wsc = -1;
            if (q.cin != q.depth) { n.wsc = one((int64_t)q.depth * q.cin); n.bnsc = bn(q.depth); t.t_wsc[u] = timg(q.cin, q.depth, 1); }
        }
        t.goff[at] = off;
        t.channels = chan;
        t.t_total = toff;
        return t;
    }();
    return net;
}

// Every unit that keeps its channel count has stride 1, so its shortcut's adjoint is the identity and aln_pick_bwd_kernel has no launch here.
constexpr bool aln_identity_units_have_stride_1() {
    for (int u = 0; u < kAlnUnits; ++u)
        if (kAlnUnit[u].cin == kAlnUnit[u].depth && kAlnUnit[u].stride != 1) return false;
    return true;
}
static_assert(aln_identity_units_have_stride_1(), "a strided identity shortcut needs aln_pick_bwd_kernel in aln_stage_bwd");

constexpr int kAlnStageSize[6] = {256, 128, 64, 64, 128, 256};       // the input size of every stage's first unit

// ---- saved state (floats; per image unless said) -------------------------------------------------------------------------------------------
struct AlnSaved { int64_t c0, feat1, c1[kAlnUnits], t1[kAlnUnits], c2[kAlnUnits], csc[kAlnUnits], y[kAlnUnits], up[3], ab, part, total_bytes; };

static bool aln_saved(int64_t n, AlnSaved* d) {
    if (n < 1 || n > 256) return false;
    int64_t off = 0;
    auto take = [&](int64_t floats) { const int64_t at = off; off += (floats + 63) / 64 * 64; return at; };
    const int64_t P = (int64_t)kAlnSize * kAlnSize;
    d->c0 = take(n * kAlnStem * P); d->feat1 = take(n * kAlnStem * P);
    for (int u = 0; u < kAlnUnits; ++u) {
        const AlnUnit q = kAlnUnit[u];
        int64_t S = kAlnStageSize[u / 3];
        for (int v = u / 3 * 3; v < u; ++v) S /= kAlnUnit[v].stride;
        const int64_t So = S / q.stride;
        d->c1[u] = take(n * q.depth * S * S); d->t1[u] = take(n * q.depth * S * S); d->c2[u] = take(n * q.depth * So * So);
        d->csc[u] = q.cin != q.depth ? take(n * q.depth * So * So) : -1;
        d->y[u] = u + 1 < kAlnUnits ? take(n * q.depth * So * So) : -1;  // the last unit writes the output
    }
    d->up[0] = take(n * 64 * (P / 16)); d->up[1] = take(n * 32 * (P / 4)); d->up[2] = take(n * 16 * P);
    d->ab = take(2 * aln_net().channels);                            // per call: the (a, b) pairs of the batch statistics
    d->part = take(2 * (aln_norm_ws_bytes(n, 112, 256 * 256) / (int64_t)sizeof(double)));   // per call: the statistics' partial sums
    d->total_bytes = off * (int64_t)sizeof(float);
    return true;
}

// ---- backward workspace (floats) -----------------------------------------------------------------------------------------------------------
struct AlnBwdWs { int64_t gy[2], gstage, gc2, gt1, gxn, gsc, gcsc, skip[3], gup, d256, wg, norm, total_bytes; };

static bool aln_bwd_ws(int64_t n, AlnBwdWs* d) {
    if (n < 1 || n > 256) return false;
    int64_t off = 0;
    auto take = [&](int64_t floats) { const int64_t at = off; off += (floats + 63) / 64 * 64; return at; };
    const int64_t P = (int64_t)kAlnSize * kAlnSize;
    d->gy[0] = take(n * 16 * P); d->gy[1] = take(n * 16 * P);      // a unit's output gradient and its input gradient, alternating
    d->gstage = take(n * 16 * P);                                    // a stage's output gradient, then its input's
    d->gc2 = take(n * 16 * P); d->gt1 = take(n * 32 * P); d->gxn = take(n * 32 * P); d->gsc = take(n * 32 * P); d->gcsc = take(n * 16 * P);
    d->skip[0] = take(n * 16 * P); d->skip[1] = take(n * 32 * (P / 4)); d->skip[2] = take(n * 48 * (P / 16));
    d->gup = take(n * 16 * P); d->d256 = take(n * kAlnIn * P);
    int64_t wg = 0;
    for (int u = 0; u < kAlnUnits; ++u) {
        const AlnUnit q = kAlnUnit[u];
        int S = kAlnStageSize[u / 3];
        for (int v = u / 3 * 3; v < u; ++v) S /= kAlnUnit[v].stride;
        const int64_t a = aln_wgrad_ws_floats(n, q.cin, q.depth, S, S, 3, 1), b = aln_wgrad_ws_floats(n, q.depth, q.depth, S, S, 3, q.stride);
        wg = a > wg ? a : wg;
        wg = b > wg ? b : wg;
    }
    const int64_t stem = aln_wgrad_ws_floats(n, kAlnIn, kAlnStem, kAlnSize, kAlnSize, 3, 1);
    d->wg = take(stem > wg ? stem : wg);
    d->norm = take(2 * (aln_norm_ws_bytes(n, 112, 256 * 256) / (int64_t)sizeof(double)));
    d->total_bytes = off * (int64_t)sizeof(float);
    return true;
}

// ---- launch helpers ---------------------------------------------------------------------------------------------------------------------------
static int aln_apply(float* out, const float* in, const float* ab, const float* slope, const float* sc, const float* sc_ab, int n, int c, int oh, int ow,
                     int sh, int sw, int stride, int mode, hipStream_t st) {
    AlnApplyArgs a;
    a.out = out; a.in = in; a.ab = reinterpret_cast<const float2*>(ab); a.slope = slope; a.sc = sc; a.sc_ab = reinterpret_cast<const float2*>(sc_ab);
    a.C = c; a.OH = oh; a.OW = ow; a.SH = sh; a.SW = sw; a.stride = stride; a.sc_mode = mode; a.total = (int64_t)n * c * oh * ow;
    aln_bn_apply_kernel<<<dim3(aln_blocks(a.total)), dim3(256), 0, st>>>(a);
    return check_launch("aln(apply)");
}

static int aln_stats(float* ab, double* stats, double* part, const float* in0, const float* in1, const float* gamma, const float* beta, int n, int c,
                     int split, int hw, hipStream_t st) {
    const int segs = aln_segments(hw);
    aln_bn_stats_kernel<<<dim3(segs, n, c), dim3(256), 0, st>>>(part, AlnSrc2{in0, in1, split, c - split}, hw);
    aln_bn_stats_fold_kernel<<<dim3((c + 63) / 64), dim3(64), 0, st>>>(reinterpret_cast<float2*>(ab), stats, part, gamma, beta, c, n * segs, (double)n * hw);
    return check_launch("aln(stats)");
}

// BatchNorm backward; gx split at gsplit (gx1 NULL: one tensor); dgamma / dbeta NULL: not wanted
static int aln_norm_bwd(float* gx0, float* gx1, int gsplit, float* dgamma, float* dbeta, const float* gy, const float* in0, const float* in1, int split,
                        const float* gamma, const double* stats, const float* rmean, const float* rvar, const float* add0, const float* add1, double* ws,
                        int n, int c, int hw, int train, hipStream_t st) {
    const int segs = aln_segments(hw);
    double* coef = ws + (int64_t)2 * c * n * segs;
    const AlnSrc2 src{in0, in1, split, c - split};
    const AlnNormStat ns{train ? stats : nullptr, rmean, rvar};
    const bool sums = train || dgamma || dbeta;
    if (sums) aln_norm_sums_kernel<<<dim3(segs, n, c), dim3(256), 0, st>>>(ws, gy, src, ns, c, hw);
    aln_norm_fold_kernel<<<dim3((c + 63) / 64), dim3(64), 0, st>>>(coef, dgamma, dbeta, sums ? ws : nullptr, gamma, ns, c, n * segs, (double)n * hw, train);
    const int64_t total = (int64_t)n * c * hw;
    aln_norm_bwd_kernel<<<dim3(aln_blocks(total)), dim3(256), 0, st>>>(AlnDst2{gx0, gx1, gx1 ? gsplit : c, gx1 ? c - gsplit : 0}, gy, src, add0, add1, coef, c,
                                                                       hw, total, train);
    return check_launch("aln(norm_bwd)");
}

static int aln_prelu_bwd(float* gx, float* dslope, const float* gy, const float* pre, const float* pre_ab, const float* slope, double* ws, int n, int c,
                         int hw, hipStream_t st) {
    const int segs = aln_segments(hw);
    aln_prelu_bwd_kernel<<<dim3(segs, n, c), dim3(256), 0, st>>>(gx, dslope ? ws : nullptr, gy, pre, reinterpret_cast<const float2*>(pre_ab), slope, c, hw);
    if (dslope) aln_prelu_fold_kernel<<<dim3((c + 63) / 64), dim3(64), 0, st>>>(dslope, ws, c, n * segs);
    return check_launch("aln(prelu_bwd)");
}

// the sum of every 4 x 4 block, rows then columns ascending, in float64: the adjoint of the nearest x4 read of the thumb
__global__ void __launch_bounds__(256) aln_down4_kernel(float* __restrict__ out, const float* __restrict__ in, int H, int W, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int hw = H * W;
    const int64_t plane = i / hw;
    const int pix = (int)(i - plane * hw), y = pix / W, x = pix - y * W;
    const float* __restrict__ p = in + (plane * 4 * H + 4 * y) * 4 * W + 4 * x;
    double s = 0.0;
    for (int dy = 0; dy < 4; ++dy)
        for (int dx = 0; dx < 4; ++dx) s += (double)p[dy * 4 * W + dx];
    out[i] = (float)s;
}

// one byte per element: 1 where a v + b (ab NULL: v) is positive
__global__ void __launch_bounds__(256) aln_branch_kernel(uint8_t* __restrict__ out, const float* __restrict__ in, const float2* __restrict__ ab, int C, int hw,
                                                         int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float v = in[i];
    if (ab) { const float2 e = ab[(i / hw) % C]; v = __fmaf_rn(e.x, v, e.y); }
    out[i] = v > 0.0f ? 1 : 0;
}

// ---- the network ---------------------------------------------------------------------------------------------------------------------------------
struct AlnRun {
    int n, train;
    const float* P; const float* const* src; float* S; AlnSaved lay; double* stats; hipStream_t st;
    const float* ab(const AlnBnRef& b, int64_t packed_off) const { return train ? S + lay.ab + 2 * b.chan : P + packed_off; }
    int batch_stats(const AlnBnRef& b, const float* in0, const float* in1, int split, int hw) const {
        if (!train) return E3DGE_OK;
        return aln_stats(S + lay.ab + 2 * b.chan, stats + 2 * b.chan, reinterpret_cast<double*>(S + lay.part), in0, in1, src[b.src], src[b.src + 1], n, b.ch, split,
                         hw, st);
    }
};

static int aln_stage_saving(const AlnRun& r, float* out, const float* in0, const float* in1, int split, int u0, int S) {
    const AlnLayout& l = aln_layout();
    const AlnNet& net = aln_net();
    int rc, size = S;
    for (int i = 0; i < 3; ++i) {
        const int u = u0 + i;
        const AlnUnit q = kAlnUnit[u];
        const AlnNetUnit& m = net.u[u];
        const int osize = aln_out_size(size, 3, q.stride), n = r.n;
        float* c1 = r.S + r.lay.c1[u];
        float* t1 = r.S + r.lay.t1[u];
        float* c2 = r.S + r.lay.c2[u];
        float* csc = q.cin != q.depth ? r.S + r.lay.csc[u] : nullptr;
        float* y = i == 2 ? out : r.S + r.lay.y[u];
        if ((rc = r.batch_stats(m.bn0, in0, in1, split, size * size))) return rc;
        if ((rc = aln_conv({c1, in0, in1, r.P + l.w1[u], r.ab(m.bn0, l.bn0[u]), nullptr, nullptr, nullptr, n, q.cin, split, 0, q.depth, size, size, 3, 1, kAlnScNone},
                           r.st)))
            return rc;
        if ((rc = aln_apply(t1, c1, nullptr, r.P + l.prelu[u], nullptr, nullptr, n, q.depth, size, size, size, size, 1, kAlnScNone, r.st))) return rc;
        if ((rc = aln_conv({c2, t1, nullptr, r.P + l.w2[u], nullptr, nullptr, nullptr, nullptr, n, q.depth, q.depth, 0, q.depth, size, size, 3, q.stride, kAlnScNone},
                           r.st)))
            return rc;
        if ((rc = r.batch_stats(m.bn4, c2, nullptr, q.depth, osize * osize))) return rc;
        if (csc) {
            if ((rc = aln_conv({csc, in0, in1, r.P + l.wsc[u], nullptr, nullptr, nullptr, nullptr, n, q.cin, split, 0, q.depth, size, size, 1, q.stride, kAlnScNone},
                               r.st)))
                return rc;
            if ((rc = r.batch_stats(m.bnsc, csc, nullptr, q.depth, osize * osize))) return rc;
            if ((rc = aln_apply(y, c2, r.ab(m.bn4, l.bn4[u]), nullptr, csc, r.ab(m.bnsc, l.bnsc[u]), n, q.depth, osize, osize, osize, osize, 1, kAlnScAffine, r.st)))
                return rc;
        } else if ((rc = aln_apply(y, c2, r.ab(m.bn4, l.bn4[u]), nullptr, in0, nullptr, n, q.depth, osize, osize, size, size, q.stride, kAlnScPick, r.st))) {
            return rc;
        }
        in0 = y; in1 = nullptr; split = q.depth;
        size = osize;
    }
    return E3DGE_OK;
}

struct AlnBwdRun {
    int n, train, want_input;
    const float* P; const float* T; const float* const* src; const uint8_t* want; const float* S; AlnSaved lay; const double* stats;
    float* W; AlnBwdWs ws; float* grads; hipStream_t st;
    float* grad(int s) const { return want[s] ? grads + aln_net().goff[s] : nullptr; }
    const float* ab(const AlnBnRef& b, int64_t packed_off) const { return train ? S + lay.ab + 2 * b.chan : P + packed_off; }
    double* norm_ws() const { return reinterpret_cast<double*>(W + ws.norm); }
    int norm_bwd(const AlnBnRef& b, float* gx0, float* gx1, int gsplit, const float* gy, const float* in0, const float* in1, int split, const float* add0,
                 const float* add1, int hw) const {
        return aln_norm_bwd(gx0, gx1, gsplit, grad(b.src), grad(b.src + 1), gy, in0, in1, split, src[b.src], train ? stats + 2 * b.chan : nullptr, src[b.src + 2], src[b.src + 3],
                            add0, add1, norm_ws(), n, b.ch, hw, train, st);
    }
};

// One stage backwards.  gy: the gradient of the stage's output (consumed).  The stage's input gradient goes to gx0 (and gx1 from channel split
// on, for a concatenated input), plus `skip` (the gradient the stage's input receives from its skip connection; may be NULL).
// Returns through *rc.
static int aln_stage_bwd(const AlnBwdRun& r, float* gx0, float* gx1, const float* gy_in, const float* in0, const float* in1, int split, int u0, int S,
                         const float* skip) {
    const AlnLayout& l = aln_layout();
    const AlnNet& net = aln_net();
    int rc, sizes[4] = {S, 0, 0, 0};
    for (int i = 0; i < 3; ++i) sizes[i + 1] = aln_out_size(sizes[i], 3, kAlnUnit[u0 + i].stride);
    const float* gy = gy_in;
    for (int i = 2; i >= 0; --i) {
        const int u = u0 + i, n = r.n;
        const AlnUnit q = kAlnUnit[u];
        const AlnNetUnit& m = net.u[u];
        const int size = sizes[i], osize = sizes[i + 1], hw = size * size, ohw = osize * osize;
        const float* x0 = i == 0 ? in0 : r.S + r.lay.y[u - 1];       // the unit's input
        const float* x1 = i == 0 ? in1 : nullptr;
        const int xs = i == 0 ? split : q.cin;
        const float* c1 = r.S + r.lay.c1[u];
        const float* t1 = r.S + r.lay.t1[u];
        const float* c2 = r.S + r.lay.c2[u];
        float* gc2 = r.W + r.ws.gc2;
        float* gt1 = r.W + r.ws.gt1;
        float* gxn = r.W + r.ws.gxn;
        float* wg = r.W + r.ws.wg;
        // res_layer.4, .3
        if ((rc = r.norm_bwd(m.bn4, gc2, nullptr, 0, gy, c2, nullptr, q.depth, nullptr, nullptr, ohw))) return rc;
        if (r.want[m.w2] && (rc = aln_wgrad({r.grad(m.w2), gc2, t1, nullptr, nullptr, wg, n, q.depth, q.depth, 0, q.depth, size, size, 3, q.stride}, r.st))) return rc;
        if ((rc = aln_dgrad({gt1, gc2, r.T + net.t_w2[u], nullptr, nullptr, n, q.depth, q.depth, size, size, 3, q.stride}, r.st))) return rc;
        // res_layer.2 (in place), .1
        if ((rc = aln_prelu_bwd(gt1, r.grad(m.prelu), gt1, c1, nullptr, r.src[m.prelu], r.norm_ws(), n, q.depth, hw, r.st))) return rc;
        if (r.want[m.w1] &&
            (rc = aln_wgrad({r.grad(m.w1), gt1, x0, x1, r.ab(m.bn0, l.bn0[u]), wg, n, q.cin, xs, 0, q.depth, size, size, 3, 1}, r.st)))
            return rc;
        if ((rc = aln_dgrad({gxn, gt1, r.T + net.t_w1[u], nullptr, nullptr, n, q.cin, q.depth, size, size, 3, 1}, r.st))) return rc;
        // the shortcut
        const float* gsc = gy;                                       // MaxPool2d(1, 1): the identity (aln_identity_units_have_stride_1)
        if (q.cin != q.depth) {
            float* gcsc = r.W + r.ws.gcsc;
            if ((rc = r.norm_bwd(m.bnsc, gcsc, nullptr, 0, gy, r.S + r.lay.csc[u], nullptr, q.depth, nullptr, nullptr, ohw))) return rc;
            if (r.want[m.wsc] && (rc = aln_wgrad({r.grad(m.wsc), gcsc, x0, x1, nullptr, wg, n, q.cin, xs, 0, q.depth, size, size, 1, q.stride}, r.st))) return rc;
            if ((rc = aln_dgrad({r.W + r.ws.gsc, gcsc, r.T + net.t_wsc[u], nullptr, nullptr, n, q.cin, q.depth, size, size, 1, q.stride}, r.st))) return rc;
            gsc = r.W + r.ws.gsc;
        }
        // res_layer.0: the unit's input gradient, with the shortcut's and (first unit) the skip connection's as addends
        float* d0 = i == 0 ? gx0 : r.W + r.ws.gy[i & 1];
        float* d1 = i == 0 ? gx1 : nullptr;
        if ((rc = r.norm_bwd(m.bn0, d0, d1, xs, gxn, x0, x1, xs, gsc, i == 0 ? skip : nullptr, hw))) return rc;
        gy = d0;
    }
    return E3DGE_OK;
}

}  // namespace e3dge
