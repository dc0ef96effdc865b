// The 2-D residual aligner (ADA): the network.  One table (aln_net) holds everything about its shape -- per unit the channels, sizes, the
// place of every tensor in the source list, the packed image, the transposed image and the BatchNorm channels; per stage its inputs; per
// feature its shape -- and every layout (packed images, gradient buffer, saved state, both workspaces) and every walk (forward in both
// forms, backward) reads it.  Composed of aln_conv_kernel and the kernels of aligner_bwd.h.  Included by aligner.hip after them.
//
// The forward is walked once (aln_forward), in one of two forms that differ in what a layer launches (AlnFwd::layer) and in where a unit's
// buffers live (AlnFwd::bufs).  Fused form (the plain forward): one aln_conv launch per layer, BatchNorm on its running statistics, PReLU
// and shortcut in its epilogue, on the reused slots of AlnWs.  Saving form (the trainable forward, on running or on batch statistics): every
// convolution runs with no trailing affine and writes its raw sums (c0; per unit c1, c2 and the 1x1 branch csc), which are what the backward
// of the BatchNorms and the PReLU branch need; aln_bn_apply_kernel then does the epilogue's own arithmetic (a v + b, PReLU, shortcut), so on
// running statistics the output is the fused form's bit for bit.  On batch statistics aln_bn_stats_kernel runs between the two and writes the
// (a, b) pair the apply step (trailing and shortcut BatchNorms, the stem's) or the next gather (leading BatchNorm: in_ab, padded taps stay
// 0) reads.
//
// Backward of a unit, from the gradient gy of its output: the trailing BatchNorm (aln_norm_*), the second convolution's weight and data
// gradient, the PReLU, the first convolution's weight and data gradient, the shortcut (1x1 branch: its BatchNorm, weight and data gradient;
// pick: gy itself -- every such unit has stride 1), and last the leading BatchNorm, whose kernel adds the shortcut's gradient
// and, at a stage's first unit, the skip connection's: every fan-in sum is an addend of that step.  The gradient of a concatenated input is
// written split (AlnDst2): the up-sampled part goes to aln_up2_bwd_kernel, the skip part waits as that addend.
#pragma once

namespace e3dge {

// ---- the network's shape: kAlnUnit (aligner.hip) and the stages here are the only statements of it on this side ----------------------------
// Feature t is the stem's output (0) or stage t - 1's.  Stage s is three units on feature s, or on cat(up2(feature s), feature `skip`).
struct AlnStage { bool up; int skip; };
constexpr int kAlnStages = kAlnUnits / 3, kAlnUps = 3;
constexpr AlnStage kAlnStage[kAlnStages] = {{false, -1}, {false, -1}, {false, -1}, {true, 2}, {true, 1}, {true, 0}};

struct AlnBn { int src, ch, chan; int64_t packed; };                 // gamma's index in the source list (beta, mean, var follow); channels; the first
                                                                     // of them among all BatchNorm channels; the (a, b) pairs in the packed image
struct AlnWeight { int src; int64_t packed, packed_t; };             // index in the source list; the A-fragment image; the transposed image
struct AlnSlope { int src; int64_t packed; };
struct AlnUnitRow { int cin, depth, stride, size, osize; bool conv_sc; AlnBn bn0, bn4, bnsc; AlnWeight w1, w2, wsc; AlnSlope prelu; };
struct AlnStageRow { int u0, size, split, up, skip; };               // split: in0's channels; up: which up-sampled map in0 is (-1: feature s itself)
struct AlnFeature { int ch, size; bool skip; };                      // skip: a later stage reads it beside its up-sampled input
struct AlnNet {
    AlnWeight stem_w; AlnBn stem_bn; AlnSlope stem_prelu;
    AlnUnitRow u[kAlnUnits];
    AlnStageRow stage[kAlnStages];
    AlnFeature feature[kAlnTaps];
    int64_t goff[kAlnSources + 1];                                   // offset of every source tensor's gradient in the gradient buffer
    int64_t packed_total, packed_t_total;
    int channels, sources;                                           // BatchNorm channels, source tensors in all
    // the widest of each kind of buffer that the walks reuse, in floats per image
    struct { int64_t t1, c2, sc, y, up, gy, gxn, gsc; int bn; } peak;
    bool fits;                                                       // every stage's first unit takes what its inputs have
};

constexpr int64_t aln_up64(int64_t floats) { return (floats + 63) / 64 * 64; }   // every block of every layout starts on a multiple of 64 floats
constexpr int64_t aln_image_floats(int cin, int cout, int ks) { return (int64_t)ig_mpad(cout) * ig_kpad(cin * ks * ks); }
constexpr int64_t aln_image_t_floats(int cin, int cout, int ks) { return (int64_t)ig_mpad(cin) * ig_kpad(cout * ks * ks); }

// The source list, the packed image and the transposed image all run in the module's order: conv_layer1 (weight, BatchNorm, PReLU), then
// per unit res_layer.0 .. .4 and the shortcut.
struct AlnNetBuilder {
    AlnNet t{};
    int64_t poff = 0, toff = 0, goff = 0;
    constexpr int source(int64_t numel) { t.goff[t.sources] = goff; goff += numel; return t.sources++; }
    constexpr int64_t take(int64_t& off, int64_t floats) { const int64_t at = off; off += aln_up64(floats); return at; }
    constexpr AlnWeight weight(int cin, int cout, int ks) {
        return {source((int64_t)cout * cin * ks * ks), take(poff, aln_image_floats(cin, cout, ks)), take(toff, aln_image_t_floats(cin, cout, ks))};
    }
    constexpr AlnBn bn(int ch) {
        const AlnBn b{source(ch), ch, t.channels, take(poff, 2 * ch)};
        source(ch); source(ch); source(ch);
        t.channels += ch;
        t.peak.bn = ch > t.peak.bn ? ch : t.peak.bn;
        return b;
    }
    constexpr AlnSlope slope(int ch) { return {source(ch), take(poff, ch)}; }
    static constexpr void widen(int64_t& peak, int64_t v) { peak = v > peak ? v : peak; }
    constexpr AlnNet build() {
        t.stem_w = weight(kAlnIn, kAlnStem, 3); t.stem_bn = bn(kAlnStem); t.stem_prelu = slope(kAlnStem);
        t.feature[0] = {kAlnStem, kAlnSize, false};
        t.peak.c2 = (int64_t)kAlnStem * kAlnSize * kAlnSize;
        t.fits = true;
        for (int s = 0, ups = 0; s < kAlnStages; ++s) {
            const AlnFeature in = t.feature[s];
            AlnStageRow& g = t.stage[s];
            g = {3 * s, kAlnStage[s].up ? 2 * in.size : in.size, in.ch, kAlnStage[s].up ? ups++ : -1, kAlnStage[s].skip};
            if (g.up >= 0) widen(t.peak.up, (int64_t)g.split * g.size * g.size);
            t.fits = t.fits && kAlnUnit[g.u0].cin == g.split + (g.skip >= 0 ? t.feature[g.skip].ch : 0) &&
                     (g.skip < 0 || (g.skip < kAlnUps && t.feature[g.skip].size == g.size));
            if (g.skip >= 0) t.feature[g.skip].skip = true;
            int size = g.size;
            for (int u = g.u0; u < g.u0 + 3; ++u) {
                AlnUnitRow& q = t.u[u];
                q.cin = kAlnUnit[u].cin; q.depth = kAlnUnit[u].depth; q.stride = kAlnUnit[u].stride;
                q.size = size; q.osize = size = aln_out_size(size, 3, q.stride);
                q.conv_sc = q.cin != q.depth;
                q.bn0 = bn(q.cin); q.w1 = weight(q.cin, q.depth, 3); q.prelu = slope(q.depth); q.w2 = weight(q.depth, q.depth, 3); q.bn4 = bn(q.depth);
                q.wsc.src = -1;
                if (q.conv_sc) { q.wsc = weight(q.cin, q.depth, 1); q.bnsc = bn(q.depth); }
                t.fits = t.fits && (u == g.u0 || q.cin == t.u[u - 1].depth);
                const int64_t in_px = (int64_t)q.size * q.size, out_px = (int64_t)q.osize * q.osize;
                widen(t.peak.t1, q.depth * in_px);
                widen(t.peak.c2, q.depth * out_px);
                widen(t.peak.gxn, q.cin * in_px);
                if (q.conv_sc) { widen(t.peak.sc, q.depth * out_px); widen(t.peak.gsc, q.cin * in_px); }
                if (u < g.u0 + 2) widen(t.peak.y, q.depth * out_px);
                if (u > g.u0) widen(t.peak.gy, q.cin * in_px);
            }
            t.feature[s + 1] = {t.u[g.u0 + 2].depth, size, false};
        }
        t.goff[t.sources] = goff;
        t.packed_total = poff; t.packed_t_total = toff;
        return t;
    }
};

constexpr AlnNet kAlnNet = AlnNetBuilder{}.build();
static const AlnNet& aln_net() { return kAlnNet; }
static_assert(kAlnNet.sources == kAlnSources && kAlnNet.fits, "the unit and stage tables disagree with each other or with E3DGE_ALIGNER_SOURCES");
static_assert(kAlnNet.feature[kAlnTaps - 1].size == kAlnSize && kAlnNet.stage[kAlnStages - 1].up == kAlnUps - 1, "the output is the input's size");

// Every unit that keeps its channel count has stride 1, so its shortcut's adjoint is the identity and aln_pick_bwd_kernel has no launch here.
constexpr bool aln_identity_units_have_stride_1() {
    for (int u = 0; u < kAlnUnits; ++u)
        if (kAlnUnit[u].cin == kAlnUnit[u].depth && kAlnUnit[u].stride != 1) return false;
    return true;
}
static_assert(aln_identity_units_have_stride_1(), "a strided identity shortcut needs aln_pick_bwd_kernel in aln_stage_bwd");

static int64_t aln_feature_floats(int t) { const AlnFeature f = aln_net().feature[t]; return (int64_t)f.ch * f.size * f.size; }   // per image

// A layout: blocks taken one after the other, each rounded up to 64 floats
struct AlnTake {
    int64_t off = 0;
    int64_t operator()(int64_t floats) { const int64_t at = off; off += aln_up64(floats); return at; }
    int64_t bytes() const { return off * (int64_t)sizeof(float); }
};

// ---- workspace of the fused forward ----------------------------------------------------------------------------------------------------------
struct AlnWs { int64_t feature[kAlnTaps - 1], t1, sc, x[2], up, total_bytes; };

static bool aln_ws(int64_t n, AlnWs* d) {
    if (n < 1 || n > 256) return false;
    const AlnNet& net = aln_net();
    AlnTake take;
    for (int t = 0; t < kAlnTaps - 1; ++t) d->feature[t] = take(n * aln_feature_floats(t));
    d->t1 = take(n * net.peak.t1);                                   // a unit's first convolution: depth channels at the input's size
    d->sc = take(n * net.peak.sc);                                   // the 1x1 branch
    d->x[0] = take(n * net.peak.y); d->x[1] = take(n * net.peak.y);  // unit outputs inside a stage
    d->up = take(n * net.peak.up);                                   // an up-sampled map
    d->total_bytes = take.bytes();
    return true;
}

// ---- saved state (floats; per image unless said) -------------------------------------------------------------------------------------------
struct AlnSaved {
    int64_t c0, feat1, c1[kAlnUnits], t1[kAlnUnits], c2[kAlnUnits], csc[kAlnUnits], y[kAlnUnits], up[kAlnUps], ab, part, total_bytes;
    int64_t feature(int t) const { return t ? y[3 * t - 1] : feat1; }   // (the last one, the output, is the caller's)
};

static bool aln_saved(int64_t n, AlnSaved* d) {
    if (n < 1 || n > 256) return false;
    const AlnNet& net = aln_net();
    AlnTake take;
    d->c0 = take(n * aln_feature_floats(0)); d->feat1 = take(n * aln_feature_floats(0));
    for (int u = 0; u < kAlnUnits; ++u) {
        const AlnUnitRow& q = net.u[u];
        const int64_t in = n * q.depth * q.size * q.size, out = n * q.depth * q.osize * q.osize;
        d->c1[u] = take(in); d->t1[u] = take(in); d->c2[u] = take(out);
        d->csc[u] = q.conv_sc ? take(out) : -1;
        d->y[u] = u + 1 < kAlnUnits ? take(out) : -1;                 // the last unit writes the output
    }
    for (const AlnStageRow& g : net.stage)
        if (g.up >= 0) d->up[g.up] = take(n * g.split * g.size * g.size);
    d->ab = take(2 * net.channels);                                  // per call: the (a, b) pairs of the batch statistics
    d->part = take(2 * (aln_norm_ws_bytes(n, net.peak.bn, kAlnSize * kAlnSize) / (int64_t)sizeof(double)));   // per call: the statistics' partial sums
    d->total_bytes = take.bytes();
    return true;
}

// ---- backward workspace (floats) -----------------------------------------------------------------------------------------------------------
struct AlnBwdWs { int64_t gy[2], gstage, gc2, gt1, gxn, gsc, gcsc, skip[kAlnUps], gup, d256, wg, norm, total_bytes; };

static bool aln_bwd_ws(int64_t n, AlnBwdWs* d) {
    if (n < 1 || n > 256) return false;
    const AlnNet& net = aln_net();
    AlnTake take;
    d->gy[0] = take(n * net.peak.gy); d->gy[1] = take(n * net.peak.gy);   // a unit's output gradient and its input gradient, alternating
    d->gstage = take(n * aln_feature_floats(0));                     // a stage's output gradient, then its input's
    d->gc2 = take(n * net.peak.c2);                                  // a trailing BatchNorm's input gradient, the stem's among them
    d->gt1 = take(n * net.peak.t1); d->gxn = take(n * net.peak.gxn); d->gsc = take(n * net.peak.gsc); d->gcsc = take(n * net.peak.sc);
    for (int t = 0; t < kAlnUps; ++t) d->skip[t] = take(n * aln_feature_floats(t));
    d->gup = take(n * net.peak.up); d->d256 = take(n * kAlnIn * kAlnSize * kAlnSize);
    int64_t wg = aln_wgrad_ws_floats(n, kAlnIn, kAlnStem, kAlnSize, kAlnSize, 3, 1);
    for (const AlnUnitRow& q : net.u) {
        const int64_t a = aln_wgrad_ws_floats(n, q.cin, q.depth, q.size, q.size, 3, 1), b = aln_wgrad_ws_floats(n, q.depth, q.depth, q.size, q.size, 3, q.stride);
        wg = a > wg ? a : wg;
        wg = b > wg ? b : wg;
    }
    d->wg = take(wg);
    d->norm = take(2 * (aln_norm_ws_bytes(n, net.peak.bn, kAlnSize * kAlnSize) / (int64_t)sizeof(double)));
    d->total_bytes = take.bytes();
    return true;
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

// ---- the forward walk ----------------------------------------------------------------------------------------------------------------------------
struct AlnUnitBufs { float* c1; float* t1; float* c2; float* sc; float* csc; float* y; };   // raw sums c1, c2, csc: the saving form's; sc: the fused form's
struct AlnLayer { const AlnBn* pre; const AlnBn* post; const float* slope; const float* sc; const AlnBn* sc_bn; };   // leading / trailing BatchNorm, PReLU, shortcut

struct AlnFwd {
    int n, train;                                                    // train: BatchNorm on batch statistics (the saving form alone)
    const float* P; const float* const* src; double* stats; hipStream_t st;
    float* S; AlnSaved lay;                                          // the saving form's state (S NULL: the fused form, lay unset)
    float* W; AlnWs ws;                                              // the fused form's workspace
    float* feature[kAlnTaps];                                        // where the stem and the stages write

    const float* ab(const AlnBn& b) const { return train ? S + lay.ab + 2 * b.chan : P + b.packed; }
    int batch_stats(const AlnBn& b, const float* in0, const float* in1, int split, int hw) const {
        if (!train) return E3DGE_OK;
        return aln_stats(S + lay.ab + 2 * b.chan, stats + 2 * b.chan, reinterpret_cast<double*>(S + lay.part), in0, in1, src[b.src], src[b.src + 1], n, b.ch, split,
                         hw, st);
    }
    float* up(int k) const { return S ? S + lay.up[k] : W + ws.up; }
    AlnUnitBufs bufs(int u) const {
        float* y = u % 3 == 2 ? feature[u / 3 + 1] : S ? S + lay.y[u] : W + ws.x[u % 3];
        if (!S) return {nullptr, W + ws.t1, nullptr, W + ws.sc, nullptr, y};
        return {S + lay.c1[u], S + lay.t1[u], S + lay.c2[u], nullptr, lay.csc[u] >= 0 ? S + lay.csc[u] : nullptr, y};
    }
    // One layer: the convolution c (its source, image and shape; the rest is filled in here) under e.  Fused: one launch to `out`.  Saving: the
    // raw sums to `raw`, the batch statistics of the BatchNorms, then the apply step to `out` (NULL: the 1x1 branch stays raw; the apply step
    // of the unit's last layer reads it under its affine).
    int layer(float* out, float* raw, AlnConv c, const AlnLayer& e) const {
        const int mode = !e.sc ? kAlnScNone : !e.sc_bn ? kAlnScPick : S ? kAlnScAffine : kAlnScRead;
        c.in_ab = e.pre ? ab(*e.pre) : nullptr;
        if (!S) {
            c.out = out; c.epi_ab = e.post ? ab(*e.post) : nullptr; c.slope = e.slope; c.sc = e.sc; c.sc_mode = mode;
            return aln_conv(c, st);
        }
        int rc;
        const int oh = aln_out_size(c.h, c.ks, c.stride), ow = aln_out_size(c.w, c.ks, c.stride);
        const bool pick = mode == kAlnScPick;
        if (e.pre && (rc = batch_stats(*e.pre, c.in0, c.in1, c.split, c.h * c.w))) return rc;
        c.out = raw;
        if ((rc = aln_conv(c, st))) return rc;
        if (e.post && (rc = batch_stats(*e.post, raw, nullptr, c.cout, oh * ow))) return rc;
        if (!out) return E3DGE_OK;
        return aln_apply(out, raw, e.post ? ab(*e.post) : nullptr, e.slope, e.sc, e.sc_bn ? ab(*e.sc_bn) : nullptr, n, c.cout, oh, ow, pick ? c.h : oh,
                         pick ? c.w : ow, pick ? c.stride : 1, mode, st);
    }
    int unit(const AlnUnitRow& q, const AlnUnitBufs& b, const float* in0, const float* in1, int split) const {
        const AlnConv x{nullptr, in0, in1, nullptr, nullptr, nullptr, nullptr, nullptr, n, q.cin, split, 0, q.depth, q.size, q.size, 3, 1, kAlnScNone};
        int rc;
        if (q.conv_sc) {                                             // independent of the two 3x3 convolutions; first, so that the last layer can read it
            AlnConv c = x;
            c.wfrag = P + q.wsc.packed; c.ks = 1; c.stride = q.stride;
            if ((rc = layer(b.sc, b.csc, c, {nullptr, &q.bnsc, nullptr, nullptr, nullptr}))) return rc;
        }
        AlnConv c1 = x;
        c1.wfrag = P + q.w1.packed;
        if ((rc = layer(b.t1, b.c1, c1, {&q.bn0, nullptr, P + q.prelu.packed, nullptr, nullptr}))) return rc;
        AlnConv c2 = x;
        c2.in0 = b.t1; c2.in1 = nullptr; c2.wfrag = P + q.w2.packed; c2.cin = c2.split = q.depth; c2.stride = q.stride;
        if (q.conv_sc) return layer(b.y, b.c2, c2, {nullptr, &q.bn4, nullptr, b.sc ? b.sc : b.csc, &q.bnsc});
        return layer(b.y, b.c2, c2, {nullptr, &q.bn4, nullptr, in0, nullptr});   // MaxPool2d(1, stride) of the unit's input
    }
};

// stem -> stages (each on the last feature, or on cat(up2 of it, an earlier one)) -> the taps the caller wants and the walk did not write in place
static int aln_forward(const AlnFwd& r, const float* res_gt, const float* thumb, int split, int thumb_up4, float* const* taps, const char* tap_launch) {
    const AlnNet& net = aln_net();
    const int n = r.n;
    int rc;
    if ((rc = r.layer(r.feature[0], r.S ? r.S + r.lay.c0 : nullptr,
                      {nullptr, res_gt, thumb, r.P + net.stem_w.packed, nullptr, nullptr, nullptr, nullptr, n, kAlnIn, split, thumb_up4, kAlnStem, kAlnSize, kAlnSize, 3,
                       1, kAlnScNone},
                      {nullptr, &net.stem_bn, r.P + net.stem_prelu.packed, nullptr, nullptr})))
        return rc;
    for (int s = 0; s < kAlnStages; ++s) {
        const AlnStageRow& g = net.stage[s];
        const float* in0 = r.feature[s];
        const float* in1 = nullptr;
        if (g.up >= 0) {
            if ((rc = aln_up2(r.up(g.up), in0, (int64_t)n * g.split, g.size / 2, g.size / 2, r.st))) return rc;
            in0 = r.up(g.up); in1 = r.feature[g.skip];
        }
        int c0 = g.split;
        for (int u = g.u0; u < g.u0 + 3; ++u) {
            const AlnUnitBufs b = r.bufs(u);
            if ((rc = r.unit(net.u[u], b, in0, in1, c0))) return rc;
            in0 = b.y; in1 = nullptr; c0 = net.u[u].depth;
        }
    }
    bool copied = false;
    for (int t = 0; t < kAlnTaps; ++t)
        if (taps[t] && taps[t] != r.feature[t]) { ig_copy(taps[t], r.feature[t], n * aln_feature_floats(t), 1.0f, 0, r.st); copied = true; }
    return copied ? check_launch(tap_launch) : E3DGE_OK;
}

// ---- the backward walk ----------------------------------------------------------------------------------------------------------------------------
struct AlnBwdRun {
    int n, train, want_input;
    const float* P; const float* T; const float* const* src; const uint8_t* want; const float* S; AlnSaved lay; const double* stats;
    float* W; AlnBwdWs ws; float* grads; hipStream_t st;
    float* grad(int s) const { return want[s] ? grads + aln_net().goff[s] : nullptr; }
    const float* ab(const AlnBn& b) const { return train ? S + lay.ab + 2 * b.chan : P + b.packed; }
    double* norm_ws() const { return reinterpret_cast<double*>(W + ws.norm); }
    int norm_bwd(const AlnBn& b, float* gx0, float* gx1, int gsplit, const float* gy, const float* in0, const float* in1, int split, const float* add0,
                 const float* add1, int hw) const {
        return aln_norm_bwd(gx0, gx1, gsplit, grad(b.src), grad(b.src + 1), gy, in0, in1, split, src[b.src], train ? stats + 2 * b.chan : nullptr, src[b.src + 2], src[b.src + 3],
                            add0, add1, norm_ws(), n, b.ch, hw, train, st);
    }
};

// Stage g backwards.  gy_in: the gradient of the stage's output (consumed).  The stage's input (in0 | in1 at channel g.split) gets its
// gradient at gx0 (and gx1 from that channel on), plus `skip` (what the stage's input receives from its skip connection; may be NULL).
static int aln_stage_bwd(const AlnBwdRun& r, const AlnStageRow& g, float* gx0, float* gx1, const float* gy_in, const float* in0, const float* in1,
                         const float* skip) {
    const AlnNet& net = aln_net();
    int rc;
    const float* gy = gy_in;
    for (int i = 2; i >= 0; --i) {
        const int u = g.u0 + i, n = r.n;
        const AlnUnitRow& q = net.u[u];
        const int size = q.size, hw = size * size, ohw = q.osize * q.osize;
        const float* x0 = i == 0 ? in0 : r.S + r.lay.y[u - 1];       // the unit's input
        const float* x1 = i == 0 ? in1 : nullptr;
        const int xs = i == 0 ? g.split : q.cin;
        const float* c1 = r.S + r.lay.c1[u];
        const float* t1 = r.S + r.lay.t1[u];
        const float* c2 = r.S + r.lay.c2[u];
        float* gc2 = r.W + r.ws.gc2;
        float* gt1 = r.W + r.ws.gt1;
        float* gxn = r.W + r.ws.gxn;
        float* wg = r.W + r.ws.wg;
        // res_layer.4, .3
        if ((rc = r.norm_bwd(q.bn4, gc2, nullptr, 0, gy, c2, nullptr, q.depth, nullptr, nullptr, ohw))) return rc;
        if (r.want[q.w2.src] && (rc = aln_wgrad({r.grad(q.w2.src), gc2, t1, nullptr, nullptr, wg, n, q.depth, q.depth, 0, q.depth, size, size, 3, q.stride}, r.st)))
            return rc;
        if ((rc = aln_dgrad({gt1, gc2, r.T + q.w2.packed_t, nullptr, nullptr, n, q.depth, q.depth, size, size, 3, q.stride}, r.st))) return rc;
        // res_layer.2 (in place), .1
        if ((rc = aln_prelu_bwd(gt1, r.grad(q.prelu.src), gt1, c1, nullptr, r.src[q.prelu.src], r.norm_ws(), n, q.depth, hw, r.st))) return rc;
        if (r.want[q.w1.src] && (rc = aln_wgrad({r.grad(q.w1.src), gt1, x0, x1, r.ab(q.bn0), wg, n, q.cin, xs, 0, q.depth, size, size, 3, 1}, r.st))) return rc;
        if ((rc = aln_dgrad({gxn, gt1, r.T + q.w1.packed_t, nullptr, nullptr, n, q.cin, q.depth, size, size, 3, 1}, r.st))) return rc;
        // the shortcut
        const float* gsc = gy;                                       // MaxPool2d(1, 1): the identity (aln_identity_units_have_stride_1)
        if (q.conv_sc) {
            float* gcsc = r.W + r.ws.gcsc;
            if ((rc = r.norm_bwd(q.bnsc, gcsc, nullptr, 0, gy, r.S + r.lay.csc[u], nullptr, q.depth, nullptr, nullptr, ohw))) return rc;
            if (r.want[q.wsc.src] && (rc = aln_wgrad({r.grad(q.wsc.src), gcsc, x0, x1, nullptr, wg, n, q.cin, xs, 0, q.depth, size, size, 1, q.stride}, r.st)))
                return rc;
            if ((rc = aln_dgrad({r.W + r.ws.gsc, gcsc, r.T + q.wsc.packed_t, nullptr, nullptr, n, q.cin, q.depth, size, size, 1, q.stride}, r.st))) return rc;
            gsc = r.W + r.ws.gsc;
        }
        // res_layer.0: the unit's input gradient, with the shortcut's and (first unit) the skip connection's as addends
        float* d0 = i == 0 ? gx0 : r.W + r.ws.gy[i & 1];
        float* d1 = i == 0 ? gx1 : nullptr;
        if ((rc = r.norm_bwd(q.bn0, d0, d1, xs, gxn, x0, x1, xs, gsc, i == 0 ? skip : nullptr, hw))) return rc;
        gy = d0;
    }
    return E3DGE_OK;
}

// The stages in reverse, from g_out to the gradient of feature 0 in ws.gstage.  A stage on cat(up2(feature s), feature k) writes the first
// part to ws.gup, which aln_up2_bwd takes to ws.gstage, and the second to ws.skip[k], which waits as the addend of the stage on feature k.
static int aln_stages_bwd(const AlnBwdRun& r, const float* g_out) {
    const AlnNet& net = aln_net();
    float* gstage = r.W + r.ws.gstage;
    float* gup = r.W + r.ws.gup;
    int rc;
    for (int s = kAlnStages - 1; s >= 0; --s) {
        const AlnStageRow& g = net.stage[s];
        const float* gy = s == kAlnStages - 1 ? g_out : gstage;
        const float* in = r.S + r.lay.feature(s);
        if (g.up >= 0) {
            if ((rc = aln_stage_bwd(r, g, gup, r.W + r.ws.skip[g.skip], gy, r.S + r.lay.up[g.up], r.S + r.lay.feature(g.skip), nullptr))) return rc;
            if ((rc = aln_up2_bwd(gstage, gup, (int64_t)r.n * g.split, g.size / 2, g.size / 2, r.st))) return rc;
        } else if ((rc = aln_stage_bwd(r, g, gstage, nullptr, gy, in, nullptr, net.feature[s].skip ? r.W + r.ws.skip[s] : nullptr))) {
            return rc;
        }
    }
    return E3DGE_OK;
}

}  // namespace e3dge
