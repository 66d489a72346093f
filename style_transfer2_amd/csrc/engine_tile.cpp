// Tile-sharded single image (BASELINE config 5): the phases of one iteration on one rank's window.
#include "engine.h"

// ---- tile-sharded single image (style_transfer2_amd/tiling.py has the design) ----------------------------------
// This context runs the window (tile + apron) of one rank.  Every reduction is restricted to the tile's region
// of each blob and left UN-normalised in a flat device buffer that the caller all-reduces (RCCL) between phases.
namespace st2e {
// blob b of a gH x gW image: every pool below it halves the size (Caffe ceil mode) and doubles the stride
BlobSize blob_size(const st_ctx* c, int b, int gH, int gW)
{
    int s = 1, gh = gH, gw = gW;
    for (int i = 1; i <= b; ++i)
        if (!c->topo[i - 1].is_conv) { gh = pooled_size(gh); gw = pooled_size(gw); s *= 2; }
    return BlobSize{gh, gw, s, (double)c->blob_c_topo(b) * gh * gw};
}

// the tile's region in blob b of the activation set `a` that holds the window (geometry `t`: the iterate's c->tile, or the style
// image's of st_tile_style_partials)
BlobRoi tile_roi(const st_ctx* c, const ActSet& a, const TileGeom& t, int b)
{
    const BlobSize g = blob_size(c, b, t.gH, t.gW);
    const int s = g.stride;
    BlobRoi r;
    r.y0 = (t.ty0 - t.wy0) / s; r.x0 = (t.tx0 - t.wx0) / s;
    r.y1 = t.ty1 == t.gH ? a.h[b] : (t.ty1 - t.wy0) / s;
    r.x1 = t.tx1 == t.gW ? a.w[b] : (t.tx1 - t.wx0) / s;
    r.n_global = g.n;
    return r;
}

// D = Graw / n_global - G_style into dbuf ([C][MPad]); sum D^2 -> pd[k]
int tile_style_D(st_ctx* c, int b, const float* graw, double n_global, float* pd_slot)
{
    const ActSet& a = c->act;
    const int C = a.C[b];
    ST_TRY(ensure_layer_part(c, b));
    float* part = c->layer_part[b] + 4 * kMaxPartials;
    int np = 0;
    GramPlan one{}; one.splits = 1;
    HIP_TRY(launch_gram_reduce(graw, nullptr, c->style_gram[b], c->dbuf, conv_mpad(C), part, &np, C, n_global, one, c->stream));
    HIP_TRY(launch_sum_partials(part, np, pd_slot, c->stream));
    return ST_OK;
}

// the phases called one by one return with their work done; inside st_tile_step they only enqueue
static int tile_sync(st_ctx* c)
{
    if (!c->tile.fused) HIP_TRY(hipStreamSynchronize(c->stream));
    return ST_OK;
}

// what every phase starts with: the configured context on its device and the layout of the objective (the preflight with it)
static int tile_begin(st_ctx* c, ObjTerms& terms)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c || !c->tile.on) return fail(ST_ERR_STATE, "st_tile_configure first");
    HIP_TRY(hipSetDevice(c->device));
    ST_TRY(act_ensure(c, c->act, c->H, c->W));
    return objective_terms(c, c->act, &c->tile, terms);
}

// phase 4, both forms.  adam: TV + p-norm + combine + Adam on the tile into x[cur ^ 1]; else the combined gradient of the tile's pixels
// into c->grad (window layout).  The 6 image sums go to p3[0..6) (p3[6..) already holds this rank's sum S^2 per style layer in steady state).
static int tile_image_pass(st_ctx* c, const float* ring_dev, bool adam, float** dev_ptr, int* n_floats)
{
    HIP_TRY(hipSetDevice(c->device));
    ObjTerms terms;
    ST_TRY(objective_terms(c, c->act, &c->tile, terms));
    const st_ctx::Tile& t = c->tile;
    ST_TRY(c->tile.p3.reserve(6 + kMaxTraceLayers));
    if (adam) { c->items1 += 1; c->items2 += 1; }
    ImageTileArgs ta{};
    ta.base = image_pass_args(c, c->x[c->cur], c->tile.wgrad, adam ? nullptr : c->grad.get(), adam, c->x[c->cur ^ 1]);
    ta.ring = ring_dev; ta.ty = t.ty0 - t.wy0; ta.tx = t.tx0 - t.wx0; ta.th = t.ty1 - t.ty0; ta.tw = t.tx1 - t.tx0;
    // the untouched apron of x_next is refreshed by the caller; start it from the current values
    if (adam) HIP_TRY(hipMemcpyAsync(c->x[c->cur ^ 1], c->x[c->cur], (size_t)3 * c->H * c->W * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    int np = 0;
    HIP_TRY(launch_image_pass_tile(ta, &np, c->stream));
    for (int k = 0; k < 6; ++k) HIP_TRY(launch_sum_partials(c->image_part + k * kMaxPartials, np, c->tile.p3 + k, c->stream));
    if (adam) c->m_zero = c->v_zero = false;
    ST_TRY(tile_sync(c));
    c->tile.evaluated = true;
    if (dev_ptr) *dev_ptr = c->tile.p3;
    if (n_floats) *n_floats = 6 + (c->tile.s2_in_p2 ? 0 : terms.n_style);
    return ST_OK;
}

// Pack (mode 0) the rectangles `rects` (y0, x0, h, w each) of the (C, h, w) device tensor into the contiguous buffer `buf`, or unpack
// them from it (1 assign, 2 add), at most kMaxStripRects per launch: the one place that fills a StripTable and holds the rectangles
// to the tensor.  Enqueues only.
int strips(st_ctx* c, float* tensor, int C, int h, int w, const std::vector<int>& rects, float* buf, int mode)
{
    const int n = (int)rects.size() / 4;
    size_t off = 0;
    for (int r0 = 0; r0 < n; r0 += kMaxStripRects) {
        StripTable t{};
        t.n = std::min(kMaxStripRects, n - r0);
        int total = 0;
        for (int r = 0; r < t.n; ++r) {
            const int* q = &rects[4 * (r0 + r)];
            t.y0[r] = q[0]; t.x0[r] = q[1]; t.h[r] = q[2]; t.w[r] = q[3];
            if (q[0] < 0 || q[1] < 0 || q[2] <= 0 || q[3] <= 0 || q[0] + q[2] > h || q[1] + q[3] > w)
                return fail(ST_ERR_ARG, "strip %d lies outside the %dx%d tensor", r0 + r, h, w);
            t.off[r] = total;
            total += C * q[2] * q[3];
        }
        t.total = total;
        HIP_TRY(launch_strip_copy(tensor, buf + off, t, C, h, w, mode, c->stream));
        off += (size_t)total;
    }
    return ST_OK;
}
}  // namespace st2e

extern "C" {

int st_tile_configure(st_ctx* c, int gH, int gW, int wy0, int wx0, int ty0, int tx0, int ty1, int tx1)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (c)
        for (const Layer& L : c->topo)
            if (L.ave) return fail(ST_ERR_ARG, "tile-sharded mode does not run average pools (layer %s); use a single-context job", L.name.c_str());
    if (!c || !c->x[0]) return fail(ST_ERR_STATE, "set the window image first (st_set_input)");
    if (c->lap.n) return fail(ST_ERR_STATE, "tile-sharded mode does not run the Laplacian term: st_set_laplacian(ctx, 0, NULL, NULL) first, or use a single-context job");
    if (c->anchor.on) return fail(ST_ERR_STATE, "tile-sharded mode does not run the anchor term: st_set_anchor(ctx, NULL, ...) first, or use a single-context job");
    if (c->mat.on) return fail(ST_ERR_STATE, "tile-sharded mode does not run the photorealism term: st_set_matting(ctx, 0, ...) first, or use a single-context job");
    if (c->jit.on) return fail(ST_ERR_STATE, "tile-sharded mode does not run jitter: st_set_jitter(ctx, 0, 0) first, or use a single-context job");
    if (c->tap.blob >= 0) return fail(ST_ERR_STATE, "tile-sharded mode does not run the diff tap: st_tap_diff(ctx, -1) first");
    if (wy0 < 0 || wx0 < 0 || wy0 + c->H > gH || wx0 + c->W > gW || ty0 < wy0 || tx0 < wx0 ||
        ty1 > wy0 + c->H || tx1 > wx0 + c->W || ty1 <= ty0 || tx1 <= tx0)
        return fail(ST_ERR_ARG, "tile/window geometry is inconsistent with the %dx%d window", c->H, c->W);
    st_ctx::Tile& t = c->tile;
    t.on = true; t.gH = gH; t.gW = gW; t.wy0 = wy0; t.wx0 = wx0; t.ty0 = ty0; t.tx0 = tx0; t.ty1 = ty1; t.tx1 = tx1;
    t.evaluated = false;
    return ST_OK;
}

// phase 1: forward on the window, region sums [d2, gc2, F2, gd2] per active layer and the RAW Gram sums
int st_tile_forward(st_ctx* c, float** dev_ptr, int* n_floats)
{
    ObjTerms terms;
    ST_TRY(tile_begin(c, terms));
    ActSet& a = c->act;
    c->tile.evaluated = false;
    c->lt.begin(c->nb);
    ST_TRY(ensure_content_features(c));
    ST_TRY(c->tile.p1.reserve(std::max<size_t>(terms.n1, 1)));
    HIP_TRY(hipMemsetAsync(c->tile.p1, 0, std::max<size_t>(terms.n1, 1) * sizeof(float), c->stream));
    // bf16 operands: the lean data flow here too -- an fp32 blob / diff is written only where something reads fp32 (the weighted
    // blobs: the region-of-interest loss kernels are fp32), pools ride on their producing conv, the backward masks from the bf16 copies
    // fp32, inside the fused iteration (st_tile_step): the full-resolution blobs of pooled, un-weighted layers are not written either
    bool lean32 = false;
    if (!c->bf16 && c->tile.fused) lean32 = lean32_enabled();
    ST_TRY(forward_range(c, a, c->x[c->cur], std::max(terms.last, 0), (c->bf16 && c->lean) || lean32));
    for (const ObjTerm& t : terms.t) {
        ST_TRY(ensure_layer_part(c, t.b));
        float* part = c->layer_part[t.b];
        if (t.al.c || t.al.d) {
            int np = 0;
            HIP_TRY(launch_layer_elem(layer_elem_args(c, t.al, t.n_norm, 0, part, t.region()), &np, c->stream));
            for (int k = 0; k < 4; ++k) HIP_TRY(launch_sum_partials(part + k * kMaxPartials, np, c->tile.p1 + t.sums + k, c->stream));
        }
        // raw sum over this rank's region (divisor 1, no target), contiguous C x C; bf16 operands: from the blob's bf16 copy
        if (t.al.s) ST_TRY(style_gram(c, a, style_term(c, a, t.b, t.region()), nullptr, c->tile.p1 + t.gram, t.C, 1.0, nullptr, nullptr));
    }
    if (dev_ptr) *dev_ptr = c->tile.p1;
    if (n_floats) *n_floats = (int)terms.n1;
    return ST_OK;
}

// phase 2a: after the all-reduce of p1.  Captures missing content / deep-dream norms.  If a style norm is still
// missing (first evaluation after reset) it returns the p2 buffer (n > 0): the caller then runs st_tile_style_raw,
// all-reduces p2 and only then calls st_tile_losses_finish.
int st_tile_losses(st_ctx* c, float** dev_ptr, int* n_floats)
{
    ObjTerms terms;
    ST_TRY(tile_begin(c, terms));
    bool missing = false;
    for (const ObjTerm& t : terms.t) if (t.al.s) missing = missing || !c->norm_valid[t.b * 3 + 1];
    ST_TRY(c->tile.p2.reserve(std::max(terms.n_style, 1)));
    ST_TRY(c->tile.pd.reserve(std::max(terms.n_style, 1)));
    c->tile.s2_in_p2 = missing;
    ST_TRY(ensure_dbuf(c));
    for (const ObjTerm& t : terms.t) {
        const int b = t.b;
        const float* sums = c->tile.p1 + t.sums;
        float* nrm = c->norms + b * 3;
        if (t.al.c && !c->norm_valid[b * 3 + 0]) { HIP_TRY(launch_finalize_norm(sums + 1, 1, t.n_norm, nrm + 0, c->stream)); c->norm_valid[b * 3 + 0] = 1; }
        if (t.al.d && !c->norm_valid[b * 3 + 2]) { HIP_TRY(launch_finalize_norm(sums + 3, 1, t.n_norm, nrm + 2, c->stream)); c->norm_valid[b * 3 + 2] = 1; }
    }
    if (dev_ptr) *dev_ptr = missing ? c->tile.p2 : nullptr;
    if (n_floats) *n_floats = missing ? terms.n_style : 0;
    return ST_OK;
}

// phase 2b: injected diffs of every active layer (region only, zero elsewhere)
int st_tile_losses_finish(st_ctx* c)
{
    ObjTerms terms;
    ST_TRY(tile_begin(c, terms));
    ActSet& a = c->act;
    const bool two_step = c->tile.s2_in_p2;
    if ((int)c->lt.n.size() != c->nb) c->lt.begin(c->nb);      // (st_tile_forward starts the record; a caller out of order gets a fresh one)
    for (const ObjTerm& t : terms.t) {
        const ActiveLayer& al = t.al;
        const int b = t.b, C = t.C;
        if (!c->inject[b]) ST_TRY(c->inject[b].alloc(t.n));
        float* nrm = c->norms + b * 3;
        bool wrote = false;
        if (al.c || al.d) {
            int np = 0;
            HIP_TRY(launch_layer_elem(layer_elem_args(c, al, t.n_norm, 1, nullptr, t.region()), &np, c->stream));
            wrote = true;
        }
        if (al.s) {
            ST_TRY(tile_style_D(c, b, c->tile.p1 + t.gram, t.n_norm, c->tile.pd + t.k));
            const float c2 = (float)(2.0 / ((double)C * C * t.n_norm));
            int np = 0;
            // norm from the all-reduced sum S^2 of the first pass (st_tile_style_raw), then saxpy
            if (two_step && !c->norm_valid[b * 3 + 1]) {
                HIP_TRY(launch_finalize_norm(c->tile.p2 + t.k, 1, t.n_norm, nrm + 1, c->stream));
                c->norm_valid[b * 3 + 1] = 1;
            }
            // (region only: the fp32 kernel on the fp32 blob, or -- bf16 operands -- the bf16 kernel on the blob's bf16 copy)
            ST_TRY(style_grad(c, a, style_term(c, a, b, t.region()), c->inject[b], c2, 1, al.sw, wrote, &np));
            if (!two_step) {
                // sum S^2 of this rank's region -> p3 tail (all-reduced with the image sums)
                ST_TRY(c->tile.p3.reserve(6 + kMaxTraceLayers));
                HIP_TRY(launch_sum_partials(c->s2_part[b], np, c->tile.p3 + 6 + t.k, c->stream));
            }
            c->lt.style_blob = b;
            if (c->lt.raw_blob != b) c->lt.raw_blob = -1;
        }
        c->lt.n[b] = t.n; c->lt.C[b] = C; c->lt.diff[b] = LT_WRITTEN;
        for (int k = 0; k < 3; ++k) c->lt.norm_ok[b * 3 + k] = c->norm_valid[b * 3 + k];
    }
    c->lt.any = true;
    return ST_OK;
}

// first evaluation only: unscaled style gradients, sum S^2 per style layer -> p2 (to be all-reduced)
int st_tile_style_raw(st_ctx* c)
{
    ObjTerms terms;
    ST_TRY(tile_begin(c, terms));
    ActSet& a = c->act;
    for (const ObjTerm& t : terms.t) {
        if (!t.al.s) continue;
        ST_TRY(tile_style_D(c, t.b, c->tile.p1 + t.gram, t.n_norm, c->tile.pd + t.k));
        const float c2 = (float)(2.0 / ((double)t.C * t.C * t.n_norm));
        if (!c->stmp) ST_TRY(c->stmp.alloc(c->max_blob));
        int np = 0;
        ST_TRY(style_grad(c, a, style_term(c, a, t.b, t.region()), c->stmp, c2, 0, t.al.sw, 0, &np));
        HIP_TRY(launch_sum_partials(c->s2_part[t.b], np, c->tile.p2 + t.k, c->stream));
        c->lt.style_blob = c->lt.raw_blob = t.b;
    }
    return ST_OK;
}

// phase 3: ranged backward on the window; returns the device pointer of the (3, wh, ww) gradient
int st_tile_backward(st_ctx* c, float** dev_grad)
{
    ObjTerms terms;
    ST_TRY(tile_begin(c, terms));
    const size_t n3 = (size_t)3 * c->H * c->W;
    if (!c->tile.wgrad) ST_TRY(c->tile.wgrad.alloc(n3));
    std::vector<const float*> inj(c->nb, nullptr);
    const int last = terms.last;
    for (const ObjTerm& t : terms.t) inj[t.b] = c->inject[t.b];
    if (last < 0) HIP_TRY(hipMemsetAsync(c->tile.wgrad, 0, n3 * sizeof(float), c->stream));
    else {
        if (!c->diffA) { ST_TRY(c->diffA.alloc(c->max_blob)); ST_TRY(c->diffB.alloc(c->max_blob)); }
        const float* g = inj[0];
        if (last > 0) ST_TRY(backward_chain(c, last, inj[last], inj, &g, c->bf16 && c->lean));
        HIP_TRY(hipMemcpyAsync(c->tile.wgrad, g, n3 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    }
    ST_TRY(tile_sync(c));
    if (dev_grad) *dev_grad = c->tile.wgrad;
    return ST_OK;
}

// phase 4: TV + p-norm + combine + Adam on the tile; ring = (3, th+2, tw+2) device tensor
int st_tile_update(st_ctx* c, const float* ring_dev, float** dev_ptr, int* n_floats)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c || !c->tile.on || !ring_dev) return fail(ST_ERR_STATE, "st_tile_configure first");
    if (c->opt_kind != ST_OPT_ADAM) return fail(ST_ERR_STATE, "the tile-sharded mode implements Adam");
    return tile_image_pass(c, ring_dev, true, dev_ptr, n_floats);
}

// The same image-space pass without an optimizer update: the combined gradient of the tile's pixels goes to the window-sized
// gradient buffer (st_tile_buffer 4), the partial sums come back as from st_tile_update.  The tile-sharded L-BFGS
// (style_transfer2_amd/tiled.py) evaluates the objective with it and owns the update itself.
int st_tile_gradient(st_ctx* c, const float* ring_dev, float** dev_ptr, int* n_floats)
{
    if (c) c->epoch++;
    if (!c || !c->tile.on || !ring_dev) return fail(ST_ERR_STATE, "st_tile_configure first");
    return tile_image_pass(c, ring_dev, false, dev_ptr, n_floats);
}

// BLAS-1 pieces for a caller that keeps its own vectors on this device (the tile-sharded L-BFGS): out_dev[0] = sum a b over n
// elements (this rank's partial sum; fixed summation order), y = alpha x + y.  Synchronous with respect to the host.
int st_vec_dot(st_ctx* c, const float* a_dev, const float* b_dev, long long n, float* out_dev)
{
    if (!c || !a_dev || !b_dev || !out_dev || n < 0) return fail(ST_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_vec_dot(a_dev, b_dev, (size_t)n, c->image_part, out_dev, c->stream));
    ST_TRY(tile_sync(c));
    return ST_OK;
}

int st_vec_axpy(st_ctx* c, float alpha, const float* x_dev, float* y_dev, long long n)
{
    if (!c || !x_dev || !y_dev || n < 0) return fail(ST_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_vec_axpy(alpha, x_dev, y_dev, (size_t)n, c->stream));
    ST_TRY(tile_sync(c));
    return ST_OK;
}

int st_vec_div(st_ctx* c, double divisor, float* y_dev, long long n)
{
    if (!c || !y_dev || n < 0 || !(divisor != 0.0)) return fail(ST_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_vec_div(divisor, y_dev, (size_t)n, c->stream));
    ST_TRY(tile_sync(c));
    return ST_OK;
}

// device pointers of the buffers the caller exchanges: which = 0 current x, 1 next x, 2 local sum D^2 per style layer
int st_tile_buffer(st_ctx* c, int which, float** dev_ptr)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c || !dev_ptr) return fail(ST_ERR_ARG, "bad argument");
    ST_TRY(tile_sync(c));
    if (which == 0) *dev_ptr = c->x[c->cur];
    else if (which == 1) *dev_ptr = c->x[c->cur ^ 1];
    else if (which == 2) *dev_ptr = c->tile.pd;
    else if (which == 3) *dev_ptr = c->norms;
    else if (which == 4) *dev_ptr = c->grad;
    else return fail(ST_ERR_ARG, "unknown buffer %d", which);
    return ST_OK;
}

// Pack (mode 0) the rectangles `rects` ([n][4] = y0, x0, h, w in window coordinates) of the (C, wh, ww) device tensor into
// the contiguous device buffer `buf`, or unpack them from it (mode 1 assign, 2 add): one launch per neighbour and phase.
int st_tile_strips(st_ctx* c, void* tensor_dev, int C, int wh, int ww, int n, const int* rects, void* buf_dev, int mode)
{
    if (!c || !tensor_dev || !buf_dev || n < 0 || n > kMaxStripRects || (n && !rects) || mode < 0 || mode > 2) return fail(ST_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    ST_TRY(strips(c, (float*)tensor_dev, C, wh, ww, std::vector<int>(rects, rects + 4 * n), (float*)buf_dev, mode));
    ST_TRY(tile_sync(c));
    return ST_OK;
}

// ---- the style targets of a sharded job, sharded as well -------------------------------------------------------------------------
// The style image has a tile grid of its own (tiling.style_grid).  Each rank forwards ITS window of the style image -- a feature inside
// the tile is what the whole-image forward computes, the apron argument of tiling.py -- and sums F F^T over the tile's region of every
// blob up to last_blob, un-normalised; the caller (or st_tile_set_style) all-reduces the buffer; the commit divides by the global C h w
// (worker.py:114).  Nothing here reads or writes c->tile's geometry: the pass neither needs st_tile_configure nor disturbs it.
int st_tile_style_partials(st_ctx* c, const void* hwc, int H, int W, int is_u8, int gH, int gW, int wy0, int wx0, int ty0, int tx0, int ty1, int tx1,
                           int last_blob, float** dev_ptr, int* n_floats)
{
    if (c) c->epoch++;
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    if (last_blob < 0 || last_blob >= c->nb) return fail(ST_ERR_ARG, "last_blob %d is not a blob of this net (0 .. %d)", last_blob, c->nb - 1);
    if (gH <= 0 || gW <= 0) return fail(ST_ERR_ARG, "bad style image size %d x %d", gH, gW);
    for (int i = 0; i < last_blob; ++i)
        if (c->topo[i].ave) return fail(ST_ERR_ARG, "tile-sharded mode does not run average pools (layer %s); use st_set_style", c->topo[i].name.c_str());
    const int stride = blob_size(c, last_blob, gH, gW).stride;
    if (hwc) {
        if (H <= 0 || W <= 0 || wy0 < 0 || wx0 < 0 || wy0 + H > gH || wx0 + W > gW || ty0 < wy0 || tx0 < wx0 || ty1 > wy0 + H || tx1 > wx0 + W ||
            ty1 <= ty0 || tx1 <= tx0)
            return fail(ST_ERR_ARG, "style tile/window geometry is inconsistent with the %dx%d window of the %dx%d style image", H, W, gH, gW);
        // the pooling windows of the window must be the global ones, and a tile must own whole cells of the deepest blob: origins and
        // inner edges on multiples of its total stride (tiling.TileGrid cuts so)
        if (wy0 % stride || wx0 % stride || ty0 % stride || tx0 % stride || (ty1 != gH && ty1 % stride) || (tx1 != gW && tx1 % stride))
            return fail(ST_ERR_ARG, "style tile/window edges must be multiples of the total stride %d of blob %d (or the image's far edge)", stride, last_blob);
    }
    HIP_TRY(hipSetDevice(c->device));
    size_t total = 0;
    for (int b = 0; b <= last_blob; ++b) { const size_t C = c->blob_c_topo(b); total += C * C; }
    if (hwc) ST_TRY(style_color_check(c));
    if (total > 0x7fffffffu) return fail(ST_ERR_ARG, "the style partials exceed 2^31 floats");
    c->tile.sp_last = -1;
    ST_TRY(c->tile.sp.reserve(total));
    HIP_TRY(hipMemsetAsync(c->tile.sp, 0, total * sizeof(float), c->stream));
    int r = ST_OK;
    if (hwc) {
        DevBuf<float> tmp;         // (tmp and aux are freed at the end of the block, after the synchronisation)
        ST_TRY(tmp.alloc((size_t)3 * H * W));
        ActSet aux;
        ActSet* a = &aux;
        const bool same = c->act.H == H && c->act.W == W && !c->act.data.empty();
        if (same) a = &c->act;
        r = preprocess_into(c, hwc, H, W, is_u8, tmp);
        if (r == ST_OK && c->style_match) r = style_recolor_enqueue(c, tmp, H, W);      // (a given transform: per pixel, so the window's is the image's)
        if (r == ST_OK) r = act_ensure(c, *a, H, W);
        if (r == ST_OK) r = forward_range(c, *a, tmp, last_blob);
        TileGeom g;
        g.gH = gH; g.gW = gW; g.wy0 = wy0; g.wx0 = wx0; g.ty0 = ty0; g.tx0 = tx0; g.ty1 = ty1; g.tx1 = tx1;
        size_t pos = 0;
        for (int b = 0; b <= last_blob && r == ST_OK; ++b) {
            const int C = a->C[b];
            const BlobRoi roi = tile_roi(c, *a, g, b);
            const int rw = roi.x1 - roi.x0, rh = roi.y1 - roi.y0;
            if (roi.y0 < 0 || roi.x0 < 0 || roi.y1 > a->h[b] || roi.x1 > a->w[b] || rw <= 0 || rh <= 0) {
                r = fail(ST_ERR_ARG, "the style tile has no region in blob %d of its window", b);
                break;
            }
            // a target: the fp32 region-of-interest kernel on the fp32 blob under every precision and gram_algo, as st_set_style's under bf16
            r = style_gram(c, *a, style_term(c, *a, b, &roi, true), nullptr, c->tile.sp + pos, C, 1.0, nullptr, nullptr);
            pos += (size_t)C * C;
        }
        (void)hipStreamSynchronize(c->stream);
        if (same) c->act.valid_to = -1;
    } else {
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (r != ST_OK) return r;
    c->tile.sp_n = (int)total; c->tile.sp_last = last_blob; c->tile.sp_gH = gH; c->tile.sp_gW = gW;
    if (dev_ptr) *dev_ptr = c->tile.sp;
    if (n_floats) *n_floats = (int)total;
    return ST_OK;
}

// after the all-reduce of the partials: style_gram[b] = sums / (C gh gw) for b <= last_blob (np.dot(x, x.T) / np.float32(x.size) with the
// GLOBAL size, worker.py:114); the blobs above have no target from now on
int st_tile_style_commit(st_ctx* c)
{
    if (c) c->epoch++;
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    if (c->tile.sp_last < 0 || !c->tile.sp) return fail(ST_ERR_STATE, "st_tile_style_partials first");
    HIP_TRY(hipSetDevice(c->device));
    size_t pos = 0;
    GramPlan one{}; one.bt = 128; one.splits = 1;          // the reduced sums are ONE full C x C slab
    for (int b = 0; b <= c->tile.sp_last; ++b) {
        const int C = c->blob_c_topo(b);
        if (!c->style_gram[b]) ST_TRY(c->style_gram[b].alloc((size_t)C * C));
        ProfScope ps(c, P_GRAM_REDUCE, 0, 8.0 * C * C);
        HIP_TRY(launch_gram_reduce(c->tile.sp + pos, nullptr, nullptr, c->style_gram[b], C, nullptr, nullptr, C, blob_size(c, b, c->tile.sp_gH, c->tile.sp_gW).n, one, c->stream));
        pos += (size_t)C * C;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int b = 0; b < c->nb; ++b) c->style_valid[b] = b <= c->tile.sp_last;
    c->have_style = true;
    c->tile.sp_last = -1;
    return ST_OK;
}

// test hook: the style target of a blob, C x C
int st_get_style_gram(st_ctx* c, int blob, float* out)
{
    if (!c || blob < 0 || blob >= c->nb || !out) return fail(ST_ERR_ARG, "bad argument");
    if (!c->have_style || !c->style_valid[blob] || !c->style_gram[blob])
        return fail(ST_ERR_STATE, "blob %d (%s) has no style target", blob, c->blob_names[blob].c_str());
    HIP_TRY(hipSetDevice(c->device));
    const size_t C = c->blob_c_topo(blob);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->style_gram[blob], C * C * sizeof(float), hipMemcpyDeviceToHost));
    return ST_OK;
}

int st_tile_swap(st_ctx* c)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    c->cur ^= 1;
    return ST_OK;
}

}  // extern "C"
