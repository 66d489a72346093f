// The objective: StyleTransfer.opfunc (worker.py:231-301) as one launch sequence, its trace, and the C ABI around it.
#include "engine.h"

namespace st2e {
// ------------------------------------------------------------------------------------ the objective's layout
int objective_terms(const st_ctx* c, const ActSet& a, const TileGeom* tile, ObjTerms& terms)
{
    terms = ObjTerms{};
    if (!c->active.empty() && ((int)a.C.size() != c->nb || a.H != c->H || a.W != c->W))
        return fail(ST_ERR_STATE, "no forward of the current input has sized the activations");
    size_t pos = 0;
    for (const ActiveLayer& al : c->active) {
        if (al.c && (!c->have_content || c->cH != c->H || c->cW != c->W))
            return fail(ST_ERR_STATE, "content features missing or of a different size than the input");
        if (al.s && !c->have_style) return fail(ST_ERR_STATE, "style Gram matrices missing");
        if (al.s && !c->style_valid[al.blob])
            return fail(ST_ERR_STATE, "blob %d (%s) carries a style weight but has no style target: the sharded style pass (st_tile_set_style) stopped below it", al.blob, c->blob_names[al.blob].c_str());
        ObjTerm t{};
        t.al = al; t.b = al.blob; t.C = a.C[t.b];
        t.n = (size_t)t.C * a.h[t.b] * a.w[t.b];
        t.has_roi = tile != nullptr;
        t.roi = tile ? tile_roi(c, a, *tile, t.b) : BlobRoi{0, 0, a.h[t.b], a.w[t.b], (double)t.n};
        t.n_norm = t.roi.n_global;
        t.sums = pos;
        pos += 4;
        t.gram = kNoSlot; t.k = -1;
        if (al.s) { t.gram = pos; pos += (size_t)t.C * t.C; t.k = terms.n_style++; }
        terms.last = std::max(terms.last, t.b);
        terms.t.push_back(t);
    }
    terms.n1 = pos;
    return ST_OK;
}

ImagePassArgs image_pass_args(const st_ctx* c, const float* x, const float* scd, float* grad, bool adam, float* x_next)
{
    ImagePassArgs ip{};
    ip.x = x; ip.scd = scd; ip.grad = grad;
    ip.C = 3; ip.H = c->H; ip.W = c->W;
    ip.tv_w = c->tv_w; ip.tv_beta = c->tv_pow; ip.p_w = c->p_w; ip.p_pow = c->p_pow;
    ip.partial = c->image_part;
    if (adam) {
        // utils.py:58-64: python doubles are rounded to fp32 when they meet the fp32 arrays
        ip.x_out = x_next; ip.m = c->m; ip.v = c->v;
        ip.d1 = (float)0.9; ip.c1 = (float)(1 - 0.9); ip.d2 = (float)0.999; ip.c2 = (float)(1 - 0.999);
        ip.corr1 = (float)(1 - pow(0.9, c->items1)); ip.corr2 = (float)(1 - pow(0.999, c->items2));
        ip.step = (float)c->step_size;
        ip.m_is_zero = c->m_zero; ip.v_is_zero = c->v_zero;
        if (c->capturing) ip.dyn = c->adam_dyn;
    }
    return ip;
}

// ------------------------------------------------------------------------------------ the objective
int eval_objective(st_ctx* c, const float* x, bool want_grad, float* grad_out, bool adam, float* x_next)
{
    if (!c->x[0]) return fail(ST_ERR_STATE, "no input image");
    ST_TRY(lap_preflight(c));
    ST_TRY(anchor_preflight(c));
    ST_TRY(mat_preflight(c));
    ST_TRY(jitter_preflight(c));
    ST_TRY(act_ensure(c, c->act, c->H, c->W));
    ActSet& a = c->act;
    ObjTerms terms;
    ST_TRY(objective_terms(c, a, nullptr, terms));
    const int last = std::max(terms.last, 0);
    // lean data flow: tensors nothing reads are not written.  bf16: the whole evaluation (st_set_precision(ctx, 1)); fp32: inside an
    // iteration (st_step / st_step_begin), where no caller can ask for a blob afterwards -- st_opfunc keeps every blob for the test hooks.
    // Identical values either way.  ST2_LEAN32=0 switches the fp32 part off (read per evaluation: A/B runs).
    const bool lean = c->bf16 && c->lean && !c->tile.on;         // the bf16 data flow (forward AND backward)
    bool lean32 = false;                                          // fp32: the forward only (dead pooled-layer blobs)
    if (!c->bf16 && c->in_step && !c->tile.on) lean32 = lean32_enabled();
    // jitter (st_set_jitter): the network terms see roll(x, s) and content features of roll(cx, s); mode off: xf == x, the features as ever
    ST_TRY(jitter_content(c));
    const float* xf = x;
    ST_TRY(jitter_roll_in(c, x, want_grad, &xf));
    ST_TRY(forward_range(c, a, xf, last, lean || lean32));

    std::vector<const float*> inj(c->nb, nullptr);
    std::fill(c->cnt.begin(), c->cnt.end(), 0);
    c->sf_in.assign(c->nb, nullptr); c->sf_w.assign(c->nb, nullptr);
    c->lt.begin(c->nb);
    for (const ObjTerm& ot : terms.t) {
        const ActiveLayer& al = ot.al;
        const int b = ot.b, C = ot.C;
        const size_t n = ot.n;
        if (!c->inject[b]) ST_TRY(c->inject[b].alloc(n));
        c->inject_roi_zero[b] = 0;
        ST_TRY(ensure_layer_part(c, b));
        float* part = c->layer_part[b];
        float* nrm = c->norms + b * 3;
        int* cnt = &c->cnt[b * 6];
        bool wrote = false;
        if (al.c || al.d) {
            LayerElemArgs e = layer_elem_args(c, al, (double)n, 1, part);
            const bool need_norm = (al.c && !c->norm_valid[b * 3 + 0]) || (al.d && !c->norm_valid[b * 3 + 2]);
            int np = 0;
            if (need_norm) {      // first evaluation after reset(): norms are captured (worker.py:253-254,274-275)
                e.write = 0;
                { ProfScope ps(c, P_LAYER_ELEM, 0, 4.0 * n * (al.c ? 2 : 1)); HIP_TRY(launch_layer_elem(e, &np, c->stream)); }
                ProfScope ps(c, P_FINALIZE, 0, 0);
                if (al.c && !c->norm_valid[b * 3 + 0]) { HIP_TRY(launch_finalize_norm(e.part_gc2, np, (double)n, nrm + 0, c->stream)); c->norm_valid[b * 3 + 0] = 1; }
                if (al.d && !c->norm_valid[b * 3 + 2]) { HIP_TRY(launch_finalize_norm(e.part_gd2, np, (double)n, nrm + 2, c->stream)); c->norm_valid[b * 3 + 2] = 1; }
            }
            e.write = 1;
            { ProfScope ps(c, P_LAYER_ELEM, 0, 4.0 * n * (al.c ? 3 : 2)); HIP_TRY(launch_layer_elem(e, &np, c->stream)); }
            cnt[0] = cnt[1] = cnt[2] = cnt[3] = np;
            wrote = true;
        }
        if (al.s) {
            ST_TRY(ensure_dbuf(c));
            // which kernels, on which copy of the blob (bf16 operands: the copy where this forward wrote one the kernels take; norm
            // known: the gradient may ride on the data-gradient conv above this blob, and only its trace value is taken here)
            const StyleTerm t = style_term(c, a, b, nullptr, false, want_grad ? last : -1);
            ST_TRY(style_gram(c, a, t, c->style_gram[b], c->dbuf, conv_mpad(C), (double)n, part + 4 * kMaxPartials, &cnt[4]));
            const float c2 = (float)(2.0 / ((double)C * C * (double)n));
            if (c->norm_valid[b * 3 + 1]) {
                ST_TRY(style_grad(c, a, t, c->inject[b], c2, 1, al.sw, wrote, &cnt[5]));
            } else {              // first evaluation: S unscaled -> norm -> saxpy (worker.py:265-269)
                if (!c->stmp) ST_TRY(c->stmp.alloc(c->max_blob));
                ST_TRY(style_grad(c, a, t, c->stmp, c2, 0, al.sw, 0, &cnt[5]));
                { ProfScope ps(c, P_FINALIZE, 0, 0);
                  HIP_TRY(launch_finalize_norm(c->s2_part[b], cnt[5], (double)n, nrm + 1, c->stream)); }
                c->norm_valid[b * 3 + 1] = 1;
                ProfScope ps(c, P_VECTOR, 0, 4.0 * n * 3);
                HIP_TRY(launch_scaled_accumulate(c->stmp, c->inject[b], al.sw, nrm + 1, wrote, n, c->stream));
                c->lt.raw_blob = b;
            }
            c->lt.style_blob = b;
            if (c->lt.raw_blob != b) c->lt.raw_blob = -1;
        }
        c->lt.n[b] = n; c->lt.C[b] = C;
        c->lt.diff[b] = c->sf_w[b] ? LT_RODE_ON_CONV : LT_WRITTEN;
        for (int k = 0; k < 3; ++k) c->lt.norm_ok[b * 3 + k] = c->norm_valid[b * 3 + k];
        inj[b] = (c->sf_w[b] && !wrote) ? nullptr : c->inject[b];          // (a fused style term writes nothing into the inject buffer)
    }

    const float* scd = nullptr;
    if (want_grad && !c->active.empty()) {
        if (!c->diffA) { ST_TRY(c->diffA.alloc(c->max_blob)); ST_TRY(c->diffB.alloc(c->max_blob)); }
        if (last == 0) scd = inj[0];
        else {
            std::vector<const float*> below = inj;
            const int rc = backward_chain(c, last, inj[last], below, &scd, lean);
            c->sf_in.assign(c->nb, nullptr); c->sf_w.assign(c->nb, nullptr);      // (the ranged-backward entry points never fuse)
            ST_TRY(rc);
        }
        ST_TRY(jitter_roll_out(c, &scd));         // jitter: the image pass, which reads the unshifted x, takes the un-rolled network gradient
    }

    // the Laplacian term (st_set_laplacian): E per level and its sums; with a gradient, g_lap for the image pass to add after p_w g_p
    const bool lap = c->lap.n > 0;
    if (lap) {
        ST_TRY(lap_forward(c, x));
        if (want_grad) ST_TRY(lap_backward(c));
    }

    // the anchor term (st_set_anchor): one launch; with a gradient it leaves extra = g_lap + g_anc (or g_anc), which takes g_lap's place
    const float* extra = lap && want_grad ? c->lap.g.get() : nullptr;
    const bool anchor = c->anchor.on;
    if (anchor) ST_TRY(anchor_eval(c, x, want_grad, extra, &extra));

    // the photorealism term (st_set_matting): two window passes; with a gradient the second leaves extra = prev + g_mat (or g_mat)
    const bool mat = c->mat.on;
    if (mat) ST_TRY(mat_eval(c, x, want_grad, extra, &extra));

    {
        const ImagePassArgs ip = image_pass_args(c, x, scd, want_grad ? grad_out : nullptr, adam, x_next);
        const double n3 = 3.0 * c->H * c->W;
        ProfScope ps(c, P_IMAGE_PASS, 0, 4.0 * n3 * ((adam ? 7 : 3) + (extra ? 1 : 0)));
        HIP_TRY(launch_image_pass(ip, &c->image_cnt, c->stream, extra));
    }
    ST_TRY(jitter_scd_sums(c));                   // jitter: scd_grad is that of the shifted evaluation (the sums of squares in ITS order)

    {
        TraceArgs t{};
        t.n_layers = (int)terms.t.size();
        for (int l = 0; l < t.n_layers; ++l) {
            const ActiveLayer& al = terms.t[l].al;
            const int b = al.blob;
            TraceLayer& L = t.layer[l];
            L.content = al.c; L.style = al.s; L.deepdream = al.d;
            L.cw = al.cw; L.sw = al.sw; L.dw = al.dw;
            L.n = (double)terms.t[l].n;
            L.gram_n = (double)a.C[b] * a.C[b];
            for (int k = 0; k < 5; ++k) { L.part[k] = c->layer_part[b] + k * kMaxPartials; L.count[k] = c->cnt[b * 6 + k]; }
            L.part[5] = c->s2_part[b]; L.count[5] = c->cnt[b * 6 + 5];
            L.norm = c->norms + b * 3;
        }
        t.image_part = c->image_part; t.image_count = c->image_cnt; t.image_n = 3.0 * c->H * c->W;
        t.tv_w = c->tv_w; t.p_w = c->p_w; t.p_pow = c->p_pow; t.have_grad = want_grad;
        t.out = c->trace_dev;
        t.sums = c->trace_sums;
        c->trace_len_last = t.n_layers * 6 + 8 + (lap ? 2 : 0) + (anchor ? 2 : 0) + (mat ? 2 : 0);
        ProfScope ps(c, P_FINALIZE, 0, 0);
        HIP_TRY(launch_finalize_trace(t, c->stream));
        if (lap) {                // l_loss and l_grad join the image part of the trace
            TraceLapArgs tl{};
            tl.levels = c->lap.n; tl.part = c->lap.part; tl.count_e = c->lap.cnt_e; tl.count_g = want_grad ? c->lap.cnt_g : 0;
            for (int l = 0; l < c->lap.n; ++l) tl.w[l] = c->lap.plan.lv[l].w;
            tl.image_n = t.image_n; tl.have_grad = want_grad; tl.image_out = c->trace_dev + t.n_layers * 6;
            HIP_TRY(launch_trace_lap(tl, c->stream));
        }
        if (anchor) ST_TRY(anchor_trace(c, want_grad, lap, c->trace_dev + t.n_layers * 6));      // a_loss and a_grad, after the Laplacian term's
        if (mat) ST_TRY(mat_trace(c, want_grad, (lap ? 1 : 0) + (anchor ? 1 : 0), c->trace_dev + t.n_layers * 6));      // m_loss and m_grad, last
    }
    c->lt.any = true;
    return ST_OK;
}

int read_trace(st_ctx* c, double* trace, float* loss)
{
    const int n = c->trace_len_last;
    HIP_TRY(hipMemcpyAsync(c->trace_host, c->trace_dev, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (trace) for (int i = 0; i < n; ++i) trace[i] = c->trace_host[i];
    c->last_loss = c->trace_host[n - 2];
    if (loss) *loss = c->last_loss;
    return ST_OK;
}
}  // namespace st2e

extern "C" {

// ---- objective
int st_set_weights(st_ctx* c, int n_rows, const int* blob_index, const float* content, const float* style,
                   const float* deepdream, const double params[4])
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c || n_rows < 0 || (n_rows && (!blob_index || !content || !style || !deepdream)) || !params)
        return fail(ST_ERR_ARG, "bad argument");
    std::vector<ActiveLayer> rows;
    for (int i = 0; i < n_rows; ++i) {
        const int b = blob_index[i];
        if (b < 0 || b >= c->nb) return fail(ST_ERR_ARG, "row %d names blob %d", i, b);
        rows.push_back(ActiveLayer{b, content[i], style[i], deepdream[i], nonzero(content[i]), nonzero(style[i]), nonzero(deepdream[i])});
    }
    c->rows = rows;
    c->active.clear();
    for (const ActiveLayer& r : rows) if (r.c || r.s || r.d) c->active.push_back(r);
    c->tile.evaluated = false;
    c->tv_w = (float)params[0]; c->tv_pow = (float)params[1]; c->p_w = (float)params[2]; c->p_pow = (float)params[3];
    // content features are kept only where a content weight reads them (ensure_content_features brings back what a later table needs)
    if (c->have_content) {
        std::vector<char> used(c->nb, 0);
        for (const ActiveLayer& al : c->active) if (al.c) used[al.blob] = 1;
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (int b = 0; b < c->nb; ++b) if (!used[b]) c->content_feat[b].reset();
    }
    return ST_OK;
}

int st_clear_norms(st_ctx* c)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    std::fill(c->norm_valid.begin(), c->norm_valid.end(), 0);
    return ST_OK;
}

// test hook: what the last evaluation left for a blob.  Reads only: no epoch bump (a captured step graph stays valid), no allocation.
int st_get_layer_terms(st_ctx* c, int index, float* D, float* raw_S, float* diff, float norms[3])
{
    if (!c || index < 0 || index >= c->nb) return fail(ST_ERR_ARG, "bad argument");
    const LayerTerms& lt = c->lt;
    const char* name = c->blob_names[index].c_str();
    if (!lt.any)
        return fail(ST_ERR_STATE, lt.resized ? "the iterate was resized after the last evaluation: its work buffers are gone; evaluate again"
                                             : "no objective evaluation has completed on this context");
    if (!lt.n[index]) return fail(ST_ERR_STATE, "blob %d (%s) carried no weight in the last evaluation", index, name);
    if ((D || raw_S) && lt.style_blob != index) {
        if (lt.style_blob < 0) return fail(ST_ERR_STATE, "the last evaluation had no style term: no D and no style gradient of blob %d (%s)", index, name);
        return fail(ST_ERR_STATE, "D and the unscaled style gradient are one buffer each for all layers: they hold those of blob %d (%s), the style layer evaluated last, not of blob %d (%s)",
                    lt.style_blob, c->blob_names[lt.style_blob].c_str(), index, name);
    }
    if (raw_S && lt.raw_blob != index)
        return fail(ST_ERR_STATE, "the last evaluation of blob %d (%s) knew its style norm and scaled the gradient in the kernel's epilogue: the unscaled one exists only after the first evaluation since reset() / st_clear_norms", index, name);
    if (diff && lt.diff[index] == LT_RODE_ON_CONV)
        return fail(ST_ERR_STATE, "the style term of blob %d (%s) rode on the data-gradient conv above it: nothing was written into its diff (ST2_STYLE_FUSE=0, or an evaluation without gradient, materialises it)", index, name);
    if (diff && lt.diff[index] == LT_OVERWRITTEN)
        return fail(ST_ERR_STATE, "st_backward has overwritten the diff of blob %d (%s) since the last evaluation", index, name);
    if (diff && (lt.diff[index] != LT_WRITTEN || !c->inject[index])) return fail(ST_ERR_STATE, "blob %d (%s) has no diff of the last evaluation", index, name);
    if ((D && !c->dbuf) || (raw_S && !c->stmp)) return fail(ST_ERR_STATE, "internal: the buffer of blob %d (%s) is gone", index, name);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t C = (size_t)lt.C[index], n = lt.n[index];
    if (D) HIP_TRY(hipMemcpy2D(D, C * sizeof(float), c->dbuf, (size_t)conv_mpad((int)C) * sizeof(float), C * sizeof(float), C, hipMemcpyDeviceToHost));
    if (raw_S) HIP_TRY(hipMemcpy(raw_S, c->stmp, n * sizeof(float), hipMemcpyDeviceToHost));
    if (diff) HIP_TRY(hipMemcpy(diff, c->inject[index], n * sizeof(float), hipMemcpyDeviceToHost));
    if (norms) {
        HIP_TRY(hipMemcpy(norms, c->norms + index * 3, 3 * sizeof(float), hipMemcpyDeviceToHost));
        for (int k = 0; k < 3; ++k) if (!lt.norm_ok[index * 3 + k]) norms[k] = 0.f;      // (a term the blob does not carry has no norm)
    }
    return ST_OK;
}

// test hook: tap the running diff of one blob (backward_chain copies what the launch that produces it wrote); -1 turns it off
int st_tap_diff(st_ctx* c, int index)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c || index < -1 || index >= c->nb) return fail(ST_ERR_ARG, "bad argument");
    if (index >= 0 && c->tile.on) return fail(ST_ERR_STATE, "the diff tap does not run on a tile-configured context");
    if (c->pipe.count) return fail(ST_ERR_STATE, "%d pipelined iteration(s) in flight: st_step_end first", c->pipe.count);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));              // (a copy of the last tapped evaluation may still be in flight)
    c->tap = DiffTap{};
    c->tap.blob = index;
    return ST_OK;
}

// test hook: the copy the last tapped evaluation made.  Reads only: no epoch bump, no allocation.
int st_get_tapped_diff(st_ctx* c, float* out32, uint16_t* out16, int* have32, int* have16)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    const DiffTap& t = c->tap;
    if (t.blob < 0) return fail(ST_ERR_STATE, "no diff is tapped: st_tap_diff first");
    const char* name = c->blob_names[t.blob].c_str();
    if (!t.have)
        return fail(ST_ERR_STATE, t.resized ? "the iterate was resized after the last tapped evaluation of blob %d (%s): its copy is that of the old size; evaluate again"
                                            : "no evaluation with a gradient (st_opfunc with out_grad) whose backward produced the diff of blob %d (%s) has completed since the tap was set",
                    t.blob, name);
    if ((t.have32 && !t.d32) || (t.have16 && !t.d16)) return fail(ST_ERR_STATE, "internal: the tapped copy of blob %d (%s) is gone", t.blob, name);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t hw = (size_t)t.h * t.w;
    if (out32 && t.have32) HIP_TRY(hipMemcpy(out32, t.d32, (size_t)t.C * hw * sizeof(float), hipMemcpyDeviceToHost));
    if (out16 && t.have16) HIP_TRY(hipMemcpy(out16, t.d16, act16_elems(t.C, hw) * sizeof(unsigned short), hipMemcpyDeviceToHost));
    if (have32) *have32 = t.have32;
    if (have16) *have16 = t.have16;
    return ST_OK;
}

int st_trace_len(st_ctx* c) { return c ? (int)c->active.size() * 6 + 8 + (c->lap.n ? 2 : 0) + (c->anchor.on ? 2 : 0) + (c->mat.on ? 2 : 0) : 0; }

int st_opfunc(st_ctx* c, float* out_loss, float* out_grad, double* trace)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    if (!c->x[0]) return fail(ST_ERR_STATE, "no input image");
    ST_TRY(lap_preflight(c));                                 // refused before anything is enqueued
    ST_TRY(anchor_preflight(c));
    ST_TRY(mat_preflight(c));
    ST_TRY(jitter_preflight(c));
    HIP_TRY(hipSetDevice(c->device));
    if (c->tap.blob >= 0 && out_grad) {                       // st_tap_diff: this evaluation's backward copies the tapped diff
        c->tap.armed = true; c->tap.captured = c->tap.have = false;
        const int rc = eval_objective(c, c->x[c->cur], true, c->grad, false, nullptr);
        c->tap.armed = false;
        ST_TRY(rc);
        c->tap.have = c->tap.captured; c->tap.resized = false;
    } else
        ST_TRY(eval_objective(c, c->x[c->cur], out_grad != nullptr, c->grad, false, nullptr));
    if (out_grad) HIP_TRY(hipMemcpyAsync(out_grad, c->grad, (size_t)3 * c->H * c->W * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    return read_trace(c, trace, out_loss);
}

}  // extern "C"
