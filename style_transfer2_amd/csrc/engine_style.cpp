// The style term of a blob (Gram of the current features, D = G - G_style, style gradient c2 D @ F, its sum S^2 partials), resolved once:
// style_shape / style_term decide, style_gram / style_grad launch what the record says.  No other engine code names these kernels
// (but the two reduces of all-reduced raw sums in engine_tile.cpp).
#include "engine.h"

namespace st2e {
StyleShape style_shape(const st_ctx* c, const ActSet& a, int b)
{
    StyleShape s{};
    if (!c->bf16 || b < 1 || !c->topo[b - 1].is_conv) return s;
    const int C = a.C[b], hw = a.h[b] * a.w[b];
    s.grad16 = conv16_ok(c, C) && style_grad16_ok(C, (size_t)hw);
    // tile-sharded mode: the region-of-interest forms of both kernels take any region (ragged last step, 4-byte stores when the
    // region's rows are not 16-byte aligned); ST2_TILE_STYLE16=0 keeps the fp32 region-of-interest kernels
    s.gram16 = s.grad16 && (c->tile.on ? !env_off("ST2_TILE_STYLE16") : hw % 64 == 0 && gram16_ok(C, hw, gram_plan16(C, hw)));
    return s;
}

size_t style_split_scratch(int C, int hw) { return gram_split_ok(C, hw) && style_grad_split_ok(C, hw) ? style_grad_split_pack_elems(C) : 0; }

// May the style gradient of blob b ride on the data-gradient conv of the layer above it (conv3x3_mfma_bf16.hip)?  (ST2_STYLE_FUSE: per evaluation)
static bool style_fuse_ok(const st_ctx* c, const ActSet& a, int b, int last)
{
    if (env_off("ST2_STYLE_FUSE") || b + 1 > last || a.C[b] % 32 != 0) return false;
    const Layer& up = c->topo[b];                       // layer b + 1: consumes blob b
    return up.is_conv && up.loaded && conv16_ok(c, up.cout) && up.cin == a.C[b];
}

StyleTerm style_term(const st_ctx* c, const ActSet& a, int b, const BlobRoi* roi, bool target, int fuse_last)
{
    const FwdRoute& fr = a.plan.fwd[b];
    StyleTerm t{};
    const int C = t.C = a.C[b];
    t.b = b; t.roi = roi != nullptr; t.book = target || !roi;      // (the phases of a tile-sharded iteration are not booked: bench.py reads the tables)
    const size_t plane = (size_t)a.h[b] * a.w[b];
    if (roi) { t.groi = GramRoi{roi->y0, roi->x0, roi->x1 - roi->x0, a.w[b], plane}; t.proi = PixRoi{roi->y0, roi->x0, roi->y1, roi->x1}; }
    const int hw = t.hw = roi ? t.groi.rw * (roi->y1 - roi->y0) : (int)plane;
    // bf16 operands, where this forward wrote a copy the kernels take (the style targets stay Grams of the fp32 blob): a whole blob
    // may have the Gram on the fp32 blob and the gradient on the copy (hw % 64 != 0), a region takes both or neither
    const bool may16 = !target && (roi || !c->tile.on);
    const bool gram16 = may16 && fr.style_all16, grad16 = may16 && (roi ? fr.style_all16 : fr.style16);
    // st_set_gram_algo(ctx, 1): fp32 features, whole blobs, not tile-sharded, a shape the split kernels take -- same plan, slabs and reduction
    const size_t split_elems = style_split_scratch(C, hw);
    const bool split = c->gram_split && !c->bf16 && !c->tile.on && !roi && split_elems > 0;
    const double fl = 2.0 * C * C * (double)hw, n = (double)C * hw;
    t.plan = gram16 ? gram_plan16(C, hw) : gram_plan(C, hw);
    t.gram = gram16 ? StyleLaunch{OPS_BF16, P_GRAM_BF16, fl, 2.0 * C * (double)hw}      // (the class names the matrix core that runs)
             : StyleLaunch{split ? OPS_SPLIT : OPS_F32, split ? P_GRAM_SPLIT : P_GRAM, fl, 4.0 * C * (double)hw};
    if (gram16 && fuse_last >= 0 && c->norm_valid[b * 3 + 1] && style_fuse_ok(c, a, b, fuse_last)) {
        t.sfuse = style_fuse_pack_elems(C, conv_mpad(C));
        t.pack = StyleLaunch{OPS_FUSED, P_MISC, 0, 4.0 * C * C + 2.0 * t.sfuse};
        t.grad = StyleLaunch{OPS_FUSED, P_STYLE_GRAD, 2.0 * C * C * (double)C, 12.0 * C * C};
        t.slots = style_s2_trace_blocks(C);
    } else if (grad16) {
        t.grad = StyleLaunch{OPS_BF16, P_STYLE_GRAD_BF16, fl, n * 6.0};
        t.slots = style_grad16_blocks(C, (size_t)hw);
    } else if (split && split_elems <= c->dsplit.cap()) {
        t.grad = StyleLaunch{OPS_SPLIT, P_STYLE_GRAD_SPLIT, fl, n * 8.0};
        t.slots = style_grad_split_blocks(C, hw);
    } else {
        t.grad = StyleLaunch{OPS_F32, P_STYLE_GRAD, fl, n * 8.0};
        t.slots = style_grad_blocks(C, a.h[b], a.w[b]);
    }
    if (grad16) t.d16 = style_grad16_pack_elems(C);       // (a fused term keeps the buffer the unfused launch of its first evaluation needs)
    t.reads16 = grad16; t.reads32 = !gram16 || !grad16; t.missing32 = t.reads32 && !fr.out32;
    return t;
}

static int missing_copy(const StyleTerm& t) { return fail(ST_ERR_STATE, t.roi ? "internal: style blob %d has no fp32 copy" : "internal: style blob %d has neither an fp32 nor a usable bf16 copy", t.b); }

int style_gram(st_ctx* c, const ActSet& a, const StyleTerm& t, const float* target, float* out, int out_ld, double divisor, float* partial, int* n_partial)
{
    if (t.missing32) return missing_copy(t);
    const int b = t.b, C = t.C;
    const GramRoi* roi = t.roi ? &t.groi : nullptr;
    ST_TRY(c->gram_slabs.reserve(t.plan.slab_floats));
    ST_TRY(c->gram_fold.reserve((size_t)gram_fold_groups(t.plan) * C * C));
    {
        ProfScope ps(c, t.gram.cls, t.gram.flops, t.gram.bytes, t.book);
        if (t.gram.ops == OPS_BF16) HIP_TRY(launch_gram16_partial(a.data16[b], c->gram_slabs, C, t.hw, t.plan, c->stream, roi));
        else if (t.gram.ops == OPS_SPLIT) HIP_TRY(launch_gram_split_partial(a.data[b], c->gram_slabs, C, t.hw, t.plan, c->stream));
        else HIP_TRY(launch_gram_partial(a.data[b], c->gram_slabs, C, t.hw, t.plan, c->stream, roi));
    }
    ProfScope ps(c, P_GRAM_REDUCE, 0, 4.0 * (double)t.plan.slab_floats, t.book);
    HIP_TRY(launch_gram_reduce(c->gram_slabs, c->gram_fold, target, out, out_ld, partial, n_partial, C, divisor, t.plan, c->stream));
    return ST_OK;
}

int style_grad(st_ctx* c, const ActSet& a, const StyleTerm& t, float* dst, float c2, int fused, float sw, int accumulate, int* np)
{
    if (t.missing32) return missing_copy(t);
    const int b = t.b, C = t.C, ld = conv_mpad(C);
    const float* norm = c->norms + b * 3 + 1;
    ST_TRY(c->s2_part[b].reserve(t.slots));
    if (t.d16) ST_TRY(c->d16.reserve(t.d16));
    float* part = c->s2_part[b];
    if (t.grad.ops == OPS_FUSED) {           // the operand of the data-gradient conv above the blob, and the trace value of the gradient
        ST_TRY(c->sfuse_w[b].reserve(t.sfuse));
        { ProfScope ps(c, t.pack.cls, t.pack.flops, t.pack.bytes, t.book);
          HIP_TRY(launch_style_fuse_pack(c->dbuf, ld, C, ld, c2, sw, norm, c->sfuse_w[b], c->stream)); }
        ProfScope ps(c, t.grad.cls, t.grad.flops, t.grad.bytes, t.book);
        HIP_TRY(launch_style_s2_trace(c->dbuf, ld, c->style_gram[b], C, (double)C * t.hw, c2, part, np, c->stream));
        c->sf_in[b] = a.data16[b]; c->sf_w[b] = c->sfuse_w[b];
        return ST_OK;
    }
    // the bf16 kernel touches the region's pixels only: the inject buffer is zeroed outside the region once
    if (t.roi && t.grad.ops == OPS_BF16 && dst == c->inject[b] && !accumulate && !c->inject_roi_zero[b]) {
        HIP_TRY(hipMemsetAsync(dst, 0, (size_t)C * t.groi.plane * sizeof(float), c->stream));
        c->inject_roi_zero[b] = 1;
    }
    ProfScope ps(c, t.grad.cls, t.grad.flops, t.grad.bytes, t.book);
    if (t.grad.ops == OPS_SPLIT) HIP_TRY(launch_style_grad_split(c->dbuf, ld, c->dsplit, a.data[b], dst, c2, fused, sw, norm, accumulate, part, np, C, t.hw, c->stream));
    else if (t.grad.ops == OPS_BF16) HIP_TRY(launch_style_grad16(c->dbuf, ld, c->d16, a.data16[b], dst, c2, fused, sw, norm, accumulate, part, np, C, (size_t)t.hw, c->stream, t.roi ? &t.groi : nullptr));
    else HIP_TRY(launch_style_grad(c->dbuf, a.data[b], dst, c2, fused, sw, norm, accumulate, part, np, C, a.h[b], a.w[b], c->stream, t.roi ? &t.proi : nullptr));
    return ST_OK;
}

int ensure_dbuf(st_ctx* c)
{
    if (c->dbuf) return ST_OK;
    size_t cc = 1;
    for (int i = 0; i < c->nb; ++i) cc = std::max(cc, (size_t)c->act.C[i] * conv_mpad(c->act.C[i]));
    ST_TRY(c->dbuf.alloc(cc));
    HIP_TRY(hipMemsetAsync(c->dbuf, 0, cc * sizeof(float), c->stream));
    return ST_OK;
}

int ensure_layer_part(st_ctx* c, int b) { return c->layer_part[b] ? ST_OK : c->layer_part[b].alloc(5 * kMaxPartials); }

LayerElemArgs layer_elem_args(const st_ctx* c, const ActiveLayer& al, double n_norm, int write, float* part, const BlobRoi* roi)
{
    const ActSet& a = c->act;
    const int b = al.blob;
    float* nrm = c->norms + b * 3;
    LayerElemArgs e{};
    e.feat = a.data[b]; e.target = al.c ? c->content_feat[b].get() : nullptr; e.inject = c->inject[b];
    e.n = (size_t)a.C[b] * a.h[b] * a.w[b]; e.cn_coef = (float)(2.0 / n_norm); e.dn_coef = (float)(-2.0 / n_norm);
    e.cw = al.cw; e.dw = al.dw; e.content = al.c; e.deepdream = al.d; e.write = write;
    e.norm_c = nrm + 0; e.norm_d = nrm + 2;
    if (part) { e.part_d2 = part; e.part_gc2 = part + kMaxPartials; e.part_f2 = part + 2 * kMaxPartials; e.part_gd2 = part + 3 * kMaxPartials; }
    if (roi) { e.h = a.h[b]; e.w = a.w[b]; e.ry0 = roi->y0; e.rx0 = roi->x0; e.ry1 = roi->y1; e.rx1 = roi->x1; }
    return e;
}
}  // namespace st2e
