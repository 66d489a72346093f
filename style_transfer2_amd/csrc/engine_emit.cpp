// Emission (emit_plan.h): every reader that hands an image out, or advances the iterate average, resolves its plan here before it enqueues
// anything, and enqueues that plan's one launch here after its own work.
#include "engine.h"

namespace st2e {
int emit_preflight(const st_ctx* c, int reader, bool want_image, EmitPlan* plan)
{
    EmitFacts f{};
    f.reader = reader; f.want_image = want_image;
    f.averaging = c->avg_decay > 0; f.avg_items = c->avg_items;
    f.luminance = c->orig_colors;
    f.content = !c->have_content || !c->content_x ? EMIT_CONTENT_ABSENT : c->cH != c->H || c->cW != c->W ? EMIT_CONTENT_OTHER_SIZE : EMIT_CONTENT_FITS;
    f.avg_fits = c->avg.cap() == (size_t)3 * c->H * c->W;
    *plan = emit_resolve(f);
    switch (plan->refusal) {
    case EMIT_GRANTED: return ST_OK;
    case EMIT_NO_CONTENT:
        return fail(plan->status, "original colours: no content image to take the chroma from (st_set_content, or st_set_original_colors(ctx, 0))");
    case EMIT_CONTENT_SIZE: return fail(plan->status, "original colours: the content image is %d x %d, the input %d x %d", c->cH, c->cW, c->H, c->W);
    case EMIT_AVERAGE_OFF: return fail(plan->status, "iterate averaging is off: st_set_iterate_average first");
    case EMIT_AVERAGE_EMPTY:
        return fail(plan->status, "the iterate average is empty: only st_tile_step updates it (the phase-by-phase entry points do not)");
    default: return fail(plan->status, "internal: the iterate average has no buffer of the input's size");
    }
}

int emit_enqueue(st_ctx* c, const EmitPlan& p, float* hwc, const float* staged_v, const float* staged_cx, int h, int w)
{
    if (!p.launch) return ST_OK;
    EmitArgs a{};
    a.source = p.source; a.colour = p.colour; a.H = h; a.W = w;
    if (p.image) a.hwc = hwc;
    if (p.source == EMIT_MEAN_READ) a.mean = const_cast<float*>(staged_v);      // (only read in this form)
    else a.x = staged_v ? staged_v : c->x[c->cur].get();
    if (p.source == EMIT_MEAN_UPDATED) a.mean = c->avg;
    if (p.colour == EMIT_LUMA) a.cx = staged_cx ? staged_cx : c->content_x.get();
    if (p.advance) {        // one more item: the scalars of its update and of the image handed out after it
        a.decay = (float)c->avg_decay; a.rest = (float)(1.0 - c->avg_decay);      // (1 - decay) in double, then fp32: NumPy with a Python scalar
        a.first = c->avg_items == 0;
        c->avg_items += 1;
    }
    if (p.source != EMIT_X) a.corr = average_corr(c);
    ProfScope ps(c, P_MISC, 0, p.book ? 4.0 * 3 * h * w * p.streams : 0.0);
    HIP_TRY(launch_emit(a, c->stream));
    return ST_OK;
}
}  // namespace st2e
