// The anchor term (include/st2.h: st_set_anchor): its buffers, its one launch inside an objective evaluation, and the C ABI around
// them.  anchor_plan.h has the validation and the grids, anchor.hip the kernels.
#include "engine.h"

namespace st2e {
namespace {
struct AnchorBufs { DevBuf<float> ax, m, extra, part; };

int anchor_alloc(const AnchorPlan& p, bool mask, AnchorBufs& b)
{
    ST_TRY(b.ax.alloc(p.pixels));
    if (mask) ST_TRY(b.m.alloc(p.plane));
    ST_TRY(b.extra.alloc(p.pixels));
    ST_TRY(b.part.alloc((size_t)kAnchorPartRows * kMaxPartials));
    return ST_OK;
}

// Everything the two setters share.  hwc: an image for preprocess_into, or NULL and `planar` the preprocessed planes on the host.
// The buffers are made and filled first: when that fails nothing has changed.
int anchor_set(st_ctx* c, const char* who, const void* hwc, int is_u8, const float* planar, int H, int W, const float* mask, double weight)
{
    const int bad = anchor_validate(H, W, mask, weight);
    if (bad) return fail(ST_ERR_ARG, "%s: %s", who, anchor_refusal_text(bad));
    if (c->pipe.count) return fail(ST_ERR_STATE, "%d pipelined iteration(s) in flight: st_step_end before %s", c->pipe.count, who);
    if (c->tile.on) return fail(ST_ERR_STATE, "the anchor term does not run on a tile-configured context");
    HIP_TRY(hipSetDevice(c->device));
    AnchorPlan p{};
    const int r = anchor_plan(H, W, weight, &p);
    if (r) return fail(ST_ERR_ARG, "%s: %s", who, anchor_refusal_text(r));
    AnchorBufs fresh;
    ST_TRY(anchor_alloc(p, mask != nullptr, fresh));
    if (hwc) ST_TRY(preprocess_into(c, hwc, H, W, is_u8, fresh.ax));
    else HIP_TRY(hipMemcpyAsync(fresh.ax, planar, p.pixels * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (mask) HIP_TRY(hipMemcpyAsync(fresh.m, mask, p.plane * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));              // (the host arrays are the caller's again; nothing queued reads the buffers that go)
    st_ctx::Anchor& A = c->anchor;
    A = st_ctx::Anchor{};
    A.on = true; A.weight = weight; A.has_mask = mask != nullptr; A.plan = p;
    A.ax = std::move(fresh.ax); A.m = std::move(fresh.m); A.extra = std::move(fresh.extra); A.part = std::move(fresh.part);
    return ST_OK;
}
}  // namespace

int anchor_preflight(const st_ctx* c)
{
    const st_ctx::Anchor& A = c->anchor;
    if (!A.on) return ST_OK;
    if (c->tile.on) return fail(ST_ERR_STATE, "the anchor term does not run on a tile-configured context");
    if (c->x[0] && (A.plan.H != c->H || A.plan.W != c->W))
        return fail(ST_ERR_STATE, "the anchor term needs an anchor of the input's size: the anchor is %d x %d, the input %d x %d (st_set_anchor again, or turn the term off)",
                    A.plan.H, A.plan.W, c->H, c->W);
    return ST_OK;
}

void anchor_input_resized(st_ctx* c)
{
    st_ctx::Anchor& A = c->anchor;
    if (A.evaluated) A.resized = true;
    A.evaluated = false; A.have_grad = false;
}

int anchor_eval(st_ctx* c, const float* x, bool want_grad, const float* g_lap, const float** extra)
{
    st_ctx::Anchor& A = c->anchor;
    ST_TRY(anchor_preflight(c));
    const AnchorPlan& p = A.plan;
    A.evaluated = false; A.have_grad = false;
    AnchorArgs a{};
    a.x = x; a.ax = A.ax; a.m = A.has_mask ? A.m.get() : nullptr;
    a.g_lap = want_grad ? g_lap : nullptr; a.extra = want_grad ? A.extra.get() : nullptr;
    a.part = A.part; a.plane = p.plane; a.W = p.W; a.w = p.w;
    const double planes = 2 + (want_grad ? 1 : 0) + (a.g_lap ? 1 : 0);
    ProfScope ps(c, P_ANCHOR, 0, 4.0 * (planes * (double)p.pixels + (a.m ? (double)p.plane : 0.0)));
    HIP_TRY(launch_anchor(a, p.grid, p.grid_vec, &A.cnt, c->stream));
    A.evaluated = true; A.have_grad = want_grad; A.resized = false;
    *extra = a.extra;
    return ST_OK;
}

int anchor_trace(st_ctx* c, bool want_grad, bool with_lap, float* image_out)
{
    const st_ctx::Anchor& A = c->anchor;
    TraceAnchorArgs t{};
    t.part = A.part; t.count_l = A.cnt; t.count_g = want_grad ? A.cnt : 0; t.w = A.plan.w;
    t.image_n = (double)A.plan.pixels; t.have_grad = want_grad; t.with_lap = with_lap; t.image_out = image_out;
    HIP_TRY(launch_trace_anchor(t, c->stream));
    return ST_OK;
}
}  // namespace st2e

extern "C" {

int st_set_anchor(st_ctx* c, const void* hwc, int H, int W, int is_u8, const float* mask_hw, double weight)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    if (!hwc) {              // off: every buffer of the term goes
        if (c->pipe.count) return fail(ST_ERR_STATE, "%d pipelined iteration(s) in flight: st_step_end before st_set_anchor", c->pipe.count);
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->anchor = st_ctx::Anchor{};
        return ST_OK;
    }
    return anchor_set(c, "st_set_anchor", hwc, is_u8, nullptr, H, W, mask_hw, weight);
}

int st_set_anchor_nchw(st_ctx* c, const float* ax, int H, int W, const float* mask_hw, double weight)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    if (!ax) return fail(ST_ERR_ARG, "st_set_anchor_nchw: the anchor planes are required (st_set_anchor(ctx, NULL, ...) turns the term off)");
    return anchor_set(c, "st_set_anchor_nchw", nullptr, 0, ax, H, W, mask_hw, weight);
}

int st_get_anchor(st_ctx* c, int* on, int* H, int* W, int* has_mask, double* weight)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    const st_ctx::Anchor& A = c->anchor;
    if (on) *on = A.on;
    if (H) *H = A.on ? A.plan.H : 0;
    if (W) *W = A.on ? A.plan.W : 0;
    if (has_mask) *has_mask = A.has_mask;
    if (weight) *weight = A.weight;
    return ST_OK;
}

// test hook: what the last evaluation used and left.  Reads only: no epoch bump, no allocation.
int st_get_anchor_terms(st_ctx* c, float* anchor_nchw, float* mask_hw, float* extra_nchw)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    const st_ctx::Anchor& A = c->anchor;
    if (!A.on) return fail(ST_ERR_STATE, "the anchor term is off");
    if (!A.evaluated)
        return fail(ST_ERR_STATE, A.resized ? "the input was resized after the last evaluation: the anchor term's buffers are those of the old size; evaluate again"
                                            : "no objective evaluation has completed with the anchor term on");
    if (mask_hw && !A.has_mask) return fail(ST_ERR_STATE, "the anchor term has no map (1 everywhere)");
    if (extra_nchw && !A.have_grad) return fail(ST_ERR_STATE, "the last evaluation computed no gradient: there is no plane of it");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (anchor_nchw) HIP_TRY(hipMemcpy(anchor_nchw, A.ax, A.plan.pixels * sizeof(float), hipMemcpyDeviceToHost));
    if (mask_hw) HIP_TRY(hipMemcpy(mask_hw, A.m, A.plan.plane * sizeof(float), hipMemcpyDeviceToHost));
    if (extra_nchw) HIP_TRY(hipMemcpy(extra_nchw, A.extra, A.plan.pixels * sizeof(float), hipMemcpyDeviceToHost));
    return ST_OK;
}

}  // extern "C"
