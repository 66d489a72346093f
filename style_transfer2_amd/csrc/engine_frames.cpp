// Frame sequences (include/st2.h: st_frames_keep .. st_anchor_from_frame): the store of earlier iterates, and the one launch that warps
// a kept frame into the iterate or into the anchor.  frames_plan.h has the validation and the grids, frames.hip the kernel.  The
// anchor built here is the anchor term's own state (engine_anchor.cpp evaluates it): nothing of an evaluation lives in this file.
#include "engine.h"

namespace st2e {
namespace {
// what every call of the block but the getter refuses
int frames_refuse(const st_ctx* c, const char* who)
{
    if (c->pipe.count) return fail(ST_ERR_STATE, "%d pipelined iteration(s) in flight: st_step_end before %s", c->pipe.count, who);
    if (c->tile.on) return fail(ST_ERR_STATE, "%s: frame sequences do not run on a tile-configured context", who);
    return ST_OK;
}

// frame j against the store and the input
int frames_slot(const st_ctx* c, const char* who, int j)
{
    const st_ctx::Frames& F = c->frames;
    if (frames_validate_index(j, F.depth)) return fail(ST_ERR_ARG, "%s: %s (frame %d, depth %d)", who, frames_refusal_text(FRAMES_INDEX), j, F.depth);
    if (!c->x[0]) return fail(ST_ERR_STATE, "%s: no input image", who);
    if (j > F.count) return fail(ST_ERR_STATE, "%s: frame %d is empty: %d frame(s) of %d x %d kept, the input is %d x %d", who, j, F.count, F.H, F.W, c->H, c->W);
    if (F.H != c->H || F.W != c->W)
        return fail(ST_ERR_STATE, "%s: the kept frames are not of the input's size: the frames are %d x %d, the input %d x %d", who, F.H, F.W, c->H, c->W);
    return ST_OK;
}

// the caller's arrays into the staging buffer: [bwd 2 plane | fwd 2 plane | mask plane] (the segments of a W % 4 == 0 image start on
// 16-byte boundaries); the device pointers come back, NULL where the host pointer is
int frames_upload(st_ctx* c, const FramesPlan& p, const float* bwd, const float* fwd, const float* mask, const float** d_bwd, const float** d_fwd, const float** d_mask)
{
    st_ctx::Frames& F = c->frames;
    if (bwd || fwd || mask) ST_TRY(F.stage.reserve(5 * p.plane));
    float* base = F.stage;
    *d_bwd = *d_fwd = *d_mask = nullptr;
    if (bwd) { HIP_TRY(hipMemcpyAsync(base, bwd, 2 * p.plane * sizeof(float), hipMemcpyHostToDevice, c->stream)); *d_bwd = base; }
    if (fwd) { HIP_TRY(hipMemcpyAsync(base + 2 * p.plane, fwd, 2 * p.plane * sizeof(float), hipMemcpyHostToDevice, c->stream)); *d_fwd = base + 2 * p.plane; }
    if (mask) { HIP_TRY(hipMemcpyAsync(base + 4 * p.plane, mask, p.plane * sizeof(float), hipMemcpyHostToDevice, c->stream)); *d_mask = base + 4 * p.plane; }
    return ST_OK;
}

int frames_launch(st_ctx* c, const FramesPlan& p, const FramesArgs& a, int accumulate)
{
    const double P = (double)p.plane;              // flow in, four neighbours of the frame's planes in, planes out; with fwd: its neighbours in,
    const double floats = (a.bwd ? 2 + 12 : 3) * P + 3 * P + (a.fwd ? 8 * P : 0) + (a.mask ? P : 0) +      // the map out; accumulating: planes and map in
                          ((a.fwd || a.mask || accumulate) ? P : 0) + (accumulate ? 4 * P : 0);
    ProfScope ps(c, P_FRAMES, 0, 4.0 * floats);
    HIP_TRY(launch_frames(a, accumulate, p.grid, p.grid_vec, c->stream));
    return ST_OK;
}
}  // namespace
}  // namespace st2e

extern "C" {

int st_frames_keep(st_ctx* c, int depth)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    if (frames_validate_depth(depth)) return fail(ST_ERR_ARG, "st_frames_keep: %s, got %d", frames_refusal_text(FRAMES_DEPTH), depth);
    if (c->pipe.count) return fail(ST_ERR_STATE, "%d pipelined iteration(s) in flight: st_step_end before st_frames_keep", c->pipe.count);
    if (c->tile.on && depth) return fail(ST_ERR_STATE, "st_frames_keep: frame sequences do not run on a tile-configured context");
    st_ctx::Frames& F = c->frames;
    if (depth < F.depth) {                          // frames go: nothing queued may still read them
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (int i = depth; i < kFramesMaxDepth; ++i) F.slot[i].reset();
        F.count = std::min(F.count, depth);
        if (!depth) { F.stage.reset(); F.H = F.W = 0; }
    }
    F.depth = depth;
    return ST_OK;
}

int st_frame_push(st_ctx* c)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    ST_TRY(frames_refuse(c, "st_frame_push"));
    st_ctx::Frames& F = c->frames;
    if (!F.depth) return fail(ST_ERR_STATE, "st_frame_push: no frames are kept (st_frames_keep first)");
    if (!c->x[0]) return fail(ST_ERR_STATE, "st_frame_push: no input image");
    HIP_TRY(hipSetDevice(c->device));
    const size_t n3 = (size_t)3 * c->H * c->W;
    if (F.count && (F.H != c->H || F.W != c->W)) { // another size: the kept frames go first
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (auto& s : F.slot) s.reset();
        F.count = 0;
    }
    // the buffer of the new frame 1: the one that drops out at full depth, else a new one -- made before anything moves
    DevBuf<float> top;
    if (F.count == F.depth) top = std::move(F.slot[F.depth - 1]);
    else ST_TRY(top.alloc(n3));
    for (int i = std::min(F.count, F.depth - 1); i >= 1; --i) F.slot[i] = std::move(F.slot[i - 1]);
    F.slot[0] = std::move(top);
    F.count = std::min(F.count + 1, F.depth);
    F.H = c->H; F.W = c->W;
    HIP_TRY(hipMemcpyAsync(F.slot[0], c->x[c->cur], n3 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));      // (st_set_input_nchw writes x outside the stream)
    return ST_OK;
}

// reads only: no epoch bump, no refusal
int st_get_frames(st_ctx* c, int* depth, int* count, int* H, int* W)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    const st_ctx::Frames& F = c->frames;
    if (depth) *depth = F.depth;
    if (count) *count = F.count;
    if (H) *H = F.count ? F.H : 0;
    if (W) *W = F.count ? F.W : 0;
    return ST_OK;
}

int st_set_input_from_frame(st_ctx* c, int j, const float* bwd_flow_hw2)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    const char* who = "st_set_input_from_frame";
    ST_TRY(frames_refuse(c, who));
    ST_TRY(frames_slot(c, who, j));
    const int bad = frames_validate_flow(c->H, c->W, bwd_flow_hw2);
    if (bad) return fail(ST_ERR_ARG, "%s: %s", who, frames_refusal_text(bad));
    HIP_TRY(hipSetDevice(c->device));
    FramesPlan p{};
    if (frames_plan(c->H, c->W, &p)) return fail(ST_ERR_ARG, "%s: %s", who, frames_refusal_text(FRAMES_SIZE));
    const float *d_bwd, *d_fwd, *d_mask;
    ST_TRY(frames_upload(c, p, bwd_flow_hw2, nullptr, nullptr, &d_bwd, &d_fwd, &d_mask));
    // what st_set_input_nchw does around its copy (the size is the input's: nothing is re-made)
    ST_TRY(set_input_common(c, c->H, c->W));
    iterate_overwritten(c);
    c->avg_items = 0;        // a new iterate: its running mean starts empty
    const float* src = c->frames.slot[j - 1];
    if (!d_bwd) HIP_TRY(hipMemcpyAsync(c->x[c->cur], src, p.pixels * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    else {
        FramesArgs a{};
        a.src = src; a.bwd = d_bwd; a.dst = c->x[c->cur]; a.H = p.H; a.W = p.W; a.plane = p.plane;
        ST_TRY(frames_launch(c, p, a, 0));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));      // (the host array is the caller's again)
    return ST_OK;
}

int st_anchor_from_frame(st_ctx* c, int j, const float* bwd_flow_hw2, const float* fwd_flow_hw2, const float* mask_hw, double weight, int accumulate)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    const char* who = "st_anchor_from_frame";
    ST_TRY(frames_refuse(c, who));
    ST_TRY(frames_slot(c, who, j));
    const int H = c->H, W = c->W;
    const int bad = anchor_validate(H, W, mask_hw, weight);
    if (bad) return fail(ST_ERR_ARG, "%s: %s", who, anchor_refusal_text(bad));
    for (const float* flow : {bwd_flow_hw2, fwd_flow_hw2}) {
        const int r = frames_validate_flow(H, W, flow);
        if (r) return fail(ST_ERR_ARG, "%s: %s", who, frames_refusal_text(r));
    }
    st_ctx::Anchor& A = c->anchor;
    if (accumulate) {
        if (!A.on || !A.has_mask)
            return fail(ST_ERR_STATE, "%s: accumulating needs the anchor term on with a map (%s)", who, A.on ? "the anchor has no map" : "the term is off");
        if (A.plan.H != H || A.plan.W != W)
            return fail(ST_ERR_STATE, "%s: accumulating needs an anchor of the input's size: the anchor is %d x %d, the input %d x %d", who, A.plan.H, A.plan.W, H, W);
        if (weight != A.weight) return fail(ST_ERR_ARG, "%s: accumulating keeps the weight in force, %.17g, got %.17g", who, A.weight, weight);
    }
    HIP_TRY(hipSetDevice(c->device));
    FramesPlan p{};
    AnchorPlan ap{};
    if (frames_plan(H, W, &p) || anchor_plan(H, W, weight, &ap)) return fail(ST_ERR_ARG, "%s: %s", who, frames_refusal_text(FRAMES_SIZE));
    const float *d_bwd, *d_fwd, *d_mask;
    ST_TRY(frames_upload(c, p, bwd_flow_hw2, fwd_flow_hw2, mask_hw, &d_bwd, &d_fwd, &d_mask));
    FramesArgs a{};
    a.src = c->frames.slot[j - 1]; a.bwd = d_bwd; a.fwd = d_fwd; a.mask = d_mask; a.H = H; a.W = W; a.plane = p.plane;
    if (accumulate) {
        a.dst = A.ax; a.map = A.m;
        ST_TRY(frames_launch(c, p, a, 1));
        HIP_TRY(hipStreamSynchronize(c->stream));
        A.evaluated = A.have_grad = A.resized = false;     // `extra` is that of another anchor
        return ST_OK;
    }
    // the buffers of st_set_anchor_nchw, made and filled first: when that fails nothing has changed
    const bool has_map = fwd_flow_hw2 || mask_hw;
    DevBuf<float> ax, m, extra, part;
    ST_TRY(ax.alloc(ap.pixels));
    if (has_map) ST_TRY(m.alloc(ap.plane));
    ST_TRY(extra.alloc(ap.pixels));
    ST_TRY(part.alloc((size_t)kAnchorPartRows * kMaxPartials));
    a.dst = ax; a.map = has_map ? m.get() : nullptr;
    ST_TRY(frames_launch(c, p, a, 0));
    HIP_TRY(hipStreamSynchronize(c->stream));              // (the host arrays are the caller's again; nothing queued reads the buffers that go)
    A = st_ctx::Anchor{};
    A.on = true; A.weight = weight; A.has_mask = has_map; A.plan = ap;
    A.ax = std::move(ax); A.m = std::move(m); A.extra = std::move(extra); A.part = std::move(part);
    return ST_OK;
}

}  // extern "C"
