// Jitter (include/st2.h: st_set_jitter): the mode's buffers, its hooks inside an objective evaluation and the C ABI around them.
// jitter_plan.h has the validation, the shift sequence and the grids, jitter.hip the kernel.
#include "engine.h"

namespace st2e {
namespace {
// the shift the next evaluation uses, as drawn or given
void jitter_now(const st_ctx* c, int* dy, int* dx)
{
    const st_ctx::Jitter& J = c->jit;
    *dy = *dx = 0;
    if (!J.on) return;
    if (J.pinned) { *dy = J.pin_dy; *dx = J.pin_dx; return; }
    jitter_shift(J.seed, (uint64_t)J.k, J.radius, dy, dx);
}

// dst = roll(src, (dy, dx)) over (3, H, W), booked with the bytes it moves
int roll_enqueue(st_ctx* c, const float* src, float* dst, int H, int W, int dy, int dx)
{
    JitterPlan p{};
    const int bad = jitter_plan(H, W, dy, dx, &p);
    if (bad) return fail(ST_ERR_ARG, "jitter: %s", jitter_refusal_text(bad));
    ProfScope ps(c, P_MISC, 0, 8.0 * (double)p.pixels);
    HIP_TRY(launch_roll(src, dst, p, c->stream));
    return ST_OK;
}

bool has_content_row(const st_ctx* c)
{
    for (const ActiveLayer& al : c->active) if (al.c) return true;
    return false;
}

// Everything the two setters share once the arguments are checked.  The buffers are made first: when that fails nothing has changed.
int jitter_set(st_ctx* c, const char* who, bool on, int radius, unsigned long long seed, bool pinned, int dy, int dx)
{
    if (c->pipe.count) return fail(ST_ERR_STATE, "%d pipelined iteration(s) in flight: st_step_end before %s", c->pipe.count, who);
    if (on && c->tile.on) return fail(ST_ERR_STATE, "jitter does not run on a tile-configured context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));              // (nothing queued reads the buffers that go)
    st_ctx::Jitter& J = c->jit;
    if (!on) {               // off: every buffer of the mode goes; content features of another shift are dropped and taken again when next read
        if (!c->act.data.empty() && J.xs && c->act.data[0] == J.xs.get()) c->act.valid_to = -1;
        J = st_ctx::Jitter{};
        if (c->feat_dy || c->feat_dx) {
            for (auto& f : c->content_feat) f.reset();
            c->feat_dy = c->feat_dx = 0;
        }
        return ST_OK;
    }
    const size_t n3 = (size_t)3 * c->H * c->W;
    DevBuf<float> xs, g;
    const bool keep = J.on && J.xs.cap() == n3 && J.g.cap() == n3;
    if (c->x[0] && !keep) {
        ST_TRY(xs.alloc(n3));
        ST_TRY(g.alloc(n3));
    }
    if (!keep) {
        if (!c->act.data.empty() && J.xs && c->act.data[0] == J.xs.get()) c->act.valid_to = -1;
        J.xs = std::move(xs); J.g = std::move(g);
    }
    J.on = true; J.radius = radius; J.seed = seed; J.k = 0;
    J.pinned = pinned; J.pin_dy = dy; J.pin_dx = dx;
    J.evaluated = J.rolled = J.have_grad = J.resized = false;
    return ST_OK;
}
}  // namespace

int jitter_preflight(const st_ctx* c)
{
    if (c->jit.on && c->tile.on) return fail(ST_ERR_STATE, "jitter does not run on a tile-configured context");
    return ST_OK;
}

void jitter_input_resized(st_ctx* c)
{
    st_ctx::Jitter& J = c->jit;
    if (J.evaluated) J.resized = true;
    J.evaluated = J.rolled = J.have_grad = false;
}

void jitter_step_begun(st_ctx* c)
{
    if (c->jit.on) c->jit.k += 1;
}

// content_feat of the shift this evaluation uses.  With the mode off they are those of (0, 0) by construction (turning it off drops the
// others) and ensure_content_features fills what is missing, as ever.  With it on: features of another shift, or a missing one, are
// taken again from roll(content_x, s) by the forward content_from_device runs; nothing is launched when they are those of s already
int jitter_content(st_ctx* c)
{
    st_ctx::Jitter& J = c->jit;
    if (!J.on) return ensure_content_features(c);
    if (!has_content_row(c)) return ST_OK;
    if (!c->have_content || !c->content_x) return fail(ST_ERR_STATE, "content image missing");
    int dy, dx;
    jitter_now(c, &dy, &dx);
    const int rdy = jitter_reduce(dy, c->cH), rdx = jitter_reduce(dx, c->cW);
    bool missing = false;
    int deepest = -1;
    for (const ActiveLayer& al : c->active)
        if (al.c) { deepest = std::max(deepest, al.blob); missing = missing || !c->content_feat[al.blob]; }
    const bool other = rdy != c->feat_dy || rdx != c->feat_dx;
    if (!other && !missing) return ST_OK;
    const float* planes = c->content_x;
    if (rdy || rdx) {
        const size_t n3 = (size_t)3 * c->cH * c->cW;
        if (J.cxs.cap() != n3) ST_TRY(J.cxs.alloc(n3));
        ST_TRY(roll_enqueue(c, c->content_x, J.cxs, c->cH, c->cW, rdy, rdx));
        planes = J.cxs;
    }
    ST_TRY(act_ensure(c, c->act, c->cH, c->cW));
    if (deepest > 0) ST_TRY(forward_range(c, c->act, planes, deepest));
    for (const ActiveLayer& al : c->active) {
        const int b = al.blob;
        if (!al.c || (!other && c->content_feat[b])) continue;
        const size_t n = (size_t)c->act.C[b] * c->act.h[b] * c->act.w[b];
        if (!c->content_feat[b]) ST_TRY(c->content_feat[b].alloc(n));
        HIP_TRY(hipMemcpyAsync(c->content_feat[b], b == 0 ? planes : c->act.data[b], n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    }
    c->act.valid_to = -1;                      // (the activations are the content image's now)
    c->feat_dy = rdy; c->feat_dx = rdx;
    return ST_OK;
}

int jitter_roll_in(st_ctx* c, const float* x, bool want_grad, const float** xf)
{
    st_ctx::Jitter& J = c->jit;
    *xf = x;
    if (!J.on) return ST_OK;
    ST_TRY(jitter_preflight(c));
    jitter_now(c, &J.last_dy, &J.last_dx);
    J.last_H = c->H; J.last_W = c->W;
    J.evaluated = J.rolled = J.have_grad = false;
    J.scd_s = nullptr;
    if (c->active.empty()) { J.evaluated = true; J.resized = false; return ST_OK; }      // no network term: nothing is rolled
    const size_t n3 = (size_t)3 * c->H * c->W;
    if (J.xs.cap() != n3) ST_TRY(J.xs.alloc(n3));
    if (want_grad && J.g.cap() != n3) ST_TRY(J.g.alloc(n3));
    ST_TRY(roll_enqueue(c, x, J.xs, c->H, c->W, J.last_dy, J.last_dx));
    J.evaluated = J.rolled = true; J.resized = false;
    *xf = J.xs;
    return ST_OK;
}

int jitter_roll_out(st_ctx* c, const float** scd)
{
    st_ctx::Jitter& J = c->jit;
    if (!J.on || !J.rolled || !*scd) return ST_OK;
    const size_t n3 = (size_t)3 * c->H * c->W;
    if (J.g.cap() != n3) ST_TRY(J.g.alloc(n3));
    // unroll = roll by -s: negate the REDUCED shift (any int may be given; -INT_MIN is not one)
    ST_TRY(roll_enqueue(c, *scd, J.g, c->H, c->W, -jitter_reduce(J.last_dy, c->H), -jitter_reduce(J.last_dx, c->W)));
    J.have_grad = true;
    J.scd_s = *scd;
    *scd = J.g;
    return ST_OK;
}

int jitter_scd_sums(st_ctx* c)
{
    st_ctx::Jitter& J = c->jit;
    if (!J.on || !J.scd_s) return ST_OK;
    const float* planes = J.scd_s;
    J.scd_s = nullptr;
    ProfScope ps(c, P_FINALIZE, 0, 0);           // (a part of the trace's sums; P_MISC stays the class of the two moves)
    HIP_TRY(launch_roll_sumsq(planes, c->H, c->W, c->image_cnt, c->image_part + 2 * kMaxPartials, c->stream));
    return ST_OK;
}
}  // namespace st2e

extern "C" {

int st_set_jitter(st_ctx* c, int radius, unsigned long long seed)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    const int bad = jitter_validate_radius(radius);
    if (bad) return fail(ST_ERR_ARG, "st_set_jitter: %s, not %d", jitter_refusal_text(bad), radius);
    return jitter_set(c, "st_set_jitter", radius > 0, radius, seed, false, 0, 0);
}

int st_set_jitter_shift(st_ctx* c, int dy, int dx)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    return jitter_set(c, "st_set_jitter_shift", true, 0, 0, true, dy, dx);
}

int st_get_jitter(st_ctx* c, int* radius, unsigned long long* seed, long long* k, int* pinned, int* dy, int* dx)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    const st_ctx::Jitter& J = c->jit;
    int ndy, ndx;
    jitter_now(c, &ndy, &ndx);
    if (radius) *radius = J.radius;
    if (seed) *seed = J.seed;
    if (k) *k = J.k;
    if (pinned) *pinned = J.pinned;
    if (dy) *dy = ndy;
    if (dx) *dx = ndx;
    return ST_OK;
}

// test hook: what the last evaluation read and handed on.  Reads only: no epoch bump, no allocation.
int st_get_jitter_terms(st_ctx* c, float* xs_nchw, float* scd_nchw, int* dy, int* dx)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    const st_ctx::Jitter& J = c->jit;
    if (!J.on) return fail(ST_ERR_STATE, "jitter is off");
    if (!J.evaluated)
        return fail(ST_ERR_STATE, J.resized ? "the input was resized after the last evaluation: the jitter buffers are those of the old size; evaluate again"
                                            : "no objective evaluation has completed with jitter on");
    if ((xs_nchw || scd_nchw) && !J.rolled) return fail(ST_ERR_STATE, "the last evaluation had no active row: nothing was rolled");
    if (scd_nchw && !J.have_grad) return fail(ST_ERR_STATE, "the last evaluation computed no gradient: there is no network gradient of it");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t bytes = (size_t)3 * J.last_H * J.last_W * sizeof(float);
    if (xs_nchw) HIP_TRY(hipMemcpy(xs_nchw, J.xs, bytes, hipMemcpyDeviceToHost));
    if (scd_nchw) HIP_TRY(hipMemcpy(scd_nchw, J.g, bytes, hipMemcpyDeviceToHost));
    if (dy) *dy = J.last_dy;
    if (dx) *dx = J.last_dx;
    return ST_OK;
}

}  // extern "C"
