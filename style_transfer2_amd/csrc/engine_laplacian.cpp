// The Laplacian-steered content term (include/st2.h: st_set_laplacian): its buffers, its targets, its launches inside an objective
// evaluation, and the C ABI around them.  laplacian_plan.h has the geometry, laplacian.hip the kernels.
#include "engine.h"

namespace st2e {
namespace {
struct LapBufs { DevBuf<float> q, t, e, g, part; };

int lap_alloc(const LapPlan& p, LapBufs& b)
{
    ST_TRY(b.q.alloc(p.total)); ST_TRY(b.t.alloc(p.total)); ST_TRY(b.e.alloc(p.total));
    ST_TRY(b.g.alloc(p.pixels));
    ST_TRY(b.part.alloc((size_t)kLapPartRows * kMaxPartials));
    return ST_OK;
}

void lap_adopt(st_ctx::Lap& L, const LapPlan& p, LapBufs& b)
{
    L.q = std::move(b.q); L.t = std::move(b.t); L.e = std::move(b.e); L.g = std::move(b.g); L.part = std::move(b.part);
    L.plan = p;
    L.targets_ok = false; L.evaluated = false; L.have_grad = false;
}

// pool of `x` into q, then the stencil: the targets (target form) or E and its partial sums
int lap_pool_stencil(st_ctx* c, const float* x, bool target)
{
    st_ctx::Lap& L = c->lap;
    const LapPlan& p = L.plan;
    LapPoolArgs pa{};
    pa.x = x; pa.q = L.q; pa.H = p.H; pa.W = p.W; pa.n = p.n; pa.max_shift = p.max_shift; pa.tiles_y = p.tiles_y; pa.tiles_x = p.tiles_x;
    LapStencilArgs sa{};
    sa.q = L.q; sa.t = L.t; sa.e = target ? nullptr : L.e.get(); sa.part = L.part; sa.n = p.n;
    for (int l = 0; l < p.n; ++l) {
        pa.shift[l] = p.lv[l].shift; pa.hp[l] = sa.hp[l] = p.lv[l].hp; pa.wp[l] = sa.wp[l] = p.lv[l].wp; pa.off[l] = sa.off[l] = p.lv[l].off;
    }
    {
        ProfScope ps(c, P_LAP_POOL, 0, 4.0 * (double)(p.pixels + p.total));
        HIP_TRY(launch_lap_pool(pa, p.pool_grid, c->stream));
    }
    ProfScope ps(c, P_LAP_STENCIL, 0, 4.0 * (double)p.total * (target ? 2 : 3));
    HIP_TRY(launch_lap_stencil(sa, p.stencil_grid, c->stream));
    return ST_OK;
}
}  // namespace

int lap_preflight(const st_ctx* c)
{
    if (!c->lap.n) return ST_OK;
    if (c->tile.on) return fail(ST_ERR_STATE, "the Laplacian term does not run on a tile-configured context");
    if (!c->have_content || !c->content_x) return fail(ST_ERR_STATE, "the Laplacian term needs a content image (st_set_content first)");
    if (c->x[0] && (c->cH != c->H || c->cW != c->W))
        return fail(ST_ERR_STATE, "the Laplacian term needs a content image of the input's size: the content is %d x %d, the input %d x %d", c->cH, c->cW, c->H, c->W);
    return ST_OK;
}

void lap_input_resized(st_ctx* c)
{
    st_ctx::Lap& L = c->lap;
    if (L.evaluated) L.resized = true;
    L.evaluated = false; L.have_grad = false;
}

int lap_forward(st_ctx* c, const float* x)
{
    st_ctx::Lap& L = c->lap;
    ST_TRY(lap_preflight(c));
    if (L.plan.n != L.n || L.plan.H != c->H || L.plan.W != c->W || !L.q) {
        LapPlan p;
        const int bad = lap_plan(L.n, L.pool, L.weight, c->H, c->W, &p);
        if (bad) return fail(ST_ERR_STATE, "internal: Laplacian plan: %s", lap_refusal_text(bad));
        HIP_TRY(hipStreamSynchronize(c->stream));          // (nothing queued reads the buffers that go)
        L.q.reset(); L.t.reset(); L.e.reset(); L.g.reset(); L.part.reset();
        LapBufs fresh;
        ST_TRY(lap_alloc(p, fresh));
        lap_adopt(L, p, fresh);
    }
    L.evaluated = false; L.have_grad = false;
    if (!L.targets_ok) {                                   // the content image or the size changed since the targets were taken
        ST_TRY(lap_pool_stencil(c, c->content_x, true));
        L.targets_ok = true;
    }
    ST_TRY(lap_pool_stencil(c, x, false));
    L.cnt_e = L.plan.stencil_grid; L.cnt_g = 0;
    L.evaluated = true; L.resized = false;
    return ST_OK;
}

int lap_backward(st_ctx* c)
{
    st_ctx::Lap& L = c->lap;
    const LapPlan& p = L.plan;
    LapGradArgs ga{};
    ga.e = L.e; ga.g = L.g; ga.part = L.part + (size_t)kLapMaxLevels * kMaxPartials; ga.H = p.H; ga.W = p.W; ga.n = p.n;
    for (int l = 0; l < p.n; ++l) {
        ga.shift[l] = p.lv[l].shift; ga.hp[l] = p.lv[l].hp; ga.wp[l] = p.lv[l].wp; ga.off[l] = p.lv[l].off; ga.w[l] = p.lv[l].w;
    }
    const bool vec = p.row_vec && ((uintptr_t)L.g.get() & 15) == 0;
    ProfScope ps(c, P_LAP_GRAD, 0, 4.0 * (double)(p.pixels + p.total));
    HIP_TRY(launch_lap_grad(ga, p.grad_grid, p.grad_grid_vec, c->stream));
    L.cnt_g = vec ? p.grad_grid_vec : p.grad_grid;
    L.have_grad = true;
    return ST_OK;
}
}  // namespace st2e

extern "C" {

int st_set_laplacian(st_ctx* c, int n_levels, const int* pool, const double* weight)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    const int bad = lap_validate(n_levels, pool, weight);
    if (bad) return fail(ST_ERR_ARG, "st_set_laplacian: %s", lap_refusal_text(bad));
    if (c->pipe.count) return fail(ST_ERR_STATE, "%d pipelined iteration(s) in flight: st_step_end before st_set_laplacian", c->pipe.count);
    if (n_levels && c->tile.on) return fail(ST_ERR_STATE, "the Laplacian term does not run on a tile-configured context");
    HIP_TRY(hipSetDevice(c->device));
    st_ctx::Lap& L = c->lap;
    if (n_levels == 0) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        L = st_ctx::Lap{};
        return ST_OK;
    }
    LapPlan p{};
    LapBufs fresh;
    if (c->x[0]) {                                         // the buffers first: when that fails nothing has changed
        const int r = lap_plan(n_levels, pool, weight, c->H, c->W, &p);
        if (r) return fail(ST_ERR_ARG, "st_set_laplacian: %s", lap_refusal_text(r));
        ST_TRY(lap_alloc(p, fresh));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    L = st_ctx::Lap{};
    L.n = n_levels;
    for (int i = 0; i < n_levels; ++i) { L.pool[i] = pool[i]; L.weight[i] = weight[i]; }
    if (c->x[0]) {
        lap_adopt(L, p, fresh);
        if (lap_preflight(c) == ST_OK) {                   // a content image of the input's size: the targets now (else before the first evaluation)
            ST_TRY(lap_pool_stencil(c, c->content_x, true));
            L.targets_ok = true;
        }
    }
    return ST_OK;
}

int st_get_laplacian(st_ctx* c, int* n_levels, int* pool, double* weight)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    if (n_levels) *n_levels = c->lap.n;
    for (int i = 0; i < c->lap.n; ++i) {
        if (pool) pool[i] = c->lap.pool[i];
        if (weight) weight[i] = c->lap.weight[i];
    }
    return ST_OK;
}

// test hook: what the last evaluation left.  Reads only: no epoch bump, no allocation.
int st_get_laplacian_terms(st_ctx* c, int level, float* target, float* diff, float* grad_nchw)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    const st_ctx::Lap& L = c->lap;
    if (!L.n) return fail(ST_ERR_STATE, "the Laplacian term is off");
    if (level < 0 || level >= L.n) return fail(ST_ERR_ARG, "level %d of %d", level, L.n);
    if (!L.evaluated)
        return fail(ST_ERR_STATE, L.resized ? "the input was resized after the last evaluation: the Laplacian term's buffers are those of the old size; evaluate again"
                                            : "no objective evaluation has completed with the Laplacian term on");
    if (grad_nchw && !L.have_grad) return fail(ST_ERR_STATE, "the last evaluation computed no gradient: there is no g_lap of it");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const LapLevel& lv = L.plan.lv[level];
    if (target) HIP_TRY(hipMemcpy(target, L.t + lv.off, lv.cells * sizeof(float), hipMemcpyDeviceToHost));
    if (diff) HIP_TRY(hipMemcpy(diff, L.e + lv.off, lv.cells * sizeof(float), hipMemcpyDeviceToHost));
    if (grad_nchw) HIP_TRY(hipMemcpy(grad_nchw, L.g, L.plan.pixels * sizeof(float), hipMemcpyDeviceToHost));
    return ST_OK;
}

}  // extern "C"
