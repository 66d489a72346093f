// The photorealism term (include/st2.h: st_set_matting): its buffers, the per-window data it takes from the content image, its two
// launches inside an objective evaluation, and the C ABI around them.  matting_plan.h has the validation, the layout and the grids,
// matting.hip the kernels.
#include "engine.h"

namespace st2e {
namespace {
struct MatBufs { DevBuf<float> I, win, extra, part; };

int mat_alloc(const MatPlan& p, MatBufs& b)
{
    ST_TRY(b.I.alloc(p.pixels));
    ST_TRY(b.win.alloc(p.win_floats));
    ST_TRY(b.extra.alloc(p.pixels));
    ST_TRY(b.part.alloc((size_t)kMatPartRows * kMaxPartials));
    return ST_OK;
}

void mat_adopt(st_ctx::Matting& M, const MatPlan& p, MatBufs& b)
{
    M.I = std::move(b.I); M.win = std::move(b.win); M.extra = std::move(b.extra); M.part = std::move(b.part);
    M.plan = p;
    M.windows_ok = false; M.evaluated = false; M.have_grad = false;
}

// I, mu and M from the content image, which mat_preflight has found to be of the plan's size
int mat_windows(st_ctx* c)
{
    st_ctx::Matting& M = c->mat;
    const MatPlan& p = M.plan;
    MatWindowsArgs a{};
    a.I = M.I; a.win = M.win; a.H = p.H; a.W = p.W; a.Ww = p.Ww; a.windows = p.windows; a.off_mu = p.off_mu; a.off_M = p.off_M; a.eps = p.eps;
    ProfScope ps(c, P_MAT_SET, 0, 4.0 * (3.0 * (double)p.pixels + 9.0 * (double)p.windows));
    HIP_TRY(launch_mat_windows(c->content_x, M.I, p.pixels, a, c->stream));
    M.windows_ok = true;
    return ST_OK;
}

bool mat_fits(const st_ctx* c) { return c->x[0] && c->H >= 3 && c->W >= 3; }
}  // namespace

int mat_preflight(const st_ctx* c)
{
    if (!c->mat.on) return ST_OK;
    if (c->tile.on) return fail(ST_ERR_STATE, "the photorealism term does not run on a tile-configured context");
    if (!c->have_content || !c->content_x) return fail(ST_ERR_STATE, "the photorealism term needs a content image (st_set_content first)");
    if (c->x[0] && (c->cH != c->H || c->cW != c->W))
        return fail(ST_ERR_STATE, "the photorealism term needs a content image of the input's size: the content is %d x %d, the input %d x %d", c->cH, c->cW, c->H, c->W);
    if (c->x[0] && (c->H < 3 || c->W < 3))
        return fail(ST_ERR_STATE, "the photorealism term needs an input of at least 3 x 3 (a window is a 3 x 3 block inside the image): the input is %d x %d", c->H, c->W);
    return ST_OK;
}

void mat_input_resized(st_ctx* c)
{
    st_ctx::Matting& M = c->mat;
    if (M.evaluated) M.resized = true;
    M.evaluated = false; M.have_grad = false;
}

int mat_eval(st_ctx* c, const float* x, bool want_grad, const float* prev, const float** extra)
{
    st_ctx::Matting& M = c->mat;
    ST_TRY(mat_preflight(c));
    if (M.plan.H != c->H || M.plan.W != c->W || !M.win) {  // no buffers yet, or those of another size
        MatPlan p;
        const int bad = mat_plan(c->H, c->W, M.weight, M.eps, &p);
        if (bad) return fail(ST_ERR_STATE, "internal: photorealism plan: %s", mat_refusal_text(bad));
        HIP_TRY(hipStreamSynchronize(c->stream));          // (nothing queued reads the buffers that go)
        M.I.reset(); M.win.reset(); M.extra.reset(); M.part.reset();
        MatBufs fresh;
        ST_TRY(mat_alloc(p, fresh));
        mat_adopt(M, p, fresh);
    }
    const MatPlan& p = M.plan;
    M.evaluated = false; M.have_grad = false;
    if (!M.windows_ok) ST_TRY(mat_windows(c));             // the content image or the size changed since they were taken
    {
        MatFitArgs a{};
        a.x = x; a.I = M.I; a.win = M.win; a.ab = M.win + p.off_ab; a.part = M.part;
        a.H = p.H; a.W = p.W; a.Hw = p.Hw; a.Ww = p.Ww; a.tiles_x = p.fit_tiles_x; a.tiles = p.fit_tiles; a.windows = p.windows;
        a.off_mu = p.off_mu; a.off_M = p.off_M; a.eps = p.eps;
        ProfScope ps(c, P_MAT_FIT, 0, mat_fit_bytes(p));
        HIP_TRY(launch_mat_fit(a, p.fit_grid, c->stream));
        M.cnt_l = p.fit_grid; M.cnt_g = 0;
    }
    if (want_grad) {
        MatApplyArgs a{};
        a.x = x; a.I = M.I; a.win = M.win; a.ab = M.win + p.off_ab; a.prev = prev; a.extra = M.extra; a.part = M.part + kMaxPartials;
        a.H = p.H; a.W = p.W; a.Hw = p.Hw; a.Ww = p.Ww; a.tiles_x = p.apply_tiles_x; a.tiles = p.apply_tiles; a.windows = p.windows;
        a.off_mu = p.off_mu; a.w = p.w;
        ProfScope ps(c, P_MAT_APPLY, 0, mat_apply_bytes(p, prev != nullptr));
        HIP_TRY(launch_mat_apply(a, p.apply_grid, c->stream));
        M.cnt_g = p.apply_grid;
        *extra = M.extra;
    }
    M.evaluated = true; M.have_grad = want_grad; M.resized = false;
    return ST_OK;
}

int mat_trace(st_ctx* c, bool want_grad, int others, float* image_out)
{
    const st_ctx::Matting& M = c->mat;
    TraceMatArgs t{};
    t.part = M.part; t.count_l = M.cnt_l; t.count_g = want_grad ? M.cnt_g : 0; t.w = M.plan.w;
    t.image_n = (double)M.plan.pixels; t.have_grad = want_grad; t.others = others; t.image_out = image_out;
    HIP_TRY(launch_trace_mat(t, c->stream));
    return ST_OK;
}
}  // namespace st2e

extern "C" {

int st_set_matting(st_ctx* c, double weight, double eps)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    const int bad = mat_validate(weight, eps);
    if (bad) return fail(ST_ERR_ARG, "st_set_matting: %s", mat_refusal_text(bad));
    if (c->pipe.count) return fail(ST_ERR_STATE, "%d pipelined iteration(s) in flight: st_step_end before st_set_matting", c->pipe.count);
    if (weight != 0.0 && c->tile.on) return fail(ST_ERR_STATE, "the photorealism term does not run on a tile-configured context");
    HIP_TRY(hipSetDevice(c->device));
    st_ctx::Matting& M = c->mat;
    if (weight == 0.0) {     // off: every buffer of the term goes
        HIP_TRY(hipStreamSynchronize(c->stream));
        M = st_ctx::Matting{};
        return ST_OK;
    }
    MatPlan p{};
    MatBufs fresh;
    const bool now = mat_fits(c);
    if (now) {               // the buffers first: when that fails nothing has changed
        const int r = mat_plan(c->H, c->W, weight, eps, &p);
        if (r) return fail(ST_ERR_ARG, "st_set_matting: %s", mat_refusal_text(r));
        ST_TRY(mat_alloc(p, fresh));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    M = st_ctx::Matting{};
    M.on = true; M.weight = weight; M.eps = eps;
    if (now) {
        mat_adopt(M, p, fresh);
        if (mat_preflight(c) == ST_OK) ST_TRY(mat_windows(c));     // a content image of the input's size: the per-window data now
    }
    return ST_OK;
}

int st_get_matting(st_ctx* c, int* on, double* weight, double* eps)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    if (on) *on = c->mat.on;
    if (weight) *weight = c->mat.weight;
    if (eps) *eps = c->mat.eps;
    return ST_OK;
}

int st_get_trace_terms(st_ctx* c, int* laplacian, int* anchor, int* matting)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    if (laplacian) *laplacian = c->lap.n > 0;
    if (anchor) *anchor = c->anchor.on;
    if (matting) *matting = c->mat.on;
    return ST_OK;
}

// test hook: what the last evaluation used and left.  Reads only: no epoch bump, no allocation.
int st_get_matting_terms(st_ctx* c, float* mu, float* M_out, float* a_pb, float* extra_nchw)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    const st_ctx::Matting& M = c->mat;
    if (!M.on) return fail(ST_ERR_STATE, "the photorealism term is off");
    if (!M.evaluated)
        return fail(ST_ERR_STATE, M.resized ? "the input was resized after the last evaluation: the photorealism term's buffers are those of the old size; evaluate again"
                                            : "no objective evaluation has completed with the photorealism term on");
    if (extra_nchw && !M.have_grad) return fail(ST_ERR_STATE, "the last evaluation computed no gradient: there is no plane of it");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const MatPlan& p = M.plan;
    if (mu) HIP_TRY(hipMemcpy(mu, M.win + p.off_mu, 3 * p.windows * sizeof(float), hipMemcpyDeviceToHost));
    if (M_out) HIP_TRY(hipMemcpy(M_out, M.win + p.off_M, 6 * p.windows * sizeof(float), hipMemcpyDeviceToHost));
    if (a_pb) HIP_TRY(hipMemcpy(a_pb, M.win + p.off_ab, 12 * p.windows * sizeof(float), hipMemcpyDeviceToHost));
    if (extra_nchw) HIP_TRY(hipMemcpy(extra_nchw, M.extra, p.pixels * sizeof(float), hipMemcpyDeviceToHost));
    return ST_OK;
}

}  // extern "C"
