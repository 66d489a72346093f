// Optical flow (include/st2.h: st_flow_estimate .. st_get_flow_level): the block's scratch buffer and the launch sequence of one
// estimate.  flow_plan.h has the validation, the level geometry and the route, flow.hip the kernels.  Nothing of the iterate, the
// optimizer, the anchor, the kept frames or the activations is read or written here, and no call bumps the epoch.
#include "engine.h"

namespace st2e {
namespace {
int flow_run(st_ctx* c, const FlowPlan& p, float* base)
{
    hipStream_t s = c->stream;
    const double f4 = sizeof(float);
    {   // both pyramids, then every level smoothed from its unsmoothed planes
        const double n0 = (double)p.lv[0].n;
        ProfScope ps(c, P_FLOW_PREP, 0, 2 * ((double)p.stage_bytes + f4 * n0));
        HIP_TRY(launch_flow_luma(p, base, s));
    }
    for (int l = 0; l + 1 < p.n; ++l) {
        ProfScope ps(c, P_FLOW_PREP, 0, 2 * f4 * ((double)p.lv[l].n + (double)p.lv[l + 1].n));
        HIP_TRY(launch_flow_pool(p, base, l, s));
    }
    for (int l = 0; l < p.n; ++l) {
        ProfScope ps(c, P_FLOW_PREP, 0, 2 * f4 * 2 * (double)p.lv[l].n);
        HIP_TRY(launch_flow_smooth(p, base, l, s));
    }
    for (int l = p.n - 1; l >= 0; --l) {
        const FlowLevel& L = p.lv[l];
        const double n = (double)L.n;
        {
            ProfScope ps(c, P_FLOW_PREP, 0, f4 * (2 * n + (l + 1 < p.n ? 2 * (double)p.lv[l + 1].n : 0)));
            HIP_TRY(launch_flow_start(p, base, l, s));
        }
        float *u = base + L.u, *v = base + L.v, *un = base + p.u2, *vn = base + p.v2;
        for (int k = 0; k < p.par.warps; ++k) {
            {   // A, B, u, v in (the gathers follow the flow: once each where it is smooth); four planes out
                ProfScope ps(c, P_FLOW_LINEAR, 0, f4 * 8 * n);
                HIP_TRY(launch_flow_linear(p, base, l, u, v, s));
            }
            if (L.one_wg) {
                ProfScope ps(c, P_FLOW_JACOBI_WG, 0, f4 * 8 * n);
                HIP_TRY(launch_flow_jacobi_wg(p, base, l, u, v, s));
            } else {
                for (int it = 0; it < p.par.iters; ++it) {
                    ProfScope ps(c, P_FLOW_JACOBI, 0, f4 * 8 * n);       // u, v and the four coefficient planes in, u', v' out
                    HIP_TRY(launch_flow_jacobi(p, base, l, u, v, un, vn, s));
                    std::swap(u, un); std::swap(v, vn);
                }
            }
        }
        if (u != base + L.u) {                             // an odd number of launches: the level's flow sits in the other half
            HIP_TRY(hipMemcpyAsync(base + L.u, u, L.n * sizeof(float), hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(base + L.v, v, L.n * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
    }
    ProfScope ps(c, P_FLOW_PREP, 0, f4 * 4 * (double)p.lv[0].n);
    HIP_TRY(launch_flow_interleave(base + p.lv[0].u, base + p.lv[0].v, base + p.out, p.lv[0].n, p.grid0, s));
    return ST_OK;
}
}  // namespace
}  // namespace st2e

extern "C" {

int st_flow_estimate(st_ctx* c, const void* from_hwc, const void* to_hwc, int H, int W, int is_u8, const st_flow_params* params, float* out_flow_hw2)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    const char* who = "st_flow_estimate";
    if (!from_hwc || !to_hwc || !out_flow_hw2) return fail(ST_ERR_ARG, "%s: %s", who, flow_refusal_text(FLOW_IMAGE));
    FlowPlan p{};
    int bad = flow_plan(H, W, is_u8, params, &p);
    if (bad) return fail(ST_ERR_ARG, "%s: %s (%d x %d)", who, flow_refusal_text(bad), H, W);
    for (const void* image : {from_hwc, to_hwc})
        if ((bad = flow_validate_image(image, H, W, is_u8))) return fail(ST_ERR_ARG, "%s: %s", who, flow_refusal_text(bad));
    if (c->pipe.count) return fail(ST_ERR_STATE, "%d pipelined iteration(s) in flight: st_step_end before %s", c->pipe.count, who);
    HIP_TRY(hipSetDevice(c->device));
    st_ctx::Flow& F = c->flow;
    if (p.total > F.scratch.cap()) {                       // the larger buffer first: when that fails nothing has changed
        DevBuf<float> grown;
        ST_TRY(grown.alloc(p.total));
        F.scratch = std::move(grown);                      // (every estimate has waited for its launches: nothing queued reads the old one)
    }
    F.have = false;                                        // the levels of the last estimate are being overwritten
    float* base = F.scratch;
    HIP_TRY(hipMemcpyAsync(base + p.stage[0], from_hwc, p.stage_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(base + p.stage[1], to_hwc, p.stage_bytes, hipMemcpyHostToDevice, c->stream));
    ST_TRY(flow_run(c, p, base));
    HIP_TRY(hipMemcpyAsync(out_flow_hw2, base + p.out, 2 * p.lv[0].n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    F.plan = p;
    F.have = true;
    return ST_OK;
}

int st_flow_release(st_ctx* c)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    c->flow.scratch.reset();                               // (every estimate has waited for its launches)
    c->flow.have = false;
    return ST_OK;
}

// reads only: no epoch bump
int st_get_flow_level(st_ctx* c, int level, int* h, int* w, float* from_l, float* to_l, float* flow_l_hw2)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    const st_ctx::Flow& F = c->flow;
    if (!F.have || !F.scratch) return fail(ST_ERR_STATE, "st_get_flow_level: no estimate to read (none yet, or st_flow_release since)");
    if (level < 0 || level >= F.plan.n) return fail(ST_ERR_ARG, "st_get_flow_level: %s (level %d of %d)", flow_refusal_text(FLOW_LEVEL), level, F.plan.n);
    const FlowLevel& L = F.plan.lv[level];
    if (h) *h = L.h;
    if (w) *w = L.w;
    if (!from_l && !to_l && !flow_l_hw2) return ST_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const float* base = F.scratch;
    if (from_l) HIP_TRY(hipMemcpy(from_l, base + L.img[0], L.n * sizeof(float), hipMemcpyDeviceToHost));
    if (to_l) HIP_TRY(hipMemcpy(to_l, base + L.img[1], L.n * sizeof(float), hipMemcpyDeviceToHost));
    if (flow_l_hw2) {
        std::vector<float> uv(2 * L.n);
        HIP_TRY(hipMemcpy(uv.data(), base + L.u, L.n * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(uv.data() + L.n, base + L.v, L.n * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < L.n; ++i) { flow_l_hw2[2 * i] = uv[i]; flow_l_hw2[2 * i + 1] = uv[L.n + i]; }
    }
    return ST_OK;
}

}  // extern "C"
