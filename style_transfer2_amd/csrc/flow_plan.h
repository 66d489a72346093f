// Optical flow (include/st2.h: st_flow_estimate .. st_get_flow_level): validation of the parameters and the images, the level geometry
// (sizes, count, the layout of the block's one scratch buffer), the launch grids and the choice between the two Jacobi routes.  The
// engine (engine_flow.cpp) and the launchers (flow.hip) both ask here.  No HIP header: tests/flow_plan_host_main.cpp compiles this file
// alone, under the host sanitizers.
#pragma once
#include "anchor_plan.h"

namespace st2 {
constexpr int kFlowMaxLevels = 12;                         // levels of a pyramid at most
constexpr int kFlowAutoMinSide = 32;                       // levels = 0: a level is pooled while its shorter side is at least this
constexpr int kFlowMaxBlocks = 4096;                       // grid cap: the launches walk larger levels in a grid-stride loop
// the single-workgroup Jacobi route: 1024 threads of four pixels each; u and v ping-pong in 4 * 4096 floats = 64 KiB of LDS (what one
// workgroup may declare), the four coefficient planes are 16 registers of a thread
constexpr int kFlowWgThreads = 1024, kFlowWgPerThread = 4, kFlowWgMaxPixels = kFlowWgThreads * kFlowWgPerThread;

enum FlowRefusal { FLOW_OK = 0, FLOW_IMAGE, FLOW_SIZE, FLOW_LEVELS, FLOW_WARPS, FLOW_ITERS, FLOW_ALPHA, FLOW_ROUTE, FLOW_VALUE, FLOW_LEVEL };

inline const char* flow_refusal_text(int r)
{
    switch (r) {
    case FLOW_OK: return "ok";
    case FLOW_IMAGE: return "both images and the output are required";
    case FLOW_SIZE: return "the images must be at least 1 x 1";
    case FLOW_LEVELS: return "levels must be between 0 (automatic) and 12";
    case FLOW_WARPS: return "warps must be between 1 and 16";
    case FLOW_ITERS: return "iters must be between 1 and 1000";
    case FLOW_ALPHA: return "alpha must be finite and between 1e-6 and 1e3";
    case FLOW_ROUTE: return "route must be 0 (automatic) or 1 (one launch per iteration)";
    case FLOW_VALUE: return "every value of a float32 image must be finite";
    case FLOW_LEVEL: return "the last estimate has no such level";
    }
    return "?";
}

inline st_flow_params flow_defaults()
{
    st_flow_params p;
    p.levels = 0; p.warps = 3; p.iters = 40; p.alpha = 0.06; p.route = 0;
    return p;
}

inline int flow_validate_params(const st_flow_params& p)
{
    if (p.levels < 0 || p.levels > kFlowMaxLevels) return FLOW_LEVELS;
    if (p.warps < 1 || p.warps > 16) return FLOW_WARPS;
    if (p.iters < 1 || p.iters > 1000) return FLOW_ITERS;
    if (!isfinite(p.alpha) || p.alpha < 1e-6 || p.alpha > 1e3) return FLOW_ALPHA;
    if (p.route != 0 && p.route != 1) return FLOW_ROUTE;
    return FLOW_OK;
}

// an H x W x 3 image of the caller's: uint8 as it is, float32 scanned here on the host
inline int flow_validate_image(const void* hwc, int H, int W, int is_u8)
{
    if (!hwc) return FLOW_IMAGE;
    if (H < 1 || W < 1) return FLOW_SIZE;
    if (!is_u8) {
        const float* f = static_cast<const float*>(hwc);
        const size_t n = (size_t)H * W * 3;
        for (size_t i = 0; i < n; ++i)
            if (!isfinite(f[i])) return FLOW_VALUE;
    }
    return FLOW_OK;
}

// One level.  Offsets are in floats from the start of the scratch buffer, each a multiple of four (16 bytes).
struct FlowLevel {
    int h, w;
    size_t n;               // h * w
    size_t raw[2];          // the unsmoothed planes of `from` and `to` (what the next level is pooled from)
    size_t img[2];          // the smoothed planes A (from) and B (to)
    size_t u, v;            // the level's flow, finished when the level is (st_get_flow_level reads it)
    bool row_vec;           // w % 4 == 0: a group of four never straddles a row
    int grid, grid_vec;     // workgroups of 256: a thread takes one pixel, or four consecutive ones, per trip
    bool one_wg;            // the Jacobi iterations of a warp run in one launch of one workgroup
};

struct FlowPlan {
    int H, W, is_u8;
    st_flow_params par;     // as validated; levels still as asked
    float a2;               // float(alpha) * float(alpha)
    int n;                  // levels built
    FlowLevel lv[kFlowMaxLevels];
    size_t ix, iy, c, den;  // the linearisation of one warp (level-0 sized, every level uses the front)
    size_t u2, v2;          // the other half of the per-iteration route's ping-pong
    size_t out;             // (H, W, 2): the interleaved flow on its way out
    size_t stage[2];        // the caller's images on their way in, stage_bytes each
    size_t stage_bytes;     // H * W * 3 bytes or floats
    size_t total;           // floats of the scratch buffer
    int grid0;              // the interleaving launch: one (dx, dy) pair per thread and trip
};

inline size_t flow_align4(size_t n) { return (n + 3) & ~(size_t)3; }

// levels pooled from an H x W image: levels == 0 pools while min(h, w) >= 32 and fewer than 12 exist; levels == L pools L - 1 times and
// stops early at 1 x 1.  Writes the sizes, returns the count
inline int flow_level_sizes(int H, int W, int levels, int* hs, int* ws)
{
    int n = 1, h = H, w = W;
    hs[0] = h; ws[0] = w;
    while (n < kFlowMaxLevels) {
        if (levels == 0 ? (h < w ? h : w) < kFlowAutoMinSide : (n >= levels || (h == 1 && w == 1))) break;
        h = (h + 1) / 2; w = (w + 1) / 2;                  // Caffe's ceil mode at kernel 2, stride 2
        hs[n] = h; ws[n] = w;
        ++n;
    }
    return n;
}

inline int flow_plan(int H, int W, int is_u8, const st_flow_params* given, FlowPlan* out)
{
    if (H < 1 || W < 1) return FLOW_SIZE;
    const st_flow_params par = given ? *given : flow_defaults();
    const int bad = flow_validate_params(par);
    if (bad) return bad;
    FlowPlan p{};
    p.H = H; p.W = W; p.is_u8 = is_u8 ? 1 : 0; p.par = par;
    p.a2 = (float)par.alpha * (float)par.alpha;
    int hs[kFlowMaxLevels], ws[kFlowMaxLevels];
    p.n = flow_level_sizes(H, W, par.levels, hs, ws);
    size_t at = 0;
    auto take = [&at](size_t n) { const size_t o = at; at += flow_align4(n); return o; };
    for (int l = 0; l < p.n; ++l) {
        FlowLevel& L = p.lv[l];
        L.h = hs[l]; L.w = ws[l];
        L.n = (size_t)L.h * L.w;
        L.raw[0] = take(L.n); L.raw[1] = take(L.n);
        L.img[0] = take(L.n); L.img[1] = take(L.n);
        L.u = take(L.n); L.v = take(L.n);
        L.row_vec = L.w % 4 == 0;
        L.grid = anchor_grid(L.n, 256, kFlowMaxBlocks);
        L.grid_vec = anchor_grid(L.n / 4, 256, kFlowMaxBlocks);
        L.one_wg = par.route == 0 && L.n <= (size_t)kFlowWgMaxPixels;
    }
    const size_t n0 = p.lv[0].n;
    p.ix = take(n0); p.iy = take(n0); p.c = take(n0); p.den = take(n0);
    p.u2 = take(n0); p.v2 = take(n0);
    p.out = take(2 * n0);
    p.stage_bytes = 3 * n0 * (is_u8 ? 1 : sizeof(float));
    p.stage[0] = take((p.stage_bytes + 3) / 4);
    p.stage[1] = take((p.stage_bytes + 3) / 4);
    p.total = at;
    p.grid0 = p.lv[0].grid;
    *out = p;
    return FLOW_OK;
}

// launches of one estimate: per image pair luma, the pools, the smooths; per level the start of the flow, per warp the linearisation and
// the Jacobi launches; the interleave
inline long long flow_launches(const FlowPlan& p)
{
    long long n = 1 + (p.n - 1) + p.n + 1;
    for (int l = 0; l < p.n; ++l) n += 1 + (long long)p.par.warps * (1 + (p.lv[l].one_wg ? 1 : p.par.iters));
    return n;
}
}  // namespace st2
