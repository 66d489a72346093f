// csrc/flow_plan.h on the host, alone (no HIP, no engine), under the address and undefined-behaviour sanitizers
// (tests/test_flow_plan_cpu.py builds and runs it).  Lines:
//   params <case> -> <refusal text>
//   image <case> -> <refusal text>
//   levels <H> <W> <asked> -> <n> <h0>x<w0> <h1>x<w1> ...
//   plan <H> <W> <is_u8> <route> -> <n> <total> <layout ok> <walk ok> <one_wg per level, finest first, as 0/1 digits> <launches>
//       layout ok: every region of the scratch buffer starts on a multiple of four floats, lies inside `total`, and no two overlap
//                  (checked by writing a tag over a buffer of exactly `total` floats and reading every region back)
//       walk ok:   the grid-stride walk of the form the launcher would take visits every pixel of every level once
//   big <H> <W> -> <n> <total> <grid of level 0> <grid_vec of level 0>
#include "../style_transfer2_amd/csrc/flow_plan.h"

#include <limits>
#include <stdio.h>
#include <vector>

using namespace st2;

struct Region { size_t off, n; };

static std::vector<Region> regions(const FlowPlan& p)
{
    std::vector<Region> r;
    for (int l = 0; l < p.n; ++l) {
        const FlowLevel& L = p.lv[l];
        for (size_t off : {L.raw[0], L.raw[1], L.img[0], L.img[1], L.u, L.v}) r.push_back({off, L.n});
    }
    const size_t n0 = p.lv[0].n;
    for (size_t off : {p.ix, p.iy, p.c, p.den, p.u2, p.v2}) r.push_back({off, n0});
    r.push_back({p.out, 2 * n0});
    r.push_back({p.stage[0], (p.stage_bytes + 3) / 4});
    r.push_back({p.stage[1], (p.stage_bytes + 3) / 4});
    return r;
}

static int layout_ok(const FlowPlan& p)
{
    std::vector<int> owner(p.total, -1);                   // exactly the size of the scratch buffer
    const std::vector<Region> rs = regions(p);
    for (size_t k = 0; k < rs.size(); ++k) {
        if (rs[k].off % 4 || rs[k].n < 1) return 0;
        for (size_t i = 0; i < rs[k].n; ++i) {
            int& o = owner.at(rs[k].off + i);
            if (o != -1) return 0;
            o = (int)k;
        }
    }
    if (p.stage_bytes != (size_t)3 * p.H * p.W * (p.is_u8 ? 1 : sizeof(float))) return 0;
    return 1;
}

static int walk_ok(const FlowPlan& p)
{
    for (int l = 0; l < p.n; ++l) {
        const FlowLevel& L = p.lv[l];
        if (L.n != (size_t)L.h * L.w || L.row_vec != (L.w % 4 == 0)) return 0;
        for (int form = 0; form < 2; ++form) {             // the scalar form; the 16-byte form where the rows allow it
            if (form && !L.row_vec) continue;
            const int px = form ? 4 : 1, grid = form ? L.grid_vec : L.grid;
            if (grid < 1 || grid > kFlowMaxBlocks || L.n % px) return 0;
            std::vector<unsigned char> seen(L.n, 0);
            const size_t n = L.n / px, stride = (size_t)grid * 256;
            for (size_t t = 0; t < stride && t < n; ++t)
                for (size_t i = t; i < n; i += stride)
                    for (int k = 0; k < px; ++k) seen.at(i * px + k) += 1;
            for (size_t i = 0; i < L.n; ++i) if (seen[i] != 1) return 0;
        }
        if (L.one_wg) {                                    // thread t of 1024 takes the pixels t + k 1024, k < 4
            if (L.n > (size_t)kFlowWgMaxPixels) return 0;
            std::vector<unsigned char> seen(L.n, 0);
            for (int t = 0; t < kFlowWgThreads; ++t)
                for (int k = 0; k < kFlowWgPerThread; ++k)
                    if ((size_t)(t + k * kFlowWgThreads) < L.n) seen.at(t + k * kFlowWgThreads) += 1;
            for (size_t i = 0; i < L.n; ++i) if (seen[i] != 1) return 0;
        }
        if (l + 1 < p.n && (p.lv[l + 1].h != (L.h + 1) / 2 || p.lv[l + 1].w != (L.w + 1) / 2)) return 0;
    }
    return 1;
}

static st_flow_params make(int levels, int warps, int iters, double alpha, int route)
{
    st_flow_params p;
    p.levels = levels; p.warps = warps; p.iters = iters; p.alpha = alpha; p.route = route;
    return p;
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    struct PCase { const char* name; st_flow_params p; };
    const PCase pcases[] = {
        {"defaults", flow_defaults()}, {"levels_-1", make(-1, 3, 40, 0.06, 0)}, {"levels_12", make(12, 3, 40, 0.06, 0)}, {"levels_13", make(13, 3, 40, 0.06, 0)},
        {"warps_0", make(0, 0, 40, 0.06, 0)}, {"warps_16", make(0, 16, 40, 0.06, 0)}, {"warps_17", make(0, 17, 40, 0.06, 0)},
        {"iters_0", make(0, 3, 0, 0.06, 0)}, {"iters_1000", make(0, 3, 1000, 0.06, 0)}, {"iters_1001", make(0, 3, 1001, 0.06, 0)},
        {"alpha_nan", make(0, 3, 40, nan, 0)}, {"alpha_inf", make(0, 3, 40, inf, 0)}, {"alpha_low", make(0, 3, 40, 0.9e-6, 0)},
        {"alpha_1e-6", make(0, 3, 40, 1e-6, 0)}, {"alpha_1e3", make(0, 3, 40, 1e3, 0)}, {"alpha_high", make(0, 3, 40, 1000.5, 0)},
        {"alpha_negative", make(0, 3, 40, -0.06, 0)}, {"route_1", make(0, 3, 40, 0.06, 1)}, {"route_2", make(0, 3, 40, 0.06, 2)}, {"route_-1", make(0, 3, 40, 0.06, -1)},
    };
    for (const PCase& c : pcases) printf("params %s -> %s\n", c.name, flow_refusal_text(flow_validate_params(c.p)));
    {
        const st_flow_params d = flow_defaults();
        printf("defaults %d %d %d %.17g %d\n", d.levels, d.warps, d.iters, d.alpha, d.route);
    }

    {
        std::vector<float> f(2 * 3 * 3, 17.5f);            // a 2 x 3 image, exactly
        std::vector<unsigned char> b(2 * 3 * 3, 200);
        const float finf = std::numeric_limits<float>::infinity(), fnan = std::numeric_limits<float>::quiet_NaN();
        printf("image null -> %s\n", flow_refusal_text(flow_validate_image(nullptr, 2, 3, 0)));
        printf("image u8 -> %s\n", flow_refusal_text(flow_validate_image(b.data(), 2, 3, 1)));
        printf("image finite -> %s\n", flow_refusal_text(flow_validate_image(f.data(), 2, 3, 0)));
        printf("image height_zero -> %s\n", flow_refusal_text(flow_validate_image(f.data(), 0, 3, 0)));
        printf("image width_negative -> %s\n", flow_refusal_text(flow_validate_image(f.data(), 2, -3, 0)));
        f[17] = fnan;
        printf("image nan_last -> %s\n", flow_refusal_text(flow_validate_image(f.data(), 2, 3, 0)));
        f[17] = -finf;
        printf("image negative_inf_last -> %s\n", flow_refusal_text(flow_validate_image(f.data(), 2, 3, 0)));
        f[17] = 1.f; f[0] = finf;
        printf("image inf_first -> %s\n", flow_refusal_text(flow_validate_image(f.data(), 2, 3, 0)));
    }

    const int sizes[][2] = {{1, 1}, {1, 9}, {7, 1}, {2, 2}, {5, 3}, {16, 16}, {31, 33}, {32, 32}, {33, 47}, {64, 64}, {65, 64}, {63, 100}, {96, 128}, {130, 70},
                            {32, 128}, {41, 100}, {512, 512}, {1024, 1024}, {1080, 1920}};
    for (const auto& s : sizes)
        for (int asked : {0, 1, 2, 5, 12}) {
            int hs[kFlowMaxLevels], ws[kFlowMaxLevels];
            const int n = flow_level_sizes(s[0], s[1], asked, hs, ws);
            printf("levels %d %d %d -> %d", s[0], s[1], asked, n);
            for (int l = 0; l < n; ++l) printf(" %dx%d", hs[l], ws[l]);
            printf("\n");
        }

    for (const auto& s : sizes)
        for (int is_u8 = 0; is_u8 < 2; ++is_u8)
            for (int route = 0; route < 2; ++route) {
                const st_flow_params par = make(0, 3, 40, 0.06, route);
                FlowPlan p;
                if (flow_plan(s[0], s[1], is_u8, &par, &p) != FLOW_OK || p.H != s[0] || p.W != s[1]) return 1;
                printf("plan %d %d %d %d -> %d %zu %d %d ", s[0], s[1], is_u8, route, p.n, p.total, layout_ok(p), walk_ok(p));
                for (int l = 0; l < p.n; ++l) printf("%d", p.lv[l].one_wg ? 1 : 0);
                printf(" %lld\n", flow_launches(p));
            }
    for (int H = 1; H <= 40; ++H)                          // every small size, both upload formats: layout and walks only
        for (int W = 1; W <= 40; ++W) {
            FlowPlan p;
            if (flow_plan(H, W, (H + W) & 1, nullptr, &p) != FLOW_OK || !layout_ok(p) || !walk_ok(p)) { printf("small_bad %d %d\n", H, W); return 1; }
        }
    printf("small_ok\n");
    {
        FlowPlan p;
        const st_flow_params bad = make(0, 3, 0, 0.06, 0);
        if (flow_plan(0, 5, 1, nullptr, &p) != FLOW_SIZE || flow_plan(5, 0, 1, nullptr, &p) != FLOW_SIZE || flow_plan(5, 5, 1, &bad, &p) != FLOW_ITERS) return 1;
        printf("plan_refused\n");
        // the single-workgroup bound: 4096 pixels are in, 4097 are out, whatever the shape
        const int edge[][2] = {{64, 64}, {1, 4096}, {4096, 1}, {1, 4097}, {4097, 1}, {64, 65}};
        for (const auto& e : edge) {
            const st_flow_params one = make(1, 3, 40, 0.06, 0);
            if (flow_plan(e[0], e[1], 1, &one, &p) != FLOW_OK) return 1;
            printf("bound %d %d -> %d\n", e[0], e[1], p.lv[0].one_wg ? 1 : 0);
        }
        // an 8192 x 8192 pair: sizes are size_t throughout, the grids stay inside their cap
        if (flow_plan(8192, 8192, 0, nullptr, &p) != FLOW_OK) return 1;
        printf("big 8192 8192 -> %d %zu %d %d\n", p.n, p.total, p.lv[0].grid, p.lv[0].grid_vec);
        if (flow_plan(70000, 70000, 1, nullptr, &p) != FLOW_OK) return 1;
        printf("big 70000 70000 -> %d %zu %d %d\n", p.n, p.total, p.lv[0].grid, p.lv[0].grid_vec);
    }
    return 0;
}
