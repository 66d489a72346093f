// csrc/anchor_plan.h on the host, alone (no HIP, no engine), under the address and undefined-behaviour sanitizers
// (tests/test_anchor_plan_cpu.py builds and runs it).  Lines:
//   validate <case> -> <refusal text>
//   plan <H> <W> -> <plane> <pixels> <row_vec> <grid> <grid_vec> <covered>      covered: 1 when the grid-stride walk of the form the
//                                                     launcher would take visits every pixel of a buffer of exactly `plane` floats once
//   big <plane> <pixels> <grid> <grid_vec>
#include "../style_transfer2_amd/csrc/anchor_plan.h"

#include <limits>
#include <stdio.h>
#include <vector>

using namespace st2;

// the walk of anchor_k: thread t of `grid` workgroups of 256 takes groups t, t + grid * 256, ... of px pixels
static int covered(const AnchorPlan& p)
{
    const int px = p.row_vec ? 4 : 1;
    const int grid = p.row_vec ? p.grid_vec : p.grid;
    if (grid < 1 || grid > kAnchorMaxBlocks || p.plane % px) return 0;
    std::vector<unsigned char> seen(p.plane, 0);           // exactly the size of the map
    const size_t n = p.plane / px, stride = (size_t)grid * 256;
    for (size_t t = 0; t < stride; ++t)
        for (size_t i = t; i < n; i += stride)
            for (int k = 0; k < px; ++k) seen.at(i * px + k) += 1;
    for (size_t i = 0; i < p.plane; ++i) if (seen[i] != 1) return 0;
    return 1;
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const double dinf = std::numeric_limits<double>::infinity(), dnan = std::numeric_limits<double>::quiet_NaN();
    std::vector<float> good(6, 0.5f);                       // a 2 x 3 map, exactly
    good[0] = 0.f; good[5] = 7.5f;
    struct Case { const char* name; int H, W; double w; int map; float poke; };      // map: 0 none, 1 good, 2 good with good[4] = poke
    const Case cases[] = {
        {"no_map", 2, 3, 1.5, 0, 0.f},
        {"map", 2, 3, -1.3, 1, 0.f},
        {"map_with_zero_and_large", 2, 3, 250, 2, 1e30f},
        {"map_negative_zero", 2, 3, 1, 2, -0.f},
        {"weight_zero", 2, 3, 0.0, 1, 0.f},
        {"weight_negative_zero", 2, 3, -0.0, 1, 0.f},
        {"weight_nan", 2, 3, dnan, 1, 0.f},
        {"weight_inf", 2, 3, dinf, 1, 0.f},
        {"weight_negative_inf", 2, 3, -dinf, 0, 0.f},
        {"weight_underflows_float", 2, 3, 1e-60, 0, 0.f},
        {"weight_overflows_float", 2, 3, 1e60, 0, 0.f},
        {"height_zero", 0, 3, 1, 0, 0.f},
        {"width_zero", 2, 0, 1, 0, 0.f},
        {"height_negative", -2, 3, 1, 0, 0.f},
        {"map_negative", 2, 3, 1, 2, -1e-30f},
        {"map_nan", 2, 3, 1, 2, nan},
        {"map_inf", 2, 3, 1, 2, inf},
        {"map_negative_inf", 2, 3, 1, 2, -inf},
        {"weight_before_map", 2, 3, 0.0, 2, nan},
    };
    for (const Case& c : cases) {
        std::vector<float> m = good;
        if (c.map == 2) m[4] = c.poke;
        printf("validate %s -> %s\n", c.name, anchor_refusal_text(anchor_validate(c.H, c.W, c.map ? m.data() : nullptr, c.w)));
    }

    for (int H = 1; H <= 70; ++H)
        for (int W = 1; W <= 70; ++W) {
            AnchorPlan p;
            if (anchor_plan(H, W, 0.7, &p) != ANCHOR_OK || p.H != H || p.W != W || p.w != 0.7f) return 1;
            printf("plan %d %d -> %zu %zu %d %d %d %d\n", H, W, p.plane, p.pixels, p.row_vec ? 1 : 0, p.grid, p.grid_vec, covered(p));
        }
    {
        AnchorPlan p;
        if (anchor_plan(0, 5, 1.0, &p) != ANCHOR_SIZE || anchor_plan(5, 0, 1.0, &p) != ANCHOR_SIZE || anchor_plan(5, 5, 0.0, &p) != ANCHOR_WEIGHT) return 1;
        printf("plan_refused\n");
        // a large image: the grids stay inside their cap and the sizes do not wrap
        if (anchor_plan(40000, 40000, 1.0, &p) != ANCHOR_OK) return 1;
        printf("big %zu %zu %d %d\n", p.plane, p.pixels, p.grid, p.grid_vec);
    }
    return 0;
}
