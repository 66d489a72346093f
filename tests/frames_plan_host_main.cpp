// csrc/frames_plan.h on the host, alone (no HIP, no engine), under the address and undefined-behaviour sanitizers
// (tests/test_frames_plan_cpu.py builds and runs it).  Lines:
//   depth <d> -> <refusal text>
//   index <j> <depth> -> <refusal text>
//   flow <case> -> <refusal text>
//   plan <H> <W> -> <plane> <pixels> <row_vec> <grid> <grid_vec> <covered>      covered: 1 when the grid-stride walk of the form the
//                                                     launcher would take visits every pixel of a buffer of exactly `plane` floats once
//   big <plane> <pixels> <grid> <grid_vec> <last offset of the walk>
#include "../style_transfer2_amd/csrc/frames_plan.h"

#include <limits>
#include <stdio.h>
#include <vector>

using namespace st2;

// the walk of frames_k: thread t of `grid` workgroups of 256 takes groups t, t + grid * 256, ... of px pixels
static int covered(const FramesPlan& p)
{
    const int px = p.row_vec ? 4 : 1;
    const int grid = p.row_vec ? p.grid_vec : p.grid;
    if (grid < 1 || grid > kFramesMaxBlocks || p.plane % px) return 0;
    std::vector<unsigned char> seen(p.plane, 0);           // exactly the size of a map
    const size_t n = p.plane / px, stride = (size_t)grid * 256;
    for (size_t t = 0; t < stride; ++t)
        for (size_t i = t; i < n; i += stride)
            for (int k = 0; k < px; ++k) {
                const size_t at = i * px + k;
                const int y = (int)(at / (size_t)p.W), x = (int)(at - (size_t)y * p.W);
                if (y < 0 || y >= p.H || x < 0 || x >= p.W) return 0;
                seen.at(at) += 1;
            }
    for (size_t i = 0; i < p.plane; ++i) if (seen[i] != 1) return 0;
    return 1;
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int d = -1; d <= 9; ++d) printf("depth %d -> %s\n", d, frames_refusal_text(frames_validate_depth(d)));
    const int pairs[][2] = {{0, 8}, {1, 8}, {8, 8}, {9, 8}, {-1, 8}, {1, 1}, {2, 1}, {1, 0}};
    for (const auto& p : pairs) printf("index %d %d -> %s\n", p[0], p[1], frames_refusal_text(frames_validate_index(p[0], p[1])));

    std::vector<float> good(2 * 3 * 2, 0.25f);              // a 2 x 3 flow, exactly
    good[0] = -1e30f; good[11] = 3e38f;
    struct Case { const char* name; int H, W; int flow; float poke; };      // flow: 0 none, 1 good, 2 good with its last value = poke
    const Case cases[] = {
        {"none", 2, 3, 0, 0.f}, {"finite", 2, 3, 1, 0.f}, {"negative_zero", 2, 3, 2, -0.f}, {"nan_last", 2, 3, 2, nan}, {"inf_last", 2, 3, 2, inf},
        {"negative_inf_last", 2, 3, 2, -inf}, {"height_zero", 0, 3, 0, 0.f}, {"width_negative", 2, -3, 0, 0.f},
    };
    for (const Case& c : cases) {
        std::vector<float> f = good;
        if (c.flow == 2) f[11] = c.poke;
        printf("flow %s -> %s\n", c.name, frames_refusal_text(frames_validate_flow(c.H, c.W, c.flow ? f.data() : nullptr)));
    }
    {
        std::vector<float> f = good;
        f[0] = nan;
        printf("flow nan_first -> %s\n", frames_refusal_text(frames_validate_flow(2, 3, f.data())));
    }

    for (int H = 1; H <= 70; ++H)
        for (int W = 1; W <= 70; ++W) {
            FramesPlan p;
            if (frames_plan(H, W, &p) != FRAMES_OK || p.H != H || p.W != W) return 1;
            printf("plan %d %d -> %zu %zu %d %d %d %d\n", H, W, p.plane, p.pixels, p.row_vec ? 1 : 0, p.grid, p.grid_vec, covered(p));
        }
    {
        FramesPlan p;
        if (frames_plan(0, 5, &p) != FRAMES_SIZE || frames_plan(5, 0, &p) != FRAMES_SIZE) return 1;
        printf("plan_refused\n");
        // an 8192 x 8192 image: the grids stay inside their cap, and the last element the walk of three planes touches is the last one
        if (frames_plan(8192, 8192, &p) != FRAMES_OK) return 1;
        const size_t n = p.plane / 4, stride = (size_t)p.grid_vec * 256;
        size_t last = 0;
        for (size_t i = (n - 1) % stride; i < n; i += stride) last = i;     // the trips of the thread that takes the last group
        printf("big %zu %zu %d %d %zu\n", p.plane, p.pixels, p.grid, p.grid_vec, 2 * p.plane + last * 4 + 3);
        // ... and a size whose pixel count does not fit 32 bits
        if (frames_plan(70000, 70000, &p) != FRAMES_OK) return 1;
        printf("huge %zu %zu %d %d\n", p.plane, p.pixels, p.grid, p.grid_vec);
    }
    return 0;
}
