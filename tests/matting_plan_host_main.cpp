// Stand-alone host program around csrc/matting_plan.h (no HIP): built by tests/test_matting_plan_cpu.py with
// -fsanitize=address,undefined and run there.  It prints every validation refusal and, per size, the plan and a walk of both passes'
// tile loops as the kernels make it: every cell marked in a buffer of exactly the planned size (small sizes), or counted (8192 x 8192).
#include "../style_transfer2_amd/csrc/matting_plan.h"

#include <limits>
#include <stdio.h>
#include <vector>

using namespace st2;

static void validate(const char* name, double w, double eps) { printf("validate %s -> %s\n", name, mat_refusal_text(mat_validate(w, eps))); }

// the tile loop of a pass over cells_y x cells_x cells: block b takes tiles b, b + grid, ...; thread t the cell (t / kMatTileW, t % kMatTileW).
// Returns the number of cells visited; marks them (seen != NULL) and counts double visits and visits outside the buffer in *bad
static size_t walk(int cells_y, int cells_x, int tiles_x, size_t tiles, int grid, std::vector<unsigned char>* seen, size_t* bad, size_t* last)
{
    size_t visited = 0;
    for (int b = 0; b < grid; ++b)
        for (size_t t = (size_t)b; t < tiles; t += (size_t)grid) {
            const int y0 = (int)(t / tiles_x) * kMatTileH, x0 = (int)(t % tiles_x) * kMatTileW;
            if (seen) {
                for (int th = 0; th < kMatThreads; ++th) {
                    const int y = y0 + th / kMatTileW, x = x0 + th % kMatTileW;
                    if (y >= cells_y || x >= cells_x) continue;
                    const size_t k = (size_t)y * cells_x + x;
                    if (k >= seen->size() || (*seen)[k]) { ++*bad; continue; }
                    (*seen)[k] = 1;
                    if (k > *last) *last = k;
                    ++visited;
                }
            } else {                                       // counted: the part of the tile inside the cells
                if (y0 >= cells_y || x0 >= cells_x) { ++*bad; continue; }
                const size_t h = (size_t)(cells_y - y0 < kMatTileH ? cells_y - y0 : kMatTileH), w = (size_t)(cells_x - x0 < kMatTileW ? cells_x - x0 : kMatTileW);
                visited += h * w;
                const size_t k = (size_t)(y0 + (int)h - 1) * cells_x + (x0 + (int)w - 1);
                if (k > *last) *last = k;
            }
        }
    return visited;
}

static void plan(int H, int W, bool mark)
{
    MatPlan p;
    const int r = mat_plan(H, W, 1e4, 1e-7, &p);
    if (r) { printf("plan %d %d -> refused: %s\n", H, W, mat_refusal_text(r)); return; }
    size_t bad = 0, last_w = 0, last_p = 0;
    std::vector<unsigned char> win(mark ? p.windows : 0), pix(mark ? p.plane : 0);
    const size_t vw = walk(p.Hw, p.Ww, p.fit_tiles_x, p.fit_tiles, p.fit_grid, mark ? &win : nullptr, &bad, &last_w);
    const size_t vp = walk(p.H, p.W, p.apply_tiles_x, p.apply_tiles, p.apply_grid, mark ? &pix : nullptr, &bad, &last_p);
    // the last float each pass touches: a_pb plane 11 of the last window; channel 2 of the last pixel
    const size_t top_win = p.off_ab + 11 * p.windows + last_w, top_pix = 2 * p.plane + last_p;
    printf("plan %d %d -> %d %d %zu %zu %zu | %zu %zu %zu %zu | %d %d %zu %d | %d %d %zu %d | %zu %zu %zu | %zu %zu\n", H, W, p.Hw, p.Ww, p.plane, p.pixels,
           p.windows, p.off_mu, p.off_M, p.off_ab, p.win_floats, p.fit_tiles_y, p.fit_tiles_x, p.fit_tiles, p.fit_grid, p.apply_tiles_y,
           p.apply_tiles_x, p.apply_tiles, p.apply_grid, vw, vp, bad, top_win, top_pix);
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    validate("on", 1e4, 1e-7);
    validate("negative", -1.3, 1e-7);
    validate("off", 0.0, 1e-7);
    validate("off_negative_zero", -0.0, 1e-7);
    validate("eps_low_end", 1.0, 1e-9);
    validate("eps_high_end", 1.0, 1.0);
    validate("weight_nan", nan, 1e-7);
    validate("weight_inf", inf, 1e-7);
    validate("weight_negative_inf", -inf, 1e-7);
    validate("weight_underflows_float", 1e-60, 1e-7);
    validate("weight_overflows_float", 1e60, 1e-7);
    validate("eps_zero", 1.0, 0.0);
    validate("eps_below", 1.0, 0.99e-9);
    validate("eps_above", 1.0, 1.0000001);
    validate("eps_negative", 1.0, -1e-7);
    validate("eps_nan", 1.0, nan);
    validate("eps_inf", 1.0, inf);
    validate("weight_before_eps", nan, 0.0);
    MatPlan p;
    printf("plan_off -> %s\n", mat_refusal_text(mat_plan(16, 16, 0.0, 1e-7, &p)));
    plan(2, 9, true);
    plan(9, 2, true);
    plan(3, 3, true);
    plan(3, 300, true);
    plan(37, 50, true);
    plan(kMatTileH + 3, kMatTileW + 3, true);
    plan(kMatTileH + 1, kMatTileW + 1, true);
    plan(300, 1030, true);                                 // more tiles than workgroups: the second sweep of both passes
    plan(8192, 8192, false);
    printf("constants %d %d %d %d %d %d %d\n", kMatTileW, kMatTileH, kMatThreads, kMatLdsW, kMatLdsH, kMatMaxBlocks, kMatPartRows);
    printf("lds %zu %zu\n", sizeof(float) * kMatFitPlanes * kMatLdsH * kMatLdsW, sizeof(float) * kMatApplyPlanes * kMatLdsH * kMatLdsW);
    return 0;
}
