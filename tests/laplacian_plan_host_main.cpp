// csrc/laplacian_plan.h on the host, alone (no HIP, no engine), under the address and undefined-behaviour sanitizers
// (tests/test_laplacian_plan_cpu.py builds and runs it).  Lines:
//   validate <case> -> <refusal text>
//   plan <p> <H> <W> -> <hp> <wp> <cells> <off> <total> <pixels> <row_vec> <tiles_y> <tiles_x> <pool_grid> <stencil_grid> <grad_grid> <grad_grid_vec>
//   walk <p0,p1,p2> <H> <W> -> <total> <offsets> ok      every cell of every level written exactly once by the pooling pass's tile walk,
//                                                         inside a buffer of exactly `total` floats (the sanitizer watches the accesses)
#include "../style_transfer2_amd/csrc/laplacian_plan.h"

#include <limits>
#include <stdio.h>
#include <vector>

using namespace st2;

static int walk(const int* pool, int n, int H, int W)
{
    const double w[3] = {1.0, -2.0, 0.5};
    LapPlan p;
    if (lap_plan(n, pool, w, H, W, &p) != LAP_OK) return 1;
    std::vector<float> q(p.total, 0.f);                      // exactly the size the engine allocates
    // the tile walk of lap_pool_k: per channel and tile, the cells of each level the tile holds
    for (int ch = 0; ch < 3; ++ch)
        for (int ty = 0; ty < p.tiles_y; ++ty)
            for (int tx = 0; tx < p.tiles_x; ++tx)
                for (int l = 0; l < p.n; ++l) {
                    const LapLevel& lv = p.lv[l];
                    const int k = lv.shift, cols = kLapTileX >> k, rows = kLapTileY >> k;
                    for (int e = 0; e < rows * cols; ++e) {
                        const int i = e / cols, j = e - i * cols;
                        const int ci = ((ty * kLapTileY) >> k) + i, cj = ((tx * kLapTileX) >> k) + j;
                        if (ci >= lv.hp || cj >= lv.wp) continue;
                        if (lap_extent(H, lv.p, ci) < 1 || lap_extent(W, lv.p, cj) < 1) return 2;
                        q.at(lv.off + ((size_t)ch * lv.hp + ci) * lv.wp + cj) += 1.f;
                    }
                }
    for (int l = 0; l < p.n; ++l) {
        const LapLevel& lv = p.lv[l];
        if (lv.off % 4 || lv.off + lv.cells > p.total) return 3;
        if (l && lv.off < p.lv[l - 1].off + p.lv[l - 1].cells) return 4;
        for (size_t c = 0; c < lv.cells; ++c) if (q[lv.off + c] != 1.f) return 5;
        long long px = 0;                                     // the clipped windows tile the image
        for (int i = 0; i < lv.hp; ++i) for (int j = 0; j < lv.wp; ++j) px += (long long)lap_extent(H, lv.p, i) * lap_extent(W, lv.p, j);
        if (px != (long long)H * W) return 6;
    }
    printf("walk %d,%d,%d %d %d -> %zu %zu,%zu,%zu ok\n", pool[0], n > 1 ? pool[1] : 0, n > 2 ? pool[2] : 0, H, W, p.total, p.lv[0].off,
           n > 1 ? p.lv[1].off : (size_t)0, n > 2 ? p.lv[2].off : (size_t)0);
    return 0;
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    struct Case { const char* name; int n; int pool[4]; double w[4]; bool null_pool, null_w; };
    const Case cases[] = {
        {"off", 0, {0}, {0}, true, true},
        {"one", 1, {4}, {1.5}, false, false},
        {"three", 3, {2, 4, 16}, {1, -2, 3}, false, false},
        {"every_pool_a", 3, {1, 2, 4}, {1, 1, 1}, false, false},
        {"every_pool_b", 3, {8, 16, 32}, {1, 1, 1}, false, false},
        {"negative_count", -1, {4}, {1}, false, false},
        {"four_levels", 4, {1, 2, 4, 8}, {1, 1, 1, 1}, false, false},
        {"null_pool", 1, {4}, {1}, true, false},
        {"null_weight", 1, {4}, {1}, false, true},
        {"pool_0", 1, {0}, {1}, false, false},
        {"pool_3", 1, {3}, {1}, false, false},
        {"pool_64", 1, {64}, {1}, false, false},
        {"pool_negative", 1, {-4}, {1}, false, false},
        {"duplicate", 2, {4, 4}, {1, 2}, false, false},
        {"duplicate_last", 3, {4, 16, 4}, {1, 2, 3}, false, false},
        {"weight_zero", 1, {4}, {0.0}, false, false},
        {"weight_negative_zero", 1, {4}, {-0.0}, false, false},
        {"weight_nan", 1, {4}, {nan}, false, false},
        {"weight_inf", 1, {4}, {inf}, false, false},
        {"weight_negative_inf", 2, {4, 8}, {1, -inf}, false, false},
        {"weight_underflows_float", 1, {4}, {1e-60}, false, false},
        {"weight_overflows_float", 1, {4}, {1e60}, false, false},
    };
    for (const Case& c : cases)
        printf("validate %s -> %s\n", c.name, lap_refusal_text(lap_validate(c.n, c.null_pool ? nullptr : c.pool, c.null_w ? nullptr : c.w)));

    const double one = 1.0;
    for (int k = 0; (1 << k) <= kLapMaxPool; ++k)
        for (int H = 1; H <= 70; ++H)
            for (int W = 1; W <= 70; ++W) {
                const int p = 1 << k;
                LapPlan pl;
                if (lap_plan(1, &p, &one, H, W, &pl) != LAP_OK) return 1;
                const LapLevel& lv = pl.lv[0];
                printf("plan %d %d %d -> %d %d %zu %zu %zu %zu %d %d %d %d %d %d %d\n", p, H, W, lv.hp, lv.wp, lv.cells, lv.off, pl.total, pl.pixels,
                       pl.row_vec ? 1 : 0, pl.tiles_y, pl.tiles_x, pl.pool_grid, pl.stencil_grid, pl.grad_grid, pl.grad_grid_vec);
            }
    {
        LapPlan pl;
        const int p = 4;
        if (lap_plan(1, &p, &one, 0, 5, &pl) != LAP_SIZE || lap_plan(1, &p, &one, 5, 0, &pl) != LAP_SIZE) return 1;
        printf("plan_size_refused\n");
        // a large image: the grids stay inside their caps and the sizes do not wrap
        if (lap_plan(1, &p, &one, 40000, 40000, &pl) != LAP_OK) return 1;
        printf("big %zu %zu %d %d %d %d\n", pl.total, pl.pixels, pl.pool_grid, pl.stencil_grid, pl.grad_grid, pl.grad_grid_vec);
    }
    const int sets[4][3] = {{2, 4, 16}, {1, 8, 32}, {32, 1, 2}, {16, 0, 0}};
    for (int s = 0; s < 4; ++s)
        for (int H = 1; H <= 70; ++H)
            for (int W = 1; W <= 70; ++W) {
                const int rc = walk(sets[s], s == 3 ? 1 : 3, H, W);
                if (rc) { printf("walk %d %d %d FAILED %d\n", s, H, W, rc); return 1; }
            }
    return 0;
}
