// The Laplacian-steered content term (include/st2.h: st_set_laplacian): level validation, cell counts, buffer sizes and offsets, and
// the launch grids.  The engine (engine_laplacian.cpp) and the launchers (laplacian.hip) both ask here.  No HIP header:
// tests/laplacian_plan_host_main.cpp compiles this file alone, under the host sanitizers.
#pragma once
#include "../../include/st2.h"

#include <math.h>
#include <stddef.h>

namespace st2 {
constexpr int kLapMaxLevels = 3;
constexpr int kLapMaxPool = 32;
// the pooling pass walks tiles of kLapTileY rows x kLapTileX columns of one channel: every pool size divides both, so a cell never
// straddles two tiles and the pool sizes nest inside one
constexpr int kLapTileY = 32, kLapTileX = 64;
constexpr int kLapPartRows = kLapMaxLevels + 1;           // partial-sum rows: sum E^2 per level, then sum g_lap^2
constexpr int kLapMaxBlocks = 1024;                        // grid cap (= partial-sum slots per row) of the reducing launches

enum LapRefusal { LAP_OK = 0, LAP_NULL, LAP_COUNT, LAP_POOL, LAP_DUPLICATE, LAP_WEIGHT, LAP_SIZE };

inline const char* lap_refusal_text(int r)
{
    switch (r) {
    case LAP_OK: return "ok";
    case LAP_NULL: return "pool and weight arrays are required for one or more levels";
    case LAP_COUNT: return "between 0 and 3 levels";
    case LAP_POOL: return "a pool size must be one of 1, 2, 4, 8, 16, 32";
    case LAP_DUPLICATE: return "two levels have the same pool size";
    case LAP_WEIGHT: return "a weight must be finite and non-zero";
    case LAP_SIZE: return "the image must be at least 1 x 1";
    }
    return "?";
}

inline int lap_log2(int p)                                 // 0 .. 5 for a valid pool size, else -1
{
    for (int k = 0; (1 << k) <= kLapMaxPool; ++k) if (p == (1 << k)) return k;
    return -1;
}

inline int lap_validate(int n_levels, const int* pool, const double* weight)
{
    if (n_levels < 0 || n_levels > kLapMaxLevels) return LAP_COUNT;
    if (n_levels && (!pool || !weight)) return LAP_NULL;
    for (int i = 0; i < n_levels; ++i) {
        if (lap_log2(pool[i]) < 0) return LAP_POOL;
        for (int j = 0; j < i; ++j) if (pool[j] == pool[i]) return LAP_DUPLICATE;
        if (!isfinite(weight[i]) || weight[i] == 0.0 || (float)weight[i] == 0.f || !isfinite((float)weight[i])) return LAP_WEIGHT;
    }
    return LAP_OK;
}

inline int lap_cells(int size, int p) { return (size + p - 1) / p; }                        // ceil: the last cell may be clipped
inline int lap_extent(int size, int p, int i) { const int a = i * p, b = a + p; return (b < size ? b : size) - a; }   // pixels of cell i along one axis

struct LapLevel {
    int p, shift;           // pool size = 1 << shift
    int hp, wp;             // cells
    size_t cells;           // 3 * hp * wp
    size_t off;             // of this level in the pooled / target / difference buffers, in floats; a multiple of 4
    float w;                // the weight as the kernels take it
};

struct LapPlan {
    int n;                  // levels (0: the term is off)
    int H, W;
    LapLevel lv[kLapMaxLevels];
    int max_shift;          // of the widest pool
    size_t total;           // floats of each of the three per-level buffers
    size_t pixels;          // 3 * H * W: floats of g_lap
    bool row_vec;           // W % 4 == 0: rows start on 16-byte boundaries when the plane does (the launchers add the pointer test)
    int tiles_y, tiles_x;   // of the pooling pass, per channel
    int pool_grid, stencil_grid, grad_grid, grad_grid_vec;
};

inline int lap_grid(size_t n, int per_block, int cap)
{
    size_t b = (n + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > (size_t)cap) b = cap;
    return (int)b;
}

// pool / weight: validated by lap_validate
inline int lap_plan(int n_levels, const int* pool, const double* weight, int H, int W, LapPlan* out)
{
    LapPlan p{};
    const int bad = lap_validate(n_levels, pool, weight);
    if (bad) return bad;
    if (H < 1 || W < 1) return LAP_SIZE;
    p.n = n_levels; p.H = H; p.W = W;
    size_t off = 0, widest = 1;
    for (int i = 0; i < n_levels; ++i) {
        LapLevel& l = p.lv[i];
        l.p = pool[i]; l.shift = lap_log2(pool[i]);
        l.hp = lap_cells(H, l.p); l.wp = lap_cells(W, l.p);
        l.cells = (size_t)3 * l.hp * l.wp;
        l.off = off;
        l.w = (float)weight[i];
        off += (l.cells + 3) / 4 * 4;
        if (l.cells > widest) widest = l.cells;
        if (l.shift > p.max_shift) p.max_shift = l.shift;
    }
    p.total = off;
    p.pixels = (size_t)3 * H * W;
    p.row_vec = W % 4 == 0;
    p.tiles_y = lap_cells(H, kLapTileY); p.tiles_x = lap_cells(W, kLapTileX);
    p.pool_grid = lap_grid((size_t)3 * p.tiles_y * p.tiles_x, 1, 8192);
    p.stencil_grid = lap_grid(widest, 256 * 4, kLapMaxBlocks);
    p.grad_grid = lap_grid(p.pixels, 256 * 4, kLapMaxBlocks);
    p.grad_grid_vec = lap_grid(p.pixels / 4, 256, kLapMaxBlocks);
    *out = p;
    return LAP_OK;
}
}  // namespace st2
