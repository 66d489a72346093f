// The photorealism term (include/st2.h: st_set_matting): validation of the weight, eps and the size, the window counts, the sizes and
// offsets of the term's buffers, the tiles of its two passes and their launch grids.  The engine (engine_matting.cpp) and the launchers
// (matting.hip) both ask here.  No HIP header: tests/matting_plan_host_main.cpp compiles this file alone, under the host sanitizers.
#pragma once
#include "../../include/st2.h"

#include <math.h>
#include <stddef.h>

namespace st2 {
constexpr int kMatPartRows = 2;                            // partial-sum rows: sum J, then sum g_mat^2
constexpr int kMatMaxBlocks = 1024;                        // grid cap (= partial-sum slots per row), that of every reducing launch
// Both passes: a workgroup of 256 threads takes tiles of kMatTileW x kMatTileH cells (windows in the first pass, pixels in the second),
// thread t the cell (t / kMatTileW, t % kMatTileW) of its tile -- a wavefront is one 256-byte row -- and walks the tiles block,
// block + grid, ... in row-major order.  The LDS tile has a one-cell apron on every side.
constexpr int kMatTileW = 64, kMatTileH = 4;
constexpr int kMatThreads = kMatTileW * kMatTileH;
constexpr int kMatLdsW = kMatTileW + 2, kMatLdsH = kMatTileH + 2;
constexpr int kMatFitPlanes = 6;                           // LDS planes of the first pass: u (3), I (3)
constexpr int kMatApplyPlanes = 15;                        // ... of the second: a, pb of the three channels (12), mu (3)
constexpr double kMatEpsMin = 1e-9, kMatEpsMax = 1.0, kMatEpsDefault = 1e-7;

enum MatRefusal { MAT_OK = 0, MAT_WEIGHT, MAT_EPS, MAT_SIZE };

inline const char* mat_refusal_text(int r)
{
    switch (r) {
    case MAT_OK: return "ok";
    case MAT_WEIGHT: return "the weight must be finite, and zero (off) or non-zero as a double and as a float";
    case MAT_EPS: return "eps must lie in [1e-9, 1]";
    case MAT_SIZE: return "the image must be at least 3 x 3: a window is a 3 x 3 block that lies wholly inside it";
    }
    return "?";
}

// weight == 0 is valid here: it turns the term off
inline int mat_validate(double weight, double eps)
{
    if (!isfinite(weight) || (weight != 0.0 && ((float)weight == 0.f || !isfinite((float)weight)))) return MAT_WEIGHT;
    if (!(eps >= kMatEpsMin) || !(eps <= kMatEpsMax)) return MAT_EPS;      // (a NaN fails the first test)
    return MAT_OK;
}

struct MatPlan {
    int H, W;               // the image
    int Hw, Ww;             // window centres: H - 2 rows of W - 2; window (wy, wx) is centred at pixel (wy + 1, wx + 1)
    size_t plane;           // H * W
    size_t pixels;          // 3 * H * W: floats of I and of `extra`
    size_t windows;         // Hw * Ww
    // one buffer of per-window floats, planes of `windows` back to back: mu (3), M (6: 00 01 02 11 12 22), then a_pb (3 channels x a0 a1 a2 pb)
    size_t off_mu, off_M, off_ab, win_floats;
    int fit_tiles_y, fit_tiles_x, apply_tiles_y, apply_tiles_x;
    size_t fit_tiles, apply_tiles;
    int fit_grid, apply_grid;
    float w;                // the weight as the kernels take it
    double eps;
};

inline int mat_grid(size_t tiles)
{
    return (int)(tiles < 1 ? 1 : tiles > (size_t)kMatMaxBlocks ? (size_t)kMatMaxBlocks : tiles);
}

inline int mat_plan(int H, int W, double weight, double eps, MatPlan* out)
{
    const int bad = mat_validate(weight, eps);
    if (bad) return bad;
    if (weight == 0.0) return MAT_WEIGHT;
    if (H < 3 || W < 3) return MAT_SIZE;
    MatPlan p{};
    p.H = H; p.W = W; p.Hw = H - 2; p.Ww = W - 2;
    p.plane = (size_t)H * W;
    p.pixels = 3 * p.plane;
    p.windows = (size_t)p.Hw * p.Ww;
    p.off_mu = 0;
    p.off_M = 3 * p.windows;
    p.off_ab = 9 * p.windows;
    p.win_floats = 21 * p.windows;
    p.fit_tiles_y = (p.Hw + kMatTileH - 1) / kMatTileH;
    p.fit_tiles_x = (p.Ww + kMatTileW - 1) / kMatTileW;
    p.apply_tiles_y = (H + kMatTileH - 1) / kMatTileH;
    p.apply_tiles_x = (W + kMatTileW - 1) / kMatTileW;
    p.fit_tiles = (size_t)p.fit_tiles_y * p.fit_tiles_x;
    p.apply_tiles = (size_t)p.apply_tiles_y * p.apply_tiles_x;
    p.fit_grid = mat_grid(p.fit_tiles);
    p.apply_grid = mat_grid(p.apply_tiles);
    p.w = (float)weight;
    p.eps = eps;
    *out = p;
    return MAT_OK;
}

// bytes the two passes move, as the profile books them: the first reads x and I and writes a_pb (mu and M come in as well);
// the second reads x, I, the per-window planes and the previous `extra` (when there is one) and writes `extra`
inline double mat_fit_bytes(const MatPlan& p) { return 4.0 * (2.0 * (double)p.pixels + 21.0 * (double)p.windows); }
inline double mat_apply_bytes(const MatPlan& p, bool prev) { return 4.0 * ((prev ? 4.0 : 3.0) * (double)p.pixels + 15.0 * (double)p.windows); }
}  // namespace st2
