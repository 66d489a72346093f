// The anchor term (include/st2.h: st_set_anchor): validation of the weight, the size and the map, and the launch grids of anchor_k.
// The engine (engine_anchor.cpp) and the launcher (anchor.hip) both ask here.  No HIP header: tests/anchor_plan_host_main.cpp compiles
// this file alone, under the host sanitizers.
#pragma once
#include "../../include/st2.h"

#include <math.h>
#include <stddef.h>

namespace st2 {
constexpr int kAnchorPartRows = 2;                         // partial-sum rows: sum e d, then sum g_anc^2
constexpr int kAnchorMaxBlocks = 1024;                     // grid cap (= partial-sum slots per row), that of the Laplacian launches

enum AnchorRefusal { ANCHOR_OK = 0, ANCHOR_WEIGHT, ANCHOR_SIZE, ANCHOR_MAP };

inline const char* anchor_refusal_text(int r)
{
    switch (r) {
    case ANCHOR_OK: return "ok";
    case ANCHOR_WEIGHT: return "the weight must be finite and non-zero, as a double and as a float";
    case ANCHOR_SIZE: return "the image must be at least 1 x 1";
    case ANCHOR_MAP: return "every value of the map must be finite and not negative";
    }
    return "?";
}

inline int anchor_validate_weight(double w)
{
    return (!isfinite(w) || w == 0.0 || (float)w == 0.f || !isfinite((float)w)) ? ANCHOR_WEIGHT : ANCHOR_OK;
}

// mask: NULL (1 everywhere) or H * W values, scanned here on the host
inline int anchor_validate(int H, int W, const float* mask, double weight)
{
    const int bad = anchor_validate_weight(weight);
    if (bad) return bad;
    if (H < 1 || W < 1) return ANCHOR_SIZE;
    if (mask) {
        const size_t n = (size_t)H * W;
        for (size_t i = 0; i < n; ++i)
            if (!(mask[i] >= 0.f) || !isfinite(mask[i])) return ANCHOR_MAP;      // (a NaN fails the first test)
    }
    return ANCHOR_OK;
}

struct AnchorPlan {
    int H, W;
    size_t plane;           // H * W: floats of the map
    size_t pixels;          // 3 * H * W: floats of the anchor and of `extra`
    bool row_vec;           // W % 4 == 0: a group of four never straddles a row or a plane (the launcher adds the pointer tests)
    int grid, grid_vec;     // workgroups: a thread takes one pixel (scalar form) or four consecutive ones (float4 form) of all three channels per trip
    float w;                // the weight as the kernel takes it
};

inline int anchor_grid(size_t n, int per_block, int cap)
{
    size_t b = (n + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > (size_t)cap) b = cap;
    return (int)b;
}

inline int anchor_plan(int H, int W, double weight, AnchorPlan* out)
{
    const int bad = anchor_validate(H, W, nullptr, weight);
    if (bad) return bad;
    AnchorPlan p{};
    p.H = H; p.W = W;
    p.plane = (size_t)H * W;
    p.pixels = 3 * p.plane;
    p.row_vec = W % 4 == 0;
    p.grid = anchor_grid(p.plane, 256, kAnchorMaxBlocks);
    p.grid_vec = anchor_grid(p.plane / 4, 256, kAnchorMaxBlocks);
    p.w = (float)weight;
    *out = p;
    return ANCHOR_OK;
}
}  // namespace st2
