// Frame sequences (include/st2.h: st_frames_keep .. st_anchor_from_frame): validation of the depth, the frame index and the flows, and
// the launch grids of frames_k.  The engine (engine_frames.cpp) and the launcher (frames.hip) both ask here.  No HIP header:
// tests/frames_plan_host_main.cpp compiles this file alone, under the host sanitizers.
#pragma once
#include "anchor_plan.h"

namespace st2 {
constexpr int kFramesMaxDepth = 8;                         // earlier iterates a context keeps at most
constexpr int kFramesMaxBlocks = 4096;                     // grid cap: the launch walks larger images in a grid-stride loop

enum FramesRefusal { FRAMES_OK = 0, FRAMES_DEPTH, FRAMES_INDEX, FRAMES_SIZE, FRAMES_FLOW };

inline const char* frames_refusal_text(int r)
{
    switch (r) {
    case FRAMES_OK: return "ok";
    case FRAMES_DEPTH: return "the depth must be between 0 and 8";
    case FRAMES_INDEX: return "the frame index must be between 1 and the depth";
    case FRAMES_SIZE: return "the image must be at least 1 x 1";
    case FRAMES_FLOW: return "every value of a flow must be finite";
    }
    return "?";
}

inline int frames_validate_depth(int depth) { return (depth < 0 || depth > kFramesMaxDepth) ? FRAMES_DEPTH : FRAMES_OK; }
inline int frames_validate_index(int j, int depth) { return (j < 1 || j > depth) ? FRAMES_INDEX : FRAMES_OK; }

// flow: NULL (none) or H * W * 2 values (dx, dy), scanned here on the host
inline int frames_validate_flow(int H, int W, const float* flow)
{
    if (H < 1 || W < 1) return FRAMES_SIZE;
    if (flow) {
        const size_t n = (size_t)H * W * 2;
        for (size_t i = 0; i < n; ++i)
            if (!isfinite(flow[i])) return FRAMES_FLOW;
    }
    return FRAMES_OK;
}

struct FramesPlan {
    int H, W;
    size_t plane;           // H * W: pixels; floats of a map, half the floats of a flow
    size_t pixels;          // 3 * H * W: floats of a frame
    bool row_vec;           // W % 4 == 0: a group of four never straddles a row (the launcher adds the pointer tests)
    int grid, grid_vec;     // workgroups: a thread takes one pixel (scalar form) or four consecutive ones (16-byte form) per trip
};

inline int frames_plan(int H, int W, FramesPlan* out)
{
    if (H < 1 || W < 1) return FRAMES_SIZE;
    FramesPlan p{};
    p.H = H; p.W = W;
    p.plane = (size_t)H * W;
    p.pixels = 3 * p.plane;
    p.row_vec = W % 4 == 0;
    p.grid = anchor_grid(p.plane, 256, kFramesMaxBlocks);
    p.grid_vec = anchor_grid(p.plane / 4, 256, kFramesMaxBlocks);
    *out = p;
    return FRAMES_OK;
}
}  // namespace st2
