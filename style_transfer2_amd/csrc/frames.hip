// Frame sequences (include/st2.h: st_set_input_from_frame, st_anchor_from_frame; frames_plan.h: validation and grids).  One launch:
//   frames_k   per pixel, once: the sample point of the backward flow, its four neighbours and weights, the reliability of the flow
//              (with a forward flow), its product with the caller's map; then the three planes of the kept frame are sampled with
//              those weights and written -- or, accumulating, composed into the anchor that is there -- and the map after them
// The gathers follow the flow, which is smooth where it is reliable: neighbouring threads read neighbouring pixels.  The arithmetic is
// jobs.warp_planar's and tests/frames_oracle.py's, in double, in their order.
// Built with -ffp-contract=off: every operation below rounds once, in the order written.
#include "st2_kernels.h"
#include <stdint.h>

namespace st2 {
namespace {
// what one pixel's sample point gives every plane: the four neighbours (element offsets inside a plane) and the weights
struct Tap { size_t i00, i01, i10, i11; double fx, fy, gx, gy; };

__device__ __forceinline__ float bilinear(const Tap& t, double p00, double p01, double p10, double p11)
{
    const double top = p00 * t.gx + p01 * t.fx;
    const double bottom = p10 * t.gx + p11 * t.fx;
    return (float)(top * t.gy + bottom * t.fy);
}

// One pixel (y, x), `at` = y W + x: v = W(frame, bwd) of the three channels (bwd == NULL: the frame's own pixel), c = the reliability
// (FWD), times the caller's map (MASK); 1 without either.
template <bool FWD, bool MASK>
__device__ __forceinline__ void frames_pixel(const FramesArgs& a, int y, int x, size_t at, float (&v)[3], float& c)
{
    const int H = a.H, W = a.W;
    const float2* bwd = reinterpret_cast<const float2*>(a.bwd);
    const bool warp = bwd != nullptr;                      // uniform
    double u = 0.0, w = 0.0;                               // the backward flow here, (dx, dy)
    if (warp) { const float2 f = bwd[at]; u = (double)f.x; w = (double)f.y; }
    const double px = (double)x + u, py = (double)y + w;   // the sample point, unclamped
    const double sx = fmin(fmax(px, 0.0), (double)(W - 1)), sy = fmin(fmax(py, 0.0), (double)(H - 1));
    const double x0d = floor(sx), y0d = floor(sy);
    const int x0 = (int)x0d, y0 = (int)y0d;                // inside the image: sx and sy are
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    Tap t;
    t.fx = sx - x0d; t.fy = sy - y0d; t.gx = 1.0 - t.fx; t.gy = 1.0 - t.fy;
    t.i00 = (size_t)y0 * W + x0; t.i01 = (size_t)y0 * W + x1; t.i10 = (size_t)y1 * W + x0; t.i11 = (size_t)y1 * W + x1;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float* p = a.src + ch * a.plane;
        v[ch] = warp ? bilinear(t, (double)p[t.i00], (double)p[t.i01], (double)p[t.i10], (double)p[t.i11]) : p[at];
    }
    double cd = 1.0;
    if constexpr (FWD) {
        const float2* fwd = reinterpret_cast<const float2*>(a.fwd);
        const float2 f00 = fwd[t.i00], f01 = fwd[t.i01], f10 = fwd[t.i10], f11 = fwd[t.i11];
        const double wx = (double)bilinear(t, (double)f00.x, (double)f01.x, (double)f10.x, (double)f11.x);     // the forward flow where the
        const double wy = (double)bilinear(t, (double)f00.y, (double)f01.y, (double)f10.y, (double)f11.y);     // backward flow lands, as a float
        const bool outside = px < 0.0 || px > (double)(W - 1) || py < 0.0 || py > (double)(H - 1);
        const double ex = wx + u, ey = wy + w;
        const bool disoccluded = ex * ex + ey * ey > 0.01 * ((wx * wx + wy * wy) + (u * u + w * w)) + 0.5;
        double ux = 0.0, uy = 0.0, vx = 0.0, vy = 0.0;     // forward differences of the backward flow
        if (warp) {
            const float2 r = bwd[(size_t)y * W + min(x + 1, W - 1)], d = bwd[(size_t)min(y + 1, H - 1) * W + x];
            ux = (double)r.x - u; uy = (double)d.x - u; vx = (double)r.y - w; vy = (double)d.y - w;
        }
        const bool boundary = (ux * ux + uy * uy) + (vx * vx + vy * vy) > 0.01 * (u * u + w * w) + 0.002;
        if (outside || disoccluded || boundary) cd = 0.0;
    }
    if constexpr (MASK) c = (float)(cd * (double)a.mask[at]);
    else c = (float)cd;
}
}  // namespace

// A thread takes one pixel (VEC: four consecutive ones of a row, 16-byte stores) per trip.  ACC: the long-term composition -- per pixel
// m = max(c - M, 0), the planes take the new sample where m > 0 and keep what they hold elsewhere, M += m.
template <bool VEC, bool FWD, bool MASK, bool ACC>
__global__ __launch_bounds__(256) void frames_k(const FramesArgs a)
{
    constexpr int PX = VEC ? 4 : 1;
    constexpr bool MAP = FWD || MASK || ACC;
    const size_t plane = a.plane, n = plane / PX;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t at = i * PX;
        const int y = (int)(at / (size_t)a.W), x = (int)(at - (size_t)y * a.W);
        float v[PX][3], c[PX];
#pragma unroll
        for (int k = 0; k < PX; ++k) frames_pixel<FWD, MASK>(a, y, x + k, at + k, v[k], c[k]);
        if constexpr (VEC) {
            float4 o[3], mo;
            if constexpr (ACC) {                           // every load of the trip before its first store
                const float4 m = *reinterpret_cast<const float4*>(a.map + at);
                float4 old[3];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) old[ch] = *reinterpret_cast<const float4*>(a.dst + ch * plane + at);
                const float g0 = fmaxf(c[0] - m.x, 0.f), g1 = fmaxf(c[1] - m.y, 0.f), g2 = fmaxf(c[2] - m.z, 0.f), g3 = fmaxf(c[3] - m.w, 0.f);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    o[ch] = make_float4(g0 > 0.f ? v[0][ch] : old[ch].x, g1 > 0.f ? v[1][ch] : old[ch].y, g2 > 0.f ? v[2][ch] : old[ch].z,
                                        g3 > 0.f ? v[3][ch] : old[ch].w);
                mo = make_float4(m.x + g0, m.y + g1, m.z + g2, m.w + g3);
            } else {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) o[ch] = make_float4(v[0][ch], v[1][ch], v[2][ch], v[3][ch]);
                mo = make_float4(c[0], c[1], c[2], c[3]);
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) *reinterpret_cast<float4*>(a.dst + ch * plane + at) = o[ch];
            if constexpr (MAP) *reinterpret_cast<float4*>(a.map + at) = mo;
        } else {
            if constexpr (ACC) {
                const float m = a.map[at];
                const float old[3] = {a.dst[at], a.dst[plane + at], a.dst[2 * plane + at]};
                const float g = fmaxf(c[0] - m, 0.f);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) a.dst[ch * plane + at] = g > 0.f ? v[0][ch] : old[ch];
                a.map[at] = m + g;
            } else {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) a.dst[ch * plane + at] = v[0][ch];
                if constexpr (MAP) a.map[at] = c[0];
            }
        }
    }
}

namespace {
template <bool VEC, bool FWD, bool MASK>
void frames_go(const FramesArgs& a, bool acc, int gr, hipStream_t s)
{
    if (acc) frames_k<VEC, FWD, MASK, true><<<gr, 256, 0, s>>>(a);
    else frames_k<VEC, FWD, MASK, false><<<gr, 256, 0, s>>>(a);
}
template <bool VEC>
void frames_pick(const FramesArgs& a, bool acc, int gr, hipStream_t s)
{
    if (a.fwd) { if (a.mask) frames_go<VEC, true, true>(a, acc, gr, s); else frames_go<VEC, true, false>(a, acc, gr, s); }
    else { if (a.mask) frames_go<VEC, false, true>(a, acc, gr, s); else frames_go<VEC, false, false>(a, acc, gr, s); }
}
}  // namespace

hipError_t launch_frames(const FramesArgs& a, int accumulate, int grid, int grid_vec, hipStream_t s)
{
    const bool wants_map = a.fwd || a.mask || accumulate;
    if (!a.src || !a.dst || a.src == a.dst || a.H < 1 || a.W < 1 || a.plane != (size_t)a.H * a.W || (wants_map && !a.map)) return hipErrorInvalidValue;
    if ((((uintptr_t)a.bwd | (uintptr_t)a.fwd) & 7) != 0) return hipErrorInvalidValue;       // the flows are read as (dx, dy) pairs
    // the 16-byte form: groups of four stay inside a row, and every plane written starts on a 16-byte boundary
    const bool vec = a.W % 4 == 0 && ((((uintptr_t)a.dst | (uintptr_t)(wants_map ? a.map : nullptr)) & 15) == 0);
    const int gr = vec ? grid_vec : grid;
    if (gr < 1 || gr > kFramesMaxBlocks) return hipErrorInvalidValue;
    if (vec) frames_pick<true>(a, accumulate != 0, gr, s);
    else frames_pick<false>(a, accumulate != 0, gr, s);
    return hipGetLastError();
}

}  // namespace st2
