// The anchor term (include/st2.h: st_set_anchor; anchor_plan.h: validation and grids).  One HBM-bound pass per evaluation:
//   anchor_k        d = x / 255 - ax / 255, e = m d (e = d without a map), g_anc = w (2 e); extra = g_lap + g_anc (or g_anc) for the image
//                   pass to add after p_w g_p, and the per-workgroup sums of e d and of g_anc^2
//   trace_anchor_k  a_loss and a_grad join the image part of the trace
// Built with -ffp-contract=off: every fp32 operation below rounds once, in the order written (tests/anchor_oracle.py restates it).
#include "st2_kernels.h"
#include "wave_reduce.h"
#include <stdint.h>

namespace st2 {
namespace {
// a thread's sum (double) -> the workgroup's fp32 partial in thread 0
__device__ __forceinline__ float block_sum_of(double acc, float* scratch)
{
    float v[1] = {(float)acc};
    block_sum(v, scratch);
    return v[0];
}

// one element: the sums in double, the value of `extra` returned (lap: g_lap's value at the element, 0 without the Laplacian term)
template <bool GRAD>
__device__ __forceinline__ float anchor_at(float x, float ax, float m, bool has_map, float lap, bool has_lap, float w, double& sum_ed, double& sum_g2)
{
    const float u = x / 255.0f, ua = ax / 255.0f;
    const float d = u - ua;
    const float e = has_map ? m * d : d;
    sum_ed += (double)e * (double)d;
    if (!GRAD) return 0.f;
    const float g = w * (2.0f * e);
    sum_g2 += (double)g * (double)g;
    return has_lap ? lap + g : g;
}
}  // namespace

// A thread takes one pixel (VEC: four consecutive ones, 16-byte loads and stores) of all three channels per trip: the map is read once
// per pixel.  GRAD == false: no plane is written and only the loss row of the partial sums.
template <bool VEC, bool GRAD>
__global__ __launch_bounds__(256) void anchor_k(const AnchorArgs a)
{
    __shared__ float scratch[4];
    constexpr int PX = VEC ? 4 : 1;
    const size_t plane = a.plane, n = plane / PX;
    const bool has_map = a.m != nullptr, has_lap = GRAD && a.g_lap != nullptr;      // uniform
    double sum_ed = 0.0, sum_g2 = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t at = i * PX;
        if constexpr (VEC) {
            float4 xv[3], av[3], lv[3];
            const float4 mv = has_map ? *reinterpret_cast<const float4*>(a.m + at) : make_float4(1.f, 1.f, 1.f, 1.f);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {               // every load of the trip before its first store
                xv[ch] = *reinterpret_cast<const float4*>(a.x + ch * plane + at);
                av[ch] = *reinterpret_cast<const float4*>(a.ax + ch * plane + at);
                lv[ch] = has_lap ? *reinterpret_cast<const float4*>(a.g_lap + ch * plane + at) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float4 o;
                o.x = anchor_at<GRAD>(xv[ch].x, av[ch].x, mv.x, has_map, lv[ch].x, has_lap, a.w, sum_ed, sum_g2);
                o.y = anchor_at<GRAD>(xv[ch].y, av[ch].y, mv.y, has_map, lv[ch].y, has_lap, a.w, sum_ed, sum_g2);
                o.z = anchor_at<GRAD>(xv[ch].z, av[ch].z, mv.z, has_map, lv[ch].z, has_lap, a.w, sum_ed, sum_g2);
                o.w = anchor_at<GRAD>(xv[ch].w, av[ch].w, mv.w, has_map, lv[ch].w, has_lap, a.w, sum_ed, sum_g2);
                if constexpr (GRAD) *reinterpret_cast<float4*>(a.extra + ch * plane + at) = o;
            }
        } else {
            const float mv = has_map ? a.m[at] : 1.f;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const size_t idx = ch * plane + at;
                const float o = anchor_at<GRAD>(a.x[idx], a.ax[idx], mv, has_map, has_lap ? a.g_lap[idx] : 0.f, has_lap, a.w, sum_ed, sum_g2);
                if constexpr (GRAD) a.extra[idx] = o;
            }
        }
    }
    const float part_ed = block_sum_of(sum_ed, scratch);
    if (threadIdx.x == 0) a.part[blockIdx.x] = part_ed;
    if constexpr (GRAD) {
        const float part_g2 = block_sum_of(sum_g2, scratch);
        if (threadIdx.x == 0) a.part[kAnchorMaxBlocks + blockIdx.x] = part_g2;
    }
}

// the float4 form: groups of four stay inside a row, and every plane starts on a 16-byte boundary
static bool anchor_vec(const AnchorArgs& a)
{
    const uintptr_t bits = (uintptr_t)a.x | (uintptr_t)a.ax | (uintptr_t)a.m | (uintptr_t)a.g_lap | (uintptr_t)a.extra;
    return a.W % 4 == 0 && (bits & 15) == 0;
}

hipError_t launch_anchor(const AnchorArgs& a, int grid, int grid_vec, int* n_partial, hipStream_t s)
{
    if (!a.x || !a.ax || !a.part || a.plane < 1 || a.W < 1 || a.plane % a.W || (a.g_lap && !a.extra) || !n_partial) return hipErrorInvalidValue;
    const bool vec = anchor_vec(a);
    const int gr = vec ? grid_vec : grid;
    if (gr < 1 || gr > kAnchorMaxBlocks) return hipErrorInvalidValue;
    *n_partial = gr;
    if (vec) {
        if (a.extra) anchor_k<true, true><<<gr, 256, 0, s>>>(a);
        else anchor_k<true, false><<<gr, 256, 0, s>>>(a);
    } else {
        if (a.extra) anchor_k<false, true><<<gr, 256, 0, s>>>(a);
        else anchor_k<false, false><<<gr, 256, 0, s>>>(a);
    }
    return hipGetLastError();
}

// the term's two trace scalars: one workgroup sums the two partial rows in double, thread 0 widens the image part of the trace
__global__ __launch_bounds__(256) void trace_anchor_k(const TraceAnchorArgs a)
{
    __shared__ double scratch[256];
    const double sum_ed = sum_partials(a.part, a.count_l, scratch);
    const double sum_g2 = a.count_g > 0 ? sum_partials(a.part + kAnchorMaxBlocks, a.count_g, scratch) : 0.0;      // uniform
    if (threadIdx.x != 0) return;
    float* g = a.image_out;
    const int half = a.with_lap ? 4 : 3;                   // losses, then as many gradient norms, then loss and grad
    const float a_loss = a.w * (float)sum_ed;
    const float a_grad = a.have_grad ? sqrtf((float)(sum_g2 / a.image_n)) : 0.f;
    float norms[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) norms[k] = k < half ? g[half + k] : 0.f;
    const float loss = g[2 * half], grad = g[2 * half + 1];
    g[half] = a_loss;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < half) g[half + 1 + k] = norms[k];
    g[2 * half + 1] = a_grad;
    g[2 * half + 2] = loss + a_loss;
    g[2 * half + 3] = grad;
}

hipError_t launch_trace_anchor(const TraceAnchorArgs& a, hipStream_t s)
{
    if (!a.part || !a.image_out || a.count_l < 1 || a.count_l > kAnchorMaxBlocks || a.count_g < 0 || a.count_g > kAnchorMaxBlocks) return hipErrorInvalidValue;
    trace_anchor_k<<<1, 256, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace st2
