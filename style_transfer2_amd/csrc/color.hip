// The content's colours (include/st2.h has the definitions): colour moments, the affine recolour of a style image (the luminance
// emission is a form of emit.hip).  Built with -ffp-contract=off: every fp32 operation below rounds once, in the order written
// (tests/color_oracle.py restates them).
//
//   image_moments_k    nine sums in double, per thread -> per workgroup -> image_moments_sum_k (workgroups in order): no atomics
//   recolor_k          s' = A s + b on the device copy of a style image
#include "st2_kernels.h"
#include "wave_reduce.h"
#include <stdint.h>

namespace st2 {

// ---------------------------------------------------------------------------------------- moments
__device__ __forceinline__ double wave_sum_d(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Nine double accumulators per thread over a grid-stride loop (products of fp32 values are exact in double: only the additions round),
// reduced over the workgroup in double (lanes by shuffles, the four waves through LDS, in a fixed association); partials[k][block].
__global__ __launch_bounds__(256) void image_moments_k(const float* __restrict__ x, size_t n, double* __restrict__ partials)
{
    __shared__ double sh[kMomentSums][4];
    double acc[kMomentSums];
#pragma unroll
    for (int k = 0; k < kMomentSums; ++k) acc[k] = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const double r = (double)x[i], g = (double)x[n + i], b = (double)x[2 * n + i];
        acc[0] += r; acc[1] += g; acc[2] += b;
        acc[3] += r * r; acc[4] += r * g; acc[5] += r * b;
        acc[6] += g * g; acc[7] += g * b; acc[8] += b * b;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kMomentSums; ++k) {
        const double w = wave_sum_d(acc[k]);
        if (lane == 0) sh[k][wave] = w;
    }
    __syncthreads();
    if (threadIdx.x < kMomentSums) {
        const int k = threadIdx.x;
        partials[(size_t)k * gridDim.x + blockIdx.x] = (sh[k][0] + sh[k][1]) + (sh[k][2] + sh[k][3]);
    }
}

// second stage: sum k is added up by thread k over the workgroups' partials, first to last
__global__ __launch_bounds__(64) void image_moments_sum_k(const double* __restrict__ partials, int blocks, double* __restrict__ out)
{
    const int k = threadIdx.x;
    if (k >= kMomentSums) return;
    double acc = 0.0;
    for (int j = 0; j < blocks; ++j) acc += partials[(size_t)k * blocks + j];
    out[k] = acc;
}

hipError_t launch_image_moments(const float* x, size_t n, double* partials, double* out, hipStream_t s)
{
    if (!x || !n || !partials || !out) return hipErrorInvalidValue;
    const int grid = reduce_grid(n, 256, kMomentBlocks);
    image_moments_k<<<grid, 256, 0, s>>>(x, n, partials);
    image_moments_sum_k<<<1, 64, 0, s>>>(partials, grid, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------- recolour
__device__ __forceinline__ float recolor_one(const RecolorArgs& a, int c, float r, float g, float b)
{
    return ((a.A[c * 3] * r + a.A[c * 3 + 1] * g) + a.A[c * 3 + 2] * b) + a.b[c];
}

template <bool VEC>
__global__ __launch_bounds__(256) void recolor_k(const RecolorArgs a)
{
    const size_t n = VEC ? a.n / 4 : a.n;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        if (VEC) {
            float4* pr = reinterpret_cast<float4*>(a.x + i * 4);
            float4* pg = reinterpret_cast<float4*>(a.x + a.n + i * 4);
            float4* pb = reinterpret_cast<float4*>(a.x + 2 * a.n + i * 4);
            const float4 r = *pr, g = *pg, b = *pb;
            *pr = make_float4(recolor_one(a, 0, r.x, g.x, b.x), recolor_one(a, 0, r.y, g.y, b.y), recolor_one(a, 0, r.z, g.z, b.z), recolor_one(a, 0, r.w, g.w, b.w));
            *pg = make_float4(recolor_one(a, 1, r.x, g.x, b.x), recolor_one(a, 1, r.y, g.y, b.y), recolor_one(a, 1, r.z, g.z, b.z), recolor_one(a, 1, r.w, g.w, b.w));
            *pb = make_float4(recolor_one(a, 2, r.x, g.x, b.x), recolor_one(a, 2, r.y, g.y, b.y), recolor_one(a, 2, r.z, g.z, b.z), recolor_one(a, 2, r.w, g.w, b.w));
        } else {
            const float r = a.x[i], g = a.x[a.n + i], b = a.x[2 * a.n + i];
            a.x[i] = recolor_one(a, 0, r, g, b);
            a.x[a.n + i] = recolor_one(a, 1, r, g, b);
            a.x[2 * a.n + i] = recolor_one(a, 2, r, g, b);
        }
    }
}

hipError_t launch_recolor(const RecolorArgs& a, hipStream_t s)
{
    if (!a.n) return hipSuccess;
    if (!a.x) return hipErrorInvalidValue;
    const bool vec = a.n % 4 == 0 && ((uintptr_t)a.x & 15) == 0;
    const int grid = reduce_grid(vec ? a.n / 4 : a.n, 256, 2048);
    if (vec) recolor_k<true><<<grid, 256, 0, s>>>(a);
    else recolor_k<false><<<grid, 256, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace st2
