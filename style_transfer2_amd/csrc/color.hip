// The content's colours (include/st2.h has the definitions): luminance emission, colour moments, the affine recolour of a style image.
// Built with -ffp-contract=off: every fp32 operation below rounds once, in the order written (tests/color_oracle.py restates them).
//
//   emit_luma_k        the image handed out under st_set_original_colors, in place of deprocess_k / iterate_average_k (passes.hip)
//   image_moments_k    nine sums in double, per thread -> per workgroup -> image_moments_sum_k (workgroups in order): no atomics
//   recolor_k          s' = A s + b on the device copy of a style image
#include "st2_kernels.h"
#include "wave_reduce.h"
#include <stdint.h>

namespace st2 {

static __constant__ float kMean[3] = {123.68f, 116.779f, 103.939f};   // worker.py:34
// Rec.601 luma
#define LUMA_R 0.299f
#define LUMA_G 0.587f
#define LUMA_B 0.114f

// one pixel: v the iterate (or its corrected mean), cx the content; out = (cx + channel mean) + luma(v - cx)
__device__ __forceinline__ void luma_pixel(const float (&v)[3], const float (&cx)[3], float (&out)[3])
{
    const float dr = v[0] - cx[0], dg = v[1] - cx[1], db = v[2] - cx[2];
    const float l = (LUMA_R * dr + LUMA_G * dg) + LUMA_B * db;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = (cx[c] + kMean[c]) + l;
}

// FORM: EMIT_PLAIN v = x; EMIT_UPDATE mean = decay * mean + rest * x (iterate_average_k's update, unchanged), v = mean / corr; EMIT_STAGED
// v = mean / corr, the mean only read.  VEC: a thread owns 4 consecutive pixels -- 16-byte reads of every plane of every stream, the 12
// consecutive floats of hwc as three 16-byte writes; else one pixel per thread.
template <int FORM, bool VEC>
__global__ __launch_bounds__(256) void emit_luma_k(const EmitLumaArgs a)
{
    const size_t plane = (size_t)a.H * a.W;
    const size_t n = VEC ? plane / 4 : plane;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        if (VEC) {
            float4 v4[3], c4[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const size_t at = (size_t)c * plane + i * 4;
                c4[c] = *reinterpret_cast<const float4*>(a.cx + at);
                if (FORM == EMIT_PLAIN)
                    v4[c] = *reinterpret_cast<const float4*>(a.x + at);
                else {
                    float4 m;
                    if (FORM == EMIT_UPDATE) {
                        const float4 x = *reinterpret_cast<const float4*>(a.x + at);
                        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (!a.first) o = *reinterpret_cast<const float4*>(a.mean + at);
                        m.x = a.decay * o.x + a.rest * x.x;
                        m.y = a.decay * o.y + a.rest * x.y;
                        m.z = a.decay * o.z + a.rest * x.z;
                        m.w = a.decay * o.w + a.rest * x.w;
                        *reinterpret_cast<float4*>(a.mean + at) = m;
                    } else
                        m = *reinterpret_cast<const float4*>(a.mean + at);
                    v4[c] = make_float4(__fdiv_rn(m.x, a.corr), __fdiv_rn(m.y, a.corr), __fdiv_rn(m.z, a.corr), __fdiv_rn(m.w, a.corr));
                }
            }
            float r[4][3];
            {
                const float v0[3] = {v4[0].x, v4[1].x, v4[2].x}, c0[3] = {c4[0].x, c4[1].x, c4[2].x};
                const float v1[3] = {v4[0].y, v4[1].y, v4[2].y}, c1[3] = {c4[0].y, c4[1].y, c4[2].y};
                const float v2[3] = {v4[0].z, v4[1].z, v4[2].z}, c2[3] = {c4[0].z, c4[1].z, c4[2].z};
                const float v3[3] = {v4[0].w, v4[1].w, v4[2].w}, c3[3] = {c4[0].w, c4[1].w, c4[2].w};
                luma_pixel(v0, c0, r[0]); luma_pixel(v1, c1, r[1]); luma_pixel(v2, c2, r[2]); luma_pixel(v3, c3, r[3]);
            }
            float4* out = reinterpret_cast<float4*>(a.hwc + i * 12);
            out[0] = make_float4(r[0][0], r[0][1], r[0][2], r[1][0]);
            out[1] = make_float4(r[1][1], r[1][2], r[2][0], r[2][1]);
            out[2] = make_float4(r[2][2], r[3][0], r[3][1], r[3][2]);
        } else {
            float v[3], cx[3], r[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const size_t at = (size_t)c * plane + i;
                cx[c] = a.cx[at];
                if (FORM == EMIT_PLAIN)
                    v[c] = a.x[at];
                else {
                    float m;
                    if (FORM == EMIT_UPDATE) {
                        const float o = a.first ? 0.f : a.mean[at];
                        m = a.decay * o + a.rest * a.x[at];
                        a.mean[at] = m;
                    } else
                        m = a.mean[at];
                    v[c] = __fdiv_rn(m, a.corr);
                }
            }
            luma_pixel(v, cx, r);
#pragma unroll
            for (int c = 0; c < 3; ++c) a.hwc[i * 3 + c] = r[c];
        }
    }
}

hipError_t launch_emit_luma(const EmitLumaArgs& a, hipStream_t s)
{
    const size_t plane = (size_t)a.H * a.W;
    if (!plane) return hipSuccess;
    if (!a.cx || !a.hwc || (a.form != EMIT_STAGED && !a.x) || (a.form != EMIT_PLAIN && !a.mean)) return hipErrorInvalidValue;
    const bool vec = plane % 4 == 0 && (((uintptr_t)a.x | (uintptr_t)a.mean | (uintptr_t)a.cx | (uintptr_t)a.hwc) & 15) == 0;
    const int grid = reduce_grid(vec ? plane / 4 : plane, 256, 2048);
    switch (a.form) {
    case EMIT_PLAIN:
        if (vec) emit_luma_k<EMIT_PLAIN, true><<<grid, 256, 0, s>>>(a);
        else emit_luma_k<EMIT_PLAIN, false><<<grid, 256, 0, s>>>(a);
        break;
    case EMIT_UPDATE:
        if (vec) emit_luma_k<EMIT_UPDATE, true><<<grid, 256, 0, s>>>(a);
        else emit_luma_k<EMIT_UPDATE, false><<<grid, 256, 0, s>>>(a);
        break;
    case EMIT_STAGED:
        if (vec) emit_luma_k<EMIT_STAGED, true><<<grid, 256, 0, s>>>(a);
        else emit_luma_k<EMIT_STAGED, false><<<grid, 256, 0, s>>>(a);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

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
