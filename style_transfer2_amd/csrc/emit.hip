// Emission: the one pass that hands an image out (st2_kernels.h: EmitArgs; emit_plan.h: which form, for whom).  Planar (3, H, W) streams
// in, the interleaved (H, W, 3) image out; under iterate averaging the running mean (utils.DecayingMean, utils.py:49-69) is updated on
// the way.  Built with -ffp-contract=off: every fp32 operation below rounds once, in the order written (tests/average_oracle.py and
// tests/color_oracle.py restate them).
#include "st2_kernels.h"
#include "channel_mean.h"
#include "wave_reduce.h"
#include <stdint.h>

#include <type_traits>

namespace st2 {
// Rec.601 luma
#define LUMA_R 0.299f
#define LUMA_G 0.587f
#define LUMA_B 0.114f

template <typename F> __device__ __forceinline__ float each(F f, float a, float b) { return f(a, b); }
template <typename F> __device__ __forceinline__ float4 each(F f, const float4& a, const float4& b) { return make_float4(f(a.x, b.x), f(a.y, b.y), f(a.z, b.z), f(a.w, b.w)); }
__device__ __forceinline__ float lane(float v, int) { return v; }
__device__ __forceinline__ float lane(const float4& v, int p) { return p == 0 ? v.x : p == 1 ? v.y : p == 2 ? v.z : v.w; }

// the value of one pixel (T = float) or of four consecutive ones (float4) in one plane, before the division: x; mean = decay * mean +
// rest * x, written back (first: the mean is empty and counts as 0, the buffer is not read); a mean that is only read
template <int SOURCE, typename T>
__device__ __forceinline__ T emit_load(const EmitArgs& a, size_t at)
{
    if (SOURCE == EMIT_X) return *reinterpret_cast<const T*>(a.x + at);
    if (SOURCE == EMIT_MEAN_READ) return *reinterpret_cast<const T*>(a.mean + at);
    const T x = *reinterpret_cast<const T*>(a.x + at);
    T o = T();
    if (!a.first) o = *reinterpret_cast<const T*>(a.mean + at);
    const T m = each([&](float oi, float xi) { return a.decay * oi + a.rest * xi; }, o, x);
    *reinterpret_cast<T*>(a.mean + at) = m;
    return m;
}

// one pixel: a mean is divided by corr (one IEEE division); then out = v + channel mean, or (cx + channel mean) + luma(v - cx)
template <int SOURCE, int COLOUR>
__device__ __forceinline__ void emit_finish(const EmitArgs& a, const float (&value)[3], const float (&cx)[3], float (&out)[3])
{
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = SOURCE == EMIT_X ? value[c] : __fdiv_rn(value[c], a.corr);
    if (COLOUR == EMIT_LUMA) {
        const float dr = v[0] - cx[0], dg = v[1] - cx[1], db = v[2] - cx[2];
        const float l = (LUMA_R * dr + LUMA_G * dg) + LUMA_B * db;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = (cx[c] + kMean[c]) + l;
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = v[c] + kMean[c];
    }
}

__device__ __forceinline__ void emit_store(float* hwc, const float (&r)[1][3])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) hwc[c] = r[0][c];
}
// four pixels: their 12 consecutive floats as three 16-byte writes
__device__ __forceinline__ void emit_store(float* hwc, const float (&r)[4][3])
{
    float4* out = reinterpret_cast<float4*>(hwc);
    out[0] = make_float4(r[0][0], r[0][1], r[0][2], r[1][0]);
    out[1] = make_float4(r[1][1], r[1][2], r[2][0], r[2][1]);
    out[2] = make_float4(r[2][2], r[3][0], r[3][1], r[3][2]);
}

// VEC: a thread owns 4 consecutive pixels -- 16-byte accesses on every plane of every stream; else one pixel per thread.  The updated
// mean without hwc is the update-only launch: it writes nothing but the mean.
template <int SOURCE, int COLOUR, bool VEC>
__global__ __launch_bounds__(256) void emit_k(const EmitArgs a)
{
    using T = typename std::conditional<VEC, float4, float>::type;
    constexpr int PX = VEC ? 4 : 1;
    const size_t plane = (size_t)a.H * a.W;
    const size_t n = plane / PX;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        T v[3], cx[3] = {T(), T(), T()};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t at = (size_t)c * plane + i * PX;
            if (COLOUR == EMIT_LUMA) cx[c] = *reinterpret_cast<const T*>(a.cx + at);
            v[c] = emit_load<SOURCE, T>(a, at);
        }
        if (SOURCE == EMIT_MEAN_UPDATED && !a.hwc) continue;
        float r[PX][3];
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            const float vp[3] = {lane(v[0], p), lane(v[1], p), lane(v[2], p)}, cp[3] = {lane(cx[0], p), lane(cx[1], p), lane(cx[2], p)};
            emit_finish<SOURCE, COLOUR>(a, vp, cp, r[p]);
        }
        emit_store(a.hwc + i * 3 * PX, r);
    }
}

template <int SOURCE, int COLOUR>
static void launch_form(const EmitArgs& a, bool vec, int grid, hipStream_t s)
{
    if (vec) emit_k<SOURCE, COLOUR, true><<<grid, 256, 0, s>>>(a);
    else emit_k<SOURCE, COLOUR, false><<<grid, 256, 0, s>>>(a);
}

template <int SOURCE>
static void launch_source(const EmitArgs& a, bool vec, int grid, hipStream_t s)
{
    if (a.colour == EMIT_LUMA) launch_form<SOURCE, EMIT_LUMA>(a, vec, grid, s);
    else launch_form<SOURCE, EMIT_ADD_MEAN>(a, vec, grid, s);
}

hipError_t launch_emit(const EmitArgs& a, hipStream_t s)
{
    const size_t plane = (size_t)a.H * a.W;
    if (!plane) return hipSuccess;
    if ((a.source != EMIT_MEAN_READ && !a.x) || (a.source != EMIT_X && !a.mean) || (a.source != EMIT_MEAN_UPDATED && !a.hwc)) return hipErrorInvalidValue;
    if ((a.colour == EMIT_LUMA && !a.cx) || (a.colour != EMIT_LUMA && a.colour != EMIT_ADD_MEAN)) return hipErrorInvalidValue;
    const bool vec = plane % 4 == 0 && (((uintptr_t)a.x | (uintptr_t)a.mean | (uintptr_t)a.cx | (uintptr_t)a.hwc) & 15) == 0;
    const int grid = reduce_grid(vec ? plane / 4 : plane, 256, 2048);
    switch (a.source) {
    case EMIT_X: launch_source<EMIT_X>(a, vec, grid, s); break;
    case EMIT_MEAN_UPDATED: launch_source<EMIT_MEAN_UPDATED>(a, vec, grid, s); break;
    case EMIT_MEAN_READ: launch_source<EMIT_MEAN_READ>(a, vec, grid, s); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace st2
