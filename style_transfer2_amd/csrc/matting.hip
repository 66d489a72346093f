// The photorealism term (include/st2.h: st_set_matting; matting_plan.h: validation, buffer layout, tiles and grids): the matting
// Laplacian of the content image applied matrix-free, as a pair of 3x3-window passes.
//   matting_unit_k     I = cx / 255                                             } when the content image or the size changes,
//   matting_windows_k  per window: mu and the cofactor inverse M, in float64   } not on the hot path
//   matting_fit_k      first pass: per window and channel the affine fit (a, pb) of u on I, and the sums of J
//   matting_apply_k    second pass: per pixel Lu = the residuals of the windows that contain it, extra = prev + w (2 Lu), sums of g_mat^2
//   trace_matting_k    m_loss and m_grad join the image part of the trace
// Built with -ffp-contract=off: every operation below rounds once, in the order written (tests/matting_oracle.py restates it).
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

// the residual of one pixel in one window: the same expression in both passes, hence the same bits
__device__ __forceinline__ float residual(float dp, float a0, float a1, float a2, float d0, float d1, float d2)
{
    return dp - ((a0 * d0 + a1 * d1) + a2 * d2);
}
}  // namespace

__global__ __launch_bounds__(256) void matting_unit_k(const float* __restrict__ cx, float* __restrict__ I, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) I[i] = cx[i] / 255.0f;
}

// one window per thread and trip, float64, the nine pixels row-major
__global__ __launch_bounds__(256) void matting_windows_k(const MatWindowsArgs a)
{
    const size_t plane = (size_t)a.H * a.W;
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < a.windows; k += (size_t)gridDim.x * 256) {
        const int wy = (int)(k / a.Ww), wx = (int)(k % a.Ww);
        double d[3][9], mu[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                d[ch][i] = (double)a.I[ch * plane + (size_t)(wy + i / 3) * a.W + (wx + i % 3)];
                s += d[ch][i];
            }
            mu[ch] = s / 9.0;
#pragma unroll
            for (int i = 0; i < 9; ++i) d[ch][i] = d[ch][i] - mu[ch];
        }
        double s[3][3];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p; q < 3; ++q) {
                double t = 0.0;
#pragma unroll
                for (int i = 0; i < 9; ++i) t += d[p][i] * d[q][i];
                s[p][q] = t / 9.0;
            }
        const double e9 = a.eps / 9.0;
        const double s00 = s[0][0] + e9, s11 = s[1][1] + e9, s22 = s[2][2] + e9, s01 = s[0][1], s02 = s[0][2], s12 = s[1][2];
        const double c00 = s11 * s22 - s12 * s12;
        const double c01 = s02 * s12 - s01 * s22;
        const double c02 = s01 * s12 - s02 * s11;
        const double det = (s00 * c00 + s01 * c01) + s02 * c02;
        const double c11 = s00 * s22 - s02 * s02;
        const double c12 = s01 * s02 - s00 * s12;
        const double c22 = s00 * s11 - s01 * s01;
        float* mu_o = a.win + a.off_mu;
        float* M_o = a.win + a.off_M;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) mu_o[ch * a.windows + k] = (float)mu[ch];
        M_o[0 * a.windows + k] = (float)(c00 / det);
        M_o[1 * a.windows + k] = (float)(c01 / det);
        M_o[2 * a.windows + k] = (float)(c02 / det);
        M_o[3 * a.windows + k] = (float)(c11 / det);
        M_o[4 * a.windows + k] = (float)(c12 / det);
        M_o[5 * a.windows + k] = (float)(c22 / det);
    }
}

hipError_t launch_mat_windows(const float* cx, float* I, size_t pixels, const MatWindowsArgs& a, hipStream_t s)
{
    if (!cx || !I || !a.I || !a.win || a.H < 3 || a.W < 3 || a.Ww != a.W - 2 || a.windows != (size_t)(a.H - 2) * a.Ww || pixels != (size_t)3 * a.H * a.W)
        return hipErrorInvalidValue;
    matting_unit_k<<<reduce_grid(pixels, 256, kMatMaxBlocks), 256, 0, s>>>(cx, I, pixels);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    matting_windows_k<<<reduce_grid(a.windows, 256, kMatMaxBlocks), 256, 0, s>>>(a);
    return hipGetLastError();
}

// First pass.  The LDS tile holds u = x / 255 and I of the (kMatTileH + 2) x (kMatTileW + 2) pixels the tile's windows cover: every pixel
// is read from memory once per tile, not nine times.
__global__ __launch_bounds__(kMatThreads) void matting_fit_k(const MatFitArgs a)
{
    __shared__ float tile[kMatFitPlanes][kMatLdsH][kMatLdsW];
    __shared__ float scratch[4];
    const int tx = threadIdx.x % kMatTileW, ty = threadIdx.x / kMatTileW;
    const size_t plane = (size_t)a.H * a.W;
    const float* mu_i = a.win + a.off_mu;
    const float* M_i = a.win + a.off_M;
    double acc = 0.0;
    for (size_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const int wy0 = (int)(t / a.tiles_x) * kMatTileH, wx0 = (int)(t % a.tiles_x) * kMatTileW;
        __syncthreads();                                   // the previous tile has been read
        for (int i = threadIdx.x; i < kMatFitPlanes * kMatLdsH * kMatLdsW; i += kMatThreads) {
            const int p = i / (kMatLdsH * kMatLdsW), r = i % (kMatLdsH * kMatLdsW), ly = r / kMatLdsW, lx = r % kMatLdsW;
            const int y = wy0 + ly, x = wx0 + lx;
            float v = 0.f;
            if (y < a.H && x < a.W) {
                const size_t at = (size_t)(p % 3) * plane + (size_t)y * a.W + x;
                v = p < 3 ? a.x[at] / 255.0f : a.I[at];
            }
            tile[p][ly][lx] = v;
        }
        __syncthreads();
        const int wy = wy0 + ty, wx = wx0 + tx;
        if (wy < a.Hw && wx < a.Ww) {
            const size_t k = (size_t)wy * a.Ww + wx;
            float dI[3][9], M[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) M[j] = M_i[j * a.windows + k];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float mu = mu_i[ch * a.windows + k];
#pragma unroll
                for (int i = 0; i < 9; ++i) dI[ch][i] = tile[3 + ch][ty + i / 3][tx + i % 3] - mu;
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float dp[9], s = 0.f;
#pragma unroll
                for (int i = 0; i < 9; ++i) { dp[i] = tile[ch][ty + i / 3][tx + i % 3]; s += dp[i]; }
                const float pb = s / 9.0f;
#pragma unroll
                for (int i = 0; i < 9; ++i) dp[i] = dp[i] - pb;
                float cov[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    float c = 0.f;
#pragma unroll
                    for (int i = 0; i < 9; ++i) c += dI[q][i] * dp[i];
                    cov[q] = c / 9.0f;
                }
                const float a0 = (M[0] * cov[0] + M[1] * cov[1]) + M[2] * cov[2];
                const float a1 = (M[1] * cov[0] + M[3] * cov[1]) + M[4] * cov[2];
                const float a2 = (M[2] * cov[0] + M[4] * cov[1]) + M[5] * cov[2];
                double J = 0.0;
#pragma unroll
                for (int i = 0; i < 9; ++i) {
                    const float r = residual(dp[i], a0, a1, a2, dI[0][i], dI[1][i], dI[2][i]);
                    J += (double)r * (double)r;
                }
                const double q = ((double)a0 * (double)a0 + (double)a1 * (double)a1) + (double)a2 * (double)a2;
                J = J + a.eps * q;
                acc += J;
                float* o = a.ab + (size_t)(ch * 4) * a.windows + k;
                o[0] = a0; o[a.windows] = a1; o[2 * a.windows] = a2; o[3 * a.windows] = pb;
            }
        }
    }
    const float part = block_sum_of(acc, scratch);
    if (threadIdx.x == 0) a.part[blockIdx.x] = part;
}

hipError_t launch_mat_fit(const MatFitArgs& a, int grid, hipStream_t s)
{
    if (!a.x || !a.I || !a.win || !a.ab || !a.part || a.H < 3 || a.W < 3 || a.Hw != a.H - 2 || a.Ww != a.W - 2 || a.tiles_x < 1 || a.tiles < 1 ||
        a.windows != (size_t)a.Hw * a.Ww || grid < 1 || grid > kMatMaxBlocks || (size_t)grid > a.tiles)
        return hipErrorInvalidValue;
    if (a.tiles != (size_t)a.tiles_x * ((a.Hw + kMatTileH - 1) / kMatTileH) || a.tiles_x != (a.Ww + kMatTileW - 1) / kMatTileW) return hipErrorInvalidValue;
    matting_fit_k<<<grid, kMatThreads, 0, s>>>(a);
    return hipGetLastError();
}

// Second pass.  The LDS tile holds a, pb of the three channels and mu of the (kMatTileH + 2) x (kMatTileW + 2) windows that contain the
// tile's pixels (windows that do not exist stay unread); the pixel's own u and I come from memory, once.
__global__ __launch_bounds__(kMatThreads) void matting_apply_k(const MatApplyArgs a)
{
    __shared__ float tile[kMatApplyPlanes][kMatLdsH][kMatLdsW];
    __shared__ float scratch[4];
    const int tx = threadIdx.x % kMatTileW, ty = threadIdx.x / kMatTileW;
    const size_t plane = (size_t)a.H * a.W;
    const float* mu_i = a.win + a.off_mu;
    const bool has_prev = a.prev != nullptr;               // uniform
    double acc = 0.0;
    for (size_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const int py0 = (int)(t / a.tiles_x) * kMatTileH, px0 = (int)(t % a.tiles_x) * kMatTileW;
        __syncthreads();                                   // the previous tile has been read
        for (int i = threadIdx.x; i < kMatApplyPlanes * kMatLdsH * kMatLdsW; i += kMatThreads) {
            const int p = i / (kMatLdsH * kMatLdsW), r = i % (kMatLdsH * kMatLdsW), ly = r / kMatLdsW, lx = r % kMatLdsW;
            const int wy = py0 - 2 + ly, wx = px0 - 2 + lx;
            float v = 0.f;
            if (wy >= 0 && wy < a.Hw && wx >= 0 && wx < a.Ww) {
                const size_t k = (size_t)wy * a.Ww + wx;
                v = p < 12 ? a.ab[(size_t)p * a.windows + k] : mu_i[(size_t)(p - 12) * a.windows + k];
            }
            tile[p][ly][lx] = v;
        }
        __syncthreads();
        const int y = py0 + ty, x = px0 + tx;
        if (y < a.H && x < a.W) {
            const size_t at = (size_t)y * a.W + x;
            float u[3], I[3], Lu[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) { u[ch] = a.x[ch * plane + at] / 255.0f; I[ch] = a.I[ch * plane + at]; }
#pragma unroll
            for (int j = 0; j < 9; ++j) {                   // the windows centred at (y - 1 .. y + 1, x - 1 .. x + 1), row-major, those that exist
                const int ly = ty + j / 3, lx = tx + j % 3;
                const int wy = y - 2 + j / 3, wx = x - 2 + j % 3;
                if (wy < 0 || wy >= a.Hw || wx < 0 || wx >= a.Ww) continue;
                const float d0 = I[0] - tile[12][ly][lx], d1 = I[1] - tile[13][ly][lx], d2 = I[2] - tile[14][ly][lx];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float dp = u[ch] - tile[ch * 4 + 3][ly][lx];
                    Lu[ch] += residual(dp, tile[ch * 4][ly][lx], tile[ch * 4 + 1][ly][lx], tile[ch * 4 + 2][ly][lx], d0, d1, d2);
                }
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float g = a.w * (2.0f * Lu[ch]);
                acc += (double)g * (double)g;
                a.extra[ch * plane + at] = has_prev ? a.prev[ch * plane + at] + g : g;
            }
        }
    }
    const float part = block_sum_of(acc, scratch);
    if (threadIdx.x == 0) a.part[blockIdx.x] = part;
}

hipError_t launch_mat_apply(const MatApplyArgs& a, int grid, hipStream_t s)
{
    if (!a.x || !a.I || !a.win || !a.ab || !a.extra || !a.part || a.H < 3 || a.W < 3 || a.Hw != a.H - 2 || a.Ww != a.W - 2 ||
        a.windows != (size_t)a.Hw * a.Ww || grid < 1 || grid > kMatMaxBlocks || (size_t)grid > a.tiles || a.tiles < 1)
        return hipErrorInvalidValue;
    if (a.tiles != (size_t)a.tiles_x * ((a.H + kMatTileH - 1) / kMatTileH) || a.tiles_x != (a.W + kMatTileW - 1) / kMatTileW) return hipErrorInvalidValue;
    matting_apply_k<<<grid, kMatThreads, 0, s>>>(a);
    return hipGetLastError();
}

// the term's two trace scalars: one workgroup sums the two partial rows in double, thread 0 widens the image part of the trace
__global__ __launch_bounds__(256) void trace_matting_k(const TraceMatArgs a)
{
    __shared__ double scratch[256];
    const double sum_j = sum_partials(a.part, a.count_l, scratch);
    const double sum_g2 = a.count_g > 0 ? sum_partials(a.part + kMatMaxBlocks, a.count_g, scratch) : 0.0;      // uniform
    if (threadIdx.x != 0) return;
    // volatile: the slots are read and rewritten in place.  Plain loads of these uniform addresses compile to scalar loads, which the
    // vector stores below do not wait for -- a slot could be read after this thread had overwritten it (seen under graph replay)
    volatile float* g = a.image_out;
    const int half = 3 + a.others;                         // losses, then as many gradient norms, then loss and grad
    const float m_loss = a.w * (float)sum_j;
    const float m_grad = a.have_grad ? sqrtf((float)(sum_g2 / a.image_n)) : 0.f;
    float norms[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) norms[k] = k < half ? g[half + k] : 0.f;
    const float loss = g[2 * half], grad = g[2 * half + 1];
    g[half] = m_loss;
#pragma unroll
    for (int k = 0; k < 5; ++k) if (k < half) g[half + 1 + k] = norms[k];
    g[2 * half + 1] = m_grad;
    g[2 * half + 2] = loss + m_loss;
    g[2 * half + 3] = grad;
}

hipError_t launch_trace_mat(const TraceMatArgs& a, hipStream_t s)
{
    if (!a.part || !a.image_out || a.count_l < 1 || a.count_l > kMatMaxBlocks || a.count_g < 0 || a.count_g > kMatMaxBlocks || a.others < 0 || a.others > 2)
        return hipErrorInvalidValue;
    trace_matting_k<<<1, 256, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace st2
