// The Laplacian-steered content term (include/st2.h: st_set_laplacian; laplacian_plan.h: the geometry).  Three HBM-bound passes:
//   lap_pool_k     u = x / 255 pooled at every configured level in one read of x (the pool sizes nest inside a 32 x 64 tile)
//   lap_stencil_k  E = D(P(u)) - T per level and the per-workgroup sums of E^2 (target form: T = D(P(u)) of the content image)
//   lap_grad_k     g_lap = sum over levels of w * 2 * D(E) / count per pixel, and the per-workgroup sums of g_lap^2
// Built with -ffp-contract=off: every fp32 operation below rounds once, in the order written (tests/laplacian_oracle.py restates it).
#include "st2_kernels.h"
#include "wave_reduce.h"
#include <stdint.h>

namespace st2 {
namespace {
// LDS of the pooling pass: the 32 x 64 tile of u, then its 2 x 2 sums level by level (16 x 32, 8 x 16, 4 x 8, 2 x 4, 1 x 2)
constexpr int kPoolLds = 2048 + 512 + 128 + 32 + 8 + 2;
__device__ __forceinline__ int pool_lds_off(int k) { return k == 0 ? 0 : k == 1 ? 2048 : k == 2 ? 2560 : k == 3 ? 2688 : k == 4 ? 2720 : 2728; }

// a thread's sum of squares (double) -> the workgroup's fp32 partial in thread 0
__device__ __forceinline__ float block_sum_sq(double acc, float* scratch)
{
    float v[1] = {(float)acc};
    block_sum(v, scratch);
    return v[0];
}

// D(q) at cell (i, j) of an hp x wp grid stored with pitch wp at q: sum of (q - neighbour) over the neighbours that exist, in the
// order up, down, left, right
__device__ __forceinline__ float lap_at(const float* __restrict__ q, int i, int j, int hp, int wp)
{
    const size_t at = (size_t)i * wp + j;
    const float c = q[at];
    float d = 0.f;
    if (i > 0) d += c - q[at - wp];
    if (i + 1 < hp) d += c - q[at + wp];
    if (j > 0) d += c - q[at - 1];
    if (j + 1 < wp) d += c - q[at + 1];
    return d;
}
}  // namespace

// One workgroup walks tiles of 32 rows x 64 columns of one channel; a thread stages 8 consecutive pixels of one row (VEC: as two
// 16-byte loads) as u = x / 255, pixels outside the image as 0.  The sums of the 2 x 2, 4 x 4, ... windows follow in LDS, each from the
// four sums of the level below as (a + b) + (c + d); a configured level's mean is its sum divided by the clipped window's pixel count.
template <bool VEC>
__global__ __launch_bounds__(256) void lap_pool_k(const LapPoolArgs a)
{
    __shared__ float s[kPoolLds];
    const int H = a.H, W = a.W, tid = threadIdx.x;
    const size_t plane = (size_t)H * W;
    const int n_tiles = 3 * a.tiles_y * a.tiles_x;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int tx = tile % a.tiles_x, rest = tile / a.tiles_x;
        const int ty = rest % a.tiles_y, ch = rest / a.tiles_y;
        const int x0 = tx * kLapTileX, y0 = ty * kLapTileY;
        __syncthreads();                                   // the previous tile is consumed
        {
            const int r = tid >> 3, c0 = (tid & 7) * 8;
            const int gy = y0 + r, gx = x0 + c0;
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (gy < H) {
                const float* row = a.x + (size_t)ch * plane + (size_t)gy * W;
                if (VEC) {
#pragma unroll
                    for (int k = 0; k < 2; ++k)
                        if (gx + 4 * k < W) {              // W % 4 == 0: four pixels are inside together
                            const float4 q = *reinterpret_cast<const float4*>(row + gx + 4 * k);
                            v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
                        }
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k) if (gx + k < W) v[k] = row[gx + k];
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) s[r * kLapTileX + c0 + k] = v[k] / 255.0f;
        }
        __syncthreads();
        for (int k = 1; k <= a.max_shift; ++k) {           // uniform
            const int cols = kLapTileX >> k, n = (kLapTileY >> k) * cols, cols2 = cols * 2;
            const float* src = s + pool_lds_off(k - 1);
            float* dst = s + pool_lds_off(k);
            for (int e = tid; e < n; e += 256) {
                const int i = e / cols, j = e - i * cols;
                const float* p = src + (2 * i) * cols2 + 2 * j;
                dst[e] = (p[0] + p[1]) + (p[cols2] + p[cols2 + 1]);
            }
            __syncthreads();
        }
        for (int l = 0; l < a.n; ++l) {
            const int k = a.shift[l], hp = a.hp[l], wp = a.wp[l];
            const int cols = kLapTileX >> k, n = (kLapTileY >> k) * cols;
            const float* src = s + pool_lds_off(k);
            float* q = a.q + a.off[l] + (size_t)ch * hp * wp;
            for (int e = tid; e < n; e += 256) {
                const int i = e / cols, j = e - i * cols;
                const int ci = (y0 >> k) + i, cj = (x0 >> k) + j;
                if (ci >= hp || cj >= wp) continue;
                const int y1 = min(H, (ci + 1) << k), x1 = min(W, (cj + 1) << k);
                const float count = (float)((y1 - (ci << k)) * (x1 - (cj << k)));
                q[(size_t)ci * wp + cj] = src[e] / count;
            }
        }
    }
}

hipError_t launch_lap_pool(const LapPoolArgs& a, int grid, hipStream_t s)
{
    if (!a.x || !a.q || a.n < 1 || a.n > kLapMaxLevels || a.H < 1 || a.W < 1 || grid < 1) return hipErrorInvalidValue;
    const bool vec = a.W % 4 == 0 && ((uintptr_t)a.x & 15) == 0;
    if (vec) lap_pool_k<true><<<grid, 256, 0, s>>>(a);
    else lap_pool_k<false><<<grid, 256, 0, s>>>(a);
    return hipGetLastError();
}

// blockIdx.y: the level.  target form (a.e == NULL): T = D(q); else E = D(q) - T, and part[level][blockIdx.x] = this workgroup's sum E^2
__global__ __launch_bounds__(256) void lap_stencil_k(const LapStencilArgs a)
{
    __shared__ float scratch[4];
    const int l = blockIdx.y;
    const int hp = a.hp[l], wp = a.wp[l];
    const size_t cells = (size_t)hp * wp, n = 3 * cells, off = a.off[l];
    const float* q = a.q + off;
    double acc = 0.0;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (size_t)gridDim.x * 256) {
        const size_t ch = idx / cells, rem = idx - ch * cells;
        const int i = (int)(rem / wp), j = (int)(rem - (size_t)i * wp);
        const float d = lap_at(q + ch * cells, i, j, hp, wp);
        if (!a.e) { a.t[off + idx] = d; continue; }
        const float e = d - a.t[off + idx];
        a.e[off + idx] = e;
        acc += (double)e * (double)e;
    }
    if (!a.e) return;                                      // uniform
    const float sum = block_sum_sq(acc, scratch);
    if (threadIdx.x == 0) a.part[(size_t)l * kLapMaxBlocks + blockIdx.x] = sum;
}

hipError_t launch_lap_stencil(const LapStencilArgs& a, int grid, hipStream_t s)
{
    if (!a.q || !a.t || (a.e && !a.part) || a.n < 1 || a.n > kLapMaxLevels || grid < 1 || grid > kLapMaxBlocks) return hipErrorInvalidValue;
    lap_stencil_k<<<dim3(grid, a.n), 256, 0, s>>>(a);
    return hipGetLastError();
}

// one pixel's (PX == 1) or four consecutive pixels' (PX == 4, x a multiple of 4) g_lap; a cell's term is computed once for the pixels
// of the group that share it
template <int PX>
__device__ __forceinline__ void lap_grad_px(const LapGradArgs& a, int ch, int y, int x, float (&g)[PX])
{
#pragma unroll
    for (int p = 0; p < PX; ++p) g[p] = 0.f;
    for (int l = 0; l < a.n; ++l) {
        const int k = a.shift[l], hp = a.hp[l], wp = a.wp[l];
        const float* e = a.e + a.off[l] + (size_t)ch * hp * wp;
        const int ci = y >> k;
        const int y1 = min(a.H, (ci + 1) << k);
        const int rows = y1 - (ci << k);
        float term = 0.f;
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            if (p == 0 || ((x + p) & ((1 << k) - 1)) == 0) {
                const int cj = (x + p) >> k;
                const int x1 = min(a.W, (cj + 1) << k);
                const float count = (float)(rows * (x1 - (cj << k)));
                const float d = lap_at(e, ci, cj, hp, wp);
                term = (a.w[l] * (2.0f * d)) / count;
            }
            g[p] += term;
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void lap_grad_k(const LapGradArgs a)
{
    __shared__ float scratch[4];
    constexpr int PX = VEC ? 4 : 1;
    const size_t plane = (size_t)a.H * a.W;
    const size_t n = 3 * plane / PX;
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t at = i * PX;
        const int ch = (int)(at / plane);
        const size_t rem = at - (size_t)ch * plane;
        const int y = (int)(rem / a.W), x = (int)(rem - (size_t)y * a.W);
        float g[PX];
        lap_grad_px<PX>(a, ch, y, x, g);
#pragma unroll
        for (int p = 0; p < PX; ++p) acc += (double)g[p] * (double)g[p];
        if constexpr (VEC) *reinterpret_cast<float4*>(a.g + at) = make_float4(g[0], g[1], g[2], g[3]);
        else a.g[at] = g[0];
    }
    const float sum = block_sum_sq(acc, scratch);
    if (threadIdx.x == 0) a.part[blockIdx.x] = sum;
}

hipError_t launch_lap_grad(const LapGradArgs& a, int grid, int grid_vec, hipStream_t s)
{
    if (!a.e || !a.g || !a.part || a.n < 1 || a.n > kLapMaxLevels || a.H < 1 || a.W < 1) return hipErrorInvalidValue;
    const bool vec = a.W % 4 == 0 && ((uintptr_t)a.g & 15) == 0;
    const int gr = vec ? grid_vec : grid;
    if (gr < 1 || gr > kLapMaxBlocks) return hipErrorInvalidValue;
    if (vec) lap_grad_k<true><<<gr, 256, 0, s>>>(a);
    else lap_grad_k<false><<<gr, 256, 0, s>>>(a);
    return hipGetLastError();
}

// the term's two trace scalars: one workgroup sums the partial rows in double, thread 0 widens the image part of the trace
__global__ __launch_bounds__(256) void trace_lap_k(const TraceLapArgs a)
{
    __shared__ double scratch[256];
    double sums[kLapPartRows];
#pragma unroll
    for (int r = 0; r < kLapPartRows; ++r) {
        const int count = r < kLapMaxLevels ? (r < a.levels ? a.count_e : 0) : a.count_g;      // uniform
        sums[r] = count > 0 ? sum_partials(a.part + (size_t)r * kLapMaxBlocks, count, scratch) : 0.0;
    }
    if (threadIdx.x != 0) return;
    float* g = a.image_out;
    float l_loss = 0.f;
    for (int l = 0; l < a.levels; ++l) l_loss += a.w[l] * (float)sums[l];
    const float l_grad = a.have_grad ? sqrtf((float)(sums[kLapMaxLevels] / a.image_n)) : 0.f;
    const float scd_grad = g[3], tv_grad = g[4], p_grad = g[5], loss = g[6], grad = g[7];
    g[3] = l_loss; g[4] = scd_grad; g[5] = tv_grad; g[6] = p_grad; g[7] = l_grad;
    g[8] = loss + l_loss;
    g[9] = grad;
}

hipError_t launch_trace_lap(const TraceLapArgs& a, hipStream_t s)
{
    if (!a.part || !a.image_out || a.levels < 1 || a.levels > kLapMaxLevels || a.count_e < 1 || a.count_e > kLapMaxBlocks || a.count_g < 0 || a.count_g > kLapMaxBlocks)
        return hipErrorInvalidValue;
    trace_lap_k<<<1, 256, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace st2
