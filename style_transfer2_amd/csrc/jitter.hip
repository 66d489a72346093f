// Jitter (include/st2.h: st_set_jitter; jitter_plan.h: the shift sequence, the source index and the grids).  One HBM-bound pass:
//   roll_k        dst = roll(src, (dy, dx)) over the three planes of (3, H, W): every element is read once and written once
//   roll_sumsq_k  the sums of squares the image pass would take of planes it is NOT given: the trace's scd_grad is that of the shifted
//                 evaluation, and a sum of fp32 squares over the un-rolled planes visits them in another order
// roll_k: no arithmetic on the values, no atomics, no LDS.  Built with -ffp-contract=off (roll_sumsq_k rounds like image_pass_k).
// A roll_k workgroup is one wave along a row times kJitBlockY rows; a thread takes kJitRows rows per trip and issues every load of the
// trip before its first store, so that a wave keeps kJitRows (16-byte form: 4 kJitRows) dword loads in flight.
#include "st2_kernels.h"
#include "wave_reduce.h"
#include <stdint.h>

namespace st2 {
// VEC: a lane owns four consecutive destination pixels of a row (W % 4 == 0, dst 16-byte aligned) and stores them as one float4.  Their
// sources start at an arbitrary column and may wrap at the row end: four dword loads.  Otherwise a lane owns one pixel.
template <bool VEC>
__global__ __launch_bounds__(kJitBlockX * kJitBlockY) void roll_k(const float* __restrict__ src, float* __restrict__ dst,
                                                                 int H, int W, int rows, int dy, int dx)
{
    constexpr int PX = VEC ? 4 : 1;
    const int x0 = (int)(blockIdx.x * kJitBlockX + threadIdx.x) * PX;
    if (x0 >= W) return;
    int sx[PX];
    sx[0] = jitter_src(x0, dx, W);
#pragma unroll
    for (int j = 1; j < PX; ++j) sx[j] = sx[j - 1] + 1 == W ? 0 : sx[j - 1] + 1;
    for (long long row0 = (long long)blockIdx.y * kJitTripRows + threadIdx.y; row0 < rows; row0 += (long long)gridDim.y * kJitTripRows) {
        float v[kJitRows][PX];
#pragma unroll
        for (int r = 0; r < kJitRows; ++r) {               // every load of the trip before its first store
            const long long row = row0 + r * kJitBlockY;
            if (row < rows) {
                const int ch = (int)(row / H), y = (int)(row - (long long)ch * H);
                const float* s = src + ((size_t)ch * H + jitter_src(y, dy, H)) * W;
#pragma unroll
                for (int j = 0; j < PX; ++j) v[r][j] = s[sx[j]];
            }
        }
#pragma unroll
        for (int r = 0; r < kJitRows; ++r) {
            const long long row = row0 + r * kJitBlockY;
            if (row < rows) {
                float* d = dst + (size_t)row * W + x0;
                if constexpr (VEC) *reinterpret_cast<float4*>(d) = make_float4(v[r][0], v[r][1], v[r][2], v[r][3]);
                else *d = v[r][0];
            }
        }
    }
}

// image_pass_k's walk (passes.hip: tiles of 4 rows x 256 columns of one channel, a thread owns a column, a workgroup strides over the
// tiles) and its accumulation acc += v * v in fp32, then the same block_sum: partial[block] has the bits that kernel writes into its
// scd row when `planes` is its scd and `grid` its grid.  The tile shape is restated here; tests/test_gpu_jitter.py holds the two together
constexpr int kIpTileY = 4, kIpTileX = 256;
__global__ __launch_bounds__(256) void roll_sumsq_k(const float* __restrict__ planes, int C, int H, int W, float* __restrict__ partial)
{
    __shared__ float scratch[4];
    const int tid = threadIdx.x;
    const size_t plane = (size_t)H * W;
    const int tiles_x = (W + kIpTileX - 1) / kIpTileX, tiles_y = (H + kIpTileY - 1) / kIpTileY;
    const int n_tiles = C * tiles_y * tiles_x;
    float acc[1] = {0.f};
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int tx = tile % tiles_x, rest = tile / tiles_x;
        const int ty = rest % tiles_y, ch = rest / tiles_y;
        const int x = tx * kIpTileX + tid, y0 = ty * kIpTileY;
        if (x < W) {
#pragma unroll
            for (int ry = 0; ry < kIpTileY; ++ry) {
                const int y = y0 + ry;
                if (y >= H) break;
                const float v = planes[(size_t)ch * plane + (size_t)y * W + x];
                acc[0] += v * v;
            }
        }
    }
    block_sum(acc, scratch);
    if (tid == 0) partial[blockIdx.x] = acc[0];
}

hipError_t launch_roll_sumsq(const float* planes, int H, int W, int grid, float* partial, hipStream_t s)
{
    const long long n_tiles = 3ll * ((H + kIpTileY - 1) / kIpTileY) * ((W + kIpTileX - 1) / kIpTileX);
    if (!planes || !partial || H < 1 || W < 1 || grid < 1 || grid > kMaxPartials || grid > n_tiles) return hipErrorInvalidValue;
    roll_sumsq_k<<<grid, 256, 0, s>>>(planes, 3, H, W, partial);
    return hipGetLastError();
}

hipError_t launch_roll(const float* src, float* dst, const JitterPlan& p, hipStream_t s)
{
    if (!src || !dst || src == dst || p.H < 1 || p.W < 1 || p.rows != 3 * p.H || p.dy < 0 || p.dy >= p.H || p.dx < 0 || p.dx >= p.W)
        return hipErrorInvalidValue;
    const bool vec = p.row_vec && p.W % 4 == 0 && ((uintptr_t)dst & 15) == 0;
    const unsigned gx = vec ? p.gx_vec : p.gx, gy = vec ? p.gy_vec : p.gy;
    if (gx < 1 || gy < 1 || gy > (unsigned)kJitMaxGridY || (unsigned long long)gx * kJitBlockX * (vec ? 4 : 1) < (unsigned long long)p.W)
        return hipErrorInvalidValue;
    const dim3 grid(gx, gy), block(kJitBlockX, kJitBlockY);
    if (vec) roll_k<true><<<grid, block, 0, s>>>(src, dst, p.H, p.W, p.rows, p.dy, p.dx);
    else roll_k<false><<<grid, block, 0, s>>>(src, dst, p.H, p.W, p.rows, p.dy, p.dx);
    return hipGetLastError();
}
}  // namespace st2
