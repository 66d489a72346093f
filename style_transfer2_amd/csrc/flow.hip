// Optical flow (include/st2.h: st_flow_estimate; flow_plan.h: validation, level geometry, grids, route).  Coarse-to-fine Horn-Schunck
// with warping and Jacobi inner iterations, every block a stencil:
//   flow_luma_k        level 0 of both pyramids from the staged HWC images
//   flow_pool_k        the next level of both pyramids: 2 x 2 / stride 2 averages in Caffe's ceil mode (the P(u) of the Laplacian block)
//   flow_smooth_k      the [1 2 1] / 4 smoothing of a level along x, then y, borders replicated; both images
//   flow_start_k       the flow a level starts from
//   flow_linear_k      one warp: Bw = bilinear(to, p + f) at the pixel and its four clamped neighbours (recomputed, the same arithmetic
//                      as the neighbour's own), Ix, Iy, c, den
//   flow_jacobi_k      one Jacobi iteration from one pair of planes into another; 16-byte form where w % 4 == 0
//   flow_jacobi_wg_k   every iteration of a warp in one workgroup: u and v ping-pong in LDS, the coefficients stay in registers
//   flow_interleave_k  (u, v) -> (h, w, 2)
// No atomics anywhere: every output element is written by one thread from inputs no launch changes while it runs.
// Built with -ffp-contract=off: every operation below rounds once, in the order written; the divisions are IEEE.
#include "st2_kernels.h"
#include <stdint.h>

namespace st2 {
namespace {
constexpr int kT = 256;

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <bool U8>
__global__ __launch_bounds__(kT) void flow_luma_k(const void* s0, const void* s1, float* d0, float* d1, size_t n)
{
    const void* src = blockIdx.y ? s1 : s0;
    float* dst = blockIdx.y ? d1 : d0;
    for (size_t i = (size_t)blockIdx.x * kT + threadIdx.x; i < n; i += (size_t)gridDim.x * kT) {
        float r, g, b;
        if constexpr (U8) {
            const unsigned char* p = static_cast<const unsigned char*>(src) + 3 * i;
            r = (float)p[0]; g = (float)p[1]; b = (float)p[2];
        } else {
            const float* p = static_cast<const float*>(src) + 3 * i;
            r = p[0]; g = p[1]; b = p[2];
        }
        dst[i] = __fdiv_rn((0.299f * r + 0.587f * g) + 0.114f * b, 255.f);
    }
}

// (h, w) -> (h2, w2) = (ceil(h / 2), ceil(w / 2)); pixels outside count 0, the divisor is the clipped window's size
__global__ __launch_bounds__(kT) void flow_pool_k(const float* s0, const float* s1, float* d0, float* d1, int h, int w, int h2, int w2)
{
    const float* src = blockIdx.y ? s1 : s0;
    float* dst = blockIdx.y ? d1 : d0;
    const size_t n = (size_t)h2 * w2;
    for (size_t i = (size_t)blockIdx.x * kT + threadIdx.x; i < n; i += (size_t)gridDim.x * kT) {
        const int Y = (int)(i / (size_t)w2), X = (int)(i - (size_t)Y * w2);
        const int y0 = 2 * Y, x0 = 2 * X;
        const bool right = x0 + 1 < w, down = y0 + 1 < h;
        const float* row = src + (size_t)y0 * w + x0;
        const float a = row[0];
        const float b = right ? row[1] : 0.f;
        const float c = down ? row[w] : 0.f;
        const float d = (right && down) ? row[w + 1] : 0.f;
        const float count = (float)((right ? 2 : 1) * (down ? 2 : 1));
        dst[i] = __fdiv_rn((a + b) + (c + d), count);
    }
}

__device__ __forceinline__ float smooth_row(const float* row, int xm, int x, int xp) { return ((row[xm] + row[xp]) + 2.f * row[x]) * 0.25f; }

__global__ __launch_bounds__(kT) void flow_smooth_k(const float* s0, const float* s1, float* d0, float* d1, int h, int w)
{
    const float* src = blockIdx.y ? s1 : s0;
    float* dst = blockIdx.y ? d1 : d0;
    const size_t n = (size_t)h * w;
    for (size_t i = (size_t)blockIdx.x * kT + threadIdx.x; i < n; i += (size_t)gridDim.x * kT) {
        const int y = (int)(i / (size_t)w), x = (int)(i - (size_t)y * w);
        const int xm = max(x - 1, 0), xp = min(x + 1, w - 1), ym = max(y - 1, 0), yp = min(y + 1, h - 1);
        const float tm = smooth_row(src + (size_t)ym * w, xm, x, xp);
        const float t0 = smooth_row(src + (size_t)y * w, xm, x, xp);
        const float tp = smooth_row(src + (size_t)yp * w, xm, x, xp);
        dst[i] = ((tm + tp) + 2.f * t0) * 0.25f;
    }
}

// uc == NULL: the coarsest level, a flow of 0
__global__ __launch_bounds__(kT) void flow_start_k(const float* uc, const float* vc, float* u, float* v, int h, int w, int wc)
{
    const size_t n = (size_t)h * w;
    for (size_t i = (size_t)blockIdx.x * kT + threadIdx.x; i < n; i += (size_t)gridDim.x * kT) {
        float a = 0.f, b = 0.f;
        if (uc) {
            const int y = (int)(i / (size_t)w), x = (int)(i - (size_t)y * w);
            const size_t at = (size_t)(y >> 1) * wc + (x >> 1);
            a = 2.f * uc[at]; b = 2.f * vc[at];
        }
        u[i] = a; v[i] = b;
    }
}

// Bw at pixel (y, x): `to` sampled at (x + u, y + v), clamped to the image
__device__ __forceinline__ float flow_sample(const float* B, const float* u, const float* v, int h, int w, int y, int x)
{
    const size_t at = (size_t)y * w + x;
    const float sx = fminf(fmaxf((float)x + u[at], 0.f), (float)(w - 1));
    const float sy = fminf(fmaxf((float)y + v[at], 0.f), (float)(h - 1));
    const float x0f = floorf(sx), y0f = floorf(sy);
    const int x0 = clampi((int)x0f, w - 1), y0 = clampi((int)y0f, h - 1);    // (inside already for finite flows; a NaN must not index)
    const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    const float fx = sx - x0f, fy = sy - y0f, gx = 1.f - fx, gy = 1.f - fy;
    const float* r0 = B + (size_t)y0 * w;
    const float* r1 = B + (size_t)y1 * w;
    const float top = r0[x0] * gx + r0[x1] * fx;
    const float bottom = r1[x0] * gx + r1[x1] * fx;
    return top * gy + bottom * fy;
}

__global__ __launch_bounds__(kT) void flow_linear_k(const float* A, const float* B, const float* u, const float* v, float* Ix, float* Iy,
                                                    float* c, float* den, int h, int w, float a2)
{
    const size_t n = (size_t)h * w;
    for (size_t i = (size_t)blockIdx.x * kT + threadIdx.x; i < n; i += (size_t)gridDim.x * kT) {
        const int y = (int)(i / (size_t)w), x = (int)(i - (size_t)y * w);
        const int xm = max(x - 1, 0), xp = min(x + 1, w - 1), ym = max(y - 1, 0), yp = min(y + 1, h - 1);
        const float bw = flow_sample(B, u, v, h, w, y, x);
        const float ix = 0.5f * (flow_sample(B, u, v, h, w, y, xp) - flow_sample(B, u, v, h, w, y, xm));
        const float iy = 0.5f * (flow_sample(B, u, v, h, w, yp, x) - flow_sample(B, u, v, h, w, ym, x));
        const float uu = u[i], vv = v[i];
        Ix[i] = ix; Iy[i] = iy;
        c[i] = ((bw - A[i]) - ix * uu) - iy * vv;
        den[i] = (a2 + ix * ix) + iy * iy;
    }
}

// one pixel of one iteration from the neighbour sums' operands
__device__ __forceinline__ void jacobi_px(float uu, float ud, float ul, float ur, float vu, float vd, float vl, float vr, float ix, float iy, float c,
                                          float den, float& un, float& vn)
{
    const float ub = ((uu + ud) + (ul + ur)) * 0.25f;
    const float vb = ((vu + vd) + (vl + vr)) * 0.25f;
    const float r = __fdiv_rn((ix * ub + iy * vb) + c, den);
    un = ub - ix * r;
    vn = vb - iy * r;
}

struct JacobiArgs { const float *u, *v, *ix, *iy, *c, *den; float *un, *vn; int h, w; };

// A thread takes one pixel (VEC: four consecutive ones of a row, 16-byte loads and stores) per trip; every load of a trip before its
// first store.  (un, vn) are other buffers than (u, v): a trip reads nothing another trip of the launch writes.
template <bool VEC>
__global__ __launch_bounds__(kT) void flow_jacobi_k(const JacobiArgs a)
{
    const int h = a.h, w = a.w;
    constexpr int PX = VEC ? 4 : 1;
    const size_t n = (size_t)h * w / PX;
    for (size_t i = (size_t)blockIdx.x * kT + threadIdx.x; i < n; i += (size_t)gridDim.x * kT) {
        const size_t at = i * PX;
        const int y = (int)(at / (size_t)w), x = (int)(at - (size_t)y * w);
        const size_t up = (size_t)max(y - 1, 0) * w + x, dn = (size_t)min(y + 1, h - 1) * w + x;
        if constexpr (VEC) {
            const float4 uu = *reinterpret_cast<const float4*>(a.u + up), ud = *reinterpret_cast<const float4*>(a.u + dn);
            const float4 vu = *reinterpret_cast<const float4*>(a.v + up), vd = *reinterpret_cast<const float4*>(a.v + dn);
            const float4 uc = *reinterpret_cast<const float4*>(a.u + at), vc = *reinterpret_cast<const float4*>(a.v + at);
            const size_t lf = (size_t)y * w + max(x - 1, 0), rt = (size_t)y * w + min(x + 4, w - 1);
            const float ul = a.u[lf], ur = a.u[rt], vl = a.v[lf], vr = a.v[rt];
            const float4 ix = *reinterpret_cast<const float4*>(a.ix + at), iy = *reinterpret_cast<const float4*>(a.iy + at);
            const float4 c = *reinterpret_cast<const float4*>(a.c + at), den = *reinterpret_cast<const float4*>(a.den + at);
            float4 un, vn;
            jacobi_px(uu.x, ud.x, ul, uc.y, vu.x, vd.x, vl, vc.y, ix.x, iy.x, c.x, den.x, un.x, vn.x);
            jacobi_px(uu.y, ud.y, uc.x, uc.z, vu.y, vd.y, vc.x, vc.z, ix.y, iy.y, c.y, den.y, un.y, vn.y);
            jacobi_px(uu.z, ud.z, uc.y, uc.w, vu.z, vd.z, vc.y, vc.w, ix.z, iy.z, c.z, den.z, un.z, vn.z);
            jacobi_px(uu.w, ud.w, uc.z, ur, vu.w, vd.w, vc.z, vr, ix.w, iy.w, c.w, den.w, un.w, vn.w);
            *reinterpret_cast<float4*>(a.un + at) = un;
            *reinterpret_cast<float4*>(a.vn + at) = vn;
        } else {
            const size_t lf = (size_t)y * w + max(x - 1, 0), rt = (size_t)y * w + min(x + 1, w - 1);
            const float uu = a.u[up], ud = a.u[dn], ul = a.u[lf], ur = a.u[rt];
            const float vu = a.v[up], vd = a.v[dn], vl = a.v[lf], vr = a.v[rt];
            const float ix = a.ix[at], iy = a.iy[at], c = a.c[at], den = a.den[at];
            float un, vn;
            jacobi_px(uu, ud, ul, ur, vu, vd, vl, vr, ix, iy, c, den, un, vn);
            a.un[at] = un;
            a.vn[at] = vn;
        }
    }
}

// One workgroup, n = h w <= kFlowWgMaxPixels: thread t owns the pixels t, t + 1024, t + 2048, t + 3072 that exist.  u and v are read
// once into LDS, `iters` iterations ping-pong between the two halves (one barrier each: an iteration writes the half the one before
// it read, and that one's reads end at its barrier), the result goes back to the planes it came from -- every global load of the launch
// is behind the first barrier, every global store after the last.
__global__ __launch_bounds__(kFlowWgThreads) void flow_jacobi_wg_k(float* u, float* v, const float* Ix, const float* Iy, const float* C, const float* Den,
                                                                     int h, int w, int iters)
{
    constexpr int K = kFlowWgPerThread, T = kFlowWgThreads, N = kFlowWgMaxPixels;
    __shared__ float su[2][N], sv[2][N];
    const int n = h * w, t = threadIdx.x;
    float ix[K], iy[K], c[K], den[K];
    int up[K], dn[K], lf[K], rt[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = t + k * T;
        ix[k] = iy[k] = c[k] = 0.f; den[k] = 1.f;
        up[k] = dn[k] = lf[k] = rt[k] = 0;
        if (i < n) {
            const int y = i / w, x = i - y * w;
            up[k] = max(y - 1, 0) * w + x; dn[k] = min(y + 1, h - 1) * w + x;
            lf[k] = y * w + max(x - 1, 0); rt[k] = y * w + min(x + 1, w - 1);
            ix[k] = Ix[i]; iy[k] = Iy[i]; c[k] = C[i]; den[k] = Den[i];
            su[0][i] = u[i]; sv[0][i] = v[i];
        }
    }
    __syncthreads();
    int cur = 0;
    for (int it = 0; it < iters; ++it) {
        const float* pu = su[cur];
        const float* pv = sv[cur];
        float* qu = su[cur ^ 1];
        float* qv = sv[cur ^ 1];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int i = t + k * T;
            if (i < n) {
                float un, vn;
                jacobi_px(pu[up[k]], pu[dn[k]], pu[lf[k]], pu[rt[k]], pv[up[k]], pv[dn[k]], pv[lf[k]], pv[rt[k]], ix[k], iy[k], c[k], den[k], un, vn);
                qu[i] = un; qv[i] = vn;
            }
        }
        __syncthreads();
        cur ^= 1;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = t + k * T;
        if (i < n) { u[i] = su[cur][i]; v[i] = sv[cur][i]; }
    }
}

__global__ __launch_bounds__(kT) void flow_interleave_k(const float* u, const float* v, float2* out, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * kT + threadIdx.x; i < n; i += (size_t)gridDim.x * kT) out[i] = make_float2(u[i], v[i]);
}

bool level_ok(const FlowPlan& p, const float* base, int l) { return base && l >= 0 && l < p.n && p.n <= kFlowMaxLevels; }
bool grid_ok(int g) { return g >= 1 && g <= kFlowMaxBlocks; }
}  // namespace

hipError_t launch_flow_luma(const FlowPlan& p, float* base, hipStream_t s)
{
    if (!level_ok(p, base, 0) || !grid_ok(p.grid0)) return hipErrorInvalidValue;
    const FlowLevel& L = p.lv[0];
    const dim3 grid(p.grid0, 2);
    if (p.is_u8) flow_luma_k<true><<<grid, kT, 0, s>>>(base + p.stage[0], base + p.stage[1], base + L.raw[0], base + L.raw[1], L.n);
    else flow_luma_k<false><<<grid, kT, 0, s>>>(base + p.stage[0], base + p.stage[1], base + L.raw[0], base + L.raw[1], L.n);
    return hipGetLastError();
}

hipError_t launch_flow_pool(const FlowPlan& p, float* base, int l, hipStream_t s)
{
    if (!level_ok(p, base, l) || l + 1 >= p.n) return hipErrorInvalidValue;
    const FlowLevel &L = p.lv[l], &M = p.lv[l + 1];
    if (M.h != (L.h + 1) / 2 || M.w != (L.w + 1) / 2 || !grid_ok(M.grid)) return hipErrorInvalidValue;
    flow_pool_k<<<dim3(M.grid, 2), kT, 0, s>>>(base + L.raw[0], base + L.raw[1], base + M.raw[0], base + M.raw[1], L.h, L.w, M.h, M.w);
    return hipGetLastError();
}

hipError_t launch_flow_smooth(const FlowPlan& p, float* base, int l, hipStream_t s)
{
    if (!level_ok(p, base, l) || !grid_ok(p.lv[l].grid)) return hipErrorInvalidValue;
    const FlowLevel& L = p.lv[l];
    flow_smooth_k<<<dim3(L.grid, 2), kT, 0, s>>>(base + L.raw[0], base + L.raw[1], base + L.img[0], base + L.img[1], L.h, L.w);
    return hipGetLastError();
}

hipError_t launch_flow_start(const FlowPlan& p, float* base, int l, hipStream_t s)
{
    if (!level_ok(p, base, l) || !grid_ok(p.lv[l].grid)) return hipErrorInvalidValue;
    const FlowLevel& L = p.lv[l];
    const bool coarsest = l == p.n - 1;
    if (!coarsest && (p.lv[l + 1].h != (L.h + 1) / 2 || p.lv[l + 1].w != (L.w + 1) / 2)) return hipErrorInvalidValue;
    flow_start_k<<<L.grid, kT, 0, s>>>(coarsest ? nullptr : base + p.lv[l + 1].u, coarsest ? nullptr : base + p.lv[l + 1].v, base + L.u, base + L.v, L.h,
                                       L.w, coarsest ? 0 : p.lv[l + 1].w);
    return hipGetLastError();
}

hipError_t launch_flow_linear(const FlowPlan& p, float* base, int l, const float* u, const float* v, hipStream_t s)
{
    if (!level_ok(p, base, l) || !u || !v || !grid_ok(p.lv[l].grid)) return hipErrorInvalidValue;
    const FlowLevel& L = p.lv[l];
    flow_linear_k<<<L.grid, kT, 0, s>>>(base + L.img[0], base + L.img[1], u, v, base + p.ix, base + p.iy, base + p.c, base + p.den, L.h, L.w, p.a2);
    return hipGetLastError();
}

hipError_t launch_flow_jacobi(const FlowPlan& p, float* base, int l, const float* u, const float* v, float* un, float* vn, hipStream_t s)
{
    if (!level_ok(p, base, l) || !u || !v || !un || !vn || u == un || v == vn || u == vn || v == un) return hipErrorInvalidValue;
    const FlowLevel& L = p.lv[l];
    const JacobiArgs a{u, v, base + p.ix, base + p.iy, base + p.c, base + p.den, un, vn, L.h, L.w};
    // the 16-byte form: groups of four stay inside a row, and every plane starts on a 16-byte boundary
    const uintptr_t bits = (uintptr_t)u | (uintptr_t)v | (uintptr_t)un | (uintptr_t)vn | (uintptr_t)a.ix | (uintptr_t)a.iy | (uintptr_t)a.c | (uintptr_t)a.den;
    const bool vec = L.row_vec && (bits & 15) == 0;
    const int gr = vec ? L.grid_vec : L.grid;
    if (!grid_ok(gr)) return hipErrorInvalidValue;
    if (vec) flow_jacobi_k<true><<<gr, kT, 0, s>>>(a);
    else flow_jacobi_k<false><<<gr, kT, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_flow_jacobi_wg(const FlowPlan& p, float* base, int l, float* u, float* v, hipStream_t s)
{
    if (!level_ok(p, base, l) || !u || !v || u == v) return hipErrorInvalidValue;
    const FlowLevel& L = p.lv[l];
    if (!L.one_wg || L.n > (size_t)kFlowWgMaxPixels || p.par.iters < 1) return hipErrorInvalidValue;       // the LDS planes hold no more
    flow_jacobi_wg_k<<<1, kFlowWgThreads, 0, s>>>(u, v, base + p.ix, base + p.iy, base + p.c, base + p.den, L.h, L.w, p.par.iters);
    return hipGetLastError();
}

hipError_t launch_flow_interleave(const float* u, const float* v, float* out_hw2, size_t n, int grid, hipStream_t s)
{
    if (!u || !v || !out_hw2 || n < 1 || !grid_ok(grid) || ((uintptr_t)out_hw2 & 7) != 0) return hipErrorInvalidValue;
    flow_interleave_k<<<grid, kT, 0, s>>>(u, v, reinterpret_cast<float2*>(out_hw2), n);
    return hipGetLastError();
}

}  // namespace st2
