// Style statistics of the fp32 feature path on the bf16 matrix cores with three-way split operands (gfx950), opt-in:
// st_set_gram_algo(ctx, 1).
//
//   gram_split_*       : G_s = F[:, slab_s] F[:, slab_s]^T     worker.py:109-114 (np.dot(x, x.T)); gram_reduce* finishes it (gram.hip)
//   style_grad_split_* : S = c2 * (D @ F)                      worker.py:258-269
//
// The arithmetic is that of conv3x3_wino_split.hip: every fp32 operand is written a = a1 + a2 + a3 exactly, each term a bf16 (a1 rounded
// to nearest, a2 and a3 by truncation; a3 is exact: 24 - 16 bits are left), and a product is taken as its six partial products of weight
// <= 2,   a b = a1 b1 + (a1 b2 + a2 b1) + (a1 b3 + a3 b1 + a2 b2)   [+ three terms below 2^-24 |a b|],
// each exact in fp32, accumulated in fp32 by v_mfma_f32_32x32x16_bf16, smallest weight first: 12 matrix-pipe cycles per k instead of the
// 32 of v_mfma_f32_32x32x2_f32.  A non-finite operand splits into Inf + NaN (Inf - Inf), so a result that the fp32 kernels give as Inf
// may come out NaN here.
//
// Both kernels stage fp32 rows of F by LDS-DMA, split the staged slab ONCE into three bf16 images in LDS (the four waves share them;
// the Gram's two operands are the same rows, its diagonal tiles split one operand only) and feed all six products from the images.
// The split runs between two barriers, not under the wave's own MFMAs: two workgroups share a CU (80 / 40 KiB of LDS) and one's
// split overlaps the other's matrix work.  The subtractions go through inline asm so that the compiler cannot pair them into packed
// fp32 instructions, which run on the matrix pipe's lanes.
//
// Gram: the layout of gram_partial_dma_* -- BT x BT tiles of the upper triangle x split-K slabs, 32 pixels per step, the raw image with
// the same quad swizzle.  The bf16 images are [term][k group of 8][row] quads: a quad is one lane's MFMA fragment (row, 8 consecutive k)
// and consecutive lanes read consecutive quads.  The pixel contraction needs no transposed read here: F is [C][hw], a row's pixels are
// contiguous (gram16.hip's ds_read_b64_tr_b16 undoes the channel blocking of the bf16 copy, which this path does not have).
// The six products of (r, c) and (c, r) are added in different orders, so a diagonal tile stores only its upper triangle and mirrors
// it (same value to both places: exactly symmetric); the wave below the diagonal issues no MFMA.
//
// Style gradient: workgroup = BM (128, or 64 where C % 128 != 0) channels x 128 pixels, 32 channels of K per chunk.  A wave owns 32 rows of D: its A
// fragments come straight from the three-term pack of D (split once per launch, L2-resident) into registers, a chunk ahead.  The
// contraction runs over CHANNELS, the memory over pixels: the split reads the raw chunk transposed (8 channel rows at one pixel, lanes
// along pixels: conflict-free) and writes [term][k group][pixel] quads = the B fragments.  Epilogue as style_grad16_*: c2 in fp32,
// optional sw / norm and accumulate, rows staged through LDS for 16-byte stores, per-block sum of S^2.
//
// Taken for C % 64 == 0, C >= 128 and tensors below 4 GiB (gram_split_ok); hw % 4 != 0 (or an unaligned blob) runs the same kernels with register staging and
// dword stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "st2_kernels.h"
#include "wave_reduce.h"

namespace st2 {

namespace {

typedef float gs_f32x16 __attribute__((ext_vector_type(16)));
typedef float gs_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 gs_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 gs_bf16x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void* gs_lptr_t;
constexpr unsigned kGsOOB = 0xffffffffu;

__device__ __forceinline__ gs_bf16x8 gs_bf(const uint4& u) { return __builtin_bit_cast(gs_bf16x8, u); }
__device__ __forceinline__ float gs_f(unsigned u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ float gs_sub(float a, float b)
{
    float r;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// {x0, x1} -> one dword per term, x0 in the low half: t1 nearest, t2 / t3 truncated (ws_cvt2 / ws_hi2 / ws_hi of conv3x3_wino_split.hip)
__device__ __forceinline__ void gs_split2(float x0, float x1, unsigned& t1, unsigned& t2, unsigned& t3)
{
    gs_f32x2 v; v.x = x0; v.y = x1;
    t1 = __builtin_bit_cast(unsigned, __builtin_convertvector(v, gs_bf16x2));
    const float r0 = gs_sub(x0, gs_f(t1 << 16)), r1 = gs_sub(x1, gs_f(t1 & 0xffff0000u));
    t2 = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, r1), __builtin_bit_cast(unsigned, r0), 0x07060302u);
    const float s0 = gs_sub(r0, gs_f(__builtin_bit_cast(unsigned, r0) & 0xffff0000u));
    const float s1 = gs_sub(r1, gs_f(__builtin_bit_cast(unsigned, r1) & 0xffff0000u));
    t3 = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, s1), __builtin_bit_cast(unsigned, s0), 0x07060302u);
}
__device__ __forceinline__ void gs_split8(const float (&x)[8], uint4& t1, uint4& t2, uint4& t3)
{
    gs_split2(x[0], x[1], t1.x, t2.x, t3.x);
    gs_split2(x[2], x[3], t1.y, t2.y, t3.y);
    gs_split2(x[4], x[5], t1.z, t2.z, t3.z);
    gs_split2(x[6], x[7], t1.w, t2.w, t3.w);
}
#define GS_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(gs_bf(a), gs_bf(b), c, 0, 0, 0)

// ------------------------------------------------------------------------------------------------ Gram partials
template <int BT>                    // 128 is the only instance: gram_plan gives 128-row tiles for every C > 64
__device__ __forceinline__ void gram_split_body(const float* __restrict__ F, unsigned f_bytes, float* __restrict__ slabs,
                                                int C, int hw, int tiles_1d, int kslab, int aligned)
{
    constexpr int T = BT / 64;                       // 32x32 MFMA tiles per wave per dimension
    constexpr int IMG = BT * 32;                     // floats per raw operand image (BT rows x 32 K)
    constexpr int PPW = IMG / 256 / 4;               // 1-KiB pieces per wave and operand
    constexpr int BQ = 4 * BT;                       // quads per bf16 term image: [k group 4][row BT]
    __shared__ __attribute__((aligned(16))) float raw[2][IMG];           // [A/B]
    __shared__ __attribute__((aligned(16))) uint4 img[2][3][BQ];         // [A/B][term]

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, khalf = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int n_ut = tiles_1d * (tiles_1d + 1) / 2;
    int tile = blockIdx.x % n_ut;
    const int split = blockIdx.x / n_ut;
    int ti = 0;
    while (tile >= tiles_1d - ti) { tile -= tiles_1d - ti; ++ti; }
    const int tj = ti + tile;
    const int i0 = ti * BT, j0 = tj * BT;
    const bool diag = ti == tj;
    const int kbeg = split * kslab;
    const int kend = min(hw, kbeg + kslab);
    const int nsteps = (kend - kbeg + 31) / 32;      // a ragged last step is zero-filled

    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)F, 0, f_bytes, 0x00020000);
    auto stage = [&](int step) {
#pragma unroll
        for (int t = 0; t < PPW; ++t) {
            const int slot = (wave + 4 * t) * 64 + lane;          // LDS quad slot: row = slot / 8, swizzled quad = slot % 8
            const int r = slot >> 3, q = (slot & 7) ^ ((r >> 1) & 7);
            const int k = kbeg + step * 32 + 4 * q;
#pragma unroll
            for (int op = 0; op < 2; ++op) {
                if (op && diag) break;
                const int row = (op ? j0 : i0) + r;
                if (aligned) {                                    // hw % 4 == 0: a quad is inside its row or outside
                    const unsigned off = (row < C && k < kend) ? ((unsigned)row * (unsigned)hw + (unsigned)k) * 4u : kGsOOB;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (gs_lptr_t)(raw[op] + (wave + 4 * t) * 256), 16, off, 0, 0, 0);
                } else {
                    float4 v;
                    const float* src = F + (size_t)(row < C ? row : 0) * hw;
                    v.x = (row < C && k + 0 < kend) ? src[k + 0] : 0.f;
                    v.y = (row < C && k + 1 < kend) ? src[k + 1] : 0.f;
                    v.z = (row < C && k + 2 < kend) ? src[k + 2] : 0.f;
                    v.w = (row < C && k + 3 < kend) ? src[k + 3] : 0.f;
                    *reinterpret_cast<float4*>(raw[op] + slot * 4) = v;
                }
            }
        }
    };
    auto split_images = [&]() {
#pragma unroll
        for (int op = 0; op < 2; ++op) {
            if (op && diag) break;
#pragma unroll
            for (int it = 0; it < BQ / 256; ++it) {
                const int idx = it * 256 + tid, row = idx % BT, kg = idx / BT, sw = (row >> 1) & 7;
                const float4 v0 = *reinterpret_cast<const float4*>(raw[op] + (row * 8 + ((2 * kg) ^ sw)) * 4);
                const float4 v1 = *reinterpret_cast<const float4*>(raw[op] + (row * 8 + ((2 * kg + 1) ^ sw)) * 4);
                const float x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                uint4 t1, t2, t3;
                gs_split8(x, t1, t2, t3);
                img[op][0][idx] = t1; img[op][1][idx] = t2; img[op][2][idx] = t3;
            }
        }
    };

    gs_f32x16 acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const bool work = !(diag && wm > wn);            // a diagonal tile's lower-left wave produces nothing that is stored
    const int bop = diag ? 0 : 1;

    if (nsteps > 0) stage(0);
    for (int st = 0; st < nsteps; ++st) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                              // step st has landed; every wave is done with the images of step st - 1
        split_images();
        __syncthreads();                              // the images are complete, the raw buffer is free
        if (st + 1 < nsteps) stage(st + 1);
        if (work) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int kg = 2 * ks + khalf;
                uint4 a[3][T], b[3][T];
#pragma unroll
                for (int s = 0; s < 3; ++s) {
#pragma unroll
                    for (int i = 0; i < T; ++i) a[s][i] = img[0][s][kg * BT + wm * (T * 32) + i * 32 + l31];
#pragma unroll
                    for (int j = 0; j < T; ++j) b[s][j] = img[bop][s][kg * BT + wn * (T * 32) + j * 32 + l31];
                }
                // smallest weight first; the T * T accumulators are independent, a dependent MFMA is T * T instructions away
#define GS_ROUND(sa, sb)                                                        \
    _Pragma("unroll") for (int i = 0; i < T; ++i)                               \
        _Pragma("unroll") for (int j = 0; j < T; ++j) acc[i][j] = GS_MFMA(a[sa][i], b[sb][j], acc[i][j]);
                GS_ROUND(2, 0) GS_ROUND(0, 2) GS_ROUND(1, 1) GS_ROUND(1, 0) GS_ROUND(0, 1) GS_ROUND(0, 0)
#undef GS_ROUND
            }
        }
    }

    float* dst = slabs + (size_t)split * C * C;
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const int col = j0 + wn * (T * 32) + j * 32 + l31;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = i0 + wm * (T * 32) + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * khalf;
                if (row < C && col < C && (!diag || row <= col)) {
                    dst[(size_t)row * C + col] = acc[i][j][e];
                    if (diag && row < col) dst[(size_t)col * C + row] = acc[i][j][e];
                }
            }
        }
}

// ------------------------------------------------------------------------------------------------ style gradient
struct StyleSplitArgs {
    const uint4* A; const float* F; float* out; const float* norm; float* partial;
    float c2, sw; int fused, accumulate, aligned;
    int C, n_mtiles; unsigned hw, f_bytes;
};

constexpr int GS_PX = 128;           // pixels per workgroup
constexpr int GS_KC = 32;            // channels per chunk (2 MFMA k-steps)
constexpr int GS_SLD = 68;           // leading dimension of a wave's output stage [32 rows][64 px]: the two k halves (4 rows apart) on different banks

// the three-term pack of D: quad[((kc * 3 + term) * 4 + kg) * C + m] = 8 bf16 of row m, channels 32 kc + 8 kg .. + 7
__global__ __launch_bounds__(256) void style_split_pack_d_k(const float* __restrict__ D, int ld, int C, uint4* __restrict__ A)
{
    const int nq = (C / GS_KC) * 12 * C;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < nq; q += gridDim.x * 256) {
        const int m = q % C, r = q / C;
        const int kg = r & 3, term = (r >> 2) % 3, kc = r / 12;
        const float* src = D + (size_t)m * ld + GS_KC * kc + 8 * kg;
        unsigned t[3][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) gs_split2(src[2 * j], src[2 * j + 1], t[0][j], t[1][j], t[2][j]);
        uint4 v;
        v.x = term == 0 ? t[0][0] : term == 1 ? t[1][0] : t[2][0];
        v.y = term == 0 ? t[0][1] : term == 1 ? t[1][1] : t[2][1];
        v.z = term == 0 ? t[0][2] : term == 1 ? t[1][2] : t[2][2];
        v.w = term == 0 ? t[0][3] : term == 1 ? t[1][3] : t[2][3];
        A[q] = v;
    }
}

template <int WR>                    // waves along the rows: BM = 32 WR channels; the other 4 / WR split the 128 pixels
__device__ __forceinline__ void style_split_body(const StyleSplitArgs& a)
{
    constexpr int BM = 32 * WR, WP = 4 / WR, NF = 4 / WP;            // NF: 32-pixel fragments per wave (4 | 2)
    constexpr int RAW_BYTES = GS_KC * GS_PX * 4, IMG_Q = 4 * GS_PX;  // raw chunk [32 ch][128 px]; quads per term image [kg 4][px 128]
    __shared__ __attribute__((aligned(16))) unsigned char smem[RAW_BYTES + 3 * IMG_Q * 16];      // 40 KiB
    static_assert(sizeof(smem) >= 4 * 32 * GS_SLD * 4, "the output stage fits");
    __shared__ float red[4];
    float* const raw = reinterpret_cast<float*>(smem);
    uint4* const bimg = reinterpret_cast<uint4*>(smem + RAW_BYTES);

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, khalf = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave % WR, wp = wave / WR;
    const int mt = blockIdx.x % a.n_mtiles, pt = blockIdx.x / a.n_mtiles;        // the M tiles of one pixel tile run together (L2 reuse of F)
    const int m0 = mt * BM + 32 * wr;                                            // this wave's first row
    const unsigned p0 = (unsigned)pt * GS_PX;
    const int nch = a.C / GS_KC;

    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.F, 0, a.f_bytes, 0x00020000);
    auto stage = [&](int ch) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int slot = (wave + 4 * t) * 64 + lane;          // [channel 32][pixel quad 32]
            const unsigned chn = (unsigned)(GS_KC * ch + (slot >> 5)), p = p0 + 4u * (slot & 31);
            if (a.aligned) {
                const unsigned off = p < a.hw ? (chn * a.hw + p) * 4u : kGsOOB;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (gs_lptr_t)(raw + (wave + 4 * t) * 256), 16, off, 0, 0, 0);
            } else {
                const float* src = a.F + (size_t)chn * a.hw;
                float4 v;
                v.x = p + 0 < a.hw ? src[p + 0] : 0.f;
                v.y = p + 1 < a.hw ? src[p + 1] : 0.f;
                v.z = p + 2 < a.hw ? src[p + 2] : 0.f;
                v.w = p + 3 < a.hw ? src[p + 3] : 0.f;
                *reinterpret_cast<float4*>(raw + slot * 4) = v;
            }
        }
    };
    auto load_a = [&](int ch, uint4 (&d)[3][2]) {
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                d[s][ks] = a.A[(size_t)((ch * 3 + s) * 4 + 2 * ks + khalf) * a.C + m0 + l31];
    };

    gs_f32x16 acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[f][e] = 0.f;

    uint4 an[3][2], ac[3][2];
    stage(0);
    load_a(0, an);
    for (int ch = 0; ch < nch; ++ch) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                              // chunk ch has landed; every wave is done with the images of chunk ch - 1
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int idx = it * 256 + tid, px = idx & 127, kg = idx >> 7;
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = raw[(8 * kg + j) * GS_PX + px];
            uint4 t1, t2, t3;
            gs_split8(x, t1, t2, t3);
            bimg[idx] = t1; bimg[IMG_Q + idx] = t2; bimg[2 * IMG_Q + idx] = t3;
        }
#pragma unroll
        for (int s = 0; s < 3; ++s) { ac[s][0] = an[s][0]; ac[s][1] = an[s][1]; }
        __syncthreads();                              // the images are complete, the raw buffer is free
        if (ch + 1 < nch) { stage(ch + 1); load_a(ch + 1, an); }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            uint4 b[3][NF];
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int f = 0; f < NF; ++f) b[s][f] = bimg[s * IMG_Q + (2 * ks + khalf) * GS_PX + (wp * NF + f) * 32 + l31];
#define GS_ROUND(sa, sb) _Pragma("unroll") for (int f = 0; f < NF; ++f) acc[f] = GS_MFMA(ac[sa][ks], b[sb][f], acc[f]);
            GS_ROUND(2, 0) GS_ROUND(0, 2) GS_ROUND(1, 1) GS_ROUND(1, 0) GS_ROUND(0, 1) GS_ROUND(0, 0)
#undef GS_ROUND
        }
    }

    // ---- epilogue (C/D map: column = lane & 31 = pixel, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5))
    const float coef = a.fused ? a.sw / *a.norm : 0.0f;
    const unsigned pw = p0 + (unsigned)(wp * NF) * 32u;               // this wave's first pixel
    float ss = 0.0f;
    if (a.aligned) {
        float* const stg = reinterpret_cast<float*>(smem) + wave * (32 * GS_SLD);       // [32 rows][64 px], this wave's own
#pragma unroll
        for (int rnd = 0; rnd < NF / 2; ++rnd) {
            __syncthreads();                          // the operand images / the previous round are consumed
#pragma unroll
            for (int ff = 0; ff < 2; ++ff)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int row = (e & 3) + 8 * (e >> 2) + 4 * khalf;
                    const float v = pw + (2 * rnd + ff) * 32 + l31 < a.hw ? acc[2 * rnd + ff][e] * a.c2 : 0.0f;
                    ss += v * v;
                    stg[row * GS_SLD + ff * 32 + l31] = a.fused ? coef * v : v;
                }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int idx = t * 64 + lane, row = idx >> 4, c4 = (idx & 15) * 4;
                const unsigned p = pw + rnd * 64 + c4;
                if (p < a.hw) {
                    float4 v = *reinterpret_cast<const float4*>(stg + row * GS_SLD + c4);
                    float* dst = a.out + (size_t)(m0 + row) * a.hw + p;
                    if (a.fused && a.accumulate) { const float4 o = *reinterpret_cast<const float4*>(dst); v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
                    *reinterpret_cast<float4*>(dst) = v;
                }
            }
        }
    } else {
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const unsigned p = pw + f * 32 + l31;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = m0 + (e & 3) + 8 * (e >> 2) + 4 * khalf;
                if (p < a.hw) {
                    const float v = acc[f][e] * a.c2;
                    ss += v * v;
                    float* dst = a.out + (size_t)row * a.hw + p;
                    *dst = a.fused ? coef * v + (a.accumulate ? *dst : 0.0f) : v;
                }
            }
        }
    }
    float sv[1] = {ss};
    block_sum(sv, red);
    if (tid == 0) a.partial[blockIdx.x] = sv[0];
}

}  // namespace

// non-template entry points (a template kernel with a waves-per-SIMD launch bound loses its host stub)
__global__ __launch_bounds__(256, 2) void gram_split_128(const float* F, unsigned f_bytes, float* slabs, int C, int hw, int tiles_1d, int kslab, int aligned)
{ gram_split_body<128>(F, f_bytes, slabs, C, hw, tiles_1d, kslab, aligned); }
__global__ __launch_bounds__(256, 2) void style_grad_split_128(const StyleSplitArgs a) { style_split_body<4>(a); }
__global__ __launch_bounds__(256, 2) void style_grad_split_64(const StyleSplitArgs a) { style_split_body<2>(a); }

// Whole blobs, C a multiple of 64 from 128 up, below 4 GiB (32-bit buffer offsets); hw is free.  C = 64 (conv1_1) is refused on a
// measurement: both GEMMs are HBM-bound there (268 / 537 MB at 1024^2) and the split kernels were 2 % slower on that layer
// (0.214 -> 0.219 ms, tools/bench_gram_algo.py --style-layers conv1_1), so it keeps the fp32 kernels.
bool gram_split_ok(int C, int hw)
{
    return C >= 128 && C % 64 == 0 && hw > 0 && 4ull * C * hw < 0xfffffff0ull;
}
bool style_grad_split_ok(int C, int hw)
{
    return gram_split_ok(C, hw);
}

// same contract, plan (gram_plan) and slab format as launch_gram_partial for a whole blob
hipError_t launch_gram_split_partial(const float* F, float* slabs, int C, int hw, const GramPlan& pl, hipStream_t s)
{
    if (!gram_split_ok(C, hw) || pl.kslab % 32 != 0) return hipErrorInvalidValue;
    const int t1 = (C + pl.bt - 1) / pl.bt;
    const unsigned grid = (unsigned)(pl.tiles * pl.splits);
    const unsigned fb = (unsigned)(4ull * C * hw);
    const int aligned = hw % 4 == 0 && (reinterpret_cast<uintptr_t>(F) & 15) == 0;
    if (pl.bt != 128) return hipErrorInvalidValue;          // gram_plan: 128-row tiles for every C > 64
    gram_split_128<<<grid, 256, 0, s>>>(F, fb, slabs, C, hw, t1, pl.kslab, aligned);
    return hipGetLastError();
}

static int style_split_bm(int C) { return C % 128 == 0 ? 128 : 64; }
size_t style_grad_split_pack_elems(int C) { return (size_t)3 * C * C; }
int style_grad_split_blocks(int C, int hw) { return ((hw + GS_PX - 1) / GS_PX) * (C / style_split_bm(C)); }

// same contract as launch_style_grad for a whole blob; Dp has leading dimension ld, A16 is scratch of style_grad_split_pack_elems(C) bf16
hipError_t launch_style_grad_split(const float* Dp, int ld, unsigned short* A16, const float* F, float* dst, float c2, int fused, float sw,
                                   const float* norm, int accumulate, float* partial, int* n_partial, int C, int hw, hipStream_t s)
{
    if (!style_grad_split_ok(C, hw) || ld < C || (reinterpret_cast<uintptr_t>(A16) & 15) != 0) return hipErrorInvalidValue;
    const int nq = (C / GS_KC) * 12 * C;
    style_split_pack_d_k<<<(nq + 255) / 256, 256, 0, s>>>(Dp, ld, C, reinterpret_cast<uint4*>(A16));
    StyleSplitArgs a{};
    a.A = reinterpret_cast<const uint4*>(A16); a.F = F; a.out = dst; a.norm = norm; a.partial = partial;
    a.c2 = c2; a.sw = sw; a.fused = fused; a.accumulate = accumulate;
    a.aligned = hw % 4 == 0 && (reinterpret_cast<uintptr_t>(F) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    a.C = C; a.n_mtiles = C / style_split_bm(C); a.hw = (unsigned)hw; a.f_bytes = (unsigned)(4ull * C * hw);
    const int grid = style_grad_split_blocks(C, hw);
    if (n_partial) *n_partial = grid;
    if (style_split_bm(C) == 128) style_grad_split_128<<<grid, 256, 0, s>>>(a);
    else style_grad_split_64<<<grid, 256, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace st2
