// The device-resident style-transfer engine behind include/st2.h: context, model (forward / ranged backward), image slots.
//
// One st_ctx == one reference worker's model + StyleTransfer + optimizer (worker.py:32-315,
// optimizers.py:7-125) with all tensors living in HBM.  The host only sequences launches on one
// HIP stream; nothing crosses PCIe inside an iteration unless the caller asks for the iterate.
// The objective lives in engine_objective.cpp, the optimizers and the iteration in engine_step.cpp, resampling in
// engine_resample.cpp, the tile-sharded phases in engine_tile.cpp.
#include "engine.h"

#include <atomic>

namespace st2e {
static thread_local char g_err[1024] = "";
int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
const char* const kProfNames[P_COUNT] = {"conv3x3_fwd_mfma_f32", "conv3x3_dgrad_mfma_f32", "maxpool_fwd", "maxpool_bwd",
                                          "gram_partial_mfma_f32", "gram_reduce", "style_grad_mfma_f32", "layer_elem",
                                          "image_pass", "finalize", "vector_ops", "misc", "conv3x3_fwd_wino_f32", "conv3x3_dgrad_wino_f32",
                                          "conv3x3_fwd_mfma_bf16", "conv3x3_dgrad_mfma_bf16", "tile_comm",
                                          "gram_partial_mfma_bf16", "style_grad_mfma_bf16", "conv3x3_fwd_wino_split_bf16x6", "conv3x3_dgrad_wino_split_bf16x6",
                                          "style_grad_fused_in_conv_dgrad_bf16", "avepool_fwd", "avepool_bwd",
                                          "gram_partial_split_bf16x6", "style_grad_split_bf16x6", "avepool_bwd_map16", "laplacian_pool", "laplacian_stencil", "laplacian_grad", "anchor",
                                          "frames", "flow_prepare", "flow_linearise", "flow_jacobi", "flow_jacobi_one_workgroup",
                                          "matting_fit", "matting_apply", "matting_windows"};

static const struct { int kind; const char* name; int cin, cout; } kVgg19[] = {
    {0, "conv1_1", 3, 64}, {0, "conv1_2", 64, 64}, {1, "pool1", 0, 0},
    {0, "conv2_1", 64, 128}, {0, "conv2_2", 128, 128}, {1, "pool2", 0, 0},
    {0, "conv3_1", 128, 256}, {0, "conv3_2", 256, 256}, {0, "conv3_3", 256, 256}, {0, "conv3_4", 256, 256}, {1, "pool3", 0, 0},
    {0, "conv4_1", 256, 512}, {0, "conv4_2", 512, 512}, {0, "conv4_3", 512, 512}, {0, "conv4_4", 512, 512}, {1, "pool4", 0, 0},
    {0, "conv5_1", 512, 512}, {0, "conv5_2", 512, 512}, {0, "conv5_3", 512, 512}, {0, "conv5_4", 512, 512}, {1, "pool5", 0, 0},
};

// ---------------------------------------------------------------------------------------- helpers
// The funnel of devbuf.h: the only place that allocates or frees device / pinned memory, and the two process-wide counters of what
// is live (requested bytes) behind st_live_bytes.
static std::atomic<long long> g_live_dev{0}, g_live_pin{0};
int raw_alloc(void** p, size_t bytes)
{
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(ST_ERR_HIP, "hipMalloc of %zu bytes: %s", bytes, hipGetErrorString(e));
    g_live_dev += (long long)bytes;
    *p = q;
    return ST_OK;
}
void raw_free(void* p, size_t bytes)
{
    if (hipFree(p) != hipSuccess) (void)hipGetLastError();   // never leave a sticky error behind
    g_live_dev -= (long long)bytes;
}
int raw_pin_alloc(void** p, size_t bytes)
{
    void* q = nullptr;
    hipError_t e = hipHostMalloc(&q, bytes, 0);
    if (e != hipSuccess) return fail(ST_ERR_HIP, "hipHostMalloc of %zu bytes: %s", bytes, hipGetErrorString(e));
    g_live_pin += (long long)bytes;
    *p = q;
    return ST_OK;
}
void raw_pin_free(void* p, size_t bytes)
{
    if (hipHostFree(p) != hipSuccess) (void)hipGetLastError();
    g_live_pin -= (long long)bytes;
}

// room for the split-K partial sums of a Winograd launch that would otherwise leave most CUs idle
int wino_scratch(st_ctx* c, ConvProblem& p, int splits)
{
    if (splits <= 1) return ST_OK;
    const size_t need = (size_t)splits * p.M * p.H * p.W;
    if (need > c->conv_scratch.cap()) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        ST_TRY(c->conv_scratch.reserve(need));
    }
    p.scratch = c->conv_scratch; p.scratch_floats = c->conv_scratch.cap();
    return ST_OK;
}

void shapes_for(const st_ctx* c, int H, int W, std::vector<int>& C, std::vector<int>& h, std::vector<int>& w)
{
    C.assign(c->nb, 0); h.assign(c->nb, 0); w.assign(c->nb, 0);
    C[0] = 3; h[0] = H; w[0] = W;
    for (int i = 1; i < c->nb; ++i) {
        const Layer& L = c->topo[i - 1];
        if (L.is_conv) { C[i] = L.cout; h[i] = h[i - 1]; w[i] = w[i - 1]; }
        else { C[i] = C[i - 1]; h[i] = pooled_size(h[i - 1]); w[i] = pooled_size(w[i - 1]); }
    }
}

int act_ensure(st_ctx* c, ActSet& a, int H, int W)
{
    if (a.H == H && a.W == W && !a.data.empty()) return ST_OK;
    a = ActSet{};
    shapes_for(c, H, W, a.C, a.h, a.w);
    a.own.resize(c->nb);
    a.data.assign(c->nb, nullptr);
    a.data16.resize(c->nb);
    a.amap.resize(c->nb);
    a.bits.resize(c->nb);
    a.plan.fwd.assign(c->nb, FwdRoute{});
    a.plan.bwd.assign(c->nb, BwdRoute{});
    for (int i = 1; i < c->nb; ++i) { ST_TRY(a.own[i].alloc((size_t)a.C[i] * a.h[i] * a.w[i])); a.data[i] = a.own[i]; }
    a.H = H; a.W = W;
    return ST_OK;
}

// the buffers of blob b beyond the fp32 one are made when a plan first names them; bf16 copy and map have one size (the map also for
// both of its layouts: the buffer is shared when the precision is switched)
static size_t elems16(const ActSet& a, int b) { return act16_elems(a.C[b], (size_t)a.h[b] * a.w[b]); }
static int pack16(st_ctx* c, const float* src, unsigned short* dst, int C, size_t hw)
{
    ProfScope ps(c, P_MISC, 0, hw * 6.0 * C);
    HIP_TRY(launch_pack_act16(src, dst, C, hw, c->stream));
    return ST_OK;
}

// Executes plan_forward's routes for layers 1 .. last (engine_route.cpp says what `lean` skips).  The profiler's figures: flops are
// the ALGORITHMIC (direct-convolution) count in every conv class -- Winograd executes 4/9 of them, the split kernel 6 x 4/9 on the
// bf16 pipe --, bytes what the launch reads and writes.
int forward_range(st_ctx* c, ActSet& a, const float* x, int last, bool lean)
{
    a.data[0] = const_cast<float*>(x);
    plan_forward(c, a, last, lean, a.plan.fwd);
    const std::vector<FwdRoute>& plan = a.plan.fwd;
    for (int i = 1; i <= last; ++i) {
        const Layer& L = c->topo[i - 1];
        const FwdRoute& r = plan[i];
        const FwdRoute& pool = plan[std::min(i + 1, c->nb - 1)];      // what the launch writes of the pooled blob (r.pools_next)
        const int C = a.C[i], H = a.h[i], W = a.w[i];
        const size_t hw = (size_t)H * W;
        const double px = (double)hw, n_in = (double)a.C[i - 1] * a.h[i - 1] * a.w[i - 1];
        if (L.is_conv && !L.loaded) return fail(ST_ERR_STATE, "weights of %s were never loaded", L.name.c_str());
        if (r.out16) ST_TRY(a.data16[i].reserve(elems16(a, i)));
        if (r.bits) ST_TRY(a.bits[i].reserve(conv16_bits_elems(C, hw)));
        if (r.pools_next && pool.out16) ST_TRY(a.data16[i + 1].reserve(elems16(a, i + 1)));
        if (r.pools_next && pool.amap != AMAP_NONE) ST_TRY(a.amap[i + 1].reserve(elems16(a, i + 1)));
        const double conv_flops = 2.0 * 9 * L.cin * L.cout * px;
        switch (r.kind) {
        case F_CONV16: {
            Conv16Problem p{};
            p.in16 = a.data16[i - 1]; p.wpack16 = L.w16_fwd; p.bias = L.bias;
            p.out = r.out32 ? a.data[i] : nullptr;
            p.out16 = r.out16 ? a.data16[i] : nullptr;
            p.bits_out = r.bits ? a.bits[i] : nullptr;
            p.K = L.cin; p.M = L.cout; p.MPad = conv_mpad(L.cout); p.H = H; p.W = W; p.relu = 1;
            double bytes = px * (2.0 * L.cin + (r.out32 ? 4.0 : 0.0) * L.cout + (r.out16 ? 2.0 : 0.0) * L.cout + (r.bits ? 0.125 : 0.0) * L.cout);
            if (r.pools_next) {         // pooled bf16 copy for the conv after it, arg-max map (average pool: sign map) for the backward
                p.pool_ave = pool.amap == AMAP_BLOCKED16_AVE;
                p.pool16 = pool.out16 ? a.data16[i + 1] : nullptr;
                p.pool32 = pool.out32 ? a.data[i + 1] : nullptr;
                p.amap = a.amap[i + 1];
                bytes += px * 0.25 * L.cout * (1.0 + (pool.out16 ? 2.0 : 0.0) + (pool.out32 ? 4.0 : 0.0));
            }
            ProfScope ps(c, P_CONV_FWD_BF16, conv_flops, bytes);
            HIP_TRY(launch_conv3x3_bf16(p, c->stream));
            break;
        }
        case F_WINO: case F_WINO_SPLIT: case F_DIRECT: case F_FIRST_SPLIT: {
            ConvProblem p{};
            p.in = a.data[i - 1]; p.wpack = L.w_fwd; p.bias = L.bias;
            p.out = r.out32 ? a.data[i] : nullptr;
            p.K = L.cin; p.M = L.cout; p.MPad = conv_mpad(L.cout); p.H = H; p.W = W; p.relu = 1;
            if (r.pools_next) { p.pool_out = a.data[i + 1]; p.pool_amap = pool.amap != AMAP_NONE ? a.amap[i + 1] : nullptr; }
            if (r.out16 && !r.pack16) p.out16 = a.data16[i];           // the epilogue writes the bf16 copy too
            {
                ProfScope ps(c, r.kind == F_WINO_SPLIT ? P_CONV_FWD_WSPLIT : r.kind == F_WINO ? P_CONV_FWD_WINO : P_CONV_FWD, conv_flops,
                             4.0 * px * (L.cin + L.cout));
                if (r.kind == F_WINO_SPLIT) {
                    p.wpack = reinterpret_cast<const float*>(L.us_fwd.get()); ST_TRY(wino_scratch(c, p, wino_split_resolve(p.K, p.M, H, W).splits));
                    HIP_TRY(launch_conv3x3_wino_split(p, c->stream));
                } else if (r.kind == F_WINO) {
                    p.wpack = L.u_fwd; ST_TRY(wino_scratch(c, p, wino_resolve(p.K, p.M, H, W).splits));
                    HIP_TRY(launch_conv3x3_wino(p, c->stream));
                } else if (r.kind == F_FIRST_SPLIT) {
                    HIP_TRY(launch_conv3x3_first_split(p.in, L.w_split, p.out, p.out16, p.K, p.M, H, W, p.relu, c->stream, r.bits ? a.bits[i] : nullptr));
                } else {
                    HIP_TRY(launch_conv3x3(p, c->stream));
                }
            }
            if (r.pack16) ST_TRY(pack16(c, a.data[i], a.data16[i], C, hw));
            break;
        }
        case F_BY_CONV_BELOW:
            break;
        case F_AVEPOOL: {
            if (!plan[i - 1].out32) return fail(ST_ERR_STATE, "internal: the input blob of average pool %s is not materialised", L.name.c_str());
            ProfScope ps(c, P_AVEPOOL_FWD, 0, 4.0 * n_in + (r.out32 ? 4.0 * C * hw : 0.0) + (r.out16 ? 2.0 * act16_elems(C, hw) : 0.0));
            HIP_TRY(launch_avepool_fwd(a.data[i - 1], r.out32 ? a.data[i] : nullptr, r.out16 ? a.data16[i] : nullptr, C, a.h[i - 1], a.w[i - 1], c->stream));
            break;
        }
        case F_MAXPOOL: {
            { ProfScope ps(c, P_POOL_FWD, 0, 4.0 * n_in * 1.25);
              HIP_TRY(launch_maxpool_fwd(a.data[i - 1], a.data[i], C, a.h[i - 1], a.w[i - 1], c->stream)); }
            if (r.pack16) ST_TRY(pack16(c, a.data[i], a.data16[i], C, hw));
            break;
        }
        case F_NONE:
            return fail(ST_ERR_STATE, "internal: no route for layer %s", L.name.c_str());
        }
    }
    a.valid_to = last;
    return ST_OK;
}

// backward chain from blob `top` whose diff is `top_diff` down to data; returns pointer in *out.  Executes plan_backward's routes;
// `lean` must be what the forward that filled c->act ran with.
int backward_chain(st_ctx* c, int top, const float* top_diff, const std::vector<const float*>& inj, const float** out, bool lean)
{
    ActSet& a = c->act;
    plan_backward(c, a, top, inj, c->sf_w, lean, a.plan.bwd);
    const std::vector<FwdRoute>& fwd = a.plan.fwd;
    const float* cur = top_diff;
    const unsigned short* cur16 = nullptr;             // bf16 copy of the running diff, when a producer already made it
    if (c->bf16 && !c->diff16A) {
        const size_t cap = c->max_blob + 8 * (size_t)a.h[0] * a.w[0];
        ST_TRY(c->diff16A.alloc(cap)); ST_TRY(c->diff16B.alloc(cap));
    }
    for (int i = top; i >= 1; --i) {
        const Layer& L = c->topo[i - 1];
        const BwdRoute& r = a.plan.bwd[i];
        const int below = i - 1;
        const int Cb = a.C[below], Hb = a.h[below], Wb = a.w[below];          // the blob the diff is propagated to
        const int H = a.h[i], W = a.w[i];
        const size_t hw = (size_t)H * W;
        const double px = (double)hw, n_below = (double)Cb * Hb * Wb;
        float* dst = (cur == c->diffA) ? c->diffB : c->diffA;
        const float* inject = inj[below];
        if (r.in16 ? !(cur16 || cur) : !cur) return fail(ST_ERR_STATE, "internal: no %s diff above %s", r.in16 ? "bf16 or fp32" : "fp32", L.name.c_str());
        if (r.pack_in16) {                                 // top diff / fp32 producer: make the bf16 copy of the running diff
            unsigned short* tmp16 = (cur16 == c->diff16A) ? c->diff16B : c->diff16A;
            ST_TRY(pack16(c, cur, tmp16, a.C[i], hw));
            cur16 = tmp16;
        }
        unsigned short* dst16 = (cur16 == c->diff16A) ? c->diff16B : c->diff16A;
        if ((r.mask == MASK_F32 || r.kind == B_POOL_CLASSIC) && !fwd[below].out32)
            return fail(ST_ERR_STATE, "internal: blob %d, which the backward of %s reads, is not materialised in fp32", below, L.name.c_str());
        // conv: the diff above is still the POOLED one, expanded through the map of the pool above (r.unpool) -- read as what the
        // forward wrote into it
        const unsigned char* unpool_amap = r.unpool ? a.amap[i + 1] : nullptr;
        const bool unpool_ave = r.unpool && fwd[i + 1].amap == AMAP_BLOCKED16_AVE;
        const double conv_flops = 2.0 * 9 * L.cin * L.cout * px;
        switch (r.kind) {
        case B_SMALLM16: {
            // bf16 feature path: this conv's operands are bf16 too
            ProfScope ps(c, P_CONV_DGRAD, conv_flops, px * (2.0 * L.cout + 4.0 * L.cin));
            HIP_TRY(launch_conv3x3_dgrad_smallM16(cur16, L.w_raw_r, dst, inject, L.cout, L.cin, H, W, c->stream));
            break;
        }
        case B_SMALLM: {
            ProfScope ps(c, P_CONV_DGRAD, conv_flops, 4.0 * px * (L.cin + L.cout));
            HIP_TRY(launch_conv3x3_dgrad_smallM(cur, L.w_raw, dst, inject, L.cout, L.cin, H, W, c->stream));
            break;
        }
        case B_CONV16: {
            Conv16Problem p{};
            p.in16 = cur16; p.wpack16 = L.w16_bwd; p.bias = nullptr;
            p.out = r.out32 ? dst : nullptr; p.out16 = r.out16 ? dst16 : nullptr;
            p.inject = inject;
            if (r.mask == MASK_F32) p.mask_src = a.data[below];
            if (r.mask == MASK_BF16) p.mask16 = a.data16[below];
            if (r.mask == MASK_BITS) p.mask_bits = a.bits[below];
            if (r.style) {              // the style gradient of blob `below` rides on this launch: out = mask(conv) + D' @ F (+ inject)
                p.s_in16 = c->sf_in[below]; p.s_wpack16 = c->sf_w[below];
                prof_note(c, P_STYLE_FUSED_BF16, 2.0 * L.cin * L.cin * px);      // (extra K chunks of the launch below; its own flops stay SURVEY 8(d)'s)
            }
            p.K = L.cout; p.M = L.cin; p.MPad = conv_mpad(L.cin); p.H = H; p.W = W; p.relu = 0;
            p.unpool_amap = unpool_amap;               // (3/4 byte per pooled channel value more, 1.5 less per full one)
            p.unpool_ave = unpool_ave;
            const double mask_bytes = r.mask == MASK_BITS ? 0.125 : r.mask == MASK_BF16 ? 2.0 : r.mask == MASK_F32 ? 4.0 : 0.0;
            ProfScope ps(c, P_CONV_DGRAD_BF16, conv_flops,
                         px * ((r.unpool ? 0.75 : 2.0) * L.cout + (r.style ? 2.0 : 0.0) * L.cin + (r.out32 ? 4.0 : 0.0) * L.cin + (r.out16 ? 2.0 : 0.0) * L.cin + mask_bytes * L.cin));
            HIP_TRY(launch_conv3x3_bf16(p, c->stream));
            break;
        }
        case B_WINO: case B_WINO_SPLIT: case B_DIRECT: {
            ConvProblem p{};
            p.in = cur; p.wpack = L.w_bwd; p.bias = nullptr; p.out = dst;
            p.mask_src = r.mask == MASK_F32 ? a.data[below] : nullptr; p.inject = inject;
            p.K = L.cout; p.M = L.cin; p.MPad = conv_mpad(L.cin); p.H = H; p.W = W; p.relu = 0;
            p.unpool_amap = unpool_amap;
            ProfScope ps(c, r.kind == B_WINO_SPLIT ? P_CONV_DGRAD_WSPLIT : r.kind == B_WINO ? P_CONV_DGRAD_WINO : P_CONV_DGRAD, conv_flops,
                         4.0 * px * (L.cin + (r.unpool ? 0.3125 : 1.0) * L.cout));
            if (r.kind == B_WINO_SPLIT) { p.wpack = reinterpret_cast<const float*>(L.us_bwd.get()); ST_TRY(wino_scratch(c, p, wino_split_resolve(p.K, p.M, H, W).splits)); HIP_TRY(launch_conv3x3_wino_split(p, c->stream)); }
            else if (r.kind == B_WINO) { p.wpack = L.u_bwd; ST_TRY(wino_scratch(c, p, wino_resolve(p.K, p.M, H, W).splits)); HIP_TRY(launch_conv3x3_wino(p, c->stream)); }
            else HIP_TRY(launch_conv3x3(p, c->stream));
            break;
        }
        case B_AVEPOOL: {
            ProfScope ps(c, P_AVEPOOL_BWD, 0, 4.0 * (double)Cb * H * W +
                         n_below * (4.0 * ((r.mask != MASK_NONE ? 1 : 0) + (inject ? 1 : 0) + (r.out32 ? 1 : 0)) + (r.out16 ? 2.0 : 0.0)));
            HIP_TRY(launch_avepool_bwd(cur, r.mask != MASK_NONE ? a.data[below] : nullptr, inject, r.out32 ? dst : nullptr, r.out16 ? dst16 : nullptr, Cb, Hb, Wb, c->stream));
            break;
        }
        case B_POOL_IDX16: {
            ProfScope ps(c, P_POOL_BWD, 0, (double)Cb * (hw * 3.0 + (size_t)Hb * Wb * 2.0));
            HIP_TRY(launch_maxpool_bwd_idx16(cur16, a.amap[i], dst16, Cb, Hb, Wb, c->stream));
            break;
        }
        case B_AVEPOOL_MAP16: {
            if (fwd[i].amap != AMAP_BLOCKED16_AVE) return fail(ST_ERR_STATE, "internal: the forward of %s wrote no sign map", L.name.c_str());
            ProfScope ps(c, P_AVEPOOL_BWD_MAP16, 0, (double)Cb * (hw * 3.0 + (size_t)Hb * Wb * 2.0));
            HIP_TRY(launch_avepool_bwd_map16(cur16, a.amap[i], dst16, Cb, Hb, Wb, c->stream));
            break;
        }
        case B_POOL_AMAP: {
            ProfScope ps(c, P_POOL_BWD, 0, (double)Cb * (px * 5.0 + (double)Hb * Wb * 4.0));
            HIP_TRY(launch_maxpool_bwd_amap(cur, a.amap[i], dst, Cb, Hb, Wb, c->stream));
            break;
        }
        case B_POOL_CLASSIC: {
            ProfScope ps(c, P_POOL_BWD, 0, 4.0 * n_below * 2.25);
            HIP_TRY(launch_maxpool_bwd(cur, a.data[below], dst, inject, r.mask != MASK_NONE, Cb, Hb, Wb, c->stream));
            break;
        }
        case B_IN_DGRAD_BELOW:
            continue;                                      // the running diff stays the pooled one: the next launch expands it
        case B_NONE:
            return fail(ST_ERR_STATE, "internal: no route for the backward of layer %s", L.name.c_str());
        }
        if (c->tap.armed && c->tap.blob == below) {        // test hook st_tap_diff: exactly what this launch wrote, before the next one overwrites it
            DiffTap& t = c->tap;
            const size_t hwb = (size_t)Hb * Wb;
            if (r.out32) {
                ST_TRY(t.d32.reserve((size_t)Cb * hwb));
                HIP_TRY(hipMemcpyAsync(t.d32, dst, (size_t)Cb * hwb * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
            }
            if (r.out16) {
                ST_TRY(t.d16.reserve(act16_elems(Cb, hwb)));
                HIP_TRY(hipMemcpyAsync(t.d16, dst16, act16_elems(Cb, hwb) * sizeof(unsigned short), hipMemcpyDeviceToDevice, c->stream));
            }
            t.have32 = r.out32; t.have16 = r.out16; t.C = Cb; t.h = Hb; t.w = Wb;
            t.captured = true;
        }
        cur = r.out32 ? dst : nullptr;
        cur16 = r.out16 ? dst16 : nullptr;
    }
    if (!cur) return fail(ST_ERR_STATE, "internal: the backward chain ended without an fp32 image gradient");
    *out = cur;
    return ST_OK;
}

int ensure_input_buffers(st_ctx* c, int H, int W)
{
    if (c->H == H && c->W == W && c->x[0]) return ST_OK;
    // the activations are those of the old geometry (blob "data" may be one of the buffers freed below; st_backward sizes its
    // work buffers by the new one): the hooks refuse until the next forward
    c->act.valid_to = -1;
    if (c->lt.any) { c->lt.any = false; c->lt.resized = true; }      // (st_get_layer_terms: the inject buffers and stmp go below)
    if (c->tap.have) { c->tap.have = false; c->tap.resized = true; }  // (st_get_tapped_diff: the copy is that of the old geometry)
    lap_input_resized(c);
    anchor_input_resized(c);
    mat_input_resized(c);
    jitter_input_resized(c);
    const size_t n3 = (size_t)3 * H * W;
    for (int i = 0; i < 2; ++i) ST_TRY(c->x[i].alloc(n3));
    ST_TRY(c->grad.alloc(n3));
    c->m.reset(); c->v.reset();
    ST_TRY(c->m.alloc(n3)); ST_TRY(c->v.alloc(n3));
    c->g_cur.reset(); c->pvec.reset();
    for (int i = 0; i <= st_ctx::kCorr; ++i) { c->hs[i].reset(); c->hy[i].reset(); }
    ST_TRY(c->hwc_dev.alloc(n3));
    c->avg.reset(); c->avg_items = 0;              // the iterate average follows the input's size and starts empty (st_resample_state puts it back)
    if (c->avg_decay > 0) ST_TRY(c->avg.alloc(n3));
    c->H = H; c->W = W; c->cur = 0;
    // work buffers that follow the input geometry
    for (auto& p : c->inject) p.reset();
    std::fill(c->inject_roi_zero.begin(), c->inject_roi_zero.end(), 0);
    c->diffA.reset(); c->diffB.reset(); c->stmp.reset(); c->diff16A.reset(); c->diff16B.reset();
    std::vector<int> C, h, w;
    shapes_for(c, H, W, C, h, w);
    c->max_blob = 0;
    for (int i = 0; i < c->nb; ++i) c->max_blob = std::max(c->max_blob, (size_t)C[i] * h[i] * w[i]);
    return ST_OK;
}

int stage_upload(st_ctx* c, const void* host, size_t bytes)
{
    ST_TRY(c->stage_dev.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(c->stage_dev, host, bytes, hipMemcpyHostToDevice, c->stream));
    return ST_OK;
}

int preprocess_into(st_ctx* c, const void* hwc, int H, int W, int is_u8, float* dst)
{
    if (!hwc || H <= 0 || W <= 0) return fail(ST_ERR_ARG, "bad image (%p, %d x %d)", hwc, H, W);
    const size_t n = (size_t)H * W * 3;
    ST_TRY(stage_upload(c, hwc, n * (is_u8 ? 1 : 4)));
    ProfScope ps(c, P_MISC, 0, 0);
    if (is_u8) HIP_TRY(launch_preprocess_u8(c->stage_dev, dst, H, W, c->stream));
    else HIP_TRY(launch_preprocess_f32((const float*)c->stage_dev.get(), dst, H, W, c->stream));
    return ST_OK;
}

// The iterate is about to be overwritten.  After an evaluation blob "data" IS the iterate's buffer (ActSet::data[0] is borrowed):
// the other blobs would no longer belong to it, so the hooks refuse until the next forward (st_forward's probe image has a buffer
// of its own and stays valid).
void iterate_overwritten(st_ctx* c)
{
    if (!c->act.data.empty() && c->act.data[0] && (c->act.data[0] == c->x[0] || c->act.data[0] == c->x[1])) c->act.valid_to = -1;
}

// an input of a new geometry: every size-dependent optimizer tensor starts from zero
int set_input_common(st_ctx* c, int H, int W)
{
    const bool reshaped = !(c->H == H && c->W == W && c->x[0]);
    ST_TRY(ensure_input_buffers(c, H, W));
    if (reshaped) {            // every size-dependent optimizer tensor starts from zero
        c->m_zero = c->v_zero = true;
        c->lb_clear = true;
        c->have_cur = false;
    }
    return ST_OK;
}
// content image on the device -> features of every blob (worker.py:204-209); also the tail of st_resample_content
int content_from_device(st_ctx* c, const float* xdev, int H, int W)
{
    ST_TRY(act_ensure(c, c->act, H, W));
    // features of the blobs that carry a content weight NOW (every blob until the first st_set_weights, like worker.py:204-209);
    // the others come from ensure_content_features if a later weight table asks for them
    std::vector<char> used(c->nb, 0);
    int deepest = -1;
    for (const ActiveLayer& al : c->active) if (al.c) { used[al.blob] = 1; deepest = std::max(deepest, al.blob); }
    if (deepest > 0) ST_TRY(forward_range(c, c->act, xdev, deepest));
    for (int i = 0; i < c->nb; ++i) {
        if (!used[i]) { c->content_feat[i].reset(); continue; }
        const size_t n = (size_t)c->act.C[i] * c->act.h[i] * c->act.w[i];
        if (c->cH != H || c->cW != W || !c->content_feat[i]) ST_TRY(c->content_feat[i].alloc(n));
        HIP_TRY(hipMemcpyAsync(c->content_feat[i], i == 0 ? xdev : c->act.data[i], n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    }
    c->act.valid_to = -1;
    if (xdev != c->content_x) {                 // keep the preprocessed image itself (== blob "data")
        if (c->cH != H || c->cW != W || !c->content_x) ST_TRY(c->content_x.alloc((size_t)3 * H * W));
        HIP_TRY(hipMemcpyAsync(c->content_x, xdev, (size_t)3 * H * W * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    }
    c->cH = H; c->cW = W;
    c->have_content = true;
    c->feat_dy = c->feat_dx = 0;                // (jitter: these are the features of the unshifted image)
    c->lap.targets_ok = false;                  // the Laplacian term's targets follow the content image: taken again before the next evaluation
    c->mat.windows_ok = false;                  // ... and so do the photorealism term's per-window data
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ST_OK;
}

// The reference keeps the content features of EVERY blob (worker.py:204-209) because the weights may change later.  Here
// st_set_weights drops the features of blobs without a content weight (11 of 12 GB for one window of the 8192^2 / 2x4 job) and
// the preprocessed image is kept instead: should such a blob gain a content weight afterwards, its features are taken again by
// the same forward (same kernels, same precision) before the next evaluation.
int ensure_content_features(st_ctx* c)
{
    int need = -1;
    for (const ActiveLayer& al : c->active) if (al.c && !c->content_feat[al.blob]) need = std::max(need, al.blob);
    if (need < 0) return ST_OK;
    if (!c->have_content || !c->content_x) return fail(ST_ERR_STATE, "content image missing");
    ST_TRY(act_ensure(c, c->act, c->cH, c->cW));
    if (need > 0) ST_TRY(forward_range(c, c->act, c->content_x, need));
    for (const ActiveLayer& al : c->active) {
        const int b = al.blob;
        if (!al.c || c->content_feat[b]) continue;
        const size_t n = (size_t)c->act.C[b] * c->act.h[b] * c->act.w[b];
        ST_TRY(c->content_feat[b].alloc(n));
        HIP_TRY(hipMemcpyAsync(c->content_feat[b], b == 0 ? c->content_x : c->act.data[b], n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    }
    c->act.valid_to = -1;                      // (the activations are the content image's now)
    return ST_OK;
}
}  // namespace st2e

extern "C" const char* st_last_error(void) { return st2e::g_err; }

// ------------------------------------------------------------------------------------------- C ABI
extern "C" {

int st_create(st_ctx** out, int device_id, const st_layer_desc* layers, int n_layers)
{
    if (!out) return fail(ST_ERR_ARG, "out is NULL");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail(ST_ERR_HIP, "no HIP device visible");
    if (device_id < 0 || device_id >= ndev) return fail(ST_ERR_ARG, "device %d out of range (%d visible)", device_id, ndev);
    HIP_TRY(hipSetDevice(device_id));
    std::unique_ptr<st_ctx, int (*)(st_ctx*)> c(new st_ctx(), st_destroy);      // every early return tears down what exists so far
    c->device = device_id;
    c->wino = env_int("ST2_WINO", c->wino) != 0;
    c->graphs = env_int("ST2_GRAPH", c->graphs) != 0;
    { const size_t side = (size_t)env_int("ST2_GRAPH_MAX_PX", 768); c->graph_max_px = side * side; }
    if (n_layers <= 0) {
        for (const auto& l : kVgg19) {
            Layer L; L.is_conv = l.kind == 0; L.name = l.name; L.cin = l.cin; L.cout = l.cout;
            c->topo.push_back(std::move(L));
        }
    } else {
        int cprev = 3;
        for (int i = 0; i < n_layers; ++i) {
            const int kind = layers[i].kind;
            if (kind != ST_LAYER_CONV && kind != ST_LAYER_POOL && kind != ST_LAYER_AVEPOOL)
                return fail(ST_ERR_ARG, "layer %d (%s): unknown kind %d", i, layers[i].name ? layers[i].name : "", kind);
            Layer L; L.is_conv = kind == ST_LAYER_CONV; L.ave = kind == ST_LAYER_AVEPOOL; L.name = layers[i].name ? layers[i].name : "";
            if (L.is_conv) {
                L.cin = layers[i].cin; L.cout = layers[i].cout;
                if (L.cin != cprev || L.cout <= 0) return fail(ST_ERR_ARG, "layer %s: cin %d does not follow %d", L.name.c_str(), L.cin, cprev);
                cprev = L.cout;
            }
            c->topo.push_back(std::move(L));
        }
    }
    if ((int)c->topo.size() + 1 > kMaxTraceLayers) return fail(ST_ERR_ARG, "too many layers");
    c->blob_names.push_back("data");
    for (const Layer& L : c->topo) c->blob_names.push_back(L.name);
    c->nb = (int)c->blob_names.size();
    HIP_TRY(hipStreamCreate(&c->stream));
    c->content_feat.resize(c->nb);
    c->style_gram.resize(c->nb);
    c->style_valid.assign(c->nb, 0);
    c->inject.resize(c->nb);
    c->inject_roi_zero.assign(c->nb, 0);
    c->layer_part.resize(c->nb);
    c->s2_part.resize(c->nb);
    c->sfuse_w.resize(c->nb);
    c->cnt.assign(c->nb * 6, 0);
    c->norm_valid.assign(c->nb * 3, 0);
    ST_TRY(c->norms.alloc(c->nb * 3));
    ST_TRY(c->image_part.alloc(6 * kMaxPartials));
    ST_TRY(c->trace_dev.alloc(kMaxTraceLayers * 6 + 8 + 6));                  // (+ l_loss, l_grad under st_set_laplacian, a_loss, a_grad under st_set_anchor, m_loss, m_grad under st_set_matting)
    ST_TRY(c->trace_sums.alloc(kMaxTraceLayers * kLayerSlots + kImageSlots));
    ST_TRY(c->lb_dev.alloc(1));
    HIP_TRY(hipMemset(c->lb_dev, 0, sizeof(LbfgsDev)));
    ST_TRY(c->lb_part.alloc(4 * kMaxPartials));
    ST_TRY(c->trace_host.alloc(kMaxTraceLayers * 6 + 8 + 6));
    // worker.py:129-133: all-ones weights over every blob until SetWeights arrives
    for (int b = 0; b < c->nb; ++b) c->rows.push_back(ActiveLayer{b, 1.f, 1.f, 1.f, true, true, true});
    c->active = c->rows;
    *out = c.release();
    return ST_OK;
}

int st_destroy(st_ctx* c)
{
    if (!c) return ST_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);      // (null: st_create failed before it had a stream; nothing ran)
    if (c->pipe.copy) (void)hipStreamSynchronize(c->pipe.copy);
    for (int i = 0; i < 2; ++i) if (c->gexec[i]) (void)hipGraphExecDestroy(c->gexec[i]);
    for (int i = 0; i < st_ctx::Pipe::kSlots; ++i) {
        if (c->pipe.ready[i]) (void)hipEventDestroy(c->pipe.ready[i]);
        if (c->pipe.done[i]) (void)hipEventDestroy(c->pipe.done[i]);
    }
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    comm_free(c);
    // the buffers go with the context, BEFORE the streams they were used on
    const hipStream_t stream = c->stream, copy = c->pipe.copy;
    delete c;
    if (copy) (void)hipStreamDestroy(copy);
    if (stream) (void)hipStreamDestroy(stream);
    return ST_OK;
}

// the split-operand Winograd packs of one conv layer (both directions where the kernel can take them); w = (Cout, Cin, 3, 3) on the host
static int make_split_packs(Layer& L, const float* w)
{
    for (int dir = 0; dir < 2; ++dir) {
        const int K = dir ? L.cout : L.cin, M = dir ? L.cin : L.cout;
        DevBuf<unsigned short>& dst = dir ? L.us_bwd : L.us_fwd;
        if (dst || !wino_split_resolve(K, M, 4, 4).ok) continue;
        std::vector<unsigned short> hu(wino_split_pack_elems(K, M), 0);
        if (dir) pack_wino_split_weights_dgrad(w, L.cout, L.cin, hu.data()); else pack_wino_split_weights_fwd(w, L.cout, L.cin, hu.data());
        ST_TRY(dst.alloc(hu.size()));
        HIP_TRY(hipMemcpy(dst, hu.data(), hu.size() * 2, hipMemcpyHostToDevice));
    }
    return ST_OK;
}

int st_load_conv_weights(st_ctx* c, const char* layer, const float* w, const float* bias)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c || !layer || !w) return fail(ST_ERR_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    for (Layer& L : c->topo) {
        if (!L.is_conv || L.name != layer) continue;
        const size_t nf = conv_pack_floats(L.cin, L.cout), nb = conv_pack_floats(L.cout, L.cin);
        std::vector<float> pf(nf), pb(nb), bp(conv_mpad(L.cout), 0.f);
        pack_conv_weights_fwd(w, L.cout, L.cin, pf.data());
        pack_conv_weights_dgrad(w, L.cout, L.cin, pb.data());
        if (bias) memcpy(bp.data(), bias, L.cout * sizeof(float));
        // the old packs go first (a reload peaks at one set); until the new ones are complete the layer counts as never loaded, so
        // that a reload that fails half-way leaves a layer forward_range refuses, not one with null packs
        L.loaded = false;
        static_cast<LayerPacks&>(L) = LayerPacks{};       // move-assigns twelve empty buffers: frees every pack, leaves name / cin / cout
        for (int dir = 0; dir < 2; ++dir) {   // Winograd packs for the directions the Winograd kernel can take (any image size)
            const int K = dir ? L.cout : L.cin, M = dir ? L.cin : L.cout;
            if (!wino_resolve(K, M, 4, 4).ok) continue;
            std::vector<float> hu(wino_pack_floats(K, M));
            if (dir) pack_wino_weights_dgrad(w, L.cout, L.cin, hu.data()); else pack_wino_weights_fwd(w, L.cout, L.cin, hu.data());
            DevBuf<float>& dst = dir ? L.u_bwd : L.u_fwd;
            ST_TRY(dst.alloc(hu.size()));
            HIP_TRY(hipMemcpy(dst, hu.data(), hu.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        {   // bf16 packs for the bf16 feature path
            const size_t n16f = conv16_pack_elems(L.cin, L.cout), n16b = conv16_pack_elems(L.cout, L.cin);
            std::vector<unsigned short> hf(n16f), hb(n16b);
            pack_conv_weights16_fwd(w, L.cout, L.cin, hf.data());
            pack_conv_weights16_dgrad(w, L.cout, L.cin, hb.data());
            ST_TRY(L.w16_fwd.alloc(n16f)); ST_TRY(L.w16_bwd.alloc(n16b));
            HIP_TRY(hipMemcpy(L.w16_fwd, hf.data(), n16f * 2, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(L.w16_bwd, hb.data(), n16b * 2, hipMemcpyHostToDevice));
        }
        if (L.cin == 3 && L.cout % 32 == 0) {   // first layer on the bf16 path: split weights for conv3x3_first_split.hip
            std::vector<unsigned short> hs(conv_first_split_pack_elems(L.cout));
            pack_conv_first_split(w, bias, L.cout, L.cin, hs.data());
            ST_TRY(L.w_split.alloc(hs.size()));
            HIP_TRY(hipMemcpy(L.w_split, hs.data(), hs.size() * 2, hipMemcpyHostToDevice));
        }
        ST_TRY(L.w_fwd.alloc(nf)); ST_TRY(L.w_bwd.alloc(nb));
        ST_TRY(L.w_raw.alloc((size_t)L.cout * L.cin * 9)); ST_TRY(L.bias.alloc(bp.size()));
        HIP_TRY(hipMemcpy(L.w_fwd, pf.data(), nf * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(L.w_bwd, pb.data(), nb * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(L.w_raw, w, (size_t)L.cout * L.cin * 9 * sizeof(float), hipMemcpyHostToDevice));
        if (conv_dgrad_smallM_ok(L.cout, L.cin) && L.cout % 8 == 0) {       // bf16 path: the first layer's dgrad multiplies bf16 operands
            std::vector<float> wr((size_t)L.cout * L.cin * 9);
            for (size_t k = 0; k < wr.size(); ++k) {
                unsigned u; memcpy(&u, &w[k], 4);
                u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;          // round to nearest even (weights are finite)
                memcpy(&wr[k], &u, 4);
            }
            ST_TRY(L.w_raw_r.alloc(wr.size()));
            HIP_TRY(hipMemcpy(L.w_raw_r, wr.data(), wr.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        HIP_TRY(hipMemcpy(L.bias, bp.data(), bp.size() * sizeof(float), hipMemcpyHostToDevice));
        if (c->wino_split) ST_TRY(make_split_packs(L, w));
        L.loaded = true;
        return ST_OK;
    }
    return fail(ST_ERR_ARG, "no conv layer named %s", layer);
}

int st_set_conv_algo(st_ctx* c, int winograd)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    if (winograd < 0 || winograd > 2) return fail(ST_ERR_ARG, "conv algorithm %d: 0 direct, 1 Winograd (fp32 matrix cores), 2 split-operand Winograd (bf16 matrix cores, fp32 results)", winograd);
    c->wino = winograd != 0;
    c->wino_split = winograd == 2;
    if (c->wino_split) {       // the packs of the layers that are loaded already (weights come back from the device copy)
        HIP_TRY(hipSetDevice(c->device));
        for (Layer& L : c->topo) {
            if (!L.is_conv || !L.loaded || !L.w_raw) continue;
            std::vector<float> w((size_t)L.cout * L.cin * 9);
            HIP_TRY(hipMemcpy(w.data(), L.w_raw, w.size() * sizeof(float), hipMemcpyDeviceToHost));
            ST_TRY(make_split_packs(L, w.data()));
        }
    }
    return ST_OK;
}

int st_set_gram_algo(st_ctx* c, int algo)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    if (algo != 0 && algo != 1) return fail(ST_ERR_ARG, "gram algorithm %d: 0 fp32 matrix cores, 1 split operands (bf16 matrix cores, fp32 results)", algo);
    if (algo == 1) {           // the operand image of D for the widest blob the kernels take; the flag is committed last
        std::vector<int> C, h, w;
        shapes_for(c, 16, 16, C, h, w);
        size_t need = 0;
        for (int i = 0; i < c->nb; ++i) need = std::max(need, style_split_scratch(C[i], 4));
        if (need > c->dsplit.cap()) {      // the new buffer exists before the old one is given up
            HIP_TRY(hipSetDevice(c->device));
            DevBuf<unsigned short> p;
            ST_TRY(p.alloc(need));
            HIP_TRY(hipStreamSynchronize(c->stream));
            c->dsplit = std::move(p);
        }
    }
    c->epoch++;                // anything but st_step may change what a step launches: captured step graphs are stale
    c->gram_split = algo == 1;
    return ST_OK;
}

int st_set_pool_algo(st_ctx* c, int algo)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    if (algo != 0 && algo != 1) return fail(ST_ERR_ARG, "pool algorithm %d: 0 every average pool a stand-alone pass, 1 fused into the bf16 conv launches around it where a build exists", algo);
    c->epoch++;                // anything but st_step may change what a step launches: captured step graphs are stale
    // (the activations stay as they are: FwdRoute::amap says which map their forward wrote, and the backward reads that record)
    c->pool_algo = algo;
    return ST_OK;
}

int st_get_pool_algo(st_ctx* c, int* algo)
{
    if (!c || !algo) return fail(ST_ERR_ARG, "NULL argument");
    *algo = c->pool_algo;
    return ST_OK;
}

int st_get_algos(st_ctx* c, int* conv, int* gram)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    if (conv) *conv = c->wino_split ? 2 : c->wino ? 1 : 0;
    if (gram) *gram = c->gram_split ? 1 : 0;
    return ST_OK;
}

int st_set_precision(st_ctx* c, int bf16_features)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    c->bf16 = bf16_features != 0;
    // 1: the lean data flow (objective evaluations write fp32 only where something reads fp32); 2: every fp32 blob and diff
    // as in round 1 (A/B reference of the tests); environment ST2_BF16_LEAN=0 forces 2
    c->lean = bf16_features == 1 && !env_off("ST2_BF16_LEAN");
    return ST_OK;
}

int st_num_blobs(st_ctx* c) { return c ? c->nb : 0; }
const char* st_blob_name(st_ctx* c, int i) { return (c && i >= 0 && i < c->nb) ? c->blob_names[i].c_str() : nullptr; }

int st_blob_shape(st_ctx* c, int index, int H, int W, int* oc, int* oh, int* ow)
{
    if (!c || index < 0 || index >= c->nb) return fail(ST_ERR_ARG, "bad blob index %d", index);
    std::vector<int> C, h, w;
    shapes_for(c, H, W, C, h, w);
    if (oc) *oc = C[index];
    if (oh) *oh = h[index];
    if (ow) *ow = w[index];
    return ST_OK;
}

// ---- model test hooks
int st_forward(st_ctx* c, const float* x_nchw, int H, int W, int last_blob)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c || !x_nchw || H <= 0 || W <= 0) return fail(ST_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    // The probe image lives in a buffer of its own: the job's iterate (x) is never touched.  A forward at ANOTHER
    // geometry re-creates the size-dependent buffers exactly like st_set_input at a new size does (optimizer state
    // starts from zero again); st_backward works on this geometry.
    ST_TRY(set_input_common(c, H, W));
    ST_TRY(act_ensure(c, c->act, H, W));
    const size_t n3 = (size_t)3 * H * W;
    ST_TRY(c->fwd_x.reserve(n3));
    HIP_TRY(hipMemcpyAsync(c->fwd_x, x_nchw, n3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (last_blob < 0 || last_blob >= c->nb) last_blob = c->nb - 1;
    ST_TRY(forward_range(c, c->act, c->fwd_x, last_blob));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ST_OK;
}

int st_get_blob(st_ctx* c, int index, float* out)
{
    if (!c || index < 0 || index >= c->nb || !out) return fail(ST_ERR_ARG, "bad argument");
    if (index > c->act.valid_to) return fail(ST_ERR_STATE, "blob %d was not computed by the last forward", index);
    if (!c->act.plan.fwd[index].out32) return fail(ST_ERR_STATE, "blob %d (%s) is not materialised in fp32 by the lean evaluation of an iteration (st_opfunc / st_forward write every fp32 blob; bf16: st_set_precision(ctx, 2))", index, c->blob_names[index].c_str());
    const size_t n = (size_t)c->act.C[index] * c->act.h[index] * c->act.w[index];
    HIP_TRY(hipMemcpy(out, c->act.data[index], n * sizeof(float), hipMemcpyDeviceToHost));
    return ST_OK;
}

int st_backward(st_ctx* c, int n, const int* blob_index, const float* const* diffs, float* out_grad)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c || !out_grad || n < 0) return fail(ST_ERR_ARG, "bad argument");
    if (c->act.valid_to < 0) return fail(ST_ERR_STATE, "st_forward first");
    HIP_TRY(hipSetDevice(c->device));
    const size_t n3 = (size_t)3 * c->H * c->W;
    std::vector<const float*> inj(c->nb, nullptr);
    int top = -1;
    for (int i = 0; i < n; ++i) {
        const int b = blob_index[i];
        if (b < 0 || b > c->act.valid_to) return fail(ST_ERR_ARG, "diff for blob %d which the last forward did not reach", b);
        const size_t nb = (size_t)c->act.C[b] * c->act.h[b] * c->act.w[b];
        if (!c->inject[b]) ST_TRY(c->inject[b].alloc(nb));
        HIP_TRY(hipMemcpyAsync(c->inject[b], diffs[i], nb * sizeof(float), hipMemcpyHostToDevice, c->stream));
        c->inject_roi_zero[b] = 0;
        if ((int)c->lt.diff.size() == c->nb) c->lt.diff[b] = LT_OVERWRITTEN;
        inj[b] = c->inject[b];
        top = std::max(top, b);
    }
    if (top < 0) { memset(out_grad, 0, n3 * sizeof(float)); return ST_OK; }
    if (!c->diffA) { ST_TRY(c->diffA.alloc(c->max_blob)); ST_TRY(c->diffB.alloc(c->max_blob)); }
    const float* g = inj[0];
    if (top > 0) ST_TRY(backward_chain(c, top, inj[top], inj, &g));
    HIP_TRY(hipMemcpyAsync(out_grad, g, n3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ST_OK;
}

int st_gram(st_ctx* c, int index, float* out)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c || index < 0 || index >= c->nb || !out) return fail(ST_ERR_ARG, "bad argument");
    if (index > c->act.valid_to) return fail(ST_ERR_STATE, "blob %d was not computed by the last forward", index);
    // (the Gram contracts the fp32 blob: what the last evaluation did not write is an earlier evaluation's, or nothing)
    if (!c->act.plan.fwd[index].out32) return fail(ST_ERR_STATE, "blob %d (%s) is not materialised in fp32 by the lean evaluation of an iteration: no Gram of it (st_opfunc / st_forward write every fp32 blob; bf16: st_set_precision(ctx, 2))", index, c->blob_names[index].c_str());
    HIP_TRY(hipSetDevice(c->device));
    const int C = c->act.C[index], hw = c->act.h[index] * c->act.w[index];
    DevBuf<float> g;
    ST_TRY(g.alloc((size_t)C * C));
    int r = style_gram(c, c->act, style_term(c, c->act, index, nullptr, true), nullptr, g, C, (double)C * hw, nullptr, nullptr);
    if (r == ST_OK) {
        hipError_t e = hipMemcpyAsync(out, g, (size_t)C * C * sizeof(float), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) r = fail(ST_ERR_HIP, "gram copy: %s", hipGetErrorString(e));
    }
    return r;
}

// ---- image slots
int st_set_input(st_ctx* c, const void* hwc, int H, int W, int is_u8)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    ST_TRY(set_input_common(c, H, W));
    iterate_overwritten(c);
    c->avg_items = 0;        // a new iterate: its running mean starts empty
    ST_TRY(preprocess_into(c, hwc, H, W, is_u8, c->x[c->cur]));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ST_OK;
}

int st_set_input_nchw(st_ctx* c, const float* x, int H, int W)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c || !x || H <= 0 || W <= 0) return fail(ST_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    ST_TRY(set_input_common(c, H, W));
    iterate_overwritten(c);
    c->avg_items = 0;        // a new iterate: its running mean starts empty
    HIP_TRY(hipMemcpy(c->x[c->cur], x, (size_t)3 * H * W * sizeof(float), hipMemcpyHostToDevice));
    return ST_OK;
}

int st_get_input_nchw(st_ctx* c, float* out)
{
    if (!c || !out || !c->x[0]) return fail(ST_ERR_STATE, "no input image");
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->x[c->cur], (size_t)3 * c->H * c->W * sizeof(float), hipMemcpyDeviceToHost));
    return ST_OK;
}

int st_input_shape(st_ctx* c, int* H, int* W)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    if (H) *H = c->H;
    if (W) *W = c->W;
    return ST_OK;
}

int st_set_content(st_ctx* c, const void* hwc, int H, int W, int is_u8)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> tmp;
    ST_TRY(tmp.alloc((size_t)3 * H * W));
    int r = preprocess_into(c, hwc, H, W, is_u8, tmp);
    if (r == ST_OK) r = content_from_device(c, tmp, H, W);
    (void)hipStreamSynchronize(c->stream);       // (before tmp goes)
    return r;
}

int st_set_content_nchw(st_ctx* c, const float* x, int H, int W)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c || !x || H <= 0 || W <= 0) return fail(ST_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> tmp;
    ST_TRY(tmp.alloc((size_t)3 * H * W));
    int r = ST_OK;
    if (hipMemcpy(tmp, x, (size_t)3 * H * W * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) r = fail(ST_ERR_HIP, "content upload failed");
    if (r == ST_OK) r = content_from_device(c, tmp, H, W);
    (void)hipStreamSynchronize(c->stream);       // (before tmp goes)
    return r;
}

int st_set_style(st_ctx* c, const void* hwc, int H, int W, int is_u8)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    ST_TRY(style_color_check(c));
    DevBuf<float> tmp;
    ST_TRY(tmp.alloc((size_t)3 * H * W));
    int r = preprocess_into(c, hwc, H, W, is_u8, tmp);
    if (r == ST_OK && c->style_match) r = style_recolor_enqueue(c, tmp, H, W);
    if (r == ST_OK) r = style_from_device(c, tmp, H, W);
    (void)hipStreamSynchronize(c->stream);       // (before tmp goes)
    return r;
}

int st_set_style_nchw(st_ctx* c, const float* x, int H, int W)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c || !x || H <= 0 || W <= 0) return fail(ST_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> tmp;
    ST_TRY(tmp.alloc((size_t)3 * H * W));
    int r = ST_OK;
    if (hipMemcpy(tmp, x, (size_t)3 * H * W * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) r = fail(ST_ERR_HIP, "style upload failed");
    if (r == ST_OK) r = style_from_device(c, tmp, H, W);
    (void)hipStreamSynchronize(c->stream);       // (before tmp goes)
    return r;
}

}  // extern "C"

namespace st2e {
// preprocessed style image on the device -> full forward, Gram of every blob (worker.py:211-218)
int style_from_device(st_ctx* c, const float* tmp, int H, int W)
{
    ActSet aux;                // (freed on return, after the synchronisation below)
    ActSet* a = &aux;
    const bool same = c->act.H == H && c->act.W == W && !c->act.data.empty();
    if (same) a = &c->act;
    int r = act_ensure(c, *a, H, W);
    if (r == ST_OK) r = forward_range(c, *a, tmp, c->nb - 1);
    for (int i = 0; i < c->nb && r == ST_OK; ++i) {
        const int C = a->C[i], hw = a->h[i] * a->w[i];
        if (!c->style_gram[i]) r = c->style_gram[i].alloc((size_t)C * C);
        if (r == ST_OK) r = style_gram(c, *a, style_term(c, *a, i, nullptr, true), nullptr, c->style_gram[i], C, (double)C * hw, nullptr, nullptr);
    }
    (void)hipStreamSynchronize(c->stream);
    if (same) c->act.valid_to = -1;
    if (r == ST_OK) { c->have_style = true; std::fill(c->style_valid.begin(), c->style_valid.end(), 1); }
    return r;
}
}  // namespace st2e

extern "C" {

// ---- measurement
int st_profile_enable(st_ctx* c, int on)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->prof_on = on != 0;
    c->prof.clear();
    c->ev_used = 0;
    return ST_OK;
}

int st_profile_num_classes(void) { return P_COUNT; }
const char* st_profile_class_name(int cls) { return (cls >= 0 && cls < P_COUNT) ? kProfNames[cls] : nullptr; }

int st_profile_read(st_ctx* c, long long* launches, double* ms, double* flops, double* bytes)
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < P_COUNT; ++i) {
        if (launches) launches[i] = 0;
        if (ms) ms[i] = 0;
        if (flops) flops[i] = 0;
        if (bytes) bytes[i] = 0;
    }
    for (const ProfRec& r : c->prof) {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, r.a, r.b));
        if (launches) launches[r.cls] += 1;
        if (ms) ms[r.cls] += t;
        if (flops) flops[r.cls] += r.flops;
        if (bytes) bytes[r.cls] += r.bytes;
    }
    c->prof.clear();
    c->ev_used = 0;
    return ST_OK;
}

// ---- test hook: what the funnel holds, over every context of the process
int st_live_bytes(long long* device, long long* pinned)
{
    if (device) *device = g_live_dev.load();
    if (pinned) *pinned = g_live_pin.load();
    return ST_OK;
}

}  // extern "C"
