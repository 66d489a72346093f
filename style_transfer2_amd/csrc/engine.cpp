// The device-resident style-transfer engine behind include/st2.h: context, model (forward / ranged backward), image slots.
//
// One st_ctx == one reference worker's model + StyleTransfer + optimizer (worker.py:32-315,
// optimizers.py:7-125) with all tensors living in HBM.  The host only sequences launches on one
// HIP stream; nothing crosses PCIe inside an iteration unless the caller asks for the iterate.
// The objective lives in engine_objective.cpp, the optimizers and the iteration in engine_step.cpp, resampling in
// engine_resample.cpp, the tile-sharded phases in engine_tile.cpp.
#include "engine.h"

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
                                          "style_grad_fused_in_conv_dgrad_bf16", "avepool_fwd", "avepool_bwd"};

static const struct { int kind; const char* name; int cin, cout; } kVgg19[] = {
    {0, "conv1_1", 3, 64}, {0, "conv1_2", 64, 64}, {1, "pool1", 0, 0},
    {0, "conv2_1", 64, 128}, {0, "conv2_2", 128, 128}, {1, "pool2", 0, 0},
    {0, "conv3_1", 128, 256}, {0, "conv3_2", 256, 256}, {0, "conv3_3", 256, 256}, {0, "conv3_4", 256, 256}, {1, "pool3", 0, 0},
    {0, "conv4_1", 256, 512}, {0, "conv4_2", 512, 512}, {0, "conv4_3", 512, 512}, {0, "conv4_4", 512, 512}, {1, "pool4", 0, 0},
    {0, "conv5_1", 512, 512}, {0, "conv5_2", 512, 512}, {0, "conv5_3", 512, 512}, {0, "conv5_4", 512, 512}, {1, "pool5", 0, 0},
};

// ---------------------------------------------------------------------------------------- helpers
int dmalloc(float** p, size_t nfloats)
{
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(nfloats, 1) * sizeof(float));
    if (e != hipSuccess) return fail(ST_ERR_HIP, "hipMalloc(%zu floats): %s", nfloats, hipGetErrorString(e));
    *p = (float*)q;
    return ST_OK;
}
void dfree(float*& p)
{
    if (p && hipFree(p) != hipSuccess) (void)hipGetLastError();   // never leave a sticky error behind
    p = nullptr;
}

// room for the split-K partial sums of a Winograd launch that would otherwise leave most CUs idle
int dmalloc16(unsigned short** p, size_t n)
{
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(n, 8) * sizeof(unsigned short));
    if (e != hipSuccess) return fail(ST_ERR_HIP, "hipMalloc(%zu bf16): %s", n, hipGetErrorString(e));
    *p = (unsigned short*)q;
    return ST_OK;
}
void dfree16(unsigned short*& p)
{
    if (p && hipFree(p) != hipSuccess) (void)hipGetLastError();
    p = nullptr;
}
// does the data gradient of conv layer L at this size run on the split-operand Winograd kernel?
static bool dgrad_takes_split(const st_ctx* c, const Layer& L, int h, int w)
{
    if (!(c->wino && c->wino_split && !c->bf16 && L.us_bwd && conv_wino_split_ok(L.cout, L.cin, h, w))) return false;
    // ST2_WS_DGRAD64=0: K <= 64 launches that the fp32 kernel could unpool (conv1_2's data gradient) stay on the fp32 matrix cores.  With
    // the first split epilogue that was the faster route (404 + 60 us of maxpool_bwd_amap_k against 429 us); since the branch-free
    // epilogue it is not (same-box A/B, profiles/r05_s_ab_split.txt: 177.4 against 176.1 it/s) -- kept as a switch for the A/B only
    { const char* e = getenv("ST2_WS_DGRAD64");
      if (e && *e == '0' && L.cout <= 64 && L.u_bwd && conv_wino_can_unpool(L.cout, L.cin, h, w)) return false; }
    return true;
}

int wino_scratch(st_ctx* c, ConvProblem& p, bool split_kernel)
{
    const int sp = split_kernel ? conv_wino_split_splits(p.K, p.M, p.H, p.W) : conv_wino_splits(p.K, p.M, p.H, p.W);
    if (sp <= 1) return ST_OK;
    const size_t need = (size_t)sp * p.M * p.H * p.W;
    if (need > c->conv_scratch_cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        dfree(c->conv_scratch); c->conv_scratch_cap = 0;
        ST_TRY(dmalloc(&c->conv_scratch, need));
        c->conv_scratch_cap = need;
    }
    p.scratch = c->conv_scratch; p.scratch_floats = c->conv_scratch_cap;
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

void act_free(ActSet& a)
{
    for (size_t i = 1; i < a.data.size(); ++i) dfree(a.data[i]);
    for (size_t i = 0; i < a.data16.size(); ++i) dfree16(a.data16[i]);
    for (size_t i = 0; i < a.amap.size(); ++i) if (a.amap[i]) { (void)hipFree(a.amap[i]); a.amap[i] = nullptr; }
    for (size_t i = 0; i < a.bits.size(); ++i) dfree16(a.bits[i]);
    a.bits.clear();
    a.data.clear();
    a.data16.clear();
    a.amap.clear();
    a.H = a.W = 0;
    a.valid_to = -1;
}

int act_ensure(st_ctx* c, ActSet& a, int H, int W)
{
    if (a.H == H && a.W == W && !a.data.empty()) return ST_OK;
    act_free(a);
    shapes_for(c, H, W, a.C, a.h, a.w);
    a.data.assign(c->nb, nullptr);
    a.data16.assign(c->nb, nullptr);
    a.amap.assign(c->nb, nullptr);
    a.has32.assign(c->nb, 0);
    a.amap_ok.assign(c->nb, 0);
    a.bits.assign(c->nb, nullptr);
    a.bits_ok.assign(c->nb, 0);
    for (int i = 1; i < c->nb; ++i) ST_TRY(dmalloc(&a.data[i], (size_t)a.C[i] * a.h[i] * a.w[i]));
    a.H = H; a.W = W;
    return ST_OK;
}

bool blob_active(const st_ctx* c, int b)
{
    for (const ActiveLayer& al : c->active) if (al.blob == b) return true;
    return false;
}

// Will the style term of blob b (a style layer) run entirely on the blob's bf16 copy (gram16.hip + style16.hip)?  Decided from
// shapes only, so that the forward (which may then skip the fp32 blob) and the objective agree.
bool style_runs16(const st_ctx* c, const ActSet& a, int b)
{
    if (!c->bf16 || b < 1 || !c->topo[b - 1].is_conv) return false;
    const int C = a.C[b], hw = a.h[b] * a.w[b];
    if (!(conv16_ok(c, C) && style_grad16_ok(C, (size_t)hw) && C % 8 == 0)) return false;
    // tile-sharded mode: the region-of-interest forms of both kernels take any region (ragged last step, 4-byte stores when the
    // region's rows are not 16-byte aligned); ST2_TILE_STYLE16=0 keeps the fp32 region-of-interest kernels
    if (c->tile.on) { const char* e = getenv("ST2_TILE_STYLE16"); return !(e && *e == '0'); }
    return hw % 64 == 0 && gram16_ok(C, hw, gram_plan16(C, hw));
}

// lean evaluation: does anything read blob b in fp32?  Content / deep-dream terms do (layer_elem_k); a style term only when
// its Gram / gradient cannot run on the bf16 copy.
bool blob_needs32(const st_ctx* c, const ActSet& a, int b)
{
    for (const ActiveLayer& al : c->active)
        if (al.blob == b && (al.c || al.d || (al.s && !style_runs16(c, a, b)))) return true;
    return false;
}

// May the style gradient of blob b ride on the data-gradient conv of the layer above it (conv3x3_mfma_bf16.hip, fused style term)?
bool style_fuse_ok(const st_ctx* c, const ActSet& a, int b, int last)
{
    const char* e = getenv("ST2_STYLE_FUSE");           // read per evaluation: the tests compare both flows in one process
    if ((e && *e == '0') || !style_runs16(c, a, b) || b + 1 > last || a.C[b] % 32 != 0) return false;
    const Layer& up = c->topo[b];                       // layer b + 1: consumes blob b
    return up.is_conv && up.loaded && conv16_ok(c, up.cout) && up.cin == a.C[b];
}

// `lean` (bf16 objective evaluations only): a conv blob whose only consumers are bf16 convs / a fused pool is not written
// in fp32 at all, and a pool that follows such a conv is computed in that conv's epilogue (bf16 pooled copy + arg-max map).
int forward_range(st_ctx* c, ActSet& a, const float* x, int last, bool lean)
{
    a.data[0] = const_cast<float*>(x);
    a.has32.assign(c->nb, 0); a.amap_ok.assign(c->nb, 0); a.bits_ok.assign(c->nb, 0);
    a.has32[0] = 1;
    const char* be = getenv("ST2_MASK_BITS");          // =0: the data gradients mask with the bf16 copies (read per forward: the tests compare both)
    const bool want_bits = lean && c->bf16 && !(be && *be == '0');
    int pooled_by_conv = -1;
    for (int i = 1; i <= last; ++i) {
        const Layer& L = c->topo[i - 1];
        if (L.is_conv) {
            if (!L.loaded) return fail(ST_ERR_STATE, "weights of %s were never loaded", L.name.c_str());
            const double px = (double)a.h[i] * a.w[i];
            // does the layer that consumes blob i run on the bf16 matrix cores?
            bool next16 = c->bf16 && i < last && c->topo[i].is_conv && conv16_ok(c, L.cout);
            const bool conv_next16 = next16;
            // ... or does the style gradient of this blob (bf16 path: style16.hip reads the bf16 copy)?
            if (c->bf16 && conv16_ok(c, L.cout) && style_grad16_ok(L.cout, (size_t)a.h[i] * a.w[i]))
                for (const ActiveLayer& al : c->active) if (al.blob == i && al.s) next16 = true;
            if (next16 && !a.data16[i]) ST_TRY(dmalloc16(&a.data16[i], act16_elems(a.C[i], (size_t)a.h[i] * a.w[i])));
            a.has32[i] = 1;
            // lean: the data gradient of the bf16 conv above masks with blob i -- through a sign map (1 bit per element, written by
            // this launch's epilogue) instead of the bf16 copy (16 bits)
            const bool bits_i = want_bits && conv_next16 && L.cout % 32 == 0;
            if (bits_i && !a.bits[i]) ST_TRY(dmalloc16(&a.bits[i], conv16_bits_elems(a.C[i], (size_t)a.h[i] * a.w[i])));
            if (c->bf16 && conv16_ok(c, L.cin) && a.data16[i - 1]) {
                Conv16Problem p{};
                p.in16 = a.data16[i - 1]; p.wpack16 = L.w16_fwd; p.bias = L.bias; p.out = a.data[i];
                p.out16 = next16 ? a.data16[i] : nullptr;
                p.K = L.cin; p.M = L.cout; p.MPad = conv_mpad(L.cout); p.H = a.h[i]; p.W = a.w[i]; p.relu = 1;
                double bytes = px * (2.0 * L.cin + 4.0 * L.cout + (next16 ? 2.0 * L.cout : 0.0));
                if (lean && !blob_needs32(c, a, i) && i < last) {
                    const bool next_pool = !c->topo[i].is_conv;
                    // (a weighted blob gets an injected diff: classic pool backward; an average pool always runs stand-alone on the fp32 blob)
                    if (next_pool && !c->topo[i].ave && !blob_active(c, i) && conv16_can_pool(p)) {
                        // the pool rides on this launch: pooled bf16 copy for the conv after it, arg-max map for the backward
                        const int pb = i + 1, pc = a.C[pb];
                        const size_t phw = (size_t)a.h[pb] * a.w[pb];
                        const bool pool_feeds16 = pb < last && c->topo[pb].is_conv && conv16_ok(c, pc);
                        if (pool_feeds16 && !a.data16[pb]) ST_TRY(dmalloc16(&a.data16[pb], act16_elems(pc, phw)));
                        if (!a.amap[pb]) HIP_TRY(hipMalloc((void**)&a.amap[pb], act16_elems(pc, phw)));
                        p.pool16 = pool_feeds16 ? a.data16[pb] : nullptr;
                        p.pool32 = (!pool_feeds16 || blob_active(c, pb) || pb == last) ? a.data[pb] : nullptr;
                        p.amap = a.amap[pb];
                        p.out = nullptr;
                        a.has32[i] = 0; a.has32[pb] = p.pool32 != nullptr; a.amap_ok[pb] = 1;
                        pooled_by_conv = pb;
                        bytes = px * (2.0 * L.cin + 0.25 * L.cout * (1.0 + (pool_feeds16 ? 2.0 : 0.0) + (p.pool32 ? 4.0 : 0.0)));
                    } else if (conv_next16) {
                        p.out = nullptr;                   // the next conv reads the bf16 copy; the backward masks with it too
                        a.has32[i] = 0;
                        bytes = px * (2.0 * L.cin + 2.0 * L.cout);
                    }
                }
                if (bits_i && p.out16) { p.bits_out = a.bits[i]; a.bits_ok[i] = 1; bytes += px * L.cout / 8.0; }
                ProfScope ps(c, P_CONV_FWD_BF16, 2.0 * 9 * L.cin * L.cout * px, bytes);
                HIP_TRY(launch_conv3x3_bf16(p, c->stream));
            } else {
                ConvProblem p{};
                bool packed = false;
                p.in = a.data[i - 1]; p.wpack = L.w_fwd; p.bias = L.bias; p.out = a.data[i];
                p.K = L.cin; p.M = L.cout; p.MPad = conv_mpad(L.cout); p.H = a.h[i]; p.W = a.w[i]; p.relu = 1;
                { const bool wino = c->wino && L.u_fwd && conv_wino_ok(p.K, p.M, p.H, p.W);
                  // st_set_conv_algo(ctx, 2): the same products as six bf16 partial products of split operands where the shape allows
                  const bool wsplit = wino && c->wino_split && !c->bf16 && L.us_fwd && conv_wino_split_ok(p.K, p.M, p.H, p.W);
                  // flops are the ALGORITHMIC (direct-convolution) count in every class; Winograd executes 4/9 of them (the split kernel 6 x 4/9 on the bf16 pipe)
                  ProfScope ps(c, wsplit ? P_CONV_FWD_WSPLIT : wino ? P_CONV_FWD_WINO : P_CONV_FWD, 2.0 * 9 * L.cin * L.cout * px, 4.0 * px * (L.cin + L.cout));
                  if (wino) {
                      p.wpack = wsplit ? reinterpret_cast<const float*>(L.us_fwd) : L.u_fwd; ST_TRY(wino_scratch(c, p, wsplit));
                      // the max-pool that follows rides on this launch's epilogue (the pooled blob is written beside the conv blob);
                      // an average pool does not (avepool_fwd reads the fp32 blob)
                      if (i < last && !c->topo[i].is_conv && !c->topo[i].ave && !c->bf16 && (wsplit ? conv_wino_split_can_pool(p.K, p.M, p.H, p.W) : conv_wino_can_pool(p.K, p.M, p.H, p.W))) {
                          p.pool_out = a.data[i + 1]; pooled_by_conv = i + 1; a.has32[i + 1] = 1;
                          // ... and a one-byte arg-max map for the pool's backward (maxpool_bwd_amap_k: neither blob is read again)
                          const char* ae = getenv("ST2_POOL_AMAP");          // =0: the classic pool backward (read per forward: the tests compare both)
                          if (!(ae && *ae == '0') && (wsplit ? conv_wino_split_pool_amap_ok(p.K, p.M, p.H, p.W) : conv_wino_pool_amap_ok(p.K, p.M, p.H, p.W))) {
                              // (sized like the bf16 path's map of the same blob: the buffer is shared when the precision is switched)
                              const size_t pn = act16_elems(a.C[i + 1], (size_t)a.h[i + 1] * a.w[i + 1]);
                              if (!a.amap[i + 1]) HIP_TRY(hipMalloc((void**)&a.amap[i + 1], pn));
                              p.pool_amap = a.amap[i + 1]; a.amap_ok[i + 1] = 2;      // 2: the fp32 layout [C][ph][pw]
                              // lean (inside an iteration): the full-resolution blob of a pooled, un-weighted layer is dead -- the next conv
                              // reads the pooled blob, the pool's backward the arg-max map (with the ReLU sign in it) -- so it is not
                              // written (conv1_2 at 1024^2: 268 MB and a quarter of the epilogue's instructions); same values everywhere else
                              if (lean && !c->bf16 && !blob_active(c, i) && (wsplit ? conv_wino_split_can_skip_out(p.K, p.M, p.H, p.W) : conv_wino_can_skip_out(p.K, p.M, p.H, p.W))) { p.out = nullptr; a.has32[i] = 0; }
                          }
                      }
                      if (wsplit) HIP_TRY(launch_conv3x3_wino_split(p, c->stream)); else
                      HIP_TRY(launch_conv3x3_wino(p, c->stream));
                  }
                  else { if (next16 && L.cout % 8 == 0) { p.out16 = a.data16[i]; packed = true; }      // the epilogue writes the bf16 copy too
                         // lean: conv1_1's fp32 blob is written only if something reads it (conv1_2, the ReLU mask and a style term take the copy)
                         if (lean && packed && conv_next16 && i < last && !blob_needs32(c, a, i)) { p.out = nullptr; a.has32[i] = 0; }
                         // bf16 path: the image keeps its fp32 precision (three-way bf16 split, six partial products on the bf16 matrix cores)
                         if (c->bf16 && L.w_split && conv_first_split_ok(p.K, p.M, p.H, p.W)) {
                             unsigned short* bits = (bits_i && p.out16) ? a.bits[i] : nullptr;
                             HIP_TRY(launch_conv3x3_first_split(p.in, L.w_split, p.out, p.out16, p.K, p.M, p.H, p.W, p.relu, c->stream, bits));
                             if (bits) a.bits_ok[i] = 1;
                         }
                         else HIP_TRY(launch_conv3x3(p, c->stream)); } }
                if (next16 && !packed) { ProfScope ps(c, P_MISC, 0, px * 6.0 * L.cout); HIP_TRY(launch_pack_act16(a.data[i], a.data16[i], a.C[i], (size_t)a.h[i] * a.w[i], c->stream)); }
            }
        } else if (i == pooled_by_conv) {
            // written by the producing conv's epilogue
        } else if (L.ave) {
            // average pool: stand-alone pass over the fp32 blob below, writing the fp32 pooled blob where something reads fp32
            // (lean rules: a weighted blob, the last blob, a consumer that is not a bf16 conv) and the bf16 copy a bf16 conv reads
            const int C = a.C[i - 1];
            const size_t hw = (size_t)a.h[i] * a.w[i];
            if (!a.has32[i - 1]) return fail(ST_ERR_STATE, "internal: the input blob of average pool %s is not materialised", L.name.c_str());
            const bool feeds16 = c->bf16 && i < last && c->topo[i].is_conv && conv16_ok(c, C);
            const bool want32 = !lean || !feeds16 || blob_active(c, i) || i == last;
            if (feeds16 && !a.data16[i]) ST_TRY(dmalloc16(&a.data16[i], act16_elems(C, hw)));
            a.has32[i] = want32;
            const double n_in = (double)C * a.h[i - 1] * a.w[i - 1];
            ProfScope ps(c, P_AVEPOOL_FWD, 0, 4.0 * n_in + (want32 ? 4.0 * C * hw : 0.0) + (feeds16 ? 2.0 * act16_elems(C, hw) : 0.0));
            HIP_TRY(launch_avepool_fwd(a.data[i - 1], want32 ? a.data[i] : nullptr, feeds16 ? a.data16[i] : nullptr, C, a.h[i - 1], a.w[i - 1], c->stream));
        } else {
            const double n_in = (double)a.C[i - 1] * a.h[i - 1] * a.w[i - 1];
            a.has32[i] = 1;
            { ProfScope ps(c, P_POOL_FWD, 0, 4.0 * n_in * 1.25);
              HIP_TRY(launch_maxpool_fwd(a.data[i - 1], a.data[i], a.C[i - 1], a.h[i - 1], a.w[i - 1], c->stream)); }
            if (c->bf16 && i < last && c->topo[i].is_conv && conv16_ok(c, a.C[i])) {
                const size_t hw = (size_t)a.h[i] * a.w[i];
                if (!a.data16[i]) ST_TRY(dmalloc16(&a.data16[i], act16_elems(a.C[i], hw)));
                ProfScope ps(c, P_MISC, 0, hw * 6.0 * a.C[i]);
                HIP_TRY(launch_pack_act16(a.data[i], a.data16[i], a.C[i], hw, c->stream));
            }
        }
    }
    a.valid_to = last;
    return ST_OK;
}

int ensure_gram_bufs(st_ctx* c, int C, int hw, GramPlan& pl, bool plan16)
{
    pl = plan16 ? gram_plan16(C, hw) : gram_plan(C, hw);
    if (pl.slab_floats > c->gram_slab_cap) {
        dfree(c->gram_slabs);
        ST_TRY(dmalloc(&c->gram_slabs, pl.slab_floats));
        c->gram_slab_cap = pl.slab_floats;
    }
    const size_t fold = (size_t)gram_fold_groups(pl) * C * C;
    if (fold > c->gram_fold_cap) {
        dfree(c->gram_fold);
        ST_TRY(dmalloc(&c->gram_fold, fold));
        c->gram_fold_cap = fold;
    }
    return ST_OK;
}

// G (or G - target) of blob data F -> out (C*C); optional sum-of-squares partials
// F16 (optional): the bf16 channel-blocked copy of the blob -- the bf16 feature path then takes the partials on the bf16 matrix cores
int gram_into(st_ctx* c, const float* F, int C, int hw, const float* target, float* out, int out_ld, float* partial, int* n_partial,
                     const unsigned short* F16)
{
    GramPlan pl;
    const bool use16 = F16 && C % 8 == 0 && hw % 64 == 0 && gram16_ok(C, hw, gram_plan16(C, hw));
    ST_TRY(ensure_gram_bufs(c, C, hw, pl, use16));
    {
        ProfScope ps(c, use16 ? P_GRAM_BF16 : P_GRAM, 2.0 * C * C * (double)hw, (use16 ? 2.0 : 4.0) * C * (double)hw);      // (the class names the matrix core that ran)
        if (use16) HIP_TRY(launch_gram16_partial(F16, c->gram_slabs, C, hw, pl, c->stream));
        else HIP_TRY(launch_gram_partial(F, c->gram_slabs, C, hw, pl, c->stream));
    }
    {
        ProfScope ps(c, P_GRAM_REDUCE, 0, 4.0 * (double)pl.slab_floats);
        HIP_TRY(launch_gram_reduce(c->gram_slabs, c->gram_fold, target, out, out_ld, partial, n_partial, C, (double)C * hw, pl, c->stream));
    }
    return ST_OK;
}

// backward chain from blob `top` whose diff is `cur` down to data; returns pointer in *out.
// `lean` must be what the forward that filled c->act ran with: the fp32 diff of a layer is then written only when its
// consumer needs fp32 (a pool without arg-max map, the 3-channel conv1_1 kernel, a non-bf16 conv), ReLU masks come from the
// bf16 copies, and pools fused into their producing conv are back-propagated through their arg-max maps in bf16.
int backward_chain(st_ctx* c, int top, const float* top_diff, const std::vector<const float*>& inj, const float** out, bool lean)
{
    const ActSet& a = c->act;
    const float* cur = top_diff;
    const unsigned short* cur16 = nullptr;             // bf16 copy of the running diff, when a producer already made it
    const unsigned char* pending_unpool = nullptr;     // arg-max map of the pool just passed: `cur` is still the POOLED diff (Winograd unpool)
    if (c->bf16 && !c->diff16A) {
        const size_t cap = c->max_blob + 8 * (size_t)a.h[0] * a.w[0];
        ST_TRY(dmalloc16(&c->diff16A, cap)); ST_TRY(dmalloc16(&c->diff16B, cap));
    }
    auto conv_takes16 = [&](int layer_index) {         // does conv layer `layer_index` (1-based blob index) read its diff as bf16?
        const Layer& P = c->topo[layer_index - 1];
        if (!P.is_conv || !conv16_ok(c, P.cout)) return false;
        const bool first_small = conv_dgrad_smallM_ok(P.cout, P.cin) && !(layer_index - 1 >= 1 && c->topo[layer_index - 2].is_conv);
        return !conv_dgrad_smallM_ok(P.cout, P.cin) || (first_small && P.w_raw_r != nullptr);
    };
    for (int i = top; i >= 1; --i) {
        const Layer& L = c->topo[i - 1];
        const int below = i - 1;
        float* dst = (cur == c->diffA) ? c->diffB : c->diffA;
        unsigned short* dst16 = (cur16 == c->diff16A) ? c->diff16B : c->diff16A;
        const bool below_is_conv = below >= 1 && c->topo[below - 1].is_conv;
        const float* mask_src = below_is_conv ? a.data[below] : nullptr;
        const float* inject = inj[below];
        if (L.is_conv) {
            const double px = (double)a.h[i] * a.w[i];
            const bool small_m = !mask_src && conv_dgrad_smallM_ok(L.cout, L.cin);
            if (small_m && pending_unpool) return fail(ST_ERR_STATE, "internal: an unpooling data gradient was planned for %s but the small-M kernel runs", L.name.c_str());
            const bool wino_bwd = !small_m && !(c->bf16 && conv16_ok(c, L.cout)) && c->wino && L.u_bwd && conv_wino_ok(L.cout, L.cin, a.h[i], a.w[i]);
            if (small_m && c->bf16 && L.w_raw_r) {
                // bf16 feature path: this conv's operands are bf16 too -- the diff arrives as (or is packed into) a bf16 copy
                const size_t hw = (size_t)a.h[i] * a.w[i];
                if (!cur16) {
                    if (!cur) return fail(ST_ERR_STATE, "internal: no diff above %s", L.name.c_str());
                    ProfScope ps(c, P_MISC, 0, hw * 6.0 * L.cout);
                    HIP_TRY(launch_pack_act16(cur, dst16, L.cout, hw, c->stream));
                    cur16 = dst16;
                }
                ProfScope ps(c, P_CONV_DGRAD, 2.0 * 9 * L.cin * L.cout * px, px * (2.0 * L.cout + 4.0 * L.cin));
                HIP_TRY(launch_conv3x3_dgrad_smallM16(cur16, L.w_raw_r, dst, inject, L.cout, L.cin, a.h[i], a.w[i], c->stream));
                cur16 = nullptr; cur = dst;
            } else if (small_m) {
                if (!cur) return fail(ST_ERR_STATE, "internal: fp32 diff missing above %s", L.name.c_str());
                ProfScope ps(c, P_CONV_DGRAD, 2.0 * 9 * L.cin * L.cout * px, 4.0 * px * (L.cin + L.cout));
                HIP_TRY(launch_conv3x3_dgrad_smallM(cur, L.w_raw, dst, inject, L.cout, L.cin, a.h[i], a.w[i], c->stream));
                cur16 = nullptr; cur = dst;
            } else if (c->bf16 && conv16_ok(c, L.cout)) {
                const size_t hw = (size_t)a.h[i] * a.w[i];
                if (!cur16) {                                      // top diff / classic pool-backward output: make the bf16 copy
                    if (!cur) return fail(ST_ERR_STATE, "internal: no diff above %s", L.name.c_str());
                    unsigned short* tmp16 = dst16;
                    ProfScope ps(c, P_MISC, 0, hw * 6.0 * L.cout);
                    HIP_TRY(launch_pack_act16(cur, tmp16, L.cout, hw, c->stream));
                    cur16 = tmp16;
                    dst16 = (cur16 == c->diff16A) ? c->diff16B : c->diff16A;
                }
                // the consumer of this launch's output takes bf16 iff it is a bf16 dgrad conv, or (lean) a pool with an arg-max map
                bool below16 = below >= 1 && conv_takes16(below);
                if (lean && below >= 1 && !c->topo[below - 1].is_conv && a.amap_ok[below] && L.cin % 8 == 0) below16 = true;
                Conv16Problem p{};
                p.in16 = cur16; p.wpack16 = L.w16_bwd; p.bias = nullptr; p.out = dst; p.out16 = below16 ? dst16 : nullptr;
                p.mask_src = mask_src; p.inject = inject;
                if (lean && mask_src && a.data16[below]) { p.mask16 = a.data16[below]; p.mask_src = nullptr; }
                const bool bits_below = lean && mask_src && a.bits_ok[below];
                const bool fused = below >= 1 && (size_t)below < c->sf_w.size() && c->sf_w[below] != nullptr;
                if (fused) {                // the style gradient of blob `below` rides on this launch: out = mask(conv) + D' @ F (+ inject)
                    p.s_in16 = c->sf_in[below]; p.s_wpack16 = c->sf_w[below];
                    if (mask_src) { p.mask16 = a.data16[below]; p.mask_src = nullptr; }      // the mask is applied in registers, from the bf16 copy
                }
                if (bits_below) { p.mask_bits = a.bits[below]; p.mask16 = nullptr; p.mask_src = nullptr; }      // ... or from the blob's sign map
                if (p.mask_src && !a.has32[below]) return fail(ST_ERR_STATE, "internal: mask blob %d missing", below);
                if (lean && below16) p.out = nullptr;
                p.K = L.cout; p.M = L.cin; p.MPad = conv_mpad(L.cin); p.H = a.h[i]; p.W = a.w[i]; p.relu = 0;
                p.unpool_amap = pending_unpool; pending_unpool = nullptr;      // cur16 is the POOLED diff then (3/4 byte per pooled channel value more, 1.5 less per full one)
                if (fused) prof_note(c, P_STYLE_FUSED_BF16, 2.0 * L.cin * L.cin * px);      // (extra K chunks of the launch below; its own flops stay SURVEY 8(d)'s)
                ProfScope ps(c, P_CONV_DGRAD_BF16, 2.0 * 9 * L.cin * L.cout * px,
                             px * ((p.unpool_amap ? 0.75 : 2.0) * L.cout + (fused ? 2.0 : 0.0) * L.cin + (p.out ? 4.0 : 0.0) * L.cin + (p.out16 ? 2.0 : 0.0) * L.cin + (mask_src ? (p.mask_bits ? 0.125 : p.mask16 ? 2.0 : 4.0) : 0.0) * L.cin));
                HIP_TRY(launch_conv3x3_bf16(p, c->stream));
                cur16 = below16 ? dst16 : nullptr;
                cur = p.out ? dst : nullptr;
            } else {
                if (!cur) return fail(ST_ERR_STATE, "internal: fp32 diff missing above %s", L.name.c_str());
                cur16 = nullptr;
                ConvProblem p{};
                p.in = cur; p.wpack = L.w_bwd; p.bias = nullptr; p.out = dst;
                p.mask_src = mask_src; p.inject = inject;
                p.K = L.cout; p.M = L.cin; p.MPad = conv_mpad(L.cin); p.H = a.h[i]; p.W = a.w[i]; p.relu = 0;
                if (pending_unpool && !wino_bwd) return fail(ST_ERR_STATE, "internal: an unpooling data gradient was planned for %s but the direct kernel runs", L.name.c_str());
                p.unpool_amap = pending_unpool; pending_unpool = nullptr;
                const bool wsplit = wino_bwd && dgrad_takes_split(c, L, a.h[i], a.w[i]);
                if (wsplit && p.unpool_amap) return fail(ST_ERR_STATE, "internal: an unpooling data gradient was planned for %s but the split-operand kernel runs", L.name.c_str());
                ProfScope ps(c, wsplit ? P_CONV_DGRAD_WSPLIT : wino_bwd ? P_CONV_DGRAD_WINO : P_CONV_DGRAD, 2.0 * 9 * L.cin * L.cout * px,
                             4.0 * px * (L.cin + (p.unpool_amap ? 0.3125 : 1.0) * L.cout));
                if (wsplit) { p.wpack = reinterpret_cast<const float*>(L.us_bwd); ST_TRY(wino_scratch(c, p, true)); HIP_TRY(launch_conv3x3_wino_split(p, c->stream)); }
                else if (wino_bwd) { p.wpack = L.u_bwd; ST_TRY(wino_scratch(c, p, false)); HIP_TRY(launch_conv3x3_wino(p, c->stream)); }
                else HIP_TRY(launch_conv3x3(p, c->stream));
                cur = dst;
            }
        } else if (L.ave) {
            // average pool: dx = mask(dy / window size) + inject in one pass; the bf16 copy for a bf16 dgrad conv below comes out of
            // the same pass (no pack_act16), the fp32 diff where the consumer below reads fp32 (or every diff is materialised)
            if (!cur) return fail(ST_ERR_STATE, "internal: fp32 diff missing above %s", L.name.c_str());
            if (mask_src && !a.has32[below]) return fail(ST_ERR_STATE, "internal: pool input blob %d missing", below);
            const bool to16 = c->bf16 && below >= 1 && conv_takes16(below);
            const bool to32 = !(lean && to16);
            const double n_in = (double)a.C[below] * a.h[below] * a.w[below];
            ProfScope ps(c, P_AVEPOOL_BWD, 0, 4.0 * (double)a.C[below] * a.h[i] * a.w[i] +
                         n_in * (4.0 * ((mask_src ? 1 : 0) + (inject ? 1 : 0) + (to32 ? 1 : 0)) + (to16 ? 2.0 : 0.0)));
            HIP_TRY(launch_avepool_bwd(cur, mask_src, inject, to32 ? dst : nullptr, to16 ? dst16 : nullptr, a.C[below], a.h[below], a.w[below], c->stream));
            cur16 = to16 ? dst16 : nullptr;
            cur = to32 ? dst : nullptr;
        } else if (lean && a.amap_ok[i] && !inject && below >= 1 && conv_takes16(below)) {
            // pool fused into its producing conv: route the bf16 diff through the arg-max map (ReLU mask of the conv blob included)
            const int C = a.C[below];
            const size_t hw_top = (size_t)a.h[i] * a.w[i], hw = (size_t)a.h[below] * a.w[below];
            if (!cur16) {
                if (!cur) return fail(ST_ERR_STATE, "internal: no diff above %s", L.name.c_str());
                unsigned short* tmp16 = dst16;
                ProfScope ps(c, P_MISC, 0, hw_top * 6.0 * C);
                HIP_TRY(launch_pack_act16(cur, tmp16, C, hw_top, c->stream));
                cur16 = tmp16;
                dst16 = (cur16 == c->diff16A) ? c->diff16B : c->diff16A;
            }
            {   // ... inside the data gradient of the conv below when it has the build (conv16_body, UNPOOL): it stages the pooled diff and
                // expands it in LDS through the map (maxpool_bwd_idx16_k, its full-resolution output and the conv's read of it are gone)
                const Layer& P = c->topo[below - 1];
                Conv16Problem q{};
                q.K = P.cout; q.M = P.cin; q.MPad = conv_mpad(P.cin); q.H = a.h[below]; q.W = a.w[below];
                if (conv16_ok(c, P.cout) && !conv_dgrad_smallM_ok(P.cout, P.cin) && conv16_can_unpool(q)) { pending_unpool = a.amap[i]; continue; }
            }
            ProfScope ps(c, P_POOL_BWD, 0, (double)C * (hw_top * 3.0 + hw * 2.0));
            HIP_TRY(launch_maxpool_bwd_idx16(cur16, a.amap[i], dst16, C, a.h[below], a.w[below], c->stream));
            cur16 = dst16; cur = nullptr;
        } else if (a.amap_ok[i] == 2 && !inject && mask_src && cur) {
            // pool fused into its producing Winograd conv (fp32): route the diff through the arg-max map, ReLU mask included ...
            const Layer& P = c->topo[below - 1];             // the conv that produced the pooled-from blob: its data gradient runs next
            const bool p_wino = !c->bf16 && c->wino && P.u_bwd && !(below - 1 < 1 && conv_dgrad_smallM_ok(P.cout, P.cin)) &&
                                conv_wino_ok(P.cout, P.cin, a.h[below], a.w[below]);
            // (the split-operand kernel has no unpooling input transform: its launches keep maxpool_bwd_amap_k)
            if (p_wino && !dgrad_takes_split(c, P, a.h[below], a.w[below]) && conv_wino_can_unpool(P.cout, P.cin, a.h[below], a.w[below])) {
                // ... inside that data gradient: it stages the pooled diff and the map and unpools in its input transform
                // (maxpool_bwd_amap_k, its full-resolution output and the conv's read of it are gone; same values bit for bit)
                pending_unpool = a.amap[i];
                continue;
            }
            ProfScope ps(c, P_POOL_BWD, 0, (double)a.C[below] * ((double)a.h[i] * a.w[i] * 5.0 + (double)a.h[below] * a.w[below] * 4.0));
            HIP_TRY(launch_maxpool_bwd_amap(cur, a.amap[i], dst, a.C[below], a.h[below], a.w[below], c->stream));
            cur16 = nullptr; cur = dst;
        } else {
            if (!cur) return fail(ST_ERR_STATE, "internal: fp32 diff missing above %s", L.name.c_str());
            if (!a.has32[below]) return fail(ST_ERR_STATE, "internal: pool input blob %d missing", below);
            const double n_in = (double)a.C[below] * a.h[below] * a.w[below];
            ProfScope ps(c, P_POOL_BWD, 0, 4.0 * n_in * 2.25);
            HIP_TRY(launch_maxpool_bwd(cur, a.data[below], dst, inject, mask_src != nullptr, a.C[below], a.h[below], a.w[below], c->stream));
            cur16 = nullptr; cur = dst;
        }
    }
    if (pending_unpool) return fail(ST_ERR_STATE, "internal: a pooled diff was left un-expanded");
    if (!cur) return fail(ST_ERR_STATE, "internal: the backward chain ended without an fp32 image gradient");
    *out = cur;
    return ST_OK;
}

int ensure_input_buffers(st_ctx* c, int H, int W)
{
    if (c->H == H && c->W == W && c->x[0]) return ST_OK;
    const size_t n3 = (size_t)3 * H * W;
    for (int i = 0; i < 2; ++i) { dfree(c->x[i]); ST_TRY(dmalloc(&c->x[i], n3)); }
    dfree(c->grad); ST_TRY(dmalloc(&c->grad, n3));
    dfree(c->m); dfree(c->v);
    ST_TRY(dmalloc(&c->m, n3)); ST_TRY(dmalloc(&c->v, n3));
    dfree(c->g_cur); dfree(c->pvec);
    for (int i = 0; i <= st_ctx::kCorr; ++i) { dfree(c->hs[i]); dfree(c->hy[i]); }
    dfree(c->hwc_dev); ST_TRY(dmalloc(&c->hwc_dev, n3));
    c->H = H; c->W = W; c->cur = 0;
    // work buffers that follow the input geometry
    for (auto& p : c->inject) dfree(p);
    std::fill(c->inject_roi_zero.begin(), c->inject_roi_zero.end(), 0);
    dfree(c->diffA); dfree(c->diffB); dfree(c->stmp); dfree16(c->diff16A); dfree16(c->diff16B);
    std::vector<int> C, h, w;
    shapes_for(c, H, W, C, h, w);
    c->max_blob = 0;
    for (int i = 0; i < c->nb; ++i) c->max_blob = std::max(c->max_blob, (size_t)C[i] * h[i] * w[i]);
    return ST_OK;
}

int stage_upload(st_ctx* c, const void* host, size_t bytes)
{
    if (bytes > c->stage_cap) {
        if (c->stage_dev) (void)hipFree(c->stage_dev);
        c->stage_dev = nullptr;
        HIP_TRY(hipMalloc(&c->stage_dev, bytes));
        c->stage_cap = bytes;
    }
    HIP_TRY(hipMemcpyAsync(c->stage_dev, host, bytes, hipMemcpyHostToDevice, c->stream));
    return ST_OK;
}

int preprocess_into(st_ctx* c, const void* hwc, int H, int W, int is_u8, float* dst)
{
    if (!hwc || H <= 0 || W <= 0) return fail(ST_ERR_ARG, "bad image (%p, %d x %d)", hwc, H, W);
    const size_t n = (size_t)H * W * 3;
    ST_TRY(stage_upload(c, hwc, n * (is_u8 ? 1 : 4)));
    ProfScope ps(c, P_MISC, 0, 0);
    if (is_u8) HIP_TRY(launch_preprocess_u8((const uint8_t*)c->stage_dev, dst, H, W, c->stream));
    else HIP_TRY(launch_preprocess_f32((const float*)c->stage_dev, dst, H, W, c->stream));
    return ST_OK;
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
        if (!used[i]) { dfree(c->content_feat[i]); continue; }
        const size_t n = (size_t)c->act.C[i] * c->act.h[i] * c->act.w[i];
        if (c->cH != H || c->cW != W || !c->content_feat[i]) { dfree(c->content_feat[i]); ST_TRY(dmalloc(&c->content_feat[i], n)); }
        HIP_TRY(hipMemcpyAsync(c->content_feat[i], i == 0 ? xdev : c->act.data[i], n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    }
    c->act.valid_to = -1;
    if (xdev != c->content_x) {                 // keep the preprocessed image itself (== blob "data")
        if (c->cH != H || c->cW != W || !c->content_x) { dfree(c->content_x); ST_TRY(dmalloc(&c->content_x, (size_t)3 * H * W)); }
        HIP_TRY(hipMemcpyAsync(c->content_x, xdev, (size_t)3 * H * W * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    }
    c->cH = H; c->cW = W;
    c->have_content = true;
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
        ST_TRY(dmalloc(&c->content_feat[b], n));
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
    st_ctx* c = new st_ctx();
    c->device = device_id;
    { const char* e = getenv("ST2_WINO"); if (e && *e) c->wino = atoi(e) != 0; }
    { const char* e = getenv("ST2_GRAPH"); if (e && *e) c->graphs = atoi(e) != 0; }
    { const char* e = getenv("ST2_GRAPH_MAX_PX"); if (e && *e) c->graph_max_px = (size_t)atoll(e) * (size_t)atoll(e); }
    if (n_layers <= 0) {
        for (const auto& l : kVgg19) {
            Layer L; L.is_conv = l.kind == 0; L.name = l.name; L.cin = l.cin; L.cout = l.cout;
            c->topo.push_back(L);
        }
    } else {
        int cprev = 3;
        for (int i = 0; i < n_layers; ++i) {
            const int kind = layers[i].kind;
            if (kind != ST_LAYER_CONV && kind != ST_LAYER_POOL && kind != ST_LAYER_AVEPOOL) {
                delete c; return fail(ST_ERR_ARG, "layer %d (%s): unknown kind %d", i, layers[i].name ? layers[i].name : "", kind);
            }
            Layer L; L.is_conv = kind == ST_LAYER_CONV; L.ave = kind == ST_LAYER_AVEPOOL; L.name = layers[i].name ? layers[i].name : "";
            if (L.is_conv) {
                L.cin = layers[i].cin; L.cout = layers[i].cout;
                if (L.cin != cprev || L.cout <= 0) { delete c; return fail(ST_ERR_ARG, "layer %s: cin %d does not follow %d", L.name.c_str(), L.cin, cprev); }
                cprev = L.cout;
            }
            c->topo.push_back(L);
        }
    }
    if ((int)c->topo.size() + 1 > kMaxTraceLayers) { delete c; return fail(ST_ERR_ARG, "too many layers"); }
    c->blob_names.push_back("data");
    for (const Layer& L : c->topo) c->blob_names.push_back(L.name);
    c->nb = (int)c->blob_names.size();
    HIP_TRY(hipStreamCreate(&c->stream));
    c->content_feat.assign(c->nb, nullptr);
    c->style_gram.assign(c->nb, nullptr);
    c->inject.assign(c->nb, nullptr);
    c->inject_roi_zero.assign(c->nb, 0);
    c->layer_part.assign(c->nb, nullptr);
    c->s2_part.assign(c->nb, nullptr);
    c->sfuse_w.assign(c->nb, nullptr); c->sfuse_cap.assign(c->nb, 0);
    c->s2_cap.assign(c->nb, 0);
    c->cnt.assign(c->nb * 6, 0);
    c->norm_valid.assign(c->nb * 3, 0);
    ST_TRY(dmalloc(&c->norms, c->nb * 3));
    ST_TRY(dmalloc(&c->image_part, 6 * kMaxPartials));
    ST_TRY(dmalloc(&c->trace_dev, kMaxTraceLayers * 6 + 8));
    HIP_TRY(hipMalloc((void**)&c->trace_sums, (kMaxTraceLayers * kLayerSlots + kImageSlots) * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&c->lb_dev, sizeof(LbfgsDev)));
    HIP_TRY(hipMemset(c->lb_dev, 0, sizeof(LbfgsDev)));
    ST_TRY(dmalloc(&c->lb_part, 4 * kMaxPartials));
    HIP_TRY(hipHostMalloc((void**)&c->trace_host, (kMaxTraceLayers * 6 + 8) * sizeof(float), 0));
    // worker.py:129-133: all-ones weights over every blob until SetWeights arrives
    for (int b = 0; b < c->nb; ++b) c->rows.push_back(ActiveLayer{b, 1.f, 1.f, 1.f, true, true, true});
    c->active = c->rows;
    *out = c;
    return ST_OK;
}

int st_destroy(st_ctx* c)
{
    if (!c) return ST_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (int i = 0; i < 2; ++i) if (c->gexec[i]) { (void)hipGraphExecDestroy(c->gexec[i]); c->gexec[i] = nullptr; }
    dfree(c->adam_dyn);
    for (Layer& L : c->topo) { dfree(L.w_fwd); dfree(L.w_bwd); dfree(L.w_raw); dfree(L.w_raw_r); dfree(L.bias); dfree16(L.w16_fwd); dfree16(L.w16_bwd); dfree16(L.w_split); dfree(L.u_fwd); dfree(L.u_bwd); dfree16(L.us_fwd); dfree16(L.us_bwd); }
    dfree16(c->diff16A); dfree16(c->diff16B);
    act_free(c->act);
    for (int i = 0; i < 2; ++i) dfree(c->x[i]);
    dfree(c->fwd_x);
    dfree(c->grad); dfree(c->m); dfree(c->v); dfree(c->g_cur); dfree(c->pvec);
    for (int i = 0; i <= st_ctx::kCorr; ++i) { dfree(c->hs[i]); dfree(c->hy[i]); }
    for (auto& p : c->content_feat) dfree(p);
    dfree(c->content_x);
    for (auto& p : c->style_gram) dfree(p);
    for (auto& p : c->inject) dfree(p);
    for (auto& p : c->layer_part) dfree(p);
    for (auto& p : c->s2_part) dfree(p);
    for (auto& p : c->sfuse_w) dfree16(p);
    dfree(c->diffA); dfree(c->diffB); dfree(c->stmp); dfree(c->gram_slabs); dfree(c->gram_fold); dfree(c->dbuf); dfree16(c->d16); dfree(c->conv_scratch);
    comm_free(c);
    dfree(c->tile.p1); dfree(c->tile.p2); dfree(c->tile.p3); dfree(c->tile.pd); dfree(c->tile.wgrad); dfree(c->tile.lb_x); dfree(c->tile.lb_sums);
    dfree(c->norms); dfree(c->image_part); dfree(c->trace_dev); dfree(c->lb_part); dfree(c->hwc_dev);
    if (c->lb_dev) (void)hipFree(c->lb_dev);
    if (c->lb_gram) (void)hipFree(c->lb_gram);
    dfree(c->lb_gpart); dfree(c->lb_dots);
    if (c->stage_dev) (void)hipFree(c->stage_dev);
    if (c->trace_sums) (void)hipFree(c->trace_sums);
    if (c->trace_host) (void)hipHostFree(c->trace_host);
    if (c->pipe.copy) {
        (void)hipStreamSynchronize(c->pipe.copy);
        for (int i = 0; i < st_ctx::Pipe::kSlots; ++i) {
            dfree(c->pipe.hwc[i]);
            if (c->pipe.pin_base[i]) (void)hipHostFree(c->pipe.pin_base[i]);
            if (c->pipe.trace_pin[i]) (void)hipHostFree(c->pipe.trace_pin[i]);
            if (c->pipe.ready[i]) (void)hipEventDestroy(c->pipe.ready[i]);
            if (c->pipe.done[i]) (void)hipEventDestroy(c->pipe.done[i]);
        }
        for (auto& r : c->pipe.retired) (void)hipHostFree(r.p);
        (void)hipStreamDestroy(c->pipe.copy);
    }
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(c->stream);
    delete c;
    return ST_OK;
}

// the split-operand Winograd packs of one conv layer (both directions where the kernel can take them); w = (Cout, Cin, 3, 3) on the host
static int make_split_packs(Layer& L, const float* w)
{
    for (int dir = 0; dir < 2; ++dir) {
        const int K = dir ? L.cout : L.cin, M = dir ? L.cin : L.cout;
        unsigned short** dst = dir ? &L.us_bwd : &L.us_fwd;
        if (*dst || !conv_wino_split_ok(K, M, 4, 4)) continue;
        std::vector<unsigned short> hu(wino_split_pack_elems(K, M), 0);
        if (dir) pack_wino_split_weights_dgrad(w, L.cout, L.cin, hu.data()); else pack_wino_split_weights_fwd(w, L.cout, L.cin, hu.data());
        ST_TRY(dmalloc16(dst, hu.size()));
        HIP_TRY(hipMemcpy(*dst, hu.data(), hu.size() * 2, hipMemcpyHostToDevice));
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
        dfree(L.w_fwd); dfree(L.w_bwd); dfree(L.w_raw); dfree(L.w_raw_r); dfree(L.bias); dfree16(L.w16_fwd); dfree16(L.w16_bwd); dfree16(L.w_split); dfree(L.u_fwd); dfree(L.u_bwd); dfree16(L.us_fwd); dfree16(L.us_bwd);
        for (int dir = 0; dir < 2; ++dir) {   // Winograd packs for the directions the Winograd kernel can take (any image size)
            const int K = dir ? L.cout : L.cin, M = dir ? L.cin : L.cout;
            if (!conv_wino_ok(K, M, 4, 4)) continue;
            std::vector<float> hu(wino_pack_floats(K, M));
            if (dir) pack_wino_weights_dgrad(w, L.cout, L.cin, hu.data()); else pack_wino_weights_fwd(w, L.cout, L.cin, hu.data());
            float** dst = dir ? &L.u_bwd : &L.u_fwd;
            ST_TRY(dmalloc(dst, hu.size()));
            HIP_TRY(hipMemcpy(*dst, hu.data(), hu.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        {   // bf16 packs for the bf16 feature path
            const size_t n16f = conv16_pack_elems(L.cin, L.cout), n16b = conv16_pack_elems(L.cout, L.cin);
            std::vector<unsigned short> hf(n16f), hb(n16b);
            pack_conv_weights16_fwd(w, L.cout, L.cin, hf.data());
            pack_conv_weights16_dgrad(w, L.cout, L.cin, hb.data());
            ST_TRY(dmalloc16(&L.w16_fwd, n16f)); ST_TRY(dmalloc16(&L.w16_bwd, n16b));
            HIP_TRY(hipMemcpy(L.w16_fwd, hf.data(), n16f * 2, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(L.w16_bwd, hb.data(), n16b * 2, hipMemcpyHostToDevice));
        }
        if (L.cin == 3 && L.cout % 32 == 0) {   // first layer on the bf16 path: split weights for conv3x3_first_split.hip
            std::vector<unsigned short> hs(conv_first_split_pack_elems(L.cout));
            pack_conv_first_split(w, bias, L.cout, L.cin, hs.data());
            ST_TRY(dmalloc16(&L.w_split, hs.size()));
            HIP_TRY(hipMemcpy(L.w_split, hs.data(), hs.size() * 2, hipMemcpyHostToDevice));
        }
        ST_TRY(dmalloc(&L.w_fwd, nf)); ST_TRY(dmalloc(&L.w_bwd, nb));
        ST_TRY(dmalloc(&L.w_raw, (size_t)L.cout * L.cin * 9)); ST_TRY(dmalloc(&L.bias, bp.size()));
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
            ST_TRY(dmalloc(&L.w_raw_r, wr.size()));
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

int st_set_precision(st_ctx* c, int bf16_features)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    c->bf16 = bf16_features != 0;
    // 1: the lean data flow (objective evaluations write fp32 only where something reads fp32); 2: every fp32 blob and diff
    // as in round 1 (A/B reference of the tests); environment ST2_BF16_LEAN=0 forces 2
    const char* e = getenv("ST2_BF16_LEAN");
    c->lean = bf16_features == 1 && !(e && *e == '0');
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
    if (n3 > c->fwd_x_cap) { dfree(c->fwd_x); c->fwd_x_cap = 0; ST_TRY(dmalloc(&c->fwd_x, n3)); c->fwd_x_cap = n3; }
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
    if (!c->act.has32[index]) return fail(ST_ERR_STATE, "blob %d (%s) is not materialised in fp32 by the lean evaluation of an iteration (st_opfunc / st_forward write every fp32 blob; bf16: st_set_precision(ctx, 2))", index, c->blob_names[index].c_str());
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
        if (!c->inject[b]) ST_TRY(dmalloc(&c->inject[b], nb));
        HIP_TRY(hipMemcpyAsync(c->inject[b], diffs[i], nb * sizeof(float), hipMemcpyHostToDevice, c->stream));
        c->inject_roi_zero[b] = 0;
        inj[b] = c->inject[b];
        top = std::max(top, b);
    }
    if (top < 0) { memset(out_grad, 0, n3 * sizeof(float)); return ST_OK; }
    if (!c->diffA) { ST_TRY(dmalloc(&c->diffA, c->max_blob)); ST_TRY(dmalloc(&c->diffB, c->max_blob)); }
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
    HIP_TRY(hipSetDevice(c->device));
    const int C = c->act.C[index], hw = c->act.h[index] * c->act.w[index];
    float* g = nullptr;
    ST_TRY(dmalloc(&g, (size_t)C * C));
    int r = gram_into(c, c->act.data[index], C, hw, nullptr, g, C, nullptr, nullptr);
    if (r == ST_OK) {
        hipError_t e = hipMemcpyAsync(out, g, (size_t)C * C * sizeof(float), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) r = fail(ST_ERR_HIP, "gram copy: %s", hipGetErrorString(e));
    }
    dfree(g);
    return r;
}

// ---- image slots
int st_set_input(st_ctx* c, const void* hwc, int H, int W, int is_u8)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    ST_TRY(set_input_common(c, H, W));
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
    float* tmp = nullptr;
    ST_TRY(dmalloc(&tmp, (size_t)3 * H * W));
    int r = preprocess_into(c, hwc, H, W, is_u8, tmp);
    if (r == ST_OK) r = content_from_device(c, tmp, H, W);
    (void)hipStreamSynchronize(c->stream);
    dfree(tmp);
    return r;
}

int st_set_content_nchw(st_ctx* c, const float* x, int H, int W)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c || !x || H <= 0 || W <= 0) return fail(ST_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    float* tmp = nullptr;
    ST_TRY(dmalloc(&tmp, (size_t)3 * H * W));
    int r = ST_OK;
    if (hipMemcpy(tmp, x, (size_t)3 * H * W * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) r = fail(ST_ERR_HIP, "content upload failed");
    if (r == ST_OK) r = content_from_device(c, tmp, H, W);
    (void)hipStreamSynchronize(c->stream);
    dfree(tmp);
    return r;
}

int st_set_style(st_ctx* c, const void* hwc, int H, int W, int is_u8)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    float* tmp = nullptr;
    ST_TRY(dmalloc(&tmp, (size_t)3 * H * W));
    ActSet aux;
    ActSet* a = &aux;
    const bool same = c->act.H == H && c->act.W == W && !c->act.data.empty();
    if (same) a = &c->act;
    int r = preprocess_into(c, hwc, H, W, is_u8, tmp);
    if (r == ST_OK) r = act_ensure(c, *a, H, W);
    if (r == ST_OK) r = forward_range(c, *a, tmp, c->nb - 1);
    for (int i = 0; i < c->nb && r == ST_OK; ++i) {
        const int C = a->C[i], hw = a->h[i] * a->w[i];
        if (!c->style_gram[i]) r = dmalloc(&c->style_gram[i], (size_t)C * C);
        if (r == ST_OK) r = gram_into(c, a->data[i], C, hw, nullptr, c->style_gram[i], C, nullptr, nullptr);
    }
    (void)hipStreamSynchronize(c->stream);
    if (!same) act_free(aux);
    else c->act.valid_to = -1;
    dfree(tmp);
    if (r == ST_OK) c->have_style = true;
    return r;
}

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

}  // extern "C"
