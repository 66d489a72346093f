// The route plan: which kernel every layer of one evaluation runs, what it writes and what it reads, decided once before the
// first launch.  forward_range / backward_chain (engine.cpp) execute the plan; nothing here touches the device or the context.
#include "engine.h"

namespace st2e {
bool lean32_enabled() { return !env_off("ST2_LEAN32"); }

static bool blob_active(const st_ctx* c, int b)
{
    for (const ActiveLayer& al : c->active) if (al.blob == b) return true;
    return false;
}

// lean evaluation: does anything read blob b in fp32?  Content / deep-dream terms do (layer_elem_k); a style term only when
// its Gram / gradient cannot both run on the bf16 copy (sty: style_shape of the style blobs).
static bool blob_needs32(const st_ctx* c, const std::vector<StyleShape>& sty, int b)
{
    for (const ActiveLayer& al : c->active)
        if (al.blob == b && (al.c || al.d || (al.s && !sty[b].gram16))) return true;
    return false;
}

// does the layer that consumes blob i run on the bf16 matrix cores?
static bool feeds_conv16(const st_ctx* c, const ActSet& a, int i, int last)
{
    return c->bf16 && i < last && c->topo[i].is_conv && conv16_ok(c, a.C[i]);
}

static Conv16Problem shape16(int K, int M, int H, int W)
{
    Conv16Problem p{};
    p.K = K; p.M = M; p.MPad = conv_mpad(M); p.H = H; p.W = W;
    return p;
}

// The Winograd launch of a conv of this shape, resolved once: the fp32 kernel where it has its pack and takes the shape (else
// w.ok is false), and in its place the split-operand kernel (st_set_conv_algo(ctx, 2): the same products as six bf16 partial
// products of split operands) where that one does too
struct WinoChoice { WinoLaunch w; bool split; };
static WinoChoice wino_choice(const st_ctx* c, const float* pack, const unsigned short* split_pack, int K, int M, int H, int W)
{
    WinoChoice ch{};
    if (!c->wino || !pack) return ch;
    ch.w = wino_resolve(K, M, H, W);
    if (ch.w.ok && c->wino_split && !c->bf16 && split_pack)
        if (const WinoLaunch ws = wino_split_resolve(K, M, H, W); ws.ok) { ch.w = ws; ch.split = true; }
    return ch;
}

namespace {
struct Dgrad;
Dgrad dgrad_route(const st_ctx* c, const ActSet& a, int i);
}
static bool ave_pool_fuse_ok(const st_ctx* c, const ActSet& a, int i);

// ------------------------------------------------------------------------------------------ forward
// `lean`: a conv blob whose only consumers are bf16 convs / a fused pool is not written in fp32 at all, a pool that follows such a
// conv is computed in that conv's epilogue (bf16 pooled copy + arg-max map; an average pool under st_set_pool_algo(ctx, 1): + sign map); fp32 (inside an iteration): the full-resolution blob
// of a pooled, un-weighted layer is not written when the Winograd epilogue pools it and writes the arg-max map.
void plan_forward(const st_ctx* c, const ActSet& a, int last, bool lean, std::vector<FwdRoute>& fwd)
{
    fwd.assign(c->nb, FwdRoute{});
    fwd[0].out32 = true;
    // ST2_MASK_BITS=0: the data gradients mask with the bf16 copies; ST2_POOL_AMAP=0: the classic pool backward
    // (both read per forward: the tests compare both)
    const bool want_bits = lean && c->bf16 && !env_off("ST2_MASK_BITS");
    const bool want_amap = !env_off("ST2_POOL_AMAP");
    // the style terms of this evaluation, from shapes alone: the forward (which may then skip an fp32 blob) and the objective agree
    std::vector<StyleShape> sty(c->nb, StyleShape{});
    for (const ActiveLayer& al : c->active) if (al.s) sty[al.blob] = style_shape(c, a, al.blob);
    for (int i = 1; i <= last; ++i) {
        const Layer& L = c->topo[i - 1];
        FwdRoute& r = fwd[i];
        const int H = a.h[i], W = a.w[i];
        if (!L.is_conv) {
            if (r.kind == F_BY_CONV_BELOW) continue;       // (filled in by the conv's entry)
            const bool to16 = feeds_conv16(c, a, i, last);
            if (L.ave) {
                // stand-alone pass over the fp32 blob below: the fp32 pooled blob where something reads fp32 (lean rules: a weighted
                // blob, the last blob, a consumer that is not a bf16 conv), the bf16 copy a bf16 conv reads from the same pass
                r.kind = F_AVEPOOL;
                r.out16 = to16;
                r.out32 = !lean || !to16 || blob_active(c, i) || i == last;
            } else {
                r.kind = F_MAXPOOL;
                r.out32 = true;
                r.out16 = r.pack16 = to16;
            }
            continue;
        }
        const bool conv_next16 = feeds_conv16(c, a, i, last);
        // ... or does the style gradient of this blob read the bf16 copy (style16.hip)?
        const bool next16 = conv_next16 || sty[i].grad16;
        // lean: the data gradient of the bf16 conv above masks with blob i -- through a sign map (1 bit per element, written by
        // this launch's epilogue) instead of the bf16 copy (16 bits)
        const bool bits_i = want_bits && conv_next16 && L.cout % 32 == 0;
        const bool next_max_pool = i < last && !c->topo[i].is_conv && !c->topo[i].ave;
        const bool next_ave_pool = i < last && !c->topo[i].is_conv && c->topo[i].ave;
        r.out32 = true;
        if (c->bf16 && conv16_ok(c, L.cin) && fwd[i - 1].out16) {
            r.kind = F_CONV16;
            r.out16 = next16;
            if (lean && !blob_needs32(c, sty, i) && i < last) {
                // (a weighted blob gets an injected diff: classic pool backward; an average pool runs stand-alone on the fp32 blob
                // unless st_set_pool_algo(ctx, 1) and its backward can go through the sign map: ave_pool_fuse_ok)
                if ((next_max_pool || (next_ave_pool && ave_pool_fuse_ok(c, a, i))) && !blob_active(c, i) && conv16_resolve(shape16(L.cin, L.cout, H, W)).can_pool) {
                    // the pool rides on this launch: pooled bf16 copy for the conv after it, arg-max / sign map for the backward
                    FwdRoute& pool = fwd[i + 1];
                    pool.kind = F_BY_CONV_BELOW;
                    pool.out16 = feeds_conv16(c, a, i + 1, last);
                    pool.out32 = !pool.out16 || blob_active(c, i + 1) || i + 1 == last;
                    pool.amap = next_ave_pool ? AMAP_BLOCKED16_AVE : AMAP_BLOCKED16;
                    r.pools_next = true;
                    r.out32 = false;
                } else if (conv_next16) {
                    r.out32 = false;                       // the next conv reads the bf16 copy; the backward masks with it too
                }
            }
            r.bits = bits_i && r.out16;
        } else if (const WinoChoice ch = wino_choice(c, L.u_fwd, L.us_fwd, L.cin, L.cout, H, W); ch.w.ok) {
            const WinoLaunch& w = ch.w;
            r.kind = ch.split ? F_WINO_SPLIT : F_WINO;
            r.out16 = r.pack16 = next16;
            // the max pool that follows rides on this launch's epilogue (the pooled blob is written beside the conv blob);
            // an average pool does not (avepool_fwd reads the fp32 blob)
            if (next_max_pool && !c->bf16 && w.can_pool) {
                FwdRoute& pool = fwd[i + 1];
                pool.kind = F_BY_CONV_BELOW;
                pool.out32 = true;
                r.pools_next = true;
                // ... and a one-byte arg-max map for the pool's backward (maxpool_bwd_amap_k: neither blob is read again)
                if (want_amap && w.pool_amap) {
                    pool.amap = AMAP_PLANAR32;
                    // lean (inside an iteration): the full-resolution blob of a pooled, un-weighted layer is dead -- the next conv
                    // reads the pooled blob, the pool's backward the arg-max map (with the ReLU sign in it) -- so it is not
                    // written (conv1_2 at 1024^2: 268 MB and a quarter of the epilogue's instructions); same values everywhere else
                    if (lean && !blob_active(c, i) && w.can_skip_out) r.out32 = false;
                }
            }
        } else {
            // bf16 path: the image keeps its fp32 precision (three-way bf16 split, six partial products on the bf16 matrix cores)
            r.kind = (c->bf16 && L.w_split && conv_first_split_ok(L.cin, L.cout, H, W)) ? F_FIRST_SPLIT : F_DIRECT;
            r.out16 = next16;
            r.pack16 = next16 && L.cout % 8 != 0;          // (otherwise the epilogue writes the bf16 copy too)
            // lean: conv1_1's fp32 blob is written only if something reads it (conv1_2, the ReLU mask and a style term take the copy)
            if (lean && next16 && !r.pack16 && conv_next16 && i < last && !blob_needs32(c, sty, i)) r.out32 = false;
            r.bits = r.kind == F_FIRST_SPLIT && bits_i && next16 && !r.pack16;
        }
    }
    for (int b = 1; b <= last; ++b) { fwd[b].style16 = fwd[b].out16 && sty[b].grad16; fwd[b].style_all16 = fwd[b].out16 && sty[b].gram16; }
}

// ----------------------------------------------------------------------------------------- backward
namespace {
// the data gradient of conv layer i (1-based; its input is blob i - 1), from shapes, weights and switches alone
struct Dgrad {
    BwdKind kind;
    bool wants16;                                  // whatever produces its incoming diff writes the bf16 copy
    // it may take the POOLED diff and expand it through the map of the pool above its output (arg-max map of a max pool, sign map of a
    // fused average pool): conv16_body's UNPOOL builds
    // stage the pooled diff and expand it in LDS; the Winograd kernel unpools in its input transform (the split-operand kernel has
    // no unpooling input transform: its launches keep maxpool_bwd_amap_k)
    bool can_unpool;
    bool reads16() const { return kind == B_SMALLM16 || kind == B_CONV16; }      // (packed first where nobody made the copy)
};

Dgrad dgrad_route(const st_ctx* c, const ActSet& a, int i)
{
    const Layer& L = c->topo[i - 1];
    const bool below_is_conv = i - 1 >= 1 && c->topo[i - 2].is_conv;
    const bool small_m = !below_is_conv && conv_dgrad_smallM_ok(L.cout, L.cin);
    if (small_m) return (c->bf16 && L.w_raw_r) ? Dgrad{B_SMALLM16, true, false} : Dgrad{B_SMALLM, false, false};
    // (a conv of few input channels ABOVE a conv keeps the bf16 kernel but is handed an fp32 diff, which it packs)
    if (c->bf16 && conv16_ok(c, L.cout))
        return Dgrad{B_CONV16, !conv_dgrad_smallM_ok(L.cout, L.cin), conv16_resolve(shape16(L.cout, L.cin, a.h[i], a.w[i])).can_unpool};
    const WinoChoice ch = wino_choice(c, L.u_bwd, L.us_bwd, L.cout, L.cin, a.h[i], a.w[i]);
    if (!ch.w.ok) return Dgrad{B_DIRECT, false, false};
    if (!ch.split) return Dgrad{B_WINO, false, ch.w.can_unpool};
    // ST2_WS_DGRAD64=0: K <= 64 launches that the fp32 kernel could unpool (conv1_2's data gradient) stay on the fp32 matrix cores.  With
    // the first split epilogue that was the faster route (404 + 60 us of maxpool_bwd_amap_k against 429 us); since the branch-free
    // epilogue it is not (same-box A/B, profiles/r05_s_ab_split.txt: 177.4 against 176.1 it/s) -- kept as a switch for the A/B only
    if (env_off("ST2_WS_DGRAD64") && L.cout <= 64 && wino_resolve(L.cout, L.cin, a.h[i], a.w[i]).can_unpool) return Dgrad{B_WINO, false, true};
    return Dgrad{B_WINO_SPLIT, false, false};
}
}  // namespace

// The one predicate of "the average pool above conv layer i rides on the bf16 conv launches around it" that is not the max pool's too:
// the switch, and a data gradient of conv i that reads a bf16 diff -- in its staged tile (can_unpool) or from avepool_bwd_map16_k.
// plan_forward fuses only where this holds and records AMAP_BLOCKED16_AVE; plan_backward goes through the map where the record says so
// and the same dgrad_route answer (next.wants16) still holds: the fp32 conv blob the forward skipped is never asked for.
static bool ave_pool_fuse_ok(const st_ctx* c, const ActSet& a, int i)
{
    return c->pool_algo == 1 && dgrad_route(c, a, i).wants16;
}

// `lean` must be what the forward that filled `a` ran with: the fp32 diff of a layer is then written only when its consumer needs
// fp32 (a pool without arg-max map, the 3-channel conv1_1 kernel, a non-bf16 conv), ReLU masks come from the bf16 copies or sign
// maps, and pools fused into their producing conv are back-propagated through their arg-max maps in bf16.
void plan_backward(const st_ctx* c, const ActSet& a, int top, const std::vector<const float*>& inj,
                   const std::vector<const unsigned short*>& fused_w, bool lean, std::vector<BwdRoute>& bwd)
{
    const std::vector<FwdRoute>& fwd = a.plan.fwd;
    bwd.assign(c->nb, BwdRoute{});
    bool have32 = true, have16 = false;            // forms of the running diff (the top diff arrives in fp32)
    bool pooled = false;                           // ... which is still the POOLED diff of the pool just passed
    for (int i = top; i >= 1; --i) {
        const Layer& L = c->topo[i - 1];
        BwdRoute& r = bwd[i];
        const int below = i - 1;
        const bool below_is_conv = below >= 1 && c->topo[below - 1].is_conv;
        const Dgrad next = below_is_conv ? dgrad_route(c, a, below) : Dgrad{B_NONE, false, false};      // the data gradient that runs after this layer's
        if (L.is_conv) {
            const Dgrad d = dgrad_route(c, a, i);
            r.kind = d.kind;
            r.mask = below_is_conv ? MASK_F32 : MASK_NONE;
            r.unpool = pooled; pooled = false;
            r.in16 = d.reads16();
            r.pack_in16 = r.in16 && !have16;
            r.out32 = true;
            if (d.kind == B_CONV16) {
                // the consumer of this launch's output takes bf16 iff it is a bf16 dgrad conv, or (lean) a pool with an arg-max map
                r.out16 = next.wants16 || (lean && below >= 1 && !c->topo[below - 1].is_conv && fwd[below].amap != AMAP_NONE && L.cin % 8 == 0);
                r.out32 = !(lean && r.out16);
                r.style = below >= 1 && (size_t)below < fused_w.size() && fused_w[below] != nullptr;
                // the mask is applied in registers: from the fp32 blob, (lean, or under a fused style term) from the bf16 copy,
                // or from the blob's sign map
                if (below_is_conv && ((lean && fwd[below].out16) || r.style)) r.mask = MASK_BF16;
                if (below_is_conv && lean && fwd[below].bits) r.mask = MASK_BITS;
            }
            have32 = r.out32; have16 = r.out16;
        } else if (L.ave && !(lean && fwd[i].amap == AMAP_BLOCKED16_AVE && !inj[below] && next.wants16)) {
            // dx = mask(dy / window size) + inject in one pass; the bf16 copy for a bf16 dgrad conv below comes out of the same pass
            // (no pack_act16), the fp32 diff where the consumer below reads fp32 (or every diff is materialised)
            r.kind = B_AVEPOOL;
            r.mask = below_is_conv ? MASK_F32 : MASK_NONE;
            r.out16 = c->bf16 && next.wants16;
            r.out32 = !(lean && r.out16);
            have32 = r.out32; have16 = r.out16;
        } else if (lean && fwd[i].amap != AMAP_NONE && !inj[below] && next.wants16) {
            // pool fused into its producing conv: the bf16 diff goes through the arg-max map (ReLU mask of the conv blob included) ...
            r.in16 = true;
            r.pack_in16 = !have16;
            have16 = true;
            // ... inside the data gradient of the conv below when it has the build (maxpool_bwd_idx16_k, its full-resolution
            // output and the conv's read of it are gone)
            // (an average pool whose forward wrote the sign map -- the record of that forward, not the switch's value now -- likewise:
            // inside the data gradient below, or avepool_bwd_map16_k)
            if (next.can_unpool) { r.kind = B_IN_DGRAD_BELOW; pooled = true; }
            else { r.kind = L.ave ? B_AVEPOOL_MAP16 : B_POOL_IDX16; r.out16 = true; have32 = false; }
        } else if (fwd[i].amap == AMAP_PLANAR32 && !inj[below] && below_is_conv && have32) {
            // pool fused into its producing Winograd conv (fp32): through the arg-max map, ReLU mask included, inside the data
            // gradient below (maxpool_bwd_amap_k, its full-resolution output and the conv's read of it are gone; same values bit
            // for bit) or stand-alone
            if (!c->bf16 && next.can_unpool) { r.kind = B_IN_DGRAD_BELOW; pooled = true; }
            else { r.kind = B_POOL_AMAP; r.out32 = true; have32 = true; have16 = false; }
        } else {
            r.kind = B_POOL_CLASSIC;
            r.mask = below_is_conv ? MASK_F32 : MASK_NONE;
            r.out32 = true;
            have32 = true; have16 = false;
        }
    }
}
}  // namespace st2e
