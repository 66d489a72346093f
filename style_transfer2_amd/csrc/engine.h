// Shared declarations of the engine translation units (engine*.cpp): the context behind include/st2.h, its helpers and the
// launch sequences (forward / ranged backward / objective / optimizer step) the C ABI entry points are built from.
#pragma once
#include "../../include/st2.h"
#include "st2_kernels.h"
#include "env.h"
#include "devbuf.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

namespace st2e {
using namespace st2;

// ------------------------------------------------------------------------------------------ errors
int fail(int code, const char* fmt, ...);
#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return st2e::fail(ST_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define ST_TRY(expr)                    \
    do {                                \
        int r_ = (expr);                \
        if (r_ != ST_OK) return r_;     \
    } while (0)

// --------------------------------------------------------------------------------------- profiling
enum ProfClass { P_CONV_FWD, P_CONV_DGRAD, P_POOL_FWD, P_POOL_BWD, P_GRAM, P_GRAM_REDUCE, P_STYLE_GRAD,
                 P_LAYER_ELEM, P_IMAGE_PASS, P_FINALIZE, P_VECTOR, P_MISC, P_CONV_FWD_WINO, P_CONV_DGRAD_WINO,
                 P_CONV_FWD_BF16, P_CONV_DGRAD_BF16, P_COMM, P_GRAM_BF16, P_STYLE_GRAD_BF16, P_CONV_FWD_WSPLIT, P_CONV_DGRAD_WSPLIT, P_STYLE_FUSED_BF16,
                 P_AVEPOOL_FWD, P_AVEPOOL_BWD, P_GRAM_SPLIT, P_STYLE_GRAD_SPLIT, P_AVEPOOL_BWD_MAP16,
                 P_LAP_POOL, P_LAP_STENCIL, P_LAP_GRAD,      // the launches of the Laplacian term (laplacian.hip), the targets' included
                 P_ANCHOR,                                   // anchor_k, the one launch of the anchor term (anchor.hip)
                 P_FRAMES,                                   // frames_k, the one launch of st_set_input_from_frame / st_anchor_from_frame (frames.hip)
                 P_FLOW_PREP, P_FLOW_LINEAR, P_FLOW_JACOBI, P_FLOW_JACOBI_WG,   // optical flow (flow.hip): pyramids, start and interleave; a warp's linearisation; one Jacobi iteration; all of a warp's in one workgroup
                 P_MAT_FIT, P_MAT_APPLY, P_MAT_SET,           // the photorealism term (matting.hip): the two passes of an evaluation; the per-window data
                 P_COUNT };
extern const char* const kProfNames[P_COUNT];
struct ProfRec { int cls; hipEvent_t a, b; double flops, bytes; };

// ------------------------------------------------------------------------------------------- types
struct LayerPacks {                // the device copies of one conv layer's weights
    DevBuf<float> w_fwd, w_bwd, w_raw, w_raw_r, bias;            // w_raw_r: w_raw rounded to bf16 values
    DevBuf<unsigned short> w16_fwd, w16_bwd;                     // bf16 packs (bf16 feature path)
    DevBuf<unsigned short> w_split;                              // first layer, bf16 path: three-way bf16 split of the weights (conv3x3_first_split.hip)
    DevBuf<float> u_fwd, u_bwd;                                  // Winograd F(2x2,3x3) packs (null: not eligible)
    DevBuf<unsigned short> us_fwd, us_bwd;                       // split-operand Winograd packs (conv3x3_wino_split.hip; made when st_set_conv_algo(ctx, 2) asks for them)
};
struct Layer : LayerPacks {
    bool is_conv = false;
    bool ave = false;                                            // pool layer: average (ST_LAYER_AVEPOOL) instead of max pooling
    std::string name;
    int cin = 0, cout = 0;
    bool loaded = false;
};

// ------------------------------------------------------------------------------------- route plan
// What every layer of one evaluation does, decided before the first launch (engine_route.cpp); forward_range and
// backward_chain only execute it.  Entry i describes layer i (topo[i - 1]) and the blob it produces; entry 0 is the image.
enum FwdKind : unsigned char { F_NONE, F_CONV16, F_WINO, F_WINO_SPLIT, F_DIRECT, F_FIRST_SPLIT, F_MAXPOOL, F_AVEPOOL,
                               F_BY_CONV_BELOW };          // F_BY_CONV_BELOW: a pool (max, or average under st_set_pool_algo 1) written by the epilogue of the conv below it
enum AmapLayout : unsigned char { AMAP_NONE, AMAP_BLOCKED16,      // channel-blocked like the bf16 copies (bf16 conv epilogue)
                                  AMAP_PLANAR32,                 // [C][ph][pw] (Winograd epilogues)
                                  AMAP_BLOCKED16_AVE };          // the buffer and layout of AMAP_BLOCKED16 holding an AVERAGE pool's sign bytes (bit e: window element e is inside the blob and > 0)
enum BwdKind : unsigned char { B_NONE, B_SMALLM, B_SMALLM16, B_CONV16, B_WINO, B_WINO_SPLIT, B_DIRECT, B_AVEPOOL, B_POOL_IDX16,
                               B_POOL_AMAP, B_POOL_CLASSIC,
                               B_IN_DGRAD_BELOW,           // a pool expanded inside the data gradient of the conv below it (through the map its forward wrote)
                               B_AVEPOOL_MAP16 };          // an average pool through its sign map, as a pass (avepool_bwd_map16_k)
enum MaskSrc : unsigned char { MASK_NONE, MASK_F32, MASK_BF16, MASK_BITS };

struct FwdRoute {
    FwdKind kind = F_NONE;
    // what the forward leaves of blob i, whichever launch writes it
    bool out32 = false, out16 = false, bits = false;       // fp32 blob, bf16 copy, sign map
    AmapLayout amap = AMAP_NONE;                           // arg-max map (average pool: sign map) of a pool blob: what THIS forward wrote, whatever the switches say later
    bool pack16 = false;                                   // the bf16 copy comes from a pack_act16 pass after the launch
    bool pools_next = false;                               // conv: the pool above rides on this launch (entry i + 1 says what it writes)
    bool style16 = false;                                  // a style blob: the bf16 copy is written and the style gradient can read it (style_shape's grad16)
    bool style_all16 = false;                              // ... and the Gram too: nothing of the style term reads the fp32 blob (style_shape's gram16)
};
struct BwdRoute {
    BwdKind kind = B_NONE;
    bool in16 = false;                                     // reads the incoming diff as its bf16 copy ...
    bool pack_in16 = false;                                // ... which nobody made: pack_act16 first
    bool out32 = false, out16 = false;                     // forms of the diff it produces
    MaskSrc mask = MASK_NONE;                              // ReLU mask of the blob below
    bool unpool = false;                                   // conv: the incoming diff is the POOLED one, expanded through the map of the pool above (either kind: FwdRoute::amap of that pool)
    bool style = false;                                    // conv: the style gradient of the blob below rides on the launch
};
struct RoutePlan { std::vector<FwdRoute> fwd; std::vector<BwdRoute> bwd; };

struct ActSet {                    // activations of one forward geometry
    int H = 0, W = 0;
    std::vector<int> C, h, w;
    std::vector<DevBuf<float>> own;        // the fp32 blobs 1 .. nb - 1; sized and filled by act_ensure ONLY (data[] points into it)
    std::vector<float*> data;              // views: data[i] == own[i] for i >= 1, data[0] is borrowed (the image itself)
    std::vector<DevBuf<unsigned short>> data16;   // bf16 channel-blocked copies of the blobs that feed a bf16 conv
    std::vector<DevBuf<unsigned char>> amap;      // arg-max maps of the pools fused into the producing conv
    std::vector<DevBuf<unsigned short>> bits;     // bf16 lean flow: sign map of a conv blob that feeds a bf16 conv (Conv16Problem::bits_out)
    RoutePlan plan;                        // of the last forward_range / backward_chain on these activations: which of the buffers above it wrote
    int valid_to = -1;
};

struct ActiveLayer { int blob; float cw, sw, dw; bool c, s, d; };

inline bool nonzero(float w) { return fabsf(w) > 1e-15f; }   // NaN compares false: worker.py:234

// one rank's share of a tile-sharded image, in global pixels: the gH x gW image, the origin of the window this context holds, the tile
struct TileGeom { int gH = 0, gW = 0, wy0 = 0, wx0 = 0, ty0 = 0, tx0 = 0, ty1 = 0, tx1 = 0; };
struct BlobRoi { int y0, x0, y1, x1; double n_global; };    // the tile's region of one blob; n_global: elements of the blob of the WHOLE image
struct BlobSize { int h, w, stride; double n; };            // blob b of a gH x gW image: height, width, total stride of its pools, elements

// ------------------------------------------------------------------------------------- objective terms
// The layout of one evaluation's objective, resolved once (objective_terms, engine_objective.cpp): per active row what it is normalised
// by, its region, and the slots it owns in the phase buffers of the tile-sharded mode
struct ObjTerm {                       // one row of c->active, laid out
    ActiveLayer al; int b, C;
    size_t n;                          // elements of the blob this context holds
    double n_norm;                     // elements of the blob of the WHOLE image (== n without a tile)
    BlobRoi roi; bool has_roi;         // the tile's region (tile mode), else the whole blob
    size_t sums;                       // offset of its four sums [d2, gc2, F2, gd2] in the phase-1 buffer
    size_t gram;                       // offset of its raw C x C Gram sums there (style rows), else kNoSlot
    int k;                             // ordinal among the style rows (slot in p2 / pd / p3 + 6), else -1
    const BlobRoi* region() const { return has_roi ? &roi : nullptr; }
};
constexpr size_t kNoSlot = ~(size_t)0;
struct ObjTerms { std::vector<ObjTerm> t; int last = -1; size_t n1 = 0; int n_style = 0; };     // last: deepest weighted blob (-1: none); n1: floats of the phase-1 buffer

// ------------------------------------------------------------------------------------- style term
// The style term of one blob, resolved once (engine_style.cpp): the kernel family of each of its two GEMMs, what the launches need and book
struct StyleShape { bool grad16, gram16; };        // from shapes and switches alone: the style gradient / also the Gram can run on the blob's bf16 copy
enum StyleOps : unsigned char { OPS_F32, OPS_SPLIT, OPS_BF16,    // the fp32 blob on the fp32 matrix cores; its three-way split on the bf16 ones (gram_split.hip); the bf16 copy (gram16.hip, style16.hip)
                                OPS_FUSED };                    // gradient only: rides on the bf16 data-gradient conv above the blob; here its operand pack and trace value
struct StyleLaunch { StyleOps ops; int cls; double flops, bytes; };      // family, profiler class and figures of one launch
struct StyleTerm {
    int b, C, hw;                                  // hw: the pixels both GEMMs contract -- the blob's, or the region's
    bool roi; GramRoi groi; PixRoi proi;           // region of interest (tile-sharded phases, sharded style pass), in both kernels' forms
    StyleLaunch gram, grad, pack;                  // Gram partials (plan below), style gradient, OPS_FUSED: the operand pack before it
    GramPlan plan;                                 // gram_plan, or gram_plan16 for OPS_BF16
    int slots;                                     // sum S^2 partials the gradient launch writes (s2_part)
    size_t d16, sfuse;                             // scratch elements the gradient needs in c->d16 / c->sfuse_w[b] (OPS_SPLIT: c->dsplit, sized by st_set_gram_algo)
    bool reads32, reads16, missing32;              // copies of the blob the term reads; missing32: it reads the fp32 blob and the forward skipped it
    bool book;                                     // the launches are booked with the profiler (the phases of a tile-sharded iteration are not)
};

// ------------------------------------------------------------------------------------- layer terms (test hook)
// What the last objective evaluation left in the work buffers, for st_get_layer_terms.  dbuf (D) and stmp (the unscaled style
// gradient) are ONE buffer each for all layers: the record says whose data they hold.  Host bookkeeping only -- nothing here is
// read by a launch.
enum LtDiff : char { LT_NONE, LT_WRITTEN, LT_RODE_ON_CONV, LT_OVERWRITTEN };
struct LayerTerms {
    bool any = false;                              // an evaluation has completed, and the buffers still have its geometry
    bool resized = false;                          // ... it had, until the iterate was resized
    int style_blob = -1;                           // the style layer evaluated last: dbuf holds its D
    int raw_blob = -1;                             // ... and stmp its unscaled gradient (a first evaluation of that layer), else -1
    std::vector<size_t> n;                         // per blob: elements of its diff in that evaluation (0: the blob carried no weight)
    std::vector<int> C;
    std::vector<char> diff;                        // per blob: LtDiff of inject[b]
    std::vector<char> norm_ok;                     // per blob * 3: the norm was known when the evaluation ended
    void begin(int nb) { any = resized = false; style_blob = raw_blob = -1; n.assign(nb, 0); C.assign(nb, 0); diff.assign(nb, LT_NONE); norm_ok.assign((size_t)nb * 3, 0); }
};

// ------------------------------------------------------------------------------------- the tapped diff (test hook)
// st_tap_diff: the running diff of ONE blob, copied out of the backward's ping-pong buffers right after the launch that wrote it
// (backward_chain), in the forms that launch wrote.  Off (blob < 0) nothing is enqueued and nothing is allocated.
struct DiffTap {
    int blob = -1;                                 // the tapped blob; -1: off
    bool armed = false;                            // inside an st_opfunc evaluation with a gradient: backward_chain copies
    bool captured = false;                         // ... and did, in this evaluation
    bool have = false;                             // an evaluation with a gradient has completed since the tap was set, and copied
    bool resized = false;                          // ... it had, until the iterate was resized
    bool have32 = false, have16 = false;           // the forms the launch wrote (BwdRoute::out32 / out16)
    int C = 0, h = 0, w = 0;                       // the blob's shape in that evaluation
    DevBuf<float> d32;                             // [C][hw]
    DevBuf<unsigned short> d16;                    // channel-blocked [C/8][hw][8]
};
}  // namespace st2e

using namespace st2e;

struct st_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool bf16 = false;                             // conv operands in bf16 (BASELINE config 3)
    bool lean = false;                             // bf16 objective evaluations skip the fp32 tensors only bf16 convs would read
    bool in_step = false;                          // inside step_enqueue: objective evaluations may skip fp32 blobs nothing reads (lean fp32)
    bool wino = true;                              // Winograd F(2x2,3x3) for the eligible fp32 convs (ST2_WINO=0 disables)
    bool wino_split = false;                       // ... on the bf16 matrix cores with three-way split operands where the shape allows (st_set_conv_algo(ctx, 2))
    int pool_algo = 0;                             // 1: an average pool rides on the bf16 conv launches around it in the lean flow (st_set_pool_algo)
    bool gram_split = false;                       // fp32 features: Gram partials and style gradients on the bf16 matrix cores with three-way split operands where the shape allows (st_set_gram_algo(ctx, 1))
    DevBuf<unsigned short> dsplit;                 // ... and the three-term operand image of D (gram_split.hip), sized for the widest blob when the option is set
    DevBuf<unsigned short> diff16A, diff16B;
    std::vector<Layer> topo;
    std::vector<std::string> blob_names;
    int nb = 0;                                    // number of blobs (= layers + 1)

    ActSet act;                                    // geometry of input/content
    // image state
    int H = 0, W = 0;                              // input geometry (0 = no input)
    DevBuf<float> x[2];
    int cur = 0;
    DevBuf<float> fwd_x;                           // image of the st_forward test hook (never the job's iterate)
    DevBuf<float> grad;                            // combined gradient (opfunc / L-BFGS)
    // content / style
    int cH = 0, cW = 0;
    std::vector<DevBuf<float>> content_feat;        // per blob
    DevBuf<float> content_x;                       // preprocessed content image (for resample_content)
    std::vector<DevBuf<float>> style_gram;          // per blob, C*C
    std::vector<char> style_valid;                 // per blob: style_gram holds a target (st_set_style: every blob; st_tile_style_commit: 0 .. last_blob)
    bool have_content = false, have_style = false;
    // objective
    std::vector<ActiveLayer> rows;                 // every row of the weights table, in order
    std::vector<ActiveLayer> active;               // rows with any non-zero weight
    float tv_w = 1, tv_pow = 1, p_w = 1, p_pow = 1;   // worker.py:133 defaults
    DevBuf<float> norms;                           // [nb][3] on device
    std::vector<char> norm_valid;                  // [nb*3]
    // work buffers (input geometry)
    std::vector<DevBuf<float>> inject;
    std::vector<char> inject_roi_zero;             // per blob: the inject buffer is zero outside the tile's region of interest (tile-sharded bf16 style term)
    DevBuf<float> diffA, diffB, stmp;
    size_t max_blob = 0;
    DevBuf<float> gram_slabs, gram_fold, dbuf;
    DevBuf<unsigned short> d16;                    // bf16 path: hi/lo operand image of D (style16.hip)
    // bf16 path, style term fused into the data-gradient conv above the style blob: per blob the scaled hi/lo image of D (kept until
    // that conv has run) and, during one objective evaluation, the operands handed to backward_chain
    std::vector<DevBuf<unsigned short>> sfuse_w;
    std::vector<const unsigned short*> sf_in, sf_w;
    LayerTerms lt;                                 // test hook st_get_layer_terms: whose data dbuf, stmp and the inject buffers hold
    DiffTap tap;                                   // test hook st_tap_diff / st_get_tapped_diff
    DevBuf<float> conv_scratch;                    // split-K partial sums of Winograd launches
    // hipGraph replay of the steady-state Adam step (launch-bound regime: small images)
    unsigned long long epoch = 0;                  // bumped by every API call that can change what a step launches
    hipGraphExec_t gexec[2] = {nullptr, nullptr};  // one per parity of the x ping-pong
    unsigned long long gepoch[2] = {0, 0};
    DevBuf<float> adam_dyn;                        // device {corr1, corr2, step}: the only per-step arguments
    bool capturing = false, graphs = false;        // opt-in (ST2_GRAPH=1): measured, no gain -- see step_graph_ok()
    int plain_steps = 0;                           // normal steps since the last epoch change (buffers are allocated lazily)
    unsigned long long plain_epoch = ~0ull;
    size_t graph_max_px = 768 * 768;
    long long graph_replays = 0;
    std::vector<DevBuf<float>> layer_part;          // per blob: 5 * kMaxPartials
    std::vector<DevBuf<float>> s2_part;             // per blob: style-grad partial sums
    std::vector<int> cnt;                          // per blob * 6 partial counts
    DevBuf<float> image_part;                      // 6 * kMaxPartials
    int image_cnt = 0;
    DevBuf<float> trace_dev;
    DevBuf<double> trace_sums;                     // device scratch of the trace finalisation
    PinBuf<float> trace_host;
    int trace_len_last = 8;
    DevBuf<float> hwc_dev;
    // pipelined iterations (st_step_begin / st_step_end): up to two in flight; the iterate of step k travels to pinned host memory
    // on its own stream while step k + 1 computes
    struct Pipe {
        // kSlots buffers although only two iterations are ever in flight: an iterate handed out by st_step_end stays valid for
        // kSlots - 1 further begins, which is what lets the worker's sender thread pickle it without a host-side copy
        static constexpr int kSlots = 6;
        hipStream_t copy = nullptr;
        DevBuf<float> hwc[kSlots]; float* img_pin[kSlots] = {}; PinBuf<float> trace_pin[kSlots];
        PinBuf<char> pin_base[kSlots];             // the pinned allocation of a slot: [head room | image | tail room]; img_pin points at the image
        hipEvent_t ready[kSlots] = {}, done[kSlots] = {};
        size_t cap = 0; long long head = 0; int count = 0, tlen[kSlots] = {}, H[kSlots] = {}, W[kSlots] = {};
        // bytes the caller may write in front of / behind an iterate handed out by st_step_end (a message frame around the image,
        // st_step_frame_room): requested, and what the current buffers were allocated with
        size_t want_head = 0, want_tail = 0, have_head = 0, have_tail = 0;
        // Buffers replaced by a re-allocation (the input grew, the frame room changed) stay alive until kSlots further begins have
        // passed: views handed out before it keep the documented lifetime.
        struct Retired { PinBuf<char> buf; long long at; };
        std::vector<Retired> retired;
        long long begins = 0;
    } pipe;
    DevBuf<unsigned char> stage_dev;               // host images on their way to preprocess_into
    // optimizer
    int opt_kind = ST_OPT_NONE;
    double step_size = 1.0;
    DevBuf<float> m, v;
    int items1 = 0, items2 = 0;
    bool m_zero = true, v_zero = true;
    // L-BFGS
    static const int kCorr = kLbfgsCorr;
    DevBuf<float> hs[kLbfgsSlots];                 // ring of s vectors (10 pairs + the one being formed)
    DevBuf<float> hy[kLbfgsSlots];
    DevBuf<LbfgsDev> lb_dev;                       // history bookkeeping (pair count, ring order, s.y, y.y): device-resident
    bool lb_clear = true;                          // history to be emptied before the next step (reset / objective_changed)
    DevBuf<float> lb_part;                         // [4][kMaxPartials] partial sums of the chained dot products
    DevBuf<LbfgsGram> lb_gram;                     // Gram form (lbfgs.hip, second half): inner-product matrix + coefficients
    DevBuf<float> lb_gpart;                        // [kLbGramRows][kMaxPartials] partial sums of the inner-product pass
    DevBuf<float> lb_dots;                         // test hook: [kLbNB][kLbNB] pairwise inner products
    bool lb_gram_form = false;                     // form of the current history (decided while it is empty)
    DevBuf<float> g_cur, pvec;
    bool have_cur = false;
    float last_loss = 0.f;
    // iterate averaging (st_set_iterate_average): utils.DecayingMean over the iterates of every optimizer step
    DevBuf<float> avg;                             // the raw mean, (3, H, W); allocated while the mode is on and an input exists
    double avg_decay = 0.0;                        // 0: off
    int avg_items = 0;                             // 0: the mean is empty (the buffer's contents do not count)
    // the content's colours (engine_color.cpp)
    bool orig_colors = false;                      // st_set_original_colors: the images handed out take their chroma from content_x
    int style_match = 0;                           // 0 off, 1 st_set_style_color_match (derive per style image), 2 st_set_style_transform (given)
    float xf_A[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, xf_b[3] = {0, 0, 0};      // the style transform given, or the one last derived and applied
    DevBuf<double> mom_part, mom_out;              // image_moments_k's per-workgroup partial sums and the nine sums
    // the Laplacian-steered content term (st_set_laplacian; engine_laplacian.cpp, laplacian_plan.h)
    struct Lap {
        int n = 0;                                 // levels; 0: off, and every buffer below is empty
        int pool[kLapMaxLevels] = {0, 0, 0};
        double weight[kLapMaxLevels] = {0, 0, 0};
        LapPlan plan{};                            // of the geometry the buffers were sized for (plan.n == 0: none yet)
        DevBuf<float> q, t, e;                     // per level, back to back (LapLevel::off): pooled iterate / content, targets T, differences E
        DevBuf<float> g;                           // g_lap, (3, H, W)
        DevBuf<float> part;                        // kLapPartRows * kMaxPartials
        bool targets_ok = false;                   // t holds D(P(content_x / 255)) of the current content image at the plan's size
        int cnt_e = 0, cnt_g = 0;                  // partial counts of the last evaluation
        bool evaluated = false, have_grad = false; // e (and g) hold the last evaluation's
        bool resized = false;                      // ... they did, until the input was resized
    } lap;
    // the anchor term (st_set_anchor; engine_anchor.cpp, anchor_plan.h)
    struct Anchor {
        bool on = false;                           // off: every buffer below is empty
        double weight = 0;
        bool has_mask = false;
        AnchorPlan plan{};                         // of the anchor's size -- the anchor does not follow the input
        DevBuf<float> ax, m;                       // the preprocessed anchor (3, H, W), the map (H, W) when there is one
        DevBuf<float> extra;                       // g_lap + g_anc, or g_anc: what the image pass adds after p_w g_p
        DevBuf<float> part;                        // kAnchorPartRows * kMaxPartials
        int cnt = 0;                               // partial count of the last evaluation
        bool evaluated = false, have_grad = false; // extra holds the last evaluation's
        bool resized = false;                      // ... it did, until the input was resized
    } anchor;
    // the photorealism term (st_set_matting; engine_matting.cpp, matting_plan.h)
    struct Matting {
        bool on = false;                           // off: every buffer below is empty
        double weight = 0, eps = 0;
        MatPlan plan{};                            // of the input's size when the buffers were made (H == 0: none yet)
        DevBuf<float> I;                           // content_x / 255, (3, H, W)
        DevBuf<float> win;                         // per-window planes: mu, M (MatPlan::off_*), then a_pb
        DevBuf<float> extra;                       // prev + g_mat, or g_mat: what the image pass adds after p_w g_p
        DevBuf<float> part;                        // kMatPartRows * kMaxPartials
        int cnt_l = 0, cnt_g = 0;                  // partial counts of the last evaluation
        bool windows_ok = false;                   // I, mu, M are those of the current content image at the plan's size
        bool evaluated = false, have_grad = false; // a_pb (and extra) hold the last evaluation's
        bool resized = false;                      // ... they did, until the input was resized
    } mat;
    // jitter (st_set_jitter; engine_jitter.cpp, jitter_plan.h): the network terms are evaluated on a rolled copy of the iterate
    struct Jitter {
        bool on = false;                           // off: every buffer below is empty
        int radius = 0;                            // 0 with a pinned shift
        unsigned long long seed = 0;
        long long k = 0;                           // optimizer steps begun since the last setter / st_optimizer_reset
        bool pinned = false; int pin_dy = 0, pin_dx = 0;
        const float* scd_s = nullptr;              // inside an evaluation: the network gradient before the un-roll (a diff buffer of the backward)
        DevBuf<float> xs, g, cxs;                  // roll(x, s); unroll of the network gradient; roll(content_x, s) (made when a content row first asks)
        // what the last evaluation left (st_get_jitter_terms)
        bool evaluated = false, rolled = false, have_grad = false, resized = false;
        int last_dy = 0, last_dx = 0, last_H = 0, last_W = 0;
    } jit;
    // the shift content_feat belongs to, reduced mod (cH, cW); (0, 0) whenever the mode has never been on
    int feat_dy = 0, feat_dx = 0;
    // frame sequences (st_frames_keep .. st_anchor_from_frame; engine_frames.cpp, frames_plan.h)
    struct Frames {
        int depth = 0;                             // 0: nothing is kept and every buffer below is empty
        int count = 0;                             // frames held: slot[0 .. count) are frames 1 .. count, the newest first
        int H = 0, W = 0;                          // their size (count > 0)
        DevBuf<float> slot[kFramesMaxDepth];       // raw iterates (3, H, W); allocated by the pushes
        DevBuf<float> stage;                       // the caller's flows and map on their way to frames_k: [bwd | fwd | mask], grown on demand
    } frames;
    // optical flow (st_flow_estimate .. st_get_flow_level; engine_flow.cpp, flow_plan.h)
    struct Flow {
        DevBuf<float> scratch;                     // everything an estimate needs, laid out by flow_plan; grown on demand, kept until st_flow_release
        FlowPlan plan{};                           // of the last estimate
        bool have = false;                         // scratch holds the levels of a finished estimate (st_get_flow_level)
    } flow;
    // tile-sharded mode (BASELINE config 5): this context holds ONE window of a larger image
    struct Tile : TileGeom {
        bool on = false;
        DevBuf<float> p1, p2, p3, pd;              // reduce buffers (device)
        bool s2_in_p2 = false;
        bool evaluated = false;                    // the phase buffers hold a complete evaluation (forward .. image pass) of the current weights: st_tile_trace may finish it
        DevBuf<float> wgrad;                       // window gradient (3, wh, ww)
        bool fused = false;                        // inside st_tile_step: the phases do not synchronise the stream on their own
        // fused L-BFGS over the sharded image (engine_comm.cpp): this rank's tile of x as a compact (3, th, tw) vector, the sums of
        // one inner-product pass (all-reduced), and the global image size the unit-RMS first direction divides by
        DevBuf<float> lb_x, lb_sums;
        // the sharded style pass (st_tile_style_partials -> all-reduce -> st_tile_style_commit): raw Gram sums of blobs 0 .. sp_last over
        // this rank's tile of the sp_gH x sp_gW style image, back to back; sp_last < 0: no partials wait for a commit
        DevBuf<float> sp; int sp_n = 0, sp_last = -1, sp_gH = 0, sp_gW = 0;
    } tile;
    // communicator of the tile-sharded mode (engine_comm.cpp): RCCL over xGMI, or caller-supplied transport functions (tests)
    struct Comm {
        void* lib = nullptr;                       // librccl.so, loaded on first use
        void* comm = nullptr;                      // ncclComm_t
        int rank = 0, world = 1;
        bool set = false;                          // st_comm_init / st_comm_callbacks has run (a fresh context looks like world 1 otherwise)
        st_allreduce_fn ar = nullptr; st_exchange_fn ex = nullptr; void* user = nullptr;
        struct Peer { int peer = 0; std::vector<int> send, recv; DevBuf<float> sbuf, rbuf; size_t sn = 0, rn = 0; };
        std::vector<Peer> plan[3];                 // per phase (ST_TILE_PLAN_*): the peers this rank exchanges strips with
        bool planned[3] = {false, false, false};
        bool self_via_rccl = false;                // test hook (ST2_COMM_SELF_VIA_RCCL=1): copies to the own rank travel through RCCL too
        DevBuf<float> ring;
        long long steps = 0;
        std::vector<float> h1, h2, h3, hd, hn;     // host side of a traced step (sized once: no allocation per step)
        DevBuf<float> tile_chw, tile_hwc;          // st_tile_get_tile's staging (kept across calls)
        DevBuf<float> tile_cx;                     // ... and, under st_set_original_colors, the matching packed tile of content_x
    } comm;
    // profiling
    bool prof_on = false;
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;

    int blob_c(int i) const { return act.C[i]; }
    int blob_c_topo(int i) const                   // channels of blob i from the topology alone (no activation set needed)
    {
        for (int k = i; k >= 1; --k) if (topo[k - 1].is_conv) return topo[k - 1].cout;
        return 3;
    }
};

namespace st2e {
// ---------------------------------------------------------------------------------------- helpers (engine.cpp)
inline size_t act16_elems(int C, size_t hw) { return (size_t)((C + 7) / 8) * hw * 8; }
inline bool conv16_ok(const st_ctx* c, int K) { (void)c; return K >= 8 && K % 8 == 0; }
int wino_scratch(st_ctx* c, ConvProblem& p, int splits);      // room for the split-K partial sums (WinoLaunch::splits) of a Winograd launch that would otherwise leave most CUs idle

struct ProfScope {
    st_ctx* c; int idx = -1;
    ProfScope(st_ctx* ctx, int cls, double flops, double bytes, bool book = true) : c(ctx)
    {
        if (!c->prof_on || !book) return;
        auto get = [&]() {
            if (c->ev_used == c->ev_pool.size()) {
                hipEvent_t e;
                (void)hipEventCreate(&e);
                c->ev_pool.push_back(e);
            }
            return c->ev_pool[c->ev_used++];
        };
        ProfRec r{cls, get(), get(), flops, bytes};
        (void)hipEventRecord(r.a, c->stream);
        c->prof.push_back(r);
        idx = (int)c->prof.size() - 1;
    }
    ~ProfScope()
    {
        if (idx >= 0) (void)hipEventRecord(c->prof[idx].b, c->stream);
    }
};

// work that rides on another class's launch (the style-gradient chunks fused into a bf16 data-gradient conv): flops booked to a class of
// their own with no time, so that the carrying class's flops stay the ones SURVEY 8(d) counts for it
inline void prof_note(st_ctx* c, int cls, double flops)
{
    if (!c->prof_on) return;
    if (c->ev_used == c->ev_pool.size()) { hipEvent_t e; (void)hipEventCreate(&e); c->ev_pool.push_back(e); }
    hipEvent_t e = c->ev_pool[c->ev_used++];
    (void)hipEventRecord(e, c->stream);
    c->prof.push_back(ProfRec{cls, e, e, flops, 0.0});
}

void shapes_for(const st_ctx* c, int H, int W, std::vector<int>& C, std::vector<int>& h, std::vector<int>& w);
int act_ensure(st_ctx* c, ActSet& a, int H, int W);
int forward_range(st_ctx* c, ActSet& a, const float* x, int last, bool lean = false);
int backward_chain(st_ctx* c, int top, const float* top_diff, const std::vector<const float*>& inj, const float** out, bool lean = false);
int ensure_input_buffers(st_ctx* c, int H, int W);
int stage_upload(st_ctx* c, const void* host, size_t bytes);
int preprocess_into(st_ctx* c, const void* hwc, int H, int W, int is_u8, float* dst);
int set_input_common(st_ctx* c, int H, int W);
void iterate_overwritten(st_ctx* c);
int content_from_device(st_ctx* c, const float* xdev, int H, int W);
int style_from_device(st_ctx* c, const float* xdev, int H, int W);      // style image on the device -> full forward, the target of every blob; returns with them in place
int ensure_content_features(st_ctx* c);          // features of content-weighted blobs dropped by st_set_weights: recompute from the kept image
// ---------------------------------------------------------------------------------------- engine_route.cpp
// The planners only decide: no HIP call, no allocation on the device, nothing in the context changes.  Every shape predicate and
// every per-call environment switch of the routing is read here, once per forward_range / backward_chain call (never cached: the
// tests flip the switches between evaluations of one process).
void plan_forward(const st_ctx* c, const ActSet& a, int last, bool lean, std::vector<FwdRoute>& fwd);
// `a.plan.fwd` must be the plan of the forward that filled `a`; inj / fused_w: per blob, non-null where a diff is injected /
// where a fused style operand waits for the data gradient above the blob
void plan_backward(const st_ctx* c, const ActSet& a, int top, const std::vector<const float*>& inj,
                   const std::vector<const unsigned short*>& fused_w, bool lean, std::vector<BwdRoute>& bwd);
bool lean32_enabled();                            // ST2_LEAN32 (read per evaluation: A/B runs)
// ---------------------------------------------------------------------------------------- engine_style.cpp
// The resolver: no HIP call, no allocation, nothing in the context changes; every predicate and per-call switch of the style term is
// read here.  style_shape: what plan_forward asks before the forward; style_term: from what that forward left (a.plan.fwd) -- roi: the
// tile's region, target: a style target (always the fp32 blob), fuse_last >= 0: the backward starts at that blob and the term may ride on it
StyleShape style_shape(const st_ctx* c, const ActSet& a, int b);
StyleTerm style_term(const st_ctx* c, const ActSet& a, int b, const BlobRoi* roi = nullptr, bool target = false, int fuse_last = -1);
size_t style_split_scratch(int C, int hw);        // elements of c->dsplit the split-operand style gradient of such a blob needs; 0: the split kernels refuse it
// launch_gram_reduce's contract over the term's Gram partials
int style_gram(st_ctx* c, const ActSet& a, const StyleTerm& t, const float* target, float* out, int out_ld, double divisor, float* partial, int* n_partial);
// launch_style_grad's contract with D in c->dbuf; the partials go to c->s2_part[b], their count to *np.  OPS_FUSED ignores dst / fused / accumulate
int style_grad(st_ctx* c, const ActSet& a, const StyleTerm& t, float* dst, float c2, int fused, float sw, int accumulate, int* np);
int ensure_dbuf(st_ctx* c);                       // [C][MPad] scratch for D = G - G_style, sized for the widest blob, zeroed once
int ensure_layer_part(st_ctx* c, int b);
// the content / deep-dream term of an active blob of c->act: n_norm divides its coefficients, part (nullable) takes the four sums
LayerElemArgs layer_elem_args(const st_ctx* c, const ActiveLayer& al, double n_norm, int write, float* part, const BlobRoi* roi = nullptr);
// ---------------------------------------------------------------------------------------- engine_objective.cpp
// The table: no HIP call, no allocation, nothing in the context changes; rebuilt per call (the tests change weights and switches between
// evaluations).  `a` holds the geometry of the evaluation (act_ensure has run); tile: the geometry of a tile-sharded context, else NULL.
// It is also the preflight: ST_ERR_STATE where a weighted row lacks its content features or its style target
int objective_terms(const st_ctx* c, const ActSet& a, const TileGeom* tile, ObjTerms& terms);
BlobSize blob_size(const st_ctx* c, int b, int gH, int gW);
BlobRoi tile_roi(const st_ctx* c, const ActSet& a, const TileGeom& t, int b);      // the tile's region in blob b of the activation set that holds the window
// launch_image_pass's arguments for the image x: adam: the fused update into x_next (the only place that names Adam's constants)
ImagePassArgs image_pass_args(const st_ctx* c, const float* x, const float* scd, float* grad, bool adam, float* x_next);
int eval_objective(st_ctx* c, const float* x, bool want_grad, float* grad_out, bool adam, float* x_next);
int read_trace(st_ctx* c, double* trace, float* loss);
// ---------------------------------------------------------------------------------------- engine_step.cpp
int lbfgs_alloc(st_ctx* c);
LbfgsArgs lbfgs_args(st_ctx* c, int apply);
int lbfgs_clear_history(st_ctx* c, bool gram_form);        // what lbfgs_step and the fused tile step do while c->lb_clear is set
float average_corr(const st_ctx* c);              // iterate averaging: the divisor float(1 - decay ** items) of utils.py:64
// ---------------------------------------------------------------------------------------- engine_emit.cpp
// Emission (emit_plan.h): the image a reader hands out, and DecayingMean.__call__(x) on the current iterate where a step advances the
// iterate average.  emit_preflight: the plan for `reader` (EmitReader; want_image: st_step's out_hwc), or the plan's refusal as a status
// and a message -- no HIP call, nothing changes: every reader asks before it enqueues anything.  emit_enqueue: the plan's one launch,
// booked as P_MISC with the bytes of its streams (plan.book), or nothing; staged_v / staged_cx: the packed (3, h, w) tiles of a tile reader in place
// of the context's own tensors (NULL: those, at h = H, w = W)
int emit_preflight(const st_ctx* c, int reader, bool want_image, EmitPlan* plan);
int emit_enqueue(st_ctx* c, const EmitPlan& plan, float* hwc, const float* staged_v, const float* staged_cx, int h, int w);
// ---------------------------------------------------------------------------------------- engine_color.cpp
// the style image on its way to the forward: refuses (ST_ERR_STATE) what colour matching cannot run on -- before anything is enqueued --
// then derives the transform where st_set_style_color_match asks for it (waits for the stream) and recolours x (3, H, W) in place
int style_color_check(const st_ctx* c);
int style_recolor_enqueue(st_ctx* c, float* x, int H, int W);
// ---------------------------------------------------------------------------------------- engine_laplacian.cpp
// The Laplacian term of an evaluation.  lap_preflight: the refusals (no content image, one of another size than the input), ST_OK with
// the term off -- no HIP call, nothing changes: every evaluation asks before it enqueues anything.  lap_forward: buffers of the input's
// size, the targets where the content or the size changed since they were taken, then pool and stencil on x.  lap_backward: g_lap
int lap_preflight(const st_ctx* c);
int lap_forward(st_ctx* c, const float* x);
int lap_backward(st_ctx* c);
void lap_input_resized(st_ctx* c);                // the input has a new size: the term's buffers are those of the old one
// ---------------------------------------------------------------------------------------- engine_anchor.cpp
// The anchor term of an evaluation.  anchor_preflight: the refusals (a tile-configured context, an anchor of another size than the
// input), ST_OK with the term off -- no HIP call, nothing changes: every evaluation asks before it enqueues anything.  anchor_eval: the
// one launch, after the Laplacian term's; g_lap: that term's gradient or NULL; *extra: what launch_image_pass takes as `lap` (NULL for an
// evaluation without a gradient).  anchor_trace: a_loss and a_grad into the image part of the trace at image_out
int anchor_preflight(const st_ctx* c);
int anchor_eval(st_ctx* c, const float* x, bool want_grad, const float* g_lap, const float** extra);
int anchor_trace(st_ctx* c, bool want_grad, bool with_lap, float* image_out);
void anchor_input_resized(st_ctx* c);             // the input has a new size: `extra` is that of an evaluation at the old one
// ---------------------------------------------------------------------------------------- engine_matting.cpp
// The photorealism term of an evaluation.  mat_preflight: the refusals (a tile-configured context, no content image, one of another size
// than the input, an input under 3 x 3), ST_OK with the term off -- no HIP call, nothing changes: every evaluation asks before it enqueues
// anything.  mat_eval: after the anchor term's launch -- buffers of the input's size, the per-window data where the content or the size
// changed since they were taken, the first pass and, with a gradient, the second; prev: what `extra` was without this term or NULL;
// *extra: what launch_image_pass takes as `lap` (left alone for an evaluation without a gradient).  mat_trace: m_loss and m_grad into the
// image part of the trace at image_out, which holds `others` (0 .. 2) optional terms already
int mat_preflight(const st_ctx* c);
int mat_eval(st_ctx* c, const float* x, bool want_grad, const float* prev, const float** extra);
int mat_trace(st_ctx* c, bool want_grad, int others, float* image_out);
void mat_input_resized(st_ctx* c);
// ---------------------------------------------------------------------------------------- engine_jitter.cpp
// Jitter inside an evaluation; with the mode off each returns at once and launches nothing.  jitter_preflight: the refusal (a
// tile-configured context) -- no HIP call, nothing changes.  jitter_content: content_feat made those of the shift this evaluation uses
// (of (0, 0) with the mode off), after objective_terms has checked the content image; skipped where they already are.  jitter_roll_in:
// *xf = the planes the forward reads, x itself or the mode's buffer holding roll(x, s).  jitter_roll_out: *scd (non-null) replaced by its
// un-rolled copy for the image pass.  jitter_scd_sums, after the image pass: the scd row of its partial sums retaken over the planes
// BEFORE the un-roll, in that kernel's order -- scd_grad has the bits of the shifted evaluation
int jitter_preflight(const st_ctx* c);
int jitter_content(st_ctx* c);
int jitter_roll_in(st_ctx* c, const float* x, bool want_grad, const float** xf);
int jitter_roll_out(st_ctx* c, const float** scd);
int jitter_scd_sums(st_ctx* c);
void jitter_step_begun(st_ctx* c);                // an optimizer step has run its evaluations: the next one draws the next shift
void jitter_input_resized(st_ctx* c);             // the input has a new size: the mode's buffers are those of the old one
// ---------------------------------------------------------------------------------------- engine_tile.cpp
// pack (mode 0) / unpack (1 assign, 2 add) the rectangles (y0, x0, h, w each) of a (C, h, w) tensor; checks them against it; enqueues only
int strips(st_ctx* c, float* tensor, int C, int h, int w, const std::vector<int>& rects, float* buf, int mode);
// ---------------------------------------------------------------------------------------- engine_comm.cpp
void comm_free(st_ctx* c);
int comm_allreduce(st_ctx* c, float* buf, int n);  // in-place sum of n floats over the ranks, ordered on the engine's stream
}  // namespace st2e
