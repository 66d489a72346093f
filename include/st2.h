/* st2.h -- C ABI of libst2_hip.so: the MI355X-resident style-transfer inner loop.
 *
 * The reference (crowsonkb/style_transfer2) has no FFI of its own: the hot path sits behind two
 * Python duck types inside worker.py -- the model (``CaffeModel``, worker.py:32-106) and the
 * objective/optimizer pair (``StyleTransfer`` worker.py:117-315, optimizers.py:7-125).  Each entry
 * point below names the reference interface it replaces.  The reference-side binding (a ctypes
 * stub that drops into worker.py) is shown in INTEGRATION.md; this repo's own host mirror is
 * style_transfer2_amd/engine.py.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success and a non-zero
 * code on failure with a message available from st_last_error(); host buffers are caller-owned
 * and are fully consumed/produced before the call returns; all device state is owned by the
 * handle; one handle is driven by one host thread.  Images cross the boundary as HxWx3 RGB
 * (uint8 or float32) exactly as in messages.py:89-110; tensors as contiguous NCHW float32.
 */
#ifndef ST2_H
#define ST2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct st_ctx st_ctx;

enum { ST_OK = 0, ST_ERR_ARG = 1, ST_ERR_STATE = 2, ST_ERR_HIP = 3 };
enum { ST_OPT_NONE = 0, ST_OPT_ADAM = 1, ST_OPT_LBFGS = 2 };
enum { ST_LAYER_CONV = 0, ST_LAYER_POOL = 1, ST_LAYER_AVEPOOL = 2 };

/* One layer of a VGG-shaped topology: Conv3x3(pad 1)+ReLU (ST_LAYER_CONV), MaxPool 2x2/2 (ST_LAYER_POOL) or AvePool 2x2/2
 * (ST_LAYER_AVEPOOL: Caffe `pool: AVE`, the divisor is the window clipped to the blob, 4, 2 or 1), both pools in Caffe ceil mode.
 * st_create refuses any other kind with ST_ERR_ARG; tile-sharded mode (st_tile_configure) refuses a net with an average pool. */
typedef struct st_layer_desc {
    int kind;            /* ST_LAYER_CONV | ST_LAYER_POOL | ST_LAYER_AVEPOOL */
    const char* name;    /* blob/layer name, e.g. "conv1_1" */
    int cin, cout;       /* conv only */
} st_layer_desc;

const char* st_last_error(void);

/* ---- model: replaces CaffeModel.__init__/reload_net (worker.py:36-61) ------------------------- */
/* n_layers == 0 selects models/vgg19.prototxt (16 conv + 5 pool). device_id follows the `gpu`
 * config key (worker.py:328): it is passed to hipSetDevice. */
int st_create(st_ctx** out, int device_id, const st_layer_desc* layers, int n_layers);
int st_destroy(st_ctx* ctx);
/* weights of one conv layer, Caffe layout (Cout, Cin, 3, 3) + bias (Cout)  [caffe.Net(weights=)] */
int st_load_conv_weights(st_ctx* ctx, const char* layer, const float* w, const float* bias);
/* 1 (default; the environment variable ST2_WINO=0 also clears it): fp32 convs whose shape allows it (reduction
 * depth % 8 == 0, >= 48 output channels; any width) run as Winograd F(2x2,3x3) on the fp32 matrix cores --
 * 2.25x fewer multiplies, same IEEE fp32 products and sums in a different association.  0: direct kernel only.
 * 2 (opt-in, round 5): as 1, and where the shape also allows it (reduction depth % 16 == 0, output channels % 64 == 0,
 * width % 4 == 0, tensors below 4 GiB) the transform-domain products are taken on the bf16 matrix cores as the six
 * exact bf16 x bf16 partial products of three-way split fp32 operands, accumulated in fp32 (conv3x3_wino_split.hip):
 * fp32-grade results (closer to a double-precision convolution than algorithm 1's), not bit-identical to them. */
int st_set_conv_algo(st_ctx* ctx, int winograd);
/* The style statistics (worker.py:109-114, 258-269) of fp32 features.  0 (default): Gram partials and style gradients on the
 * fp32 matrix cores.  1 (opt-in): where the shape allows it (whole blobs, channels % 64 == 0 from 128 up, tensors below 4 GiB) both GEMMs
 * run on the bf16 matrix cores as the six exact bf16 x bf16 partial products of three-way split fp32 operands, accumulated
 * in fp32 (gram_split.hip): fp32-grade results, not bit-identical to algorithm 0's; every other shape runs algorithm 0's
 * kernels bit for bit.  Anything else is ST_ERR_ARG.  It applies to every Gram and style gradient the context computes
 * afterwards, st_gram and the style targets of st_set_style included; targets computed earlier are kept as they are.
 * It has effect only with fp32 features: under st_set_precision(ctx, 1 | 2) the bf16 kernels keep running; and the
 * tile-sharded mode keeps the fp32 kernels whatever the option says.  A non-finite feature gives a non-finite Gram under
 * both algorithms, but entries that algorithm 0 gives as Inf may be NaN under 1 (the split forms Inf - Inf).
 * The call allocates its scratch first: when that fails it returns the error and changes nothing. */
int st_set_gram_algo(st_ctx* ctx, int algo);
/* the algorithms in force: *conv = 0 | 1 | 2 (st_set_conv_algo), *gram = 0 | 1 (st_set_gram_algo); either pointer may be NULL */
int st_get_algos(st_ctx* ctx, int* conv, int* gram);
/* Average pools (ST_LAYER_AVEPOOL).  0 (default): every average pool is a stand-alone pass over the fp32 conv blob below it, forward
 * and backward.  1 (opt-in): an average pool rides on the conv launches around it wherever a fused build exists -- the lean bf16 flow
 * of st_set_precision(ctx, 1): the epilogue of the bf16 conv below writes the pooled bf16 copy (and the fp32 pooled blob where
 * something reads it) plus one byte per window with the ReLU signs of its four elements, and does not write the fp32 conv blob; the
 * backward expands the pooled bf16 diff through that byte inside the data gradient of the same conv (at most 128 output channels,
 * even height and width) or in a pass of its own.  Same additions in the same order and power-of-two factors: loss, gradient, trace
 * and iterates are those of 0 bit for bit unless an element of a diff is smaller than 2^-124.  A pool whose conv blob carries a weight,
 * fp32 features, st_set_precision(ctx, 2) and every evaluation that writes all blobs (st_forward, st_set_content, st_set_style) route exactly as
 * under 0; tile-sharded mode refuses average pools either way.  After a lean evaluation under 1 the conv blob below a fused pool is not
 * materialised in fp32 (st_get_blob / st_gram say so), as below a fused max pool.  Anything else is ST_ERR_ARG.  The call leaves the
 * activations as they are: a backward that follows reads the map the last forward wrote, whatever the option says by then. */
int st_set_pool_algo(st_ctx* ctx, int algo);
/* the value in force: *algo = 0 | 1 */
int st_get_pool_algo(st_ctx* ctx, int* algo);
/* 0 (default): fp32 throughout.  1: bf16 feature path (BASELINE config 3) -- conv operands (activations, weights,
 * backward diffs) in bf16 on v_mfma_f32_32x32x16_bf16, fp32 accumulate; Gram, losses, optimizer stay fp32.  Objective
 * evaluations then write an fp32 blob / diff only where something reads fp32 (weighted layers, pools without a fused
 * producer, the 3-channel first layer): st_get_blob reports the others as not materialised.  2: as 1 with every fp32 blob
 * and diff written (same results bit for bit; the A/B reference of the tests; environment ST2_BF16_LEAN=0 forces it). */
int st_set_precision(st_ctx* ctx, int bf16_features);
/* CaffeModel.layers (worker.py:73-75): blob names in network order, "data" first */
int st_num_blobs(st_ctx* ctx);
const char* st_blob_name(st_ctx* ctx, int index);
int st_blob_shape(st_ctx* ctx, int index, int H, int W, int* c, int* h, int* w);

/* ---- model test hooks: CaffeModel.forward / backward (worker.py:77-106) ----------------------- */
/* runs the net on a preprocessed (1,3,H,W) image up to blob `last_blob` (-1: whole net) */
int st_forward(st_ctx* ctx, const float* x_nchw, int H, int W, int last_blob);
/* The three hooks below read the ONE activation set of the context, which every evaluation overwrites: st_forward, and the
 * forward inside st_opfunc / st_step / st_step_begin (then up to the deepest weighted blob).  They answer for the image
 * that evaluation read or fail with ST_ERR_STATE / ST_ERR_ARG naming the blob: a blob above the last one computed; a blob
 * the evaluation did not write in fp32 (the lean forward of an fp32 iteration skips pooled, un-weighted conv blobs, the
 * bf16 flow of st_set_precision(ctx, 1) every fp32 blob only bf16 convs read); any blob after st_set_content / st_set_style,
 * after the iterate was overwritten or resized (st_set_input*, st_resample_state) under an evaluation that read it. */
int st_get_blob(st_ctx* ctx, int index, float* out_chw);
/* ranged backward with per-blob diff injection after st_forward; diffs[i] is (C,h,w) of blob
 * blob_index[i]; writes d/d(data) as (3,H,W).  After a lean evaluation it fails, naming the blob, where it would read
 * an fp32 blob that evaluation did not write (a ReLU mask, the input of a pool without arg-max map). */
int st_backward(st_ctx* ctx, int n, const int* blob_index, const float* const* diffs, float* out_grad);
/* gram_matrix (worker.py:109-114) of a blob of the last st_forward: out is C*C.  Contracts the fp32 blob: refused, as
 * st_get_blob refuses it, for a blob the last evaluation did not write in fp32. */
int st_gram(st_ctx* ctx, int index, float* out);
/* Test hook: what the LAST objective evaluation (st_opfunc with or without out_grad, st_step*, or the tile-sharded phases up to
 * st_tile_losses_finish) left for blob `index` in the context's own work buffers.  Any pointer may be NULL.
 *   D      C*C    G - G_style exactly as the style-gradient launch read it (row-major, row padding stripped)
 *   raw_S  C*h*w  c2 * D @ F unscaled, c2 = float(2 / (C C n)): it exists only after the first evaluation since reset() / st_clear_norms
 *                 (tile-sharded: after st_tile_style_raw)
 *   diff   C*h*w  the injected layer diff: content + style + deep-dream terms (tile-sharded: the window's blob, zero outside the tile's region)
 *   norms  3      the c, s, d norms of the blob as that evaluation used them; 0 for a term the blob does not carry
 * It waits for the stream and copies; nothing in the context changes (no allocation, a captured step graph stays valid).  D and raw_S
 * live in ONE buffer each for all layers, so the hook refuses (ST_ERR_STATE, the message says why) rather than hand out another layer's
 * data: any pointer before an evaluation has completed, after the iterate was resized (st_set_input* / st_forward at another size,
 * st_resample_state), or for a blob that carried no weight; D or raw_S for a blob that was not the style layer evaluated last; raw_S
 * after an evaluation that knew the style norm; diff where the style term rode on the data-gradient conv above the blob (bf16 flow with
 * a gradient wanted, ST2_STYLE_FUSE: nothing was written) or after st_backward overwrote it. */
int st_get_layer_terms(st_ctx* ctx, int index, float* D, float* raw_S, float* diff, float norms[3]);
/* Test hook: tap the RUNNING diff of blob `index` (-1: off).  The diffs of a backward live in ping-pong buffers that the next launch
 * overwrites, and the bf16 flow often writes them in bf16 only; while a tap is set, every st_opfunc evaluation with out_grad enqueues --
 * right after the launch whose output is the diff of that blob -- device-to-device copies of exactly what that launch wrote (the fp32
 * diff, the channel-blocked bf16 diff [C/8][hw][8], or both) into two buffers the context owns, sized on demand.  No kernel, route or
 * plan changes: with the tap off an evaluation launches what it launched before, with it on the same launches plus the copies.  Only
 * st_opfunc honours the tap: st_step / st_step_begin are refused (ST_ERR_STATE, before anything is enqueued) while one is set, and so
 * are st_tap_diff on a tile-configured context and st_tile_configure under a tap.  st_get_tapped_diff waits for the stream and copies
 * (no epoch bump, no allocation): out32 receives C*h*w floats when *have32, out16 the ceil(C/8)*8*h*w bf16 bit patterns when *have16
 * (any pointer may be NULL).  It refuses (ST_ERR_STATE, the message names the blob) until an evaluation with a gradient whose backward
 * produced that diff has completed since the tap was set, and after the iterate was resized. */
int st_tap_diff(st_ctx* ctx, int index);
int st_get_tapped_diff(st_ctx* ctx, float* out32, uint16_t* out16, int* have32, int* have16);

/* ---- image slots: StyleTransfer.set_input / set_content / set_style (worker.py:191-218) ------- */
/* preprocess (worker.py:63-66) + upload.  is_u8: 1 = uint8 HWC, 0 = float32 HWC. */
int st_set_input(st_ctx* ctx, const void* hwc, int H, int W, int is_u8);
/* st_set_content: + forward; keeps the preprocessed image and the features of the blobs that carry a content weight at the time
 * (every blob until the first st_set_weights, like worker.py:204-209).  st_set_weights drops the features no content weight reads;
 * an evaluation whose weight table names a blob without features takes them again from the kept image first (same kernels). */
int st_set_content(st_ctx* ctx, const void* hwc, int H, int W, int is_u8);
int st_set_style(st_ctx* ctx, const void* hwc, int H, int W, int is_u8);     /* + full forward, Gram of every blob */
/* already-preprocessed NCHW variants (resample paths, worker.py:154-170) */
int st_set_input_nchw(st_ctx* ctx, const float* x, int H, int W);
int st_set_content_nchw(st_ctx* ctx, const float* x, int H, int W);
int st_get_input_nchw(st_ctx* ctx, float* out);          /* current x, (3,H,W) */
int st_input_shape(st_ctx* ctx, int* H, int* W);

/* ---- objective: StyleTransfer.set_weights / reset / opfunc (worker.py:172-175,226-301) -------- */
/* rows in DataFrame order; NaN cells allowed (treated as zero, worker.py:234). params = tv,
 * tv_power, p, p_power (messages.py:147). */
int st_set_weights(st_ctx* ctx, int n_rows, const int* blob_index, const float* content,
                   const float* style, const float* deepdream, const double params[4]);
int st_clear_norms(st_ctx* ctx);                          /* the `norms` half of reset() */
/* number of trace scalars an evaluation produces: 6 per active layer + 8 (+ 2 while st_set_laplacian is on, + 2 while st_set_anchor is, + 2 while st_set_matting is) */
int st_trace_len(st_ctx* ctx);
/* evaluates opfunc at the current input; out_grad (3,H,W) may be NULL (return_grad=False) */
int st_opfunc(st_ctx* ctx, float* out_loss, float* out_grad, double* trace);

/* ---- optimizers: optimizers.py:7-125 ------------------------------------------------------------ */
int st_optimizer_reset(st_ctx* ctx, int kind, double step_size);   /* new optimizer instance */
int st_optimizer_set_step(st_ctx* ctx, double step_size);
int st_optimizer_kind(st_ctx* ctx);
int st_objective_changed(st_ctx* ctx);
/* Adam state for the host-side resample path (optimizers.py:29-40); arrays are (3,H,W) */
int st_adam_get_state(st_ctx* ctx, float* m, float* v, int* items1, int* items2);
int st_adam_set_state(st_ctx* ctx, const float* m, const float* v, int items1, int items2);
/* one StyleTransfer.step (worker.py:303-310): optimizer step + deprocess.
 * out_hwc (H,W,3 float32) and trace may be NULL: then nothing is copied back and the call does not
 * synchronise (device-resident loop). */
int st_step(st_ctx* ctx, float* out_hwc, double* trace, float* out_loss);
/* The same iteration in two halves, for the worker loop (worker.py:380-395: step, send Iterate, poll the socket, step ...).
 * st_step_begin queues one StyleTransfer.step and the asynchronous copy of its iterate and trace into pinned host memory (own
 * stream) and returns at once; st_step_end waits for the OLDEST queued iteration and hands it over: *out_hwc points at a
 * (H,W,3) float32 array owned by the context, valid for the next FIVE calls of st_step_begin (six buffers rotate; a sender that
 * is at most four iterates behind can serialise it in place).  At most two iterations may
 * be in flight; while any is, st_step refuses.  Calling begin(k+1) before end(k) lets the GPU compute iteration k+1 while
 * iterate k crosses PCIe and is pickled -- the results are those of st_step, bit for bit. */
int st_step_begin(st_ctx* ctx);
int st_step_end(st_ctx* ctx, const float** out_hwc, int* out_h, int* out_w, double* trace, float* out_loss);
int st_step_pending(st_ctx* ctx);      /* iterations begun and not yet ended (0..2) */
/* Room for a message frame around the iterate (worker.py:351-353 sends messages.Iterate(image, i, trace) as ONE pickle, messages.py:64-74):
 * from the next st_step_begin on, the caller may write `head_bytes` in front of and `tail_bytes` behind the image st_step_end hands out
 * (same pinned allocation, same lifetime), so that the pickle's fixed header, the image the GPU copied in and the variable tail form one
 * contiguous buffer the transport sends without a host-side copy.  At most 1 MiB each; the image stays page-aligned.  Buffers replaced
 * by a re-allocation (a larger input, other rooms) stay valid for the views already handed out, for the same five further begins.
 * Refused (ST_ERR_STATE) while an iteration is in flight: its slot was sized without the room -- collect with st_step_end first. */
int st_step_frame_room(st_ctx* ctx, size_t head_bytes, size_t tail_bytes);
/* Iterate averaging: hand out a bias-corrected exponentially weighted mean of the iterates instead of the raw iterate (utils.DecayingMean,
 * utils.py:49-69, which the reference keeps for Adam's moments; crowsonkb's style_transfer CLI averages its iterates this way).  After every
 * optimizer step, Adam or L-BFGS, on the iterate x that step produced (preprocessed NCHW), in NumPy's float32 arithmetic:
 *   mean = float(decay) * mean + float(1.0 - decay) * x   (two fp32 products and one fp32 sum, no FMA; the empty mean is 0);  items += 1
 * and the image of st_step (out_hwc) and st_step_end is deprocess(mean / float(1.0 - decay ** items)): power and subtraction in double,
 * rounded once, one IEEE fp32 division, then the channel mean.  x, the optimizer state, the loss and the trace are untouched -- the
 * trajectory is that of the mode off, bit for bit -- and the raw iterate stays available from st_get_input_nchw.  st_step(ctx, NULL, ..)
 * and every st_step_begin update the mean too; begin / end give the images of st_step bit for bit, frame rooms work unchanged.
 * With an image wanted the update and the image are ONE launch in place of the deprocess pass; without, one extra launch per step.
 *   decay 0.0 (default): off, the buffer is freed, every path launches what it launched without the mode.  0 < decay < 1: on, the mean is
 *   cleared.  Anything else, NaN included: ST_ERR_ARG.  ST_ERR_STATE while a pipelined iteration is in flight.  The buffer (one image,
 *   re-created with the input buffers when the size changes) is allocated first: when that fails the call changes nothing.
 * The mean is CLEARED (items = 0) by this call, by st_optimizer_reset and by what replaces the iterate: st_set_input, st_set_input_nchw,
 * st_resample_state with new_x_nchw (and a st_forward at another size, which re-creates the input buffers); KEPT across
 * st_objective_changed, st_set_weights, st_set_content, st_set_style, st_optimizer_set_step; RESAMPLED by st_resample_state without a new
 * image: the raw mean goes through the Lanczos tables of x (the correction is a scalar and commutes), items is kept.
 * Tile-sharded mode: st_tile_step updates the mean over the whole window at its end, once that step's x and its refreshed apron are
 * final; the phase-by-phase entry points (st_tile_update, st_tile_swap, ...) do NOT update it. */
int st_set_iterate_average(st_ctx* ctx, double decay);
/* the decay in force (0: off), the item count, and the RAW, uncorrected mean (3,H,W) of the context's image (tile-sharded: the window).
 * Any pointer may be NULL; mean_nchw with items == 0 is ST_ERR_STATE. */
int st_get_iterate_average(st_ctx* ctx, double* decay, int* items, float* mean_nchw);
/* ---- the content's colours (Gatys et al., "Preserving Color in Neural Artistic Style Transfer"; no reference counterpart) ---------
 * Two independent modes, both off by default: off, every launch, result and message is what it is without them.  Throughout, x, cx and
 * s are preprocessed planar images (mean-subtracted RGB, no channel flip, as st_set_input leaves them) and kMean is the channel mean of
 * worker.py:34; fp32 arithmetic rounds once per operation (no FMA).
 * Luminance-only output: the image handed out takes its luminance from the iterate and its chroma from the content image.  Per pixel,
 * with v the iterate x (under st_set_iterate_average: v_c = mean_c / corr, the division of the averaged image):
 *   d_c = v_c - cx_c;   l = (0.299f * d_R + 0.587f * d_G) + 0.114f * d_B;   out_c = (cx_c + kMean_c) + l
 * -- "Y of the iterate, chroma of the content" in any luma / colour-difference space with Rec.601 luma (the luma column of the inverse
 * transform is (1, 1, 1)).  One launch in place of the deprocess / averaging pass, one more read stream.  The optimisation, the iterate,
 * its running mean, st_get_input_nchw and st_get_iterate_average are untouched: only the images of st_step, st_step_end,
 * st_tile_get_tile and st_tile_get_tile_average change (tile-sharded: the chroma of the window's own content).  While the mode is on,
 * st_step with an image wanted, st_step_begin, st_tile_get_tile and st_tile_get_tile_average return ST_ERR_STATE without a content
 * image or with one of another size than the input, before anything is enqueued.  ST_ERR_STATE while a pipelined iteration is in flight. */
int st_set_original_colors(st_ctx* ctx, int on);
/* Colour mean (image scale, 0..255) and population covariance (upper triangle: RR, RG, RB, GG, GB, BB) of an image, taken as st_set_style
 * would preprocess it: the nine sums of p_c and p_c p_k (c <= k) over the preprocessed values on the device, every product and addition
 * in double, per thread, per workgroup and in a second stage that adds the workgroups' partial sums in a fixed order (no atomics: the
 * same image gives the same bits); then in double on the host mean = sum / N + kMean, cov = sum_ck / N - (sum_c / N)(sum_k / N). */
int st_image_moments(st_ctx* ctx, const void* hwc, int H, int W, int is_u8, double mean[3], double cov[6]);
/* The ridge of the colour-matching transform, in this value scale (what linear colour transfer implementations add to both covariances). */
#define ST_COLOR_RIDGE (1e-5 * 255.0 * 255.0)
/* Linear colour transfer: the affine map s' = A s + b (preprocessed coordinates, A row-major) that gives the style image's pixels the
 * content image's colour mean and covariance.  With cov + ST_COLOR_RIDGE I = L L^T (Cholesky):  A = L_c L_s^-1 (a triangular solve, no
 * general inverse),  b = (mean_c - kMean) - A (mean_s - kMean); all of it 3 x 3 closed form in double, A and b rounded once to fp32.  A
 * grey style image (rank-1 covariance) is a normal input: the ridge keeps A finite.  Host only, no context.  ST_ERR_ARG: a non-finite
 * input, a covariance with a negative diagonal entry or, ridge added, without a Cholesky factor. */
int st_color_transform(const double mean_c[3], const double cov_c[6], const double mean_s[3], const double cov_s[6], float A[9], float b[3]);
/* An affine colour map for the style image: every later st_set_style, st_tile_style_partials and st_tile_set_style applies
 *   s'_c = ((A[c][0] * s_R + A[c][1] * s_G) + A[c][2] * s_B) + b[c]       (fp32, in place on the device copy, before the forward)
 * to the preprocessed style image (window).  The map is per pixel: a sharded style image needs nothing more than the same A, b on every
 * rank.  Both NULL turns it off; one NULL or a non-finite entry is ST_ERR_ARG.  Turns the colour matching below off. */
int st_set_style_transform(st_ctx* ctx, const float A[9], const float b[3]);
/* The single-context convenience: while on, st_set_style takes the moments of the kept content image and of the style image itself,
 * derives A, b as st_color_transform does and applies them; ST_ERR_STATE there without a content image.  The targets follow the content
 * image of the moment the style is set: a later st_set_content leaves them as they are, as the reference keeps its `grams`.  Refused
 * (ST_ERR_STATE) on a tile-sharded context, whose content is the window's and not the image's: derive A, b once for the whole images
 * and hand them to every rank with st_set_style_transform.  Turning it on drops a transform given by st_set_style_transform. */
int st_set_style_color_match(st_ctx* ctx, int on);
/* *original_colors = 0 | 1; *style_match = 0 (off), 1 (st_set_style_color_match) or 2 (a transform given by st_set_style_transform);
 * A, b: the transform last applied to a style image, or the one given and waiting to be (the identity and zero before either).  Any
 * pointer may be NULL. */
int st_get_color_modes(st_ctx* ctx, int* original_colors, int* style_match, float A[9], float b[3]);
/* st_set_style for an already-preprocessed (1,3,H,W) image, the sibling of st_set_input_nchw / st_set_content_nchw.  No colour
 * transform is applied: the image is what the caller gives. */
int st_set_style_nchw(st_ctx* ctx, const float* x, int H, int W);
/* Test hook: the preprocessed, recoloured image (3,H,W) exactly as st_set_style would forward it under the modes in force. */
int st_style_recolor(st_ctx* ctx, const void* hwc, int H, int W, int is_u8, float* out_nchw);
/* ---- the Laplacian-steered content term (Li, Xu, Nie, Liu: "Laplacian-Steered Neural Style Transfer", ACM MM 2017) ----------------
 * An image-space term like TV and the p-norm; no reference counterpart, this text is the definition.  With u = x / 255 and uc = cx / 255
 * (x, cx: the preprocessed planar iterate and content image) a level is a pool size p in {1, 2, 4, 8, 16, 32} and a finite non-zero
 * weight w; at most three levels, with distinct p.  Per level and channel:
 *   P(u)[i, j]   the mean of u over the window [i p, (i + 1) p) x [j p, (j + 1) p) clipped to the image, divided by the clipped window's
 *                pixel count (Caffe's AVE rule); ceil(H / p) x ceil(W / p) cells; p = 1: the identity
 *   D(q)[i, j]   sum of q[i, j] - q[n] over those of the four neighbours n that exist (the graph Laplacian of the grid: a constant gives
 *                0, nothing wraps, D is symmetric, a 1 x 1 grid gives 0)
 *   E = D(P(u)) - T with the target T = D(P(uc));  loss = w * sum E^2 over channels and cells
 *   g_lap[c, y, x] = sum over levels of w * 2 * D(E)[c, y / p, x / p] / count(y / p, x / p), the derivative with respect to u, added to
 *                the image gradient as it is: grad = ((scd + tv_w g_tv) + p_w g_p) + g_lap, one fp32 value per pixel, added last
 * fp32 arithmetic, one rounding per operation: u = x / 255 (IEEE division); a window's sum from the sums of its four quarters as
 * (a + b) + (c + d), down to single pixels, pixels outside the image counting 0; one IEEE division by the count; D accumulates
 * q - q[n] from 0 in the order up, down, left, right; E = D - T; a level's term of g_lap is (w * (2 * D(E))) / count, the levels are
 * added in their order from 0.  Sums of E^2 and g_lap^2 are taken in double per thread, fp32 per workgroup, double across workgroups.
 * The trace gains two scalars while the term is on: its image part is [scd_loss, t_loss, p_loss, l_loss, scd_grad, tv_grad, p_grad,
 * l_grad, loss, grad] with l_loss = sum over levels, in their order, of w * float(sum E^2), added to loss after p_loss, and
 * l_grad = sqrt(float(sum g_lap^2 / (3 H W))).  With the term off the trace is what it was.
 *
 * st_set_laplacian: n_levels = 0 is off, the default: the buffers are freed and every path launches what it launched before.
 * ST_ERR_ARG: a pool size outside the set, two levels with one pool size, more than three levels, a zero, NaN or infinite weight.
 * ST_ERR_STATE: while a pipelined iteration is in flight; with levels on a tile-configured context (st_tile_configure refuses a
 * context with the term on).  The buffers are allocated first: when that fails nothing has changed.  The targets are taken here when a
 * content image of the input's size exists, and again before the next evaluation whenever the content image (st_set_content*,
 * st_resample_content) or the input's size changed since.  An evaluation (st_opfunc, st_step, st_step_begin) with the term on returns
 * ST_ERR_STATE without a content image or with one of another size than the input, before anything is enqueued. */
int st_set_laplacian(st_ctx* ctx, int n_levels, const int* pool, const double* weight);
/* the levels in force; pool / weight take n_levels entries (room for 3); any pointer may be NULL */
int st_get_laplacian(st_ctx* ctx, int* n_levels, int* pool, double* weight);
/* Test hook, reads only: T (3, hp, wp) and E (3, hp, wp) of `level` (an index into the levels in force) from the last evaluation, and
 * the summed g_lap (3, H, W), the same at every level index.  Any pointer may be NULL.  ST_ERR_STATE, the message saying why: before an
 * evaluation with the term on, after the input was resized, and for grad_nchw after an evaluation without a gradient. */
int st_get_laplacian_terms(st_ctx* ctx, int level, float* target, float* diff, float* grad_nchw);
/* ---- the anchor term: a per-pixel weighted pull toward a given image ------------------------------------------------------------
 * An image-space term like TV, the p-norm and the Laplacian term; no reference counterpart, this text is the definition.  It is what
 * temporal consistency between the frames of a sequence (Ruder, Dosovitskiy, Brox: "Artistic Style Transfer for Videos", GCPR 2016:
 * the previous stylised frame, warped by the optical flow, weighted by the flow's reliability), protected regions and an
 * auxiliary-image regulariser are made of.  Symbols: u = x / 255, ua = ax / 255 (x: the preprocessed planar iterate; ax: the
 * preprocessed planar anchor image of the input's size, (3, H, W)); m: an optional (H, W) fp32 map, every value finite and >= 0,
 * shared by the three channels, absent meaning 1 everywhere; w: a weight that is finite and non-zero, as a double and as a float.
 *   d = u - ua
 *   loss  = w * sum over c, y, x of m[y, x] * d^2
 *   g_anc = w * (2 * (m * d))     the derivative with respect to u, added to the image gradient as it is (no 1 / 255 chain factor,
 *                                 like g_tv, g_p and g_lap)
 *   grad  = ((scd + tv_w g_tv) + p_w g_p) + extra,  extra = g_lap + g_anc with the Laplacian term on (one fp32 addition, g_lap
 *                                 first), else g_anc
 * fp32 arithmetic, one rounding per operation, in the order written: x / 255 and ax / 255 are IEEE divisions; e = m * d (without a
 * map there is no multiplication and e = d); the factor 2 comes next, then w as a float.  The sums of e * d (each product
 * (double)e * (double)d) and of g_anc^2 are taken in double per thread, fp32 per workgroup and double across workgroups, exactly as the
 * Laplacian term's.  While the term is on the trace gains two scalars; its image part becomes [scd_loss, t_loss, p_loss, (l_loss,)
 * a_loss, scd_grad, tv_grad, p_grad, (l_grad,) a_grad, loss, grad] with a_loss = w * float(sum e d), added to loss last, after l_loss,
 * and a_grad = sqrt(float(sum g_anc^2 / (3 H W))), 0 for an evaluation without a gradient; grad is the rms of the combined gradient.
 * With the term off every trace is what it was.
 *
 * st_set_anchor: hwc (H, W, 3), uint8 or float32, is preprocessed on the device as st_set_content's image is; hwc == NULL is off, the
 * default: every buffer of the term is freed and every path launches what it launched before.  mask_hw: H * W floats or NULL.
 * st_set_anchor_nchw takes the preprocessed planes (3, H, W) instead.
 * ST_ERR_ARG: a zero, NaN, infinite, float-underflowing or float-overflowing weight; a map value that is negative, NaN or infinite
 * (the map is scanned on the host here); H or W < 1.  ST_ERR_STATE: while a pipelined iteration is in flight; on a tile-configured
 * context (st_tile_configure refuses a context with the term on).  The buffers are allocated and filled first: when that fails
 * nothing has changed.  The anchor does not follow the input: after st_set_input* or st_resample_state to another size it stays, and
 * every evaluation (st_opfunc, st_step, st_step_begin) returns ST_ERR_STATE naming both sizes, before anything is enqueued, until an
 * anchor of the new size is set or the term is turned off. */
int st_set_anchor(st_ctx* ctx, const void* hwc, int H, int W, int is_u8, const float* mask_hw, double weight);
int st_set_anchor_nchw(st_ctx* ctx, const float* ax, int H, int W, const float* mask_hw, double weight);
/* the term in force (H = W = 0 while it is off); any pointer may be NULL */
int st_get_anchor(st_ctx* ctx, int* on, int* H, int* W, int* has_mask, double* weight);
/* Test hook, reads only: the anchor planes (3, H, W) and the map (H, W) the last evaluation read, and `extra` (3, H, W) as it left it.
 * Any pointer may be NULL.  ST_ERR_STATE, the message saying why: with the term off, before an evaluation with the term on, after the
 * input was resized, for mask_hw without a map, and for extra_nchw after an evaluation without a gradient. */
int st_get_anchor_terms(st_ctx* ctx, float* anchor_nchw, float* mask_hw, float* extra_nchw);
/* ---- the photorealism term: the matting-Laplacian regulariser ----------------------------------------------------------------------
 * An image-space term like TV, the p-norm, the Laplacian and the anchor term; no reference counterpart, this text is the definition.
 * It is the photorealism regulariser of Luan, Paris, Shechtman, Bala ("Deep Photo Style Transfer", CVPR 2017): w * sum_c u_c' L u_c with
 * L the matting Laplacian of the content image (Levin, Lischinski, Weiss: "A Closed-Form Solution to Natural Image Matting"), zero
 * exactly when every 3 x 3 window of the result is an affine function of the content's colours in that window.  L is never formed: the
 * term is evaluated matrix-free, as Levin's cost at its minimum, window by window.
 * Symbols: u = x / 255, planar (3, H, W), x the preprocessed iterate; I = cx / 255, cx the preprocessed content image of the input's
 * size (both divisions fp32 IEEE).  A window k is the 3 x 3 block centred at a pixel with 1 <= ky <= H - 2, 1 <= kx <= W - 2: only windows
 * wholly inside the image exist, so H, W >= 3, there are (H - 2)(W - 2) of them and each has nine pixels, always visited row-major
 * (dy = -1 .. 1 outer, dx = -1 .. 1 inner); every sum starts from 0 in that order.  w: finite and non-zero as a double and as a float;
 * eps in [1e-9, 1].
 * Per window, taken when the content image or the input's size changes (float64, one rounding per operation, no contraction):
 *   mu_a = (sum_i I_a,i) / 9;  dI_a,i = I_a,i - mu_a;  s_ab = (sum_i dI_a,i * dI_b,i) / 9 (a <= b);  eps / 9 is added to s_00, s_11, s_22;
 *   c00 = s11 s22 - s12 s12; c01 = s02 s12 - s01 s22; c02 = s01 s12 - s02 s11; det = (s00 c00 + s01 c01) + s02 c02;
 *   c11 = s00 s22 - s02 s02; c12 = s01 s02 - s00 s12; c22 = s00 s11 - s01 s01;  M_ab = c_ab / det.
 *   Stored: mu (3) and M (6), each rounded once to fp32; I as three fp32 planes.
 * Per evaluation, first pass (per window k and channel c of u; fp32, one rounding per operation, in the order written):
 *   pb = (sum_i u_i) / 9;  dp_i = u_i - pb;  dI_a,i = I_a,i - mu_a (the stored fp32 mu);  cov_a = (sum_i dI_a,i * dp_i) / 9;
 *   a_a = (M_a0 cov_0 + M_a1 cov_1) + M_a2 cov_2;  r_i = dp_i - ((a_0 dI_0,i + a_1 dI_1,i) + a_2 dI_2,i);
 *   J = (sum_i (double)r_i * (double)r_i) + eps * (((double)a_0 * a_0 + (double)a_1 * a_1) + (double)a_2 * a_2), all in double.
 *   a_0, a_1, a_2, pb are written per window and channel.  A workgroup of 256 threads takes tiles of 64 x 4 windows, thread t the window
 *   (t / 64, t % 64) of its tile, and walks the tiles (row-major) block, block + grid, ... with grid = min(tiles, 1024); a thread adds its
 *   J (channel 0, 1, 2 of a window, tile after tile) in double, the workgroup's sum is fp32 (the wave and workgroup trees of the other
 *   terms), the sum across workgroups double -- exactly as the Laplacian and anchor terms do.
 * Second pass, only with a gradient (per pixel i and channel c):
 *   Lu_i = sum of r_ik over the existing windows k that contain i (ky = y - 1 .. y + 1, kx = x - 1 .. x + 1 clipped to the valid
 *   centres, row-major, from 0), r_ik recomputed by the expression above from the stored a, pb, mu and the pixel's u, I: the same bits.
 *   g_mat = w * (2 * Lu_i): the factor 2 first, then w as a float; the derivative with respect to u, added to the image gradient as it
 *   is (no 1 / 255 chain factor, like g_tv, g_p, g_lap, g_anc).
 *   grad = ((scd + tv_w g_tv) + p_w g_p) + extra,  extra = prev + g_mat (one fp32 addition, prev first) with prev what extra was without
 *   this term (g_lap, g_anc or g_lap + g_anc); extra = g_mat when neither other term is on.  The sums of g_mat^2 go over tiles of
 *   64 x 4 pixels the same way (channel 0, 1, 2 of a pixel).
 * While the term is on the trace gains two scalars; its image part becomes [scd_loss, t_loss, p_loss, (l_loss,) (a_loss,) m_loss,
 * scd_grad, tv_grad, p_grad, (l_grad,) (a_grad,) m_grad, loss, grad] with m_loss = w * float(sum J), added to loss last, after a_loss,
 * and m_grad = sqrt(float(sum g_mat^2 / (3 H W))), 0 for an evaluation without a gradient; grad is the rms of the combined gradient.
 * With the term off every trace is what it was.  Jitter does not touch the term: it reads the unshifted iterate and content image.
 *
 * st_set_matting: weight == 0 is off, the default: every buffer of the term is freed and every path launches what it launched before.
 * ST_ERR_ARG: a NaN, infinite, float-underflowing or float-overflowing weight; eps outside [1e-9, 1].  ST_ERR_STATE: while a pipelined
 * iteration is in flight; on a tile-configured context (st_tile_configure refuses a context with the term on).  The buffers are
 * allocated first: when that fails nothing has changed.  The per-window data are taken here when a content image of the input's size
 * exists, and again before the next evaluation whenever the content image (st_set_content*, st_resample_content) or the input's size
 * has changed since.  An evaluation (st_opfunc, st_step, st_step_begin) with the term on returns ST_ERR_STATE, the sizes named, before
 * anything is enqueued: without a content image, with one of another size than the input, and with H < 3 or W < 3. */
int st_set_matting(st_ctx* ctx, double weight, double eps);
/* the term in force; any pointer may be NULL */
int st_get_matting(st_ctx* ctx, int* on, double* weight, double* eps);
/* Test hook, reads only: mu (3, H - 2, W - 2), M (6, H - 2, W - 2) in the order 00 01 02 11 12 22, a_pb (3, 4, H - 2, W - 2) as the
 * last evaluation's first pass left it, and `extra` (3, H, W) as its second pass did.  Any pointer may be NULL.  ST_ERR_STATE, the
 * message saying why: with the term off, before an evaluation with the term on, after the input was resized, and for extra_nchw after
 * an evaluation without a gradient. */
int st_get_matting_terms(st_ctx* ctx, float* mu, float* M, float* a_pb, float* extra_nchw);
/* Which optional image-space terms are on, in the order the trace lists them (1 or 0 each; any pointer may be NULL): what a caller needs
 * to name the scalars of the image part, whose length alone does not say.  Reads host state only. */
int st_get_trace_terms(st_ctx* ctx, int* laplacian, int* anchor, int* matting);
/* ---- frame sequences: earlier iterates kept on the device, warped into the iterate and into the anchor -----------------------------
 * What the seam between two frames of a stylised sequence needs (Ruder, Dosovitskiy, Brox: "Artistic Style Transfer for Videos", GCPR
 * 2016): the next frame starts from the previous stylised frame warped by the optical flow and is pulled toward it by the anchor term
 * above, weighted by the flow's reliability; regions that were covered for a few frames are pulled toward an older frame (the
 * long-term loss, which for 0 / 1 maps is ONE anchor term whose image and map are composed per pixel from several frames).  No
 * reference counterpart, this text is the definition; jobs.warp_planar and tests/frames_oracle.py restate it in NumPy.
 *
 * The store.  st_frames_keep: depth 0 (default) .. 8 earlier iterates are kept; a smaller depth drops the oldest beyond it, 0 frees every
 * buffer of the block; anything else is ST_ERR_ARG.  st_frame_push: the current RAW iterate x (the preprocessed planes of
 * st_get_input_nchw, never the averaged or recoloured image handed out) becomes frame 1, frames 1.. become 2.., the oldest beyond the
 * depth is dropped; ST_ERR_STATE with depth 0 or without an input; a push at another size than the kept frames' drops those first.
 * st_get_frames: the depth, the number of frames held and their size (0 x 0 while none is); any pointer may be NULL; it reads only.
 *
 * Flows are H * W * 2 host floats (dx, dy) in pixels, of the input's size: `bwd` from the frame being stylised back to frame j, `fwd`
 * from frame j to the frame being stylised.  They are scanned on the host, as the anchor's map is: a non-finite entry is ST_ERR_ARG.
 * Frame index: j < 1 or j > depth is ST_ERR_ARG; an empty slot, or kept frames of another size than the input's (or no input), is
 * ST_ERR_STATE naming both sizes.
 *
 * Warp  W(P, f)  of planes P (H, W) by a flow f, every operation in double and rounded once, no contraction, in this order:
 *   sx = min(max(x + dx, 0), W - 1), sy likewise;  x0 = floor(sx), x1 = min(x0 + 1, W - 1), fx = sx - x0, y0, y1, fy likewise
 *   top = P[y0, x0] * (1 - fx) + P[y0, x1] * fx;  bottom = P[y1, x0] * (1 - fx) + P[y1, x1] * fx;  out = float(top * (1 - fy) + bottom * fy)
 * -- jobs.warp_planar, bit for bit.
 * Reliability  c(bwd, fwd),  in double from the float inputs.  At (y, x): (u, v) = bwd[y, x]; (wx, wy) = W(fwd's two planes, bwd)[y, x],
 * rounded to float as the warp is.  c = 0 where any of
 *   outside      x + u < 0, x + u > W - 1, y + v < 0 or y + v > H - 1      (the unclamped sample point leaves the image)
 *   disoccluded  (wx + u)^2 + (wy + v)^2 > 0.01 * ((wx^2 + wy^2) + (u^2 + v^2)) + 0.5
 *   boundary     (ux^2 + uy^2) + (vx^2 + vy^2) > 0.01 * (u^2 + v^2) + 0.002,  forward differences clamped to the image:
 *                ux = bwd[y, min(x + 1, W - 1)].u - u,  uy = bwd[min(y + 1, H - 1), x].u - u,  vx, vy likewise
 * holds, else 1 (Ruder et al.'s inequalities; the difference scheme and the "outside" rule are this text's).  fwd == NULL: c = 1
 * everywhere.  With mask_hw (the anchor map's rules: finite, >= 0, scanned on the host) c becomes float(c * mask).  bwd == NULL is no
 * warp: W(P, NULL) = P, and (u, v) = 0 in the tests above.
 *
 * st_set_input_from_frame: x = W(frame j, bwd); everything else of the state is what st_set_input_nchw of those planes leaves (the
 * iterate average is cleared, captured graphs are stale, nothing is re-made at the equal size).
 * st_anchor_from_frame, accumulate == 0: the anchor planes are W(frame j, bwd), the map is c when fwd or mask_hw is given and absent
 * otherwise, the term is on with `weight` (st_set_anchor's rules) -- afterwards every observer (st_get_anchor, st_get_anchor_terms,
 * st_trace_len, every evaluation) answers as after st_set_anchor_nchw of those planes and that map.  The buffers are made and filled
 * first: when that fails nothing has changed.  accumulate == 1 (the long-term term) needs the term on at the input's size with a map
 * (else ST_ERR_STATE) and `weight` equal to the weight in force (else ST_ERR_ARG), and composes per pixel, in float:
 *   m = max(c - M, 0);   ax = m > 0 ? W(frame j, bwd) : ax  (the three channels);   M = M + m
 * so that calls in the order j = 1, 2, 4, .. give every pixel the newest frame that reliably shows it.  Warp, reliability, map product
 * and composition are ONE launch per call.
 * Every call of the block but st_get_frames bumps the epoch and is refused (ST_ERR_STATE) while a pipelined iteration is in flight and
 * on a tile-configured context (where st_frames_keep(ctx, 0) stays allowed). */
int st_frames_keep(st_ctx* ctx, int depth);
int st_frame_push(st_ctx* ctx);
int st_get_frames(st_ctx* ctx, int* depth, int* count, int* H, int* W);
int st_set_input_from_frame(st_ctx* ctx, int j, const float* bwd_flow_hw2);
int st_anchor_from_frame(st_ctx* ctx, int j, const float* bwd_flow_hw2, const float* fwd_flow_hw2, const float* mask_hw, double weight,
                         int accumulate);
/* ---- optical flow: the flows of the frames block, estimated on the device -------------------------------------------------------
 * A dense estimator for callers who have only frames: coarse-to-fine Horn-Schunck with warping and Jacobi inner iterations (Horn,
 * Schunck: "Determining Optical Flow", 1981; the warping scheme of Brox et al., ECCV 2004, with the quadratic penalties).  Every block
 * is a stencil, so tests/flow_oracle.py restates it in NumPy bit for bit.  No reference counterpart; this text is the definition.
 * All arithmetic is float32: one rounding per operation, no contraction, IEEE division, operations in the order written.
 *
 * estimate(from, to) = f = (dx, dy) per pixel of `from` with from(p) ~ to(p + f(p)): with from = frame t and to = frame t - j it is the
 * `bwd` flow of the frames block, with from = frame t - j and to = frame t the `fwd` flow.
 *   luma      g = ((0.299f R + 0.587f G) + 0.114f B) / 255f             per pixel of an H x W x 3 image, uint8 or float32 on the 0 .. 255 scale
 *   pyramid   level 0 = g; level l + 1 = the 2 x 2 / stride 2 average of level l in Caffe's ceil mode, ((a + b) + (c + d)) / count with
 *             pixels outside counting 0 and count the clipped window's size (4, 2 or 1): the P(u) of the Laplacian block at p = 2.
 *             levels = 0: pool while min(h, w) >= 32 and fewer than 12 levels exist; levels = L (1 .. 12): pool L - 1 times, stopping
 *             early at a 1 x 1 level.  After the pyramid is built from the unsmoothed planes, every level of both images is smoothed
 *             once, borders replicated:  t = ((g[x-1] + g[x+1]) + 2f g) 0.25f along x, then the same along y on t
 *   start     u = v = 0 at the coarsest level; moving to a finer level (h x w): u[y, x] = 2f u_coarse[y >> 1, x >> 1], v likewise
 *   per level, `warps` times, with A the `from` level and B the `to` level:
 *     Bw  = bilinear(B, x + u, y + v): sample coordinates (float)x + u clamped to [0, w - 1], x0 = floor, x1 = min(x0 + 1, w - 1),
 *           fx = sx - x0, gx = 1f - fx (y likewise); top = B00 gx + B01 fx, bottom = B10 gx + B11 fx, Bw = top gy + bottom fy
 *     Ix  = 0.5f (Bw[x+1] - Bw[x-1]), Iy likewise, indices clamped
 *     c   = ((Bw - A) - Ix u) - Iy v
 *     den = (a2 + Ix Ix) + Iy Iy,  a2 = float(alpha) float(alpha)
 *     then `iters` Jacobi iterations, each reading the previous iterate only:
 *       ub = ((u[y-1] + u[y+1]) + (u[x-1] + u[x+1])) 0.25f, indices clamped; vb likewise
 *       r  = ((Ix ub + Iy vb) + c) / den;   u' = ub - Ix r,  v' = vb - Iy r
 *   result    (u, v) of level 0, interleaved as (H, W, 2)
 * Defaults (params == NULL): alpha 0.06, warps 3, iters 40, levels 0.  The limit: a pyramid resolves motion of a few pixels at its
 * coarsest level, so at 96 x 128 (three levels) shifts of up to about 4 pixels are recovered to a few hundredths of a pixel, while a
 * shift of (12, -9) is beyond it (mean error 3.8 px); larger frames have more levels and reach proportionally further.
 *
 * st_flow_estimate uploads the two images, runs on the engine's stream, waits, and copies the flow out.  It reads and writes nothing of
 * the iterate, the optimizer, the anchor, the kept frames or the activations, and bumps no epoch: hooks and captured graphs stay valid.
 * It is allowed on a tile-configured context.  Its scratch is sized on demand and kept until st_flow_release, st_destroy or a larger
 * request; when the allocation fails nothing has changed.  route: a test switch, 0 automatic (levels of up to 4096 pixels run all the
 * Jacobi iterations of a warp in one launch of one workgroup), 1 one launch per Jacobi iteration at every level; the bits are the same.
 * ST_ERR_ARG: a NULL image or output; H or W < 1; levels outside 0 .. 12, warps outside 1 .. 16, iters outside 1 .. 1000; alpha
 * non-finite or outside [1e-6, 1e3]; route outside {0, 1}; a non-finite value in a float32 image (scanned on the host).  ST_ERR_STATE:
 * a pipelined iteration is in flight.  A refused call enqueues nothing.
 * st_get_flow_level (test hook, reads only): the size of one level of the last estimate, its smoothed planes (h w floats each) and its
 * finished flow (h w 2); any pointer may be NULL.  ST_ERR_STATE before an estimate or after a release, ST_ERR_ARG for a level that
 * does not exist. */
typedef struct st_flow_params { int levels, warps, iters; double alpha; int route; } st_flow_params;
int st_flow_estimate(st_ctx* ctx, const void* from_hwc, const void* to_hwc, int H, int W, int is_u8, const st_flow_params* params,
                     float* out_flow_hw2);
int st_flow_release(st_ctx* ctx);
int st_get_flow_level(st_ctx* ctx, int level, int* h, int* w, float* from_l, float* to_l, float* flow_l_hw2);
/* ---- jitter: the network terms evaluated on a randomly rolled iterate ---------------------------------------------------------
 * Pool windows, Winograd output tiles and the stride-16 grid of the deep layers sit at the same pixels in every iteration; the regular
 * grid artefacts of DeepDream and Gram-matrix style transfer come from that.  With the mode on, every evaluation shows the network the
 * iterate rolled by a small shift s = (dy, dx) and rolls the gradient back.  No reference counterpart; this text is the definition.
 *   roll(P, (dy, dx))[c, y, x] = P[c, (y - dy) mod H, (x - dx) mod W]      (np.roll(P, (dy, dx), (1, 2)); any integers), unroll = roll by -s
 *   x_s   = roll(x, s)                    x: the preprocessed planar iterate (3, H, W), never moved itself
 *   F_c,s = content features of roll(cx, s), cx the kept preprocessed content image -- taken by exactly the launches st_set_content_nchw
 *           of those planes would use, only when an active row carries a content weight, and kept while the shift stays
 *   scd_loss_s, the per-layer losses, the norms = worker.py:239-279 at x_s against F_c,s and the (unshifted) style targets
 *   scd   = unroll(d scd_loss_s / d x_s)  what the image pass receives as the network gradient
 * TV (periodic) and the p-norm (pointwise) are roll-invariant; they, the Laplacian and the anchor term, Adam / L-BFGS, the iterate
 * average, emission, frames and resampling read and write the unshifted x, in the order and arithmetic they have without the mode.  The
 * trace keeps its length and layout; its layer entries and scd_* are those of the shifted evaluation.  With no active row nothing is
 * rolled.  The two rolls are launches of roll_k (jitter.hip), a pure move: 2 x 25.2 MB at 1024^2.  scd_grad, the RMS of the network
 * gradient, is summed over the planes before the un-roll in the image pass's own order (roll_sumsq_k), so that every layer entry and
 * scd_* of the trace have the bits of a mode-off evaluation that is given roll(x, s) and roll(cx, s).
 * Measured at 1024^2 (VGG19, Adam, fp32; profiles/jitter_1024.txt): roll_k 9.0 us per launch (2.8 TB/s); with style rows only 21 us
 * per 6.98 ms step (0.30 %); with a content row at conv4_2 and a shift that changes every step, one more forward to conv4_2 per step:
 * 2.46 ms per 7.00 ms step (35 % more time).  A shift that stays (st_set_jitter_shift) pays that forward once.
 * The shift of step k, in 64-bit unsigned wrap-around arithmetic (splitmix64, output k + 1 from state `seed`):
 *   mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *   r_k = mix(seed + (k + 1) * 0x9E3779B97F4A7C15)
 *   dy_k = (int)((r_k >> 32) % (2R + 1)) - R;      dx_k = (int)((r_k & 0xFFFFFFFF) % (2R + 1)) - R
 * Pinned: r_0..2 for seed 1234567 = 6457827717110365317, 3203168211198807973, 9817491932198370423 (the published splitmix64 vectors);
 *   (dy, dx) for seed 7, R 3, k = 0..7 = (-1,-2) (-1,-1) (-2,0) (-2,3) (-3,2) (-3,3) (-3,2) (2,-2); seed 0, R 16, k = 0..5 = (5,0) (16,9)
 *   (-9,-10) (-6,2) (5,6) (9,-2); seed 2^64 - 1, R 1024, k = 0..3 = (-548,1001) (-1010,873) (-210,611) (-662,-816).
 * k is host state: the optimizer steps begun since the last st_set_jitter, st_set_jitter_shift or st_optimizer_reset.  st_step and
 * st_step_begin use shift k for EVERY evaluation of the step (L-BFGS's first step evaluates twice, with one shift), then k += 1;
 * st_opfunc uses shift k and leaves k alone.
 * L-BFGS caveat: from its second step on the optimizer forms its curvature pair from gradients of two consecutive shifts,
 * y = g(x_{k+1}; s_{k+1}) - g(x_k; s_k), as the predecessor CLI did: y then holds the change of the objective as well as that of the
 * iterate.  Nothing guards against it but the s.y > 1e-10 gate the optimizer has anyway; Adam has no such memory.
 * While the mode is on: st_get_blob, st_get_layer_terms and st_tap_diff answer in the shifted coordinates of the evaluation they
 * describe; steps are never replayed as a hipGraph (the shift is a per-step argument).  The engine tracks the shift the kept content
 * features belong to and takes them again before the next evaluation that needs another -- also back to (0, 0) after the mode goes off.
 * st_set_jitter: radius 0 turns the mode off (the default) and frees every buffer of it; every path then launches what it launched
 *   before.  ST_ERR_ARG: radius < 0 or > 4096.  ST_ERR_STATE: a pipelined iteration in flight; a tile-configured context
 *   (st_tile_configure in turn refuses a context with the mode on).  Buffers are allocated first: when that fails nothing has changed.
 * st_set_jitter_shift: the mode on with this shift held for every evaluation (any integers); k still counts.  Same refusals.
 * Both bump the epoch and zero k.
 * st_get_jitter: any pointer may be NULL.  dy, dx: what the next evaluation will use (0, 0 with the mode off).
 * st_get_jitter_terms (test hook, reads only): xs_nchw: the planes the last evaluation's forward read; scd_nchw: the un-rolled network
 *   gradient it handed to the image pass; dy, dx: the shift it used, as drawn or given (not reduced).  ST_ERR_STATE with a reason: the
 *   mode off; no evaluation yet; after a resize; an evaluation without an active row; scd after one without gradient. */
int st_set_jitter(st_ctx* ctx, int radius, unsigned long long seed);
int st_set_jitter_shift(st_ctx* ctx, int dy, int dx);
int st_get_jitter(st_ctx* ctx, int* radius, unsigned long long* seed, long long* k, int* pinned, int* dy, int* dx);
int st_get_jitter_terms(st_ctx* ctx, float* xs_nchw, float* scd_nchw, int* dy, int* dx);
/* Steps so far that ran as a hipGraph replay.  Opt-in (environment ST2_GRAPH=1; ST2_GRAPH_MAX_PX=<edge>, default 768):
 * steady-state Adam steps are captured once per ping-pong parity and replayed, bit-identical to plain launches.  Measured
 * on MI355X it is no faster (the step is bound by the dependent kernels' execution latency), hence off by default. */
int st_graph_replays(st_ctx* ctx, long long* n);
/* Test hook for LBFGSOptimizer.inv_hv (optimizers.py:89-108): p = H g by the device two-loop recursion for a given
 * history of n_pairs <= 10 (s, y) pairs, oldest first, each a (3,H,W) array of the current input geometry with
 * s.y > 1e-10; nothing is applied to the iterate.  Replaces the optimizer's history (the next step starts empty). */
int st_lbfgs_inv_hv(st_ctx* ctx, int n_pairs, const float* const* s, const float* const* y, const float* g, float* out_p);
int st_sync(st_ctx* ctx);
/* Test hook: device and pinned host memory the engine holds right now, in requested bytes, over EVERY context of the process
 * (no context argument).  Every allocation of the engine passes one funnel that counts it; after st_destroy of all contexts
 * both figures are what they were before the first st_create.  Either pointer may be NULL. */
int st_live_bytes(long long* device, long long* pinned);

/* ---- measurement ----------------------------------------------------------------------------------- */
/* per-kernel-class HIP-event timing on the engine's own stream */
int st_profile_enable(st_ctx* ctx, int on);
int st_profile_num_classes(void);
const char* st_profile_class_name(int cls);
/* sums since the last call: launches, milliseconds, algorithmic FLOPs and bytes per class */
int st_profile_read(st_ctx* ctx, long long* launches, double* ms, double* flops, double* bytes);

/* ---- device-resident resampling: optimizer.resample / StyleTransfer.resample_content ------------------------
 * (optimizers.py:29-40,110-119; worker.py:154-170; utils.py:130-160 = Pillow Image.resize on float planes).
 * A table describes one axis exactly as Pillow's precompute_coeffs does (host-computed): for output index i the
 * window starts at lo[i], has n[i] taps, coefficients k[i*kmax .. ] (double, normalised). */
typedef struct st_resample_table { const int* lo; const int* n; const double* k; int kmax; int out_size; } st_resample_table;
/* Resamples the optimizer state to (lan_y.out_size x lan_x.out_size): x by Lanczos (or replaced by new_x_nchw when not
 * NULL), Adam's m by Lanczos, Adam's v by bilinear then max(0, .); L-BFGS: x only (the caller then signals
 * objective_changed).  bil_* may be NULL for L-BFGS. */
int st_resample_state(st_ctx* ctx, const st_resample_table* lan_x, const st_resample_table* lan_y,
                      const st_resample_table* bil_x, const st_resample_table* bil_y, const float* new_x_nchw);
/* Resamples the preprocessed content image by Lanczos and recomputes the content features. */
int st_resample_content(st_ctx* ctx, const st_resample_table* lan_x, const st_resample_table* lan_y);
int st_get_content_nchw(st_ctx* ctx, float* out, int* H, int* W);   /* out may be NULL to query the shape */

/* ---- tile-sharded single image (BASELINE config 5; style_transfer2_amd/tiling.py) ------------------------------------
 * One context = one rank's window (tile + apron) of a gH x gW image.  No reference counterpart: the reference
 * runs one image per worker; its numerics (global Gram normalisation worker.py:114, global RMS norms :254,266,275,
 * periodic TV utils.py:232-254) fix what must be reduced/exchanged.  Phases of one Adam iteration; the caller
 * all-reduces the returned device buffers (RCCL) and exchanges gradient / image strips between them:
 *   st_tile_forward -> [AR p1] -> st_tile_losses -> (first eval: st_tile_style_raw -> [AR p2]) -> st_tile_losses_finish
 *   -> st_tile_backward -> [overlap-add window gradient] -> st_tile_update(ring) -> [AR p3] -> [apron refresh] -> st_tile_swap
 * p1 = per active layer {sum d^2, sum gc^2, sum F^2, sum gd^2} (+ C*C raw Gram sums for style layers), p2/p3 tail =
 * sum S^2 per style layer, p3 head = {tv, p, scd^2, tvg^2, pg^2, grad^2} sums over the tile. */
int st_tile_configure(st_ctx* ctx, int gH, int gW, int wy0, int wx0, int ty0, int tx0, int ty1, int tx1);
int st_tile_forward(st_ctx* ctx, float** dev_ptr, int* n_floats);
int st_tile_losses(st_ctx* ctx, float** dev_ptr, int* n_floats);
int st_tile_style_raw(st_ctx* ctx);
int st_tile_losses_finish(st_ctx* ctx);
int st_tile_backward(st_ctx* ctx, float** dev_grad);
int st_tile_update(st_ctx* ctx, const float* ring_dev, float** dev_ptr, int* n_floats);
/* st_tile_update without the optimizer: the combined gradient (network + TV + p-norm) of the tile's pixels is written to the
 * window-sized gradient buffer (st_tile_buffer 4), the six partial sums (+ style-gradient sums) come back as from st_tile_update.
 * The tile-sharded L-BFGS (optimizers.py:62-108 with all-reduced dot products) evaluates its objective through this. */
int st_tile_gradient(st_ctx* ctx, const float* ring_dev, float** dev_ptr, int* n_floats);
/* utils.dot / utils.axpy (utils.py:29-47) on vectors the caller keeps on this device: out_dev[0] = sum a b (this rank's partial
 * sum, to be all-reduced); y = alpha x + y.  Both return when the result is in place. */
int st_vec_dot(st_ctx* ctx, const float* a_dev, const float* b_dev, long long n, float* out_dev);
int st_vec_axpy(st_ctx* ctx, float alpha, const float* x_dev, float* y_dev, long long n);
/* y = float(double(y) / divisor): `p /= np.sqrt(dot(p, p) / p.size)` of optimizers.py:99 divides by a float64 scalar */
int st_vec_div(st_ctx* ctx, double divisor, float* y_dev, long long n);
/* which: 0 current x (3,wh,ww), 1 next x, 2 local sum D^2 per style layer, 3 norms [blob][c,s,d], 4 gradient (3,wh,ww) */
int st_tile_buffer(st_ctx* ctx, int which, float** dev_ptr);
int st_tile_swap(st_ctx* ctx);
/* strips exchanged with ONE neighbour: rects [n][4] = {y0, x0, h, w} (window coordinates, n <= 12) of the (C, wh, ww) device
 * tensor <-> one contiguous device buffer (rect r stored as (C, h_r, w_r), in order).  mode 0 pack, 1 unpack, 2 unpack-add. */
int st_tile_strips(st_ctx* ctx, void* tensor_dev, int C, int wh, int ww, int n, const int* rects, void* buf_dev, int mode);


/* ---- the tile-sharded iteration with its communication inside the engine (BASELINE config 5: "RCCL halo exchange over xGMI") -----
 * The phases above leave the collectives to the caller.  Here the engine owns them: one RCCL communicator per context, the two
 * all-reduces and the three strip exchanges of an Adam iteration are enqueued on the engine's own stream between the compute phases
 * (ncclAllReduce in place on the phase buffers; one grouped ncclSend / ncclRecv per neighbour and phase on packed strip buffers), and
 * the host synchronises once per iteration, to read the trace.  No reference counterpart (the reference runs one image per worker);
 * what must cross ranks is fixed by worker.py:114 (global Gram normalisation), :254,266,275 (global RMS norms) and utils.py:232-254
 * (periodic TV).  The geometry and the exchange plan come from the caller (style_transfer2_amd/tiling.py). */
#define ST_COMM_ID_BYTES 128
int st_comm_unique_id(char out_id[ST_COMM_ID_BYTES]);                       /* ncclGetUniqueId: on rank 0, then handed to every rank */
/* ncclCommInitRank on the context's device.  Preflight first, so that a mis-launch is an error here and not a hang in the first
 * collective: RCCL >= 2.7 (grouped send / recv), every peer of a plan already handed over < world (world = rows x cols of the grid);
 * devices without direct peer access are reported on stderr. */
int st_comm_init(st_ctx* ctx, const char id[ST_COMM_ID_BYTES], int rank, int world);
/* A caller-supplied transport in place of RCCL (the tests run several ranks on ONE GPU, which RCCL refuses): allreduce sums `n` floats
 * in place over the ranks; exchange sends send_buf[i] (send_count[i] floats) to send_peer[i] and fills recv_buf[j] from recv_peer[j].
 * All buffers are device memory; the engine has synchronised its stream before the call and the data must be in place on return. */
typedef int (*st_allreduce_fn)(void* user, float* dev_buf, int n);
typedef int (*st_exchange_fn)(void* user, int n_send, const int* send_peer, float* const* send_buf, const int* send_count,
                              int n_recv, const int* recv_peer, float* const* recv_buf, const int* recv_count);
int st_comm_callbacks(st_ctx* ctx, int rank, int world, st_allreduce_fn allreduce, st_exchange_fn exchange, void* user);
int st_comm_destroy(st_ctx* ctx);
int st_comm_barrier(st_ctx* ctx);                                            /* all-reduce of one float + stream synchronisation */
/* The strips this rank exchanges in one phase.  rects are [n][4] = {y0, x0, h, w}: send rects in the coordinates of the tensor packed
 * (the window), recv rects in those of the tensor unpacked into (the window; the (3, th + 2, tw + 2) ring for ST_TILE_PLAN_RING).
 * A peer equal to the own rank (ring phase only: the image's periodic wrap may land on this rank's own tile) is a local copy;
 * its send and recv rects pair up one to one. */
enum { ST_TILE_PLAN_OVERLAP = 0, ST_TILE_PLAN_RING = 1, ST_TILE_PLAN_REFRESH = 2 };
typedef struct st_tile_peer { int peer; int n_send; const int* send_rects; int n_recv; const int* recv_rects; } st_tile_peer;
int st_tile_plan(st_ctx* ctx, int phase, int n_peers, const st_tile_peer* peers);
/* One iteration of the tile-sharded image with the optimizer st_optimizer_reset chose (after st_tile_configure, st_comm_init /
 * st_comm_callbacks and the three st_tile_plan calls).
 * Adam (optimizers.py:20-27): forward -> all-reduce -> losses (first evaluation: style gradients raw -> all-reduce) -> backward ->
 * overlap-add exchange -> ring exchange -> TV / p-norm / Adam on the tile -> all-reduce -> apron refresh exchange -> swap.
 * L-BFGS (optimizers.py:62-108, the reference's default: worker.py:135-136): every rank keeps its tile of x, of the gradient and of the
 * <= 10 curvature pairs; the direction is formed in the Gram form (coefficients from the matrix of inner products of {s_i, y_i, g}):
 * apply s = -step * H g to the tile -> apron refresh exchange -> the evaluation above with the combined gradient in place of the Adam
 * update -> ONE all-reduce of this step's 2 (2 k + 3) new inner products -> the s.y > 1e-10 gate, eviction and the next coefficients,
 * identically on every rank.  The first step after a reset evaluates twice (optimizers.py:64-65).
 * trace: st_trace_len(ctx) values, the layout of st_step's; NULL: nothing is read back and the call does not wait for the GPU.  The
 * collective sequence is the same either way (round 5: the few KB of image-space sums that only the trace reads are reduced on every
 * call), so ranks may choose NULL independently of each other. */
int st_tile_step(st_ctx* ctx, double* trace);
/* The trace of the last complete evaluation of the tile-sharded image, finished from the reduced sums in the reference's fp32 order
 * (worker.py:249-301: the per-layer losses and gradient RMS values, the scd / tv / p losses, the total): st_trace_len(ctx) values, the
 * layout of st_step's.  st_tile_step finishes its trace through it; a caller that drives the phases itself calls it once p1, p2 (first
 * evaluation) and p3 are all-reduced in place -- the device buffers stay valid until the next st_tile_forward, and every rank then
 * finishes the same numbers.  Waits for the engine's stream.  ST_ERR_STATE before st_tile_configure, and until an evaluation has reached
 * st_tile_update / st_tile_gradient under the current weights. */
int st_tile_trace(st_ctx* ctx, double* trace);
int st_tile_get_tile(st_ctx* ctx, float* out_hwc);                           /* this rank's tile of the current iterate, (th, tw, 3) deprocessed */
/* this rank's tile of the corrected, deprocessed iterate average (st_set_iterate_average), (th, tw, 3): mean / corr + channel mean on the
 * packed tile, the arithmetic of st_step's averaged image.  ST_ERR_STATE when the mode is off or the mean is empty (only st_tile_step
 * updates it).  st_tile_get_tile keeps returning the raw iterate. */
int st_tile_get_tile_average(st_ctx* ctx, float* out_hwc);

/* ---- the style targets of a tile-sharded job, sharded as well -------------------------------------------------------------------
 * st_set_style forwards the WHOLE style image on the context that calls it; in a sharded job every rank would repeat that pass, and the
 * style image would have to fit one engine.  Here the style image has a tile grid of its own (tiling.style_grid: edges on multiples of
 * the total stride of `last_blob`, the deepest blob whose Gram is wanted; apron = its receptive reach).  Each rank forwards only its
 * window -- a feature inside the tile is then what the whole-image forward computes -- and contracts F F^T over the tile's region of
 * blobs 0 .. last_blob; the raw sums are added over the ranks and divided by the GLOBAL C h w (worker.py:114).
 *   hwc, H, W, is_u8: this rank's window of the gH x gW style image, as st_set_style takes an image; hwc == NULL: this rank has no style
 *   tile and contributes zeros (H, W and the geometry after gW are ignored).  (wy0, wx0): origin of the window; [ty0, ty1) x [tx0, tx1): the
 *   tile; global pixels.  ST_ERR_ARG: a window outside the image, a tile outside the window or empty, an origin or inner edge that is no
 *   multiple of last_blob's total stride, a net with an average pool at or below last_blob.
 * The window is forwarded (every fp32 blob written) in an activation set of its own unless it has the iterate's size, exactly as
 * st_set_style does; the iterate, the content features and st_tile_configure's geometry are not touched, and none of them is needed.
 * The Gram partials are the fp32 region-of-interest kernel on the fp32 blob under every st_set_precision and st_set_gram_algo -- the
 * kernel of st_set_style's targets under bf16 operands, and the one the tile-sharded iteration keeps (see st_set_gram_algo). */
/* raw sums of this rank into one flat device buffer owned by the context: blob 0's 3 x 3, blob 1's C x C, ... blob last_blob's, back to back
 * (*n_floats = sum of C^2).  The caller all-reduces it over the ranks, then calls st_tile_style_commit.  Returns with the buffer in place. */
int st_tile_style_partials(st_ctx* ctx, const void* hwc, int H, int W, int is_u8, int gH, int gW, int wy0, int wx0, int ty0, int tx0,
                           int ty1, int tx1, int last_blob, float** dev_ptr, int* n_floats);
/* targets of blobs 0 .. last_blob = reduced sums / (C gh gw), (gh, gw) the blob's size for the gH x gW image.  These blobs then have a
 * target, the blobs above last_blob have none (st_set_style gives every blob one): an evaluation, whole-image or tiled, whose weight
 * table puts a style weight on a blob without target fails with ST_ERR_STATE naming it.  ST_ERR_STATE without partials. */
int st_tile_style_commit(st_ctx* ctx);
/* partials -> all-reduce on the engine's stream (RCCL, or the caller's transport) -> commit.  COLLECTIVE: every rank of the communicator
 * calls it, the ranks without a style tile with hwc == NULL.  ST_ERR_STATE before st_comm_init / st_comm_callbacks; an argument error is
 * returned before the all-reduce, so the caller must then release the other ranks.  Across two or more devices the collective has not
 * been exercised yet (like the rest of the RCCL path: the tests run the ranks on one GPU over a caller-supplied transport, and a
 * one-rank RCCL communicator). */
int st_tile_set_style(st_ctx* ctx, const void* hwc, int H, int W, int is_u8, int gH, int gW, int wy0, int wx0, int ty0, int tx0,
                      int ty1, int tx1, int last_blob);
/* test hook: the style target of `blob`, C x C.  ST_ERR_STATE when the context holds none for it. */
int st_get_style_gram(st_ctx* ctx, int blob, float* out);

#ifdef __cplusplus
}
#endif
#endif /* ST2_H */
