// The content's colours (include/st2.h): the colour-matched style image, on the device copy of the style image on its way to the forward,
// and the setters (the luminance-only output is a form of the emission pass, engine_emit.cpp).
#include "engine.h"
#include "color_match.h"

namespace st2e {
// ---- moments and the style transform --------------------------------------------------------------------------------------------
// the nine sums of a planar (3, n) device image -> mean, cov; waits for the stream
static int moments_of(st_ctx* c, const float* x, size_t n, double mean[3], double cov[6])
{
    if (!c->mom_part) ST_TRY(c->mom_part.alloc((size_t)kMomentSums * kMomentBlocks));
    if (!c->mom_out) ST_TRY(c->mom_out.alloc(kMomentSums));
    double sums[kMomentSums];
    {
        ProfScope ps(c, P_MISC, 0, 12.0 * n);
        HIP_TRY(launch_image_moments(x, n, c->mom_part, c->mom_out, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(sums, c->mom_out, sizeof sums, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    st2c::moments_finish(sums, (double)n, mean, cov);
    return ST_OK;
}

int style_color_check(const st_ctx* c)
{
    if (c->style_match != 1) return ST_OK;
    if (c->tile.on)
        return fail(ST_ERR_STATE, "colour matching takes the content image's moments, and a tile-sharded context holds one window of it: derive A, b "
                                  "for the whole images (st_image_moments, st_color_transform) and give them to every rank with st_set_style_transform");
    if (!c->have_content || !c->content_x) return fail(ST_ERR_STATE, "colour matching: no content image to match the style's colours to (st_set_content first)");
    return ST_OK;
}

int style_recolor_enqueue(st_ctx* c, float* x, int H, int W)
{
    if (!c->style_match) return ST_OK;
    const size_t n = (size_t)H * W;
    if (c->style_match == 1) {                     // (the caller has run style_color_check)
        double mc[3], cc[6], ms[3], cs[6];
        ST_TRY(moments_of(c, c->content_x, (size_t)c->cH * c->cW, mc, cc));
        ST_TRY(moments_of(c, x, n, ms, cs));
        float A[9], b[3];
        const char* why = "";
        if (st2c::color_transform(mc, cc, ms, cs, A, b, &why) != ST_OK) return fail(ST_ERR_ARG, "colour matching: %s", why);
        memcpy(c->xf_A, A, sizeof A); memcpy(c->xf_b, b, sizeof b);
    }
    RecolorArgs r{};
    r.x = x; r.n = n;
    memcpy(r.A, c->xf_A, sizeof r.A); memcpy(r.b, c->xf_b, sizeof r.b);
    ProfScope ps(c, P_MISC, 0, 24.0 * n);
    HIP_TRY(launch_recolor(r, c->stream));
    return ST_OK;
}
}  // namespace st2e

extern "C" {

int st_set_original_colors(st_ctx* c, int on)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    if (on != 0 && on != 1) return fail(ST_ERR_ARG, "original_colors must be 0 or 1, not %d", on);
    if (c->pipe.count) return fail(ST_ERR_STATE, "%d pipelined iteration(s) in flight: st_step_end before st_set_original_colors", c->pipe.count);
    c->orig_colors = on != 0;
    return ST_OK;
}

int st_image_moments(st_ctx* c, const void* hwc, int H, int W, int is_u8, double mean[3], double cov[6])
{
    if (!c || !hwc || H <= 0 || W <= 0 || !mean || !cov) return fail(ST_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> tmp;
    ST_TRY(tmp.alloc((size_t)3 * H * W));
    int r = preprocess_into(c, hwc, H, W, is_u8, tmp);
    if (r == ST_OK) r = moments_of(c, tmp, (size_t)H * W, mean, cov);
    (void)hipStreamSynchronize(c->stream);       // (before tmp goes)
    return r;
}

int st_color_transform(const double mean_c[3], const double cov_c[6], const double mean_s[3], const double cov_s[6], float A[9], float b[3])
{
    const char* why = "";
    if (st2c::color_transform(mean_c, cov_c, mean_s, cov_s, A, b, &why) != ST_OK) return fail(ST_ERR_ARG, "st_color_transform: %s", why);
    return ST_OK;
}

int st_set_style_transform(st_ctx* c, const float A[9], const float b[3])
{
    if (c) c->epoch++;
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    if (!A != !b) return fail(ST_ERR_ARG, "st_set_style_transform takes A and b, or NULL for both (off)");
    if (!A) {
        if (c->style_match == 2) c->style_match = 0;
        return ST_OK;
    }
    for (int i = 0; i < 9; ++i) if (!isfinite(A[i])) return fail(ST_ERR_ARG, "A[%d] is not finite", i);
    for (int i = 0; i < 3; ++i) if (!isfinite(b[i])) return fail(ST_ERR_ARG, "b[%d] is not finite", i);
    memcpy(c->xf_A, A, sizeof c->xf_A); memcpy(c->xf_b, b, sizeof c->xf_b);
    c->style_match = 2;
    return ST_OK;
}

int st_set_style_color_match(st_ctx* c, int on)
{
    if (c) c->epoch++;
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    if (on != 0 && on != 1) return fail(ST_ERR_ARG, "style_color_match must be 0 or 1, not %d", on);
    if (!on) {
        if (c->style_match == 1) c->style_match = 0;
        return ST_OK;
    }
    if (c->tile.on)
        return fail(ST_ERR_STATE, "colour matching takes the content image's moments, and a tile-sharded context holds one window of it: derive A, b "
                                  "for the whole images (st_image_moments, st_color_transform) and give them to every rank with st_set_style_transform");
    c->style_match = 1;
    return ST_OK;
}

int st_get_color_modes(st_ctx* c, int* original_colors, int* style_match, float A[9], float b[3])
{
    if (!c) return fail(ST_ERR_ARG, "ctx is NULL");
    if (original_colors) *original_colors = c->orig_colors ? 1 : 0;
    if (style_match) *style_match = c->style_match;
    if (A) memcpy(A, c->xf_A, sizeof c->xf_A);
    if (b) memcpy(b, c->xf_b, sizeof c->xf_b);
    return ST_OK;
}

int st_style_recolor(st_ctx* c, const void* hwc, int H, int W, int is_u8, float* out_nchw)
{
    if (!c || !hwc || H <= 0 || W <= 0 || !out_nchw) return fail(ST_ERR_ARG, "bad argument");
    ST_TRY(style_color_check(c));
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> tmp;
    ST_TRY(tmp.alloc((size_t)3 * H * W));
    int r = preprocess_into(c, hwc, H, W, is_u8, tmp);
    if (r == ST_OK) r = style_recolor_enqueue(c, tmp, H, W);
    if (r == ST_OK && hipMemcpyAsync(out_nchw, tmp, (size_t)3 * H * W * sizeof(float), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        r = fail(ST_ERR_HIP, "recoloured image copy failed");
    if (hipStreamSynchronize(c->stream) != hipSuccess && r == ST_OK) r = fail(ST_ERR_HIP, "recoloured image copy failed");
    return r;
}

}  // extern "C"
