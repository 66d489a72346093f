// Device-resident resampling (Pillow-exact; utils.py:130-160, optimizers.py:29-40,110-119, worker.py:154-170).
#include "engine.h"

namespace st2e {
struct DevTable { DevBuf<int> lo, n; DevBuf<double> k; ResampleTable t{}; int out = 0; };

int table_upload(const st_resample_table* h, DevTable* d)
{
    if (!h || !h->lo || !h->n || !h->k || h->kmax <= 0 || h->out_size <= 0) return fail(ST_ERR_ARG, "bad resample table");
    const size_t no = (size_t)h->out_size;
    ST_TRY(d->lo.alloc(no)); ST_TRY(d->n.alloc(no)); ST_TRY(d->k.alloc(no * h->kmax));
    HIP_TRY(hipMemcpy(d->lo, h->lo, no * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->n, h->n, no * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->k, h->k, no * h->kmax * sizeof(double), hipMemcpyHostToDevice));
    d->t = ResampleTable{d->lo, d->n, d->k, h->kmax};
    d->out = h->out_size;
    return ST_OK;
}
int tables_valid_for(const st_resample_table* x, const st_resample_table* y, int H, int W)
{
    for (int i = 0; x && i < x->out_size; ++i) if (x->lo[i] < 0 || x->n[i] < 0 || x->lo[i] + x->n[i] > W || x->n[i] > x->kmax) return 0;
    for (int i = 0; y && i < y->out_size; ++i) if (y->lo[i] < 0 || y->n[i] < 0 || y->lo[i] + y->n[i] > H || y->n[i] > y->kmax) return 0;
    return 1;
}
}  // namespace st2e

extern "C" {

int st_resample_state(st_ctx* c, const st_resample_table* lan_x, const st_resample_table* lan_y,
                      const st_resample_table* bil_x, const st_resample_table* bil_y, const float* new_x_nchw)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c || !c->x[0]) return fail(ST_ERR_STATE, "no input image");
    if (!lan_x || !lan_y) return fail(ST_ERR_ARG, "Lanczos tables are required");
    HIP_TRY(hipSetDevice(c->device));
    const int H = c->H, W = c->W, H2 = lan_y->out_size, W2 = lan_x->out_size;
    const bool adam = c->opt_kind == ST_OPT_ADAM;
    if (adam && (!bil_x || !bil_y || bil_x->out_size != W2 || bil_y->out_size != H2)) return fail(ST_ERR_ARG, "Adam needs bilinear tables of the same output size");
    if (!tables_valid_for(lan_x, lan_y, H, W) || (adam && !tables_valid_for(bil_x, bil_y, H, W))) return fail(ST_ERR_ARG, "resample table does not fit the %dx%d state", H, W);
    HIP_TRY(hipStreamSynchronize(c->stream));
    DevTable lx, ly, bx, by;
    ST_TRY(table_upload(lan_x, &lx)); ST_TRY(table_upload(lan_y, &ly));
    if (adam) { ST_TRY(table_upload(bil_x, &bx)); ST_TRY(table_upload(bil_y, &by)); }
    const size_t n2 = (size_t)3 * H2 * W2, ntmp = (size_t)3 * H * W2;
    const bool keep_m = adam && !c->m_zero, keep_v = adam && !c->v_zero;
    // the iterate average: the raw mean goes through x's Lanczos tables (the bias correction is a scalar and commutes), its item count
    // is kept; a new image starts an empty mean
    const bool keep_avg = c->avg_decay > 0 && c->avg_items > 0 && !new_x_nchw;
    // (an early return below frees the temporaries and tables while a launch that reads them may still be queued: hipFree waits
    // for the device first, so that is safe)
    DevBuf<float> tx, tm, tv, ta, tmp;
    ST_TRY(tx.alloc(n2)); ST_TRY(tmp.alloc(ntmp));
    if (keep_m) ST_TRY(tm.alloc(n2));
    if (keep_v) ST_TRY(tv.alloc(n2));
    if (keep_avg) ST_TRY(ta.alloc(n2));
    if (new_x_nchw) HIP_TRY(hipMemcpyAsync(tx, new_x_nchw, n2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    else HIP_TRY(launch_resample(c->x[c->cur], tmp, tx, 3, H, W, H2, W2, lx.t, ly.t, 0, c->stream));
    if (keep_m) HIP_TRY(launch_resample(c->m, tmp, tm, 3, H, W, H2, W2, lx.t, ly.t, 0, c->stream));
    if (keep_v) HIP_TRY(launch_resample(c->v, tmp, tv, 3, H, W, H2, W2, bx.t, by.t, 1, c->stream));   // np.maximum(0, .)
    if (keep_avg) HIP_TRY(launch_resample(c->avg, tmp, ta, 3, H, W, H2, W2, lx.t, ly.t, 0, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const bool mz = c->m_zero, vz = c->v_zero;
    const int i1 = c->items1, i2 = c->items2, ia = c->avg_items;
    ST_TRY(ensure_input_buffers(c, H2, W2));           // frees and re-creates x, m, v, L-BFGS vectors
    c->lb_clear = true; c->have_cur = false;
    iterate_overwritten(c);                            // (a resample to the SAME size keeps the buffers)
    HIP_TRY(hipMemcpyAsync(c->x[c->cur], tx, n2 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if (keep_m) HIP_TRY(hipMemcpyAsync(c->m, tm, n2 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if (keep_v) HIP_TRY(hipMemcpyAsync(c->v, tv, n2 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if (keep_avg) HIP_TRY(hipMemcpyAsync(c->avg, ta, n2 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->m_zero = mz; c->v_zero = vz; c->items1 = i1; c->items2 = i2;
    c->avg_items = keep_avg ? ia : 0;
    return ST_OK;
}

int st_resample_content(st_ctx* c, const st_resample_table* lan_x, const st_resample_table* lan_y)
{
    if (c) c->epoch++;       // anything but st_step may change what a step launches: captured step graphs are stale
    if (!c || !c->have_content || !c->content_x) return fail(ST_ERR_STATE, "no content image");
    if (!lan_x || !lan_y) return fail(ST_ERR_ARG, "Lanczos tables are required");
    HIP_TRY(hipSetDevice(c->device));
    const int H = c->cH, W = c->cW, H2 = lan_y->out_size, W2 = lan_x->out_size;
    if (!tables_valid_for(lan_x, lan_y, H, W)) return fail(ST_ERR_ARG, "resample table does not fit the %dx%d content", H, W);
    DevTable lx, ly;
    ST_TRY(table_upload(lan_x, &lx)); ST_TRY(table_upload(lan_y, &ly));
    DevBuf<float> tx, tmp;         // (freed on an early return too; hipFree waits for the device, as above)
    ST_TRY(tx.alloc((size_t)3 * H2 * W2)); ST_TRY(tmp.alloc((size_t)3 * H * W2));
    HIP_TRY(launch_resample(c->content_x, tmp, tx, 3, H, W, H2, W2, lx.t, ly.t, 0, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int rc = content_from_device(c, tx, H2, W2);
    (void)hipStreamSynchronize(c->stream);             // (before tx goes)
    return rc;
}

int st_get_content_nchw(st_ctx* c, float* out, int* H, int* W)
{
    if (!c || !c->have_content || !c->content_x) return fail(ST_ERR_STATE, "no content image");
    if (H) *H = c->cH;
    if (W) *W = c->cW;
    if (out) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(out, c->content_x, (size_t)3 * c->cH * c->cW * sizeof(float), hipMemcpyDeviceToHost));
    }
    return ST_OK;
}

}  // extern "C"
