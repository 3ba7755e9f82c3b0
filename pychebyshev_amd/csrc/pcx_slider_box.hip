// pcx_slider_box.hip -- C ABI of libpcx_hip.so (see include/pcx.h): batched box integrals of a slider.  gfx950 only.
//
// f(x) = pv + sum_i (s_i(x_Gi) - pv), so the integral of a row's box T at its kept coordinates is
//     pv vol_T + sum_i vol(T \ G_i) (I_i - pv vol(T n G_i))
// with I_i slide i's own box integral (pcx_bary_box_batch_dev; its value where none of its dimensions is integrated).
// Per slide: k_slider_box_row gathers the slide's box row out of the slider's, the slide's box launch fills I_i;
// k_slider_box_combine then forms the sum, slides in partition order, every volume as a product of the row's widths.

#include "pcx_slider_internal.h"
#include "slider_calc_kernels.h"

// rows per pass of a device-resident batch: bounds the scratch (a slide's rows and the n_slides integrals)
static const int64_t kSliderBoxChunk = 1 << 20;

struct SliderBoxPlan {
    int width = 0;                       // slider row: one double per kept dimension, two per integrated one
    std::vector<int32_t> flags;          // by dimension
    std::vector<int> off;                // column of dimension u: u + the number of flags set below u
    DevBuf tab;                          // device: off, integ, owner (d ints each), then every slide's source columns
    std::vector<int> src_at;             // slide -> offset (ints) of its source columns in tab
    std::vector<int> w;                  // slide -> width of its own box row
    int max_w = 1;
};

static int slider_box_plan(pcx_slider *h, const int32_t *flags, const double *lo, const double *hi, SliderBoxPlan &p) {
    const int d = h->d, ns = (int)h->slides.size();
    p.flags.assign(flags, flags + d);
    p.off.resize(d);
    for (int u = 0; u < d; ++u) {
        if (flags[u] != 0 && flags[u] != 1) return fail(PCX_ERR_INVALID, "flags[%d] = %d is neither 0 nor 1", u, (int)flags[u]);
        if (!(lo[u] < hi[u]) || !std::isfinite(lo[u]) || !std::isfinite(hi[u]))
            return fail(PCX_ERR_INVALID, "domain[%d]: lo must be < hi", u);
        p.off[u] = p.width;
        p.width += 1 + flags[u];
    }
    std::vector<int> tab(3 * (size_t)d);
    for (int u = 0; u < d; ++u) { tab[u] = p.off[u]; tab[d + u] = flags[u]; tab[2 * d + u] = h->owner[u]; }
    for (int s = 0; s < ns; ++s) {
        const SliderCols &c = h->cols[s];
        p.src_at.push_back((int)tab.size());
        for (int k = 0; k < c.nc; ++k) {
            tab.push_back(p.off[c.col[k]]);
            if (flags[c.col[k]]) tab.push_back(p.off[c.col[k]] + 1);
        }
        p.w.push_back((int)tab.size() - p.src_at[s]);
        p.max_w = std::max(p.max_w, p.w[s]);
    }
    int rc = p.tab.alloc(tab.size() * sizeof(int));
    if (rc) return rc;
    HIP_TRY(hipMemcpy(p.tab.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice));
    return PCX_OK;
}

// cnt device-resident slider rows into d_out, queued on st.  Caller holds h->mu; each slide's box launch takes the
// slide's own mutex (the evaluation's order).
static int slider_box_chunk(pcx_slider *h, SliderBoxPlan &p, const double *lo, const double *hi, const double *d_rows, long cnt,
                            double *d_out, hipStream_t st) {
    const int d = h->d, ns = (int)h->slides.size();
    int rc = h->s_cols.reserve((size_t)cnt * p.max_w * sizeof(double));
    if (!rc) rc = h->s_vals.reserve((size_t)cnt * ns * sizeof(double));
    if (rc) return rc;
    double *srow = (double *)h->s_cols.ptr, *ints = (double *)h->s_vals.ptr;
    const int *tab = p.tab.as<int>();
    for (int s = 0; s < ns; ++s) {
        const SliderCols &c = h->cols[s];
        int32_t sf[PCX_MAX_DIMS];
        double slo[PCX_MAX_DIMS], shi[PCX_MAX_DIMS];
        for (int k = 0; k < c.nc; ++k) { sf[k] = p.flags[c.col[k]]; slo[k] = lo[c.col[k]]; shi[k] = hi[c.col[k]]; }
        const long total = cnt * p.w[s];
        hipLaunchKernelGGL(k_slider_box_row, dim3((unsigned)std::min<long>((total + 255) / 256, 8192)), dim3(256), 0, st, d_rows,
                           cnt, p.width, tab + p.src_at[s], p.w[s], srow);
        HIP_TRY(hipGetLastError());
        if ((rc = pcx_bary_box_batch_dev(h->slides[s], sf, slo, shi, srow, cnt, ints + (size_t)s * cnt, (void *)st))) return rc;
    }
    hipLaunchKernelGGL(k_slider_box_combine, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, d_rows, cnt, p.width, d, tab,
                       tab + d, tab + 2 * d, ns, h->pivot, (const double *)ints, d_out);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

static int slider_box_check(pcx_slider *h, const int32_t *flags, const double *lo, const double *hi, const void *rows, int64_t N,
                            const void *out) {
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    if (!flags || !lo || !hi) return fail(PCX_ERR_INVALID, "NULL flags or domain");
    if (N < 0) return fail(PCX_ERR_INVALID, "N < 0");
    if (N > 0 && (!rows || !out)) return fail(PCX_ERR_INVALID, "NULL buffer");
    return PCX_OK;
}

extern "C" int pcx_slider_box_batch_dev(pcx_slider *h, const int32_t *flags, const double *lo, const double *hi,
                                        const double *d_rows, int64_t N, double *d_out) {
    PCX_API_BEGIN
    int rc = slider_box_check(h, flags, lo, hi, d_rows, N, d_out);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    SliderBoxPlan p;
    if ((rc = slider_box_plan(h, flags, lo, hi, p))) return rc;
    for (int64_t start = 0; start < N && !rc; start += kSliderBoxChunk) {
        const long cnt = (long)std::min<int64_t>(kSliderBoxChunk, N - start);
        rc = slider_box_chunk(h, p, lo, hi, d_rows + (size_t)start * p.width, cnt, d_out + start, h->stream);
    }
    const hipError_t e = hipStreamSynchronize(h->stream);     // the plan's table is freed on return
    if (rc) return rc;
    HIP_TRY(e);
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_slider_box_batch(pcx_slider *h, const int32_t *flags, const double *lo, const double *hi, const double *rows,
                                    int64_t N, double *out) {
    PCX_API_BEGIN
    int rc = slider_box_check(h, flags, lo, hi, rows, N, out);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    SliderBoxPlan p;
    if ((rc = slider_box_plan(h, flags, lo, hi, p))) return rc;
    if (N == 0) return PCX_OK;
    return stage_host_batch(h->stage, h->device, h->stream, rows, N, p.width, 1, out,
                            StagePlan{kSliderBoxChunk, kSliderBoxChunk, false, true},
                            [&](int, hipStream_t st, const double *dp, long cnt, double *dout) {
                                return slider_box_chunk(h, p, lo, hi, dp, cnt, dout, st);
                            });
    PCX_API_END
}
