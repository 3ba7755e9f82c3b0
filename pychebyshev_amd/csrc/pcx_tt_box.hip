// pcx_tt_box.hip -- C ABI of libpcx_hip.so (see include/pcx.h): batched box integrals of a tensor train.  gfx950 only.

#include "pcx_internal.h"
#include "tt_box_kernels.h"

// integrated: d flags by USER dimension.  The row offsets follow the user's order; the kernels walk storage positions.
static int tt_box_plan(const TTBoxView &v, const int32_t *integrated, TTBoxCols *cols) {
    const TTDims &dims = v.plan->dims;
    const int d = dims.d;
    int user_off[PCX_MAX_DIMS];
    int width = 0;
    for (int u = 0; u < d; ++u) {
        if (integrated[u] != 0 && integrated[u] != 1)
            return fail(PCX_ERR_INVALID, "integrated[%d] = %d is neither 0 nor 1", u, (int)integrated[u]);
        user_off[u] = width;
        width += 1 + integrated[u];
    }
    *cols = TTBoxCols{};
    cols->width = width;
    for (int k = 0; k < d; ++k) {
        const int u = dims.col[k];
        cols->off[k] = user_off[u];
        cols->integ[k] = integrated[u];
        cols->half[k] = (dims.hi[k] - dims.lo[k]) / 2.0;
    }
    return PCX_OK;
}

// N device-resident rows, queued on st.  Caller holds the handle's mutex.
static int tt_box_launch(const TTBoxView &v, const TTBoxCols &cols, const double *d_rows, long N, double *d_out,
                         hipStream_t st) {
    if (N == 0) return PCX_OK;
    const int d = v.plan->dims.d;
    if (v.d_lpp_img) {
        const long blocks = (N + PCX_LPP_WG - 1) / PCX_LPP_WG;
        if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
        const size_t lds = (size_t)v.plan->rmax * PCX_LPP_WG * sizeof(double);
        const TTLppDim *tab = v.d_lpp_tab;
        tt_lpp_for_model(v.plan->lppCap, v.plan->lpp_nodes, [&](auto rcap, auto nj) {
            hipLaunchKernelGGL((k_tt_box_lpp<decltype(rcap)::value, decltype(nj)::value>), dim3((unsigned)blocks), dim3(PCX_LPP_WG),
                               lds, st, tab, d, cols, v.d_lpp_img, d_rows, d_out, N);
        });
        HIP_TRY(hipGetLastError());
        return PCX_OK;
    }
    if (!v.d_cores) return fail(PCX_ERR_UNSUPPORTED, "the handle holds neither a lane-per-point image nor plain cores");
    const TTWaveModel gi = tt_wave_model(v);
    if (!*v.d_rinv) {
        // 1 / j for j = 1 .. nmax + 1 (entry 0 unused): the divisions of the antiderivatives, done once per handle
        std::vector<double> rinv((size_t)gi.nmax + 2, 0.0);
        for (size_t j = 1; j < rinv.size(); ++j) rinv[j] = 1.0 / (double)j;
        double *p = nullptr;
        HIP_TRY(hipMalloc((void **)&p, rinv.size() * sizeof(double)));
        const hipError_t e = hipMemcpy(p, rinv.data(), rinv.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(p); HIP_TRY(e); }
        *v.d_rinv = p;
    }
    size_t lds;
    const int rc = tt_wave_lds((const void *)k_tt_box_generic, v, 2 * (size_t)v.plan->rmax + v.plan->nmax, "box", "2 rank + nodes", &lds);
    if (rc) return rc;
    const long blocks = std::min<long>((N + 3) / 4, 256L * 8);
    hipLaunchKernelGGL(k_tt_box_generic, dim3((unsigned)blocks), dim3(256), lds, st, gi, cols, v.d_cores, *v.d_rinv, d_rows, d_out, N);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

extern "C" int pcx_tt_box_batch_dev(pcx_tt *h, const int32_t *integrated, const double *d_rows, int64_t N, double *d_out,
                                    void *stream) {
    PCX_API_BEGIN
    TTBoxView v;
    int rc = tt_box_view(h, &v);
    if (rc) return rc;
    if (!integrated) return fail(PCX_ERR_INVALID, "integrated is NULL");
    if (N < 0) return fail(PCX_ERR_INVALID, "N < 0");
    if (N > 0 && (!d_rows || !d_out)) return fail(PCX_ERR_INVALID, "NULL device buffer");
    TTBoxCols cols;
    if ((rc = tt_box_plan(v, integrated, &cols))) return rc;
    if (N == 0) return PCX_OK;
    HIP_TRY(hipSetDevice(v.device));
    std::lock_guard<std::mutex> lk(*v.mu);
    return tt_box_launch(v, cols, d_rows, (long)N, d_out, stream ? (hipStream_t)stream : v.stream);
    PCX_API_END
}

extern "C" int pcx_tt_box_batch(pcx_tt *h, const int32_t *integrated, const double *rows, int64_t N, double *out) {
    PCX_API_BEGIN
    TTBoxView v;
    int rc = tt_box_view(h, &v);
    if (rc) return rc;
    if (!integrated) return fail(PCX_ERR_INVALID, "integrated is NULL");
    if (N < 0) return fail(PCX_ERR_INVALID, "N < 0");
    if (N > 0 && (!rows || !out)) return fail(PCX_ERR_INVALID, "NULL buffer");
    TTBoxCols cols;
    if ((rc = tt_box_plan(v, integrated, &cols))) return rc;
    if (N == 0) return PCX_OK;
    HIP_TRY(hipSetDevice(v.device));
    std::lock_guard<std::mutex> lk(*v.mu);
    // as pcx_tt_eval_batch: ~10 MB of rows per piece, two slots from two pieces on
    const int w = cols.width;
    const int64_t piece = std::max<int64_t>(65536, (((int64_t)10 << 20) / (w * 8)) & ~(int64_t)65535);
    const bool piped = N >= 2 * piece;
    const int64_t chunk = piped ? piece : kChunkPoints;
    return stage_host_batch(*v.stage, v.device, v.stream, rows, N, w, 1, out, StagePlan{chunk, chunk, piped, true},
                            [&](int, hipStream_t st, const double *dp, long cnt, double *dout) {
                                return tt_box_launch(v, cols, dp, cnt, dout, st);
                            });
    PCX_API_END
}
