// pcx_tt_ladder.hip -- C ABI of libpcx_hip.so (see include/pcx.h): ladders and fibres of a tensor train along one
// dimension.  gfx950 only.

#include "pcx_internal.h"
#include "tt_ladder_kernels.h"

// dim in the USER's frame (range-checked by ladder_check) -> its storage position and, per storage position, the column
// of `fixed` it reads
static int tt_ladder_plan(const TTBoxView &v, int dim, int m, TTLadder *lp) {
    const TTDims &dims = v.plan->dims;
    const int d = dims.d;
    *lp = TTLadder{};
    lp->d = d;
    lp->m = m;
    lp->rmax = v.plan->rmax;
    lp->p = -1;
    for (int k = 0; k < d; ++k) {
        const int u = dims.col[k];
        if (u == dim) lp->p = k;
        lp->fcol[k] = u < dim ? u : u - 1;
    }
    if (lp->p < 0) return fail(PCX_ERR_INTERNAL, "dim %d is not in the handle's dimension order", dim);
    return PCX_OK;
}

// N device-resident rows, queued on st.  Caller holds the handle's mutex.
static int tt_ladder_launch(const TTBoxView &v, const TTLadder &lp, const double *d_fixed, long fstride, const double *d_xs,
                            long xstride, long N, double *d_out, hipStream_t st) {
    if (N == 0 || lp.m == 0) return PCX_OK;
    if (v.d_lpp_img) {
        const long blocks = (N + PCX_LPP_WG - 1) / PCX_LPP_WG;
        if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
        const size_t lds = (size_t)3 * v.plan->rmax * PCX_LPP_WG * sizeof(double);
        hipLaunchKernelGGL(k_tt_ladder_lpp, dim3((unsigned)blocks), dim3(PCX_LPP_WG), lds, st, v.d_lpp_tab, lp,
                           v.d_lpp_img, d_fixed, fstride, d_xs, xstride, d_out, N);
        HIP_TRY(hipGetLastError());
        return PCX_OK;
    }
    if (!v.d_cores) return fail(PCX_ERR_UNSUPPORTED, "the handle holds neither a lane-per-point image nor plain cores");
    const TTWaveModel gi = tt_wave_model(v);
    size_t lds;
    const int rc = tt_wave_lds((const void *)k_tt_ladder_generic, v, 3 * (size_t)v.plan->rmax + 2 * v.plan->nmax, "ladder", "3 rank + 2 nodes", &lds);
    if (rc) return rc;
    const long blocks = std::min<long>((N + 3) / 4, 256L * 8);
    hipLaunchKernelGGL(k_tt_ladder_generic, dim3((unsigned)blocks), dim3(256), lds, st, gi, lp, v.d_cores, d_fixed, fstride, d_xs,
                       xstride, d_out, N);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

// the handle's view, ladder_check on its dimensions (a TT ladder takes no spec), then the plan
static int tt_ladder_check(pcx_tt *h, TTBoxView *v, int dim, const void *fixed, int64_t N, const void *xs, int m, int xs_per_row,
                           const void *out, TTLadder *lp) {
    int rc = tt_box_view(h, v);
    if (!rc) rc = ladder_check(h, v->plan->dims.d, dim, nullptr, fixed, N, xs, m, xs_per_row, out);
    return rc ? rc : tt_ladder_plan(*v, dim, m, lp);
}

extern "C" int pcx_tt_ladder_batch_dev(pcx_tt *h, int dim, const double *d_fixed, int64_t N, const double *xs, int m,
                                       int xs_per_row, double *d_out, void *stream) {
    PCX_API_BEGIN
    TTBoxView v;
    TTLadder lp;
    int rc = tt_ladder_check(h, &v, dim, d_fixed, N, xs, m, xs_per_row, d_out, &lp);
    if (rc) return rc;
    if (N == 0 || m == 0) return PCX_OK;
    HIP_TRY(hipSetDevice(v.device));
    std::lock_guard<std::mutex> lk(*v.mu);
    hipStream_t st = stream ? (hipStream_t)stream : v.stream;
    const int nq = lp.d - 1;
    if (xs_per_row) return tt_ladder_launch(v, lp, d_fixed, nq, xs, m, (long)N, d_out, st);
    // shared values come from the host: a buffer of this call's, so the call waits for its kernel before it frees it
    DevBuf dxs;
    const double *d_shared = nullptr;
    if ((rc = ladder_shared_xs(dxs, xs, m, true, st, &d_shared))) return rc;
    rc = tt_ladder_launch(v, lp, d_fixed, nq, d_shared, 0, (long)N, d_out, st);
    const hipError_t e = hipStreamSynchronize(st);
    if (rc) return rc;
    HIP_TRY(e);
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_tt_ladder_batch(pcx_tt *h, int dim, const double *fixed, int64_t N, const double *xs, int m,
                                   int xs_per_row, double *out) {
    PCX_API_BEGIN
    TTBoxView v;
    TTLadder lp;
    int rc = tt_ladder_check(h, &v, dim, fixed, N, xs, m, xs_per_row, out, &lp);
    if (rc) return rc;
    if (N == 0 || m == 0) return PCX_OK;
    HIP_TRY(hipSetDevice(v.device));
    std::lock_guard<std::mutex> lk(*v.mu);
    DevBuf dxs;
    const double *d_shared = nullptr;
    if (!xs_per_row && (rc = ladder_shared_xs(dxs, xs, m, false, nullptr, &d_shared))) return rc;
    return ladder_host_passes(*v.stage, v.device, v.stream, lp.d - 1, fixed, N, xs, d_shared, m, xs_per_row, out,
                              [&](const double *df, long fs, const double *dx, long xstr, long cnt, double *dout, hipStream_t st) {
                                  return tt_ladder_launch(v, lp, df, fs, dx, xstr, cnt, dout, st);
                              });
    PCX_API_END
}
