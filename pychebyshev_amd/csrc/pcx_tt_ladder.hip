// pcx_tt_ladder.hip -- C ABI of libpcx_hip.so (see include/pcx.h): ladders and fibres of a tensor train along one
// dimension.  gfx950 only.

#include "pcx_internal.h"
#include "tt_ladder_kernels.h"

// as pcx_bary_ladder_batch: doubles of the wider side one pass of a host-pointer batch stages
static const int64_t kLadderPassDoubles = (int64_t)1 << 20;

// dim in the USER's frame -> its storage position and, per storage position, the column of `fixed` it reads
static int tt_ladder_plan(const TTBoxView &v, int dim, int m, TTLadder *lp) {
    const TTDims &dims = *v.dims;
    const int d = dims.d;
    if (dim < 0 || dim >= d) return fail(PCX_ERR_INVALID, "dim %d out of range [0, %d]", dim, d - 1);
    *lp = TTLadder{};
    lp->d = d;
    lp->m = m;
    lp->rmax = v.rmax;
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
    const int d = lp.d;
    if (v.lppCap) {
        const long blocks = (N + PCX_LPP_WG - 1) / PCX_LPP_WG;
        if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
        const size_t lds = (size_t)3 * v.rmax * PCX_LPP_WG * sizeof(double);
        hipLaunchKernelGGL(k_tt_ladder_lpp, dim3((unsigned)blocks), dim3(PCX_LPP_WG), lds, st, (const TTLppDim *)v.d_lpp_tab, lp,
                           v.d_lpp_img, d_fixed, fstride, d_xs, xstride, d_out, N);
        HIP_TRY(hipGetLastError());
        return PCX_OK;
    }
    if (!v.d_cores) return fail(PCX_ERR_UNSUPPORTED, "the handle holds neither a lane-per-point image nor plain cores");
    TTLadderGeneric gi{};
    gi.nmax = v.nmax;
    for (int k = 0; k < d; ++k) {
        gi.rank[k] = v.ranks[k];
        gi.n[k] = v.dims->n[k];
        gi.coff[k] = v.coff[k];
        gi.lo[k] = v.dims->lo[k];
        gi.scale[k] = v.dims->scale[k];
    }
    gi.rank[d] = v.ranks[d];
    const size_t lds = (size_t)4 * (3 * v.rmax + 2 * v.nmax) * sizeof(double);
    if (lds > 160 * 1024)
        return fail(PCX_ERR_UNSUPPORTED, "TT rank %d with %d nodes exceeds the generic ladder kernel's LDS budget "
                    "(3 rank + 2 nodes <= 5120)", v.rmax, v.nmax);
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)k_tt_ladder_generic, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long blocks = std::min<long>((N + 3) / 4, 256L * 8);
    hipLaunchKernelGGL(k_tt_ladder_generic, dim3((unsigned)blocks), dim3(256), lds, st, gi, lp, v.d_cores, d_fixed, fstride, d_xs,
                       xstride, d_out, N);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

static int tt_ladder_check(pcx_tt *h, TTBoxView *v, int dim, const void *fixed, int64_t N, const void *xs, int m, int xs_per_row,
                           const void *out, TTLadder *lp) {
    int rc = tt_box_view(h, v);
    if (rc) return rc;
    if (N < 0) return fail(PCX_ERR_INVALID, "N < 0");
    if (m < 0) return fail(PCX_ERR_INVALID, "m < 0");
    if (xs_per_row != 0 && xs_per_row != 1) return fail(PCX_ERR_INVALID, "xs_per_row = %d is neither 0 nor 1", xs_per_row);
    if ((rc = tt_ladder_plan(*v, dim, m, lp))) return rc;
    if (N > 0 && lp->d > 1 && !fixed) return fail(PCX_ERR_INVALID, "fixed is NULL");
    if (m > 0 && (xs_per_row ? N > 0 : true) && !xs) return fail(PCX_ERR_INVALID, "xs is NULL");
    if (N > 0 && m > 0 && !out) return fail(PCX_ERR_INVALID, "out is NULL");
    return PCX_OK;
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
    if ((rc = dxs.alloc((size_t)m * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpyAsync(dxs.p, xs, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
    rc = tt_ladder_launch(v, lp, d_fixed, nq, dxs.as<double>(), 0, (long)N, d_out, st);
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
    if (!xs_per_row) {
        if ((rc = dxs.alloc((size_t)m * sizeof(double)))) return rc;
        HIP_TRY(hipMemcpy(dxs.p, xs, (size_t)m * sizeof(double), hipMemcpyHostToDevice));
    }
    // staged rows and passes as pcx_bary_ladder_batch
    const int nq = lp.d - 1;
    const int w = std::max(1, nq + (xs_per_row ? m : 0));
    const int64_t pass = std::max<int64_t>(1, kLadderPassDoubles / std::max(w, m));
    const bool direct = !xs_per_row && nq > 0;
    std::vector<double> rows;
    for (int64_t start = 0; start < N; start += pass) {
        const int64_t cnt = std::min<int64_t>(pass, N - start);
        const double *src = fixed + (size_t)start * nq;
        if (!direct) {
            rows.assign((size_t)cnt * w, 0.0);
            for (int64_t r = 0; r < cnt; ++r) {
                double *dst = rows.data() + (size_t)r * w;
                if (nq) memcpy(dst, fixed + (size_t)(start + r) * nq, (size_t)nq * sizeof(double));
                if (xs_per_row) memcpy(dst + nq, xs + (size_t)(start + r) * m, (size_t)m * sizeof(double));
            }
            src = rows.data();
        }
        rc = stage_host_batch(*v.stage, v.device, v.stream, src, cnt, w, m, out + (size_t)start * m,
                              StagePlan{cnt, cnt, false, true},
                              [&](int, hipStream_t st, const double *dp, long c, double *dout) {
                                  return xs_per_row ? tt_ladder_launch(v, lp, dp, w, dp + nq, w, c, dout, st)
                                                    : tt_ladder_launch(v, lp, dp, w, dxs.as<double>(), 0, c, dout, st);
                              });
        if (rc) return rc;
    }
    return PCX_OK;
    PCX_API_END
}
