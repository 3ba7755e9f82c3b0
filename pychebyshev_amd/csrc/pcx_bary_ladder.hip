// pcx_bary_ladder.hip -- C ABI of libpcx_hip.so (see include/pcx.h): ladders and fibres of the full-tensor barycentric
// interpolant along one dimension.  gfx950 only.

#include "pcx_bary_internal.h"
#include "bary_ladder_kernels.h"

static const int kLadderLdsMax = 64 * 1024;      // the MFMA form's wave: above it the rows form

static size_t ladder_mfma_lds(const BaryLadder &lp) {
    return ((size_t)lp.wrows * 16 + (size_t)lp.Klo4 * 16 + (size_t)16 * (16 * lp.CT + 1)) * sizeof(double);
}

// The contraction along every dimension but `dim`, and the MFMA form's geometry when the handle takes it (lp->CT != 0):
// at least one other dimension, at most 64 nodes along dim (four column tiles of accumulators), a low part of the
// trailing other dimensions while it stays within 256 entries (at least the last one), and a wave's tables within 64 KB
// of LDS.  pcx_bary_set_kernel(h, 1) forces the rows form.
PCX_HIDDEN int bary_ladder_plan(const pcx_bary *h, int dim, BaryLadder *lp) {
    const BaryDims &dims = h->dims;
    const int d = dims.d;
    if (dim < 0 || dim >= d) return fail(PCX_ERR_INVALID, "dim %d out of range [0, %d]", dim, d - 1);
    *lp = BaryLadder{};
    lp->dim = dim;
    lp->n = dims.n[dim];
    long st[PCX_MAX_DIMS];
    long run = 1;
    for (int k = d - 1; k >= 0; --k) { st[k] = run; run *= dims.n[k]; }
    lp->dstride = st[dim];
    lp->K = 1;
    for (int k = 0; k < d; ++k) {
        if (k == dim) continue;
        const int i = lp->nq++;
        lp->q[i] = k;
        lp->stride[i] = st[k];
        lp->wrow[i] = lp->wrows;
        lp->wrows += dims.n[k];
        lp->K *= dims.n[k];
    }
    if (h->variant == 1 || lp->nq == 0 || lp->n > 64) return PCX_OK;
    long klo = 1;
    int nlo = 0;
    for (int i = lp->nq - 1; i >= 0; --i) {
        const long next = klo * dims.n[lp->q[i]];
        if (nlo > 0 && next > 256) break;
        klo = next;
        ++nlo;
    }
    if (klo > 4096) return PCX_OK;
    lp->nlo = nlo;
    lp->Klo = (int)klo;
    lp->Klo4 = (int)((klo + 3) / 4 * 4);
    lp->Khi = lp->K / klo;
    lp->CT = (lp->n + 15) / 16;
    if (ladder_mfma_lds(*lp) > (size_t)kLadderLdsMax) lp->CT = 0;
    return PCX_OK;
}

// The B image of (dt, dim), packed on first use and kept with the derived tensor (evicted and freed with it).
// Caller holds h->mu.
static int bary_ladder_image(pcx_bary *h, DerivedTensor *dt, const BaryLadder &lp, const double **img) {
    if (!dt->ladder[lp.dim]) {
        const long total = lp.Khi * lp.Klo4 * 16 * lp.CT;
        DevBuf buf;
        int rc = buf.alloc(((size_t)total + PCX_LADDER_PAD) * sizeof(double));
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(buf.as<double>() + total, 0, PCX_LADDER_PAD * sizeof(double), h->stream));
        hipLaunchKernelGGL(k_pack_ladder, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, h->dims, lp, dt->plain,
                           buf.as<double>(), total);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(h->stream));        // a _dev caller may read it from a stream of its own
        dt->ladder[lp.dim] = buf.release<double>();
    }
    *img = dt->ladder[lp.dim];
    return PCX_OK;
}

// N device-resident rows, queued on st: row r reads fixed[r * fstride + i] and xs[r * xstride + x].  Caller holds h->mu.
PCX_HIDDEN int bary_ladder_launch(pcx_bary *h, const BaryLadder &lp, const int32_t *deriv, const double *d_fixed, long fstride,
                                  const double *d_xs, long xstride, int m, long N, double *d_out, hipStream_t st) {
    if (N == 0 || m == 0) return PCX_OK;
    DerivedTensor *dt = nullptr;
    h->call_mark = h->clock;
    int rc = bary_get_tensor(h, deriv, &dt);
    if (rc) return rc;
    if (lp.CT) {
        const double *img = nullptr;
        if ((rc = bary_ladder_image(h, dt, lp, &img))) return rc;
        const size_t lds = ladder_mfma_lds(lp);
        const long blocks = (N + 15) / 16;
        if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
#define PCX_LADDER_GO(CT)                                                                                                  \
        hipLaunchKernelGGL((k_bary_ladder_mfma<CT>), dim3((unsigned)blocks), dim3(64), lds, st, h->dims, lp, h->d_nodes,    \
                           h->d_wts, img, d_fixed, fstride, d_xs, xstride, m, d_out, N)
        switch (lp.CT) {
        case 1: PCX_LADDER_GO(1); break;
        case 2: PCX_LADDER_GO(2); break;
        case 3: PCX_LADDER_GO(3); break;
        default: PCX_LADDER_GO(4); break;
        }
#undef PCX_LADDER_GO
        HIP_TRY(hipGetLastError());
        return PCX_OK;
    }
    const int ppw = 256 / h->lpp;
    const size_t lds = (size_t)ppw * (h->dims.sum_n + lp.n) * sizeof(double);
    if (lds > 160 * 1024) return fail(PCX_ERR_UNSUPPORTED, "sum of node counts %d too large for the rows kernel", h->dims.sum_n);
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)k_bary_ladder_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long blocks = (N + ppw - 1) / ppw;
    if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
    hipLaunchKernelGGL(k_bary_ladder_rows, dim3((unsigned)blocks), dim3(256), lds, st, h->dims, lp, h->lpp, h->d_nodes, h->d_wts,
                       dt->plain, d_fixed, fstride, d_xs, xstride, m, d_out, N);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

// ladder_check on the handle's dimensions, then the plan (its dim check has passed by then)
static int bary_ladder_check(pcx_bary *h, int dim, const int32_t *deriv, const void *fixed, int64_t N, const void *xs, int m,
                             int xs_per_row, const void *out, BaryLadder *lp) {
    const int rc = ladder_check(h, h ? h->dims.d : 0, dim, deriv, fixed, N, xs, m, xs_per_row, out);
    return rc ? rc : bary_ladder_plan(h, dim, lp);
}

extern "C" int pcx_bary_ladder_batch_dev(pcx_bary *h, int dim, const int32_t *deriv, const double *d_fixed, int64_t N,
                                         const double *xs, int m, int xs_per_row, double *d_out, void *stream) {
    PCX_API_BEGIN
    BaryLadder lp;
    int rc = bary_ladder_check(h, dim, deriv, d_fixed, N, xs, m, xs_per_row, d_out, &lp);
    if (rc) return rc;
    if (N == 0 || m == 0) return PCX_OK;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    if (xs_per_row) return bary_ladder_launch(h, lp, deriv, d_fixed, lp.nq, xs, m, m, (long)N, d_out, st);
    // shared values come from the host: a buffer of this call's, so the call waits for its kernel before it frees it
    DevBuf dxs;
    const double *d_shared = nullptr;
    if ((rc = ladder_shared_xs(dxs, xs, m, true, st, &d_shared))) return rc;
    rc = bary_ladder_launch(h, lp, deriv, d_fixed, lp.nq, d_shared, 0, m, (long)N, d_out, st);
    const hipError_t e = hipStreamSynchronize(st);
    if (rc) return rc;
    HIP_TRY(e);
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_bary_ladder_batch(pcx_bary *h, int dim, const int32_t *deriv, const double *fixed, int64_t N,
                                     const double *xs, int m, int xs_per_row, double *out) {
    PCX_API_BEGIN
    BaryLadder lp;
    int rc = bary_ladder_check(h, dim, deriv, fixed, N, xs, m, xs_per_row, out, &lp);
    if (rc) return rc;
    if (N == 0 || m == 0) return PCX_OK;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    DevBuf dxs;
    const double *d_shared = nullptr;
    if (!xs_per_row && (rc = ladder_shared_xs(dxs, xs, m, false, nullptr, &d_shared))) return rc;
    return ladder_host_passes(h->stage, h->device, h->stream, lp.nq, fixed, N, xs, d_shared, m, xs_per_row, out,
                              [&](const double *df, long fs, const double *dx, long xstr, long cnt, double *dout, hipStream_t st) {
                                  return bary_ladder_launch(h, lp, deriv, df, fs, dx, xstr, m, cnt, dout, st);
                              });
    PCX_API_END
}

extern "C" int pcx_bary_ladder_info(pcx_bary *h, int dim, int32_t *info) {
    PCX_API_BEGIN
    if (!h || !info) return fail(PCX_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    BaryLadder lp;
    int rc = bary_ladder_plan(h, dim, &lp);
    if (rc) return rc;
    info[0] = lp.CT ? 1 : 0;
    info[1] = lp.CT ? (int)std::min<long>(lp.Khi * (lp.Klo4 / 4), 0x7fffffffL) : 0;
    info[2] = lp.CT;
    return PCX_OK;
    PCX_API_END
}
