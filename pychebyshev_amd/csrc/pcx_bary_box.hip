// pcx_bary_box.hip -- C ABI of libpcx_hip.so (see include/pcx.h): batched box integrals of the full-tensor
// barycentric interpolant.  gfx950 only.

#include "pcx_bary_internal.h"
#include "bary_box_kernels.h"

// flags: d entries by dimension; lo / hi: the domain.  The row offsets follow the dimensions in order.
static int bary_box_plan(const pcx_bary *h, const int32_t *flags, const double *lo, const double *hi, BaryBoxCols *cols) {
    const int d = h->dims.d;
    *cols = BaryBoxCols{};
    int width = 0;
    for (int k = 0; k < d; ++k) {
        if (flags[k] != 0 && flags[k] != 1) return fail(PCX_ERR_INVALID, "flags[%d] = %d is neither 0 nor 1", k, (int)flags[k]);
        if (!(lo[k] < hi[k]) || !std::isfinite(lo[k]) || !std::isfinite(hi[k]))
            return fail(PCX_ERR_INVALID, "domain[%d]: lo must be < hi", k);
        cols->off[k] = width;
        cols->integ[k] = flags[k];
        cols->qoff[k] = h->doff[k];
        cols->a[k] = lo[k];
        cols->scale[k] = 2.0 / (hi[k] - lo[k]);
        cols->half[k] = (hi[k] - lo[k]) / 2.0;
        width += 1 + flags[k];
    }
    cols->width = width;
    return PCX_OK;
}

// The handle's box table: Q_n per dimension (n_k x n_k, row j = node j ascending, at doff[k]) and behind them, at
// box_rinv_offset, 1 / j for j = 1 .. max n + 1 (entry 0 unused).
static size_t box_rinv_offset(const pcx_bary *h) {
    const int last = h->dims.d - 1;
    return (size_t)h->doff[last] + (size_t)h->dims.n[last] * h->dims.n[last];
}

// Uploaded on the first box call.  Caller holds h->mu.
static int bary_box_tables(pcx_bary *h) {
    if (h->d_boxq) return PCX_OK;
    const int d = h->dims.d;
    const double pi = 3.14159265358979323846;
    int nmax = 1;
    for (int k = 0; k < d; ++k) nmax = std::max(nmax, h->dims.n[k]);
    const size_t sum_n2 = box_rinv_offset(h);
    std::vector<double> tab(sum_n2 + (size_t)nmax + 2, 0.0);
    for (int k = 0; k < d; ++k) {
        const int n = h->dims.n[k];
        double *Q = tab.data() + h->doff[k];
        for (int j = 0; j < n; ++j) {
            Q[(size_t)j * n] = 1.0 / n;
            for (int q = 1; q < n; ++q)
                Q[(size_t)j * n + q] = (2.0 / n) * std::cos(pi * (double)q * (double)(2 * (n - 1 - j) + 1) / (2.0 * n));
        }
    }
    for (int j = 1; j <= nmax + 1; ++j) tab[sum_n2 + j] = 1.0 / (double)j;
    DevBuf buf;
    int rc = buf.alloc(tab.size() * sizeof(double));
    if (rc) return rc;
    HIP_TRY(hipMemcpy(buf.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    h->d_boxq = buf.release<double>();
    return PCX_OK;
}

// LDS of one wave of the MFMA form: its weight table and its B operands
static size_t box_wave_lds(const pcx_bary *h, int nt) {
    return ((size_t)h->plan.rows * 16 * nt + (size_t)h->plan.KS * nt * 64) * sizeof(double);
}

// Geometry of the MFMA form: column tiles per wave (0: the rows form) and waves per workgroup.  The MFMA form serves
// handles whose fragment image is the row-code packing -- unless auto evaluates them on a lane-per-point kernel (a few
// row tiles: the MFMA form would be all prologue) and no variant was asked for.  Four-wave workgroups with two column
// tiles, then with one, while two of them share a CU's LDS (80 KB each); longer plans run one wave per workgroup with
// one column tile, so that the CU holds as many waves as its LDS allows (11^5: 22 KB per wave, seven waves).
static int box_mfma_nt(const pcx_bary *h, int *wpb = nullptr) {
    int w = 4, nt = 0;
    if (!h->mfma_ok || h->grid_ok || h->kfold_ok || h->variant == 1) return 0;
    if (h->variant == 0 && (h->small_preferred || h->sq_preferred)) return 0;
    if (4 * box_wave_lds(h, 2) <= (size_t)80 * 1024) nt = 2;
    else if (4 * box_wave_lds(h, 1) <= (size_t)80 * 1024) nt = 1;
    else if (box_wave_lds(h, 1) <= (size_t)160 * 1024) { nt = 1; w = 1; }
    if (wpb) *wpb = w;
    return nt;
}

// N device-resident rows, queued on st.  Caller holds h->mu.
static int bary_box_launch(pcx_bary *h, const BaryBoxCols &cols, const double *d_rows, long N, double *d_out, hipStream_t st) {
    if (N == 0) return PCX_OK;
    int rc = bary_box_tables(h);
    if (rc) return rc;
    const double *rinv = h->d_boxq + box_rinv_offset(h);
    DerivedTensor *dt = nullptr;
    h->call_mark = h->clock;
    if ((rc = bary_get_tensor(h, nullptr, &dt))) return rc;
    int wpb = 4;
    const int nt = box_mfma_nt(h, &wpb);
    if (nt) {
        if (!dt->frag) return fail(PCX_ERR_HIP, "the handle has no fragment image");
        const size_t lds = wpb * box_wave_lds(h, nt);
        const long blocks = (N + 16 * nt * wpb - 1) / (16 * nt * wpb);
        if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
#define PCX_BOX_GO(NT)                                                                                                      \
        do {                                                                                                                \
            if (lds > 64 * 1024)                                                                                            \
                HIP_TRY(hipFuncSetAttribute((const void *)k_bary_box_mfma<NT>, hipFuncAttributeMaxDynamicSharedMemorySize,  \
                                            (int)lds));                                                                     \
            hipLaunchKernelGGL((k_bary_box_mfma<NT>), dim3((unsigned)blocks), dim3(64 * wpb), lds, st, h->dims, h->plan, cols,   \
                               h->wide ? 1 : 0, h->d_nodes, h->d_wts, h->d_boxq, rinv, dt->frag, h->d_rowcode, h->d_kcode,  \
                               h->d_rowcode_hi, h->d_kcode_hi, d_rows, d_out, N);                                           \
        } while (0)
        if (nt == 2) PCX_BOX_GO(2); else PCX_BOX_GO(1);
#undef PCX_BOX_GO
        HIP_TRY(hipGetLastError());
        return PCX_OK;
    }
    const int ppw = 256 / h->lpp;
    const size_t lds = (size_t)ppw * h->dims.sum_n * sizeof(double);
    if (lds > 160 * 1024) return fail(PCX_ERR_UNSUPPORTED, "sum of node counts %d too large for the rows kernel", h->dims.sum_n);
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)k_bary_box_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long blocks = (N + ppw - 1) / ppw;
    if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
    hipLaunchKernelGGL(k_bary_box_rows, dim3((unsigned)blocks), dim3(256), lds, st, h->dims, cols, h->lpp, h->d_nodes, h->d_wts,
                       h->d_boxq, rinv, dt->plain, d_rows, d_out, N);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

static int bary_box_check(pcx_bary *h, const int32_t *flags, const double *lo, const double *hi, const void *rows,
                          int64_t N, const void *out, BaryBoxCols *cols) {
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    if (!flags || !lo || !hi) return fail(PCX_ERR_INVALID, "NULL flags or domain");
    if (N < 0) return fail(PCX_ERR_INVALID, "N < 0");
    if (N > 0 && (!rows || !out)) return fail(PCX_ERR_INVALID, "NULL buffer");
    return bary_box_plan(h, flags, lo, hi, cols);
}

extern "C" int pcx_bary_box_batch_dev(pcx_bary *h, const int32_t *flags, const double *lo, const double *hi,
                                      const double *d_rows, int64_t N, double *d_out, void *stream) {
    PCX_API_BEGIN
    BaryBoxCols cols;
    int rc = bary_box_check(h, flags, lo, hi, d_rows, N, d_out, &cols);
    if (rc) return rc;
    if (N == 0) return PCX_OK;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    return bary_box_launch(h, cols, d_rows, (long)N, d_out, stream ? (hipStream_t)stream : h->stream);
    PCX_API_END
}

extern "C" int pcx_bary_box_batch(pcx_bary *h, const int32_t *flags, const double *lo, const double *hi, const double *rows,
                                  int64_t N, double *out) {
    PCX_API_BEGIN
    BaryBoxCols cols;
    int rc = bary_box_check(h, flags, lo, hi, rows, N, out, &cols);
    if (rc) return rc;
    if (N == 0) return PCX_OK;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    // ~10 MB of rows per piece, two slots from two pieces on (as pcx_tt_box_batch)
    const int w = cols.width;
    const int64_t piece = std::max<int64_t>(65536, (((int64_t)10 << 20) / (w * 8)) & ~(int64_t)65535);
    const bool piped = N >= 2 * piece;
    const int64_t chunk = piped ? piece : kChunkPoints;
    return stage_host_batch(h->stage, h->device, h->stream, rows, N, w, 1, out, StagePlan{chunk, chunk, piped, true},
                            [&](int, hipStream_t st, const double *dp, long cnt, double *dout) {
                                return bary_box_launch(h, cols, dp, cnt, dout, st);
                            });
    PCX_API_END
}

extern "C" int pcx_bary_box_info(pcx_bary *h, int32_t *info) {
    PCX_API_BEGIN
    if (!h || !info) return fail(PCX_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    const int nt = box_mfma_nt(h);
    info[0] = nt ? 1 : 0;
    info[1] = nt ? h->plan.KS : 0;
    info[2] = nt ? h->plan.R : 0;
    info[3] = nt ? (h->wide ? 1 : 0) : 0;
    return PCX_OK;
    PCX_API_END
}
