// pcx_mode_product.hip -- the rectangular FP64 mode product and what is built from it: tensor-product grid evaluation
// of the barycentric handle (pcx_bary_eval_tensor_grid[_dev]) and of tensor-train value cores (pcx_tt_tensor_grid).
// gfx950 only.
//
// A grid x_0 x ... x x_{d-1} needs no per-point contraction: the result is the value tensor multiplied along each axis
// by the m_k x n_k matrix W_k of barycentric weights (grid_plan.h), prod m . n flops in all instead of prod m . prod n.
// Every device buffer is allocated before the first launch.

#include <climits>
#include <cstdlib>

#include "pcx_bary_internal.h"
#include "grid_plan.h"
#include "mode_product_kernels.h"

static const long kMpMaxBlocks = 1L << 20;       // grid-stride kernels: more blocks than this buy nothing
static const size_t kMpLdsBytes = 48 * 1024;     // W of an inner == 1 pass is staged in LDS up to this size (three workgroups per CU)
static const long kMpMaxCount = 1L << 40;        // elements of X, W or Y

// The form auto picks (profiles/eval_grid_probe.txt): the MFMA form, which was never the slower one at any
// measured pass -- n from 3 to 64, tiles down to 4 live rows or columns -- and up to 4.7x faster where a pass writes
// tens of MB.  Below a quarter of a tile in either direction (m < 4, or fewer than 4 columns: inner, or outer when
// inner == 1) nothing was measured; the VALU form does no dead work there and keeps those shapes.
static int mode_product_auto(long outer, long inner, int m) {
    const long cols = inner > 1 ? inner : outer;
    return m >= 4 && cols >= 4 ? 2 : 1;
}

// Y = W x_axis X on `st`; X, W, Y (and hot, may be NULL) in HBM.  variant 0 auto, 1 VALU, 2 MFMA.
static int mode_product_launch(const double *X, const double *W, double *Y, long outer, int n, long inner, long m_rows, int variant,
                               const int *hot, hipStream_t st) {
    if (outer < 1 || n < 1 || inner < 1 || m_rows < 1) return fail(PCX_ERR_INVALID, "mode product: outer, n, inner and m must be at least 1");
    if (m_rows > INT_MAX) return fail(PCX_ERR_UNSUPPORTED, "mode product: m=%ld exceeds 2^31 - 1", m_rows);
    const int m = (int)m_rows;
    if (variant < 0 || variant > 2) return fail(PCX_ERR_INVALID, "mode product: variant %d outside [0, 2]", variant);
    if ((double)outer * n * (double)inner > (double)kMpMaxCount || (double)outer * m * (double)inner > (double)kMpMaxCount)
        return fail(PCX_ERR_UNSUPPORTED, "mode product: more than 2^40 elements");
    if (variant == 0) variant = mode_product_auto(outer, inner, m);
    if (variant == 1) {
        const long total = outer * m * inner;
        const long blocks = std::min(kMpMaxBlocks, (total + PCX_MP_THREADS - 1) / PCX_MP_THREADS);
        hipLaunchKernelGGL(k_mode_product_rect, dim3((unsigned)blocks), dim3(PCX_MP_THREADS), 0, st, X, W, Y, outer, n, inner, m, hot);
    } else if (inner > 1) {
        const int MT = (m + 15) / 16;
        const long QT = (inner + 15) / 16;
        const long tiles = outer * MT * QT;
        const long blocks = std::min(kMpMaxBlocks, (tiles + PCX_MP_WAVES - 1) / PCX_MP_WAVES);
        hipLaunchKernelGGL(k_mode_product_mfma, dim3((unsigned)blocks), dim3(PCX_MP_THREADS), 0, st, X, W, Y, outer, n, inner, m, MT,
                           QT, tiles, hot);
    } else {
        const int MT = (m + 15) / 16;
        const long tiles = ((outer + 15) / 16) * MT;
        const long blocks = std::min(kMpMaxBlocks, (tiles + PCX_MP_WAVES - 1) / PCX_MP_WAVES);
        const int ldw = n | 1;
        const size_t lds = (size_t)m * ldw * sizeof(double);
        // staging W pays when a workgroup walks several tiles with it, and it has to fit
        if (lds <= kMpLdsBytes)
            hipLaunchKernelGGL((k_mode_product_mfma_last<true>), dim3((unsigned)blocks), dim3(PCX_MP_THREADS), lds, st, X, W, Y,
                               outer, n, m, MT, tiles, ldw, hot);
        else
            hipLaunchKernelGGL((k_mode_product_mfma_last<false>), dim3((unsigned)blocks), dim3(PCX_MP_THREADS), 0, st, X, W, Y,
                               outer, n, m, MT, tiles, ldw, hot);
    }
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

// PCX_GRID_VARIANT=1|2 forces one form on every pass of the orchestrators (A/B runs: tools/eval_grid_probe.py)
static int grid_env_variant() {
    const char *v = getenv("PCX_GRID_VARIANT");
    const int k = v ? atoi(v) : 0;
    return k == 1 || k == 2 ? k : 0;
}

// PCX_GRID_LOG=1: every pass of the orchestrators is timed on its own (two events and a wait per pass) and reported on
// stderr with the bytes it wrote -- the last pass's write bandwidth of tools/eval_grid_probe.py.  Slows the call down.
struct PassLog {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool on = false;
    PassLog() {
        on = getenv("PCX_GRID_LOG") != nullptr && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
    }
    ~PassLog() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    void begin(hipStream_t st) { if (on) (void)hipEventRecord(e0, st); }
    void end(hipStream_t st, const char *what, int pass, int passes, long outer, int n, long inner, long m, int variant) {
        if (!on) return;
        float ms = 0.f;
        if (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return;
        const double out_bytes = 8.0 * (double)outer * (double)m * (double)inner, in_bytes = 8.0 * ((double)outer * n * (double)inner + (double)m * n);
        fprintf(stderr, "[pcx] %s pass %d/%d: outer %ld n %d inner %ld m %ld form %s: %.1f us, writes %.2f MB at %.0f GB/s, reads %.2f MB (X and W)\n",
                what, pass + 1, passes, outer, n, inner, m,
                (variant ? variant : mode_product_auto(outer, inner, (int)m)) == 2 ? "mfma" : "valu", ms * 1e3, out_bytes / 1e6,
                ms > 0.f ? out_bytes / (ms * 1e6) : 0.0, in_bytes / 1e6);
    }
};

extern "C" int pcx_tensor_mode_product(int device, int64_t outer, int n, int64_t inner, const double *X, int m, const double *W,
                                       double *Y, int variant) {
    PCX_API_BEGIN
    if (!X || !W || !Y) return fail(PCX_ERR_INVALID, "NULL argument");
    if (outer < 1 || n < 1 || inner < 1 || m < 1) return fail(PCX_ERR_INVALID, "outer, n, inner and m must be at least 1");
    if (variant < 0 || variant > 2) return fail(PCX_ERR_INVALID, "variant %d outside [0, 2]", variant);
    if ((double)outer * n * (double)inner > (double)kMpMaxCount || (double)outer * m * (double)inner > (double)kMpMaxCount)
        return fail(PCX_ERR_UNSUPPORTED, "more than 2^40 elements");
    int rc = use_device(device);
    if (rc) return rc;
    // one-hot rows of W are gathers (mode_product_kernels.h)
    std::vector<int> hot((size_t)m, -1);
    for (int j = 0; j < m; ++j) {
        int at = -1, others = 0;
        for (int i = 0; i < n; ++i) {
            const double w = W[(size_t)j * n + i];
            if (w == 1.0 && at < 0) at = i;
            else if (w != 0.0) ++others;
        }
        if (at >= 0 && others == 0) hot[j] = at;
    }
    const size_t xc = (size_t)outer * n * inner, wc = (size_t)m * n, yc = (size_t)outer * m * inner;
    DevBuf dx, dw, dy, dh;
    if ((rc = dx.alloc(xc * sizeof(double))) || (rc = dw.alloc(wc * sizeof(double))) || (rc = dy.alloc(yc * sizeof(double))) ||
        (rc = dh.alloc((size_t)m * sizeof(int))))
        return rc;
    HIP_TRY(hipMemcpy(dx.p, X, xc * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dw.p, W, wc * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dh.p, hot.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice));
    if ((rc = mode_product_launch(dx.as<double>(), dw.as<double>(), dy.as<double>(), (long)outer, n, (long)inner, m, variant,
                                  dh.as<int>(), 0)))
        return rc;
    HIP_TRY(hipMemcpy(Y, dy.p, yc * sizeof(double), hipMemcpyDeviceToHost));
    return PCX_OK;
    PCX_API_END
}

// ---------------------------------------------------------------------------------
// barycentric handle on a tensor-product grid
// ---------------------------------------------------------------------------------
// The d passes of the plan on `st`, from the derivative tensor of `deriv` into d_out (device).  Caller holds h->mu.
static int bary_grid_run(pcx_bary *h, const int32_t *deriv, const int32_t *m, const double *axes_cat, double *d_out, hipStream_t st) {
    const int d = h->dims.d;
    GridPlan gp;
    char err[PCX_ERR_LEN];
    int rc = grid_make_plan(d, h->dims.n, h->h_nodes.data(), h->h_wts.data(), m, axes_cat, gp, err, sizeof err);
    if (rc) return fail(rc, "%s", err);
    for (const GridPass &ps : gp.passes)
        if (ps.out_count > kMpMaxCount) return fail(PCX_ERR_UNSUPPORTED, "grid pass along dimension %d: more than 2^40 elements", ps.dim);
    // the buffers of an earlier call may still be read on another stream
    if (h->grid_done) HIP_TRY(hipEventSynchronize(h->grid_done));
    else HIP_TRY(hipEventCreateWithFlags(&h->grid_done, hipEventDisableTiming));
    // W_k, then the one-hot columns (int32) behind them: one upload
    const size_t wcount = gp.W.size(), hcount = (gp.hot.size() + 1) / 2;
    h->grid_w_host.assign(wcount + hcount, 0.0);
    memcpy(h->grid_w_host.data(), gp.W.data(), wcount * sizeof(double));
    memcpy(h->grid_w_host.data() + wcount, gp.hot.data(), gp.hot.size() * sizeof(int32_t));
    if ((rc = h->s_gridw.reserve(h->grid_w_host.size() * sizeof(double)))) return rc;
    for (Scratch &sc : h->s_grid)
        if ((rc = sc.reserve((size_t)gp.max_intermediate * sizeof(double)))) return rc;
    // the derivative tensor last: building it launches, and no allocation of this call may follow a launch
    h->call_mark = h->clock;
    DerivedTensor *dt = nullptr;
    if ((rc = bary_get_tensor(h, deriv, &dt))) return rc;
    HIP_TRY(hipMemcpyAsync(h->s_gridw.ptr, h->grid_w_host.data(), h->grid_w_host.size() * sizeof(double), hipMemcpyHostToDevice, st));
    const double *d_w = (const double *)h->s_gridw.ptr;
    const int *d_hot = (const int *)(d_w + wcount);
    const int variant = grid_env_variant();
    const double *src = dt->plain;
    PassLog log;
    for (int p = 0; p < d; ++p) {
        const GridPass &ps = gp.passes[p];
        double *dst = p + 1 == d ? d_out : (double *)h->s_grid[p & 1].ptr;
        log.begin(st);
        if ((rc = mode_product_launch(src, d_w + ps.w_off, dst, ps.outer, ps.n, ps.inner, ps.m, variant, d_hot + gp.hot_off[ps.dim], st)))
            return rc;
        log.end(st, "grid", p, d, ps.outer, ps.n, ps.inner, ps.m, variant);
        src = dst;
    }
    HIP_TRY(hipEventRecord(h->grid_done, st));
    return PCX_OK;
}

static int bary_grid_check(pcx_bary *h, const int32_t *m, const double *axes_cat, const void *out, long *total) {
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    if (!m || !axes_cat || !out) return fail(PCX_ERR_INVALID, "NULL argument");
    *total = 1;
    for (int k = 0; k < h->dims.d; ++k) {
        if (m[k] < 1) return fail(PCX_ERR_INVALID, "m[%d]=%d: the axis of dimension %d is empty", k, m[k], k);
        if ((double)*total * m[k] > (double)kMpMaxCount) return fail(PCX_ERR_UNSUPPORTED, "grid of more than 2^40 points");
        *total *= m[k];
    }
    return PCX_OK;
}

extern "C" int pcx_bary_eval_tensor_grid_dev(pcx_bary *h, const int32_t *deriv, const int32_t *m, const double *axes_cat,
                                             double *d_out, void *stream) {
    PCX_API_BEGIN
    long total = 0;
    int rc = bary_grid_check(h, m, axes_cat, d_out, &total);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    return bary_grid_run(h, deriv, m, axes_cat, d_out, stream ? (hipStream_t)stream : h->stream);
    PCX_API_END
}

extern "C" int pcx_bary_eval_tensor_grid(pcx_bary *h, const int32_t *deriv, const int32_t *m, const double *axes_cat, double *out) {
    PCX_API_BEGIN
    long total = 0;
    int rc = bary_grid_check(h, m, axes_cat, out, &total);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->grid_done) HIP_TRY(hipEventSynchronize(h->grid_done));      // s_gridout may still be written
    if ((rc = h->s_gridout.reserve((size_t)total * sizeof(double)))) return rc;
    rc = bary_grid_run(h, deriv, m, axes_cat, (double *)h->s_gridout.ptr, h->stream);
    if (!rc) {
        const hipError_t e = hipMemcpyAsync(out, h->s_gridout.ptr, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, h->stream);
        if (e != hipSuccess) rc = fail(PCX_ERR_HIP, "download of the grid: %s", hipGetErrorString(e));
    }
    const hipError_t es = hipStreamSynchronize(h->stream);          // whatever happened, nothing is left queued
    if (rc) return rc;
    HIP_TRY(es);
    return PCX_OK;
    PCX_API_END
}

// ---------------------------------------------------------------------------------
// tensor-train value cores on a grid: the dense tensor as a chain of mode products
// ---------------------------------------------------------------------------------
extern "C" int pcx_tt_tensor_grid(int device, int d, const int32_t *m, const int32_t *ranks, const double *grid_cores_cat, double *out) {
    PCX_API_BEGIN
    if (!grid_cores_cat || !out) return fail(PCX_ERR_INVALID, "NULL argument");
    TTGridPlan tp;
    char err[PCX_ERR_LEN];
    int rc = tt_grid_make_plan(d, m, ranks, tp, err, sizeof err);
    if (rc) return fail(rc, "%s", err);
    if (tp.total > kMpMaxCount) return fail(PCX_ERR_UNSUPPORTED, "grid of more than 2^40 points");
    for (const TTGridStep &s : tp.steps)
        if (s.m > INT_MAX) return fail(PCX_ERR_UNSUPPORTED, "chain step at core %d: %lld rows exceed 2^31 - 1", s.core, (long long)s.m);
    if ((rc = use_device(device))) return rc;
    const size_t ccount = (size_t)tp.core_off[d];
    if (d == 1) {                                    // the only core IS the result
        memcpy(out, grid_cores_cat, ccount * sizeof(double));
        return PCX_OK;
    }
    DevBuf dc, dres, ping[2];
    if ((rc = dc.alloc(ccount * sizeof(double))) || (rc = dres.alloc((size_t)tp.total * sizeof(double)))) return rc;
    for (DevBuf &b : ping)
        if ((rc = b.alloc((size_t)tp.max_intermediate * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpy(dc.p, grid_cores_cat, ccount * sizeof(double), hipMemcpyHostToDevice));
    const int variant = grid_env_variant();
    const double *cores = dc.as<double>();
    const double *run = cores + tp.core_off[tp.from_right ? d - 1 : 0];
    PassLog log;
    for (size_t s = 0; s < tp.steps.size(); ++s) {
        const TTGridStep &stp = tp.steps[s];
        const double *core = cores + tp.core_off[stp.core];
        double *dst = s + 1 == tp.steps.size() ? dres.as<double>() : ping[s & 1].as<double>();
        log.begin(0);
        if ((rc = mode_product_launch(stp.w_is_core ? run : core, stp.w_is_core ? core : run, dst, 1, stp.n, (long)stp.inner, (long)stp.m,
                                      variant, nullptr, 0)))
            return rc;
        log.end(0, tp.from_right ? "tt chain (from the right)" : "tt chain (from the left)", (int)s, d - 1, 1, stp.n, (long)stp.inner,
                (long)stp.m, variant);
        run = dst;
    }
    HIP_TRY(hipMemcpy(out, dres.p, (size_t)tp.total * sizeof(double), hipMemcpyDeviceToHost));
    return PCX_OK;
    PCX_API_END
}
