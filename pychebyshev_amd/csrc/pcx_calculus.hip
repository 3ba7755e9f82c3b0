// pcx_calculus.hip -- C ABI of libpcx_hip.so (see include/pcx.h): roots, minima and maxima of an interpolant along one
// dimension, batched over rows of fixed values of the other dimensions (reference _calculus.py:198-355).  gfx950 only.
//
// A handle entry expands every row into the n points (fixed..., x_j) of its fibre (k_calc_expand, x_j the handle's own
// node values), evaluates them with the handle's existing device evaluation (the node rule of the barycentric kernels
// makes the weight of dimension `dim` one-hot there) and solves every fibre with k_cheb1d_calculus.  Fibres and results
// stay in HBM until the one download of the results.
//
// The slider entry (pcx_slider_calculus_batch) uses the slider's structure instead of its evaluation: along `dim` only
// the slide that owns `dim` varies, so every other slide is evaluated once per row and the owner once per fibre point --
// or not at all when it is one-dimensional, its value tensor being the fibre.  k_slider_fibre_sum then adds them up in
// the evaluation's order and the same solver runs.
//
// The spline entry (pcx_spline_calculus_batch) has P pieces along `dim`, each with its own interval and node count: the
// fibre points of all pieces go through the spline's own chunk evaluation (spline_eval_chunk: route, bucket, the pieces'
// barycentric kernels), one launch solves the rows x P fibres (k_cheb1d_calculus_pieces, the same calc_row) and
// k_spline_calc_merge joins the pieces of every row (spline_calc_kernels.h).

#include "pcx_slider_internal.h"
#include "pcx_spline_internal.h"
#include "calculus_kernels.h"
#include "slider_calc_kernels.h"
#include "spline_calc_kernels.h"

// rows per pass of the expand / evaluate / solve pipeline: at most this many fibre points in flight
static const long kCalcChunkPoints = 1L << 21;

static int calc_check(int n, int mode, int64_t N, double lo, double hi, const double *diff, double *roots_out,
                      int32_t *counts_out, double *val_out, double *loc_out) {
    if (n < 1 || n > PCX_CALC_MAX_N)
        return fail(PCX_ERR_INVALID, "n=%d outside [1, %d]: the device root solver takes fibres of at most %d nodes", n,
                    PCX_CALC_MAX_N, PCX_CALC_MAX_N);
    if (mode < 0 || mode > 2) return fail(PCX_ERR_INVALID, "mode=%d (0 roots, 1 minimize, 2 maximize)", mode);
    if (N < 0) return fail(PCX_ERR_INVALID, "N=%lld < 0", (long long)N);
    if (!(lo < hi)) return fail(PCX_ERR_INVALID, "domain: lo must be < hi");
    if (!counts_out) return fail(PCX_ERR_INVALID, "counts_out is NULL");
    if (mode == 0 && !roots_out) return fail(PCX_ERR_INVALID, "roots_out is NULL");
    if (mode != 0 && (!val_out || !loc_out)) return fail(PCX_ERR_INVALID, "val_out / loc_out is NULL");
    if (mode != 0 && !diff) return fail(PCX_ERR_INVALID, "diff is NULL (modes 1 and 2 need the differentiation matrix)");
    return PCX_OK;
}

// device outputs of a batch of N rows
struct CalcDevOut {
    DevBuf roots, counts, val, loc;
    int alloc(int mode, long N, int W) {
        int rc = counts.alloc((size_t)N * sizeof(int32_t));
        if (!rc && mode == 0) rc = roots.alloc((size_t)N * W * sizeof(double));
        if (!rc && mode != 0) rc = val.alloc((size_t)N * sizeof(double));
        if (!rc && mode != 0) rc = loc.alloc((size_t)N * sizeof(double));
        return rc;
    }
    int download(int mode, long N, int W, double *roots_out, int32_t *counts_out, double *val_out, double *loc_out,
                 hipStream_t st) {
        HIP_TRY(hipMemcpyAsync(counts_out, counts.p, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (mode == 0) {
            HIP_TRY(hipMemcpyAsync(roots_out, roots.p, (size_t)N * W * sizeof(double), hipMemcpyDeviceToHost, st));
        } else {
            HIP_TRY(hipMemcpyAsync(val_out, val.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(loc_out, loc.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
        return PCX_OK;
    }
};

// k_cheb1d_calculus over `rows` fibres (a.vals and the outputs already offset to the first row): one wave per fibre,
// the LDS class chosen by the largest colleague matrix a fibre of n nodes can produce (n - 1)
static int calc_launch(const CalcArgs &a, long rows, hipStream_t st) {
    if (rows <= 0) return PCX_OK;
    if (rows > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "too many rows for one launch");
    const int m = a.n - 1;
    if (m <= 16) hipLaunchKernelGGL(k_cheb1d_calculus<16>, dim3((unsigned)rows), dim3(64), 0, st, a);
    else if (m <= 32) hipLaunchKernelGGL(k_cheb1d_calculus<32>, dim3((unsigned)rows), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(k_cheb1d_calculus<64>, dim3((unsigned)rows), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

// fixed rows (N x (d - 1), the columns of every dimension but `dim` in increasing order) inside [lo, hi] of their
// dimensions; NaN passes, as in the reference's comparisons
static int calc_check_fixed(const double *fixed, int64_t N, int d, int dim, const double *lo, const double *hi) {
    if (d > 1 && N > 0 && !fixed) return fail(PCX_ERR_INVALID, "fixed is NULL");
    for (int64_t r = 0; r < N; ++r)
        for (int c = 0, k = 0; k < d; ++k) {
            if (k == dim) continue;
            const double v = fixed[r * (d - 1) + c++];
            if (v < lo[k] || v > hi[k])
                return fail(PCX_ERR_INVALID, "Fixed value %.17g for dim %d outside domain [%.17g, %.17g] (row %lld)", v, k,
                            lo[k], hi[k], (long long)r);
        }
    return PCX_OK;
}

// The pipeline of the handle entries: per pass of rows, expand -> evaluate (eval(d_pts, points, d_vals)) -> solve.
template <typename Eval>
static int calc_fibres(int d, int dim, int mode, const double *fixed, int64_t N, CalcArgs a, hipStream_t st, Eval eval,
                       double *roots_out, int32_t *counts_out, double *val_out, double *loc_out) {
    const int n = a.n;
    const long chunk = std::max<long>(1, std::min<long>(N, kCalcChunkPoints / n));
    DevBuf d_fixed, d_pts, d_vals;
    CalcDevOut out;
    int rc = d_fixed.alloc((size_t)N * (d - 1) * sizeof(double));
    if (!rc) rc = d_pts.alloc((size_t)chunk * n * d * sizeof(double));
    if (!rc) rc = d_vals.alloc((size_t)chunk * n * sizeof(double));
    if (!rc) rc = out.alloc(mode, N, a.W);
    if (rc) return rc;
    if (d > 1) HIP_TRY(hipMemcpyAsync(d_fixed.p, fixed, (size_t)N * (d - 1) * sizeof(double), hipMemcpyHostToDevice, st));
    for (long r0 = 0; r0 < N; r0 += chunk) {
        const long rows = std::min<long>(chunk, N - r0);
        const long total = rows * n * d;
        const unsigned blocks = (unsigned)std::min<long>((total + 255) / 256, 8192);
        hipLaunchKernelGGL(k_calc_expand, dim3(blocks), dim3(256), 0, st, d_fixed.as<double>() + (size_t)r0 * (d - 1), rows,
                           d, dim, n, a.nodes, d_pts.as<double>());
        HIP_TRY(hipGetLastError());
        if ((rc = eval(d_pts.as<double>(), rows * n, d_vals.as<double>()))) return rc;
        CalcArgs c = a;
        c.vals = d_vals.as<double>();
        c.counts = out.counts.as<int32_t>() + r0;
        if (mode == 0) c.roots = out.roots.as<double>() + (size_t)r0 * a.W;
        else { c.val = out.val.as<double>() + r0; c.loc = out.loc.as<double>() + r0; }
        if ((rc = calc_launch(c, rows, st))) return rc;
    }
    return out.download(mode, N, a.W, roots_out, counts_out, val_out, loc_out, st);
}

extern "C" int pcx_cheb1d_calculus(int device, int n, double lo, double hi, const double *nodes, const double *weights,
                                   const double *diff, const double *values, int64_t N, int mode, double *roots_out,
                                   int32_t *counts_out, double *val_out, double *loc_out) {
    PCX_API_BEGIN
    int rc = calc_check(n, mode, N, lo, hi, diff, roots_out, counts_out, val_out, loc_out);
    if (rc) return rc;
    if (!nodes || !weights || (N > 0 && !values)) return fail(PCX_ERR_INVALID, "NULL argument");
    if (N == 0) return PCX_OK;
    if ((rc = use_device(device))) return rc;
    const int W = std::max(n - 1, 1);
    DevBuf d_grid, d_vals;                                     // nodes, weights, D in one buffer
    CalcDevOut out;
    rc = d_grid.alloc((size_t)(2 * n + n * n) * sizeof(double));
    if (!rc) rc = d_vals.alloc((size_t)N * n * sizeof(double));
    if (!rc) rc = out.alloc(mode, N, W);
    if (rc) return rc;
    double *g = d_grid.as<double>();
    HIP_TRY(hipMemcpy(g, nodes, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g + n, weights, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    if (mode != 0) HIP_TRY(hipMemcpy(g + 2 * n, diff, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_vals.p, values, (size_t)N * n * sizeof(double), hipMemcpyHostToDevice));
    CalcArgs a{};
    a.n = n; a.mode = mode; a.W = W; a.lo = lo; a.hi = hi;
    a.nodes = g; a.wts = g + n; a.diff = g + 2 * n; a.vals = d_vals.as<double>();
    a.counts = out.counts.as<int32_t>();
    a.roots = out.roots.as<double>(); a.val = out.val.as<double>(); a.loc = out.loc.as<double>();
    if ((rc = calc_launch(a, (long)N, nullptr))) return rc;
    return out.download(mode, (long)N, W, roots_out, counts_out, val_out, loc_out, nullptr);
    PCX_API_END
}

extern "C" int pcx_bary_calculus_batch(pcx_bary *h, int dim, const double *lo, const double *hi, const double *fixed,
                                       int64_t N, int mode, double *roots_out, int32_t *counts_out, double *val_out,
                                       double *loc_out) {
    PCX_API_BEGIN
    if (!h || !lo || !hi) return fail(PCX_ERR_INVALID, "NULL argument");
    const int d = h->dims.d;
    if (dim < 0 || dim >= d) return fail(PCX_ERR_INVALID, "dim %d out of range [0, %d]", dim, d - 1);
    const int n = h->dims.n[dim];
    int rc = calc_check(n, mode, N, lo[dim], hi[dim], h->d_diff, roots_out, counts_out, val_out, loc_out);
    if (!rc) rc = calc_check_fixed(fixed, N, d, dim, lo, hi);
    if (rc) return rc;
    if (N == 0) return PCX_OK;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    h->call_mark = h->clock;
    DerivedTensor *dt = nullptr;
    if ((rc = bary_get_tensor(h, nullptr, &dt))) return rc;
    CalcArgs a{};
    a.n = n; a.mode = mode; a.W = std::max(n - 1, 1); a.lo = lo[dim]; a.hi = hi[dim];
    a.nodes = h->d_nodes + h->dims.off[dim];
    a.wts = h->d_wts + h->dims.off[dim];
    a.diff = h->d_diff + h->doff[dim];
    auto eval = [&](const double *d_pts, long npts, double *d_vals) {
        return bary_launch(h, &dt, 1, dt->slot, d_pts, npts, d_vals, 1, 0, h->stream, &h->s_partial);
    };
    return calc_fibres(d, dim, mode, fixed, N, a, h->stream, eval, roots_out, counts_out, val_out, loc_out);
    PCX_API_END
}

extern "C" int pcx_tt_calculus_batch(pcx_tt *h, int dim, const double *fixed, int64_t N, int mode, double *roots_out,
                                     int32_t *counts_out, double *val_out, double *loc_out) {
    PCX_API_BEGIN
    int device = 0;
    TTDims dims{};
    hipStream_t st = nullptr;
    int rc = tt_handle_view(h, &device, &dims, &st);
    if (rc) return rc;
    const int d = dims.d;
    if (dim < 0 || dim >= d) return fail(PCX_ERR_INVALID, "dim %d out of range [0, %d]", dim, d - 1);
    // the domain in the user's frame: user dimension dims.col[k] lives at storage position k
    double lo[PCX_MAX_DIMS], hi[PCX_MAX_DIMS];
    int nn[PCX_MAX_DIMS];
    for (int k = 0; k < d; ++k) {
        lo[dims.col[k]] = dims.lo[k];
        hi[dims.col[k]] = dims.hi[k];
        nn[dims.col[k]] = dims.n[k];
    }
    const int n = nn[dim];
    // the fibre's grid as the host builds it (barycentric.py chebyshev_nodes, compute_barycentric_weights,
    // compute_differentiation_matrix): ascending type-I nodes, weights by a division chain, D from the weights
    std::vector<double> grid((size_t)2 * n + (size_t)n * n);
    double *x = grid.data(), *w = x + n, *D = w + n;
    for (int j = 0; j < n; ++j) {
        const double t = std::sin(0.5 * M_PI / n * (double)(2 * j - n + 1));      // chebpts1, ascending
        x[j] = 0.5 * (lo[dim] + hi[dim]) + 0.5 * (hi[dim] - lo[dim]) * t;
    }
    std::sort(x, x + n);
    for (int i = 0; i < n; ++i) {
        w[i] = 1.0;
        for (int j = 0; j < n; ++j)
            if (j != i) w[i] /= (x[i] - x[j]);
    }
    for (int i = 0; i < n; ++i) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) {
            if (j == i) continue;
            D[(size_t)i * n + j] = w[j] / ((x[i] - x[j]) * w[i]);
            s += D[(size_t)i * n + j];
        }
        D[(size_t)i * n + i] = -s;
    }
    rc = calc_check(n, mode, N, lo[dim], hi[dim], D, roots_out, counts_out, val_out, loc_out);
    if (!rc) rc = calc_check_fixed(fixed, N, d, dim, lo, hi);
    if (rc) return rc;
    if (N == 0) return PCX_OK;
    HIP_TRY(hipSetDevice(device));
    DevBuf d_grid;
    if ((rc = d_grid.alloc(grid.size() * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpyAsync(d_grid.p, grid.data(), grid.size() * sizeof(double), hipMemcpyHostToDevice, st));
    CalcArgs a{};
    a.n = n; a.mode = mode; a.W = std::max(n - 1, 1); a.lo = lo[dim]; a.hi = hi[dim];
    a.nodes = d_grid.as<double>();
    a.wts = a.nodes + n;
    a.diff = a.nodes + 2 * n;
    auto eval = [&](const double *d_pts, long npts, double *d_vals) {
        return pcx_tt_eval_batch_dev(h, d_pts, npts, d_vals, (void *)st);   // points in the user's column order
    };
    rc = calc_fibres(d, dim, mode, fixed, N, a, st, eval, roots_out, counts_out, val_out, loc_out);
    (void)hipStreamSynchronize(st);                            // d_grid is freed on return
    return rc;
    PCX_API_END
}

// Columns of the (d - 1)-wide fixed rows (every dimension but `dim`, increasing) that hold the dimensions `dims[0 .. nc)`.
static SliderCols slider_fixed_cols(const int *dims, int nc, int dim) {
    SliderCols c;
    c.nc = nc;
    for (int k = 0; k < PCX_MAX_DIMS; ++k) c.col[k] = 0;
    for (int k = 0; k < nc; ++k) c.col[k] = dims[k] < dim ? dims[k] : dims[k] - 1;
    return c;
}

extern "C" int pcx_slider_calculus_batch(pcx_slider *h, int dim, const double *lo, const double *hi, const double *fixed,
                                         int64_t N, int mode, double *roots_out, int32_t *counts_out, double *val_out,
                                         double *loc_out) {
    PCX_API_BEGIN
    if (!h || !lo || !hi) return fail(PCX_ERR_INVALID, "NULL argument");
    const int d = h->d;
    if (dim < 0 || dim >= d) return fail(PCX_ERR_INVALID, "dim %d out of range [0, %d]", dim, d - 1);
    const int o = h->owner[dim];                               // the slide that owns dim, and dim's place in its group
    pcx_bary *po = h->slides[o];
    const SliderCols &oc = h->cols[o];
    int lk = 0;
    while (oc.col[lk] != dim) ++lk;
    const int g = oc.nc;
    const int n = po->dims.n[lk];
    int rc = calc_check(n, mode, N, lo[dim], hi[dim], po->d_diff, roots_out, counts_out, val_out, loc_out);
    if (!rc) rc = calc_check_fixed(fixed, N, d, dim, lo, hi);
    if (rc) return rc;
    if (N == 0) return PCX_OK;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk_h(h->mu);
    hipStream_t st = h->stream;
    const int ns = (int)h->slides.size();
    CalcArgs a{};
    a.n = n; a.mode = mode; a.W = std::max(n - 1, 1); a.lo = lo[dim]; a.hi = hi[dim];
    a.nodes = po->d_nodes + po->dims.off[lk];
    a.wts = po->d_wts + po->dims.off[lk];
    a.diff = po->d_diff + po->doff[lk];
    const long chunk = std::max<long>(1, std::min<long>(N, kCalcChunkPoints / n));
    // s_cols: a slide's gathered columns (chunk x nc), or the owner's gathered columns and behind them its fibre points
    const size_t own_cols = g > 1 ? (((size_t)chunk * (g - 1) + 31) & ~(size_t)31) : 0;      // the points stay 256-byte aligned
    const size_t cols_doubles = std::max<size_t>((size_t)chunk * h->max_cols, own_cols + (g > 1 ? (size_t)chunk * n * g : 0));
    DevBuf d_fixed, d_vals;
    CalcDevOut out;
    rc = h->s_cols.reserve(cols_doubles * sizeof(double));
    if (!rc) rc = h->s_vals.reserve((size_t)chunk * ns * sizeof(double));
    if (!rc) rc = d_fixed.alloc((size_t)N * (d - 1) * sizeof(double));
    if (!rc) rc = d_vals.alloc((size_t)chunk * n * sizeof(double));
    if (!rc) rc = out.alloc(mode, N, a.W);
    if (rc) return rc;
    if (d > 1) HIP_TRY(hipMemcpyAsync(d_fixed.p, fixed, (size_t)N * (d - 1) * sizeof(double), hipMemcpyHostToDevice, st));
    double *cols = (double *)h->s_cols.ptr, *svals = (double *)h->s_vals.ptr, *vals = d_vals.as<double>();
    for (long r0 = 0; r0 < N; r0 += chunk) {
        const long rows = std::min<long>(chunk, N - r0);
        const double *frows = d_fixed.as<double>() + (size_t)r0 * (d - 1);
        // every other slide once per row, into column s of svals (column o stays unread)
        for (int s = 0; s < ns; ++s) {
            if (s == o) continue;
            pcx_bary *pc = h->slides[s];
            const SliderCols c = slider_fixed_cols(h->cols[s].col, h->cols[s].nc, dim);
            const long elems = rows * c.nc;
            hipLaunchKernelGGL(k_gather_columns, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, frows, rows, d - 1, c, cols);
            HIP_TRY(hipGetLastError());
            std::lock_guard<std::mutex> plk(pc->mu);
            pc->call_mark = pc->clock;
            DerivedTensor *dt = nullptr;
            if ((rc = bary_get_tensor(pc, nullptr, &dt))) return rc;
            if ((rc = bary_launch(pc, &dt, 1, dt->slot, cols, rows, svals, ns, s, st, &h->s_partial))) return rc;
        }
        {
            std::lock_guard<std::mutex> plk(po->mu);
            po->call_mark = po->clock;
            DerivedTensor *dt = nullptr;
            if ((rc = bary_get_tensor(po, nullptr, &dt))) return rc;
            const double *plain = dt->plain;                   // one-dimensional owner: its value tensor is the fibre
            if (g > 1) {
                // the owner's other columns (group order), expanded into the n fibre points of the group's own frame
                int others[PCX_MAX_DIMS];
                for (int k = 0, c = 0; k < g; ++k)
                    if (k != lk) others[c++] = oc.col[k];
                const SliderCols c = slider_fixed_cols(others, g - 1, dim);
                const long elems = rows * (g - 1);
                hipLaunchKernelGGL(k_gather_columns, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, frows, rows, d - 1, c, cols);
                HIP_TRY(hipGetLastError());
                double *pts = cols + own_cols;
                const long total = rows * n * g;
                hipLaunchKernelGGL(k_calc_expand, dim3((unsigned)std::min<long>((total + 255) / 256, 8192)), dim3(256), 0, st,
                                   (const double *)cols, rows, g, lk, n, a.nodes, pts);
                HIP_TRY(hipGetLastError());
                if ((rc = bary_launch(po, &dt, 1, dt->slot, pts, rows * n, vals, 1, 0, st, &h->s_partial))) return rc;
                plain = nullptr;
            }
            const long total = rows * n;
            hipLaunchKernelGGL(k_slider_fibre_sum, dim3((unsigned)std::min<long>((total + 255) / 256, 8192)), dim3(256), 0, st, vals,
                               plain, (const double *)svals, rows, n, ns, o, h->pivot);
            HIP_TRY(hipGetLastError());
        }
        CalcArgs c = a;
        c.vals = vals;
        c.counts = out.counts.as<int32_t>() + r0;
        if (mode == 0) c.roots = out.roots.as<double>() + (size_t)r0 * a.W;
        else { c.val = out.val.as<double>() + r0; c.loc = out.loc.as<double>() + r0; }
        if ((rc = calc_launch(c, rows, st))) return rc;
    }
    return out.download(mode, N, a.W, roots_out, counts_out, val_out, loc_out, st);
    PCX_API_END
}

extern "C" int pcx_spline_calculus_batch(pcx_spline *h, int dim, const double *lo, const double *hi, const double *fixed,
                                         int64_t N, int mode, double *roots_out, int32_t *counts_out, double *val_out,
                                         double *loc_out) {
    PCX_API_BEGIN
    if (!h || !lo || !hi) return fail(PCX_ERR_INVALID, "NULL argument");
    const int d = h->sd.d;
    if (dim < 0 || dim >= d) return fail(PCX_ERR_INVALID, "dim %d out of range [0, %d]", dim, d - 1);
    // the pieces along dim: index j there, 0 in every other dimension (C order over the per-dimension intervals)
    const int P = h->sd.shape[dim];
    long stride = 1;
    for (int k = dim + 1; k < d; ++k) stride *= h->sd.shape[k];
    std::vector<SplineCalcPiece> tab(P);
    long F = 0, Wtot = 0;
    int nmax = 1;
    for (int j = 0; j < P; ++j) {
        const pcx_bary *pc = h->pieces[(size_t)j * stride];
        SplineCalcPiece &e = tab[j];
        e.n = pc->dims.n[dim];
        e.W = std::max(e.n - 1, 1);
        e.lo = j == 0 ? lo[dim] : h->knots[h->sd.koff[dim] + j - 1];
        e.hi = j == P - 1 ? hi[dim] : h->knots[h->sd.koff[dim] + j];
        e.nodes = pc->d_nodes + pc->dims.off[dim];
        e.wts = pc->d_wts + pc->dims.off[dim];
        e.diff = pc->d_diff + pc->doff[dim];
        e.voff = F;
        e.roff = Wtot;
        int rc = calc_check(e.n, mode, N, e.lo, e.hi, pc->d_diff, roots_out, counts_out, val_out, loc_out);
        if (rc) return rc;
        F += e.n;
        Wtot += e.W;
        nmax = std::max(nmax, e.n);
    }
    for (int i = 0; i < h->n_pieces; ++i)                      // one grid per index along dim (auto-N pieces may differ)
        if (h->pieces[i]->dims.n[dim] != tab[(i / stride) % P].n)
            return fail(PCX_ERR_INVALID, "piece %d has %d nodes along dim %d, the pieces of its interval %d", i,
                        h->pieces[i]->dims.n[dim], dim, tab[(i / stride) % P].n);
    int rc = calc_check_fixed(fixed, N, d, dim, lo, hi);
    if (rc) return rc;
    if (N == 0) return PCX_OK;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    hipStream_t st = h->stream;
    const long chunk = std::max<long>(1, std::min<long>(N, kCalcChunkPoints / F));
    // the expand kernel carries the piece index in grid.y, and one pass goes through spline_eval_chunk as one chunk
    if (P > 65535) return fail(PCX_ERR_UNSUPPORTED, "%d pieces along dim %d: at most 65535", P, dim);
    if (chunk * F > kChunkPoints) return fail(PCX_ERR_UNSUPPORTED, "%ld fibre points per row: at most %lld", F, (long long)kChunkPoints);
    DevBuf d_tab, d_fixed, d_pts, d_vals, p_roots, p_counts, p_val, p_loc;
    CalcDevOut out;
    rc = d_tab.alloc((size_t)P * sizeof(SplineCalcPiece));
    if (!rc) rc = d_fixed.alloc((size_t)N * (d - 1) * sizeof(double));
    if (!rc) rc = d_pts.alloc((size_t)chunk * F * d * sizeof(double));
    if (!rc) rc = d_vals.alloc((size_t)chunk * F * sizeof(double));
    if (!rc) rc = p_roots.alloc(mode == 0 ? (size_t)chunk * Wtot * sizeof(double) : 0);
    if (!rc) rc = p_counts.alloc((size_t)chunk * P * sizeof(int32_t));
    if (!rc) rc = p_val.alloc(mode != 0 ? (size_t)chunk * P * sizeof(double) : 0);
    if (!rc) rc = p_loc.alloc(mode != 0 ? (size_t)chunk * P * sizeof(double) : 0);
    if (!rc) rc = out.alloc(mode, N, (int)Wtot);
    if (rc) return rc;
    // the table once per call, with a blocking copy: `tab` (pageable) has left the host when it returns
    HIP_TRY(hipMemcpy(d_tab.p, tab.data(), (size_t)P * sizeof(SplineCalcPiece), hipMemcpyHostToDevice));
    if (d > 1) HIP_TRY(hipMemcpyAsync(d_fixed.p, fixed, (size_t)N * (d - 1) * sizeof(double), hipMemcpyHostToDevice, st));
    const SplineCalcPiece *dt = d_tab.as<SplineCalcPiece>();
    SplineCalcOut po;
    po.vals = d_vals.as<double>();
    po.roots = p_roots.as<double>();
    po.counts = p_counts.as<int32_t>();
    po.val = p_val.as<double>();
    po.loc = p_loc.as<double>();
    const int m = nmax - 1;                                    // the LDS class, as calc_launch chooses it
    auto finish = [&](int code) {                              // the device buffers are freed on return
        (void)hipStreamSynchronize(st);
        return code;
    };
    for (long r0 = 0; r0 < N; r0 += chunk) {
        const long rows = std::min<long>(chunk, N - r0);
        const unsigned bx = (unsigned)std::min<long>((rows * nmax * d + 255) / 256, 4096);
        hipLaunchKernelGGL(k_spline_calc_expand, dim3(bx, (unsigned)P), dim3(256), 0, st,
                           d_fixed.as<double>() + (size_t)r0 * (d - 1), rows, d, dim, dt, d_pts.as<double>());
        if (hipGetLastError() != hipSuccess) return finish(fail(PCX_ERR_HIP, "k_spline_calc_expand launch failed"));
        if ((rc = spline_eval_chunk(h, d_pts.as<double>(), rows * F, nullptr, 1, d_vals.as<double>()))) return finish(rc);
        const unsigned fibres = (unsigned)(rows * P);
        if (m <= 16) hipLaunchKernelGGL(k_cheb1d_calculus_pieces<16>, dim3(fibres), dim3(64), 0, st, dt, rows, mode, po);
        else if (m <= 32) hipLaunchKernelGGL(k_cheb1d_calculus_pieces<32>, dim3(fibres), dim3(64), 0, st, dt, rows, mode, po);
        else hipLaunchKernelGGL(k_cheb1d_calculus_pieces<64>, dim3(fibres), dim3(64), 0, st, dt, rows, mode, po);
        if (hipGetLastError() != hipSuccess) return finish(fail(PCX_ERR_HIP, "k_cheb1d_calculus_pieces launch failed"));
        hipLaunchKernelGGL(k_spline_calc_merge, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, dt, P, rows, mode,
                           (int)Wtot, lo[dim], hi[dim], po, mode == 0 ? out.roots.as<double>() + (size_t)r0 * Wtot : nullptr,
                           out.counts.as<int32_t>() + r0, mode != 0 ? out.val.as<double>() + r0 : nullptr,
                           mode != 0 ? out.loc.as<double>() + r0 : nullptr);
        if (hipGetLastError() != hipSuccess) return finish(fail(PCX_ERR_HIP, "k_spline_calc_merge launch failed"));
    }
    return finish(out.download(mode, N, (int)Wtot, roots_out, counts_out, val_out, loc_out, st));
    PCX_API_END
}
