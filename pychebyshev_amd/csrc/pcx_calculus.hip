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
//
// The pcx_*_solve_batch entries run the same pipelines with a target per row (SolveReq): method 0 subtracts the row's
// level from its fibre in HBM (k_calc_level, between the evaluation and the same solver launch: all roots at the level),
// method 1 replaces the eigenvalue solver by the lane-per-fibre bracketed inversion of invert_kernels.h.  The
// pcx_*_calculus_batch entries pass no request and launch exactly what they launched before.

#include "pcx_slider_internal.h"
#include "pcx_spline_internal.h"
#include "calculus_kernels.h"
#include "slider_calc_kernels.h"
#include "spline_calc_kernels.h"
#include "invert_kernels.h"

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

// What a pcx_*_solve_batch entry asks for on top of the shared pipeline; the calculus entries pass none.
struct SolveReq {
    const double *targets;    // N levels (method 0) or targets (method 1), host
    int method;               // 0 all roots at the level (outputs as mode 0), 1 bracketed inversion
    double *x_out;            // N (method 1)
    int32_t *status_out;      // N (method 1)
};

static int solve_check(int n, const SolveReq &sq, int64_t N, double lo, double hi, double *roots_out, int32_t *counts_out) {
    if (n < 1 || n > PCX_INV_MAX_N)
        return fail(PCX_ERR_INVALID, "n=%d outside [1, %d]: the device solvers take fibres of at most %d nodes", n,
                    PCX_INV_MAX_N, PCX_INV_MAX_N);
    if (sq.method < 0 || sq.method > 1) return fail(PCX_ERR_INVALID, "method=%d (0 roots at a level, 1 inversion)", sq.method);
    if (N < 0) return fail(PCX_ERR_INVALID, "N=%lld < 0", (long long)N);
    if (!(lo < hi)) return fail(PCX_ERR_INVALID, "domain: lo must be < hi");
    if (N > 0 && !sq.targets) return fail(PCX_ERR_INVALID, "targets is NULL");
    if (sq.method == 0 && !counts_out) return fail(PCX_ERR_INVALID, "counts_out is NULL");
    if (sq.method == 0 && !roots_out) return fail(PCX_ERR_INVALID, "roots_out is NULL");
    if (sq.method == 1 && (!sq.x_out || !sq.status_out)) return fail(PCX_ERR_INVALID, "x_out / status_out is NULL");
    return PCX_OK;
}

// the argument check of an entry: calc_check without a request, solve_check with one
static int calc_check_req(int n, int mode, int64_t N, double lo, double hi, const double *diff, double *roots_out,
                          int32_t *counts_out, double *val_out, double *loc_out, const SolveReq *sq) {
    if (sq) return solve_check(n, *sq, N, lo, hi, roots_out, counts_out);
    return calc_check(n, mode, N, lo, hi, diff, roots_out, counts_out, val_out, loc_out);
}

// device side of a request: the targets of all N rows, and the outputs of method 1
struct SolveDev {
    DevBuf targets, x, status;
    bool invert = false;
    int alloc(const SolveReq *sq, long N) {
        if (!sq) return PCX_OK;
        invert = sq->method == 1;
        int rc = targets.alloc((size_t)N * sizeof(double));
        if (!rc && invert) rc = x.alloc((size_t)N * sizeof(double));
        if (!rc && invert) rc = status.alloc((size_t)N * sizeof(int32_t));
        return rc;
    }
    int upload(const SolveReq *sq, long N, hipStream_t st) {
        if (sq) HIP_TRY(hipMemcpyAsync(targets.p, sq->targets, (size_t)N * sizeof(double), hipMemcpyHostToDevice, st));
        return PCX_OK;
    }
    int download(const SolveReq *sq, long N, hipStream_t st) {
        HIP_TRY(hipMemcpyAsync(sq->x_out, x.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(sq->status_out, status.p, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return PCX_OK;
    }
};

// launch KERNEL<NP> with NP the fibre-length class of the inversion's LDS tile
#define INV_DISPATCH(n, KERNEL, grid, st, ...)                                                   \
    do {                                                                                         \
        if ((n) <= 16) hipLaunchKernelGGL(KERNEL<16>, grid, dim3(64), 0, st, __VA_ARGS__);        \
        else if ((n) <= 32) hipLaunchKernelGGL(KERNEL<32>, grid, dim3(64), 0, st, __VA_ARGS__);   \
        else hipLaunchKernelGGL(KERNEL<64>, grid, dim3(64), 0, st, __VA_ARGS__);                  \
    } while (0)

// k_cheb1d_invert over a.rows fibres (pointers already offset to the first row): one lane per fibre, 64 per workgroup
static int inv_launch(const InvArgs &a, hipStream_t st) {
    if (a.rows <= 0) return PCX_OK;
    const long blocks = (a.rows + 63) / 64;
    if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "too many rows for one launch");
    INV_DISPATCH(a.n, k_cheb1d_invert, dim3((unsigned)blocks), st, a);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

// One pass of `rows` fibres of a request (vals and the outputs of `c` already offset to the pass, r0 its first row):
// the inversion, or the level subtracted in place and the root solver
static int solve_pass(const CalcArgs &c, double *vals, long rows, long r0, SolveDev &sd, hipStream_t st) {
    const double *t = sd.targets.as<double>() + r0;
    if (sd.invert) {
        InvArgs ia{};
        ia.n = c.n; ia.rows = rows; ia.lo = c.lo; ia.hi = c.hi; ia.nodes = c.nodes; ia.wts = c.wts;
        ia.vals = vals; ia.targets = t;
        ia.x = sd.x.as<double>() + r0;
        ia.status = sd.status.as<int32_t>() + r0;
        ia.iters = nullptr;
        return inv_launch(ia, st);
    }
    const long total = rows * c.n;
    hipLaunchKernelGGL(k_calc_level, dim3((unsigned)std::min<long>((total + 255) / 256, 8192)), dim3(256), 0, st, vals, t, rows,
                       c.n);
    HIP_TRY(hipGetLastError());
    return calc_launch(c, rows, st);
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
                       double *roots_out, int32_t *counts_out, double *val_out, double *loc_out,
                       const SolveReq *sq = nullptr) {
    const int n = a.n;
    const long chunk = std::max<long>(1, std::min<long>(N, kCalcChunkPoints / n));
    DevBuf d_fixed, d_pts, d_vals;
    CalcDevOut out;
    SolveDev sd;
    int rc = d_fixed.alloc((size_t)N * (d - 1) * sizeof(double));
    if (!rc) rc = d_pts.alloc((size_t)chunk * n * d * sizeof(double));
    if (!rc) rc = d_vals.alloc((size_t)chunk * n * sizeof(double));
    if (!rc) rc = sd.alloc(sq, N);
    if (!rc && !sd.invert) rc = out.alloc(mode, N, a.W);
    if (rc) return rc;
    if (d > 1) HIP_TRY(hipMemcpyAsync(d_fixed.p, fixed, (size_t)N * (d - 1) * sizeof(double), hipMemcpyHostToDevice, st));
    if ((rc = sd.upload(sq, N, st))) return rc;
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
        if (!sd.invert) {                                      // the inversion has its own outputs (SolveDev)
            c.counts = out.counts.as<int32_t>() + r0;
            if (mode == 0) c.roots = out.roots.as<double>() + (size_t)r0 * a.W;
            else { c.val = out.val.as<double>() + r0; c.loc = out.loc.as<double>() + r0; }
        }
        if ((rc = sq ? solve_pass(c, d_vals.as<double>(), rows, r0, sd, st) : calc_launch(c, rows, st))) return rc;
    }
    if (sd.invert) return sd.download(sq, N, st);
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

// pcx_cheb1d_calculus with a target per row: method 0 solves values - targets[:, None] for all its roots, method 1 inverts
extern "C" int pcx_cheb1d_solve(int device, int n, double lo, double hi, const double *nodes, const double *weights,
                                const double *values, const double *targets, int64_t N, int method, double *roots_out,
                                int32_t *counts_out, double *x_out, int32_t *status_out) {
    PCX_API_BEGIN
    const SolveReq sq{targets, method, x_out, status_out};
    int rc = solve_check(n, sq, N, lo, hi, roots_out, counts_out);
    if (rc) return rc;
    if (!nodes || !weights || (N > 0 && !values)) return fail(PCX_ERR_INVALID, "NULL argument");
    if (N == 0) return PCX_OK;
    if ((rc = use_device(device))) return rc;
    const int W = std::max(n - 1, 1);
    DevBuf d_grid, d_vals;                                     // nodes, weights in one buffer
    CalcDevOut out;
    SolveDev sd;
    rc = d_grid.alloc((size_t)2 * n * sizeof(double));
    if (!rc) rc = d_vals.alloc((size_t)N * n * sizeof(double));
    if (!rc) rc = sd.alloc(&sq, N);
    if (!rc && !sd.invert) rc = out.alloc(0, N, W);
    if (rc) return rc;
    double *g = d_grid.as<double>();
    HIP_TRY(hipMemcpy(g, nodes, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g + n, weights, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_vals.p, values, (size_t)N * n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(sd.targets.p, targets, (size_t)N * sizeof(double), hipMemcpyHostToDevice));
    CalcArgs a{};
    a.n = n; a.mode = 0; a.W = W; a.lo = lo; a.hi = hi;
    a.nodes = g; a.wts = g + n; a.diff = nullptr; a.vals = d_vals.as<double>();
    a.counts = out.counts.as<int32_t>();
    a.roots = out.roots.as<double>();
    if ((rc = solve_pass(a, d_vals.as<double>(), (long)N, 0, sd, nullptr))) return rc;
    if (sd.invert) return sd.download(&sq, (long)N, nullptr);
    return out.download(0, (long)N, W, roots_out, counts_out, nullptr, nullptr, nullptr);
    PCX_API_END
}

static int bary_calc_impl(pcx_bary *h, int dim, const double *lo, const double *hi, const double *fixed, int64_t N, int mode,
                          double *roots_out, int32_t *counts_out, double *val_out, double *loc_out, const SolveReq *sq) {
    if (!h || !lo || !hi) return fail(PCX_ERR_INVALID, "NULL argument");
    const int d = h->dims.d;
    if (dim < 0 || dim >= d) return fail(PCX_ERR_INVALID, "dim %d out of range [0, %d]", dim, d - 1);
    const int n = h->dims.n[dim];
    int rc = calc_check_req(n, mode, N, lo[dim], hi[dim], h->d_diff, roots_out, counts_out, val_out, loc_out, sq);
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
    return calc_fibres(d, dim, mode, fixed, N, a, h->stream, eval, roots_out, counts_out, val_out, loc_out, sq);
}

extern "C" int pcx_bary_calculus_batch(pcx_bary *h, int dim, const double *lo, const double *hi, const double *fixed,
                                       int64_t N, int mode, double *roots_out, int32_t *counts_out, double *val_out,
                                       double *loc_out) {
    PCX_API_BEGIN
    return bary_calc_impl(h, dim, lo, hi, fixed, N, mode, roots_out, counts_out, val_out, loc_out, nullptr);
    PCX_API_END
}

extern "C" int pcx_bary_solve_batch(pcx_bary *h, int dim, const double *lo, const double *hi, const double *fixed,
                                    const double *targets, int64_t N, int method, double *roots_out, int32_t *counts_out,
                                    double *x_out, int32_t *status_out) {
    PCX_API_BEGIN
    const SolveReq sq{targets, method, x_out, status_out};
    return bary_calc_impl(h, dim, lo, hi, fixed, N, 0, roots_out, counts_out, nullptr, nullptr, &sq);
    PCX_API_END
}

static int tt_calc_impl(pcx_tt *h, int dim, const double *fixed, int64_t N, int mode, double *roots_out, int32_t *counts_out,
                        double *val_out, double *loc_out, const SolveReq *sq) {
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
    rc = calc_check_req(n, mode, N, lo[dim], hi[dim], D, roots_out, counts_out, val_out, loc_out, sq);
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
    rc = calc_fibres(d, dim, mode, fixed, N, a, st, eval, roots_out, counts_out, val_out, loc_out, sq);
    (void)hipStreamSynchronize(st);                            // d_grid is freed on return
    return rc;
}

extern "C" int pcx_tt_calculus_batch(pcx_tt *h, int dim, const double *fixed, int64_t N, int mode, double *roots_out,
                                     int32_t *counts_out, double *val_out, double *loc_out) {
    PCX_API_BEGIN
    return tt_calc_impl(h, dim, fixed, N, mode, roots_out, counts_out, val_out, loc_out, nullptr);
    PCX_API_END
}

extern "C" int pcx_tt_solve_batch(pcx_tt *h, int dim, const double *fixed, const double *targets, int64_t N, int method,
                                  double *roots_out, int32_t *counts_out, double *x_out, int32_t *status_out) {
    PCX_API_BEGIN
    const SolveReq sq{targets, method, x_out, status_out};
    return tt_calc_impl(h, dim, fixed, N, 0, roots_out, counts_out, nullptr, nullptr, &sq);
    PCX_API_END
}

static int slider_calc_impl(pcx_slider *h, int dim, const double *lo, const double *hi, const double *fixed, int64_t N,
                            int mode, double *roots_out, int32_t *counts_out, double *val_out, double *loc_out,
                            const SolveReq *sq) {
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
    int rc = calc_check_req(n, mode, N, lo[dim], hi[dim], po->d_diff, roots_out, counts_out, val_out, loc_out, sq);
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
    SolveDev sd;
    rc = h->s_cols.reserve(cols_doubles * sizeof(double));
    if (!rc) rc = h->s_vals.reserve((size_t)chunk * ns * sizeof(double));
    if (!rc) rc = d_fixed.alloc((size_t)N * (d - 1) * sizeof(double));
    if (!rc) rc = d_vals.alloc((size_t)chunk * n * sizeof(double));
    if (!rc) rc = sd.alloc(sq, N);
    if (!rc && !sd.invert) rc = out.alloc(mode, N, a.W);
    if (rc) return rc;
    if (d > 1) HIP_TRY(hipMemcpyAsync(d_fixed.p, fixed, (size_t)N * (d - 1) * sizeof(double), hipMemcpyHostToDevice, st));
    if ((rc = sd.upload(sq, N, st))) return rc;
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
        if (!sd.invert) {                                      // the inversion has its own outputs (SolveDev)
            c.counts = out.counts.as<int32_t>() + r0;
            if (mode == 0) c.roots = out.roots.as<double>() + (size_t)r0 * a.W;
            else { c.val = out.val.as<double>() + r0; c.loc = out.loc.as<double>() + r0; }
        }
        if ((rc = sq ? solve_pass(c, vals, rows, r0, sd, st) : calc_launch(c, rows, st))) return rc;
    }
    if (sd.invert) return sd.download(sq, N, st);
    return out.download(mode, N, a.W, roots_out, counts_out, val_out, loc_out, st);
}

extern "C" int pcx_slider_calculus_batch(pcx_slider *h, int dim, const double *lo, const double *hi, const double *fixed,
                                         int64_t N, int mode, double *roots_out, int32_t *counts_out, double *val_out,
                                         double *loc_out) {
    PCX_API_BEGIN
    return slider_calc_impl(h, dim, lo, hi, fixed, N, mode, roots_out, counts_out, val_out, loc_out, nullptr);
    PCX_API_END
}

extern "C" int pcx_slider_solve_batch(pcx_slider *h, int dim, const double *lo, const double *hi, const double *fixed,
                                      const double *targets, int64_t N, int method, double *roots_out, int32_t *counts_out,
                                      double *x_out, int32_t *status_out) {
    PCX_API_BEGIN
    const SolveReq sq{targets, method, x_out, status_out};
    return slider_calc_impl(h, dim, lo, hi, fixed, N, 0, roots_out, counts_out, nullptr, nullptr, &sq);
    PCX_API_END
}

static int spline_calc_impl(pcx_spline *h, int dim, const double *lo, const double *hi, const double *fixed, int64_t N,
                            int mode, double *roots_out, int32_t *counts_out, double *val_out, double *loc_out,
                            const SolveReq *sq) {
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
        int rc = calc_check_req(e.n, mode, N, e.lo, e.hi, pc->d_diff, roots_out, counts_out, val_out, loc_out, sq);
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
    SolveDev sd;
    const bool invert = sq && sq->method == 1;                 // p_val / p_counts then hold the pieces' x / status
    rc = d_tab.alloc((size_t)P * sizeof(SplineCalcPiece));
    if (!rc) rc = sd.alloc(sq, N);
    if (!rc) rc = d_fixed.alloc((size_t)N * (d - 1) * sizeof(double));
    if (!rc) rc = d_pts.alloc((size_t)chunk * F * d * sizeof(double));
    if (!rc) rc = d_vals.alloc((size_t)chunk * F * sizeof(double));
    if (!rc) rc = p_roots.alloc(mode == 0 && !invert ? (size_t)chunk * Wtot * sizeof(double) : 0);
    if (!rc) rc = p_counts.alloc((size_t)chunk * P * sizeof(int32_t));
    if (!rc) rc = p_val.alloc(mode != 0 || invert ? (size_t)chunk * P * sizeof(double) : 0);
    if (!rc) rc = p_loc.alloc(mode != 0 ? (size_t)chunk * P * sizeof(double) : 0);
    if (!rc && !invert) rc = out.alloc(mode, N, (int)Wtot);
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
    if ((rc = sd.upload(sq, N, st))) return finish(rc);
    for (long r0 = 0; r0 < N; r0 += chunk) {
        const long rows = std::min<long>(chunk, N - r0);
        const unsigned bx = (unsigned)std::min<long>((rows * nmax * d + 255) / 256, 4096);
        hipLaunchKernelGGL(k_spline_calc_expand, dim3(bx, (unsigned)P), dim3(256), 0, st,
                           d_fixed.as<double>() + (size_t)r0 * (d - 1), rows, d, dim, dt, d_pts.as<double>());
        if (hipGetLastError() != hipSuccess) return finish(fail(PCX_ERR_HIP, "k_spline_calc_expand launch failed"));
        if ((rc = spline_eval_chunk(h, d_pts.as<double>(), rows * F, nullptr, 1, d_vals.as<double>()))) return finish(rc);
        if (invert) {                                          // a lane per (row, piece) fibre, then the lowest piece
            const dim3 grid((unsigned)((rows + 63) / 64), (unsigned)P);
            INV_DISPATCH(nmax, k_cheb1d_invert_pieces, grid, st, dt, rows, (const double *)d_vals.as<double>(),
                         (const double *)sd.targets.as<double>() + r0, p_val.as<double>(), p_counts.as<int32_t>());
            if (hipGetLastError() != hipSuccess) return finish(fail(PCX_ERR_HIP, "k_cheb1d_invert_pieces launch failed"));
            hipLaunchKernelGGL(k_spline_invert_merge, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, P, rows,
                               (const double *)p_val.as<double>(), (const int32_t *)p_counts.as<int32_t>(),
                               sd.x.as<double>() + r0, sd.status.as<int32_t>() + r0);
            if (hipGetLastError() != hipSuccess) return finish(fail(PCX_ERR_HIP, "k_spline_invert_merge launch failed"));
            continue;
        }
        if (sq) {                                              // roots at a level: every (row, piece) fibre minus its row's
            const unsigned lx = (unsigned)std::min<long>((rows * nmax + 255) / 256, 4096);
            hipLaunchKernelGGL(k_spline_calc_level, dim3(lx, (unsigned)P), dim3(256), 0, st, dt, d_vals.as<double>(),
                               (const double *)sd.targets.as<double>() + r0, rows);
            if (hipGetLastError() != hipSuccess) return finish(fail(PCX_ERR_HIP, "k_spline_calc_level launch failed"));
        }
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
    if (invert) return finish(sd.download(sq, N, st));
    return finish(out.download(mode, N, (int)Wtot, roots_out, counts_out, val_out, loc_out, st));
}

extern "C" int pcx_spline_calculus_batch(pcx_spline *h, int dim, const double *lo, const double *hi, const double *fixed,
                                         int64_t N, int mode, double *roots_out, int32_t *counts_out, double *val_out,
                                         double *loc_out) {
    PCX_API_BEGIN
    return spline_calc_impl(h, dim, lo, hi, fixed, N, mode, roots_out, counts_out, val_out, loc_out, nullptr);
    PCX_API_END
}

extern "C" int pcx_spline_solve_batch(pcx_spline *h, int dim, const double *lo, const double *hi, const double *fixed,
                                      const double *targets, int64_t N, int method, double *roots_out, int32_t *counts_out,
                                      double *x_out, int32_t *status_out) {
    PCX_API_BEGIN
    const SolveReq sq{targets, method, x_out, status_out};
    return spline_calc_impl(h, dim, lo, hi, fixed, N, 0, roots_out, counts_out, nullptr, nullptr, &sq);
    PCX_API_END
}
