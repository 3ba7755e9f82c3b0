// pcx_piecewise_grid.hip -- tensor-product grid evaluation of piecewise interpolants and sliders
// (pcx_spline_eval_tensor_grid[_dev], pcx_slider_eval_tensor_grid[_dev]).  gfx950 only.
//
// Both are built out of the barycentric handle's own grid evaluation (pcx_bary_eval_tensor_grid_dev: d FP64 mode
// products, pcx_mode_product.hip) and one bandwidth-bound kernel that writes the result (piecewise_grid_kernels.h):
//   spline   the grid falls apart into one sub-grid per piece (spline_grid_plan.h); every live piece evaluates its own
//            into its block of a packed staging buffer, k_spline_grid_place copies every element to its place;
//   slider   every slide evaluates the grid of its own group of dimensions, k_slider_grid_sum forms
//            pivot + sum_s (G_s - pivot) over the whole grid, G_s broadcast over the dimensions slide s does not own.
// The handle's own reservations all precede its first launch of a call (Scratch::reserve frees); a call waits for the
// grid_done event of the call before it reuses them.  Lock order: the handle's mu, then a piece's or slide's mu (taken
// inside pcx_bary_eval_tensor_grid_dev), as in spline_eval_chunk.

#include <cstdlib>

#include "pcx_slider_internal.h"
#include "pcx_spline_internal.h"
#include "spline_grid_plan.h"
#include "piecewise_grid_kernels.h"

static const long kPgMaxCount = 1L << 40;        // grid points
static const long kPgMaxBlocks = 1L << 16;       // grid-stride kernels: 256 workgroups per CU and more buy nothing

// PCX_PIECEWISE_GRID_LOG=1: the assembly kernel of a call is timed on its own (two events and a wait) and reported on
// stderr with the bytes it wrote, as PCX_GRID_LOG does for the passes of pcx_mode_product.hip (which it leaves alone: a
// spline of 64 pieces has 192 of them) -- tools/piecewise_grid_probe.py.  Slows the call down.
struct AssemblyLog {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool on = false;
    AssemblyLog() { on = getenv("PCX_PIECEWISE_GRID_LOG") != nullptr && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess; }
    ~AssemblyLog() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    void begin(hipStream_t st) { if (on) (void)hipEventRecord(e0, st); }
    void end(hipStream_t st, const char *kernel, long total, long parts, double read_bytes) {
        if (!on) return;
        float ms = 0.f;
        if (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return;
        fprintf(stderr, "[pcx] %s: %ld points from %ld parts: %.1f us, writes %.2f MB at %.0f GB/s, reads %.2f MB\n", kernel, total, parts,
                ms * 1e3, 8.0 * total / 1e6, ms > 0.f ? 8.0 * total / (ms * 1e6) : 0.0, read_bytes / 1e6);
    }
};

static unsigned pg_blocks(long total) {
    return (unsigned)std::min(kPgMaxBlocks, (total + PCX_PG_THREADS - 1) / PCX_PG_THREADS);
}

// The `_run` forms (piecewise_grid_kernels.h) walk the grid with eight workgroups per CU, so that a lane's one decode is
// spread over total / (2048 * 256) elements.  PCX_PIECEWISE_GRID_DECODE=1 forces the plain forms, which divide per
// element (A/B runs: tools/piecewise_grid_probe.py; the tests run both); PCX_PIECEWISE_GRID_BLOCKS=<n> walks with n
// workgroups instead of 2048 (1 .. 65536: with one, the lanes of a 20,000-point test grid walk 78 elements each).  Both
// read per call.
static const long kPgRunBlocks = 2048;
static unsigned pg_run_blocks(long total) {
    const char *v = getenv("PCX_PIECEWISE_GRID_BLOCKS");
    const long want = v ? atol(v) : 0;
    return (unsigned)std::min(want >= 1 && want <= kPgMaxBlocks ? want : kPgRunBlocks, (total + PCX_PG_THREADS - 1) / PCX_PG_THREADS);
}
static bool pg_run_form(int live_dims) {
    const char *v = getenv("PCX_PIECEWISE_GRID_DECODE");
    return live_dims >= 1 && live_dims <= PCX_PG_RUN_DIMS && !(v && v[0] == '1');
}
// axis lengths m[0 .. D) and the digits of the launch's stride in their mixed radix
static GridWalk pg_walk(int D, const int *m, long total, unsigned blocks) {
    GridWalk gw;
    long stride = ((long)blocks * PCX_PG_THREADS) % total;
    for (int k = 0; k < PCX_PG_RUN_DIMS; ++k) { gw.m[k] = 1; gw.step[k] = 0; }
    for (int k = D - 1; k >= 0; --k) {
        gw.m[k] = m[k];
        gw.step[k] = (int)(stride % m[k]);
        stride /= m[k];
    }
    return gw;
}
// the instantiation of a `_run` kernel for D dimensions and the index type of `total`
#define PG_RUN_CASE(KERNEL, Dv, ...)                                                                                      \
    case Dv:                                                                                                              \
        if (total < (1L << 32)) hipLaunchKernelGGL((KERNEL<Dv, unsigned>), dim3(blocks), dim3(PCX_PG_THREADS), 0, st, __VA_ARGS__); \
        else hipLaunchKernelGGL((KERNEL<Dv, unsigned long>), dim3(blocks), dim3(PCX_PG_THREADS), 0, st, __VA_ARGS__);    \
        break;
#define PG_RUN_SWITCH(KERNEL, D, ...)                                                                                     \
    switch (D) {                                                                                                          \
        PG_RUN_CASE(KERNEL, 1, __VA_ARGS__) PG_RUN_CASE(KERNEL, 2, __VA_ARGS__) PG_RUN_CASE(KERNEL, 3, __VA_ARGS__)      \
        PG_RUN_CASE(KERNEL, 4, __VA_ARGS__) PG_RUN_CASE(KERNEL, 5, __VA_ARGS__) PG_RUN_CASE(KERNEL, 6, __VA_ARGS__)      \
    }

// the axis lengths of a d-dimensional grid: PCX_ERR_INVALID for an empty axis, PCX_ERR_UNSUPPORTED above 2^40 points
static int pg_total(int d, const int32_t *m, long *total) {
    *total = 1;
    for (int k = 0; k < d; ++k) {
        if (m[k] < 1) return fail(PCX_ERR_INVALID, "m[%d]=%d: the axis of dimension %d is empty", k, m[k], k);
        if ((double)*total * m[k] > (double)kPgMaxCount) return fail(PCX_ERR_UNSUPPORTED, "grid of more than 2^40 points");
        *total *= m[k];
    }
    return PCX_OK;
}

static int pg_wait_done(hipEvent_t *done) {
    if (*done) HIP_TRY(hipEventSynchronize(*done));          // the buffers of an earlier call may still be read on another stream
    else HIP_TRY(hipEventCreateWithFlags(done, hipEventDisableTiming));
    return PCX_OK;
}

// ---------------------------------------------------------------------------------
// spline
// ---------------------------------------------------------------------------------
// The grid into d_out (device) on `st`; host_bytes > 0 also reserves the host form's staging of the result.  Caller
// holds h->mu.
static int spline_grid_run(pcx_spline *h, const int32_t *deriv, const int32_t *m, const double *axes_cat, double *d_out,
                           size_t host_bytes, hipStream_t st) {
    const int d = h->sd.d;
    SplineGridPlan sp;
    char err[PCX_ERR_LEN];
    int rc = spline_grid_make_plan(d, h->sd.nknots, h->knots.data(), m, axes_cat, kPgMaxCount, sp, err, sizeof err);
    if (rc) return fail(rc, "%s", err);
    if ((rc = pg_wait_done(&h->grid_done))) return rc;
    if (host_bytes) {
        if ((rc = h->s_gridout.reserve(host_bytes))) return rc;
        d_out = (double *)h->s_gridout.ptr;
    }
    const long live = (long)sp.blocks.size();
    if (live == 1) {
        // every axis lies in one interval: the lists are the axes, the block is the result
        const SplineGridBlock &b = sp.blocks[0];
        if ((rc = pcx_bary_eval_tensor_grid_dev(h->pieces[b.piece], deriv, b.m, sp.sub_axes.data() + b.axes_off, d_out, st))) return rc;
        HIP_TRY(hipEventRecord(h->grid_done, st));
        return PCX_OK;
    }
    // tables: block_off per piece (8 bytes each), then interval, rank (per axis entry) and count (per interval) as int32
    const long sm = sp.axis_off[d], sc = sp.cnt_off[d];
    const size_t n_int = (size_t)(2 * sm + sc);
    h->grid_tab_host.assign((size_t)sp.n_pieces + (n_int + 1) / 2, 0);
    memcpy(h->grid_tab_host.data(), sp.block_off.data(), (size_t)sp.n_pieces * sizeof(long));
    int32_t *ti = (int32_t *)(h->grid_tab_host.data() + sp.n_pieces);
    memcpy(ti, sp.interval.data(), (size_t)sm * sizeof(int32_t));
    memcpy(ti + sm, sp.rank.data(), (size_t)sm * sizeof(int32_t));
    memcpy(ti + 2 * sm, sp.count.data(), (size_t)sc * sizeof(int32_t));
    if ((rc = h->s_gridtab.reserve(h->grid_tab_host.size() * sizeof(long)))) return rc;
    if ((rc = h->s_gridstage.reserve((size_t)sp.total * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpyAsync(h->s_gridtab.ptr, h->grid_tab_host.data(), h->grid_tab_host.size() * sizeof(long), hipMemcpyHostToDevice, st));
    double *stage = (double *)h->s_gridstage.ptr;
    // the pieces' grids are independent: with several of them they go round-robin over the side streams, which wait
    // for `st` (fork) and for which `st` waits (join); no host synchronization in between
    const bool fan = h->ev_fork && live > 2;
    if (fan) {
        HIP_TRY(hipEventRecord(h->ev_fork, st));
        for (int i = 0; i < pcx_spline::kSide; ++i) HIP_TRY(hipStreamWaitEvent(h->side[i], h->ev_fork, 0));
    }
    long turn = 0;
    for (const SplineGridBlock &b : sp.blocks) {
        hipStream_t ps = fan ? h->side[turn % pcx_spline::kSide] : st;
        ++turn;
        if ((rc = pcx_bary_eval_tensor_grid_dev(h->pieces[b.piece], deriv, b.m, sp.sub_axes.data() + b.axes_off, stage + b.offset, ps))) break;
    }
    if (fan)
        for (int i = 0; i < pcx_spline::kSide && i < turn; ++i) {
            HIP_TRY(hipEventRecord(h->ev_join[i], h->side[i]));
            HIP_TRY(hipStreamWaitEvent(st, h->ev_join[i], 0));
        }
    if (rc) return rc;
    SplineGridDims gd;
    gd.d = d;
    for (int k = 0; k < PCX_MAX_DIMS; ++k) {
        gd.m[k] = k < d ? m[k] : 1;
        gd.shape[k] = k < d ? h->sd.shape[k] : 1;
        gd.aoff[k] = k < d ? sp.axis_off[k] : 0;
        gd.coff[k] = k < d ? sp.cnt_off[k] : 0;
    }
    const long *d_boff = (const long *)h->s_gridtab.ptr;
    const int *d_iv = (const int *)(d_boff + sp.n_pieces), *d_rk = d_iv + sm, *d_cnt = d_rk + sm;
    AssemblyLog log;
    log.begin(st);
    const long total = sp.total;
    const bool run = pg_run_form(d);
    if (run) {
        const unsigned blocks = pg_run_blocks(total);
        const GridWalk gw = pg_walk(d, gd.m, total, blocks);
        PG_RUN_SWITCH(k_spline_grid_place_run, d, gd, gw, d_iv, d_rk, d_cnt, d_boff, (const double *)stage, d_out, total)
    } else if (total < (1L << 32))
        hipLaunchKernelGGL(k_spline_grid_place<unsigned>, dim3(pg_blocks(total)), dim3(PCX_PG_THREADS), 0, st, gd, d_iv, d_rk, d_cnt,
                           d_boff, (const double *)stage, d_out, total);
    else
        hipLaunchKernelGGL(k_spline_grid_place<unsigned long>, dim3(pg_blocks(total)), dim3(PCX_PG_THREADS), 0, st, gd, d_iv, d_rk,
                           d_cnt, d_boff, (const double *)stage, d_out, total);
    HIP_TRY(hipGetLastError());
    log.end(st, run ? "k_spline_grid_place_run" : "k_spline_grid_place", total, live, 8.0 * total);
    HIP_TRY(hipEventRecord(h->grid_done, st));
    return PCX_OK;
}

static int spline_grid_check(pcx_spline *h, const int32_t *m, const double *axes_cat, const void *out, long *total) {
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    if (!m || !axes_cat || !out) return fail(PCX_ERR_INVALID, "NULL argument");
    return pg_total(h->sd.d, m, total);
}

extern "C" int pcx_spline_eval_tensor_grid_dev(pcx_spline *h, const int32_t *deriv, const int32_t *m, const double *axes_cat,
                                               double *d_out, void *stream) {
    PCX_API_BEGIN
    long total = 0;
    int rc = spline_grid_check(h, m, axes_cat, d_out, &total);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    return spline_grid_run(h, deriv, m, axes_cat, d_out, 0, stream ? (hipStream_t)stream : h->stream);
    PCX_API_END
}

extern "C" int pcx_spline_eval_tensor_grid(pcx_spline *h, const int32_t *deriv, const int32_t *m, const double *axes_cat, double *out) {
    PCX_API_BEGIN
    long total = 0;
    int rc = spline_grid_check(h, m, axes_cat, out, &total);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    rc = spline_grid_run(h, deriv, m, axes_cat, nullptr, (size_t)total * sizeof(double), h->stream);
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
// slider
// ---------------------------------------------------------------------------------
// Caller holds h->mu.
static int slider_grid_run(pcx_slider *h, const int32_t *deriv, const int32_t *m, const double *axes_cat, long total, double *d_out,
                           size_t host_bytes, hipStream_t st) {
    const int d = h->d, ns_all = (int)h->slides.size();
    // the slides that own a differentiated dimension: more than one -> the mixed partial is identically zero
    int active = -1, n_active = 0;
    if (deriv) {
        std::vector<char> seen((size_t)ns_all, 0);
        for (int k = 0; k < d; ++k) {
            if (deriv[k] < 0) return fail(PCX_ERR_INVALID, "derivative order %d at dim %d", deriv[k], k);
            if (deriv[k] > 0 && !seen[h->owner[k]]) {
                seen[h->owner[k]] = 1;
                active = h->owner[k];
                ++n_active;
            }
        }
    }
    int rc = pg_wait_done(&h->grid_done);
    if (rc) return rc;
    if (host_bytes) {
        if ((rc = h->s_gridout.reserve(host_bytes))) return rc;
        d_out = (double *)h->s_gridout.ptr;
    }
    if (n_active > 1) {
        HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)total * sizeof(double), st));
        HIP_TRY(hipEventRecord(h->grid_done, st));
        return PCX_OK;
    }
    const int first = n_active == 1 ? active : 0, ns = n_active == 1 ? 1 : ns_all;
    std::vector<long> aoff((size_t)d + 1, 0), cstride((size_t)d, 1);
    for (int k = 0; k < d; ++k) aoff[k + 1] = aoff[k] + m[k];
    for (int k = d - 2; k >= 0; --k) cstride[k] = cstride[k + 1] * m[k + 1];
    // per slide: its axes (the group's own order), its grid's shape and offset in s_grid, and its terms of the table
    std::vector<double> sub_axes;
    std::vector<int32_t> sub_m((size_t)ns * PCX_MAX_DIMS, 1), sub_spec((size_t)ns * PCX_MAX_DIMS, 0);
    std::vector<long> sub_aoff((size_t)ns), term_begin((size_t)ns + 1, 0), g_off((size_t)ns, 0), terms;
    // the axes longer than 1, in the result's order: what the `_run` form walks; col_of[k] is dimension k's place among them
    std::vector<int> live_m, col_of((size_t)d, -1);
    for (int k = 0; k < d; ++k)
        if (m[k] > 1) { col_of[k] = (int)live_m.size(); live_m.push_back(m[k]); }
    const int D = (int)live_m.size();
    const bool run = pg_run_form(D);
    std::vector<long> dense(run ? (size_t)ns * D : 0, 0);        // stride[ns][D] of the `_run` form
    long g_total = 0;
    for (int i = 0; i < ns; ++i) {
        const SliderCols &c = h->cols[first + i];
        sub_aoff[i] = (long)sub_axes.size();
        g_off[i] = g_total;
        long cnt = 1;
        for (int j = 0; j < c.nc; ++j) {
            const int k = c.col[j];
            sub_m[(size_t)i * PCX_MAX_DIMS + j] = m[k];
            sub_spec[(size_t)i * PCX_MAX_DIMS + j] = deriv ? deriv[k] : 0;
            sub_axes.insert(sub_axes.end(), axes_cat + aoff[k], axes_cat + aoff[k + 1]);
            cnt *= m[k];
        }
        long gs = cnt;
        for (int j = 0; j < c.nc; ++j) {
            const int k = c.col[j];
            gs /= m[k];                               // the C-order stride of the group's j-th dimension in G_s
            if (m[k] > 1) {
                terms.push_back(cstride[k]);
                terms.push_back(m[k]);
                terms.push_back(gs);
                if (run) dense[(size_t)i * D + col_of[k]] = gs;
            }
        }
        term_begin[i + 1] = (long)terms.size() / 3;
        g_total += cnt;
    }
    std::vector<long> &tab = h->grid_tab_host;
    tab.clear();
    if (run) {
        tab.insert(tab.end(), g_off.begin(), g_off.end());
        tab.insert(tab.end(), dense.begin(), dense.end());
    } else {
        tab.insert(tab.end(), term_begin.begin(), term_begin.end());
        tab.insert(tab.end(), g_off.begin(), g_off.end());
        tab.insert(tab.end(), terms.begin(), terms.end());
    }
    if ((rc = h->s_gridtab.reserve(tab.size() * sizeof(long)))) return rc;
    if ((rc = h->s_grid.reserve((size_t)g_total * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpyAsync(h->s_gridtab.ptr, tab.data(), tab.size() * sizeof(long), hipMemcpyHostToDevice, st));
    double *G = (double *)h->s_grid.ptr;
    for (int i = 0; i < ns; ++i)
        if ((rc = pcx_bary_eval_tensor_grid_dev(h->slides[first + i], n_active == 1 ? &sub_spec[(size_t)i * PCX_MAX_DIMS] : nullptr,
                                                &sub_m[(size_t)i * PCX_MAX_DIMS], sub_axes.data() + sub_aoff[i], G + g_off[i], st)))
            return rc;
    AssemblyLog log;
    log.begin(st);
    const long *d_tab = (const long *)h->s_gridtab.ptr;
    const int plain = n_active == 1 ? 1 : 0;
    if (run) {
        const unsigned blocks = pg_run_blocks(total);
        const GridWalk gw = pg_walk(D, live_m.data(), total, blocks);
        PG_RUN_SWITCH(k_slider_grid_sum_run, D, gw, (const double *)G, d_tab, ns, h->pivot, plain, d_out, total)
    } else if (total < (1L << 32))
        hipLaunchKernelGGL(k_slider_grid_sum<unsigned>, dim3(pg_blocks(total)), dim3(PCX_PG_THREADS), 0, st, (const double *)G, d_tab, ns,
                           h->pivot, plain, d_out, total);
    else
        hipLaunchKernelGGL(k_slider_grid_sum<unsigned long>, dim3(pg_blocks(total)), dim3(PCX_PG_THREADS), 0, st, (const double *)G, d_tab,
                           ns, h->pivot, plain, d_out, total);
    HIP_TRY(hipGetLastError());
    log.end(st, run ? "k_slider_grid_sum_run" : "k_slider_grid_sum", total, ns, 8.0 * g_total);
    HIP_TRY(hipEventRecord(h->grid_done, st));
    return PCX_OK;
}

static int slider_grid_check(pcx_slider *h, const int32_t *m, const double *axes_cat, const void *out, long *total) {
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    if (!m || !axes_cat || !out) return fail(PCX_ERR_INVALID, "NULL argument");
    return pg_total(h->d, m, total);
}

extern "C" int pcx_slider_eval_tensor_grid_dev(pcx_slider *h, const int32_t *deriv, const int32_t *m, const double *axes_cat,
                                               double *d_out, void *stream) {
    PCX_API_BEGIN
    long total = 0;
    int rc = slider_grid_check(h, m, axes_cat, d_out, &total);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    return slider_grid_run(h, deriv, m, axes_cat, total, d_out, 0, stream ? (hipStream_t)stream : h->stream);
    PCX_API_END
}

extern "C" int pcx_slider_eval_tensor_grid(pcx_slider *h, const int32_t *deriv, const int32_t *m, const double *axes_cat, double *out) {
    PCX_API_BEGIN
    long total = 0;
    int rc = slider_grid_check(h, m, axes_cat, out, &total);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    rc = slider_grid_run(h, deriv, m, axes_cat, total, nullptr, (size_t)total * sizeof(double), h->stream);
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
