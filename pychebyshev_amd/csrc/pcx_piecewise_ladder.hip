// pcx_piecewise_ladder.hip -- C ABI of libpcx_hip.so (see include/pcx.h): ladders of the piecewise interpolant and of the
// slider along one dimension.  The fibre contraction is the borrowed pieces' / slides' own (bary_ladder_launch,
// pcx_bary_ladder.hip); this file is the structure around it (piecewise_ladder_kernels.h).  gfx950 only.

#include "pcx_slider_internal.h"
#include "pcx_spline_internal.h"
#include "piecewise_ladder_kernels.h"

// doubles of fibres (spline) or of result (slider) one chunk of rows holds: the calculus batches' kCalcChunkPoints
static const long kLadderChunkDoubles = 1L << 21;

static unsigned grid_for(long total) { return (unsigned)std::max<long>(1, std::min<long>((total + 255) / 256, 8192)); }

// ---------------------------------------------------------------------------------
// spline
// ---------------------------------------------------------------------------------
struct SplineLadderCall {
    int dim = 0, nq = 0, P = 0, n_sections = 0;
    long stride = 1;                     // flat-index stride of dim over the pieces
    const int32_t *deriv = nullptr;
    int m = 0;
    std::vector<SplineLadderPiece> tab;  // by index along dim
    std::vector<char> live;
    long Flive = 0;                      // fibre doubles per row: the live indices' node counts
    long chunk = 1;                      // rows per chunk
    DevView d_tab{}, d_packed{}, d_slot{}, d_F{};   // in the handle's s_ladder scratch: kept between calls
};

// the piece index along dim of one value, the kernels' rule (spline_dim_piece) on the host
static int spline_host_piece(const pcx_spline *h, int dim, double x) {
    const int nk = h->sd.nknots[dim];
    int idx = 0;
    if (x != x) idx = nk;
    else
        for (int j = 0; j < nk; ++j) idx += (h->knots[h->sd.koff[dim] + j] <= x) ? 1 : 0;
    return std::min(idx, h->sd.shape[dim] - 1);
}

// The per-index table, the live set (host_xs: `count` values on the host, NULL: every index is live) and the call's
// buffers for batches of up to max_rows rows.  Caller holds h->mu.
static int spline_ladder_prepare(pcx_spline *h, int dim, const int32_t *deriv, int m, const double *host_xs, size_t count,
                                 int64_t max_rows, SplineLadderCall &c) {
    const int d = h->sd.d;
    c.dim = dim; c.nq = d - 1; c.deriv = deriv; c.m = m;
    c.P = h->sd.shape[dim];
    c.stride = 1;
    for (int k = dim + 1; k < d; ++k) c.stride *= h->sd.shape[k];
    c.n_sections = h->n_pieces / c.P;
    if (c.P > 65535) return fail(PCX_ERR_UNSUPPORTED, "%d pieces along dim %d: at most 65535", c.P, dim);
    c.tab.assign(c.P, SplineLadderPiece{});
    for (int j = 0; j < c.P; ++j) {
        const pcx_bary *pc = h->pieces[(size_t)j * c.stride];
        c.tab[j].n = pc->dims.n[dim];
        c.tab[j].nodes = pc->d_nodes + pc->dims.off[dim];
        c.tab[j].wts = pc->d_wts + pc->dims.off[dim];
    }
    for (int i = 0; i < h->n_pieces; ++i)                      // one grid per index along dim (auto-N pieces may differ)
        if (h->pieces[i]->dims.n[dim] != c.tab[(i / c.stride) % c.P].n)
            return fail(PCX_ERR_INVALID, "piece %d has %d nodes along dim %d, the pieces of its interval %d", i,
                        h->pieces[i]->dims.n[dim], dim, c.tab[(i / c.stride) % c.P].n);
    c.live.assign(c.P, host_xs ? 0 : 1);
    if (host_xs)
        for (size_t i = 0; i < count; ++i) c.live[spline_host_piece(h, dim, host_xs[i])] = 1;
    c.Flive = 0;
    for (int j = 0; j < c.P; ++j)
        if (c.live[j]) { c.tab[j].foff = c.Flive; c.Flive += c.tab[j].n; }
    c.chunk = std::max<long>(1, std::min<long>((long)max_rows, kLadderChunkDoubles / std::max<long>(c.Flive, 1)));
    int rc = h->s_ladder[0].reserve((size_t)c.P * sizeof(SplineLadderPiece));
    if (!rc) rc = h->s_ladder[1].reserve(std::max<size_t>((size_t)c.chunk * c.nq, 1) * sizeof(double));
    if (!rc) rc = h->s_ladder[2].reserve((size_t)c.chunk * sizeof(int));
    if (!rc) rc = h->s_ladder[3].reserve((size_t)c.chunk * c.Flive * sizeof(double));
    if (!rc) rc = h->s_piece.reserve((size_t)c.chunk * sizeof(int));
    if (!rc) rc = h->s_perm.reserve((size_t)c.chunk * sizeof(int));
    if (rc) return rc;
    c.d_tab.p = h->s_ladder[0].ptr; c.d_packed.p = h->s_ladder[1].ptr; c.d_slot.p = h->s_ladder[2].ptr; c.d_F.p = h->s_ladder[3].ptr;
    // the table once per call, with a blocking copy: `tab` (pageable) has left the host when it returns
    HIP_TRY(hipMemcpy(c.d_tab.p, c.tab.data(), (size_t)c.P * sizeof(SplineLadderPiece), hipMemcpyHostToDevice));
    return PCX_OK;
}

// N device-resident rows (fixed: stride fstride, xs: stride xstride, both readable by every stream of the handle) into
// d_out (N x m), chunk by chunk; everything is queued on h->stream and its side streams, joined into h->stream.
// Caller holds h->mu.
static int spline_ladder_rows(pcx_spline *h, SplineLadderCall &c, const double *d_fixed, long fstride, const double *d_xs,
                              long xstride, long N, double *d_out) {
    hipStream_t st = h->stream;
    const int nq = c.nq, m = c.m;
    int *section = (int *)h->s_piece.ptr;
    const int *perm = (const int *)h->s_perm.ptr;
    double *packed = c.d_packed.as<double>(), *F = c.d_F.as<double>();
    int *slot_of = c.d_slot.as<int>();
    int n_live = 0;
    for (int j = 0; j < c.P; ++j) n_live += c.live[j] ? 1 : 0;
    std::vector<int> counts, offsets;
    for (long r0 = 0; r0 < N; r0 += c.chunk) {
        const long rows = std::min<long>(c.chunk, N - r0);
        const double *frows = d_fixed + (size_t)r0 * fstride;
        const double *xrows = d_xs + (size_t)r0 * xstride;
        HIP_TRY(hipMemsetAsync(h->d_counts, 0, (size_t)c.n_sections * sizeof(int), st));
        const unsigned blocks = (unsigned)((rows + PCX_LADDER_BLOCK_ROWS - 1) / PCX_LADDER_BLOCK_ROWS);
        hipLaunchKernelGGL(k_spline_row_section, dim3(blocks), dim3(256), 0, st, h->sd, h->d_knots, c.dim, frows, fstride, rows,
                           section, h->d_counts, c.n_sections, h->lds_hist);
        HIP_TRY(hipGetLastError());
        int rc = spline_scatter_keys(h, rows, c.n_sections, h->lds_hist, counts, offsets);
        if (rc) return rc;
        hipLaunchKernelGGL(k_spline_ladder_gather, dim3(grid_for(rows * std::max(nq, 1))), dim3(256), 0, st, frows, fstride, nq,
                           perm, rows, packed, slot_of);
        HIP_TRY(hipGetLastError());
        int busy = 0;
        for (int q = 0; q < c.n_sections; ++q) busy += counts[q] ? 1 : 0;
        // the (cross-section, live index) launches are independent: round-robin over the side streams, as spline_eval_chunk
        const bool fan = h->ev_fork && (long)busy * n_live > 2;
        if (fan) {
            HIP_TRY(hipEventRecord(h->ev_fork, st));
            for (int i = 0; i < pcx_spline::kSide; ++i) HIP_TRY(hipStreamWaitEvent(h->side[i], h->ev_fork, 0));
        }
        int turn = 0;
        for (int q = 0; q < c.n_sections; ++q) {
            if (counts[q] == 0) continue;
            const long head = (q / c.stride) * (c.P * c.stride) + q % c.stride;     // the piece of q with index 0 along dim
            for (int j = 0; j < c.P; ++j) {
                if (!c.live[j]) continue;
                pcx_bary *pc = h->pieces[(size_t)(head + j * c.stride)];
                const int n = c.tab[j].n;
                BaryLadder lp;
                if ((rc = bary_ladder_plan(pc, c.dim, &lp))) return rc;
                std::lock_guard<std::mutex> plk(pc->mu);
                hipStream_t ls = fan ? h->side[turn % pcx_spline::kSide] : st;
                ++turn;
                // the piece's own nodes along dim as shared values: the ladder there is the fibre itself
                rc = bary_ladder_launch(pc, lp, c.deriv, packed + (size_t)offsets[q] * nq, nq, pc->d_nodes + pc->dims.off[c.dim], 0, n,
                                        counts[q], F + (size_t)c.tab[j].foff * rows + (size_t)offsets[q] * n, ls);
                if (rc) return rc;
            }
        }
        if (fan)
            for (int i = 0; i < pcx_spline::kSide && i < turn; ++i) {
                HIP_TRY(hipEventRecord(h->ev_join[i], h->side[i]));
                HIP_TRY(hipStreamWaitEvent(st, h->ev_join[i], 0));
            }
        hipLaunchKernelGGL(k_spline_ladder_interp, dim3(grid_for(rows * m)), dim3(256), 0, st, h->sd, h->d_knots, c.dim,
                           (const SplineLadderPiece *)c.d_tab.as<SplineLadderPiece>(), (const double *)F, (const int *)slot_of,
                           xrows, xstride, m, rows, d_out + (size_t)r0 * m);
        HIP_TRY(hipGetLastError());
    }
    return PCX_OK;
}

// everything the call queued has finished before its buffers are freed, whatever the code
static int spline_ladder_finish(pcx_spline *h, int code) {
    hipError_t e = hipStreamSynchronize(h->stream);
    for (int i = 0; i < pcx_spline::kSide; ++i)
        if (h->side[i]) { const hipError_t es = hipStreamSynchronize(h->side[i]); if (e == hipSuccess) e = es; }
    if (code) return code;
    HIP_TRY(e);
    return PCX_OK;
}

extern "C" int pcx_spline_ladder_batch_dev(pcx_spline *h, int dim, const int32_t *deriv, const double *d_fixed, int64_t N,
                                           const double *xs, int m, int xs_per_row, double *d_out, void *stream) {
    PCX_API_BEGIN
    (void)stream;                                              // the work runs on the handle's streams; complete on return
    int rc = ladder_check(h, h ? h->sd.d : 0, dim, deriv, d_fixed, N, xs, m, xs_per_row, d_out);
    if (rc) return rc;
    if (N == 0 || m == 0) return PCX_OK;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    SplineLadderCall c;
    const double *d_xs = xs;
    if ((rc = spline_ladder_prepare(h, dim, deriv, m, xs_per_row ? nullptr : xs, (size_t)m, N, c))) return rc;
    if (!xs_per_row && (rc = ladder_shared_xs(h->s_ladder[4], xs, m, false, nullptr, &d_xs))) return rc;     // shared values come from the host
    rc = spline_ladder_rows(h, c, d_fixed, c.nq, d_xs, xs_per_row ? m : 0, (long)N, d_out);
    return spline_ladder_finish(h, rc);
    PCX_API_END
}

extern "C" int pcx_spline_ladder_batch(pcx_spline *h, int dim, const int32_t *deriv, const double *fixed, int64_t N,
                                       const double *xs, int m, int xs_per_row, double *out) {
    PCX_API_BEGIN
    int rc = ladder_check(h, h ? h->sd.d : 0, dim, deriv, fixed, N, xs, m, xs_per_row, out);
    if (rc) return rc;
    if (N == 0 || m == 0) return PCX_OK;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    SplineLadderCall c;
    const double *d_shared = nullptr;
    const int64_t pass = ladder_pass_rows(h->sd.d - 1, m, xs_per_row);
    if ((rc = spline_ladder_prepare(h, dim, deriv, m, xs, xs_per_row ? (size_t)N * m : (size_t)m, std::min<int64_t>(pass, N), c)))
        return rc;
    if (!xs_per_row && (rc = ladder_shared_xs(h->s_ladder[4], xs, m, false, nullptr, &d_shared))) return rc;
    // the rows run on the handle's streams: the stage's stream of a pass is h->stream
    rc = ladder_host_passes(h->stage, h->device, h->stream, c.nq, fixed, N, xs, d_shared, m, xs_per_row, out,
                            [&](const double *df, long fs, const double *dx, long xstr, long cnt, double *dout, hipStream_t) {
                                return spline_ladder_rows(h, c, df, fs, dx, xstr, cnt, dout);
                            });
    return spline_ladder_finish(h, rc);
    PCX_API_END
}

// ---------------------------------------------------------------------------------
// slider
// ---------------------------------------------------------------------------------
struct SliderLadderCall {
    int dim = 0, m = 0;
    int o = 0, lk = 0;                   // the slide that owns dim, and dim's place in its group
    int kind = 0;                        // 0 values, 1 a spec inside the owner, 2 a spec inside slide `other`, 3 across slides
    int other = -1;
    int32_t sub[PCX_MAX_DIMS] = {};      // the spec in the frame of the slide it lives in
    BaryLadder lp;                       // the owner's ladder along lk
    long chunk = 1;
    double *d_own = nullptr;             // a one-dimensional owner's shared ladder (m doubles, in the handle's s_ladder[1])
    bool own_shared = false;
};

static int slider_ladder_prepare(pcx_slider *h, int dim, const int32_t *deriv, int m, int64_t max_rows, SliderLadderCall &c) {
    c.dim = dim; c.m = m;
    c.o = h->owner[dim];
    const SliderCols &oc = h->cols[c.o];
    c.lk = 0;
    while (oc.col[c.lk] != dim) ++c.lk;
    int active = -1, n_active = 0;                             // the slides that own a differentiated dimension
    if (deriv)
        for (int k = 0; k < h->d; ++k)
            if (deriv[k] > 0 && h->owner[k] != active) {
                bool counted = false;
                for (int j = 0; j < k; ++j) counted = counted || (deriv[j] > 0 && h->owner[j] == h->owner[k]);
                if (!counted) ++n_active;
                active = h->owner[k];
            }
    c.kind = n_active == 0 ? 0 : (n_active > 1 ? 3 : (active == c.o ? 1 : 2));
    c.other = c.kind == 2 ? active : -1;
    if (c.kind == 1 || c.kind == 2)
        for (int k = 0; k < h->cols[active].nc; ++k) c.sub[k] = deriv[h->cols[active].col[k]];
    int rc = bary_ladder_plan(h->slides[c.o], c.lk, &c.lp);
    if (rc) return rc;
    const int ns = (int)h->slides.size();
    c.chunk = std::max<long>(1, std::min<long>((long)max_rows, kLadderChunkDoubles / std::max(m, 1)));
    rc = h->s_cols.reserve((size_t)c.chunk * h->max_cols * sizeof(double));
    if (!rc) rc = h->s_vals.reserve((size_t)c.chunk * ns * sizeof(double));
    return rc;
}

// slide s at the columns of the fixed rows that hold its dimensions, spec `sub`, into svals[r * ostride + ooff]
static int slider_ladder_slide(pcx_slider *h, int s, int dim, const double *frows, long fstride, long rows, const int32_t *sub,
                               double *svals, long ostride, long ooff) {
    pcx_bary *pc = h->slides[s];
    const SliderCols cc = slider_fixed_cols(h->cols[s].col, h->cols[s].nc, dim);
    double *cols = (double *)h->s_cols.ptr;
    const long elems = rows * cc.nc;
    hipLaunchKernelGGL(k_gather_columns, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, h->stream, frows, rows, (int)fstride, cc, cols);
    HIP_TRY(hipGetLastError());
    std::lock_guard<std::mutex> plk(pc->mu);
    pc->call_mark = pc->clock;
    DerivedTensor *dt = nullptr;
    int rc = bary_get_tensor(pc, sub, &dt);
    if (rc) return rc;
    return bary_launch(pc, &dt, 1, dt->slot, cols, rows, svals, ostride, ooff, h->stream, &h->s_partial);
}

// N device-resident rows into d_out (N x m), chunk by chunk, queued on h->stream.  d_xs: the values on the device
// (xstride 0: shared).  Caller holds h->mu.
static int slider_ladder_rows(pcx_slider *h, SliderLadderCall &c, const double *d_fixed, long fstride, const double *d_xs,
                              long xstride, long N, double *d_out) {
    hipStream_t st = h->stream;
    const int ns = (int)h->slides.size(), m = c.m;
    pcx_bary *po = h->slides[c.o];
    const SliderCols &oc = h->cols[c.o];
    const int g = oc.nc;
    double *cols = (double *)h->s_cols.ptr, *svals = (double *)h->s_vals.ptr;
    int rc;
    if (c.kind == 3) {                                         // a mixed partial across slides is identically zero
        hipLaunchKernelGGL(k_ladder_fill, dim3(grid_for(N * m)), dim3(256), 0, st, d_out, N * m, 0.0);
        HIP_TRY(hipGetLastError());
        return PCX_OK;
    }
    // a one-dimensional owner's fibre is its tensor: with shared values its ladder is one row, the same for every row of
    // the batch (a dense row's bits do not depend on its batch)
    const bool one_row = c.kind == 0 && g == 1 && xstride == 0;
    if (one_row && !c.own_shared) {
        if ((rc = h->s_ladder[1].reserve((size_t)m * sizeof(double)))) return rc;
        c.d_own = (double *)h->s_ladder[1].ptr;
        std::lock_guard<std::mutex> plk(po->mu);
        if ((rc = bary_ladder_launch(po, c.lp, nullptr, nullptr, 0, d_xs, 0, m, 1, c.d_own, st))) return rc;
        c.own_shared = true;
    }
    for (long r0 = 0; r0 < N; r0 += c.chunk) {
        const long rows = std::min<long>(c.chunk, N - r0);
        const double *frows = d_fixed + (size_t)r0 * fstride;
        double *dout = d_out + (size_t)r0 * m;
        if (c.kind == 2) {                                     // another slide's derivative at the row, at every value
            if ((rc = slider_ladder_slide(h, c.other, c.dim, frows, fstride, rows, c.sub, svals, 1, 0))) return rc;
            hipLaunchKernelGGL(k_slider_ladder_broadcast, dim3(grid_for(rows * m)), dim3(256), 0, st, (const double *)svals, 1L, 0L,
                               rows, m, dout);
            HIP_TRY(hipGetLastError());
            continue;
        }
        if (c.kind == 0)                                       // every other slide once per row (column o stays unread)
            for (int s = 0; s < ns; ++s)
                if (s != c.o && (rc = slider_ladder_slide(h, s, c.dim, frows, fstride, rows, nullptr, svals, ns, s))) return rc;
        if (!one_row) {
            const double *ofixed = nullptr;
            if (g > 1) {                                       // the owner's other columns, group order
                int others[PCX_MAX_DIMS];
                for (int k = 0, cc = 0; k < g; ++k)
                    if (k != c.lk) others[cc++] = oc.col[k];
                const SliderCols cc = slider_fixed_cols(others, g - 1, c.dim);
                const long elems = rows * (g - 1);
                hipLaunchKernelGGL(k_gather_columns, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, frows, rows, (int)fstride,
                                   cc, cols);
                HIP_TRY(hipGetLastError());
                ofixed = cols;
            }
            std::lock_guard<std::mutex> plk(po->mu);
            rc = bary_ladder_launch(po, c.lp, c.kind == 1 ? c.sub : nullptr, ofixed, g - 1, d_xs + (size_t)r0 * xstride, xstride, m,
                                    rows, dout, st);
            if (rc) return rc;
        }
        if (c.kind == 0) {
            hipLaunchKernelGGL(k_slider_ladder_sum, dim3(grid_for(rows * m)), dim3(256), 0, st, dout,
                               one_row ? (const double *)c.d_own : (const double *)nullptr, (const double *)svals, rows, m,
                               ns, c.o, h->pivot);
            HIP_TRY(hipGetLastError());
        }
    }
    return PCX_OK;
}

static int slider_ladder_finish(pcx_slider *h, int code) {
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (code) return code;
    HIP_TRY(e);
    return PCX_OK;
}

extern "C" int pcx_slider_ladder_batch_dev(pcx_slider *h, int dim, const int32_t *deriv, const double *d_fixed, int64_t N,
                                           const double *xs, int m, int xs_per_row, double *d_out, void *stream) {
    PCX_API_BEGIN
    (void)stream;                                              // the work runs on the handle's stream; complete on return
    int rc = ladder_check(h, h ? h->d : 0, dim, deriv, d_fixed, N, xs, m, xs_per_row, d_out);
    if (rc) return rc;
    if (N == 0 || m == 0) return PCX_OK;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    SliderLadderCall c;
    const double *d_xs = xs;
    if ((rc = slider_ladder_prepare(h, dim, deriv, m, N, c))) return rc;
    if (!xs_per_row && (rc = ladder_shared_xs(h->s_ladder[0], xs, m, false, nullptr, &d_xs))) return rc;     // shared values come from the host
    rc = slider_ladder_rows(h, c, d_fixed, h->d - 1, d_xs, xs_per_row ? m : 0, (long)N, d_out);
    return slider_ladder_finish(h, rc);
    PCX_API_END
}

extern "C" int pcx_slider_ladder_batch(pcx_slider *h, int dim, const int32_t *deriv, const double *fixed, int64_t N,
                                       const double *xs, int m, int xs_per_row, double *out) {
    PCX_API_BEGIN
    int rc = ladder_check(h, h ? h->d : 0, dim, deriv, fixed, N, xs, m, xs_per_row, out);
    if (rc) return rc;
    if (N == 0 || m == 0) return PCX_OK;
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    SliderLadderCall c;
    const double *d_shared = nullptr;
    const int64_t pass = ladder_pass_rows(h->d - 1, m, xs_per_row);
    if ((rc = slider_ladder_prepare(h, dim, deriv, m, std::min<int64_t>(pass, N), c))) return rc;
    if (!xs_per_row && (rc = ladder_shared_xs(h->s_ladder[0], xs, m, false, nullptr, &d_shared))) return rc;
    rc = ladder_host_passes(h->stage, h->device, h->stream, h->d - 1, fixed, N, xs, d_shared, m, xs_per_row, out,
                            [&](const double *df, long fs, const double *dx, long xstr, long cnt, double *dout, hipStream_t) {
                                return slider_ladder_rows(h, c, df, fs, dx, xstr, cnt, dout);
                            });
    return slider_ladder_finish(h, rc);
    PCX_API_END
}
