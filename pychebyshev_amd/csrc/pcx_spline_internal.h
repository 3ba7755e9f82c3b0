// pcx_spline_internal.h -- the spline (piecewise) handle as the translation units that serve it see it (pcx_spline.hip
// creates and evaluates it, pcx_calculus.hip runs its calculus).  Not part of the ABI.
#pragma once

#include "pcx_bary_internal.h"

// ---------------------------------------------------------------------------------
// spline (piecewise) handle
// ---------------------------------------------------------------------------------
struct pcx_spline {
    int device = 0;
    hipStream_t stream = nullptr;
    SplineDims sd;
    int n_pieces = 0;
    std::vector<pcx_bary *> pieces;      // borrowed
    std::vector<double> knots;           // knots_cat on the host (the piece edges of pcx_spline_calculus_batch)
    double *d_knots = nullptr;
    int *d_counts = nullptr;             // n_pieces: histogram, then bucket cursors
    int lds_hist = 1;                    // routing kernels count per workgroup in LDS (<= PCX_SPLINE_LDS_PIECES pieces)
    // the per-piece launches of one batch are independent: they go round-robin over a few side streams so
    // that small buckets overlap instead of queueing behind each other's launch latency
    static const int kSide = 4;
    hipStream_t side[kSide] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[kSide] = {nullptr, nullptr, nullptr, nullptr};
    std::mutex mu;
    HostStage stage;                     // host-pointer batches (and the points of pcx_spline_piece_ids)
    Scratch s_piece, s_perm, s_partial;
    // one launch for all pieces (pieces of equal shape on the lane-per-point kernel): per-piece model table,
    // per-workgroup (piece, first slot) lists; staged through a pinned host buffer
    bool fused_ok = false;
    Scratch s_models, s_blk;
    void *pin_stage = nullptr;
    size_t pin_cap = 0;
    // tensor-product grids (pcx_piecewise_grid.hip): the pieces' blocks are staged in s_gridstage, the placement
    // kernel's tables sit in s_gridtab (uploaded from grid_tab_host), a host result is staged in s_gridout; grid_done is
    // recorded behind the placement of a call, and the next call waits for it before it touches any of them
    Scratch s_gridstage, s_gridtab, s_gridout;
    std::vector<long> grid_tab_host;
    hipEvent_t grid_done = nullptr;
    // ladders (pcx_piecewise_ladder.hip): the per-index table, the rows in bucket order, their slots, the fibres, shared xs
    Scratch s_ladder[5];
};

// pcx_spline.hip: one chunk of cnt device-resident points (cnt x d) through routing, bucketing and the per-piece
// launches on h->stream, m specs (derivs NULL: the values), results into dout (cnt x m) in point order; the launches are
// queued, not awaited.  Caller holds h->mu.
PCX_HIDDEN int spline_eval_chunk(pcx_spline *h, const double *dp, long cnt, const int32_t *derivs, int m, double *dout);
// pcx_spline.hip: the second half of bucketing, for keys somebody else wrote (pcx_piecewise_ladder.hip buckets rows by
// cross-section).  h->s_piece holds cnt keys in [0, n_keys), h->d_counts their histogram, both queued on h->stream;
// h->s_perm is reserved.  Returns counts / offsets on the host and the permutation in h->s_perm, complete.  n_keys <=
// h->n_pieces; lds_hist as in the handle.  Caller holds h->mu.
PCX_HIDDEN int spline_scatter_keys(pcx_spline *h, long cnt, int n_keys, int lds_hist, std::vector<int> &counts,
                                   std::vector<int> &offsets);
