// spline_grid_plan.h -- the plan of a tensor-product grid evaluation of a piecewise interpolant (pcx_piecewise_grid.hip):
// which piece every axis entry belongs to, the sub-grid every piece evaluates, where its block lies in the packed
// staging buffer, and the per-axis tables from which the placement kernel finds every result element again.
//
// Piece routing is separable per dimension (ChebyshevSpline.eval_batch, reference spline.py:633-700): the interval of a
// coordinate is searchsorted(knots_k, x, side='right') clipped to the last piece -- the number of knots <= x, a
// coordinate on a knot belongs to the right-hand piece, one outside the domain to the end piece, a NaN to the last
// piece (as k_spline_piece_id routes it).  So the grid x_0 x ... x x_{d-1} falls apart into one sub-grid per piece: the
// entries of axis k that lie in the piece's interval of dimension k, in ascending position.
//
// The planner is pure: it calls nothing of the HIP runtime and launches no kernel, so every rule of it runs on a machine
// without a GPU (tests/host/spline_grid_plan_main.cpp prints the plan of any case; tests/test_piecewise_grid_host.py).
#pragma once

#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/pcx.h"

// One live piece: a piece is live when every one of its d lists is non-empty.
struct SplineGridBlock {
    long piece;                 // flat piece index (C order over the pieces per dimension)
    long offset;                // first double of the block in the packed staging buffer
    long count;                 // prod m
    int32_t m[PCX_MAX_DIMS];    // the block's shape: entries of axis k in the piece's interval of dimension k
    long axes_off;              // its sub-axes in SplineGridPlan::sub_axes: sum m doubles, dimension 0 first, list order
};

struct SplineGridPlan {
    int d = 0;
    long total = 0;                      // prod m_k: the blocks tile exactly this many doubles
    long n_pieces = 0;
    std::vector<long> axis_off;          // d + 1: offset of dimension k's entries in axes_cat, interval, rank and list
    std::vector<long> cnt_off;           // d + 1: offset of dimension k's intervals in count and list_off
    std::vector<int32_t> interval;       // per axis entry: its interval along its dimension
    std::vector<int32_t> rank;           // per axis entry: its position in its interval's list
    std::vector<int32_t> count;          // per (dimension, interval): entries in the list
    std::vector<long> list_off;          // per (dimension, interval): where the list starts in `list`
    std::vector<int32_t> list;           // per dimension, the positions grouped by interval, ascending inside one (stable)
    std::vector<SplineGridBlock> blocks; // the live pieces, ascending flat index; block after block in the staging buffer
    std::vector<long> block_off;         // per piece: the offset of its block, -1 for a dead piece
    std::vector<double> sub_axes;        // the blocks' sub-axes one behind the other
};

// number of knots <= x; a NaN compares false with everything and goes to the last interval
static inline int spline_grid_interval(const double *knots, int nknots, double x) {
    if (x != x) return nknots;
    int idx = 0;
    for (int j = 0; j < nknots; ++j) idx += (knots[j] <= x) ? 1 : 0;
    return idx;             // <= nknots = pieces - 1: the clip of the reference never bites
}

// PCX_OK, PCX_ERR_INVALID (a NULL array, d out of range, an empty axis: names the dimension) or PCX_ERR_UNSUPPORTED (more
// than max_total grid points) with the reason in err.  knots_cat holds the knots of dimension 0 first (sorted per
// dimension, n_knots[k] of them; may be NULL when there are none at all).
static inline int spline_grid_make_plan(int d, const int32_t *n_knots, const double *knots_cat, const int32_t *m,
                                        const double *axes_cat, long max_total, SplineGridPlan &sp, char *err, size_t errlen) {
    if (d < 1 || d > PCX_MAX_DIMS) {
        snprintf(err, errlen, "d=%d outside [1, %d]", d, PCX_MAX_DIMS);
        return PCX_ERR_INVALID;
    }
    if (!n_knots || !m || !axes_cat) {
        snprintf(err, errlen, "NULL argument");
        return PCX_ERR_INVALID;
    }
    sp.d = d;
    sp.axis_off.assign(d + 1, 0);
    sp.cnt_off.assign(d + 1, 0);
    sp.total = 1;
    sp.n_pieces = 1;
    long nk_total = 0;
    for (int k = 0; k < d; ++k) {
        if (n_knots[k] < 0) {
            snprintf(err, errlen, "n_knots[%d]=%d < 0", k, n_knots[k]);
            return PCX_ERR_INVALID;
        }
        if (m[k] < 1) {
            snprintf(err, errlen, "m[%d]=%d: the axis of dimension %d is empty", k, m[k], k);
            return PCX_ERR_INVALID;
        }
        if ((double)sp.total * m[k] > (double)max_total) {
            snprintf(err, errlen, "grid of more than 2^40 points");
            return PCX_ERR_UNSUPPORTED;
        }
        sp.total *= m[k];
        sp.n_pieces *= n_knots[k] + 1;
        sp.axis_off[k + 1] = sp.axis_off[k] + m[k];
        sp.cnt_off[k + 1] = sp.cnt_off[k] + n_knots[k] + 1;
        nk_total += n_knots[k];
    }
    if (nk_total > 0 && !knots_cat) {
        snprintf(err, errlen, "knots_cat is NULL");
        return PCX_ERR_INVALID;
    }
    const long sm = sp.axis_off[d], sc = sp.cnt_off[d];
    sp.interval.assign((size_t)sm, 0);
    sp.rank.assign((size_t)sm, 0);
    sp.list.assign((size_t)sm, 0);
    sp.count.assign((size_t)sc, 0);
    sp.list_off.assign((size_t)sc, 0);
    // per dimension: intervals, a counting sort of the positions by interval (stable), ranks
    long koff = 0;
    for (int k = 0; k < d; ++k) {
        const long a0 = sp.axis_off[k], c0 = sp.cnt_off[k];
        const int shape = n_knots[k] + 1;
        for (int i = 0; i < m[k]; ++i) {
            const int iv = spline_grid_interval(knots_cat + koff, n_knots[k], axes_cat[a0 + i]);
            sp.interval[a0 + i] = iv;
            sp.rank[a0 + i] = sp.count[c0 + iv]++;
        }
        long at = a0;
        for (int j = 0; j < shape; ++j) {
            sp.list_off[c0 + j] = at;
            at += sp.count[c0 + j];
        }
        for (int i = 0; i < m[k]; ++i) sp.list[sp.list_off[c0 + sp.interval[a0 + i]] + sp.rank[a0 + i]] = i;
        koff += n_knots[k];
    }
    // the live pieces in ascending flat index: an odometer over the non-empty intervals of every dimension
    std::vector<std::vector<int>> alive(d);
    for (int k = 0; k < d; ++k)
        for (int j = 0; j <= n_knots[k]; ++j)
            if (sp.count[sp.cnt_off[k] + j]) alive[k].push_back(j);
    sp.block_off.assign((size_t)sp.n_pieces, -1);
    sp.blocks.clear();
    sp.sub_axes.clear();
    std::vector<size_t> pos(d, 0);
    long offset = 0;
    for (;;) {
        SplineGridBlock b;
        b.piece = 0;
        b.count = 1;
        b.offset = offset;
        b.axes_off = (long)sp.sub_axes.size();
        for (int k = 0; k < PCX_MAX_DIMS; ++k) b.m[k] = 1;
        for (int k = 0; k < d; ++k) {
            const int j = alive[k][pos[k]];
            const long c = sp.cnt_off[k] + j;
            b.piece = b.piece * (n_knots[k] + 1) + j;
            b.m[k] = sp.count[c];
            b.count *= b.m[k];
            for (int r = 0; r < b.m[k]; ++r) sp.sub_axes.push_back(axes_cat[sp.axis_off[k] + sp.list[sp.list_off[c] + r]]);
        }
        sp.block_off[b.piece] = offset;
        offset += b.count;
        sp.blocks.push_back(b);
        int k = d - 1;
        while (k >= 0 && ++pos[k] == alive[k].size()) pos[k--] = 0;
        if (k < 0) break;
    }
    return PCX_OK;
}
