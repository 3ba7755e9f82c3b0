// spline_calc_kernels.h -- the spline's own kernels for roots, minima and maxima along one dimension
// (pcx_spline_calculus_batch, reference spline.py:1762-1910: "solve every piece along the dimension, merge").  gfx950.
//
// Along `dim` the spline has P pieces over [e_j, e_j+1], piece j with n_j nodes.  A pass of `rows` rows keeps three
// piece-major layouts (noff / woff: prefix sums of n_j / max(n_j - 1, 1)):
//
//   points, values   piece j's block at rows noff[j], row r at + r n_j: every fibre is a contiguous row of n_j
//   piece roots      piece j's block at rows woff[j], row r at + r W_j
//   piece counts, values, locations      [j rows + r]
//
// k_spline_calc_expand writes the points, the spline's own evaluation fills the values, k_cheb1d_calculus_pieces solves
// all rows P fibres in one launch (calc_row of calculus_kernels.h, unchanged) and k_spline_calc_merge joins the pieces of
// every row.  Only pcx_calculus.hip includes this file.
#pragma once

#include "calculus_kernels.h"

#pragma clang fp contract(off)     // the merge's tolerance and differences round as the NumPy statements do

// one piece along `dim`, as the kernels read it (device table, entry j: wave-uniform scalar loads)
struct SplineCalcPiece {
    int n, W;                        // nodes of the piece along dim, its roots row stride max(n - 1, 1)
    double lo, hi;                   // [e_j, e_j+1]
    const double *nodes, *wts, *diff;   // of the piece whose other indices are 0: shared by every piece with index j
    long voff;                       // noff[j]: the piece's points / values start at rows * voff
    long roff;                       // woff[j]: its roots at rows * roff, and its columns in a row of the merged output
};

#if defined(__HIPCC__)
// Fibre points.  Grid (x over the piece's rows n d elements, y = piece j): point (r, j, i) = the fixed values of row r in
// every column but `dim` (increasing column order) and piece j's node i, copied bit for bit, in column `dim`.
__global__ __launch_bounds__(256) void k_spline_calc_expand(const double *__restrict__ fixed, long rows, int d, int dim,
                                                            const SplineCalcPiece *__restrict__ tab,
                                                            double *__restrict__ pts) {
    const SplineCalcPiece pc = tab[blockIdx.y];
    const int n = pc.n;
    const long total = rows * n * d;
    double *out = pts + rows * pc.voff * d;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int e = (int)(idx % d);
        const long p = idx / d;
        const int i = (int)(p % n);
        const long r = p / n;
        out[idx] = e == dim ? pc.nodes[i] : fixed[r * (d - 1) + (e < dim ? e : e - 1)];
    }
}

// One wave (workgroup) per fibre: block j rows + r solves row r of piece j.  MP bounds the largest colleague matrix of
// any piece (max_j n_j - 1) and sizes the LDS as in k_cheb1d_calculus.
struct SplineCalcOut {
    const double *vals;              // rows * F fibre values
    double *roots;                   // rows * W piece roots (mode 0)
    int32_t *counts;                 // P * rows
    double *val, *loc;               // P * rows each (modes 1, 2)
};

template <int MP>
__global__ __launch_bounds__(64) void k_cheb1d_calculus_pieces(const SplineCalcPiece *__restrict__ tab, long rows, int mode,
                                                               SplineCalcOut o) {
    __shared__ double lds[MP * (MP + 1) + PCX_CALC_EXTRA];
    const long j = (long)blockIdx.x / rows;
    const long r = (long)blockIdx.x - j * rows;
    const SplineCalcPiece pc = tab[j];
    CalcArgs a;
    a.n = pc.n; a.mode = mode; a.W = pc.W; a.lo = pc.lo; a.hi = pc.hi;
    a.nodes = pc.nodes; a.wts = pc.wts; a.diff = pc.diff;
    a.vals = o.vals + rows * pc.voff;
    a.counts = o.counts + j * rows;
    a.roots = nullptr; a.val = nullptr; a.loc = nullptr;       // only the mode's own outputs exist
    if (mode == 0) a.roots = o.roots + rows * pc.roff;
    else { a.val = o.val + j * rows; a.loc = o.loc + j * rows; }
    calc_row<MP + 1>(a, r, lds, MP);
}

// One thread per row: the pieces' results, in piece order, into row r of the outputs (already offset to the pass).
//   roots: the pieces' roots concatenated (pieces are ordered, a piece's roots ascend inside its interval); element q is
//          kept iff q == 0 or x_q - x_(q-1) > tol with x_(q-1) its immediate predecessor in the concatenation, kept or
//          not (np.diff(combined) > tol); the rest of the row is NaN; counts = roots kept
//   min / max: (+inf, 0) / (-inf, 0), replaced by a piece only on strict < / >; counts = the pieces' critical points
// A row with a failed piece (count -1) gets counts -1 and NaN everywhere.
__global__ __launch_bounds__(256) void k_spline_calc_merge(const SplineCalcPiece *__restrict__ tab, int P, long rows, int mode,
                                                           int Wtot, double dom_lo, double dom_hi, SplineCalcOut o,
                                                           double *__restrict__ roots_out, int32_t *__restrict__ counts_out,
                                                           double *__restrict__ val_out, double *__restrict__ loc_out) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    bool failed = false;
    int sum = 0;
    for (int j = 0; j < P; ++j) {
        const int c = o.counts[(long)j * rows + r];
        failed = failed || c < 0;
        sum += c;
    }
    if (mode == 0) {
        double *out = roots_out + r * Wtot;
        int kept = 0;
        if (!failed) {
            const double scale = fabs(dom_hi - dom_lo) + 1.0;
            const double tol = 1e-10 * scale;
            bool first = true;
            double prev = 0.0;
            for (int j = 0; j < P; ++j) {
                const SplineCalcPiece pc = tab[j];
                const double *src = o.roots + rows * pc.roff + r * pc.W;
                const int c = o.counts[(long)j * rows + r];
                for (int q = 0; q < c; ++q) {
                    const double x = src[q];
                    if (first || (x - prev) > tol) out[kept++] = x;
                    first = false;
                    prev = x;
                }
            }
        }
        for (int q = kept; q < Wtot; ++q) out[q] = NAN;
        counts_out[r] = failed ? -1 : kept;
        return;
    }
    if (failed) {
        counts_out[r] = -1;
        val_out[r] = NAN;
        loc_out[r] = NAN;
        return;
    }
    double bv = mode == 1 ? INFINITY : -INFINITY, bl = 0.0;
    for (int j = 0; j < P; ++j) {
        const double v = o.val[(long)j * rows + r];
        if (mode == 1 ? v < bv : v > bv) { bv = v; bl = o.loc[(long)j * rows + r]; }
    }
    counts_out[r] = sum;
    val_out[r] = bv;
    loc_out[r] = bl;
}
#endif
