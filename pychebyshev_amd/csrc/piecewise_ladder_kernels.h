// piecewise_ladder_kernels.h -- the structure around the dense fibre contraction (bary_ladder_kernels.h) that turns it
// into ladders of the piecewise interpolant (ChebyshevSpline.ladder_batch) and of the slider (ChebyshevSlider.ladder_batch).
// gfx950.  `static`: the one translation unit that includes it (pcx_piecewise_ladder.hip) carries the kernels.
//
// Spline.  A row's d - 1 fixed coordinates select its CROSS-SECTION: the piece index in every dimension but `dim`, as a
// flat C-order index over those dimensions.  Rows are bucketed by cross-section, every piece (cross-section q, index j
// along dim) contracts the fibres of q's rows on its own tensor, and each (row, x) cell interpolates the fibre of the
// piece its x falls into.  Fibres live in one region per index j along dim, rows x n_j doubles in bucket-slot order:
//     F[(foff_j * rows) + slot * n_j + node],      foff_j = sum of n_j' over the live j' < j
// so piece (q, j) writes dense at start_q * n_j and the interpolation needs no table beyond SplineLadderPiece[j].
//
// No LDS beyond the routing histogram, no atomics outside it, a fixed order of additions.
#pragma once

#include "bary_ladder_kernels.h"

// number of knots <= x, clamped to the last piece; NaN sorts behind every knot (k_spline_piece_id's rule per dimension)
__device__ __forceinline__ int spline_dim_piece(const SplineDims &sd, const double *__restrict__ knots, int k, double x) {
    int idx = 0;
    if (x != x) idx = sd.nknots[k];
    else
        for (int j = 0; j < sd.nknots[k]; ++j) idx += (knots[sd.koff[k] + j] <= x) ? 1 : 0;
    return idx > sd.shape[k] - 1 ? sd.shape[k] - 1 : idx;
}

#define PCX_LADDER_LDS_SECTIONS 4096      // histograms of up to this many cross-sections live in LDS
#define PCX_LADDER_BLOCK_ROWS 4096        // rows per workgroup of the routing kernel

// Routing + histogram of the rows, k_spline_piece_id's scheme: section[r] = the flat index over the dimensions but dim of
// the pieces that hold fixed[r * fstride + i]; each workgroup counts its rows in LDS and adds one number per non-empty
// cross-section to counts (lds_hist = 0, more cross-sections than LDS holds: one global atomic per row).
static __global__ void __launch_bounds__(256)
k_spline_row_section(SplineDims sd, const double *__restrict__ knots, int dim, const double *__restrict__ fixed, long fstride,
                     long rows, int *__restrict__ section, int *__restrict__ counts, int n_sections, int lds_hist) {
    __shared__ int hist[PCX_LADDER_LDS_SECTIONS];
    const long lo = (long)blockIdx.x * PCX_LADDER_BLOCK_ROWS;
    const long hi = lo + PCX_LADDER_BLOCK_ROWS < rows ? lo + PCX_LADDER_BLOCK_ROWS : rows;
    if (lds_hist) {
        for (int i = threadIdx.x; i < n_sections; i += 256) hist[i] = 0;
        __syncthreads();
    }
    for (long r = lo + threadIdx.x; r < hi; r += 256) {
        int flat = 0;
        for (int k = 0, i = 0; k < sd.d; ++k) {
            if (k == dim) continue;
            flat = flat * sd.shape[k] + spline_dim_piece(sd, knots, k, fixed[r * fstride + i]);
            ++i;
        }
        section[r] = flat;
        atomicAdd(lds_hist ? &hist[flat] : &counts[flat], 1);
    }
    if (lds_hist) {
        __syncthreads();
        for (int i = threadIdx.x; i < n_sections; i += 256)
            if (hist[i]) atomicAdd(&counts[i], hist[i]);
    }
}

// The rows in bucket order, packed nq wide: packed[slot * nq + i] = fixed[perm[slot] * fstride + i], and where each row
// went: slot_of[perm[slot]] = slot.
static __global__ void __launch_bounds__(256)
k_spline_ladder_gather(const double *__restrict__ fixed, long fstride, int nq, const int *__restrict__ perm, long rows,
                       double *__restrict__ packed, int *__restrict__ slot_of) {
    const long total = rows * (nq > 0 ? nq : 1);
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long slot = nq > 0 ? e / nq : e;
        const int i = nq > 0 ? (int)(e - slot * nq) : 0;
        const long r = perm[slot];
        if (nq > 0) packed[e] = fixed[r * fstride + i];
        if (i == 0) slot_of[r] = (int)slot;
    }
}

// index j along dim: its grid (the piece with index 0 in every other dimension holds it; all pieces of index j share the
// node count) and where its fibres start, in doubles per row of the chunk (-1: no value of the call falls into j)
struct SplineLadderPiece {
    int n;
    long foff;
    const double *nodes, *wts;
};

// out[r * m + x] = the 1-D interpolant of the fibre of (row r, the piece that holds xs[r * xstride + x]) at that value:
// the piece along dim by the knot rule, the fibre through the row's bucket slot.  One thread per cell, x fastest.
static __global__ void __launch_bounds__(256)
k_spline_ladder_interp(SplineDims sd, const double *__restrict__ knots, int dim, const SplineLadderPiece *__restrict__ tab,
                       const double *__restrict__ F, const int *__restrict__ slot_of, const double *__restrict__ xs,
                       long xstride, int m, long rows, double *__restrict__ out) {
    const long total = rows * m;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long r = e / m;
        const int xi = (int)(e - r * m);
        const double x = xs[r * xstride + xi];
        const SplineLadderPiece p = tab[spline_dim_piece(sd, knots, dim, x)];
        out[e] = ladder_interp_1d(x, p.nodes, p.wts, p.n, F + p.foff * rows + (long)slot_of[r] * p.n);
    }
}

// Slider, in place over the (rows x m) block: cell (r, x) holds the owner slide's ladder value v_o -- or, shared != NULL,
// takes it from shared[x] (a one-dimensional owner with shared values: its ladder is the same for every row) -- and
// becomes ((pivot + (v_0 - pivot)) + (v_1 - pivot)) + ..., slides in partition order, v_i = slide_vals[r * n_slides + i]
// for every slide but the owner: k_slider_sum's order of operations (additions and subtractions only: nothing to fuse).
static __global__ void __launch_bounds__(256)
k_slider_ladder_sum(double *__restrict__ out, const double *__restrict__ shared, const double *__restrict__ slide_vals,
                    long rows, int m, int n_slides, int owner, double pivot) {
    const long total = rows * m;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long r = e / m;
        const double own = shared ? shared[e - r * m] : out[e];
        double acc = pivot;
        for (int i = 0; i < n_slides; ++i) acc += (i == owner ? own : slide_vals[r * n_slides + i]) - pivot;
        out[e] = acc;
    }
}

// out[r * m + x] = vals[r * vstride + voff]: a slide's derivative at the row, the same at every value along dim
static __global__ void __launch_bounds__(256)
k_slider_ladder_broadcast(const double *__restrict__ vals, long vstride, long voff, long rows, int m, double *__restrict__ out) {
    const long total = rows * m;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x)
        out[e] = vals[(e / m) * vstride + voff];
}

// out[e] = v, e < total
static __global__ void __launch_bounds__(256) k_ladder_fill(double *__restrict__ out, long total, double v) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) out[e] = v;
}
