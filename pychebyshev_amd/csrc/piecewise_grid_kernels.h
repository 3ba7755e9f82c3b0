// piecewise_grid_kernels.h -- the two assembly kernels of tensor-product grid evaluation on piecewise interpolants and
// sliders (pcx_piecewise_grid.hip).  gfx950.
//
// Both write the whole result in one launch, one double per lane and step, consecutive lanes along the LAST dimension
// (coalesced 512-byte stores per wave); both are bandwidth-bound copies: nothing is summed that the per-piece or
// per-slide grids have not already computed.  Indices are 64-bit; the multi-index of an element is decoded in 32-bit
// arithmetic when the grid has fewer than 2^32 points (template parameter I).  No atomics; a lane past the end forms
// no address.
//
// Each kernel has two forms.  The `_run` form (grids of up to PCX_PG_RUN_DIMS dimensions) decodes a lane's multi-index
// ONCE, with D divisions, and then walks the grid in strides of the whole launch: the stride's digits in the mixed radix
// m_0 .. m_{D-1} are added to the multi-index with a carry (GridWalk), so the lanes of a wave stay on consecutive
// elements and a further element costs D adds and compares in registers.  The plain form divides D times per element
// and takes any number of dimensions.  (profiles/piecewise_grid_probe.txt has both.)
#pragma once

#include "pcx_common.h"

#define PCX_PG_THREADS 256
#define PCX_PG_RUN_DIMS 6

// the walk of the `_run` forms: axis lengths and the digits of the launch's stride (blocks * PCX_PG_THREADS mod the grid)
struct GridWalk {
    int m[PCX_PG_RUN_DIMS];
    int step[PCX_PG_RUN_DIMS];
};

template <int D, typename I>
__device__ __forceinline__ void grid_walk_decode(const GridWalk &gw, long e, int (&idx)[D]) {
    I rem = (I)e;
#pragma unroll
    for (int k = D - 1; k >= 0; --k) {
        const I q = rem / (I)gw.m[k];
        idx[k] = (int)(rem - q * (I)gw.m[k]);
        rem = q;
    }
}

// idx += step in the mixed radix: digits and steps are below m, so one subtraction settles a digit
template <int D>
__device__ __forceinline__ void grid_walk_advance(const GridWalk &gw, int (&idx)[D]) {
    int carry = 0;
#pragma unroll
    for (int k = D - 1; k >= 0; --k) {
        const int v = idx[k] + gw.step[k] + carry;
        carry = v >= gw.m[k] ? 1 : 0;
        idx[k] = carry ? v - gw.m[k] : v;
    }
}

// the result's shape and where each dimension's tables start (spline_grid_plan.h)
struct SplineGridDims {
    int d;
    int m[PCX_MAX_DIMS];        // axis lengths
    int shape[PCX_MAX_DIMS];    // pieces per dimension
    long aoff[PCX_MAX_DIMS];    // dimension k's entries in interval / rank
    long coff[PCX_MAX_DIMS];    // dimension k's intervals in count
};

// out[i_0, .., i_{d-1}] = stage[block_off[piece] + local]: per dimension the entry's interval selects the piece and the
// extent of its block, the entry's rank in the interval's list is its index inside the block (C order).  Reads are
// contiguous runs of the staging buffer wherever the last axis is sorted.
template <typename I>
__global__ void __launch_bounds__(PCX_PG_THREADS)
k_spline_grid_place(SplineGridDims gd, const int *__restrict__ interval, const int *__restrict__ rank,
                    const int *__restrict__ count, const long *__restrict__ block_off, const double *__restrict__ stage,
                    double *__restrict__ out, long total) {
    const long step = (long)gridDim.x * PCX_PG_THREADS;
    for (long e = (long)blockIdx.x * PCX_PG_THREADS + threadIdx.x; e < total; e += step) {
        I rem = (I)e;
        long local = 0, mul = 1, piece = 0, pmul = 1;
        for (int k = gd.d - 1; k >= 0; --k) {
            const I q = rem / (I)gd.m[k];
            const long i = (long)(rem - q * (I)gd.m[k]);
            rem = q;
            const int iv = interval[gd.aoff[k] + i];
            local += rank[gd.aoff[k] + i] * mul;
            mul *= count[gd.coff[k] + iv];
            piece += iv * pmul;
            pmul *= gd.shape[k];
        }
        out[e] = stage[block_off[piece] + local];
    }
}

template <int D, typename I>
__global__ void __launch_bounds__(PCX_PG_THREADS)
k_spline_grid_place_run(SplineGridDims gd, GridWalk gw, const int *__restrict__ interval, const int *__restrict__ rank,
                        const int *__restrict__ count, const long *__restrict__ block_off, const double *__restrict__ stage,
                        double *__restrict__ out, long total) {
    const long step = (long)gridDim.x * PCX_PG_THREADS;
    long e = (long)blockIdx.x * PCX_PG_THREADS + threadIdx.x;
    if (e >= total) return;
    int idx[D];
    grid_walk_decode<D, I>(gw, e, idx);
    for (; e < total; e += step) {
        long local = 0, mul = 1, piece = 0, pmul = 1;
#pragma unroll
        for (int k = D - 1; k >= 0; --k) {
            const int iv = interval[gd.aoff[k] + idx[k]];
            local += rank[gd.aoff[k] + idx[k]] * mul;
            mul *= count[gd.coff[k] + iv];
            piece += iv * pmul;
            pmul *= gd.shape[k];
        }
        out[e] = stage[block_off[piece] + local];
        grid_walk_advance<D>(gw, idx);
    }
}

// Slider: out[i] = ((pivot + (G_0[i|g_0] - pivot)) + (G_1[i|g_1] - pivot)) + ...  -- k_slider_sum's order of operations
// (route_kernels.h) on the slides' own grids G_s, each indexed by the coordinates of its group only.  `tab` (8-byte
// words): term_begin[ns + 1], g_off[ns], then per term (cs, m, gs): the dimension's C-order stride in the result, its
// axis length, and its stride in G_s -- the table of one stride per (slide, dimension) with the zero entries (the
// dimensions the slide does not own) and the axes of length 1 left out, so an element costs one division pair per
// dimension of the grid, not per (slide, dimension).  plain != 0: one slide, no pivot terms, out[i] = G_0[i|g_0]
// (a derivative that lies in one slide, broadcast over every other dimension).
template <typename I>
__global__ void __launch_bounds__(PCX_PG_THREADS)
k_slider_grid_sum(const double *__restrict__ G, const long *__restrict__ tab, int ns, double pivot, int plain,
                  double *__restrict__ out, long total) {
    const long *term_begin = tab, *g_off = tab + ns + 1, *terms = tab + 2 * ns + 1;
    const long step = (long)gridDim.x * PCX_PG_THREADS;
    for (long e = (long)blockIdx.x * PCX_PG_THREADS + threadIdx.x; e < total; e += step) {
        double r = pivot;
        for (int s = 0; s < ns; ++s) {
            long off = g_off[s];
            for (long j = term_begin[s]; j < term_begin[s + 1]; ++j) {
                const I cs = (I)terms[3 * j], m = (I)terms[3 * j + 1];
                off += (long)(((I)e / cs) % m) * terms[3 * j + 2];
            }
            const double v = G[off];
            r = plain ? v : r + (v - pivot);
        }
        out[e] = r;
    }
}

// The `_run` form over the D axes longer than 1: `tab` = g_off[ns], then the dense table stride[ns][D] of G_s's stride
// along each of them, zero where slide s does not own the dimension.
template <int D, typename I>
__global__ void __launch_bounds__(PCX_PG_THREADS)
k_slider_grid_sum_run(GridWalk gw, const double *__restrict__ G, const long *__restrict__ tab, int ns, double pivot, int plain,
                      double *__restrict__ out, long total) {
    const long *g_off = tab, *stride = tab + ns;
    const long step = (long)gridDim.x * PCX_PG_THREADS;
    long e = (long)blockIdx.x * PCX_PG_THREADS + threadIdx.x;
    if (e >= total) return;
    int idx[D];
    grid_walk_decode<D, I>(gw, e, idx);
    for (; e < total; e += step) {
        double r = pivot;
        for (int s = 0; s < ns; ++s) {
            I off = 0;
#pragma unroll
            for (int k = 0; k < D; ++k) off += (I)idx[k] * (I)stride[(long)s * D + k];
            const double v = G[g_off[s] + (long)off];
            r = plain ? v : r + (v - pivot);
        }
        out[e] = r;
        grid_walk_advance<D>(gw, idx);
    }
}
