// slider_calc_kernels.h -- the slider's own kernels for calculus along one dimension (pcx_slider_calculus_batch) and for
// per-row box integrals (pcx_slider_box_batch).  A slider is f(x) = pv + sum_i (s_i(x_Gi) - pv): along one dimension only
// the slide that owns it varies, and a box integral is a sum of the slides' own box integrals scaled by box widths.
// `static`: each translation unit that includes it carries its own copy.
#pragma once

#include "pcx_common.h"

#pragma clang fp contract(off)     // eval()'s roundings: no fused multiply-add

// Fibre values in place.  Element (r, j): acc = pivot, then acc += v_i - pivot for the slides in partition order, where
// v_i is the owner's fibre value at (r, j) -- vals[r n + j], or owner_plain[j] when the owner is one-dimensional and its
// value tensor IS the fibre -- and slide_vals[r n_slides + i] for every other slide.  pcx_slider_eval's order.
static __global__ __launch_bounds__(256) void k_slider_fibre_sum(double *__restrict__ vals, const double *__restrict__ owner_plain,
                                                                  const double *__restrict__ slide_vals, long rows, int n,
                                                                  int n_slides, int owner, double pivot) {
    const long total = rows * n;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long r = idx / n;
        const int j = (int)(idx - r * n);
        const double own = owner_plain ? owner_plain[j] : vals[idx];
        double acc = pivot;
        for (int i = 0; i < n_slides; ++i) acc += (i == owner ? own : slide_vals[r * n_slides + i]) - pivot;
        vals[idx] = acc;
    }
}

// A slide's box row out of the slider's: out[r][c] = rows[r][src[c]], c < w (src: device table of w source columns --
// one per kept dimension of the slide, two per integrated one)
static __global__ __launch_bounds__(256) void k_slider_box_row(const double *__restrict__ rows, long N, int width,
                                                                const int *__restrict__ src, int w, double *__restrict__ out) {
    const long total = N * w;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long r = idx / w;
        const int c = (int)(idx - r * w);
        out[idx] = rows[r * width + src[c]];
    }
}

// out[r] = pv vol_T + sum_i vol(T \ G_i) (I_i - pv vol(T n G_i)), slides in partition order; I_i = ints[i N + r].
// vol(S): the product of the row's hi - lo over the integrated dimensions in S, in increasing dimension order (1 when
// there is none), always a product -- a row with lo == hi gives exactly 0.  off / integ / owner: d entries each.
static __global__ __launch_bounds__(256) void k_slider_box_combine(const double *__restrict__ rows, long N, int width, int d,
                                                                    const int *__restrict__ off, const int *__restrict__ integ,
                                                                    const int *__restrict__ owner, int n_slides, double pivot,
                                                                    const double *__restrict__ ints, double *__restrict__ out) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const double *row = rows + r * width;
    double vol_t = 1.0;
    for (int u = 0; u < d; ++u)
        if (integ[u]) vol_t *= row[off[u] + 1] - row[off[u]];
    double acc = pivot * vol_t;
    for (int i = 0; i < n_slides; ++i) {
        double vin = 1.0, vout = 1.0;
        for (int u = 0; u < d; ++u) {
            if (!integ[u]) continue;
            const double wu = row[off[u] + 1] - row[off[u]];
            if (owner[u] == i) vin *= wu; else vout *= wu;
        }
        acc += vout * (ints[(long)i * N + r] - pivot * vin);
    }
    out[r] = acc;
}
