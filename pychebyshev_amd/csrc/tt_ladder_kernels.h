// tt_ladder_kernels.h -- ladders of a tensor train in Chebyshev coefficient space: for every row of the batch, the model
// along one dimension at m values (ChebyshevTT.ladder_batch / fibre_batch; gfx950).
//
// With the dimension at storage position p, a row's restriction to it is a Chebyshev series of n_p coefficients:
//     L = prod_{k < p} (sum_j T_j(s_k) G_k[:, j, :])          (1 x r_{p-1}, positions 0 .. p-1 in order)
//     R = prod_{k > p} (sum_j T_j(s_k) G_k[:, j, :])          (r_p x 1, from the last position down to p + 1)
//     c_i = L . G_p[:, i, :] . R,        ladder[x] = sum_i c_i T_i(s(x))
// with s = fma(x - lo, 2 / (hi - lo), -1) and T_0 = 1, T_1 = s, T_j = fma(2 s, T_{j-1}, -T_{j-2}) as the evaluation
// kernels form them.  The two chains and the coefficients cost the row about one evaluation; each of its m values then
// costs n_p FMAs.
//
//   k_tt_ladder_lpp       one row per lane on the lane-per-point image (ranks <= 16, n <= 16): core elements are
//                         wave-uniform scalar operands, the node count of a dimension is a compile-time value (one body
//                         per count, picked per dimension), the ranks run at run time through lane-private LDS columns
//   k_tt_ladder_generic   one row per wave on the plain cores, for every other model
//
// `fixed` holds the user's dimensions but `dim` in increasing order; fcol[k] is the column storage position k reads
// (dim_order applied here, on the device).  No atomics, every sum in a fixed order: a row's bits depend neither on the
// batch nor on m.
#pragma once

#include "tt_lpp_kernels.h"
#include "tt_wave_kernels.h"

struct TTLadder {
    int d, p;                     // dimensions; storage position of the ladder's dimension
    int m;
    int rmax;
    int fcol[PCX_MAX_DIMS];       // column of `fixed` read by storage position k (unused at p)
};

// sum_j T_j G[j]: one core fibre (a, :, b) of the image
template <int NJ>
__device__ __forceinline__ double tt_ladder_fold(pcx_lpp_cptr G, const double (&T)[NJ]) {
    double M = G[0] * T[0];
#pragma unroll
    for (int j = 1; j < NJ; ++j) M = __builtin_fma(T[j], G[j], M);
    return M;
}

// v'[b] = sum_a v[a] M[a][b]   (image: img[(b * rl + a) * n + j])
template <int NJ>
__device__ __forceinline__ void tt_ladder_left(pcx_lpp_cptr G, int rl, int rr, double x, const double *vin, double *vout) {
    double T[NJ];
    tt_lpp_basis<NJ, false>(x, T);
    for (int b = 0; b < rr; ++b) {
        double s = 0.0;
        for (int a = 0; a < rl; ++a, G += NJ) s = __builtin_fma(vin[a * PCX_LPP_WG], tt_ladder_fold<NJ>(G, T), s);
        vout[b * PCX_LPP_WG] = s;
    }
}

// R'[a] = sum_b M[a][b] R[b]
template <int NJ>
__device__ __forceinline__ void tt_ladder_right(pcx_lpp_cptr G, int rl, int rr, double x, const double *rin, double *rout) {
    double T[NJ];
    tt_lpp_basis<NJ, false>(x, T);
    for (int a = 0; a < rl; ++a) {
        double s = 0.0;
        for (int b = 0; b < rr; ++b) s = __builtin_fma(tt_ladder_fold<NJ>(G + (b * rl + a) * NJ, T), rin[b * PCX_LPP_WG], s);
        rout[a * PCX_LPP_WG] = s;
    }
}

// c_i = sum_b sum_a (L[a] R[b]) G[a][i][b], then the row's m values (y == NULL: a lane past the batch, no store)
template <int NJ>
__device__ __forceinline__ void tt_ladder_core(pcx_lpp_cptr G, int rl, int rr, const double *L, const double *R, double lo,
                                               double sc, const double *xs, int m, double *y) {
    double c[NJ];
#pragma unroll
    for (int i = 0; i < NJ; ++i) c[i] = 0.0;
    for (int b = 0; b < rr; ++b) {
        const double rb = R[b * PCX_LPP_WG];
        for (int a = 0; a < rl; ++a, G += NJ) {
            const double w = L[a * PCX_LPP_WG] * rb;
#pragma unroll
            for (int i = 0; i < NJ; ++i) c[i] = __builtin_fma(w, G[i], c[i]);
        }
    }
    for (int xi = 0; xi < m; ++xi) {
        double T[NJ];
        tt_lpp_basis<NJ, false>(__builtin_fma(xs[xi] - lo, sc, -1.0), T);
        double s = c[0] * T[0];
#pragma unroll
        for (int i = 1; i < NJ; ++i) s = __builtin_fma(c[i], T[i], s);
        if (y) y[xi] = s;
    }
}

// One wave per workgroup, one row per lane; dynamic LDS = 3 * max rank * 64 * 8 bytes: the right chain alternates
// between two lane-private columns, the left chain between the one it leaves free and a third.  Lanes past N work on
// row N - 1 and store nothing.
__global__ void __launch_bounds__(PCX_LPP_WG)
k_tt_ladder_lpp(const TTLppDim *__restrict__ tab, TTLadder lp, const double *__restrict__ img,
                const double *__restrict__ fixed, long fstride, const double *__restrict__ xs, long xstride,
                double *__restrict__ out, long N) {
    extern __shared__ double lds_lad[];
    typedef const TTLppDim __attribute__((address_space(4))) *tab_cptr;
    const tab_cptr ct = (tab_cptr)(unsigned long long)tab;
    const pcx_lpp_cptr cimg = (pcx_lpp_cptr)(unsigned long long)img;
    const long p = (long)blockIdx.x * PCX_LPP_WG + threadIdx.x;
    const long pc = p < N ? p : N - 1;
    const double *row = fixed + pc * fstride;
    const size_t col = (size_t)lp.rmax * PCX_LPP_WG;
    double *rin = lds_lad + threadIdx.x, *rout = rin + col, *lout = rout + col;
    rin[0] = 1.0;
    for (int k = lp.d - 1; k > lp.p; --k) {
        const double x = __builtin_fma(row[lp.fcol[k]] - ct[k].lo, ct[k].scale, -1.0);
        const pcx_lpp_cptr G = cimg + ct[k].off;
        const int rl = ct[k].rl, rr = ct[k].rr;
        tt_lpp_for_nodes(ct[k].n, [&](auto nj) { tt_ladder_right<decltype(nj)::value>(G, rl, rr, x, rin, rout); });
        double *t = rin; rin = rout; rout = t;
    }
    double *lin = rout;
    lin[0] = 1.0;
    for (int k = 0; k < lp.p; ++k) {
        const double x = __builtin_fma(row[lp.fcol[k]] - ct[k].lo, ct[k].scale, -1.0);
        const pcx_lpp_cptr G = cimg + ct[k].off;
        const int rl = ct[k].rl, rr = ct[k].rr;
        tt_lpp_for_nodes(ct[k].n, [&](auto nj) { tt_ladder_left<decltype(nj)::value>(G, rl, rr, x, lin, lout); });
        double *t = lin; lin = lout; lout = t;
    }
    {
        const int k = lp.p;
        const pcx_lpp_cptr G = cimg + ct[k].off;
        const int rl = ct[k].rl, rr = ct[k].rr;
        const double lo = ct[k].lo, sc = ct[k].scale;
        const double *xr = xs + pc * xstride;
        double *y = p < N ? out + p * lp.m : nullptr;
        tt_lpp_for_nodes(ct[k].n, [&](auto nj) { tt_ladder_core<decltype(nj)::value>(G, rl, rr, lin, rin, lo, sc, xr, lp.m, y); });
    }
}

// Every other model (rank > 16 or n > 16): one wave per row on the plain cores G_k[a][j][b] (tt_wave_kernels.h).
// Per wave in LDS: three rank vectors (the chains, as above), the basis q and the coefficients c
// (3 rmax + 2 nmax doubles).  Lane 0 forms a dimension's basis; the lanes share the right rank (left chain), the left
// rank (right chain), the coefficients and at last the m values.
__global__ void __launch_bounds__(256)
k_tt_ladder_generic(TTWaveModel gi, TTLadder lp, const double *__restrict__ cores, const double *__restrict__ fixed,
                    long fstride, const double *__restrict__ xs, long xstride, double *__restrict__ out, long N) {
    extern __shared__ double lds_ladg[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    double *b0 = lds_ladg + (size_t)wave * (3 * lp.rmax + 2 * gi.nmax);
    double *q = b0 + 3 * lp.rmax;
    double *c = q + gi.nmax;
    for (long p = (long)blockIdx.x * 4 + wave; p < N; p += (long)gridDim.x * 4) {
        const double *row = fixed + p * fstride;
        double *rin = b0, *rout = b0 + lp.rmax, *lout = b0 + 2 * lp.rmax;
        if (lane == 0) rin[0] = 1.0;
        for (int k = lp.d - 1; k > lp.p; --k) {
            const int rl = gi.rank[k], rr = gi.rank[k + 1], n = gi.n[k];
            if (lane == 0) tt_wave_basis(__builtin_fma(row[lp.fcol[k]] - gi.lo[k], gi.scale[k], -1.0), n, q);
            const double *G = cores + gi.coff[k];
            for (int a = lane; a < rl; a += 64) {
                double s = 0.0;
                for (int j = 0; j < n; ++j) {
                    const double *gp = G + ((long)a * n + j) * rr;
                    double w = 0.0;
                    for (int b = 0; b < rr; ++b) w = __builtin_fma(gp[b], rin[b], w);
                    s = __builtin_fma(q[j], w, s);
                }
                rout[a] = s;
            }
            double *t = rin; rin = rout; rout = t;
        }
        double *lin = rout;
        if (lane == 0) lin[0] = 1.0;
        for (int k = 0; k < lp.p; ++k) {
            const int rl = gi.rank[k], rr = gi.rank[k + 1], n = gi.n[k];
            if (lane == 0) tt_wave_basis(__builtin_fma(row[lp.fcol[k]] - gi.lo[k], gi.scale[k], -1.0), n, q);
            tt_wave_left(cores + gi.coff[k], rl, n, rr, q, lin, lout, lane);
            double *t = lin; lin = lout; lout = t;
        }
        const int k = lp.p;
        const int rl = gi.rank[k], rr = gi.rank[k + 1], n = gi.n[k];
        const double *G = cores + gi.coff[k];
        for (int i = lane; i < n; i += 64) {
            double s = 0.0;
            for (int a = 0; a < rl; ++a) {
                const double *gp = G + ((long)a * n + i) * rr;
                double w = 0.0;
                for (int b = 0; b < rr; ++b) w = __builtin_fma(gp[b], rin[b], w);
                s = __builtin_fma(lin[a], w, s);
            }
            c[i] = s;
        }
        const double lo = gi.lo[k], sc = gi.scale[k];
        for (int xi = lane; xi < lp.m; xi += 64) {
            const double s = __builtin_fma(xs[p * xstride + xi] - lo, sc, -1.0);
            const double x2 = s + s;
            double tp = 1.0, tc = s, y = 0.0;
            for (int i = 0; i < n; ++i) {
                y = __builtin_fma(c[i], tp, y);
                const double tn = __builtin_fma(x2, tc, -tp);
                tp = tc;
                tc = tn;
            }
            out[p * lp.m + xi] = y;
        }
    }
}
