// tt_box_kernels.h -- batched box integrals of a tensor train in Chebyshev coefficient space (gfx950).
//
// out[r] = integral of the model over a box in the row's integrated dimensions, at the row's coordinates in the
// kept ones (ChebyshevTT.integrate_batch; the reference's integrate(dims, bounds).eval(point),
// tensor_train.py:1505-1702, one row at a time).  It is the evaluation chain
//     v <- v . (sum_j q_j G_k[:, j, :])
// with another basis vector in an integrated dimension:
//     kept:        q_j = T_j(s),  s = fma(x - lo_k, 2 / (hi_k - lo_k), -1)           (as k_tt_eval_lpp)
//     integrated:  q_j = (hi_k - lo_k) / 2 . (F_j(t_hi) - F_j(t_lo)),  t mapped like s,
//                  F_0 = t,  F_1 = t^2 / 2,  F_j = (T_{j+1} / (j + 1) - T_{j-1} / (j - 1)) / 2  for j >= 2
// (Trefethen, ATAP ch. 19, the antiderivatives of T_j).  Each F_j is formed by the same operations at both ends and
// q_j is their difference, so a row with lo == hi gives exactly 0.  Contraction of products into FMAs is switched
// off where q is formed (an FMA fused across the difference would break that) and written out where it is wanted.
//
// Row layout: for user dimensions 0 .. d-1 in order, one double (the coordinate) for a kept dimension, two (lo, hi)
// for an integrated one.  TTBoxCols gives, per STORAGE position, the row offset and the flag; it is a kernel argument,
// so both are wave-uniform and the branch on the flag is a scalar branch.
//
// Two forms: lane per row on the lane-per-point image of tt_lpp_kernels.h (ranks <= 16, n <= 16: core elements are
// scalar operands), and the wave-per-row form on the plain cores for every other model.
#pragma once

#include "tt_lpp_kernels.h"
#include "tt_wave_kernels.h"

struct TTBoxCols {
    int width;                    // doubles per row: d + (integrated dimensions)
    int off[PCX_MAX_DIMS];        // row offset of storage position k
    int integ[PCX_MAX_DIMS];      // 1: storage position k is integrated (off, off + 1 = lo, hi)
    double half[PCX_MAX_DIMS];    // (hi_k - lo_k) / 2
};

// the basis of one dimension in registers: ta == tb and T_j(ta) for a kept dimension
template <int NJ>
__device__ __forceinline__ void tt_box_basis(bool integ, double ta, double tb, double half, double (&q)[NJ]) {
#pragma clang fp contract(off)
    if (!integ) return tt_lpp_basis<NJ>(ta, q);
    q[0] = half * (tb - ta);
    if constexpr (NJ > 1) q[1] = half * (0.5 * (tb * tb) - 0.5 * (ta * ta));
    if constexpr (NJ > 2) {
        const double a2 = ta + ta, b2 = tb + tb;
        double am = ta, ac = __builtin_fma(a2, ta, -1.0);       // T_{j-1}, T_j at t_lo, j = 2
        double bm = tb, bc = __builtin_fma(b2, tb, -1.0);       // ... at t_hi
#pragma unroll
        for (int j = 2; j < NJ; ++j) {
            const double ap = __builtin_fma(a2, ac, -am), bp = __builtin_fma(b2, bc, -bm);       // T_{j+1}
            const double c1 = 1.0 / (j + 1), c2 = 1.0 / (j - 1);
            const double fa = 0.5 * (ap * c1 - am * c2), fb = 0.5 * (bp * c1 - bm * c2);
            q[j] = half * (fb - fa);
            am = ac; ac = ap;
            bm = bc; bc = bp;
        }
    }
}

template <int RCAP, int NJ>
__device__ __forceinline__ void tt_box_dim(int rl, pcx_lpp_cptr G, int rr, bool integ, double ta, double tb, double half,
                                           double *vl) {
    double q[NJ];
    tt_box_basis<NJ>(integ, ta, tb, half, q);
    tt_lpp_for_rank<RCAP>(rl, [&](auto r) { tt_lpp_contract<decltype(r)::value, NJ>(G, rr, q, vl); });
}

// One wave per workgroup, one row per lane; dynamic LDS = max rank * 64 * 8 bytes.  RCAP and NJ as k_tt_eval_lpp.
// Lanes past N work on row N - 1 and store nothing.  A kept dimension reads its coordinate twice (off + integ == off):
// the loads do not branch.
template <int RCAP, int NJ>
__global__ void __launch_bounds__(PCX_LPP_WG, RCAP <= 8 ? PCX_LPP_MINB8 : (RCAP <= 12 ? PCX_LPP_MINB12 : 4))
k_tt_box_lpp(const TTLppDim *__restrict__ tab, int d, TTBoxCols cols, const double *__restrict__ img,
             const double *__restrict__ rows, double *__restrict__ out, long N) {
    extern __shared__ double lds_box[];
    double *vl = lds_box + threadIdx.x;
    typedef const TTLppDim __attribute__((address_space(4))) *tab_cptr;
    const tab_cptr ct = (tab_cptr)(unsigned long long)tab;
    const pcx_lpp_cptr cimg = (pcx_lpp_cptr)(unsigned long long)img;
    const long p = (long)blockIdx.x * PCX_LPP_WG + threadIdx.x;
    const long pc = p < N ? p : N - 1;
    const double *row = rows + pc * cols.width;
    double an = row[cols.off[0]], bn = row[cols.off[0] + cols.integ[0]];
    vl[0] = 1.0;
    for (int k = 0; k < d; ++k) {
        const double lo = ct[k].lo, sc = ct[k].scale;
        const double ta = __builtin_fma(an - lo, sc, -1.0), tb = __builtin_fma(bn - lo, sc, -1.0);
        if (k + 1 < d) {
            an = row[cols.off[k + 1]];
            bn = row[cols.off[k + 1] + cols.integ[k + 1]];
        }
        const pcx_lpp_cptr G = cimg + ct[k].off;
        const int rl = ct[k].rl, rr = ct[k].rr;
        const bool integ = cols.integ[k] != 0;
        const double half = cols.half[k];
        if constexpr (NJ > 0) {
            tt_box_dim<RCAP, NJ>(rl, G, rr, integ, ta, tb, half, vl);
        } else {
            tt_lpp_for_nodes(ct[k].n, [&](auto nj) { tt_box_dim<RCAP, decltype(nj)::value>(rl, G, rr, integ, ta, tb, half, vl); });
        }
    }
    if (p < N) out[p] = vl[0];
}

// Every other model (rank > 16 or n > 16): one wave per row (tt_wave_kernels.h), 2 rmax + nmax doubles of LDS per wave.
// rinv[j] = 1 / j (nmax + 2 doubles, the handle's) spares lane 0 the divisions of the antiderivatives.
__global__ void __launch_bounds__(256)
k_tt_box_generic(TTWaveModel gi, TTBoxCols cols, const double *__restrict__ cores, const double *__restrict__ rinv,
                 const double *__restrict__ rows, double *__restrict__ out, long N) {
#pragma clang fp contract(off)
    extern __shared__ double lds_boxg[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    double *va = lds_boxg + (size_t)wave * (2 * gi.rmax + gi.nmax);
    double *vb = va + gi.rmax;
    double *q = vb + gi.rmax;
    for (long p = (long)blockIdx.x * 4 + wave; p < N; p += (long)gridDim.x * 4) {
        const double *row = rows + p * cols.width;
        if (lane == 0) va[0] = 1.0;
        for (int k = 0; k < gi.d; ++k) {
            const int rl = gi.rank[k], rr = gi.rank[k + 1], n = gi.n[k];
            if (lane == 0) {
                const double ta = __builtin_fma(row[cols.off[k]] - gi.lo[k], gi.scale[k], -1.0);
                if (!cols.integ[k]) {
                    tt_wave_basis(ta, n, q);
                } else {
                    const double tb = __builtin_fma(row[cols.off[k] + 1] - gi.lo[k], gi.scale[k], -1.0);
                    const double half = cols.half[k];
                    q[0] = half * (tb - ta);
                    if (n > 1) q[1] = half * (0.5 * (tb * tb) - 0.5 * (ta * ta));
                    const double a2 = ta + ta, b2 = tb + tb;
                    double am = ta, ac = __builtin_fma(a2, ta, -1.0);
                    double bm = tb, bc = __builtin_fma(b2, tb, -1.0);
                    for (int j = 2; j < n; ++j) {
                        const double ap = __builtin_fma(a2, ac, -am), bp = __builtin_fma(b2, bc, -bm);
                        const double c1 = rinv[j + 1], c2 = rinv[j - 1];          // 1 / (j + 1), 1 / (j - 1): a table, no division per row
                        const double fa = 0.5 * (ap * c1 - am * c2), fb = 0.5 * (bp * c1 - bm * c2);
                        q[j] = half * (fb - fa);
                        am = ac; ac = ap;
                        bm = bc; bc = bp;
                    }
                }
            }
            tt_wave_left(cores + gi.coff[k], rl, n, rr, q, va, vb, lane);
            double *t = va; va = vb; vb = t;
        }
        if (lane == 0) out[p] = va[0];
    }
}
