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
    if (!integ) {
        const double x2 = ta + ta;
        q[0] = 1.0;
        asm volatile("" : "+v"(q[0]));       // as tt_lpp_body: one v_mul_f64 per core element of j = 0
        if constexpr (NJ > 1) q[1] = ta;
#pragma unroll
        for (int j = 2; j < NJ; ++j) q[j] = __builtin_fma(x2, q[j - 1], -q[j - 2]);
        return;
    }
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

// tt_lpp_body with the basis handed in
template <int RL, int NJ>
__device__ __forceinline__ void tt_box_body(pcx_lpp_cptr G, int rr, const double (&q)[NJ], double *vl) {
    double v[RL];
#pragma unroll
    for (int a = 0; a < RL; ++a) v[a] = vl[a * PCX_LPP_WG];
    for (int b = 0; b < rr; ++b, G += RL * NJ) {
        double M[RL];
#pragma unroll
        for (int a = 0; a < RL; ++a) M[a] = G[a * NJ] * q[0];
#pragma unroll
        for (int j = 1; j < NJ; ++j)
#pragma unroll
            for (int a = 0; a < RL; ++a) M[a] = __builtin_fma(q[j], G[a * NJ + j], M[a]);
        double s;
        if constexpr (RL < 4) {
            s = v[0] * M[0];
#pragma unroll
            for (int a = 1; a < RL; ++a) s = __builtin_fma(v[a], M[a], s);
        } else {
            double s0 = v[0] * M[0], s1 = v[1] * M[1];
#pragma unroll
            for (int a = 2; a < RL; a += 2) {
                s0 = __builtin_fma(v[a], M[a], s0);
                if (a + 1 < RL) s1 = __builtin_fma(v[a + 1], M[a + 1], s1);
            }
            s = s0 + s1;
        }
        vl[b * PCX_LPP_WG] = s;
    }
}

#define PCX_BOX_RANK_CASES_8(NJ)                                                                          \
    case 1: tt_box_body<1, NJ>(G, rr, q, vl); break; case 2: tt_box_body<2, NJ>(G, rr, q, vl); break;     \
    case 3: tt_box_body<3, NJ>(G, rr, q, vl); break; case 4: tt_box_body<4, NJ>(G, rr, q, vl); break;     \
    case 5: tt_box_body<5, NJ>(G, rr, q, vl); break; case 6: tt_box_body<6, NJ>(G, rr, q, vl); break;     \
    case 7: tt_box_body<7, NJ>(G, rr, q, vl); break; case 8: tt_box_body<8, NJ>(G, rr, q, vl); break;
#define PCX_BOX_RANK_CASES_12(NJ)                                                                         \
    case 9: tt_box_body<9, NJ>(G, rr, q, vl); break; case 10: tt_box_body<10, NJ>(G, rr, q, vl); break;   \
    case 11: tt_box_body<11, NJ>(G, rr, q, vl); break; case 12: tt_box_body<12, NJ>(G, rr, q, vl); break;
#define PCX_BOX_RANK_CASES_16(NJ)                                                                         \
    case 13: tt_box_body<13, NJ>(G, rr, q, vl); break; case 14: tt_box_body<14, NJ>(G, rr, q, vl); break; \
    case 15: tt_box_body<15, NJ>(G, rr, q, vl); break; case 16: tt_box_body<16, NJ>(G, rr, q, vl); break;

template <int RCAP, int NJ>
__device__ __forceinline__ void tt_box_dim(int rl, pcx_lpp_cptr G, int rr, bool integ, double ta, double tb, double half,
                                           double *vl) {
    double q[NJ];
    tt_box_basis<NJ>(integ, ta, tb, half, q);
    switch (rl) {
        PCX_BOX_RANK_CASES_8(NJ)
        default:
            if constexpr (RCAP > 12) {
                switch (rl) { PCX_BOX_RANK_CASES_12(NJ) PCX_BOX_RANK_CASES_16(NJ) default: break; }
            } else if constexpr (RCAP > 8) {
                switch (rl) { PCX_BOX_RANK_CASES_12(NJ) default: break; }
            }
            break;
    }
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
            switch (ct[k].n) {
            case 1: tt_box_dim<RCAP, 1>(rl, G, rr, integ, ta, tb, half, vl); break;
            case 2: tt_box_dim<RCAP, 2>(rl, G, rr, integ, ta, tb, half, vl); break;
            case 3: tt_box_dim<RCAP, 3>(rl, G, rr, integ, ta, tb, half, vl); break;
            case 4: tt_box_dim<RCAP, 4>(rl, G, rr, integ, ta, tb, half, vl); break;
            case 5: tt_box_dim<RCAP, 5>(rl, G, rr, integ, ta, tb, half, vl); break;
            case 6: tt_box_dim<RCAP, 6>(rl, G, rr, integ, ta, tb, half, vl); break;
            case 7: tt_box_dim<RCAP, 7>(rl, G, rr, integ, ta, tb, half, vl); break;
            case 8: tt_box_dim<RCAP, 8>(rl, G, rr, integ, ta, tb, half, vl); break;
            case 9: tt_box_dim<RCAP, 9>(rl, G, rr, integ, ta, tb, half, vl); break;
            case 10: tt_box_dim<RCAP, 10>(rl, G, rr, integ, ta, tb, half, vl); break;
            case 11: tt_box_dim<RCAP, 11>(rl, G, rr, integ, ta, tb, half, vl); break;
            case 12: tt_box_dim<RCAP, 12>(rl, G, rr, integ, ta, tb, half, vl); break;
            case 13: tt_box_dim<RCAP, 13>(rl, G, rr, integ, ta, tb, half, vl); break;
            case 14: tt_box_dim<RCAP, 14>(rl, G, rr, integ, ta, tb, half, vl); break;
            case 15: tt_box_dim<RCAP, 15>(rl, G, rr, integ, ta, tb, half, vl); break;
            case 16: tt_box_dim<RCAP, 16>(rl, G, rr, integ, ta, tb, half, vl); break;
            default: break;
            }
        }
    }
    if (p < N) out[p] = vl[0];
}

// Every other model (rank > 16 or n > 16): one wave per row as k_tt_eval_generic -- lanes over the right rank, the
// cores in their natural (r, n, r') layout, v and q in the wave's LDS slice (2 rmax + nmax doubles per wave).  Lane 0
// forms the basis as in k_tt_eval_generic; rinv[j] = 1 / j (nmax + 2 doubles, the handle's) spares it the divisions.
struct TTBoxGeneric {
    int d;
    int rank[PCX_MAX_DIMS + 1];
    int n[PCX_MAX_DIMS];
    long coff[PCX_MAX_DIMS];
    double lo[PCX_MAX_DIMS];
    double scale[PCX_MAX_DIMS];
    int rmax, nmax;
};

__global__ void __launch_bounds__(256)
k_tt_box_generic(TTBoxGeneric gi, TTBoxCols cols, const double *__restrict__ cores, const double *__restrict__ rinv,
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
                if (!cols.integ[k]) {             // T_0 .. T_{n-1} by the forward recurrence
                    double tp = 1.0, tc = ta;
                    const double x2 = ta + ta;
                    for (int j = 0; j < n; ++j) {
                        q[j] = tp;
                        const double tn = __builtin_fma(x2, tc, -tp);
                        tp = tc;
                        tc = tn;
                    }
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
            // wave-private LDS: operations of one wave execute in order, no barrier needed
            const double *G = cores + gi.coff[k];
            for (int b = lane; b < rr; b += 64) {
                double s = 0.0;
                for (int a = 0; a < rl; ++a) {
                    const double *ga = G + ((long)a * n) * rr + b;
                    double w = 0.0;
                    for (int j = 0; j < n; ++j) w = __builtin_fma(q[j], ga[(long)j * rr], w);
                    s = __builtin_fma(va[a], w, s);
                }
                vb[b] = s;
            }
            double *t = va; va = vb; vb = t;
        }
        if (lane == 0) out[p] = va[0];
    }
}
