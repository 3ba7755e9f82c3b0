// tt_deriv_kernels.h -- analytic derivatives of a tensor train in Chebyshev coefficient space (gfx950).
//
// out[row * m + spec] = the partial derivative of the interpolant with the orders of `spec` (0, 1 or 2 per dimension)
// at the row's point (ChebyshevTT.eval_multi_batch(..., method="analytic")).  It is the evaluation chain
//     v <- v . (sum_j q_j G_k[:, j, :])
// with the differentiated basis in the differentiated dimensions -- the counterpart of tt_box_kernels.h, which puts the
// antiderivatives there.  For storage position k with order p:
//     q_j = sc^p . T_j^(p)(s),   s = fma(x - lo_k, sc, -1),   sc = 2 / (hi_k - lo_k)
// from the three-term recurrences, run together:
//     T_{j+1}   = 2 s T_j   - T_{j-1}
//     T'_{j+1}  = 2 s T'_j  - T'_{j-1}  + 2 T_j
//     T''_{j+1} = 2 s T''_j - T''_{j-1} + 4 T'_j
// No division, nothing singular at a node or at s = +-1 (T'_j(+-1) and T''_j(+-1) are integers and come out exact).
// T^(p)_j = 0 for j < p, so a spec with p >= n_k gives exactly 0.  p = 0 is the value basis (tt_lpp_basis), as in tt_box_basis'
// kept branch: a spec of zeros is the box kernel without an integrated dimension.  One chain per (row, spec): no stencil, no truncation error, any
// number of differentiated dimensions.
//
// Specs go on blockIdx.y; their orders travel by value (TTDerivPack: two bits per STORAGE position), so the branch on
// p is a scalar branch.  Two forms, as the box kernels: lane per row on the lane-per-point image (ranks <= 16,
// n <= 16) and wave per row on the plain cores for every other model.
#pragma once

#include "tt_lpp_kernels.h"
#include "tt_wave_kernels.h"

#define PCX_DERIV_PACK 64         // specs per launch

struct TTDerivPack {
    unsigned int ord[PCX_DERIV_PACK];     // bits 2k, 2k + 1: the order at storage position k (PCX_MAX_DIMS = 16 positions)
};

__device__ __forceinline__ int tt_deriv_order(unsigned int ord, int k) { return (int)((ord >> (2 * k)) & 3u); }

// the basis of one dimension in registers; o is wave-uniform
template <int NJ>
__device__ __forceinline__ void tt_deriv_basis(int o, double s, double sc, double (&q)[NJ]) {
#pragma clang fp contract(off)
    if (o == 0) return tt_lpp_basis<NJ>(s, q);
    const double x2 = s + s;
    if (o == 1) {
        q[0] = 0.0;
        if constexpr (NJ > 1) q[1] = sc;
        double tm = 1.0, tc = s;             // T_{j-1}, T_j
        double um = 0.0, uc = 1.0;           // T'_{j-1}, T'_j          (j = 1)
#pragma unroll
        for (int j = 2; j < NJ; ++j) {
            const double un = __builtin_fma(x2, uc, __builtin_fma(2.0, tc, -um));
            const double tn = __builtin_fma(x2, tc, -tm);
            q[j] = sc * un;
            tm = tc; tc = tn;
            um = uc; uc = un;
        }
        return;
    }
    const double sc2 = sc * sc;
    q[0] = 0.0;
    if constexpr (NJ > 1) q[1] = 0.0;
    double tm = 1.0, tc = s;
    double um = 0.0, uc = 1.0;
    double wm = 0.0, wc = 0.0;               // T''_{j-1}, T''_j        (j = 1)
#pragma unroll
    for (int j = 2; j < NJ; ++j) {
        const double wn = __builtin_fma(x2, wc, __builtin_fma(4.0, uc, -wm));
        const double un = __builtin_fma(x2, uc, __builtin_fma(2.0, tc, -um));
        const double tn = __builtin_fma(x2, tc, -tm);
        q[j] = sc2 * wn;
        tm = tc; tc = tn;
        um = uc; uc = un;
        wm = wc; wc = wn;
    }
}

template <int RCAP, int NJ>
__device__ __forceinline__ void tt_deriv_dim(int rl, pcx_lpp_cptr G, int rr, int o, double s, double sc, double *vl) {
    double q[NJ];
    tt_deriv_basis<NJ>(o, s, sc, q);
    tt_lpp_for_rank<RCAP>(rl, [&](auto r) { tt_lpp_contract<decltype(r)::value, NJ>(G, rr, q, vl); });
}

// One wave per workgroup, one row per lane, one spec per blockIdx.y (gridDim.y <= PCX_DERIV_PACK); dynamic LDS =
// max rank * 64 * 8 bytes.  RCAP and NJ as k_tt_box_lpp.  Lanes past N work on row N - 1 and store nothing.
// Spec blockIdx.y of this launch is column s0 + blockIdx.y of the N x m result.
template <int RCAP, int NJ>
__global__ void __launch_bounds__(PCX_LPP_WG, RCAP <= 8 ? PCX_LPP_MINB8 : (RCAP <= 12 ? PCX_LPP_MINB12 : 4))
k_tt_deriv_lpp(const TTLppDim *__restrict__ tab, int d, TTDerivPack pack, const double *__restrict__ img,
               const double *__restrict__ pts, double *__restrict__ out, long N, int m, int s0) {
    extern __shared__ double lds_deriv[];
    double *vl = lds_deriv + threadIdx.x;
    typedef const TTLppDim __attribute__((address_space(4))) *tab_cptr;
    const tab_cptr ct = (tab_cptr)(unsigned long long)tab;
    const pcx_lpp_cptr cimg = (pcx_lpp_cptr)(unsigned long long)img;
    const unsigned int ord = pack.ord[blockIdx.y];
    const long p = (long)blockIdx.x * PCX_LPP_WG + threadIdx.x;
    const long pc = p < N ? p : N - 1;
    const double *row = pts + pc * d;
    double xn = row[ct[0].col];
    vl[0] = 1.0;
    for (int k = 0; k < d; ++k) {
        const double sc = ct[k].scale;
        const double s = __builtin_fma(xn - ct[k].lo, sc, -1.0);
        if (k + 1 < d) xn = row[ct[k + 1].col];
        const pcx_lpp_cptr G = cimg + ct[k].off;
        const int rl = ct[k].rl, rr = ct[k].rr;
        const int o = tt_deriv_order(ord, k);
        if constexpr (NJ > 0) {
            tt_deriv_dim<RCAP, NJ>(rl, G, rr, o, s, sc, vl);
        } else {
            tt_lpp_for_nodes(ct[k].n, [&](auto nj) { tt_deriv_dim<RCAP, decltype(nj)::value>(rl, G, rr, o, s, sc, vl); });
        }
    }
    if (p < N) out[p * m + s0 + (long)blockIdx.y] = vl[0];
}

// Every other model (rank > 16 or n > 16): one wave per row (tt_wave_kernels.h), 2 rmax + nmax doubles of LDS per wave.
// col[k] = the user column read by storage position k.
struct TTDerivGeneric {
    TTWaveModel g;
    int col[PCX_MAX_DIMS];
};

__global__ void __launch_bounds__(256)
k_tt_deriv_generic(TTDerivGeneric gd, TTDerivPack pack, const double *__restrict__ cores, const double *__restrict__ pts,
                   double *__restrict__ out, long N, int m, int s0) {
#pragma clang fp contract(off)
    extern __shared__ double lds_derivg[];
    const TTWaveModel &gi = gd.g;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const unsigned int ord = pack.ord[blockIdx.y];
    double *va = lds_derivg + (size_t)wave * (2 * gi.rmax + gi.nmax);
    double *vb = va + gi.rmax;
    double *q = vb + gi.rmax;
    for (long p = (long)blockIdx.x * 4 + wave; p < N; p += (long)gridDim.x * 4) {
        const double *row = pts + p * gi.d;
        if (lane == 0) va[0] = 1.0;
        for (int k = 0; k < gi.d; ++k) {
            const int rl = gi.rank[k], rr = gi.rank[k + 1], n = gi.n[k];
            if (lane == 0) {
                const double sc = gi.scale[k];
                const double s = __builtin_fma(row[gd.col[k]] - gi.lo[k], sc, -1.0);
                const int o = tt_deriv_order(ord, k);
                if (o == 0) {
                    tt_wave_basis(s, n, q);
                } else {
                    const double x2 = s + s;
                    const double f = o == 1 ? sc : sc * sc;
                    double tm = 1.0, tc = s, um = 0.0, uc = 1.0, wm = 0.0, wc = 0.0;      // T, T', T'' at j - 1 and j; j = 1
                    q[0] = 0.0;
                    if (n > 1) q[1] = o == 1 ? sc : 0.0;
                    for (int j = 2; j < n; ++j) {
                        const double wn = __builtin_fma(x2, wc, __builtin_fma(4.0, uc, -wm));
                        const double un = __builtin_fma(x2, uc, __builtin_fma(2.0, tc, -um));
                        const double tn = __builtin_fma(x2, tc, -tm);
                        q[j] = f * (o == 1 ? un : wn);
                        tm = tc; tc = tn;
                        um = uc; uc = un;
                        wm = wc; wc = wn;
                    }
                }
            }
            tt_wave_left(cores + gi.coff[k], rl, n, rr, q, va, vb, lane);
            double *t = va; va = vb; vb = t;
        }
        if (lane == 0) out[p * m + s0 + (long)blockIdx.y] = va[0];
    }
}
