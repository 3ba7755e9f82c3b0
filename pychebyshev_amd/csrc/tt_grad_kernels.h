// tt_grad_kernels.h -- value, gradient and Hessian diagonal of a tensor train in one forward-backward pass per row
// (ChebyshevTT.gradient_batch; gfx950).
//
// With M_k = sum_j T_j(s_k) G_k[:, j, :] the folded core of storage position k,
//     L_k = M_0 ... M_{k-1}   (1 x r_k),      R_k = M_k ... M_{d-1}   (r_k x 1),      f = L_d = R_0
// and, with M1_k / M2_k the same fold over sc_k T'_j(s_k) / sc_k^2 T''_j(s_k) (tt_deriv_kernels.h: s = fma(x - lo, sc, -1),
// sc = 2 / (hi - lo), the three recurrences run together),
//     df/dx_k   = L_k . M1_k . R_{k+1}
//     d2f/dx_k2 = L_k . M2_k . R_{k+1}
// A right sweep k = d-1 .. 1 forms and KEEPS every R_k; a left sweep k = 0 .. d-1 folds each core with the three bases
// from one set of core loads and takes, per right index b,
//     L'[b] = sum_a L[a] M[a][b],    g_k += (sum_a L[a] M1[a][b]) R_{k+1}[b],    h_k += (sum_a L[a] M2[a][b]) R_{k+1}[b]
// -- one chain's worth of folds for the right sweep and two for the left, three with the diagonal: 3 and 4 chains'
// worth whatever d is (measured: 3.7 and 4.7 evaluations), where one chain per (row, spec) (k_tt_deriv_lpp) takes
// d + 1 and 2 d + 1.  T'_0 = 0 and T''_0 = T''_1 = 0 are left out of
// the folds, so a dimension with one node has gradient and second derivative exactly 0.0, one with two nodes second
// derivative exactly 0.0.  R_d = 1 is not stored.
//
// out is row-major N x C, C = 1 + d (value, gradient) or 1 + 2 d (SECOND: then the diagonal); column 1 + u and
// 1 + d + u belong to the USER's dimension u = col[k] (dim_order applied here, on the device).
//
//   k_tt_grad_lpp       one row per lane on the lane-per-point image (ranks <= 16, n <= 16); core elements are scalar
//                       operands, the left rank and the node count compile-time, b runs at run time (tt_lpp_kernels.h)
//   k_tt_grad_generic   one row per wave on the plain cores, for every other model (tt_wave_kernels.h)
//
// No atomics; every sum in a fixed order (b ascending, the two partial sums of tt_lpp_contract over a from RL = 4): a
// row's bits depend on nothing but the row.
//
// k_tt_hess_lpp and k_tt_hess_generic (tt_hess_kernels.h) restate both sweeps with vectors carried beside L and must give
// these kernels' bits: an edit to a sweep, a basis or a left body here has its twin there.  Restated, not shared: moved
// into functions both pairs call, each changed the generated code of the kernels it touched.  What the
// launchers of the two pairs share is at the end of this file.
#pragma once

#include <atomic>

#include "tt_lpp_kernels.h"
#include "tt_wave_kernels.h"

// T_j, sc T'_j and (SECOND) sc^2 T''_j, j < NJ, in one pass: tt_deriv_basis' arithmetic for every order at once
template <int NJ, bool SECOND>
__device__ __forceinline__ void tt_grad_basis(double s, double sc, double (&q0)[NJ], double (&q1)[NJ], double (&q2)[NJ]) {
#pragma clang fp contract(off)
    const double x2 = s + s;
    const double sc2 = sc * sc;
    q0[0] = 1.0;
    asm volatile("" : "+v"(q0[0]));          // T_0 in a register: M = g * T_0 is one v_mul_f64 (PCX_LPP_BASIS)
    q1[0] = 0.0;
    q2[0] = 0.0;
    if constexpr (NJ > 1) {
        q0[1] = s;
        q1[1] = sc;
        q2[1] = 0.0;
    }
    double tm = 1.0, tc = s;                 // T_{j-1}, T_j          (j = 1)
    double um = 0.0, uc = 1.0;               // T'_{j-1}, T'_j
    double wm = 0.0, wc = 0.0;               // T''_{j-1}, T''_j
#pragma unroll
    for (int j = 2; j < NJ; ++j) {
        const double un = __builtin_fma(x2, uc, __builtin_fma(2.0, tc, -um));
        const double tn = __builtin_fma(x2, tc, -tm);
        q0[j] = tn;
        q1[j] = sc * un;
        if constexpr (SECOND) {
            const double wn = __builtin_fma(x2, wc, __builtin_fma(4.0, uc, -wm));
            q2[j] = sc2 * wn;
            wm = wc; wc = wn;
        }
        tm = tc; tc = tn;
        um = uc; uc = un;
    }
}

// sum_a v[a] M[a]: tt_lpp_contract's rule (one chain below RL = 4, two partial sums from there on)
template <int RL>
__device__ __forceinline__ double tt_grad_dot(const double (&v)[RL], const double (&M)[RL]) {
    if constexpr (RL < 4) {
        double s = v[0] * M[0];
#pragma unroll
        for (int a = 1; a < RL; ++a) s = __builtin_fma(v[a], M[a], s);
        return s;
    } else {
        double s0 = v[0] * M[0], s1 = v[1] * M[1];
#pragma unroll
        for (int a = 2; a < RL; a += 2) {
            s0 = __builtin_fma(v[a], M[a], s0);
            if (a + 1 < RL) s1 = __builtin_fma(v[a + 1], M[a + 1], s1);
        }
        return s0 + s1;
    }
}

// Right sweep, one left rank: R'[a] = sum_b M[a][b] R[b], a < RL, accumulated in registers over b ascending.  The
// image (b * RL + a) * NJ + j is walked front to back.  rin == nullptr: the last position, R = (1.0), rr = 1.
template <int RL, int NJ>
__device__ __forceinline__ void tt_grad_right(pcx_lpp_cptr G, int rr, const double (&q)[NJ], const double *rin, double *rout) {
    double acc[RL];
#pragma unroll
    for (int a = 0; a < RL; ++a) acc[a] = 0.0;
    for (int b = 0; b < rr; ++b, G += RL * NJ) {
        const double rb = rin ? rin[b * PCX_LPP_WG] : 1.0;
        double M[RL];
#pragma unroll
        for (int a = 0; a < RL; ++a) M[a] = G[a * NJ] * q[0];
#pragma unroll
        for (int j = 1; j < NJ; ++j)
#pragma unroll
            for (int a = 0; a < RL; ++a) M[a] = __builtin_fma(q[j], G[a * NJ + j], M[a]);
#pragma unroll
        for (int a = 0; a < RL; ++a) acc[a] = __builtin_fma(M[a], rb, acc[a]);
    }
#pragma unroll
    for (int a = 0; a < RL; ++a) rout[a * PCX_LPP_WG] = acc[a];
}

// Left sweep, one left rank: L (in place, through the lane's LDS column), *g and *h of this position.  One scalar load
// of G[a][j][b] feeds the two or three folds.  rnext == nullptr: the last position, R_{k+1} = (1.0).
template <int RL, int NJ, bool SECOND>
__device__ __forceinline__ void tt_grad_left(pcx_lpp_cptr G, int rr, const double (&q0)[NJ], const double (&q1)[NJ],
                                             const double (&q2)[NJ], double *L, const double *rnext, double *g, double *h) {
    double v[RL];
#pragma unroll
    for (int a = 0; a < RL; ++a) v[a] = L[a * PCX_LPP_WG];       // position 0 reads the 1.0 the kernel put there
    double gs = 0.0, hs = 0.0;
    for (int b = 0; b < rr; ++b, G += RL * NJ) {
        double M[RL], M1[RL], M2[RL];
#pragma unroll
        for (int a = 0; a < RL; ++a) M[a] = G[a * NJ] * q0[0];
#pragma unroll
        for (int j = 1; j < NJ; ++j)
#pragma unroll
            for (int a = 0; a < RL; ++a) {
                const double c = G[a * NJ + j];
                M[a] = __builtin_fma(q0[j], c, M[a]);
                M1[a] = j == 1 ? c * q1[j] : __builtin_fma(q1[j], c, M1[a]);         // T'_0 = 0
                if constexpr (SECOND) {
                    if (j == 2) M2[a] = c * q2[j];                                   // T''_0 = T''_1 = 0
                    if (j > 2) M2[a] = __builtin_fma(q2[j], c, M2[a]);
                }
            }
        const double s = tt_grad_dot<RL>(v, M);
        if constexpr (NJ > 1) {
            const double rb = rnext ? rnext[b * PCX_LPP_WG] : 1.0;
            gs = __builtin_fma(tt_grad_dot<RL>(v, M1), rb, gs);
            if constexpr (SECOND && NJ > 2) hs = __builtin_fma(tt_grad_dot<RL>(v, M2), rb, hs);
        }
        L[b * PCX_LPP_WG] = s;
    }
    *g = gs;
    *h = hs;
}

template <int RCAP, int NJ>
__device__ __forceinline__ void tt_grad_right_dim(int rl, pcx_lpp_cptr G, int rr, double s, const double *rin, double *rout) {
    double q[NJ];
    tt_lpp_basis<NJ>(s, q);
    tt_lpp_for_rank<RCAP>(rl, [&](auto r) { tt_grad_right<decltype(r)::value, NJ>(G, rr, q, rin, rout); });
}

template <int RCAP, int NJ, bool SECOND>
__device__ __forceinline__ void tt_grad_left_dim(int rl, pcx_lpp_cptr G, int rr, double s, double sc, double *L,
                                                 const double *rnext, double *g, double *h) {
    double q0[NJ], q1[NJ], q2[NJ];
    tt_grad_basis<NJ, SECOND>(s, sc, q0, q1, q2);
    tt_lpp_for_rank<RCAP>(rl, [&](auto r) { tt_grad_left<decltype(r)::value, NJ, SECOND>(G, rr, q0, q1, q2, L, rnext, g, h); });
}

// r_1 + ... + r_{d-1}: what R_1 .. R_{d-1} take, in columns (lane-per-row) or doubles (wave-per-row)
static inline int tt_grad_rank_sum(const int *ranks, int d) {
    int sum = 0;
    for (int k = 1; k < d; ++k) sum += ranks[k];
    return sum;
}
// columns (of 64 doubles) of dynamic LDS k_tt_grad_lpp takes: R_1 .. R_{d-1}, then L
static inline size_t tt_grad_lpp_columns(const int *ranks, int d, int rmax) { return (size_t)tt_grad_rank_sum(ranks, d) + rmax; }

// One wave per workgroup, one row per lane; dynamic LDS = (r_1 + ... + r_{d-1} + max rank) * 64 * 8 bytes: R_k in its
// own lane-private columns at r_1 + ... + r_{k-1}, L in the last max-rank columns.  RCAP and NJ as k_tt_deriv_lpp.  The
// LDS, not the registers, bounds the waves of a CU here (config 3: 19 KiB a wave, 8 waves; config 5: 80 KiB, 2), so
// the register budget is the one that residency leaves free, not k_tt_deriv_lpp's 8 / 6 / 4 waves per SIMD: the left
// body holds three folds and three bases (up to 230 VGPRs as compiled) and is expected to spill under those -- expected,
// not compiled or timed; models with little LDS are untimed under these bounds.  Lanes past N work on row N - 1 and
// store nothing.
template <int RCAP, int NJ, bool SECOND>
__global__ void __launch_bounds__(PCX_LPP_WG, RCAP <= 12 ? 2 : 1)
k_tt_grad_lpp(const TTLppDim *__restrict__ tab, int d, const double *__restrict__ img, const double *__restrict__ pts,
              double *__restrict__ out, long N) {
    extern __shared__ double lds_grad[];
    double *base = lds_grad + threadIdx.x;
    typedef const TTLppDim __attribute__((address_space(4))) *tab_cptr;
    const tab_cptr ct = (tab_cptr)(unsigned long long)tab;
    const pcx_lpp_cptr cimg = (pcx_lpp_cptr)(unsigned long long)img;
    const long p = (long)blockIdx.x * PCX_LPP_WG + threadIdx.x;
    const long pc = p < N ? p : N - 1;
    const double *row = pts + pc * d;
    int tot = 0;                                      // columns of R_1 .. R_{d-1}
    for (int k = 1; k < d; ++k) tot += ct[k].rl;
    int off = tot;                                    // column of R_{k+1}
    for (int k = d - 1; k >= 1; --k) {
        const int rl = ct[k].rl, rr = ct[k].rr;
        const double *rin = k + 1 < d ? base + (size_t)off * PCX_LPP_WG : nullptr;
        off -= rl;
        double *rout = base + (size_t)off * PCX_LPP_WG;
        const double s = __builtin_fma(row[ct[k].col] - ct[k].lo, ct[k].scale, -1.0);
        const pcx_lpp_cptr G = cimg + ct[k].off;
        if constexpr (NJ > 0) {
            tt_grad_right_dim<RCAP, NJ>(rl, G, rr, s, rin, rout);
        } else {
            tt_lpp_for_nodes(ct[k].n, [&](auto nj) { tt_grad_right_dim<RCAP, decltype(nj)::value>(rl, G, rr, s, rin, rout); });
        }
    }
    double *L = base + (size_t)tot * PCX_LPP_WG;
    double *o = out + p * (long)(1 + (SECOND ? 2 : 1) * d);
    L[0] = 1.0;
    off = 0;                                          // column of R_{k+1}: R_1 first
    for (int k = 0; k < d; ++k) {
        const int rl = ct[k].rl, rr = ct[k].rr;
        const double *rnext = k + 1 < d ? base + (size_t)off * PCX_LPP_WG : nullptr;
        off += rr;
        const double sc = ct[k].scale;
        const double s = __builtin_fma(row[ct[k].col] - ct[k].lo, sc, -1.0);
        const pcx_lpp_cptr G = cimg + ct[k].off;
        double g = 0.0, h = 0.0;
        if constexpr (NJ > 0) {
            tt_grad_left_dim<RCAP, NJ, SECOND>(rl, G, rr, s, sc, L, rnext, &g, &h);
        } else {
            tt_lpp_for_nodes(ct[k].n, [&](auto nj) {
                tt_grad_left_dim<RCAP, decltype(nj)::value, SECOND>(rl, G, rr, s, sc, L, rnext, &g, &h);
            });
        }
        if (p < N) {
            o[1 + ct[k].col] = g;
            if constexpr (SECOND) o[1 + d + ct[k].col] = h;
        }
    }
    if (p < N) o[0] = L[0];
}

// Every other model (rank > 16 or n > 16): one wave per row on the plain cores G_k[a][j][b].  Per wave in LDS:
// R_1 .. R_{d-1} (r_1 + ... + r_{d-1} doubles), two rank vectors L alternates between, the three bases
// (tt_grad_generic_doubles: sum of ranks + 2 rmax + 3 nmax; without SECOND the third basis is neither formed nor read).
// Lane 0 forms the bases; the lanes share the left rank on the right sweep
// and the right rank b on the left sweep (tt_wave_left), where each lane adds its own b's terms of g and h in ascending
// order and a butterfly over the wave adds the lanes: a fixed order.  col[k] = the user column of storage position k.
struct TTGradGeneric {
    TTWaveModel g;
    int col[PCX_MAX_DIMS];
    int rsum;                     // r_1 + ... + r_{d-1}
};

// doubles of LDS per wave: the launcher's size and the kernel's slice stride
__host__ __device__ static inline size_t tt_grad_generic_doubles(int rsum, int rmax, int nmax) {
    return (size_t)rsum + 2 * rmax + 3 * nmax;
}

__device__ __forceinline__ double tt_grad_wave_sum(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

template <bool SECOND>
__global__ void __launch_bounds__(256)
k_tt_grad_generic(TTGradGeneric gd, const double *__restrict__ cores, const double *__restrict__ pts,
                  double *__restrict__ out, long N) {
#pragma clang fp contract(off)
    extern __shared__ double lds_gradg[];
    const TTWaveModel &gi = gd.g;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int d = gi.d;
    const long C = 1 + (SECOND ? 2 : 1) * d;
    double *R = lds_gradg + (size_t)wave * tt_grad_generic_doubles(gd.rsum, gi.rmax, gi.nmax);
    double *l0 = R + gd.rsum;
    double *q0 = l0 + 2 * gi.rmax;
    double *q1 = q0 + gi.nmax;
    double *q2 = q1 + gi.nmax;
    for (long p = (long)blockIdx.x * 4 + wave; p < N; p += (long)gridDim.x * 4) {
        const double *row = pts + p * d;
        double *o = out + p * C;
        int off = gd.rsum;                            // offset of R_{k+1}
        for (int k = d - 1; k >= 1; --k) {
            const int rl = gi.rank[k], rr = gi.rank[k + 1], n = gi.n[k];
            if (lane == 0) tt_wave_basis(__builtin_fma(row[gd.col[k]] - gi.lo[k], gi.scale[k], -1.0), n, q0);
            const double *rin = R + off;              // not read at k = d - 1
            const bool last = k + 1 == d;
            off -= rl;
            double *rout = R + off;
            const double *G = cores + gi.coff[k];
            for (int a = lane; a < rl; a += 64) {
                double s = 0.0;
                for (int j = 0; j < n; ++j) {
                    const double *gp = G + ((long)a * n + j) * rr;
                    double w = 0.0;
                    if (last) w = gp[0];
                    else
                        for (int b = 0; b < rr; ++b) w = __builtin_fma(gp[b], rin[b], w);
                    s = __builtin_fma(q0[j], w, s);
                }
                rout[a] = s;
            }
        }
        double *lin = l0, *lout = l0 + gi.rmax;
        if (lane == 0) lin[0] = 1.0;
        off = 0;
        for (int k = 0; k < d; ++k) {
            const int rl = gi.rank[k], rr = gi.rank[k + 1], n = gi.n[k];
            if (lane == 0) {
                const double sc = gi.scale[k];
                const double s = __builtin_fma(row[gd.col[k]] - gi.lo[k], sc, -1.0);
                const double x2 = s + s, sc2 = sc * sc;
                double tm = 1.0, tc = s, um = 0.0, uc = 1.0, wm = 0.0, wc = 0.0;      // T, T', T'' at j - 1 and j; j = 1
                q0[0] = 1.0; q1[0] = 0.0;
                if (n > 1) { q0[1] = s; q1[1] = sc; }
                if (SECOND) { q2[0] = 0.0; if (n > 1) q2[1] = 0.0; }
                for (int j = 2; j < n; ++j) {
                    const double un = __builtin_fma(x2, uc, __builtin_fma(2.0, tc, -um));
                    const double tn = __builtin_fma(x2, tc, -tm);
                    q0[j] = tn; q1[j] = sc * un;
                    if (SECOND) {
                        const double wn = __builtin_fma(x2, wc, __builtin_fma(4.0, uc, -wm));
                        q2[j] = sc2 * wn;
                        wm = wc; wc = wn;
                    }
                    tm = tc; tc = tn;
                    um = uc; uc = un;
                }
            }
            const double *rnext = R + off;            // not read at k = d - 1
            const bool last = k + 1 == d;
            off += rr;
            const double *G = cores + gi.coff[k];
            double gs = 0.0, hs = 0.0;
            for (int b = lane; b < rr; b += 64) {
                double s0 = 0.0, s1 = 0.0, s2 = 0.0;
                for (int a = 0; a < rl; ++a) {
                    const double *ga = G + ((long)a * n) * rr + b;
                    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
                    for (int j = 0; j < n; ++j) {
                        const double c = ga[(long)j * rr];
                        w0 = __builtin_fma(q0[j], c, w0);
                        if (j >= 1) w1 = __builtin_fma(q1[j], c, w1);
                        if (SECOND && j >= 2) w2 = __builtin_fma(q2[j], c, w2);
                    }
                    const double va = lin[a];
                    s0 = __builtin_fma(va, w0, s0);
                    s1 = __builtin_fma(va, w1, s1);
                    if (SECOND) s2 = __builtin_fma(va, w2, s2);
                }
                lout[b] = s0;
                const double rb = last ? 1.0 : rnext[b];
                gs = __builtin_fma(s1, rb, gs);
                if (SECOND) hs = __builtin_fma(s2, rb, hs);
            }
            gs = tt_grad_wave_sum(gs);
            if (SECOND) hs = tt_grad_wave_sum(hs);
            if (lane == 0) {
                o[1 + gd.col[k]] = gs;
                if (SECOND) o[1 + d + gd.col[k]] = hs;
            }
            double *t = lin; lin = lout; lout = t;
        }
        if (lane == 0) o[0] = lin[0];
    }
}

// ---- host side: what the launchers of pcx_tt_grad.hip and pcx_tt_hess.hip share -----------------------------------------
#define PCX_TT_GRAD_LDS_MAX (160 * 1024)      // the LDS of a workgroup
// the handle's form (true: lane-per-row), or an error for a handle that holds neither image nor cores
static inline int tt_grad_form(const TTBoxView &v, bool *lane) {
    *lane = v.d_lpp_img != nullptr;
    if (!*lane && !v.d_cores) return fail(PCX_ERR_UNSUPPORTED, "the handle holds neither a lane-per-point image nor plain cores");
    return PCX_OK;
}
// A lane-per-row launch above the 64 KiB default of dynamic LDS: lifted to a workgroup's 160 KiB once per instantiation and
// device (`lifted`: the instantiation's own static; bit = device, an index past 63 lifts at every launch), so that it stays
// off the launch path of a batch in pieces
static inline int tt_grad_lift_lds(const void *kernel, std::atomic<unsigned long long> &lifted, int device, size_t lds) {
    const unsigned long long bit = device < 64 ? 1ull << device : 0;
    if (lds > 64 * 1024 && !(lifted.load(std::memory_order_relaxed) & bit)) {
        HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PCX_TT_GRAD_LDS_MAX));
        lifted.fetch_or(bit, std::memory_order_relaxed);
    }
    return PCX_OK;
}
// workgroups of a lane-per-row launch (64 rows each), refused beyond one launch's grid
static inline int tt_grad_lpp_blocks(long N, long *blocks) {
    *blocks = (N + PCX_LPP_WG - 1) / PCX_LPP_WG;
    return *blocks > 0x7fffffffL ? fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch") : PCX_OK;
}
// workgroups of a wave-per-row launch (four rows each; from 2048 on the waves stride over the rows)
static inline long tt_grad_generic_blocks(long N) { return std::min<long>((N + 3) / 4, 256L * 8); }
static inline TTGradGeneric tt_grad_generic_model(const TTBoxView &v) {
    TTGradGeneric gd{};
    gd.g = tt_wave_model(v);
    for (int k = 0; k < gd.g.d; ++k) gd.col[k] = v.plan->dims.col[k];
    gd.rsum = tt_grad_rank_sum(v.plan->ranks, gd.g.d);
    return gd;
}
