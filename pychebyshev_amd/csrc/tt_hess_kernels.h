// tt_hess_kernels.h -- value, gradient and the FULL Hessian of a tensor train from one right sweep and one blocked left
// sweep per row (ChebyshevTT.hessian_batch; gfx950).
//
// With M_k, M1_k, M2_k, L_k and R_k as in tt_grad_kernels.h, for storage positions i < k
//     d2f/dx_i dx_k = (L_i M1_i) . M_{i+1} ... M_{k-1} . M1_k . R_{k+1}
// D_i = L_i M1_i is the vector the gradient's left sweep already forms per right index b (g_i = D_i . R_{i+1}).  It is
// kept and CARRIED to the right beside L: at every later position k, per right index b, from the folds M[a], M1[a] the
// left sweep holds in registers anyway,
//     D_i'[b] = sum_a D_i[a] M[a][b],        H_ik += (sum_a D_i[a] M1[a][b]) R_{k+1}[b]
// -- two vector-matrix products (r_l r_r FMAs each) per carried vector and position, where a fold is n r_l r_r per basis.
//
// Blocked carrying: a carried vector needs the vector it is read from and the one it is written to (the b loop reads all
// of D_i for every b), and one accumulator.  Not every model has room for d - 1 of them, so the kernels take a run-time
// block size B: pass 0 is the gradient's left sweep (three folds: value, gradient, diagonal) with sources 0 .. B - 1
// carried; pass p >= 1 carries sources p B .. p B + B - 1: the plain one-basis fold up to its first source, the folds M
// and M1 from there.  Every H_ik is the same sequence of operations whatever B is -- L by tt_lpp_contract's rule in every
// pass, D_i and its products by tt_grad_dot's, b ascending -- so a row's bits depend neither on B nor on the batch.
// No atomics.  T'_0 and T''_0 = T''_1 are left out of the folds: the Hessian row and column of a one-node dimension
// and the diagonal entry of a two-node dimension are exactly 0.0.
//
// out is row-major N x C, C = 1 + d + d^2: the value, the gradient at 1 + u, d2f/dx_u dx_v at 1 + d + u d + v for the
// USER's dimensions u = col[i], v = col[k] (dim_order applied here); both triangles are written from the one number.
//
//   k_tt_hess_lpp       one row per lane on the lane-per-point image (ranks <= 16, n <= 16)
//   k_tt_hess_generic   one row per wave on the plain cores, for every other model
#pragma once

#include "tt_grad_kernels.h"

// ---- the LDS rule: the one statement of it (launchers, pcx_tt_hess_info) ----------------------------------------------
// lane-per-row: columns of 64 doubles -- the gradient's (R_1 .. R_{d-1}, L), and per carried vector two vectors of max
// rank columns (read / written, alternating by position) and one column for its accumulator.
static inline size_t tt_hess_lpp_columns(const int *ranks, int d, int rmax, int B) {
    return tt_grad_lpp_columns(ranks, d, rmax) + (size_t)B * (2 * (size_t)rmax + 1);
}
// wave-per-row: doubles per wave -- the gradient's (R, two L, three bases), and per carried vector two rank vectors, the
// 64 lanes' two products of the current b and the 64 lanes' partial sums of H_ik.
static inline size_t tt_hess_generic_doubles(int rsum, int rmax, int nmax, int B) {
    return tt_grad_generic_doubles(rsum, rmax, nmax) + (size_t)B * (2 * (size_t)rmax + 3 * 64);
}
// dynamic LDS bytes of a workgroup at block size B (lane: one wave of 64 rows; else four waves of one row each)
static inline size_t tt_hess_lds_bytes(const TTPlan &p, bool lane, int B) {
    const int d = p.dims.d;
    if (lane) return tt_hess_lpp_columns(p.ranks, d, p.rmax, B) * PCX_LPP_WG * sizeof(double);
    return 4 * tt_hess_generic_doubles(tt_grad_rank_sum(p.ranks, d), p.rmax, p.nmax, B) * sizeof(double);
}
static inline int tt_hess_block_limit(int d) { return d - 1 > 1 ? d - 1 : 1; }
// the largest B <= max(1, d - 1) whose launch fits a workgroup's LDS; 0: not even B = 1 does
static inline int tt_hess_block_max(const TTPlan &p, bool lane) {
    int B = tt_hess_block_limit(p.dims.d);
    while (B > 0 && tt_hess_lds_bytes(p, lane, B) > PCX_TT_GRAD_LDS_MAX) --B;
    return B;
}
// Folds of one row at block size B, in units of one core folded with one basis: the right sweep (d - 1), pass 0 (three
// per position), a pass from source `first` on (one per position before it, two from there).
static inline int tt_hess_fold_units(int d, int B) {
    int units = (d - 1) + 3 * d;
    for (int first = B; first < d - 1; first += B) units += first + 2 * (d - first);
    return units;
}
// Waves a CU holds by LDS: workgroups of `bytes` each, allocated in granules of 1280 bytes (160 KiB / 128), times the
// waves of a workgroup.  The granule is what the table of DESIGN 3.20 shows: 53.0 KiB a wave runs as two waves a CU do,
// not as three (3 x 53.0 = 159 KiB, but 3 x 43 granules are 161.25 KiB).
static inline int tt_hess_resident_waves(size_t bytes, bool lane) {
    const size_t alloc = (bytes + 1279) / 1280 * 1280;
    return (int)(PCX_TT_GRAD_LDS_MAX / alloc) * (lane ? 1 : 4);
}
// The planner's B: passes against LDS residency.  A later pass repeats the L fold up to its first source and the two
// folds from there; a larger B keeps fewer waves on a CU, and these kernels are bound by the latency a second wave hides,
// so their rate goes with the resident waves (up to the two per SIMD the gradient's config-3 launch has; beyond: not
// measured).  Cost of a row = (fold units + one unit per carried (vector, position) pair, d (d - 1) / 2 whatever B is)
// / resident waves; the B of least cost, the larger B on a tie.  Set from the measurement of every admissible B on the
// config-3 and config-5 shapes (tools/tt_hess_probe.py, profiles/tt_hess_probe.txt): it orders all eight as measured and
// takes B = 2 and B = 4 there.  The wave-per-row form takes the same rule with the CU's 32 waves as the cap: untimed.
static inline int tt_hess_block_plan(const TTPlan &p, bool lane) {
    const int d = p.dims.d, fits = tt_hess_block_max(p, lane), cap = lane ? 8 : 32;
    int best = fits;
    double best_cost = 0.0;
    for (int B = fits; B >= 1; --B) {
        const int waves = std::min(cap, tt_hess_resident_waves(tt_hess_lds_bytes(p, lane, B), lane));
        const double cost = (double)(tt_hess_fold_units(d, B) + d * (d - 1) / 2) / waves;
        if (B == fits || cost < best_cost) { best = B; best_cost = cost; }
    }
    return best;
}

// ---- lane-per-row ---------------------------------------------------------------------------------------------------
// tt_grad_left (SECOND) extended by the carried vectors.  FIRST: pass 0 (M2, *g and *h as the gradient takes them); else
// the folds M and M1 only.  nc carried vectors, vector c read from din + c * cstride and written to dout + c * cstride,
// its accumulator acc[c * PCX_LPP_WG] (left holding H_ck); src: this position is a source, the nc-th of the pass, and
// stores sum_a L[a] M1[a][b] as its D[b].
template <int RL, int NJ, bool FIRST>
__device__ __forceinline__ void tt_hess_left(pcx_lpp_cptr G, int rr, const double (&q0)[NJ], const double (&q1)[NJ],
                                             const double (&q2)[NJ], double *L, const double *rnext, double *g, double *h,
                                             int nc, bool src, const double *din, double *dout, double *acc, size_t cstride) {
    double v[RL];
#pragma unroll
    for (int a = 0; a < RL; ++a) v[a] = L[a * PCX_LPP_WG];
    double gs = 0.0, hs = 0.0;
    for (int c = 0; c < nc; ++c) acc[c * PCX_LPP_WG] = 0.0;
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
                if constexpr (FIRST) {
                    if (j == 2) M2[a] = c * q2[j];                                   // T''_0 = T''_1 = 0
                    if (j > 2) M2[a] = __builtin_fma(q2[j], c, M2[a]);
                }
            }
        const double s = tt_grad_dot<RL>(v, M);
        const double rb = rnext ? rnext[b * PCX_LPP_WG] : 1.0;
        double own = 0.0;                                                            // D[b] of this position: 0 for one node
        if constexpr (NJ > 1) {
            own = tt_grad_dot<RL>(v, M1);
            if constexpr (FIRST) {
                gs = __builtin_fma(own, rb, gs);
                if constexpr (NJ > 2) hs = __builtin_fma(tt_grad_dot<RL>(v, M2), rb, hs);
            }
        }
        L[b * PCX_LPP_WG] = s;
        if (src) dout[nc * cstride + b * PCX_LPP_WG] = own;
        for (int c = 0; c < nc; ++c) {
            const double *dc = din + c * cstride;
            double dv[RL];
#pragma unroll
            for (int a = 0; a < RL; ++a) dv[a] = dc[a * PCX_LPP_WG];
            dout[c * cstride + b * PCX_LPP_WG] = tt_grad_dot<RL>(dv, M);
            if constexpr (NJ > 1) acc[c * PCX_LPP_WG] = __builtin_fma(tt_grad_dot<RL>(dv, M1), rb, acc[c * PCX_LPP_WG]);
        }
    }
    *g = gs;
    *h = hs;
}

template <int RCAP, int NJ, bool FIRST>
__device__ __forceinline__ void tt_hess_left_dim(int rl, pcx_lpp_cptr G, int rr, double s, double sc, double *L,
                                                 const double *rnext, double *g, double *h, int nc, bool src,
                                                 const double *din, double *dout, double *acc, size_t cstride) {
    double q0[NJ], q1[NJ], q2[NJ];
    tt_grad_basis<NJ, FIRST>(s, sc, q0, q1, q2);
    tt_lpp_for_rank<RCAP>(rl, [&](auto r) {
        tt_hess_left<decltype(r)::value, NJ, FIRST>(G, rr, q0, q1, q2, L, rnext, g, h, nc, src, din, dout, acc, cstride);
    });
}

// One wave per workgroup, one row per lane; dynamic LDS = tt_hess_lpp_columns(...) * 64 * 8 bytes: R_k and L where
// k_tt_grad_lpp has them, behind L carried vector c's two vectors at (2 c + parity) * rmax columns (the parity of the
// position: read at k & 1, written at the other), behind those the B accumulator columns.  1 <= B, and the launcher has
// checked the LDS rule.  Launch bounds as k_tt_grad_lpp: the LDS bounds the waves of a CU.  Lanes past N work on row
// N - 1 and store nothing.
template <int RCAP, int NJ>
__global__ void __launch_bounds__(PCX_LPP_WG, RCAP <= 12 ? 2 : 1)
k_tt_hess_lpp(const TTLppDim *__restrict__ tab, int d, int rmax, int B, const double *__restrict__ img,
              const double *__restrict__ pts, double *__restrict__ out, long N) {
    extern __shared__ double lds_hess[];
    double *base = lds_hess + threadIdx.x;
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
    double *D = L + (size_t)rmax * PCX_LPP_WG;
    const size_t vec = (size_t)rmax * PCX_LPP_WG, cstride = 2 * vec;
    double *acc = D + (size_t)B * cstride;
    const long C = 1 + (long)d + (long)d * d;
    double *o = out + p * C;
    double *H = o + 1 + d;
    for (int first = 0; first == 0 || first < d - 1; first += B) {        // sources first .. last - 1
        const int last = first + B < d - 1 ? first + B : d - 1;
        L[0] = 1.0;
        off = 0;                                      // column of R_{k+1}: R_1 first
        for (int k = 0; k < d; ++k) {
            const int rl = ct[k].rl, rr = ct[k].rr;
            const double *rnext = k + 1 < d ? base + (size_t)off * PCX_LPP_WG : nullptr;
            off += rr;
            const double sc = ct[k].scale;
            const double s = __builtin_fma(row[ct[k].col] - ct[k].lo, sc, -1.0);
            const pcx_lpp_cptr G = cimg + ct[k].off;
            if (k < first) {                          // a later pass on its way to its first source: L alone
                if constexpr (NJ > 0) {
                    tt_lpp_dim<RCAP, NJ>(rl, G, rr, s, L);
                } else {
                    tt_lpp_for_nodes(ct[k].n, [&](auto nj) { tt_lpp_dim<RCAP, decltype(nj)::value>(rl, G, rr, s, L); });
                }
                continue;
            }
            const int nc = (k < last ? k : last) - first;
            const bool src = k < last;
            const double *din = D + (size_t)(k & 1) * vec;
            double *dout = D + (size_t)((k + 1) & 1) * vec;
            double g = 0.0, h = 0.0;
            if (first == 0) {
                if constexpr (NJ > 0) {
                    tt_hess_left_dim<RCAP, NJ, true>(rl, G, rr, s, sc, L, rnext, &g, &h, nc, src, din, dout, acc, cstride);
                } else {
                    tt_lpp_for_nodes(ct[k].n, [&](auto nj) {
                        tt_hess_left_dim<RCAP, decltype(nj)::value, true>(rl, G, rr, s, sc, L, rnext, &g, &h, nc, src, din, dout, acc, cstride);
                    });
                }
            } else {
                if constexpr (NJ > 0) {
                    tt_hess_left_dim<RCAP, NJ, false>(rl, G, rr, s, sc, L, rnext, &g, &h, nc, src, din, dout, acc, cstride);
                } else {
                    tt_lpp_for_nodes(ct[k].n, [&](auto nj) {
                        tt_hess_left_dim<RCAP, decltype(nj)::value, false>(rl, G, rr, s, sc, L, rnext, &g, &h, nc, src, din, dout, acc, cstride);
                    });
                }
            }
            if (p < N) {
                const int v = ct[k].col;
                if (first == 0) {
                    o[1 + v] = g;
                    H[v * d + v] = h;
                }
                for (int c = 0; c < nc; ++c) {
                    const int u = ct[first + c].col;
                    const double x = acc[c * PCX_LPP_WG];
                    H[u * d + v] = x;
                    H[v * d + u] = x;
                }
            }
        }
        if (first == 0 && p < N) o[0] = L[0];
    }
}

// ---- wave-per-row -----------------------------------------------------------------------------------------------------
// k_tt_grad_generic<true> with the carried vectors in the wave's LDS slice (tt_hess_generic_doubles): behind the three
// bases, carried vector c's two rank vectors at (2 c + parity) * rmax, then per c the 64 lanes' products with M and M1
// of the lane's current b (2 x 64) and the 64 lanes' partial sums of H_ck (64).  The lanes share b; lane 0 forms the
// bases; a lane adds its own b's terms in ascending order and tt_grad_wave_sum adds the lanes: a fixed order.
struct TTHessGeneric {
    TTGradGeneric gd;
    int B;
};

__global__ void __launch_bounds__(256)
k_tt_hess_generic(TTHessGeneric hd, const double *__restrict__ cores, const double *__restrict__ pts,
                  double *__restrict__ out, long N) {
#pragma clang fp contract(off)
    extern __shared__ double lds_hessg[];
    const TTWaveModel &gi = hd.gd.g;
    const int *col = hd.gd.col;
    const int rsum = hd.gd.rsum, B = hd.B;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int d = gi.d;
    const long C = 1 + (long)d + (long)d * d;
    const size_t vec = (size_t)gi.rmax;
    // tt_hess_generic_doubles, restated: calling it here changed this kernel's code (tt_grad_kernels.h)
    double *R = lds_hessg + (size_t)wave * ((size_t)rsum + 2 * vec + 3 * gi.nmax + (size_t)B * (2 * vec + 3 * 64));
    double *l0 = R + rsum;
    double *q0 = l0 + 2 * vec;
    double *q1 = q0 + gi.nmax;
    double *q2 = q1 + gi.nmax;
    double *D = q2 + gi.nmax;                         // carried c: D + (2 c + parity) * vec
    double *P = D + (size_t)B * 2 * vec + lane;       // carried c: P[c * 192], P[c * 192 + 64] the products, P[c * 192 + 128] the sum
    for (long p = (long)blockIdx.x * 4 + wave; p < N; p += (long)gridDim.x * 4) {
        const double *row = pts + p * d;
        double *o = out + p * C;
        double *H = o + 1 + d;
        int off = rsum;                               // offset of R_{k+1}
        for (int k = d - 1; k >= 1; --k) {
            const int rl = gi.rank[k], rr = gi.rank[k + 1], n = gi.n[k];
            if (lane == 0) tt_wave_basis(__builtin_fma(row[col[k]] - gi.lo[k], gi.scale[k], -1.0), n, q0);
            const double *rin = R + off;              // not read at k = d - 1
            const bool lastk = k + 1 == d;
            off -= rl;
            double *rout = R + off;
            const double *G = cores + gi.coff[k];
            for (int a = lane; a < rl; a += 64) {
                double s = 0.0;
                for (int j = 0; j < n; ++j) {
                    const double *gp = G + ((long)a * n + j) * rr;
                    double w = 0.0;
                    if (lastk) w = gp[0];
                    else
                        for (int b = 0; b < rr; ++b) w = __builtin_fma(gp[b], rin[b], w);
                    s = __builtin_fma(q0[j], w, s);
                }
                rout[a] = s;
            }
        }
        for (int first = 0; first == 0 || first < d - 1; first += B) {
            const int last = first + B < d - 1 ? first + B : d - 1;
            const bool pass0 = first == 0;
            double *lin = l0, *lout = l0 + vec;
            if (lane == 0) lin[0] = 1.0;
            off = 0;
            for (int k = 0; k < d; ++k) {
                const int rl = gi.rank[k], rr = gi.rank[k + 1], n = gi.n[k];
                const double *G = cores + gi.coff[k];
                if (k < first) {                      // a later pass on its way to its first source: L alone
                    if (lane == 0) tt_wave_basis(__builtin_fma(row[col[k]] - gi.lo[k], gi.scale[k], -1.0), n, q0);
                    tt_wave_left(G, rl, n, rr, q0, lin, lout, lane);
                    off += rr;
                    double *t = lin; lin = lout; lout = t;
                    continue;
                }
                if (lane == 0) {
                    const double sc = gi.scale[k];
                    const double s = __builtin_fma(row[col[k]] - gi.lo[k], sc, -1.0);
                    const double x2 = s + s, sc2 = sc * sc;
                    double tm = 1.0, tc = s, um = 0.0, uc = 1.0, wm = 0.0, wc = 0.0;      // T, T', T'' at j - 1 and j; j = 1
                    q0[0] = 1.0; q1[0] = 0.0; q2[0] = 0.0;
                    if (n > 1) { q0[1] = s; q1[1] = sc; q2[1] = 0.0; }
                    for (int j = 2; j < n; ++j) {
                        const double un = __builtin_fma(x2, uc, __builtin_fma(2.0, tc, -um));
                        const double tn = __builtin_fma(x2, tc, -tm);
                        const double wn = __builtin_fma(x2, wc, __builtin_fma(4.0, uc, -wm));
                        q0[j] = tn; q1[j] = sc * un; q2[j] = sc2 * wn;
                        wm = wc; wc = wn;
                        tm = tc; tc = tn;
                        um = uc; uc = un;
                    }
                }
                const int nc = (k < last ? k : last) - first;
                const bool src = k < last;
                const double *din = D + (size_t)(k & 1) * vec;
                double *dout = D + (size_t)((k + 1) & 1) * vec;
                const double *rnext = R + off;        // not read at k = d - 1
                const bool lastk = k + 1 == d;
                off += rr;
                double gs = 0.0, hs = 0.0;
                for (int c = 0; c < nc; ++c) P[c * 192 + 128] = 0.0;
                for (int b = lane; b < rr; b += 64) {
                    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
                    for (int c = 0; c < nc; ++c) { P[c * 192] = 0.0; P[c * 192 + 64] = 0.0; }
                    for (int a = 0; a < rl; ++a) {
                        const double *ga = G + ((long)a * n) * rr + b;
                        double w0 = 0.0, w1 = 0.0, w2 = 0.0;
                        for (int j = 0; j < n; ++j) {
                            const double c = ga[(long)j * rr];
                            w0 = __builtin_fma(q0[j], c, w0);
                            if (j >= 1) w1 = __builtin_fma(q1[j], c, w1);
                            if (pass0 && j >= 2) w2 = __builtin_fma(q2[j], c, w2);
                        }
                        const double va = lin[a];
                        s0 = __builtin_fma(va, w0, s0);
                        s1 = __builtin_fma(va, w1, s1);
                        s2 = __builtin_fma(va, w2, s2);
                        for (int c = 0; c < nc; ++c) {
                            const double da = din[(size_t)c * 2 * vec + a];
                            P[c * 192] = __builtin_fma(da, w0, P[c * 192]);
                            P[c * 192 + 64] = __builtin_fma(da, w1, P[c * 192 + 64]);
                        }
                    }
                    lout[b] = s0;
                    const double rb = lastk ? 1.0 : rnext[b];
                    gs = __builtin_fma(s1, rb, gs);
                    hs = __builtin_fma(s2, rb, hs);
                    if (src) dout[(size_t)nc * 2 * vec + b] = s1;
                    for (int c = 0; c < nc; ++c) {
                        dout[(size_t)c * 2 * vec + b] = P[c * 192];
                        P[c * 192 + 128] = __builtin_fma(P[c * 192 + 64], rb, P[c * 192 + 128]);
                    }
                }
                const int v = col[k];
                if (pass0) {
                    gs = tt_grad_wave_sum(gs);
                    hs = tt_grad_wave_sum(hs);
                    if (lane == 0) {
                        o[1 + v] = gs;
                        H[v * d + v] = hs;
                    }
                }
                for (int c = 0; c < nc; ++c) {
                    const double x = tt_grad_wave_sum(P[c * 192 + 128]);
                    if (lane == 0) {
                        const int u = col[first + c];
                        H[u * d + v] = x;
                        H[v * d + u] = x;
                    }
                }
                double *t = lin; lin = lout; lout = t;
            }
            if (pass0 && lane == 0) o[0] = lin[0];
        }
    }
}
