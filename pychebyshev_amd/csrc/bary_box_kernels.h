// bary_box_kernels.h -- batched box integrals of the full-tensor barycentric interpolant (gfx950).
//
// out[r] = integral of the interpolant over a box in the row's integrated dimensions, at the row's coordinates in the
// kept ones (ChebyshevApproximation.integrate_batch; the reference computes one with integrate(dims, bounds) and then
// vectorized_eval(point), barycentric.py:2160-2275).  It is the contraction of an evaluation,
//     out[r] = sum_i T[i] prod_k v_k[i_k],
// with another weight vector in an integrated dimension:
//     kept:        v = normalised barycentric weights at the coordinate            (bary_weights_1d, unchanged)
//     integrated:  v[j] = (b - a) / 2 . sum_{q < n} Q_n[j][q] mu_q,  mu_q = F_q(t_hi) - F_q(t_lo),
//                  t = fma(x - a, 2 / (b - a), -1),  F_0 = t,  F_1 = t^2 / 2,
//                  F_q = (T_{q+1} / (q + 1) - T_{q-1} / (q - 1)) / 2  for q >= 2      (Trefethen, ATAP ch. 19)
//                  Q_n[j][0] = 1 / n,  Q_n[j][q] = (2 / n) cos(pi q (2 (n - 1 - j) + 1) / (2 n))
// Q_n . mu are the sub-interval Fejer-1 weights at the ascending type-I nodes (reference _calculus.py:76-128, a DCT-III
// of the moments); Q_n depends on n only and is built on the host in double (pcx_bary_box.hip).  Every F_q is formed by
// the same operations at both ends and mu_q is their difference, with contraction into FMAs switched off, so a row with
// lo == hi has mu == 0 and its result is exactly 0 (as tt_box_basis).
//
// Row layout: for dimensions 0 .. d-1 in order, one double (the coordinate) for a kept dimension, two (lo, hi) for an
// integrated one.  BaryBoxCols gives the row offset, the flag and the domain per dimension; it is a kernel argument, so
// lanes that work on the same dimension take the same side of the branch.  Both prologues spread the lanes of a wave
// over dimensions as well as rows (k = ph + i PH, k = sub + i LPP): the branch is uniform within such a group of
// lanes, and a wave whose groups hold a kept and an integrated dimension at the same step runs the two routines one
// after the other.
//
//   k_bary_box_rows   any shape, on the plain tensor: k_bary_rows with the box prologue
//   k_bary_box_mfma   v_mfma_f64_16x16x4_f64 on the row-code fragment image of k_bary_mfma (same image, seed columns,
//                     row / k codes), with the k-step count, R and wide / narrow as runtime values
#pragma once

#include "bary_kernels.h"

struct BaryBoxCols {
    int width;                    // doubles per row: d + (integrated dimensions)
    int off[PCX_MAX_DIMS];        // row offset of dimension k
    int integ[PCX_MAX_DIMS];      // 1: dimension k is integrated (off, off + 1 = lo, hi)
    int qoff[PCX_MAX_DIMS];       // offset of Q_{n_k} in the handle's quadrature table
    double a[PCX_MAX_DIMS];       // lower end of the domain
    double scale[PCX_MAX_DIMS];   // 2 / (b - a)
    double half[PCX_MAX_DIMS];    // (b - a) / 2
};

// Sub-interval quadrature weights of one dimension for one row, written to dst[j * stride] like bary_weights_1d.
// q ascending; per q the moment from three live T values per end, then one pass over the column: dst[j] += Q[j][q] mu_q
// (a fixed order: q = 0 starts the sum, every later q is one FMA onto it, the factor (b - a) / 2 comes last).
// rinv[i] = 1 / i (a table of the handle: no division per row).
__device__ __forceinline__ void box_weights_1d(double lo, double hi, double a, double scale, double half,
                                               const double *__restrict__ Q, const double *__restrict__ rinv, int n,
                                               double *dst, int stride) {
#pragma clang fp contract(off)
    const double ta = __builtin_fma(lo - a, scale, -1.0), tb = __builtin_fma(hi - a, scale, -1.0);
    {
        const double mu = tb - ta;
        for (int j = 0; j < n; ++j) dst[j * stride] = Q[(long)j * n] * mu;
    }
    if (n > 1) {
        const double mu = 0.5 * (tb * tb) - 0.5 * (ta * ta);
        for (int j = 0; j < n; ++j) dst[j * stride] = __builtin_fma(Q[(long)j * n + 1], mu, dst[j * stride]);
    }
    const double a2 = ta + ta, b2 = tb + tb;
    double am = ta, ac = __builtin_fma(a2, ta, -1.0);       // T_{q-1}, T_q at t_lo, q = 2
    double bm = tb, bc = __builtin_fma(b2, tb, -1.0);       // ... at t_hi
    for (int q = 2; q < n; ++q) {
        const double ap = __builtin_fma(a2, ac, -am), bp = __builtin_fma(b2, bc, -bm);       // T_{q+1}
        const double c1 = rinv[q + 1], c2 = rinv[q - 1];
        const double fa = 0.5 * (ap * c1 - am * c2), fb = 0.5 * (bp * c1 - bm * c2);
        const double mu = fb - fa;
        for (int j = 0; j < n; ++j) dst[j * stride] = __builtin_fma(Q[(long)j * n + q], mu, dst[j * stride]);
        am = ac; ac = ap;
        bm = bc; bc = bp;
    }
    for (int j = 0; j < n; ++j) dst[j * stride] *= half;
}

// the weight vector of dimension k for one row (valid == false: a lane past the batch; it works on a node / an empty box)
__device__ __forceinline__ void box_dim_weights(const BaryDims &dims, const BaryBoxCols &cols, int k, bool valid,
                                                const double *__restrict__ row, const double *__restrict__ nodes,
                                                const double *__restrict__ wts, const double *__restrict__ boxq,
                                                const double *__restrict__ rinv, double *dst, int stride) {
    const double *nd = nodes + dims.off[k];
    if (cols.integ[k]) {
        const double lo = valid ? row[cols.off[k]] : cols.a[k];
        const double hi = valid ? row[cols.off[k] + 1] : cols.a[k];
        box_weights_1d(lo, hi, cols.a[k], cols.scale[k], cols.half[k], boxq + cols.qoff[k], rinv, dims.n[k], dst, stride);
    } else {
        const double x = valid ? row[cols.off[k]] : nd[0];
        bary_weights_1d(x, nd, wts + dims.off[k], dims.n[k], dst, stride);
    }
}

// ---------------------------------------------------------------------------------
// Any shape: k_bary_rows (same row walk, same shuffle reduction) with the box prologue.
// dynamic LDS = (256 / LPP) * sum_n * 8 bytes.
// ---------------------------------------------------------------------------------
static __global__ void __launch_bounds__(256)
k_bary_box_rows(BaryDims dims, BaryBoxCols cols, int LPP, const double *__restrict__ nodes,
                const double *__restrict__ wts, const double *__restrict__ boxq, const double *__restrict__ rinv,
                const double *__restrict__ T, const double *__restrict__ rows, double *__restrict__ out, long N) {
    extern __shared__ double lds[];
    const int ppw = 256 / LPP;                 // rows per workgroup
    const int pl = threadIdx.x / LPP;          // local row
    const int sub = threadIdx.x % LPP;         // lane within the row's group
    const long pidx = (long)blockIdx.x * ppw + pl;
    const bool valid = pidx < N;
    const double *rp = rows + (valid ? pidx : 0) * cols.width;
    double *bw = lds + (size_t)pl * dims.sum_n;
    for (int k = sub; k < dims.d; k += LPP)
        box_dim_weights(dims, cols, k, valid, rp, nodes, wts, boxq, rinv, bw + dims.off[k], 1);
    __syncthreads();
    const int d = dims.d;
    const int K = dims.n[d - 1];
    long M = 1;
    for (int k = 0; k < d - 1; ++k) M *= dims.n[k];
    const double *bl = bw + dims.off[d - 1];
    double acc = 0.0;
    for (long m = sub; m < M; m += LPP) {
        double w = 1.0;
        long rem = m;
        for (int k = d - 2; k >= 0; --k) {
            int nk = dims.n[k];
            int i = (int)(rem % nk);
            rem /= nk;
            w *= bw[dims.off[k] + i];
        }
        const double *trow = T + m * K;
        double s = 0.0;
        for (int j = 0; j < K; ++j) s = __builtin_fma(trow[j], bl[j], s);
        acc = __builtin_fma(s, w, acc);
    }
    for (int o = LPP >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (sub == 0 && valid) out[pidx] = acc;
}

// ---------------------------------------------------------------------------------
// MFMA form on the row-code image.  One wave owns PW = 16 NT rows of the batch; a workgroup is four waves, or one where
// four waves' LDS would leave a CU to a single workgroup (the host chooses: pcx_bary_box.hip).
//
//   prologue  weight vectors of every dimension -> the wave's LDS table bw[row][point] (the layout k_bary_mfma
//             documents: head rows, ones, tail rows, ones);
//             B operands Bl[s][nt][lane] (lane l: k = R + 4 s + (l >> 4), point 16 nt + (l & 15)) = product of the
//             tail weights named by kcode[4 s + (l >> 4)] -> the wave's LDS, behind its table: the k-step count is a
//             runtime value, so they cannot be held in registers;
//             seed weights ws[nt][r] (kcode[4 KS + r]) in registers, R <= 2.
//   main      for each row tile t: acc[nt] = seed + sum_s mfma(A = frag[t][s], Bl[s][nt]); the seed is +0.0, then the
//             R columns as FMAs; cs[nt] += acc[nt][j] * (head weight product named by the row codes); every
//             PCX_CHUNK_TILES tiles cs is added to the lane's total -- the operations of k_bary_mfma in its order.
//   One workgroup walks all row tiles of its rows: no split launches, so a result does not depend on the batch size.
//   All four code fields are read whatever the plan: a dead field names the ones row and a product with exactly 1.0
//   changes no bit.
// dynamic LDS = waves * (plan.rows * PW + KS * NT * 64) * 8 bytes.
// ---------------------------------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(256)
k_bary_box_mfma(BaryDims dims, BaryMfmaPlan plan, BaryBoxCols cols, int wide, const double *__restrict__ nodes,
                const double *__restrict__ wts, const double *__restrict__ boxq, const double *__restrict__ rinv,
                const double *__restrict__ frag_, const unsigned *__restrict__ rowcode,
                const unsigned *__restrict__ kcode, const unsigned *__restrict__ rowcode_hi,
                const unsigned *__restrict__ kcode_hi, const double *__restrict__ rows, double *__restrict__ out, long N) {
    static_assert(NT == 1 || NT == 2, "one or two column tiles per wave");
    constexpr int PW = 16 * NT;
    constexpr int PH = 64 / PW;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane >> 4;
    const int c = lane & 15;
    const int KS = plan.KS, R = plan.R;
    double *bw = lds + (size_t)wave * ((size_t)plan.rows * PW + (size_t)KS * NT * 64);
    const double *bwt = bw + (size_t)plan.tail_base * PW;      // tail part: what the k codes index
    double *Bl = bw + (size_t)plan.rows * PW;
    const long base = ((long)blockIdx.x * (blockDim.x >> 6) + wave) * PW;     // one or four waves per workgroup
    typedef const double __attribute__((address_space(1))) *gptr_t;
    const gptr_t frag = (gptr_t)frag_;
    const pcx_seed_ptr seed = (pcx_seed_ptr)(frag + (size_t)plan.MT * KS * 64);

    // ---- prologue 1: weight vectors (lane -> row lane % PW of the wave, dims strided by PH)
    {
        const int pp = lane % PW;
        const int ph = lane / PW;
        const long pidx = base + pp;
        const bool valid = pidx < N;
        const double *rp = rows + (valid ? pidx : 0) * cols.width;
        for (int k = ph; k < dims.d; k += PH) {
            const int trow = dims.off[k] + (k >= plan.split ? 1 : 0);
            box_dim_weights(dims, cols, k, valid, rp, nodes, wts, boxq, rinv, bw + (size_t)trow * PW + pp, PW);
        }
        if (ph == 0) {
            bw[(size_t)(plan.tail_base - 1) * PW + pp] = 1.0;
            bw[(size_t)(plan.rows - 1) * PW + pp] = 1.0;
        }
    }
    __syncthreads();

    // ---- prologue 2: B operands -> LDS, seed weights -> registers
    for (int s = 0; s < KS; ++s) {
        const unsigned code = kcode[4 * s + g];
        double b[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) b[nt] = code_weight(code, bwt + 16 * nt + c, PW);
        if (wide) {
            const unsigned hi = kcode_hi[4 * s + g];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[nt] *= code_weight(hi, bwt + 16 * nt + c, PW);
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) Bl[((size_t)s * NT + nt) * 64 + lane] = b[nt];
    }
    double ws[NT][2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) ws[nt][r] = 0.0;
        if (r < R) {
            const unsigned code = kcode[4 * KS + r];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) ws[nt][r] = code_weight(code, bwt + 16 * nt + c, PW);
            if (wide) {
                const unsigned hi = kcode_hi[4 * KS + r];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) ws[nt][r] *= code_weight(hi, bwt + 16 * nt + c, PW);
            }
        }
    }
    __syncthreads();

    // ---- main loop over all row tiles
    double total[NT], cs[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { total[nt] = 0.0; cs[nt] = 0.0; }
    const gptr_t tf = frag + lane;
    const double *bl = Bl + lane;
    constexpr int U = 6;                // k-steps per group (11^5: 30 = 5 groups)
    const int ngrp = KS / U;
    double a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = ngrp > 0 ? tf[(size_t)u * 64] : 0.0;
    for (int t = 0; t < plan.MT; ++t) {
        pcx_d4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = (pcx_d4){0.0, 0.0, 0.0, 0.0};
        for (int r = 0; r < R; ++r) {
            const pcx_d4 sd = seed[((size_t)4 * t + g) * R + r];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const double w = r == 0 ? ws[nt][0] : ws[nt][1];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[nt][j] = __builtin_fma(sd[j], w, acc[nt][j]);
            }
        }
        const pcx_u4 q = load_row_codes(rowcode, t, g);
        pcx_u4 qh = q;
        if (wide) qh = load_row_codes(rowcode_hi, t, g);
        const gptr_t tt = tf + (size_t)t * KS * 64;
        double w[NT][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) w[nt][j] = code_weight(q.v[j], bw + 16 * nt + c, PW);
            if (wide) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) w[nt][j] *= code_weight(qh.v[j], bw + 16 * nt + c, PW);
            }
        }
        // whole groups of U k-steps: the fragments of the next group (at a tile's last group: the first group of the
        // next tile -- the image is one stream) are fetched before this group's matrix instructions are issued
        for (int gq = 0; gq < ngrp; ++gq) {
            const gptr_t nx = gq + 1 < ngrp ? tt + (size_t)(gq + 1) * U * 64
                                            : tf + (size_t)(t + 1 < plan.MT ? t + 1 : t) * KS * 64;
            double an[U];
#pragma unroll
            for (int u = 0; u < U; ++u) an[u] = nx[(size_t)u * 64];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], bl[((size_t)(gq * U + u) * NT + nt) * 64], acc[nt], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u) a[u] = an[u];
        }
        for (int s = ngrp * U; s < KS; ++s) {
            const double ar = tt[(size_t)s * 64];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bl[((size_t)s * NT + nt) * 64], acc[nt], 0, 0, 0);
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int j = 0; j < 4; ++j) cs[nt] = __builtin_fma(acc[nt][j], w[nt][j], cs[nt]);
        if (((t + 1) % PCX_CHUNK_TILES == 0) || (t + 1 == plan.MT)) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) { total[nt] += cs[nt]; cs[nt] = 0.0; }
        }
    }

    // ---- add the four 16-lane groups: lane group 0 ends with (s0 + s1) + (s2 + s3)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        double v = total[nt];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        const long pidx = base + 16 * nt + c;
        if (g == 0 && pidx < N) out[pidx] = v;
    }
}
