// bary_ladder_kernels.h -- ladders of the full-tensor barycentric interpolant: for every row of the batch, the model along
// one dimension at m values (ChebyshevApproximation.ladder_batch / fibre_batch; gfx950).
//
// The tensor-product barycentric formula is separable, so a row's restriction to dimension `dim` is exact:
//     F[r][j] = sum_{i_q, q != dim} T[i_0, .., j, .., i_{d-1}] prod_{q != dim} v_q[r][i_q]        (the row's FIBRE)
// with v_q the normalised barycentric weights of the row's coordinate in dimension q (bary_weights_1d, unchanged: the
// one-hot rule within 1e-14 of a node included), and the ladder is the 1-D barycentric interpolant of F[r][:] at the
// row's m values (ladder_interp_1d).  One contraction per row where m point evaluations make m.
//
//   k_bary_ladder_rows   any shape, on the plain tensor read with strides: k_bary_rows' walk with n_dim running sums
//   k_bary_ladder_mfma   v_mfma_f64_16x16x4_f64: D (16 rows x 16 fibre nodes per column tile) += A (16 rows x 4 k,
//                        the weight products, formed in-kernel) . B (4 k x 16 nodes, the tensor with `dim` innermost:
//                        an image packed once per (spec, dim) by k_pack_ladder)
//
// The K axis (the other dimensions, C order) is cut in two: the last `nlo` of them form the LOW part (Klo entries,
// padded to Klo4 = 4 ceil(Klo / 4)), the ones in front the HIGH part (Khi entries).  The image is
//     img[(kh * Klo4 + kl) * NP + j] = T[kh, kl, j]   (kl < Klo, j < n_dim; zero elsewhere),   NP = 16 CT,
// so no k-step straddles two kh, and A[r][kh, kl] = wh[r][kh] * P[r][kl]: P, the weight products of the low part, sits
// in LDS (one read per matrix instruction), wh is formed once per kh.  A padded kl multiplies zeros of the image.
//
// Both kernels: no atomics, a fixed order of additions, one workgroup per block of rows and no split launches, so a
// row's bits depend neither on the batch it is in nor on m.  Rows and xs have their own strides: the host-pointer
// entry stages (fixed, xs) of a row side by side.
#pragma once

#include "bary_kernels.h"

struct BaryLadder {
    int dim, n;                   // the dimension left uncontracted and its node count
    int nq;                       // the other dimensions: d - 1
    int q[PCX_MAX_DIMS];          // ... in increasing order (the columns of `fixed`)
    long stride[PCX_MAX_DIMS];    // element stride of dimension q[i] in the C-order tensor
    long dstride;                 // ... of dim
    long K;                       // prod n[q[i]]
    // MFMA form (CT == 0: not available)
    int CT;                       // column tiles of 16 fibre nodes
    int nlo;                      // trailing other dimensions in the low part
    int Klo, Klo4;
    long Khi;
    int wrow[PCX_MAX_DIMS];       // first row of q[i] in the wave's weight table
    int wrows;                    // its rows: sum of n[q[i]]
};

// zeroed doubles behind a ladder image: k_bary_ladder_mfma fetches its B operands two groups of k-steps ahead
#define PCX_LADDER_PAD 2048

// The 1-D barycentric interpolant of the fibre F (n values at the ascending nodes) at x, by bary_weights_1d's rule:
// the first node within 1e-14 of x gives F at that node itself, else sum_j u_j F_j / sum_j u_j, u_j = w_j / (x - x_j),
// both sums j ascending.  A NaN x fails every node test and gives NaN.
__device__ __forceinline__ double ladder_interp_1d(double x, const double *__restrict__ nodes, const double *__restrict__ wts,
                                                   int n, const double *F) {
    int exact = -1;
    for (int j = 0; j < n; ++j) {
        const double diff = x - nodes[j];
        if (exact < 0 && __builtin_fabs(diff) < 1e-14) exact = j;
    }
    if (exact >= 0) return F[exact];
    double su = 0.0, sf = 0.0;
    for (int j = 0; j < n; ++j) {
        const double u = wts[j] / (x - nodes[j]);
        su += u;
        sf = __builtin_fma(u, F[j], sf);
    }
    return sf / su;
}

// offset in the plain tensor of entry `kap` of the K axis (dim at index 0), and the product of the row's weights there
// (bw: the row's weights by nodes_cat offset, stride 1)
__device__ __forceinline__ long ladder_k_offset(const BaryDims &dims, const BaryLadder &lp, long kap, const double *bw, double *w_out) {
    double w = 1.0;
    long base = 0, rem = kap;
    for (int i = lp.nq - 1; i >= 0; --i) {
        const int k = lp.q[i];
        const int nk = dims.n[k];
        const int idx = (int)(rem % nk);
        rem /= nk;
        if (bw) w *= bw[dims.off[k] + idx];
        base += idx * lp.stride[i];
    }
    if (w_out) *w_out = w;
    return base;
}

// ---------------------------------------------------------------------------------
// Any shape.  LPP lanes share one row: weights -> LDS, then lane `sub` walks entries sub, sub + LPP, ... of the K axis
// with 8 fibre nodes at a time in registers (a fibre of any length: ceil(n / 8) walks), a shuffle tree over the LPP
// lanes adds them, the fibre goes to LDS and the LPP lanes share the row's m values.
// dynamic LDS = (256 / LPP) * (sum_n + n_dim) * 8 bytes.
// ---------------------------------------------------------------------------------
#define PCX_LADDER_JC 8
static __global__ void __launch_bounds__(256)
k_bary_ladder_rows(BaryDims dims, BaryLadder lp, int LPP, const double *__restrict__ nodes, const double *__restrict__ wts,
                   const double *__restrict__ T, const double *__restrict__ fixed, long fstride,
                   const double *__restrict__ xs, long xstride, int m, double *__restrict__ out, long N) {
    extern __shared__ double lds[];
    const int ppw = 256 / LPP;                 // rows per workgroup
    const int pl = threadIdx.x / LPP;          // local row
    const int sub = threadIdx.x % LPP;         // lane within the row's group
    const long pidx = (long)blockIdx.x * ppw + pl;
    const bool valid = pidx < N;
    double *bw = lds + (size_t)pl * (dims.sum_n + lp.n);
    double *F = bw + dims.sum_n;
    for (int i = sub; i < lp.nq; i += LPP) {
        const int k = lp.q[i];
        const double *nd = nodes + dims.off[k];
        const double x = valid ? fixed[pidx * fstride + i] : nd[0];
        bary_weights_1d(x, nd, wts + dims.off[k], dims.n[k], bw + dims.off[k], 1);
    }
    __syncthreads();
    for (int j0 = 0; j0 < lp.n; j0 += PCX_LADDER_JC) {
        double acc[PCX_LADDER_JC];
#pragma unroll
        for (int jj = 0; jj < PCX_LADDER_JC; ++jj) acc[jj] = 0.0;
        for (long kap = sub; kap < lp.K; kap += LPP) {
            double w;
            const double *tp = T + ladder_k_offset(dims, lp, kap, bw, &w) + j0 * lp.dstride;
#pragma unroll
            for (int jj = 0; jj < PCX_LADDER_JC; ++jj)
                if (j0 + jj < lp.n) acc[jj] = __builtin_fma(tp[jj * lp.dstride], w, acc[jj]);
        }
#pragma unroll
        for (int jj = 0; jj < PCX_LADDER_JC; ++jj) {
            for (int o = LPP >> 1; o > 0; o >>= 1) acc[jj] += __shfl_xor(acc[jj], o, 64);
            if (sub == 0 && j0 + jj < lp.n) F[j0 + jj] = acc[jj];
        }
    }
    __syncthreads();
    if (!valid) return;
    const double *nd = nodes + dims.off[lp.dim], *wd = wts + dims.off[lp.dim];
    for (int xi = sub; xi < m; xi += LPP)
        out[pidx * m + xi] = ladder_interp_1d(xs[pidx * xstride + xi], nd, wd, lp.n, F);
}

// The B image of one (spec, dim): see the head of this file.  total = Khi * Klo4 * NP (the host zeroes PCX_LADDER_PAD
// doubles behind it).
static __global__ void __launch_bounds__(256)
k_pack_ladder(BaryDims dims, BaryLadder lp, const double *__restrict__ T, double *__restrict__ img, long total) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int NP = 16 * lp.CT;
    const int j = (int)(idx % NP);
    const long r = idx / NP;
    const int kl = (int)(r % lp.Klo4);
    const long kh = r / lp.Klo4;
    double v = 0.0;
    if (j < lp.n && kl < lp.Klo) v = T[ladder_k_offset(dims, lp, kh * lp.Klo + kl, nullptr, nullptr) + j * lp.dstride];
    img[idx] = v;
}

// ---------------------------------------------------------------------------------
// MFMA form.  One wave per workgroup owns 16 rows of the batch.
//   prologue  weights of the other dimensions -> bw[table row][row] (lane: row c = lane & 15, dimensions strided by the
//             four lane groups); low-part products -> P[kl][row];
//   main      for each kh: wh = product of the high part's weights at kh (lane's row c); for each k-step s of the low
//             part: A = wh * P[4 s + g][c] (lane l holds A[l & 15][l >> 4]), B = img[kh][4 s + g][16 ct + c], one
//             matrix instruction per column tile; the k-steps of all kh run as one stream in groups of U = 16 / 8 / 4
//             (CT = 1 / 2 / 3, 4) whose B operands are fetched one group ahead;
//   epilogue  accumulators (lane l, register i: row g + 4 i, node 16 ct + c) -> LDS, then the 16 m (row, x) pairs over
//             the lanes, x fastest, through ladder_interp_1d.
// dynamic LDS = (wrows * 16 + Klo4 * 16 + 16 * (16 CT + 1)) * 8 bytes.
// ---------------------------------------------------------------------------------
template <int CT>
__global__ void __launch_bounds__(64)
k_bary_ladder_mfma(BaryDims dims, BaryLadder lp, const double *__restrict__ nodes, const double *__restrict__ wts,
                   const double *__restrict__ img, const double *__restrict__ fixed, long fstride,
                   const double *__restrict__ xs, long xstride, int m, double *__restrict__ out, long N) {
    constexpr int NP = 16 * CT;
    constexpr int FS = NP + 1;
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int g = lane >> 4;
    const int c = lane & 15;
    double *bw = lds;
    double *P = bw + (size_t)lp.wrows * 16;
    double *F = P + (size_t)lp.Klo4 * 16;
    const long base = (long)blockIdx.x * 16;
    {
        const long pidx = base + c;
        const bool valid = pidx < N;
        for (int i = g; i < lp.nq; i += 4) {
            const int k = lp.q[i];
            const double *nd = nodes + dims.off[k];
            const double x = valid ? fixed[pidx * fstride + i] : nd[0];
            bary_weights_1d(x, nd, wts + dims.off[k], dims.n[k], bw + (size_t)lp.wrow[i] * 16 + c, 16);
        }
    }
    __syncthreads();
    const int ihi = lp.nq - lp.nlo;            // other dimensions [0, ihi) are the high part
    for (int kl = g; kl < lp.Klo4; kl += 4) {
        double w = 0.0;
        if (kl < lp.Klo) {
            w = 1.0;
            int rem = kl;
            for (int i = lp.nq - 1; i >= ihi; --i) {
                const int nk = dims.n[lp.q[i]];
                const int idx = rem % nk;
                rem /= nk;
                w *= bw[(size_t)(lp.wrow[i] + idx) * 16 + c];
            }
        }
        P[kl * 16 + c] = w;
    }
    __syncthreads();

    pcx_d4 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = (pcx_d4){0.0, 0.0, 0.0, 0.0};
    // The image is one stream of S = Khi KS k-steps (step t at t * 4 NP doubles).  Groups of U steps without a branch
    // inside: the A and B operands of the next group are fetched (LDS, global) before this group's matrix instructions
    // are issued.  A group spans at most two kh when KS >= U: its steps take wh0 or wh1 by a select.  The steps of the
    // last group behind S multiply the PCX_LADDER_PAD zeroed doubles behind the image (the fetch reaches two groups
    // past the last step) by weights of a wrapped kh: they add zeros.  Shorter low parts (KS < U) take the plain loop.
    constexpr int U = CT == 1 ? 16 : (CT == 2 ? 8 : 4);
    static_assert(2 * U * 4 * NP <= PCX_LADDER_PAD, "the prefetch reaches two groups past the last step");
    const int KS = lp.Klo4 >> 2;
    const long S = lp.Khi * KS;
    const double *pa = P + g * 16 + c;
    const double *bt = img + (size_t)g * NP + c;
    auto high_weight = [&](long kh) {          // kh >= Khi (behind the last step) wraps inside the table
        double w = 1.0;
        long rem = kh;
        for (int i = ihi - 1; i >= 0; --i) {
            const int nk = dims.n[lp.q[i]];
            const int idx = (int)(rem % nk);
            rem /= nk;
            w *= bw[(size_t)(lp.wrow[i] + idx) * 16 + c];
        }
        return w;
    };
    if (KS >= U) {
        long kh = 0;
        int s0 = 0;
        double wh0 = high_weight(0), wh1 = high_weight(1);
        double ac[U], bc[U][CT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ac[u] = wh0 * pa[u * 64];            // KS >= U: group 0 lies within kh = 0
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) bc[u][ct] = bt[(size_t)u * 4 * NP + 16 * ct];
        }
        for (long t0 = 0; t0 < S; t0 += U) {
            s0 += U;
            if (s0 >= KS) {
                s0 -= KS;
                wh0 = wh1;
                wh1 = high_weight(++kh + 1);
            }
            const double *nx = bt + (size_t)(t0 + U) * 4 * NP;
            double an[U], bn[U][CT];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool over = s0 + u >= KS;
                an[u] = (over ? wh1 : wh0) * pa[(over ? s0 + u - KS : s0 + u) * 64];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) bn[u][ct] = nx[(size_t)u * 4 * NP + 16 * ct];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
                    acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[u], bc[u][ct], acc[ct], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                ac[u] = an[u];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) bc[u][ct] = bn[u][ct];
            }
        }
    } else {
        for (long kh = 0; kh < lp.Khi; ++kh) {
            const double wh = high_weight(kh);
            const double *bk = bt + (size_t)kh * lp.Klo4 * NP;
            for (int s = 0; s < KS; ++s) {
                const double a = wh * pa[s * 64];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
                    acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bk[(size_t)s * 4 * NP + 16 * ct], acc[ct], 0, 0, 0);
            }
        }
    }

#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int i = 0; i < 4; ++i) F[(g + 4 * i) * FS + 16 * ct + c] = acc[ct][i];
    __syncthreads();
    const double *nd = nodes + dims.off[lp.dim], *wd = wts + dims.off[lp.dim];
    const long pairs = 16L * m;
    for (long p = lane; p < pairs; p += 64) {
        const int r = (int)(p / m);
        const int xi = (int)(p - (long)r * m);
        const long pidx = base + r;
        if (pidx < N) out[pidx * m + xi] = ladder_interp_1d(xs[pidx * xstride + xi], nd, wd, lp.n, F + r * FS);
    }
}
