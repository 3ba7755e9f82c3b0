// tt_als_kernels.h -- fixed-rank TT completion (ALS in projection form) and core orthogonalisation on gfx950.
//
// With the cores on either side of position k in orthonormal form the least-squares design matrix of core k is
// L (x) I (x) R with orthonormal columns, so the solve is the projection C_k = L^T T R^T: chains of two tall-skinny
// FP64 contractions over the target tensor,
//   left   out (r' x R) = Q^T (r' x K) . P (K x R)      Q (K x r') row-major, R the contiguous remainder
//   right  out (R x r)  = P (R x K) . C^T (K x r)       C (r x K) row-major, K contiguous per row of P
// both memory-bound at the ranks this library serves.  Each has two forms, as the evaluation kernels (tt_kernels.h):
// one output column (row) per lane on VALU FMAs with the core elements as uniform operands, and 16 x 16 output tiles on
// v_mfma_f64_16x16x4_f64.  The host picks by rank (pcx_tt_als.hip, mfma_min_rank).  Every shape may be ragged: K, R
// and the ranks need not be multiples of 4 or 16; loads are guarded and padded with zeros, stores are guarded.
// The QR factorisation of one unfolding is a Householder sweep in one workgroup (not the hot path).
// Every sum runs in a fixed order -- one thread, one MFMA accumulator chain, or a fixed tree in LDS -- and nothing
// uses floating-point atomics: equal input gives equal bits.
// All kernels are static: the header may be included by more than one translation unit.
#pragma once

#include "pcx_common.h"

#define TTA_THREADS 256
#define TTA_RED_BLOCKS 1024

// ---------------------------------------------------------------------------------
// contractions, VALU forms: RC accumulators per lane, rows (columns) i0 .. i0 + RC of the small factor
// ---------------------------------------------------------------------------------
template <int RC>
static __global__ void __launch_bounds__(TTA_THREADS)
k_tta_left_valu(const double *__restrict__ Q, const double *__restrict__ P, double *__restrict__ out, int K, int rp, long R) {
    const long j = (long)blockIdx.x * TTA_THREADS + threadIdx.x;
    if (j >= R) return;
    const int i0 = blockIdx.y * RC;
    double acc[RC];
#pragma unroll
    for (int c = 0; c < RC; ++c) acc[c] = 0.0;
    for (int k = 0; k < K; ++k) {
        const double p = P[(long)k * R + j];
        const double *q = Q + (long)k * rp;
#pragma unroll
        for (int c = 0; c < RC; ++c) acc[c] = __builtin_fma(q[min(i0 + c, rp - 1)], p, acc[c]);     // uniform operand
    }
#pragma unroll
    for (int c = 0; c < RC; ++c)
        if (i0 + c < rp) out[(long)(i0 + c) * R + j] = acc[c];
}

template <int RC>
static __global__ void __launch_bounds__(TTA_THREADS)
k_tta_right_valu(const double *__restrict__ P, const double *__restrict__ C, double *__restrict__ out, long R, int K, int r) {
    const long j = (long)blockIdx.x * TTA_THREADS + threadIdx.x;
    if (j >= R) return;
    const int i0 = blockIdx.y * RC;
    const double *prow = P + j * K;
    double acc[RC];
#pragma unroll
    for (int c = 0; c < RC; ++c) acc[c] = 0.0;
    for (int k = 0; k < K; ++k) {
        const double p = prow[k];
#pragma unroll
        for (int c = 0; c < RC; ++c) acc[c] = __builtin_fma(C[(long)min(i0 + c, r - 1) * K + k], p, acc[c]);
    }
#pragma unroll
    for (int c = 0; c < RC; ++c)
        if (i0 + c < r) out[j * r + i0 + c] = acc[c];
}

// ---------------------------------------------------------------------------------
// contractions, MFMA forms.  v_mfma_f64_16x16x4_f64: lane l = 16 g + c holds A[c][g] and B[g][c]; result register v
// of lane l is D[g + 4 v][c].  One wave owns 64 columns (rows) of the large operand = 4 tiles, RT tiles of the rank.
// ---------------------------------------------------------------------------------
template <int RT>
static __global__ void __launch_bounds__(TTA_THREADS)
k_tta_left_mfma(const double *__restrict__ Q, const double *__restrict__ P, double *__restrict__ out, int K, int rp, long R) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, c16 = lane & 15;
    const long j0 = ((long)blockIdx.x * 4 + wave) * 64;
    if (j0 >= R) return;                                   // wave-uniform
    const int i0 = blockIdx.y * 16 * RT;
    pcx_d4 acc[RT][4];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[t][nt] = (pcx_d4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + g;
        const bool kok = k < K;
        double a[RT], b[4];
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            const int i = i0 + 16 * t + c16;
            a[t] = (kok && i < rp) ? Q[(long)k * rp + i] : 0.0;
        }
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const long j = j0 + 16 * nt + c16;
            b[nt] = (kok && j < R) ? P[(long)k * R + j] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[t][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], b[nt], acc[t][nt], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int i = i0 + 16 * t + g + 4 * v;
                const long j = j0 + 16 * nt + c16;
                if (i < rp && j < R) out[(long)i * R + j] = acc[t][nt][v];
            }
}

template <int RT>
static __global__ void __launch_bounds__(TTA_THREADS)
k_tta_right_mfma(const double *__restrict__ P, const double *__restrict__ C, double *__restrict__ out, long R, int K, int r) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, c16 = lane & 15;
    const long j0 = ((long)blockIdx.x * 4 + wave) * 64;
    if (j0 >= R) return;                                   // wave-uniform
    const int i0 = blockIdx.y * 16 * RT;
    pcx_d4 acc[RT][4];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[t][nt] = (pcx_d4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + g;
        const bool kok = k < K;
        double a[RT], b[4];
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            const int i = i0 + 16 * t + c16;
            a[t] = (kok && i < r) ? C[(long)i * K + k] : 0.0;
        }
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const long j = j0 + 16 * nt + c16;
            b[nt] = (kok && j < R) ? P[j * K + k] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[t][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], b[nt], acc[t][nt], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int i = i0 + 16 * t + g + 4 * v;
                const long j = j0 + 16 * nt + c16;
                if (i < r && j < R) out[j * r + i] = acc[t][nt][v];
            }
}

// ---------------------------------------------------------------------------------
// small dense helpers (cores and factors of a few kilobytes; the last step of a reconstruction writes prod(n) values)
// ---------------------------------------------------------------------------------
// C (M x N) = A (M x K) . B, B[k][j] = Bp[k * bsk + j * bsj]: one output per thread, k ascending
static __global__ void __launch_bounds__(TTA_THREADS)
k_tta_gemm(const double *__restrict__ A, const double *__restrict__ Bp, long bsk, long bsj, double *__restrict__ C, long M,
           long N, int K) {
    const long total = M * N;
    for (long e = (long)blockIdx.x * TTA_THREADS + threadIdx.x; e < total; e += (long)gridDim.x * TTA_THREADS) {
        const long i = e / N, j = e - i * N;
        const double *a = A + i * K;
        double s = 0.0;
        for (int k = 0; k < K; ++k) s = __builtin_fma(a[k], Bp[(long)k * bsk + j * bsj], s);
        C[e] = s;
    }
}

// out (cols x rows) = in^T, in (rows x cols) row-major
static __global__ void __launch_bounds__(TTA_THREADS)
k_tta_transpose(const double *__restrict__ in, long rows, long cols, double *__restrict__ out) {
    const long total = rows * cols;
    for (long e = (long)blockIdx.x * TTA_THREADS + threadIdx.x; e < total; e += (long)gridDim.x * TTA_THREADS) {
        const long r = e / cols, c = e - r * cols;
        out[c * rows + r] = in[e];
    }
}

// ---------------------------------------------------------------------------------
// Householder QR of A (m x c, row-major, overwritten), c <= 256, in ONE workgroup: Q (m x p) with orthonormal columns,
// R (p x c) upper triangular, p = min(m, c).  Columns are taken in their own order, no pivoting.  A column that is
// zero below its diagonal takes the identity reflector (LAPACK's tau = 0), so Q stays orthonormal whatever the rank of
// A.  The reflectors live below the diagonal of A (v_j = 1 implied) until Q is formed from them, last to first.
// Each column's norm is taken on the column times a power of two, so Q does not depend on the scale of A and R follows
// it exactly, for any finite FP64 magnitudes (tests/test_gpu_als_steps.py, 2^-900 .. 2^900).
// Threads are 8 row groups x 32 columns: a column's inner product is 8 partial sums over interleaved rows, added in
// row-group order.
// ---------------------------------------------------------------------------------
static __device__ __forceinline__ void tta_reflect(const double *A, int c, int j, double tau, double *X, int xc, int col_lo,
                                                   int col_hi, long m, double (*part)[33]) {
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int cb = col_lo; cb < col_hi; cb += 32) {
        const int col = cb + tx;
        const bool ok = col < col_hi;
        double w = 0.0;
        if (ok)
            for (long i = j + ty; i < m; i += 8) {
                const double v = (i == j) ? 1.0 : A[i * c + j];
                w = __builtin_fma(v, X[i * xc + col], w);
            }
        part[ty][tx] = w;
        __syncthreads();
        double ws = 0.0;
        for (int q = 0; q < 8; ++q) ws += part[q][tx];
        ws *= tau;
        if (ok)
            for (long i = j + ty; i < m; i += 8) {
                const double v = (i == j) ? 1.0 : A[i * c + j];
                X[i * xc + col] = __builtin_fma(-ws, v, X[i * xc + col]);
            }
        __syncthreads();
    }
}

static __global__ void __launch_bounds__(TTA_THREADS)
k_tta_householder(double *__restrict__ A, long m, int c, double *__restrict__ Q, double *__restrict__ R) {
    __shared__ double s_tau[256];
    __shared__ double s_red[TTA_THREADS];
    __shared__ double s_part[8][33];
    __shared__ double s_sc[2];
    const int t = threadIdx.x;
    const int p = (int)(m < (long)c ? m : (long)c);
    for (int j = 0; j < p; ++j) {
        // the column from the diagonal down times 2^-ex, ex the exponent of its largest magnitude: the squares can
        // neither overflow nor vanish together, and a power of two changes no bit of tau, of v or (undone) of beta
        double mx = 0.0;
        for (long i = j + t; i < m; i += TTA_THREADS) mx = fmax(mx, fabs(A[i * c + j]));
        s_red[t] = mx;
        __syncthreads();
        for (int h = TTA_THREADS / 2; h > 0; h >>= 1) {
            if (t < h) s_red[t] = fmax(s_red[t], s_red[t + h]);
            __syncthreads();
        }
        mx = s_red[0];
        const int ex = (mx > 0.0 && mx < INFINITY) ? max(ilogb(mx), -1022) : 0;     // 2^1022 is the largest 2^-ex
        const double down = scalbn(1.0, -ex);
        __syncthreads();
        double s = 0.0;
        for (long i = j + 1 + t; i < m; i += TTA_THREADS) {
            const double a = A[i * c + j] * down;
            s = __builtin_fma(a, a, s);
        }
        s_red[t] = s;
        __syncthreads();
        for (int h = TTA_THREADS / 2; h > 0; h >>= 1) {
            if (t < h) s_red[t] += s_red[t + h];
            __syncthreads();
        }
        if (t == 0) {
            const double sigma = s_red[0], alpha = A[(long)j * c + j] * down;
            double tau = 0.0, scale = 0.0, beta = A[(long)j * c + j];
            if (sigma != 0.0) {
                const double b = -copysign(sqrt(__builtin_fma(alpha, alpha, sigma)), alpha);
                tau = (b - alpha) / b;
                scale = 1.0 / (alpha - b);
                beta = scalbn(b, ex);
            }
            s_tau[j] = tau;
            s_sc[0] = scale;
            s_sc[1] = beta;
        }
        __syncthreads();
        const double tau = s_tau[j];
        if (tau != 0.0) {                                  // uniform over the workgroup
            const double scale = s_sc[0];
            for (long i = j + 1 + t; i < m; i += TTA_THREADS) A[i * c + j] = A[i * c + j] * down * scale;
            __syncthreads();
            tta_reflect(A, c, j, tau, A, c, j + 1, c, m, s_part);
            if (t == 0) A[(long)j * c + j] = s_sc[1];
        }
        __syncthreads();
    }
    for (long e = t; e < (long)p * c; e += TTA_THREADS) {
        const long i = e / c, col = e - i * c;
        R[e] = col >= i ? A[e] : 0.0;
    }
    for (long e = t; e < m * p; e += TTA_THREADS) {
        const long i = e / p, col = e - i * p;
        Q[e] = i == col ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int j = p - 1; j >= 0; --j) {
        const double tau = s_tau[j];
        if (tau != 0.0) tta_reflect(A, c, j, tau, Q, p, j, p, m, s_part);
    }
}

// ---------------------------------------------------------------------------------
// convergence: the four sums of squares of one outer iteration in one pass over the resident tensors
//   s0 = |new - prev|^2, s1 = |prev|^2, s2 = |new - target|^2, s3 = |target|^2
// per-block partial sums (fixed grid, fixed tree), then one block adds the partials
// ---------------------------------------------------------------------------------
static __device__ __forceinline__ double tta_block_sum(double v, double *red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int h = TTA_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    return red[0];
}

static __global__ void __launch_bounds__(TTA_THREADS)
k_tta_norms(const double *__restrict__ tnew, const double *__restrict__ tprev, const double *__restrict__ target, long G,
            double *__restrict__ partial) {
    __shared__ double red[TTA_THREADS];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (long e = (long)blockIdx.x * TTA_THREADS + threadIdx.x; e < G; e += (long)gridDim.x * TTA_THREADS) {
        const double a = tnew[e], b = tprev[e], c = target[e];
        s0 = __builtin_fma(a - b, a - b, s0);
        s1 = __builtin_fma(b, b, s1);
        s2 = __builtin_fma(a - c, a - c, s2);
        s3 = __builtin_fma(c, c, s3);
    }
    const double r0 = tta_block_sum(s0, red), r1 = tta_block_sum(s1, red), r2 = tta_block_sum(s2, red),
                 r3 = tta_block_sum(s3, red);
    if (threadIdx.x == 0) {
        double *o = partial + (long)blockIdx.x * 4;
        o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3;
    }
}

static __global__ void __launch_bounds__(TTA_THREADS)
k_tta_norms_final(const double *__restrict__ partial, int blocks, double *__restrict__ out4) {
    __shared__ double red[TTA_THREADS];
    for (int q = 0; q < 4; ++q) {
        double s = 0.0;
        for (int b = threadIdx.x; b < blocks; b += TTA_THREADS) s += partial[(long)b * 4 + q];
        const double r = tta_block_sum(s, red);
        if (threadIdx.x == 0) out4[q] = r;
    }
}
