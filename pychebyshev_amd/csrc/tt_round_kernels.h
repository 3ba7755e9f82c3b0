// tt_round_kernels.h -- TT rounding and adjacent-core swaps on the device (gfx950).
//
// The factorisations themselves are the one-sided row-Jacobi iteration of ttsvd_kernels.h: every step of
// a rounding or a swap factors a short, wide matrix M (m x N, m <= N in the cases that matter) as M = U B
// with U orthogonal and the rows of B mutually orthogonal, B's row norms being the singular values.  Rows
// that are exactly dependent (the stacked cores of a + a or a - a) rotate into exact zero rows, so the
// orthogonalisation needs no Gram matrix and no pivoting to survive rank deficiency.
// The kernels here only move data around those factorisations: unfold a core, split the factors into the
// new cores, and multiply a factor into the neighbouring core.  Every sum runs in a fixed order in one
// thread, so the results do not depend on the launch order.
#pragma once

#include "pcx_common.h"

#define TTR_THREADS 256

// out (cols x rows) = in^T, in row-major (rows x cols): the (r_l n) x r_r unfolding of a core into the
// r_r x (r_l n) matrix whose rows the Jacobi iteration orthogonalises
__global__ void __launch_bounds__(TTR_THREADS)
k_ttr_transpose(const double *__restrict__ in, long rows, long cols, double *__restrict__ out) {
    __shared__ double tile[32][33];
    const long r0 = (long)blockIdx.y * 32, c0 = (long)blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8 threads
    for (int k = ty; k < 32; k += 8) {
        const long r = r0 + k, c = c0 + tx;
        if (r < rows && c < cols) tile[k][tx] = in[r * cols + c];
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const long c = c0 + k, r = r0 + tx;
        if (r < rows && c < cols) out[c * rows + r] = tile[tx][k];
    }
}

// out[a * oa + b * ob] = scale[a] * src[sel[a] * sa + b * sb]   (a < na, b < nb)
// One strided gather covers every way a factor is cut into a core: the kept rows of B divided by their
// singular values (row-orthonormal, or transposed for a left-orthonormal core), and the kept columns of U
// times their singular values (pushed into the neighbouring core, or stored as the left core of a swap).
__global__ void __launch_bounds__(TTR_THREADS)
k_ttr_pick(const double *__restrict__ src, long sa, long sb, const int *__restrict__ sel,
           const double *__restrict__ scale, int na, long nb, double *__restrict__ out, long oa, long ob) {
    const long total = (long)na * nb;
    for (long e = (long)blockIdx.x * TTR_THREADS + threadIdx.x; e < total; e += (long)gridDim.x * TTR_THREADS) {
        const long a = e / nb, b = e - a * nb;
        out[a * oa + b * ob] = scale[a] * src[(long)sel[a] * sa + b * sb];
    }
}

// C (M x N) = A (M x K) B (K x N), row-major: one output per thread, k ascending
__global__ void __launch_bounds__(TTR_THREADS)
k_ttr_gemm(const double *__restrict__ A, const double *__restrict__ B, double *__restrict__ C, long M, long N, int K) {
    const long total = M * N;
    for (long e = (long)blockIdx.x * TTR_THREADS + threadIdx.x; e < total; e += (long)gridDim.x * TTR_THREADS) {
        const long i = e / N, j = e - i * N;
        const double *a = A + i * K;
        double s = 0.0;
        for (int k = 0; k < K; ++k) s = __builtin_fma(a[k], B[(long)k * N + j], s);
        C[e] = s;
    }
}

// The merged pair of an adjacent swap with its node axes exchanged:
//   out[(l, b), (a, r)] = sum_m A[l, a, m] B[m, b, r]
// A (rl, na, rm), B (rm, nb, rr); out is (rl nb) x (na rr), row-major.
__global__ void __launch_bounds__(TTR_THREADS)
k_ttr_merge_swapped(const double *__restrict__ A, const double *__restrict__ B, int rl, int na, int rm, int nb,
                    int rr, double *__restrict__ out) {
    const long cols = (long)na * rr, total = (long)rl * nb * cols;
    for (long e = (long)blockIdx.x * TTR_THREADS + threadIdx.x; e < total; e += (long)gridDim.x * TTR_THREADS) {
        const long row = e / cols, col = e - row * cols;
        const int l = (int)(row / nb), b = (int)(row - (long)l * nb);
        const int a = (int)(col / rr), r = (int)(col - (long)a * rr);
        const double *pa = A + ((long)l * na + a) * rm;
        const double *pb = B + (long)b * rr + r;
        const long sb = (long)nb * rr;
        double s = 0.0;
        for (int m = 0; m < rm; ++m) s = __builtin_fma(pa[m], pb[m * sb], s);
        out[e] = s;
    }
}
