// mode_product_kernels.h -- the rectangular FP64 mode product (gfx950)
//
//   Y[o, j, q] = sum_i W[j, i] * X[o, i, q]        o < outer, i < n, j < m, q < inner     (C order)
//
// the pass of a tensor-product grid evaluation (pcx_bary_eval_tensor_grid: W = barycentric weights of one axis) and
// the step of a tensor-train grid chain (pcx_tt_tensor_grid).  Three kernels, all with 64-bit indices:
//
//   k_mode_product_rect        any shape: one fma chain per output, i ascending (k_mode_product made rectangular)
//   k_mode_product_mfma        inner > 1:  v_mfma_f64_16x16x4_f64 with A = a 16 x 4 block of W (rows j), B = a 4 x 16
//                              block of X_o (columns q: consecutive lanes on consecutive q, 128-byte rows), D rows = j,
//                              D columns = q: stores coalesced along q
//   k_mode_product_mfma_last   inner == 1: A = 16 rows of X (rows o), B = W^T (columns j), D columns = j: stores
//                              contiguous along j; W staged in LDS per workgroup when it fits, read in place otherwise
//
// Lane map of v_mfma_f64_16x16x4_f64: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]; result register v of lane l
// is D[(l >> 4) + 4 v][l & 15].  The instruction is a k-ordered fma chain that starts from C, and the k-steps run
// i ascending, so every output is the SAME chain as in k_mode_product_rect, wherever it falls in a tile.
//
// Ragged tiles and the K remainder: a lane whose row, column or k index is dead gets a ZERO OPERAND by a select and
// loads nothing (never an address outside X or W, and never 0 * NaN); only the live part of a tile is stored.
//
// One-hot rows: hot[j] >= 0 says that row j of W is one-hot at that column (a grid coordinate on a node).  Such an
// output is the GATHER X[o, hot[j], q], as in the reference's pointwise rule, not a sum with zero weights: it carries
// the tensor's bits (a -0.0 included) and stays finite when another entry of its fibre is NaN or Inf.  hot == NULL:
// every row is summed.
#pragma once

#include "pcx_common.h"

#define PCX_MP_THREADS 256
#define PCX_MP_WAVES (PCX_MP_THREADS / PCX_WAVE)

static __global__ __launch_bounds__(PCX_MP_THREADS) void k_mode_product_rect(const double *__restrict__ X,
                                                                             const double *__restrict__ W,
                                                                             double *__restrict__ Y, long outer, int n,
                                                                             long inner, int m, const int *__restrict__ hot) {
    const long total = outer * m * inner;
    const long step = (long)gridDim.x * blockDim.x;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += step) {
        const long q = idx % inner;
        const long t = idx / inner;
        const int j = (int)(t % m);
        const long o = t / m;
        const double *src = X + (o * n) * inner + q;
        const double *wrow = W + (long)j * n;
        const int hv = hot ? hot[j] : -1;
        double s = 0.0;
        if (hv >= 0) s = src[(long)hv * inner];
        else
            for (int i = 0; i < n; ++i) s = __builtin_fma(wrow[i], src[(long)i * inner], s);
        Y[idx] = s;
    }
}

// tiles = outer * MT * QT 16 x 16 output tiles, tile t = (o * MT + jt) * QT + qt; one wave per tile, grid-stride
static __global__ __launch_bounds__(PCX_MP_THREADS) void k_mode_product_mfma(const double *__restrict__ X,
                                                                             const double *__restrict__ W,
                                                                             double *__restrict__ Y, long outer, int n,
                                                                             long inner, int m, int MT, long QT, long tiles,
                                                                             const int *__restrict__ hot) {
    const int lane = threadIdx.x & 63;
    const int c = lane & 15, g = lane >> 4;
    const int KS = (n + 3) >> 2;
    for (long t = (long)blockIdx.x * PCX_MP_WAVES + (threadIdx.x >> 6); t < tiles; t += (long)gridDim.x * PCX_MP_WAVES) {
        const long qt = t % QT;
        const long r = t / QT;
        const int jt = (int)(r % MT);
        const long o = r / MT;
        const int j = jt * 16 + c;            // row of W this lane feeds (A operand)
        const long q = qt * 16 + c;           // column of X_o this lane feeds (B operand) and stores
        const bool j_live = j < m, q_live = q < inner;
        const double *wrow = W + (long)(j_live ? j : 0) * n;
        const double *xcol = X + (o * n) * inner + (q_live ? q : 0);
        pcx_d4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int s = 0; s < KS; ++s) {
            const int i = 4 * s + g;
            const bool i_live = i < n;
            double a = 0.0, b = 0.0;
            if (i_live && j_live) a = wrow[i];
            if (i_live && q_live) b = xcol[(long)i * inner];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        if (q_live) {
            double *ycol = Y + (o * m) * inner + q;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int jj = jt * 16 + g + 4 * v;
                if (jj < m) {
                    const int hv = hot ? hot[jj] : -1;
                    double val = acc[v];
                    if (hv >= 0) val = xcol[(long)hv * inner];
                    ycol[(long)jj * inner] = val;
                }
            }
        }
    }
}

// inner == 1: Y[o, j] = sum_i X[o, i] W[j, i].  tiles = OT * MT, tile t = ot * MT + jt.  WLDS: the workgroup first copies
// W into LDS, rows ldw doubles apart (ldw odd: the 16 rows a k-step reads fall into different banks).
template <bool WLDS>
static __global__ __launch_bounds__(PCX_MP_THREADS) void k_mode_product_mfma_last(const double *__restrict__ X,
                                                                                  const double *__restrict__ W,
                                                                                  double *__restrict__ Y, long outer, int n,
                                                                                  int m, int MT, long tiles, int ldw,
                                                                                  const int *__restrict__ hot) {
    extern __shared__ double mp_w_lds[];
    if (WLDS) {
        const long cnt = (long)m * n;
        for (long e = threadIdx.x; e < cnt; e += PCX_MP_THREADS) mp_w_lds[(e / n) * ldw + e % n] = W[e];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int c = lane & 15, g = lane >> 4;
    const int KS = (n + 3) >> 2;
    for (long t = (long)blockIdx.x * PCX_MP_WAVES + (threadIdx.x >> 6); t < tiles; t += (long)gridDim.x * PCX_MP_WAVES) {
        const int jt = (int)(t % MT);
        const long ot = t / MT;
        const long o = ot * 16 + c;           // row of X this lane feeds (A operand)
        const int j = jt * 16 + c;            // row of W = column of W^T this lane feeds (B operand) and stores
        const bool o_live = o < outer, j_live = j < m;
        const double *xrow = X + (o_live ? o : 0) * n;
        const double *wrow = WLDS ? mp_w_lds + (long)(j_live ? j : 0) * ldw : W + (long)(j_live ? j : 0) * n;
        pcx_d4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int s = 0; s < KS; ++s) {
            const int i = 4 * s + g;
            const bool i_live = i < n;
            double a = 0.0, b = 0.0;
            if (i_live && o_live) a = xrow[i];
            if (i_live && j_live) b = wrow[i];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        if (j_live) {
            const int hv = hot ? hot[j] : -1;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const long oo = ot * 16 + g + 4 * v;
                if (oo < outer) Y[oo * m + j] = hv >= 0 ? X[oo * n + hv] : acc[v];
            }
        }
    }
}
