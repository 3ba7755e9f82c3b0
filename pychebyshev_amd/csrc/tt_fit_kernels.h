// tt_fit_kernels.h -- the normal equations of one ALS step of a tensor train on scattered samples (ChebyshevTT.fit_samples,
// pcx_tt_fit_normal; gfx950).
//
// At storage position k the design row of sample i is a_i = L_i (x) T (x) R_i in C order (a, j, b), P = rl n rr entries:
//     L_i = M_0 ... M_{k-1}   (1 x rl),      R_i = M_{k+1} ... M_{d-1}   (rr x 1),      T_j = T_j(t_k(x_ik)),  j < n
// with M_m the folded core of position m (tt_grad_kernels.h).  Wanted: G = sum_i a_i a_i^T (P x P) and b = sum_i y_i a_i.
//
//   k_ttf_interface   one wave per sample on the plain cores: the left sweep is the evaluation chain's (tt_wave_basis,
//                     tt_wave_left of tt_wave_kernels.h, the code k_tt_eval_generic runs), the right sweep
//                     k_tt_grad_generic's fold (lanes over the left rank a; that kernel holds it inline, so it is
//                     restated here as tt_fit_wave_right, not shared: DESIGN 3.20).  A sample's row of V (width W + 2,
//                     W = rl + n + rr) is L, T, R, then y_i and 1.0, so that the Gram kernels read column P of the
//                     augmented matrix [A | y] as (y * 1) * 1 through the same three loads as any other column.
//   k_ttf_gram_mfma   G' = [A | y]^T [A | y] on v_mfma_f64_16x16x4_f64 with the samples as K: a workgroup owns a 64 x 64
//                     block of G' (block row <= block column) over one chunk of samples, wave w the 16 rows 16 w .. and
//                     four 16 x 16 tiles; per k-step of four samples a lane forms its entry of the A operand and of
//                     the four B operands, (L[a] * T[j]) * R[b] each, from V.  32 accumulator registers.
//   k_ttf_gram_valu   the same blocks at 16 x 16, one output per lane, samples ascending: any P.
//   k_ttf_reduce      G'[p][q] = the chunks' partial sums added in ascending order, read at (min, max) so that both
//                     triangles carry the same bits; G, b and sum y^2 go to their outputs.
//
// The chunks are fixed by N and P alone (tt_fit_chunking), the order inside a chunk by the kernel: no atomics, equal
// input gives equal bits.  The partial Grams are padded to a multiple of 64 each way, so no store needs a bound; a padded
// column reads column P again and is never read back.  A sample past the chunk's end contributes +0.0 (a select, not
// a product: no 0 * inf).
#pragma once

#include "tt_wave_kernels.h"

#define TTF_THREADS 256
#define TTF_BLOCK 64          // rows and columns of G' a workgroup of k_ttf_gram_mfma owns
#define TTF_MIN_CHUNK 256     // samples per chunk at least (a multiple of 4: whole k-steps)
#define TTF_PARTIAL_DOUBLES (1L << 25)      // budget of the partial Grams: 256 MiB
#define TTF_MAX_CHUNKS 32768

struct TTFitDomain {
    int d;
    double lo[PCX_MAX_DIMS];
    double hi[PCX_MAX_DIMS];
};

// flags[0]: a coordinate is not finite; [1]: a value is not finite; [2 + k]: a coordinate of dimension k lies outside
// [lo, hi].  Every store writes 1: the race between lanes is over equal values.
static __global__ void __launch_bounds__(TTF_THREADS)
k_ttf_check(TTFitDomain dm, const double *__restrict__ pts, const double *__restrict__ y, long N, int *__restrict__ flags) {
    for (long i = (long)blockIdx.x * TTF_THREADS + threadIdx.x; i < N; i += (long)gridDim.x * TTF_THREADS) {
        const double v = y[i];
        if (!(v - v == 0.0)) flags[1] = 1;
        for (int k = 0; k < dm.d; ++k) {
            const double x = pts[i * dm.d + k];
            if (!(x - x == 0.0)) flags[0] = 1;
            else if (x < dm.lo[k] || x > dm.hi[k]) flags[2 + k] = 1;
        }
    }
}

// vout[a] = sum_j q[j] sum_b G[a][j][b] vin[b], the lanes over a (k_tt_grad_generic's right sweep); last: rr = 1, vin = (1.0)
__device__ __forceinline__ void tt_fit_wave_right(const double *G, int rl, int n, int rr, const double *q, const double *vin,
                                                  bool last, double *vout, int lane) {
    for (int a = lane; a < rl; a += 64) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) {
            const double *gp = G + ((long)a * n + j) * rr;
            double w = 0.0;
            if (last) w = gp[0];
            else
                for (int b = 0; b < rr; ++b) w = __builtin_fma(gp[b], vin[b], w);
            s = __builtin_fma(q[j], w, s);
        }
        vout[a] = s;
    }
}

// t = 2 (x - lo) / (hi - lo) - 1 with the division, as k_tt_eval_generic forms it: -1 and +1 exactly at the domain's ends
__device__ __forceinline__ double tt_fit_t(double x, double lo, double hi) { return 2.0 * (x - lo) / (hi - lo) - 1.0; }

// doubles of LDS per wave: two rank vectors the sweeps alternate between and one basis
__host__ __device__ static inline size_t tt_fit_interface_doubles(int rmax, int nmax) { return 2 * (size_t)rmax + nmax; }

// V[i] = (L_i, T, R_i, y_i, 1.0) at position k; storage-order points (column m belongs to position m)
static __global__ void __launch_bounds__(TTF_THREADS)
k_ttf_interface(TTWaveModel gi, TTFitDomain dm, const double *__restrict__ cores, const double *__restrict__ pts,
                const double *__restrict__ y, long N, int k, double *__restrict__ V) {
    extern __shared__ double lds_fit[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int d = gi.d;
    const int rl = gi.rank[k], rr = gi.rank[k + 1], n = gi.n[k];
    const long Wv = rl + n + rr + 2;
    double *v0 = lds_fit + (size_t)wave * tt_fit_interface_doubles(gi.rmax, gi.nmax);
    double *v1 = v0 + gi.rmax;
    double *q = v1 + gi.rmax;
    for (long p = (long)blockIdx.x * 4 + wave; p < N; p += (long)gridDim.x * 4) {
        const double *row = pts + p * d;
        double *o = V + p * Wv;
        double *va = v0, *vb = v1;
        if (lane == 0) va[0] = 1.0;
        for (int m = 0; m < k; ++m) {
            if (lane == 0) tt_wave_basis(tt_fit_t(row[m], dm.lo[m], dm.hi[m]), gi.n[m], q);
            tt_wave_left(cores + gi.coff[m], gi.rank[m], gi.n[m], gi.rank[m + 1], q, va, vb, lane);
            double *t = va; va = vb; vb = t;
        }
        for (int a = lane; a < rl; a += 64) o[a] = va[a];
        va = v0; vb = v1;
        if (lane == 0) va[0] = 1.0;
        for (int m = d - 1; m > k; --m) {
            if (lane == 0) tt_wave_basis(tt_fit_t(row[m], dm.lo[m], dm.hi[m]), gi.n[m], q);
            tt_fit_wave_right(cores + gi.coff[m], gi.rank[m], gi.n[m], gi.rank[m + 1], q, va, m == d - 1, vb, lane);
            double *t = va; va = vb; vb = t;
        }
        for (int b = lane; b < rr; b += 64) o[rl + n + b] = va[b];
        if (lane == 0) {
            tt_wave_basis(tt_fit_t(row[k], dm.lo[k], dm.hi[k]), n, q);
            o[rl + n + rr] = y[p];
            o[rl + n + rr + 1] = 1.0;
        }
        for (int j = lane; j < n; j += 64) o[rl + j] = q[j];
    }
}

// where column c of [A | y] finds its three factors in a row of V; a column past P reads column P (never read back)
struct TTFitCol { int oa, oj, ob; };
__device__ __forceinline__ TTFitCol tt_fit_col(int c, int rl, int n, int rr) {
    const int P = rl * n * rr, W = rl + n + rr;
    TTFitCol t;
    if (c >= P) { t.oa = W; t.oj = W + 1; t.ob = W + 1; return t; }
    const int b = c % rr, aj = c / rr;
    t.oa = aj / n;
    t.oj = rl + aj % n;
    t.ob = rl + n + b;
    return t;
}
__device__ __forceinline__ double tt_fit_entry(const double *row, const TTFitCol &t, bool live) {
#pragma clang fp contract(off)
    const double v = (row[t.oa] * row[t.oj]) * row[t.ob];
    return live ? v : 0.0;
}

// grid (TB * TB, chunks), TB = Ppad / 64: the block (I, J) = (x / TB, x % TB), I <= J, of chunk y
static __global__ void __launch_bounds__(TTF_THREADS)
k_ttf_gram_mfma(const double *__restrict__ V, int rl, int n, int rr, long N, long chunk, int Ppad,
                double *__restrict__ partial) {
    const int TB = Ppad / TTF_BLOCK;
    const int I = blockIdx.x / TB, J = blockIdx.x % TB;
    if (I > J) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, c16 = lane & 15;
    const long Wv = rl + n + rr + 2;
    const int i0 = I * TTF_BLOCK + 16 * wave, j0 = J * TTF_BLOCK;
    const TTFitCol ca = tt_fit_col(i0 + c16, rl, n, rr);
    TTFitCol cb[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) cb[nt] = tt_fit_col(j0 + 16 * nt + c16, rl, n, rr);
    const long s_lo = (long)blockIdx.y * chunk;
    const long s_hi = s_lo + chunk < N ? s_lo + chunk : N;
    pcx_d4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = (pcx_d4){0.0, 0.0, 0.0, 0.0};
    for (long s0 = s_lo; s0 < s_hi; s0 += 4) {
        const long s = s0 + g;
        const bool live = s < s_hi;
        const double *row = V + (live ? s : s_hi - 1) * Wv;
        const double a = tt_fit_entry(row, ca, live);
        double b[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) b[nt] = tt_fit_entry(row, cb[nt], live);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[nt], acc[nt], 0, 0, 0);
    }
    double *out = partial + (long)blockIdx.y * Ppad * Ppad;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int v = 0; v < 4; ++v) out[(long)(i0 + g + 4 * v) * Ppad + j0 + 16 * nt + c16] = acc[nt][v];
}

// grid (T * T, chunks), T = Ppad / 16: the 16 x 16 tile (I, J), I <= J, of chunk y; one output per lane
static __global__ void __launch_bounds__(TTF_THREADS)
k_ttf_gram_valu(const double *__restrict__ V, int rl, int n, int rr, long N, long chunk, int Ppad,
                double *__restrict__ partial) {
    const int T = Ppad / 16;
    const int I = blockIdx.x / T, J = blockIdx.x % T;
    if (I > J) return;
    const long Wv = rl + n + rr + 2;
    const int p = I * 16 + (threadIdx.x >> 4), q = J * 16 + (threadIdx.x & 15);
    const TTFitCol cp = tt_fit_col(p, rl, n, rr), cq = tt_fit_col(q, rl, n, rr);
    const long s_lo = (long)blockIdx.y * chunk;
    const long s_hi = s_lo + chunk < N ? s_lo + chunk : N;
    double acc = 0.0;
    for (long s = s_lo; s < s_hi; ++s) {
        const double *row = V + s * Wv;
        acc = __builtin_fma(tt_fit_entry(row, cp, true), tt_fit_entry(row, cq, true), acc);
    }
    partial[(long)blockIdx.y * Ppad * Ppad + (long)p * Ppad + q] = acc;
}

// one thread per (p, q) of the (P + 1) x (P + 1) augmented Gram; out = G (P * P), then b (P), then sum y^2
static __global__ void __launch_bounds__(TTF_THREADS)
k_ttf_reduce(const double *__restrict__ partial, int chunks, int Ppad, int P, double *__restrict__ out) {
    const long P1 = (long)P + 1;
    const long e = (long)blockIdx.x * TTF_THREADS + threadIdx.x;
    if (e >= P1 * P1) return;
    const int p = (int)(e / P1), q = (int)(e % P1);
    if (p == P && q < P) return;                       // b^T: b is taken from the last column
    const int lo = p < q ? p : q, hi = p < q ? q : p;
    const double *src = partial + (long)lo * Ppad + hi;
    double s = src[0];
    for (int c = 1; c < chunks; ++c) s += src[(long)c * Ppad * Ppad];
    if (q < P) out[(long)p * P + q] = s;
    else if (p < P) out[(long)P * P + p] = s;
    else out[(long)P * P + P] = s;
}

// ---- host side ----------------------------------------------------------------------------------------------------
// The chunks of N samples at Gram size P: as many as the partial Grams' budget holds, at most TTF_MAX_CHUNKS, of at
// least TTF_MIN_CHUNK samples, whole k-steps each but the last.  A function of N and P alone.
static inline void tt_fit_chunking(long N, int P, int *Ppad, long *chunk, int *chunks) {
    *Ppad = (P + 1 + TTF_BLOCK - 1) / TTF_BLOCK * TTF_BLOCK;
    const long cap = std::max<long>(1, std::min<long>(TTF_MAX_CHUNKS, TTF_PARTIAL_DOUBLES / ((long)*Ppad * *Ppad)));
    long c = std::max<long>(TTF_MIN_CHUNK, (N + cap - 1) / cap);
    c = (c + 3) / 4 * 4;
    *chunk = c;
    *chunks = (int)((N + c - 1) / c);
}
