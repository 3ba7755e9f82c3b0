// sobol_kernels.h -- variance-based sensitivity (Sobol) indices of a Chebyshev coefficient tensor (gfx950).
//
// Replaces the per-element Python loop of the reference's _compute_sobol_from_coeffs (_sensitivity.py:67-140).
// Coefficient c_a of multi-index a, z = number of nonzero a_k: its energy is e = c^2 pi^d 2^-z (the product of the
// Chebyshev norms pi for degree 0 and pi/2 above).  The constant term (z = 0) is skipped; every other e is added to the
// variance, to first[k] when k is its only nonzero index and to total[k] for every nonzero a_k.
//
//   k_sobol_energy   one pass over the tensor: lanes of a wave read along the last axis (coalesced), the head
//                    indices are decomposed once per row; per-lane sums, then the wave (shuffles) and the block (LDS),
//                    one row of PCX_SOBOL_SLOTS(d) partials per block into a slab
//   k_sobol_finish   one block: adds the slab column by column, a wave per column, in a fixed order
//
// No atomics: the result is the same bit for bit from run to run for a given shape.
#pragma once

#include "pcx_common.h"

// slab row / result layout for d dimensions (PCX_SOBOL_SLOTS(d) doubles):
//   [0] variance, [1 + k] first[k], [1 + d + k] total[k], [2d + 1] count of non-finite coefficients
#define PCX_SOBOL_SLOTS(d) (2 * (d) + 2)
#define PCX_SOBOL_THREADS 256
#define PCX_SOBOL_UNROLL 4          // row groups a wave reads before it does their bookkeeping (loads in flight)
#define PCX_SOBOL_MAX_BLOCKS 2048
#define PCX_SOBOL_FINISH_THREADS 1024

struct SobolDims {
    int L;                    // nodes of the last dimension: the length of a row
    int lw;                   // log2(W), W = min(64, next power of two >= L) lanes per row
    long rows;                // prod n[0 : d-1]
    unsigned n[PCX_MAX_DIMS]; // nodes per dimension (only the d-1 head dimensions are read)
    double pid;               // pi^d as the reference forms it: a product of d factors pi
};

__device__ inline double sobol_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// D dimensions (the accumulators and the head loop unroll to exactly D), IT the integer type of the row
// decomposition: 32-bit while the row count fits (a 64-bit division is several times the work).
template <int D, typename IT>
__global__ __launch_bounds__(PCX_SOBOL_THREADS) void k_sobol_energy(const double *__restrict__ coef,
                                                                   double *__restrict__ slab, SobolDims sd) {
    constexpr int S = PCX_SOBOL_SLOTS(D);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W = 1 << sd.lw, G = 64 >> sd.lw;            // lanes per row, rows per wave pass
    const int sub = lane >> sd.lw, jl = lane & (W - 1);
    const long nw = (long)gridDim.x * (PCX_SOBOL_THREADS / 64);
    const long step = nw * G * PCX_SOBOL_UNROLL;
    double var = 0.0, bad = 0.0, fo[D], to[D];
#pragma unroll
    for (int k = 0; k < D; ++k) fo[k] = to[k] = 0.0;

    for (long base = ((long)blockIdx.x * (PCX_SOBOL_THREADS / 64) + wave) * G * PCX_SOBOL_UNROLL; base < sd.rows;
         base += step) {
        // the first element of each of the UNROLL rows this lane works on, read before any bookkeeping
        double v0[PCX_SOBOL_UNROLL];
#pragma unroll
        for (int u = 0; u < PCX_SOBOL_UNROLL; ++u) {
            const long r = base + (long)u * G + sub;
            v0[u] = (r < sd.rows && jl < sd.L) ? coef[r * sd.L + jl] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < PCX_SOBOL_UNROLL; ++u) {
            const long r = base + (long)u * G + sub;
            if (r >= sd.rows || jl >= sd.L) continue;
            // head multi-index of row r: which indices are nonzero, how many
            bool nz[D > 1 ? D - 1 : 1];
            int zh = 0;
            IT t = (IT)r;
#pragma unroll
            for (int k = D - 2; k >= 0; --k) {
                const IT q = t / (IT)sd.n[k];
                nz[k] = t != q * (IT)sd.n[k];
                zh += nz[k];
                t = q;
            }
            const double w0 = ldexp(sd.pid, -zh), w1 = ldexp(sd.pid, -zh - 1);   // element 0 of the row / the others
            const double *row = coef + r * sd.L;
            double e0 = 0.0, e1 = 0.0;
            double v = v0[u];
            bad += isfinite(v) ? 0.0 : 1.0;
            if (jl == 0) e0 = zh > 0 ? v * v * w0 : 0.0;   // the reference's c * c * norm
            else e1 = v * v * w1;
            for (int j = jl + W; j < sd.L; j += W) {
                v = row[j];
                bad += isfinite(v) ? 0.0 : 1.0;
                e1 += v * v * w1;
            }
            const double et = e0 + e1;
            var += et;
#pragma unroll
            for (int k = 0; k < D - 1; ++k) {
                to[k] += nz[k] ? et : 0.0;
                fo[k] += (nz[k] && zh == 1) ? e0 : 0.0;
            }
            to[D - 1] += e1;
            fo[D - 1] += zh == 0 ? e1 : 0.0;
        }
    }

    __shared__ double red[PCX_SOBOL_THREADS / 64][S];
    var = sobol_wave_sum(var);
    bad = sobol_wave_sum(bad);
    if (lane == 0) {
        red[wave][0] = var;
        red[wave][S - 1] = bad;
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double f = sobol_wave_sum(fo[k]), s = sobol_wave_sum(to[k]);
        if (lane == 0) {
            red[wave][1 + k] = f;
            red[wave][1 + D + k] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x < S) {
        double s = red[0][threadIdx.x];
        for (int w = 1; w < PCX_SOBOL_THREADS / 64; ++w) s += red[w][threadIdx.x];
        slab[(long)blockIdx.x * S + threadIdx.x] = s;
    }
}

// One block: out[s] = sum over the nblocks slab rows of column s.  Wave w takes columns w, w + 16, ...; its lanes
// stride over the rows, then a shuffle tree: a fixed order for a given nblocks.
__global__ __launch_bounds__(PCX_SOBOL_FINISH_THREADS) void k_sobol_finish(const double *__restrict__ slab, int nblocks,
                                                                          int nslots, double *__restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s = wave; s < nslots; s += PCX_SOBOL_FINISH_THREADS / 64) {
        double acc = 0.0;
        for (int b = lane; b < nblocks; b += 64) acc += slab[(long)b * nslots + s];
        acc = sobol_wave_sum(acc);
        if (lane == 0) out[s] = acc;
    }
}
