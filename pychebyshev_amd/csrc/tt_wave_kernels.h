// tt_wave_kernels.h -- what the wave-per-row tensor-train kernels share (gfx950): k_tt_eval_generic, k_tt_box_generic,
// k_tt_deriv_generic and k_tt_ladder_generic, the forms for every model without a lane-per-point image (rank > 16 or
// n > 16).  One wave walks one row through the chain
//     v <- v . (sum_j q_j G_k[:, j, :])
// on the plain cores G_k[a][j][b]: lane 0 forms a dimension's basis q in the wave's LDS slice, the lanes share the right
// rank (coalesced core reads from L2), v alternates between two rank vectors of that slice.  Wave-private LDS: the
// operations of one wave execute in order, so no step needs a barrier.  Four waves per workgroup.
#pragma once

#include "pcx_internal.h"
#include "tt_plan.h"

struct TTWaveModel {
    int d;
    int rank[PCX_MAX_DIMS + 1];
    int n[PCX_MAX_DIMS];
    long coff[PCX_MAX_DIMS];      // offset (doubles) of storage position k in the plain cores
    double lo[PCX_MAX_DIMS];
    double scale[PCX_MAX_DIMS];   // 2 / (hi - lo): s = fma(x - lo, scale, -1)
    int rmax, nmax;
};

// q[j] = T_j(s), j < n, by the forward recurrence (one lane)
__device__ __forceinline__ void tt_wave_basis(double s, int n, double *q) {
    double tp = 1.0, tc = s;
    const double x2 = s + s;
    for (int j = 0; j < n; ++j) {
        q[j] = tp;
        const double tn = __builtin_fma(x2, tc, -tp);
        tp = tc;
        tc = tn;
    }
}

// vout[b] = sum_a vin[a] sum_j q[j] G[a][j][b], the lanes over b
__device__ __forceinline__ void tt_wave_left(const double *G, int rl, int n, int rr, const double *q, const double *vin,
                                             double *vout, int lane) {
    for (int b = lane; b < rr; b += 64) {
        double s = 0.0;
        for (int a = 0; a < rl; ++a) {
            const double *ga = G + ((long)a * n) * rr + b;
            double w = 0.0;
            for (int j = 0; j < n; ++j) w = __builtin_fma(q[j], ga[(long)j * rr], w);
            s = __builtin_fma(vin[a], w, s);
        }
        vout[b] = s;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
static inline TTWaveModel tt_wave_model(const TTBoxView &v) {
    TTWaveModel gi{};
    const TTPlan &p = *v.plan;
    const int d = p.dims.d;
    gi.d = d;
    gi.rmax = p.rmax;
    gi.nmax = p.nmax;
    for (int k = 0; k < d; ++k) {
        gi.rank[k] = p.ranks[k];
        gi.n[k] = p.dims.n[k];
        gi.coff[k] = p.coff[k];
        gi.lo[k] = p.dims.lo[k];
        gi.scale[k] = p.dims.scale[k];
    }
    gi.rank[d] = p.ranks[d];
    return gi;
}

// *lds = the dynamic LDS of a launch whose waves take `per_wave` doubles each; refuses a model beyond the 160 KiB of a
// workgroup (`what` kernel, `budget` = per_wave spelled out) and lifts the kernel's 64 KiB default where needed
static inline int tt_wave_lds(const void *kernel, const TTBoxView &v, size_t per_wave, const char *what, const char *budget,
                              size_t *lds) {
    *lds = 4 * per_wave * sizeof(double);
    if (*lds > 160 * 1024)
        return fail(PCX_ERR_UNSUPPORTED, "TT rank %d with %d nodes exceeds the generic %s kernel's LDS budget (%s <= 5120)",
                    v.plan->rmax, v.plan->nmax, what, budget);
    if (*lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)*lds));
    return PCX_OK;
}
