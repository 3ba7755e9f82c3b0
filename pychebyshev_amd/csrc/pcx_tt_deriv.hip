// pcx_tt_deriv.hip -- C ABI of libpcx_hip.so (see include/pcx.h): analytic derivatives of a tensor train, batched.
// gfx950 only.

#include "pcx_internal.h"
#include "tt_deriv_kernels.h"

// derivs: m x d orders in the USER's dimension order; the kernels walk storage positions (position k reads user
// column dims.col[k]).  One pack per launch of up to PCX_DERIV_PACK specs.
static int tt_deriv_plan(const TTBoxView &v, const int32_t *derivs, int m, std::vector<TTDerivPack> &packs) {
    const TTDims &dims = v.plan->dims;
    const int d = dims.d;
    packs.assign(((size_t)m + PCX_DERIV_PACK - 1) / PCX_DERIV_PACK, TTDerivPack{});
    for (int s = 0; s < m; ++s) {
        unsigned int ord = 0;
        for (int k = 0; k < d; ++k) {
            const int o = derivs[(size_t)s * d + dims.col[k]];
            if (o < 0 || o > 2)
                return fail(PCX_ERR_INVALID, "Derivative order %d not supported (use 0, 1 or 2)", o);
            ord |= (unsigned int)o << (2 * k);
        }
        packs[(size_t)s / PCX_DERIV_PACK].ord[s % PCX_DERIV_PACK] = ord;
    }
    return PCX_OK;
}

// N device-resident points x m specs -> d_out[p * m + s]; queued on st, not awaited.  Caller holds the handle's mutex.
static int tt_deriv_launch(const TTBoxView &v, const std::vector<TTDerivPack> &packs, int m, const double *d_pts, long N,
                           double *d_out, hipStream_t st) {
    if (N == 0 || m == 0) return PCX_OK;
    const int d = v.plan->dims.d;
    if (v.d_lpp_img) {
        const long blocks = (N + PCX_LPP_WG - 1) / PCX_LPP_WG;
        if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
        const size_t lds = (size_t)v.plan->rmax * PCX_LPP_WG * sizeof(double);
        const TTLppDim *tab = v.d_lpp_tab;
        for (int s0 = 0; s0 < m; s0 += PCX_DERIV_PACK) {
            const TTDerivPack &pack = packs[(size_t)s0 / PCX_DERIV_PACK];
            const dim3 grid((unsigned)blocks, (unsigned)std::min(PCX_DERIV_PACK, m - s0));
            tt_lpp_for_model(v.plan->lppCap, v.plan->lpp_nodes, [&](auto rcap, auto nj) {
                hipLaunchKernelGGL((k_tt_deriv_lpp<decltype(rcap)::value, decltype(nj)::value>), grid, dim3(PCX_LPP_WG), lds, st, tab,
                                   d, pack, v.d_lpp_img, d_pts, d_out, N, m, s0);
            });
            HIP_TRY(hipGetLastError());
        }
        return PCX_OK;
    }
    if (!v.d_cores) return fail(PCX_ERR_UNSUPPORTED, "the handle holds neither a lane-per-point image nor plain cores");
    TTDerivGeneric gd{};
    gd.g = tt_wave_model(v);
    for (int k = 0; k < d; ++k) gd.col[k] = v.plan->dims.col[k];
    size_t lds;
    const int rc = tt_wave_lds((const void *)k_tt_deriv_generic, v, 2 * (size_t)v.plan->rmax + v.plan->nmax, "derivative", "2 rank + nodes", &lds);
    if (rc) return rc;
    const long blocks = std::min<long>((N + 3) / 4, 256L * 8);
    for (int s0 = 0; s0 < m; s0 += PCX_DERIV_PACK) {
        const dim3 grid((unsigned)blocks, (unsigned)std::min(PCX_DERIV_PACK, m - s0));
        hipLaunchKernelGGL(k_tt_deriv_generic, grid, dim3(256), lds, st, gd, packs[(size_t)s0 / PCX_DERIV_PACK], v.d_cores,
                           d_pts, d_out, N, m, s0);
        HIP_TRY(hipGetLastError());
    }
    return PCX_OK;
}

// the checks both entry points share; *go = false: a successful no-op (N = 0 or m = 0)
static int tt_deriv_args(pcx_tt *h, TTBoxView *v, const void *pts, int64_t N, const int32_t *derivs, int m, const void *out,
                         std::vector<TTDerivPack> &packs, bool *go) {
    *go = false;
    int rc = tt_box_view(h, v);
    if (rc) return rc;
    if (N < 0 || m < 0) return fail(PCX_ERR_INVALID, "bad N or m");
    if (m > 0 && !derivs) return fail(PCX_ERR_INVALID, "derivs is NULL");
    if ((rc = tt_deriv_plan(*v, derivs, m, packs))) return rc;
    if (N > 0 && m > 0 && (!pts || !out)) return fail(PCX_ERR_INVALID, "NULL buffer");
    *go = N > 0 && m > 0;
    return PCX_OK;
}

extern "C" int pcx_tt_deriv_batch_dev(pcx_tt *h, const double *d_pts, int64_t N, const int32_t *derivs, int m,
                                      double *d_out, void *stream) {
    PCX_API_BEGIN
    TTBoxView v;
    std::vector<TTDerivPack> packs;
    bool go;
    const int rc = tt_deriv_args(h, &v, d_pts, N, derivs, m, d_out, packs, &go);
    if (rc || !go) return rc;
    HIP_TRY(hipSetDevice(v.device));
    std::lock_guard<std::mutex> lk(*v.mu);
    return tt_deriv_launch(v, packs, m, d_pts, (long)N, d_out, stream ? (hipStream_t)stream : v.stream);
    PCX_API_END
}

extern "C" int pcx_tt_deriv_batch(pcx_tt *h, const double *pts, int64_t N, const int32_t *derivs, int m, double *out) {
    PCX_API_BEGIN
    TTBoxView v;
    std::vector<TTDerivPack> packs;
    bool go;
    const int rc = tt_deriv_args(h, &v, pts, N, derivs, m, out, packs, &go);
    if (rc || !go) return rc;
    HIP_TRY(hipSetDevice(v.device));
    std::lock_guard<std::mutex> lk(*v.mu);
    // as pcx_tt_eval_multi_batch: pieces of 2^18 points alternate between the two staging slots (8 m bytes per point
    // come back against 8 d going in; the kernel is m chains per point)
    const int64_t chunk = 1 << 18;
    return stage_host_batch(*v.stage, v.device, v.stream, pts, N, v.plan->dims.d, m, out, StagePlan{chunk, chunk, N > chunk, true},
                            [&](int, hipStream_t st, const double *dp, long cnt, double *dout) {
                                return tt_deriv_launch(v, packs, m, dp, cnt, dout, st);
                            });
    PCX_API_END
}
