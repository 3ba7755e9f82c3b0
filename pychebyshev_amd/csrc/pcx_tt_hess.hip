// pcx_tt_hess.hip -- C ABI of libpcx_hip.so (see include/pcx.h): value, gradient and full Hessian of a tensor train
// from one right sweep and one blocked left sweep per row, batched.  gfx950 only.

#include "pcx_internal.h"
#include "tt_hess_kernels.h"

static int tt_hess_columns(int d) { return 1 + d + d * d; }

template <int RCAP, int NJ>
static int tt_hess_launch_lpp(const TTBoxView &v, size_t lds, long blocks, int B, const double *d_pts, long N, double *d_out,
                              hipStream_t st) {
    const auto kernel = k_tt_hess_lpp<RCAP, NJ>;
    static std::atomic<unsigned long long> lifted{0};
    if (const int rc = tt_grad_lift_lds((const void *)kernel, lifted, v.device, lds)) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(PCX_LPP_WG), lds, st, v.d_lpp_tab, v.plan->dims.d, v.plan->rmax, B,
                       v.d_lpp_img, d_pts, d_out, N);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

// N device-resident points -> d_out[p * C + column] at block size B (checked by tt_hess_args); queued on st, not awaited.
// Caller holds the handle's mutex.
static int tt_hess_launch(const TTBoxView &v, int B, const double *d_pts, long N, double *d_out, hipStream_t st) {
    if (N == 0) return PCX_OK;
    int rc;
    if (v.d_lpp_img) {
        long blocks;
        if ((rc = tt_grad_lpp_blocks(N, &blocks))) return rc;
        const size_t lds = tt_hess_lds_bytes(*v.plan, true, B);
        tt_lpp_for_model(v.plan->lppCap, v.plan->lpp_nodes, [&](auto rcap, auto nj) {
            rc = tt_hess_launch_lpp<decltype(rcap)::value, decltype(nj)::value>(v, lds, blocks, B, d_pts, N, d_out, st);
        });
        return rc;
    }
    const TTHessGeneric hd{tt_grad_generic_model(v), B};
    size_t lds;
    if ((rc = tt_wave_lds((const void *)k_tt_hess_generic, v, tt_hess_generic_doubles(hd.gd.rsum, v.plan->rmax, v.plan->nmax, B),
                          "Hessian", "sum of ranks + 2 rank + 3 nodes + B (2 rank + 192)", &lds)))
        return rc;
    const long blocks = tt_grad_generic_blocks(N);
    hipLaunchKernelGGL(k_tt_hess_generic, dim3((unsigned)blocks), dim3(256), lds, st, hd, v.d_cores, d_pts, d_out, N);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

// the checks both entry points share, all before any launch; *B = the block size to run at; *go = false: a successful
// no-op (N = 0)
static int tt_hess_args(pcx_tt *h, TTBoxView *v, const void *pts, int64_t N, int block, const void *out, int *B, bool *go) {
    *go = false;
    int rc = tt_box_view(h, v);
    if (rc) return rc;
    if (N < 0) return fail(PCX_ERR_INVALID, "bad N");
    const int limit = tt_hess_block_limit(v->plan->dims.d);
    if (block < 0 || block > limit) return fail(PCX_ERR_INVALID, "block = %d is neither 0 nor in 1 .. %d", block, limit);
    if (N > 0 && (!pts || !out)) return fail(PCX_ERR_INVALID, "NULL buffer");
    bool lane;
    if ((rc = tt_grad_form(*v, &lane))) return rc;
    const int fits = tt_hess_block_max(*v->plan, lane);
    if (block > fits || fits == 0)
        return fail(PCX_ERR_UNSUPPORTED, "block = %d: the Hessian launch takes %zu bytes of LDS a workgroup, above %d (largest block that fits: %d)",
                    block ? block : 1, tt_hess_lds_bytes(*v->plan, lane, block ? block : 1), PCX_TT_GRAD_LDS_MAX, fits);
    *B = block ? block : tt_hess_block_plan(*v->plan, lane);
    *go = N > 0;
    return PCX_OK;
}

extern "C" int pcx_tt_hess_info(pcx_tt *h, int32_t *info_out) {
    PCX_API_BEGIN
    TTBoxView v;
    int rc = tt_box_view(h, &v);
    if (rc) return rc;
    if (!info_out) return fail(PCX_ERR_INVALID, "NULL info_out");
    bool lane;
    if ((rc = tt_grad_form(v, &lane))) return rc;
    const int fits = tt_hess_block_max(*v.plan, lane);
    const int B = fits ? tt_hess_block_plan(*v.plan, lane) : 0;
    info_out[0] = lane ? 1 : 2;
    info_out[1] = B;
    info_out[2] = (int32_t)tt_hess_lds_bytes(*v.plan, lane, B ? B : 1);
    info_out[3] = fits;
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_tt_hess_batch_dev(pcx_tt *h, const double *d_pts, int64_t N, int block, double *d_out, void *stream) {
    PCX_API_BEGIN
    TTBoxView v;
    int B;
    bool go;
    const int rc = tt_hess_args(h, &v, d_pts, N, block, d_out, &B, &go);
    if (rc || !go) return rc;
    HIP_TRY(hipSetDevice(v.device));
    std::lock_guard<std::mutex> lk(*v.mu);
    return tt_hess_launch(v, B, d_pts, (long)N, d_out, stream ? (hipStream_t)stream : v.stream);
    PCX_API_END
}

extern "C" int pcx_tt_hess_batch(pcx_tt *h, const double *pts, int64_t N, int block, double *out) {
    PCX_API_BEGIN
    TTBoxView v;
    int B;
    bool go;
    const int rc = tt_hess_args(h, &v, pts, N, block, out, &B, &go);
    if (rc || !go) return rc;
    HIP_TRY(hipSetDevice(v.device));
    std::lock_guard<std::mutex> lk(*v.mu);
    // as pcx_tt_grad_batch, the piece scaled by (1 + 2 d) / C and rounded down to whole workgroups: a staging slot is
    // never larger than gradient_batch(second=True)'s for the same d
    const int d = v.plan->dims.d;
    const int C = tt_hess_columns(d);
    const int64_t chunk = std::max<int64_t>(64, ((int64_t)(1 << 18) * (1 + 2 * d) / C) / 64 * 64);
    return stage_host_batch(*v.stage, v.device, v.stream, pts, N, d, C, out, StagePlan{chunk, chunk, N > chunk, true},
                            [&](int, hipStream_t st, const double *dp, long cnt, double *dout) {
                                return tt_hess_launch(v, B, dp, cnt, dout, st);
                            });
    PCX_API_END
}
