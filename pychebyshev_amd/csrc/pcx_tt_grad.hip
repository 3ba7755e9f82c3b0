// pcx_tt_grad.hip -- C ABI of libpcx_hip.so (see include/pcx.h): value, gradient and Hessian diagonal of a tensor
// train in one forward-backward pass per row, batched.  gfx950 only.

#include "pcx_internal.h"
#include "tt_grad_kernels.h"

static int tt_grad_columns(int d, int second) { return 1 + (second ? 2 : 1) * d; }

template <int RCAP, int NJ, bool SECOND>
static int tt_grad_launch_lpp(const TTBoxView &v, size_t lds, long blocks, const double *d_pts, long N, double *d_out,
                              hipStream_t st) {
    const auto kernel = k_tt_grad_lpp<RCAP, NJ, SECOND>;
    static std::atomic<unsigned long long> lifted{0};
    if (const int rc = tt_grad_lift_lds((const void *)kernel, lifted, v.device, lds)) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(PCX_LPP_WG), lds, st, v.d_lpp_tab, v.plan->dims.d,
                       v.d_lpp_img, d_pts, d_out, N);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

// N device-resident points -> d_out[p * C + column]; queued on st, not awaited.  Caller holds the handle's mutex.
static int tt_grad_launch(const TTBoxView &v, int second, const double *d_pts, long N, double *d_out, hipStream_t st) {
    if (N == 0) return PCX_OK;
    const int d = v.plan->dims.d;
    bool lane;
    int rc = tt_grad_form(v, &lane);
    if (rc) return rc;
    if (lane) {
        long blocks;
        if ((rc = tt_grad_lpp_blocks(N, &blocks))) return rc;
        // a lane-per-point image has d <= 16 and ranks <= 16: 128 KiB at most, inside the 160 KiB of a workgroup
        const size_t lds = tt_grad_lpp_columns(v.plan->ranks, d, v.plan->rmax) * PCX_LPP_WG * sizeof(double);
        tt_lpp_for_model(v.plan->lppCap, v.plan->lpp_nodes, [&](auto rcap, auto nj) {
            constexpr int RCAP = decltype(rcap)::value, NJ = decltype(nj)::value;
            rc = second ? tt_grad_launch_lpp<RCAP, NJ, true>(v, lds, blocks, d_pts, N, d_out, st)
                        : tt_grad_launch_lpp<RCAP, NJ, false>(v, lds, blocks, d_pts, N, d_out, st);
        });
        return rc;
    }
    const TTGradGeneric gd = tt_grad_generic_model(v);
    const void *kernel = second ? (const void *)k_tt_grad_generic<true> : (const void *)k_tt_grad_generic<false>;
    size_t lds;
    if ((rc = tt_wave_lds(kernel, v, tt_grad_generic_doubles(gd.rsum, gd.g.rmax, gd.g.nmax), "gradient", "sum of ranks + 2 rank + 3 nodes", &lds)))
        return rc;
    const long blocks = tt_grad_generic_blocks(N);
    if (second) hipLaunchKernelGGL(k_tt_grad_generic<true>, dim3((unsigned)blocks), dim3(256), lds, st, gd, v.d_cores, d_pts, d_out, N);
    else hipLaunchKernelGGL(k_tt_grad_generic<false>, dim3((unsigned)blocks), dim3(256), lds, st, gd, v.d_cores, d_pts, d_out, N);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

// the checks both entry points share; *go = false: a successful no-op (N = 0)
static int tt_grad_args(pcx_tt *h, TTBoxView *v, const void *pts, int64_t N, int second, const void *out, bool *go) {
    *go = false;
    const int rc = tt_box_view(h, v);
    if (rc) return rc;
    if (N < 0) return fail(PCX_ERR_INVALID, "bad N");
    if (second != 0 && second != 1) return fail(PCX_ERR_INVALID, "second = %d is neither 0 nor 1", second);
    if (N > 0 && (!pts || !out)) return fail(PCX_ERR_INVALID, "NULL buffer");
    *go = N > 0;
    return PCX_OK;
}

extern "C" int pcx_tt_grad_batch_dev(pcx_tt *h, const double *d_pts, int64_t N, int second, double *d_out, void *stream) {
    PCX_API_BEGIN
    TTBoxView v;
    bool go;
    const int rc = tt_grad_args(h, &v, d_pts, N, second, d_out, &go);
    if (rc || !go) return rc;
    HIP_TRY(hipSetDevice(v.device));
    std::lock_guard<std::mutex> lk(*v.mu);
    return tt_grad_launch(v, second, d_pts, (long)N, d_out, stream ? (hipStream_t)stream : v.stream);
    PCX_API_END
}

extern "C" int pcx_tt_grad_batch(pcx_tt *h, const double *pts, int64_t N, int second, double *out) {
    PCX_API_BEGIN
    TTBoxView v;
    bool go;
    const int rc = tt_grad_args(h, &v, pts, N, second, out, &go);
    if (rc || !go) return rc;
    HIP_TRY(hipSetDevice(v.device));
    std::lock_guard<std::mutex> lk(*v.mu);
    // as pcx_tt_deriv_batch: pieces of 2^18 points alternate between the two staging slots (d doubles in, C out per row)
    const int64_t chunk = 1 << 18;
    const int d = v.plan->dims.d;
    return stage_host_batch(*v.stage, v.device, v.stream, pts, N, d, tt_grad_columns(d, second), out,
                            StagePlan{chunk, chunk, N > chunk, true},
                            [&](int, hipStream_t st, const double *dp, long cnt, double *dout) {
                                return tt_grad_launch(v, second, dp, cnt, dout, st);
                            });
    PCX_API_END
}
