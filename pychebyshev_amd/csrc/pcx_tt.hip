// pcx_tt.hip -- C ABI of libpcx_hip.so (see include/pcx.h): tensor-train evaluation.  gfx950 only.

#include <memory>

#include "pcx_internal.h"
#include "tt_plan.h"
#include "tt_kernels.h"
#include "tt_lpp_kernels.h"
#include "tt_fd_kernels.h"

// ---------------------------------------------------------------------------------
// tensor-train handle: the plan (tt_plan.h), what was uploaded for it, and the state launches fill lazily
// ---------------------------------------------------------------------------------
struct pcx_tt {
    int device = 0;
    hipStream_t stream = nullptr;
    TTPlan plan{};
    TTImages up{};               // which of the plan's optional images exist: one that failed to allocate only switches its form off
    double *d_frag = nullptr;    // 16x16x4 direct form: packed cores
    double *d_last = nullptr;    // last core [a][j] (right rank 1), zero-padded to 4 RC rows, for the VALU tail
    double *d_img = nullptr;     // W-first image
    double *d_img4 = nullptr;    // 4x4x4 image
    double *d_lpp_img = nullptr; // lane-per-point image [b][a][j] + per-dim table
    TTLppDim *d_lpp_tab = nullptr;
    double *d_cores = nullptr;   // plain cores: the generic kernel's, and the wave-per-row kernels' of every model without a lane-per-point image
    double *d_rinv = nullptr;    // 1 / j, j = 1 .. nmax + 1, for the wave-per-row box kernel (uploaded on its first launch)
    long w_resident = 0;         // workgroups of the W-first kernel the device keeps resident (lazy)
    long d4_resident = 0;        // ... of the 4x4x4 kernel
    int variant = 0;             // 0 auto, 1 direct form (16x16x4), 2 W-first form, 3 direct form (4x4x4), 4 lane per point
    std::mutex mu;
    HostStage stage;      // host-pointer batches
    Scratch s_fd_batch, s_fd_vals;   // finite-difference stencil batch and its values (models off the lane-per-point kernel)
};

extern "C" int pcx_tt_destroy(pcx_tt *h) {
    PCX_API_BEGIN
    if (!h) return PCX_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    (void)hipFree(h->d_frag);
    (void)hipFree(h->d_last);
    (void)hipFree(h->d_img);
    (void)hipFree(h->d_img4);
    (void)hipFree(h->d_lpp_img);
    (void)hipFree(h->d_lpp_tab);
    (void)hipFree(h->d_cores);
    (void)hipFree(h->d_rinv);
    h->stage.release();
    h->s_fd_batch.release(); h->s_fd_vals.release();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return PCX_OK;
    PCX_API_END
}

// a host array as a device buffer the handle owns from here on
template <typename T>
static int tt_upload(T *&dst, const T *src, size_t count) {
    HIP_TRY(hipMalloc((void **)&dst, count * sizeof(T)));
    HIP_TRY(hipMemcpy(dst, src, count * sizeof(T), hipMemcpyHostToDevice));
    return PCX_OK;
}

// an optional image: false (and nothing pending in the runtime's error state) when it could not be allocated or copied
template <typename T>
static bool tt_upload_optional(T *&dst, const std::vector<T> &v) {
    const bool ok = hipMalloc((void **)&dst, v.size() * sizeof(T)) == hipSuccess &&
                    hipMemcpy(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    return ok;
}

// validate and plan (tt_make_plan: pcx_tt_plan.hip decides everything about the launches), upload.  The handle owns
// every device allocation from the moment it is made: whatever path leaves early, pcx_tt_destroy frees it.
extern "C" int pcx_tt_create(int device, int d, const int32_t *n_nodes, const int32_t *ranks,
                             const double *lo, const double *hi, const double *cores_cat,
                             const int32_t *dim_order, pcx_tt **out) {
    PCX_API_BEGIN
    if (!out) return fail(PCX_ERR_INVALID, "out is NULL");
    *out = nullptr;
    std::unique_ptr<pcx_tt, int (*)(pcx_tt *)> h(new (std::nothrow) pcx_tt(), pcx_tt_destroy);
    if (!h) return fail(PCX_ERR_NOMEM, "out of host memory");
    // missing cores are reported where the planner reports any missing model array
    int rc = tt_make_plan(d, cores_cat ? n_nodes : nullptr, ranks, lo, hi, dim_order, h->plan);
    if (rc || (rc = use_device(device))) return rc;
    h->device = device;
    const TTPlan &p = h->plan;
    HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    if ((rc = tt_upload(h->d_cores, cores_cat, (size_t)p.core_total))) return rc;
    if (p.generic) {
        *out = h.release();
        return PCX_OK;
    }
    HIP_TRY(hipMalloc((void **)&h->d_frag, p.frag_total * sizeof(double)));
    const std::vector<double> last = tt_pack_last_core(p, cores_cat);
    if ((rc = tt_upload(h->d_last, last.data(), last.size()))) return rc;
    for (int k = 0; k < d; ++k) {
        long cnt = (long)p.dims.n[k] * p.rk.rc[k] * p.rk.rt[k] * 64;
        hipLaunchKernelGGL(k_tt_pack_core, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream,
                           h->d_cores + p.coff[k], h->d_frag + p.dims.frag_off[k], p.ranks[k], p.dims.n[k],
                           p.ranks[k + 1], p.rk.rc[k], p.rk.rt[k]);
    }
    if (p.wR) {
        h->up.wfirst = hipMalloc((void **)&h->d_img, p.wplan.total * sizeof(double)) == hipSuccess;
        if (!h->up.wfirst) (void)hipGetLastError();
    }
    for (int k = 0; k < d && h->up.wfirst; ++k) {
        const int last_dim = (k == d - 1), R = p.wR, ks = p.wplan.ks, nt = p.wplan.ntiles[k];
        long cnt = last_dim ? (long)R * 4 * ks : (long)ks * nt * 64;
        dim3 grid((unsigned)((cnt + 255) / 256)), block(256);
        double *dst = h->d_img + p.wplan.lds_off[k];
        const double *src = h->d_cores + p.coff[k];
        if (R == 4) hipLaunchKernelGGL(k_tt_pack_wfirst<4>, grid, block, 0, h->stream, src, dst, p.ranks[k], p.dims.n[k], p.ranks[k + 1], ks, nt, last_dim);
        else if (R == 8) hipLaunchKernelGGL(k_tt_pack_wfirst<8>, grid, block, 0, h->stream, src, dst, p.ranks[k], p.dims.n[k], p.ranks[k + 1], ks, nt, last_dim);
        else hipLaunchKernelGGL(k_tt_pack_wfirst<12>, grid, block, 0, h->stream, src, dst, p.ranks[k], p.dims.n[k], p.ranks[k + 1], ks, nt, last_dim);
    }
    if (p.d4RA) h->up.d4 = tt_upload_optional(h->d_img4, tt_pack_d4_image(p, cores_cat));
    if (p.lppCap)
        h->up.lpp = tt_upload_optional(h->d_lpp_img, tt_pack_lpp_image(p, cores_cat)) && tt_upload_optional(h->d_lpp_tab, tt_lpp_table(p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->up.lpp) {            // the pack kernels are done; every entry point of such a model reads the lane-per-point image
        (void)hipFree(h->d_cores);
        h->d_cores = nullptr;
    }
    *out = h.release();
    return PCX_OK;
    PCX_API_END
}

// The workgroups of `kern` (256 threads, `lds` bytes) the device keeps resident, counted on the first launch.
static int tt_resident(const void *kern, size_t lds, int device, long *resident) {
    if (*resident) return PCX_OK;
    if (lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, lds));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    *resident = std::max(1, per_cu) * std::max(1, prop.multiProcessorCount);
    return PCX_OK;
}

template <int R, int KS, int NT>
static int tt_launch_wfirst(pcx_tt *h, const double *d_pts, long N, double *d_out, hipStream_t st) {
    auto kern = k_tt_eval_wfirst<R, KS, NT>;
    const size_t lds = tt_wfirst_lds_bytes(h->plan, NT);
    const int rc = tt_resident((const void *)kern, lds, h->device, &h->w_resident);
    if (rc) return rc;
    long per_wg = 4L * 16 * NT;
    long batches = (N + per_wg - 1) / per_wg;
    // persistent workgroups, four per resident slot (a second and third wave of workgroups
    // evens out the tail: +4 % over exactly-resident on 10^7 points), each walks a grid-stride
    // range of batches so the LDS image is loaded once per workgroup
    long blocks = std::min<long>(batches, h->w_resident * 4);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, st, h->plan.dims, h->plan.wplan, h->d_img, d_pts, d_out, N);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

template <int RA>
static int tt_launch_d4(pcx_tt *h, const double *d_pts, long N, double *d_out, hipStream_t st) {
    auto kern = k_tt_eval_d4<RA>;
    const size_t lds = tt_d4_lds_bytes(h->plan);
    const int rc = tt_resident((const void *)kern, lds, h->device, &h->d4_resident);
    if (rc) return rc;
    long batches = (N + 63) / 64;
    // persistent workgroups, four per resident slot: later rounds of workgroups even out the tail
    static const int mult = [] { const char *e = getenv("PCX_D4_MULT"); return e ? std::max(1, atoi(e)) : 4; }();
    long blocks = std::min<long>(batches, h->d4_resident * mult);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, st, h->plan.dims, h->plan.d4plan, h->d_img4, d_pts, d_out, N);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

template <int R, int NT>
static int tt_launch_wfirst_ks(pcx_tt *h, const double *d_pts, long N, double *d_out, hipStream_t st) {
    switch (h->plan.wplan.ks) {
    case 1: return tt_launch_wfirst<R, 1, NT>(h, d_pts, N, d_out, st);
    case 2: return tt_launch_wfirst<R, 2, NT>(h, d_pts, N, d_out, st);
    case 3: return tt_launch_wfirst<R, 3, NT>(h, d_pts, N, d_out, st);
    case 4: return tt_launch_wfirst<R, 4, NT>(h, d_pts, N, d_out, st);
    case 5: return tt_launch_wfirst<R, 5, NT>(h, d_pts, N, d_out, st);
    case 6: return tt_launch_wfirst<R, 6, NT>(h, d_pts, N, d_out, st);
    case 7: return tt_launch_wfirst<R, 7, NT>(h, d_pts, N, d_out, st);
    case 8: return tt_launch_wfirst<R, 8, NT>(h, d_pts, N, d_out, st);
    }
    return fail(PCX_ERR_UNSUPPORTED, "W-first TT kernel: %d k-steps not instantiated", h->plan.wplan.ks);
}

static int tt_launch(pcx_tt *h, const double *d_pts, long N, double *d_out, hipStream_t st) {
    if (N == 0) return PCX_OK;
    const TTPlan &p = h->plan;
    const int form = tt_auto_variant(p, h->up, h->variant);
    if (form < 0) return form;
    if (form == 0) {
        const size_t lds = tt_generic_lds_bytes(p);
        if (lds > 64 * 1024)
            HIP_TRY(hipFuncSetAttribute((const void *)k_tt_eval_generic, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        long blocks = std::min<long>((N + 3) / 4, 256L * 8);
        hipLaunchKernelGGL(k_tt_eval_generic, dim3((unsigned)blocks), dim3(256), lds, st, p.dims, p.gi, h->d_cores, d_pts, d_out, N);
        HIP_TRY(hipGetLastError());
        return PCX_OK;
    }
    if (form == 4) {
        const long blocks = (N + PCX_LPP_WG - 1) / PCX_LPP_WG;
        if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
        tt_lpp_for_model(p.lppCap, p.lpp_nodes, [&](auto rcap, auto nj) {
            hipLaunchKernelGGL((k_tt_eval_lpp<decltype(rcap)::value, decltype(nj)::value>), dim3((unsigned)blocks), dim3(PCX_LPP_WG),
                               tt_lpp_lds_bytes(p), st, h->d_lpp_tab, p.dims.d, h->d_lpp_img, d_pts, d_out, N);
        });
        HIP_TRY(hipGetLastError());
        return PCX_OK;
    }
    if (form == 3) {
        if (p.d4RA == 1) return tt_launch_d4<1>(h, d_pts, N, d_out, st);
        if (p.d4RA == 2) return tt_launch_d4<2>(h, d_pts, N, d_out, st);
        return tt_launch_d4<3>(h, d_pts, N, d_out, st);
    }
    if (form == 2) {
        if (p.wR == 4) return tt_launch_wfirst_ks<4, 4>(h, d_pts, N, d_out, st);
        if (p.wR == 8) return tt_launch_wfirst_ks<8, 1>(h, d_pts, N, d_out, st);
        return tt_launch_wfirst_ks<12, 1>(h, d_pts, N, d_out, st);
    }
    auto go = [&](auto kern, int nt) -> int {
        long per_wg = 4L * 16 * nt;
        long blocks = (N + per_wg - 1) / per_wg;
        if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), tt_direct_lds_bytes(p, nt), st, p.dims, p.rk, h->d_frag, h->d_last,
                           p.last_lds_doubles ? p.rl_last : 0, d_pts, d_out, N);
        HIP_TRY(hipGetLastError());
        return PCX_OK;
    };
    if (p.cls == 0) {
        if (p.rmax <= 4) return go(k_tt_eval_mfma<1, 1, 4>, 4);
        if (p.rmax <= 8) return go(k_tt_eval_mfma<2, 1, 4>, 4);
        if (p.rmax <= 12) return go(k_tt_eval_mfma<3, 1, 4>, 4);
        return go(k_tt_eval_mfma<4, 1, 4>, 4);
    }
    if (p.cls == 1) return go(k_tt_eval_mfma<8, 2, 2>, 2);
    return go(k_tt_eval_mfma<16, 4, 1>, 1);
}

extern "C" int pcx_tt_eval_batch_dev(pcx_tt *h, const double *d_pts, int64_t N, double *d_out,
                                     void *stream) {
    PCX_API_BEGIN
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    if (N < 0) return fail(PCX_ERR_INVALID, "N < 0");
    if (N > 0 && (!d_pts || !d_out)) return fail(PCX_ERR_INVALID, "NULL device buffer");
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);      // tt_launch reads h->variant and fills the lazy residency counts
    return tt_launch(h, d_pts, (long)N, d_out, stream ? (hipStream_t)stream : h->stream);
    PCX_API_END
}

extern "C" int pcx_tt_eval_batch(pcx_tt *h, const double *pts, int64_t N, double *out) {
    PCX_API_BEGIN
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    if (N < 0) return fail(PCX_ERR_INVALID, "N < 0");
    if (N > 0 && (!pts || !out)) return fail(PCX_ERR_INVALID, "NULL buffer");
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    const int d = h->plan.dims.d;
    // The path is transfer-bound (48 .. 88 bytes per point against ~0.1 ns of kernel): pieces of ~10 MB of coordinates alternate
    // between two staging slots on two streams, so the upload of piece i+1 runs while piece i is evaluated and piece
    // i-1 is downloaded (both PCIe directions busy; the downloads are issued by a helper thread, see stage_host_batch).  From page-locked caller memory (pcx_host_register, or the `pin`
    // flag of pcx_tt_group_eval_batch) the copies are asynchronous DMA; from pageable memory the driver stages them.
    // ~10 MB of coordinates per piece for batches of a few pieces (N = 10^6: 1.08 -> 1.00 ms), up to ~40 MB for long ones
    // (N = 10^7: 8.9 ms with 40 MB pieces against 9.4 ms with 10 MB pieces)
    const int64_t piece_lo = std::max<int64_t>(65536, (((int64_t)10 << 20) / (d * 8)) & ~(int64_t)65535);
    const int64_t kTTPipePoints = std::min<int64_t>(4 * piece_lo, std::max<int64_t>(piece_lo, (N / 8) & ~(int64_t)65535));
    const bool piped = N >= 2 * kTTPipePoints;
    const int64_t chunk = piped ? kTTPipePoints : kChunkPoints;
    return stage_host_batch(h->stage, h->device, h->stream, pts, N, d, 1, out, StagePlan{chunk, chunk, piped, true},
                            [&](int, hipStream_t st, const double *dp, long cnt, double *dout) {
                                return tt_launch(h, dp, cnt, dout, st);
                            });
    PCX_API_END
}

// ---------------------------------------------------------------------------------
// Finite-difference Greeks, batched (reference eval_multi + _fd_*, tensor_train.py:2267-2463; tt_fd_kernels.h)
// ---------------------------------------------------------------------------------
// derivs: m x d orders in the USER's dimension order (as ChebyshevTT.eval_multi takes them); the rules run in the
// storage frame: storage dimension k is user column dims.col[k].
static int tt_fd_plan(const pcx_tt *h, const int32_t *derivs, int m, std::vector<TTFdSpec> &specs) {
    const int d = h->plan.dims.d;
    specs.assign((size_t)m, TTFdSpec{});
    for (int s = 0; s < m; ++s) {
        TTFdSpec &sp = specs[(size_t)s];
        sp.nact = 0;
        sp.nleaf = 1;
        for (int k = 0; k < d; ++k) {
            const int o = derivs ? derivs[(size_t)s * d + h->plan.dims.col[k]] : 0;
            if (o == 0) continue;
            if (o != 1 && o != 2) return fail(PCX_ERR_INVALID, "Derivative order %d not supported (use 1 or 2)", o);
            if (sp.nact == PCX_FD_MAX_ACTIVE)
                return fail(PCX_ERR_UNSUPPORTED, "more than %d differenced dimensions in one spec: evaluate the stencil on the host",
                            PCX_FD_MAX_ACTIVE);
            const int i = sp.nact++;
            sp.dim[i] = k;
            sp.order[i] = o;
            sp.col[i] = h->plan.dims.col[k];
            sp.lo[i] = h->plan.dims.lo[k];
            sp.hi[i] = h->plan.dims.hi[k];
            sp.h[i] = (h->plan.dims.hi[k] - h->plan.dims.lo[k]) * 1e-4;          // tensor_train.py:2324
            sp.need[i] = sp.h[i] * 1.5;                                 // :2331
            sp.nleaf *= o + 1;
        }
        sp.kind = sp.nact == 0 ? 0 : 1;
        if (sp.nact == 2 && sp.order[0] == 1 && sp.order[1] == 1) sp.kind = 2;       // :2413-2441, the 4-point mixed partial
    }
    return PCX_OK;
}

static bool tt_runs_lpp(const pcx_tt *h) {
    return tt_auto_variant(h->plan, h->up, h->variant) == 4;
}

// N device-resident points x m specs -> d_out[p * ostride + s]; queued on st, not awaited.  Caller holds h->mu.
static int tt_fd_launch(pcx_tt *h, const double *d_pts, long N, const std::vector<TTFdSpec> &specs, double *d_out,
                        long ostride, hipStream_t st) {
    if (N == 0) return PCX_OK;
    const int m = (int)specs.size(), d = h->plan.dims.d;
    for (int s0 = 0; s0 < m; s0 += PCX_FD_PACK) {
        TTFdPack pack;
        pack.m = std::min(PCX_FD_PACK, m - s0);
        pack.slots = 0;
        for (int s = 0; s < pack.m; ++s) {
            pack.s[s] = specs[(size_t)(s0 + s)];
            pack.s[s].slot0 = pack.slots;
            pack.slots += pack.s[s].nleaf;
        }
        if (tt_runs_lpp(h)) {
            const long blocks = (N + PCX_LPP_WG - 1) / PCX_LPP_WG;
            if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
            const int rmax = h->plan.rmax;
            const size_t lds = (size_t)(rmax + 3 * PCX_FD_MAX_ACTIVE + 1) * PCX_LPP_WG * sizeof(double);
            tt_lpp_for_model(h->plan.lppCap, h->plan.lpp_nodes, [&](auto rcap, auto nj) {
                hipLaunchKernelGGL((k_tt_fd_lpp<decltype(rcap)::value, decltype(nj)::value>), dim3((unsigned)blocks), dim3(PCX_LPP_WG),
                                   lds, st, h->d_lpp_tab, d, rmax, h->d_lpp_img, d_pts, d_out, N, ostride, (long)s0, pack);
            });
            HIP_TRY(hipGetLastError());
            continue;
        }
        // any other evaluation kernel: stencil batch in HBM, in pieces that keep it under ~256 MB
        const long piece = std::max<long>(4096, std::min<long>(N, (256L << 20) / ((long)pack.slots * d * 8)));
        int rc = h->s_fd_batch.reserve((size_t)pack.slots * piece * d * sizeof(double));
        if (rc) return rc;
        if ((rc = h->s_fd_vals.reserve((size_t)pack.slots * piece * sizeof(double)))) return rc;
        for (long p0 = 0; p0 < N; p0 += piece) {
            const long cnt = std::min(piece, N - p0);
            hipLaunchKernelGGL(k_tt_fd_points, dim3((unsigned)((cnt + 255) / 256), (unsigned)pack.slots), dim3(256), 0, st,
                               d_pts + (size_t)p0 * d, cnt, d, (double *)h->s_fd_batch.ptr, pack);
            HIP_TRY(hipGetLastError());
            rc = tt_launch(h, (const double *)h->s_fd_batch.ptr, (long)pack.slots * cnt, (double *)h->s_fd_vals.ptr, st);
            if (rc) return rc;
            hipLaunchKernelGGL(k_tt_fd_combine, dim3((unsigned)((cnt + PCX_LPP_WG - 1) / PCX_LPP_WG)), dim3(PCX_LPP_WG), 0, st,
                               (const double *)h->s_fd_vals.ptr, cnt, d_out + (size_t)p0 * ostride, ostride, (long)s0, pack);
            HIP_TRY(hipGetLastError());
        }
    }
    return PCX_OK;
}

extern "C" int pcx_tt_eval_multi_batch_dev(pcx_tt *h, const double *d_pts, int64_t N, const int32_t *derivs, int m,
                                           double *d_out, void *stream) {
    PCX_API_BEGIN
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    if (N < 0 || m < 1) return fail(PCX_ERR_INVALID, "bad N or m");
    if (N > 0 && (!d_pts || !d_out)) return fail(PCX_ERR_INVALID, "NULL device buffer");
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    std::vector<TTFdSpec> specs;
    int rc = tt_fd_plan(h, derivs, m, specs);
    if (rc) return rc;
    // the generic path stages through the handle's scratch: its launches must stay on the handle's own stream
    hipStream_t st = (stream && tt_runs_lpp(h)) ? (hipStream_t)stream : h->stream;
    if (stream && st != (hipStream_t)stream) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    rc = tt_fd_launch(h, d_pts, (long)N, specs, d_out, m, st);
    if (rc) return rc;
    if (stream && st != (hipStream_t)stream) HIP_TRY(hipStreamSynchronize(st));
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_tt_eval_multi_batch(pcx_tt *h, const double *pts, int64_t N, const int32_t *derivs, int m, double *out) {
    PCX_API_BEGIN
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    if (N < 0 || m < 1) return fail(PCX_ERR_INVALID, "bad N or m");
    if (N > 0 && (!pts || !out)) return fail(PCX_ERR_INVALID, "NULL buffer");
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    std::vector<TTFdSpec> specs;
    int rc = tt_fd_plan(h, derivs, m, specs);
    if (rc) return rc;
    // pieces of 2^18 points alternate between the two staging slots: the upload of piece i + 1 overlaps the kernel of
    // piece i (8 m bytes per point come back against 8 d going in; the kernel is (stencil points) chains per point)
    const int64_t chunk = 1 << 18;
    const bool two = N > chunk && tt_runs_lpp(h);        // the generic path's scratch is single
    return stage_host_batch(h->stage, h->device, h->stream, pts, N, h->plan.dims.d, m, out, StagePlan{chunk, chunk, two, true},
                            [&](int, hipStream_t st, const double *dp, long cnt, double *dout) {
                                return tt_fd_launch(h, dp, cnt, specs, dout, m, st);
                            });
    PCX_API_END
}

extern "C" int pcx_tt_group_eval_batch(pcx_tt *const *handles, int n_handles, const double *pts, int64_t N, double *out,
                                       int pin) {
    PCX_API_BEGIN
    if (!handles || n_handles < 1) return fail(PCX_ERR_INVALID, "no handles");
    for (int g = 0; g < n_handles; ++g) {
        if (!handles[g]) return fail(PCX_ERR_INVALID, "handle %d is NULL", g);
        if (handles[g]->plan.dims.d != handles[0]->plan.dims.d) return fail(PCX_ERR_INVALID, "handle %d holds a different model", g);
    }
    if (N < 0) return fail(PCX_ERR_INVALID, "N < 0");
    if (N > 0 && (!pts || !out)) return fail(PCX_ERR_INVALID, "NULL buffer");
    const int d = handles[0]->plan.dims.d;
    return fan_out_host(n_handles, handles[0]->device, pin, N, pts, (size_t)N * d * sizeof(double), out, (size_t)N * sizeof(double),
                        [&](int g, int64_t lo, int64_t cnt) { return pcx_tt_eval_batch(handles[g], pts + (size_t)lo * d, cnt, out + lo); });
    PCX_API_END
}

extern "C" int pcx_tt_set_kernel(pcx_tt *h, int variant) {
    PCX_API_BEGIN
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    if (variant < 0 || variant > 4) return fail(PCX_ERR_INVALID, "variant %d outside [0, 4]", variant);
    const int form = tt_auto_variant(h->plan, h->up, variant);
    if (form < 0) return form;
    std::lock_guard<std::mutex> lk(h->mu);
    h->variant = variant;
    return PCX_OK;
    PCX_API_END
}

int tt_handle_view(pcx_tt *h, int *device, TTDims *dims, hipStream_t *stream) {
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    *device = h->device;
    *dims = h->plan.dims;
    *stream = h->stream;
    return PCX_OK;
}

int tt_box_view(pcx_tt *h, TTBoxView *v) {
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    v->device = h->device;
    v->stream = h->stream;
    v->plan = &h->plan;
    v->d_lpp_img = h->up.lpp ? h->d_lpp_img : nullptr;
    v->d_lpp_tab = h->d_lpp_tab;
    v->d_cores = h->d_cores;
    v->d_rinv = &h->d_rinv;
    v->mu = &h->mu;
    v->stage = &h->stage;
    return PCX_OK;
}

extern "C" int pcx_tt_stream(pcx_tt *h, void **stream) {
    PCX_API_BEGIN
    if (!h || !stream) return fail(PCX_ERR_INVALID, "NULL argument");
    *stream = (void *)h->stream;
    return PCX_OK;
    PCX_API_END
}
