// pcx_tt_fit.hip -- the fit session of ChebyshevTT.fit_samples: samples resident on the device, the normal equations of
// one ALS position (tt_fit_kernels.h) and the residual on the samples (the evaluation kernels of pcx_tt.hip, then the
// reduction of tt_als_kernels.h).  Everything but the evaluation runs on the null stream.
#include <memory>

#include "pcx_internal.h"
#include "tt_als_kernels.h"
#include "tt_fit_kernels.h"

#define TTF_MAX_RANK 256
#define TTF_MAX_NODES 256
#define TTF_GUARD_DOUBLES 256
#define TTF_MAX_V_DOUBLES (1LL << 31)      // the interface vectors of all samples: 16 GiB

struct pcx_tt_fit {
    int device = 0;
    int d = 0;
    long N = 0;
    int form = 0;
    double lo[PCX_MAX_DIMS], hi[PCX_MAX_DIMS];
    const double *d_pts = nullptr, *d_y = nullptr;      // the samples: own_* or the caller's
    DevBuf own_pts, own_y;
    Scratch cores, V, partial, out, eval, red, sums;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};      // around the three kernels of pcx_tt_fit_normal
    float ms[3] = {0.0f, 0.0f, 0.0f};
    std::mutex mu;
    ~pcx_tt_fit() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        cores.release(); V.release(); partial.release(); out.release(); eval.release(); red.release(); sums.release();
    }
};

namespace {

enum { TTF_FORM_AUTO = 0, TTF_FORM_VALU = 1, TTF_FORM_MFMA = 2 };

int check_session_args(int d, const double *lo, const double *hi, const void *pts, const void *values, int64_t N,
                       pcx_tt_fit **out) {
    if (!out) return fail(PCX_ERR_INVALID, "TT fit: out is NULL");
    *out = nullptr;
    if (d < 1 || d > PCX_MAX_DIMS) return fail(PCX_ERR_INVALID, "TT fit: d = %d outside [1, %d]", d, PCX_MAX_DIMS);
    if (!lo || !hi || !pts || !values) return fail(PCX_ERR_INVALID, "TT fit: NULL buffer");
    if (N < 1) return fail(PCX_ERR_INVALID, "TT fit: N = %lld samples, at least 1 needed", (long long)N);
    for (int k = 0; k < d; ++k)
        if (!(lo[k] < hi[k]) || !std::isfinite(lo[k]) || !std::isfinite(hi[k]))
            return fail(PCX_ERR_INVALID, "TT fit: domain of dimension %d is not lo < hi, both finite", k);
    if (N > PCX_TT_FIT_MAX_SAMPLES)
        return fail(PCX_ERR_UNSUPPORTED, "TT fit: more than %lld samples", (long long)PCX_TT_FIT_MAX_SAMPLES);
    return PCX_OK;
}

int new_session(int device, int d, const double *lo, const double *hi, int64_t N, std::unique_ptr<pcx_tt_fit> &s) {
    s.reset(new pcx_tt_fit());
    s->device = device;
    s->d = d;
    s->N = (long)N;
    for (int k = 0; k < d; ++k) { s->lo[k] = lo[k]; s->hi[k] = hi[k]; }
    return PCX_OK;
}

int check_model(const pcx_tt_fit *s, int d, const int32_t *n_nodes, const int32_t *ranks, const double *cores) {
    if (!s) return fail(PCX_ERR_INVALID, "TT fit: session is NULL");
    if (!n_nodes || !ranks || !cores) return fail(PCX_ERR_INVALID, "TT fit: NULL buffer");
    if (d != s->d) return fail(PCX_ERR_INVALID, "TT fit: the cores have %d dimensions, the session %d", d, s->d);
    if (ranks[0] != 1 || ranks[d] != 1) return fail(PCX_ERR_INVALID, "TT fit: boundary ranks must be 1");
    for (int k = 0; k < d; ++k) {
        if (n_nodes[k] < 1 || ranks[k + 1] < 1)
            return fail(PCX_ERR_INVALID, "TT fit: core %d has shape (%d, %d, %d)", k, (int)ranks[k], (int)n_nodes[k],
                        (int)ranks[k + 1]);
        if (ranks[k] > TTF_MAX_RANK || ranks[k + 1] > TTF_MAX_RANK || n_nodes[k] > TTF_MAX_NODES)
            return fail(PCX_ERR_UNSUPPORTED, "TT fit: core %d of shape (%d, %d, %d) exceeds ranks %d / %d nodes", k,
                        (int)ranks[k], (int)n_nodes[k], (int)ranks[k + 1], TTF_MAX_RANK, TTF_MAX_NODES);
    }
    return PCX_OK;
}

}  // namespace

extern "C" int pcx_tt_fit_destroy(pcx_tt_fit *s) {
    PCX_API_BEGIN
    if (!s) return PCX_OK;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    delete s;
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_tt_fit_create(int device, int d, const double *lo, const double *hi, const double *pts,
                                 const double *values, int64_t N, pcx_tt_fit **out) {
    PCX_API_BEGIN
    int rc = check_session_args(d, lo, hi, pts, values, N, out);
    if (rc) return rc;
    for (int64_t i = 0; i < N; ++i) {
        if (!std::isfinite(values[i])) return fail(PCX_ERR_INVALID, "TT fit: values contain NaN or Inf (sample %lld)", (long long)i);
        for (int k = 0; k < d; ++k) {
            const double x = pts[i * d + k];
            if (!std::isfinite(x)) return fail(PCX_ERR_INVALID, "TT fit: points contain NaN or Inf (sample %lld)", (long long)i);
            if (x < lo[k] || x > hi[k])
                return fail(PCX_ERR_INVALID, "TT fit: a coordinate of storage dimension %d lies outside its domain [%g, %g]", k, lo[k], hi[k]);
        }
    }
    if ((rc = use_device(device))) return rc;
    std::unique_ptr<pcx_tt_fit> s;
    if ((rc = new_session(device, d, lo, hi, N, s))) return rc;
    if ((rc = s->own_pts.alloc((size_t)N * d * sizeof(double)))) return rc;
    if ((rc = s->own_y.alloc((size_t)N * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpy(s->own_pts.p, pts, (size_t)N * d * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->own_y.p, values, (size_t)N * sizeof(double), hipMemcpyHostToDevice));
    s->d_pts = s->own_pts.as<double>();
    s->d_y = s->own_y.as<double>();
    *out = s.release();
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_tt_fit_create_dev(int device, int d, const double *lo, const double *hi, const double *d_pts,
                                     const double *d_values, int64_t N, pcx_tt_fit **out) {
    PCX_API_BEGIN
    int rc = check_session_args(d, lo, hi, d_pts, d_values, N, out);
    if (rc) return rc;
    if ((rc = use_device(device))) return rc;
    std::unique_ptr<pcx_tt_fit> s;
    if ((rc = new_session(device, d, lo, hi, N, s))) return rc;
    TTFitDomain dm{};
    dm.d = d;
    for (int k = 0; k < d; ++k) { dm.lo[k] = lo[k]; dm.hi[k] = hi[k]; }
    DevBuf dflags;
    int flags[2 + PCX_MAX_DIMS] = {0};
    if ((rc = dflags.alloc(sizeof(flags)))) return rc;
    HIP_TRY(hipMemset(dflags.p, 0, sizeof(flags)));
    const unsigned blocks = (unsigned)std::max<long>(1, std::min<long>((N + TTF_THREADS - 1) / TTF_THREADS, 4096));
    hipLaunchKernelGGL(k_ttf_check, dim3(blocks), dim3(TTF_THREADS), 0, 0, dm, d_pts, d_values, (long)N, dflags.as<int>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(flags, dflags.p, sizeof(flags), hipMemcpyDeviceToHost));
    if (flags[1]) return fail(PCX_ERR_INVALID, "TT fit: values contain NaN or Inf");
    if (flags[0]) return fail(PCX_ERR_INVALID, "TT fit: points contain NaN or Inf");
    for (int k = 0; k < d; ++k)
        if (flags[2 + k])
            return fail(PCX_ERR_INVALID, "TT fit: a coordinate of storage dimension %d lies outside its domain [%g, %g]", k, lo[k], hi[k]);
    s->d_pts = d_pts;
    s->d_y = d_values;
    *out = s.release();
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_tt_fit_set_form(pcx_tt_fit *s, int form) {
    PCX_API_BEGIN
    if (!s) return fail(PCX_ERR_INVALID, "TT fit: session is NULL");
    if (form < TTF_FORM_AUTO || form > TTF_FORM_MFMA) return fail(PCX_ERR_INVALID, "TT fit: form must be 0, 1 or 2, got %d", form);
    std::lock_guard<std::mutex> lk(s->mu);
    s->form = form;
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_tt_fit_normal(pcx_tt_fit *s, int d, const int32_t *n_nodes, const int32_t *ranks,
                                 const double *coeff_cores, int k, double *G_out, double *b_out) {
    PCX_API_BEGIN
    int rc = check_model(s, d, n_nodes, ranks, coeff_cores);
    if (rc) return rc;
    if (!G_out || !b_out) return fail(PCX_ERR_INVALID, "TT fit: NULL output");
    if (k < 0 || k >= d) return fail(PCX_ERR_INVALID, "TT fit: position %d outside [0, %d]", k, d - 1);
    const int rl = ranks[k], n = n_nodes[k], rr = ranks[k + 1];
    const long Pl = (long)rl * n * rr;
    if (Pl > PCX_TT_FIT_MAX_P)
        return fail(PCX_ERR_UNSUPPORTED, "TT fit: position %d has %lld unknowns (%d x %d x %d), more than %d", k, (long long)Pl,
                    rl, n, rr, PCX_TT_FIT_MAX_P);
    const int P = (int)Pl;
    const long Wv = rl + n + rr + 2;
    if (s->N > TTF_MAX_V_DOUBLES / Wv)
        return fail(PCX_ERR_UNSUPPORTED, "TT fit: %lld samples of %ld interface numbers exceed %lld doubles", (long long)s->N, Wv,
                    (long long)TTF_MAX_V_DOUBLES);
    HIP_TRY(hipSetDevice(s->device));
    std::lock_guard<std::mutex> lk(s->mu);
    const long N = s->N;

    TTWaveModel gi{};
    gi.d = d;
    long off = 0;
    for (int m = 0; m < d; ++m) {
        gi.rank[m] = ranks[m];
        gi.n[m] = n_nodes[m];
        gi.coff[m] = off;
        gi.lo[m] = s->lo[m];
        gi.scale[m] = 2.0 / (s->hi[m] - s->lo[m]);
        gi.rmax = std::max(gi.rmax, std::max((int)ranks[m], (int)ranks[m + 1]));
        gi.nmax = std::max(gi.nmax, (int)n_nodes[m]);
        off += (long)ranks[m] * n_nodes[m] * ranks[m + 1];
    }
    gi.rank[d] = ranks[d];
    TTFitDomain dm{};
    dm.d = d;
    for (int m = 0; m < d; ++m) { dm.lo[m] = s->lo[m]; dm.hi[m] = s->hi[m]; }

    int Ppad, chunks;
    long chunk;
    tt_fit_chunking(N, P, &Ppad, &chunk, &chunks);
    const size_t nout = (size_t)P * P + P + 1;
    if ((rc = s->cores.reserve((size_t)off * sizeof(double)))) return rc;
    if ((rc = s->V.reserve((size_t)N * Wv * sizeof(double)))) return rc;
    if ((rc = s->partial.reserve((size_t)chunks * Ppad * Ppad * sizeof(double)))) return rc;
    if ((rc = s->out.reserve((nout + TTF_GUARD_DOUBLES) * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpy(s->cores.ptr, coeff_cores, (size_t)off * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(s->out.ptr, 0xFF, (nout + TTF_GUARD_DOUBLES) * sizeof(double)));      // all bits set: a NaN

    for (hipEvent_t &e : s->ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(s->ev[0], 0));
    const size_t lds = 4 * tt_fit_interface_doubles(gi.rmax, gi.nmax) * sizeof(double);      // at most 24 KiB
    const unsigned wg = (unsigned)std::min<long>((N + 3) / 4, 256L * 16);
    hipLaunchKernelGGL(k_ttf_interface, dim3(wg), dim3(TTF_THREADS), lds, 0, gi, dm, (const double *)s->cores.ptr, s->d_pts,
                       s->d_y, N, k, (double *)s->V.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev[1], 0));
    const int form = s->form == TTF_FORM_AUTO ? (P >= 16 ? TTF_FORM_MFMA : TTF_FORM_VALU) : s->form;
    if (form == TTF_FORM_MFMA) {
        const unsigned tb = (unsigned)(Ppad / TTF_BLOCK);
        hipLaunchKernelGGL(k_ttf_gram_mfma, dim3(tb * tb, (unsigned)chunks), dim3(TTF_THREADS), 0, 0, (const double *)s->V.ptr,
                           rl, n, rr, N, chunk, Ppad, (double *)s->partial.ptr);
    } else {
        const unsigned t = (unsigned)(Ppad / 16);
        hipLaunchKernelGGL(k_ttf_gram_valu, dim3(t * t, (unsigned)chunks), dim3(TTF_THREADS), 0, 0, (const double *)s->V.ptr,
                           rl, n, rr, N, chunk, Ppad, (double *)s->partial.ptr);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev[2], 0));
    const long cells = ((long)P + 1) * (P + 1);
    hipLaunchKernelGGL(k_ttf_reduce, dim3((unsigned)((cells + TTF_THREADS - 1) / TTF_THREADS)), dim3(TTF_THREADS), 0, 0,
                       (const double *)s->partial.ptr, chunks, Ppad, P, (double *)s->out.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev[3], 0));
    HIP_TRY(hipDeviceSynchronize());
    for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(&s->ms[i], s->ev[i], s->ev[i + 1]));
    const double *dout = (const double *)s->out.ptr;
    uint64_t guard[TTF_GUARD_DOUBLES];
    HIP_TRY(hipMemcpy(guard, dout + nout, sizeof(guard), hipMemcpyDeviceToHost));
    for (int i = 0; i < TTF_GUARD_DOUBLES; ++i)
        if (guard[i] != ~(uint64_t)0)
            return fail(PCX_ERR_INTERNAL, "TT fit: a kernel wrote %d doubles past its output (position %d, form %d, P = %d, N = %lld)",
                        i, k, form, P, (long long)N);
    HIP_TRY(hipMemcpy(G_out, dout, (size_t)P * P * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(b_out, dout + (size_t)P * P, (size_t)P * sizeof(double), hipMemcpyDeviceToHost));
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_tt_fit_times(pcx_tt_fit *s, float *ms_out) {
    PCX_API_BEGIN
    if (!s || !ms_out) return fail(PCX_ERR_INVALID, "TT fit: NULL argument");
    std::lock_guard<std::mutex> lk(s->mu);
    for (int i = 0; i < 3; ++i) ms_out[i] = s->ms[i];
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_tt_fit_residual(pcx_tt_fit *s, int d, const int32_t *n_nodes, const int32_t *ranks,
                                   const double *coeff_cores, double *sumsq_out) {
    PCX_API_BEGIN
    int rc = check_model(s, d, n_nodes, ranks, coeff_cores);
    if (rc) return rc;
    if (!sumsq_out) return fail(PCX_ERR_INVALID, "TT fit: NULL output");
    HIP_TRY(hipSetDevice(s->device));
    std::lock_guard<std::mutex> lk(s->mu);
    const long N = s->N;
    if ((rc = s->eval.reserve((size_t)N * sizeof(double)))) return rc;
    if ((rc = s->red.reserve((size_t)TTA_RED_BLOCKS * 4 * sizeof(double)))) return rc;
    if ((rc = s->sums.reserve(4 * sizeof(double)))) return rc;
    pcx_tt *h = nullptr;
    if ((rc = pcx_tt_create(s->device, d, n_nodes, ranks, s->lo, s->hi, coeff_cores, nullptr, &h))) return rc;
    std::unique_ptr<pcx_tt, int (*)(pcx_tt *)> owner(h, pcx_tt_destroy);
    void *st = nullptr;
    if ((rc = pcx_tt_stream(h, &st))) return rc;
    if ((rc = pcx_tt_eval_batch_dev(h, s->d_pts, N, (double *)s->eval.ptr, st))) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)st));
    const double *e = (const double *)s->eval.ptr;
    const int blocks = (int)std::max<long>(1, std::min<long>((N + TTA_THREADS - 1) / TTA_THREADS, TTA_RED_BLOCKS));
    hipLaunchKernelGGL(k_tta_norms, dim3(blocks), dim3(TTA_THREADS), 0, 0, e, e, s->d_y, N, (double *)s->red.ptr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tta_norms_final, dim3(1), dim3(TTA_THREADS), 0, 0, (const double *)s->red.ptr, blocks, (double *)s->sums.ptr);
    HIP_TRY(hipGetLastError());
    double sums[4];
    HIP_TRY(hipMemcpy(sums, s->sums.ptr, sizeof(sums), hipMemcpyDeviceToHost));
    sumsq_out[0] = sums[2];
    sumsq_out[1] = sums[3];
    return PCX_OK;
    PCX_API_END
}
