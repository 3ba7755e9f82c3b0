// pcx_bary.hip -- C ABI of libpcx_hip.so (see include/pcx.h): the barycentric handle.  gfx950 only.
//
// Host side: argument validation, device buffers, kernel launches, host-pointer pipelines and the single-process
// fan-out; the launch plan of a handle is made in pcx_bary_plan.hip (bary_plan.h).  No CPU arithmetic fallback lives here: every numeric result comes from a HIP kernel.

#include <memory>

#include "pcx_bary_internal.h"
#include "bary_kernels.h"
#include "bary_mfma_launch.h"
#include "gather_kernels.h"
#include "sobol_kernels.h"

// ---------------------------------------------------------------------------------
// barycentric handle
// ---------------------------------------------------------------------------------
static const int kCacheSpecs = 96;    // derivative tensors kept per handle besides the untransformed one

// everything the handle owns; the caller has made its device current and drained its stream (pcx_bary_destroy)
pcx_bary::~pcx_bary() {
    for (auto &kv : cache) kv.second.free_all();
    for (void *p : {(void *)d_tab, (void *)d_nodes, (void *)d_wts, (void *)d_diff, (void *)d_cheb, (void *)d_boxq, (void *)d_snodes,
                    (void *)d_gsnodes, (void *)d_rowcode, (void *)d_kcode, (void *)d_rowcode_hi, (void *)d_kcode_hi,
                    (void *)d_rowcode_g0, (void *)d_rowoff[0], (void *)d_rowoff[1]})
        (void)hipFree(p);
    for (Scratch *sc : {&s_partial, &s_cheb[0], &s_cheb[1], &s_sobol, &s_rot, &s_rot2, &s_grid[0], &s_grid[1], &s_gridw, &s_gridout})
        sc->release();
    if (grid_done) (void)hipEventDestroy(grid_done);
    for (pcx_bary *r : rot)
        if (r) pcx_bary_destroy(r);
    stage.release();
    if (stream) (void)hipStreamDestroy(stream);
}

extern "C" int pcx_bary_destroy(pcx_bary *h) {
    PCX_API_BEGIN
    if (!h) return PCX_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    delete h;
    return PCX_OK;
    PCX_API_END
}

// Packs dt.plain into MFMA fragments; on failure dt.frag / dt.slot are released again.
static int bary_pack(pcx_bary *h, DerivedTensor &dt) {
    if (!h->mfma_ok) return PCX_OK;
    const BaryMfmaPlan &p = h->plan;
    size_t cnt = h->kfold_ok ? bary_kfold_frag_count(h->kf) : (size_t)(h->grid_ok ? h->gp.MT : p.MT) * p.KS * 64;
    const size_t nseed = (size_t)p.MT * 16 * p.R;                 // the seed columns, behind the image (R = 0: none)
    DevBuf frag, slot;
    int rc = frag.alloc((cnt + nseed) * sizeof(double));
    if (rc) return rc;
    if (h->kfold_ok) {
        if ((rc = bary_pack_kfold(h, dt.plain, frag.as<double>()))) return rc;
    } else if (h->grid_ok) {
        if ((rc = bary_pack_grid(h, dt.plain, frag.as<double>()))) return rc;
    } else {
        int blocks = (int)((cnt + 255) / 256);
        hipLaunchKernelGGL(k_pack_fragments, dim3(blocks), dim3(256), 0, h->stream, dt.plain, frag.as<double>(),
                           p.M, p.K, p.MT, p.KS, p.R);
        HIP_TRY(hipGetLastError());
        if (nseed) {
            hipLaunchKernelGGL(k_pack_seed, dim3((unsigned)((nseed + 255) / 256)), dim3(256), 0, h->stream, dt.plain,
                               frag.as<double>() + cnt, p.M, p.K, p.MT, p.R, 0);
            HIP_TRY(hipGetLastError());
        }
    }
    if ((rc = slot.alloc(sizeof(double *)))) return rc;
    double *fp = frag.as<double>();
    HIP_TRY(hipMemcpy(slot.p, &fp, sizeof(double *), hipMemcpyHostToDevice));
    dt.frag = frag.release<double>();
    dt.slot = slot.release<double *>();
    return PCX_OK;
}

// a host-built table (or any host array) as a device buffer the handle owns from here on
template <typename T>
static int upload(T *&dst, const T *src, size_t count) {
    HIP_TRY(hipMalloc((void **)&dst, count * sizeof(T)));
    HIP_TRY(hipMemcpy(dst, src, count * sizeof(T), hipMemcpyHostToDevice));
    return PCX_OK;
}
template <typename T>
static int upload(T *&dst, const std::vector<T> &v) { return upload(dst, v.data(), v.size()); }

// validate, plan (bary_make_plan: pcx_bary_plan.hip decides everything about the launches), upload
extern "C" int pcx_bary_create(int device, int d, const int32_t *n_nodes, const double *nodes_cat,
                               const double *weights_cat, const double *diffmat_cat,
                               const double *tensor, pcx_bary **out) {
    PCX_API_BEGIN
    if (!out) return fail(PCX_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (d < 1 || d > PCX_MAX_DIMS) return fail(PCX_ERR_INVALID, "d=%d outside [1, %d]", d, PCX_MAX_DIMS);
    if (!n_nodes || !nodes_cat || !weights_cat || !diffmat_cat || !tensor)
        return fail(PCX_ERR_INVALID, "NULL model array");
    int rc = use_device(device);
    if (rc) return rc;
    std::unique_ptr<pcx_bary, int (*)(pcx_bary *)> h(new (std::nothrow) pcx_bary(), pcx_bary_destroy);
    if (!h) return fail(PCX_ERR_NOMEM, "out of host memory");
    h->device = device;
    h->dims.d = d;
    long total = 1, sum_n = 0, sum_n2 = 0;
    for (int k = 0; k < d; ++k) {
        if (n_nodes[k] < 1 || n_nodes[k] > 4096) return fail(PCX_ERR_INVALID, "n_nodes[%d]=%d outside [1, 4096]", k, n_nodes[k]);
        h->dims.n[k] = n_nodes[k];
        h->dims.off[k] = (int)sum_n;
        h->doff.push_back((int)sum_n2);
        sum_n += n_nodes[k];
        sum_n2 += (long)n_nodes[k] * n_nodes[k];
        total *= n_nodes[k];
        if (total > (1L << 33)) return fail(PCX_ERR_UNSUPPORTED, "tensor larger than 2^33 elements");
    }
    for (int k = d; k < PCX_MAX_DIMS; ++k) { h->dims.n[k] = 1; h->dims.off[k] = 0; }
    h->dims.sum_n = (int)sum_n;
    h->total = total;
    const BaryDims &dm = h->dims;

    // shapes no kernel covers fail here, at create, not at the first evaluation
    const BaryEnv env = bary_read_env();
    h->g0_span = env.g0_span;
    h->group_tol = env.group_tol;
    if ((rc = bary_make_plan(dm, total, nodes_cat, env, *h))) return rc;
    h->h_nodes.assign(nodes_cat, nodes_cat + sum_n);
    h->h_wts.assign(weights_cat, weights_cat + sum_n);

    // the grid arrays and the tables the plan asks for
    HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    if ((rc = upload(h->d_nodes, nodes_cat, sum_n)) || (rc = upload(h->d_wts, weights_cat, sum_n)) ||
        (rc = upload(h->d_diff, diffmat_cat, sum_n2)))
        return rc;
    if (h->small_nlp && (rc = upload(h->d_snodes, bary_scaled_nodes(dm, nodes_cat, false)))) return rc;
    if ((h->grid_ok || h->kfold_ok) && (rc = upload(h->d_gsnodes, bary_scaled_nodes(dm, nodes_cat, true)))) return rc;
    if (h->mfma_ok) {
        const std::vector<unsigned> rowcode = bary_row_codes(dm, h->plan, 0);
        if ((rc = upload(h->d_rowcode, rowcode)) || (rc = upload(h->d_kcode, bary_k_codes(dm, h->plan, 0)))) return rc;
        if (h->wide && ((rc = upload(h->d_rowcode_hi, bary_row_codes(dm, h->plan, 1))) ||
                        (rc = upload(h->d_kcode_hi, bary_k_codes(dm, h->plan, 1)))))
            return rc;
        for (int nt = 1; nt <= 2 && bary_plan_row_offsets(*h); ++nt)
            if ((rc = upload(h->d_rowoff[nt - 1], bary_row_offsets(rowcode, nt)))) return rc;
        if (h->g0_ok && (rc = upload(h->d_rowcode_g0, bary_slab_row_codes(dm, *h)))) return rc;
    }

    // value tensor (derivative spec all-zero) enters the cache at create
    DerivedTensor &dt = h->cache[std::vector<int>(d, 0)];
    {
        DevBuf plain;
        if ((rc = alloc_plain(plain, total))) return rc;
        dt.plain = plain.release<double>();
    }
    HIP_TRY(hipMemcpy(dt.plain, tensor, total * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = bary_pack(h.get(), dt))) return rc;
    HIP_TRY(hipMalloc((void **)&h->d_tab, kMaxSpecs * sizeof(double *)));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *out = h.release();
    return PCX_OK;
    PCX_API_END
}

// ---- .pcb loader (host-side parsing and grid metadata; no evaluation arithmetic) ------
static void host_grid_metadata(double lo, double hi, int n, double *x, double *w, double *D) {
    const double pi = 3.14159265358979323846;
    for (int k = 0; k < n; ++k)   // numpy chebpts1: sin(0.5 pi / n * (-n + 1 + 2k)), ascending
        x[k] = 0.5 * (lo + hi) + 0.5 * (hi - lo) * std::sin(0.5 * pi / n * (double)(-n + 1 + 2 * k));
    std::sort(x, x + n);
    for (int i = 0; i < n; ++i) {
        double wi = 1.0;
        for (int j = 0; j < n; ++j)
            if (j != i) wi /= (x[i] - x[j]);
        w[i] = wi;
    }
    for (int i = 0; i < n; ++i) {
        double rowsum = 0.0;
        for (int j = 0; j < n; ++j) {
            double v = (i == j) ? 0.0 : w[j] / ((x[i] - x[j]) * w[i]);
            D[(size_t)i * n + j] = v;
            rowsum += v;
        }
        D[(size_t)i * n + i] = -rowsum;
    }
}

extern "C" int pcx_bary_create_from_pcb(int device, const char *path, pcx_bary **out) {
    PCX_API_BEGIN
    if (!out) return fail(PCX_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!path) return fail(PCX_ERR_INVALID, "path is NULL");
    FILE *f = fopen(path, "rb");
    if (!f) return fail(PCX_ERR_INVALID, "cannot open %s", path);
    auto bail = [&](const char *why) { fclose(f); return fail(PCX_ERR_INVALID, "%s: %s", path, why); };
    unsigned char head[12];
    if (fread(head, 1, 12, f) != 12) return bail("shorter than the 12-byte .pcb header");
    if (memcmp(head, "PCB\0", 4) != 0) return bail("not a PyChebyshev binary file (bad magic)");
    if (head[4] != 1) return bail("unsupported .pcb major version");
    if ((head[6] | (head[7] << 8)) != 1) return bail("class tag is not ChebyshevApproximation");
    if (head[8] | head[9] | head[10] | head[11]) return bail("reserved header bytes nonzero");
    uint32_t d = 0;
    if (fread(&d, 4, 1, f) != 1) return bail("unexpected EOF reading num_dimensions");
    if (d < 1 || d > PCX_MAX_DIMS) return bail("num_dimensions outside [1, 16]");
    std::vector<double> lo(d), hi(d);
    std::vector<uint32_t> nn(d);
    if (fread(lo.data(), 8, d, f) != d || fread(hi.data(), 8, d, f) != d || fread(nn.data(), 4, d, f) != d)
        return bail("unexpected EOF reading domain / n_nodes");
    size_t total = 1, sum_n = 0, sum_n2 = 0;
    std::vector<int32_t> n(d);
    for (uint32_t k = 0; k < d; ++k) {
        if (!(lo[k] < hi[k])) return bail("domain lo must be < hi");
        if (nn[k] < 1 || nn[k] > 4096) return bail("n_nodes outside [1, 4096]");
        n[k] = (int32_t)nn[k];
        total *= nn[k];
        sum_n += nn[k];
        sum_n2 += (size_t)nn[k] * nn[k];
        if (total > ((size_t)1 << 33)) return bail("tensor larger than 2^33 elements");
    }
    std::vector<double> tensor(total);
    if (fread(tensor.data(), 8, total, f) != total) return bail("unexpected EOF reading tensor_values");
    fclose(f);
    for (size_t i = 0; i < total; ++i)
        if (!std::isfinite(tensor[i])) return fail(PCX_ERR_INVALID, "%s: tensor_values contains NaN or Inf", path);
    std::vector<double> nodes(sum_n), wts(sum_n), diff(sum_n2);
    size_t o1 = 0, o2 = 0;
    for (uint32_t k = 0; k < d; ++k) {
        host_grid_metadata(lo[k], hi[k], n[k], nodes.data() + o1, wts.data() + o1, diff.data() + o2);
        o1 += n[k];
        o2 += (size_t)n[k] * n[k];
    }
    int rc = pcx_bary_create(device, (int)d, n.data(), nodes.data(), wts.data(), diff.data(), tensor.data(), out);
    if (rc == PCX_OK) { (*out)->dom_lo = lo; (*out)->dom_hi = hi; }
    return rc;
    PCX_API_END
}

// .pcb v1 writer (reference _binary.py:208-283, write side): 12-byte header, d, lower bounds,
// upper bounds, n_nodes, tensor_values in C order -- all little-endian, no padding.  The tensor
// is the handle's untransformed device copy, so load -> save reproduces the file byte for byte.
extern "C" int pcx_bary_save_pcb(pcx_bary *h, const char *path, const double *lo, const double *hi) {
    PCX_API_BEGIN
    if (!h || !path) return fail(PCX_ERR_INVALID, "NULL argument");
    const int d = h->dims.d;
    if ((lo == nullptr) != (hi == nullptr)) return fail(PCX_ERR_INVALID, "pass both domain bounds or neither");
    if (!lo) {
        if ((int)h->dom_lo.size() != d)
            return fail(PCX_ERR_INVALID, "the handle does not know its domain (not loaded from a .pcb file): pass lo / hi");
        lo = h->dom_lo.data();
        hi = h->dom_hi.data();
    }
    for (int k = 0; k < d; ++k)
        if (!(lo[k] < hi[k])) return fail(PCX_ERR_INVALID, "domain[%d]: lo must be < hi", k);
    std::vector<double> tensor((size_t)h->total);
    {
        HIP_TRY(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lk(h->mu);
        const DerivedTensor &base = h->cache[std::vector<int>(d, 0)];
        HIP_TRY(hipMemcpy(tensor.data(), base.plain, (size_t)h->total * sizeof(double), hipMemcpyDeviceToHost));
    }
    FILE *f = fopen(path, "wb");
    if (!f) return fail(PCX_ERR_INVALID, "cannot open %s for writing", path);
    const unsigned char head[12] = {'P', 'C', 'B', 0, 1, 0, 1, 0, 0, 0, 0, 0};   // magic, major 1, minor 0, class tag 1
    const uint32_t du = (uint32_t)d;
    std::vector<uint32_t> nn(d);
    for (int k = 0; k < d; ++k) nn[k] = (uint32_t)h->dims.n[k];
    bool ok = fwrite(head, 1, 12, f) == 12 && fwrite(&du, 4, 1, f) == 1 && fwrite(lo, 8, d, f) == (size_t)d &&
              fwrite(hi, 8, d, f) == (size_t)d && fwrite(nn.data(), 4, d, f) == (size_t)d &&
              fwrite(tensor.data(), 8, tensor.size(), f) == tensor.size();
    ok = (fclose(f) == 0) && ok;
    if (!ok) return fail(PCX_ERR_INVALID, "short write to %s", path);
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_bary_shape(pcx_bary *h, int32_t *d_out, int32_t *n_nodes_out) {
    PCX_API_BEGIN
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    if (d_out) *d_out = h->dims.d;
    if (n_nodes_out)
        for (int k = 0; k < PCX_MAX_DIMS; ++k) n_nodes_out[k] = k < h->dims.d ? h->dims.n[k] : 0;
    return PCX_OK;
    PCX_API_END
}

// Returns (building on first use) the derivative-transformed tensor for `deriv`.
// Caller holds h->mu.  Work is enqueued on h->stream.
PCX_HIDDEN int bary_get_tensor(pcx_bary *h, const int32_t *deriv, DerivedTensor **out) {
    const int d = h->dims.d;
    std::vector<int> key(d, 0);
    if (deriv)
        for (int k = 0; k < d; ++k) {
            if (deriv[k] < 0 || deriv[k] > 8) return fail(PCX_ERR_INVALID, "derivative order %d at dim %d outside [0, 8]", deriv[k], k);
            key[k] = deriv[k];
        }
    auto it = h->cache.find(key);
    if (it != h->cache.end()) {
        it->second.last_use = ++h->clock;
        *out = &it->second;
        return PCX_OK;
    }
    // The cache holds the untransformed tensor plus up to kCacheSpecs derivative tensors; beyond
    // that the least recently used one that the current call has not asked for is dropped.
    // Kernels reading it may still be queued (on any stream of a _dev caller): drain the device first.
    if (h->cache.size() > (size_t)kCacheSpecs) {
        auto victim = h->cache.end();
        for (auto c = h->cache.begin(); c != h->cache.end(); ++c) {
            bool is_base = true;
            for (int v : c->first) is_base = is_base && v == 0;
            if (is_base || c->second.last_use > h->call_mark) continue;
            if (victim == h->cache.end() || c->second.last_use < victim->second.last_use) victim = c;
        }
        if (victim == h->cache.end())
            return fail(PCX_ERR_UNSUPPORTED, "more than %d distinct derivative specs in one call", kCacheSpecs);
        HIP_TRY(hipDeviceSynchronize());
        if (!h->tab_host.empty()) h->tab_host.clear();      // the multi-spec table may name the victim
        victim->second.free_all();
        h->cache.erase(victim);
    }

    DerivedTensor &base = h->cache[std::vector<int>(d, 0)];
    DevBuf cur, tmp;
    int rc = alloc_plain(cur, h->total);
    if (rc) return rc;
    if ((rc = alloc_plain(tmp, h->total))) return rc;
    HIP_TRY(hipMemcpyAsync(cur.p, base.plain, h->total * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    // barycentric.py:982-989: dims descending, order[k] passes each
    for (int k = d - 1; k >= 0; --k) {
        long outer = 1, inner = 1;
        for (int q = 0; q < k; ++q) outer *= h->dims.n[q];
        for (int q = k + 1; q < d; ++q) inner *= h->dims.n[q];
        for (int r = 0; r < key[k]; ++r) {
            int blocks = (int)((h->total + 255) / 256);
            hipLaunchKernelGGL(k_mode_product, dim3(blocks), dim3(256), 0, h->stream, cur.as<double>(), tmp.as<double>(),
                               h->d_diff + h->doff[k], outer, h->dims.n[k], inner);
            std::swap(cur.p, tmp.p);
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    DerivedTensor dt;
    dt.plain = cur.as<double>();
    if ((rc = bary_pack(h, dt))) return rc;          // cur still owns the tensor: freed on this path
    (void)cur.release<double>();
    dt.last_use = ++h->clock;
    auto ins = h->cache.emplace(key, dt);
    *out = &ins.first->second;
    return PCX_OK;
}

static int launch_rows(pcx_bary *h, const DerivedTensor &dt, const double *d_pts, long N,
                       double *d_out, long ostride, long ooff, hipStream_t st, const int *perm) {
    int ppw = 256 / h->lpp;
    size_t lds = (size_t)ppw * h->dims.sum_n * sizeof(double);
    if (lds > 160 * 1024) return fail(PCX_ERR_UNSUPPORTED, "sum of node counts %d too large for the rows kernel", h->dims.sum_n);
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)k_bary_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    long blocks = (N + ppw - 1) / ppw;
    if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
    hipLaunchKernelGGL(k_bary_rows, dim3((unsigned)blocks), dim3(256), lds, st, h->dims, h->lpp,
                       h->d_nodes, h->d_wts, dt.plain, d_pts, d_out, N, ostride, ooff, perm);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

// Evaluate m specs (dts[0..m)) at N device-resident points; out[p*ostride + ooff + s].
// T_tab (device table of m plain tensors) or, when NULL, the single tensor dt
template <int DOUT, int NLP>
static int launch_small_t(pcx_bary *h, const DerivedTensor &dt, const double *const *T_tab, int m, const double *d_pts,
                          long N, double *d_out, long ostride, long ooff, hipStream_t st, const int *perm) {
    auto kern = k_bary_small<DOUT, NLP>;
    size_t lds = (size_t)(h->dims.sum_n - h->dims.n[DOUT]) * 64 * sizeof(double);
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    long blocks = (N + 63) / 64;
    if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(64), lds, st, h->dims, h->small_scale, h->d_snodes, h->d_nodes,
                       h->d_wts, dt.plain, T_tab, m, d_pts, d_out, N, ostride, ooff, perm);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

template <int DOUT>
static int launch_small_d(pcx_bary *h, const DerivedTensor &dt, const double *const *T_tab, int m, const double *d_pts,
                          long N, double *d_out, long ostride, long ooff, hipStream_t st, const int *perm) {
    switch (h->small_nlp) {
#define CASE_NLP(v) case v: return launch_small_t<DOUT, v>(h, dt, T_tab, m, d_pts, N, d_out, ostride, ooff, st, perm);
    CASE_NLP(2) CASE_NLP(3) CASE_NLP(4) CASE_NLP(5) CASE_NLP(6) CASE_NLP(7) CASE_NLP(8) CASE_NLP(9) CASE_NLP(10) CASE_NLP(11)
    CASE_NLP(12) CASE_NLP(13) CASE_NLP(14) CASE_NLP(15) CASE_NLP(16) CASE_NLP(24) CASE_NLP(32) CASE_NLP(48) CASE_NLP(64)
#undef CASE_NLP
    }
    return fail(PCX_ERR_UNSUPPORTED, "lane-per-point kernel does not cover this shape");
}

static int launch_small(pcx_bary *h, const DerivedTensor &dt, const double *const *T_tab, int m, const double *d_pts,
                        long N, double *d_out, long ostride, long ooff, hipStream_t st, const int *perm) {
    switch (h->dims.d) {
    case 1: return launch_small_d<0>(h, dt, T_tab, m, d_pts, N, d_out, ostride, ooff, st, perm);
    case 2: return launch_small_d<1>(h, dt, T_tab, m, d_pts, N, d_out, ostride, ooff, st, perm);
    case 3: return launch_small_d<2>(h, dt, T_tab, m, d_pts, N, d_out, ostride, ooff, st, perm);
    case 4: return launch_small_d<3>(h, dt, T_tab, m, d_pts, N, d_out, ostride, ooff, st, perm);
    }
    return fail(PCX_ERR_UNSUPPORTED, "lane-per-point kernel does not cover this shape");
}


template <int NL>
static int launch_sq_t(pcx_bary *h, const DerivedTensor &dt, const double *const *T_tab, int m, const double *d_pts,
                       long N, double *d_out, long ostride, long ooff, hipStream_t st, const int *perm) {
    const int d = h->dims.d;
    size_t lds = 0;
    for (int k = 0; k < d - 2; ++k) lds += (size_t)h->dims.n[k] * 64 * sizeof(double);
    long blocks = (N + 63) / 64;
    if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
#define PCX_SQ_GO(LEAD)                                                                                               \
    hipLaunchKernelGGL((k_bary_sq<NL, LEAD>), dim3((unsigned)blocks), dim3(64), lds, st, h->dims, h->small_scale,    \
                       h->d_snodes, h->d_nodes, h->d_wts, dt.plain, T_tab, m, d_pts, d_out, N, ostride, ooff, perm)
    if (d == 2) PCX_SQ_GO(0);
    else if (d == 3) PCX_SQ_GO(1);
    else PCX_SQ_GO(2);
#undef PCX_SQ_GO
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

static int launch_sq(pcx_bary *h, const DerivedTensor &dt, const double *const *T_tab, int m, const double *d_pts,
                     long N, double *d_out, long ostride, long ooff, hipStream_t st, const int *perm) {
    switch (h->sq_nl) {
#define CASE_NL(v) case v: return launch_sq_t<v>(h, dt, T_tab, m, d_pts, N, d_out, ostride, ooff, st, perm);
    CASE_NL(4) CASE_NL(5) CASE_NL(6) CASE_NL(7) CASE_NL(8) CASE_NL(9) CASE_NL(10) CASE_NL(11) CASE_NL(12) CASE_NL(13)
    CASE_NL(14) CASE_NL(15) CASE_NL(16) CASE_NL(17) CASE_NL(18) CASE_NL(19) CASE_NL(20) CASE_NL(21) CASE_NL(22)
    CASE_NL(23) CASE_NL(24) CASE_NL(26) CASE_NL(28) CASE_NL(30) CASE_NL(32)
#undef CASE_NL
    }
    return fail(PCX_ERR_UNSUPPORTED, "square-trailing lane-per-point kernel does not cover this shape");
}

// ---- dim-0 group launches (BaryG0) --------------------------------------------------------------
// Slab-packs dt.plain on first use (caller holds h->mu; enqueued on h->stream and synchronised).
static int bary_pack_g0(pcx_bary *h, DerivedTensor &dt) {
    if (dt.frag_g0) return PCX_OK;
    const BaryMfmaPlan &p = h->plan;
    const int n0 = h->dims.n[0];
    const size_t cnt = (size_t)n0 * h->g0_tps * p.KS * 64;
    const size_t nseed = (size_t)n0 * h->g0_tps * 16 * p.R;       // the slabs' seed columns, behind the image
    DevBuf frag, slot;
    int rc = frag.alloc((cnt + nseed) * sizeof(double));
    if (rc) return rc;
    hipLaunchKernelGGL(k_pack_fragments_slabs, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream, dt.plain,
                       frag.as<double>(), n0, p.M / n0, p.K, h->g0_tps, p.KS, p.R);
    HIP_TRY(hipGetLastError());
    if (nseed) {
        hipLaunchKernelGGL(k_pack_seed, dim3((unsigned)((nseed + 255) / 256)), dim3(256), 0, h->stream, dt.plain,
                           frag.as<double>() + cnt, p.M / n0, p.K, n0 * h->g0_tps, p.R, h->g0_tps);
        HIP_TRY(hipGetLastError());
    }
    if ((rc = slot.alloc(sizeof(double *)))) return rc;
    double *fp = frag.as<double>();
    HIP_TRY(hipMemcpy(slot.p, &fp, sizeof(double *), hipMemcpyHostToDevice));
    HIP_TRY(hipStreamSynchronize(h->stream));
    dt.frag_g0 = frag.release<double>();
    dt.slot_g0 = slot.release<double *>();
    return PCX_OK;
}

static const long kG0MinPoints = 65536;      // below: per-spec launches (they split over row tiles and need no second pass)

// the kernel a launch will take: 1 rows, 2 MFMA 16x16x4, 3 MFMA 4x4x4, 4 lane-per-point, 5 k_bary_sq
PCX_HIDDEN int bary_effective_variant(const pcx_bary *h) { return h->variant != 0 ? h->variant : bary_auto_variant(*h); }

// frag_tab is a device table holding the m tensor pointers of a multi-spec launch: fragment images for
// the MFMA kernels, plain tensors for the lane-per-point kernel (see bary_spec_table); for m = 1 the MFMA
// kernels read dts[0]->slot and the lane-per-point kernel takes dts[0]->plain directly.
// split_scratch (nullable): where split launches of small batches keep their per-chunk sums;
// perm (nullable): evaluate rows perm[0..N) of d_pts / d_out instead of rows 0..N.
PCX_HIDDEN int bary_launch(pcx_bary *h, DerivedTensor *const *dts, int m, const double *const *frag_tab,
                       const double *d_pts, long N, double *d_out, long ostride, long ooff,
                       hipStream_t st, Scratch *split_scratch, const int *perm) {
    if (N == 0) return PCX_OK;
    const int variant = bary_effective_variant(h);
    if (variant == 4) {
        if (!h->small_nlp) return fail(PCX_ERR_UNSUPPORTED, "lane-per-point kernel does not cover this shape");
        return launch_small(h, *dts[0], m > 1 ? frag_tab : nullptr, m, d_pts, N, d_out, ostride, ooff, st, perm);
    }
    if (variant == 5) {
        if (!h->sq_nl) return fail(PCX_ERR_UNSUPPORTED, "square-trailing lane-per-point kernel does not cover this shape");
        return launch_sq(h, *dts[0], m > 1 ? frag_tab : nullptr, m, d_pts, N, d_out, ostride, ooff, st, perm);
    }
    if (variant == 3) {
        if (!h->mfma4_ok) return fail(PCX_ERR_UNSUPPORTED, "4x4x4 MFMA kernel does not cover this shape");
        switch (h->plan.R) {
        case 1: return bary_launch_mfma4_seed1(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, perm);
        case 2: return bary_launch_mfma4_seed2(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, perm);
        }
        return launch_mfma4<0>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, perm);
    }
    if (variant == 2) {
        if (!h->mfma_ok) return fail(PCX_ERR_UNSUPPORTED, "MFMA kernel does not cover this shape");
        if (h->kfold_ok) return bary_launch_kfold(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, perm);
        if (h->grid_ok) return bary_launch_grid(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm);
        switch (h->plan.R) {
        case 1: return bary_launch_rowcode_seed1(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm);
        case 2: return bary_launch_rowcode_seed2(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm);
        }
        return launch_rowcode<0>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm);
    }
    for (int s = 0; s < m; ++s) {
        int rc = launch_rows(h, *dts[s], d_pts, N, d_out, ostride, ooff + s, st, perm);
        if (rc) return rc;
    }
    return PCX_OK;
}

// The model with dimension q moved to the front (the other dimensions keep their order), or NULL when that shape has
// no slab plan -- which the planner says from the node counts and nodes, before anything else is downloaded.  Built on
// first use from the device copies of the grid arrays and the value tensor: a transposed copy of a tensor of at most
// 2^24 elements, once per handle and dimension.  Caller holds h->mu.
static const long kRotMaxElems = 1L << 24;
static pcx_bary *bary_rot(pcx_bary *h, int q) {
    if (h->rot_state[q]) return h->rot[q];
    h->rot_state[q] = 2;
    const int d = h->dims.d;
    if (q < 1 || q >= d || h->total > kRotMaxElems || h->dims.n[q] < 2 || h->dims.n[q] > 16) return nullptr;
    int pd[PCX_MAX_DIMS];                       // pd[c] = original dimension at position c of the sub-model
    pd[0] = q;
    for (int k = 0, c = 1; k < d; ++k)
        if (k != q) pd[c++] = k;
    // ask the planner first: the rotated node counts and nodes decide whether that shape has a slab plan
    const long sum_n = h->dims.sum_n;
    std::vector<double> nodes((size_t)sum_n), rn;
    if (hipMemcpy(nodes.data(), h->d_nodes, sum_n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    std::vector<int32_t> nn(d);
    BaryDims rdm = h->dims;
    for (int c = 0, off = 0; c < d; off += nn[c], ++c) {
        const int k = pd[c];
        nn[c] = rdm.n[c] = h->dims.n[k];
        rdm.off[c] = off;
        rn.insert(rn.end(), nodes.begin() + h->dims.off[k], nodes.begin() + h->dims.off[k] + nn[c]);
    }
    BaryLaunchPlan rplan;
    if (bary_make_plan(rdm, h->total, rn.data(), bary_read_env(), rplan) != PCX_OK || !rplan.g0_ok) return nullptr;
    long sum_n2 = 0;
    for (int k = 0; k < d; ++k) sum_n2 += (long)h->dims.n[k] * h->dims.n[k];
    std::vector<double> wts((size_t)sum_n), diff((size_t)sum_n2), T((size_t)h->total), TR((size_t)h->total);
    const DerivedTensor &val = h->cache[std::vector<int>(d, 0)];
    if (hipMemcpy(wts.data(), h->d_wts, sum_n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(diff.data(), h->d_diff, sum_n2 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(T.data(), val.plain, h->total * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    std::vector<double> rw, rd;
    long stride[PCX_MAX_DIMS];                  // element strides of the original C-order tensor
    { long acc = 1; for (int k = d - 1; k >= 0; --k) { stride[k] = acc; acc *= h->dims.n[k]; } }
    for (int c = 0; c < d; ++c) {
        const int k = pd[c], n = h->dims.n[k];
        rw.insert(rw.end(), wts.begin() + h->dims.off[k], wts.begin() + h->dims.off[k] + n);
        rd.insert(rd.end(), diff.begin() + h->doff[k], diff.begin() + h->doff[k] + (long)n * n);
    }
    {   // TR[i_q, i_0, ..] = T[i_0, .., i_q, ..]: an odometer over the sub-model's index, the source offset kept alongside
        int idx[PCX_MAX_DIMS] = {};
        long src = 0;
        for (long e = 0; e < h->total; ++e) {
            TR[(size_t)e] = T[(size_t)src];
            for (int c = d - 1; c >= 0; --c) {
                src += stride[pd[c]];
                if (++idx[c] < nn[c]) break;
                src -= stride[pd[c]] * nn[c];
                idx[c] = 0;
            }
        }
    }
    pcx_bary *r = nullptr;
    if (pcx_bary_create(h->device, d, nn.data(), rn.data(), rw.data(), rd.data(), TR.data(), &r) != PCX_OK || !r) return nullptr;
    h->rot[q] = r;
    h->rot_state[q] = 1;
    return r;
}

// One slab launch: the specs `lower` + rel[i] e_q (lower: a spec in h's dimension order whose order along q is the
// group's base) into columns col[i].  pp: the batch in the column order of the model that runs it (h for q = 0, else
// h->rot[q]).  Caller holds h->mu.
static int bary_launch_group(pcx_bary *h, int q, const int32_t *lower, const int *rel, const int *col, int nmem,
                             const double *pp, long N, double *d_out, long ostride, long ooff, hipStream_t st) {
    const int d = h->dims.d;
    pcx_bary *g = q == 0 ? h : h->rot[q];
    std::vector<int32_t> bspec(d);
    if (q == 0) bspec.assign(lower, lower + d);
    else { bspec[0] = lower[q]; for (int k = 0, c = 1; k < d; ++k) if (k != q) bspec[c++] = lower[k]; }
    if (g != h) g->call_mark = g->clock;
    DerivedTensor *base = nullptr;
    int rc = bary_get_tensor(g, bspec.data(), &base);
    if (rc) return rc;
    if ((rc = bary_pack_g0(g, *base))) return rc;
    BaryG0 gs{};
    gs.nmem = nmem;
    gs.tps = g->g0_tps;
    gs.n0 = g->dims.n[0];
    for (int i = 0; i < nmem; ++i) {
        gs.order[i] = rel[i];
        gs.col[i] = col[i];
        gs.maxorder = std::max(gs.maxorder, rel[i]);
    }
    switch (g->plan.R) {
    case 1: return bary_launch_g0_seed1(g, *base, gs, pp, N, d_out, ostride, ooff, st);
    case 2: return bary_launch_g0_seed2(g, *base, gs, pp, N, d_out, ostride, ooff, st);
    }
    return launch_g0<0>(g, *base, gs, pp, N, d_out, ostride, ooff, st);
}

// How far does the spec lower + e_q come out of lower's GEMM from where its own GEMM puts it?  Differentiating after
// the contraction rounds differently from the reference's batch path, by an amount that depends on the data and that
// no cheap bound predicts (5-D Black-Scholes: delta out of the price tensor 1e-13, vega 7e-13, rho 1e-12, vanna out of
// the delta tensor along sigma 6e-12).  So it is MEASURED, once per handle and (lower, q): a probe batch -- a quarter
// interior points, a quarter domain corners, half mixtures of lo / hi / interior coordinates: the roundings are
// largest where the weights are -- goes through the slab launch and through the spec's own GEMM; returned is
// max |shared - own| / max |own| over it (infinity when the pair cannot run).  Caller holds h->mu; q's model exists.
static const int kProbePoints = 2048;
static double bary_pair_deviation(pcx_bary *h, const std::vector<int> &lower, int q) {
    std::vector<int> key = lower;
    key.push_back(q);
    auto it = h->pair_dev.find(key);
    if (it != h->pair_dev.end()) return it->second;
    // a probe that could not RUN (allocation, copy or launch failed) is not remembered: the pair stays ungrouped for this
    // call and is measured again by the next one; PCX_BARY_PROBE_LOG=1 reports it
    struct Forget {
        pcx_bary *h; const std::vector<int> &key; bool keep = false;
        ~Forget() {
            if (keep) return;
            h->pair_dev.erase(key);
            (void)hipGetLastError();
            if (getenv("PCX_BARY_PROBE_LOG")) fprintf(stderr, "[pcx] pair probe could not run: not cached, retried by the next call\n");
        }
    } forget{h, key};
    double &dev = h->pair_dev[key];
    dev = INFINITY;
    const int d = h->dims.d;
    // the domain from the outer nodes (Chebyshev points of the first kind: x_0 = mid - half cos(pi / 2n))
    std::vector<double> nodes((size_t)h->dims.sum_n);
    if (hipMemcpy(nodes.data(), h->d_nodes, nodes.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return dev;
    std::vector<double> lo(d), hi(d);
    for (int k = 0; k < d; ++k) {
        const int n = h->dims.n[k];
        const double a = nodes[h->dims.off[k]], b = nodes[h->dims.off[k] + n - 1];
        const double half = n > 1 ? 0.5 * (b - a) / std::cos(3.14159265358979323846 / (2.0 * n)) : 0.0;
        lo[k] = 0.5 * (a + b) - half;
        hi[k] = 0.5 * (a + b) + half;
    }
    const long N = kProbePoints;
    std::vector<double> P((size_t)N * d);
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); };
    for (long p = 0; p < N; ++p) {
        const int mode = (int)(p % 4);              // 0 interior, 1 corner, 2 / 3 a mix of lo, hi and interior coordinates
        for (int k = 0; k < d; ++k) {
            const uint32_t r = rnd();
            const double uni = lo[k] + (hi[k] - lo[k]) * ((double)(r >> 8) / 8388608.0);
            const int pick = mode == 0 ? 2 : (mode == 1 ? (int)(r & 1) : (int)(r % 3));
            P[(size_t)p * d + k] = pick == 0 ? lo[k] : (pick == 1 ? hi[k] : uni);
        }
    }
    DevBuf dp, dr, dout;
    if (dp.alloc(P.size() * sizeof(double)) || dr.alloc(P.size() * sizeof(double)) || dout.alloc((size_t)N * 2 * sizeof(double))) return dev;
    if (hipMemcpy(dp.p, P.data(), P.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return dev;
    const double *gp = dp.as<double>();
    if (q > 0) {
        SliderCols cols{};
        cols.nc = d;
        cols.col[0] = q;
        for (int k = 0, c = 1; k < d; ++k)
            if (k != q) cols.col[c++] = k;
        hipLaunchKernelGGL(k_gather_columns, dim3((unsigned)((N * d + 255) / 256)), dim3(256), 0, h->stream, dp.as<double>(), N, d,
                           cols, dr.as<double>());
        gp = dr.as<double>();
    }
    std::vector<int32_t> lspec(lower.begin(), lower.end()), uspec(lower.begin(), lower.end());
    ++uspec[q];
    const int rel = 1, col = 0;
    if (bary_launch_group(h, q, lspec.data(), &rel, &col, 1, gp, N, dout.as<double>(), 2, 0, h->stream)) return dev;
    DerivedTensor *own = nullptr;
    if (bary_get_tensor(h, uspec.data(), &own)) return dev;
    DerivedTensor *one[1] = {own};
    if (bary_launch(h, one, 1, own->slot, dp.as<double>(), N, dout.as<double>(), 2, 1, h->stream, &h->s_partial)) return dev;
    std::vector<double> R((size_t)N * 2);
    if (hipStreamSynchronize(h->stream) != hipSuccess ||
        hipMemcpy(R.data(), dout.p, R.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return dev;
    }
    double scale = 0.0, diff = 0.0;
    for (long p = 0; p < N; ++p) {
        scale = std::max(scale, std::fabs(R[2 * p + 1]));
        diff = std::max(diff, std::fabs(R[2 * p] - R[2 * p + 1]));
    }
    if (std::isfinite(diff) && std::isfinite(scale)) dev = scale > 0.0 ? diff / scale : (diff == 0.0 ? 0.0 : INFINITY);
    forget.keep = true;                           // measured (an infinite deviation included: non-finite model values)
    static const bool log = getenv("PCX_BARY_PROBE_LOG") != nullptr;
    if (log) {
        fprintf(stderr, "[pcx] pair probe (");
        for (int k = 0; k < d; ++k) fprintf(stderr, "%d%s", lower[k], k + 1 < d ? "," : "");
        fprintf(stderr, ") + e_%d out of one GEMM: %.3g of the scale from its own GEMM (tolerance %.3g)\n", q, dev, h->group_tol);
    }
    return dev;
}

// a group = the specs one slab GEMM serves: equal orders off dimension q, orders along q in [base, base + span]
struct BaryGroup { int q; int base; std::vector<int> members; };

// Which specs of a multi-spec launch share a GEMM (caller holds h->mu; may build sub-models and run probes).
//  * span >= 2 (opt-in, not probed): specs with equal orders along dimensions 1 .. d-1 and dim-0 orders within
//    [base, base + span].
//  * then PAIRS: a spec and the spec one order below it along any one dimension q (delta / gamma from the delta
//    tensor's GEMM, price / vega along the volatility axis, ...), found greedily from the highest total order down,
//    dimension 0 first; q > 0 runs on the sub-model with q in front (bary_rot), own streams only (its column-permuted
//    batch lives in the handle).  A pair is formed only when the probe has MEASURED the derived member within
//    h->group_tol of its own GEMM (bary_pair_deviation).
// N = the size of the CALL's batch: every piece of a pipelined host batch and every block of a fan-out is planned with it,
// so that a (point, spec) gets the same rounding whichever piece it lands in.
static void bary_plan_groups(pcx_bary *h, const int32_t *derivs, int m, long N, bool own_stream, std::vector<BaryGroup> &subs,
                             std::vector<char> &grouped) {
    const int d = h->dims.d;
    grouped.assign(m, 0);
    const int span = h->g0_span;
    if (!(span > 0 && derivs && m > 1 && N >= kG0MinPoints && bary_effective_variant(h) == 2)) return;
    auto spec = [&](int s) { return std::vector<int>(derivs + (size_t)s * d, derivs + (size_t)(s + 1) * d); };
    if (span >= 2 && h->g0_ok) {
        std::map<std::vector<int>, std::vector<int>> by_key;       // orders[1:] -> specs, in column order
        for (int s = 0; s < m; ++s)
            by_key[std::vector<int>(derivs + (size_t)s * d + 1, derivs + (size_t)(s + 1) * d)].push_back(s);
        for (auto &kv : by_key) {
            std::vector<int> &mem = kv.second;
            if (mem.size() < 2) continue;
            std::sort(mem.begin(), mem.end(), [&](int a, int b) {
                const int oa = derivs[(size_t)a * d], ob = derivs[(size_t)b * d];
                return oa != ob ? oa < ob : a < b;
            });
            for (size_t i = 0; i < mem.size();) {
                const int base = derivs[(size_t)mem[i] * d];
                size_t e = i;
                while (e < mem.size() && derivs[(size_t)mem[e] * d] <= base + span && e - i < PCX_G0_MAX) ++e;
                if (e - i >= 2) {
                    subs.push_back(BaryGroup{0, base, std::vector<int>(mem.begin() + i, mem.begin() + e)});
                    for (size_t q = i; q < e; ++q) grouped[mem[q]] = 1;
                }
                i = e;
            }
        }
    }
    std::map<std::vector<int>, int> first;                          // orders -> first column still on its own
    std::vector<int> by_order;
    for (int s = 0; s < m; ++s)
        if (!grouped[s] && first.emplace(spec(s), s).second) by_order.push_back(s);
    auto total_order = [&](int s) { int t = 0; for (int k = 0; k < d; ++k) t += derivs[(size_t)s * d + k]; return t; };
    std::stable_sort(by_order.begin(), by_order.end(), [&](int a, int b) { return total_order(a) > total_order(b); });
    for (int b : by_order) {
        if (grouped[b]) continue;
        std::vector<int> lower = spec(b);
        for (int q = 0; q < d; ++q) {
            if (lower[q] < 1) continue;
            --lower[q];
            auto it = first.find(lower);
            ++lower[q];
            if (it == first.end() || grouped[it->second]) continue;
            if (q == 0 ? !h->g0_ok : !(own_stream && bary_rot(h, q))) continue;
            --lower[q];
            const double dev = bary_pair_deviation(h, lower, q);
            ++lower[q];
            if (!(dev <= h->group_tol)) continue;
            subs.push_back(BaryGroup{q, lower[q] - 1, {it->second, b}});
            grouped[it->second] = grouped[b] = 1;
            break;
        }
    }
}

// Multi-spec launch with shared contractions: specs (rows of `derivs`, m x d) one order apart along one dimension --
// price / delta, delta / gamma, price / vega -- share one slab-packed GEMM over the tensor of the lower order (the
// reference's own order in vectorized_eval_multi, barycentric.py:1098-1110: contract the other dimensions, then apply
// D_q); every other spec keeps its own GEMM, launched in runs of consecutive columns.  Large batches on the MFMA
// kernel only; results of grouped specs differ from the per-spec path by rounding (<= 2e-13 of the scale on 5-D
// Black-Scholes), as the reference's multi and batch paths do.  Caller holds h->mu.
static int bary_launch_specs(pcx_bary *h, const int32_t *derivs, DerivedTensor *const *dts, int m,
                             const double *const *frag_tab, const double *d_pts, long N, double *d_out, long ostride,
                             long ooff, hipStream_t st, Scratch *split_scratch, long N_call = -1) {
    const int d = h->dims.d;
    std::vector<BaryGroup> subs;
    std::vector<char> grouped;
    const bool own_stream = st == h->stream || (h->stage.second && st == h->stage.second);
    bary_plan_groups(h, derivs, m, N_call > 0 ? N_call : N, own_stream, subs, grouped);
    // runs of consecutive ungrouped specs: ordinary launches
    for (int s = 0; s < m;) {
        if (grouped[s]) { ++s; continue; }
        int e = s;
        while (e < m && !grouped[e]) ++e;
        int rc = bary_launch(h, dts + s, e - s, (e - s == 1) ? (const double *const *)dts[s]->slot : frag_tab + s, d_pts, N,
                             d_out, ostride, ooff + s, st, split_scratch);
        if (rc) return rc;
        s = e;
    }
    // the batch in the column order of every sub-model this call uses: one gather per dimension
    const double *rpts[PCX_MAX_DIMS] = {};
    {
        int nq = 0;
        for (const BaryGroup &sub : subs)
            if (sub.q > 0 && !rpts[sub.q]) { rpts[sub.q] = d_pts; ++nq; }
        if (nq) {
            Scratch &sc = (h->stage.second && st == h->stage.second) ? h->s_rot2 : h->s_rot;
            int rc = sc.reserve((size_t)nq * N * d * sizeof(double));
            if (rc) return rc;
            double *dst = (double *)sc.ptr;
            for (int q = 1; q < d; ++q) {
                if (!rpts[q]) continue;
                SliderCols cols{};
                cols.nc = d;
                cols.col[0] = q;
                for (int k = 0, c = 1; k < d; ++k)
                    if (k != q) cols.col[c++] = k;
                const long elems = N * d;
                hipLaunchKernelGGL(k_gather_columns, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, d_pts, N, d, cols, dst);
                HIP_TRY(hipGetLastError());
                rpts[q] = dst;
                dst += (size_t)N * d;
            }
        }
    }
    for (const BaryGroup &sub : subs) {
        std::vector<int32_t> lower(derivs + (size_t)sub.members[0] * d, derivs + (size_t)(sub.members[0] + 1) * d);
        lower[sub.q] = sub.base;
        int rel[PCX_G0_MAX], col[PCX_G0_MAX];
        const int nmem = (int)sub.members.size();
        for (int i = 0; i < nmem; ++i) {
            rel[i] = derivs[(size_t)sub.members[i] * d + sub.q] - sub.base;
            col[i] = sub.members[i];
        }
        int rc = bary_launch_group(h, sub.q, lower.data(), rel, col, nmem, sub.q == 0 ? d_pts : rpts[sub.q], N, d_out, ostride,
                                   ooff, st);
        if (rc) return rc;
    }
    return PCX_OK;
}

// GEMM launches a multi-spec call of N points would execute (groups count once); builds what the call would build.
extern "C" int pcx_bary_count_gemms(pcx_bary *h, const int32_t *derivs, int m, int64_t N, int32_t *gemms_out) {
    PCX_API_BEGIN
    if (!h || !derivs || !gemms_out || m < 1) return fail(PCX_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    std::vector<BaryGroup> subs;
    std::vector<char> grouped;
    bary_plan_groups(h, derivs, m, (long)N, true, subs, grouped);
    int count = (int)subs.size();
    for (int s = 0; s < m; ++s) count += !grouped[s];
    *gemms_out = count;
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_bary_eval_batch_dev(pcx_bary *h, const double *d_pts, int64_t N,
                                       const int32_t *deriv, double *d_out, void *stream) {
    PCX_API_BEGIN
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    if (N < 0) return fail(PCX_ERR_INVALID, "N=%lld < 0", (long long)N);
    if (N > 0 && (!d_pts || !d_out)) return fail(PCX_ERR_INVALID, "NULL device buffer");
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    h->call_mark = h->clock;
    DerivedTensor *dt = nullptr;
    int rc = bary_get_tensor(h, deriv, &dt);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    // split launches share the handle's scratch: only on the handle's own stream
    return bary_launch(h, &dt, 1, dt->slot, d_pts, (long)N, d_out, 1, 0, st,
                       st == h->stream ? &h->s_partial : nullptr);
    PCX_API_END
}

// The derived tensors of m specs (rows of `derivs`, m x d; NULL: the value) and the fragment table a launch of them
// reads: the single spec's own slot, else h->d_tab.  d_tab is rewritten only when the spec set changes, and only after
// the whole device has drained: launches still in flight on any stream may read it (device-resident calls return without
// waiting).  Caller holds h->mu.
PCX_HIDDEN int bary_spec_tensors(pcx_bary *h, const int32_t *derivs, int m, std::vector<DerivedTensor *> &dts,
                                 const double *const **frag_tab) {
    const int d = h->dims.d;
    dts.resize(m);
    for (int s = 0; s < m; ++s) {
        int rc = bary_get_tensor(h, derivs ? derivs + (size_t)s * d : nullptr, &dts[s]);
        if (rc) return rc;
    }
    *frag_tab = dts[0]->slot;
    const int eff = bary_effective_variant(h);
    if (m > 1 && (eff == 4 || eff == 5 || h->mfma_ok)) {
        std::vector<double *> tab(m);
        for (int s = 0; s < m; ++s) tab[s] = (eff == 4 || eff == 5) ? dts[s]->plain : dts[s]->frag;
        if (tab != h->tab_host) {
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(hipMemcpy(h->d_tab, tab.data(), m * sizeof(double *), hipMemcpyHostToDevice));
            h->tab_host = tab;
        }
        *frag_tab = h->d_tab;
    }
    return PCX_OK;
}

// m specs at N device-resident points into d_out (N x m row-major); groups of kMaxSpecs specs per launch.
extern "C" int pcx_bary_eval_multi_batch_dev(pcx_bary *h, const double *d_pts, int64_t N, const int32_t *derivs,
                                             int m, double *d_out, void *stream) {
    PCX_API_BEGIN
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    if (N < 0 || m < 1) return fail(PCX_ERR_INVALID, "bad N or m");
    if (!derivs) return fail(PCX_ERR_INVALID, "derivs is NULL");
    if (N == 0) return PCX_OK;
    if (!d_pts || !d_out) return fail(PCX_ERR_INVALID, "NULL device buffer");
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    h->call_mark = h->clock;
    const int d = h->dims.d;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    for (int s0 = 0; s0 < m; s0 += kMaxSpecs) {
        const int mc = std::min(kMaxSpecs, m - s0);
        std::vector<DerivedTensor *> dts;
        const double *const *frag_tab = nullptr;
        int rc = bary_spec_tensors(h, derivs + (size_t)s0 * d, mc, dts, &frag_tab);
        if (rc) return rc;
        rc = bary_launch_specs(h, derivs + (size_t)s0 * d, dts.data(), mc, frag_tab, d_pts, (long)N, d_out, m, s0, st,
                               st == h->stream ? &h->s_partial : nullptr);
        if (rc) return rc;
    }
    return PCX_OK;
    PCX_API_END
}

// N_call: the batch of the API call this block belongs to (fan-out blocks pass the whole call's N), -1 = N itself
static int bary_eval_host(pcx_bary *h, const double *pts, int64_t N, const int32_t *derivs, int m,
                          double *out, int64_t N_call = -1) {
    if (N_call < N) N_call = N;
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    if (N < 0 || m < 1) return fail(PCX_ERR_INVALID, "bad N or m");
    if (N > 0 && (!pts || !out)) return fail(PCX_ERR_INVALID, "NULL buffer");
    if (m > kMaxSpecs)
        return eval_spec_groups(N, derivs, h->dims.d, m, out, [&](const int32_t *group, int mc, double *part) {
            return bary_eval_host(h, pts, N, group, mc, part, N_call);
        });
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    h->call_mark = h->clock;
    const int d = h->dims.d;
    std::vector<DerivedTensor *> dts;
    const double *const *frag_tab = nullptr;
    int rc = bary_spec_tensors(h, derivs, m, dts, &frag_tab);
    if (rc) return rc;
    // pieces of 2^18 points (10 MB of 5-D coordinates); low-dimensional models take more points per piece so that a
    // piece still moves ~10 MB (12 x 12 at 2x10^7 points: 4 MB pieces ran the path at 13 GB/s).  Two slots from two
    // pieces on, behind a short first piece (one round of workgroups): the first kernel starts after 2.6 MB instead of
    // 10 MB of upload, and nothing overlaps the first upload.
    const int64_t piece = std::min<int64_t>((int64_t)1 << 21, std::max<int64_t>(kPipeChunkPoints, (((int64_t)10 << 20) / (d * 8)) & ~(int64_t)65535));
    const StagePlan plan = N >= 2 * piece ? StagePlan{1 << 16, piece, true, true} : StagePlan{kChunkPoints, kChunkPoints, false, true};
    // every piece, the zero-copy window included, is planned with the call's N (bary_plan_groups); split launches share
    // the handle's s_partial, so the second slot launches without it
    return stage_host_batch(h->stage, h->device, h->stream, pts, N, d, m, out, plan,
                            [&](int slot, hipStream_t st, const double *dp, long cnt, double *dout) {
                                return bary_launch_specs(h, derivs, dts.data(), m, frag_tab, dp, cnt, dout, m, 0, st,
                                                         slot ? nullptr : &h->s_partial, (long)N_call);
                            });
}

extern "C" int pcx_bary_eval_batch(pcx_bary *h, const double *pts, int64_t N, const int32_t *deriv,
                                   double *out) {
    PCX_API_BEGIN
    return bary_eval_host(h, pts, N, deriv, 1, out);
    PCX_API_END
}

extern "C" int pcx_bary_eval_multi_batch(pcx_bary *h, const double *pts, int64_t N,
                                         const int32_t *derivs, int m, double *out) {
    PCX_API_BEGIN
    if (!derivs) return fail(PCX_ERR_INVALID, "derivs is NULL");
    return bary_eval_host(h, pts, N, derivs, m, out);
    PCX_API_END
}

// ---- all equal-shape pieces of a piecewise interpolant in one launch (called from pcx_spline.hip) ---------------
template <int DOUT, int NLP>
static void launch_small_pieces_t(const pcx_bary *p0, const SplinePieceModel *models, const int *blk_piece,
                                  const int *blk_first, const int *piece_end, int m, long blocks, const double *dp,
                                  double *dout, const int *perm, hipStream_t st) {
    auto kern = k_bary_small_pieces<DOUT, NLP>;
    const size_t lds = (size_t)(p0->dims.sum_n - p0->dims.n[DOUT]) * 64 * sizeof(double);
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(64), lds, st, p0->dims, models, blk_piece, blk_first, piece_end, m,
                       dp, dout, (long)m, 0L, perm);
}

template <int DOUT>
static int launch_small_pieces_d(const pcx_bary *p0, const SplinePieceModel *models, const int *blk_piece,
                                 const int *blk_first, const int *piece_end, int m, long blocks, const double *dp,
                                 double *dout, const int *perm, hipStream_t st) {
    switch (p0->small_nlp) {
#define CASE_NLP(v) case v: launch_small_pieces_t<DOUT, v>(p0, models, blk_piece, blk_first, piece_end, m, blocks, dp, dout, perm, st); return PCX_OK;
    CASE_NLP(2) CASE_NLP(3) CASE_NLP(4) CASE_NLP(5) CASE_NLP(6) CASE_NLP(7) CASE_NLP(8) CASE_NLP(9) CASE_NLP(10) CASE_NLP(11)
    CASE_NLP(12) CASE_NLP(13) CASE_NLP(14) CASE_NLP(15) CASE_NLP(16) CASE_NLP(24) CASE_NLP(32) CASE_NLP(48) CASE_NLP(64)
#undef CASE_NLP
    }
    return fail(PCX_ERR_UNSUPPORTED, "lane-per-point kernel does not cover this shape");
}

// All non-empty pieces in one launch.  Returns PCX_OK with *done = false when the batch does not qualify
// (a piece forced onto another kernel form): the caller then launches per piece.
template <int NL>
static int launch_sq_pieces_t(const pcx_bary *p0, const SplinePieceModel *models, const int *blk_piece, const int *blk_first,
                              const int *piece_end, int m, long blocks, const double *dp, double *dout, const int *perm,
                              hipStream_t st) {
    const int d = p0->dims.d;
    size_t lds = 0;
    for (int k = 0; k < d - 2; ++k) lds += (size_t)p0->dims.n[k] * 64 * sizeof(double);
#define PCX_SQP_GO(LEAD)                                                                                              \
    hipLaunchKernelGGL((k_bary_sq_pieces<NL, LEAD>), dim3((unsigned)blocks), dim3(64), lds, st, p0->dims, models, blk_piece, \
                       blk_first, piece_end, m, dp, dout, (long)m, 0L, perm)
    if (d == 2) PCX_SQP_GO(0);
    else if (d == 3) PCX_SQP_GO(1);
    else PCX_SQP_GO(2);
#undef PCX_SQP_GO
    return PCX_OK;
}

PCX_HIDDEN int bary_launch_sq_pieces(const pcx_bary *p0, const SplinePieceModel *models, const int *blk_piece, const int *blk_first,
                            const int *piece_end, int m, long blocks, const double *dp, double *dout, const int *perm,
                            hipStream_t st) {
    switch (p0->sq_nl) {
#define CASE_NL(v) case v: return launch_sq_pieces_t<v>(p0, models, blk_piece, blk_first, piece_end, m, blocks, dp, dout, perm, st);
    CASE_NL(4) CASE_NL(5) CASE_NL(6) CASE_NL(7) CASE_NL(8) CASE_NL(9) CASE_NL(10) CASE_NL(11) CASE_NL(12) CASE_NL(13)
    CASE_NL(14) CASE_NL(15) CASE_NL(16) CASE_NL(17) CASE_NL(18) CASE_NL(19) CASE_NL(20) CASE_NL(21) CASE_NL(22)
    CASE_NL(23) CASE_NL(24) CASE_NL(26) CASE_NL(28) CASE_NL(30) CASE_NL(32)
#undef CASE_NL
    }
    return fail(PCX_ERR_UNSUPPORTED, "square-trailing lane-per-point kernel does not cover this piece shape");
}
PCX_HIDDEN int bary_launch_small_pieces(int dout, const pcx_bary *p0, const SplinePieceModel *models, const int *blk_piece,
                                        const int *blk_first, const int *piece_end, int m, long blocks, const double *dp,
                                        double *dout_buf, const int *perm, hipStream_t st) {
    switch (dout) {
    case 0: return launch_small_pieces_d<0>(p0, models, blk_piece, blk_first, piece_end, m, blocks, dp, dout_buf, perm, st);
    case 1: return launch_small_pieces_d<1>(p0, models, blk_piece, blk_first, piece_end, m, blocks, dp, dout_buf, perm, st);
    case 2: return launch_small_pieces_d<2>(p0, models, blk_piece, blk_first, piece_end, m, blocks, dp, dout_buf, perm, st);
    case 3: return launch_small_pieces_d<3>(p0, models, blk_piece, blk_first, piece_end, m, blocks, dp, dout_buf, perm, st);
    }
    return fail(PCX_ERR_UNSUPPORTED, "lane-per-point kernel covers d <= 4");
}

// ---------------------------------------------------------------------------------
// Single-process fan-out over several devices (contiguous row blocks, model replicated, "G parallel
// D2H copies straight into the host result", no collective).  handles[g] is the same model on device g (the same
// device may appear twice: two handles then pipeline on it); block g = rows [g ceil(N/G), min(N, (g+1) ceil(N/G)))
// is evaluated by the ordinary host-pointer path of handle g on its own host thread, its download landing in the
// caller's `out` slice.  pin != 0 page-locks the caller's arrays for the duration of the call (hipHostRegister,
// portable): the copies then run asynchronously at PCIe rate instead of through the driver's pageable staging.
// A point's result does not depend on the block it lands in: every block of a grouped multi-spec launch is planned with
// the call's N (bary_plan_groups).
// ---------------------------------------------------------------------------------
extern "C" int pcx_bary_group_eval_multi_batch(pcx_bary *const *handles, int n_handles, const double *pts, int64_t N,
                                               const int32_t *derivs, int m, double *out, int pin) {
    PCX_API_BEGIN
    if (!handles || n_handles < 1) return fail(PCX_ERR_INVALID, "no handles");
    for (int g = 0; g < n_handles; ++g) {
        if (!handles[g]) return fail(PCX_ERR_INVALID, "handle %d is NULL", g);
        if (handles[g]->dims.d != handles[0]->dims.d || handles[g]->total != handles[0]->total)
            return fail(PCX_ERR_INVALID, "handle %d holds a different model", g);
    }
    if (N < 0 || m < 1) return fail(PCX_ERR_INVALID, "bad N or m");
    if (N > 0 && (!pts || !out)) return fail(PCX_ERR_INVALID, "NULL buffer");
    const int d = handles[0]->dims.d;
    return fan_out_host(n_handles, handles[0]->device, pin, N, pts, (size_t)N * d * sizeof(double), out,
                        (size_t)N * m * sizeof(double), [&](int g, int64_t lo, int64_t cnt) {
                            return bary_eval_host(handles[g], pts + (size_t)lo * d, cnt, derivs, m, out + (size_t)lo * m, N);
                        });
    PCX_API_END
}

extern "C" int pcx_bary_derivative_tensor(pcx_bary *h, const int32_t *deriv, double *tensor_out) {
    PCX_API_BEGIN
    if (!h || !tensor_out) return fail(PCX_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    h->call_mark = h->clock;
    DerivedTensor *dt = nullptr;
    int rc = bary_get_tensor(h, deriv, &dt);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(tensor_out, dt->plain, h->total * sizeof(double), hipMemcpyDeviceToHost));
    return PCX_OK;
    PCX_API_END
}

// ---------------------------------------------------------------------------------
// Chebyshev coefficients and Sobol indices (reference _sensitivity.py)
// ---------------------------------------------------------------------------------
// Per dimension the reference reverses the values, applies a DCT-II, divides by n and halves c_0 (_sensitivity.py:14-49):
// M[m, i] = (2 / n) cos(pi m (2 (n-1-i) + 1) / (2n)), row 0 halved.  The angle is reduced to [0, 2 pi) in integers
// first, so every entry is a correctly reduced cosine whatever n.  Uploaded once per handle, laid out like d_diff.
static int bary_cheb_matrices(pcx_bary *h) {
    if (h->d_cheb) return PCX_OK;
    const int d = h->dims.d;
    std::vector<double> M((size_t)h->doff[d - 1] + (size_t)h->dims.n[d - 1] * h->dims.n[d - 1]);
    for (int k = 0; k < d; ++k) {
        const long n = h->dims.n[k];
        double *Mk = M.data() + h->doff[k];
        for (long m = 0; m < n; ++m)
            for (long i = 0; i < n; ++i) {
                const long p = (m * (2 * (n - 1 - i) + 1)) % (4 * n);      // angle = pi p / (2n)
                Mk[m * n + i] = (2.0 / (double)n) * std::cos(M_PI * (double)p / (2.0 * (double)n)) * (m == 0 ? 0.5 : 1.0);
            }
    }
    DevBuf b;
    int rc = b.alloc(M.size() * sizeof(double));
    if (rc) return rc;
    HIP_TRY(hipMemcpy(b.p, M.data(), M.size() * sizeof(double), hipMemcpyHostToDevice));
    h->d_cheb = b.release<double>();
    return PCX_OK;
}

// The coefficient tensor of the handle's values: d k_mode_product passes (dimension 0 first) ping-ponging between the
// handle's two coefficient scratch buffers; *coeffs points into one of them.  Everything is allocated before the first
// launch.  Caller holds h->mu.  Work is enqueued on h->stream.
static int bary_cheb_coeffs(pcx_bary *h, const double **coeffs) {
    int rc = bary_cheb_matrices(h);
    if (rc) return rc;
    DerivedTensor *base = nullptr;
    if ((rc = bary_get_tensor(h, nullptr, &base))) return rc;
    for (Scratch &sc : h->s_cheb)
        if ((rc = sc.reserve((size_t)h->total * sizeof(double)))) return rc;
    const int d = h->dims.d;
    const double *src = base->plain;
    double *dst = (double *)h->s_cheb[0].ptr, *other = (double *)h->s_cheb[1].ptr;
    const int blocks = (int)((h->total + 255) / 256);
    for (int k = 0; k < d; ++k) {
        long outer = 1, inner = 1;
        for (int q = 0; q < k; ++q) outer *= h->dims.n[q];
        for (int q = k + 1; q < d; ++q) inner *= h->dims.n[q];
        hipLaunchKernelGGL(k_mode_product, dim3(blocks), dim3(256), 0, h->stream, src, dst, h->d_cheb + h->doff[k], outer,
                           h->dims.n[k], inner);
        src = dst;
        std::swap(dst, other);
    }
    HIP_TRY(hipGetLastError());
    *coeffs = src;
    return PCX_OK;
}

extern "C" int pcx_bary_chebyshev_coefficients(pcx_bary *h, double *coeffs_out) {
    PCX_API_BEGIN
    if (!h || !coeffs_out) return fail(PCX_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    h->call_mark = h->clock;
    const double *coeffs = nullptr;
    int rc = bary_cheb_coeffs(h, &coeffs);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(coeffs_out, coeffs, (size_t)h->total * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_bary_sobol(pcx_bary *h, double *variance_out, double *first_out, double *total_out) {
    PCX_API_BEGIN
    if (!h || !variance_out || !first_out || !total_out) return fail(PCX_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    h->call_mark = h->clock;
    const int d = h->dims.d;
    SobolDims sd{};
    sd.L = h->dims.n[d - 1];
    sd.rows = h->total / sd.L;
    int W = 1;
    while (W < 64 && W < sd.L) W <<= 1;
    for (sd.lw = 0; (1 << sd.lw) < W; ++sd.lw) {}
    for (int k = 0; k < PCX_MAX_DIMS; ++k) sd.n[k] = k < d ? (unsigned)h->dims.n[k] : 1u;
    sd.pid = 1.0;
    for (int k = 0; k < d; ++k) sd.pid *= M_PI;
    const long per_block = (long)(PCX_SOBOL_THREADS / 64) * (64 / W) * PCX_SOBOL_UNROLL;     // rows per block pass
    const int blocks = (int)std::min<long>(PCX_SOBOL_MAX_BLOCKS, (sd.rows + per_block - 1) / per_block);
    const int S = PCX_SOBOL_SLOTS(d);
    int rc = h->s_sobol.reserve(((size_t)blocks + 1) * S * sizeof(double));     // slab rows, then the result row
    if (rc) return rc;
    double *slab = (double *)h->s_sobol.ptr, *res = slab + (size_t)blocks * S;
    const double *coeffs = nullptr;
    if ((rc = bary_cheb_coeffs(h, &coeffs))) return rc;
    const bool narrow = sd.rows <= 0xffffffffL;
    switch (d) {
#define CASE_D(v)                                                                                                        \
    case v:                                                                                                              \
        if (narrow) hipLaunchKernelGGL((k_sobol_energy<v, unsigned>), dim3(blocks), dim3(PCX_SOBOL_THREADS), 0, h->stream, \
                                       coeffs, slab, sd);                                                   \
        else hipLaunchKernelGGL((k_sobol_energy<v, unsigned long long>), dim3(blocks), dim3(PCX_SOBOL_THREADS), 0,       \
                                h->stream, coeffs, slab, sd);                                               \
        break;
        CASE_D(1) CASE_D(2) CASE_D(3) CASE_D(4) CASE_D(5) CASE_D(6) CASE_D(7) CASE_D(8)
        CASE_D(9) CASE_D(10) CASE_D(11) CASE_D(12) CASE_D(13) CASE_D(14) CASE_D(15) CASE_D(16)
#undef CASE_D
        default: return fail(PCX_ERR_INVALID, "d=%d outside [1, %d]", d, PCX_MAX_DIMS);
    }
    hipLaunchKernelGGL(k_sobol_finish, dim3(1), dim3(PCX_SOBOL_FINISH_THREADS), 0, h->stream,
                       (const double *)slab, blocks, S, res);
    HIP_TRY(hipGetLastError());
    double r[PCX_SOBOL_SLOTS(PCX_MAX_DIMS)];
    HIP_TRY(hipMemcpyAsync(r, res, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (r[S - 1] != 0.0)
        return fail(PCX_ERR_INVALID, "coefficients contain NaN or Inf; sobol_indices() requires finite spectral coefficients");
    // the reference's rules (_sensitivity.py:87-140): one dimension -> 1.0 / 1.0 when there is any variance;
    // no variance -> every index 0.0
    const double var = r[0];
    for (int k = 0; k < d; ++k) {
        if (d == 1) {
            first_out[k] = total_out[k] = var > 0.0 ? 1.0 : 0.0;
        } else if (var == 0.0) {
            first_out[k] = total_out[k] = 0.0;
        } else {
            first_out[k] = r[1 + k] / var;
            total_out[k] = r[1 + d + k] / var;
        }
    }
    *variance_out = var;
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_tensor_contract_axis(int device, int d, const int32_t *n_nodes, const double *tensor,
                                        int axis, const double *vec, double *out) {
    PCX_API_BEGIN
    if (d < 1 || d > PCX_MAX_DIMS || !n_nodes || !tensor || !vec || !out) return fail(PCX_ERR_INVALID, "bad argument");
    if (axis < 0 || axis >= d) return fail(PCX_ERR_INVALID, "axis %d outside [0, %d)", axis, d);
    long outer = 1, inner = 1;
    for (int k = 0; k < d; ++k) {
        if (n_nodes[k] < 1) return fail(PCX_ERR_INVALID, "n_nodes[%d] < 1", k);
        if (k < axis) outer *= n_nodes[k];
        if (k > axis) inner *= n_nodes[k];
    }
    const int na = n_nodes[axis];
    int rc = use_device(device);
    if (rc) return rc;
    DevBuf din, dvec, dout;
    HIP_TRY(hipMalloc(&din.p, (size_t)outer * na * inner * sizeof(double)));
    HIP_TRY(hipMalloc(&dvec.p, (size_t)na * sizeof(double)));
    HIP_TRY(hipMalloc(&dout.p, (size_t)outer * inner * sizeof(double)));
    HIP_TRY(hipMemcpy(din.p, tensor, (size_t)outer * na * inner * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dvec.p, vec, (size_t)na * sizeof(double), hipMemcpyHostToDevice));
    long cnt = outer * inner;
    hipLaunchKernelGGL(k_contract_axis, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, 0, (const double *)din.p,
                       (double *)dout.p, (const double *)dvec.p, outer, na, inner);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout.p, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost));
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_bary_set_kernel(pcx_bary *h, int variant) {
    PCX_API_BEGIN
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    if (variant < 0 || variant > 5) return fail(PCX_ERR_INVALID, "variant %d outside [0, 5]", variant);
    static const char *const kName[] = {"MFMA", "4x4x4 MFMA", "lane-per-point", "square-trailing lane-per-point"};
    if (variant >= 2 && !bary_plan_has_variant(*h, variant))
        return fail(PCX_ERR_UNSUPPORTED, "%s kernel does not cover this shape", kName[variant - 2]);
    std::lock_guard<std::mutex> lk(h->mu);
    h->variant = variant;
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_bary_set_group_span(pcx_bary *h, int span) {
    PCX_API_BEGIN
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    if (span < 0 || span > 8) return fail(PCX_ERR_INVALID, "span %d outside [0, 8]", span);
    std::lock_guard<std::mutex> lk(h->mu);
    h->g0_span = span;
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_bary_set_group_tolerance(pcx_bary *h, double tol) {
    PCX_API_BEGIN
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    if (!(tol >= 0.0)) return fail(PCX_ERR_INVALID, "tolerance must be >= 0");
    std::lock_guard<std::mutex> lk(h->mu);
    h->group_tol = tol;
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_bary_kernel_info(pcx_bary *h, int32_t *info) {
    PCX_API_BEGIN
    if (!h || !info) return fail(PCX_ERR_INVALID, "NULL argument");
    bary_plan_kernel_info(*h, h->dims, info);
    return PCX_OK;
    PCX_API_END
}

// [0] workgroups of the row-code MFMA kernel the device holds at once (launch_mfma_t's `slots`, for batches of 65,536
// points or more), [1] points per workgroup there, [2] chunks of row tiles, [3] the tail-split mode (PCX_BARY_TAIL:
// 0 never, 1 where it pays, 2 wherever the geometry allows), [4] workgroups per tail block in the latest row-code launch (0: it was not split) and
// [5] its tail blocks.  All zero when launches do not take the row-code form.
extern "C" int pcx_bary_tail_info(pcx_bary *h, int32_t *info) {
    PCX_API_BEGIN
    if (!h || !info) return fail(PCX_ERR_INVALID, "NULL argument");
    bary_plan_tail_info(*h, info);
    std::lock_guard<std::mutex> lk(h->mu);
    if (!bary_plan_rowcode_form(*h)) return PCX_OK;
    if (!h->slots[h->nt - 1]) {
        int rc = use_device(h->device);
        if (rc) return rc;
        h->slots_query = true;           // the launch tables know the instantiation: they fill h->slots and return
        switch (h->plan.R) {
        case 1: rc = bary_launch_rowcode_seed1(h, nullptr, 1, nullptr, 65536, nullptr, 1, 0, h->stream, nullptr, nullptr); break;
        case 2: rc = bary_launch_rowcode_seed2(h, nullptr, 1, nullptr, 65536, nullptr, 1, 0, h->stream, nullptr, nullptr); break;
        default: rc = launch_rowcode<0>(h, nullptr, 1, nullptr, 65536, nullptr, 1, 0, h->stream, nullptr, nullptr);
        }
        h->slots_query = false;
        if (rc) return rc;
    }
    info[0] = h->slots[h->nt - 1];
    info[4] = h->last_tail_P;
    info[5] = h->last_tail_blocks;
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_bary_grid_info(pcx_bary *h, int32_t *info) {
    PCX_API_BEGIN
    if (!h || !info) return fail(PCX_ERR_INVALID, "NULL argument");
    bary_plan_grid_info(*h, info);
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_bary_stream(pcx_bary *h, void **stream) {
    PCX_API_BEGIN
    if (!h || !stream) return fail(PCX_ERR_INVALID, "NULL argument");
    *stream = (void *)h->stream;
    return PCX_OK;
    PCX_API_END
}
