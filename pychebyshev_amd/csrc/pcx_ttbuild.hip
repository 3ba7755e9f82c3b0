// pcx_ttbuild.hip -- C ABI of libpcx_hip.so (see include/pcx.h): the dense steps of the TT-Cross and TT-SVD builds,
// and the rounding and adjacent swaps of TT algebra.
// gfx950 only.

#include "pcx_internal.h"
#include "ttcross_kernels.h"
#include "ttsvd_kernels.h"
#include "tt_round_kernels.h"

// ---------------------------------------------------------------------------------
// TT-Cross build steps
// ---------------------------------------------------------------------------------

extern "C" int pcx_tt_value_to_coeff_core(int device, const double *value_core, int rl, int n, int rr,
                                          double *coeff_core) {
    PCX_API_BEGIN
    if (!value_core || !coeff_core || rl < 1 || n < 1 || rr < 1) return fail(PCX_ERR_INVALID, "bad argument");
    int rc = use_device(device);
    if (rc) return rc;
    size_t cnt = (size_t)rl * n * rr;
    DevBuf in, out;
    if ((rc = in.alloc(cnt * sizeof(double)))) return rc;
    if ((rc = out.alloc(cnt * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpy(in.p, value_core, cnt * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_value_to_coeff_core, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, 0,
                       in.as<double>(), out.as<double>(), rl, n, rr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(coeff_core, out.p, cnt * sizeof(double), hipMemcpyDeviceToHost));
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_tt_grid_eval(int device, int d, const int32_t *n_nodes, const int32_t *ranks,
                                const double *value_cores_cat, const int32_t *idx, int count,
                                double *out) {
    PCX_API_BEGIN
    if (d < 1 || d > PCX_MAX_DIMS || !n_nodes || !ranks || !value_cores_cat || count < 0) return fail(PCX_ERR_INVALID, "bad argument");
    if (count == 0) return PCX_OK;
    if (!idx || !out) return fail(PCX_ERR_INVALID, "NULL buffer");
    int rc = use_device(device);
    if (rc) return rc;
    std::vector<long> coff(d);
    long core_total = 0;
    int rmax = 1;
    for (int k = 0; k < d; ++k) {
        if (n_nodes[k] < 1 || ranks[k] < 1 || ranks[k + 1] < 1) return fail(PCX_ERR_INVALID, "bad n_nodes/ranks at dim %d", k);
        coff[k] = core_total;
        core_total += (long)ranks[k] * n_nodes[k] * ranks[k + 1];
        rmax = std::max(rmax, std::max(ranks[k], ranks[k + 1]));
    }
    for (long i = 0; i < (long)count * d; ++i)
        if (idx[i] < 0 || idx[i] >= n_nodes[i % d]) return fail(PCX_ERR_INVALID, "grid index out of range");
    DevBuf dn, dr, dc, dcores, didx, dout, dwork;
    if ((rc = dn.alloc(d * sizeof(int)))) return rc;
    if ((rc = dr.alloc((d + 1) * sizeof(int)))) return rc;
    if ((rc = dc.alloc(d * sizeof(long)))) return rc;
    if ((rc = dcores.alloc(core_total * sizeof(double)))) return rc;
    if ((rc = didx.alloc((size_t)count * d * sizeof(int)))) return rc;
    if ((rc = dout.alloc((size_t)count * sizeof(double)))) return rc;
    if ((rc = dwork.alloc((size_t)count * 2 * rmax * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpy(dn.p, n_nodes, d * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dr.p, ranks, (d + 1) * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dc.p, coff.data(), d * sizeof(long), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dcores.p, value_cores_cat, core_total * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(didx.p, idx, (size_t)count * d * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_tt_grid_eval, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, 0, d, dn.as<int>(),
                       dr.as<int>(), dc.as<long>(), dcores.as<double>(), didx.as<int>(), count,
                       dout.as<double>(), dwork.as<double>(), rmax);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout.p, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
    return PCX_OK;
    PCX_API_END
}

// ---------------------------------------------------------------------------------
// Row-Jacobi factorisation shared by TT-SVD, TT rounding and TT swaps
// ---------------------------------------------------------------------------------

// Grow-only work buffers of a sequence of factorisations.
struct JacobiWork {
    Scratch sU, snrm, sG;
    DevBuf drot;                 // {pairs rotated, pairs rotated that were > 1e-8 from orthogonal}
    std::vector<double> hnorm;   // squared row norms of B after the last factorisation
    ~JacobiWork() { sU.release(); snrm.release(); sG.release(); }
};

// Factor the m x N matrix C in `cur` (row stride N) as C = U B by the row-Jacobi iteration of ttsvd_kernels.h:
// on return cur holds B, whose rows are mutually orthogonal, w.sU the m x m rotation product U (row-major) and
// w.hnorm the squared row norms of B.  `nxt` (m x N doubles at least) is work space for the Gram preconditioner,
// which swaps the two buffers.  tol > 0 leaves pairs far below the cut tol * sigma_max unrotated (see
// k_rowjacobi_step); tol = 0 rotates every pair above the noise floor.
static int rowjacobi_factor(DevBuf &cur, DevBuf &nxt, int m, long N, double tol, JacobiWork &w, int &sweeps_total) {
    int rc;
    if (!w.drot.p && (rc = w.drot.alloc(2 * sizeof(int)))) return rc;
    if ((rc = w.sU.reserve((size_t)m * m * sizeof(double)))) return rc;
    if ((rc = w.snrm.reserve((size_t)m * sizeof(double)))) return rc;
    DevView U{w.sU.ptr}, nrm{w.snrm.ptr};
    DevBuf &drot = w.drot;
    Scratch &sG = w.sG;
    std::vector<double> &hnorm = w.hnorm;
    hipLaunchKernelGGL(k_set_identity, dim3((unsigned)(((long)m * m + 255) / 256)), dim3(256), 0, 0, U.as<double>(), m);
    const int mp = (m + 1) & ~1;
    // squared norm of the largest row bounds sigma_max^2 from below (and sigma_max^2 <= m times it)
    hipLaunchKernelGGL(k_row_sqnorms, dim3(m), dim3(TTSVD_THREADS), 0, 0, cur.as<double>(), N, N, nrm.as<double>());
    hnorm.resize(m);
    HIP_TRY(hipMemcpy(hnorm.data(), nrm.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
    double fro2 = 0.0;
    for (int i = 0; i < m; ++i) fro2 += hnorm[i];
    const double eps64 = 8.0 * 2.220446049250313e-16;   // rows below 8 eps ||C||_F: noise
    const double floor2 = eps64 * eps64 * fro2;
    // pairs of rows whose squared norms add up to less than (tol * largest row norm)^2 / m are not rotated
    // against each other: see k_rowjacobi_step
    double row_max2 = 0.0;
    for (int i = 0; i < m; ++i) row_max2 = std::max(row_max2, hnorm[i]);
    const double sig2 = tol * tol * row_max2 / (double)m;
    const double rot_tol = std::max(1e-15, 2.0 * 2.220446049250313e-16 * std::sqrt((double)N));
    size_t lds_rows = (size_t)m * N * sizeof(double);
    if (m > 1 && lds_rows <= 144 * 1024) {
        // small unfolding: the whole iteration in one workgroup, rows (and U when it fits) in LDS, one launch
        const int u_in_lds = (lds_rows + (size_t)m * m * sizeof(double) <= 156 * 1024) ? 1 : 0;
        if (u_in_lds) lds_rows += (size_t)m * m * sizeof(double);
        if (lds_rows > 48 * 1024)
            HIP_TRY(hipFuncSetAttribute((const void *)k_rowjacobi_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_rows));
        HIP_TRY(hipMemsetAsync(drot.p, 0, sizeof(int), 0));
        hipLaunchKernelGGL(k_rowjacobi_lds, dim3(1), dim3(TTSVD_LDS_THREADS), lds_rows, 0, cur.as<double>(), m, (int)N,
                           U.as<double>(), floor2, rot_tol, sig2, 60, drot.as<int>(), u_in_lds);
        HIP_TRY(hipGetLastError());
        int sw = 0;
        HIP_TRY(hipMemcpy(&sw, drot.p, sizeof(int), hipMemcpyDeviceToHost));
        sweeps_total += sw;
    } else if (m > 1) {
        // large unfolding: one launch per tournament step, a sweep's (mp - 1) launches recorded once
        // in a hipGraph and replayed per sweep (the host could not issue ~100 tiny launches per
        // sweep at the rate the device finishes them: ~4 us each against ~1.5 us per boundary)
        // Gram preconditioner (ttsvd_kernels.h): rotations found on the m x m matrix C C^T in LDS make the
        // rows nearly orthogonal before the accurate row iteration starts
        const size_t lds_sym = ((size_t)2 * m * m + 2 * ((m + 1) / 2 + 1)) * sizeof(double) + (size_t)(m + 2) * sizeof(int);
        if (N > 2L * m && lds_sym <= 156 * 1024) {
            if ((rc = sG.reserve((size_t)m * m * sizeof(double)))) return rc;
            DevView G{sG.ptr};
            hipLaunchKernelGGL(k_gram_rows, dim3(m, m), dim3(TTSVD_THREADS), 0, 0, cur.as<double>(), N, m, N, G.as<double>());
            if (lds_sym > 48 * 1024)
                HIP_TRY(hipFuncSetAttribute((const void *)k_symjacobi_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_sym));
            hipLaunchKernelGGL(k_symjacobi_lds, dim3(1), dim3(TTSVD_LDS_THREADS), lds_sym, 0, G.as<double>(), m, U.as<double>(),
                               std::max(floor2, 1e-13 * fro2), 1e-9, 30);
            hipLaunchKernelGGL(k_apply_vt, dim3((unsigned)((N + 255) / 256), m), dim3(256), 0, 0, cur.as<double>(), N, m, N,
                               U.as<double>(), nxt.as<double>());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipDeviceSynchronize());
            std::swap(cur.p, nxt.p);
        }
        if (mp - 1 <= 16) {
            // a short tournament (the 11-row first unfolding): plain launches, no graph to build
            for (int sweep = 0; sweep < 60; ++sweep) {
                HIP_TRY(hipMemsetAsync(drot.p, 0, 2 * sizeof(int), 0));
                for (int step = 0; step < mp - 1; ++step)
                    hipLaunchKernelGGL(k_rowjacobi_step, dim3(mp / 2), dim3(TTSVD_THREADS), 0, 0, cur.as<double>(), N, m, N,
                                       U.as<double>(), step, drot.as<int>(), floor2, rot_tol, sig2);
                HIP_TRY(hipGetLastError());
                int rotated[2] = {0, 0};
                HIP_TRY(hipMemcpy(rotated, drot.p, 2 * sizeof(int), hipMemcpyDeviceToHost));
                ++sweeps_total;
                if (rotated[1] == 0) break;
            }
        } else {
        hipStream_t cs = nullptr;
        HIP_TRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        auto cleanup = [&]() {
            if (exec) (void)hipGraphExecDestroy(exec);
            if (graph) (void)hipGraphDestroy(graph);
            (void)hipStreamDestroy(cs);
        };
        HIP_TRY(hipDeviceSynchronize());       // the identity / norm kernels above ran on the NULL stream
        hipError_t ge = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
        if (ge == hipSuccess) {
            for (int step = 0; step < mp - 1; ++step)
                hipLaunchKernelGGL(k_rowjacobi_step, dim3(mp / 2), dim3(TTSVD_THREADS), 0, cs, cur.as<double>(), N, m, N,
                                   U.as<double>(), step, drot.as<int>(), floor2, rot_tol, sig2);
            ge = hipStreamEndCapture(cs, &graph);
        }
        if (ge == hipSuccess) ge = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        if (ge != hipSuccess) { cleanup(); return fail(PCX_ERR_HIP, "TT-SVD sweep graph: %s", hipGetErrorString(ge)); }
        for (int sweep = 0; sweep < 60; ++sweep) {
            int rotated[2] = {0, 0};
            hipError_t e = hipMemsetAsync(drot.p, 0, 2 * sizeof(int), cs);
            if (e == hipSuccess) e = hipGraphLaunch(exec, cs);
            if (e == hipSuccess) e = hipMemcpyAsync(rotated, drot.p, 2 * sizeof(int), hipMemcpyDeviceToHost, cs);
            if (e == hipSuccess) e = hipStreamSynchronize(cs);
            if (e != hipSuccess) { cleanup(); return fail(PCX_ERR_HIP, "TT-SVD sweep: %s", hipGetErrorString(e)); }
            ++sweeps_total;
            if (rotated[1] == 0) break;
        }
        cleanup();
        }
    }
    hipLaunchKernelGGL(k_row_sqnorms, dim3(m), dim3(TTSVD_THREADS), 0, 0, cur.as<double>(), N, N, nrm.as<double>());
    HIP_TRY(hipGetLastError());
    hnorm.resize(m);
    HIP_TRY(hipMemcpy(hnorm.data(), nrm.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
    return PCX_OK;
}

// TT-SVD of a dense value tensor (reference _tt_svd_from_tensor, tensor_train.py:638-690).
extern "C" int pcx_tt_svd(int device, int d, const int32_t *n_nodes, const double *tensor, int max_rank,
                          double tol, int32_t *ranks_out, double *cores_out, int64_t cores_cap,
                          int64_t *cores_len, int32_t *sweeps_out) {
    PCX_API_BEGIN
    if (d < 1 || d > PCX_MAX_DIMS || !n_nodes || !tensor || !ranks_out || !cores_out || !cores_len)
        return fail(PCX_ERR_INVALID, "bad argument");
    if (max_rank < 1) return fail(PCX_ERR_INVALID, "max_rank must be >= 1");
    long total = 1;
    for (int k = 0; k < d; ++k) {
        if (n_nodes[k] < 1) return fail(PCX_ERR_INVALID, "n_nodes[%d] < 1", k);
        total *= n_nodes[k];
        if (total > (1L << 33)) return fail(PCX_ERR_UNSUPPORTED, "dense tensor too large for TT-SVD");
    }
    int rc = use_device(device);
    if (rc) return rc;
    DevBuf cur, nxt;
    JacobiWork w;
    Scratch srows;
    struct Release { Scratch &a; ~Release() { a.release(); } } rel{srows};
    if ((rc = cur.alloc((size_t)total * sizeof(double)))) return rc;
    if ((rc = nxt.alloc((size_t)total * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpy(cur.p, tensor, (size_t)total * sizeof(double), hipMemcpyHostToDevice));
    long elems = total;
    int r_prev = 1;
    int64_t written = 0;
    int sweeps_total = 0;
    ranks_out[0] = 1;
    std::vector<double> hU;
    std::vector<int> order;
    for (int k = 0; k < d - 1; ++k) {
        const long m_l = (long)r_prev * n_nodes[k];
        if (m_l > 8192) return fail(PCX_ERR_UNSUPPORTED, "TT-SVD unfolding with %ld rows (> 8192)", m_l);
        const int m = (int)m_l;
        const long N = elems / m;
        if ((rc = rowjacobi_factor(cur, nxt, m, N, tol, w, sweeps_total))) return rc;
        if ((rc = srows.reserve((size_t)m * sizeof(int)))) return rc;
        DevView rows{srows.ptr};
        const std::vector<double> &hnorm = w.hnorm;
        order.resize(m);
        for (int i = 0; i < m; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return hnorm[a] > hnorm[b]; });
        // rank rule of the reference (:673-678): cap, then drop S <= tol * S[0]
        const long len_s = std::min<long>(m, N);
        int rank = (int)std::min<long>(max_rank, len_s);
        const double s0 = std::sqrt(hnorm[order[0]]);
        if (s0 > 0.0) {
            int effective = 0;
            for (int i = 0; i < len_s; ++i) effective += (std::sqrt(hnorm[order[i]]) > tol * s0) ? 1 : 0;
            rank = std::max(1, std::min(rank, effective));
        } else {
            rank = 1;       // an all-zero unfolding: one zero row carries it (the reference keeps min(max_rank, len(S)) of them)
        }
        if (written + (int64_t)m * rank > cores_cap) return fail(PCX_ERR_INVALID, "cores_out too small");
        hU.resize((size_t)m * m);
        HIP_TRY(hipMemcpy(hU.data(), w.sU.ptr, (size_t)m * m * sizeof(double), hipMemcpyDeviceToHost));
        for (int i = 0; i < m; ++i)
            for (int c = 0; c < rank; ++c) cores_out[written + (int64_t)i * rank + c] = hU[(size_t)i * m + order[c]];
        written += (int64_t)m * rank;
        HIP_TRY(hipMemcpy(rows.p, order.data(), (size_t)rank * sizeof(int), hipMemcpyHostToDevice));
        unsigned gx = (unsigned)std::min<long>((N + 255) / 256, 1024);
        hipLaunchKernelGGL(k_gather_rows, dim3(gx, rank), dim3(256), 0, 0, cur.as<double>(), N, N, rows.as<int>(), nxt.as<double>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        std::swap(cur.p, nxt.p);
        elems = (long)rank * N;
        r_prev = rank;
        ranks_out[k + 1] = rank;
    }
    ranks_out[d] = 1;
    if (written + elems > cores_cap) return fail(PCX_ERR_INVALID, "cores_out too small");
    HIP_TRY(hipMemcpy(cores_out + written, cur.p, (size_t)elems * sizeof(double), hipMemcpyDeviceToHost));
    written += elems;
    *cores_len = written;
    if (sweeps_out) *sweeps_out = sweeps_total;
    return PCX_OK;
    PCX_API_END
}

// ---------------------------------------------------------------------------------
// TT rounding and adjacent swaps (reference _algebra.py::_tt_round_cores, ::_tt_swap_adjacent)
// ---------------------------------------------------------------------------------

#define TTR_MAX_RANK 256          // stacked ranks: two rank-128 operands
#define TTR_MAX_NODES 256
#define TTR_SWAP_MAX_ROWS 4096    // r_l n of a merged swap pair: the Jacobi iteration costs rows^2 x cols per sweep
#define TTR_SWAP_MAX_ELEMS (1L << 24)

static unsigned ttr_blocks(long total) {
    return (unsigned)std::max<long>(1, std::min<long>((total + TTR_THREADS - 1) / TTR_THREADS, 1L << 16));
}

// The cores of one TT on the device, each in its own buffer, C order (r_{k-1}, n_k, r_k).
struct TTCores {
    std::vector<DevBuf> core;
    std::vector<int> n, r;          // n[d], r[d + 1]
    explicit TTCores(int d) : core(d), n(d), r(d + 1) {}
    long size(int k) const { return (long)r[k] * n[k] * r[k + 1]; }
};

// The state a rounding or a swap sequence carries between factorisations.
struct TTRWork {
    JacobiWork w;
    DevBuf cur, nxt;                // the matrix being factored and the Gram preconditioner's work space
    size_t cap = 0;                 // doubles in each of cur and nxt (the preconditioner swaps them)
    Scratch ssel, sinv, ssig, sT;
    std::vector<int> order;
    std::vector<double> sig, inv;
    int sweeps = 0;
    ~TTRWork() { ssel.release(); sinv.release(); ssig.release(); sT.release(); }

    int reserve(size_t elems) {
        if (elems <= cap) return PCX_OK;
        if (cur.p) { (void)hipFree(cur.p); cur.p = nullptr; }
        if (nxt.p) { (void)hipFree(nxt.p); nxt.p = nullptr; }
        cap = 0;
        int rc;
        if ((rc = cur.alloc(elems * sizeof(double)))) return rc;
        if ((rc = nxt.alloc(elems * sizeof(double)))) return rc;
        cap = elems;
        return PCX_OK;
    }

    // singular values of the last factorisation in descending order (ties keep the row order)
    void sort_rows(int m) {
        const std::vector<double> &h = w.hnorm;
        order.resize(m);
        for (int i = 0; i < m; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return h[a] > h[b]; });
        sig.resize(m);
        inv.resize(m);
        for (int i = 0; i < m; ++i) {
            sig[i] = std::sqrt(h[order[i]]);
            inv[i] = sig[i] > 0.0 ? 1.0 / sig[i] : 0.0;
        }
    }

    // the kept rows order[0 .. keep) with their singular values and inverses, on the device
    int upload(int keep) {
        int rc;
        if ((rc = ssel.reserve((size_t)keep * sizeof(int)))) return rc;
        if ((rc = sinv.reserve((size_t)keep * sizeof(double)))) return rc;
        if ((rc = ssig.reserve((size_t)keep * sizeof(double)))) return rc;
        HIP_TRY(hipMemcpy(ssel.ptr, order.data(), (size_t)keep * sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(sinv.ptr, inv.data(), (size_t)keep * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(ssig.ptr, sig.data(), (size_t)keep * sizeof(double), hipMemcpyHostToDevice));
        return PCX_OK;
    }

    // out[a * oa + b * ob] = scale[a] * src[sel[a] * sa + b * sb] over the kept rows a < keep
    void pick(const void *src, long sa, long sb, bool by_inverse, int keep, long nb, void *out, long oa, long ob) {
        hipLaunchKernelGGL(k_ttr_pick, dim3(ttr_blocks((long)keep * nb)), dim3(TTR_THREADS), 0, 0, (const double *)src, sa, sb,
                           (const int *)ssel.ptr, (const double *)(by_inverse ? sinv.ptr : ssig.ptr), keep, nb,
                           (double *)out, oa, ob);
    }
};

// the reference's rank rule for a truncated SVD: cap at max_rank, then drop S <= tol * S[0] when S[0] > 0 and
// tol > 0, and keep at least one
static int ttr_keep(const std::vector<double> &s, long len_s, int max_rank, double tol) {
    int keep = (int)std::min<long>(max_rank, len_s);
    if (s[0] > 0.0 && tol > 0.0) {
        int effective = 0;
        for (long i = 0; i < len_s; ++i) effective += (s[i] > tol * s[0]) ? 1 : 0;
        keep = std::min(keep, effective);
    }
    return std::max(1, keep);
}

static int ttr_check_shape(int d, const int32_t *n_nodes, const int32_t *ranks, int max_rank, const char *what) {
    if (d < 1 || d > PCX_MAX_DIMS || !n_nodes || !ranks) return fail(PCX_ERR_INVALID, "%s: bad argument", what);
    if (max_rank < 1) return fail(PCX_ERR_INVALID, "%s: max_rank must be >= 1", what);
    if (ranks[0] != 1 || ranks[d] != 1) return fail(PCX_ERR_INVALID, "%s: boundary ranks must be 1", what);
    for (int k = 0; k < d; ++k) {
        if (n_nodes[k] < 1 || ranks[k + 1] < 1) return fail(PCX_ERR_INVALID, "%s: core %d has shape (%d, %d, %d)", what, k,
                                                            (int)ranks[k], (int)n_nodes[k], (int)ranks[k + 1]);
        if (ranks[k] > TTR_MAX_RANK || ranks[k + 1] > TTR_MAX_RANK || n_nodes[k] > TTR_MAX_NODES)
            return fail(PCX_ERR_UNSUPPORTED, "%s: core %d of shape (%d, %d, %d) exceeds ranks %d / %d nodes", what, k,
                        (int)ranks[k], (int)n_nodes[k], (int)ranks[k + 1], TTR_MAX_RANK, TTR_MAX_NODES);
    }
    return PCX_OK;
}

static int ttr_upload(TTCores &t, const int32_t *n_nodes, const int32_t *ranks, const double *cores) {
    const int d = (int)t.n.size();
    for (int k = 0; k < d; ++k) t.n[k] = n_nodes[k];
    for (int k = 0; k <= d; ++k) t.r[k] = ranks[k];
    long off = 0;
    for (int k = 0; k < d; ++k) {
        int rc;
        if ((rc = t.core[k].alloc((size_t)t.size(k) * sizeof(double)))) return rc;
        HIP_TRY(hipMemcpy(t.core[k].p, cores + off, (size_t)t.size(k) * sizeof(double), hipMemcpyHostToDevice));
        off += t.size(k);
    }
    return PCX_OK;
}

static int ttr_download(TTCores &t, int32_t *n_out, int32_t *ranks_out, double *cores_out, int64_t cap, int64_t *len) {
    const int d = (int)t.n.size();
    int64_t total = 0;
    for (int k = 0; k < d; ++k) total += t.size(k);
    if (total > cap) return fail(PCX_ERR_INVALID, "cores_out too small (%lld < %lld doubles)", (long long)cap, (long long)total);
    int64_t off = 0;
    for (int k = 0; k < d; ++k) {
        HIP_TRY(hipMemcpy(cores_out + off, t.core[k].p, (size_t)t.size(k) * sizeof(double), hipMemcpyDeviceToHost));
        off += t.size(k);
    }
    for (int k = 0; k <= d; ++k) ranks_out[k] = t.r[k];
    if (n_out)
        for (int k = 0; k < d; ++k) n_out[k] = t.n[k];
    *len = total;
    return PCX_OK;
}

// a fresh device buffer of `elems` doubles (swapped into a core by the caller)
static int ttr_fresh(DevBuf &fresh, long elems) { return fresh.alloc((size_t)elems * sizeof(double)); }

// Right-to-left orthogonalisation step at core k >= 1: core k = T Q with Q row-orthonormal, T pushed into core k-1.
// Rows of the factored unfolding below 8 eps ||core||_F are dropped: those are the exact dependencies of a
// stacked sum (they rotate into zero rows), and keeping them would leave noise directions in the basis.
static int ttr_orthogonalise_right(TTCores &t, int k, TTRWork &x) {
    const int m = t.r[k];
    const long N = (long)t.n[k] * t.r[k + 1];
    int rc;
    if ((rc = x.reserve((size_t)m * N))) return rc;
    HIP_TRY(hipMemcpy(x.cur.p, t.core[k].p, (size_t)m * N * sizeof(double), hipMemcpyDeviceToDevice));
    if ((rc = rowjacobi_factor(x.cur, x.nxt, m, N, 0.0, x.w, x.sweeps))) return rc;
    x.sort_rows(m);
    double fro2 = 0.0;
    for (int i = 0; i < m; ++i) fro2 += x.w.hnorm[i];
    const double eps64 = 8.0 * 2.220446049250313e-16;
    const double floor2 = eps64 * eps64 * fro2;
    int keep = 0;
    while (keep < m && x.sig[keep] * x.sig[keep] > floor2) ++keep;
    keep = std::max(keep, 1);
    if ((rc = x.upload(keep))) return rc;
    DevBuf q, prev;
    if ((rc = ttr_fresh(q, (long)keep * N))) return rc;
    x.pick(x.cur.p, N, 1, true, keep, N, q.p, N, 1);                          // Q = rows of B / sigma
    if ((rc = x.sT.reserve((size_t)m * keep * sizeof(double)))) return rc;
    x.pick(x.w.sU.ptr, 1, m, false, keep, m, x.sT.ptr, 1, keep);             // T = U[:, kept] sigma  (m x keep)
    const long P = (long)t.r[k - 1] * t.n[k - 1];
    if ((rc = ttr_fresh(prev, P * keep))) return rc;
    hipLaunchKernelGGL(k_ttr_gemm, dim3(ttr_blocks(P * keep)), dim3(TTR_THREADS), 0, 0, t.core[k - 1].as<double>(),
                       (const double *)x.sT.ptr, prev.as<double>(), P, (long)keep, m);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    std::swap(t.core[k].p, q.p);
    std::swap(t.core[k - 1].p, prev.p);
    t.r[k] = keep;
    return PCX_OK;
}

// Left-to-right truncation step at core k <= d-2: the (r_l n) x r_r unfolding = U S V^T, truncated by the rank
// rule; U becomes core k (left-orthonormal), S V^T is pushed into core k+1.  The row iteration runs on the
// transposed unfolding, whose rows are the r_r columns.
static int ttr_truncate_left(TTCores &t, int k, int max_rank, double tol, TTRWork &x) {
    const long rows = (long)t.r[k] * t.n[k];
    const int m = t.r[k + 1];
    int rc;
    if ((rc = x.reserve((size_t)m * rows))) return rc;
    hipLaunchKernelGGL(k_ttr_transpose, dim3((unsigned)((m + 31) / 32), (unsigned)((rows + 31) / 32)), dim3(TTR_THREADS), 0, 0,
                       t.core[k].as<double>(), rows, (long)m, x.cur.as<double>());
    HIP_TRY(hipGetLastError());
    if ((rc = rowjacobi_factor(x.cur, x.nxt, m, rows, tol, x.w, x.sweeps))) return rc;
    x.sort_rows(m);
    const int keep = ttr_keep(x.sig, std::min<long>(m, rows), max_rank, tol);
    if ((rc = x.upload(keep))) return rc;
    DevBuf u, next;
    if ((rc = ttr_fresh(u, rows * keep))) return rc;
    x.pick(x.cur.p, rows, 1, true, keep, rows, u.p, 1, keep);                 // U = (rows of B / sigma)^T
    if ((rc = x.sT.reserve((size_t)m * keep * sizeof(double)))) return rc;
    x.pick(x.w.sU.ptr, 1, m, false, keep, m, x.sT.ptr, m, 1);                // S V^T  (keep x m)
    const long Q = (long)t.n[k + 1] * t.r[k + 2];
    if ((rc = ttr_fresh(next, (long)keep * Q))) return rc;
    hipLaunchKernelGGL(k_ttr_gemm, dim3(ttr_blocks((long)keep * Q)), dim3(TTR_THREADS), 0, 0, (const double *)x.sT.ptr,
                       t.core[k + 1].as<double>(), next.as<double>(), (long)keep, Q, m);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    std::swap(t.core[k].p, u.p);
    std::swap(t.core[k + 1].p, next.p);
    t.r[k + 1] = keep;
    return PCX_OK;
}

// Swap storage axes i and i+1: merge the two cores with their node axes exchanged, factor the
// (r_l n_b) x (n_a r_r) matrix, truncate by the rank rule, core i = U S and core i+1 = V^T.
static int ttr_swap(TTCores &t, int i, int max_rank, double tol, TTRWork &x) {
    const int rl = t.r[i], na = t.n[i], rm = t.r[i + 1], nb = t.n[i + 1], rr = t.r[i + 2];
    const long rows = (long)rl * nb, cols = (long)na * rr;
    if (rows > TTR_SWAP_MAX_ROWS || rows * cols > TTR_SWAP_MAX_ELEMS)
        return fail(PCX_ERR_UNSUPPORTED, "TT swap at %d: merged pair (%d, %d, %d, %d) exceeds %d rows / %ld elements", i, rl, nb,
                    na, rr, TTR_SWAP_MAX_ROWS, TTR_SWAP_MAX_ELEMS);
    int rc;
    if ((rc = x.reserve((size_t)rows * cols))) return rc;
    hipLaunchKernelGGL(k_ttr_merge_swapped, dim3(ttr_blocks(rows * cols)), dim3(TTR_THREADS), 0, 0, t.core[i].as<double>(),
                       t.core[i + 1].as<double>(), rl, na, rm, nb, rr, x.cur.as<double>());
    HIP_TRY(hipGetLastError());
    const int m = (int)rows;
    if ((rc = rowjacobi_factor(x.cur, x.nxt, m, cols, tol, x.w, x.sweeps))) return rc;
    x.sort_rows(m);
    const int keep = ttr_keep(x.sig, std::min<long>(rows, cols), max_rank, tol);
    if ((rc = x.upload(keep))) return rc;
    DevBuf a, b;
    if ((rc = ttr_fresh(a, rows * keep))) return rc;
    if ((rc = ttr_fresh(b, (long)keep * cols))) return rc;
    x.pick(x.w.sU.ptr, 1, m, false, keep, m, a.p, 1, keep);                  // U S  (rows x keep)
    x.pick(x.cur.p, cols, 1, true, keep, cols, b.p, cols, 1);                // V^T = rows of B / sigma
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    std::swap(t.core[i].p, a.p);
    std::swap(t.core[i + 1].p, b.p);
    t.n[i] = nb;
    t.n[i + 1] = na;
    t.r[i + 1] = keep;
    return PCX_OK;
}

extern "C" int pcx_tt_round(int device, int d, const int32_t *n_nodes, const int32_t *ranks, const double *cores,
                            int max_rank, double tol, int32_t *ranks_out, double *cores_out, int64_t cores_cap,
                            int64_t *cores_len, int32_t *sweeps_out) {
    PCX_API_BEGIN
    int rc = ttr_check_shape(d, n_nodes, ranks, max_rank, "TT rounding");
    if (rc) return rc;
    if (!cores || !ranks_out || !cores_out || !cores_len) return fail(PCX_ERR_INVALID, "TT rounding: NULL buffer");
    if (!(tol >= 0.0)) return fail(PCX_ERR_INVALID, "TT rounding: tol must be >= 0");
    if ((rc = use_device(device))) return rc;
    TTCores t(d);
    if ((rc = ttr_upload(t, n_nodes, ranks, cores))) return rc;
    TTRWork x;
    for (int k = d - 1; k >= 1; --k)
        if ((rc = ttr_orthogonalise_right(t, k, x))) return rc;
    for (int k = 0; k < d - 1; ++k)
        if ((rc = ttr_truncate_left(t, k, max_rank, tol, x))) return rc;
    if ((rc = ttr_download(t, nullptr, ranks_out, cores_out, cores_cap, cores_len))) return rc;
    if (sweeps_out) *sweeps_out = x.sweeps;
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_tt_reorder(int device, int d, const int32_t *n_nodes, const int32_t *ranks, const double *cores,
                              int n_swaps, const int32_t *swaps, int max_rank, double tol, int32_t *n_nodes_out,
                              int32_t *ranks_out, double *cores_out, int64_t cores_cap, int64_t *cores_len,
                              int32_t *sweeps_out) {
    PCX_API_BEGIN
    int rc = ttr_check_shape(d, n_nodes, ranks, max_rank, "TT reorder");
    if (rc) return rc;
    if (!cores || !n_nodes_out || !ranks_out || !cores_out || !cores_len || n_swaps < 0 || (n_swaps > 0 && !swaps))
        return fail(PCX_ERR_INVALID, "TT reorder: bad argument");
    if (!(tol >= 0.0)) return fail(PCX_ERR_INVALID, "TT reorder: tol must be >= 0");
    for (int s = 0; s < n_swaps; ++s)
        if (swaps[s] < 0 || swaps[s] >= d - 1) return fail(PCX_ERR_INVALID, "TT reorder: swap position %d out of range [0, %d)", (int)swaps[s], d - 1);
    if (n_swaps > 0) {        // the first swap's shape is known before anything runs
        const int i = swaps[0];
        const long rows = (long)ranks[i] * n_nodes[i + 1], cols = (long)n_nodes[i] * ranks[i + 2];
        if (rows > TTR_SWAP_MAX_ROWS || rows * cols > TTR_SWAP_MAX_ELEMS)
            return fail(PCX_ERR_UNSUPPORTED, "TT swap at %d: merged pair (%d, %d, %d, %d) exceeds %d rows / %ld elements", i,
                        (int)ranks[i], (int)n_nodes[i + 1], (int)n_nodes[i], (int)ranks[i + 2], TTR_SWAP_MAX_ROWS, TTR_SWAP_MAX_ELEMS);
    }
    if ((rc = use_device(device))) return rc;
    TTCores t(d);
    if ((rc = ttr_upload(t, n_nodes, ranks, cores))) return rc;
    TTRWork x;
    for (int s = 0; s < n_swaps; ++s)
        if ((rc = ttr_swap(t, swaps[s], max_rank, tol, x))) return rc;
    if ((rc = ttr_download(t, n_nodes_out, ranks_out, cores_out, cores_cap, cores_len))) return rc;
    if (sweeps_out) *sweeps_out = x.sweeps;
    return PCX_OK;
    PCX_API_END
}

// The dense steps take at most 8192 x 64 entries: checked on the host before the upload.  A NaN or an infinity would
// come back as pivots and a rank like any others.
static int require_finite(const char *what, const double *A, int m, int r) {
    for (long f = 0; f < (long)m * r; ++f)
        if (!std::isfinite(A[f]))
            return fail(PCX_ERR_INVALID, "%s: entry (%ld, %ld) of the %d x %d matrix is not finite", what, f / r, f % r, m, r);
    return PCX_OK;
}

extern "C" int pcx_maxvol(int device, const double *A, int m, int r, double tol, int max_iters,
                          int64_t *idx_out) {
    PCX_API_BEGIN
    if (!A || !idx_out || m < 1 || r < 1) return fail(PCX_ERR_INVALID, "bad argument");
    if (m <= r) {  // tensor_train.py:85-86
        for (int i = 0; i < m; ++i) idx_out[i] = i;
        return PCX_OK;
    }
    if (r > TTX_MAX_R || m > TTX_MAX_M) return fail(PCX_ERR_UNSUPPORTED, "maxvol: %d x %d exceeds %d x %d", m, r, TTX_MAX_M, TTX_MAX_R);
    int rc = require_finite("maxvol", A, m, r);
    if (rc) return rc;
    if ((rc = use_device(device))) return rc;
    DevBuf dA, dB, didx;
    if ((rc = dA.alloc((size_t)m * r * sizeof(double)))) return rc;
    if ((rc = dB.alloc((size_t)m * r * sizeof(double)))) return rc;
    if ((rc = didx.alloc((size_t)r * sizeof(long long)))) return rc;
    HIP_TRY(hipMemcpy(dA.p, A, (size_t)m * r * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_maxvol, dim3(1), dim3(TTX_THREADS), 0, 0, dA.as<double>(), m, r, tol, max_iters,
                       dB.as<double>(), didx.as<long long>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(idx_out, didx.p, (size_t)r * sizeof(long long), hipMemcpyDeviceToHost));
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_tt_cross_step(int device, const double *C, int m, int c, int cap, double rel_thresh,
                                 double *chat, int64_t *pivots, int32_t *rank_out) {
    PCX_API_BEGIN
    if (!C || !chat || !pivots || !rank_out || m < 1 || c < 1 || cap < 1) return fail(PCX_ERR_INVALID, "bad argument");
    if (c > TTX_MAX_R || m > TTX_MAX_M) return fail(PCX_ERR_UNSUPPORTED, "cross step: %d x %d exceeds %d x %d", m, c, TTX_MAX_M, TTX_MAX_R);
    int rc = require_finite("cross step", C, m, c);  // the reference's SVD raises LinAlgError here
    if (rc) return rc;
    if ((rc = use_device(device))) return rc;
    DevBuf dC, dU, dB, dchat, dpiv, drank;
    if ((rc = dC.alloc((size_t)m * c * sizeof(double)))) return rc;
    if ((rc = dU.alloc((size_t)m * c * sizeof(double)))) return rc;
    if ((rc = dB.alloc((size_t)m * c * sizeof(double)))) return rc;
    if ((rc = dchat.alloc((size_t)m * c * sizeof(double)))) return rc;
    if ((rc = dpiv.alloc((size_t)c * sizeof(long long)))) return rc;
    if ((rc = drank.alloc(sizeof(int)))) return rc;
    HIP_TRY(hipMemcpy(dC.p, C, (size_t)m * c * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_cross_step, dim3(1), dim3(TTX_THREADS), 0, 0, dC.as<double>(), m, c, cap, rel_thresh,
                       dU.as<double>(), dB.as<double>(), dchat.as<double>(), dpiv.as<long long>(),
                       drank.as<int>());
    HIP_TRY(hipGetLastError());
    int rank = 0;
    HIP_TRY(hipMemcpy(&rank, drank.p, sizeof(int), hipMemcpyDeviceToHost));
    if (rank < 1 || rank > c) return fail(PCX_ERR_HIP, "cross step returned rank %d", rank);
    HIP_TRY(hipMemcpy(chat, dchat.p, (size_t)m * rank * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pivots, dpiv.p, (size_t)rank * sizeof(long long), hipMemcpyDeviceToHost));
    *rank_out = rank;
    return PCX_OK;
    PCX_API_END
}

