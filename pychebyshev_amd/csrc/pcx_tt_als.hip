// pcx_tt_als.hip -- pcx_tt_orth and pcx_tt_als: core orthogonalisation and fixed-rank completion (ALS in projection
// form) of a tensor train against a dense target.  Kernels: tt_als_kernels.h.  Everything runs on the null stream.
#include "pcx_internal.h"
#include "tt_als_kernels.h"

#define TTA_MAX_RANK 256
#define TTA_MAX_NODES 256

namespace {

struct AlsTT {
    std::vector<int> n, r;
    std::vector<DevBuf> core;
    explicit AlsTT(int d) : n(d), r(d + 1), core(d) {}
    int d() const { return (int)n.size(); }
    long size(int k) const { return (long)r[k] * n[k] * r[k + 1]; }
    double *p(int k) { return core[k].as<double>(); }
};

// scratch of one call: the matrix a factorisation overwrites, its transposed input, and the ping-pong buffers of a
// projection chain and of the carried tensor
struct AlsWork {
    Scratch qr, tr, chain[2], carry[2], partial, sums;
    ~AlsWork() {
        qr.release(); tr.release(); partial.release(); sums.release();
        for (int i = 0; i < 2; ++i) { chain[i].release(); carry[i].release(); }
    }
};

unsigned blocks_for(long total) {
    return (unsigned)std::max<long>(1, std::min<long>((total + TTA_THREADS - 1) / TTA_THREADS, 1L << 20));
}

// The rank from which the contractions run on the matrix cores: 16, one full tile, as in the evaluation kernels.
// Measured (profiles/tt_completion_probe.txt) the MFMA form is already level with the VALU form at rank 4 and 12 - 27 %
// ahead of it at ranks 8 - 12 per outer iteration, so the switch can move down.  Both forms are tested at every rank
// class through pcx_tt_als_project (tests/test_gpu_als_steps.py).  PCX_TT_ALS_MFMA_MIN moves the switch (that is how
// the probe runs either form at every rank).
int mfma_min_rank() {
    static const int v = [] {
        const char *e = getenv("PCX_TT_ALS_MFMA_MIN");
        const int x = e ? atoi(e) : 0;
        return x >= 1 ? x : 16;
    }();
    return v;
}

int check_shape(int d, const int32_t *n_nodes, const int32_t *ranks, const char *what) {
    if (d < 1 || d > PCX_MAX_DIMS || !n_nodes || !ranks) return fail(PCX_ERR_INVALID, "%s: bad argument", what);
    if (ranks[0] != 1 || ranks[d] != 1) return fail(PCX_ERR_INVALID, "%s: boundary ranks must be 1", what);
    for (int k = 0; k < d; ++k) {
        if (n_nodes[k] < 1 || ranks[k + 1] < 1)
            return fail(PCX_ERR_INVALID, "%s: core %d has shape (%d, %d, %d)", what, k, (int)ranks[k], (int)n_nodes[k],
                        (int)ranks[k + 1]);
        if (ranks[k] > TTA_MAX_RANK || ranks[k + 1] > TTA_MAX_RANK || n_nodes[k] > TTA_MAX_NODES)
            return fail(PCX_ERR_UNSUPPORTED, "%s: core %d of shape (%d, %d, %d) exceeds ranks %d / %d nodes", what, k,
                        (int)ranks[k], (int)n_nodes[k], (int)ranks[k + 1], TTA_MAX_RANK, TTA_MAX_NODES);
    }
    return PCX_OK;
}

int upload(AlsTT &t, const int32_t *n_nodes, const int32_t *ranks, const double *cores) {
    const int d = t.d();
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

int download(AlsTT &t, int32_t *ranks_out, double *cores_out, int64_t cap, int64_t *len) {
    const int d = t.d();
    int64_t total = 0;
    for (int k = 0; k < d; ++k) total += t.size(k);
    if (total > cap) return fail(PCX_ERR_INVALID, "cores_out too small (%lld < %lld doubles)", (long long)cap, (long long)total);
    int64_t off = 0;
    for (int k = 0; k < d; ++k) {
        HIP_TRY(hipMemcpy(cores_out + off, t.core[k].p, (size_t)t.size(k) * sizeof(double), hipMemcpyDeviceToHost));
        off += t.size(k);
    }
    for (int k = 0; k <= d; ++k) ranks_out[k] = t.r[k];
    *len = total;
    return PCX_OK;
}

// The form a contraction of rank r runs in.  form 0: the rule of the sweeps, MFMA from mfma_min_rank() on; 1: VALU; 2:
// MFMA (the diagnostic entry point asks for either at any rank).
enum { TTA_FORM_AUTO = 0, TTA_FORM_VALU = 1, TTA_FORM_MFMA = 2 };

int pick_form(int form, int r) {
    if (form == TTA_FORM_AUTO) return r >= mfma_min_rank() ? TTA_FORM_MFMA : TTA_FORM_VALU;
    return form;
}

// out (rp x R) = Q^T P, Q (K x rp), P (K x R)
int left_project(const double *Q, const double *P, double *out, int K, int rp, long R, int form = TTA_FORM_AUTO,
                 int *form_used = nullptr) {
    const unsigned bx = (unsigned)((R + TTA_THREADS - 1) / TTA_THREADS);
    form = pick_form(form, rp);
    if (form_used) *form_used = form;
    if (form == TTA_FORM_MFMA) {
        if (rp <= 16) hipLaunchKernelGGL(k_tta_left_mfma<1>, dim3(bx, 1), dim3(TTA_THREADS), 0, 0, Q, P, out, K, rp, R);
        else hipLaunchKernelGGL(k_tta_left_mfma<2>, dim3(bx, (unsigned)((rp + 31) / 32)), dim3(TTA_THREADS), 0, 0, Q, P, out, K, rp, R);
    } else if (rp <= 4) {
        hipLaunchKernelGGL(k_tta_left_valu<4>, dim3(bx, 1), dim3(TTA_THREADS), 0, 0, Q, P, out, K, rp, R);
    } else if (rp <= 8) {
        hipLaunchKernelGGL(k_tta_left_valu<8>, dim3(bx, 1), dim3(TTA_THREADS), 0, 0, Q, P, out, K, rp, R);
    } else if (rp <= 12) {
        hipLaunchKernelGGL(k_tta_left_valu<12>, dim3(bx, 1), dim3(TTA_THREADS), 0, 0, Q, P, out, K, rp, R);
    } else {
        hipLaunchKernelGGL(k_tta_left_valu<16>, dim3(bx, (unsigned)((rp + 15) / 16)), dim3(TTA_THREADS), 0, 0, Q, P, out, K, rp, R);
    }
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

// out (R x r) = P C^T, P (R x K), C (r x K)
int right_project(const double *P, const double *C, double *out, long R, int K, int r, int form = TTA_FORM_AUTO,
                  int *form_used = nullptr) {
    const unsigned bx = (unsigned)((R + TTA_THREADS - 1) / TTA_THREADS);
    form = pick_form(form, r);
    if (form_used) *form_used = form;
    if (form == TTA_FORM_MFMA) {
        if (r <= 16) hipLaunchKernelGGL(k_tta_right_mfma<1>, dim3(bx, 1), dim3(TTA_THREADS), 0, 0, P, C, out, R, K, r);
        else hipLaunchKernelGGL(k_tta_right_mfma<2>, dim3(bx, (unsigned)((r + 31) / 32)), dim3(TTA_THREADS), 0, 0, P, C, out, R, K, r);
    } else if (r <= 4) {
        hipLaunchKernelGGL(k_tta_right_valu<4>, dim3(bx, 1), dim3(TTA_THREADS), 0, 0, P, C, out, R, K, r);
    } else if (r <= 8) {
        hipLaunchKernelGGL(k_tta_right_valu<8>, dim3(bx, 1), dim3(TTA_THREADS), 0, 0, P, C, out, R, K, r);
    } else if (r <= 12) {
        hipLaunchKernelGGL(k_tta_right_valu<12>, dim3(bx, 1), dim3(TTA_THREADS), 0, 0, P, C, out, R, K, r);
    } else {
        hipLaunchKernelGGL(k_tta_right_valu<16>, dim3(bx, (unsigned)((r + 15) / 16)), dim3(TTA_THREADS), 0, 0, P, C, out, R, K, r);
    }
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

// Householder QR of `in` (m x c, left untouched): Q (m x p) and R (p x c) in fresh buffers, p = min(m, c)
int qr(const double *in, long m, int c, AlsWork &w, DevBuf &Q, DevBuf &R, int *p_out) {
    const int p = (int)std::min<long>(m, c);
    int rc;
    if ((rc = w.qr.reserve((size_t)m * c * sizeof(double)))) return rc;
    if ((rc = Q.alloc((size_t)m * p * sizeof(double)))) return rc;
    if ((rc = R.alloc((size_t)p * c * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpyAsync(w.qr.ptr, in, (size_t)m * c * sizeof(double), hipMemcpyDeviceToDevice, 0));
    hipLaunchKernelGGL(k_tta_householder, dim3(1), dim3(TTA_THREADS), 0, 0, (double *)w.qr.ptr, m, c, Q.as<double>(), R.as<double>());
    HIP_TRY(hipGetLastError());
    *p_out = p;
    return PCX_OK;
}

int transpose(const double *in, long rows, long cols, double *out) {
    hipLaunchKernelGGL(k_tta_transpose, dim3(blocks_for(rows * cols)), dim3(TTA_THREADS), 0, 0, in, rows, cols, out);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

int gemm(const double *A, const double *B, long bsk, long bsj, double *C, long M, long N, int K) {
    hipLaunchKernelGGL(k_tta_gemm, dim3(blocks_for(M * N)), dim3(TTA_THREADS), 0, 0, A, B, bsk, bsj, C, M, N, K);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

// Core k (k <= d-2) becomes Q of the QR of its (r_k n_k) x r_{k+1} unfolding; the bond shrinks to min(r_k n_k, r_{k+1}).
// push: R is multiplied into core k+1 (the tensor is unchanged).  Without it core k+1 is left with its old left rank:
// the caller is about to replace it.
int orth_left_step(AlsTT &t, int k, bool push, AlsWork &w) {
    const long m = (long)t.r[k] * t.n[k];
    const int c = t.r[k + 1];
    DevBuf Q, R;
    int p, rc;
    if ((rc = qr(t.p(k), m, c, w, Q, R, &p))) return rc;
    if (push) {
        const long N = (long)t.n[k + 1] * t.r[k + 2];
        DevBuf next;
        if ((rc = next.alloc((size_t)p * N * sizeof(double)))) return rc;
        if ((rc = gemm(R.as<double>(), t.p(k + 1), N, 1, next.as<double>(), p, N, c))) return rc;
        HIP_TRY(hipDeviceSynchronize());
        std::swap(t.core[k + 1].p, next.p);
    }
    HIP_TRY(hipDeviceSynchronize());
    std::swap(t.core[k].p, Q.p);
    t.r[k + 1] = p;
    return PCX_OK;
}

// Core k (k >= 1) becomes Q^T of the QR of its transposed r_k x (n_k r_{k+1}) unfolding (rows orthonormal); the bond
// shrinks to min(r_k, n_k r_{k+1}).  push: core k-1 = core k-1 . R^T.
int orth_right_step(AlsTT &t, int k, bool push, AlsWork &w) {
    const int c = t.r[k];
    const long N = (long)t.n[k] * t.r[k + 1];
    int rc, p;
    if ((rc = w.tr.reserve((size_t)N * c * sizeof(double)))) return rc;
    if ((rc = transpose(t.p(k), c, N, (double *)w.tr.ptr))) return rc;
    DevBuf Q, R, fresh;
    if ((rc = qr((const double *)w.tr.ptr, N, c, w, Q, R, &p))) return rc;
    if ((rc = fresh.alloc((size_t)p * N * sizeof(double)))) return rc;
    if ((rc = transpose(Q.as<double>(), N, p, fresh.as<double>()))) return rc;
    if (push) {
        const long M = (long)t.r[k - 1] * t.n[k - 1];
        DevBuf prev;
        if ((rc = prev.alloc((size_t)M * p * sizeof(double)))) return rc;
        if ((rc = gemm(t.p(k - 1), R.as<double>(), 1, c, prev.as<double>(), M, p, c))) return rc;      // B[k][j] = R[j][k]
        HIP_TRY(hipDeviceSynchronize());
        std::swap(t.core[k - 1].p, prev.p);
    }
    HIP_TRY(hipDeviceSynchronize());
    std::swap(t.core[k].p, fresh.p);
    t.r[k] = p;
    return PCX_OK;
}

// the dense tensor of the train, C order, into out (prod(n) doubles)
int reconstruct(AlsTT &t, double *out, AlsWork &w) {
    const int d = t.d();
    if (d == 1) {
        HIP_TRY(hipMemcpyAsync(out, t.p(0), (size_t)t.n[0] * sizeof(double), hipMemcpyDeviceToDevice, 0));
        return PCX_OK;
    }
    const double *X = t.p(0);
    long M = t.n[0];
    for (int k = 1; k < d; ++k) {
        const long N = (long)t.n[k] * t.r[k + 1];
        double *dst = out;
        int rc;
        if (k < d - 1) {
            if ((rc = w.chain[k & 1].reserve((size_t)M * N * sizeof(double)))) return rc;
            dst = (double *)w.chain[k & 1].ptr;
        }
        if ((rc = gemm(X, t.p(k), N, 1, dst, M, N, t.r[k]))) return rc;
        X = dst;
        M *= t.n[k];
    }
    return PCX_OK;
}

int replace_core(AlsTT &t, int k, const double *src, long elems) {
    DevBuf fresh;
    int rc;
    if ((rc = fresh.alloc((size_t)elems * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpy(fresh.p, src, (size_t)elems * sizeof(double), hipMemcpyDeviceToDevice));
    std::swap(t.core[k].p, fresh.p);
    return PCX_OK;
}

// Left-to-right half sweep.  Cores k+1 .. d-1 are row-orthonormal on entry.  P_k = the target with cores 0 .. k-1
// projected out, shape (r_k, n_k, ..., n_{d-1}); core k = P_k with cores d-1 .. k+1 projected out from the right; its QR
// gives the orthonormal core k and P_{k+1} = Q_k^T P_k.  first_solved: core 0 already holds its solution (the end of
// the previous right-to-left half sweep).
int sweep_left_to_right(AlsTT &t, const double *T, long G, bool first_solved, AlsWork &w) {
    const int d = t.d();
    const double *P = T;
    long psize = G;                                        // elements of P_k
    int rc;
    for (int k = 0; k < d; ++k) {
        if (k == d - 1) return replace_core(t, k, P, psize);             // (r_{d-1} x n_{d-1})
        if (!(k == 0 && first_solved)) {
            const double *X = P;
            long xsize = psize;
            int flip = 0;
            for (int j = d - 1; j > k; --j) {
                const int K = t.n[j] * t.r[j + 1];
                const long rows = xsize / K;
                if ((rc = w.chain[flip].reserve((size_t)rows * t.r[j] * sizeof(double)))) return rc;
                if ((rc = right_project(X, t.p(j), (double *)w.chain[flip].ptr, rows, K, t.r[j]))) return rc;
                X = (const double *)w.chain[flip].ptr;
                xsize = rows * t.r[j];
                flip ^= 1;
            }
            if ((rc = replace_core(t, k, X, xsize))) return rc;           // (r_k n_k) x r_{k+1}
        }
        if ((rc = orth_left_step(t, k, false, w))) return rc;
        const int K = t.r[k] * t.n[k];
        const long R = psize / K;
        Scratch &dst = w.carry[k & 1];
        if ((rc = dst.reserve((size_t)t.r[k + 1] * R * sizeof(double)))) return rc;
        if ((rc = left_project(t.p(k), P, (double *)dst.ptr, K, t.r[k + 1], R))) return rc;
        P = (const double *)dst.ptr;
        psize = (long)t.r[k + 1] * R;
    }
    return PCX_OK;
}

// Right-to-left half sweep, the mirror image.  Cores 0 .. d-2 are left-orthonormal and core d-1 holds its solution on
// entry.  S_k = the target with cores k+1 .. d-1 projected out, shape (n_0, ..., n_k, r_{k+1}).
int sweep_right_to_left(AlsTT &t, const double *T, long G, AlsWork &w) {
    const int d = t.d();
    const double *S = T;
    long ssize = G;
    int rc;
    for (int k = d - 1; k >= 0; --k) {
        if (k == 0) return replace_core(t, 0, S, ssize);                  // (n_0 x r_1)
        if (k < d - 1) {
            const double *X = S;
            long xsize = ssize;
            int flip = 0;
            for (int j = 0; j < k; ++j) {
                const int K = t.r[j] * t.n[j];
                const long R = xsize / K;
                if ((rc = w.chain[flip].reserve((size_t)t.r[j + 1] * R * sizeof(double)))) return rc;
                if ((rc = left_project(t.p(j), X, (double *)w.chain[flip].ptr, K, t.r[j + 1], R))) return rc;
                X = (const double *)w.chain[flip].ptr;
                xsize = (long)t.r[j + 1] * R;
                flip ^= 1;
            }
            if ((rc = replace_core(t, k, X, xsize))) return rc;           // r_k x (n_k r_{k+1})
        }
        if ((rc = orth_right_step(t, k, false, w))) return rc;
        const int K = t.n[k] * t.r[k + 1];
        const long rows = ssize / K;
        Scratch &dst = w.carry[k & 1];
        if ((rc = dst.reserve((size_t)rows * t.r[k] * sizeof(double)))) return rc;
        if ((rc = right_project(S, t.p(k), (double *)dst.ptr, rows, K, t.r[k]))) return rc;
        S = (const double *)dst.ptr;
        ssize = rows * t.r[k];
    }
    return PCX_OK;
}

// the four sums of squares of k_tta_norms on the host
int norms(const double *tnew, const double *tprev, const double *target, long G, AlsWork &w, double sums[4]) {
    int rc;
    if ((rc = w.partial.reserve((size_t)TTA_RED_BLOCKS * 4 * sizeof(double)))) return rc;
    if ((rc = w.sums.reserve(4 * sizeof(double)))) return rc;
    const int blocks = (int)std::max<long>(1, std::min<long>((G + TTA_THREADS - 1) / TTA_THREADS, TTA_RED_BLOCKS));
    hipLaunchKernelGGL(k_tta_norms, dim3(blocks), dim3(TTA_THREADS), 0, 0, tnew, tprev, target, G, (double *)w.partial.ptr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tta_norms_final, dim3(1), dim3(TTA_THREADS), 0, 0, (const double *)w.partial.ptr, blocks, (double *)w.sums.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(sums, w.sums.ptr, 4 * sizeof(double), hipMemcpyDeviceToHost));
    return PCX_OK;
}

double residual_of(const double sums[4]) {
    if (sums[3] > 0.0) return std::sqrt(sums[2]) / std::sqrt(sums[3]);
    return sums[2] > 0.0 ? INFINITY : 0.0;
}

}  // namespace

extern "C" int pcx_tt_orth(int device, int d, const int32_t *n_nodes, const int32_t *ranks, const double *cores, int side,
                           int position, int32_t *ranks_out, double *cores_out, int64_t cores_cap, int64_t *cores_len) {
    PCX_API_BEGIN
    int rc = check_shape(d, n_nodes, ranks, "TT orthogonalisation");
    if (rc) return rc;
    if (!cores || !ranks_out || !cores_out || !cores_len) return fail(PCX_ERR_INVALID, "TT orthogonalisation: NULL buffer");
    if (side != 0 && side != 1) return fail(PCX_ERR_INVALID, "TT orthogonalisation: side must be 0 (left) or 1 (right), got %d", side);
    if (side == 0 && !(position >= 1 && position < d))
        return fail(PCX_ERR_INVALID, "position must be in [1, %d] for orth_left, got %d", d - 1, position);
    if (side == 1 && !(position >= 0 && position < d - 1))
        return fail(PCX_ERR_INVALID, "position must be in [0, %d] for orth_right, got %d", d - 2, position);
    if ((rc = use_device(device))) return rc;
    AlsTT t(d);
    if ((rc = upload(t, n_nodes, ranks, cores))) return rc;
    AlsWork w;
    if (side == 0) {
        for (int k = 0; k < position; ++k)
            if ((rc = orth_left_step(t, k, true, w))) return rc;
    } else {
        for (int k = d - 1; k > position; --k)
            if ((rc = orth_right_step(t, k, true, w))) return rc;
    }
    return download(t, ranks_out, cores_out, cores_cap, cores_len);
    PCX_API_END
}

extern "C" int pcx_tt_als(int device, int d, const int32_t *n_nodes, const int32_t *ranks, const double *value_cores,
                          const double *target, double tolerance, int max_iter, int32_t *ranks_out, double *cores_out,
                          int64_t cores_cap, int64_t *cores_len, int32_t *iters_out, double *rel_change_out,
                          double *grid_residual_out) {
    PCX_API_BEGIN
    int rc = check_shape(d, n_nodes, ranks, "TT completion");
    if (rc) return rc;
    if (!value_cores || !target || !ranks_out || !cores_out || !cores_len || !iters_out || !grid_residual_out ||
        (max_iter > 0 && !rel_change_out))
        return fail(PCX_ERR_INVALID, "TT completion: NULL buffer");
    if (tolerance != tolerance) return fail(PCX_ERR_INVALID, "TT completion: tolerance is NaN");
    long G = 1;
    for (int k = 0; k < d; ++k) {
        G *= n_nodes[k];
        if (G > PCX_TT_ALS_MAX_GRID)
            return fail(PCX_ERR_UNSUPPORTED, "TT completion: the grid exceeds %lld points", (long long)PCX_TT_ALS_MAX_GRID);
    }
    if ((rc = use_device(device))) return rc;
    AlsTT t(d);
    if ((rc = upload(t, n_nodes, ranks, value_cores))) return rc;
    AlsWork w;
    DevBuf T, prev, cur;
    const size_t gbytes = (size_t)G * sizeof(double);
    if ((rc = T.alloc(gbytes))) return rc;
    if ((rc = prev.alloc(gbytes))) return rc;
    if ((rc = cur.alloc(gbytes))) return rc;
    HIP_TRY(hipMemcpy(T.p, target, gbytes, hipMemcpyHostToDevice));
    if ((rc = reconstruct(t, prev.as<double>(), w))) return rc;
    double sums[4];
    int iters = 0;
    if (max_iter > 0) {
        for (int k = d - 1; k >= 1; --k)
            if ((rc = orth_right_step(t, k, true, w))) return rc;
        for (int it = 0; it < max_iter; ++it) {
            if ((rc = sweep_left_to_right(t, T.as<double>(), G, it > 0, w))) return rc;
            if ((rc = sweep_right_to_left(t, T.as<double>(), G, w))) return rc;
            if ((rc = reconstruct(t, cur.as<double>(), w))) return rc;
            if ((rc = norms(cur.as<double>(), prev.as<double>(), T.as<double>(), G, w, sums))) return rc;
            const double rel = std::sqrt(sums[0]) / (std::sqrt(sums[1]) + 1e-30);
            rel_change_out[it] = rel;
            iters = it + 1;
            std::swap(prev.p, cur.p);
            if (rel < tolerance) break;
        }
    } else {
        if ((rc = norms(prev.as<double>(), prev.as<double>(), T.as<double>(), G, w, sums))) return rc;
    }
    HIP_TRY(hipDeviceSynchronize());
    *iters_out = iters;
    *grid_residual_out = residual_of(sums);
    return download(t, ranks_out, cores_out, cores_cap, cores_len);
    PCX_API_END
}

// ---------------------------------------------------------------------------------
// diagnostic entry points: one dense step each (include/pcx.h)
// ---------------------------------------------------------------------------------
#define TTA_GUARD_DOUBLES 256

extern "C" int pcx_tt_als_project(int device, int side, int form, const double *small, const double *big, double *out,
                                  int K, int r, int64_t R, int32_t *form_used) {
    PCX_API_BEGIN
    if (!small || !big || !out || !form_used) return fail(PCX_ERR_INVALID, "TT projection: NULL buffer");
    if (side != 0 && side != 1) return fail(PCX_ERR_INVALID, "TT projection: side must be 0 (left) or 1 (right), got %d", side);
    if (form < TTA_FORM_AUTO || form > TTA_FORM_MFMA) return fail(PCX_ERR_INVALID, "TT projection: form must be 0, 1 or 2, got %d", form);
    if (K < 1 || r < 1 || R < 1) return fail(PCX_ERR_INVALID, "TT projection: K = %d, r = %d, R = %lld", K, r, (long long)R);
    if (r > TTA_MAX_RANK) return fail(PCX_ERR_UNSUPPORTED, "TT projection: rank %d exceeds %d", r, TTA_MAX_RANK);
    if (R > PCX_TT_ALS_MAX_GRID / K)
        return fail(PCX_ERR_UNSUPPORTED, "TT projection: K R exceeds %lld elements", (long long)PCX_TT_ALS_MAX_GRID);
    int rc = use_device(device);
    if (rc) return rc;
    const size_t nsmall = (size_t)K * r, nbig = (size_t)K * R, nout = (size_t)r * R;
    DevBuf ds, db, dout;
    if ((rc = ds.alloc(nsmall * sizeof(double)))) return rc;
    if ((rc = db.alloc(nbig * sizeof(double)))) return rc;
    if ((rc = dout.alloc((nout + TTA_GUARD_DOUBLES) * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpy(ds.p, small, nsmall * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(db.p, big, nbig * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dout.p, 0xFF, (nout + TTA_GUARD_DOUBLES) * sizeof(double)));      // all bits set: a NaN
    int used = 0;
    if (side == 0) rc = left_project(ds.as<double>(), db.as<double>(), dout.as<double>(), K, r, (long)R, form, &used);
    else rc = right_project(db.as<double>(), ds.as<double>(), dout.as<double>(), (long)R, K, r, form, &used);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    uint64_t guard[TTA_GUARD_DOUBLES];
    HIP_TRY(hipMemcpy(guard, dout.as<double>() + nout, sizeof(guard), hipMemcpyDeviceToHost));
    for (int i = 0; i < TTA_GUARD_DOUBLES; ++i)
        if (guard[i] != ~(uint64_t)0)
            return fail(PCX_ERR_INTERNAL, "TT projection: the kernel wrote %d doubles past its output (side %d, form %d, K = %d, r = %d, R = %lld)",
                        i, side, used, K, r, (long long)R);
    HIP_TRY(hipMemcpy(out, dout.p, nout * sizeof(double), hipMemcpyDeviceToHost));
    *form_used = used;
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_tt_als_qr(int device, const double *A, int64_t m, int c, double *Q, double *R) {
    PCX_API_BEGIN
    if (!A || !Q || !R) return fail(PCX_ERR_INVALID, "TT QR: NULL buffer");
    if (m < 1 || c < 1) return fail(PCX_ERR_INVALID, "TT QR: shape (%lld, %d)", (long long)m, c);
    if (c > TTA_MAX_RANK) return fail(PCX_ERR_UNSUPPORTED, "TT QR: %d columns exceed %d", c, TTA_MAX_RANK);
    if (m > PCX_TT_ALS_MAX_GRID / c) return fail(PCX_ERR_UNSUPPORTED, "TT QR: m c exceeds %lld elements", (long long)PCX_TT_ALS_MAX_GRID);
    int rc = use_device(device);
    if (rc) return rc;
    DevBuf dA, dQ, dR;
    AlsWork w;
    int p = 0;
    if ((rc = dA.alloc((size_t)m * c * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpy(dA.p, A, (size_t)m * c * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = qr(dA.as<double>(), (long)m, c, w, dQ, dR, &p))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(Q, dQ.p, (size_t)m * p * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(R, dR.p, (size_t)p * c * sizeof(double), hipMemcpyDeviceToHost));
    return PCX_OK;
    PCX_API_END
}

extern "C" int pcx_tt_als_norms(int device, const double *tnew, const double *tprev, const double *target, int64_t G,
                                double *out4) {
    PCX_API_BEGIN
    if (!tnew || !tprev || !target || !out4) return fail(PCX_ERR_INVALID, "TT norms: NULL buffer");
    if (G < 1) return fail(PCX_ERR_INVALID, "TT norms: G = %lld", (long long)G);
    if (G > PCX_TT_ALS_MAX_GRID) return fail(PCX_ERR_UNSUPPORTED, "TT norms: G exceeds %lld", (long long)PCX_TT_ALS_MAX_GRID);
    int rc = use_device(device);
    if (rc) return rc;
    DevBuf d[3];
    const double *src[3] = {tnew, tprev, target};
    for (int i = 0; i < 3; ++i) {
        if ((rc = d[i].alloc((size_t)G * sizeof(double)))) return rc;
        HIP_TRY(hipMemcpy(d[i].p, src[i], (size_t)G * sizeof(double), hipMemcpyHostToDevice));
    }
    AlsWork w;
    return norms(d[0].as<double>(), d[1].as<double>(), d[2].as<double>(), (long)G, w, out4);
    PCX_API_END
}
