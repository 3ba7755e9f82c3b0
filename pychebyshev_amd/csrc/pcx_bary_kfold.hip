// pcx_bary_kfold.hip -- packing and launching of k_bary_mfma_kfold (bary_kfold_kernels.h): the MFMA form for 3-D tensors one
// of whose dimensions fills row tiles well.  Part of the barycentric handle (pcx_bary.hip; planned in pcx_bary_plan.hip).

#include "pcx_bary_internal.h"
#include "bary_kfold_kernels.h"

PCX_HIDDEN int bary_pack_kfold(pcx_bary *h, const double *plain, double *frag) {
    const size_t cnt = bary_kfold_frag_count(h->kf);
    hipLaunchKernelGGL(k_pack_fragments_kfold, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream, plain, frag, h->kf);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

template <int MT, int KS2, int NT, bool STR>
static int launch_kfold_t(pcx_bary *h, const double *const *frag_tab, int m, const double *d_pts, long N, double *d_out,
                          long ostride, long ooff, hipStream_t st, const int *perm) {
    if constexpr (MT * KS2 < 8 || (STR && (KS2 < 6 || KS2 > 8))) {
        return fail(PCX_ERR_UNSUPPORTED, "no k-fold MFMA instantiation for MT=%d KS2=%d", MT, KS2);
    } else {
        // small batches: one row tile per wave (split-M launch) while that still leaves CUs idle -- a wave's chain of matrix
        // instructions is what a single query waits for
        if constexpr (NT == 1 && MT >= 2) {
            const long tiles = (N + 15) / 16;
            if (tiles * m <= 1024) {
                const size_t lds = (size_t)MT * h->kf.trows * 16 * sizeof(double) + 64 * sizeof(double);
                auto kern = k_bary_mfma_kfold<MT, KS2, 1, STR, true>;
                if (lds > 64 * 1024)
                    HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                hipLaunchKernelGGL(kern, dim3((unsigned)tiles, 1, (unsigned)m), dim3(64 * MT), lds, st, h->dims, h->kf, h->d_nodes,
                                   h->d_wts, h->grid_prod ? h->d_gsnodes : nullptr, frag_tab, d_pts, d_out, N, ostride, ooff, perm);
                HIP_TRY(hipGetLastError());
                return PCX_OK;
            }
        }
        const size_t lds = bary_kfold_lds_bytes(h->kf, NT);
        auto kern = k_bary_mfma_kfold<MT, KS2, NT, STR>;
        if (lds > 64 * 1024)
            HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const long per_wg = 64L * NT;
        const long blocks = (N + per_wg - 1) / per_wg;
        if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks, 1, (unsigned)m), dim3(256), lds, st, h->dims, h->kf, h->d_nodes, h->d_wts,
                           h->grid_prod ? h->d_gsnodes : nullptr, frag_tab, d_pts, d_out, N, ostride, ooff, perm);
        HIP_TRY(hipGetLastError());
        return PCX_OK;
    }
}

template <int MT, int NT>
static int launch_kfold_mt(pcx_bary *h, const double *const *frag_tab, int m, const double *d_pts, long N, double *d_out,
                           long ostride, long ooff, hipStream_t st, const int *perm) {
    switch (h->kf.KS2) {
#define CASE_KS(v) case v: return h->kf.str ? launch_kfold_t<MT, v, NT, true>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, perm) \
                                        : launch_kfold_t<MT, v, NT, false>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, perm);
        CASE_KS(2) CASE_KS(3) CASE_KS(4) CASE_KS(5) CASE_KS(6) CASE_KS(7) CASE_KS(8) CASE_KS(9)
        CASE_KS(10) CASE_KS(11) CASE_KS(12) CASE_KS(13) CASE_KS(14) CASE_KS(15) CASE_KS(16)
#undef CASE_KS
    }
    return fail(PCX_ERR_UNSUPPORTED, "no k-fold MFMA instantiation for KS2=%d", h->kf.KS2);
}

PCX_HIDDEN int bary_launch_kfold(pcx_bary *h, const double *const *frag_tab, int m, const double *d_pts, long N, double *d_out,
                                 long ostride, long ooff, hipStream_t st, const int *perm) {
    // two column tiles per wave for throughput; one when the batch cannot fill the chip (same sums either way)
    const bool two = N >= 65536 && h->nt == 2;
#define GO(MTv) (two ? launch_kfold_mt<MTv, 2>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, perm) \
                     : launch_kfold_mt<MTv, 1>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, perm))
    switch (h->kf.MT) {
        case 1: return GO(1);
        case 2: return GO(2);
        case 3: return GO(3);
        case 4: return GO(4);
    }
#undef GO
    return fail(PCX_ERR_UNSUPPORTED, "no k-fold MFMA instantiation for MT=%d", h->kf.MT);
}
