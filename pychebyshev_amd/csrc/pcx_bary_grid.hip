// pcx_bary_grid.hip -- packing and launching of k_bary_mfma_grid (bary_grid_kernels.h): the MFMA form for short plans, row
// tiles laid over the last two head dimensions.  Part of the barycentric handle (pcx_bary.hip; planned in pcx_bary_plan.hip).

#include "pcx_bary_internal.h"
#include "bary_grid_kernels.h"

PCX_HIDDEN int bary_pack_grid(pcx_bary *h, const double *plain, double *frag) {
    const long cnt = (long)h->gp.MT * h->plan.KS * 64;
    hipLaunchKernelGGL(k_pack_fragments_grid, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream, plain, frag, h->gp,
                       h->plan.K, h->plan.KS);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

template <int KS, int NT, int WPB, bool AF>
static int launch_grid_t(pcx_bary *h, const double *const *frag_tab, int m, const double *d_pts, long N, double *d_out,
                         long ostride, long ooff, hipStream_t st, Scratch *split_scratch, const int *perm) {
    const size_t lds = bary_grid_lds_bytes(h->gp, NT);
    auto kern = k_bary_mfma_grid<KS, NT, WPB, AF>;
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long per_wg = 16L * NT * WPB;
    const long blocks = (N + per_wg - 1) / per_wg;
    if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
    const int nchunks = h->gp.nchunks;
    int nsplit = 1, cps = nchunks;
    const long want = 2048 / WPB;   // waves that fill 256 CUs at two per SIMD
    if (split_scratch && blocks * m < want && nchunks > 1) {
        nsplit = (int)std::min<long>(nchunks, (want + blocks * m - 1) / (blocks * m));
        cps = (nchunks + nsplit - 1) / nsplit;
        nsplit = (nchunks + cps - 1) / cps;
    }
    double *partial = nullptr;
    if (nsplit > 1) {
        int rc = split_scratch->reserve((size_t)m * nchunks * 4 * (size_t)N * sizeof(double));
        if (rc) return rc;
        partial = (double *)split_scratch->ptr;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)nsplit, (unsigned)m), dim3(64 * WPB), lds, st, h->dims, h->plan, h->gp,
                       h->d_nodes, h->d_wts, h->grid_prod ? h->d_gsnodes : nullptr, frag_tab, h->d_kcode, d_pts, d_out, N, ostride, ooff,
                       cps, partial, perm);
    HIP_TRY(hipGetLastError());
    if (nsplit > 1) {
        const long cnt = N * m;
        hipLaunchKernelGGL(k_bary_grid_reduce, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, partial, d_out, N, nchunks, m,
                           ostride, ooff, perm);
        HIP_TRY(hipGetLastError());
    }
    return PCX_OK;
}

template <int NT>
static int launch_grid_nt(pcx_bary *h, const double *const *frag_tab, int m, const double *d_pts, long N, double *d_out,
                          long ostride, long ooff, hipStream_t st, Scratch *split_scratch, const int *perm) {
    switch (h->plan.KS) {
#define GRID_GO(v, W, A) launch_grid_t<v, NT, W, A>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm)
#define CASE_KS(v) case v: return h->gp.wpb == 4 ? (h->gp.af ? GRID_GO(v, 4, true) : GRID_GO(v, 4, false)) \
                                        : (h->gp.af ? GRID_GO(v, 1, true) : GRID_GO(v, 1, false));
        CASE_KS(1) CASE_KS(2) CASE_KS(3) CASE_KS(4) CASE_KS(5) CASE_KS(6) CASE_KS(7) CASE_KS(8)
        CASE_KS(9) CASE_KS(10) CASE_KS(11) CASE_KS(12) CASE_KS(13) CASE_KS(14) CASE_KS(15) CASE_KS(16)
        CASE_KS(17) CASE_KS(18) CASE_KS(19) CASE_KS(20) CASE_KS(21) CASE_KS(22) CASE_KS(23) CASE_KS(24)
        CASE_KS(25) CASE_KS(26) CASE_KS(27) CASE_KS(28) CASE_KS(29) CASE_KS(30) CASE_KS(31) CASE_KS(32)
#undef CASE_KS
#undef GRID_GO
    }
    return fail(PCX_ERR_UNSUPPORTED, "no grid MFMA instantiation for KS=%d", h->plan.KS);
}

PCX_HIDDEN int bary_launch_grid(pcx_bary *h, const double *const *frag_tab, int m, const double *d_pts, long N, double *d_out,
                                long ostride, long ooff, hipStream_t st, Scratch *split_scratch, const int *perm) {
    // two column tiles per wave for throughput; one when the batch cannot fill the chip.  (Four, for plans of up to 8 k-steps,
    // were measured in round 4: 20^3 0.487 -> 0.323, 23^3 0.500 -> 0.432, 24^3 0.559 -> 0.484, 25^3 0.425 -> 0.468 -- not kept.)
    const int nt = (N >= 65536) ? h->nt : 1;
    return nt == 2 ? launch_grid_nt<2>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm)
                   : launch_grid_nt<1>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm);
}
