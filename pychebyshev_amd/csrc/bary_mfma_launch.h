// bary_mfma_launch.h -- launch tables of the row-code MFMA kernels (k_bary_mfma, k_bary_mfma4; bary_kernels.h).
//
// Every table is a template over R, the number of K-remainder columns that enter as the accumulators' seed
// (BaryMfmaPlan::R).  Each R is instantiated in a translation unit of its own -- pcx_bary.hip holds R = 0,
// pcx_bary_seed1.hip R = 1, pcx_bary_seed2.hip R = 2 -- so that the three sets of kernels compile side by side;
// bary_launch and bary_launch_group (pcx_bary.hip) pick the set by h->plan.R.
#pragma once

#include "pcx_bary_internal.h"
#include "bary_kernels.h"

// Workgroups of `kern` the device holds at once (256 threads, `lds` bytes each): the occupancy query times the
// compute units, at most the 512 (256 CUs at two per CU) every launch was sized for before the query existed.
static int resident_slots(const void *kern, size_t lds, int device, int *slots) {
    int per_cu = 0, cus = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, lds));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    *slots = (int)std::max<long>(1, std::min<long>(512, (long)per_cu * cus));
    return PCX_OK;
}

// One MFMA launch for m specs (frag_tab: device table of m fragment pointers).  Small
// batches are split over grid.y (chunks of row tiles) so that a handful of points still
// uses the whole chip; the per-chunk totals are then added by k_bary_reduce in the fixed
// chunk order, which makes every result independent of the batch size.
// Large batches end in a ragged round: `blocks` workgroups over `slots` resident ones leave tail = blocks mod slots
// for the last round.  When that round is at most half full (and m = 1: launches of several specs keep their
// geometry), each tail block is walked by P = min(nchunks, slots / tail) workgroups of the SAME grid, a contiguous
// range of chunks each, and k_bary_reduce finishes the tail points -- the additions of a split launch, so the same
// bits.  The finishing kernel costs about 7 us in the stream (9^4: 0.326 -> 0.334 ms per 10^6 points with the split, 7^5
// level, 11^5 -0.8 %), so the split is taken where a workgroup's walk -- MT (KS + 5) NT matrix-instruction slots, the
// planner's price of a tile -- is long enough that a third of it outweighs that: from kTailMinWork on (about 0.1 ms; 11^5
// is 5,880, 7^5 748, 9^4 300).  PCX_BARY_TAIL=0 at create keeps the one-workgroup-per-block geometry, =2 splits wherever the
// geometry allows (tests).
static const long kTailMinWork = 2048;
template <int KS, int NT, bool WIDE, int NF, int R>
static int launch_mfma_t(pcx_bary *h, const double *const *frag_tab, int m, const double *d_pts, long N,
                         double *d_out, long ostride, long ooff, hipStream_t st, Scratch *split_scratch,
                         const int *perm) {
    const bool allow_split = split_scratch != nullptr;
    size_t lds = mfma_lds_bytes(h->dims, NT);
    auto kern = k_bary_mfma<KS, NT, WIDE, NF, false, R>;
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    long per_wg = 4L * 16 * NT;
    long blocks = (N + per_wg - 1) / per_wg;
    if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
    int nchunks = (h->plan.MT + PCX_CHUNK_TILES - 1) / PCX_CHUNK_TILES;
    int nsplit = 1, cps = nchunks;
    if (KS >= 12 && !WIDE && !h->d_rowoff[NT - 1]) return fail(PCX_ERR_UNSUPPORTED, "row offsets of the pipelined loop were not built");
    if (!h->slots[NT - 1]) {
        int rc = resident_slots((const void *)kern, lds, h->device, &h->slots[NT - 1]);
        if (rc) return rc;
    }
    if (h->slots_query) return PCX_OK;
    const long want = h->slots[NT - 1];   // workgroups that fill the device
    if (allow_split && blocks * m < want && nchunks > 1) {
        nsplit = (int)std::min<long>(nchunks, (want + blocks * m - 1) / (blocks * m));
        cps = (nchunks + nsplit - 1) / nsplit;
        nsplit = (nchunks + cps - 1) / cps;
    }
    BaryTail tail{0, 0, 0};
    long grid_x = blocks;
    const long tail_blocks = blocks % want;
    const bool tail_pays = h->tail_mode == 2 || (h->tail_mode == 1 && (long)h->plan.MT * (KS + 5) * NT >= kTailMinWork);
    if (tail_pays && allow_split && m == 1 && nsplit == 1 && nchunks > 1 && blocks > want && tail_blocks > 0 &&
        2 * tail_blocks <= want) {
        int P = (int)std::min<long>(nchunks, want / tail_blocks);
        tail.cpp = (nchunks + P - 1) / P;
        P = (nchunks + tail.cpp - 1) / tail.cpp;       // no empty pieces
        if (P > 1 && blocks + want <= 0x7fffffffL) {
            tail.first = (int)(blocks - tail_blocks);
            tail.P = P;
            grid_x = tail.first + tail_blocks * P;     // <= blocks + slots
        }
    }
    h->last_tail_P = tail.P;
    h->last_tail_blocks = tail.P ? (int)tail_blocks : 0;
    const long part_p0 = tail.P ? (long)tail.first * per_wg : 0;    // first point `partial` holds
    double *partial = nullptr;
    if (nsplit > 1 || tail.P) {
        int rc = split_scratch->reserve((size_t)m * nchunks * 4 * (size_t)(N - part_p0) * sizeof(double));
        if (rc) return rc;
        partial = (double *)split_scratch->ptr;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)grid_x, (unsigned)nsplit, (unsigned)m), dim3(256), lds, st,
                       h->dims, h->plan, h->d_nodes, h->d_wts, frag_tab, h->d_rowcode, h->d_kcode,
                       h->d_rowcode_hi, h->d_kcode_hi, d_pts, d_out, N, ostride, ooff, cps, partial, perm, BaryG0{}, nullptr,
                       h->d_rowoff[NT - 1], tail);
    HIP_TRY(hipGetLastError());
    if (nsplit > 1 || tail.P) {
        long cnt = (N - part_p0) * m;
        hipLaunchKernelGGL(k_bary_reduce, dim3((unsigned)((cnt + 63) / 64)), dim3(256), 0, st, partial, d_out,
                           N - part_p0, nchunks, m, ostride, ooff, perm, part_p0);
        HIP_TRY(hipGetLastError());
    }
    return PCX_OK;
}

// 4x4x4_4b form: 512-thread workgroups (8 waves x 32 points), row tiles staged through LDS.
template <int KS, int R>
static int launch_mfma4_t(pcx_bary *h, const double *const *frag_tab, int m, const double *d_pts, long N,
                          double *d_out, long ostride, long ooff, hipStream_t st, const int *perm) {
    size_t lds = mfma4_lds_bytes(h->dims, KS);
    auto kern = k_bary_mfma4<KS, R>;
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    long blocks = (N + 255) / 256;
    if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks, 1, (unsigned)m), dim3(512), lds, st, h->dims, h->plan,
                       h->d_nodes, h->d_wts, frag_tab, h->d_rowcode, h->d_kcode, d_pts, d_out, N, ostride, ooff, perm);
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

#define PCX_CASES_KS_1_32                                                                  \
    CASE_KS(1) CASE_KS(2) CASE_KS(3) CASE_KS(4) CASE_KS(5) CASE_KS(6) CASE_KS(7) CASE_KS(8) \
    CASE_KS(9) CASE_KS(10) CASE_KS(11) CASE_KS(12) CASE_KS(13) CASE_KS(14) CASE_KS(15) CASE_KS(16) \
    CASE_KS(17) CASE_KS(18) CASE_KS(19) CASE_KS(20) CASE_KS(21) CASE_KS(22) CASE_KS(23) CASE_KS(24) \
    CASE_KS(25) CASE_KS(26) CASE_KS(27) CASE_KS(28) CASE_KS(29) CASE_KS(30) CASE_KS(31) CASE_KS(32)

template <int R>
static int launch_mfma4(pcx_bary *h, const double *const *frag_tab, int m, const double *d_pts, long N,
                        double *d_out, long ostride, long ooff, hipStream_t st, const int *perm) {
    switch (h->plan.KS) {
#define CASE_KS(v) case v: return launch_mfma4_t<v, R>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, perm);
        PCX_CASES_KS_1_32
#undef CASE_KS
    }
    return fail(PCX_ERR_UNSUPPORTED, "no MFMA instantiation for KS=%d", h->plan.KS);
}

// NF: live fields of a row code = head dimensions (1..4), known per handle: the kernel reads only those
// (16 LDS reads and multiplies fewer per row tile with a two-dimensional head; 11^5, head of three: +1.4 %).
template <int NT, bool WIDE, int NF, int R>
static int launch_mfma_nf(pcx_bary *h, const double *const *frag_tab, int m, const double *d_pts, long N,
                          double *d_out, long ostride, long ooff, hipStream_t st, Scratch *split_scratch,
                          const int *perm) {
    switch (h->plan.KS) {
#define CASE_KS(v) case v: return launch_mfma_t<v, NT, WIDE, NF, R>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm);
        PCX_CASES_KS_1_32
#undef CASE_KS
    }
    if constexpr (NT == 1) {
        switch (h->plan.KS) {
#define CASE_KS(v) case v: return launch_mfma_t<v, 1, WIDE, NF, R>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm);
            CASE_KS(36) CASE_KS(40) CASE_KS(44) CASE_KS(48) CASE_KS(52) CASE_KS(56) CASE_KS(60) CASE_KS(64)
#undef CASE_KS
        }
        if constexpr (R > 0) {      // 13 x 13 = 1 + 4 x 42: a count only a seeded plan asks for (pick_ks)
            if (h->plan.KS == 42)
                return launch_mfma_t<42, 1, WIDE, NF, R>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm);
        }
    }
    if constexpr (NT == 2 && !WIDE) {
        switch (h->plan.KS) {
#define CASE_KS(v) case v: return launch_mfma_t<v, 2, WIDE, NF, R>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm);
            CASE_KS(36) CASE_KS(40)
#undef CASE_KS
        }
    }
    return fail(PCX_ERR_UNSUPPORTED, "no MFMA instantiation for KS=%d, NT=%d", h->plan.KS, NT);
}

template <int NT, bool WIDE, int R>
static int launch_mfma_nt(pcx_bary *h, const double *const *frag_tab, int m, const double *d_pts, long N,
                          double *d_out, long ostride, long ooff, hipStream_t st, Scratch *split_scratch,
                          const int *perm) {
    if constexpr (!WIDE) {
        if (h->plan.split <= 2)
            return launch_mfma_nf<NT, false, 2, R>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm);
        if (h->plan.split == 3)
            return launch_mfma_nf<NT, false, 3, R>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm);
    }
    return launch_mfma_nf<NT, WIDE, 4, R>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm);
}

// k_bary_mfma for a batch of N points: two column tiles per wave for throughput; one when the batch cannot fill the chip
template <int R>
static int launch_rowcode(pcx_bary *h, const double *const *frag_tab, int m, const double *d_pts, long N, double *d_out,
                          long ostride, long ooff, hipStream_t st, Scratch *split_scratch, const int *perm) {
    int nt = (N >= 65536) ? h->nt : 1;
    if (h->wide)
        return nt == 2 ? launch_mfma_nt<2, true, R>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm)
                       : launch_mfma_nt<1, true, R>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm);
    return nt == 2 ? launch_mfma_nt<2, false, R>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm)
                   : launch_mfma_nt<1, false, R>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm);
}

// ---- dim-0 group launches (BaryG0) --------------------------------------------------------------
template <int KS, int NF, int R>
static int launch_g0_t(pcx_bary *h, const DerivedTensor &base, const BaryG0 &gs, const double *d_pts, long N, double *d_out,
                       long ostride, long ooff, hipStream_t st) {
    auto kern = k_bary_mfma<KS, 2, false, NF, true, R>;
    const size_t lds = mfma_lds_bytes(h->dims, 2);
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long blocks = (N + 127) / 128;
    if (blocks > 0x7fffffffL) return fail(PCX_ERR_UNSUPPORTED, "batch too large for one launch");
    BaryMfmaPlan plan = h->plan;
    plan.MT = gs.tps * gs.n0;
    const int nchunks = (plan.MT + PCX_CHUNK_TILES - 1) / PCX_CHUNK_TILES;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks, 1, 1), dim3(256), lds, st, h->dims, plan, h->d_nodes, h->d_wts,
                       (const double *const *)base.slot_g0, h->d_rowcode_g0, h->d_kcode, nullptr, nullptr, d_pts, d_out, N,
                       ostride, ooff, nchunks, nullptr, nullptr, gs, h->d_diff + h->doff[0], nullptr, BaryTail{0, 0, 0});
    HIP_TRY(hipGetLastError());
    return PCX_OK;
}

template <int NF, int R>
static int launch_g0_nf(pcx_bary *h, const DerivedTensor &base, const BaryG0 &gs, const double *d_pts, long N, double *d_out,
                        long ostride, long ooff, hipStream_t st) {
    switch (h->plan.KS) {
#define CASE_KS(v) case v: return launch_g0_t<v, NF, R>(h, base, gs, d_pts, N, d_out, ostride, ooff, st);
        PCX_CASES_KS_1_32
#undef CASE_KS
    }
    return fail(PCX_ERR_UNSUPPORTED, "no dim-0 group instantiation for KS=%d", h->plan.KS);
}

template <int R>
static int launch_g0(pcx_bary *h, const DerivedTensor &base, const BaryG0 &gs, const double *d_pts, long N, double *d_out,
                     long ostride, long ooff, hipStream_t st) {
    return (h->g0_nf == 2) ? launch_g0_nf<2, R>(h, base, gs, d_pts, N, d_out, ostride, ooff, st)
                           : launch_g0_nf<3, R>(h, base, gs, d_pts, N, d_out, ostride, ooff, st);
}

// The three entry points of a seeded set (R = 1, 2), defined by the translation unit that instantiates it.
#define PCX_DEFINE_SEED_LAUNCHERS(R)                                                                                             \
    PCX_HIDDEN int bary_launch_rowcode_seed##R(pcx_bary *h, const double *const *frag_tab, int m, const double *d_pts, long N,   \
                                               double *d_out, long ostride, long ooff, hipStream_t st, Scratch *split_scratch,   \
                                               const int *perm) {                                                                \
        return launch_rowcode<R>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, split_scratch, perm);                       \
    }                                                                                                                            \
    PCX_HIDDEN int bary_launch_mfma4_seed##R(pcx_bary *h, const double *const *frag_tab, int m, const double *d_pts, long N,     \
                                             double *d_out, long ostride, long ooff, hipStream_t st, const int *perm) {          \
        return launch_mfma4<R>(h, frag_tab, m, d_pts, N, d_out, ostride, ooff, st, perm);                                        \
    }                                                                                                                            \
    PCX_HIDDEN int bary_launch_g0_seed##R(pcx_bary *h, const DerivedTensor &base, const BaryG0 &gs, const double *d_pts, long N, \
                                          double *d_out, long ostride, long ooff, hipStream_t st) {                              \
        return launch_g0<R>(h, base, gs, d_pts, N, d_out, ostride, ooff, st);                                                    \
    }
