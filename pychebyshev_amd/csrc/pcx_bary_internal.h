// pcx_bary_internal.h -- the barycentric handle as the other translation units see it (pcx_spline.hip builds
// piecewise interpolants and sliders out of pcx_bary handles).  Not part of the ABI.
#pragma once

#include "pcx_internal.h"

// "Plain" (C-order) tensors carry PCX_PLAIN_PAD zeroed doubles behind their end: k_bary_small reads a
// row with a fixed-width run of scalar loads that may reach past the last row.
static int alloc_plain(DevBuf &b, long total) {
    int rc = b.alloc(((size_t)total + PCX_PLAIN_PAD) * sizeof(double));
    if (rc) return rc;
    HIP_TRY(hipMemset((char *)b.p + (size_t)total * sizeof(double), 0, PCX_PLAIN_PAD * sizeof(double)));
    return PCX_OK;
}

struct DerivedTensor {
    double *plain = nullptr;  // C-order tensor after the derivative passes (prod n doubles)
    double *frag = nullptr;   // MFMA A-fragment packing of `plain` (MT*KS*64 doubles, then MT*16*R seed doubles) or NULL
    double **slot = nullptr;  // device table with the single entry `frag` (kernel's frag_tab)
    double *frag_g0 = nullptr;   // slab packing for dim-0 group launches (n0 * tps * (KS * 64 + 16 R) doubles), built on first use
    double **slot_g0 = nullptr;  // device table with the single entry `frag_g0`
    uint64_t last_use = 0;    // handle clock at the last request (least-recently-used eviction)
    void free_all() {
        if (plain) (void)hipFree(plain);
        if (frag) (void)hipFree(frag);
        if (slot) (void)hipFree(slot);
        if (frag_g0) (void)hipFree(frag_g0);
        if (slot_g0) (void)hipFree(slot_g0);
        plain = frag = frag_g0 = nullptr;
        slot = slot_g0 = nullptr;
    }
};

struct pcx_bary {
    int device = 0;
    hipStream_t stream = nullptr;
    BaryDims dims;
    long total = 0;
    std::vector<int> doff;           // offsets of D_k in diff_cat
    double *d_nodes = nullptr, *d_wts = nullptr, *d_diff = nullptr;
    double *d_boxq = nullptr;        // box integrals (pcx_bary_box.hip; lazy): Q_n per dimension at doff[k], then 1 / j for j <= max n + 1
    double *d_cheb = nullptr;        // values -> Chebyshev coefficients matrix per dimension, at doff[k] (pcx_bary_sobol; lazy)
    Scratch s_cheb[2];               // the coefficient passes ping-pong between these (prod n doubles each, kept after first use)
    Scratch s_sobol;                 // k_sobol_energy's slab + k_sobol_finish's result
    // launch plan
    bool mfma_ok = false;
    bool seed = true;                // K-remainder columns seed the accumulators (PCX_BARY_SEED=0 at create: never)
    BaryMfmaPlan plan;
    int nt = 2;                      // point tiles per wave in the MFMA kernel
    unsigned *d_rowcode = nullptr, *d_kcode = nullptr;
    unsigned *d_rowcode_hi = nullptr, *d_kcode_hi = nullptr;   // fields 4..7 (wide plans only)
    bool wide = false;      // more than four head or tail dimensions
    // pipelined narrow plans (KS >= 12): the row codes as pre-scaled LDS byte offsets, one table per PW = 16, 32 (bary_kernels.h)
    unsigned *d_rowoff[2] = {nullptr, nullptr};
    int tail_mode = 1;               // tail split of large launches (launch_mfma_t): 1 where the row-tile walk is long enough to pay
                                     // for the second kernel; PCX_BARY_TAIL=0 at create: never, =2: wherever the geometry allows
    int slots[2] = {0, 0};           // resident workgroups of the row-code kernel per NT = 1, 2; queried at the first launch
    int last_tail_P = 0, last_tail_blocks = 0;   // geometry of the latest launch_mfma_t (pcx_bary_tail_info: the tests' witness)
    bool slots_query = false;        // the launch tables only fill `slots` (pcx_bary_tail_info)
    // short plans: row tiles = RA x RB blocks of the last two head dimensions, no row codes (bary_grid_kernels.h);
    // the fragment image of every derivative tensor is then packed in that order
    bool grid_ok = false;
    BaryGridPlan gp;
    double *d_gsnodes = nullptr;     // nodes times a power of two per dimension, then the PCX_MAX_DIMS scales themselves
    bool kfold_ok = false;           // 3-D, whole row tiles along dimension 0: k_bary_mfma_kfold (bary_kfold_kernels.h)
    BaryKfoldPlan kf;
    bool grid_prod = false;          // every dimension <= 64 nodes: division-free weights (grid_weights_prod)
    // dim-0 groups (BaryG0): specs differing only in their dim-0 order share one slab-packed GEMM
    bool g0_ok = false;
    int g0_tps = 0;                  // row tiles per dim-0 slab
    int g0_nf = 2;                   // live row-code fields (head dimensions 1 .. split-1, at least two)
    unsigned *d_rowcode_g0 = nullptr;
    int g0_span = 1;                 // dim-0 orders above its base tensor's a slab GEMM serves (pcx_bary_set_group_span)
    // dim-q groups (q > 0): the same model with dimension q moved to the front, built on first use (bary_rot); a pair of
    // specs one order apart along q shares ITS dim-0 slab GEMM, on the batch with its columns in that order
    pcx_bary *rot[PCX_MAX_DIMS] = {};
    char rot_state[PCX_MAX_DIMS] = {};   // 0 untried, 1 ready, 2 not available
    Scratch s_rot, s_rot2;           // the batch in a sub-model's column order (per staging slot)
    // what the probe measured for "spec base + e_q out of base's GEMM": |shared - own GEMM| / scale (bary_pair_deviation);
    // a pair is formed when that is at most group_tol
    std::map<std::vector<int>, double> pair_dev;
    double group_tol = 3e-13;
    int lpp = 64;                    // lanes per point in the rows kernel
    bool mfma4_ok = false;           // 4x4x4_4b form available (LDS budget)
    int small_nlp = 0;               // lane-per-point kernel for small tensors: padded last-dim width, 0 = not available
    std::vector<double> dom_lo, dom_hi;   // the domain, when the handle came from a .pcb file (pcx_bary_save_pcb)
    BarySmallScale small_scale;      // its power-of-two coordinate scales and the nodes times them
    double *d_snodes = nullptr;
    bool small_preferred = false;    // auto picks it (few row tiles: the MFMA kernel would be all prologue)
    int sq_nl = 0;                   // k_bary_sq (last two dimensions of sq_nl nodes each, d <= 4): 0 = not available
    bool sq_preferred = false;       // auto picks it
    int variant = 0;                 // 0 auto, 1 rows, 2 mfma 16x16x4, 3 mfma 4x4x4_4b, 4 lane-per-point (small tensors)
    std::mutex mu;
    std::map<std::vector<int>, DerivedTensor> cache;
    uint64_t clock = 0;              // bumped per request; entries used since `call_mark` are never evicted
    uint64_t call_mark = 0;
    HostStage stage;                 // host-pointer batches
    double **d_tab = nullptr;        // frag table for multi-spec launches (kMaxSpecs entries)
    std::vector<double *> tab_host;  // what d_tab currently holds
    Scratch s_partial;               // per-chunk totals of split launches
};

static const int kMaxSpecs = 64;      // derivative specs evaluated by one launch (grid.z)

// More specs than one launch takes (the reference has no limit: a gradient plus full Hessian in 10-D is 65): groups of
// kMaxSpecs, eval(derivs of the group, mc, part) each into a host buffer of N x mc, copied into its columns of `out`.
template <typename Fn>
static int eval_spec_groups(int64_t N, const int32_t *derivs, int d, int m, double *out, Fn &&eval) {
    if (!derivs) return fail(PCX_ERR_INVALID, "derivs is NULL");
    std::vector<double> part;
    for (int s0 = 0; s0 < m; s0 += kMaxSpecs) {
        const int mc = std::min(kMaxSpecs, m - s0);
        part.resize((size_t)N * mc);
        int rc = eval(derivs + (size_t)s0 * d, mc, part.data());
        if (rc) return rc;
        for (int64_t i = 0; i < N; ++i)
            memcpy(out + (size_t)i * m + s0, part.data() + (size_t)i * mc, (size_t)mc * sizeof(double));
    }
    return PCX_OK;
}

// pcx_bary_grid.hip
PCX_HIDDEN bool bary_plan_grid(const BaryDims &dm, const BaryMfmaPlan &plan, BaryGridPlan &gp);
PCX_HIDDEN int bary_pack_grid(pcx_bary *h, const double *plain, double *frag);
PCX_HIDDEN size_t bary_grid_lds_bytes(const pcx_bary *h, int nt);
PCX_HIDDEN long bary_plan_kfold(const BaryDims &dm, BaryKfoldPlan &kp);
PCX_HIDDEN long bary_kfold_estimate(const BaryKfoldPlan &kp, long eff);
PCX_HIDDEN bool bary_kfold_take(const BaryKfoldPlan &kp, long eff, long grid_eff, int grid_ks);
PCX_HIDDEN size_t bary_kfold_frag_count(const BaryKfoldPlan &kp);
PCX_HIDDEN size_t bary_kfold_lds_bytes(const BaryKfoldPlan &kp, int nt);
PCX_HIDDEN int bary_pack_kfold(pcx_bary *h, const double *plain, double *frag);
PCX_HIDDEN int bary_launch_kfold(pcx_bary *h, const double *const *frag_tab, int m, const double *d_pts, long N, double *d_out,
                                 long ostride, long ooff, hipStream_t st, const int *perm);
PCX_HIDDEN int bary_launch_grid(pcx_bary *h, const double *const *frag_tab, int m, const double *d_pts, long N, double *d_out,
                                long ostride, long ooff, hipStream_t st, Scratch *split_scratch, const int *perm);

// pcx_bary_seed1.hip, pcx_bary_seed2.hip: the row-code MFMA launch tables for plans with R = 1 and R = 2 seed columns
// (bary_mfma_launch.h; R = 0 lives in pcx_bary.hip)
#define PCX_DECLARE_SEED_LAUNCHERS(R)                                                                                            \
    PCX_HIDDEN int bary_launch_rowcode_seed##R(pcx_bary *h, const double *const *frag_tab, int m, const double *d_pts, long N,   \
                                               double *d_out, long ostride, long ooff, hipStream_t st, Scratch *split_scratch,   \
                                               const int *perm);                                                                 \
    PCX_HIDDEN int bary_launch_mfma4_seed##R(pcx_bary *h, const double *const *frag_tab, int m, const double *d_pts, long N,     \
                                             double *d_out, long ostride, long ooff, hipStream_t st, const int *perm);           \
    PCX_HIDDEN int bary_launch_g0_seed##R(pcx_bary *h, const DerivedTensor &base, const BaryG0 &gs, const double *d_pts, long N, \
                                          double *d_out, long ostride, long ooff, hipStream_t st);
PCX_DECLARE_SEED_LAUNCHERS(1)
PCX_DECLARE_SEED_LAUNCHERS(2)

// pcx_bary.hip
PCX_HIDDEN int bary_get_tensor(pcx_bary *h, const int32_t *deriv, DerivedTensor **out);
PCX_HIDDEN int bary_spec_tensors(pcx_bary *h, const int32_t *derivs, int m, std::vector<DerivedTensor *> &dts,
                                 const double *const **frag_tab);
PCX_HIDDEN int bary_effective_variant(const pcx_bary *h);
PCX_HIDDEN int bary_launch(pcx_bary *h, DerivedTensor *const *dts, int m, const double *const *frag_tab,
                           const double *d_pts, long N, double *d_out, long ostride, long ooff, hipStream_t st,
                           Scratch *split_scratch, const int *perm = nullptr);
PCX_HIDDEN int bary_launch_small_pieces(int dout, const pcx_bary *p0, const SplinePieceModel *models, const int *blk_piece,
                                        const int *blk_first, const int *piece_end, int m, long blocks, const double *dp,
                                        double *dout_buf, const int *perm, hipStream_t st);
PCX_HIDDEN int bary_launch_sq_pieces(const pcx_bary *p0, const SplinePieceModel *models, const int *blk_piece, const int *blk_first,
                                     const int *piece_end, int m, long blocks, const double *dp, double *dout, const int *perm,
                                     hipStream_t st);
