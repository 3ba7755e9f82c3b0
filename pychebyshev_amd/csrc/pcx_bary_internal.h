// pcx_bary_internal.h -- the barycentric handle as the other translation units see it (pcx_spline.hip builds
// piecewise interpolants and sliders out of pcx_bary handles).  Not part of the ABI.
#pragma once

#include "pcx_internal.h"
#include "bary_plan.h"

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
    double *ladder[PCX_MAX_DIMS] = {};   // ladder B images by dimension (bary_ladder_kernels.h), each packed on first use
    uint64_t last_use = 0;    // handle clock at the last request (least-recently-used eviction)
    void free_all() {
        for (double *&img : ladder) { if (img) (void)hipFree(img); img = nullptr; }
        if (plain) (void)hipFree(plain);
        if (frag) (void)hipFree(frag);
        if (slot) (void)hipFree(slot);
        if (frag_g0) (void)hipFree(frag_g0);
        if (slot_g0) (void)hipFree(slot_g0);
        plain = frag = frag_g0 = nullptr;
        slot = slot_g0 = nullptr;
    }
};

// The launch plan (BaryLaunchPlan, bary_plan.h: made by bary_make_plan at create and constant afterwards) and what the
// device holds for it.  The destructor releases everything the handle owns, the sub-models of `rot` included.
struct pcx_bary : BaryLaunchPlan {
    ~pcx_bary();
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
    // tensor-product grids (pcx_mode_product.hip): the passes ping-pong between s_grid, the W_k sit in s_gridw, a host
    // result is staged in s_gridout; grid_done is recorded behind the last pass of a call, and the next call waits for
    // it before it touches any of them (a _dev caller may be on a stream of its own)
    std::vector<double> h_nodes, h_wts;   // host copies of nodes_cat / weights_cat: the grid planner forms W_k from them
    Scratch s_grid[2], s_gridw, s_gridout;
    std::vector<double> grid_w_host;
    hipEvent_t grid_done = nullptr;
    // the plan's tables (bary_plan.h has their builders)
    unsigned *d_rowcode = nullptr, *d_kcode = nullptr;
    unsigned *d_rowcode_hi = nullptr, *d_kcode_hi = nullptr;   // fields 4..7 (wide plans only)
    // pipelined narrow plans (KS >= 12): the row codes as pre-scaled LDS byte offsets, one table per PW = 16, 32 (bary_kernels.h)
    unsigned *d_rowoff[2] = {nullptr, nullptr};
    unsigned *d_rowcode_g0 = nullptr;   // dim-0 groups: the slabs' row codes
    double *d_gsnodes = nullptr;     // grid and k-fold forms: nodes times a power of two per dimension, then the PCX_MAX_DIMS scales themselves
    double *d_snodes = nullptr;      // lane-per-point kernels: the nodes times small_scale
    int slots[2] = {0, 0};           // resident workgroups of the row-code kernel per NT = 1, 2; queried at the first launch
    int last_tail_P = 0, last_tail_blocks = 0;   // geometry of the latest launch_mfma_t (pcx_bary_tail_info: the tests' witness)
    bool slots_query = false;        // the launch tables only fill `slots` (pcx_bary_tail_info)
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
    std::vector<double> dom_lo, dom_hi;   // the domain, when the handle came from a .pcb file (pcx_bary_save_pcb)
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

// pcx_bary_grid.hip, pcx_bary_kfold.hip
PCX_HIDDEN int bary_pack_grid(pcx_bary *h, const double *plain, double *frag);
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

// pcx_bary_ladder.hip (BaryLadder: bary_ladder_kernels.h): the contraction plan of a ladder along `dim`, and N
// device-resident rows queued on st -- row r reads fixed[r * fstride + i] and xs[r * xstride + x], out is N x m dense.
// The launch's caller holds h->mu.
struct BaryLadder;
PCX_HIDDEN int bary_ladder_plan(const pcx_bary *h, int dim, BaryLadder *lp);
PCX_HIDDEN int bary_ladder_launch(pcx_bary *h, const BaryLadder &lp, const int32_t *deriv, const double *d_fixed, long fstride,
                                  const double *d_xs, long xstride, int m, long N, double *d_out, hipStream_t st);

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
