// bary_plan.h -- the launch plan of a barycentric handle and the host-built tables it asks for (pcx_bary_plan.hip).
//
// The planner is pure: it reads node counts, the nodes and a BaryEnv, calls nothing of the HIP runtime and launches no
// kernel, so every rule of it runs on a machine without a GPU (tests/host/bary_plan_main.cpp prints the plan and the
// tables of any shape; tests/test_bary_plan_host.py).  pcx_bary_create validates, plans, uploads.
#pragma once

#include <vector>

#include "pcx_common.h"

#ifndef PCX_HIDDEN
#define PCX_HIDDEN __attribute__((visibility("hidden")))
#endif
#ifndef PCX_CHUNK_TILES
#define PCX_CHUNK_TILES 4        // row tiles per chunk of a split launch: bary_kernels.h owns it; this unit includes no kernel header
#endif

// The environment switches of the planner, read in ONE place (bary_read_env).
struct BaryEnv {
    bool seed = true;            // PCX_BARY_SEED=0: no plan seeds its accumulators (per handle)
    int tail_mode = 1;           // PCX_BARY_TAIL: 0 never, 1 where it pays, 2 wherever the geometry allows (per handle)
    bool sq_auto = true;         // PCX_BARY_SQ=0: auto never picks k_bary_sq (per process)
    int grid = 1;                // PCX_BARY_GRID: 0 no grid form, 1 where it is ahead, 2 every eligible plan (per handle)
    bool grid_prod = true;       // PCX_BARY_GRID_PROD=0: the grid / k-fold weights by division (per handle)
    int g0_span = 1;             // PCX_BARY_G0_SPAN (per process)
    double group_tol = 3e-13;    // PCX_BARY_GROUP_TOL (per process)
    bool kfold = true;           // PCX_BARY_KFOLD=0: no k-fold form (per handle)
    bool kfold_straddle = true;  // PCX_BARY_KFOLD_STRADDLE=0: pad n2 = 26, 30 instead (A/B; per handle)
    int kfold_eff = 0;           // PCX_BARY_KFOLD_EFF=<percent>: one bar instead of the pricing (experiments; per handle)
};
PCX_HIDDEN BaryEnv bary_read_env();

// What pcx_bary_create decides about a shape: which kernel forms exist, which one auto picks, and their geometry.
struct BaryLaunchPlan {
    bool mfma_ok = false;
    bool seed = true;                // K-remainder columns seed the accumulators (PCX_BARY_SEED=0 at create: never)
    BaryMfmaPlan plan;
    int nt = 2;                      // point tiles per wave in the MFMA kernel
    bool wide = false;               // more than four head or tail dimensions
    int tail_mode = 1;               // tail split of large launches (launch_mfma_t): 1 where the row-tile walk is long enough to pay
                                     // for the second kernel; PCX_BARY_TAIL=0 at create: never, =2: wherever the geometry allows
    // short plans: row tiles = RA x RB blocks of the last two head dimensions, no row codes (bary_grid_kernels.h);
    // the fragment image of every derivative tensor is then packed in that order
    bool grid_ok = false;
    BaryGridPlan gp;
    bool kfold_ok = false;           // 3-D, whole row tiles along dimension 0: k_bary_mfma_kfold (bary_kfold_kernels.h)
    BaryKfoldPlan kf;
    bool grid_prod = false;          // every dimension <= 64 nodes: division-free weights (grid_weights_prod)
    // dim-0 groups (BaryG0): specs differing only in their dim-0 order share one slab-packed GEMM
    bool g0_ok = false;
    int g0_tps = 0;                  // row tiles per dim-0 slab
    int g0_nf = 2;                   // live row-code fields (head dimensions 1 .. split-1, at least two)
    int lpp = 64;                    // lanes per point in the rows kernel
    bool mfma4_ok = false;           // 4x4x4_4b form available (LDS budget)
    int small_nlp = 0;               // lane-per-point kernel for small tensors: padded last-dim width, 0 = not available
    BarySmallScale small_scale;      // its power-of-two coordinate scales
    bool small_preferred = false;    // auto picks it (few row tiles: the MFMA kernel would be all prologue)
    int sq_nl = 0;                   // k_bary_sq (last two dimensions of sq_nl nodes each, d <= 4): 0 = not available
    bool sq_preferred = false;       // auto picks it
};

// Everything pcx_bary_create decides, from the node counts (dm), their product and the nodes alone.  PCX_OK, or
// PCX_ERR_UNSUPPORTED (message set) for shapes no kernel covers.
PCX_HIDDEN int bary_make_plan(const BaryDims &dm, long total, const double *nodes_cat, const BaryEnv &env, BaryLaunchPlan &lp);

// the planners and sizes the launch code calls by name
PCX_HIDDEN bool bary_plan_grid(const BaryDims &dm, const BaryMfmaPlan &plan, const BaryEnv &env, BaryGridPlan &gp);
PCX_HIDDEN long bary_plan_kfold(const BaryDims &dm, const BaryEnv &env, BaryKfoldPlan &kp);
PCX_HIDDEN long bary_kfold_estimate(const BaryKfoldPlan &kp, long eff);
PCX_HIDDEN bool bary_kfold_take(const BaryKfoldPlan &kp, long eff, long grid_eff, int grid_ks, const BaryEnv &env);
PCX_HIDDEN size_t bary_kfold_frag_count(const BaryKfoldPlan &kp);
PCX_HIDDEN size_t mfma_lds_bytes(const BaryDims &dm, int nt);
PCX_HIDDEN size_t mfma4_lds_bytes(const BaryDims &dm, int ks);
PCX_HIDDEN size_t bary_kfold_lds_bytes(const BaryKfoldPlan &kp, int nt);
PCX_HIDDEN size_t bary_grid_lds_bytes(const BaryGridPlan &gp, int nt);

// ---- what the info entry points report of a plan (pcx_bary_kernel_info, _grid_info, _tail_info[1..3], _set_kernel) ----
PCX_HIDDEN int bary_auto_variant(const BaryLaunchPlan &lp);        // 1 rows, 2 MFMA 16x16x4, 4 lane-per-point, 5 k_bary_sq
PCX_HIDDEN bool bary_plan_has_variant(const BaryLaunchPlan &lp, int variant);    // variant 1 .. 5
PCX_HIDDEN void bary_plan_kernel_info(const BaryLaunchPlan &lp, const BaryDims &dm, int32_t info[6]);
PCX_HIDDEN void bary_plan_grid_info(const BaryLaunchPlan &lp, int32_t info[4]);
PCX_HIDDEN bool bary_plan_rowcode_form(const BaryLaunchPlan &lp);  // launches take the row-code MFMA kernel (tail_info: else all zero)
PCX_HIDDEN void bary_plan_tail_info(const BaryLaunchPlan &lp, int32_t info[6]);  // [1], [2], [3]; the device's part and the rest: 0

// ---- host-built tables (device layouts: see the builders) ----
// row codes of the plan's head part, word 0 (fields 0..3) or 1 (fields 4..7: wide plans), in lane order: MT * 16 entries
PCX_HIDDEN std::vector<unsigned> bary_row_codes(const BaryDims &dm, const BaryMfmaPlan &p, int word);
// the lane-ordered low row codes as LDS byte offsets for PW = 16 nt: MT * 32 entries
PCX_HIDDEN std::vector<unsigned> bary_row_offsets(const std::vector<unsigned> &rowcode, int nt);
PCX_HIDDEN bool bary_plan_row_offsets(const BaryLaunchPlan &lp);   // the plan's launches read them
// row codes of the dim-0 slabs (lp.g0_ok), lane-ordered: n0 * g0_tps * 16 entries
PCX_HIDDEN std::vector<unsigned> bary_slab_row_codes(const BaryDims &dm, const BaryLaunchPlan &lp);
// k codes, word 0 or 1: 4 KS entries, then the R seed columns
PCX_HIDDEN std::vector<unsigned> bary_k_codes(const BaryDims &dm, const BaryMfmaPlan &p, int word);
// nodes times a power of two per dimension (sum_n doubles); with_scales: then the PCX_MAX_DIMS scales themselves
PCX_HIDDEN std::vector<double> bary_scaled_nodes(const BaryDims &dm, const double *nodes_cat, bool with_scales);
