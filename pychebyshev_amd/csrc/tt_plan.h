// tt_plan.h -- what pcx_tt_create decides about a tensor train, the sizes its launches share with it and the host-built
// core images (pcx_tt_plan.hip).
//
// The planner is pure: it reads node counts, ranks, the domain and dim_order, calls nothing of the HIP runtime and launches
// no kernel, so every rule of it runs on a machine without a GPU (tests/host/tt_plan_main.cpp prints the plan and the
// tables of any model; tests/test_tt_plan_host.py).  pcx_tt_create validates, plans, uploads.
#pragma once

#include <vector>

#include "pcx_common.h"

#ifndef PCX_HIDDEN
#define PCX_HIDDEN __attribute__((visibility("hidden")))
#endif

// Everything pcx_tt_create decides from (d, n_nodes, ranks, lo, hi, dim_order) alone.  A form the plan allows may still
// be missing from a handle whose image failed to allocate: that is TTImages, kept beside the plan.
struct TTPlan {
    TTDims dims;                 // frag_off included
    int ranks[PCX_MAX_DIMS + 1];
    long coff[PCX_MAX_DIMS];     // offset (doubles) of storage dim k in the plain cores
    long core_total;             // doubles in the plain cores
    long frag_total;             // doubles in the direct form's packed cores (0: generic)
    int rmax, nmax;
    bool generic;                // ranks > 64: wave-per-point kernel on the plain cores, nothing below applies
    TTGeneric gi;
    // direct form on the 16x16x4 MFMA
    int cls;                     // 0: RC<=4,RT=1,NT=4   1: RC<=8,RT=2,NT=2   2: RC<=16,RT=4,NT=1
    TTRanks rk;
    int rl_last;
    int last_rows;               // rows (4 RC) of the last core's zero-padded [a][j] table, for the VALU tail
    long last_lds_doubles;       // the table's size when it is small enough to be copied to LDS, else 0
    // small-rank "W first" form (ranks <= 12, n <= 32, packed cores resident in LDS)
    int wR;                      // 0 = not available, else padded rank 4 / 8 / 12
    TTWPlan wplan;
    // small-rank direct form on the 4x4x4 MFMA (ranks <= 12, n <= 16, packed cores resident in LDS)
    int d4RA;                    // 0 = not available, else left/right chunks of 4: 1, 2, 3
    TTD4Plan d4plan;
    bool d4_preferred;           // auto: the cheaper of this form and the W-first form (cycle estimate)
    // lane-per-point VALU form (tt_lpp_kernels.h; ranks <= 16, n <= 16)
    int lppCap;                  // 0 = not available, else the instantiation's rank cap: 8, 12 or 16
    int lpp_nodes;               // the node count every dimension shares (instantiations with one switch level), 0 = they differ
    bool lpp_preferred;          // auto takes it (ranks <= 15: measured ahead of every MFMA form, profiles/r03_tt_rate_probe.txt)
};

// which of the plan's optional images a handle actually holds
struct TTImages {
    bool wfirst, d4, lpp;
};

// All of pcx_tt_create's validation of the model arrays but the cores, and every rule of the plan.  PCX_OK, or
// PCX_ERR_INVALID / PCX_ERR_UNSUPPORTED with the message set.  dim_order may be NULL (storage order = user order).
PCX_HIDDEN int tt_make_plan(int d, const int32_t *n_nodes, const int32_t *ranks, const double *lo, const double *hi,
                            const int32_t *dim_order, TTPlan &p);

// ---- dynamic LDS of each form's launch, in bytes: the planner's budget tests and the launches read the same function ----
PCX_HIDDEN size_t tt_generic_lds_bytes(const TTPlan &p);
PCX_HIDDEN size_t tt_d4_lds_bytes(const TTPlan &p);
PCX_HIDDEN size_t tt_wfirst_lds_bytes(const TTPlan &p, int NT);
PCX_HIDDEN size_t tt_direct_lds_bytes(const TTPlan &p, int nt);
PCX_HIDDEN size_t tt_lpp_lds_bytes(const TTPlan &p);

// ---- which form a launch takes ----
// requested: pcx_tt_set_kernel's variant, 0 = auto.  Returns 0 generic, 1 direct form (16x16x4), 2 W-first, 3 direct form
// (4x4x4), 4 lane per point; PCX_ERR_UNSUPPORTED (message set) when the model or the handle's images do not cover it.
PCX_HIDDEN int tt_auto_variant(const TTPlan &p, const TTImages &up, int requested);
PCX_HIDDEN bool tt_plan_has_variant(const TTPlan &p, const TTImages &up, int variant);

// ---- host-built tables (cores = the caller's plain cores G_k[a][j][b], concatenated) ----
// the last core as an [a][j] table zero-padded to last_rows rows
PCX_HIDDEN std::vector<double> tt_pack_last_core(const TTPlan &p, const double *cores);
// the 4x4x4 image (tt_kernels.h, k_tt_eval_d4): dim 0 [s][slot][NMP], mid dims [j][c][slot][NMP], last dim [4 RA][n]
PCX_HIDDEN std::vector<double> tt_pack_d4_image(const TTPlan &p, const double *cores);
// the lane-per-point image img[off_k + (b rl + a) n + j] = G_k[a][j][b], nothing padded; 64 zeroed doubles behind the
// end (scalar loads are merged into 64-byte reads); and its per-dimension table
PCX_HIDDEN std::vector<double> tt_pack_lpp_image(const TTPlan &p, const double *cores);
PCX_HIDDEN std::vector<TTLppDim> tt_lpp_table(const TTPlan &p);
