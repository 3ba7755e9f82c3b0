// pcx_bary_plan.hip -- the launch planner of the barycentric handle (bary_plan.h): which kernel form a shape runs on and
// with what geometry, and the host-built code tables.  No kernel and no HIP runtime call lives here: every function is a
// pure function of node counts, nodes and a BaryEnv, so the whole decision tree runs -- and is tested -- without a GPU.

#include "pcx_internal.h"
#include "bary_plan.h"

// ---- the environment switches ----
// g0_span: how many dim-0 orders above its base tensor's a slab GEMM serves.  Differentiating AFTER the contraction (as the
// reference's vectorized_eval_multi does) rounds differently from the reference's batch path, which differentiates the
// tensor first: each D_0 applied to the partial sums amplifies their rounding by ~|D_0| |P| / |result|.  One level keeps
// 5-D Black-Scholes delta / vanna within 2e-13 of the reference's batch result; two levels put gamma at 4.4e-12 --
// outside the 1e-12 bar -- so the default is 1 (price + delta share a GEMM, gamma keeps its own);
// PCX_BARY_G0_SPAN=2 trades that for one GEMM less, 0 switches the grouping off.
//
// group_tol: largest measured deviation of a shared spec from its own GEMM (relative to the probe batch's scale) at which a
// pair is still formed.  3e-13 keeps a factor of three to the 1e-12 parity bar for whatever batch and pairing order follow
// (PCX_BARY_GROUP_TOL / pcx_bary_set_group_tolerance override it).
//
static const int g_g0_span_default = [] { const char *e = getenv("PCX_BARY_G0_SPAN"); return e ? std::min(8, std::max(0, atoi(e))) : 1; }();
static const double g_group_tol_default = [] { const char *e = getenv("PCX_BARY_GROUP_TOL"); double v = e ? atof(e) : 0.0; return v > 0.0 ? v : 3e-13; }();

// PCX_BARY_SQ, PCX_BARY_G0_SPAN and PCX_BARY_GROUP_TOL are read once per process, the others per handle: a process may
// build both forms (tests, tools/seed_ab.py).
PCX_HIDDEN BaryEnv bary_read_env() {
    static const bool sq_auto = [] { const char *e = getenv("PCX_BARY_SQ"); return !(e && e[0] == '0'); }();
    auto first = [](const char *name) { const char *e = getenv(name); return e ? e[0] : '\0'; };
    BaryEnv env;
    env.seed = first("PCX_BARY_SEED") != '0';
    env.tail_mode = first("PCX_BARY_TAIL") == '0' ? 0 : (first("PCX_BARY_TAIL") == '2' ? 2 : 1);
    env.sq_auto = sq_auto;
    env.grid = first("PCX_BARY_GRID") == '0' ? 0 : (first("PCX_BARY_GRID") == '2' ? 2 : 1);
    env.grid_prod = first("PCX_BARY_GRID_PROD") != '0';
    env.g0_span = g_g0_span_default;
    env.group_tol = g_group_tol_default;
    env.kfold = first("PCX_BARY_KFOLD") != '0';
    env.kfold_straddle = first("PCX_BARY_KFOLD_STRADDLE") != '0';
    { const char *e = getenv("PCX_BARY_KFOLD_EFF"); env.kfold_eff = e ? atoi(e) : 0; }
    return env;
}

// ---- LDS sizes ----
PCX_HIDDEN size_t mfma4_lds_bytes(const BaryDims &dm, int ks) { return ((size_t)8 * (dm.sum_n + 2) * 32 + (size_t)2 * ks * 64) * sizeof(double); }
PCX_HIDDEN size_t mfma_lds_bytes(const BaryDims &dm, int nt) { return (size_t)4 * (dm.sum_n + 2) * 16 * nt * sizeof(double); }
// per workgroup (the k-fold form: of four waves)
PCX_HIDDEN size_t bary_grid_lds_bytes(const BaryGridPlan &gp, int nt) { return (size_t)gp.wpb * gp.trows * 16 * nt * sizeof(double); }
PCX_HIDDEN size_t bary_kfold_lds_bytes(const BaryKfoldPlan &kp, int nt) { return (size_t)4 * kp.trows * 16 * nt * sizeof(double); }
PCX_HIDDEN size_t bary_kfold_frag_count(const BaryKfoldPlan &kp) { return ((size_t)kp.nbody * kp.P * kp.MT + PCX_KFOLD_PAD) * 64; }

// ---- the row-code MFMA plan ----
static const long kSmallTensorElems = 4096;   // auto: tensors up to this size run on k_bary_small

// every k-step count up to 32 is instantiated: no padding of the folded K axis beyond 4;
// 36..64 (one column tile per wave only: the B operands alone are up to 128 VGPRs) let two
// tail dimensions of 12..16 nodes fold into K; 42 exists in the seeded sets only (13 x 13 = 1 + 4 x 42)
static const int kKsList[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22,
                              23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 36, 40, 42, 44, 48, 52, 56, 60, 64};

// K columns of which the first R are the accumulators' seed: the instantiated k-step count that runs the rest
static int pick_ks(int K, int R = 0) {
    int need = (K - R + 3) / 4;
    for (int ks : kKsList)
        if (ks >= need && (ks != 42 || R > 0)) return ks;
    return -1;
}

// K mod 4 = 1 or 2: those columns become the seed of the accumulators (R vector FMAs per accumulator register)
// and the k-loop runs (K - R) / 4 whole k-steps -- against a k-step of its own that multiplies mostly padding.
// A remainder of 3 stays a k-step (12 NT vector FMAs against NT matrix instructions).  PCX_BARY_SEED=0, read per
// handle (a process may build both forms: tests, tools/seed_ab.py), keeps every plan unseeded.
static int seed_columns(long K, bool seed) {
    const int r = (int)(K % 4);
    return (seed && K > 4 && (r == 1 || r == 2)) ? r : 0;
}

// choose the head/tail split minimising the estimated time: MT row tiles, each KS MFMAs plus
// an epilogue (head-weight look-ups and products) worth about 5 MFMAs (measured on 15^4,
// tools/bary_rate_probe.py); the single-column-tile kernels re-read A twice as often
// (costs in half MFMAs: a seeded tile pays about half a matrix instruction for its R x 4 NT vector FMAs)
static bool plan_mfma(const BaryDims &dm, BaryMfmaPlan &best, bool seed) {
    bool found = false;
    long best_cost = 0;
    for (int split = std::max(0, dm.d - 2 * PCX_CODE_FIELDS); split < dm.d; ++split) {
        if (split > 2 * PCX_CODE_FIELDS) continue;  // head dims must fit the two words of a row code
        long M = 1, K = 1, head_rows = 0, tail_rows = 0;
        for (int k = 0; k < split; ++k) { M *= dm.n[k]; head_rows += dm.n[k]; }
        for (int k = split; k < dm.d; ++k) { K *= dm.n[k]; tail_rows += dm.n[k]; }
        if (K > 256 || M > (1 << 24)) continue;
        if (head_rows > PCX_MAX_PART_ROWS || tail_rows > PCX_MAX_PART_ROWS) continue;   // 8-bit code fields per table part
        const int R = seed_columns(K, seed);
        int ks = pick_ks((int)K, R);
        if (ks < 0) continue;
        long mt = (M + 15) / 16;
        long cost = mt * (2 * ks + 10 + (R > 0 ? 1 : 0)) * (ks > 32 ? 23 : 20);
        if (!found || cost < best_cost || (cost == best_cost && K > best.K)) {
            found = true;
            best_cost = cost;
            best.split = split; best.M = (int)M; best.K = (int)K; best.MT = (int)mt; best.KS = ks; best.R = R;
            best.tail_base = (int)head_rows + 1;
            best.rows = dm.sum_n + 2;
        }
    }
    return found;
}

// ---- the grid form (k_bary_mfma_grid, bary_grid_kernels.h) ----
// Is the grid form ahead of the row-code form for this plan?  Cost per point block in matrix-instruction units: a row
// tile is KS instructions plus its epilogue -- about 5 for the row-code look-ups (plan_mfma, measured on 15^4), about 1
// here (four FMAs on four table rows at fixed strides).  The grid pads dimension A to RA and B to 16 / RA rows per tile:
// RA is chosen for the fewest tiles.  A margin of 8 % keeps the long plans (11^5: 31 k-steps) where they are.
// env.grid: PCX_BARY_GRID, read per handle (a process may build both forms: tests).
PCX_HIDDEN bool bary_plan_grid(const BaryDims &dm, const BaryMfmaPlan &plan, const BaryEnv &env, BaryGridPlan &gp) {
    if (env.grid == 0) return false;
    const int split = plan.split;
    if (split < 2 || split > 4 || dm.d - split > PCX_CODE_FIELDS || plan.KS > 32) return false;
    const int nA = dm.n[split - 2], nB = dm.n[split - 1];
    long O = 1;
    for (int k = 0; k < split - 2; ++k) O *= dm.n[k];
    long best = -1;
    for (int RA : {4, 2, 1}) {
        const int RB = 16 / RA;
        const long tiles = O * ((nA + RA - 1) / RA) * ((nB + RB - 1) / RB);
        if (best < 0 || tiles < best) {
            best = tiles;
            gp.RA = RA;
            gp.gbs = RA == 4 ? 0 : (RA == 2 ? 1 : 2);
        }
    }
    if (best > (1L << 26)) return false;
    gp.nA = nA; gp.nB = nB;
    gp.TA = (nA + gp.RA - 1) / gp.RA;
    gp.TB = (nB + 16 / gp.RA - 1) / (16 / gp.RA);
    gp.af = gp.TB * plan.KS >= 48 ? 1 : 0;                          // long chunks: A's weight formed per chunk, no table rows for A
    gp.rowA = dm.off[split - 2];
    gp.rowB = gp.af ? dm.off[split - 2] : dm.off[split - 1];
    gp.nouter = split - 2;
    gp.no1 = split == 4 ? dm.n[1] : 1;
    gp.rowo0 = dm.off[0]; gp.rowo1 = split == 4 ? dm.off[1] : 0;
    gp.nchunks = (int)(O * gp.TA);
    gp.MT = (int)best;
    const int tail_rows = dm.sum_n - dm.off[split];
    gp.hrows = gp.rowB + gp.TB * (16 / gp.RA);                       // outer rows, (A rows,) B rows, zeroed slack of B's last tile
    gp.trows = std::max(gp.hrows, tail_rows + 1) + 2;                // + 1 / S and the exact-node index of dimension A per point (af)
    // Four waves per workgroup wherever two such workgroups fit a CU (or the image is beyond L2 anyway): waves started
    // together walk the fragment image in step, so one wave's L2 fetch is an L1 hit for the other three.  With one wave per
    // workgroup every fragment load of every wave misses L1 (TCP_PENDING_STALL_CYCLES: half the kernel's cycles on 30^3;
    // measured 30^3 0.50 -> 0.54, 20^3 / 48^3 +3 %, the rest +1 %).
    const size_t table = (size_t)gp.trows * 32 * sizeof(double);
    gp.wpb = ((size_t)gp.MT * plan.KS * 512 > ((size_t)1 << 20) || 4 * table <= 80 * 1024) ? 4 : 1;

    // Measured (profiles/r04_bary_rate_probe.txt, fraction of the FP64 peak, row codes -> grid): 30^3 0.41 -> 0.55, 40^3
    // 0.54 -> 0.71, 48^3 0.78, 32^3 0.46 -> 0.64, 28^3 0.42 -> 0.58, 20^3 0.44 -> 0.49, 64^4 0.58 -> 0.84, 65^3 0.61 -> 0.74; 21^3
    // 0.39 -> 0.41 (18 % more row tiles), 7^5 0.66 -> 0.56 (27 % more): from 13 k-steps on the row-code kernel's
    // hand-pipelined loop stays ahead unless the grid pads little AND forms A's weight per chunk.
    const double cost_grid = (double)gp.MT * (plan.KS + 1.0), cost_codes = (double)plan.MT * (plan.KS + 5.0);
    if (env.grid == 2) return true;                                   // experiments: every eligible plan
    if (plan.KS > 12) return gp.MT == plan.MT || (gp.af && gp.MT * 100L <= plan.MT * 112L);      // 65^3: 289 tiles for 265, 0.61 -> 0.74
    return cost_grid <= 0.85 * cost_codes;
}

// ---- the k-fold form (k_bary_mfma_kfold, bary_kfold_kernels.h) ----
// Eligible (kfold_try): three dimensions -- any of them may play the rows --, n0 <= 64 (four row tiles in the accumulators),
// n2 <= 64 (sixteen B operands of dimension 2 in registers), at least 8 fragments per i1 (the prefetch ring).  Whether an
// eligible plan is TAKEN is decided by bary_kfold_take below (priced against the grid plan; fixed bars otherwise).
// PCX_BARY_KFOLD=0 switches the form off, PCX_BARY_KFOLD_EFF=<percent> replaces the pricing by one bar (experiments).
// One assignment of the three tensor dimensions to the roles (rows, loop, b2 registers): fills kp, returns the share of real
// products in hundredths of a percent (0: not eligible).
static long kfold_try(const BaryDims &dm, int dr, int da, int db, bool straddle, BaryKfoldPlan &kp) {
    kp.dim[0] = dr; kp.dim[1] = da; kp.dim[2] = db;
    const long st[3] = {(long)dm.n[1] * dm.n[2], (long)dm.n[2], 1L};
    for (int q = 0; q < 3; ++q) kp.stride[q] = st[kp.dim[q]];
    kp.n0 = dm.n[dr]; kp.n1 = dm.n[da]; kp.n2 = dm.n[db];
    if (kp.n0 > 64 || kp.n2 > 64 || kp.n2 < 2) return 0;
    kp.MT = (kp.n0 + 15) / 16;
    kp.KS2 = (kp.n2 + 3) / 4;
    if (kp.MT * kp.KS2 < 8) return 0;
    kp.trows = std::max(std::max(16 * kp.MT, kp.n1 + 1), 4 * kp.KS2);
    // n2 = 26, 30 (and 22): two indices of dimension 1 share a k-step instead of padding each to a multiple of four
    kp.str = (kp.n2 % 4 == 2 && kp.KS2 >= 6 && kp.KS2 <= 8 && straddle) ? 1 : 0;
    if (kp.str && ((kp.n1 + 1) / 2) * (2 * kp.KS2 - 1) >= kp.n1 * kp.KS2) kp.str = 0;      // a short odd n1: nothing saved
    kp.P = kp.str ? 2 * kp.KS2 - 1 : kp.KS2;
    kp.nbody = kp.str ? (kp.n1 + 1) / 2 : kp.n1;
    const long used = (long)kp.n0 * kp.n1 * kp.n2, padded = 16L * kp.MT * kp.nbody * kp.P * 4;
    return used * 10000 / padded;                     // hundredths of a percent
}

// What the matrix pipe makes of a row-tile count (one multiply and one fragment load feed MT x NT matrix instructions):
// measured busy x clock of the unpadded shapes, 15 x 33 x 31 0.65, 32^3 0.75, 48^3 0.84, 64^3 0.91 -- relative weights for
// choosing between assignments of equal padding (20 x 16 x 64: 64 rows in four tiles, not 16 rows in one).
static long kfold_tile_weight(int MT) { return MT >= 4 ? 100 : (MT == 3 ? 93 : (MT == 2 ? 83 : 72)); }

// The best assignment of the roles: fills kp and returns the share of real products in hundredths of a percent (0: the form is
// switched off or no assignment is eligible).  Whether the form is TAKEN is the caller's decision (bary_kfold_take).
PCX_HIDDEN long bary_plan_kfold(const BaryDims &dm, const BaryEnv &env, BaryKfoldPlan &kp) {
    if (!env.kfold || dm.d != 3) return 0;
    // the roles go to the assignment with the least padding; the natural order (rows = dimension 0, b2 = the contiguous last
    // dimension) wins ties, so cubes are packed and summed as before
    static const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    long best = 0, best_w = 0;
    BaryKfoldPlan cand;
    for (const auto &pm : perms) {
        const long sc = kfold_try(dm, pm[0], pm[1], pm[2], env.kfold_straddle, cand);
        if (sc * kfold_tile_weight(cand.MT) > best_w) { best_w = sc * kfold_tile_weight(cand.MT); best = sc; kp = cand; }
    }
    return best;
}

// Take the k-fold form?  eff: bary_plan_kfold's share of real products (1e-4).  grid_eff > 0: the grid form is the alternative, with
// that share of real products over its padded tiles and grid_ks k-steps per tile -- then both are priced by what the matrix pipe was
// measured to make of them (fraction of the FP64 peak at full tiles: k-fold by row tiles 0.65 / 0.745 / 0.84 / 0.91 -- 15 x 33 x 31,
// 32^3, 48^3, 64^3 --, grid by k-steps per tile 0.49 (5), 0.56, 0.58, 0.64, 0.67, 0.71 (10), 0.745, 0.78 (12), 0.84 (16) -- 20^3,
// 24^3, 28^3, 32^3, 40^3, 48^3, 64^4) and the k-fold form must be 6 % ahead (23^3, 24^3, 21^3 are level: they stay; 48^3, 0.84 / 0.78
// estimated, 0.885 / 0.805 measured, must not fall back); the estimates
// reproduce the measured pairs of profiles/r04_bary_rate_probe_kfold50.txt (26^3 0.605 / 0.465, 29^3 0.61 / 0.48, 40^3 0.70 / 0.71,
// 52^3 0.74 / 0.77, 36^3 0.63 / 0.65) and send 25^3 (0.52 / 0.41) to the k-fold form.  No grid plan (dim-0 groups or a row-code
// plan instead): the fixed bars, 85 % of the padded products real, more than 75 % with one or two row tiles.
// env.kfold_eff (PCX_BARY_KFOLD_EFF=<percent>) replaces all of it by one bar (experiments).
static const int kKfoldTileFrac[5] = {0, 650, 745, 840, 910};       // permille of the FP64 peak at full tiles, by row tiles

// the fraction of the FP64 peak (permille) expected of the plan: share of real products x the row-tile figure above
PCX_HIDDEN long bary_kfold_estimate(const BaryKfoldPlan &kp, long eff) {
    return eff <= 0 ? 0 : eff * kKfoldTileFrac[kp.MT < 4 ? kp.MT : 4] / 10000;
}

PCX_HIDDEN bool bary_kfold_take(const BaryKfoldPlan &kp, long eff, long grid_eff, int grid_ks, const BaryEnv &env) {
    if (eff <= 0) return false;
    if (env.kfold_eff > 0 && env.kfold_eff <= 100) return eff >= env.kfold_eff * 100L;
    if (grid_eff > 0) {
        static const int g_ks[18] = {400, 400, 400, 420, 450, 487, 560, 580, 640, 670, 710, 745, 780, 800, 815, 830, 840, 850};
        const long est_k = eff * kKfoldTileFrac[kp.MT < 4 ? kp.MT : 4];
        const long est_g = grid_eff * g_ks[grid_ks < 17 ? grid_ks : 17];
        return est_k * 100 > est_g * 106;
    }
    return kp.MT <= 2 ? eff > 7500 : eff >= 8500;
}

// ---- the plan of a handle ----
// 2^e ~ 2 / (node span): exact to apply, keeps the prefix / suffix products of the weights in range
static double node_scale(const double *nd, int n) {
    const double span = nd[n - 1] - nd[0];
    int e = 0;
    if (span > 0.0 && std::isfinite(span)) (void)std::frexp(2.0 / span, &e);
    return std::ldexp(1.0, e - 1);
}

// the lane-per-point kernels (k_bary_small, k_bary_sq): which exist for the shape and whether auto prefers them
static void plan_lane_per_point(const BaryDims &dm, long total, const double *nodes_cat, const BaryEnv &env, bool kfold_ahead,
                                BaryLaunchPlan &lp) {
    // lane-per-point kernel (k_bary_small): d <= 4, last dimension <= 64 nodes (weights in registers),
    // outer weights table (sum of outer n) x 64 lanes x 8 B within 64 KB.  Preferred by auto while the
    // tensor is small enough that the MFMA kernel's prologue outweighs its tiles
    // (tools/bary_rate_probe.py, profiles/r02_bary_rate_probe.txt).
    // every node count up to 16 has its own instantiation (no padding, no per-node tests); classes above
    static const int kNlp[] = {2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 24, 32, 48, 64};
    const int d = dm.d, nl = dm.n[d - 1];
    const long outer_rows = dm.sum_n - nl;
    if (!(d <= 4 && nl <= 64 && outer_rows * 64 * (long)sizeof(double) <= 64 * 1024 && total <= (1L << 22))) return;
    for (int v : kNlp)
        if (v >= nl) { lp.small_nlp = v; break; }
    for (int k = 0; k < d; ++k) lp.small_scale.s[k] = node_scale(nodes_cat + dm.off[k], dm.n[k]);
    // ... and 2-D tensors with a last dimension of 49 ... 64 nodes while the first has at most 48 (round 4,
    // lane-per-point / MFMA in 1e9 pts/s: 20 x 64 5.8 / 2.2, 30 x 50 3.5 / 2.6, 40 x 64 2.7 / 1.9, 48 x 64 2.1 / 1.9; 50^2
    // 2.0 / 2.1, 60^2 1.6 / 1.9, 64^2 1.6 / 1.7; 3-D shapes of that kind -- 8 x 8 x 50 -- stay on the MFMA kernel)
    // where the k-fold form is taken it is also ahead of the lane-per-point kernels (round 4, k-fold / k_bary_sq in fractions of
    // the FP64 peak: 45 x 20 x 20 0.68 / 0.31, 30 x 20 x 20 0.65 / 0.42, 32 x 16 x 16 0.65 / 0.41, 64 x 8 x 8 0.45 / 0.21, 24 x 20 x 20
    // 0.53 / 0.46, 22^3 0.49 / 0.46; without it -- 40 x 12 x 12, 26 x 14 x 14, 21^3 -- they keep their rule)
    // -- for tensors of 4,096 elements or more and plans expected at half the peak or better: (2, 17, 17) stays where it was
    lp.small_preferred = !kfold_ahead && total <= kSmallTensorElems && (nl <= 48 || (d == 2 && dm.n[0] <= 48));
    // mid-size tensors with equal trailing node counts: both trailing weight vectors in registers (k_bary_sq)
    if (d >= 2 && dm.n[d - 2] == nl && ((nl >= 4 && nl <= 24) || nl == 26 || nl == 28 || nl == 30 || nl == 32) &&
        (outer_rows - nl) * 64 * (long)sizeof(double) <= 48 * 1024) {
        lp.sq_nl = nl;
        // tools/bary_rate_probe.py (profiles/r03_bary_rate_probe.txt): ahead of k_bary_small everywhere it applies
        // (12^2 +33 %, 8^3 +37 %, 11^3 +44 %, 6^4 +50 %) and of the MFMA kernel's short plans for d <= 3
        // (17^3 +48 %, 20^3 +11 %, 24^3 +15 %); from 10^4 up the MFMA kernel (K = n^2 >= 100) is ahead
        // 21 and 23 nodes: hipcc runs out of scalar registers on the odd row length (SGPR spills in the block,
        // 0.37 / 0.36 of the peak against 0.39 / 0.44 on the MFMA kernel): available, not preferred
        // 26 / 28 / 30 nodes: ahead in 2-D (26^2 0.40 against 0.21), behind the MFMA kernel in 3-D (30^3 0.32 against 0.42)
        // round 4 (k_bary_mfma_grid): 20^3 0.45 -> 0.48, 24^3 0.545 -> 0.56, 32^3 0.48 -> 0.63 on the MFMA kernel
        // (21 nodes: 0.44 here against 0.40 on the grid MFMA kernel -- preferred again; 23: 0.465 against 0.47)
        lp.sq_preferred = !kfold_ahead && env.sq_auto && (d <= 3 || total <= kSmallTensorElems) && nl != 23 &&
                          !(d >= 3 && nl >= 24) && !(d == 3 && nl == 20 && dm.n[0] == 20);      // 24^3: grid 0.56, here 0.545
    }
}

// dim-0 groups: head = dimension 0 x (dimensions 1 .. split-1); the rows of one i0 form a slab padded to whole
// tiles.  Needs two column tiles per wave (large batches only), narrow codes, and room for two n0-vectors
// per point in the tail part of the LDS table (dead once the B operands are in registers); n0 <= 16 bounds the
// rounding amplification of the D_0 step (~ n0^2 eps).  Returns the row tiles per slab, 0: the shape has no slab plan.
static int plan_slabs(const BaryDims &dm, const BaryMfmaPlan &p, bool wide, int nt) {
    long M1 = 1;
    for (int k = 1; k < p.split; ++k) M1 *= dm.n[k];
    if (!(!wide && p.split >= 2 && p.split <= PCX_CODE_FIELDS && nt == 2 && p.KS <= 32 && M1 >= 16 &&
          2 * dm.n[0] <= p.rows - p.tail_base && dm.n[0] >= 2 && dm.n[0] <= 16))
        return 0;
    const int tps = (int)((M1 + 15) / 16);
    // padding must stay cheap: at most 15 % more row tiles than the plain plan
    return (long)tps * dm.n[0] * 100 <= (long)p.MT * 115 ? tps : 0;
}

PCX_HIDDEN int bary_make_plan(const BaryDims &dm, long total, const double *nodes_cat, const BaryEnv &env, BaryLaunchPlan &lp) {
    lp = BaryLaunchPlan();
    const int d = dm.d;
    const long sum_n = dm.sum_n;
    // rows kernel geometry: lanes per point = smallest power of two >= number of rows
    const long Mrows = total / dm.n[d - 1];
    int lpp = 1;
    while (lpp < 64 && lpp < Mrows) lpp <<= 1;
    // its LDS weight table is (256 / lpp) points x sum_n doubles: widen the groups until it fits
    while (lpp < 64 && (size_t)(256 / lpp) * sum_n * sizeof(double) > 48 * 1024) lpp <<= 1;
    lp.lpp = lpp;
    lp.seed = env.seed;
    lp.tail_mode = env.tail_mode;

    // the row-code MFMA plan (seeded where the seed pays) and its column tiles per wave
    BaryMfmaPlan seeded{};
    bool mfma_ok = plan_mfma(dm, seeded, env.seed);
    const bool narrow = mfma_ok && seeded.split <= PCX_CODE_FIELDS && d - seeded.split <= PCX_CODE_FIELDS;
    int nt = 2;
    if (mfma_ok) {
        // two column tiles per wave while the B operands fit the register file beside them: up to 32 k-steps, 36 and 40 with
        // narrow codes (232 ... 256 VGPRs at two waves per SIMD; round 4, one against two column tiles: 12^4 0.642 -> 0.683,
        // 12 x 12 x 10 x 16 0.629 -> 0.682, 6 x 6 x 6 x 12 x 12 0.644 -> 0.692 -- each fragment load feeds two matrix instructions)
        nt = (seeded.KS <= 32 || (narrow && seeded.KS <= 40)) ? 2 : 1;
        if (mfma_lds_bytes(dm, nt) > 150 * 1024) nt = 1;
        if (mfma_lds_bytes(dm, nt) > 150 * 1024) mfma_ok = false;
    }
    // shapes no kernel covers fail here, at create, not at the first evaluation: the rows kernel
    // keeps (256 / lpp) x sum_n weights in LDS
    if (!mfma_ok && (size_t)(256 / lpp) * sum_n * sizeof(double) > 160 * 1024)
        return fail(PCX_ERR_UNSUPPORTED, "sum of node counts %ld too large for any kernel (MFMA plan: each of the "
                    "head / tail parts <= %d rows and a tail product <= 256; row kernel: sum <= 5120)", sum_n, PCX_MAX_PART_ROWS);
    lp.mfma_ok = mfma_ok;
    lp.wide = mfma_ok && !narrow;
    const int slab_tps = mfma_ok ? plan_slabs(dm, seeded, lp.wide, nt) : 0;

    // short plans: the grid form (bary_grid_kernels.h) -- unless the shape can share GEMMs between specs one order apart
    // (dim-0 groups), which needs the slab packing of the row-code form
    // Their planners and packers know no seed: they are priced, and where one of them is taken run, on the plan with
    // every column in the k-loop
    BaryMfmaPlan uplan = seeded;
    uplan.R = 0;
    if (mfma_ok) uplan.KS = pick_ks(uplan.K);
    long kfold_est = 0;                               // permille of the FP64 peak expected of the k-fold plan
    if (mfma_ok && narrow) {
        // 3-D tensors one of whose dimensions fills whole row tiles: the k-fold form (bary_kfold_kernels.h) ahead of the grid
        // form -- and of the dim-0 groups: 9 x 48 x 30 runs at 0.30 of the peak on the row-code form a group would share, the
        // k-fold form (rows = the 48) takes every launch of it to 0.8
        const long keff = bary_plan_kfold(dm, env, lp.kf);
        kfold_est = bary_kfold_estimate(lp.kf, keff);
        long geff = 0;
        if (keff > 0 && !slab_tps) {
            // the alternative is the grid form -- or the row-code form where the grid planner declines, which it does when it
            // expects no more of its own form: priced as a grid plan either way (25 x 25 x 40: row codes 0.44, k-fold 0.6)
            BaryGridPlan gtry;
            gtry.MT = 0;
            (void)bary_plan_grid(dm, uplan, env, gtry);
            if (gtry.MT > 0)
                geff = (long)((double)uplan.M * uplan.K * 10000.0 / ((double)gtry.MT * 16.0 * uplan.KS * 4.0));
        }
        if (bary_kfold_take(lp.kf, keff, geff, uplan.KS, env)) {
            const int nt_kf = bary_kfold_lds_bytes(lp.kf, 2) > (size_t)72 * 1024 ? 1 : 2;      // two workgroups per CU
            lp.kfold_ok = bary_kfold_lds_bytes(lp.kf, nt_kf) <= (size_t)150 * 1024;            // else: a very long middle dimension
            if (lp.kfold_ok) nt = nt_kf;
        }
        if (!lp.kfold_ok && !slab_tps && bary_plan_grid(dm, uplan, env, lp.gp)) {
            const size_t cap = (size_t)(lp.gp.wpb == 4 ? 150 : 64) * 1024;
            nt = (uplan.KS > 32 || bary_grid_lds_bytes(lp.gp, 2) > cap) ? 1 : 2;   // the table is per wave and holds one part at a time
            lp.grid_ok = bary_grid_lds_bytes(lp.gp, nt) <= cap;
        }
    }
    lp.nt = nt;
    lp.plan = (lp.grid_ok || lp.kfold_ok) ? uplan : seeded;
    lp.g0_ok = slab_tps > 0 && !lp.kfold_ok;          // the k-fold form takes the slab plan's place where both exist (above)
    lp.g0_tps = lp.g0_ok ? slab_tps : 0;
    if (lp.g0_ok) lp.g0_nf = std::max(2, seeded.split - 1);
    // division-free weights for the grid and k-fold forms (bary_weights.h; as k_bary_small): nodes scaled by 2^e ~ 2 / span
    // per dimension, every dimension <= 64 nodes; PCX_BARY_GRID_PROD=0 (read per handle) keeps the weights by division (A/B measurements)
    lp.grid_prod = (lp.grid_ok || lp.kfold_ok) && env.grid_prod && *std::max_element(dm.n, dm.n + d) <= 64;
    lp.mfma4_ok = mfma_ok && !lp.grid_ok && !lp.kfold_ok && mfma4_lds_bytes(dm, seeded.KS) <= 160 * 1024 && seeded.KS <= 32 && narrow;
    plan_lane_per_point(dm, total, nodes_cat, env, lp.kfold_ok && total >= kSmallTensorElems && kfold_est >= 500, lp);
    return PCX_OK;
}

// ---- what the info entry points report ----
// the kernel a launch takes while no variant is set: 1 rows, 2 MFMA 16x16x4, 4 lane-per-point, 5 k_bary_sq
PCX_HIDDEN int bary_auto_variant(const BaryLaunchPlan &lp) {
    if (lp.sq_nl && lp.sq_preferred) return 5;
    return (lp.small_nlp && (lp.small_preferred || !lp.mfma_ok)) ? 4 : (lp.mfma_ok ? 2 : 1);
}

PCX_HIDDEN bool bary_plan_has_variant(const BaryLaunchPlan &lp, int variant) {
    const bool has[6] = {false, true, lp.mfma_ok, lp.mfma4_ok, lp.small_nlp != 0, lp.sq_nl != 0};
    return variant >= 1 && variant <= 5 && has[variant];
}

PCX_HIDDEN void bary_plan_kernel_info(const BaryLaunchPlan &lp, const BaryDims &dm, int32_t info[6]) {
    info[0] = bary_auto_variant(lp);
    info[1] = lp.mfma_ok ? (lp.kfold_ok ? lp.kf.MT : (lp.grid_ok ? lp.gp.MT : lp.plan.MT)) : 0;
    info[2] = lp.mfma_ok ? (lp.kfold_ok ? lp.kf.nbody * lp.kf.P : lp.plan.KS) : 0;
    info[3] = lp.mfma_ok ? (int32_t)(lp.kfold_ok ? bary_kfold_lds_bytes(lp.kf, lp.nt)
                                                  : (lp.grid_ok ? bary_grid_lds_bytes(lp.gp, lp.nt) : mfma_lds_bytes(dm, lp.nt)))
                         : (256 / lp.lpp) * dm.sum_n * 8;
    info[4] = lp.mfma_ok ? 64 * lp.nt : 256 / lp.lpp;
    info[5] = lp.mfma_ok ? lp.plan.split : dm.d - 1;
}

PCX_HIDDEN void bary_plan_grid_info(const BaryLaunchPlan &lp, int32_t info[4]) {
    info[0] = lp.grid_ok ? 1 : (lp.kfold_ok ? 2 : 0);
    info[1] = lp.grid_ok ? lp.gp.RA : 0;
    info[2] = lp.grid_ok ? lp.gp.MT : (lp.kfold_ok ? lp.kf.MT : 0);
    info[3] = lp.grid_ok ? lp.gp.nchunks : (lp.kfold_ok ? lp.kf.KS2 : 0);
}

PCX_HIDDEN bool bary_plan_rowcode_form(const BaryLaunchPlan &lp) { return lp.mfma_ok && !lp.kfold_ok && !lp.grid_ok; }

// all zero when launches do not take the row-code form; [0], [4], [5] are the device's and the latest launch's (pcx_bary_tail_info)
PCX_HIDDEN void bary_plan_tail_info(const BaryLaunchPlan &lp, int32_t info[6]) {
    for (int i = 0; i < 6; ++i) info[i] = 0;
    if (!bary_plan_rowcode_form(lp)) return;
    info[1] = 64 * lp.nt;
    info[2] = (lp.plan.MT + PCX_CHUNK_TILES - 1) / PCX_CHUNK_TILES;
    info[3] = lp.tail_mode;
}

// ---- host-built tables ----
// One code: index `idx` over dimensions [first, last) -- the last one fastest -- as table rows relative to `base`, one 8-bit
// field per dimension from field 0 on; every other field, and every field of an index beyond `count`, names the all-ones
// row `ones`.  Returned is word 0 (fields 0 .. 3) or word 1 (fields 4 .. 7).
static unsigned code_word(const BaryDims &dm, int first, int last, int base, long idx, long count, unsigned ones, int word) {
    unsigned f[2 * PCX_CODE_FIELDS] = {ones, ones, ones, ones, ones, ones, ones, ones};
    if (idx < count) {
        long rem = idx;
        for (int k = last - 1; k >= first; --k) {
            f[k - first] = (unsigned)(dm.off[k] - base + (int)(rem % dm.n[k]));
            rem /= dm.n[k];
        }
    }
    const unsigned *w = f + PCX_CODE_FIELDS * word;
    return w[0] | (w[1] << 8) | (w[2] << 16) | (w[3] << 24);
}

// device layout of the row codes: the four codes a lane needs for a tile (rows g, g+4, g+8, g+12 of
// tile t) side by side, [t][g][j], so that one 16-byte load fetches them
static std::vector<unsigned> lane_order(const std::vector<unsigned> &v) {
    std::vector<unsigned> o(v.size());
    for (size_t t = 0; t < v.size() / 16; ++t)
        for (int g = 0; g < 4; ++g)
            for (int j = 0; j < 4; ++j) o[(4 * t + g) * 4 + j] = v[16 * t + g + 4 * j];
    return o;
}

// all-ones rows: the last row of the head part (row codes) and of the tail part (k codes)
PCX_HIDDEN std::vector<unsigned> bary_row_codes(const BaryDims &dm, const BaryMfmaPlan &p, int word) {
    std::vector<unsigned> rc((size_t)p.MT * 16);
    for (size_t m = 0; m < rc.size(); ++m) rc[m] = code_word(dm, 0, p.split, 0, (long)m, p.M, (unsigned)(p.tail_base - 1), word);
    return lane_order(rc);
}

// the pipelined loop of the narrow instantiations (k_bary_mfma, KS >= 12) reads row OFFSETS: every field as
// the LDS byte offset row * PW * 8 of its table row, 16 bits each (rows <= 255, PW <= 32), two 16-byte words
// per (tile, lane group): [t][g][fields 0 | 1 << 16, fields 2 | 3 << 16][j].  One table per PW = 16 NT.
PCX_HIDDEN bool bary_plan_row_offsets(const BaryLaunchPlan &lp) { return bary_plan_rowcode_form(lp) && !lp.wide && lp.plan.KS >= 12; }

PCX_HIDDEN std::vector<unsigned> bary_row_offsets(const std::vector<unsigned> &rowcode, int nt) {
    std::vector<unsigned> offs(rowcode.size() * 2);
    const unsigned sc = 16u * nt * sizeof(double);
    for (size_t q = 0; q < rowcode.size() / 4; ++q)              // q = 4 t + g
        for (int j = 0; j < 4; ++j) {
            const unsigned code = rowcode[4 * q + j];
            offs[8 * q + j] = ((code & 255u) * sc) | ((((code >> 8) & 255u) * sc) << 16);
            offs[8 * q + 4 + j] = (((code >> 16) & 255u) * sc) | (((code >> 24) * sc) << 16);
        }
    return offs;
}

PCX_HIDDEN std::vector<unsigned> bary_slab_row_codes(const BaryDims &dm, const BaryLaunchPlan &lp) {
    const BaryMfmaPlan &p = lp.plan;
    const long M1 = p.M / dm.n[0];
    std::vector<unsigned> rc((size_t)lp.g0_tps * dm.n[0] * 16);
    for (size_t m = 0; m < rc.size(); ++m)
        rc[m] = code_word(dm, 1, p.split, 0, (long)((m / 16) % lp.g0_tps) * 16 + (long)(m % 16), M1, (unsigned)(p.tail_base - 1), 0);
    return lane_order(rc);
}

// k codes: entry kk names column R + kk (the fragment image starts behind the seed columns); the R seed
// columns 0 .. R-1 follow at 4 KS + r.  Rows are relative to the tail part.
PCX_HIDDEN std::vector<unsigned> bary_k_codes(const BaryDims &dm, const BaryMfmaPlan &p, int word) {
    std::vector<unsigned> kc((size_t)p.KS * 4 + p.R);
    for (long kk = 0; kk < (long)kc.size(); ++kk) {
        const long col = kk < (long)p.KS * 4 ? p.R + kk : kk - (long)p.KS * 4;
        kc[kk] = code_word(dm, p.split, dm.d, dm.off[p.split], col, p.K, (unsigned)(p.rows - 1 - p.tail_base), word);
    }
    return kc;
}

PCX_HIDDEN std::vector<double> bary_scaled_nodes(const BaryDims &dm, const double *nodes_cat, bool with_scales) {
    std::vector<double> sn((size_t)dm.sum_n + (with_scales ? PCX_MAX_DIMS : 0), 0.0);
    for (int k = 0; k < dm.d; ++k) {
        const double sck = node_scale(nodes_cat + dm.off[k], dm.n[k]);
        if (with_scales) sn[(size_t)dm.sum_n + k] = sck;
        for (int j = 0; j < dm.n[k]; ++j) sn[dm.off[k] + j] = nodes_cat[dm.off[k] + j] * sck;
    }
    return sn;
}
