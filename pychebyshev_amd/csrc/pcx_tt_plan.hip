// pcx_tt_plan.hip -- the planner of the tensor-train handle (tt_plan.h): which evaluation forms a model has and with what
// geometry, the LDS each launch takes, which form a launch runs, and the host-built core images.  No kernel and no HIP
// runtime call lives here: every function is a pure function of the model's shape (the packers: and its cores), so the
// whole decision tree runs -- and is tested -- without a GPU.

#include "pcx_internal.h"
#include "tt_plan.h"

// ---- dynamic LDS per launch ----
// generic kernel: 2 rmax + nmax doubles per wave, 4 waves per workgroup
PCX_HIDDEN size_t tt_generic_lds_bytes(const TTPlan &p) { return (size_t)4 * (2 * p.rmax + p.nmax) * sizeof(double); }

// 4x4x4 form: the image, the bounds table and per wave the query rows of a batch and a 6-double record per point
PCX_HIDDEN size_t tt_d4_lds_bytes(const TTPlan &p) {
    const size_t per_wave = (size_t)16 * p.dims.d + 16 * 6;
    return ((size_t)p.d4plan.total + (size_t)2 * 16 * p.dims.d + 4 * per_wave) * sizeof(double);
}

PCX_HIDDEN size_t tt_wfirst_lds_bytes(const TTPlan &p, int NT) {
    return ((size_t)p.wplan.total + (size_t)(4 + 2) * 16 * NT * p.dims.d) * sizeof(double);
}

// 16x16x4 direct form: query rows + the last core when it is small
PCX_HIDDEN size_t tt_direct_lds_bytes(const TTPlan &p, int nt) {
    return ((size_t)4 * 16 * nt * p.dims.d + (size_t)p.last_lds_doubles) * sizeof(double);
}

PCX_HIDDEN size_t tt_lpp_lds_bytes(const TTPlan &p) { return (size_t)p.rmax * PCX_LPP_WG * sizeof(double); }

// ---- the plan ----
static void tt_plan_direct(TTPlan &p) {
    const int d = p.dims.d;
    p.cls = p.rmax <= 16 ? 0 : (p.rmax <= 32 ? 1 : 2);
    // dim 0 stores one left chunk; later dims are padded to the kernel's compile-time RC chunks x RT tiles so that its
    // node loop is branch-free
    const int RC = p.cls == 0 ? (p.rmax + 3) / 4 : (p.cls == 1 ? 8 : 16);
    const int RT = p.cls == 0 ? 1 : (p.cls == 1 ? 2 : 4);
    for (int k = 0; k < d; ++k) {
        p.rk.rc[k] = (k == 0) ? 1 : RC;
        p.rk.rt[k] = RT;
        p.dims.frag_off[k] = p.frag_total;
        p.frag_total += (long)p.dims.n[k] * p.rk.rc[k] * p.rk.rt[k] * 64;
    }
    p.rl_last = p.ranks[d - 1];
    p.last_rows = 4 * RC;
    const size_t last = (size_t)p.last_rows * p.dims.n[d - 1];
    p.last_lds_doubles = (last * sizeof(double) <= 16 * 1024) ? (long)last : 0;
}

// W-first image (small ranks, n <= 32): every dim but the last as (R*R) x n GEMM fragments padded to a common k-step
// count, the last dim as an [R][4 ks] table; the whole image must fit the kernel's LDS budget.
static void tt_plan_wfirst(TTPlan &p) {
    if (p.rmax > 12 || p.nmax > 32) return;
    const int d = p.dims.d, R = 4 * ((p.rmax + 3) / 4), ks = (p.nmax + 3) / 4;
    long total = 0;
    for (int k = 0; k < d; ++k) {
        p.wplan.ntiles[k] = (k == 0) ? (R + 15) / 16 : R * R / 16;   // compile-time tile counts of the kernel
        p.wplan.lds_off[k] = (int)total;
        total += (k == d - 1) ? (long)R * 4 * ks : (long)ks * p.wplan.ntiles[k] * 64;
    }
    p.wplan.ks = ks;
    p.wplan.total = (int)total;
    if (total * (long)sizeof(double) <= 96 * 1024) p.wR = R;
}

static void tt_plan_d4(TTPlan &p) {
    if (p.rmax > 12 || p.nmax > PCX_D4_MAX_NODES) return;
    const int d = p.dims.d, RA = (p.rmax + 3) / 4, NMP = RA == 3 ? 4 : RA;
    long total = 0;
    for (int k = 0; k < d; ++k) {
        p.d4plan.lds_off[k] = (int)total;
        const long nk = p.dims.n[k];
        total += (k == d - 1) ? 4L * RA * nk : (k == 0) ? ((nk + 3) / 4) * 16L * NMP : nk * RA * 16L * NMP;
    }
    p.d4plan.total = (int)total;
    if (tt_d4_lds_bytes(p) > 72 * 1024) return;     // two workgroups per CU at least
    p.d4RA = RA;
    // which small-rank form auto takes: FP64-pipe cycles per 16 points and middle dimension, from tools/tt_rate_probe.py
    // (profiles/r02_tt_rate_probe.txt): the 4x4x4 form issues n RA^2 instructions of ~20 cycles and pads nothing; the
    // W-first form R^2/16 ceil(n/4) instructions of ~75 cycles plus a fold.  Ranks <= 4 always favour the 4x4x4 form.
    if (p.wR && RA > 1) {
        long c4 = 0, cw = 0;
        for (int k = 1; k < d - 1; ++k) {
            c4 += (long)p.dims.n[k] * RA * RA * 20 + 100;
            cw += (long)(p.wR * p.wR / 16) * p.wplan.ks * 75 + 160;
        }
        p.d4_preferred = c4 <= cw;
    }
}

static void tt_plan_lpp(TTPlan &p) {
    if (p.rmax > PCX_LPP_MAX_RANK || p.nmax > PCX_LPP_MAX_NODES) return;
    p.lppCap = p.rmax <= 8 ? 8 : (p.rmax <= 12 ? 12 : 16);
    p.lpp_nodes = p.dims.n[0];
    for (int k = 1; k < p.dims.d; ++k)
        if (p.dims.n[k] != p.dims.n[0]) p.lpp_nodes = 0;
    p.lpp_preferred = p.rmax <= 15;       // rank 16: the 16x16x4 direct form is ahead (0.70-0.79 vs 0.66-0.69)
}

PCX_HIDDEN int tt_make_plan(int d, const int32_t *n_nodes, const int32_t *ranks, const double *lo, const double *hi,
                            const int32_t *dim_order, TTPlan &p) {
    p = TTPlan{};
    p.rmax = p.nmax = 1;
    p.d4_preferred = true;
    if (d < 1 || d > PCX_MAX_DIMS) return fail(PCX_ERR_INVALID, "d=%d outside [1, %d]", d, PCX_MAX_DIMS);
    if (!n_nodes || !ranks || !lo || !hi) return fail(PCX_ERR_INVALID, "NULL model array");
    if (ranks[0] != 1 || ranks[d] != 1) return fail(PCX_ERR_INVALID, "boundary TT ranks must be 1");
    p.dims.d = d;
    bool seen[PCX_MAX_DIMS] = {false};
    for (int k = 0; k < d; ++k) {
        if (n_nodes[k] < 1 || n_nodes[k] > 4096 || ranks[k] < 1 || ranks[k + 1] < 1)
            return fail(PCX_ERR_INVALID, "bad n_nodes/ranks at dim %d", k);
        if (!(lo[k] < hi[k])) return fail(PCX_ERR_INVALID, "domain[%d]: lo must be < hi", k);
        const int col = dim_order ? dim_order[k] : k;
        if (col < 0 || col >= d || seen[col]) return fail(PCX_ERR_INVALID, "dim_order is not a permutation");
        seen[col] = true;
        p.dims.n[k] = n_nodes[k];
        p.dims.col[k] = col;
        p.dims.lo[k] = lo[k];
        p.dims.hi[k] = hi[k];
        p.dims.scale[k] = 2.0 / (hi[k] - lo[k]);
        p.coff[k] = p.core_total;
        p.core_total += (long)ranks[k] * n_nodes[k] * ranks[k + 1];
        p.ranks[k] = ranks[k];
        p.ranks[k + 1] = ranks[k + 1];
        p.nmax = std::max(p.nmax, (int)n_nodes[k]);
        p.rmax = std::max(p.rmax, std::max(ranks[k], ranks[k + 1]));
    }
    if (p.rmax > 64) {
        // outside the MFMA tilings: the generic wave-per-point kernel on the plain cores
        if (p.rmax > 4096) return fail(PCX_ERR_UNSUPPORTED, "TT rank %d > 4096", p.rmax);
        if (tt_generic_lds_bytes(p) > 160 * 1024)
            return fail(PCX_ERR_UNSUPPORTED, "TT rank %d with %d nodes exceeds the generic kernel's LDS budget "
                        "(2 rank + nodes <= 5120)", p.rmax, p.nmax);
        p.generic = true;
        p.gi.rmax = p.rmax;
        p.gi.nmax = p.nmax;
        for (int k = 0; k < d; ++k) p.gi.coff[k] = p.coff[k];
        for (int k = 0; k <= d; ++k) p.gi.rank[k] = ranks[k];
        return PCX_OK;
    }
    tt_plan_direct(p);
    tt_plan_wfirst(p);
    tt_plan_d4(p);
    tt_plan_lpp(p);
    return PCX_OK;
}

// ---- which form a launch takes ----
PCX_HIDDEN int tt_auto_variant(const TTPlan &p, const TTImages &up, int requested) {
    const bool w = p.wR && up.wfirst, d4 = p.d4RA && up.d4, lpp = p.lppCap && up.lpp;
    if (requested == 2 && !w) return fail(PCX_ERR_UNSUPPORTED, "W-first TT kernel does not cover this model");
    if (requested == 3 && !d4) return fail(PCX_ERR_UNSUPPORTED, "4x4x4 direct TT kernel does not cover this model");
    if (requested == 4 && !lpp) return fail(PCX_ERR_UNSUPPORTED, "lane-per-point TT kernel does not cover this model");
    if (p.generic) return requested ? fail(PCX_ERR_UNSUPPORTED, "ranks above 64 run on the generic kernel only") : 0;
    if (lpp && (requested == 4 || (requested == 0 && p.lpp_preferred))) return 4;
    if (d4 && (requested == 3 || (requested == 0 && (!w || p.d4_preferred)))) return 3;
    if (w && requested != 1) return 2;
    return 1;
}

PCX_HIDDEN bool tt_plan_has_variant(const TTPlan &p, const TTImages &up, int variant) {
    return tt_auto_variant(p, up, variant) >= 0;
}

// ---- host-built tables ----
PCX_HIDDEN std::vector<double> tt_pack_last_core(const TTPlan &p, const double *cores) {
    const int d = p.dims.d;
    const size_t nl = (size_t)p.dims.n[d - 1];
    std::vector<double> padded((size_t)p.last_rows * nl, 0.0);
    for (size_t a = 0; a < (size_t)p.ranks[d - 1]; ++a)
        for (size_t j = 0; j < nl; ++j) padded[a * nl + j] = cores[p.coff[d - 1] + a * nl + j];
    return padded;
}

PCX_HIDDEN std::vector<double> tt_pack_d4_image(const TTPlan &p, const double *cores) {
    const int d = p.dims.d, RA = p.d4RA, NMP = RA == 3 ? 4 : RA;
    const int *n = p.dims.n;
    std::vector<double> img((size_t)p.d4plan.total, 0.0);
    auto G = [&](int k, int a, int j, int b) -> double {
        if (a >= p.ranks[k] || b >= p.ranks[k + 1] || j >= n[k]) return 0.0;
        return cores[p.coff[k] + ((long)a * n[k] + j) * p.ranks[k + 1] + b];
    };
    for (int k = 0; k < d - 1; ++k) {
        double *dst = img.data() + p.d4plan.lds_off[k];
        if (k == 0) {
            const int ks0 = (n[0] + 3) / 4;
            for (int s0 = 0; s0 < ks0; ++s0)
                for (int k4 = 0; k4 < 4; ++k4)
                    for (int i = 0; i < 4; ++i)
                        for (int m = 0; m < RA; ++m)
                            dst[s0 * 16 * NMP + (k4 * 4 + i) * NMP + m] = G(0, 0, 4 * s0 + k4, 4 * m + i);
        } else {
            for (int j = 0; j < n[k]; ++j)
                for (int c = 0; c < RA; ++c)
                    for (int k4 = 0; k4 < 4; ++k4)
                        for (int i = 0; i < 4; ++i)
                            for (int m = 0; m < RA; ++m)
                                dst[(j * RA + c) * 16 * NMP + (k4 * 4 + i) * NMP + m] = G(k, 4 * c + k4, j, 4 * m + i);
        }
    }
    double *dst = img.data() + p.d4plan.lds_off[d - 1];
    const int nl = n[d - 1];
    for (int a = 0; a < 4 * RA; ++a)
        for (int j = 0; j < nl; ++j) dst[a * nl + j] = G(d - 1, a, j, 0);
    return img;
}

PCX_HIDDEN std::vector<double> tt_pack_lpp_image(const TTPlan &p, const double *cores) {
    std::vector<double> img((size_t)p.core_total + 64, 0.0);
    for (int k = 0; k < p.dims.d; ++k) {
        const int rl = p.ranks[k], rr = p.ranks[k + 1], nk = p.dims.n[k];
        double *dst = img.data() + p.coff[k];
        const double *G = cores + p.coff[k];
        for (int b = 0; b < rr; ++b)
            for (int a = 0; a < rl; ++a)
                for (int j = 0; j < nk; ++j) dst[((size_t)b * rl + a) * nk + j] = G[((size_t)a * nk + j) * rr + b];
    }
    return img;
}

PCX_HIDDEN std::vector<TTLppDim> tt_lpp_table(const TTPlan &p) {
    std::vector<TTLppDim> tab((size_t)p.dims.d);
    for (int k = 0; k < p.dims.d; ++k)
        tab[k] = TTLppDim{(int)p.coff[k], p.ranks[k], p.ranks[k + 1], p.dims.n[k], p.dims.col[k], 0, p.dims.lo[k], p.dims.scale[k]};
    return tab;
}
