// bary_plan_main.cpp -- the launch planner of the barycentric handle (csrc/bary_plan.h, csrc/pcx_bary_plan.hip) as a
// stand-alone program, for tests/test_bary_plan_host.py: built with the address and undefined-behaviour sanitizers on the
// host side.  No HIP call is made: the program needs no GPU.  It is also how a plan is printed on any machine:
//
//   echo "5 11 11 11 11 11  1 1 1 1 1" | bary_plan_main [--tables] [--kfold=0] [--kfold-eff=PERCENT] [--kfold-straddle=0]
//
// Input (a file named on the command line, else stdin), one case per line:
//   d n_0 .. n_{d-1}  seed tail sq grid grid_prod        (the switches as PCX_BARY_SEED, _TAIL, _SQ, _GRID, _GRID_PROD set them)
// --kfold=0 plans every case of the run as PCX_BARY_KFOLD=0 does (no k-fold form); without it the default, 1.
// --kfold-eff=PERCENT and --kfold-straddle=0 do the same for PCX_BARY_KFOLD_EFF and PCX_BARY_KFOLD_STRADDLE
// (BaryEnv::kfold_eff, ::kfold_straddle); without them the defaults, 0 and 1.
// The nodes are Chebyshev points of the first kind on [-1, 1].  Output, one JSON object per case: "rc" and "error" of
// bary_make_plan; every field of BaryLaunchPlan ("plan"); what the info entry points report of it ("kernel_info",
// "grid_info", "tail_info" = entries 1 .. 3, "set_kernel" = variants 2 .. 5), computed by the functions those entry points
// call; per table its length and 64-bit FNV-1a hash ("tables"), with --tables its entries as well.
#include "pcx_internal.h"
#include "bary_plan.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

PCX_HIDDEN char *pcx_err_buf() noexcept {         // the library keeps it in pcx_core.hip
    static thread_local char buf[PCX_ERR_LEN];
    return buf;
}

static bool g_dump = false;
static bool g_kfold = true;
static bool g_kfold_straddle = true;
static int g_kfold_eff = 0;

template <typename T>
static void put_table(const char *name, const std::vector<T> &v, bool &first) {
    uint64_t hsh = 1469598103934665603ull;
    const unsigned char *b = (const unsigned char *)v.data();
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) hsh = (hsh ^ b[i]) * 1099511628211ull;
    printf("%s\"%s\": {\"len\": %zu, \"fnv\": \"%016" PRIx64 "\"", first ? "" : ", ", name, v.size(), hsh);
    if (g_dump) {
        printf(", \"data\": [");
        for (size_t i = 0; i < v.size(); ++i) {
            if (i) printf(",");
            if (sizeof(T) == sizeof(double)) printf("%.17g", (double)v[i]);
            else printf("%u", (unsigned)v[i]);
        }
        printf("]");
    }
    printf("}");
    first = false;
}

static void put_ints(const char *name, const int32_t *v, int count) {
    printf(", \"%s\": [", name);
    for (int i = 0; i < count; ++i) printf("%s%d", i ? ", " : "", v[i]);
    printf("]");
}

static void put_plan(const BaryLaunchPlan &lp, int d) {
#define F(x) printf(", \"" #x "\": %ld", (long)lp.x)
    printf(", \"plan\": {\"mfma_ok\": %d", (int)lp.mfma_ok);
    F(seed); F(plan.split); F(plan.M); F(plan.K); F(plan.MT); F(plan.KS); F(plan.R); F(plan.tail_base); F(plan.rows);
    F(nt); F(wide); F(tail_mode); F(grid_ok); F(kfold_ok); F(grid_prod); F(g0_ok); F(g0_tps); F(g0_nf); F(lpp); F(mfma4_ok);
    F(small_nlp); F(small_preferred); F(sq_nl); F(sq_preferred);
    if (lp.grid_ok) {
        F(gp.RA); F(gp.gbs); F(gp.nA); F(gp.nB); F(gp.TA); F(gp.TB); F(gp.rowA); F(gp.rowB); F(gp.nouter); F(gp.no1); F(gp.rowo0);
        F(gp.rowo1); F(gp.nchunks); F(gp.hrows); F(gp.trows); F(gp.af); F(gp.wpb); F(gp.MT);
    }
    if (lp.kfold_ok) {
        F(kf.dim[0]); F(kf.dim[1]); F(kf.dim[2]); F(kf.stride[0]); F(kf.stride[1]); F(kf.stride[2]); F(kf.n0); F(kf.n1); F(kf.n2);
        F(kf.MT); F(kf.KS2); F(kf.trows); F(kf.str); F(kf.P); F(kf.nbody);
    }
#undef F
    if (lp.small_nlp) {
        printf(", \"small_scale\": [");
        for (int k = 0; k < d; ++k) printf("%s%.17g", k ? ", " : "", lp.small_scale.s[k]);
        printf("]");
    }
    printf("}");
}

int main(int argc, char **argv) {
    FILE *in = stdin;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--tables")) g_dump = true;
        else if (!strncmp(argv[i], "--kfold=", 8)) g_kfold = argv[i][8] != '0';
        else if (!strncmp(argv[i], "--kfold-eff=", 12)) g_kfold_eff = atoi(argv[i] + 12);
        else if (!strncmp(argv[i], "--kfold-straddle=", 17)) g_kfold_straddle = argv[i][17] != '0';
        else if (!(in = fopen(argv[i], "r"))) { fprintf(stderr, "bary_plan_main: cannot open %s\n", argv[i]); return 2; }
    }
    const double pi = 3.14159265358979323846;
    int d;
    while (fscanf(in, "%d", &d) == 1) {
        if (d < 1 || d > PCX_MAX_DIMS) { fprintf(stderr, "bary_plan_main: d=%d\n", d); return 2; }
        BaryDims dm{};
        long total = 1;
        int sum_n = 0;
        for (int k = 0; k < PCX_MAX_DIMS; ++k) {
            dm.n[k] = 1;
            if (k >= d) continue;
            if (fscanf(in, "%d", &dm.n[k]) != 1 || dm.n[k] < 1 || dm.n[k] > 4096) { fprintf(stderr, "bary_plan_main: bad node count\n"); return 2; }
            dm.off[k] = sum_n;
            sum_n += dm.n[k];
            total *= dm.n[k];
        }
        dm.d = d;
        dm.sum_n = sum_n;
        int sw[5];
        for (int &v : sw)
            if (fscanf(in, "%d", &v) != 1) { fprintf(stderr, "bary_plan_main: five switches per case\n"); return 2; }
        BaryEnv env;
        env.seed = sw[0] != 0; env.tail_mode = sw[1]; env.sq_auto = sw[2] != 0; env.grid = sw[3]; env.grid_prod = sw[4] != 0;
        env.kfold = g_kfold; env.kfold_eff = g_kfold_eff; env.kfold_straddle = g_kfold_straddle;
        std::vector<double> nodes((size_t)sum_n);            // exactly sum_n doubles: a read past them is the sanitizer's
        for (int k = 0; k < d; ++k)
            for (int j = 0; j < dm.n[k]; ++j) nodes[dm.off[k] + j] = -std::cos((2 * j + 1) * pi / (2.0 * dm.n[k]));

        BaryLaunchPlan lp;
        const int rc = bary_make_plan(dm, total, nodes.data(), env, lp);
        printf("{\"rc\": %d", rc);
        if (rc != PCX_OK) {
            printf(", \"error\": \"%s\"}\n", pcx_err_buf());
            continue;
        }
        put_plan(lp, d);
        int32_t ki[6], gi[4], ti[6], sk[4];
        bary_plan_kernel_info(lp, dm, ki);
        bary_plan_grid_info(lp, gi);
        bary_plan_tail_info(lp, ti);
        for (int v = 2; v <= 5; ++v) sk[v - 2] = bary_plan_has_variant(lp, v);
        put_ints("kernel_info", ki, 6);
        put_ints("grid_info", gi, 4);
        put_ints("tail_info", ti + 1, 3);
        put_ints("set_kernel", sk, 4);
        printf(", \"tables\": {");
        bool first = true;
        if (lp.small_nlp) put_table("snodes", bary_scaled_nodes(dm, nodes.data(), false), first);
        if (lp.grid_ok || lp.kfold_ok) put_table("gsnodes", bary_scaled_nodes(dm, nodes.data(), true), first);
        if (lp.mfma_ok) {
            const std::vector<unsigned> rowcode = bary_row_codes(dm, lp.plan, 0);
            put_table("rowcode", rowcode, first);
            put_table("kcode", bary_k_codes(dm, lp.plan, 0), first);
            if (lp.wide) {
                put_table("rowcode_hi", bary_row_codes(dm, lp.plan, 1), first);
                put_table("kcode_hi", bary_k_codes(dm, lp.plan, 1), first);
            }
            if (bary_plan_row_offsets(lp)) {
                put_table("rowoff1", bary_row_offsets(rowcode, 1), first);
                put_table("rowoff2", bary_row_offsets(rowcode, 2), first);
            }
            if (lp.g0_ok) put_table("rowcode_g0", bary_slab_row_codes(dm, lp), first);
        }
        printf("}}\n");
    }
    return 0;
}
