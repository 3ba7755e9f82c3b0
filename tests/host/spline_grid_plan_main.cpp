// spline_grid_plan_main.cpp -- prints what the planner of a piecewise grid evaluation (csrc/spline_grid_plan.h) decides,
// one JSON line per case, without a GPU.
//
//   spline_grid_plan_main <cases.txt>
//
// A case is one line of blank-separated tokens, doubles as C hex floats (or "nan"):
//   S d  nknots_0 .. nknots_{d-1}  m_0 .. m_{d-1}  knots_cat (sum nknots)  axes_cat (sum m)
// Built by tests/test_piecewise_grid_host.py under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "spline_grid_plan.h"

template <typename T>
static void print_ints(const char *name, const std::vector<T> &v) {
    printf(", \"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%lld", i ? ", " : "", (long long)v[i]);
    printf("]");
}

static void print_case(std::istringstream &in) {
    int d = 0;
    in >> d;
    std::vector<int32_t> nk(d > 0 ? d : 0), m(d > 0 ? d : 0);
    long sk = 0, sm = 0;
    for (int k = 0; k < d; ++k) { in >> nk[k]; sk += nk[k] > 0 ? nk[k] : 0; }
    for (int k = 0; k < d; ++k) { in >> m[k]; sm += m[k] > 0 ? m[k] : 0; }
    std::vector<double> knots(sk), axes(sm);
    std::string tok;
    for (double &v : knots) { in >> tok; v = strtod(tok.c_str(), nullptr); }
    for (double &v : axes) { in >> tok; v = strtod(tok.c_str(), nullptr); }
    // one spare element each: a NULL data() of an empty vector is not what an empty axis is about
    knots.push_back(0.0); axes.push_back(0.0);
    SplineGridPlan sp;
    char err[256] = "";
    const int rc = spline_grid_make_plan(d, nk.data(), knots.data(), m.data(), axes.data(), 1L << 40, sp, err, sizeof err);
    printf("{\"rc\": %d, \"error\": \"%s\"", rc, err);
    if (rc == PCX_OK) {
        printf(", \"total\": %ld, \"n_pieces\": %ld", sp.total, sp.n_pieces);
        print_ints("axis_off", sp.axis_off);
        print_ints("cnt_off", sp.cnt_off);
        print_ints("interval", sp.interval);
        print_ints("rank", sp.rank);
        print_ints("count", sp.count);
        print_ints("list_off", sp.list_off);
        print_ints("list", sp.list);
        print_ints("block_off", sp.block_off);
        printf(", \"blocks\": [");
        for (size_t b = 0; b < sp.blocks.size(); ++b) {
            const SplineGridBlock &blk = sp.blocks[b];
            printf("%s[%ld, %ld, %ld, %ld", b ? ", " : "", blk.piece, blk.offset, blk.count, blk.axes_off);
            for (int k = 0; k < d; ++k) printf(", %d", blk.m[k]);
            printf("]");
        }
        printf("], \"sub_axes\": [");
        for (size_t i = 0; i < sp.sub_axes.size(); ++i) printf("%s\"%a\"", i ? ", " : "", sp.sub_axes[i]);
        printf("]");
    }
    printf("}\n");
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: spline_grid_plan_main <cases.txt>\n");
        return 2;
    }
    std::ifstream fh(argv[1]);
    if (!fh) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    std::string line;
    while (std::getline(fh, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string kind;
        in >> kind;
        if (kind == "S") print_case(in);
        else {
            fprintf(stderr, "unknown case kind '%s'\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
