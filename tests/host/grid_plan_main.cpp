// grid_plan_main.cpp -- prints what the grid planner (csrc/grid_plan.h) decides, one JSON line per case, without a GPU.
//
//   grid_plan_main <cases.txt>
//
// A case is one line of blank-separated tokens, doubles as C hex floats:
//   G d  n_0 .. n_{d-1}  m_0 .. m_{d-1}  nodes_cat (sum n)  weights_cat (sum n)  axes_cat (sum m)
//   T d  m_0 .. m_{d-1}  ranks_0 .. ranks_d
// Built by tests/test_eval_grid_host.py under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "grid_plan.h"

static void print_grid(std::istringstream &in) {
    int d = 0;
    in >> d;
    std::vector<int32_t> n(d > 0 ? d : 0), m(d > 0 ? d : 0);
    long sn = 0, sm = 0;
    for (int k = 0; k < d; ++k) { in >> n[k]; sn += n[k] > 0 ? n[k] : 0; }
    for (int k = 0; k < d; ++k) { in >> m[k]; sm += m[k] > 0 ? m[k] : 0; }
    std::vector<double> nodes(sn), wts(sn), axes(sm);
    std::string tok;
    for (double &v : nodes) { in >> tok; v = strtod(tok.c_str(), nullptr); }
    for (double &v : wts) { in >> tok; v = strtod(tok.c_str(), nullptr); }
    for (double &v : axes) { in >> tok; v = strtod(tok.c_str(), nullptr); }
    GridPlan gp;
    char err[256] = "";
    // one spare element each: a NULL data() of an empty vector is not what an empty axis is about
    nodes.push_back(0.0); wts.push_back(0.0); axes.push_back(0.0);
    const int rc = grid_make_plan(d, n.data(), nodes.data(), wts.data(), m.data(), axes.data(), gp, err, sizeof err);
    printf("{\"rc\": %d, \"error\": \"%s\"", rc, err);
    if (rc == PCX_OK) {
        printf(", \"max_intermediate\": %ld, \"passes\": [", gp.max_intermediate);
        for (size_t p = 0; p < gp.passes.size(); ++p) {
            const GridPass &ps = gp.passes[p];
            printf("%s[%d, %ld, %d, %ld, %d, %ld, %ld]", p ? ", " : "", ps.dim, ps.outer, ps.n, ps.inner, ps.m, ps.w_off, ps.out_count);
        }
        printf("], \"hot\": [");
        for (size_t i = 0; i < gp.hot.size(); ++i) printf("%s%d", i ? ", " : "", gp.hot[i]);
        printf("], \"W\": [");
        for (size_t i = 0; i < gp.W.size(); ++i) printf("%s\"%a\"", i ? ", " : "", gp.W[i]);
        printf("]");
    }
    printf("}\n");
}

static void print_tt(std::istringstream &in) {
    int d = 0;
    in >> d;
    std::vector<int32_t> m(d > 0 ? d : 0), r(d > 0 ? d + 1 : 1);
    for (int32_t &v : m) in >> v;
    for (int32_t &v : r) in >> v;
    TTGridPlan tp;
    char err[256] = "";
    const int rc = tt_grid_make_plan(d, m.data(), r.data(), tp, err, sizeof err);
    printf("{\"rc\": %d, \"error\": \"%s\"", rc, err);
    if (rc == PCX_OK) {
        printf(", \"from_right\": %d, \"max_intermediate\": %lld, \"total\": %lld, \"steps\": [", (int)tp.from_right,
               (long long)tp.max_intermediate, (long long)tp.total);
        for (size_t s = 0; s < tp.steps.size(); ++s) {
            const TTGridStep &st = tp.steps[s];
            printf("%s[%d, %d, %lld, %d, %lld, %lld]", s ? ", " : "", st.core, (int)st.w_is_core, (long long)st.m, st.n,
                   (long long)st.inner, (long long)st.out_count);
        }
        printf("]");
    }
    printf("}\n");
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: grid_plan_main <cases.txt>\n");
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
        if (kind == "G") print_grid(in);
        else if (kind == "T") print_tt(in);
        else {
            fprintf(stderr, "unknown case kind '%s'\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
