// calc_host_main.cpp -- the host compilation pass of calc_row (csrc/calculus_kernels.h) as a stand-alone program, for
// tests/test_calculus_host_pass.py: built with the address and undefined-behaviour sanitizers on the host side, it runs
// the solver's own source on a CPU with its "LDS" on the heap, sized exactly as the kernels size it and filled with NaN
// bit patterns before every row.  An index past the buffer stops the program, a read of a slot the row did not write
// shows in the results.  No HIP call is made: the program needs no GPU.
//
//   calc_host_main <in> <out>
//
// <in>:  int32 cases, then per case: int32 n, rows, mode, 0; double lo, hi; nodes[n], weights[n], diff[n n],
//        values[rows n]
// <out>: per case: int32 counts[rows]; mode 0: double roots[rows max(n - 1, 1)]; modes 1, 2: double val[rows], loc[rows]
#include "calculus_kernels.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

template <int MP>
static void run_rows(const CalcArgs &a, long rows) {
    const size_t len = (size_t)MP * (MP + 1) + PCX_CALC_EXTRA;        // the kernels' __shared__ array
    double *lds = (double *)malloc(len * sizeof(double));
    if (!lds) abort();
    for (long r = 0; r < rows; ++r) {
        memset(lds, 0xff, len * sizeof(double));
        calc_row<MP + 1>(a, r, lds, MP);
    }
    free(lds);
}

template <typename T>
static std::vector<T> take(FILE *f, size_t count) {
    std::vector<T> v(count);
    if (count && fread(v.data(), sizeof(T), count, f) != count) {
        fprintf(stderr, "calc_host_main: short input\n");
        exit(2);
    }
    return v;
}

template <typename T>
static void put(FILE *f, const std::vector<T> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
        fprintf(stderr, "calc_host_main: short output\n");
        exit(2);
    }
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: calc_host_main <in> <out>\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "calc_host_main: cannot open the files\n");
        return 2;
    }
    const int cases = take<int32_t>(in, 1)[0];
    for (int c = 0; c < cases; ++c) {
        const std::vector<int32_t> head = take<int32_t>(in, 4);
        const int n = head[0], mode = head[2];
        const long rows = head[1];
        if (n < 1 || n > PCX_CALC_MAX_N || rows < 0 || mode < 0 || mode > 2) {
            fprintf(stderr, "calc_host_main: case %d: n=%d rows=%ld mode=%d\n", c, n, rows, mode);
            return 2;
        }
        const std::vector<double> dom = take<double>(in, 2);
        const std::vector<double> nodes = take<double>(in, n), wts = take<double>(in, n);
        const std::vector<double> diff = take<double>(in, (size_t)n * n), vals = take<double>(in, (size_t)rows * n);
        const int W = n - 1 > 1 ? n - 1 : 1;
        std::vector<int32_t> counts(rows);
        std::vector<double> roots(mode == 0 ? (size_t)rows * W : 0), val(mode != 0 ? rows : 0), loc(mode != 0 ? rows : 0);
        CalcArgs a{};
        a.n = n; a.mode = mode; a.W = W; a.lo = dom[0]; a.hi = dom[1];
        a.nodes = nodes.data(); a.wts = wts.data(); a.diff = diff.data(); a.vals = vals.data();
        a.counts = counts.data();
        a.roots = mode == 0 ? roots.data() : nullptr;                 // only the mode's own outputs exist
        a.val = mode != 0 ? val.data() : nullptr;
        a.loc = mode != 0 ? loc.data() : nullptr;
        const int m = n - 1;                                          // the class rule of calc_launch
        if (m <= 16) run_rows<16>(a, rows);
        else if (m <= 32) run_rows<32>(a, rows);
        else run_rows<64>(a, rows);
        put(out, counts);
        put(out, roots);
        put(out, val);
        put(out, loc);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
