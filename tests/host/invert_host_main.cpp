// invert_host_main.cpp -- the host compilation pass of inv_block (csrc/invert_kernels.h) as a stand-alone program, for
// tests/test_invert_host_pass.py: built with the address and undefined-behaviour sanitizers on the host side, it runs
// the solver's own source on a CPU with its LDS tile on the heap, sized exactly as the kernel's __shared__ array of the
// fibre's class and filled with NaN bit patterns before every block of 64 rows.  An index past the tile stops the
// program, a read of a slot the block did not write shows in the results.  No HIP call is made: the program needs no GPU.
//
//   invert_host_main <in> <out>
//
// <in>:  int32 cases, then per case: int32 n, rows; double lo, hi; nodes[n], weights[n], values[rows n], targets[rows]
// <out>: per case: double x[rows]; int32 status[rows], iterations[rows]
#include "invert_kernels.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

template <int NP>
static void run_rows(const InvArgs &a) {
    const size_t len = INV_TILE(NP);                                  // the kernel's __shared__ array
    double *tile = (double *)malloc(len * sizeof(double));
    if (!tile) abort();
    for (long block = 0; block * 64 < a.rows; ++block) {
        memset(tile, 0xff, len * sizeof(double));
        inv_block<NP>(a, block, tile);
    }
    free(tile);
}

template <typename T>
static std::vector<T> take(FILE *f, size_t count) {
    std::vector<T> v(count);
    if (count && fread(v.data(), sizeof(T), count, f) != count) {
        fprintf(stderr, "invert_host_main: short input\n");
        exit(2);
    }
    return v;
}

template <typename T>
static void put(FILE *f, const std::vector<T> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
        fprintf(stderr, "invert_host_main: short output\n");
        exit(2);
    }
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: invert_host_main <in> <out>\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "invert_host_main: cannot open the files\n");
        return 2;
    }
    const int cases = take<int32_t>(in, 1)[0];
    for (int c = 0; c < cases; ++c) {
        const std::vector<int32_t> head = take<int32_t>(in, 2);
        const int n = head[0];
        const long rows = head[1];
        if (n < 1 || n > PCX_INV_MAX_N || rows < 0) {
            fprintf(stderr, "invert_host_main: case %d: n=%d rows=%ld\n", c, n, rows);
            return 2;
        }
        const std::vector<double> dom = take<double>(in, 2);
        const std::vector<double> nodes = take<double>(in, n), wts = take<double>(in, n);
        const std::vector<double> vals = take<double>(in, (size_t)rows * n), targets = take<double>(in, rows);
        std::vector<double> x(rows);
        std::vector<int32_t> status(rows), iters(rows);
        InvArgs a{};
        a.n = n; a.rows = rows; a.lo = dom[0]; a.hi = dom[1];
        a.nodes = nodes.data(); a.wts = wts.data(); a.vals = vals.data(); a.targets = targets.data();
        a.x = x.data(); a.status = status.data(); a.iters = iters.data();
        if (n <= 16) run_rows<16>(a);                                 // the class rule of INV_DISPATCH
        else if (n <= 32) run_rows<32>(a);
        else run_rows<64>(a);
        put(out, x);
        put(out, status);
        put(out, iters);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
