// invert_kernels.h -- batched inversion of 1-D Chebyshev interpolants: the x at which a fibre equals its row's target
// (gfx950).
//
// The device half of invert_batch().  A fibre is the n <= 64 values of a 1-D interpolant p at its ascending type-I
// nodes; the row's target t turns it into g = p - t.  On the knots s_0 = lo, s_1 .. s_n = the nodes, s_(n+1) = hi:
//
//   g_0 = p(lo) - t, g_i = v_(i-1) - t, g_(n+1) = p(hi) - t; p at the two ends by the barycentric formula, a sequential
//   sum over j = 0 .. n-1 with the project's within-1e-14-of-a-node rule (as calc_row evaluates its candidates)
//   segment i (0 <= i <= n) brackets when g_i == 0 or g_i and g_(i+1) have opposite signs (the sign of g_i g_(i+1),
//   taken from the two signs so that a product that underflows still counts); g_(n+1) == 0 counts as one more
//   status = the number of bracketing segments: 0 -> x = NaN; > 1 -> x is the lowest; -1 and NaN when the fibre or the
//   target is not finite, or when the iteration cap is reached
//   x = s_i exactly when g_i == 0, else the root inside the lowest bracketing segment [a, b]:
//
//       every step evaluates g once, at a point strictly inside (a, b), and replaces the end of the same sign, so the
//       root never leaves the bracket.  The point is the Illinois secant point (false position; an end that stays twice
//       has its weight halved), kept at least tol = 4 eps max(|a|, |b|) away from both ends, which pulls the far end in
//       once the secant has converged; the midpoint instead when b - a <= 2 tol or when two steps in a row failed to
//       halve the bracket.  Stop at g(x) == 0, or when a and b are adjacent doubles (x = the end with the smaller |g|,
//       a on a tie), or at INV_MAX_ITERS evaluations (status -1).  No loop without a fixed bound.
//
//       Adjacent doubles alone would be a stop relative to |x|: a root at or near 0 inside a domain that contains 0
//       would ask for a bracket of 1e-33 and less -- some 1100 halvings down to the subnormals -- around a g that, x - x_j
//       being rounded to the spacing of doubles near the nodes, is a step function of x at about eps max(|lo|, |hi|)
//       there.  So the stop and tol carry a floor tied to the fibre's interval, flo = 2^-10 eps max(|lo|, |hi|)
//       (2.2e-19 on [-1, 1]): the bracket also stops at b - a <= flo, and tol is at least flo.  A root with
//       |x| >= 2^-9 max(|lo|, |hi|) still ends at adjacent doubles, the spacing there being above the floor; a smaller
//       one is returned to within flo, far below what g can resolve.
//
//       A push that does not cross the root (the new point replaces the end it was pushed from) doubles the next
//       push, tol 2^creep, until one crosses or is not needed: where g is tiny at one end and large at the other -- a
//       target one ulp off a node's value meets the jump of the within-1e-14 rule there -- the secant point sits on
//       that end for good, and equal pushes would leave all the work to the forced midpoints.
//
//       The cap cannot be reached on a finite fibre whose evaluations stay finite: any three consecutive steps at least
//       halve the bracket (the third is a midpoint when the first two did not), and from b - a <= 2 max(|lo|, |hi|)
//       down to flo there are 1 + 10 + 52 = 63 halvings, 189 steps < INV_MAX_ITERS = 192.
//
// One LANE per fibre, not one wave: a fibre costs a few dozen O(n) barycentric sums, which a wave per fibre would spend
// with 63 lanes idle.  A workgroup is one wave of 64 fibres.  The fibres sit in an LDS tile laid out [j][lane] with a
// lane stride of INV_LS = 65 doubles: in the solve lane l reads element j at (j 65 + l), consecutive 8-byte words,
// which ds_read_b64 serves without a bank conflict, and the staging write -- consecutive lanes hold consecutive j of
// one row, coalesced from HBM -- lands at stride 65 doubles, conflict-free as well (stride 64 would put a whole wave on
// one bank).  Nodes and weights follow the tile and are read by every lane at the same address (a broadcast).  NP, the
// fibre-length class (16, 32, 64), sizes the tile: 8.6, 17.1, 34.3 KiB per workgroup, so at least four waves share a
// CU at the longest fibres.  Lanes whose fibre is done are masked off; the wave runs to its slowest lane's iteration
// count, and every iteration has the same shape (one barycentric sum, one bracket update), so divergence costs
// iterations, not code paths.
//
// No atomics: a row's result depends on its own fibre and target only, bit for bit, whatever the batch size or the
// row's position in it.
//
// The routine is written once for both compilation passes, as calc_row is: on the device the INV_LANES loops are the 64
// lanes and INV_SYNC is a workgroup barrier; on the host they are plain loops over a tile on the heap, which lets the
// arithmetic be checked on a CPU.
#pragma once

#include "pcx_common.h"
#include "spline_calc_kernels.h"     // SplineCalcPiece: the spline entries solve every piece along the dimension

#include <float.h>
#include <math.h>

#pragma clang fp contract(off)     // no fused multiply-add: the same roundings as the NumPy statements restated here

#define PCX_INV_MAX_N 64           // fibre length limit, as PCX_CALC_MAX_N
#define INV_MAX_ITERS 192          // evaluations of g inside the bracket; reaching it gives status -1 (see above)
#define INV_FLOOR 0x1p-10          // the bracket also stops at INV_FLOOR eps max(|lo|, |hi|): see above
#define INV_LS 65                  // lane stride of the tile, in doubles
#define INV_TILE(NP) ((NP) * INV_LS + 2 * (NP))    // doubles: the tile, then nodes and weights

#define INV_FN __host__ __device__ inline
#if defined(__HIP_DEVICE_COMPILE__)
#define INV_LANES(l) for (int l = (int)threadIdx.x, l##_once = 1; l##_once; l##_once = 0)
#define INV_SYNC() __syncthreads()
#else
#define INV_LANES(l) for (int l = 0; l < 64; ++l)
#define INV_SYNC() ((void)0)
#endif

struct InvArgs {
    int n;                    // fibre length, 1 .. PCX_INV_MAX_N
    long rows;                // fibres of this launch
    double lo, hi;            // the fibre's physical interval
    const double *nodes;      // n ascending nodes
    const double *wts;        // n barycentric weights
    const double *vals;       // rows x n fibre values
    const double *targets;    // rows
    double *x;                // rows
    int32_t *status;          // rows
    int32_t *iters;           // rows, or NULL: evaluations of g inside the bracket (the host pass reports them)
};

// p(x) of the fibre v[0], v[INV_LS], ... : the first node within 1e-14 gives its value, else num / den
INV_FN double inv_eval(int n, const double *nd, const double *wt, const double *v, double x) {
    int exact = -1;
    double num = 0.0, den = 0.0;
    for (int j = 0; j < n; ++j) {
        const double dx = x - nd[j];
        if (fabs(dx) < 1e-14) {
            if (exact < 0) exact = j;
        } else {
            const double t = wt[j] / dx;
            num += t * v[(size_t)j * INV_LS];
            den += t;
        }
    }
    return exact >= 0 ? v[(size_t)exact * INV_LS] : num / den;
}

// One fibre against its target -> status; x and the evaluations spent inside the bracket.
INV_FN int inv_solve(int n, double lo, double hi, const double *nd, const double *wt, const double *v, double t,
                     double &xout, int &iters) {
    xout = NAN;
    iters = 0;
    bool finite = fabs(t) <= DBL_MAX;
    for (int j = 0; j < n; ++j) finite = finite && fabs(v[(size_t)j * INV_LS]) <= DBL_MAX;
    if (!finite) return -1;
    int count = 0;
    bool exact = false;
    double a = 0.0, b = 0.0, ga = 0.0, gb = 0.0;
    double sp = lo, gp = inv_eval(n, nd, wt, v, lo) - t;      // s_i, g_i
    for (int i = 0; i <= n; ++i) {                              // segment i: [s_i, s_(i+1)]
        const double sn = i < n ? nd[i] : hi;
        const double gn = i < n ? v[(size_t)i * INV_LS] - t : inv_eval(n, nd, wt, v, hi) - t;
        const bool zero = gp == 0.0;
        if (zero || (gp < 0.0 && gn > 0.0) || (gp > 0.0 && gn < 0.0)) {
            if (count == 0) { a = sp; b = sn; ga = gp; gb = gn; exact = zero; }
            ++count;
        }
        sp = sn;
        gp = gn;
    }
    if (gp == 0.0) {                                            // g_(n+1) == 0: the solution at hi
        if (count == 0) { a = sp; exact = true; }
        ++count;
    }
    if (count == 0) return 0;
    if (exact) { xout = a; return count; }
    const double flo = INV_FLOOR * DBL_EPSILON * fmax(fabs(lo), fabs(hi));
    double fa = ga, fb = gb;                                    // the Illinois weights of the two ends
    int side = 0, slow = 0, creep = 0;
    for (int it = 0; it < INV_MAX_ITERS; ++it) {
        const double w = b - a;
        const double m = a + 0.5 * w;
        if (!(a < m && m < b) || !(w > flo)) {                  // adjacent doubles, or the floor
            xout = fabs(ga) <= fabs(gb) ? a : b;
            return count;
        }
        const double tol = ldexp(fmax(4.0 * DBL_EPSILON * fmax(fabs(a), fabs(b)), flo), creep);
        double x = b - fb * (w / (fb - fa));
        int pushed = 0;                                         // -1 / +1: x was pushed tol away from a / b
        if (slow >= 2 || !(w > 2.0 * tol)) {
            x = m;
            slow = 0;
        } else {
            if (!(x > a + tol)) { x = a + tol; pushed = -1; }
            else if (!(x < b - tol)) { x = b - tol; pushed = 1; }
            if (!(a < x && x < b)) { x = m; pushed = 0; }
        }
        const double gx = inv_eval(n, nd, wt, v, x) - t;
        ++iters;
        if (gx == 0.0) { xout = x; return count; }
        const bool left = (gx < 0.0) == (ga < 0.0);
        if (left) {
            a = x; ga = gx; fa = gx;
            if (side == -1) fb = fb * 0.5;
            side = -1;
        } else {
            b = x; gb = gx; fb = gx;
            if (side == 1) fa = fa * 0.5;
            side = 1;
        }
        if (pushed != 0) creep = (left ? -1 : 1) == pushed ? creep + 1 : 0;     // the push did not cross the root: double it
        slow = (b - a) > 0.5 * w ? slow + 1 : 0;
    }
    xout = NAN;
    return -1;
}

// The 64 fibres block * 64 .. of a launch: stage them into the tile, solve a lane each.  tile: INV_TILE(NP) doubles.
template <int NP>
INV_FN void inv_block(const InvArgs &a, long block, double *tile) {
    const int n = a.n;
    double *nd = tile + NP * INV_LS, *wt = nd + NP;
    const long r0 = block * 64;
    const long live = a.rows - r0 < 64 ? a.rows - r0 : 64;      // rows of this block
    const double *src = a.vals + (size_t)r0 * n;
    INV_LANES(l) {
        for (int j = l; j < n; j += 64) {
            nd[j] = a.nodes[j];
            wt[j] = a.wts[j];
        }
        for (long e = l; e < live * n; e += 64) {               // element e = (row e / n, node e % n) -> [j][row]
            const int r = (int)(e / n), j = (int)(e - (long)r * n);
            tile[(size_t)j * INV_LS + r] = src[e];
        }
    }
    INV_SYNC();
    INV_LANES(l) {
        if (l < live) {
            double x;
            int iters;
            const int st = inv_solve(n, a.lo, a.hi, nd, wt, tile + l, a.targets[r0 + l], x, iters);
            a.x[r0 + l] = x;
            a.status[r0 + l] = st;
            if (a.iters) a.iters[r0 + l] = iters;
        }
    }
}

#if defined(__HIPCC__)
template <int NP>
__global__ __launch_bounds__(64) void k_cheb1d_invert(InvArgs a) {
    __shared__ double tile[INV_TILE(NP)];
    inv_block<NP>(a, (long)blockIdx.x, tile);
}

// v[r, j] - t[r] in place, one rounding: the fibres of roots(level=) before the eigenvalue solver
__global__ __launch_bounds__(256) void k_calc_level(double *__restrict__ vals, const double *__restrict__ targets, long rows,
                                                    int n) {
    const long total = rows * n;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x)
        vals[idx] = vals[idx] - targets[idx / n];
}

// The spline's forms (piece-major layouts of spline_calc_kernels.h; grid.y = piece j).  Every (row, piece) fibre takes
// its row's level or target.
__global__ __launch_bounds__(256) void k_spline_calc_level(const SplineCalcPiece *__restrict__ tab, double *__restrict__ vals,
                                                           const double *__restrict__ targets, long rows) {
    const SplineCalcPiece pc = tab[blockIdx.y];
    const long total = rows * pc.n;
    double *v = vals + rows * pc.voff;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x)
        v[idx] = v[idx] - targets[idx / pc.n];
}

// piece j's results at [j rows + r]
template <int NP>
__global__ __launch_bounds__(64) void k_cheb1d_invert_pieces(const SplineCalcPiece *__restrict__ tab, long rows,
                                                             const double *__restrict__ vals,
                                                             const double *__restrict__ targets, double *__restrict__ px,
                                                             int32_t *__restrict__ pstatus) {
    __shared__ double tile[INV_TILE(NP)];
    const long j = (long)blockIdx.y;
    const SplineCalcPiece pc = tab[j];
    InvArgs a;
    a.n = pc.n; a.rows = rows; a.lo = pc.lo; a.hi = pc.hi;
    a.nodes = pc.nodes; a.wts = pc.wts;
    a.vals = vals + rows * pc.voff;
    a.targets = targets;
    a.x = px + j * rows;
    a.status = pstatus + j * rows;
    a.iters = nullptr;
    inv_block<NP>(a, (long)blockIdx.x, tile);
}

// One thread per row: the lowest x of the pieces with status > 0 (the pieces are ordered, so the first such piece),
// the sum of the pieces' statuses; a -1 in any piece makes the row -1 and NaN.  A solution exactly on an interior knot
// is counted by both pieces that find it.
__global__ __launch_bounds__(256) void k_spline_invert_merge(int P, long rows, const double *__restrict__ px,
                                                             const int32_t *__restrict__ pstatus, double *__restrict__ x_out,
                                                             int32_t *__restrict__ status_out) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    bool failed = false;
    int sum = 0;
    double x = NAN;
    for (int j = 0; j < P; ++j) {
        const int s = pstatus[(long)j * rows + r];
        failed = failed || s < 0;
        if (s > 0) {
            const double xj = px[(long)j * rows + r];
            if (sum == 0 || xj < x) x = xj;
            sum += s;
        }
    }
    x_out[r] = failed ? NAN : x;
    status_out[r] = failed ? -1 : sum;
}
#endif
