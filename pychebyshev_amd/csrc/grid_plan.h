// grid_plan.h -- the plan of a tensor-product grid evaluation (pcx_mode_product.hip): the matrices W_k of barycentric
// weights, the order in which the dimensions are contracted, and the chain direction of a tensor-train grid.
//
// The planner is pure: it reads node counts, nodes, weights and the axes, calls nothing of the HIP runtime and launches
// no kernel, so every rule of it runs on a machine without a GPU (tests/host/grid_plan_main.cpp prints the plan of any
// case; tests/test_eval_grid_host.py).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/pcx.h"

// One mode product of the plan: Y[o, j, q] = sum_i W[j, i] X[o, i, q] along dimension `dim`, with the dimensions in
// front of it at their current sizes (m_k where already contracted, n_k otherwise).
struct GridPass {
    int dim;
    long outer;
    int n;
    long inner;
    int m;
    long w_off;        // offset (doubles) of W_dim in GridPlan::W
    long out_count;    // outer * m * inner
};

struct GridPlan {
    std::vector<double> W;          // W_k (m_k x n_k, C order) one behind the other, dimension 0 first
    std::vector<long> w_off;        // offset of W_k in W
    std::vector<int32_t> hot;       // per axis entry, laid out like axes_cat: the column a one-hot row selects, else -1
    std::vector<long> hot_off;      // offset of dimension k's entries in hot
    std::vector<GridPass> passes;   // in the order they run
    long max_intermediate = 0;      // the largest output of a pass that is not the last one (0 when d == 1)
};

// np.sum of a contiguous float64 array (NumPy's pairwise summation: blocks of 128, eight running sums), so that a row
// is the reference's  w / diff / np.sum(w / diff)  to the last bit.
static inline double grid_pairwise_sum(const double *a, long n) {
    if (n < 8) {
        double s = 0.0;
        for (long i = 0; i < n; ++i) s += a[i];
        return s;
    }
    if (n <= 128) {
        double r[8];
        for (int u = 0; u < 8; ++u) r[u] = a[u];
        long i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int u = 0; u < 8; ++u) r[u] += a[i + u];
        double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) s += a[i];
        return s;
    }
    long n2 = n / 2;
    n2 -= n2 % 8;
    return grid_pairwise_sum(a, n2) + grid_pairwise_sum(a + n2, n - n2);
}

// Row of W for the coordinate x (reference barycentric.py:941-947): one-hot at the FIRST node within 1e-14 of x, else
// (w_i / (x - node_i)) / sum_i (w_i / (x - node_i)).  x is not checked against the domain.  Returns the one-hot column or -1.
static inline int grid_weight_row(double x, const double *nodes, const double *wts, int n, double *row, double *tmp) {
    for (int i = 0; i < n; ++i)
        if (std::fabs(x - nodes[i]) < 1e-14) {
            for (int j = 0; j < n; ++j) row[j] = 0.0;
            row[i] = 1.0;
            return i;
        }
    for (int i = 0; i < n; ++i) tmp[i] = wts[i] / (x - nodes[i]);
    const double s = grid_pairwise_sum(tmp, n);
    for (int i = 0; i < n; ++i) row[i] = tmp[i] / s;
    return -1;
}

// The contraction order: ascending m_k / n_k, compared exactly as m_a n_b < m_b n_a in 64-bit integers, ties to the
// higher dimension index first: the dimensions that shrink most go first, so the intermediates stay small.
static inline std::vector<int> grid_order(int d, const int32_t *n, const int32_t *m) {
    std::vector<int> order(d);
    for (int k = 0; k < d; ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        const int64_t l = (int64_t)m[a] * n[b], r = (int64_t)m[b] * n[a];
        return l != r ? l < r : a > b;
    });
    return order;
}

// PCX_OK, or PCX_ERR_INVALID with the reason in err (an empty axis, a node count below 1, a NULL array).
static inline int grid_make_plan(int d, const int32_t *n, const double *nodes_cat, const double *weights_cat, const int32_t *m,
                                 const double *axes_cat, GridPlan &gp, char *err, size_t errlen) {
    if (d < 1 || d > PCX_MAX_DIMS) {
        snprintf(err, errlen, "d=%d outside [1, %d]", d, PCX_MAX_DIMS);
        return PCX_ERR_INVALID;
    }
    if (!n || !nodes_cat || !weights_cat || !m || !axes_cat) {
        snprintf(err, errlen, "NULL argument");
        return PCX_ERR_INVALID;
    }
    long wtotal = 0;
    int nmax = 1;
    gp.w_off.assign(d, 0);
    gp.hot_off.assign(d, 0);
    long mtotal = 0;
    for (int k = 0; k < d; ++k) {
        if (n[k] < 1) {
            snprintf(err, errlen, "n_nodes[%d]=%d < 1", k, n[k]);
            return PCX_ERR_INVALID;
        }
        if (m[k] < 1) {
            snprintf(err, errlen, "m[%d]=%d: the axis of dimension %d is empty", k, m[k], k);
            return PCX_ERR_INVALID;
        }
        gp.w_off[k] = wtotal;
        wtotal += (long)m[k] * n[k];
        gp.hot_off[k] = mtotal;
        mtotal += m[k];
        nmax = std::max(nmax, (int)n[k]);
    }
    gp.W.assign((size_t)wtotal, 0.0);
    gp.hot.assign((size_t)mtotal, -1);
    std::vector<double> tmp((size_t)nmax);
    long noff = 0, aoff = 0;
    for (int k = 0; k < d; ++k) {
        for (int r = 0; r < m[k]; ++r)
            gp.hot[aoff + r] = grid_weight_row(axes_cat[aoff + r], nodes_cat + noff, weights_cat + noff, n[k],
                                               gp.W.data() + gp.w_off[k] + (long)r * n[k], tmp.data());
        noff += n[k];
        aoff += m[k];
    }
    const std::vector<int> order = grid_order(d, n, m);
    std::vector<long> cur(n, n + d);
    gp.passes.clear();
    gp.max_intermediate = 0;
    for (int p = 0; p < d; ++p) {
        const int k = order[p];
        GridPass ps;
        ps.dim = k;
        ps.outer = ps.inner = 1;
        for (int q = 0; q < k; ++q) ps.outer *= cur[q];
        for (int q = k + 1; q < d; ++q) ps.inner *= cur[q];
        ps.n = n[k];
        ps.m = m[k];
        ps.w_off = gp.w_off[k];
        ps.out_count = ps.outer * ps.m * ps.inner;
        cur[k] = m[k];
        if (p + 1 < d) gp.max_intermediate = std::max(gp.max_intermediate, ps.out_count);
        gp.passes.push_back(ps);
    }
    return PCX_OK;
}

// ---------------------------------------------------------------------------------
// Tensor-train grids: the dense tensor of value cores G_k (r_k, m_k, r_{k+1}) is the chain of their products.  From the
// left,  P_{k+1} (M_k m_k x r_{k+1}) = P_k (M_k x r_k) . G_k (r_k x m_k r_{k+1})  with M_k = m_0 .. m_{k-1}; from the
// right,  Q_k (r_k m_k x N_k) = G_k (r_k m_k x r_{k+1}) . Q_{k+1} (r_{k+1} x N_k)  with N_k = m_{k+1} .. m_{d-1}.  Each
// step is one mode product with outer = 1:  Y (m x inner) = W (m x n) . X (n x inner).
// ---------------------------------------------------------------------------------
struct TTGridStep {
    int core;          // the core that enters at this step
    bool w_is_core;    // from the right W is the core and X the running product; from the left the other way round
    int64_t m;         // rows of W
    int n;             // the contracted rank
    int64_t inner;
    int64_t out_count; // m * inner
};

struct TTGridPlan {
    bool from_right = false;
    std::vector<long> core_off;      // offset (doubles) of G_k in grid_cores_cat; [d] = its length
    std::vector<TTGridStep> steps;   // d - 1 of them
    int64_t max_intermediate = 0;    // the largest output of a step that is not the last one
    int64_t total = 0;               // prod m_k
};

static inline void tt_grid_steps(int d, const int32_t *m, const int32_t *r, bool from_right, std::vector<TTGridStep> &steps,
                                 int64_t &max_inter) {
    steps.clear();
    max_inter = 0;
    int64_t run = from_right ? m[d - 1] : m[0];      // N_{k} or M_{k}
    for (int s = 1; s < d; ++s) {
        TTGridStep st;
        st.w_is_core = from_right;
        if (from_right) {
            const int k = d - 1 - s;
            st.core = k;
            st.m = (int64_t)r[k] * m[k];
            st.n = r[k + 1];
            st.inner = run;
            run *= m[k];
        } else {
            const int k = s;
            st.core = k;
            st.m = run;
            st.n = r[k];
            st.inner = (int64_t)m[k] * r[k + 1];
            run *= m[k];
        }
        st.out_count = st.m * st.inner;
        if (s + 1 < d) max_inter = std::max(max_inter, st.out_count);
        steps.push_back(st);
    }
}

// The direction with the smaller largest intermediate; a tie goes from the left.
static inline int tt_grid_make_plan(int d, const int32_t *m, const int32_t *ranks, TTGridPlan &tp, char *err, size_t errlen) {
    if (d < 1 || d > PCX_MAX_DIMS) {
        snprintf(err, errlen, "d=%d outside [1, %d]", d, PCX_MAX_DIMS);
        return PCX_ERR_INVALID;
    }
    if (!m || !ranks) {
        snprintf(err, errlen, "NULL argument");
        return PCX_ERR_INVALID;
    }
    if (ranks[0] != 1 || ranks[d] != 1) {
        snprintf(err, errlen, "boundary ranks must be 1");
        return PCX_ERR_INVALID;
    }
    tp.core_off.assign(d + 1, 0);
    tp.total = 1;
    for (int k = 0; k < d; ++k) {
        if (m[k] < 1) {
            snprintf(err, errlen, "m[%d]=%d: the axis of dimension %d is empty", k, m[k], k);
            return PCX_ERR_INVALID;
        }
        if (ranks[k + 1] < 1) {
            snprintf(err, errlen, "ranks[%d]=%d < 1", k + 1, ranks[k + 1]);
            return PCX_ERR_INVALID;
        }
        tp.core_off[k + 1] = tp.core_off[k] + (long)ranks[k] * m[k] * ranks[k + 1];
        tp.total *= m[k];
    }
    std::vector<TTGridStep> left, right;
    int64_t il = 0, ir = 0;
    tt_grid_steps(d, m, ranks, false, left, il);
    tt_grid_steps(d, m, ranks, true, right, ir);
    tp.from_right = ir < il;
    tp.steps = tp.from_right ? right : left;
    tp.max_intermediate = tp.from_right ? ir : il;
    return PCX_OK;
}
