#!/usr/bin/env python3
"""Generate tests/golden/g22_tt_transforms.npz: the reference's ``ChebyshevTT.slice`` / ``extrude`` / ``integrate`` /
``inner_product`` and, row by row, ``integrate(dims, bounds).eval(point)`` -- what ``integrate_batch`` computes.

Run in the build container only (the reference checkout does not travel to the GPU box):

    python tests/golden/generate_golden_tt_transforms.py --ref <reference checkout>

It imports PyChebyshev v0.21.1 from ``<ref>/src`` and stores arrays only.  Nothing is built by TT-Cross: the models
are seeded random coefficient cores ``normal * DECAY**j / sqrt(r_left)`` (j = the coefficient index), so the ranks are
exactly the ones listed, wrapped in reference objects through ``__new__``; a model with a storage order gets it as
``_dim_order`` directly.

    model  d  n            ranks            order           reaches
    A      1  6            1,1              id              m = d = 1, row width 2
    B      2  2,3          1,2,1            [1,0]           n = 2, n = 3, first and last core integrated, reorder
    C      5  11 x 5       1,8,8,8,6,1      id              rank cap 8, one node count (the bench's 5-D shape)
    C2     5  11 x 5       1,8,8,8,6,1      [2,0,4,1,3]     the same cores behind a storage order
    D      4  7,16,5,9     1,12,9,10,1      [3,1,0,2]       rank cap 12, mixed node counts, n = 16
    E      4  16,3,12,7    1,16,16,9,1      id              rank cap 16
    F      3  5,20,4       1,20,17,1        id              generic form: rank > 16 and n > 16

Keys, ``<M>`` a model:

    <M>_core<k>, <M>_domain (storage frame), <M>_order
    <M>_box<i>_dims, _bounds (N, m, 2), _points (N, d - m), _ref (N,)        integrate_batch groups
        row 0: the whole domain in every integrated dimension; row 1: lo == hi in the first integrated dimension;
        rows 2 and 3: the first kept coordinate on its lower / upper domain end.  Box widths are uniform in 5 % - 100 %
        of the domain.  A group's seed is the first for which at least MIN_SHARE of its rows have
        |ref| >= 1e-3 max|ref| (the rows the pointwise bound of tests/conftest.py looks at).
    <M>_int_full, <M>_int_sub_bounds (d, 2), <M>_int_sub                      scalar integrate()
    The rest for the models of TRANSFORM_MODELS (inner products: IP_MODELS): d = 1, a two-core reordered model, the 5-D
    identity-order model and the 4-D reordered one (E and F repeat D's and C's paths with cores three times the size):
    <M>_<op><i>_params, _single, _core<k>, _order, _domain, _n, _pts, _vals   op = slice / extrude / integ
        slice params rows (dim, value); extrude rows (dim, lo, hi, n); integ rows (dim, lo, hi), NaN = whole domain;
        _single = 1: the test passes the lone tuple (or int) form; _pts / _vals: points in the result's user frame and the
        reference's eval there.
    <M>_other_core<k>, <M>_ip_self, <M>_ip_other, <M>_sum_core<k>, <M>_ip_sum  inner_product (sum = self + other by the
        reference, ip_sum = sum . self)
"""
from __future__ import annotations

import argparse
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DECAY = 0.55
ROWS = 48
MIN_SHARE = 0.92
TRANSFORM_MODELS = ("A", "B", "C", "D")     # slice / extrude / partial integrate results are stored for these:
IP_MODELS = ("B", "C", "D")               # ... and inner products for these.  C has the identity order, B and D a storage order

MODELS = {
    "A": (101, [6], [1, 1], None),
    "B": (102, [2, 3], [1, 2, 1], [1, 0]),
    "C": (103, [11] * 5, [1, 8, 8, 8, 6, 1], None),
    "C2": (103, [11] * 5, [1, 8, 8, 8, 6, 1], [2, 0, 4, 1, 3]),
    "D": (104, [7, 16, 5, 9], [1, 12, 9, 10, 1], [3, 1, 0, 2]),
    "E": (105, [16, 3, 12, 7], [1, 16, 16, 9, 1], None),
    "F": (106, [5, 20, 4], [1, 20, 17, 1], None),
}
DOMAINS = [[-1.0, 1.0], [0.5, 3.0], [-2.0, -0.25], [10.0, 14.0], [0.0, 1.0]]     # storage position k: DOMAINS[k]
SUBSETS = {4: [[0], [3], [1, 2], [0, 2], [0, 1, 2, 3], [0, 1, 3]],
           5: [[0], [4], [1, 2], [0, 3], [0, 1, 2, 3, 4], [1, 3, 4]]}


def model_cores(seed, n, ranks):
    rng = np.random.default_rng(seed)
    cores = []
    for k, nk in enumerate(n):
        c = rng.standard_normal((ranks[k], nk, ranks[k + 1])) * (DECAY ** np.arange(nk))[None, :, None]
        cores.append(c / np.sqrt(ranks[k]))
    return cores


def subsets(d):
    if d <= 3:
        return [list(s) for m in range(1, d + 1) for s in itertools.combinations(range(d), m)]
    return SUBSETS[d]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of PyChebyshev v0.21.1")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.ref, "src"))
    import pychebyshev as ref
    from pychebyshev import ChebyshevTT

    print("reference version", ref.__version__)

    def make_tt(cores, domain, order):
        obj = ChebyshevTT.__new__(ChebyshevTT)
        obj.function = None
        obj.num_dimensions = len(cores)
        obj.domain = [list(b) for b in domain]
        obj.n_nodes = [c.shape[1] for c in cores]
        obj.max_rank = 64
        obj.tolerance = 1e-14
        obj.max_sweeps = 10
        obj.max_derivative_order = 2
        obj.additional_data = None
        obj.descriptor = ""
        obj.method = "cross"
        obj._coeff_cores = [np.array(c) for c in cores]
        obj._tt_ranks = [1] + [c.shape[2] for c in cores]
        obj._built = True
        obj._build_time = 0.0
        obj._total_build_evals = 0
        obj._cached_error_estimate = None
        obj._dim_order = list(range(len(cores))) if order is None else list(order)
        return obj

    out = {}

    def store_result(prefix, res, seed):
        for k, c in enumerate(res._coeff_cores):
            out[f"{prefix}_core{k}"] = np.array(c)
        out[f"{prefix}_order"] = np.array(res._dim_order, dtype=np.int64)
        out[f"{prefix}_domain"] = np.array(res.domain, dtype=float)
        out[f"{prefix}_n"] = np.array(res.n_nodes, dtype=np.int64)
        rng = np.random.default_rng(seed)
        udom = [res.domain[res._dim_order.index(u)] for u in range(res.num_dimensions)]
        pts = np.column_stack([rng.uniform(a, b, 24) for a, b in udom])
        out[f"{prefix}_pts"] = pts
        out[f"{prefix}_vals"] = np.array([res.eval(list(p)) for p in pts])

    for tag, (seed, n, ranks, order) in MODELS.items():
        d = len(n)
        cores = model_cores(seed, n, ranks)
        domain = DOMAINS[:d]
        tt = make_tt(cores, domain, order)
        dim_order = tt._dim_order
        udom = [domain[dim_order.index(u)] for u in range(d)]          # user frame
        for k, c in enumerate(cores):
            out[f"{tag}_core{k}"] = c
        out[f"{tag}_domain"] = np.array(domain, dtype=float)
        out[f"{tag}_order"] = np.array(dim_order, dtype=np.int64)

        # ---- integrate_batch groups
        for gi, dims in enumerate(subsets(d)):
            m = len(dims)
            kept = [u for u in range(d) if u not in dims]
            for attempt in range(400):
                rng = np.random.default_rng(seed * 1000 + gi * 401 + attempt)
                bounds = np.empty((ROWS, m, 2))
                for j, u in enumerate(dims):
                    a, b = udom[u]
                    w = rng.uniform(0.05, 1.0, ROWS) * (b - a)
                    lo = a + rng.uniform(0.0, 1.0, ROWS) * ((b - a) - w)
                    bounds[:, j, 0] = np.clip(lo, a, b)
                    bounds[:, j, 1] = np.clip(lo + w, a, b)
                    bounds[0, j] = (a, b)
                bounds[1, 0, 1] = bounds[1, 0, 0]
                points = np.column_stack([rng.uniform(*udom[u], ROWS) for u in kept]) if kept else np.empty((ROWS, 0))
                if kept:
                    points[2, 0] = udom[kept[0]][0]
                    points[3, 0] = udom[kept[0]][1]
                vals = np.empty(ROWS)
                for r in range(ROWS):
                    res = tt.integrate(dims, bounds=[(float(lo), float(hi)) for lo, hi in bounds[r]])
                    vals[r] = res if not kept else res.eval([float(v) for v in points[r]])
                share = float(np.mean(np.abs(vals) >= 1e-3 * np.max(np.abs(vals))))
                if share >= MIN_SHARE:
                    break
            else:
                raise SystemExit(f"{tag} dims {dims}: no seed reaches {MIN_SHARE}")
            print(f"{tag} box{gi} dims {dims}: attempt {attempt}, share {share:.3f}, max|ref| {np.max(np.abs(vals)):.3e}")
            assert vals[1] == 0.0 or abs(vals[1]) < 1e-13 * np.max(np.abs(vals))
            out[f"{tag}_box{gi}_dims"] = np.array(dims, dtype=np.int64)
            out[f"{tag}_box{gi}_bounds"] = bounds
            out[f"{tag}_box{gi}_points"] = points
            out[f"{tag}_box{gi}_ref"] = vals

        # ---- scalar integrate
        rng = np.random.default_rng(seed + 7000)
        out[f"{tag}_int_full"] = np.array(tt.integrate())
        sub = np.array([[a + 0.2 * (b - a) * rng.uniform(), b - 0.3 * (b - a) * rng.uniform()] for a, b in udom])
        out[f"{tag}_int_sub_bounds"] = sub
        out[f"{tag}_int_sub"] = np.array(tt.integrate(None, bounds=[tuple(map(float, r)) for r in sub]))

        # ---- inner products
        if tag not in TRANSFORM_MODELS:
            continue
        rng = np.random.default_rng(seed + 8000)
        other = make_tt([c * (1.0 + 0.25 * rng.standard_normal(c.shape)) for c in cores], domain, order)
        if tag in IP_MODELS:
            for k, c in enumerate(other._coeff_cores):
                out[f"{tag}_other_core{k}"] = c
            out[f"{tag}_ip_self"] = np.array(tt.inner_product(tt))
            out[f"{tag}_ip_other"] = np.array(tt.inner_product(other))
            total = tt + other
            for k, c in enumerate(total._coeff_cores):
                out[f"{tag}_sum_core{k}"] = np.array(c)
            out[f"{tag}_ip_sum"] = np.array(total.inner_product(tt))

        # ---- extrude (any d)
        ext = [[(0, (-3.0, -1.0), 4)], [(d, (2.0, 5.0), 3)], [(1, (0.0, 2.0), 5), (d + 1, (-1.0, 1.0), 2)]]
        for i, params in enumerate(ext):
            single = 1 if len(params) == 1 and i == 0 else 0
            res = tt.extrude(params[0] if single else params)
            out[f"{tag}_extrude{i}_params"] = np.array([[p[0], p[1][0], p[1][1], p[2]] for p in params], dtype=float)
            out[f"{tag}_extrude{i}_single"] = np.array(single)
            store_result(f"{tag}_extrude{i}", res, seed + 9000 + i)
        if d < 2:
            continue

        # ---- slice and partial integrate
        rng = np.random.default_rng(seed + 9500)
        inside = lambda u: float(rng.uniform(*udom[u]))                                   # noqa: E731
        pos_last = dim_order[d - 1]                          # the user dimension stored last
        node = lambda u: float(np.sort(0.5 * (udom[u][0] + udom[u][1]) + 0.5 * (udom[u][1] - udom[u][0])   # noqa: E731
                                       * np.cos(np.pi * (2 * np.arange(tt.n_nodes[dim_order.index(u)]) + 1)
                                                / (2 * tt.n_nodes[dim_order.index(u)])))[1])
        sl = [[(0, inside(0))], [(pos_last, inside(pos_last))], [(d - 1, node(d - 1))]]
        if d >= 3:
            sl.append([(0, inside(0)), (d - 1, inside(d - 1))])
            sl.append([(1, udom[1][0]), (2, inside(2))])
        for i, params in enumerate(sl):
            single = 1 if i == 0 else 0
            res = tt.slice(params[0] if single else params)
            out[f"{tag}_slice{i}_params"] = np.array(params, dtype=float)
            out[f"{tag}_slice{i}_single"] = np.array(single)
            store_result(f"{tag}_slice{i}", res, seed + 9600 + i)
        box = lambda u: (udom[u][0] + 0.1 * (udom[u][1] - udom[u][0]), udom[u][1] - 0.25 * (udom[u][1] - udom[u][0]))  # noqa: E731
        nan = (np.nan, np.nan)
        ig = [[(0, *nan)], [(pos_last, *box(pos_last))], [(d - 1, *nan)]]
        if d >= 3:
            ig.append([(0, *box(0)), (1, *nan)])
            ig.append([(d - 2, *nan), (d - 1, *box(d - 1))])
            ig.append([(0, *box(0)), (d - 1, *box(d - 1))])
        for i, params in enumerate(ig):
            single = 1 if i == 0 else 0
            dims = [p[0] for p in params]
            bnds = None if all(np.isnan(p[1]) for p in params) else [None if np.isnan(p[1]) else (p[1], p[2]) for p in params]
            res = tt.integrate(dims[0] if single else dims, bounds=bnds)
            out[f"{tag}_integ{i}_params"] = np.array(params, dtype=float)
            out[f"{tag}_integ{i}_single"] = np.array(single)
            store_result(f"{tag}_integ{i}", res, seed + 9700 + i)

    path = os.path.join(HERE, "g22_tt_transforms.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
