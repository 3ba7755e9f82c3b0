#!/usr/bin/env python3
"""Generate tests/golden/g25_slider_calculus.npz: the reference's ChebyshevSlider roots / minimize / maximize,
integrate, slice and extrude.

Run in the build container only (the reference checkout does not travel to the GPU box):

    python tests/golden/generate_golden_slider_calculus.py [--ref /root/reference]

It imports PyChebyshev v0.21.1 from ``<ref>/src`` and stores arrays only.  The cases (``CASES``), their functions and
every set of arguments below are imported by the tests.

  <c>_d<k>_rows / _roots / _count / _min / _max
                    case c along dimension k: ``calculus_rows(c, k)`` (the other dimensions in increasing order),
                    roots NaN-padded to n_k - 1 columns with their counts, min and max as (value, location) rows
  <c>_int_full      integrate() over everything;  <c>_int_sub: integrate(None, SUB_BOUNDS[c])
  <c>_int<i>_*      integrate(*INT_SETS[c][i]): a slider (stored as below) and its values at ``_points``
  <c>_box<i>_*      BOX_SETS[c][i] = dims: ``_bounds`` (8, m, 2) and ``_points`` (8, d - m) from ``box_rows(c, i)``,
                    ``_values`` the reference's integrate(dims, bounds[r]) then eval(points[r]), one call per row
  <c>_sl<i>_*       slice(SLICE_SETS[c][i]);   <c>_ex<i>_*: extrude(EXTRUDE_SETS[c][i])
  a stored slider   ``_part_sizes`` / ``_part_dims`` (the partition, flattened), ``_pivot_value``, ``_domain``,
                    ``_n_nodes``, ``_tensor<j>`` per slide, ``_points`` (about eight, seeded) and ``_values``
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import functions as F  # noqa: E402

SEED = 2525
N_RANDOM_ROWS = 10
N_POINTS = 8


def f_b(x, _=None):
    """SLIDER_CASES["b"] shifted down by 8: fibres along spot cross zero."""
    return F.bs_5d(x) - 8.0


def f_c(x, _=None):
    return math.sin(3.0 * x[0]) * math.cos(2.0 * x[1]) + x[2] * x[2] - 0.3 + 0.5 * x[3] * math.exp(0.5 * x[2])


def f_l(x, _=None):
    return math.sin(9.0 * x[0]) + 0.3 * x[1]


_A, _B = F.SLIDER_CASES["a"], F.SLIDER_CASES["b"]
CASES = {
    "a": dict(f=getattr(F, _A["f"]), d=_A["d"], domain=_A["domain"], n_nodes=_A["n_nodes"], partition=_A["partition"],
              pivot=_A["pivot"]),
    "b": dict(f=f_b, d=_B["d"], domain=_B["domain"], n_nodes=_B["n_nodes"], partition=_B["partition"], pivot=_B["pivot"]),
    "c": dict(f=f_c, d=4, domain=[[-1.0, 1.0]] * 3 + [[-0.5, 1.5]], n_nodes=[15, 13, 9, 6], partition=[[0, 1], [2, 3]],
              pivot=[0.2, -0.1, 0.3, 0.1]),
    "l": dict(f=f_l, d=2, domain=[[-1.0, 1.0]] * 2, n_nodes=[70, 5], partition=[[0], [1]], pivot=[0.0, 0.0]),
}
L_FIXED = 0.4          # case l along dimension 0: the over-64-nodes host path, 5 roots

# integrate(dims, bounds): full / partial / none slides, groups split by dims
INT_SETS = {
    "a": [([0], None), ([0, 2], [(-0.5, 0.3), None])],
    "b": [([0], None), ([1, 2], [(95.0, 108.0), None]), ([0, 1, 3], None), ([2, 3, 4], [(0.3, 0.9), None, (0.02, 0.05)])],
    "c": [([0], None), ([1, 2], [(-0.4, 0.7), (0.0, 1.0)]), ([0, 1], None), ([0, 2, 3], [None, (-1.0, 0.25), (0.0, 1.5)])],
    "l": [([0], None)],
}
SUB_BOUNDS = {
    "a": [(-0.5, 0.3), (0.0, 1.0), (-1.0, -0.2)],
    "b": [(85.0, 115.0), (95.0, 108.0), (0.3, 0.9), (0.2, 0.3), (0.02, 0.05)],
    "c": [(-0.4, 0.7), (-1.0, 0.0), (0.0, 1.0), (0.0, 1.5)],
    "l": [(-0.3, 0.9), (-1.0, 0.5)],
}
BOX_SETS = {
    "a": [[0], [0, 1, 2]],
    "b": [[1, 2], [0, 1, 2, 3, 4], [3]],
    "c": [[0], [1, 2], [0, 1, 2, 3]],
}


def node(case: str, k: int, j: int) -> float:
    """Node j (ascending) of dimension k: the arithmetic of the reference's ``_make_nodes_for_dim``."""
    lo, hi = CASES[case]["domain"][k]
    n = CASES[case]["n_nodes"][k]
    return float(np.sort(0.5 * (lo + hi) + 0.5 * (hi - lo) * np.polynomial.chebyshev.chebpts1(n))[j])


# slice: a one-dimension group, a multi-dimension group, an exact node, several at once
SLICE_SETS = {
    "a": [[(1, 0.3)], [(0, node("a", 0, 4)), (2, -0.4)]],
    "b": [[(2, 0.5)], [(0, 101.3)], [(1, node("b", 1, 6))], [(3, node("b", 3, 2)), (2, node("b", 2, 1))],
          [(0, 93.0), (2, 0.7), (4, 0.03)]],
    "c": [[(0, 0.1)], [(3, node("c", 3, 4))], [(1, 0.2), (2, 0.3)]],
}
EXTRUDE_SETS = {
    "a": [[(1, (0.0, 2.0), 5)]],
    "b": [[(0, (-1.0, 1.0), 4), (6, (0.0, 3.0), 3)], [(3, (1.0, 2.0), 6)]],
    "c": [[(2, (1.0, 2.0), 6)], [(4, (-2.0, 0.0), 3), (0, (0.0, 1.0), 2)]],
}


def calculus_rows(case: str, dim: int) -> np.ndarray:
    """The fixed rows of (case, dim), columns = the other dimensions in increasing order: N_RANDOM_ROWS seeded rows
    inside 5-95 % of each domain, one row of exact node values and one at the domain corners."""
    c = CASES[case]
    if case == "l" and dim == 0:
        return np.array([[L_FIXED]])
    others = [k for k in range(c["d"]) if k != dim]
    rng = np.random.default_rng([SEED, sorted(CASES).index(case), dim])
    rows = np.empty((N_RANDOM_ROWS + 2, len(others)))
    for col, k in enumerate(others):
        lo, hi = c["domain"][k]
        rows[:N_RANDOM_ROWS, col] = lo + (hi - lo) * rng.uniform(0.05, 0.95, N_RANDOM_ROWS)
        rows[N_RANDOM_ROWS, col] = node(case, k, (k + 2) % c["n_nodes"][k])
        rows[N_RANDOM_ROWS + 1, col] = lo if (k + dim) % 2 == 0 else hi
    return rows


def points_in(domain, seed_key) -> np.ndarray:
    """N_POINTS seeded points of a domain (list of (lo, hi))."""
    rng = np.random.default_rng([SEED] + list(seed_key))
    dom = np.asarray(domain, dtype=float).reshape(-1, 2)
    return dom[:, 0] + (dom[:, 1] - dom[:, 0]) * rng.uniform(0.0, 1.0, (N_POINTS, dom.shape[0]))


def box_rows(case: str, i: int):
    """(bounds (N_POINTS, m, 2), points (N_POINTS, d - m)) of BOX_SETS[case][i]; row 0 integrates the whole domain."""
    c = CASES[case]
    dims = BOX_SETS[case][i]
    rng = np.random.default_rng([SEED, 77, sorted(CASES).index(case), i])
    dom = np.asarray(c["domain"], dtype=float)
    u = np.sort(rng.uniform(0.0, 1.0, (N_POINTS, len(dims), 2)), axis=2)
    u[0, :, 0], u[0, :, 1] = 0.0, 1.0
    lo, w = dom[dims, 0][None, :, None], (dom[dims, 1] - dom[dims, 0])[None, :, None]
    bounds = lo + w * u
    kept = [k for k in range(c["d"]) if k not in dims]
    return bounds, points_in(dom[kept], [78, sorted(CASES).index(case), i]) if kept else np.empty((N_POINTS, 0))


def build(cls, case: str):
    c = CASES[case]
    obj = cls(c["f"], c["d"], c["domain"], c["n_nodes"], partition=c["partition"], pivot_point=c["pivot"])
    obj.build(verbose=False)
    return obj


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.ref, "src"))
    import pychebyshev as ref
    from pychebyshev import ChebyshevSlider

    print("reference version", ref.__version__)
    t0 = time.time()
    out = {}

    def store_slider(tag, s, seed_key):
        out[f"{tag}_part_sizes"] = np.array([len(g) for g in s.partition], dtype=np.int32)
        out[f"{tag}_part_dims"] = np.array([d for g in s.partition for d in g], dtype=np.int32)
        out[f"{tag}_pivot_value"] = np.array(float(s.pivot_value))
        out[f"{tag}_domain"] = np.asarray(s.domain, dtype=float).reshape(-1, 2)
        out[f"{tag}_n_nodes"] = np.array(s.n_nodes, dtype=np.int32)
        for j, slide in enumerate(s.slides):
            out[f"{tag}_tensor{j}"] = np.asarray(slide.tensor_values, dtype=float)
        pts = points_in(s.domain, seed_key)
        out[f"{tag}_points"] = pts
        out[f"{tag}_values"] = np.array([float(s.eval(list(p), [0] * s.num_dimensions)) for p in pts])

    for ci, case in enumerate(sorted(CASES)):
        c = CASES[case]
        sl = build(ChebyshevSlider, case)
        d = c["d"]
        for k in range(d):
            rows = calculus_rows(case, k)
            others = [q for q in range(d) if q != k]
            W = max(c["n_nodes"][k] - 1, 1)
            R = np.full((rows.shape[0], W), np.nan)
            cnt = np.zeros(rows.shape[0], dtype=np.int32)
            mn, mx = np.empty((rows.shape[0], 2)), np.empty((rows.shape[0], 2))
            for r, row in enumerate(rows):
                fixed = {q: float(v) for q, v in zip(others, row)}
                got = np.asarray(sl.roots(k, fixed), dtype=float)
                cnt[r] = got.size
                R[r, :got.size] = got
                mn[r], mx[r] = sl.minimize(k, fixed), sl.maximize(k, fixed)
            out[f"{case}_d{k}_rows"], out[f"{case}_d{k}_roots"], out[f"{case}_d{k}_count"] = rows, R, cnt
            out[f"{case}_d{k}_min"], out[f"{case}_d{k}_max"] = mn, mx
        out[f"{case}_int_full"] = np.array(float(sl.integrate()))
        out[f"{case}_int_sub"] = np.array(float(sl.integrate(None, list(SUB_BOUNDS[case]))))
        for i, (dims, bounds) in enumerate(INT_SETS[case]):
            store_slider(f"{case}_int{i}", sl.integrate(dims, bounds), [ci, 1, i])
        for i, dims in enumerate(BOX_SETS.get(case, [])):
            bounds, pts = box_rows(case, i)
            vals = np.empty(N_POINTS)
            for r in range(N_POINTS):
                res = sl.integrate(dims, [tuple(b) for b in bounds[r]])
                vals[r] = float(res) if len(dims) == d else float(res.eval(list(pts[r]), [0] * (d - len(dims))))
            out[f"{case}_box{i}_bounds"], out[f"{case}_box{i}_points"], out[f"{case}_box{i}_values"] = bounds, pts, vals
        for i, params in enumerate(SLICE_SETS.get(case, [])):
            store_slider(f"{case}_sl{i}", sl.slice(params), [ci, 2, i])
        for i, params in enumerate(EXTRUDE_SETS.get(case, [])):
            store_slider(f"{case}_ex{i}", sl.extrude(params), [ci, 3, i])

    path = os.path.join(HERE, "g25_slider_calculus.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote g25_slider_calculus.npz ({os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays) in {time.time() - t0:.1f} s")
    for case in sorted(CASES):
        print(" ", case, "root counts by dimension:", {k: out[f"{case}_d{k}_count"].tolist() for k in range(CASES[case]["d"])})


if __name__ == "__main__":
    main()
