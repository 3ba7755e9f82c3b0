#!/usr/bin/env python3
"""Generate tests/golden/g26_spline_transforms.npz: the reference's ChebyshevSpline roots / minimize / maximize along
every dimension, slice and extrude, and ChebyshevApproximation.extrude.

Run in the build container only (the reference checkout does not travel to the GPU box):

    python tests/golden/generate_golden_spline_transforms.py [--ref /root/reference]

It imports PyChebyshev v0.21.1 from ``<ref>/src`` and stores arrays only.  The cases (``CASES``), their functions and
every set of arguments below are imported by the tests.

  <c>_d<k>_rows / _roots / _count / _min / _max
                    case c along dimension k: ``calculus_rows(c, k)`` (the other dimensions in increasing order), roots
                    NaN-padded to W = sum_j max(n_j - 1, 1) columns with their counts, min and max as (value, location)
  <c>_d<k>_proots / _pcount
                    the roots of every piece of the reference's sliced 1-D spline, (N, P, max_j W_j) NaN-padded, and
                    their counts (N, P): what the reference concatenates, sorts and de-duplicates
  <c>_sl<i>_*       slice(SLICE_SETS[c][i]);   <c>_ex<i>_*: extrude(EXTRUDE_SETS[c][i])
  dense_ex<i>_*     ChebyshevApproximation.extrude(DENSE_EXTRUDE_SETS[i]) on ``build_dense``: ``_domain``, ``_n_nodes``,
                    ``_tensor``, ``_points``, ``_values``
  a stored spline   ``_domain``, ``_nknots`` and ``_knots`` (the knots per dimension, flattened), ``_shape``, ``_nested``,
                    ``_n_nodes`` (flat: d entries; nested: the per-dimension lists flattened, ``_shape`` entries each),
                    ``_tensor<j>`` per piece in C order, ``_points`` (about eight, seeded) and ``_values``

Every stored root of the cases k, m and o keeps at least ``1e-6 (b - a)`` from every piece edge and from every other root
of its row (asserted here), so the counts cannot depend on last-bit differences.  Case z is exempt: its root lies on the
knot on purpose, both pieces find it and the merge returns it once.
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

SEED = 2626
N_RANDOM_ROWS = 10
N_POINTS = 8
MARGIN = 1e-6


def f_k(x, _=None):
    return abs(x[0] - 0.2) * math.exp(x[1]) + max(x[1] - 0.5, 0.0) ** 2 - 0.45


def f_m(x, _=None):
    return math.sin(0.45 * (x[0] - 80.0)) * (1.0 + 2.0 * x[1]) + 6.0 * (x[2] - 0.25) + 0.02 * abs(x[0] - 100.0) - 0.3


def f_z(x, _=None):
    return (x[0] - 0.2) * math.exp(x[1])


def f_o(x, _=None):
    return math.sin(7.0 * x[0]) + 0.25 * abs(x[0] + 0.3)


CASES = {
    "k": dict(f=f_k, d=2, domain=[[-1.0, 1.0], [0.0, 1.0]], n_nodes=[[7, 9], [6, 8]], knots=[[0.2], [0.5]]),
    "m": dict(f=f_m, d=3, domain=[[80.0, 120.0], [0.01, 0.25], [0.1, 0.4]], n_nodes=[9, 7, 6],
              knots=[[95.0, 100.0, 105.0], [], [0.2]]),
    "z": dict(f=f_z, d=2, domain=[[-1.0, 1.0], [0.0, 1.0]], n_nodes=[8, 5], knots=[[0.2], []]),
    "o": dict(f=f_o, d=1, domain=[[-1.0, 1.0]], n_nodes=[[11, 13, 9]], knots=[[-0.3, 0.4]]),
}
DENSE = dict(f=f_k, d=2, domain=[[-1.0, 0.2], [0.0, 0.5]], n_nodes=[7, 6])      # case k's first piece as a dense model


def edges(case: str, k: int) -> list:
    c = CASES[case]
    return [c["domain"][k][0]] + list(c["knots"][k]) + [c["domain"][k][1]]


def piece_counts(case: str, k: int) -> list:
    """Node counts of the pieces along dimension k."""
    c = CASES[case]
    nk = c["n_nodes"][k]
    return list(nk) if isinstance(nk, list) else [nk] * (len(c["knots"][k]) + 1)


def node(case: str, k: int, j: int, i: int) -> float:
    """Node i (ascending) of piece j along dimension k: the arithmetic of the reference's node construction."""
    e = edges(case, k)
    lo, hi = e[j], e[j + 1]
    return float(np.sort(0.5 * (lo + hi) + 0.5 * (hi - lo) * np.polynomial.chebyshev.chebpts1(piece_counts(case, k)[j]))[i])


# slice: one dimension, two at once, a value on a knot (the right-hand piece), on a node, at a domain end
SLICE_SETS = {
    "k": [[(0, 0.35)], [(1, 0.5)], [(1, node("k", 1, 1, 3))], [(0, -1.0)], [(0, 0.2)]],
    "m": [[(1, 0.1)], [(0, 97.3), (2, 0.33)], [(0, 100.0)], [(2, 0.2), (1, 0.25)], [(1, node("m", 1, 0, 3))], [(0, 120.0)],
          [(0, node("m", 0, 2, 5))]],
    "z": [[(1, 0.37)], [(0, 0.2)]],
}
# extrude: a new dimension in front, in the middle, at the end, two at once
EXTRUDE_SETS = {
    "k": [[(0, (0.0, 2.0), 4)], [(1, (1.0, 2.0), 3)], [(2, (-1.0, 0.0), 5)], [(3, (2.0, 3.0), 3), (0, (0.0, 1.0), 2)]],
    "m": [[(1, (0.0, 1.0), 3)], [(3, (-2.0, 0.0), 4)]],
    "o": [[(0, (0.0, 1.0), 3)], [(1, (1.0, 3.0), 4)]],
}
DENSE_EXTRUDE_SETS = [[(0, (0.0, 2.0), 4)], [(1, (1.0, 2.0), 3)], [(2, (-1.0, 0.0), 5)], [(3, (2.0, 3.0), 3), (0, (0.0, 1.0), 2)]]


def calculus_rows(case: str, dim: int) -> np.ndarray:
    """The fixed rows of (case, dim), columns = the other dimensions in increasing order: N_RANDOM_ROWS seeded rows
    inside 5-95 % of each domain, one row on the other dimensions' first knots (lower bounds where there is none) and
    one at the upper corner.  A 1-D case has rows of no columns."""
    c = CASES[case]
    others = [k for k in range(c["d"]) if k != dim]
    rng = np.random.default_rng([SEED, sorted(CASES).index(case), dim])
    rows = np.empty((N_RANDOM_ROWS + 2, len(others)))
    for col, k in enumerate(others):
        lo, hi = c["domain"][k]
        rows[:N_RANDOM_ROWS, col] = lo + (hi - lo) * rng.uniform(0.05, 0.95, N_RANDOM_ROWS)
        rows[N_RANDOM_ROWS, col] = c["knots"][k][0] if c["knots"][k] else lo
        rows[N_RANDOM_ROWS + 1, col] = hi
    return rows


def points_in(domain, seed_key) -> np.ndarray:
    """N_POINTS seeded points of a domain (list of (lo, hi))."""
    rng = np.random.default_rng([SEED] + list(seed_key))
    dom = np.asarray(domain, dtype=float).reshape(-1, 2)
    return dom[:, 0] + (dom[:, 1] - dom[:, 0]) * rng.uniform(0.0, 1.0, (N_POINTS, dom.shape[0]))


def build(cls, case: str):
    c = CASES[case]
    obj = cls(c["f"], c["d"], [list(b) for b in c["domain"]],
              n_nodes=[list(v) if isinstance(v, list) else v for v in c["n_nodes"]], knots=[list(k) for k in c["knots"]])
    obj.build(verbose=False)
    return obj


def build_dense(cls):
    obj = cls(DENSE["f"], DENSE["d"], [list(b) for b in DENSE["domain"]], list(DENSE["n_nodes"]))
    obj.build(verbose=False)
    return obj


def stored_spline(g, tag: str) -> dict:
    """A spline stored by ``store_spline`` (see the module docstring) back as ``domain``, ``knots``, ``shape``, ``nested``,
    ``n_nodes`` (in the spline's own form) and ``tensors``."""
    nk = g[f"{tag}_nknots"].tolist()
    flat, knots, at = g[f"{tag}_knots"].tolist(), [], 0
    for c in nk:
        knots.append(flat[at:at + c])
        at += c
    shape = tuple(int(v) for v in g[f"{tag}_shape"])
    nested = bool(g[f"{tag}_nested"])
    n_nodes = g[f"{tag}_n_nodes"].tolist()
    if nested:
        cat, n_nodes, at = n_nodes, [], 0
        for c in shape:
            n_nodes.append(cat[at:at + c])
            at += c
    return dict(domain=g[f"{tag}_domain"], knots=knots, shape=shape, nested=nested, n_nodes=n_nodes,
                tensors=[g[f"{tag}_tensor{j}"] for j in range(int(np.prod(shape)))])


def build_mixed(spline_cls, dense_cls):
    """Two pieces along dimension 1 that share index 0 along dimension 0 with 5 and 7 nodes there, as auto-N pieces may."""
    def f(x, _=None):
        return math.sin(3.0 * x[0]) + x[1] - 0.4
    pieces = []
    for n0, (lo, hi) in ((5, (0.0, 0.5)), (7, (0.5, 1.0))):
        piece = dense_cls(f, 2, [[-1.0, 1.0], [lo, hi]], [n0, 4])
        piece.build(verbose=False)
        pieces.append(piece)
    return spline_cls.from_pieces(pieces, 2, [[-1.0, 1.0], [0.0, 1.0]], [[], [0.5]])


def check_structure(got, want, parent, tag):
    """``got`` (a result of ``parent.slice`` / ``extrude``) against a ``stored_spline``: everything but the numbers in the tensors."""
    assert type(got) is type(parent) and got._built and got.function is None, tag
    assert got.build_time == 0.0 and got.descriptor == "" and got._device_spline is None, tag
    assert got.max_derivative_order == parent.max_derivative_order and got._device_index == parent._device_index, tag
    assert got.num_dimensions == want["domain"].shape[0] == len(got.knots) == len(got.n_nodes), tag
    assert np.array_equal(np.asarray(got.domain, dtype=float), want["domain"]), tag
    assert [list(k) for k in got.knots] == want["knots"], tag
    assert got._shape == want["shape"] and got.num_pieces == len(want["tensors"]) == len(got._pieces), tag
    assert got._n_nodes_nested == want["nested"] == parent._n_nodes_nested, tag
    assert [list(v) if isinstance(v, list) else v for v in got.n_nodes] == want["n_nodes"], tag
    assert [len(iv) for iv in got._intervals] == list(want["shape"]), tag
    for k, iv in enumerate(got._intervals):
        edges = [got.domain[k][0]] + list(got.knots[k]) + [got.domain[k][1]]
        assert [tuple(e) for e in iv] == list(zip(edges[:-1], edges[1:])), tag
    for multi, piece, t in zip(np.ndindex(*got._shape), got._pieces, want["tensors"]):
        assert piece.tensor_values.shape == t.shape == tuple(piece.n_nodes), (tag, multi)
        assert [list(b) for b in piece.domain] == [list(got._intervals[k][multi[k]]) for k in range(got.num_dimensions)]
        assert piece.max_derivative_order == parent.max_derivative_order


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.ref, "src"))
    import pychebyshev as ref
    from pychebyshev import ChebyshevApproximation, ChebyshevSpline
    from pychebyshev._calculus import _roots_1d

    print("reference version", ref.__version__)
    t0 = time.time()
    out = {}
    worst = {}

    def store_spline(tag, s, seed_key):
        d = s.num_dimensions
        nested = bool(getattr(s, "_n_nodes_nested", False))
        out[f"{tag}_domain"] = np.asarray(s.domain, dtype=float).reshape(-1, 2)
        out[f"{tag}_nknots"] = np.array([len(k) for k in s.knots], dtype=np.int32)
        out[f"{tag}_knots"] = np.array([v for k in s.knots for v in k], dtype=float)
        out[f"{tag}_shape"] = np.array(s._shape, dtype=np.int32)
        out[f"{tag}_nested"] = np.array(nested)
        out[f"{tag}_n_nodes"] = np.array([v for row in s.n_nodes for v in row] if nested else list(s.n_nodes), dtype=np.int32)
        assert len(s._pieces) == int(np.prod(s._shape))
        for j, piece in enumerate(s._pieces):
            out[f"{tag}_tensor{j}"] = np.asarray(piece.tensor_values, dtype=float)
        pts = points_in(s.domain, seed_key)
        out[f"{tag}_points"] = pts
        out[f"{tag}_values"] = np.array([float(s.eval(list(p), [0] * d)) for p in pts])

    for ci, case in enumerate(sorted(CASES)):
        c = CASES[case]
        sp = build(ChebyshevSpline, case)
        d = c["d"]
        for k in range(d):
            rows = calculus_rows(case, k)
            others = [q for q in range(d) if q != k]
            counts = piece_counts(case, k)
            P, Wj = len(counts), [max(n - 1, 1) for n in counts]
            a, b = c["domain"][k]
            e = np.array(edges(case, k))
            N = rows.shape[0]
            R = np.full((N, sum(Wj)), np.nan)
            cnt = np.zeros(N, dtype=np.int32)
            PR = np.full((N, P, max(Wj)), np.nan)
            pc = np.zeros((N, P), dtype=np.int32)
            mn, mx = np.empty((N, 2)), np.empty((N, 2))
            for r, row in enumerate(rows):
                fixed = {q: float(v) for q, v in zip(others, row)} if d > 1 else None
                got = np.asarray(sp.roots(k, fixed), dtype=float)
                cnt[r] = got.size
                R[r, :got.size] = got
                mn[r], mx[r] = sp.minimize(k, fixed), sp.maximize(k, fixed)
                one = sp.slice(list(fixed.items())) if d > 1 else sp
                assert len(one._pieces) == P
                found = [np.asarray(_roots_1d(p.tensor_values, p.domain[0]), dtype=float) for p in one._pieces]
                for j, pr in enumerate(found):
                    pc[r, j] = pr.size
                    PR[r, j, :pr.size] = pr
                cat = np.concatenate(found)
                assert np.array_equal(cat, np.sort(cat)), (case, k, r, "the pieces' roots are not in order")
                if case != "z" and got.size:
                    gap = np.min(np.abs(got[:, None] - e[None, :]))
                    if got.size > 1:
                        gap = min(gap, float(np.min(np.diff(got))))
                    worst[case] = min(worst.get(case, np.inf), gap / (b - a))
                    assert gap >= MARGIN * (b - a), (case, k, r, gap)
                    assert cat.size == got.size, (case, k, r)
            out[f"{case}_d{k}_rows"], out[f"{case}_d{k}_roots"], out[f"{case}_d{k}_count"] = rows, R, cnt
            out[f"{case}_d{k}_min"], out[f"{case}_d{k}_max"] = mn, mx
            out[f"{case}_d{k}_proots"], out[f"{case}_d{k}_pcount"] = PR, pc
        for i, params in enumerate(SLICE_SETS.get(case, [])):
            store_spline(f"{case}_sl{i}", sp.slice(params), [ci, 2, i])
        for i, params in enumerate(EXTRUDE_SETS.get(case, [])):
            store_spline(f"{case}_ex{i}", sp.extrude(params), [ci, 3, i])

    dense = build_dense(ChebyshevApproximation)
    for i, params in enumerate(DENSE_EXTRUDE_SETS):
        ex = dense.extrude(params)
        tag = f"dense_ex{i}"
        out[f"{tag}_domain"] = np.asarray(ex.domain, dtype=float).reshape(-1, 2)
        out[f"{tag}_n_nodes"] = np.array(ex.n_nodes, dtype=np.int32)
        out[f"{tag}_tensor"] = np.asarray(ex.tensor_values, dtype=float)
        pts = points_in(ex.domain, [9, i])
        out[f"{tag}_points"] = pts
        out[f"{tag}_values"] = np.array([float(ex.vectorized_eval(list(p), [0] * ex.num_dimensions)) for p in pts])

    path = os.path.join(HERE, "g26_spline_transforms.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote g26_spline_transforms.npz ({os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays) in {time.time() - t0:.1f} s")
    for case in sorted(CASES):
        print(" ", case, "root counts by dimension:", {k: out[f"{case}_d{k}_count"].tolist() for k in range(CASES[case]["d"])})
    print("  smallest distance of a root to a piece edge or another root, in (b - a):", {k: f"{v:.2e}" for k, v in worst.items()})


if __name__ == "__main__":
    main()
