#!/usr/bin/env python3
"""Generate tests/golden/g24_bary_box.npz: row by row, the reference's ``ChebyshevApproximation.integrate(dims,
bounds).vectorized_eval(point)`` and ``ChebyshevSpline.integrate(dims, bounds).eval(point)`` -- what the two
``integrate_batch`` methods compute -- and the spline's ``integrate`` results.

Run in the build container only (the reference checkout does not travel to the GPU box):

    python tests/golden/generate_golden_bary_box.py --ref <reference checkout>

It imports PyChebyshev v0.21.1 from ``<ref>/src`` and stores arrays only.  Every tensor is :func:`box_function` on the
model's grid (strictly positive and smooth, so that few rows are small against the largest); the tests rebuild the
tensors from the same function, which is why it lives here and this module imports without the reference.

    model  shape                   reaches
    A      (6,)                    m = d = 1, row width 2
    B      (3, 4)                  n = 3, first and last dimension integrated
    S      (12, 12)                a handle whose evaluation prefers the lane-per-point kernel
    R1     (7, 11, 5, 5)           row-code plan, K = 25, R = 1, 5 row tiles with the last ragged
    R2     (5, 15, 6, 3)           R = 2
    R0     (5, 17, 4, 4)           R = 0, n = 17
    W      (2,) * 9 + (3,)         d = 10, wide codes
    G      (17, 17, 17)            the smallest n^3, 8 <= n <= 24, for which pcx_bary_grid_info reports a grid or k-fold
                                   plan on an MI355X (the GPU test asserts it): the rows form on an MFMA-able handle
    L      (11,) * 5               row-code plan with 30 k-steps, R = 1, 84 row tiles: the MFMA form's long-plan launch
                                   (one wave per workgroup, whole groups of k-steps with the next group fetched ahead)
    P      spline, 2-D, knots [[0.3], []], n = [5, 6]
    Q      spline, 3-D, knots [[0.3], [], [-1.5, -0.8]], n = [5, 4, 6], six pieces

Keys, ``<M>`` a model or spline:

    <M>_shape                                                                 domain and knots: domain_of, SPLINES
    <M>_box<i> (ROWS, 2 m + (d - m) + 1)                                      integrate_batch group i (split_group):
        bounds (m, 2) flattened, the kept coordinates, the reference's result.  One array per group and inputs on a
        grid of 2^-8 keep the file small (an archive member costs about 250 bytes whatever it holds).
        models: dims = model_groups(d) = [0], [d - 1], all dimensions, [0, d - 1].  Row 0: the whole domain; row 1: lo == hi in the first
        integrated dimension; rows 2 and 3: the first kept coordinate on its lower / upper domain end; row 4: the first
        kept coordinate exactly on a node.  Box widths are uniform in 40 % - 100 % of the domain; in groups with m <= 2
        every fourth row narrows one integrated dimension to 5 %.
        splines: dims = SPLINES[<M>][2]: a knotted dimension, an unknotted one, all dimensions, a mix.  Row 0 and 1 as above; row 2: a box inside
        one piece; row 3: across one knot; row 4: across every knot of the dimension; rows 5 and 6: the lower / upper
        edge exactly on a knot (rows 2 - 6 in the first knotted integrated dimension).  Kept coordinates stay 0.05 away
        from the knots.
        A group's seed is the first for which at least MIN_SHARE of its rows have |ref| >= 1e-3 max|ref|.
    <M>_int (d + 1, 2)                                                        scalar integrate(): row 0 = (whole
        domain, sub-box), rows 1 .. d = the sub-box
    <S>_part<i>_knots<k>, _domain, _piece<j>, _eval (ROWS, d - m + 1)
        partial integrate() of a spline over SPLINE_PARTIALS[<S>][i]: the result's knots, domain and pieces in C
        order, and points with the reference's eval there in the last column
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = 48
MIN_SHARE = 0.92
DOMAINS = [[-1.0, 1.0], [0.5, 3.0], [-2.0, -0.25], [10.0, 14.0], [0.0, 1.0]]     # dimension k: DOMAINS[k % 5]
MODELS = {
    "A": (6,),
    "B": (3, 4),
    "S": (12, 12),
    "R1": (7, 11, 5, 5),
    "R2": (5, 15, 6, 3),
    "R0": (5, 17, 4, 4),
    "W": (2,) * 9 + (3,),
    "G": (17, 17, 17),
    "L": (11,) * 5,
}
SPLINES = {
    "P": ([5, 6], [[0.3], []], [[0], [1], [0, 1]]),
    "Q": ([5, 4, 6], [[0.3], [], [-1.5, -0.8]], [[2], [1], [0, 1, 2], [0, 1], [0, 2]]),
}
SPLINE_PARTIALS = {          # (dims, bounds per dim or None)
    "P": [([0], None), ([0], [(-0.5, 0.7)]), ([1], [(1.0, 2.5)])],
    "Q": [([2], None), ([0, 2], [(-0.2, 0.3), (-1.9, -0.5)]), ([1], [(0.75, 2.0)])],
}


def domain_of(d):
    return [list(DOMAINS[k % 5]) for k in range(d)]


def box_function(x):
    """exp(0.3 x0) (1.5 + sin(x1 + 0.5 x2)) + 0.2 x0 x2 + 0.05 (x3 - 12)^2 + 0.02 sum_{k >= 4} x_k^2 on points
    ``(..., d)``; a missing coordinate takes x1 = 1, x2 = -1, x3 = 12.  At least 0.35 on the domains above."""
    x = np.asarray(x, dtype=float)
    d = x.shape[-1]
    x0 = x[..., 0]
    x1 = x[..., 1] if d > 1 else 1.0
    x2 = x[..., 2] if d > 2 else -1.0
    x3 = x[..., 3] if d > 3 else 12.0
    out = np.exp(0.3 * x0) * (1.5 + np.sin(x1 + 0.5 * x2)) + 0.2 * x0 * x2 + 0.05 * (x3 - 12.0) ** 2
    for k in range(4, d):
        out = out + 0.02 * x[..., k] ** 2
    return out


def grid_values(nodes_per_dim):
    """box_function on the tensor grid of the given per-dimension nodes."""
    mesh = np.meshgrid(*[np.asarray(v, dtype=float) for v in nodes_per_dim], indexing="ij")
    return box_function(np.stack(mesh, axis=-1))


def model_groups(d):
    groups = [[0], [d - 1], list(range(d)), [0, d - 1]]
    out = []
    for g in groups:
        g = sorted(set(g))
        if g not in out:
            out.append(g)
    return out


def coarse(x):
    """Random inputs on a grid of 2^-8: exact in double, and the file compresses."""
    return np.round(np.asarray(x) * 256.0) / 256.0


def join_group(b, p, ref):
    return np.column_stack([b.reshape(len(b), -1), p, ref])


def split_group(rows, m):
    """bounds (N, m, 2), points (N, d - m) and ref (N,) of a stored group with m integrated dimensions."""
    return rows[:, :2 * m].reshape(len(rows), m, 2), rows[:, 2 * m:-1], rows[:, -1]


def random_boxes(rng, dom, dims, narrow):
    b = np.empty((ROWS, len(dims), 2))
    for j, k in enumerate(dims):
        a_, b_ = dom[k]
        w = rng.uniform(0.4, 1.0, ROWS) * (b_ - a_)
        if narrow:
            hit = (np.arange(ROWS) % 4 == 3) & ((np.arange(ROWS) // 4) % len(dims) == j)
            w[hit] = 0.05 * (b_ - a_)
        lo = np.maximum(coarse(a_ + rng.uniform(0.0, 1.0, ROWS) * ((b_ - a_) - w)), a_)
        b[:, j, 0] = lo
        b[:, j, 1] = np.minimum(lo + coarse(w), b_)
    return b


def model_group_rows(rng, dom, nodes, dims):
    d = len(dom)
    kept = [k for k in range(d) if k not in dims]
    b = random_boxes(rng, dom, dims, len(dims) <= 2)
    for j, k in enumerate(dims):
        b[0, j] = dom[k]
    b[1, 0, 1] = b[1, 0, 0]
    p = (np.column_stack([np.clip(coarse(rng.uniform(dom[k][0], dom[k][1], ROWS)), *dom[k]) for k in kept]) if kept
         else np.zeros((ROWS, 0)))
    if kept:
        p[2, 0], p[3, 0] = dom[kept[0]]
        p[4, 0] = nodes[kept[0]][len(nodes[kept[0]]) // 2]
    return b, p


def spline_group_rows(rng, dom, knots, dims):
    d = len(dom)
    kept = [k for k in range(d) if k not in dims]
    b = random_boxes(rng, dom, dims, False)
    for j, k in enumerate(dims):
        b[0, j] = dom[k]
    b[1, 0, 1] = b[1, 0, 0]
    knotted = [j for j, k in enumerate(dims) if knots[k]]
    if knotted:
        j = knotted[0]
        k = dims[j]
        a_, b_ = dom[k]
        kn = knots[k]
        b[2, j] = [a_ + 0.2 * (kn[0] - a_), a_ + 0.8 * (kn[0] - a_)]
        b[3, j] = [a_ + 0.5 * (kn[0] - a_), kn[0] + 0.5 * ((kn[1] if len(kn) > 1 else b_) - kn[0])]
        b[4, j] = [a_ + 0.5 * (kn[0] - a_), kn[-1] + 0.5 * (b_ - kn[-1])]
        b[5, j] = [kn[0], kn[0] + 0.6 * (b_ - kn[0])]
        b[6, j] = [a_ + 0.3 * (kn[-1] - a_), kn[-1]]
    cols = []
    for k in kept:
        x = np.clip(coarse(rng.uniform(dom[k][0], dom[k][1], ROWS)), *dom[k])
        for kn in knots[k]:
            near = np.abs(x - kn) < 0.05
            x[near] = coarse(kn + 0.0625 + 0.1 * rng.uniform(0.0, 1.0, int(near.sum())))
        cols.append(x)
    p = np.column_stack(cols) if kept else np.zeros((ROWS, 0))
    return b, p


def share(ref):
    return float(np.mean(np.abs(ref) >= 1e-3 * np.max(np.abs(ref))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of PyChebyshev v0.21.1")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.ref, "src"))
    from pychebyshev import ChebyshevApproximation, ChebyshevSpline

    out = {}

    def sub_box(rng, dom):
        lo = np.array([a + rng.uniform(0.05, 0.3) * (b - a) for a, b in dom])
        hi = np.array([b - rng.uniform(0.05, 0.3) * (b - a) for a, b in dom])
        return np.column_stack([lo, hi])

    for tag, shape in MODELS.items():
        d = len(shape)
        dom = domain_of(d)
        info = ChebyshevApproximation.nodes(d, dom, list(shape))
        nodes = [np.asarray(v, dtype=float) for v in info["nodes_per_dim"]]
        cheb = ChebyshevApproximation.from_values(grid_values(nodes), d, dom, list(shape))
        out[f"{tag}_shape"] = np.asarray(shape, dtype=np.int64)

        def ref_rows(dims, b, p):
            kept_n = d - len(dims)
            ref = np.empty(ROWS)
            for r in range(ROWS):
                res = cheb.integrate(dims=dims, bounds=[(float(b[r, j, 0]), float(b[r, j, 1])) for j in range(len(dims))])
                ref[r] = res if kept_n == 0 else res.vectorized_eval([float(v) for v in p[r]], [0] * kept_n)
            return ref

        for i, dims in enumerate(model_groups(d)):
            for seed in range(200):
                rng = np.random.default_rng([sum(shape), i, seed])
                b, p = model_group_rows(rng, dom, nodes, dims)
                ref = ref_rows(dims, b, p)
                if share(ref) >= MIN_SHARE:
                    break
            assert share(ref) >= MIN_SHARE, (tag, dims, share(ref))
            assert ref[1] == 0.0, (tag, dims, ref[1])
            out[f"{tag}_box{i}"] = join_group(b, p, ref)
            print(f"{tag} box{i} dims={dims} seed={seed} share={share(ref):.3f} max|ref|={np.max(np.abs(ref)):.4g}")
        rng = np.random.default_rng([sum(shape), 99])
        sb = sub_box(rng, dom)
        out[f"{tag}_int"] = np.vstack([[cheb.integrate(), cheb.integrate(bounds=[(float(lo), float(hi)) for lo, hi in sb])],
                                       sb])

    for tag, (n, knots, groups) in SPLINES.items():
        d = len(n)
        dom = domain_of(d)
        info = ChebyshevSpline.nodes(d, dom, n, knots)
        vals = [grid_values(piece["nodes_per_dim"]) for piece in info["pieces"]]
        sp = ChebyshevSpline.from_values(vals, d, dom, n, knots)
        out[f"{tag}_shape"] = np.asarray(n, dtype=np.int64)

        def spline_ref(dims, b, p):
            kept_n = d - len(dims)
            ref = np.empty(len(b))
            for r in range(len(b)):
                res = sp.integrate(dims=dims, bounds=[(float(b[r, j, 0]), float(b[r, j, 1])) for j in range(len(dims))])
                ref[r] = res if kept_n == 0 else res.eval([float(v) for v in p[r]], [0] * kept_n)
            return ref

        for i, dims in enumerate(groups):
            for seed in range(200):
                rng = np.random.default_rng([1000 + sum(n), i, seed])
                b, p = spline_group_rows(rng, dom, knots, dims)
                ref = spline_ref(dims, b, p)
                if share(ref) >= MIN_SHARE:
                    break
            assert share(ref) >= MIN_SHARE, (tag, dims, share(ref))
            assert ref[1] == 0.0, (tag, dims, ref[1])
            out[f"{tag}_box{i}"] = join_group(b, p, ref)
            print(f"{tag} box{i} dims={dims} seed={seed} share={share(ref):.3f} max|ref|={np.max(np.abs(ref)):.4g}")
        rng = np.random.default_rng([1000 + sum(n), 99])
        sb = sub_box(rng, dom)
        out[f"{tag}_int"] = np.vstack([[sp.integrate(), sp.integrate(bounds=[(float(lo), float(hi)) for lo, hi in sb])], sb])
        for i, (dims, bnds) in enumerate(SPLINE_PARTIALS[tag]):
            res = sp.integrate(dims=dims, bounds=bnds)
            kept = [k for k in range(d) if k not in dims]
            out[f"{tag}_part{i}_domain"] = np.asarray(res.domain, dtype=float)
            for k in range(len(kept)):
                out[f"{tag}_part{i}_knots{k}"] = np.asarray(res.knots[k], dtype=float)
            for j, piece in enumerate(res._pieces):
                out[f"{tag}_part{i}_piece{j}"] = np.asarray(piece.tensor_values, dtype=float)
            rng = np.random.default_rng([1000 + sum(n), 50 + i])
            _, pts = spline_group_rows(rng, dom, knots, dims)
            out[f"{tag}_part{i}_eval"] = np.column_stack([pts, [res.eval([float(v) for v in q], [0] * len(kept)) for q in pts]])

    path = os.path.join(HERE, "g24_bary_box.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
