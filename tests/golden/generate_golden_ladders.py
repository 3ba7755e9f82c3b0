#!/usr/bin/env python3
"""Generate tests/golden/g34_ladders.npz: ladders -- for every row of a batch, the model along one dimension at m values,
what ``ladder_batch`` computes -- by the reference's pointwise rule, ``ChebyshevApproximation.vectorized_eval`` (with the
spec) and ``ChebyshevTT.eval`` at EVERY ``(fixed..., x)`` point.

Run in the build container only (the reference checkout does not travel to the GPU box):

    python tests/golden/generate_golden_ladders.py --ref <reference checkout>

It imports PyChebyshev v0.21.1 from ``<ref>/src`` and stores arrays only.

Dense cases (DENSE below): functions of tests/golden/functions.py; per (case, dim, spec) one batch of ROWS rows with a
shared ``xs`` of ``m`` values and the first ROWS_PER_ROW rows again with values of their own.  The tests take the batch
sizes 1, 15, 16, 17, 100 and the ladder lengths 1, 16, 17, 33 as leading slices of these (a row's ladder depends on
neither), so the features sit in front: rows 0 .. 7 of a batch hold, in a fixed dimension that rotates with the row, the
lower domain end, the upper end, an exact node and a value 5e-15 from a node (inside the reference's 1e-14 one-hot
window), the other rows are interior; the first 16 values of an ``xs`` hold interior points, both ends, two exact nodes,
one value 5e-15 from a node, a repeated value and two values 10 % of the width outside the domain, in a non-monotone
order.  bs_5d carries the specs value, [1,0,0,0,0], [2,0,0,0,0] and [0,0,0,1,0] along each of its five dimensions.

TT cases: models A and C of g22_tt_transforms.npz (C with the order TT_C_ORDER, as generate_golden_eval_grid.py
gives it) run on the lane-per-row kernel; its model F (ranks 20 and 17, 20 nodes) and model G -- synthetic cores by
g5's recipe with a rank of 18 and a dimension of 18 nodes -- have no lane-per-point image and run on the wave-per-row
kernel.  ``dim`` is the first, a middle and the
last user dimension.

What a golden value is worth: as generate_golden_eval_grid.py says.  Every stored ladder is checked here against the
same rule in ``np.longdouble``, cell by cell, and a value is USABLE only when the reference is within REF_SHARE = 1/2
of both bounds the tests use (1e-12 normwise, spec_point_tol pointwise) AND, outside the domain, the rounding any FP64
evaluation of the last sum carries, n 2^-53 sum |term|, is within that share too (usable_cells).  Every value inside the domain must be
usable, else the case is not stored; it may name ``alternatives`` (function, domain).  Outside the domain the sum is
conditioned like |T_n(1.2)| = cosh(n acosh 1.2) at 10 % of the width (40 at n = 7, 4.7e2 at n = 11, 2e4 at n = 17,
4e8 at n = 33, 1e17 at n = 64): on the longer dimensions two FP64 summation orders differ there by more than the
bounds and the reference's value is no yardstick.  Those values stay in ``xs`` (the kernels run them) and their
reference values are stored, with masks that say which the tests compare: ``..._refok`` (m,) by column for the shared
values, ``..._refrowok`` by cell for the per-row ones.  What was dropped is printed.

Keys:  dense  d<i>_n, d<i>_domain, d<i>_tensor, d<i>_dims, d<i>_nspec, d<i>_s<j>_spec,
              d<i>_k<dim>_fixed (ROWS, d-1), d<i>_k<dim>_xs (m,), d<i>_k<dim>_xsrow (ROWS_PER_ROW, m),
              d<i>_k<dim>_s<j>_ref (ROWS, m), d<i>_k<dim>_s<j>_refrow (ROWS_PER_ROW, m), ..._refok, ..._refrowok
       TT     t<M>_order, t<M>_dims, t<M>_k<dim>_fixed / _xs / _xsrow / _ref / _refrow / _refok / _refrowok; tG_core<k>, tG_domain
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import functions as F  # noqa: E402

BS_SPECS = [[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [2, 0, 0, 0, 0], [0, 0, 0, 1, 0]]
DENSE = [
    dict(f="sin_sum_nd", n=(3,), dims=[0], m=33, domain=[[-1.0, 1.0]]),
    dict(f="sin_cos_2d", n=(5, 7), dims=[0, 1], m=33, domain=[[-1.0, 1.0], [0.0, 2.0]]),
    dict(f="exp_mix_3d", n=(4, 11, 6), dims=[0, 1, 2], m=33, domain=[[-1.0, 1.0], [0.5, 2.0], [-0.5, 1.5]]),
    dict(f="exp_mix_3d", n=(17, 3, 2), dims=[0], m=33, domain=[[-1.0, 1.0], [0.5, 2.0], [-0.5, 1.5]]),
    dict(f="sin_cos_2d", n=(33, 2), dims=[0], m=33, domain=[[-1.0, 1.0], [0.0, 2.0]]),
    dict(f="sin_cos_2d", n=(64, 5), dims=[0], m=33, domain=[[-1.0, 1.0], [0.0, 2.0]]),
    dict(f="exp_mix_3d", n=(12, 12, 12), dims=[1], m=33, domain=[[-2.0, 2.0]] * 3),
    dict(f="bs_5d", n=(3, 4, 5, 3, 4), dims=[0, 1, 2, 3, 4], m=17, domain=F.BS5_DOMAIN, specs=BS_SPECS),
]
TT_C_ORDER = [2, 0, 4, 1, 3]
TT_M = 17
TT_G = dict(n=[5, 18, 6, 4], ranks=[1, 4, 18, 5, 1], domain=[[-1.0, 1.0], [0.0, 2.0], [0.5, 1.5], [-2.0, 0.0]], order=[0, 1, 2, 3])
ROWS = 100
ROWS_PER_ROW = 17
REF_SHARE = 0.5
LD = np.longdouble


def point_tol(spec):
    """spec_point_tol of tests/conftest.py"""
    return 1e-12 * 10.0 ** min(sum(abs(int(v)) for v in spec), 3)


def usable_cells(ref, ld, absum, n, ptol, inside):
    """Cell by cell: is the reference's value a yardstick at REF_SHARE of both bounds?  The measured condition: the
    reference is that close to the long-double value.  Outside the domain a structural one as well, from the number
    format: the last sum of the rule has n terms that grow and cancel there, so ANY FP64 evaluation of it carries up to
    n 2^-53 sum |term| of rounding -- where that alone exceeds the share, agreement of the reference is luck and a second
    FP64 route need not repeat it.  (Inside the domain the terms do not cancel beyond the Lebesgue constant and the
    worst-case bound is far above what any route shows: the measured condition alone, as generate_golden_eval_grid.py.)
    absum = sum |term| (long double).  The scale is that of the cells inside the domain.  Returns (mask, all cells inside the domain usable)."""
    ld, absum = np.asarray(ld, dtype=LD), np.asarray(absum, dtype=LD)
    inside = np.broadcast_to(inside, ld.shape)
    scale = np.max(np.abs(ld[inside]))
    err = np.abs(np.asarray(ref, dtype=LD) - ld)
    err = np.where(inside, err, np.maximum(err, n * LD(2.0) ** -53 * absum))
    big = np.abs(ld) >= 1e-3 * scale
    ok = err <= REF_SHARE * 1e-12 * scale
    ok &= ~big | (err <= REF_SHARE * ptol * np.abs(ld))
    return np.asarray(ok, dtype=bool), bool(ok[inside].all())


def make_rows(rng, domain, nodes, others, rows):
    """`rows` rows over the dimensions `others`: interior, with the features of the module docstring in rows 0 .. 7"""
    out = np.empty((rows, len(others)))
    for c, k in enumerate(others):
        lo, hi = domain[k]
        out[:, c] = rng.uniform(lo + 0.02 * (hi - lo), hi - 0.02 * (hi - lo), rows)
    for r in range(min(rows, 8)):
        if not others:
            break
        c = (r // 4 + r) % len(others)
        k = others[c]
        lo, hi = domain[k]
        nd = np.asarray(nodes[k], dtype=float)
        out[r, c] = [lo, hi, nd[(1 + r) % nd.size], nd[(2 + r) % nd.size] + 5e-15][r % 4]
    return out


def make_xs(rng, lo, hi, nodes, m, shift=0):
    """m values along the ladder's dimension: the feature list within the first 16, in a non-monotone order"""
    nd = np.asarray(nodes, dtype=float)
    n = nd.size
    w = hi - lo
    inner = rng.uniform(lo, hi, 3)
    feats = [inner[0], lo, nd[(1 + shift) % n], hi, nd[(2 + shift) % n] + 5e-15, nd[(n // 2 + shift) % n], inner[0], inner[1],
             lo - 0.1 * w, hi + 0.1 * w, inner[2]]
    head = np.array(feats + list(rng.uniform(lo, hi, 16 - len(feats))), dtype=float)
    head = head[rng.permutation(16)]
    if np.all(np.diff(head) >= 0):
        head = head[::-1].copy()
    xs = np.concatenate([head, rng.uniform(lo, hi, max(0, m - 16))])
    return xs[:m].copy() if m <= 16 else xs


def bary_rows_ld(nodes, xs):
    """(len(xs), n) long-double barycentric rows: one-hot within 1e-14 of a node (the FP64 test the reference makes)"""
    x = np.asarray(nodes, dtype=LD)
    n = x.size
    w = np.ones(n, dtype=LD)
    for j in range(n):
        keep = np.arange(n) != j
        w[keep] /= (x[keep] - x[j])
    rows = np.zeros((len(xs), n), dtype=LD)
    for r, xv in enumerate(xs):
        exact = np.where(np.abs(np.float64(xv) - np.asarray(nodes, dtype=float)) < 1e-14)[0]
        if len(exact):
            rows[r, exact[0]] = 1
        else:
            diff = LD(xv) - x
            rows[r] = (w / diff) / np.sum(w / diff)
    return rows, w


def derived_ld(tensor, nodes, spec):
    cur = np.asarray(tensor, dtype=LD)
    for k in range(cur.ndim):
        if not spec[k]:
            continue
        x = np.asarray(nodes[k], dtype=LD)
        _, w = bary_rows_ld(nodes[k], [])
        gap = x[:, None] - x[None, :]
        np.fill_diagonal(gap, LD(1))
        D = w[None, :] / (gap * w[:, None])
        np.fill_diagonal(D, LD(0))
        np.fill_diagonal(D, -D.sum(axis=1))
        for _ in range(int(spec[k])):
            cur = np.moveaxis(np.tensordot(D, cur, axes=([1], [k])), 0, k)
    return cur


def ladder_ld(cur, nodes, dim, fixed, xs):
    """The pointwise rule in long double on the derived tensor `cur`: per row the weights of the fixed dimensions, then
    of its values along dim.  xs is (m,) or (rows, m).  Returns the values and, per value, the sum of |terms| of the last sum."""
    d = cur.ndim
    others = [k for k in range(d) if k != dim]
    out = np.empty((fixed.shape[0], np.shape(xs)[-1]), dtype=LD)
    absum = np.empty_like(out)
    for r in range(fixed.shape[0]):
        fib = np.moveaxis(cur, dim, 0)
        for c in reversed(range(len(others))):
            wr, _ = bary_rows_ld(nodes[others[c]], [fixed[r, c]])
            fib = np.tensordot(fib, wr[0], axes=([fib.ndim - 1], [0]))
        xr = xs if np.ndim(xs) == 1 else xs[r]
        wx, _ = bary_rows_ld(nodes[dim], xr)
        out[r] = wx @ fib
        absum[r] = np.abs(wx) @ np.abs(fib)
    return out, absum


def tt_ladder_ld(cores, domain, order, dim, fixed, xs):
    """ChebyshevTT.eval in long double at the points of a ladder batch (dim, fixed, xs in the user's frame): the chains
    on both sides of dim's core give the n coefficients of the row's restriction, the values are that series.  Returns
    the values and, per value, the sum of |c_i T_i|."""
    d = len(cores)
    p = list(order).index(dim)

    def basis(k, x):
        a, b = domain[k]
        s = LD(2) * (LD(x) - LD(a)) / (LD(b) - LD(a)) - LD(1)
        n = cores[k].shape[1]
        T = np.empty(n, dtype=LD)
        T[0] = 1
        if n > 1:
            T[1] = s
        for j in range(2, n):
            T[j] = 2 * s * T[j - 1] - T[j - 2]
        return T

    out = np.empty((fixed.shape[0], np.shape(xs)[-1]), dtype=LD)
    absum = np.empty_like(out)
    for r in range(fixed.shape[0]):
        coord = {u: fixed[r, u if u < dim else u - 1] for u in range(d) if u != dim}
        L = np.ones(1, dtype=LD)
        for k in range(p):
            L = L @ np.tensordot(np.asarray(cores[k], dtype=LD), basis(k, coord[order[k]]), axes=([1], [0]))
        R = np.ones(1, dtype=LD)
        for k in range(d - 1, p, -1):
            R = np.tensordot(np.asarray(cores[k], dtype=LD), basis(k, coord[order[k]]), axes=([1], [0])) @ R
        c = np.tensordot(np.tensordot(L, np.asarray(cores[p], dtype=LD), axes=([0], [0])), R, axes=([1], [0]))
        xr = xs if np.ndim(xs) == 1 else xs[r]
        for i, x in enumerate(xr):
            T = basis(p, x)
            out[r, i] = c @ T
            absum[r, i] = np.abs(c) @ np.abs(T)
    return out, absum


def expand(d, dim, fixed, xs):
    """(rows * m, d) points of a ladder batch, row by row"""
    rows, m = fixed.shape[0], np.shape(xs)[-1]
    pts = np.empty((rows, m, d))
    others = [k for k in range(d) if k != dim]
    for c, k in enumerate(others):
        pts[:, :, k] = fixed[:, c][:, None]
    pts[:, :, dim] = xs[None, :] if np.ndim(xs) == 1 else xs
    return pts.reshape(rows * m, d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of PyChebyshev v0.21.1")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.ref, "src"))
    import pychebyshev as ref
    from pychebyshev import ChebyshevApproximation, ChebyshevTT

    print("reference version", ref.__version__, " long double eps", np.finfo(LD).eps)
    assert np.finfo(LD).eps < 1e-18, "np.longdouble carries no more than float64 on this machine"
    out = {}
    dropped = []

    def dense_case(i, c, fname, domain):
        d = len(c["n"])
        model = ChebyshevApproximation(getattr(F, fname), d, [list(b) for b in domain], list(c["n"]), max_derivative_order=2)
        model.build(verbose=False)
        nodes = [np.asarray(x, dtype=float) for x in model.nodes]
        specs = c.get("specs", [[0] * d])
        pre = f"d{i}"
        got = {f"{pre}_n": np.array(c["n"], dtype=np.int64), f"{pre}_domain": np.array(domain, dtype=float),
               f"{pre}_tensor": np.asarray(model.tensor_values, dtype=float), f"{pre}_dims": np.array(c["dims"], dtype=np.int64),
               f"{pre}_nspec": np.array(len(specs), dtype=np.int64)}
        for j, spec in enumerate(specs):
            got[f"{pre}_s{j}_spec"] = np.array(spec, dtype=np.int64)
        derived = [derived_ld(model.tensor_values, nodes, spec) for spec in specs]
        for dim in c["dims"]:
            rng = np.random.default_rng(3400 + 16 * i + dim)
            others = [k for k in range(d) if k != dim]
            fixed = make_rows(rng, domain, nodes, others, ROWS)
            lo, hi = domain[dim]
            xs = make_xs(rng, lo, hi, nodes[dim], c["m"], dim)
            xsrow = np.stack([make_xs(rng, lo, hi, nodes[dim], c["m"], dim + r) for r in range(ROWS_PER_ROW)])
            key = f"{pre}_k{dim}"
            got[f"{key}_fixed"], got[f"{key}_xs"], got[f"{key}_xsrow"] = fixed, xs, xsrow
            for j, spec in enumerate(specs):
                for tag, f_, x_ in (("ref", fixed, xs), ("refrow", fixed[:ROWS_PER_ROW], xsrow)):
                    pts = expand(d, dim, f_, x_)
                    res = np.array([model.vectorized_eval([float(v) for v in p], list(spec)) for p in pts]).reshape(f_.shape[0], -1)
                    inside = (np.asarray(x_) >= lo) & (np.asarray(x_) <= hi)
                    ld, absum = ladder_ld(derived[j], nodes, dim, f_, x_)
                    cells, ok = usable_cells(res, ld, absum, c["n"][dim], point_tol(spec), inside)
                    mask = cells.all(axis=0) if tag == "ref" else cells
                    print(f"  d{i} {fname} n={c['n']} dim {dim} {spec} {tag}: {int(mask.size - mask.sum())} of {mask.size} "
                          f"{'columns' if tag == 'ref' else 'cells'} dropped (all outside the domain){'' if ok else '  -- a value INSIDE the domain fails: NOT usable'}")
                    if not ok:
                        return None
                    got[f"{key}_s{j}_{tag}ok"] = mask
                    got[f"{key}_s{j}_{tag}"] = res
        return got

    for i, c in enumerate(DENSE):
        for fname, domain in [(c["f"], c["domain"])] + list(c.get("alternatives", [])):
            got = dense_case(i, c, fname, domain)
            if got is not None:
                out.update(got)
                print(f"d{i}: stored {fname} n={c['n']} on {domain}")
                break
            dropped.append(f"d{i} {fname} on {domain}")
        else:
            raise SystemExit(f"d{i}: no choice of function passes the reference's own error check")

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
        obj._dim_order = list(order)
        return obj

    G = np.load(os.path.join(HERE, "g22_tt_transforms.npz"))
    models = {}
    for tag in ("A", "C", "F"):
        cores, k = [], 0
        while f"{tag}_core{k}" in G.files:
            cores.append(G[f"{tag}_core{k}"])
            k += 1
        models[tag] = (cores, G[f"{tag}_domain"].tolist(), TT_C_ORDER if tag == "C" else G[f"{tag}_order"].tolist())
    rng = np.random.default_rng(3416)
    gn, gr = TT_G["n"], TT_G["ranks"]
    gcores = [rng.standard_normal((gr[k], gn[k], gr[k + 1])) / np.sqrt(gr[k] * gn[k]) for k in range(len(gn))]
    models["G"] = (gcores, TT_G["domain"], TT_G["order"])
    for k, core in enumerate(gcores):
        out[f"tG_core{k}"] = core
    out["tG_domain"] = np.array(TT_G["domain"], dtype=float)

    for tag, (cores, domain, order) in models.items():
        d = len(cores)
        n = [c.shape[1] for c in cores]
        tt = make_tt(cores, domain, order)
        udom = [domain[order.index(u)] for u in range(d)]
        unodes = []
        for u in range(d):
            (a, b), nu = udom[u], n[order.index(u)]
            unodes.append(np.sort(0.5 * (a + b) + 0.5 * (b - a) * np.cos(np.pi * (2 * np.arange(nu) + 1) / (2 * nu))))
        dims = sorted({0, d // 2, d - 1})
        out[f"t{tag}_order"] = np.array(order, dtype=np.int64)
        out[f"t{tag}_dims"] = np.array(dims, dtype=np.int64)
        for dim in dims:
            rng = np.random.default_rng(3450 + 16 * ord(tag) + dim)
            others = [u for u in range(d) if u != dim]
            fixed = make_rows(rng, udom, unodes, others, ROWS)
            lo, hi = udom[dim]
            xs = make_xs(rng, lo, hi, unodes[dim], TT_M, dim)
            xsrow = np.stack([make_xs(rng, lo, hi, unodes[dim], TT_M, dim + r) for r in range(ROWS_PER_ROW)])
            key = f"t{tag}_k{dim}"
            out[f"{key}_fixed"], out[f"{key}_xs"], out[f"{key}_xsrow"] = fixed, xs, xsrow
            for name, f_, x_ in (("ref", fixed, xs), ("refrow", fixed[:ROWS_PER_ROW], xsrow)):
                pts = expand(d, dim, f_, x_)
                res = np.array([tt.eval([float(v) for v in p]) for p in pts])
                res = res.reshape(f_.shape[0], -1)
                inside = (np.asarray(x_) >= lo) & (np.asarray(x_) <= hi)
                ld, absum = tt_ladder_ld(cores, domain, order, dim, f_, x_)
                cells, ok = usable_cells(res, ld, absum, n[order.index(dim)], 1e-12, inside)
                mask = cells.all(axis=0) if name == "ref" else cells
                print(f"  TT {tag} dim {dim} {name}: {int(mask.size - mask.sum())} of {mask.size} "
                      f"{'columns' if name == 'ref' else 'cells'} dropped (all outside the domain)")
                if not ok:
                    raise SystemExit(f"TT {tag} dim {dim}: the reference misses its share of the bound inside the domain")
                out[f"{key}_{name}ok"] = mask
                out[f"{key}_{name}"] = res.reshape(f_.shape[0], -1)

    print("dropped:", dropped if dropped else "nothing")
    path = os.path.join(HERE, "g34_ladders.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
