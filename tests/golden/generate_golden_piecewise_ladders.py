#!/usr/bin/env python3
"""Generate tests/golden/g35_piecewise_ladders*.npz: ladders of ``ChebyshevSpline`` and ``ChebyshevSlider`` -- for every
row of a batch, the model along one dimension at m values, what their ``ladder_batch`` computes -- by the reference's
pointwise rules: ``ChebyshevSpline.eval_batch`` on the expanded points (spline.py:633-700: a coordinate on a knot belongs
to the right-hand piece, one outside the domain to the end piece, no knot check for derivative specs) and
``ChebyshevSlider.eval`` (slider.py:284-318) looped over EVERY ``(fixed..., x)`` point.

Run in the build container only (the reference checkout does not travel to the GPU box):

    python tests/golden/generate_golden_piecewise_ladders.py --ref <reference checkout>

It imports PyChebyshev v0.21.1 from ``<ref>/src`` and stores arrays only.  The models are the cases o, k, z, m of
generate_golden_spline_transforms.py and a, b, c, l of generate_golden_slider_calculus.py (their case tables and ``build``
are imported, so the tests build the same models with this package's classes), along every dimension, with the value
spec and the derivative specs generate_golden_piecewise_grid.py uses for the case (``SPLINE_SPECS``, ``SLIDER_SPECS``; case
l, which has no grid, carries the values).  ``make_rows``, ``make_xs``, ``usable_cells`` and the long-double rule are
those of generate_golden_ladders.py: ROWS rows with a shared ``xs`` of m values (33; 17 on the 5-D case b, as there) and
the first ROWS_PER_ROW rows again with values of their own.  On top of ``make_rows``' features in rows 0 .. 7, rows 8 ..
hold, per fixed dimension, the lower and upper domain end, an exact node, a value 5e-15 from a node and every knot, each
in a row of its own; positions 16 .. of every ``xs`` hold the knots of ``dim``.

Every stored value is checked in ``np.longdouble`` with ``usable_cells``: the reference must be within REF_SHARE = 1/2 of
both bounds the tests use (1e-12 normwise, spec_point_tol pointwise); cells outside the domain are masked where the
rounding of the last sum alone exceeds that share (``..._refok`` by column for the shared values, ``..._refrowok`` by cell
for the per-row ones).  A case in which a cell inside the domain fails stops the generator.  No spec whose exact result is
identically zero is stored: case c's [1, 0, 1, 0] is asserted to be all ``+0.0`` here and in the tests.

The arrays of all cases together exceed what one committed file may hold, so they go into three files (``FILES``): the
3-D spline m and the 4-D slider c have one each.

Keys:  spline case c   s<c>_k<dim>_fixed (ROWS, d-1), _xs (m,), _xsrow (ROWS_PER_ROW, m),
                       s<c>_k<dim>_s<j>_ref / _refok / _refrow / _refrowok  (spec j of SPLINE_SPECS[c])
       slider case c   l<c>_k<dim>_...  the same with SLIDER_SPECS[c]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import generate_golden_ladders as LG  # noqa: E402
import generate_golden_piecewise_grid as PG  # noqa: E402
import generate_golden_slider_calculus as SL  # noqa: E402
import generate_golden_spline_transforms as SP  # noqa: E402

LD = np.longdouble
SEED = 3500
ROWS, ROWS_PER_ROW = LG.ROWS, LG.ROWS_PER_ROW
SPLINE_CASES = ["o", "k", "z", "m"]
SLIDER_CASES = ["a", "b", "c", "l"]


def _grid_specs(grids, case, d):
    specs = [[0] * d]
    for g in grids:
        if g["case"] == case:
            specs += [list(s) for s in g["specs"] if list(s) not in specs]
    return specs


SPLINE_SPECS = {c: _grid_specs(PG.SPLINE_GRIDS, c, SP.CASES[c]["d"]) for c in SPLINE_CASES}
SLIDER_SPECS = {c: _grid_specs(PG.SLIDER_GRIDS, c, SL.CASES[c]["d"]) for c in SLIDER_CASES}
SLIDER_ZERO = PG.SLIDER_ZERO
M = {"b": 17}                                # ladder lengths other than 33
FILES = {"g35_piecewise_ladders": ["so", "sk", "sz", "la", "lb", "ll"], "g35_piecewise_ladders_m": ["sm"],
         "g35_piecewise_ladders_c": ["lc"]}


def file_of(tag: str) -> str:
    """The golden file that holds the arrays of ``tag`` (``s<case>`` / ``l<case>``)"""
    return next(name for name, tags in FILES.items() if tag in tags)


def ladder_m(case: str) -> int:
    return M.get(case, 33)


def add_features(fixed, domain, nodes, knots, others):
    """Rows 8 .. of ``fixed``: per fixed dimension its lower end, upper end, an exact node, a value 5e-15 from a node and
    every knot, each in a row of its own (the other columns stay interior)"""
    r = 8
    for c, k in enumerate(others):
        lo, hi = domain[k]
        nd = np.asarray(nodes[k], dtype=float)
        for v in [lo, hi, nd[(3 + c) % nd.size], nd[(5 + c) % nd.size] + 5e-15] + list(knots[k]):
            fixed[r, c] = v
            r += 1
    assert r <= fixed.shape[0]
    return fixed


def add_knots(xs, knots):
    """The knots of dim at positions 16 .. of a ladder's values (the last axis)"""
    for i, v in enumerate(knots):
        xs[..., 16 + i] = v
    return xs


def batch(seed, domain, nodes, knots, dim, m):
    """(fixed, xs, xsrow) of one (case, dim)"""
    d = len(domain)
    rng = np.random.default_rng(seed)
    others = [k for k in range(d) if k != dim]
    fixed = add_features(LG.make_rows(rng, domain, nodes, others, ROWS), domain, nodes, knots, others)
    lo, hi = domain[dim]
    xs = add_knots(LG.make_xs(rng, lo, hi, nodes[dim], m, dim), knots[dim])
    xsrow = add_knots(np.stack([LG.make_xs(rng, lo, hi, nodes[dim], m, dim + r) for r in range(ROWS_PER_ROW)]), knots[dim])
    return fixed, xs, xsrow


def spline_nodes(sp, k):
    """The nodes of the pieces along dimension k (index 0 in every other dimension), concatenated"""
    stride = int(np.prod(sp._shape[k + 1:], dtype=int))
    return np.concatenate([np.asarray(sp._pieces[j * stride].nodes[k], dtype=float) for j in range(sp._shape[k])])


def spline_ld(sp, derived, dim, fixed, xs):
    """The spline's ladders in long double: per cell the piece by PG.route, then generate_golden_ladders.ladder_ld on that
    piece's derived tensor.  Returns the values, the sum of |terms| of the last sum and the node count of that sum."""
    d = sp.num_dimensions
    others = [k for k in range(d) if k != dim]
    rows, m = fixed.shape[0], np.shape(xs)[-1]
    out, absum, n = np.empty((rows, m), dtype=LD), np.empty((rows, m), dtype=LD), np.empty((rows, m))
    sec = [PG.route(sp.knots[k], sp._shape[k], fixed[:, c]) for c, k in enumerate(others)]
    for r in range(rows):
        xr = np.asarray(xs if np.ndim(xs) == 1 else xs[r], dtype=float)
        along = PG.route(sp.knots[dim], sp._shape[dim], xr)
        for j in np.unique(along):
            multi = [0] * d
            for c, k in enumerate(others):
                multi[k] = int(sec[c][r])
            multi[dim] = int(j)
            flat = int(np.ravel_multi_index(multi, sp._shape))
            piece = sp._pieces[flat]
            pos = np.flatnonzero(along == j)
            v, a = LG.ladder_ld(derived[flat], [np.asarray(x, dtype=float) for x in piece.nodes], dim, fixed[r:r + 1], xr[pos])
            out[r, pos], absum[r, pos], n[r, pos] = v[0], a[0], piece.n_nodes[dim]
    return out, absum, n


def slider_ld(sl, derived, spec, dim, fixed, xs):
    """The slider's ladders in long double, ``eval``'s rule: the owner slide's ladder, every other slide's value at the
    row, summed in slide order; a derivative inside one slide is that slide alone.  ``derived[s]``: slide s's tensor
    under its part of the spec."""
    d = sl.num_dimensions
    rows, m = fixed.shape[0], np.shape(xs)[-1]
    col = {k: (k if k < dim else k - 1) for k in range(d) if k != dim}
    o = next(s for s, group in enumerate(sl.partition) if dim in group)
    active = sorted({s for s, group in enumerate(sl.partition) for k in group if spec[k] > 0})
    assert len(active) < 2

    def slide(s):
        group = list(sl.partition[s])
        nodes = [np.asarray(x, dtype=float) for x in sl.slides[s].nodes]
        if s == o:
            lk = group.index(dim)
            f = np.column_stack([fixed[:, col[k]] for k in group if k != dim]) if len(group) > 1 else np.empty((rows, 0))
            v, a = LG.ladder_ld(derived[s], nodes, lk, f, xs)
            return v, a, sl.slides[s].n_nodes[lk]
        v, a = np.empty((rows, 1), dtype=LD), np.empty((rows, 1), dtype=LD)
        for r in range(rows):                     # the slide's value at the row: a ladder of one value along its dimension 0
            f = np.array([[fixed[r, col[k]] for k in group[1:]]])
            v[r], a[r] = (t[0] for t in LG.ladder_ld(derived[s], nodes, 0, f, np.array([fixed[r, col[group[0]]]])))
        return np.broadcast_to(v, (rows, m)), np.broadcast_to(a, (rows, m)), sl.slides[s].n_nodes[0]

    if active:
        return slide(active[0])
    res = np.full((rows, m), LD(sl.pivot_value), dtype=LD)
    own = None
    for s in range(len(sl.partition)):
        v, a, n = slide(s)
        res = res + (v - LD(sl.pivot_value))
        if s == o:
            own = (a, n)
    return res, own[0], own[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of PyChebyshev v0.21.1")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.ref, "src"))
    import pychebyshev as ref
    from pychebyshev import ChebyshevSlider, ChebyshevSpline

    print("reference version", ref.__version__, " long double eps", np.finfo(LD).eps)
    assert np.finfo(LD).eps < 1e-18, "np.longdouble carries no more than float64 on this machine"
    out = {name: {} for name in FILES}

    def check_and_store(dst, key, j, spec, tag, res, ld, absum, n, x_, lo, hi):
        inside = (np.asarray(x_) >= lo) & (np.asarray(x_) <= hi)
        assert float(np.max(np.abs(np.asarray(ld, dtype=float)))) > 0.0, (key, spec, "identically zero")
        cells, ok = LG.usable_cells(res, ld, absum, n, LG.point_tol(spec), inside)
        mask = cells.all(axis=0) if tag == "ref" else cells
        print(f"  {key} {spec} {tag}: {int(mask.size - mask.sum())} of {mask.size} {'columns' if tag == 'ref' else 'cells'} dropped"
              f" (all outside the domain)")
        if not ok:
            raise SystemExit(f"{key} {spec} {tag}: the reference misses its share of the bounds inside the domain")
        dst[f"{key}_s{j}_{tag}ok"] = mask
        dst[f"{key}_s{j}_{tag}"] = res

    for ci, case in enumerate(SPLINE_CASES):
        c = SP.CASES[case]
        d = c["d"]
        sp = SP.build(ChebyshevSpline, case)
        dst = out[file_of("s" + case)]
        nodes = [spline_nodes(sp, k) for k in range(d)]
        derived = {tuple(spec): [LG.derived_ld(p.tensor_values, [np.asarray(x, dtype=float) for x in p.nodes], spec)
                                 for p in sp._pieces] for spec in SPLINE_SPECS[case]}
        for dim in range(d):
            fixed, xs, xsrow = batch(SEED + 16 * ci + dim, c["domain"], nodes, c["knots"], dim, ladder_m(case))
            key = f"s{case}_k{dim}"
            dst[f"{key}_fixed"], dst[f"{key}_xs"], dst[f"{key}_xsrow"] = fixed, xs, xsrow
            lo, hi = c["domain"][dim]
            for j, spec in enumerate(SPLINE_SPECS[case]):
                for tag, f_, x_ in (("ref", fixed, xs), ("refrow", fixed[:ROWS_PER_ROW], xsrow)):
                    res = np.asarray(sp.eval_batch(LG.expand(d, dim, f_, x_), list(spec)), dtype=float).reshape(f_.shape[0], -1)
                    ld, absum, n = spline_ld(sp, derived[tuple(spec)], dim, f_, x_)
                    check_and_store(dst, key, j, spec, tag, res, ld, absum, n, x_, lo, hi)

    for ci, case in enumerate(SLIDER_CASES):
        c = SL.CASES[case]
        d = c["d"]
        sl = SL.build(ChebyshevSlider, case)
        dst = out[file_of("l" + case)]
        nodes = []
        for k in range(d):
            s = next(s for s, group in enumerate(sl.partition) if k in group)
            nodes.append(np.asarray(sl.slides[s].nodes[list(sl.partition[s]).index(k)], dtype=float))
        for dim in range(d):
            fixed, xs, xsrow = batch(SEED + 100 + 16 * ci + dim, c["domain"], nodes, [[]] * d, dim, ladder_m(case))
            key = f"l{case}_k{dim}"
            dst[f"{key}_fixed"], dst[f"{key}_xs"], dst[f"{key}_xsrow"] = fixed, xs, xsrow
            lo, hi = c["domain"][dim]
            for j, spec in enumerate(SLIDER_SPECS[case]):
                derived = [LG.derived_ld(s_.tensor_values, [np.asarray(x, dtype=float) for x in s_.nodes], [spec[k] for k in group])
                           for s_, group in zip(sl.slides, sl.partition)]
                for tag, f_, x_ in (("ref", fixed, xs), ("refrow", fixed[:ROWS_PER_ROW], xsrow)):
                    pts = LG.expand(d, dim, f_, x_)
                    res = np.array([sl.eval([float(v) for v in p], list(spec)) for p in pts]).reshape(f_.shape[0], -1)
                    ld, absum, n = slider_ld(sl, derived, spec, dim, f_, x_)
                    check_and_store(dst, key, j, spec, tag, res, ld, absum, n, x_, lo, hi)
            if case in SLIDER_ZERO:
                zero = np.array([sl.eval([float(v) for v in p], SLIDER_ZERO[case]) for p in LG.expand(d, dim, fixed[:ROWS_PER_ROW], xs)])
                assert np.all(zero == 0.0) and not np.any(np.signbit(zero)), "a cross-slide derivative is +0.0 in the reference"

    for name, arrays in out.items():
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path), "bytes,", len(arrays), "arrays")
        assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
