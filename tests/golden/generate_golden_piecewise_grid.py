#!/usr/bin/env python3
"""Generate tests/golden/g32_piecewise_grid.npz: ``ChebyshevSpline`` and ``ChebyshevSlider`` on tensor-product grids, what
their ``eval_grid`` computes, by the reference's pointwise rules -- ``ChebyshevSpline.eval_batch`` on the meshgrid
(spline.py:633-700: a coordinate on a knot belongs to the right-hand piece, one outside the domain to the end piece, no
knot check for derivative specs) and ``ChebyshevSlider.eval`` (slider.py:284-318) looped over EVERY grid point.

Run in the build container only (the reference checkout does not travel to the GPU box):

    python tests/golden/generate_golden_piecewise_grid.py --ref <reference checkout>

It imports PyChebyshev v0.21.1 from ``<ref>/src`` and stores arrays only.  The models are the cases k, m, z, o of
generate_golden_spline_transforms.py and a, b, c of generate_golden_slider_calculus.py (their case tables and ``build``
are imported, so the tests build the same models with this package's classes); ``grid_ld``, ``ref_error``,
``point_tol`` and ``REF_SHARE`` are those of generate_golden_eval_grid.py.  The grids (``SPLINE_GRIDS``,
``SLIDER_GRIDS``) and ``route`` below are imported by the tests.

Every axis mixes interior points, both domain ends, every knot of its dimension, an exact node of a piece, a point 5e-15
from a node (inside the reference's 1e-14 one-hot window), one repeated value and a non-monotone order; where a grid is
marked ``outside`` also one value 1 % of the width outside each end.  An axis too short to hold them all keeps the knots
and takes a slice of the other features that starts at a different one per dimension (with the outside value as the only
coordinate of case m's dimension 1, the reference's [1, 1, 0] is 5.3e-13 from the long-double value: over its share);
the grid (3, 4, 2) of case m has hand-picked axes that leave two of its eight pieces without a point.  Every grid has
fewer than 20,000 points.

Every stored grid is checked against the same rule in ``np.longdouble``: per piece (per slide) ``grid_ld`` on the entries
the piece (the slide) sees, assembled as the planner of csrc/spline_grid_plan.h (the sum kernel) assembles them.  A grid
is stored only when the reference is within REF_SHARE = 1/2 of both bounds of it -- 1e-12 normwise, ``point_tol(spec)``
pointwise; a case that fails stops the generator.  No spec whose exact result is identically zero is stored (a relative
bound on rounding noise tests nothing): case c's [1, 0, 1, 0] is asserted to be all ``+0.0`` here and in the tests, and
case m's [0, 2, 0], [0, 0, 2], [1, 0, 1] and [0, 1, 1] are left out (f_m is linear in dimensions 1 and 2).

Keys:  spline grid i   s<i>_ax<k>, s<i>_r<j> (spec j of SPLINE_GRIDS[i], shape m)
       slider grid i   l<i>_ax<k>, l<i>_r<j> (spec j of SLIDER_GRIDS[i], shape m)
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import generate_golden_eval_grid as EG  # noqa: E402
import generate_golden_slider_calculus as SL  # noqa: E402
import generate_golden_spline_transforms as SP  # noqa: E402

LD = np.longdouble
SEED = 3200
MAX_POINTS = 20000

SPLINE_GRIDS = [
    dict(case="o", m=(12,), outside=True, specs=[[0], [1], [2]]),
    dict(case="k", m=(17, 6), outside=True, specs=[[0, 0], [1, 0], [0, 2], [1, 1]]),
    dict(case="z", m=(5, 18), outside=False, specs=[[0, 0], [0, 1]]),
    dict(case="m", m=(9, 1, 18), outside=True, specs=[[0, 0, 0], [1, 0, 0], [2, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1]]),
    # hand-picked axes: dimension 0 misses its interval [95, 100), so 6 of the 8 pieces are live; 100.0 and 0.2 are knots
    dict(case="m", m=(3, 4, 2), outside=False, specs=[[0, 0, 0]],
         axes=[[100.0, 83.7, 120.0], [0.2, 0.01, 0.13, 0.2], [0.2, 0.17]]),
]
SLIDER_GRIDS = [
    dict(case="a", m=(3, 17, 2), specs=[[0, 0, 0]]),
    dict(case="b", m=(2, 3, 5, 1, 4), specs=[[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [2, 0, 0, 0, 0]]),
    dict(case="c", m=(5, 3, 17, 2), specs=[[0, 0, 0, 0], [1, 0, 0, 0], [1, 1, 0, 0], [0, 0, 2, 0], [0, 0, 1, 1]]),
]
SLIDER_ZERO = {"c": [1, 0, 1, 0]}          # spans two slides: +0.0 everywhere, asserted and not stored


def grid_id(g) -> str:
    return g["case"] + "_" + "x".join(map(str, g["m"]))


def route(knots, shape, axis) -> np.ndarray:
    """The interval of every axis entry: ``searchsorted(knots, x, side='right')`` clipped to the last piece (a NaN sorts
    behind every knot: the last piece)."""
    if len(knots) == 0:
        return np.zeros(len(axis), dtype=np.int64)
    return np.minimum(np.searchsorted(np.asarray(knots, dtype=float), np.asarray(axis, dtype=float), side="right"), shape - 1)


def spline_axis(rng, lo, hi, knots, nodes, m, outside, k):
    """m coordinates for dimension k: the knots and the feature list, filled up with interior points and shuffled into a
    non-monotone order; an axis too short for that keeps the knots and takes a slice of the list that starts at a
    different feature per dimension (generate_golden_eval_grid.make_axis does the same)."""
    w = hi - lo
    inner = rng.uniform(lo, hi, 3)
    n = len(nodes)
    rest = ([lo - 0.01 * w, hi + 0.01 * w] if outside else [])
    rest += [lo, hi, nodes[n // 2], nodes[(n // 3) % n] + 5e-15, inner[0], inner[0], inner[1], inner[2]]   # inner[0] twice
    feats = list(knots) + rest
    if m <= len(feats):
        r = (2 * k) % len(rest)
        ax = np.array((list(knots) + rest[r:] + rest[:r])[:m], dtype=float)
    else:
        ax = np.array(feats + list(rng.uniform(lo, hi, m - len(feats))), dtype=float)
        ax = ax[rng.permutation(m)]
    if m > 2 and np.all(np.diff(ax) >= 0):
        ax = ax[::-1].copy()
    return ax


def spline_ld(sp, axes, spec):
    """The spline's grid in long double, assembled as the planner assembles it: per live piece ``grid_ld`` on the entries
    of its intervals (ascending position), placed with ``np.ix_``."""
    d = sp.num_dimensions
    iv = [route(sp.knots[k], sp._shape[k], axes[k]) for k in range(d)]
    out = np.full(tuple(len(a) for a in axes), np.nan, dtype=LD)
    for multi in np.ndindex(*sp._shape):
        pos = [np.flatnonzero(iv[k] == multi[k]) for k in range(d)]
        if any(p.size == 0 for p in pos):
            continue
        piece = sp._pieces[int(np.ravel_multi_index(multi, sp._shape))]
        out[np.ix_(*pos)] = EG.grid_ld(piece.tensor_values, piece.nodes, [np.asarray(axes[k])[pos[k]] for k in range(d)], spec)
    assert not np.any(np.isnan(out)), "the pieces' blocks do not tile the grid"
    return out


def slider_ld(sl, axes, spec):
    """The slider's grid in long double: per slide ``grid_ld`` on the axes of its group, broadcast and summed in ``eval``'s
    order; a derivative inside one slide is that slide's grid, broadcast."""
    d = sl.num_dimensions
    shape = tuple(len(a) for a in axes)

    def spread(s, sub):
        group = sl.partition[s]
        g = EG.grid_ld(sl.slides[s].tensor_values, sl.slides[s].nodes, [axes[k] for k in group], sub)
        order = np.argsort(group)                       # the group's dimensions in the result's order
        view = [1] * d
        for k in group:
            view[k] = shape[k]
        return np.broadcast_to(np.transpose(g, order).reshape(view), shape)

    active = sorted({s for s, group in enumerate(sl.partition) for k in group if spec[k] > 0})
    assert len(active) < 2
    if active:
        return np.array(spread(active[0], [spec[k] for k in sl.partition[active[0]]]), dtype=LD)
    res = np.full(shape, LD(sl.pivot_value), dtype=LD)
    for s, group in enumerate(sl.partition):
        res = res + (spread(s, [0] * len(group)) - LD(sl.pivot_value))
    return res


def usable(tag, spec, ref, ld):
    e_norm, e_point = EG.ref_error(ref, ld)
    ok = e_norm <= EG.REF_SHARE * 1e-12 and e_point <= EG.REF_SHARE * EG.point_tol(spec)
    print(f"  {tag} {spec}: reference vs long double E_norm {e_norm:.2e} E_point {e_point:.2e}{'' if ok else '  -- NOT usable'}")
    if not ok:
        raise SystemExit(f"{tag} {spec}: the reference misses its share of the bounds")
    assert float(np.max(np.abs(np.asarray(ld, dtype=float)))) > 0.0, (tag, spec, "identically zero")


def mesh(axes):
    return np.column_stack([g.ravel() for g in np.meshgrid(*axes, indexing="ij")])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of PyChebyshev v0.21.1")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.ref, "src"))
    import pychebyshev as ref
    from pychebyshev import ChebyshevSlider, ChebyshevSpline

    print("reference version", ref.__version__, " long double eps", np.finfo(LD).eps)
    assert np.finfo(LD).eps < 1e-18, "np.longdouble carries no more than float64 on this machine"
    out = {}
    splines = {}
    for i, g in enumerate(SPLINE_GRIDS):
        case, m = g["case"], g["m"]
        c = SP.CASES[case]
        sp = splines.setdefault(case, SP.build(ChebyshevSpline, case))
        d = c["d"]
        assert int(np.prod(m)) < MAX_POINTS and len(m) == d
        rng = np.random.default_rng(SEED + i)
        if "axes" in g:
            axes = [np.array(a, dtype=float) for a in g["axes"]]
        else:
            axes = []
            for k in range(d):
                multi = [0] * d
                multi[k] = k % sp._shape[k]
                piece = sp._pieces[int(np.ravel_multi_index(multi, sp._shape))]
                axes.append(spline_axis(rng, c["domain"][k][0], c["domain"][k][1], c["knots"][k], np.asarray(piece.nodes[k]), m[k],
                                        g["outside"], k))
        assert tuple(a.size for a in axes) == tuple(m)
        live = int(np.prod([np.unique(route(sp.knots[k], sp._shape[k], axes[k])).size for k in range(d)]))
        for k in range(d):
            out[f"s{i}_ax{k}"] = axes[k]
        pts = mesh(axes)
        for j, spec in enumerate(g["specs"]):
            res = np.asarray(sp.eval_batch(pts, list(spec)), dtype=float).reshape(m)
            usable(f"spline {grid_id(g)}", spec, res, spline_ld(sp, axes, spec))
            out[f"s{i}_r{j}"] = res
        print(f"spline {grid_id(g)}: {int(np.prod(m))} points, {live} of {len(sp._pieces)} pieces live, {len(g['specs'])} specs")

    sliders = {}
    for i, g in enumerate(SLIDER_GRIDS):
        case, m = g["case"], g["m"]
        c = SL.CASES[case]
        sl = sliders.setdefault(case, SL.build(ChebyshevSlider, case))
        d = c["d"]
        assert int(np.prod(m)) < MAX_POINTS and len(m) == d
        rng = np.random.default_rng(SEED + 100 + i)
        axes = []
        for k in range(d):
            s = next(s for s, group in enumerate(sl.partition) if k in group)
            nodes = np.asarray(sl.slides[s].nodes[list(sl.partition[s]).index(k)])
            axes.append(EG.make_axis(rng, c["domain"][k][0], c["domain"][k][1], nodes, m[k], k))
        for k in range(d):
            out[f"l{i}_ax{k}"] = axes[k]
        for j, spec in enumerate(g["specs"]):
            res = np.empty(m)
            for idx in np.ndindex(*m):
                res[idx] = sl.eval([float(axes[k][idx[k]]) for k in range(d)], list(spec))
            usable(f"slider {grid_id(g)}", spec, res, slider_ld(sl, axes, spec))
            out[f"l{i}_r{j}"] = res
        if case in SLIDER_ZERO:
            zero = np.array([sl.eval([float(axes[k][idx[k]]) for k in range(d)], SLIDER_ZERO[case]) for idx in np.ndindex(*m)])
            assert np.all(zero == 0.0) and not np.any(np.signbit(zero)), "a cross-slide derivative is +0.0 in the reference"
        print(f"slider {grid_id(g)}: {int(np.prod(m))} points, {len(g['specs'])} specs")

    path = os.path.join(HERE, "g32_piecewise_grid.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
