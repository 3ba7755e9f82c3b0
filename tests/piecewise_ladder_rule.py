"""NumPy restatement of the rule ``ChebyshevSpline.ladder_batch`` and ``ChebyshevSlider.ladder_batch`` compute
(csrc/piecewise_ladder_kernels.h around the dense fibre-then-1-D rule of tests/ladder_rule.py): routing of rows and
values, the fibre of the piece a value falls into and its 1-D interpolant, the slider's sum with one varying slide.  No
GPU; tests/test_piecewise_ladders_host.py holds it to the golden ladders of g35, which shows that the RULE, not only the
kernels, meets them."""
from __future__ import annotations

import numpy as np

import ladder_rule


def route(knots, n_pieces: int, values) -> np.ndarray:
    """spline_dim_piece: the number of knots <= x, clamped to the last piece; a NaN goes to the last piece"""
    v = np.asarray(values, dtype=float)
    k = np.asarray(knots, dtype=float)
    idx = (k[None, :] <= v.reshape(-1, 1)).sum(axis=1) if k.size else np.zeros(v.size, dtype=np.int64)
    idx = np.where(np.isnan(v.reshape(-1)), k.size, idx)
    return np.minimum(idx, n_pieces - 1).reshape(v.shape)


def spline_ladder(tensors, domains, knots, shape, dim, fixed, xs, spec=None):
    """``tensors`` / ``domains``: the pieces' tensors and domains in C order over ``shape``.  Per row the cross-section
    from ``fixed``, per value the index along dim, then the owning piece's dense ladder (fibre, then 1-D interpolant)."""
    d = len(shape)
    others = [k for k in range(d) if k != dim]
    fixed = np.asarray(fixed, dtype=float)
    xs = np.asarray(xs, dtype=float)
    out = np.empty((fixed.shape[0], xs.shape[-1]))
    sec = [route(knots[k], shape[k], fixed[:, c]) for c, k in enumerate(others)]
    for r in range(fixed.shape[0]):
        xr = xs if xs.ndim == 1 else xs[r]
        along = route(knots[dim], shape[dim], xr)
        for j in np.unique(along):
            multi = [0] * d
            for c, k in enumerate(others):
                multi[k] = int(sec[c][r])
            multi[dim] = int(j)
            flat = int(np.ravel_multi_index(multi, shape))
            pos = np.flatnonzero(along == j)
            out[r, pos] = ladder_rule.dense_ladder(tensors[flat], domains[flat], dim, fixed[r:r + 1], xr[pos], spec)[0]
    return out


def spline_rule(sp, dim, fixed, xs, spec=None):
    """:func:`spline_ladder` on a built ``ChebyshevSpline``"""
    return spline_ladder([p.tensor_values for p in sp._pieces], [[list(b) for b in p.domain] for p in sp._pieces],
                         [list(k) for k in sp.knots], tuple(sp._shape), dim, fixed, xs, spec)


def slider_rule(sl, dim, fixed, xs, spec=None):
    """:func:`slider_ladder` on a built ``ChebyshevSlider``"""
    return slider_ladder([s.tensor_values for s in sl.slides], [[list(b) for b in s.domain] for s in sl.slides],
                         [list(g) for g in sl.partition], sl.pivot_value, dim, fixed, xs, spec)


def slider_ladder(tensors, domains, partition, pivot, dim, fixed, xs, spec=None):
    """``tensors`` / ``domains``: the slides' tensors and domains.  Values: ``pivot + sum_s (v_s - pivot)``, slides in
    order, v_o the owner's ladder and v_s every other slide's value at the row.  A spec inside the owner: its derivative
    ladder alone; inside another slide: that slide's derivative at the row, at every value; across slides: +0.0."""
    d = sum(len(g) for g in partition)
    fixed = np.asarray(fixed, dtype=float)
    xs = np.asarray(xs, dtype=float)
    rows, m = fixed.shape[0], xs.shape[-1]
    col = {k: (k if k < dim else k - 1) for k in range(d) if k != dim}
    o = next(s for s, g in enumerate(partition) if dim in g)
    spec = [0] * d if spec is None else list(spec)
    active = sorted({s for s, g in enumerate(partition) for k in g if spec[k] > 0})
    if len(active) > 1:
        return np.zeros((rows, m))

    def slide(s):
        g = list(partition[s])
        sub = [spec[k] for k in g]
        if s == o:
            f = np.column_stack([fixed[:, col[k]] for k in g if k != dim]) if len(g) > 1 else np.empty((rows, 0))
            return ladder_rule.dense_ladder(tensors[s], domains[s], g.index(dim), f, xs, sub)
        v = np.empty((rows, 1))
        for r in range(rows):            # the slide's value at the row: a ladder of one value along its dimension 0
            f = np.array([[fixed[r, col[k]] for k in g[1:]]])
            v[r] = ladder_rule.dense_ladder(tensors[s], domains[s], 0, f, np.array([fixed[r, col[g[0]]]]), sub)[0]
        return np.broadcast_to(v, (rows, m))

    if active:
        return np.array(slide(active[0]))
    res = np.full((rows, m), float(pivot))
    for s in range(len(partition)):
        res = res + (slide(s) - float(pivot))
    return res
