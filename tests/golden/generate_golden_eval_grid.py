#!/usr/bin/env python3
"""Generate tests/golden/g29_eval_grid.npz: the interpolant on tensor-product grids, what ``eval_grid`` computes, by the
reference's pointwise rule -- ``ChebyshevApproximation.vectorized_eval`` (with derivative orders) and ``ChebyshevTT.eval``
looped over EVERY grid point.

Run in the build container only (the reference checkout does not travel to the GPU box):

    python tests/golden/generate_golden_eval_grid.py --ref <reference checkout>

It imports PyChebyshev v0.21.1 from ``<ref>/src`` and stores arrays only.

Dense cases (DENSE below): the functions of tests/golden/functions.py on the node counts ``n`` and the grid shapes ``m``
that exercise every tile edge of the mode-product kernels (one point, a K remainder, ragged 16-tiles along every role,
n = 64 with m < n).  The 3-D cases also carry the specs [1,0,0], [0,2,0], [1,1,0].  TT cases: models A, C and F of
g22_tt_transforms.npz (cores and domains are read from that file, loaded into the reference as
generate_golden_tt_derivatives.py does); C's storage order is the identity there, so it is given the order TT_C_ORDER
here (the cores stay where they are: storage dimension k then holds the user's dimension TT_C_ORDER[k]).

The axes of a case together mix: interior points, both domain ends, two exact nodes, one point 5e-15 from a node (inside
the reference's 1e-14 one-hot window), one repeated value, and a non-monotone order; an axis too short to hold them all
takes a slice of the list that starts at a different feature per dimension.  Every case has at most 20,000 grid points.

What a golden value is worth: the tests hold ``eval_grid`` to 1e-12 normwise (and spec_point_tol pointwise) against these
values, which means something only where the reference ITSELF is that close to the interpolant it evaluates.  A second
derivative goes through D_k^2, which amplifies rounding by about n^4 / width^2: on a narrow domain two equally valid FP64
summation orders differ by more than 1e-12 of a small result.  So every stored grid is checked here against the same
rule evaluated in ``np.longdouble`` (weights, differentiation matrices, derivative passes and contractions; the one-hot
window kept), and a case is stored only when the reference is within REF_SHARE = 1/2 of both bounds of it (two FP64
routes share a bound equally) -- the reference's own error, measured without any code of this repository.  A case may name ``alternatives`` (function,
domain): the first choice that passes is stored and printed.  (Tried for (12, 12, 12): the reference's
[0, 2, 0] is 6.7e-12 from the long-double value for bs_3d on [80, 120] x [0.25, 1] x [0.15, 0.35] and 4.9e-12 for
sin_sum_3d on [-1, 1]^3, and 3.8e-10 pointwise for exp_mix_3d on the box of the (4, 11, 6) case; a wider domain divides
that by its width squared, and sin_sum_3d has no mixed derivative to compare.  exp_mix_3d on [-2, 2]^3 passes.)

Keys:  dense  d<i>_n, d<i>_domain, d<i>_tensor, d<i>_ax<k>, d<i>_nspec, d<i>_s<j>_spec, d<i>_s<j>_ref (shape m)
       TT     t<M>_order, t<M>_ax<u> (user dimension u), t<M>_ref (shape m in the user's order)
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import functions as F  # noqa: E402

SPECS_3D = [[0, 0, 0], [1, 0, 0], [0, 2, 0], [1, 1, 0]]
DENSE = [
    dict(f="sin_sum_nd", n=(3,), m=(1,), domain=[[-1.0, 1.0]]),
    dict(f="sin_sum_nd", n=(3,), m=(17,), domain=[[-1.0, 1.0]]),
    dict(f="sin_cos_2d", n=(5, 7), m=(16, 1), domain=[[-1.0, 1.0], [0.0, 2.0]]),
    dict(f="sin_cos_2d", n=(5, 7), m=(17, 33), domain=[[-1.0, 1.0], [0.0, 2.0]]),
    dict(f="exp_mix_3d", n=(4, 11, 6), m=(3, 18, 5), domain=[[-1.0, 1.0], [0.5, 2.0], [-0.5, 1.5]]),
    # bs_3d, exp_mix_3d on its narrower box and sin_sum_3d do not pass the reference's own error check here (see above)
    dict(f="exp_mix_3d", n=(12, 12, 12), m=(16, 32, 16), domain=[[-2.0, 2.0]] * 3),
    dict(f="bs_5d", n=(3, 4, 5, 3, 4), m=(2, 3, 17, 1, 5), domain=F.BS5_DOMAIN),
    dict(f="sin_cos_2d", n=(64, 5), m=(3, 40), domain=[[-1.0, 1.0], [0.0, 2.0]]),
]
TT_GRIDS = {"A": (9,), "C": (4, 5, 3, 6, 4), "F": (6, 19, 5)}      # in the USER's dimension order
TT_C_ORDER = [2, 0, 4, 1, 3]
MAX_POINTS = 20000
REF_SHARE = 0.5
LD = np.longdouble


def point_tol(spec):
    """spec_point_tol of tests/conftest.py"""
    return 1e-12 * 10.0 ** min(sum(abs(int(v)) for v in spec), 3)


def grid_ld(tensor, nodes, axes, spec):
    """The reference's rule in long double: D_k^order passes on the tensor, then per axis one-hot rows within 1e-14 of a
    node and barycentric rows elsewhere."""
    cur = np.asarray(tensor, dtype=LD)
    d = cur.ndim
    for k in range(d):
        x = np.asarray(nodes[k], dtype=LD)
        n = x.size
        w = np.ones(n, dtype=LD)
        for j in range(n):
            keep = np.arange(n) != j
            w[keep] /= (x[keep] - x[j])
        if spec[k]:
            gap = x[:, None] - x[None, :]
            np.fill_diagonal(gap, LD(1))
            D = w[None, :] / (gap * w[:, None])
            np.fill_diagonal(D, LD(0))
            np.fill_diagonal(D, -D.sum(axis=1))
            for _ in range(int(spec[k])):
                cur = np.moveaxis(np.tensordot(D, cur, axes=([1], [k])), 0, k)
        rows = np.zeros((len(axes[k]), n), dtype=LD)
        for r, xv in enumerate(axes[k]):
            diff = LD(xv) - x
            exact = np.where(np.abs(np.float64(xv) - np.asarray(nodes[k], dtype=float)) < 1e-14)[0]
            if len(exact):
                rows[r, exact[0]] = 1
            else:
                rows[r] = (w / diff) / np.sum(w / diff)
        cur = np.moveaxis(np.tensordot(rows, cur, axes=([1], [k])), 0, k)
    return cur


def ref_error(ref, ld):
    """(E_norm, E_point) of tests/conftest.py::parity, of the reference against the long-double grid"""
    ld64 = np.asarray(ld, dtype=LD)
    scale = float(np.max(np.abs(ld64)))
    err = np.abs(np.asarray(ref, dtype=LD) - ld64)
    big = np.abs(ld64) >= 1e-3 * scale
    return float(np.max(err) / scale), float(np.max(err[big] / np.abs(ld64[big])))


def case_id(i):
    c = DENSE[i]
    return f"d{i}_" + "x".join(map(str, c["n"])) + "_to_" + "x".join(map(str, c["m"]))


def make_axis(rng, lo, hi, nodes, m, k):
    """m coordinates for dimension k: the feature list, rotated by k when it has to be cut, shuffled otherwise."""
    n = len(nodes)
    inner = rng.uniform(lo, hi, 3)
    na, nb = nodes[(1 + k) % n], nodes[(n // 2 + k) % n]
    near = nodes[(2 + k) % n] + 5e-15
    feats = [inner[0], lo, na, hi, near, nb, inner[0], inner[1], inner[2]]        # inner[0] twice: the repeated value
    if m < len(feats):
        r = (2 * k) % len(feats)
        return np.array((feats[r:] + feats[:r])[:m], dtype=float)
    ax = np.array(feats + list(rng.uniform(lo, hi, m - len(feats))), dtype=float)
    ax = ax[rng.permutation(m)]
    if np.all(np.diff(ax) >= 0):
        ax = ax[::-1].copy()
    return ax


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

    def dense_case(i, c, fname, domain):
        c = dict(c, f=fname, domain=domain)
        d = len(c["n"])
        assert int(np.prod(c["m"])) <= MAX_POINTS
        model = ChebyshevApproximation(getattr(F, c["f"]), d, [list(b) for b in c["domain"]], list(c["n"]), max_derivative_order=2)
        model.build(verbose=False)
        rng = np.random.default_rng(2900 + i)
        axes = [make_axis(rng, c["domain"][k][0], c["domain"][k][1], np.asarray(model.nodes[k]), c["m"][k], k) for k in range(d)]
        pre = f"d{i}"
        out = {}
        out[f"{pre}_n"] = np.array(c["n"], dtype=np.int64)
        out[f"{pre}_domain"] = np.array(c["domain"], dtype=float)
        out[f"{pre}_tensor"] = np.asarray(model.tensor_values, dtype=float)
        for k in range(d):
            out[f"{pre}_ax{k}"] = axes[k]
        specs = SPECS_3D if d == 3 else [[0] * d]
        out[f"{pre}_nspec"] = np.array(len(specs), dtype=np.int64)
        for j, spec in enumerate(specs):
            res = np.empty(c["m"])
            for idx in np.ndindex(*c["m"]):
                res[idx] = model.vectorized_eval([float(axes[k][idx[k]]) for k in range(d)], list(spec))
            out[f"{pre}_s{j}_spec"] = np.array(spec, dtype=np.int64)
            out[f"{pre}_s{j}_ref"] = res
            e_norm, e_point = ref_error(res, grid_ld(model.tensor_values, model.nodes, axes, spec))
            ok = e_norm <= REF_SHARE * 1e-12 and e_point <= REF_SHARE * point_tol(spec)
            print(f"  d{i} {fname} {spec}: reference vs long double E_norm {e_norm:.2e} E_point {e_point:.2e}{'' if ok else '  -- NOT usable'}")
            if not ok:
                return None
        hot = sum(int(np.any(np.abs(x - np.asarray(model.nodes[k])) < 1e-14)) for k in range(d) for x in axes[k])
        print(f"{case_id(i)}: {fname} on {domain}, {len(specs)} specs, {int(np.prod(c['m']))} points, {hot} one-hot coordinates")
        return out

    for i, c in enumerate(DENSE):
        for fname, domain in [(c["f"], c["domain"])] + list(c.get("alternatives", [])):
            got = dense_case(i, c, fname, domain)
            if got is not None:
                out.update(got)
                break
        else:
            raise SystemExit(f"{case_id(i)}: no choice of function passes the reference's own error check")

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
    for tag, m in TT_GRIDS.items():
        cores, k = [], 0
        while f"{tag}_core{k}" in G.files:
            cores.append(G[f"{tag}_core{k}"])
            k += 1
        d = len(cores)
        assert int(np.prod(m)) <= MAX_POINTS and len(m) == d
        domain = G[f"{tag}_domain"].tolist()                       # by storage position
        order = TT_C_ORDER if tag == "C" else G[f"{tag}_order"].tolist()
        n = [c.shape[1] for c in cores]
        tt = make_tt(cores, domain, order)
        rng = np.random.default_rng(2950 + ord(tag))
        axes = []
        for u in range(d):
            pos = order.index(u)
            (a, b), nu = domain[pos], n[pos]
            nodes = np.sort(0.5 * (a + b) + 0.5 * (b - a) * np.cos(np.pi * (2 * np.arange(nu) + 1) / (2 * nu)))
            axes.append(make_axis(rng, a, b, nodes, m[u], u))
        res = np.empty(m)
        for idx in np.ndindex(*m):
            res[idx] = tt.eval([float(axes[u][idx[u]]) for u in range(d)])
        out[f"t{tag}_order"] = np.array(order, dtype=np.int64)
        for u in range(d):
            out[f"t{tag}_ax{u}"] = axes[u]
        out[f"t{tag}_ref"] = res
        print(f"TT {tag}: order {order}, grid {m}, max|ref| {float(np.max(np.abs(res))):.3e}")

    path = os.path.join(HERE, "g29_eval_grid.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
