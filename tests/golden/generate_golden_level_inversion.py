#!/usr/bin/env python3
"""Generate tests/golden/g33_level_inversion.npz: the reference's roots of models of ``f - t``, for the ``level=``
keyword of roots() / roots_batch().

Run in the build container only (the reference checkout does not travel to the GPU box):

    python tests/golden/generate_golden_level_inversion.py [--ref /root/reference]

It imports PyChebyshev v0.21.1 from ``<ref>/src`` and stores arrays only.  For every case of ``CASES`` and each of its
three levels ``t`` the reference's model of ``f - t`` is built -- the callback computes ``f`` and then subtracts -- and
its ``roots(dim, fixed)`` recorded on ``N_ROWS`` fixed rows (one row for the 1-D spline).  The cases, their functions,
levels and ``fixed_rows`` below are imported by the tests, which build the model of ``f`` itself and ask it for
``roots(dim, fixed, level=t)``.

  <c>_rows          (rows, d - 1): the other dimensions in increasing order
  <c>_levels        (3,)
  <c>_L<i>_roots    (rows, W) NaN-padded, <c>_L<i>_count (rows,)

A stored root is at least ``MIN_GAP (b - a)`` away from its neighbours and from both ends of the domain along ``dim``
(asserted here: the levels stay away from the extrema of the fibres), so the tests leave no row out.
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

SEED = 3333
N_ROWS = 12
MIN_GAP = 1e-8


def wave_3d(x, _=None):
    return math.sin(3.0 * x[0]) * math.cos(2.0 * x[1]) + 0.4 * x[2] * x[2] + 0.2 * x[0]


_SA, _SC, _SL = F.SPLINE_CASES["a"], F.SPLINE_CASES["c"], F.SLIDER_CASES["a"]
CASES = {
    "approx": dict(kind="approx", f=wave_3d, d=3, domain=[[-1.0, 1.0]] * 3, n_nodes=[17, 11, 9], dim=0,
                   levels=[-0.35, 0.15, 0.5]),
    "spline1": dict(kind="spline", f=getattr(F, _SA["f"]), d=1, domain=_SA["domain"], n_nodes=_SA["n_nodes"],
                    knots=_SA["knots"], dim=0, levels=[0.25, 0.5, 0.8]),
    "spline3": dict(kind="spline", f=getattr(F, _SC["f"]), d=3, domain=_SC["domain"], n_nodes=_SC["n_nodes"],
                    knots=_SC["knots"], dim=0, levels=[1.5, 6.0, 12.0]),
    "slider": dict(kind="slider", f=getattr(F, _SL["f"]), d=3, domain=_SL["domain"], n_nodes=_SL["n_nodes"],
                   partition=_SL["partition"], pivot=_SL["pivot"], dim=0, levels=[-0.45, 0.1, 0.55]),
}


def fixed_rows(case: str) -> np.ndarray:
    """The fixed rows of a case, columns = the dimensions other than ``dim`` in increasing order: seeded, inside
    10-90 % of each domain."""
    c = CASES[case]
    others = [k for k in range(c["d"]) if k != c["dim"]]
    if not others:
        return np.empty((1, 0))
    rng = np.random.default_rng([SEED, sorted(CASES).index(case)])
    rows = np.empty((N_ROWS, len(others)))
    for col, k in enumerate(others):
        lo, hi = c["domain"][k]
        rows[:, col] = lo + (hi - lo) * rng.uniform(0.1, 0.9, N_ROWS)
    return rows


def build(classes, case: str, level: float = 0.0):
    """The model of ``f - level`` of a case (``level = 0``: of ``f``) from the classes of either package."""
    c = CASES[case]
    f = c["f"]
    fn = f if level == 0.0 else (lambda x, data=None: f(x, data) - level)
    if c["kind"] == "approx":
        obj = classes["approx"](fn, c["d"], c["domain"], c["n_nodes"])
        obj.build(verbose=False)
    elif c["kind"] == "spline":
        obj = classes["spline"](fn, c["d"], c["domain"],
                                n_nodes=[list(v) if isinstance(v, list) else v for v in c["n_nodes"]], knots=c["knots"])
        obj.build(verbose=False)
    else:
        obj = classes["slider"](fn, c["d"], c["domain"], c["n_nodes"], partition=c["partition"], pivot_point=c["pivot"])
        obj.build(verbose=False)
    return obj


def fixed_dict(case: str, row) -> dict | None:
    c = CASES[case]
    others = [k for k in range(c["d"]) if k != c["dim"]]
    return {k: float(v) for k, v in zip(others, row)} if others else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.ref, "src"))
    import pychebyshev as ref
    from pychebyshev import ChebyshevApproximation, ChebyshevSlider, ChebyshevSpline

    print("reference version", ref.__version__)
    classes = {"approx": ChebyshevApproximation, "spline": ChebyshevSpline, "slider": ChebyshevSlider}
    t0 = time.time()
    out = {}
    for case in sorted(CASES):
        c = CASES[case]
        rows = fixed_rows(case)
        a, b = c["domain"][c["dim"]]
        out[f"{case}_rows"] = rows
        out[f"{case}_levels"] = np.array(c["levels"], dtype=float)
        for i, t in enumerate(c["levels"]):
            model = build(classes, case, t)
            found = [np.asarray(model.roots(c["dim"], fixed_dict(case, row)), dtype=float) for row in rows]
            W = max(max(r.size for r in found), 1)
            R = np.full((rows.shape[0], W), np.nan)
            for r, got in enumerate(found):
                R[r, :got.size] = got
                edges = np.concatenate([[a], got, [b]])
                assert np.all(np.diff(edges) >= MIN_GAP * (b - a)), (case, t, r, got)
            out[f"{case}_L{i}_roots"] = R
            out[f"{case}_L{i}_count"] = np.array([r.size for r in found], dtype=np.int32)
            print(f"  {case} level {t}: root counts {[int(r.size) for r in found]}")
        assert any(out[f"{case}_L{i}_count"].max() > 0 for i in range(len(c["levels"]))), case
    path = os.path.join(HERE, "g33_level_inversion.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote g33_level_inversion.npz ({os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays) in {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
