#!/usr/bin/env python3
"""Generate tests/golden/g20_calculus.npz: the reference's roots / minimize / maximize on 1-D fibres, dense, spline
and TT inputs.

Run in the build container only (the reference checkout does not travel to the GPU box):

    python tests/golden/generate_golden_calculus.py [--ref /root/reference]

It imports PyChebyshev v0.21.1 from ``<ref>/src`` and stores arrays only.  Every result is stored as
``<tag>_roots`` (possibly empty), ``<tag>_min`` and ``<tag>_max`` (value, location).

  fib_<name>        1-D fibres: ``fib_<name>_values`` at the ascending type-I nodes of ``fib_<name>_domain``
  rand<n>           RAND_COUNT seeded smooth random series of n in (8, 16, 32, 64) nodes on [-1, 1], regenerated
                    by ``rand_fibres(seed, n)`` below (the tests restate it; ``rand<n>_head`` guards the regeneration):
                    ``rand<n>_roots`` (NaN-padded rows), ``rand<n>_count``, ``rand<n>_min`` / ``rand<n>_max`` rows
  sc2_d<k>_<i>      g1_sincos2d (domain [-1, 1]^2) along dimension k, the other one fixed at SC2_FIXED[i]
  spot_<i>          from_values(g2 tensor - 10) roots along spot (dim 0), the others fixed at BS5_FIXED[i]
  bs5_d<k>          g2 tensor min / max along dimension k, the others fixed at BS5_FIXED[0]
  spline_<case>_<i> functions.SPLINE_CASES along dimension 0, the others fixed at SPLINE_FIXED[case][i]
  tt4_d<k> / tt5_d<k>   g4 rank-8 cores on BS5_DOMAIN / g5 cores with g5["perm"] as dim_order on [-1, 1]^10: min /
                    max along user dimension k, the others fixed at TT4_FIXED / TT5_FIXED
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import functions as F  # noqa: E402

RAND_SEED = 2020
RAND_COUNT = 200
SC2_FIXED = [-1.0, -0.3, 0.1, 0.45, 1.0]   # not 0: sin(0) cos(y) is a zero fibre whose roots are rounding noise
BS5_FIXED = [[100.0, 0.5, 0.25, 0.03], [90.0, 0.3, 0.2, 0.05], [110.0, 0.9, 0.32, 0.01]]   # the 4 other coordinates
SPLINE_FIXED = {"a": [[]], "b": [[0.25], [0.5], [0.9]], "c": [[0.1, 0.15], [0.2, 0.3]]}
TT4_FIXED = [100.0, 100.0, 0.6, 0.25, 0.04]      # by user dimension (the entry of `dim` is skipped)
TT5_FIXED = [0.3, -0.2, 0.7, -0.9, 0.1, 0.5, -0.6, 0.25, -0.4, 0.8]
TT_DIMS = {"tt4": [0, 2, 3], "tt5": [0, 3, 7]}


def rand_fibres(seed: int, n: int, count: int = RAND_COUNT) -> np.ndarray:
    """count x n values at the ascending type-I nodes of [-1, 1] of smooth random Chebyshev series."""
    rng = np.random.default_rng([seed, n])
    decay = rng.uniform(0.05, 0.5, (count, 1))
    coef = rng.standard_normal((count, n)) * np.exp(-decay * np.arange(n))
    t = np.sort(np.polynomial.chebyshev.chebpts1(n))
    return np.polynomial.chebyshev.chebval(t, coef.T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.ref, "src"))
    import pychebyshev as ref
    from pychebyshev import ChebyshevApproximation, ChebyshevSpline, ChebyshevTT

    print("reference version", ref.__version__)
    t0 = time.time()
    out = {}

    def record(tag, obj, dim=None, fixed=None, roots=True, opt=True):
        if roots:
            out[f"{tag}_roots"] = np.asarray(obj.roots(dim, fixed), dtype=float)
        if opt:
            out[f"{tag}_min"] = np.array(obj.minimize(dim, fixed), dtype=float)
            out[f"{tag}_max"] = np.array(obj.maximize(dim, fixed), dtype=float)

    def fib(name, values, domain):
        values = np.asarray(values, dtype=float)
        out[f"fib_{name}_values"] = values
        out[f"fib_{name}_domain"] = np.array(domain, dtype=float)
        record(f"fib_{name}", ChebyshevApproximation.from_values(values, 1, [list(domain)], [values.size]))

    def nodes(lo, hi, n):
        return np.sort(0.5 * (lo + hi) + 0.5 * (hi - lo) * np.polynomial.chebyshev.chebpts1(n))

    # ---- 1-D fibres
    fib("sin3x", np.sin(3.0 * nodes(-1.0, 1.0, 20)), (-1.0, 1.0))
    fib("x2", nodes(-1.0, 1.0, 12) ** 2 - 0.25, (-1.0, 1.0))
    fib("exp01", np.exp(nodes(0.0, 1.0, 14)), (0.0, 1.0))
    fib("x01", nodes(0.0, 1.0, 10), (0.0, 1.0))
    fib("linear", nodes(-2.0, 3.0, 2) - 0.5, (-2.0, 3.0))
    for n in (1, 2, 5, 10, 17, 33, 64):
        fib(f"const{n}", np.full(n, 5.0), (-1.0, 1.0))
    for k in (5, 17, 40):
        t = nodes(-1.0, 1.0, 64)
        fib(f"T{k}", np.cos(k * np.arccos(t)), (-1.0, 1.0))
    out["rand_seed"] = np.array(RAND_SEED)
    out["rand_count"] = np.array(RAND_COUNT)
    for n in (8, 16, 32, 64):
        V = rand_fibres(RAND_SEED, n)
        out[f"rand{n}_head"] = V[0, :4].copy()
        R = np.full((RAND_COUNT, n - 1), np.nan)
        cnt = np.zeros(RAND_COUNT, dtype=np.int32)
        mn, mx = np.empty((RAND_COUNT, 2)), np.empty((RAND_COUNT, 2))
        for i in range(RAND_COUNT):
            c = ChebyshevApproximation.from_values(V[i], 1, [[-1.0, 1.0]], [n])
            r = c.roots()
            cnt[i] = r.size
            R[i, :r.size] = r
            mn[i], mx[i] = c.minimize(), c.maximize()
        out[f"rand{n}_roots"], out[f"rand{n}_count"], out[f"rand{n}_min"], out[f"rand{n}_max"] = R, cnt, mn, mx

    # ---- dense
    sc2 = np.load(os.path.join(HERE, "g1_sincos2d.npz"))["tensor"]
    c1 = ChebyshevApproximation.from_values(sc2, 2, [[-1.0, 1.0], [-1.0, 1.0]], [12, 12])
    for k in (0, 1):
        for i, v in enumerate(SC2_FIXED):
            record(f"sc2_d{k}_{i}", c1, k, {1 - k: v}, opt=False)
    bs = np.load(os.path.join(HERE, "g2_bs5d.npz"))["tensor"]
    spot = ChebyshevApproximation.from_values(bs - 10.0, 5, F.BS5_DOMAIN, F.BS5_NODES)
    for i, row in enumerate(BS5_FIXED):
        record(f"spot_{i}", spot, 0, {k + 1: v for k, v in enumerate(row)}, opt=False)
    c2 = ChebyshevApproximation.from_values(bs, 5, F.BS5_DOMAIN, F.BS5_NODES)
    for k in range(5):
        full = [100.0] + BS5_FIXED[0]
        record(f"bs5_d{k}", c2, k, {q: full[q] for q in range(5) if q != k}, roots=False)

    # ---- splines (along dimension 0)
    for case_name, case in F.SPLINE_CASES.items():
        sp = ChebyshevSpline(getattr(F, case["f"]), case["d"], case["domain"],
                             n_nodes=[list(v) if isinstance(v, list) else v for v in case["n_nodes"]], knots=case["knots"])
        sp.build(verbose=False)
        for i, row in enumerate(SPLINE_FIXED[case_name]):
            fixed = {k + 1: v for k, v in enumerate(row)} if case["d"] > 1 else None
            record(f"spline_{case_name}_{i}", sp, 0, fixed)

    # ---- tensor trains
    def make_tt(cores, domain, order=None):
        d = len(cores)
        obj = ChebyshevTT(None, d, [list(b) for b in domain], [c.shape[1] for c in cores])
        obj._coeff_cores = [np.array(c) for c in cores]
        obj._tt_ranks = [1] + [c.shape[2] for c in cores]
        obj._built = True
        obj.method = "cross"
        obj._dim_order = list(order) if order is not None else list(range(d))
        return obj

    g4 = np.load(os.path.join(HERE, "g4_tt_bs5d.npz"))
    g5 = np.load(os.path.join(HERE, "g5_tt_rank16.npz"))
    tts = {"tt4": (make_tt([g4[f"r8_core{k}"] for k in range(5)], F.BS5_DOMAIN), TT4_FIXED),
           "tt5": (make_tt([g5[f"core{k}"] for k in range(10)], [[-1.0, 1.0]] * 10, [int(v) for v in g5["perm"]]),
                   TT5_FIXED)}
    for name, (tt, fx) in tts.items():
        for k in TT_DIMS[name]:
            record(f"{name}_d{k}", tt, k, {q: fx[q] for q in range(len(fx)) if q != k}, roots=False)

    path = os.path.join(HERE, "g20_calculus.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote g20_calculus.npz ({os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays) in {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
