#!/usr/bin/env python3
"""Generate tests/golden/g21_algebra.npz: the reference's arithmetic operators and ``ChebyshevTT.reorder``.

Run in the build container only (the reference checkout does not travel to the GPU box):

    python tests/golden/generate_golden_algebra.py [--ref /root/reference]

It imports PyChebyshev v0.21.1 from ``<ref>/src`` and stores arrays only.  The operands are rebuilt by the tests
from inputs that already live in the golden set:

  dense     a = g2_bs5d["tensor"] on the 5-D Black-Scholes grid, b = the same tensor flipped along axis 0
  spline    a = functions.SPLINE_CASES[tag] built with its callback, b = every piece's values flipped along axis 0
            (a spline of the same knots and node counts, through from_values)
  slider    a = functions.SLIDER_CASES["b"] (bs_5d), b = the same case with poly_5d_fixture
  tt        g4_tt_bs5d r8 cores, g5_tt_rank16 cores, g5b_tt_mixed cores; seeded random cores
            (np.random.default_rng(seed).standard_normal, shapes below); b = a's cores times
            (1 + 0.25 * standard_normal) from np.random.default_rng(b_seed), core by core, except for g4, whose
            b is a / 2 (core 0 halved)

Dense, spline and slider: ``<tag>_<op>`` holds the combination evaluated at ``<tag>_points`` for every spec of
``<tag>_specs`` (rows = specs).  Ops: add (a + b), sub (a - b), lin (2.5 * a - b / 3), chain (a += b; a *= 0.5;
a -= b / 4, in place).
TT: ``tt_<tag>_<op>_ranks`` and ``tt_<tag>_<op>_eval`` at ``tt_<tag>_points`` for add, sub and lin, and
``tt_<tag>_rev_ranks`` / ``_rev_eval`` for ``reorder`` into the reversed order (points in the user's frame).  Every
truncation of these cases has its singular values at least 20x clear of the cut (checked here with NumPy SVDs;
``tt_<tag>_tol`` is the first tolerance of TT_TOLS for which that holds), so the ranks are fair to compare; the
swaps of ``reorder`` are checked the same way and ``tt_<tag>_rev_fair`` says whether they passed.
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

DENSE_SPECS = [[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [2, 0, 0, 0, 0], [1, 1, 0, 0, 0], [0, 0, 0, 1, 1]]
TT_TOLS = (1e-10, 1e-9, 1e-11, 1e-12, 1e-8, 1e-13, 1e-7)   # the first that is MARGIN x clear is used
MARGIN = 20.0
# tag: (source, max_rank of both operands, b_seed); random sources: (seed, d, n, r)
TT_CASES = {
    "g4": ("g4", 16, None),
    "g5": ("g5", 32, 501),
    "g5b": ("g5b", 16, 511),
    "rand16": ((1616, 8, 16, 16), 32, 1617),
    "rand64": ((6464, 10, 16, 64), 128, 6465),
}


def tt_sources():
    g4 = np.load(os.path.join(HERE, "g4_tt_bs5d.npz"))
    g5 = np.load(os.path.join(HERE, "g5_tt_rank16.npz"))
    g5b = np.load(os.path.join(HERE, "g5b_tt_mixed.npz"))
    return {
        "g4": ([g4[f"r8_core{k}"] for k in range(5)], F.BS5_DOMAIN),
        "g5": ([g5[f"core{k}"] for k in range(10)], [[-1.0, 1.0]] * 10),
        "g5b": ([g5b[f"core{k}"] for k in range(4)], [[0.0, 2.0], [-3.0, -1.0], [10.0, 11.0], [-1.0, 1.0]]),
    }


def tt_operands(tag):
    """(cores_a, cores_b, domain, max_rank) of a TT case: the recipe the tests repeat."""
    src, max_rank, b_seed = TT_CASES[tag]
    if isinstance(src, str):
        cores, domain = tt_sources()[src]
        cores = [np.array(c, dtype=float) for c in cores]
    else:
        seed, d, n, r = src
        rng = np.random.default_rng(seed)
        rk = [1] + [r] * (d - 1) + [1]
        cores = [rng.standard_normal((rk[k], n, rk[k + 1])) / np.sqrt(rk[k] * n) for k in range(d)]
        domain = [[-1.0, 1.0]] * d
    if b_seed is None:          # a smooth function's spectrum has no gap: b = a / 2 keeps a's own bond spectra
        other = [c.copy() for c in cores]
        other[0] = other[0] * 0.5
    else:
        rng = np.random.default_rng(b_seed)
        other = [c * (1.0 + 0.25 * rng.standard_normal(c.shape)) for c in cores]
    return cores, other, domain, max_rank


def tt_points(domain, n=256, seed=2121):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(lo, hi, n) for lo, hi in domain])


# ---- margins: every truncation's singular values well clear of the cut -----------------------------------
def _cut_margin(S, max_rank, tol):
    """(kept, ratio): ratio > 1 measures how far the kept / dropped singular values are from the cut."""
    S = np.asarray(S)
    if S[0] == 0:
        return len(S), 0.0
    keep = min(max_rank, len(S), int(np.sum(S > tol * S[0])))
    keep = max(1, keep)
    worst = np.inf
    if keep < len(S):
        lo_kept = S[keep - 1]
        hi_drop = S[keep]
        cut = tol * S[0] if keep < min(max_rank, len(S)) else None
        if cut is None:        # capped by max_rank: the gap itself must be clear
            worst = min(worst, lo_kept / max(hi_drop, 1e-300))
        else:
            worst = min(worst, lo_kept / cut, cut / max(hi_drop, 1e-300))
    else:
        worst = min(worst, S[keep - 1] / (tol * S[0]))
    return keep, worst


def rounding_margin(cores, max_rank, tol):
    cores = [c.copy() for c in cores]
    d = len(cores)
    for k in range(d - 1, 0, -1):
        rl, n, rr = cores[k].shape
        q, r = np.linalg.qr(cores[k].reshape(rl, n * rr).T)
        cores[k] = q.T.reshape(-1, n, rr)
        cores[k - 1] = np.einsum("ljs,sr->ljr", cores[k - 1], r.T)
    worst = np.inf
    for k in range(d - 1):
        rl, n, rr = cores[k].shape
        u, s, vt = np.linalg.svd(cores[k].reshape(rl * n, rr), full_matrices=False)
        keep, m = _cut_margin(s, max_rank, tol)
        worst = min(worst, m)
        cores[k] = u[:, :keep].reshape(rl, n, keep)
        cores[k + 1] = np.einsum("lr,rjs->ljs", s[:keep, None] * vt[:keep], cores[k + 1])
    return worst


def swap_margins(cores, swaps, max_rank, tol):
    cores = [c.copy() for c in cores]
    worst = np.inf
    for i in swaps:
        a, b = cores[i], cores[i + 1]
        rl, na, _ = a.shape
        _, nb, rr = b.shape
        m = np.einsum("lab,brs->lars", a, b).transpose(0, 2, 1, 3).reshape(rl * nb, na * rr)
        u, s, vt = np.linalg.svd(m, full_matrices=False)
        keep, mg = _cut_margin(s, max_rank, tol)
        worst = min(worst, mg)
        cores[i] = (u[:, :keep] * s[:keep]).reshape(rl, nb, keep)
        cores[i + 1] = vt[:keep].reshape(keep, na, rr)
    return worst


def bubble_swaps(current, target):
    current, swaps = list(current), []
    for k in range(len(target)):
        j = current.index(target[k])
        while j > k:
            swaps.append(j - 1)
            current[j - 1], current[j] = current[j], current[j - 1]
            j -= 1
    return swaps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.ref, "src"))
    import pychebyshev as ref
    from pychebyshev import ChebyshevApproximation, ChebyshevSlider, ChebyshevSpline, ChebyshevTT
    from pychebyshev._algebra import _tt_add_cores

    print("reference version", ref.__version__)
    t0 = time.time()
    out = {}

    def record(tag, make_a, make_b, points, specs, evaluate):
        a, b = make_a(), make_b()
        combos = {"add": a + b, "sub": a - b, "lin": 2.5 * a - b / 3}
        c = make_a()
        c += b
        c *= 0.5
        c -= b / 4
        combos["chain"] = c
        out[f"{tag}_points"] = points
        out[f"{tag}_specs"] = np.array(specs)
        for op, obj in combos.items():
            out[f"{tag}_{op}"] = np.stack([evaluate(obj, points, s) for s in specs])

    # ---- dense
    T = np.load(os.path.join(HERE, "g2_bs5d.npz"))["tensor"]
    record("dense", lambda: ChebyshevApproximation.from_values(T, 5, F.BS5_DOMAIN, F.BS5_NODES),
           lambda: ChebyshevApproximation.from_values(np.ascontiguousarray(T[::-1]), 5, F.BS5_DOMAIN, F.BS5_NODES),
           F.bs5_query_points(400, seed=2101), DENSE_SPECS,
           lambda o, p, s: o.vectorized_eval_batch(p, s))

    # ---- splines
    for tag in ("b", "c"):
        case = F.SPLINE_CASES[tag]

        def build(case=case):
            sp = ChebyshevSpline(getattr(F, case["f"]), case["d"], case["domain"],
                                 n_nodes=[list(v) if isinstance(v, list) else v for v in case["n_nodes"]],
                                 knots=case["knots"])
            sp.build(verbose=False)
            return sp

        def flipped(case=case):
            sp = build()
            for p in sp._pieces:
                p.tensor_values = np.ascontiguousarray(p.tensor_values[::-1])
            return sp

        rng = np.random.default_rng(2102 + ord(tag))
        pts = np.column_stack([rng.uniform(lo, hi, 300) for lo, hi in case["domain"]])
        record(f"spline_{tag}", build, flipped, pts, case["specs"], lambda o, p, s: o.eval_batch(p, s))

    # ---- slider
    case = F.SLIDER_CASES["b"]

    def slider(fn):
        sl = ChebyshevSlider(fn, case["d"], case["domain"], case["n_nodes"], partition=case["partition"],
                             pivot_point=case["pivot"])
        sl.build(verbose=False)
        return sl

    rng = np.random.default_rng(2103)
    pts = np.column_stack([rng.uniform(lo, hi, 200) for lo, hi in case["domain"]])
    record("slider", lambda: slider(F.bs_5d), lambda: slider(F.poly_5d_fixture), pts, case["specs"],
           lambda o, p, s: np.array([o.eval(list(q), s) for q in p]))

    # ---- tensor trains
    def make_tt(cores, domain, max_rank, tol):
        obj = ChebyshevTT.__new__(ChebyshevTT)
        obj.function = None
        obj.num_dimensions = len(cores)
        obj.domain = [list(b) for b in domain]
        obj.n_nodes = [c.shape[1] for c in cores]
        obj.max_rank = max_rank
        obj.tolerance = tol
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
        obj._dim_order = list(range(len(cores)))
        return obj

    for tag in TT_CASES:
        ca, cb, domain, max_rank = tt_operands(tag)
        d = len(ca)
        rev = list(range(d))[::-1]
        pairs = lambda a, b: {"add": (a, b), "sub": (a, -b), "lin": (2.5 * a, -(b / 3))}   # noqa: E731

        def margin_at(tol):
            a, b = make_tt(ca, domain, max_rank, tol), make_tt(cb, domain, max_rank, tol)
            return min(rounding_margin(_tt_add_cores(x._coeff_cores, y._coeff_cores), max_rank, tol)
                       for x, y in pairs(a, b).values())

        tol = next((t for t in TT_TOLS if margin_at(t) > MARGIN), None)
        assert tol is not None, f"tt {tag}: no tolerance of {TT_TOLS} is {MARGIN}x clear of every singular value"
        out[f"tt_{tag}_tol"] = np.array(tol)
        # a smooth function's swapped pairs have no spectral gap: their ranks are compared only where there is one
        out[f"tt_{tag}_rev_fair"] = np.array(swap_margins(ca, bubble_swaps(range(d), rev), max_rank, tol) > MARGIN)
        a, b = make_tt(ca, domain, max_rank, tol), make_tt(cb, domain, max_rank, tol)
        pts = tt_points(domain)
        out[f"tt_{tag}_points"] = pts
        for op, (x, y) in pairs(a, b).items():
            res = x + y
            out[f"tt_{tag}_{op}_ranks"] = np.array(res.tt_ranks if not callable(res.tt_ranks) else res.tt_ranks())
            out[f"tt_{tag}_{op}_eval"] = res.eval_batch(pts)
        r = a.reorder(rev)
        out[f"tt_{tag}_rev_ranks"] = np.array(r.tt_ranks if not callable(r.tt_ranks) else r.tt_ranks())
        out[f"tt_{tag}_rev_eval"] = r.eval_batch(pts)
        print(f"  tt {tag}: tol {tol:g}, add ranks {list(out[f'tt_{tag}_add_ranks'])}, reorder ranks {list(out[f'tt_{tag}_rev_ranks'])} (fair: {bool(out[f'tt_{tag}_rev_fair'])})")

    path = os.path.join(HERE, "g21_algebra.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote g21_algebra.npz ({os.path.getsize(path) / 1024:.1f} KiB) in {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
