#!/usr/bin/env python3
"""Rows per second of the spline's batched calculus (``roots_batch`` / ``minimize_batch``: ``pcx_spline_calculus_batch``)
at N = 10^3, 10^4 and 10^5 rows on two splines -- "m": three dimensions, 9 x 7 x 6 nodes in each of 4 x 1 x 2 pieces of
equal shape (the evaluation takes all pieces in one launch), solved along dimension 0 (4 pieces); "k": two dimensions
with nested, unequal node counts [[7, 9, 11], [6, 8]] (one evaluation launch per piece), solved along dimension 0
(3 pieces) -- next to

  (a) the only route there was before the batch: a loop of single calls that solve piece by piece (every piece's own
      ``roots`` / ``minimize``, one device call each, merged on the host), timed over 200 rows and quoted per row,
  (b) the solver alone: ``_calculus.cheb1d_calculus`` (``pcx_cheb1d_calculus``) on the same N P fibres, one call per piece
      index; the fibres come from ``eval_batch`` beforehand and their upload is part of the call.

    python tools/spline_calculus_probe.py                 # every step, each in a child process under its own time limit
    python tools/spline_calculus_probe.py --step m        # one step in this process
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/spline_calculus_probe.py --step trace-m
                                                          # 1 + 5 calls of each batch at N = 10^4, for the per-kernel times

Host clock around the synchronous calls (each ends in a download), one warm-up call per shape, then REPEATS timed calls:
the median is reported with the fastest and slowest call.  Kernel times are not claimed here."""
import argparse
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [1_000, 10_000, 100_000]
N_SINGLE = 200
N_TRACE = 10_000
REPEATS = 7
STEP_LIMIT_S = 240

SHAPES = {
    "m": dict(d=3, domain=[[80.0, 120.0], [0.01, 0.25], [0.1, 0.4]], n_nodes=[9, 7, 6], knots=[[95.0, 100.0, 105.0], [], [0.2]],
              f=lambda x, _=None: (math.sin(0.45 * (x[0] - 80.0)) * (1.0 + 2.0 * x[1]) + 6.0 * (x[2] - 0.25)
                                   + 0.02 * abs(x[0] - 100.0) - 0.3), dim=0),
    "k": dict(d=2, domain=[[-1.0, 1.0], [0.0, 1.0]], n_nodes=[[7, 9, 11], [6, 8]], knots=[[-0.3, 0.4], [0.5]],
              f=lambda x, _=None: math.sin(5.0 * x[0]) * math.exp(x[1]) + 0.3 * abs(x[0] - 0.4) + max(x[1] - 0.5, 0.0) ** 2 - 0.2,
              dim=0),
}


def timed(fn):
    fn()
    t = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), min(t), max(t)


def line(what, n, stats):
    med, lo, hi = stats
    print(f"  {what:<58} {n:>7} rows  {med * 1e3:>9.2f} ms  [{lo * 1e3:.2f} .. {hi * 1e3:.2f}]  {n / med:>10.3e} rows/s",
          flush=True)
    return n / med


def make(tag):
    from pychebyshev_amd import ChebyshevSpline
    c = SHAPES[tag]
    sp = ChebyshevSpline(c["f"], c["d"], c["domain"], n_nodes=[list(v) if isinstance(v, list) else v for v in c["n_nodes"]],
                         knots=c["knots"])
    sp.build(verbose=False)
    return sp


def rows_of(tag, n):
    c = SHAPES[tag]
    rng = np.random.default_rng(11)
    dom = np.asarray(c["domain"])
    others = [k for k in range(c["d"]) if k != c["dim"]]
    return np.ascontiguousarray(dom[others, 0] + (dom[others, 1] - dom[others, 0]) * rng.uniform(0.02, 0.98, (n, len(others))))


def piece_route(sp, dim, fixed, mode):
    """The single call as it was before the batch: every piece on its own, merged on the host."""
    from pychebyshev_amd import _calculus
    dim, pieces, sub = sp._calculus_pieces(dim, fixed)
    if mode == "roots":
        return _calculus.merge_pieces("roots", [p.roots(dim, sub) for p in pieces], sp.domain[dim])
    return _calculus.merge_pieces(mode, [p.minimize(dim, sub) for p in pieces])


def step(tag):
    from pychebyshev_amd import _calculus
    c = SHAPES[tag]
    d, dim = c["d"], c["dim"]
    sp = make(tag)
    others = [k for k in range(d) if k != dim]
    counts = sp._dim_counts(dim)
    print(f"shape {tag}: nodes {c['n_nodes']}, knots {c['knots']}, along dimension {dim}: {len(counts)} pieces of {counts} nodes")
    fixed_all = rows_of(tag, max(SIZES))
    singles = [{k: float(v) for k, v in zip(others, row)} for row in fixed_all[:N_SINGLE]]
    loop_roots = line("(a) loop of per-piece roots, merged on the host", N_SINGLE,
                      timed(lambda: [piece_route(sp, dim, fx, "roots") for fx in singles]))
    loop_min = line("(a) loop of per-piece minimize, merged on the host", N_SINGLE,
                    timed(lambda: [piece_route(sp, dim, fx, "min") for fx in singles]))
    line("loop of roots(dim, fixed): the one-row batch", N_SINGLE, timed(lambda: [sp.roots(dim, fx) for fx in singles]))
    # representatives of the piece indices along dim (the other indices 0): their grids are the batch's
    stride = int(np.prod(sp._shape[dim + 1:]))
    reps = [sp._pieces[j * stride] for j in range(len(counts))]
    for n in SIZES:
        fixed = fixed_all[:n]
        got_r = line("roots_batch", n, timed(lambda: sp.roots_batch(dim, fixed)))
        got_m = line("minimize_batch", n, timed(lambda: sp.minimize_batch(dim, fixed)))
        fibres = []
        for p in reps:                     # fibres of piece index j for every row, through the spline's evaluation
            x = p.nodes[dim]
            pts = np.empty((n, x.size, d))
            pts[:, :, others] = fixed[:, None, :]
            pts[:, :, dim] = x[None, :]
            fibres.append(sp.eval_batch(pts.reshape(-1, d), [0] * d).reshape(n, x.size))

        def solver(mode):
            for p, v in zip(reps, fibres):
                _calculus.cheb1d_calculus(v, p.nodes[dim], p.weights[dim], p.diff_matrices[dim] if mode != "roots" else None,
                                          tuple(p.domain[dim]), mode)
        sol_r = line("(b) solver alone, roots: cheb1d_calculus per piece index", n, timed(lambda: solver("roots")))
        sol_m = line("(b) solver alone, minimize", n, timed(lambda: solver("min")))
        print(f"    N = {n}: roots_batch {got_r / loop_roots:.1f} x route (a), {got_r / sol_r:.2f} x route (b);  "
              f"minimize_batch {got_m / loop_min:.1f} x (a), {got_m / sol_m:.2f} x (b)", flush=True)
    R, cnt = sp.roots_batch(dim, fixed_all[:N_SINGLE])
    agree = sum(np.array_equal(piece_route(sp, dim, fx, "roots"), R[i, :cnt[i]]) for i, fx in enumerate(singles))
    print(f"  {agree} of {N_SINGLE} per-piece roots equal their batch rows bit for bit", flush=True)


def trace(tag):
    sp = make(tag)
    fixed = rows_of(tag, N_TRACE)
    for _ in range(6):
        sp.roots_batch(SHAPES[tag]["dim"], fixed)
        sp.minimize_batch(SHAPES[tag]["dim"], fixed)
    print(f"trace {tag}: 6 roots_batch and 6 minimize_batch calls of {N_TRACE} rows", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(SHAPES) + ["trace-" + t for t in sorted(SHAPES)])
    args = ap.parse_args()
    if args.step:
        if args.step.startswith("trace-"):
            trace(args.step[6:])
        else:
            step(args.step)
        return 0
    for tag in sorted(SHAPES):          # a fresh process per step, stopped at its own time limit; nothing runs after a failure
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", tag], timeout=STEP_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            print(f"step {tag}: ended at its time limit of {STEP_LIMIT_S} s", flush=True)
            return 124
        if rc:
            print(f"step {tag}: exit status {rc}", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
