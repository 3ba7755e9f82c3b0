#!/usr/bin/env python3
"""Rows per second of ``invert_batch`` (one lane per fibre, ``csrc/invert_kernels.h``) against ``roots_batch(level=)``
(one wave per fibre, the colleague-matrix solver) on the same rows and targets, for the four classes:

  dense    a 5-D 11^5 tensor, along dimension 0
  tt       the 5-D rank-8 Black-Scholes train of tests/golden/g4_tt_bs5d.npz, along volatility (dimension 3)
  slider   the [[0, 1], [2], [3, 4]] Black-Scholes slider of tests/golden/functions.py, along spot (dimension 0)
  spline   the 8-piece 3-D call-price spline of tests/golden/functions.py, along spot (4 pieces of 9 nodes)

at N = 10^5 and 10^6 rows: host clock around the synchronous call (fixed rows and targets are host arrays -- the API
takes no device arrays here -- so every figure includes their upload and the download of the results), one warm-up call,
then the median of ``REPS`` timed calls with the fastest and slowest next to it.  Every target is the model's own value
at a random point of the row's fibre, so it is reached.

Kernel times do not come from the host clock: the script runs itself again under ``rocprofv3 --kernel-trace --stats``,
one fresh child process per trace, and reads the kernel statistics --

  solver   ``k_cheb1d_invert`` against ``k_cheb1d_calculus`` on the same 10^5 given fibres (``pcx_cheb1d_solve`` method 1
           and ``pcx_cheb1d_calculus`` on ``V - t``), n in {11, 33, 64}
  share    each class's ``invert_batch`` and ``roots_batch(level=)`` at N = 10^5: the solve kernels' share of all kernel
           time of the call, the rest being fibre evaluation, expansion, copies and the merge

    python tools/invert_probe.py [--out profiles/invert_probe.txt]

A child that fails ends the run: nothing more is started on the device after it."""
import argparse
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import functions as F  # noqa: E402

from pychebyshev_amd import ChebyshevApproximation, ChebyshevSlider, ChebyshevSpline, ChebyshevTT, _calculus  # noqa: E402
from pychebyshev_amd.barycentric import chebyshev_nodes, compute_barycentric_weights  # noqa: E402

REPS = 5
SIZES = (100_000, 1_000_000)
SOLVER_N = (11, 33, 64)
TRACE_ROWS = 100_000
CLASSES = ("dense", "tt", "slider", "spline")
DENSE_DOMAIN = [[80.0, 120.0], [0.25, 1.0], [0.15, 0.35], [0.01, 0.08], [0.0, 0.05]]


def make(name):
    """(model, dim, domain by dimension, evaluate(points))."""
    if name == "dense":
        grids = [chebyshev_nodes(lo, hi, 11) for lo, hi in DENSE_DOMAIN]
        X = np.meshgrid(*grids, indexing="ij")
        T = np.sin(0.3 * (X[0] - 100.0)) * (1.0 + X[1]) + X[2] - 0.25 + 10.0 * X[3] * np.cos(40.0 * X[4])
        m = ChebyshevApproximation.from_values(T, 5, DENSE_DOMAIN, [11] * 5)
        return m, 0, DENSE_DOMAIN, lambda p: m.vectorized_eval_batch(p, [0] * 5)
    if name == "tt":
        g4 = np.load(os.path.join(ROOT, "tests", "golden", "g4_tt_bs5d.npz"))
        m = ChebyshevTT.from_coeff_cores([g4[f"r8_core{k}"] for k in range(5)], F.BS5_DOMAIN)
        return m, 3, F.BS5_DOMAIN, m.eval_batch
    if name == "slider":
        c = F.SLIDER_CASES["b"]
        m = ChebyshevSlider(getattr(F, c["f"]), c["d"], c["domain"], c["n_nodes"], partition=c["partition"],
                            pivot_point=c["pivot"])
        m.build(verbose=False)
        return m, 0, c["domain"], lambda p: m.eval_batch(p, [0] * 5)
    c = F.SPLINE_CASES["c"]
    m = ChebyshevSpline(getattr(F, c["f"]), c["d"], c["domain"], n_nodes=c["n_nodes"], knots=c["knots"])
    m.build(verbose=False)
    return m, 0, c["domain"], lambda p: m.eval_batch(p, [0] * 3)


def inputs(domain, dim, evaluate, N, seed=0):
    """(fixed rows (N, d - 1), targets (N,)): the model's own values at a random point of every row's fibre."""
    rng = np.random.default_rng(seed)
    pts = np.column_stack([rng.uniform(lo + 0.02 * (hi - lo), hi - 0.02 * (hi - lo), N) for lo, hi in domain])
    t = np.asarray(evaluate(pts), dtype=float)
    return np.ascontiguousarray(np.delete(pts, dim, axis=1)), t


def timed(fn):
    fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def solver_fibres(n, N=TRACE_ROWS):
    """Smooth random series at n nodes of [-1, 1] and a target inside every row's range."""
    rng = np.random.default_rng([5, n])
    coef = rng.standard_normal((N, n)) * np.exp(-rng.uniform(0.05, 0.5, (N, 1)) * np.arange(n))
    x = chebyshev_nodes(-1.0, 1.0, n)
    V = np.ascontiguousarray(np.polynomial.chebyshev.chebval(x, coef.T))
    t = V.min(axis=1) + rng.uniform(0.05, 0.95, N) * (V.max(axis=1) - V.min(axis=1))
    return x, compute_barycentric_weights(x), V, t


# ------------------------------------------------------------------ the traced steps (children)
def step_solver(n):
    x, w, V, t = solver_fibres(n)
    S = V - t[:, None]
    for _ in range(4):
        _calculus.cheb1d_invert(V, t, x, w, (-1.0, 1.0))
        _calculus.cheb1d_calculus(S, x, w, None, (-1.0, 1.0), "roots")


def step_share(name, method):
    m, dim, domain, evaluate = make(name)
    rows, t = inputs(domain, dim, evaluate, TRACE_ROWS)
    for _ in range(4):
        if method == "invert":
            m.invert_batch(dim, rows, t)
        else:
            m.roots_batch(dim, rows, level=t)


def trace(args, lines):
    """Run this script's step `args` under rocprofv3 in a fresh child -> [(kernel, calls, total ns)], by total time."""
    tmp = tempfile.mkdtemp(prefix="invert_probe_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "trace", "--", sys.executable,
               os.path.abspath(__file__)] + args
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        if res.returncode != 0:
            lines.append(f"trace {' '.join(args)}: exit {res.returncode}\n{res.stdout[-2000:]}")
            return None
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            seen = [os.path.relpath(p, tmp) for p in glob.glob(os.path.join(tmp, "**", "*"), recursive=True)]
            lines.append(f"trace {' '.join(args)}: no kernel statistics written; files: {seen}")
            return None
        with open(found[0], newline="") as fh:
            rows = [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(fh)]
        return sorted(rows, key=lambda r: -r[2])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def is_solve(kernel):
    return "k_cheb1d_invert" in kernel or "k_cheb1d_calculus" in kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "invert_probe.txt"))
    ap.add_argument("--step", nargs="*")
    args = ap.parse_args()
    if args.step:
        if args.step[0] == "solver":
            step_solver(int(args.step[1]))
        else:
            step_share(args.step[1], args.step[2])
        return 0
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def finish(rc):
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        return rc

    say(f"invert_batch against roots_batch(level=) on the same rows and targets; host clock around the synchronous call, "
        f"1 warm-up, median of {REPS} [fastest .. slowest]")
    for name in CLASSES:
        m, dim, domain, evaluate = make(name)
        n_txt = m._dim_counts(dim) if name == "spline" else int(m.n_nodes[m._dim_order.index(dim)] if name == "tt" else m.n_nodes[dim])
        say(f"{name}: along dimension {dim}, nodes {n_txt}")
        for N in SIZES:
            rows, t = inputs(domain, dim, evaluate, N)
            ti = timed(lambda: m.invert_batch(dim, rows, t))
            tr = timed(lambda: m.roots_batch(dim, rows, level=t))
            x, s = m.invert_batch(dim, rows, t)
            R, cnt = m.roots_batch(dim, rows, level=t)
            one = (s >= 1) & (cnt == s)                      # both see the same solutions: x is the lowest root
            span = domain[dim][1] - domain[dim][0]
            diff = float(np.max(np.abs(x[one] - R[one, 0]), initial=0.0)) / span
            say(f"  N = {N:>7}  invert_batch {ti[0] * 1e3:>9.2f} ms [{ti[1] * 1e3:.2f} .. {ti[2] * 1e3:.2f}] {N / ti[0]:.3e} rows/s"
                f"   roots_batch(level=) {tr[0] * 1e3:>9.2f} ms [{tr[1] * 1e3:.2f} .. {tr[2] * 1e3:.2f}] {N / tr[0]:.3e} rows/s"
                f"   {tr[0] / ti[0]:.2f} x")
            say(f"               status: {int(np.sum(s == 1))} unique, {int(np.sum(s > 1))} not unique, {int(np.sum(s == 0))} not "
                f"reached, {int(np.sum(s < 0))} failed; on the {int(one.sum())} rows where roots_batch(level=) counts as many "
                f"solutions, x is its lowest root within {diff:.1e} (b - a)")
        del m
    say()
    say(f"solver kernels alone on {TRACE_ROWS} given fibres (rocprofv3 --kernel-trace --stats, 4 calls each, average per call):")
    for n in SOLVER_N:
        stats = trace(["--step", "solver", str(n)], lines)
        if stats is None:
            return finish(1)
        inv = [r for r in stats if "k_cheb1d_invert" in r[0]]
        cal = [r for r in stats if "k_cheb1d_calculus" in r[0]]
        if not inv or not cal:
            say(f"  n = {n}: solver kernels missing from the trace")
            return finish(1)
        ai, ac = inv[0][2] / inv[0][1], cal[0][2] / cal[0][1]
        say(f"  n = {n:>2}: k_cheb1d_invert {ai / 1e3:>10.1f} us ({TRACE_ROWS / ai * 1e9:.3e} fibres/s)   k_cheb1d_calculus "
            f"{ac / 1e3:>10.1f} us ({TRACE_ROWS / ac * 1e9:.3e} fibres/s)   {ac / ai:.1f} x")
    say()
    say(f"share of the kernel time of one call at N = {TRACE_ROWS} (rocprofv3 --kernel-trace --stats, 4 calls):")
    for name in CLASSES:
        for method in ("invert", "level"):
            stats = trace(["--step", "share", name, method], lines)
            if stats is None:
                return finish(1)
            total = sum(r[2] for r in stats)
            solve = sum(r[2] for r in stats if is_solve(r[0]))
            top = ", ".join(f"{r[0].split('(')[0].replace('void ', '')[:40]} {100.0 * r[2] / total:.1f} %" for r in stats[:4])
            say(f"  {name:>6} {'invert_batch' if method == 'invert' else 'roots_batch(level=)':>20}: solve {100.0 * solve / total:5.1f} %, "
                f"evaluation and the rest {100.0 * (total - solve) / total:5.1f} % of {total / 4e6:.2f} ms per call;  {top}")
    return finish(0)


if __name__ == "__main__":
    sys.exit(main())
