#!/usr/bin/env python3
"""Fibres per second of the batched roots / minimum solver (``roots_batch`` / ``minimize_batch``: expand, evaluate,
``k_cheb1d_calculus``) on a 5-D dense model whose first dimension has n in {11, 16, 32, 64} nodes, for N in
{10^3, 10^4, 10^5} rows (host clock around the synchronous call, after warm-up), next to the reference-shaped host
loop over the same rows (``slice`` to 1-D on the device, then NumPy ``chebroots`` per row) on a sample of rows.

    python tools/calculus_probe.py              # the table
    python tools/calculus_probe.py --profile    # n = 11 and 64 at N = 10^4 only, 1 warm-up + 3 calls each: run under
                                                # rocprofv3 --kernel-trace --stats for the kernel split

Kernel times come from the separate rocprofv3 run; this script does not claim any."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pychebyshev_amd import ChebyshevApproximation, _calculus  # noqa: E402
from pychebyshev_amd.barycentric import chebyshev_nodes  # noqa: E402

DOMAIN = [[80.0, 120.0], [0.25, 1.0], [0.15, 0.35], [0.01, 0.08], [0.0, 0.05]]


def model(n):
    """A smooth 5-D tensor (n x 7^4) with a few sign changes along dimension 0."""
    grids = [chebyshev_nodes(lo, hi, m) for (lo, hi), m in zip(DOMAIN, [n, 7, 7, 7, 7])]
    X = np.meshgrid(*grids, indexing="ij")
    T = np.sin(0.3 * (X[0] - 100.0)) * (1.0 + X[1]) + X[2] - 0.25 + 10.0 * X[3] * np.cos(40.0 * X[4])
    return ChebyshevApproximation.from_values(T, 5, DOMAIN, [n, 7, 7, 7, 7])


def rows(N, seed=0):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(lo, hi, N) for lo, hi in DOMAIN[1:]])


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if args.profile:
        for n in (11, 64):
            c, R = model(n), rows(10_000)
            for _ in range(4):
                c.roots_batch(0, R)
        print("profile run done")
        return
    print(f"{'n':>3} {'N':>7} {'roots ms':>10} {'roots fibres/s':>15} {'min ms':>10} {'min fibres/s':>14} "
          f"{'host loop ms/row':>17}")
    for n in (11, 16, 32, 64):
        c = model(n)
        sample = rows(50, seed=1)
        c.slice([(k + 1, float(v)) for k, v in enumerate(sample[0])])          # warm-up
        t0 = time.perf_counter()
        for r in sample:
            sl = c.slice([(k + 1, float(v)) for k, v in enumerate(r)])
            _calculus.roots_1d(sl.tensor_values, tuple(DOMAIN[0]))
        host = (time.perf_counter() - t0) / len(sample)
        for N in (1_000, 10_000, 100_000):
            R = rows(N)
            reps = 5 if N <= 10_000 else 2
            tr = timed(lambda: c.roots_batch(0, R), reps)
            tm = timed(lambda: c.minimize_batch(0, R), reps)
            print(f"{n:>3} {N:>7} {tr * 1e3:>10.2f} {N / tr:>15.3e} {tm * 1e3:>10.2f} {N / tm:>14.3e} {host * 1e3:>17.3f}",
                  flush=True)
        Rs = rows(200, seed=2)
        got, cnt = c.roots_batch(0, Rs)
        bad = 0
        for i, r in enumerate(Rs):
            sl = c.slice([(k + 1, float(v)) for k, v in enumerate(r)])
            want = _calculus.roots_1d(sl.tensor_values, tuple(DOMAIN[0]))
            bad += want.size != cnt[i] or (want.size and np.max(np.abs(want - got[i, :cnt[i]])) > 1e-10 * 40.0)
        print(f"    n={n}: 200 rows against slice + chebroots: {200 - bad} agree", flush=True)


if __name__ == "__main__":
    main()
