#!/usr/bin/env python3
"""Wall time of ``sobol_indices()`` on the device (host clock around the synchronous call, after warm-up) for
dense interpolants and a 64-piece spline, next to a vectorised NumPy host restatement of the same arithmetic
(one tensordot per axis, then masked sums).  Prints one line per case and the agreement of the two.

    python tools/sobol_probe.py                 # the table
    python tools/sobol_probe.py --profile       # only the 64^4 case, 2 warm-up + 5 calls: run under
                                                # rocprofv3 --kernel-trace --stats for kernel times

Kernel times come from the separate rocprofv3 run; this script does not claim any."""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from pychebyshev_amd import ChebyshevApproximation, ChebyshevSpline  # noqa: E402


def numpy_sobol(T):
    """Host restatement: coefficients by tensordot with the per-axis DCT matrix, energies c^2 pi^d 2^-z."""
    d = T.ndim
    C = T
    for k, n in enumerate(T.shape):
        m = np.arange(n)[:, None]
        i = np.arange(n)[None, :]
        M = (2.0 / n) * np.cos(np.pi * ((m * (2 * (n - 1 - i) + 1)) % (4 * n)) / (2.0 * n))
        M[0] *= 0.5
        C = np.moveaxis(np.tensordot(M, C, axes=([1], [k])), 0, k)
    z = np.zeros(T.shape, dtype=np.int8)
    for k, n in enumerate(T.shape):
        shape = [1] * d
        shape[k] = n
        z += (np.arange(n) > 0).astype(np.int8).reshape(shape)
    E = C * C * (math.pi ** d) * np.exp2(-z.astype(float))
    tot = E.sum()
    var = tot - E[(0,) * d]
    first, total = np.empty(d), np.empty(d)
    for k in range(d):
        line = [0] * d
        line[k] = slice(1, None)
        first[k] = E[tuple(line)].sum() / var
        total[k] = (tot - E.take(0, axis=k).sum()) / var
    return first, total, var


def timed(fn, reps):
    fn()
    fn()                                                   # warm-up: code objects, matrices, the handle's caches
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts))


def dense_cases():
    g2 = np.load(os.path.join(ROOT, "tests", "golden", "g2_bs5d.npz"))["tensor"]
    rng = np.random.default_rng(7)
    yield "11^5 (BS5)", g2
    yield "32^3", rng.standard_normal((32, 32, 32))
    yield "64^4", rng.standard_normal((64, 64, 64, 64))
    yield "65^3", rng.standard_normal((65, 65, 65))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile", action="store_true",
                    help="only 64^4: two warm-up calls, then five more (for rocprofv3; the trace holds all seven)")
    args = ap.parse_args()

    if args.profile:
        T = np.random.default_rng(7).standard_normal((64, 64, 64, 64))
        c = ChebyshevApproximation.from_values(T, 4, [[-1.0, 1.0]] * 4, [64] * 4)
        for _ in range(2 + 5):
            c.sobol_indices()
        print("profile run: 2 warm-up + 5 calls of sobol_indices() on 64^4 (each: 4 k_mode_product, k_sobol_energy, "
              "k_sobol_finish); read the last five calls' dispatches")
        return

    print(f"{'case':<22}{'elements':>12}{'device median ms':>18}{'device min ms':>15}{'NumPy host ms':>15}"
          f"{'max |dS|':>11}{'rel dVar':>11}")
    for name, T in dense_cases():
        d = T.ndim
        c = ChebyshevApproximation.from_values(T, d, [[-1.0, 1.0]] * d, list(T.shape))
        med, best = timed(c.sobol_indices, args.reps)
        res = c.sobol_indices()
        t0 = time.perf_counter()
        wf, wt, wv = numpy_sobol(T)
        host = time.perf_counter() - t0
        f = np.array([res["first_order"][k] for k in range(d)])
        t = np.array([res["total_order"][k] for k in range(d)])
        ds = max(np.max(np.abs(f - wf)), np.max(np.abs(t - wt)))
        print(f"{name:<22}{T.size:>12,}{med * 1e3:>18.3f}{best * 1e3:>15.3f}{host * 1e3:>15.1f}{ds:>11.1e}"
              f"{abs(res['variance'] - wv) / wv:>11.1e}", flush=True)

    # 64-piece 3-D spline: 4 x 4 x 4 pieces of 12^3 nodes
    knots = [[-0.5, 0.0, 0.5]] * 3
    rng = np.random.default_rng(8)
    vals = [rng.standard_normal((12, 12, 12)) for _ in range(64)]
    sp = ChebyshevSpline.from_values(vals, 3, [[-1.0, 1.0]] * 3, [12, 12, 12], knots)
    med, best = timed(sp.sobol_indices, args.reps)

    def host_spline():
        tv, fe, te = 0.0, np.zeros(3), np.zeros(3)
        for v in vals:
            f, t, var = numpy_sobol(v)
            vol = 0.5 ** 3
            tv += vol * var
            fe += vol * f * var
            te += vol * t * var
        return fe / tv, te / tv, tv
    t0 = time.perf_counter()
    wf, wt, wv = host_spline()
    host = time.perf_counter() - t0
    res = sp.sobol_indices()
    ds = max(max(abs(res["first_order"][k] - wf[k]) for k in range(3)), max(abs(res["total_order"][k] - wt[k]) for k in range(3)))
    print(f"{'spline 64 x 12^3':<22}{64 * 12 ** 3:>12,}{med * 1e3:>18.3f}{best * 1e3:>15.3f}{host * 1e3:>15.1f}{ds:>11.1e}"
          f"{abs(res['variance'] - wv) / wv:>11.1e}", flush=True)


if __name__ == "__main__":
    main()
