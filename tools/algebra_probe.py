#!/usr/bin/env python3
"""Wall time of TT algebra on the device against a NumPy restatement on the same host, and of a 100-trade dense
book, written to profiles/algebra_probe.txt (and printed).

  * ``a + b`` of two random TTs of rank r (d dims, n nodes): block-diagonal stacking plus ``pcx_tt_round``, against
    the same rounding in NumPy (QR right-to-left, truncated SVD left-to-right), both with max_rank r, tol 1e-10.
  * a full reversal by ``reorder`` (d (d-1) / 2 adjacent swaps, ``pcx_tt_reorder``) against the swaps in NumPy.
  * a 100-trade 11^5 dense book: the time to combine it (``w1 * t1 + ... + w100 * t100``), then one 10^6-point
    evaluation of the book against 100 separate evaluations of the trades.

    python tools/algebra_probe.py              # the table
    python tools/algebra_probe.py --profile    # two sums at (10, 16, 64): run under
                                               # rocprofv3 --kernel-trace --stats for kernel times
                                               # (reorder is left out: DESIGN 3.7)

Times are host wall clock around synchronous calls after one warm-up call; kernel times come from the rocprofv3 run."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pychebyshev_amd import ChebyshevApproximation, ChebyshevTT  # noqa: E402

SIZES = [(5, 11, 8), (10, 16, 16), (8, 16, 32), (10, 16, 64)]
TOL = 1e-10


def random_tt(d, n, r, seed):
    rng = np.random.default_rng(seed)
    rk = [1] + [r] * (d - 1) + [1]
    cores = [rng.standard_normal((rk[k], n, rk[k + 1])) / np.sqrt(rk[k] * n) for k in range(d)]
    tt = ChebyshevTT.from_coeff_cores(cores, [[-1.0, 1.0]] * d)
    tt.max_rank, tt.tolerance = r, TOL
    return tt


def keep_count(S, max_rank, tol):
    keep = min(max_rank, len(S))
    if S[0] > 0 and tol > 0:
        keep = max(1, min(keep, int(np.sum(S > tol * S[0]))))
    return max(1, keep)


def numpy_round(cores, max_rank, tol):
    cores = [c.copy() for c in cores]
    d = len(cores)
    for k in range(d - 1, 0, -1):
        rl, n, rr = cores[k].shape
        q, r = np.linalg.qr(cores[k].reshape(rl, n * rr).T)
        cores[k] = q.T.reshape(-1, n, rr)
        cores[k - 1] = np.einsum("ljs,sr->ljr", cores[k - 1], r.T)
    for k in range(d - 1):
        rl, n, rr = cores[k].shape
        u, s, vt = np.linalg.svd(cores[k].reshape(rl * n, rr), full_matrices=False)
        keep = keep_count(s, max_rank, tol)
        cores[k] = u[:, :keep].reshape(rl, n, keep)
        cores[k + 1] = np.einsum("lr,rjs->ljs", s[:keep, None] * vt[:keep], cores[k + 1])
    return cores


def numpy_stack(a, b):
    d = len(a)
    out = []
    for k in range(d):
        if k == 0:
            out.append(np.concatenate([a[k], b[k]], axis=2))
        elif k == d - 1:
            out.append(np.concatenate([a[k], b[k]], axis=0))
        else:
            c = np.zeros((a[k].shape[0] + b[k].shape[0], a[k].shape[1], a[k].shape[2] + b[k].shape[2]))
            c[:a[k].shape[0], :, :a[k].shape[2]] = a[k]
            c[a[k].shape[0]:, :, a[k].shape[2]:] = b[k]
            out.append(c)
    return out


def numpy_reverse(cores, max_rank, tol):
    cores = [c.copy() for c in cores]
    d = len(cores)
    order = list(range(d))
    target = order[::-1]
    for k in range(d):
        j = order.index(target[k])
        while j > k:
            i = j - 1
            a, b = cores[i], cores[i + 1]
            rl, na, _ = a.shape
            _, nb, rr = b.shape
            m = np.einsum("lab,brs->lars", a, b).transpose(0, 2, 1, 3).reshape(rl * nb, na * rr)
            u, s, vt = np.linalg.svd(m, full_matrices=False)
            keep = keep_count(s, max_rank, tol)
            cores[i] = (u[:, :keep] * s[:keep]).reshape(rl, nb, keep)
            cores[i + 1] = vt[:keep].reshape(keep, na, rr)
            order[i], order[j] = order[j], order[i]
            j -= 1
    return cores


def timed(fn, reps=1):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "algebra_probe.txt"))
    args = ap.parse_args()
    if args.profile:
        a, b = random_tt(10, 16, 64, 1), random_tt(10, 16, 64, 2)
        for _ in range(2):
            a + b
        return
    lines = ["# TT algebra on one MI355X vs NumPy on the same host (tools/algebra_probe.py); tol 1e-10, max_rank r",
             "# case                      device s    numpy s   speed-up  ranks (device)                  max |dev - numpy| / max|numpy|"]
    rng = np.random.default_rng(7)
    for d, n, r in SIZES:
        a, b = random_tt(d, n, r, 1), random_tt(d, n, r, 2)
        pts = rng.uniform(-1, 1, (2000, d))
        t_dev, s = timed(lambda: a + b)
        t_np, ref = timed(lambda: numpy_round(numpy_stack(a._coeff_cores, b._coeff_cores), r, TOL))
        ref_tt = ChebyshevTT.from_coeff_cores(ref, [[-1.0, 1.0]] * d)
        want = ref_tt.eval_batch(pts)
        err = float(np.max(np.abs(s.eval_batch(pts) - want)) / np.max(np.abs(want)))
        lines.append(f"add  (d={d:2d}, n={n}, r={r:2d})   {t_dev:9.4f} {t_np:10.4f} {t_np / t_dev:9.1f}x  "
                     f"{str(s.tt_ranks):30s}  {err:.2e}")
        print(lines[-1], flush=True)
        rev = list(range(d))[::-1]
        t_dev, s = timed(lambda: a.reorder(rev))
        t_np, ref = timed(lambda: numpy_reverse(a._coeff_cores, r, TOL))
        ref_tt = ChebyshevTT.from_coeff_cores(ref, [[-1.0, 1.0]] * d, dim_order=rev)
        want = ref_tt.eval_batch(pts)
        err = float(np.max(np.abs(s.eval_batch(pts) - want)) / np.max(np.abs(want)))
        lines.append(f"rev  (d={d:2d}, n={n}, r={r:2d})   {t_dev:9.4f} {t_np:10.4f} {t_np / t_dev:9.1f}x  "
                     f"{str(s.tt_ranks):30s}  {err:.2e}")
        print(lines[-1], flush=True)

    # ---- a 100-trade 11^5 dense book
    dom = [[80.0, 120.0], [90.0, 110.0], [0.25, 1.0], [0.15, 0.35], [0.01, 0.08]]
    trades = [ChebyshevApproximation.from_values(rng.standard_normal((11,) * 5), 5, dom, [11] * 5) for _ in range(100)]
    w = rng.uniform(-1, 1, 100)

    def combine():
        book = trades[0] * float(w[0])
        for wi, t in zip(w[1:], trades[1:]):
            book = book + wi * t
        return book

    t_combine, book = timed(combine)
    pts = np.column_stack([rng.uniform(lo, hi, 1_000_000) for lo, hi in dom])
    spec = [0] * 5
    for t in trades:
        t.vectorized_eval_batch(pts[:10], spec)             # device models built before timing
    t_book, yb = timed(lambda: book.vectorized_eval_batch(pts, spec))
    t_sep, ys = timed(lambda: sum(wi * t.vectorized_eval_batch(pts, spec) for wi, t in zip(w, trades)))
    err = float(np.max(np.abs(yb - ys)) / np.max(np.abs(ys)))
    lines.append(f"book 100 x 11^5: combine {t_combine:.4f} s; 10^6 points: book {t_book:.4f} s, "
                 f"100 separate evaluations {t_sep:.4f} s ({t_sep / t_book:.1f}x); max diff / max {err:.2e}")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
