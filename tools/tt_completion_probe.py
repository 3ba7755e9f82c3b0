#!/usr/bin/env python3
"""Time per outer ALS iteration of ``ChebyshevTT.run_completion`` (``pcx_tt_als``) on one MI355X, written to
profiles/tt_completion_probe.txt (and printed).

  * two grids: 11^5 at rank 8 (the bench's 5-D shape) and 16^6 at rank 12 (1.7e7 points, 134 MB);
  * milliseconds per outer iteration = (wall time of 1 + K iterations - wall time of 1 iteration) / K, tolerance 0.0 so
    that the counts are fixed: the upload of the target, the allocations and the host-side conversions cancel;
    median of REPEATS such differences after one warm-up call of each length (guide "measuring on MI355X");
  * the bytes the kernels of one iteration read and write (counted from the shapes of every contraction, the
    reconstruction and the norms) divided by that time, next to the measured device copy rate of 6.29 TB/s;
  * the same iteration in host NumPy, projection form (one iteration, timed once for 16^6);
  * the reference's recorded seconds for M16 and M5 from tests/golden/g23_tt_completion.npz;
  * VALU form against MFMA form of the two contractions at ranks 4 .. 32: each in a fresh child process with
    PCX_TT_ALS_MFMA_MIN = 999 (VALU always) or 1 (MFMA always).  This table is what the switch at rank 16 rests on.

    python tools/tt_completion_probe.py
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE_TBS = 6.29
REPEATS = 5
EXTRA = 4            # K: iterations added to the second call
FORM_CASES = [(5, 11, 4), (5, 11, 8), (5, 11, 12), (5, 11, 16), (5, 11, 24), (6, 16, 8), (6, 16, 12), (6, 16, 16), (6, 16, 32)]


def dense(cores):
    out = cores[0]
    for c in cores[1:]:
        out = np.einsum("...i,ijk->...jk", out, c)
    return out[0, ..., 0]


def make_case(d, n, r, seed=1):
    """A rank-r target with 1e-3 relative noise (so every iteration has something to fit) and random start cores."""
    rng = np.random.default_rng(seed)
    rk = [1] + [r] * (d - 1) + [1]
    T = dense([rng.standard_normal((rk[k], n, rk[k + 1])) / np.sqrt(rk[k]) for k in range(d)])
    T += 1e-3 * np.sqrt(np.mean(T * T)) * rng.standard_normal(T.shape)
    start = [rng.standard_normal((rk[k], n, rk[k + 1])) / np.sqrt(rk[k] * n) for k in range(d)]
    return T, start


def numpy_iteration(cores, T):
    """One outer iteration in projection form; the cores come in right-orthonormal."""
    n, d = T.shape, len(cores)
    P = T.reshape(1, -1)
    for k in range(d):
        rl = P.shape[0]
        C = X = P.reshape(rl * n[k], -1)
        for j in range(d - 1, k, -1):
            Cj = cores[j].reshape(cores[j].shape[0], -1)
            C = C.reshape(-1, Cj.shape[1]) @ Cj.T
        cores[k] = C.reshape(rl, n[k], -1)
        if k < d - 1:
            Q, _ = np.linalg.qr(C.reshape(rl * n[k], -1))
            cores[k], P = Q.reshape(rl, n[k], -1), Q.T @ X
    S = T.reshape(-1, 1)
    for k in range(d - 1, -1, -1):
        rr = S.shape[1]
        C = X = S.reshape(-1, n[k] * rr)
        for j in range(k):
            Qj = cores[j].reshape(-1, cores[j].shape[2])
            C = Qj.T @ C.reshape(Qj.shape[0], -1)
        cores[k] = C.reshape(-1, n[k], rr)
        if k > 0:
            Q, _ = np.linalg.qr(C.reshape(-1, n[k] * rr).T)
            cores[k], S = Q.T.reshape(-1, n[k], rr), X @ Q
    return cores


def right_orthonormal(cores):
    cores = [c.copy() for c in cores]
    for k in range(len(cores) - 1, 0, -1):
        r0, nk, r1 = cores[k].shape
        Q, R = np.linalg.qr(cores[k].reshape(r0, -1).T)
        cores[k], cores[k - 1] = Q.T.reshape(-1, nk, r1), np.einsum("anb,cb->anc", cores[k - 1], R)
    return cores


def bytes_per_iteration(d, n, r):
    """Doubles read + written by the kernels of one steady-state outer iteration (ranks r, none shrinking), times 8."""
    G = n ** d
    rk = [1] + [min(r, n ** k, n ** (d - k)) for k in range(1, d)] + [1]
    total = 0
    for k in range(d - 1):                                   # left to right
        psize = rk[k] * n ** (d - k)
        if k > 0:                                            # core 0 holds its solution already
            x = psize
            for j in range(d - 1, k, -1):
                y = x // (n * rk[j + 1]) * rk[j]
                total += x + y
                x = y
        total += psize + psize // (rk[k] * n) * rk[k + 1]    # P_{k+1} = Q_k^T P_k
    for k in range(d - 1, 0, -1):                            # right to left
        ssize = n ** (k + 1) * rk[k + 1]
        if k < d - 1:
            x = ssize
            for j in range(k):
                y = x // (rk[j] * n) * rk[j + 1]
                total += x + y
                x = y
        total += ssize + ssize // (n * rk[k + 1]) * rk[k]
    rows = n
    for k in range(1, d):                                    # reconstruction
        total += rows * rk[k] + rows * n * rk[k + 1]
        rows *= n
    total += 3 * G                                           # norms
    return 8 * total


def child(d, n, r):
    from pychebyshev_amd import ChebyshevTT
    T, start = make_case(d, n, r)
    dom = [[-1.0, 1.0]] * d

    def run(iters):
        tt = ChebyshevTT.from_coeff_cores(start, dom)
        t0 = time.perf_counter()
        tt.run_completion(tolerance=0.0, max_iter=iters, values=T)
        return time.perf_counter() - t0, tt

    run(1)
    run(1 + EXTRA)
    diffs, ones = [], []
    for _ in range(REPEATS):
        t1, _ = run(1)
        tk, tt = run(1 + EXTRA)
        diffs.append((tk - t1) / EXTRA)
        ones.append(t1)
    print(json.dumps({"ms_iter": 1e3 * float(np.median(diffs)), "ms_iter_min": 1e3 * float(np.min(diffs)),
                      "ms_iter_max": 1e3 * float(np.max(diffs)), "s_first": float(np.median(ones)),
                      "residual": tt.completion_info["grid_residual"], "ranks": tt.tt_ranks}))


def spawn(d, n, r, mfma_min=None):
    env = dict(os.environ)
    env.pop("PCX_TT_ALS_MFMA_MIN", None)
    if mfma_min is not None:
        env["PCX_TT_ALS_MFMA_MIN"] = str(mfma_min)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(d), str(n), str(r)], env=env,
                         capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        raise SystemExit(f"child ({d}, {n}, {r}, {mfma_min}) failed with {res.returncode}:\n{res.stderr[-2000:]}")
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=3, type=int)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tt_completion_probe.txt"))
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    lines = ["# run_completion (pcx_tt_als) on one MI355X: time per outer ALS iteration (tools/tt_completion_probe.py)",
             f"# ms / iteration = (t[1 + {EXTRA} iterations] - t[1 iteration]) / {EXTRA}, median (min .. max) of {REPEATS}; "
             f"bytes = reads + writes of every kernel of one iteration",
             "# grid      rank  ms/iter (min .. max)        MB/iter   TB/s  of 6.29   first call s  numpy s/iter  speed-up  grid residual"]
    for d, n, r in ((5, 11, 8), (6, 16, 12)):
        got = spawn(d, n, r)
        T, start = make_case(d, n, r)
        cores = right_orthonormal(start)
        if n ** d < 10 ** 6:
            numpy_iteration([c.copy() for c in cores], T)       # warm-up (the large grid is timed cold, once)
        t0 = time.perf_counter()
        numpy_iteration(cores, T)
        t_np = time.perf_counter() - t0
        b = bytes_per_iteration(d, n, r)
        rate = b / (got["ms_iter"] * 1e-3) / 1e12
        lines.append(f"{n}^{d:<6d} {r:5d}  {got['ms_iter']:8.3f} ({got['ms_iter_min']:.3f} .. {got['ms_iter_max']:.3f})  "
                     f"{b / 1e6:9.1f}  {rate:5.2f}  {100 * rate / COPY_RATE_TBS:5.1f} %  {got['s_first']:12.3f}  {t_np:12.4f}  "
                     f"{t_np / (got['ms_iter'] * 1e-3):8.1f}x  {got['residual']:.2e}")
        print(lines[-1], flush=True)
    g = np.load(os.path.join(ROOT, "tests", "golden", "g23_tt_completion.npz"))
    lines.append("# the reference (dense lstsq per core, CPU), recorded by the golden generator: three outer iterations")
    for tag in ("M16", "M5"):
        shape = "x".join(str(int(v)) for v in g[f"{tag}_n"])
        lines.append(f"reference {tag} ({shape}): {float(g[f'{tag}_ref_seconds'][1]):.1f} s for 3 iterations "
                     f"= {float(g[f'{tag}_ref_seconds'][1]) / 3:.2f} s / iteration")
        print(lines[-1], flush=True)
    lines.append("# VALU form (one output column or row per lane) against MFMA form (v_mfma_f64_16x16x4_f64) of both contractions")
    lines.append("# grid      rank   VALU ms/iter   MFMA ms/iter   MFMA / VALU")
    for d, n, r in FORM_CASES:
        valu, mfma = spawn(d, n, r, 999), spawn(d, n, r, 1)
        lines.append(f"{n}^{d:<6d} {r:5d}  {valu['ms_iter']:12.3f}  {mfma['ms_iter']:12.3f}  {mfma['ms_iter'] / valu['ms_iter']:10.2f}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
