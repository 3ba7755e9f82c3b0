#!/usr/bin/env python3
"""Time of one ALS step on scattered samples (``pcx_tt_fit_normal``, csrc/tt_fit_kernels.h) and of a whole
``ChebyshevTT.fit_samples`` iteration, next to the NumPy restatement of the step on the host.

Models: the 5-D shape of BASELINE config 3 (ranks [1,8,8,8,6,1], n = 11; the step at position 2 has P = 704 unknowns) and
the shape of config 5 (10-D, rank 16, n = 11; position 4, P = 2816), at N = 10^5 and 10^6 samples resident on the device.

  kernels ms      the three kernels of one step (interface vectors, Gram, reduction) from the events the library records
                  around them: one warm-up call, the median of ``--steps`` calls
  step ms         the whole call on the host's clock: the upload of the cores, the kernels, the download of G (P^2 doubles)
  of peak         the step's N P^2 FMAs over the Gram kernel's time, as a fraction of the FP64 matrix peak (78.6 TFLOP/s
                  = 39.3 x 10^12 FMA/s)
  host ms         the restatement: the design rows by einsum and ``A.T @ A`` through the host BLAS with ``--threads``
                  threads, timed on ``--host-rows`` rows and scaled by N over that (the work is linear in N; the full
                  N x P matrix of the 10-D shape at 10^6 rows is 22 GB)
  iteration s     one outer iteration of ``fit_samples`` (2 d - 2 steps with their host Cholesky solves and QR moves,
                  then the residual), wall clock: one warm-up, the median of ``--iters`` calls; a starred figure is a
                  single call without a warm-up (``--single-call-flops``)

    python tools/tt_fit_probe.py [--steps 5] [--iters 5] [--sizes 100000 1000000] [--out profiles/tt_fit_probe.txt]
"""
import argparse
import ctypes
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--host-rows", type=int, default=32768)
ap.add_argument("--single-call-flops", type=float, default=5e12,
                help="a (shape, N) whose iteration needs more FMAs than this is timed once, without a warm-up")
ap.add_argument("--out", default=None)
args = ap.parse_args()
for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[var] = str(args.threads)          # before NumPy loads its BLAS

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pychebyshev_amd import _lib  # noqa: E402
from pychebyshev_amd import tensor_train as tt_mod  # noqa: E402
from pychebyshev_amd.device import DeviceArray  # noqa: E402
from tt_deriv_probe import SHAPES, make_model  # noqa: E402

PEAK_FMA = 39.3e12
POSITION = {5: 2, 10: 4}


def host_step_ms(cores, pts, y, k):
    """The restatement's step on the host: bases by the recurrence, interface vectors and design rows by einsum,
    G = A^T A and b = A^T y through the BLAS."""
    t0 = time.perf_counter()
    d = len(cores)
    Ts = []
    for m in range(d):
        n = cores[m].shape[1]
        t = pts[:, m]                                      # the probe's domain is [-1, 1]
        T = np.empty((pts.shape[0], n))
        T[:, 0] = 1.0
        T[:, 1] = t
        for j in range(2, n):
            T[:, j] = 2.0 * t * T[:, j - 1] - T[:, j - 2]
        Ts.append(T)
    L = np.ones((pts.shape[0], 1))
    for m in range(k):
        L = np.einsum("ia,ij,ajb->ib", L, Ts[m], cores[m], optimize=True)
    R = np.ones((pts.shape[0], 1))
    for m in range(d - 1, k, -1):
        R = np.einsum("ajb,ij,ib->ia", cores[m], Ts[m], R, optimize=True)
    A = (L[:, :, None, None] * Ts[k][:, None, :, None] * R[:, None, None, :]).reshape(pts.shape[0], -1)
    G = A.T @ A
    b = A.T @ y
    return (time.perf_counter() - t0) * 1e3, G, b


def main():
    out = args.out or os.path.join(ROOT, "profiles", "tt_fit_probe.txt")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"{'model':<40} {'N':>8} {'P':>5} {'interface ms':>12} {'Gram ms':>9} {'reduce ms':>9} {'step ms':>9} {'of peak':>8} "
        f"{'host ms':>10} {'host/step':>9} {'iteration s':>11}  G against the host, normwise")
    for name, (ranks, n) in SHAPES.items():
        tt = make_model(ranks, n, 31)
        d = tt.num_dimensions
        k = POSITION[d]
        cores = [np.array(c) for c in tt._coeff_cores]
        for kk in range(d - 1, 0, -1):                     # the state a step sees: the other cores orthonormal
            tt_mod._fit_move_centre(cores, kk, kk - 1)
        for kk in range(k):
            tt_mod._fit_move_centre(cores, kk, kk + 1)
        P = cores[k].size
        for N in args.sizes:
            rng = np.random.default_rng(5)
            pts = rng.uniform(-1.0, 1.0, (N, d))
            y = np.sin(pts.sum(axis=1))
            session = tt_mod._FitSession(tt, DeviceArray.from_host(pts), DeviceArray.from_host(y), N)
            ms = (ctypes.c_float * 3)()
            kern, wall = [], []
            for rep in range(args.steps + 1):
                t0 = time.perf_counter()
                G, b = session.normal(cores, k)
                t1 = time.perf_counter()
                _lib.check(session.lib.pcx_tt_fit_times(session.handle, ms), session.lib)
                if rep:                                     # the first call is the warm-up
                    kern.append([float(v) for v in ms])
                    wall.append((t1 - t0) * 1e3)
            ki, kg, kr = (float(np.median([t[i] for t in kern])) for i in range(3))
            step = float(np.median(wall))
            session.close()
            rows = min(N, args.host_rows)
            host_step_ms(cores, pts[:rows], y[:rows], k)                       # warm-up
            host = [host_step_ms(cores, pts[:rows], y[:rows], k)[0] for _ in range(3)]
            host_ms = float(np.median(host)) * (N / rows)
            if rows == N:
                Gh = host_step_ms(cores, pts, y, k)[1]
                dist = f"{np.linalg.norm(G - Gh) / np.linalg.norm(Gh):.2e}"
            else:
                s2 = tt_mod._FitSession(tt, pts[:rows], y[:rows], rows)
                Gs = s2.normal(cores, k)[0]
                s2.close()
                Gh = host_step_ms(cores, pts[:rows], y[:rows], k)[1]
                dist = f"{np.linalg.norm(Gs - Gh) / np.linalg.norm(Gh):.2e} (first {rows} rows)"
            flops = sum(float(N) * c.size ** 2 for c in cores) * 2
            single = flops > args.single_call_flops
            times = []
            for rep in range(1 if single else args.iters + 1):
                model = make_model(ranks, n, 31)
                t0 = time.perf_counter()
                model.fit_samples(pts, y, max_iter=1)
                if rep or single:
                    times.append(time.perf_counter() - t0)
            iteration = f"{float(np.median(times)):.3f}" + ("*" if single else "")
            say(f"{name:<40} {N:>8} {P:>5} {ki:>12.3f} {kg:>9.3f} {kr:>9.3f} {step:>9.3f} {N * P * P / (kg * 1e-3) / PEAK_FMA:>8.3f} "
                f"{host_ms:>10.1f} {host_ms / step:>9.2f} {iteration:>11}  {dist}")
    say("* one call, no warm-up")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
