#!/usr/bin/env python3
"""Tensor-product grid evaluation against the pointwise route on the same grid (one MI355X).

    python tools/eval_grid_probe.py [--quick] > profiles/eval_grid_probe.txt 2>&1

Per shape:
  eval_grid        ChebyshevApproximation.eval_grid(axes, out=DeviceArray) -- device-resident result, the W_k built
                   and uploaded inside the call -- with the kernel form auto picks and with each form forced on every
                   pass (PCX_GRID_VARIANT=1 VALU, =2 MFMA); ChebyshevTT.eval_grid returns NumPy, so its time includes
                   the host's value cores on the grid and the download of the dense result (both are reported)
  pointwise        vectorized_eval_batch / eval_batch over the meshgrid, the batch already in HBM and the result left
                   there: the route a grid had to take before (to_dense still takes it)
  passes           one more eval_grid call under PCX_GRID_LOG=1: each pass timed on its own by device events, with the
                   bytes it writes; the LAST line of a shape is the last pass and its achieved write bandwidth

Times are host-clock medians over calls that end in a device synchronise, after warm-up calls of the same shape; each
timed window is at least MIN_WINDOW seconds.  Not a test, not read by bench.py."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pychebyshev_amd import ChebyshevApproximation, ChebyshevTT, _lib  # noqa: E402
from pychebyshev_amd.device import DeviceArray, trim_pool  # noqa: E402

MIN_WINDOW = 0.3
DENSE = [((11,) * 5, (20,) * 5), ((32,) * 3, (200,) * 3), ((12, 12), (1000, 1000)), ((64,) * 4, (32,) * 4)]
# beside the shapes above: few nodes per dimension and thin tiles, where the auto rule has to decide between the forms
RULE = [((5,) * 4, (40,) * 4), ((7,) * 3, (150,) * 3), ((3,) * 6, (12,) * 6), ((16, 16, 4), (300, 300, 4))]


def timed(fn, warm=3, min_window=MIN_WINDOW, max_reps=200):
    """median seconds per call; fn ends in a device synchronise"""
    for _ in range(warm):
        fn()
    times, t_all = [], time.perf_counter()
    while len(times) < 5 or (time.perf_counter() - t_all < min_window and len(times) < max_reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), len(times)


def mesh(axes):
    return np.column_stack([g.ravel() for g in np.meshgrid(*axes, indexing="ij")])


def with_variant(v, fn):
    os.environ["PCX_GRID_VARIANT"] = v
    try:
        return timed(fn)
    finally:
        os.environ["PCX_GRID_VARIANT"] = ""


def logged(fn, variant=""):
    if variant:
        print(f"  passes with PCX_GRID_VARIANT={variant} ({'VALU' if variant == '1' else 'MFMA'} on every pass):")
    sys.stdout.flush()
    os.environ["PCX_GRID_LOG"] = "1"
    os.environ["PCX_GRID_VARIANT"] = variant
    try:
        fn()
    finally:
        del os.environ["PCX_GRID_LOG"]
        os.environ["PCX_GRID_VARIANT"] = ""
    sys.stderr.flush()


def dense_shape(n, m, rng, ab=False):
    d = len(n)
    name = "x".join(map(str, n)) + " -> " + "x".join(map(str, m))
    model = ChebyshevApproximation.from_values(rng.standard_normal(n), d, [[-1.0, 1.0]] * d, list(n))
    axes = [np.sort(rng.uniform(-1.0, 1.0, mk)) for mk in m]
    dev = model._model().device
    out = DeviceArray.empty(m, dev)
    points = int(np.prod(m))
    t_auto, reps = timed(lambda: model.eval_grid(axes, out=out))
    t_valu, _ = with_variant("1", lambda: model.eval_grid(axes, out=out))
    t_mfma, _ = with_variant("2", lambda: model.eval_grid(axes, out=out))
    got = out.to_host()
    pts = DeviceArray.from_host(mesh(axes), dev)
    spec = [0] * d
    t_pw, reps_pw = timed(lambda: model.vectorized_eval_batch(pts, spec))
    want = model.vectorized_eval_batch(pts, spec).to_host().reshape(m)
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(f"{name}: {points:,} points")
    print(f"  eval_grid  auto {t_auto * 1e3:9.3f} ms ({reps} calls)   VALU on every pass {t_valu * 1e3:9.3f} ms   MFMA on every pass {t_mfma * 1e3:9.3f} ms")
    print(f"  pointwise       {t_pw * 1e3:9.3f} ms ({reps_pw} calls)   ratio pointwise / eval_grid(auto) = {t_pw / t_auto:.1f}x"
          f"   E_norm between the two = {err:.1e}", flush=True)
    logged(lambda: model.eval_grid(axes, out=out))
    if ab:
        for v in ("1", "2"):
            logged(lambda: model.eval_grid(axes, out=out), v)
    del pts, out, model
    trim_pool()


def tt_shape(name, cores, domain, m, rng):
    d = len(cores)
    tt = ChebyshevTT.from_coeff_cores(cores, domain)
    tt.to_device()
    axes = [np.sort(rng.uniform(a, b, mk)) for (a, b), mk in zip(domain, m)]
    points = int(np.prod(m))
    t_grid, reps = timed(lambda: tt.eval_grid(axes), warm=2)
    got = tt.eval_grid(axes)
    t_copy, _ = timed(lambda: DeviceArray.from_host(got).to_host(), warm=1)
    pts = DeviceArray.from_host(mesh(axes), tt._dev().device)
    t_pw, reps_pw = timed(lambda: tt.eval_batch(pts), warm=2)
    t_pwh, _ = timed(lambda: tt.eval_batch(pts).to_host(), warm=2)
    want = tt.eval_batch(pts).to_host().reshape(m)
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(f"{name}, ranks {tt.tt_ranks} -> " + "x".join(map(str, m)) + f": {points:,} points")
    print(f"  eval_grid (NumPy result) {t_grid * 1e3:9.3f} ms ({reps} calls), of which an upload + download of the dense result alone"
          f" takes {t_copy * 1e3:.3f} ms")
    print(f"  pointwise (device-resident) {t_pw * 1e3:9.3f} ms ({reps_pw} calls)   ratio pointwise / eval_grid = {t_pw / t_grid:.1f}x"
          f"   E_norm between the two = {err:.1e}")
    print(f"  pointwise with its result downloaded to NumPy as well {t_pwh * 1e3:9.3f} ms   ratio to eval_grid = {t_pwh / t_grid:.1f}x", flush=True)
    logged(lambda: tt.eval_grid(axes))
    for v in ("1", "2"):
        logged(lambda: tt.eval_grid(axes), v)
    del pts
    trim_pool()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small shapes only (a rehearsal of the script)")
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("eval_grid_probe: no GPU; nothing is measured without one")
    rng = np.random.default_rng(29)
    for n, m in ([((5, 6), (30, 40)), ((4, 5, 6), (9, 10, 11))] if args.quick else DENSE):
        dense_shape(n, m, rng)
    print("-- shapes for the auto rule: few nodes, thin tiles")
    for n, m in ([((3, 3), (20, 20))] if args.quick else RULE):
        dense_shape(n, m, rng, ab=True)
    print("-- tensor trains")
    g4 = np.load(os.path.join(ROOT, "tests", "golden", "g4_tt_bs5d.npz"))
    bs_domain = [[80.0, 120.0], [90.0, 110.0], [0.25, 1.0], [0.15, 0.35], [0.01, 0.08]]
    tt_shape("5-D Black-Scholes TT", [g4[f"r8_core{k}"] for k in range(5)], bs_domain, (6,) * 5 if args.quick else (25,) * 5, rng)
    ranks = [1] + [16] * 9 + [1]
    r16 = np.random.default_rng(16)
    cores = [r16.standard_normal((ranks[k], 11, ranks[k + 1])) / np.sqrt(ranks[k] * 11) for k in range(10)]
    tt_shape("10-D synthetic TT", cores, [[-1.0, 1.0]] * 10, (2,) * 10 if args.quick else (5,) * 10, rng)


if __name__ == "__main__":
    main()
