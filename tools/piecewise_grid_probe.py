#!/usr/bin/env python3
"""``ChebyshevSpline.eval_grid`` / ``ChebyshevSlider.eval_grid`` against the routes a grid had to take before (one MI355X).

    python tools/piecewise_grid_probe.py [--quick] > profiles/piecewise_grid_probe.txt 2>&1

Per shape:
  eval_grid        ``eval_grid(axes, out=DeviceArray)`` -- device-resident result; the plan, the tables and every piece's
                   (slide's) weight matrices are built and uploaded inside the call -- and the same call returning NumPy
  pointwise        the class's ``eval_batch`` over the meshgrid, the batch already in HBM and the result left there
  host composition a Python loop of per-piece (per-slide) ``eval_grid`` calls plus the NumPy assembly of
                   tests/test_gpu_piecewise_grid.py (``np.ix_`` placement; broadcast sum): what a caller could do
                   with ``ChebyshevApproximation.eval_grid`` alone; its result is a NumPy array
  assembly         two more calls under PCX_PIECEWISE_GRID_LOG=1: k_spline_grid_place / k_slider_grid_sum timed on its own
                   by device events, with the bytes it writes and its achieved write bandwidth (to set beside the
                   1.3 - 1.6 TB/s of the last mode-product pass in profiles/eval_grid_probe.txt): first the `_run` form
                   (multi-index decoded once per lane, then walked), then the per-element decode
                   (PCX_PIECEWISE_GRID_DECODE=1), which is also timed as a whole call

Times are host-clock medians over calls that end in a device synchronise, after warm-up calls of the same shape; each
timed window is at least MIN_WINDOW seconds (timed() of tools/eval_grid_probe.py).  Not a test, not read by bench.py."""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import generate_golden_piecewise_grid as G  # noqa: E402
from eval_grid_probe import mesh, timed  # noqa: E402
from pychebyshev_amd import ChebyshevSlider, ChebyshevSpline, _lib  # noqa: E402
from pychebyshev_amd.device import DeviceArray, trim_pool  # noqa: E402


def f64(x, _=None):
    return math.sin(3.0 * x[0]) * math.exp(0.5 * x[1]) + abs(x[0] - 0.1) + abs(x[1] + 0.2) * x[2] + abs(x[2] - 0.3)


def spline_pieces(sp, axes, spec):
    d = sp.num_dimensions
    iv = [G.route(sp.knots[k], sp._shape[k], axes[k]) for k in range(d)]
    out = np.empty(tuple(len(a) for a in axes))
    for multi in np.ndindex(*sp._shape):
        pos = [np.flatnonzero(iv[k] == multi[k]) for k in range(d)]
        if all(p.size for p in pos):
            piece = sp._pieces[int(np.ravel_multi_index(multi, sp._shape))]
            out[np.ix_(*pos)] = piece.eval_grid([axes[k][pos[k]] for k in range(d)], spec)
    return out


def slider_slides(sl, axes, spec):
    d = sl.num_dimensions
    shape = tuple(len(a) for a in axes)
    res = np.full(shape, float(sl.pivot_value))
    for s, group in enumerate(sl.partition):
        g = sl.slides[s].eval_grid([axes[k] for k in group], [0] * len(group))
        view = [1] * d
        for k in group:
            view[k] = shape[k]
        res = res + (np.transpose(g, np.argsort(group)).reshape(view) - float(sl.pivot_value))
    return res


def logged(fn, decode=""):
    sys.stdout.flush()
    os.environ["PCX_PIECEWISE_GRID_LOG"] = "1"
    os.environ["PCX_PIECEWISE_GRID_DECODE"] = decode
    try:
        fn()
    finally:
        del os.environ["PCX_PIECEWISE_GRID_LOG"]
        os.environ["PCX_PIECEWISE_GRID_DECODE"] = ""
    sys.stderr.flush()


def shape(name, obj, m, rng, compose):
    d = obj.num_dimensions
    axes = [np.sort(rng.uniform(lo, hi, mk)) for (lo, hi), mk in zip(obj.domain, m)]
    dev = obj._dev().device
    points = int(np.prod(m))
    spec = [0] * d
    out = DeviceArray.empty(m, dev)
    t_dev, reps = timed(lambda: obj.eval_grid(axes, out=out))
    os.environ["PCX_PIECEWISE_GRID_DECODE"] = "1"
    t_div, _ = timed(lambda: obj.eval_grid(axes, out=out))
    os.environ["PCX_PIECEWISE_GRID_DECODE"] = ""
    t_np, _ = timed(lambda: obj.eval_grid(axes))
    got = out.to_host()
    t_host, reps_h = timed(lambda: compose(obj, axes, spec), warm=1, max_reps=20)
    same = np.array_equal(got, compose(obj, axes, spec))
    pts = DeviceArray.from_host(mesh(axes), dev)
    t_pw, reps_pw = timed(lambda: obj.eval_batch(pts, spec), warm=2, max_reps=50)
    want = obj.eval_batch(pts, spec).to_host().reshape(m)
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(f"{name} -> " + "x".join(map(str, m)) + f": {points:,} points")
    print(f"  eval_grid  out=DeviceArray {t_dev * 1e3:9.3f} ms ({reps} calls)   with the per-element decode {t_div * 1e3:9.3f} ms"
          f"   NumPy result {t_np * 1e3:9.3f} ms")
    print(f"  pointwise (device-resident) {t_pw * 1e3:9.3f} ms ({reps_pw} calls)   ratio pointwise / eval_grid(out=DeviceArray) = {t_pw / t_dev:.1f}x"
          f"   E_norm between the two = {err:.1e}")
    print(f"  host composition (NumPy result) {t_host * 1e3:9.3f} ms ({reps_h} calls)   ratio to eval_grid(NumPy result) = {t_host / t_np:.1f}x"
          f"   bit-identical to eval_grid: {same}", flush=True)
    logged(lambda: obj.eval_grid(axes, out=out))
    logged(lambda: obj.eval_grid(axes, out=out), decode="1")
    del pts, out
    trim_pool()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small grids only (a rehearsal of the script)")
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("piecewise_grid_probe: no GPU; nothing is measured without one")
    rng = np.random.default_rng(32)
    q = args.quick
    sp_m = G.SP.build(ChebyshevSpline, "m")
    shape("spline m: 3-D, 4x1x2 = 8 pieces of 9x7x6 nodes", sp_m, (12, 9, 10) if q else (200,) * 3, rng, spline_pieces)
    shape("spline m on a small grid", sp_m, (9, 1, 18), rng, spline_pieces)
    sp_z = G.SP.build(ChebyshevSpline, "z")
    shape("spline z: 2-D, 2x1 = 2 pieces of 8x5 nodes", sp_z, (30, 40) if q else (1000, 1000), rng, spline_pieces)
    sp64 = ChebyshevSpline(f64, 3, [[-1.0, 1.0]] * 3, [8, 8, 8], knots=[[-0.5, 0.1, 0.6], [-0.6, -0.2, 0.5], [-0.4, 0.3, 0.7]])
    sp64.build(verbose=False)
    shape("spline: 3-D, 4x4x4 = 64 pieces of 8x8x8 nodes", sp64, (20, 21, 22) if q else (200,) * 3, rng, spline_pieces)
    shape("the 64-piece spline on a small grid", sp64, (16, 16, 16), rng, spline_pieces)
    print("-- sliders")
    sl_b = G.SL.build(ChebyshevSlider, "b")
    shape("slider b: [[0, 1], [2], [3, 4]], nodes 9, 9, 7, 7, 5", sl_b, (4, 5, 6, 3, 4) if q else (20,) * 5, rng, slider_slides)
    shape("slider b on a small grid", sl_b, (2, 3, 5, 1, 4), rng, slider_slides)
    sl_a = G.SL.build(ChebyshevSlider, "a")
    shape("slider a: three 1-D slides of 11 nodes", sl_a, (12, 9, 10) if q else (200,) * 3, rng, slider_slides)


if __name__ == "__main__":
    main()
