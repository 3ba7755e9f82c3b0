#!/usr/bin/env python3
"""Rows per second of the slider's batched calculus and box integrals (``roots_batch`` / ``minimize_batch``:
``pcx_slider_calculus_batch``; ``integrate_batch``: ``pcx_slider_box_batch``) on two sliders -- "a": three
one-dimensional slides of 11 nodes, "b": the mixed partition [[0, 1], [2], [3, 4]] with 9, 9, 7, 7, 5 nodes -- next to

  * the loop of single calls (``roots`` / ``minimize`` / ``integrate_batch`` of one row) over a sample of the same rows,
  * the floor: ``pcx_bary_calculus_batch`` / ``pcx_bary_box_batch`` on the owner slide ALONE for the same row count
    (its own columns of the rows).  A slider call does that work plus the other slides' evaluations or box integrals.

    python tools/slider_calculus_probe.py                 # every step, each in a child process under its own time limit
    python tools/slider_calculus_probe.py --step a        # one step in this process

Host clock around the synchronous calls (each ends in a download), one warm-up call per shape, then REPEATS timed calls:
the median is reported with the fastest and slowest call.  Kernel times are not claimed."""
import argparse
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ROWS = 200_000
N_SINGLE = 200
REPEATS = 7
STEP_LIMIT_S = 240

SHAPES = {
    "a": dict(d=3, domain=[[-1.0, 1.0]] * 3, n_nodes=[11, 11, 11], partition=[[0], [1], [2]], pivot=[0.1, -0.2, 0.3],
              f=lambda x, _=None: math.sin(3.0 * x[0]) + math.sin(2.0 * x[1]) + x[2] * x[2] - 0.4,
              dim=0, box_dims=[0, 2]),
    "b": dict(d=5, domain=[[-1.0, 1.0]] * 5, n_nodes=[9, 9, 7, 7, 5], partition=[[0, 1], [2], [3, 4]],
              pivot=[0.1, -0.2, 0.3, 0.0, 0.2],
              f=lambda x, _=None: (math.sin(3.0 * x[0]) * math.cos(x[1]) + 0.5 * x[2] * x[2] - 0.2
                                   + 0.3 * x[3] * math.exp(0.5 * x[4])),
              dim=0, box_dims=[1, 2, 3]),
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


def step(tag):
    from pychebyshev_amd import ChebyshevSlider
    c = SHAPES[tag]
    d, dim = c["d"], c["dim"]
    sl = ChebyshevSlider(c["f"], d, c["domain"], c["n_nodes"], partition=c["partition"], pivot_point=c["pivot"])
    sl.build(verbose=False)
    rng = np.random.default_rng(11)
    dom = np.asarray(c["domain"])
    pts = dom[:, 0] + (dom[:, 1] - dom[:, 0]) * rng.uniform(0.02, 0.98, (N_ROWS, d))
    others = [k for k in range(d) if k != dim]
    fixed = np.ascontiguousarray(pts[:, others])
    owner = sl._dim_to_slide[dim]
    group = list(sl.partition[owner])
    slide = sl.slides[owner]
    own_fixed = np.ascontiguousarray(pts[:, [k for k in group if k != dim]])
    print(f"shape {tag}: partition {c['partition']}, nodes {c['n_nodes']}, along dimension {dim} "
          f"(owner slide {owner}, group {group})")
    line("slider roots_batch", N_ROWS, timed(lambda: sl.roots_batch(dim, fixed)))
    line("slider minimize_batch", N_ROWS, timed(lambda: sl.minimize_batch(dim, fixed)))
    line("floor: owner slide alone, roots_batch", N_ROWS, timed(lambda: slide.roots_batch(group.index(dim), own_fixed)))
    line("floor: owner slide alone, minimize_batch", N_ROWS, timed(lambda: slide.minimize_batch(group.index(dim), own_fixed)))
    singles = [{k: float(v) for k, v in zip(others, row)} for row in fixed[:N_SINGLE]]
    line("loop of roots(dim, fixed)", N_SINGLE, timed(lambda: [sl.roots(dim, fx) for fx in singles]))
    line("loop of minimize(dim, fixed)", N_SINGLE, timed(lambda: [sl.minimize(dim, fx) for fx in singles]))

    dims = c["box_dims"]
    kept = [k for k in range(d) if k not in dims]
    u = np.sort(rng.uniform(0.0, 1.0, (N_ROWS, len(dims), 2)), axis=2)
    bounds = dom[dims, 0][None, :, None] + (dom[dims, 1] - dom[dims, 0])[None, :, None] * u
    kept_pts = np.ascontiguousarray(pts[:, kept])
    line(f"slider integrate_batch dims={dims}", N_ROWS, timed(lambda: sl.integrate_batch(dims, bounds, kept_pts)))
    # the floor: the slide with the most integrated dimensions, on its own columns
    best = max(range(len(sl.partition)), key=lambda i: (sum(k in dims for k in sl.partition[i]), len(sl.partition[i])))
    grp = list(sl.partition[best])
    local = [i for i, k in enumerate(grp) if k in dims]
    b_loc = np.ascontiguousarray(bounds[:, [dims.index(grp[i]) for i in local], :])
    p_loc = np.ascontiguousarray(pts[:, [k for k in grp if k not in dims]])
    box_slide = sl.slides[best]
    line(f"floor: slide {best} {grp} alone, integrate_batch dims={local}", N_ROWS,
         timed(lambda: box_slide.integrate_batch(local, b_loc, p_loc if p_loc.shape[1] else None)))
    line("loop of one-row integrate_batch", N_SINGLE,
         timed(lambda: [sl.integrate_batch(dims, bounds[r:r + 1], kept_pts[r:r + 1]) for r in range(N_SINGLE)]))
    # what was timed is what the loop computes
    R, cnt = sl.roots_batch(dim, fixed[:N_SINGLE])
    agree = sum(np.array_equal(sl.roots(dim, fx), R[i, :cnt[i]]) for i, fx in enumerate(singles))
    print(f"  {agree} of {N_SINGLE} single roots() calls equal their batch rows bit for bit", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(SHAPES))
    args = ap.parse_args()
    if args.step:
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
