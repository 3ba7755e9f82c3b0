#!/usr/bin/env python3
"""Rates of ChebyshevSpline / ChebyshevSlider ladder_batch against the class's own eval_batch on the expanded points, on
the device (writes profiles/piecewise_ladder_probe.txt).

    python tools/piecewise_ladder_probe.py [--rows 100000] [--out profiles/piecewise_ladder_probe.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/piecewise_ladder_probe.py --trace   (the kernel split, a run of its own)

Method (tools/ladder_probe.py's): rows and result device-resident; one warm-up call, then the median of 5 calls, host clock
around a call that is complete on return.  The baseline is existing code, eval_batch on the device-resident expanded
N m points, timed the same way.  m = the fibre (the nodes along dim: for a spline those of all pieces along dim), 21, 101.

Per case: rows/s, the ratio to the baseline's rows/s (= its points/s over m), and the kernel launches of one call, counted
from the call's structure: spline 4 (route, scatter, gather, interpolate) + non-empty cross-sections x live indices per
chunk; slider 2 per slide that does not own dim (gather, evaluate) + the owner's ladder (+ its gather) + the sum per chunk.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pychebyshev_amd import ChebyshevSlider, ChebyshevSpline  # noqa: E402
from pychebyshev_amd.device import DeviceArray  # noqa: E402


def median_time(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def expand(d, dim, fixed, xs):
    rows, m = fixed.shape[0], xs.size
    pts = np.empty((rows, m, d))
    others = [k for k in range(d) if k != dim]
    for c, k in enumerate(others):
        pts[:, :, k] = fixed[:, c][:, None]
    pts[:, :, dim] = xs[None, :]
    return pts.reshape(rows * m, d)


def route(knots, n_pieces, values):
    k = np.asarray(knots, dtype=float)
    return np.minimum(np.searchsorted(k, values, side="right"), n_pieces - 1) if k.size else np.zeros(len(values), dtype=int)


def spline_launches(sp, dim, fixed, xs):
    d = sp.num_dimensions
    live = np.unique(route(sp.knots[dim], sp._shape[dim], xs))
    counts = [int(sp._pieces[int(j) * int(np.prod(sp._shape[dim + 1:], dtype=int))].n_nodes[dim]) for j in live]
    chunk = max(1, min(fixed.shape[0], (1 << 21) // sum(counts)))
    total = 0
    for r0 in range(0, fixed.shape[0], chunk):
        sec = np.zeros(min(chunk, fixed.shape[0] - r0), dtype=int)
        for c, k in enumerate(q for q in range(d) if q != dim):
            sec = sec * sp._shape[k] + route(sp.knots[k], sp._shape[k], fixed[r0:r0 + chunk, c])
        total += 4 + np.unique(sec).size * live.size
    return total


def slider_launches(sl, dim, N, m, shared=True):
    o = sl._dim_to_slide[dim]
    g = len(sl.partition[o])
    chunks = -(-N // max(1, min(N, (1 << 21) // m)))
    one_row = g == 1 and shared
    per = 2 * (len(sl.partition) - 1) + (0 if one_row else 1) + (1 if g > 1 else 0) + 1
    return chunks * per + (1 if one_row else 0)


def case(log, name, obj, dim, N, trace, launches):
    d = obj.num_dimensions
    rng = np.random.default_rng(7)
    others = [k for k in range(d) if k != dim]
    fixed = np.column_stack([rng.uniform(obj.domain[k][0], obj.domain[k][1], N) for k in others]) if others else np.empty((N, 0))
    dev = obj._dev().device
    dfixed = DeviceArray.from_host(fixed, dev)
    if isinstance(obj, ChebyshevSpline):
        stride = int(np.prod(obj._shape[dim + 1:], dtype=int))
        nodes = np.concatenate([np.asarray(obj._pieces[j * stride].nodes[dim], dtype=float) for j in range(obj._shape[dim])])
    else:
        nodes = np.asarray(obj._owner_grid(dim)[0], dtype=float)
    for m in ("fibre", 21, 101):
        xs = nodes if m == "fibre" else np.linspace(obj.domain[dim][0], obj.domain[dim][1], m)
        out = DeviceArray.empty((N, xs.size), dev)
        t = median_time(lambda: obj.ladder_batch(dim, dfixed, xs, out=out), reps=1 if trace else 5)
        if trace:
            continue
        dpts = DeviceArray.from_host(expand(d, dim, fixed, xs), dev)
        tb = median_time(lambda: obj.eval_batch(dpts, [0] * d))
        base = N / tb
        log(f"{name:<22} dim {dim} m {xs.size:>3}{' (fibre)' if m == 'fibre' else '        '} {N / t:10.3e} rows/s  x{(N / t) / base:6.2f} of "
            f"pointwise ({base:9.3e} rows/s = {base * xs.size:9.3e} pts/s)  {launches(fixed, xs):>4} launches per call")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "piecewise_ladder_probe.txt"))
    ap.add_argument("--trace", action="store_true", help="one warm-up and one timed call per case, no baseline: for rocprofv3 --kernel-trace")
    args = ap.parse_args()
    import math

    import generate_golden_slider_calculus as SL
    from spline_calculus_probe import SHAPES, make
    N = args.rows
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"piecewise_ladder_probe: N = {N} rows, device-resident, median of 5 after one warm-up, host clock around a call that is "
        f"complete on return")
    for tag, label in (("m", "spline 3-D 8 pieces"), ("k", "spline 2-D 6 pieces")):
        sp = make(tag)
        case(log, label, sp, SHAPES[tag]["dim"], N, args.trace, lambda f, x, sp=sp, dim=SHAPES[tag]["dim"]: spline_launches(sp, dim, f, x))
    knots = [[-0.5, 0.0, 0.5]] * 3
    s64 = ChebyshevSpline(lambda x, _=None: math.sin(3.0 * x[0]) * math.exp(0.5 * x[1]) + abs(x[2] - 0.1) + 0.2 * abs(x[0]), 3,
                          [[-1.0, 1.0]] * 3, n_nodes=[8, 8, 8], knots=knots)
    s64.build(verbose=False)
    case(log, "spline 3-D 64 pieces", s64, 0, N, args.trace, lambda f, x: spline_launches(s64, 0, f, x))
    sa = SL.build(ChebyshevSlider, "a")
    case(log, "slider [0][1][2]", sa, 0, N, args.trace, lambda f, x: slider_launches(sa, 0, f.shape[0], x.size))
    sb = SL.build(ChebyshevSlider, "b")
    for dim in (0, 2):
        case(log, "slider [0,1][2][3,4]", sb, dim, N, args.trace, lambda f, x, dim=dim: slider_launches(sb, dim, f.shape[0], x.size))
    if not args.trace:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
