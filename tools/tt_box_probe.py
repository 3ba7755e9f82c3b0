#!/usr/bin/env python3
"""Rows per second of the batched TT box integral (``pcx_tt_box_batch_dev``, csrc/tt_box_kernels.h) next to
``pcx_tt_eval_batch_dev`` on the same model, same N, same process -- the evaluation kernel is the yardstick: a box row
is the same chain with ~6 n more vector instructions per integrated dimension and 8 more bytes per integrated dimension.

Models: the 5-D shape of BASELINE config 3 (ranks [1,8,8,8,6,1], n = 11) with 1, 2 and 5 integrated dimensions, the
shape of config 5 (10-D, rank 16, n = 11) with 2, and two 4-D models whose node counts differ per dimension (rank caps
12 and 16: the kernel instantiations that dispatch on the node count as well) and a 3-D model with rank 20 and 20
nodes, which runs the wave-per-row kernel on the plain cores.  Device-resident rows, timed with events
around each launch after a warm-up; box and evaluation launches alternate, and each figure is the median of ``--steps``
launches.  Beside it the host-pointer rate of ``integrate_batch`` (host clock around the
synchronous call) and the "before": ``integrate(dims, bounds).eval(point)`` in a Python loop over 10^3 rows.

    python tools/tt_box_probe.py [--steps 20] [--sizes 1000000 10000000]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pychebyshev_amd import ChebyshevTT, _lib  # noqa: E402

SHAPES = {
    "config 3 (5-D, ranks 1,8,8,8,6,1, n 11)": ([1, 8, 8, 8, 6, 1], 11, [[0], [1, 3], [0, 1, 2, 3, 4]]),
    "config 5 (10-D, rank 16, n 11)": ([1] + [16] * 9 + [1], 11, [[2, 7]]),
    "mixed n 7,16,5,9 (4-D, ranks 1,12,9,10,1)": ([1, 12, 9, 10, 1], [7, 16, 5, 9], [[1, 3]]),
    "mixed n 16,3,12,7 (4-D, ranks 1,16,16,9,1)": ([1, 16, 16, 9, 1], [16, 3, 12, 7], [[0, 2]]),
    "wave per row 5,20,4 (3-D, ranks 1,20,17,1)": ([1, 20, 17, 1], [5, 20, 4], [[1]]),
}


def make_model(ranks, n, seed):
    rng = np.random.default_rng(seed)
    d = len(ranks) - 1
    nodes = [n] * d if isinstance(n, int) else list(n)
    cores = [rng.standard_normal((ranks[k], nodes[k], ranks[k + 1])) * (0.6 ** np.arange(nodes[k]))[None, :, None]
             / np.sqrt(ranks[k]) for k in range(d)]
    return ChebyshevTT.from_coeff_cores(cores, [[-1.0, 1.0]] * d)


def make_rows(d, dims, N, seed):
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.05, 1.0, (N, len(dims))) * 2.0
    lo = -1.0 + rng.uniform(0.0, 1.0, (N, len(dims))) * (2.0 - w)
    bounds = np.stack([lo, np.minimum(lo + w, 1.0)], axis=2)
    points = rng.uniform(-1.0, 1.0, (N, d - len(dims)))
    return bounds, points


class DeviceTimer:
    def __init__(self, lib, dev):
        self.lib, self.dev = lib, dev
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(lib.pcx_event_create(dev, ctypes.byref(self.a)), lib)
        _lib.check(lib.pcx_event_create(dev, ctypes.byref(self.b)), lib)

    def once_ms(self, launch, stream):
        _lib.check(self.lib.pcx_event_record(self.a, stream), self.lib)
        launch()
        _lib.check(self.lib.pcx_event_record(self.b, stream), self.lib)
        ms = ctypes.c_float()
        _lib.check(self.lib.pcx_event_elapsed_ms(self.a, self.b, ctypes.byref(ms)), self.lib)
        return float(ms.value)

    def median_pair_ms(self, first, second, stream, warm, steps):
        """Medians of two launches timed in turn (first, second, first, ...), so that both see the same clock."""
        for _ in range(warm):
            first()
            second()
        _lib.check(self.lib.pcx_stream_synchronize(stream), self.lib)
        times = [(self.once_ms(first, stream), self.once_ms(second, stream)) for _ in range(steps)]
        return float(np.median([t[0] for t in times])), float(np.median([t[1] for t in times]))


def upload(lib, dev, arr):
    arr = np.ascontiguousarray(arr, dtype=np.float64)
    p = ctypes.c_void_p()
    _lib.check(lib.pcx_dev_malloc(dev, max(arr.nbytes, 8), ctypes.byref(p)), lib)
    _lib.check(lib.pcx_memcpy_h2d(dev, p, arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes), lib)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 10_000_000])
    args = ap.parse_args()
    dev = _lib.default_device()
    print(f"{'model':<42} {'m':>2} {'N':>9} {'box ms':>9} {'box rows/s':>11} {'eval ms':>9} {'eval pts/s':>11} "
          f"{'box/eval':>8} {'host rows/s':>11}", flush=True)
    for name, (ranks, n, dim_sets) in SHAPES.items():
        tt = make_model(ranks, n, 31)
        d = tt.num_dimensions
        t = tt._dev()
        lib = t.lib
        st = ctypes.c_void_p()
        _lib.check(lib.pcx_tt_stream(t.handle, ctypes.byref(st)), lib)
        timer = DeviceTimer(lib, dev)
        for N in args.sizes:
            pts = np.random.default_rng(5).uniform(-1.0, 1.0, (N, d))
            d_pts, d_out, d_val = upload(lib, dev, pts), upload(lib, dev, np.zeros(N)), upload(lib, dev, np.zeros(N))
            for dims in dim_sets:
                bounds, points = make_rows(d, dims, N, 7 + len(dims))
                flags, rows = tt._box_rows(dims, bounds, points if points.shape[1] else None)
                d_rows = upload(lib, dev, rows)
                box, ev = timer.median_pair_ms(
                    lambda: _lib.check(lib.pcx_tt_box_batch_dev(t.handle, _lib.p_i32(flags), d_rows, N, d_out, st), lib),
                    lambda: _lib.check(lib.pcx_tt_eval_batch_dev(t.handle, d_pts, N, d_val, st), lib),
                    st, args.warmup, args.steps)
                lib.pcx_dev_free(dev, d_rows)
                tt.integrate_batch(dims, bounds[:1000], points[:1000] if points.shape[1] else None)      # warm-up
                t0 = time.perf_counter()
                tt.integrate_batch(dims, bounds, points if points.shape[1] else None)
                host = time.perf_counter() - t0
                print(f"{name:<42} {len(dims):>2} {N:>9} {box:>9.3f} {N / box * 1e3:>11.3e} {ev:>9.3f} {N / ev * 1e3:>11.3e} "
                      f"{box / ev:>8.3f} {N / host:>11.3e}", flush=True)
            for p in (d_pts, d_out, d_val):
                lib.pcx_dev_free(dev, p)
        # the "before": one reduced model per row
        dims = dim_sets[min(1, len(dim_sets) - 1)]
        bounds, points = make_rows(d, dims, 1000, 3)
        t0 = time.perf_counter()
        loop = np.array([tt.integrate(dims, [tuple(b) for b in bounds[r]]).eval(points[r]) for r in range(1000)])
        per_row = (time.perf_counter() - t0) / 1000
        batch = tt.integrate_batch(dims, bounds, points)
        err = float(np.max(np.abs(batch - loop)) / np.max(np.abs(loop)))
        print(f"    per-row integrate(...).eval(...) loop, m = {len(dims)}: {per_row * 1e3:.3f} ms per row = {1 / per_row:.3e} rows/s; "
              f"integrate_batch against it on those 1,000 rows: normwise {err:.2e}", flush=True)


if __name__ == "__main__":
    main()
