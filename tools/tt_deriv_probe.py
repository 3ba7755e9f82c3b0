#!/usr/bin/env python3
"""Time of the analytic TT Greeks (``pcx_tt_deriv_batch_dev``, csrc/tt_deriv_kernels.h) next to two yardsticks on the
same model, same N, same process: today's finite-difference Greeks (``pcx_tt_eval_multi_batch_dev``) for the same four
outputs -- value, delta, gamma, vega -- and one evaluation chain (``pcx_tt_eval_batch_dev``).  An analytic (row, spec) is
one chain with a few more vector instructions per differentiated dimension; the finite differences walk 1 + 2 + 3 + 2 = 8
chains for these four specs.

Models: the 5-D shape of BASELINE config 3 (ranks [1,8,8,8,6,1], n = 11) and the shape of config 5 (10-D, rank 16,
n = 11), whose ``eval_batch`` runs the MFMA form while the analytic kernel runs one row per lane.  Device-resident rows,
timed with events around each launch after a warm-up; the three launches alternate, and each figure is the median of
``--steps`` launches.  The last column is the normwise distance of the finite differences from the analytic values per
spec on the first 10^6 rows.

    python tools/tt_deriv_probe.py [--steps 20] [--sizes 1000000 10000000]
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pychebyshev_amd import ChebyshevTT, _lib  # noqa: E402

SHAPES = {
    "config 3 (5-D, ranks 1,8,8,8,6,1, n 11)": ([1, 8, 8, 8, 6, 1], 11),
    "config 5 (10-D, rank 16, n 11)": ([1] + [16] * 9 + [1], 11),
}
COMPARE_ROWS = 1_000_000


def make_model(ranks, n, seed):
    rng = np.random.default_rng(seed)
    d = len(ranks) - 1
    cores = [rng.standard_normal((ranks[k], n, ranks[k + 1])) * (0.6 ** np.arange(n))[None, :, None] / np.sqrt(ranks[k])
             for k in range(d)]
    return ChebyshevTT.from_coeff_cores(cores, [[-1.0, 1.0]] * d)


def greek_specs(d):
    """value, delta and gamma in dimension 0, vega in dimension 3"""
    specs = np.zeros((4, d), dtype=np.int32)
    specs[1, 0] = 1
    specs[2, 0] = 2
    specs[3, 3] = 1
    return specs


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

    def medians_ms(self, launches, stream, warm, steps):
        """Medians of several launches timed in turn (first, second, third, first, ...), so that all see the same clock."""
        for _ in range(warm):
            for launch in launches:
                launch()
        _lib.check(self.lib.pcx_stream_synchronize(stream), self.lib)
        times = [[self.once_ms(launch, stream) for launch in launches] for _ in range(steps)]
        return [float(np.median([t[i] for t in times])) for i in range(len(launches))]


def upload(lib, dev, arr):
    arr = np.ascontiguousarray(arr, dtype=np.float64)
    p = ctypes.c_void_p()
    _lib.check(lib.pcx_dev_malloc(dev, max(arr.nbytes, 8), ctypes.byref(p)), lib)
    _lib.check(lib.pcx_memcpy_h2d(dev, p, arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes), lib)
    return p


def download(lib, dev, ptr, shape):
    out = np.empty(shape)
    _lib.check(lib.pcx_memcpy_d2h(dev, out.ctypes.data_as(ctypes.c_void_p), ptr, out.nbytes), lib)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 10_000_000])
    args = ap.parse_args()
    dev = _lib.default_device()
    print(f"{'model':<40} {'N':>9} {'analytic ms':>11} {'fd ms':>9} {'eval ms':>9} {'(row,spec)/eval':>15} {'fd/analytic':>11}  "
          f"fd - analytic, normwise per spec (value, delta, gamma, vega)", flush=True)
    for name, (ranks, n) in SHAPES.items():
        tt = make_model(ranks, n, 31)
        d = tt.num_dimensions
        specs = greek_specs(d)
        m = specs.shape[0]
        t = tt._dev()
        lib = t.lib
        st = ctypes.c_void_p()
        _lib.check(lib.pcx_tt_stream(t.handle, ctypes.byref(st)), lib)
        timer = DeviceTimer(lib, dev)
        for N in args.sizes:
            pts = np.random.default_rng(5).uniform(-1.0, 1.0, (N, d))
            d_pts = upload(lib, dev, pts)
            del pts
            d_an, d_fd = upload(lib, dev, np.zeros((N, m))), upload(lib, dev, np.zeros((N, m)))
            d_val = upload(lib, dev, np.zeros(N))
            an, fd, ev = timer.medians_ms(
                [lambda: _lib.check(lib.pcx_tt_deriv_batch_dev(t.handle, d_pts, N, _lib.p_i32(specs), m, d_an, st), lib),
                 lambda: _lib.check(lib.pcx_tt_eval_multi_batch_dev(t.handle, d_pts, N, _lib.p_i32(specs), m, d_fd, st), lib),
                 lambda: _lib.check(lib.pcx_tt_eval_batch_dev(t.handle, d_pts, N, d_val, st), lib)],
                st, args.warmup, args.steps)
            _lib.check(lib.pcx_stream_synchronize(st), lib)
            rows = min(N, COMPARE_ROWS)
            ya, yf = download(lib, dev, d_an, (rows, m)), download(lib, dev, d_fd, (rows, m))
            dist = np.max(np.abs(yf - ya), axis=0) / np.max(np.abs(ya), axis=0)
            print(f"{name:<40} {N:>9} {an:>11.3f} {fd:>9.3f} {ev:>9.3f} {an / m / ev:>15.3f} {fd / an:>11.2f}  "
                  + " ".join(f"{v:.2e}" for v in dist), flush=True)
            for p in (d_pts, d_an, d_fd, d_val):
                lib.pcx_dev_free(dev, p)


if __name__ == "__main__":
    main()
