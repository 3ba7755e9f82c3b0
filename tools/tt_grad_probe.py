#!/usr/bin/env python3
"""Time of ``ChebyshevTT.gradient_batch`` (``pcx_tt_grad_batch_dev``, csrc/tt_grad_kernels.h: one forward-backward pass
per row) next to the route it replaces, on the same model, same N, same process: the analytic
``pcx_tt_deriv_batch_dev`` with the same d + 1 (value, gradient) or 2 d + 1 (and the Hessian's diagonal) single-dimension
specs -- one chain per (row, spec) -- and one evaluation chain (``pcx_tt_eval_batch_dev``).

Models: the 5-D shape of BASELINE config 3 (ranks [1,8,8,8,6,1], n = 11: 19 KiB of LDS per wave, 8 waves a CU) and the
shape of config 5 (10-D, rank 16, n = 11: 80 KiB, 2 waves a CU), by the method of tools/tt_deriv_probe.py: device-resident
rows, events around each launch, 5 warm-up rounds, the median of ``--steps`` launches, the three launches alternating.
The last column is the normwise distance between the two routes' results on the first 10^6 rows, worst column.

    python tools/tt_grad_probe.py [--steps 20] [--sizes 1000000 10000000] [--out profiles/tt_grad_probe.txt]
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pychebyshev_amd import _lib  # noqa: E402
from tt_deriv_probe import COMPARE_ROWS, SHAPES, DeviceTimer, download, make_model, upload  # noqa: E402


def gradient_specs(d, second):
    """The zero spec, then order 1 and (second) order 2 in every dimension in turn: gradient_batch's columns."""
    specs = np.zeros((1 + (2 if second else 1) * d, d), dtype=np.int32)
    for o in (1, 2)[:2 if second else 1]:
        for u in range(d):
            specs[1 + (o - 1) * d + u, u] = o
    return specs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tt_grad_probe.txt"))
    args = ap.parse_args()
    dev = _lib.default_device()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"{'model':<40} {'N':>9} {'second':>6} {'C':>3} {'gradient ms':>11} {'per-spec ms':>11} {'eval ms':>9} {'gradient/eval':>13} "
        f"{'per-spec/gradient':>17}  gradient - per-spec, normwise, worst column")
    for name, (ranks, n) in SHAPES.items():
        tt = make_model(ranks, n, 31)
        d = tt.num_dimensions
        t = tt._dev()
        lib = t.lib
        st = ctypes.c_void_p()
        _lib.check(lib.pcx_tt_stream(t.handle, ctypes.byref(st)), lib)
        timer = DeviceTimer(lib, dev)
        for N in args.sizes:
            pts = np.random.default_rng(5).uniform(-1.0, 1.0, (N, d))
            d_pts = upload(lib, dev, pts)
            del pts
            d_val = upload(lib, dev, np.zeros(N))
            for second in (0, 1):
                specs = gradient_specs(d, second)
                m = specs.shape[0]
                d_gr, d_an = upload(lib, dev, np.zeros((N, m))), upload(lib, dev, np.zeros((N, m)))
                gr, an, ev = timer.medians_ms(
                    [lambda: _lib.check(lib.pcx_tt_grad_batch_dev(t.handle, d_pts, N, second, d_gr, st), lib),
                     lambda: _lib.check(lib.pcx_tt_deriv_batch_dev(t.handle, d_pts, N, _lib.p_i32(specs), m, d_an, st), lib),
                     lambda: _lib.check(lib.pcx_tt_eval_batch_dev(t.handle, d_pts, N, d_val, st), lib)],
                    st, args.warmup, args.steps)
                _lib.check(lib.pcx_stream_synchronize(st), lib)
                rows = min(N, COMPARE_ROWS)
                yg, ya = download(lib, dev, d_gr, (rows, m)), download(lib, dev, d_an, (rows, m))
                dist = float(np.max(np.max(np.abs(yg - ya), axis=0) / np.max(np.abs(ya), axis=0)))
                say(f"{name:<40} {N:>9} {second:>6} {m:>3} {gr:>11.3f} {an:>11.3f} {ev:>9.3f} {gr / ev:>13.2f} {an / gr:>17.2f}  {dist:.2e}")
                for p in (d_gr, d_an):
                    lib.pcx_dev_free(dev, p)
            for p in (d_pts, d_val):
                lib.pcx_dev_free(dev, p)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
