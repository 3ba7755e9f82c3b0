#!/usr/bin/env python3
"""Time of ``ChebyshevTT.hessian_batch`` (``pcx_tt_hess_batch_dev``, csrc/tt_hess_kernels.h: one right sweep and a left
sweep in passes of B carried vectors) at EVERY admissible block size B, next to code it does not touch, on the same
model, same N, same process: the analytic ``pcx_tt_deriv_batch_dev`` with the 1 + d + d (d + 1) / 2 specs of the value,
the gradient, the diagonal and the upper triangle -- one chain per (row, spec) --, ``pcx_tt_grad_batch_dev(second = 1)``
and one evaluation chain (``pcx_tt_eval_batch_dev``).

Models: the shapes of BASELINE config 3 and config 5 (tools/tt_deriv_probe.py), by its method: device-resident rows,
events around each launch, 5 warm-up rounds, the median of ``--steps`` launches, all launches alternating.  "LDS" is the
dynamic LDS of a workgroup (one wave) at that B from ``pcx_tt_hess_info``'s rule, "waves/CU" what 160 KiB hold of it in
granules of 1280 bytes (the planner's count, not a measured one).
The last column is the normwise distance between the Hessian's and the per-spec route's results on the first 10^6 rows,
worst column.

    python tools/tt_hess_probe.py [--steps 20] [--sizes 1000000 10000000] [--out profiles/tt_hess_probe.txt]
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

CU_LDS = 160 * 1024
LDS_GRANULE = 1280            # tt_hess_resident_waves (csrc/tt_hess_kernels.h)


def hessian_specs(d):
    """(specs, the Hessian result's column of each): value, gradient, diagonal, then the upper triangle."""
    specs, cols = [[0] * d], [0]
    for u in range(d):
        specs.append([int(v == u) for v in range(d)])
        cols.append(1 + u)
    for u in range(d):
        specs.append([2 * int(v == u) for v in range(d)])
        cols.append(1 + d + u * d + u)
    for u in range(d):
        for w in range(u + 1, d):
            specs.append([int(v in (u, w)) for v in range(d)])
            cols.append(1 + d + u * d + w)
    return np.array(specs, dtype=np.int32), cols


def dev_alloc(lib, dev, doubles):
    p = ctypes.c_void_p()
    _lib.check(lib.pcx_dev_malloc(dev, max(8 * doubles, 8), ctypes.byref(p)), lib)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tt_hess_probe.txt"))
    args = ap.parse_args()
    dev = _lib.default_device()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"{'model':<40} {'N':>9} {'B':>2} {'passes':>6} {'LDS KiB':>8} {'waves/CU':>8} {'hessian ms':>10} {'per-spec ms':>11} "
        f"{'gradient ms':>11} {'eval ms':>9} {'hessian/eval':>12} {'per-spec/hessian':>16}  hessian - per-spec, normwise, worst column")
    for name, (ranks, n) in SHAPES.items():
        tt = make_model(ranks, n, 31)
        d = tt.num_dimensions
        t = tt._dev()
        lib = t.lib
        st = ctypes.c_void_p()
        _lib.check(lib.pcx_tt_stream(t.handle, ctypes.byref(st)), lib)
        info = np.zeros(4, dtype=np.int32)
        _lib.check(lib.pcx_tt_hess_info(t.handle, _lib.p_i32(info)), lib)
        form, plan, plan_lds, fits = (int(v) for v in info)
        assert form == 1, "both shapes have a lane-per-point image"
        # the rule of csrc/tt_hess_kernels.h (tt_hess_lpp_columns), held to the library's own figure at the planner's B
        lds = {B: (sum(ranks[1:-1]) + max(ranks) + B * (2 * max(ranks) + 1)) * 64 * 8 for B in range(1, fits + 1)}
        assert lds[plan] == plan_lds, (lds, plan, plan_lds)
        say(f"# {name}: planner's B = {plan}, largest B that fits = {fits}, gradient_batch LDS {(sum(ranks[1:-1]) + max(ranks)) * 512 / 1024:.1f} KiB")
        specs, cols = hessian_specs(d)
        m, C = specs.shape[0], 1 + d + d * d
        timer = DeviceTimer(lib, dev)
        for N in args.sizes:
            pts = np.random.default_rng(5).uniform(-1.0, 1.0, (N, d))
            d_pts = upload(lib, dev, pts)
            del pts
            d_val, d_gr, d_an = dev_alloc(lib, dev, N), dev_alloc(lib, dev, N * (1 + 2 * d)), dev_alloc(lib, dev, N * m)
            d_he = {B: dev_alloc(lib, dev, N * C) for B in range(1, fits + 1)}
            launches = [(lambda B=B: _lib.check(lib.pcx_tt_hess_batch_dev(t.handle, d_pts, N, B, d_he[B], st), lib)) for B in d_he]
            launches += [lambda: _lib.check(lib.pcx_tt_deriv_batch_dev(t.handle, d_pts, N, _lib.p_i32(specs), m, d_an, st), lib),
                         lambda: _lib.check(lib.pcx_tt_grad_batch_dev(t.handle, d_pts, N, 1, d_gr, st), lib),
                         lambda: _lib.check(lib.pcx_tt_eval_batch_dev(t.handle, d_pts, N, d_val, st), lib)]
            med = timer.medians_ms(launches, st, args.warmup, args.steps)
            _lib.check(lib.pcx_stream_synchronize(st), lib)
            an, gr, ev = med[-3:]
            rows = min(N, COMPARE_ROWS)
            ya = download(lib, dev, d_an, (rows, m))
            for i, B in enumerate(d_he):
                yh = download(lib, dev, d_he[B], (rows, C))
                assert np.array_equal(yh[:, 1 + d:].reshape(rows, d, d), yh[:, 1 + d:].reshape(rows, d, d).transpose(0, 2, 1))
                dist = float(np.max(np.max(np.abs(yh[:, cols] - ya), axis=0) / np.max(np.abs(ya), axis=0)))
                he = med[i]
                say(f"{name:<40} {N:>9} {B:>2} {max(1, -(-(d - 1) // B)):>6} {lds[B] / 1024:>8.1f} {CU_LDS // (-(-lds[B] // LDS_GRANULE) * LDS_GRANULE):>8} {he:>10.3f} {an:>11.3f} "
                    f"{gr:>11.3f} {ev:>9.3f} {he / ev:>12.2f} {an / he:>16.2f}  {dist:.2e}")
            for p in [d_pts, d_val, d_gr, d_an] + list(d_he.values()):
                lib.pcx_dev_free(dev, p)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
