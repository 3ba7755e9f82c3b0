#!/usr/bin/env python3
"""A/B of the tail split of large k_bary_mfma launches in ONE process on one GPU.

Two handles of the headline model: one created under PCX_BARY_TAIL=0 (one workgroup per point block, the parent's
geometry), one with the default (a last round at most half full is split over the idle workgroup slots,
bary_mfma_launch.h).  Per batch size: after WARM launches per arm and ~30 ms of launches in front of the first pair,
PAIRS interleaved pairs of REPS launches each are timed with events on the handle's stream.  Printed per batch size: the
geometry of both arms (pcx_bary_tail_info), per-arm median / min / max of the per-launch time over the pairs, the ratio
of medians, and whether the two arms' results are bit-identical.

    python tools/tail_ab.py [--pairs 12] [--reps 20] [--points 1000000,82523,983040] [--extra 7x7x7x7x7,9x9x9x9]

983,040 points are exactly 15 rounds of 512 workgroups: no tail, the arms launch the same grid.
--extra adds random tensors of the given shapes on [-1, 1]^d, each at the first batch size (short row-tile walks, where
the second kernel of a split launch weighs most: the default rule does not split them, --force does).
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import functions as F                                                  # noqa: E402
from pychebyshev_amd import ChebyshevApproximation, _lib               # noqa: E402

WARM = 5


def make(T, dom, tail):
    os.environ["PCX_BARY_TAIL"] = str(tail)
    os.environ["PCX_BARY_GRID"] = "0"          # the row-code form, also where a short plan would take the grid form
    c = ChebyshevApproximation.from_values(T, T.ndim, dom, list(T.shape))
    c.to_device()
    m = c._model()
    _lib.check(m.lib.pcx_bary_set_kernel(m.handle, 2), m.lib)
    return c, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", default="1000000,82523,983040", help="comma-separated batch sizes")
    ap.add_argument("--extra", default="", help="comma-separated shapes, e.g. 7x7x7x7x7")
    ap.add_argument("--force", action="store_true", help="PCX_BARY_TAIL=2 for the split arm: also where the default rule declines")
    a = ap.parse_args()
    lib = _lib.load()
    dev = int(os.environ.get("PCX_DEVICE", "0"))

    def chk(rc):
        _lib.check(rc, lib)

    rng = np.random.default_rng(5)
    sizes = [int(v) for v in a.points.split(",")]
    cases = [("bs5d 11^5 (headline)", np.load(os.path.join(ROOT, "tests", "golden", "g2_bs5d.npz"))["tensor"], F.BS5_DOMAIN, n)
             for n in sizes]
    for sh in filter(None, a.extra.split(",")):
        shape = tuple(int(v) for v in sh.split("x"))
        cases.append((sh, rng.standard_normal(shape), [[-1.0, 1.0]] * len(shape), sizes[0]))
    for name, T, dom, n in cases:
        d = T.ndim
        pts = np.ascontiguousarray(np.column_stack([rng.uniform(lo, hi, n) for lo, hi in dom]))
        arms = [make(T, dom, 0), make(T, dom, 2 if a.force else 1)]            # 0: one workgroup per block (the parent's geometry), 1: tail split
        spec = _lib.i32([0] * d)
        d_pts = [ctypes.c_void_p(), ctypes.c_void_p()]
        d_out = [ctypes.c_void_p(), ctypes.c_void_p()]
        streams, events = [], []
        try:
            for i, (c, m) in enumerate(arms):
                chk(lib.pcx_dev_malloc(dev, pts.nbytes, ctypes.byref(d_pts[i])))
                chk(lib.pcx_dev_malloc(dev, n * 8, ctypes.byref(d_out[i])))
                chk(lib.pcx_memcpy_h2d(dev, d_pts[i], pts.ctypes.data_as(ctypes.c_void_p), pts.nbytes))
                st = ctypes.c_void_p()
                chk(lib.pcx_bary_stream(m.handle, ctypes.byref(st)))
                streams.append(st)
                e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
                chk(lib.pcx_event_create(dev, ctypes.byref(e0)))
                chk(lib.pcx_event_create(dev, ctypes.byref(e1)))
                events.append((e0, e1))

            def run(i, reps, timed):
                m = arms[i][1]
                if timed:
                    chk(lib.pcx_event_record(events[i][0], streams[i]))
                for _ in range(reps):
                    chk(lib.pcx_bary_eval_batch_dev(m.handle, d_pts[i], n, _lib.p_i32(spec), d_out[i], streams[i]))
                if timed:
                    chk(lib.pcx_event_record(events[i][1], streams[i]))
                chk(lib.pcx_device_synchronize(dev))
                if not timed:
                    return 0.0
                ms = ctypes.c_float()
                chk(lib.pcx_event_elapsed_ms(events[i][0], events[i][1], ctypes.byref(ms)))
                return ms.value / reps

            for i in (0, 1):
                run(i, WARM, False)
            for i in (0, 1):                                        # ~30 ms and more of launches in front of the first pair
                run(i, a.reps, False)
            times = [[], []]
            for _ in range(a.pairs):
                for i in (0, 1):
                    times[i].append(run(i, a.reps, True))
            outs, info = [], []
            for i in (0, 1):
                k = _lib.i32(np.zeros(6))
                chk(lib.pcx_bary_tail_info(arms[i][1].handle, _lib.p_i32(k)))
                info.append([int(v) for v in k])
                y = np.empty(n)
                chk(lib.pcx_memcpy_d2h(dev, y.ctypes.data_as(ctypes.c_void_p), d_out[i], y.nbytes))
                outs.append(y)
        finally:
            for i in (0, 1):
                if d_pts[i]:
                    lib.pcx_dev_free(dev, d_pts[i])
                if d_out[i]:
                    lib.pcx_dev_free(dev, d_out[i])
            for e0, e1 in events:
                lib.pcx_event_destroy(e0)
                lib.pcx_event_destroy(e1)
        med = [statistics.median(t) for t in times]
        print(f"{name}: N = {n:,}, {a.pairs} interleaved pairs x {a.reps} launches")
        for i, label in ((0, "PCX_BARY_TAIL=0"), (1, "tail split     ")):
            print(f"  {label}  slots={info[i][0]} chunks={info[i][2]} tail blocks={info[i][5]} x P={info[i][4]}  ms/launch median {med[i]:.4f}  "
                  f"min {min(times[i]):.4f}  max {max(times[i]):.4f}  spread {max(times[i]) - min(times[i]):.4f}")
        gain = med[0] - med[1]
        spread = max(max(t) - min(t) for t in times)
        print(f"  ratio of medians split / unsplit = {med[1] / med[0]:.4f}  (gain {gain:.4f} ms, larger spread {spread:.4f} ms: "
              f"{'above' if gain > spread else 'NOT above'} the spread);  results bit-identical: {np.array_equal(outs[0], outs[1])}")
        sys.stdout.flush()
        del arms


if __name__ == "__main__":
    main()
