#!/usr/bin/env python3
"""A/B of the seeded and the unseeded row-code MFMA plan in ONE process on one GPU.

Two handles per model: one created under PCX_BARY_SEED=0 (every column of the folded tail in the k-loop, the remainder
padded to a whole k-step), one with the default (K mod 4 = 1 or 2 columns seed the accumulators).  After WARM launches
per arm and ~30 ms of launches in front of the first pair (the FP64 clock transient at the start of a stream),
PAIRS interleaved pairs of REPS launches each are timed with events on the handle's stream.  Printed per model: k-steps of
both plans, per-arm median / min / max of the per-launch time over the pairs, the ratio of medians, and whether the two
arms' results are bit-identical.

    python tools/seed_ab.py [--pairs 12] [--reps 20] [--points 1000000] [--extra 11x11x10x11,12x12x7x23]

--extra adds random tensors of the given shapes on [-1, 1]^d (e.g. plans whose seeded instantiation uses scratch).
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


def make(T, dom, seed_on):
    os.environ["PCX_BARY_SEED"] = "1" if seed_on else "0"
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
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--extra", default="", help="comma-separated shapes, e.g. 11x11x10x11")
    a = ap.parse_args()
    lib = _lib.load()
    dev = int(os.environ.get("PCX_DEVICE", "0"))

    def chk(rc):
        _lib.check(rc, lib)

    rng = np.random.default_rng(5)
    models = [("bs5d 11^5 (headline)", np.load(os.path.join(ROOT, "tests", "golden", "g2_bs5d.npz"))["tensor"], F.BS5_DOMAIN),
              ("7^5", rng.standard_normal((7,) * 5), [[-1.0, 1.0]] * 5),
              ("9^4", rng.standard_normal((9,) * 4), [[-1.0, 1.0]] * 4)]
    for sh in filter(None, a.extra.split(",")):
        shape = tuple(int(v) for v in sh.split("x"))
        models.append((sh, rng.standard_normal(shape), [[-1.0, 1.0]] * len(shape)))
    for name, T, dom in models:
        d = T.ndim
        n = a.points
        pts = np.ascontiguousarray(np.column_stack([rng.uniform(lo, hi, n) for lo, hi in dom]))
        arms = [make(T, dom, False), make(T, dom, True)]            # 0: unseeded (the parent's form), 1: seeded
        info = []
        for c, m in arms:
            k = _lib.i32(np.zeros(6))
            chk(lib.pcx_bary_kernel_info(m.handle, _lib.p_i32(k)))
            info.append((int(k[1]), int(k[2]), int(k[5])))
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
            outs = []
            for i in (0, 1):
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
        for i, label in ((0, "PCX_BARY_SEED=0"), (1, "seeded        ")):
            print(f"  {label}  MT={info[i][0]} k-steps={info[i][1]} split={info[i][2]}  ms/launch median {med[i]:.4f}  "
                  f"min {min(times[i]):.4f}  max {max(times[i]):.4f}  spread {max(times[i]) - min(times[i]):.4f}")
        gain = med[0] - med[1]
        spread = max(max(t) - min(t) for t in times)
        print(f"  ratio of medians seeded / unseeded = {med[1] / med[0]:.4f}  (gain {gain:.4f} ms, larger spread {spread:.4f} ms: "
              f"{'above' if gain > spread else 'NOT above'} the spread);  results bit-identical: {np.array_equal(outs[0], outs[1])}")
        sys.stdout.flush()
        del arms


if __name__ == "__main__":
    main()
