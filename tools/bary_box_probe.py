#!/usr/bin/env python3
"""Rows per second of the batched box integral of the full-tensor interpolant (``pcx_bary_box_batch_dev``,
csrc/bary_box_kernels.h) next to ``pcx_bary_eval_batch_dev`` on the same handle, same N, same process.  The evaluation
kernel is the yardstick: a box row is the same contraction, with m n^2 more FMAs in the prologue (under 0.2 % of prod n
for 11^5) -- what the ratio shows is the runtime k-step loop with its B operands in LDS against the specialised
``k_bary_mfma``, or the rows form against whatever kernel the handle evaluates with.

Legs: the 11^5 bench model (tests/golden/g2_bs5d.npz) with m = 1, 2 and 5 integrated dimensions; the same with the rows
form forced (``pcx_bary_set_kernel(h, 1)``, a smaller batch); a 12 x 12 model and a 20^3 model (a grid / k-fold plan),
which run the rows form.  Device-resident rows, events around each launch after a warm-up; box and evaluation launches
alternate and each figure is the median of ``--steps`` launches.  Then the "before": ``integrate(dims,
bounds).vectorized_eval(point)`` in a Python loop over 200 rows of the 11^5 model, and the normwise agreement of
``integrate_batch`` with it on those rows.

    python tools/bary_box_probe.py [--steps 20] [--warmup 5] [--n 1000000]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import functions as F  # noqa: E402
from pychebyshev_amd import ChebyshevApproximation, _lib  # noqa: E402
from pychebyshev_amd._calculus import box_rows  # noqa: E402
from tt_box_probe import DeviceTimer, upload  # noqa: E402


def make_rows(dom, dims, N, seed):
    rng = np.random.default_rng(seed)
    dom = np.asarray(dom, dtype=float)
    kept = [k for k in range(len(dom)) if k not in dims]
    span = (dom[dims, 1] - dom[dims, 0])[None, :]
    w = rng.uniform(0.05, 1.0, (N, len(dims))) * span
    lo = dom[dims, 0][None, :] + rng.uniform(0.0, 1.0, (N, len(dims))) * (span - w)
    bounds = np.stack([lo, np.minimum(lo + w, dom[dims, 1][None, :])], axis=2)
    points = np.column_stack([rng.uniform(dom[k, 0], dom[k, 1], N) for k in kept]) if kept else None
    return bounds, points


def smooth_model(shape):
    d = len(shape)
    dom = [[-1.0, 1.0], [0.5, 3.0], [-2.0, -0.25]][:d]
    nodes = ChebyshevApproximation.nodes(d, dom, list(shape))["nodes_per_dim"]
    mesh = np.meshgrid(*nodes, indexing="ij")
    T = np.exp(0.3 * mesh[0]) * (1.5 + np.sin(mesh[1] + (0.5 * mesh[2] if d > 2 else 0.0)))
    return ChebyshevApproximation.from_values(T, d, dom, list(shape))


def info(c, name, k):
    m = c._model()
    a = _lib.i32(np.zeros(k))
    _lib.check(getattr(m.lib, name)(m.handle, _lib.p_i32(a)), m.lib)
    return [int(v) for v in a]


def leg(name, c, dims, N, variant, args):
    m = c._model()
    lib, dev = m.lib, m.device
    _lib.check(lib.pcx_bary_set_kernel(m.handle, 0), lib)
    d = c.num_dimensions
    dom = np.asarray(c.domain, dtype=float)
    lo, hi = _lib.f64(dom[:, 0]), _lib.f64(dom[:, 1])
    st = ctypes.c_void_p()
    _lib.check(lib.pcx_bary_stream(m.handle, ctypes.byref(st)), lib)
    timer = DeviceTimer(lib, dev)
    bounds, points = make_rows(dom, dims, N, 7 + len(dims))
    flags, rows = box_rows(d, c.domain, dims, bounds, points)
    flags = _lib.i32(flags)
    pts = np.column_stack([np.random.default_rng(5).uniform(a, b, N) for a, b in dom])
    d_rows, d_pts = upload(lib, dev, rows), upload(lib, dev, pts)
    d_out, d_val = upload(lib, dev, np.zeros(N)), upload(lib, dev, np.zeros(N))

    def box():
        # the forced form holds for the box launch only: the evaluation stays on the handle's own choice
        _lib.check(lib.pcx_bary_set_kernel(m.handle, variant), lib)
        _lib.check(lib.pcx_bary_box_batch_dev(m.handle, _lib.p_i32(flags), _lib.p_f64(lo), _lib.p_f64(hi), d_rows, N, d_out, st), lib)
        _lib.check(lib.pcx_bary_set_kernel(m.handle, 0), lib)

    def ev():
        _lib.check(lib.pcx_bary_eval_batch_dev(m.handle, d_pts, N, None, d_val, st), lib)

    _lib.check(lib.pcx_bary_set_kernel(m.handle, variant), lib)
    form = info(c, "pcx_bary_box_info", 4)
    _lib.check(lib.pcx_bary_set_kernel(m.handle, 0), lib)
    t_box, t_ev = timer.median_pair_ms(box, ev, st, args.warmup, args.steps)
    for p in (d_rows, d_pts, d_out, d_val):
        lib.pcx_dev_free(dev, p)
    flops = 2.0 * float(np.prod(c.n_nodes)) * N
    print(f"{name:<28} {len(dims):>2} {N:>8} {('mfma' if form[0] else 'rows'):>5} {t_box:>9.3f} {N / t_box * 1e3:>11.3e} "
          f"{flops / t_box * 1e-9:>8.2f} {t_ev:>9.3f} {N / t_ev * 1e3:>11.3e} {flops / t_ev * 1e-9:>8.2f} {t_box / t_ev:>8.3f}",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000)
    args = ap.parse_args()
    T = np.load(os.path.join(ROOT, "tests", "golden", "g2_bs5d.npz"))["tensor"]
    bs = ChebyshevApproximation.from_values(T, 5, F.BS5_DOMAIN, F.BS5_NODES)
    print(f"11^5: kernel_info {info(bs, 'pcx_bary_kernel_info', 6)} box_info {info(bs, 'pcx_bary_box_info', 4)}")
    print(f"{'model':<28} {'m':>2} {'N':>8} {'form':>5} {'box ms':>9} {'box rows/s':>11} {'TFLOP/s':>8} {'eval ms':>9} "
          f"{'eval pts/s':>11} {'TFLOP/s':>8} {'box/eval':>8}", flush=True)
    for dims in ([0], [1, 3], [0, 1, 2, 3, 4]):
        leg("11^5 bench model", bs, dims, args.n, 0, args)
    leg("11^5, rows form forced", bs, [1, 3], max(1, args.n // 10), 1, args)
    sq = smooth_model((12, 12))
    leg("12 x 12", sq, [0], args.n, 0, args)
    cube = smooth_model((20, 20, 20))
    print(f"20^3: grid_info {info(cube, 'pcx_bary_grid_info', 4)}")
    leg("20^3 (grid / k-fold plan)", cube, [0, 2], args.n, 0, args)
    # the "before": one reduced model and one device handle per row
    dims = [1, 3]
    bounds, points = make_rows(F.BS5_DOMAIN, dims, 200, 3)
    t0 = time.perf_counter()
    loop = np.array([bs.integrate(dims, [tuple(b) for b in bounds[r]]).vectorized_eval(points[r], [0, 0, 0]) for r in range(200)])
    per_row = (time.perf_counter() - t0) / 200
    batch = bs.integrate_batch(dims, bounds, points)
    err = float(np.max(np.abs(batch - loop)) / np.max(np.abs(loop)))
    print(f"per-row integrate(...).vectorized_eval(...) loop on 11^5, m = 2: {per_row * 1e3:.3f} ms per row = {1 / per_row:.3e} rows/s; "
          f"integrate_batch against it on those 200 rows: normwise {err:.2e}", flush=True)


if __name__ == "__main__":
    main()
