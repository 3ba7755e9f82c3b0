#!/usr/bin/env python3
"""Rates of ladder_batch / fibre_batch against the pointwise route, on the device (writes profiles/ladder_probe.txt).

    python tools/ladder_probe.py [--rows 100000] [--out profiles/ladder_probe.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/ladder_probe.py --trace      (the kernel split, a run of its own)

Method: rows, values and result device-resident; one warm-up call, then the median of 5 calls, host clock around a
call that ends in a stream synchronise (ladder_batch with device rows is complete on return).  The baseline is existing
code, vectorized_eval_batch / eval_batch on the device-resident expanded N m points, timed the same way.

Per case: rows/s of each form, the ratio to the baseline's rows/s (= its points/s over m), for the MFMA form the share
of the 78.6 TFLOP/s FP64 peak by EXECUTED matrix instructions (k-steps x column tiles x 2048 flop per 16 rows, from
pcx_bary_ladder_info: padding included, the epilogue's time included in the denominator), and the share of the 1-D
epilogue, estimated as 1 - t(m = 1) / t(m) on the same rows (the contraction does not depend on m).
"""
from __future__ import annotations

import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from pychebyshev_amd import ChebyshevApproximation, ChebyshevTT, _lib  # noqa: E402
from pychebyshev_amd.device import DeviceArray  # noqa: E402

PEAK = 78.6e12


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


def uniform_rows(rng, domain, dim, N):
    others = [k for k in range(len(domain)) if k != dim]
    return np.column_stack([rng.uniform(domain[k][0], domain[k][1], N) for k in others]) if others else np.empty((N, 0))


def dense_case(log, name, model, domain, dim, ms, N, trace):
    d = model.num_dimensions
    rng = np.random.default_rng(7)
    fixed = uniform_rows(rng, domain, dim, N)
    dev = model._model()
    dfixed = DeviceArray.from_host(fixed, dev.device)
    info = np.zeros(3, dtype=np.int32)
    for m in ms:
        xs = np.asarray(model.nodes[dim], dtype=float) if m == "fibre" else np.linspace(domain[dim][0], domain[dim][1], m)
        mm = xs.size
        out = DeviceArray.empty((N, mm), dev.device)
        out1 = DeviceArray.empty((N, 1), dev.device)
        res = {}
        for form in ("auto", "rows"):
            _lib.check(dev.lib.pcx_bary_set_kernel(dev.handle, 1 if form == "rows" else 0), dev.lib)
            _lib.check(dev.lib.pcx_bary_ladder_info(dev.handle, dim, _lib.p_i32(info)), dev.lib)
            if form == "auto" and not info[0]:
                continue
            t = median_time(lambda: model.ladder_batch(dim, dfixed, xs, out=out))
            t1 = median_time(lambda: model.ladder_batch(dim, dfixed, xs[:1], out=out1))
            res[form] = (t, t1, int(info[1]) * int(info[2]))
            if trace:
                break
        _lib.check(dev.lib.pcx_bary_set_kernel(dev.handle, 0), dev.lib)
        if trace:
            continue
        dpts = DeviceArray.from_host(expand(d, dim, fixed, xs), dev.device)
        tb = median_time(lambda: model.vectorized_eval_batch(dpts, [0] * d))
        base = N / tb
        for form, (t, t1, instr) in res.items():
            label = "mfma" if form == "auto" else "rows"
            peak = f"  {instr * 2048.0 * (N / 16.0) / t / PEAK:.3f} of FP64 peak (executed MFMA)" if form == "auto" else ""
            log(f"{name:<14} dim {dim} m {mm:>3} {label:<5} {N / t:10.3e} rows/s  x{(N / t) / base:6.2f} of pointwise "
                f"({base:9.3e} rows/s = {base * mm:9.3e} pts/s)  epilogue share {max(0.0, 1.0 - t1 / t):.2f}{peak}")


def tt_case(log, name, tt, dim, m, N, trace):
    d = tt.num_dimensions
    udom = tt._user_frame_domain()
    rng = np.random.default_rng(8)
    fixed = uniform_rows(rng, udom, dim, N)
    t_ = tt._dev()
    dfixed = DeviceArray.from_host(fixed, t_.device)
    xs = np.linspace(udom[dim][0], udom[dim][1], m)
    out = DeviceArray.empty((N, m), t_.device)
    out1 = DeviceArray.empty((N, 1), t_.device)
    t = median_time(lambda: tt.ladder_batch(dim, dfixed, xs, out=out))
    if trace:
        return
    t1 = median_time(lambda: tt.ladder_batch(dim, dfixed, xs[:1], out=out1))
    dpts = DeviceArray.from_host(expand(d, dim, fixed, xs), t_.device)
    tb = median_time(lambda: tt.eval_batch(dpts))
    base = N / tb
    log(f"{name:<14} dim {dim} m {m:>3} tt    {N / t:10.3e} rows/s  x{(N / t) / base:6.2f} of pointwise "
        f"({base:9.3e} rows/s = {base * m:9.3e} pts/s)  series share {max(0.0, 1.0 - t1 / t):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ladder_probe.txt"))
    ap.add_argument("--trace", action="store_true", help="one timed pass per case and no baseline: for rocprofv3 --kernel-trace")
    args = ap.parse_args()
    import functions as F
    N = args.rows
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"ladder_probe: N = {N} rows, device-resident, median of 5 after one warm-up, host clock around a synchronised call")
    g2 = np.load(os.path.join(ROOT, "tests", "golden", "g2_bs5d.npz"))
    bs = ChebyshevApproximation.from_values(g2["tensor"], 5, F.BS5_DOMAIN, list(F.BS5_NODES))
    for dim in (0, 4):
        dense_case(log, "bs 11^5", bs, F.BS5_DOMAIN, dim, ["fibre", 21, 101], N, args.trace)
    dom2 = [[-1.0, 1.0], [0.0, 2.0]]
    n2 = [12, 12]
    nodes2 = ChebyshevApproximation.nodes(2, dom2, n2)["nodes_per_dim"]
    t2 = np.sin(nodes2[0])[:, None] * np.cos(nodes2[1])[None, :]
    dense_case(log, "12 x 12", ChebyshevApproximation.from_values(t2, 2, dom2, n2), dom2, 0, [21], N, args.trace)
    dom3 = [[-1.0, 1.0]] * 3
    n3 = [32, 32, 32]
    nodes3 = ChebyshevApproximation.nodes(3, dom3, n3)["nodes_per_dim"]
    t3 = np.sin(nodes3[0])[:, None, None] + np.sin(nodes3[1])[None, :, None] * np.cos(nodes3[2])[None, None, :]
    dense_case(log, "32^3", ChebyshevApproximation.from_values(t3, 3, dom3, n3), dom3, 1, [21], N, args.trace)

    g22 = np.load(os.path.join(ROOT, "tests", "golden", "g22_tt_transforms.npz"))
    ttc = ChebyshevTT.from_coeff_cores([g22[f"C_core{k}"] for k in range(5)], g22["C_domain"].tolist())
    tt_case(log, "TT 5-D r8", ttc, 2, 21, N, args.trace)
    g5 = np.load(os.path.join(ROOT, "tests", "golden", "g5_tt_rank16.npz"))
    cores = [g5[f"core{k}"] for k in range(10)]
    tt10 = ChebyshevTT.from_coeff_cores(cores, [[-1.0, 1.0]] * 10)
    tt_case(log, "TT 10-D r16", tt10, 5, 21, N, args.trace)

    if not args.trace:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
