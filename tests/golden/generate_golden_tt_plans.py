"""Accepted kernels and output digests of the tensor-train handle, one case per evaluation form and rank class.

    python tests/golden/generate_golden_tt_plans.py [--out tests/golden/g36_tt_plans.npz]

needs an MI355X and talks to the library through its C ABI only (pychebyshev_amd._lib), so the same file runs on any
commit that has the ABI.  For every case it creates a handle on seeded random cores and records

  * the return code of pcx_tt_create and, where it fails, the error text,
  * which of set_kernel(1..4) are accepted,
  * the SHA-256 of eval_batch at N = 333 seeded in-domain points (full 64- and 256-point blocks and a ragged one) on auto
    ("0") and on every accepted variant ("1".."4"),
  * the SHA-256 of eval_multi_batch on auto for the value, one first-order and one second-order spec.

Every digest is evaluated twice; a case whose two runs differ is not written (its name is printed).
tests/test_gpu_tt_plan.py measures the same records with the library under test and compares them exactly;
tests/test_tt_plan_host.py checks the plan itself on a CPU.

The file written holds one JSON text ("records") and nothing else.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "g36_tt_plans.npz")
N_POINTS = 333


def _c(name, n, ranks, order=None, lo=None):
    return {"id": name, "n": list(n), "ranks": list(ranks), "order": order, "lo": lo}


def _u(d, n, r):
    """d dimensions of n nodes with every inner rank r."""
    return [n] * d, [1] + [r] * (d - 1) + [1]


CASES = [
    _c("d1", [7], [1, 1]),                                        # one dimension: every small-rank form, lane-per-point on auto
    _c("d16_n2_r2", *_u(16, 2, 2)),
    _c("r4_n8", *_u(4, 8, 4)),                                    # lane-per-point cap 8
    _c("r8_n11", *_u(4, 11, 8)),                                  # 4x4x4 preferred to W-first
    _c("r12_n12", *_u(4, 12, 12)),                                # W-first preferred to 4x4x4, lane-per-point cap 12
    _c("r13_n9", *_u(4, 9, 13)),                                  # lane-per-point cap 16, no small-rank MFMA form
    _c("r16_n10", *_u(4, 10, 16)),                                # lane-per-point exists, auto takes the 16x16x4 form
    _c("r5_n17", *_u(4, 17, 5)),                                  # W-first only
    _c("r5_n33", *_u(3, 33, 5)),                                  # class 0 direct only
    _c("r12_n32_d3", *_u(3, 32, 12)),                             # W-first inside its 96 KiB
    _c("r12_n32_d5", *_u(5, 32, 12)),                             # ... and past it
    _c("r17_n6", *_u(4, 6, 17)),                                  # class 1
    _c("r32_n5", *_u(3, 5, 32)),
    _c("r33_n5", *_u(3, 5, 33)),                                  # class 2
    _c("r64_n4", *_u(3, 4, 64)),
    _c("r65_n4", *_u(3, 4, 65)),                                  # generic
    _c("mixed_order", [5, 9, 4, 7], [1, 3, 5, 2, 1], order=[2, 0, 3, 1]),
    _c("mixed_r20", [3, 18, 6], [1, 20, 7, 1], order=[1, 2, 0]),
    _c("r4097", [1, 1], [1, 4097, 1]),                            # UNSUPPORTED
    _c("lds_over", [5, 5], [1, 2558, 1]),                         # 2 rank + nodes = 5121: UNSUPPORTED
    _c("bad_boundary", [4, 4], [2, 3, 1]),
    _c("bad_domain", [4, 4], [1, 3, 1], lo=[0.0, 5.0]),           # lo[1] >= hi[1]
    _c("bad_order", [4, 4], [1, 3, 1], order=[1, 1]),
]


def model_arrays(case):
    """n_nodes, ranks, lo, hi, the seeded cores (concatenated [a][j][b]) and dim_order (or None) of a case."""
    n, ranks = case["n"], case["ranks"]
    d = len(n)
    lo = np.array(case["lo"] if case["lo"] else [-1.0 - 0.125 * k for k in range(d)])
    hi = np.array([1.0 + 0.25 * k for k in range(d)])
    seed = int.from_bytes(hashlib.sha256(case["id"].encode()).digest()[:4], "little")
    rng = np.random.default_rng(seed)
    cores = np.concatenate([rng.standard_normal(ranks[k] * n[k] * ranks[k + 1]) / np.sqrt(ranks[k]) for k in range(d)])
    return np.array(n, np.int32), np.array(ranks, np.int32), lo, hi, cores, case["order"]


def _twice(run):
    """SHA-256 of run()'s output, evaluated twice: None when the two runs differ."""
    seen = [hashlib.sha256(run().tobytes()).hexdigest() for _ in range(2)]
    return seen[0] if seen[0] == seen[1] else None


def measure(case, device=0):
    """The record of one case with the library as it is built now."""
    from pychebyshev_amd import _lib as L
    lib = L.load()
    n, ranks, lo, hi, cores, order = model_arrays(case)
    d = len(n)
    rec = {"id": case["id"]}
    h = ctypes.c_void_p()
    rc = lib.pcx_tt_create(device, d, L.p_i32(n), L.p_i32(ranks), L.p_f64(lo), L.p_f64(hi), L.p_f64(cores),
                           L.p_i32(L.i32(order)) if order else None, ctypes.byref(h))
    rec["rc"] = int(rc)
    if rc != 0:
        rec["error"] = L.last_error(lib)
        return rec
    try:
        rec["set_kernel"] = [lib.pcx_tt_set_kernel(h, v) == 0 for v in (1, 2, 3, 4)]
        pts = np.random.default_rng(36).uniform(lo, hi, (N_POINTS, d))       # columns in the user's order, as the domain is

        def values():
            out = np.full(N_POINTS, np.nan)
            L.check(lib.pcx_tt_eval_batch(h, L.p_f64(pts), N_POINTS, L.p_f64(out)), lib)
            return out

        rec["digest"] = {}
        for v in [0] + [v for v, ok in zip((1, 2, 3, 4), rec["set_kernel"]) if ok]:
            L.check(lib.pcx_tt_set_kernel(h, v), lib)
            rec["digest"][str(v)] = _twice(values)
        L.check(lib.pcx_tt_set_kernel(h, 0), lib)
        specs = np.zeros((3, d), np.int32)
        specs[1, 0] = 1
        specs[2, d - 1] = 2

        def greeks():
            out = np.full((N_POINTS, 3), np.nan)
            L.check(lib.pcx_tt_eval_multi_batch(h, L.p_f64(pts), N_POINTS, L.p_i32(specs), 3, L.p_f64(out)), lib)
            return out

        rec["digest_multi"] = _twice(greeks)
    finally:
        lib.pcx_tt_destroy(h)
    return rec


def unstable(rec):
    return rec["rc"] == 0 and (rec["digest_multi"] is None or None in rec["digest"].values())


def load(path=OUT):
    """id -> record of the committed fixture."""
    with np.load(path) as z:
        return {r["id"]: r for r in json.loads(str(z["records"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    records, dropped = [], []
    for case in CASES:
        r = measure(case)
        (dropped if unstable(r) else records).append(r)
        print(json.dumps(r), flush=True)
    if dropped:
        print("NOT WRITTEN (two runs of a digest differed):", [r["id"] for r in dropped])
    assert len(dropped) <= 2, "more than two cases have no stable digest: the digest approach does not hold"
    np.savez_compressed(args.out, records=np.array(json.dumps(records)))
    print(f"wrote {len(records)} records to {args.out}")


if __name__ == "__main__":
    main()
