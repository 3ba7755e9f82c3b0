#!/usr/bin/env python3
"""Generate tests/golden/g23_tt_completion.npz: the reference's ``ChebyshevTT.run_completion`` (fixed-rank ALS with a
dense ``lstsq`` per core) on six small models.

Run in the build container only (the reference checkout does not travel to the GPU box), on the CPU:

    python tests/golden/generate_golden_tt_completion.py --ref <reference checkout>

It imports PyChebyshev v0.21.1 from ``<ref>/src`` and stores arrays only.

    model  d  n           start ranks     reaches
    M1     1  6           1,1             single core = values
    M2     2  9,7         1,3,1           no middle core
    M3     3  6,5,7       1,8,8,1         bonds shrink to 6 and 7
    M4     4  7,6,8,5     1,3,4,3,1       small ranks, all ragged; the tolerance-stopped run
    M4o                                   M4's cores behind dim_order [2,0,3,1] (the ``values=`` path)
    M16    4  18,3,19,4   1,17,16,4,1     ranks on both sides of 16, nothing a multiple of 4
    M5     5  8^5         1,4,5,5,4,1     five cores, about 30 s in the reference

The target ``T`` is :func:`target_function` on the Chebyshev grid of the model's domain (storage frame, ascending
nodes: ``from_values``' order), evaluated point by point, so the reference's callback sees exactly the stored values.
The start cores are a TT-SVD of ``T`` truncated to the listed ranks (NumPy SVDs), every entry multiplied by
``1 + 0.05 N(0, 1)`` (seeded); where an unfolding cannot hold a listed rank the surplus rows and columns are filled with
``0.05 max|core| N(0, 1)``.  They are stored as coefficient cores (the reference's value -> coefficient conversion).

Keys, ``<M>`` a model:

    <M>_n, <M>_domain (storage frame), <M>_order, <M>_start_core<k> (coefficient cores)
    <M>_T                        the target; not stored for M5 (a third of the file): target_tensor(domain, n) rebuilds it
    <M>_pts (32, d) in the user frame, <M>_eval_m1, <M>_eval_m3, <M>_dense_m1, <M>_dense_m3
        the reference's eval / to_dense() after run_completion(tolerance=0.0, max_iter=m) from the start cores
        (tolerance 0.0 fixes the iteration count); m = 1 is the first of three single steps, m = 3 one call
    <M>_dense_m0, <M>_dense_m2   the start tensor and the tensor after two single steps (SMALL models only)
    <M>_rel_change (3,)          ||T_i - T_{i-1}||_F / (||T_{i-1}||_F + 1e-30) over the single steps, recomputed here
                                 from the successive to_dense() tensors (the reference only prints three digits)
    <M>_ref_seconds (2,)         the reference's wall time of the three single steps and of the m = 3 call
    M4_tol, M4_tol_iters, M4_tol_dense, M4_tol_history
        a run stopped by the tolerance: tolerance = geometric mean of two consecutive rel_change values a factor of at
        least 100 apart, so the iteration count does not hinge on rounding
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NOISE = 0.05
MODELS = {
    "M1": (201, [6], [1, 1], None),
    "M2": (202, [9, 7], [1, 3, 1], None),
    "M3": (203, [6, 5, 7], [1, 8, 8, 1], None),
    "M4": (204, [7, 6, 8, 5], [1, 3, 4, 3, 1], None),
    "M4o": (204, [7, 6, 8, 5], [1, 3, 4, 3, 1], [2, 0, 3, 1]),
    "M16": (216, [18, 3, 19, 4], [1, 17, 16, 4, 1], None),
    "M5": (205, [8] * 5, [1, 4, 5, 5, 4, 1], None),
}
SMALL = ("M1", "M2", "M3", "M4")            # every intermediate tensor is stored for these
RECOMPUTED_T = ("M5",)                      # the target is not stored (file size): target_tensor() gives it again
DOMAINS = [[-1.0, 1.0], [0.5, 3.0], [-2.0, -0.25], [0.0, 1.0], [-1.5, 0.5]]     # storage position k: DOMAINS[k]
COEF_Q = [0.9, 0.35, 0.6, 1.1, 0.5]
COEF_S = [1.3, 0.7, -0.9, 1.7, 0.8]


def target_function(point, _data=None):
    """Smooth, bounded away from zero (1.2 .. 2.8), TT ranks that decay slowly."""
    q = 1.0
    s = 0.0
    for k, x in enumerate(point):
        q += COEF_Q[k] * x * x
        s += COEF_S[k] * x
    return 1.5 + 1.0 / q + 0.25 * float(np.sin(s))


def grids_for(domain, n):
    from numpy.polynomial.chebyshev import chebpts1
    return [np.sort(0.5 * (a + b) + 0.5 * (b - a) * chebpts1(nk)) for (a, b), nk in zip(domain, n)]


def target_tensor(domain, n):
    grids = grids_for(domain, n)
    T = np.empty(n)
    for idx in np.ndindex(*n):
        T[idx] = target_function([float(grids[k][idx[k]]) for k in range(len(n))])
    return T


def start_value_cores(T, ranks, seed):
    """Truncated TT-SVD at the listed ranks, padded where an unfolding is too small, with multiplicative noise."""
    rng = np.random.default_rng(seed)
    n = T.shape
    d = len(n)
    cores = []
    C = T.reshape(1, -1)
    r_prev = 1
    for k in range(d - 1):
        C = C.reshape(r_prev * n[k], -1)
        U, S, Vt = np.linalg.svd(C, full_matrices=False)
        r = min(ranks[k + 1], len(S))
        cores.append(U[:, :r].reshape(r_prev, n[k], r))
        C = S[:r, None] * Vt[:r]
        r_prev = r
    cores.append(C.reshape(r_prev, n[-1], 1))
    out = []
    for k, c in enumerate(cores):
        full = NOISE * np.max(np.abs(c)) * rng.standard_normal((ranks[k], n[k], ranks[k + 1]))
        full[:c.shape[0], :, :c.shape[2]] = c * (1.0 + NOISE * rng.standard_normal(c.shape))
        out.append(full)
    return out


def rel_changes(tensors):
    return np.array([np.linalg.norm(tensors[i + 1] - tensors[i]) / (np.linalg.norm(tensors[i]) + 1e-30)
                     for i in range(len(tensors) - 1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of PyChebyshev v0.21.1")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.ref, "src"))
    import pychebyshev as ref
    from pychebyshev import ChebyshevTT
    from pychebyshev.tensor_train import _value_core_to_coeff_core

    print("reference version", ref.__version__)

    def make_tt(coeff_cores, domain, order):
        n = [c.shape[1] for c in coeff_cores]
        obj = ChebyshevTT(target_function, len(n), [list(b) for b in domain], n, max_rank=64)
        obj._coeff_cores = [np.array(c) for c in coeff_cores]
        obj._tt_ranks = [1] + [c.shape[2] for c in coeff_cores]
        obj._built = True
        obj.method = "svd"
        if order is not None:
            obj._dim_order = list(order)
        return obj

    out = {}
    for tag, (seed, n, ranks, order) in MODELS.items():
        d = len(n)
        domain = DOMAINS[:d]
        T = target_tensor(domain, n)
        start = [_value_core_to_coeff_core(c) for c in start_value_cores(T, ranks, seed)]
        dim_order = list(range(d)) if order is None else list(order)
        udom = [domain[dim_order.index(u)] for u in range(d)]
        rng = np.random.default_rng(seed + 5000)
        pts = np.column_stack([rng.uniform(a, b, 32) for a, b in udom])
        out[f"{tag}_n"] = np.array(n, dtype=np.int64)
        out[f"{tag}_domain"] = np.array(domain, dtype=float)
        out[f"{tag}_order"] = np.array(dim_order, dtype=np.int64)
        if tag not in RECOMPUTED_T:
            out[f"{tag}_T"] = T
        out[f"{tag}_pts"] = pts
        for k, c in enumerate(start):
            out[f"{tag}_start_core{k}"] = c

        stepper = make_tt(start, domain, order)
        tensors = [stepper.to_dense()]
        t0 = time.time()
        for step in range(3):
            stepper.run_completion(tolerance=0.0, max_iter=1)
            tensors.append(stepper.to_dense())
            if step == 0:
                out[f"{tag}_dense_m1"] = tensors[1]
                out[f"{tag}_eval_m1"] = np.array([stepper.eval(list(p)) for p in pts])
        t_steps = time.time() - t0
        once = make_tt(start, domain, order)
        t0 = time.time()
        once.run_completion(tolerance=0.0, max_iter=3)
        t_once = time.time() - t0
        out[f"{tag}_dense_m3"] = once.to_dense()
        out[f"{tag}_eval_m3"] = np.array([once.eval(list(p)) for p in pts])
        out[f"{tag}_rel_change"] = rel_changes(tensors)
        out[f"{tag}_ref_seconds"] = np.array([t_steps, t_once])
        if tag in SMALL:
            out[f"{tag}_dense_m0"] = tensors[0]
            out[f"{tag}_dense_m2"] = tensors[2]
        scale = np.max(np.abs(T))
        print(f"{tag}: ranks after {[1] + [c.shape[2] for c in once._coeff_cores]}, rel_change {out[f'{tag}_rel_change']}, "
              f"|steps - once| / max|T| = {np.max(np.abs(tensors[3] - out[f'{tag}_dense_m3'])) / scale:.2e}, "
              f"reference {t_steps:.1f} s + {t_once:.1f} s")

        if tag == "M4":
            for _ in range(5):
                stepper.run_completion(tolerance=0.0, max_iter=1)
                tensors.append(stepper.to_dense())
            hist = rel_changes(tensors)
            pick = next((i for i in range(len(hist) - 1) if hist[i + 1] > 0 and hist[i] / hist[i + 1] >= 100.0), None)
            assert pick is not None, f"no two consecutive rel_change values a factor 100 apart: {hist}"
            tol = float(np.sqrt(hist[pick] * hist[pick + 1]))
            assert np.min(hist[:pick + 1]) >= 10.0 * tol and hist[pick + 1] <= tol / 10.0, (hist, tol)
            stopped = make_tt(start, domain, order)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                stopped.run_completion(tolerance=tol, max_iter=50, verbose=True)
            iters = sum(1 for line in buf.getvalue().splitlines() if "ALS iter" in line)
            assert iters == pick + 2, (iters, pick, hist, tol)
            out["M4_tol"] = np.array(tol)
            out["M4_tol_iters"] = np.array(iters, dtype=np.int64)
            out["M4_tol_dense"] = stopped.to_dense()
            out["M4_tol_history"] = hist
            print(f"M4 tolerance run: history {hist}, tolerance {tol:.3e}, stops after {iters} iterations")

    path = os.path.join(HERE, "g23_tt_completion.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
