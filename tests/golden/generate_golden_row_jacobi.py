#!/usr/bin/env python3
"""Generate tests/golden/g30_row_jacobi.npz: what the row-Jacobi factorisation (rowjacobi_factor in
csrc/pcx_ttbuild.hip) is held to on every (shape, family) of tests/row_jacobi.py.  CPU only, NumPy and mpmath:

    python tests/golden/generate_golden_row_jacobi.py            # write the fixture
    python tests/golden/generate_golden_row_jacobi.py --search   # print graded seeds that meet the gap condition

Only numbers are stored, no matrices -- the tests rebuild every matrix from its seed.  Per case <m>x<N>_<family>:

  _sum, _sumsq   int64: the sum and the sum of squares of every integer drawn for the matrix
  _fig           figures (a) .. (d) of tests/row_jacobi.figures for the NumPy restatement of the iteration
  _sweeps        its sweep count
  _sigma         graded only: the singular values, the square roots of the eigenvalues of C C^T (or C^T C
                 when that is smaller).  The entries are integers times 2^-k, so the Gram matrix is accumulated exactly
                 in Python integers; mpmath solves it at 80 digits
  _rel           graded and hadamard: the restatement's relative figure (row_jacobi.relative_figure)
                 against _sigma / the exact values

The rank-rule cases (row_jacobi.RANK_SHAPES, graded) must keep every singular value a factor row_jacobi.RANK_GAP
away from each cut tol * sigma_0, tol in RANK_TOLS: asserted here, a condition on the inputs.  The file is written with
fixed zip time stamps, so a second run reproduces it byte for byte.
"""
from __future__ import annotations

import io
import os
import sys
import time
import zipfile

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import row_jacobi as RJ  # noqa: E402

DIGITS = 80


def exact_sigma(C):
    """Singular values of an integer-times-2^-k matrix from the exact Gram matrix, 80 digits, descending, as float64."""
    m, N = C.shape
    A = C if m <= N else C.T
    scaled = A * 2.0 ** 40
    ints = scaled.astype(np.int64)
    assert np.array_equal(ints.astype(float), scaled)
    Ai = ints.astype(object)
    G = Ai @ Ai.T
    with mpmath.workdps(DIGITS):
        ev = mpmath.eigsy(mpmath.matrix(G.tolist()), eigvals_only=True)
        s = sorted((mpmath.sqrt(max(v, 0)) / mpmath.mpf(2) ** 40 for v in ev), reverse=True)
        return np.array([float(v) for v in s])


def gap_ok(m, sigma):
    g = RJ.RANK_GAP
    for tol in RJ.RANK_TOLS:
        cut = tol * sigma[0]
        if np.any((sigma > cut / g) & (sigma < cut * g)):
            return False
    return True


def search():
    for (m, N) in RJ.RANK_SHAPES:
        for seed in range(10000):
            RJ.GRADED_SEED[(m, N)] = seed
            RJ.matrix.cache_clear()
            if gap_ok(m, np.linalg.svd(RJ.matrix("graded", m, N)[0], compute_uv=False)):
                print(f"({m}, {N}): {seed},")
                break
        else:
            raise SystemExit(f"no seed for {m}x{N}")


def write(path, out):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(out[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    if "--search" in sys.argv[1:]:
        return search()
    t0 = time.time()
    out = {}
    worst = {k: 0.0 for k in "abcd"}
    for (m, N, fam) in RJ.cases():
        C, draw = RJ.matrix(fam, m, N)
        key = RJ.key(m, N, fam)
        out[key + "_sum"], out[key + "_sumsq"] = (np.int64(v) for v in RJ.checksum(draw))
        sref = None
        if fam == "hadamard":
            sref = RJ.hadamard_sigma(m, N)
        elif fam == "graded":
            sref = out[key + "_sigma"] = exact_sigma(C)
            if (m, N) in RJ.RANK_SHAPES:
                assert gap_ok(m, sref), f"{key}: a singular value next to a cut; run --search and update GRADED_SEED"
        U, B, sweeps = RJ.restatement(C)
        assert sweeps < RJ.MAX_SWEEPS
        Us, Bs = RJ.select(U, B)
        f = RJ.figures(C, Us, Bs, sref)
        out[key + "_fig"] = np.array([f[k] for k in "abcd"])
        out[key + "_sweeps"] = np.int32(sweeps)
        line = f"  {key:>20}: sweeps {sweeps:2d}  " + "  ".join(f"{k} {f[k]:.1e}" for k in "abcd")
        if sref is not None:
            rel = out[key + "_rel"] = np.float64(RJ.relative_figure(Bs, sref, m))
            line += f"  rel {rel:.1e}"
        print(line, flush=True)
        for k in "abcd":
            worst[k] = max(worst[k], f[k])
    path = os.path.join(HERE, "g30_row_jacobi.npz")
    write(path, out)
    print(f"  wrote g30_row_jacobi.npz ({os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays) in {time.time() - t0:.1f} s;"
          f" restatement worst " + ", ".join(f"{k} {worst[k]:.1e}" for k in "abcd"))
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
