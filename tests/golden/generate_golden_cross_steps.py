#!/usr/bin/env python3
"""Generate tests/golden/g31_cross_steps.npz: what the TT-Cross dense steps (csrc/ttcross_kernels.h) are held to on
every case of tests/cross_steps.py.  CPU only, NumPy, SciPy (through oracle._cross_step) and mpmath:

    python tests/golden/generate_golden_cross_steps.py            # write the fixture
    python tests/golden/generate_golden_cross_steps.py --search   # print seeds that meet the input conditions

No matrix that a seed can rebuild is stored.  Per case <m>x<c>_<family>, from the FP64 matrix C as given:

  _sum, _sumsq   the checksum of the Gaussian draws behind C; _csum: the same two figures of C itself
  _sigma         the singular values: square roots of the eigenvalues of C^T C (C C^T when m < c), the Gram matrix
                 accumulated exactly in Python integers and solved by mpmath.eigsy at 80 digits
  _rank          the reference's rank: #{sigma > 1e-12 sigma_0}, capped by cap, m and c
  _utop          m <= 256: the leading `rank` left singular vectors at 80 digits, rounded to FP64 (equal_sigma: the
                 Hadamard columns in the stable order of the exactly equal values; zero: absent)
  _piv, _margin  the pivots of cross_steps.maxvol_restated(U_top) and the smallest decision margin it met; for
                 m > 256 U_top is LAPACK's.  _ontol: whether it stopped on tol (and not on max_iters)
  _dev           oracle_dev = max|C_hat_LAPACK - C_hat_ref|, C_hat_LAPACK from oracle._cross_step and
                 C_hat_ref = U_top inv(U_top[piv]) in longdouble at the same pivots (m <= 256; 0 where LAPACK's choice
                 inside an exactly degenerate pair is cut by cap, and for the zero matrix)

and per (rl, n, rr) of the DCT cases dct_<rl>x<n>x<rr>: the coefficient core at 40 digits or better (cosines from
mpmath at 60 digits as integers times 2^-150, the sums exact in Python integers, one correctly rounded division).

The input conditions of tests/cross_steps.py are asserted here.  Fixed zip time stamps: a second run reproduces the
file byte for byte.
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
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import cross_steps as CS  # noqa: E402

DIGITS = 80


# ---------------------------------------------------------------------------------------------- 80-digit SVD
def exact_ints(C):
    """(object array of Python integers, e) with C = ints * 2^e exactly."""
    C = np.asarray(C, dtype=np.float64)
    nz = C[C != 0.0]
    if nz.size == 0:
        return np.zeros(C.shape, dtype=object), 0
    e = int(np.min(np.frexp(nz)[1])) - 53
    scaled = np.ldexp(C, -e)
    assert np.all(np.isfinite(scaled)) and np.array_equal(scaled, np.rint(scaled))
    return np.array([[int(v) for v in row] for row in scaled], dtype=object), e


def svd80(C, rank):
    """(sigma (min(m, c),) float64 descending, U_top (m x rank) float64 or None when m > U_TOP_MAX_M)."""
    m, c = C.shape
    Ai, e = exact_ints(C)
    small_left = m < c
    G = (Ai @ Ai.T) if small_left else (Ai.T @ Ai)
    want_u = m <= CS.U_TOP_MAX_M
    with mpmath.workdps(DIGITS):
        Gm = mpmath.matrix(G.tolist())
        if want_u:
            ev, V = mpmath.eigsy(Gm)
        else:
            ev, V = mpmath.eigsy(Gm, eigvals_only=True), None
        k = len(ev)
        order = sorted(range(k), key=lambda i: -ev[i])
        two_e = mpmath.mpf(2) ** e
        sig = [mpmath.sqrt(max(ev[i], 0)) * two_e for i in order]
        sigma = np.array([float(s) for s in sig])
        if not want_u:
            return sigma, None
        U = np.zeros((m, rank))
        for t in range(rank):
            v = [V[i, order[t]] for i in range(k)]
            if small_left:
                col = v
            else:
                col = [mpmath.fsum(int(Ai[i, j]) * v[j] for j in range(k)) * two_e / sig[t] for i in range(m)]
            nrm = mpmath.sqrt(mpmath.fsum(x * x for x in col))
            U[:, t] = [float(x / nrm) for x in col]
        return sigma, U


def reference(m, c, fam, cap, seed=None, fast=False):
    """(sigma, rank, U_ref) of a case; `fast` takes LAPACK throughout (the seed search)."""
    C, _ = CS.matrix(m, c, fam, cap, seed)
    if fam == "zero":
        return np.zeros(min(m, c)), 1, None
    if fam == "equal_sigma":
        s = CS.equal_sigma_scales(c)
        order = np.argsort(-s, kind="stable")
        sigma = s[order] * np.sqrt(float(m))
        rank = CS.expected_rank(sigma, m, c, cap)
        return sigma, rank, CS.sylvester(m)[:, order[:rank]] / np.sqrt(float(m))
    if fast or m > CS.U_TOP_MAX_M:
        U, S, _ = np.linalg.svd(C, full_matrices=False)
        sigma = S if fast else svd80(C, 0)[0]
        rank = CS.expected_rank(sigma, m, c, cap)
        return sigma, rank, U[:, :rank]
    sigma = np.linalg.svd(C, compute_uv=False)
    rank = CS.expected_rank(sigma, m, c, cap)
    sigma, U = svd80(C, rank)
    assert rank == CS.expected_rank(sigma, m, c, cap)
    return sigma, rank, U


def gaps_ok(sigma, fam, cap):
    if sigma[0] == 0.0:
        return True
    cut = CS.REL_THRESH * sigma[0]
    if np.any((sigma > cut / CS.CUT_GAP) & (sigma < cut * CS.CUT_GAP)):
        return False
    if fam == "capcut" and not sigma[cap - 1] >= CS.CAP_GAP * sigma[cap]:
        return False
    return True


def margin_floor(dev):
    return max(CS.MARGIN_MIN, CS.MARGIN_OVER_DEV * dev)


def swap_case_ok(m, r, seed):
    """Three swaps at tol = 1, every decision with its margin, and pivots after two and after three swaps that differ
    from those of the update without its division: max_iters = k then tests the update, not only the count."""
    A = CS.swap_matrix(m, r, seed)
    for k in (2, 3):
        piv, tr = CS.maxvol_restated(A, 1.0, k)
        bad, trb = CS.maxvol_restated(A, 1.0, k, wrong_update=True)
        if tr.swaps != k or tr.margin < CS.MARGIN_MIN or trb.margin < CS.MARGIN_MIN or np.array_equal(piv, bad):
            return False
    return True


# ---------------------------------------------------------------------------------------------- the seed search
def search():
    print("SEEDS = {")
    for (m, c, fam, cap) in CS.CASES:
        if fam in ("zero", "equal_sigma"):
            continue
        for seed in range(20000):
            sigma, rank, U = reference(m, c, fam, cap, seed, fast=True)
            if not gaps_ok(sigma, fam, cap):
                continue
            if m <= rank:
                break
            _, tr = CS.maxvol_restated(U)
            # LAPACK's own deviation is about eps sigma_0 / sigma_rank / 2: leave a factor 4 for the real figure
            if tr.stopped_on_tol and tr.margin >= margin_floor(2.0 * CS.EPS * sigma[0] / sigma[rank - 1]):
                break
        else:
            raise SystemExit(f"no seed for {CS.key(m, c, fam)}")
        if seed:
            print(f'    "{CS.key(m, c, fam)}": {seed},', flush=True)
    print("}\nTIE_SEEDS = {")
    for dist in CS.TIE_DISTANCES:
        for neg in (False, True):
            for phase in (1, 2):
                for seed in range(200000):
                    first = int(np.random.default_rng([31, 102, seed]).integers(0, CS.TIE_M - dist))
                    A = CS.tie_matrix(dist, neg, seed, first, phase)
                    _, tr = CS.maxvol_restated(A)
                    hit = tr.tie_rows1 if phase == 1 else tr.tie_rows2
                    if first in hit and tr.stopped_on_tol and tr.margin >= CS.MARGIN_MIN:
                        break
                else:
                    raise SystemExit(f"no tie seed for {dist} {neg} {phase}")
                print(f"    ({dist}, {neg}, {phase}): ({seed}, {first}),", flush=True)
    print("}")
    m, r, _ = CS.SWAP_CASE
    for seed in range(10000):
        if swap_case_ok(m, r, seed):
            print(f"SWAP_CASE = ({m}, {r}, {seed})")
            break


# ---------------------------------------------------------------------------------------------- the DCT at 40 digits
def dct_exact(x):
    """k_value_to_coeff_core's definition with 150-bit cosines and exact sums, rounded once to FP64."""
    rl, n, rr = x.shape
    shift = 150
    with mpmath.workdps(60):
        T = np.array([[int(mpmath.floor(mpmath.cos(mpmath.pi * k * (2 * j + 1) / (2 * n)) * mpmath.mpf(2) ** shift + 0.5))
                       for j in range(n)] for k in range(n)], dtype=object)
    X = np.ascontiguousarray(x[:, ::-1, :].transpose(1, 0, 2)).reshape(n, rl * rr)
    Xi, e = exact_ints(X)
    S = T @ Xi                                                   # n x (rl rr) Python integers, times 2^(e - shift)
    out = np.zeros((n, rl * rr))
    for k in range(n):
        num_scale = 2 if k else 1                                # 2 / n, halved at k = 0
        for f in range(rl * rr):
            num, den = int(S[k, f]) * num_scale, n << shift
            if e >= 0:
                num <<= e
            else:
                den <<= -e
            out[k, f] = num / den
    return out.reshape(n, rl, rr).transpose(1, 0, 2).copy()


def write(path, out):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(out[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    if "--search" in sys.argv[1:]:
        return search()
    import oracle
    t0 = time.time()
    out = {}
    for (m, c, fam, cap) in CS.CASES:
        key = CS.key(m, c, fam)
        C, draw = CS.matrix(m, c, fam, cap)
        out[key + "_sum"], out[key + "_sumsq"] = (np.float64(v) for v in CS.checksum(draw))
        out[key + "_csum"] = np.array(CS.checksum(C.ravel()))
        sigma, rank, U = reference(m, c, fam, cap)
        assert gaps_ok(sigma, fam, cap), f"{key}: a singular value next to a cut; run --search and update SEEDS"
        out[key + "_sigma"], out[key + "_rank"] = sigma, np.int32(rank)
        if fam == "zero":
            piv, margin, ontol, dev = np.zeros(1, dtype=np.int64), np.inf, True, 0.0
        else:
            piv, tr = CS.maxvol_restated(U)
            margin, ontol = tr.margin, (tr.stopped_on_tol or m <= rank)
            dev = 0.0
            if m <= CS.U_TOP_MAX_M:
                out[key + "_utop"] = U
                degenerate_cut = fam == "equal_sigma" and rank < len(sigma) and sigma[rank - 1] == sigma[rank]
                if not degenerate_cut:
                    # at the oracle's own pivots: they are the restatement's, except among the exactly tied rows of
                    # equal_sigma, where the choice is LAPACK's
                    want_chat, want_piv, want_rank = oracle._cross_step(C, cap)
                    assert want_rank == rank, (key, want_rank, rank)
                    assert fam == "equal_sigma" or np.array_equal(want_piv[:rank], piv), (key, want_piv, piv)
                    dev = float(np.max(np.abs(want_chat.astype(CS.LD) - CS.chat_longdouble(U, want_piv[:rank]))))
            assert m <= rank or fam == "equal_sigma" or margin >= margin_floor(dev), f"{key}: decision margin {margin:.1e} with oracle_dev {dev:.1e}"
        out[key + "_piv"], out[key + "_margin"] = np.asarray(piv, dtype=np.int64), np.float64(margin)
        out[key + "_ontol"], out[key + "_dev"] = np.bool_(ontol), np.float64(dev)
        print(f"  {key:>20}: rank {rank:2d}  sigma_0/sigma_rank {sigma[0] / sigma[rank - 1] if sigma[0] > 0 else 1:.1e}"
              f"  margin {margin:.1e}  oracle_dev {dev:.1e}  on tol {ontol}  ({time.time() - t0:.0f} s)", flush=True)
    # the maxvol cases that need no fixture entry, only their conditions
    m, r, seed = CS.SWAP_CASE
    assert swap_case_ok(m, r, seed), "SWAP_CASE needs three swaps at tol = 1 that notice a wrong update; run --search"
    worst = 0.0
    for n in CS.DCT_N:
        for (rl, rr) in CS.DCT_RANKS:
            x = CS.dct_input(n, rl, rr)
            ref = out[CS.dct_key(n, rl, rr)] = dct_exact(x)
            worst = max(worst, float(np.max(np.abs(CS.dct_restated(x) - ref) / CS.dct_bound(x))))
    print(f"  DCT: the NumPy restatement is within {worst:.3f} of the bound")
    path = os.path.join(HERE, "g31_cross_steps.npz")
    write(path, out)
    print(f"  wrote g31_cross_steps.npz ({os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays) in {time.time() - t0:.1f} s")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
