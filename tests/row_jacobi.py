"""Shared by the row-Jacobi tests: the dispatch of rowjacobi_factor (csrc/pcx_ttbuild.hip) restated, a plain NumPy
restatement of the iteration of csrc/ttsvd_kernels.h, the figures a factorisation C = U B is judged by, the exact
matrix families and the call of one device factorisation through the C ABI.  Only device_factor needs a GPU.

Every family is built from np.random.default_rng(seed).integers(-64, 65, ...), so its entries, its exact dependencies
and its power-of-two scalings are exact in FP64 on any machine:

  gauss     the integers as they are
  lowrank   (m x r integers) (r x N integers), r = ceil(min(m, N) / 3): exact dependencies, rows rotate into zeros
  dup       row 1 = row 0, last row = -2 row 2, row m // 2 all zero (m >= 6)
  graded    row i times 2^-round(40 i / (m - 1)), the row order shuffled: 12 decades of singular values (m >= 2)
  hadamard  H_m[:, :r] diag(2^-3i) H_N[:r, :] with Sylvester Hadamard matrices, r = min(m, N, 14): the singular values
            are exactly 2^-3i sqrt(m N); power-of-two shapes only, seed unused
  zero      all zeros
"""
import ctypes
import functools

import numpy as np

LD = np.longdouble
EPS = 2.220446049250313e-16
MAX_SWEEPS = 60                     # the cap of every sweep loop of rowjacobi_factor

# ---------------------------------------------------------------------------------------------- the dispatch
# Mirrors the constants of rowjacobi_factor: the row image limit `lds_rows <= 144 * 1024`, the limit with U
# `lds_rows + m * m * sizeof(double) <= 156 * 1024`, TTSVD_LDS_THREADS / 16 = 64 pairs per round of k_rowjacobi_lds,
# the Gram condition `N > 2L * m && lds_sym <= 156 * 1024` with lds_sym as computed there, and `mp - 1 <= 16` for the
# plain launches.
LDS_ROWS_BYTES = 144 * 1024
LDS_ALL_BYTES = 156 * 1024
LDS_PAIRS_PER_ROUND = 64
PLAIN_MAX_STEPS = 16
PATHS = ("none", "lds_u", "lds_hbm", "lds_second", "gram_plain", "gram_graph", "nogram")
GRAM_PATHS = ("gram_plain", "gram_graph")


def u_in_lds(m, N):
    return 8 * m * N + 8 * m * m <= LDS_ALL_BYTES


def path_of(m, N):
    """The path rowjacobi_factor takes for an m x N matrix, one of PATHS."""
    mp = (m + 1) & ~1
    if m == 1:
        return "none"
    if 8 * m * N <= LDS_ROWS_BYTES:
        if mp // 2 > LDS_PAIRS_PER_ROUND:
            return "lds_second"
        return "lds_u" if u_in_lds(m, N) else "lds_hbm"
    lds_sym = (2 * m * m + 2 * ((m + 1) // 2 + 1)) * 8 + (m + 2) * 4
    if N > 2 * m and lds_sym <= LDS_ALL_BYTES:
        return "gram_plain" if mp - 1 <= PLAIN_MAX_STEPS else "gram_graph"
    return "nogram"


# the smallest shapes at which each path and each of its edges exists, under the path they are meant to reach
SHAPES = {
    "none": [(1, 50)],
    "lds_u": [(2, 3), (6, 140), (88, 11), (40, 30), (15, 300), (127, 20), (40, 459)],
    "lds_hbm": [(40, 460), (96, 192)],
    "lds_second": [(130, 20), (129, 140)],
    "gram_plain": [(2, 9217), (3, 6145), (15, 1300), (16, 1153)],
    "gram_graph": [(96, 193), (17, 1085), (99, 199)],
    "nogram": [(99, 198), (100, 201), (140, 140), (200, 100), (201, 95)],
}
HADAMARD_SHAPES = {"lds_u": (32, 64), "gram_plain": (16, 2048), "gram_graph": (64, 512), "nogram": (128, 256)}
ALL_SHAPES = [s for p in PATHS for s in SHAPES[p]]
RANK_SHAPES = [(6, 140), (40, 460), (16, 1153), (17, 1085), (64, 512)]       # graded
RANK_TOLS = (1e-6, 1e-10, 1e-12)

# graded seeds: chosen by generate_golden_row_jacobi.py so that no singular value sits next to a cut tol * sigma_0
GRADED_SEED = {(6, 140): 0, (40, 460): 0, (16, 1153): 0, (17, 1085): 0, (64, 512): 0}


# The factor by which every singular value of a rank-rule case stays away from each cut tol * sigma_0.  A factor 2 cannot
# be had: the last row of every graded matrix is scaled by 2^-40 = 9.1e-13, so its singular value is 0.87 .. 0.95 of the
# cut 1e-12 sigma_0 whatever the seed (the row norms of a wide integer draw differ by a few per cent only), and at 40
# and 64 rows consecutive scalings are a factor 2 or less apart.  What the rank needs is the absolute accuracy of
# figure (d), 1e-14 sigma_0: 1 % of the lowest cut.  The gap is five times that.
RANK_GAP = 1.05


def families_of(m, N):
    fams = ["gauss", "lowrank", "zero"]
    if m >= 6:
        fams.append("dup")
    if m >= 2:
        fams.append("graded")
    return fams


def cases():
    """Every (m, N, family) of the fixture, in a fixed order."""
    out = [(m, N, f) for (m, N) in ALL_SHAPES for f in families_of(m, N)]
    out += [(m, N, "hadamard") for (m, N) in HADAMARD_SHAPES.values()]
    out += [(m, N, "graded") for (m, N) in RANK_SHAPES if (m, N) not in ALL_SHAPES]
    out.append((96, 150, "gauss"))                    # the base of the appended-zero-rows relation
    return out


def key(m, N, family):
    return f"{m}x{N}_{family}"


# ---------------------------------------------------------------------------------------------- the families
_FAMILY_ID = {"gauss": 1, "lowrank": 2, "dup": 3, "graded": 4, "hadamard": 5, "zero": 6}


def sylvester(n):
    assert n >= 1 and n & (n - 1) == 0, n
    H = np.ones((1, 1), dtype=np.int64)
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    return H


def hadamard_rank(m, N):
    return min(m, N, 14)


def hadamard_sigma(m, N):
    """The exact singular values 2^-3i sqrt(m N), in extended precision."""
    r = hadamard_rank(m, N)
    return np.sqrt(LD(m * N)) * LD(2.0) ** (-3 * np.arange(r, dtype=LD))


@functools.lru_cache(maxsize=None)
def matrix(family, m, N):
    """(C, draw): the read-only m x N FP64 matrix and every integer drawn for it (int64, one row), for the checksum."""
    seed = GRADED_SEED.get((m, N), 0) if family == "graded" else 0
    rng = np.random.default_rng([30, _FAMILY_ID[family], m, N, seed])
    draw = np.zeros(0, dtype=np.int64)
    if family == "zero":
        C = np.zeros((m, N))
    elif family == "hadamard":
        r = hadamard_rank(m, N)
        C = (sylvester(m)[:, :r] * 2.0 ** (-3 * np.arange(r))) @ sylvester(N)[:r, :].astype(float)
    elif family == "lowrank":
        r = -(-min(m, N) // 3)
        A, B = rng.integers(-64, 65, (m, r)), rng.integers(-64, 65, (r, N))
        draw = np.concatenate([A.ravel(), B.ravel()])
        C = (A @ B).astype(float)
    else:
        G = rng.integers(-64, 65, (m, N))
        draw = G.ravel()
        C = G.astype(float)
        if family == "dup":
            assert m >= 6
            C[1] = C[0]
            C[m - 1] = -2.0 * C[2]
            C[m // 2] = 0.0
        elif family == "graded":
            assert m >= 2
            k = (80 * np.arange(m) + (m - 1)) // (2 * (m - 1))          # round(40 i / (m - 1)), halves up
            perm = rng.permutation(m)
            draw = np.concatenate([draw, perm])
            C = (C * 2.0 ** -k[:, None].astype(float))[perm]
    C.setflags(write=False)
    return C, draw.astype(np.int64)


def checksum(draw):
    """(sum, sum of squares) of the draw as exact Python integers."""
    return int(np.sum(draw, dtype=np.int64)), int(np.sum(draw * draw, dtype=np.int64))


# ---------------------------------------------------------------------------------------------- the restatement
def rot_tol(N):
    return max(1e-15, 2.0 * EPS * np.sqrt(float(N)))


def restatement(C, tol=0.0, trace=None):
    """k_rowjacobi_step sweep by sweep in NumPy FP64 from U = I: the same tournament order, floor2, rot_tol and sig2,
    the same rotation formula and stop rule (a sweep without a pair further than 1e-8 from orthogonal is the last), no
    Gram preconditioner.  Returns (U (m x m), B (m x N), sweeps) with U B = C.  `trace(sweep, U, B)` is called after
    every sweep."""
    B = np.array(C, dtype=np.float64)
    m, N = B.shape
    U = np.eye(m)
    if m == 1:
        return U, B, 0
    hn = np.einsum("ij,ij->i", B, B)
    fro2 = float(hn.sum())
    floor2 = (8.0 * EPS) ** 2 * fro2
    sig2 = tol * tol * float(hn.max()) / m
    rt2 = rot_tol(N) ** 2
    mp = (m + 1) & ~1
    i = np.arange(mp // 2)
    sweeps = 0
    for _ in range(MAX_SWEEPS):
        large = 0
        for step in range(mp - 1):
            p = np.where(i == 0, mp - 1, (step + i) % (mp - 1))
            q = np.where(i == 0, step % (mp - 1), (step - i + 2 * (mp - 1)) % (mp - 1))
            ok = (p < m) & (q < m)                                          # the bye of an odd field
            lo, hi = np.minimum(p, q)[ok], np.maximum(p, q)[ok]
            a, b = B[lo], B[hi]
            aa, bb, ab = (np.einsum("ij,ij->i", x, y) for x, y in ((a, a), (b, b), (a, b)))
            rot = (aa > floor2) & (bb > floor2) & ~(aa + bb < sig2) & (ab * ab > rt2 * aa * bb)
            if not rot.any():
                continue
            lo, hi, a, b, aa, bb, ab = (v[rot] for v in (lo, hi, a, b, aa, bb, ab))
            large += int(np.sum(ab * ab > 1e-16 * aa * bb))
            zeta = (bb - aa) / (2.0 * ab)
            t = np.copysign(1.0, zeta) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
            c = 1.0 / np.sqrt(1.0 + t * t)
            s = c * t
            B[lo], B[hi] = c[:, None] * a - s[:, None] * b, s[:, None] * a + c[:, None] * b
            x, y = U[:, lo], U[:, hi]
            U[:, lo], U[:, hi] = c * x - s * y, s * x + c * y
        sweeps += 1
        if trace is not None:
            trace(sweeps, U, B)
        if large == 0:
            break
    return U, B, sweeps


def select(U, B, max_rank=None, tol=0.0):
    """What pcx_tt_svd keeps of a factorisation: rows by descending norm (stable), the reference's rank rule."""
    m, N = B.shape
    hn = np.einsum("ij,ij->i", B, B)
    order = np.argsort(-hn, kind="stable")
    len_s = min(m, N)
    rank = min(len_s if max_rank is None else int(max_rank), len_s)
    s = np.sqrt(hn[order])
    rank = max(1, min(rank, int(np.sum(s[:len_s] > tol * s[0])))) if s[0] > 0.0 else 1
    return U[:, order[:rank]], B[order[:rank]]


# ---------------------------------------------------------------------------------------------- the figures
def sigma_of(B, count):
    """Row norms of B (taken in extended precision), descending, padded with zeros to `count` values."""
    Bl = np.asarray(B).astype(LD)
    s = np.sort(np.sqrt(np.einsum("ij,ij->i", Bl, Bl)))[::-1]
    out = np.zeros(count, dtype=LD)
    out[:min(count, s.size)] = s[:count]
    return out


def figures(C, U, B, sref=None):
    """(a) max|U B - C| / ||C||_F, (b) max|U^T U - I|, (c) the largest cosine between two rows of B above
    32 eps ||C||_F, (d) max|sigma_i - sref_i| / sref_0 over the leading min(m, N) values, sigma = the row norms of B
    sorted descending; every product in np.longdouble.  sref defaults to np.linalg.svd(C).  A zero C gives zeros."""
    C = np.asarray(C)
    m, N = C.shape
    Cl, Ul, Bl = C.astype(LD), np.asarray(U).astype(LD), np.asarray(B).astype(LD)
    fro = float(np.sqrt(np.sum(Cl * Cl)))
    if fro == 0.0:
        return {"a": float(np.max(np.abs(Ul @ Bl))), "b": float(np.max(np.abs(Ul.T @ Ul - np.eye(Ul.shape[1])))),
                "c": 0.0, "d": float(np.max(np.abs(Bl)))}
    a = float(np.max(np.abs(Ul @ Bl - Cl))) / fro
    b = float(np.max(np.abs(Ul.T @ Ul - np.eye(Ul.shape[1], dtype=LD))))
    G = Bl @ Bl.T
    nrm = np.sqrt(np.diag(G))
    big = np.nonzero(nrm > 32.0 * EPS * fro)[0]
    c = 0.0
    if big.size > 1:
        cos = np.abs(G[np.ix_(big, big)]) / np.outer(nrm[big], nrm[big])
        np.fill_diagonal(cos, 0.0)
        c = float(cos.max())
    k = min(m, N)
    if sref is None:
        sref = np.linalg.svd(C, compute_uv=False)
    sref = np.asarray(sref).astype(LD)[:k]
    sig = sigma_of(B, k)
    want = np.zeros(k, dtype=LD)
    want[:sref.size] = sref
    d = float(np.max(np.abs(sig - want)) / want[0])
    return {"a": a, "b": b, "c": c, "d": d}


def relative_figure(B, sref, m):
    """max|sigma_i / sref_i - 1| over the sref_i > 64 eps sqrt(m) sref_0."""
    sref = np.asarray(sref).astype(LD)
    keep = sref > 64.0 * EPS * np.sqrt(float(m)) * sref[0]
    sig = sigma_of(B, sref.size)
    return float(np.max(np.abs(sig[keep] / sref[keep] - 1)))


# ---------------------------------------------------------------------------------------------- the device
def device_factor(C, max_rank=None, tol=0.0):
    """One rowjacobi_factor on the device: pcx_tt_svd with d = 2, n = (m, N).  Returns (U[:, order[:rank]] (m x rank),
    the kept rows of B (rank x N), the sweep count)."""
    from pychebyshev_amd import _lib
    lib = _lib.load()
    C = _lib.f64(C)
    m, N = C.shape
    r = min(m, N) if max_rank is None else int(max_rank)
    n = _lib.i32([m, N])
    cap = (m + N) * min(r, m, N)
    cores = np.full(cap, np.nan)
    ranks = np.zeros(3, dtype=np.int32)
    used, sweeps = ctypes.c_int64(0), ctypes.c_int32(-1)
    _lib.check(lib.pcx_tt_svd(_lib.default_device(), 2, _lib.p_i32(n), _lib.p_f64(C.ravel()), r, float(tol),
                              _lib.p_i32(ranks), _lib.p_f64(cores), cap, ctypes.byref(used), ctypes.byref(sweeps)), lib)
    rank = int(ranks[1])
    assert ranks[0] == 1 and ranks[2] == 1 and used.value == (m + N) * rank, (ranks, used.value)
    return cores[:m * rank].reshape(m, rank).copy(), cores[m * rank:(m + N) * rank].reshape(rank, N).copy(), int(sweeps.value)
