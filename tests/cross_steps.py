"""Shared by the tests of the TT-Cross dense steps (csrc/ttcross_kernels.h): the case table, the seeded matrix
families, and NumPy restatements of the kernels' own algorithms -- the greedy maxvol of maxvol_device with the
decision margins it met, and the one-sided Jacobi loop of k_cross_step with and without its power-of-two prescaling.
NumPy only; nothing here needs a GPU.

Every family is C = Q diag(sigma) Z^T with Q (m x k) and Z (c x k) the orthonormal factors of seeded Gaussian draws,
k = min(m, c), and a prescribed spectrum:

  flat         sigma = 1 ... 0.05, equally spaced
  graded       10^-(11 j / (k - 2)), j = 0 .. k - 2, i.e. 1 down to 1e-11, and a last value 1e-13 below the 1e-12 cut
  capcut       2^-j, and a further factor 1/2 from position `cap` on: the rank is cut by `cap`, with a ratio 4 at the cut
  zerocols     flat in c - 3 columns, and columns 0, c // 2 and c - 1 exactly zero
  dupcols      flat in c - 1 columns, and column c - 1 a bitwise copy of column 1
  equal_sigma  H_m[:, :c] diag(s), H_m the Sylvester Hadamard matrix and s powers of two out of order, several of them
               repeated: the columns are exactly orthogonal, the singular values s_j sqrt(m) exact and exactly equal
               where s repeats
  zero         all zeros

A case is (m, c, family, cap); its key is "<m>x<c>_<family>".  The seeds come from
tests/golden/generate_golden_cross_steps.py --search, which looks for draws that meet the input conditions below.
"""
import functools
import math

import numpy as np

LD = np.longdouble
EPS = 2.220446049250313e-16
MAX_R = 64                      # TTX_MAX_R
MAX_M = 8192                    # TTX_MAX_M
LANES = 64                      # TTX_THREADS: row i (phase 1) and flat index f (phase 2) live on lane i % 64, f % 64
JACOBI_SWEEPS = 60
REL_THRESH = 1e-12
MAXVOL_TOL = 1.05
MAXVOL_ITERS = 100
U_TOP_MAX_M = 256               # above this the fixture holds no singular vectors

# ---------------------------------------------------------------------------------------------- input conditions
MARGIN_MIN = 1e-6               # every non-tie decision of maxvol_restated is at least this far from flipping ...
MARGIN_OVER_DEV = 100.0         # ... and at least this many times the LAPACK subspace's own deviation (oracle_dev):
#                                 a perturbation of U of size delta moves a squared residual norm or an entry of B by
#                                 O(delta) relative to the winner, so a decision with a margin of 100 delta cannot flip
CUT_GAP = 2.0                   # no singular value within this factor of REL_THRESH * sigma_0
CAP_GAP = 2.0                   # capcut: sigma_cap / sigma_(cap + 1) at least this

# ---------------------------------------------------------------------------------------------- the case table
# (m, c, family, cap).  m on both sides of the lane stride (63 .. 65, 127 .. 129), c = 1, 2, 8, 63, 64, m < c,
# m = rank + 1 (the smallest maxvol), m = c = rank, the host limits 8192 rows and 64 columns.
CASES = [
    (1, 1, "flat", 1), (2, 1, "flat", 1), (1, 2, "flat", 2), (2, 2, "flat", 2),
    (129, 1, "flat", 1), (65, 2, "flat", 2), (64, 2, "flat", 1),
    (63, 8, "flat", 8), (64, 8, "flat", 8), (127, 8, "flat", 8), (128, 8, "flat", 8), (129, 8, "flat", 8),
    (9, 8, "flat", 8), (8, 8, "flat", 8), (4, 8, "flat", 8), (40, 64, "flat", 64),
    (65, 64, "flat", 64), (129, 63, "flat", 63), (64, 63, "flat", 20),
    (704, 64, "flat", 64), (8192, 8, "flat", 8),
    (65, 8, "graded", 8), (127, 8, "graded", 8), (128, 8, "graded", 5),
    (129, 24, "capcut", 10), (64, 8, "capcut", 3), (63, 16, "capcut", 5),
    (65, 8, "zerocols", 8), (128, 16, "zerocols", 16),
    (65, 8, "dupcols", 8), (127, 8, "dupcols", 8),
    (64, 8, "equal_sigma", 8), (128, 16, "equal_sigma", 5),
    (12, 3, "zero", 3), (65, 8, "zero", 8),
]
UNSUPPORTED = [(8193, 8), (8, 65)]
SCALE_CASES = [(65, 8, "graded", 8), (129, 24, "capcut", 10), (9, 8, "flat", 8)]
SCALE_EXPONENTS = (-900, -520, -250, 0, 250, 520, 900)

# chosen by generate_golden_cross_steps.py --search; cases not listed use seed 0
SEEDS = {
    "65x64_flat": 1,
}

_FAMILY_ID = {"flat": 1, "graded": 2, "capcut": 3, "zerocols": 4, "dupcols": 5, "equal_sigma": 6, "zero": 7}


def key(m, c, family):
    return f"{m}x{c}_{family}"


def case_ids():
    return [key(m, c, f) for (m, c, f, _) in CASES]


def sylvester(n):
    assert n >= 1 and n & (n - 1) == 0, n
    H = np.ones((1, 1))
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    return H


def equal_sigma_scales(c):
    """Powers of two 2^-((3 j) mod 7), out of order and repeating with period 7, and s_5 = s_2."""
    s = 2.0 ** -((3 * np.arange(c)) % 7).astype(float)
    s[5] = s[2]
    return s


def spectrum(family, k, cap):
    if family == "flat":
        return np.linspace(1.0, 0.05, k) if k > 1 else np.ones(1)
    if family == "graded":
        assert k >= 3
        return np.concatenate([10.0 ** (-11.0 * np.arange(k - 1) / (k - 2)), [1e-13]])
    if family == "capcut":
        assert cap < k
        return 2.0 ** -(np.arange(k) + (np.arange(k) >= cap)).astype(float)
    raise ValueError(family)


def _orthonormal(G):
    """Modified Gram-Schmidt, twice, with elementwise operations and exactly rounded sums (math.fsum) only: no BLAS or
    LAPACK call, so the matrix a seed stands for is the same on every machine, to the bit."""
    Q = np.array(G, dtype=np.float64)
    for j in range(Q.shape[1]):
        v = Q[:, j].copy()
        for _ in range(2):
            for i in range(j):
                v = v - math.fsum(Q[:, i] * v) * Q[:, i]
        Q[:, j] = v / math.sqrt(math.fsum(v * v))
    return Q


@functools.lru_cache(maxsize=None)
def matrix(m, c, family, cap, seed=None):
    """(C, draw): the read-only m x c FP64 matrix and the Gaussian draws behind it (one row), for the checksum."""
    if seed is None:
        seed = SEEDS.get(key(m, c, family), 0)
    rng = np.random.default_rng([31, _FAMILY_ID[family], m, c, seed])
    draw = np.zeros(0)
    if family == "zero":
        C = np.zeros((m, c))
    elif family == "equal_sigma":
        assert c >= 6
        C = sylvester(m)[:, :c] * equal_sigma_scales(c)
    else:
        cols = {"zerocols": c - 3, "dupcols": c - 1}.get(family, c)
        k = min(m, cols)
        gq, gz = rng.standard_normal((m, k)), rng.standard_normal((cols, k))
        draw = np.concatenate([gq.ravel(), gz.ravel()])
        sigma = spectrum("flat" if family in ("zerocols", "dupcols") else family, k, cap)
        Q, Z = _orthonormal(gq), _orthonormal(gz)
        D = np.zeros((m, cols))
        for j in range(k):                                        # in this order, one rounding per operation
            D = D + (Q[:, j] * sigma[j])[:, None] * Z[:, j][None, :]
        if family == "zerocols":
            C = np.zeros((m, c))
            C[:, [j for j in range(c) if j not in (0, c // 2, c - 1)]] = D
        elif family == "dupcols":
            C = np.concatenate([D, D[:, 1:2]], axis=1)
        else:
            C = D
    C = np.ascontiguousarray(C)
    C.setflags(write=False)
    return C, draw


def checksum(draw):
    """(sum, sum of squares) of the values, each exactly rounded (math.fsum): the same on every machine."""
    d = np.asarray(draw, dtype=np.float64).ravel()
    return math.fsum(d), math.fsum(d * d)


def expected_rank(sigma, m, c, cap):
    """The reference's rule (oracle._cross_step): #{sigma > 1e-12 sigma_0}, capped by cap, m and c; 1 for a zero matrix."""
    sigma = np.asarray(sigma, dtype=float)
    eff = int(np.sum(sigma > REL_THRESH * sigma[0])) if sigma[0] > 0.0 else 1
    return max(1, min(cap, eff, m, c))


# ---------------------------------------------------------------------------------------------- maxvol, restated
def _first_argmax(v):
    """(index, value, runner, tie): np.argmax (first index), the largest value not bitwise equal to the winner's
    (-inf without one), and whether another candidate equals the winner bitwise."""
    i = int(np.argmax(v))
    best = v[i]
    tie = bool(np.count_nonzero(v == best) > 1)
    rest = v[v != best]
    return i, float(best), (float(rest.max()) if rest.size else -np.inf), tie


class MaxvolTrace:
    """What maxvol_restated met: `margin`, the smallest relative distance of a decision from flipping -- (winner -
    runner-up) / winner at every arg-max, |best - tol| / tol at every stop test -- with bitwise-equal candidates
    counted as ties and not as margins; `tie_rows1`, the rows that won a phase-1 arg-max on an exact tie, and
    `tie_rows2`, the rows swapped in by phase 2 on one; `phase1`, the pivots before phase 2; `swaps`;
    `stopped_on_tol`."""

    def __init__(self):
        self.margin, self.tie_rows1, self.tie_rows2, self.swaps, self.stopped_on_tol = np.inf, [], [], 0, False
        self.phase1 = None

    def _argmax(self, v, stop_at=None):
        """`stop_at`: the winner's index matters only if its value exceeds it (phase 2: at the last stop test the
        pivot rows' own entries 1 +- ulp compete, and nothing is done with the winner)."""
        i, best, runner, tie = _first_argmax(v)
        if stop_at is not None:
            self.margin = min(self.margin, abs(best - stop_at) / stop_at)
        if best > 0.0 and np.isfinite(runner) and (stop_at is None or best > stop_at):
            self.margin = min(self.margin, (best - runner) / best)
        return i, best, tie


def maxvol_restated(A, tol=MAXVOL_TOL, max_iters=MAXVOL_ITERS, wrong_update=False):
    """maxvol_device in NumPy FP64 for an m x r matrix: (pivots, MaxvolTrace).

    Phase 1 picks, r times, the row with the largest squared residual norm, projects it out of every row and zeroes
    it.  Phase 2 forms B = A inv(A[pivots]) and, while the largest |B| exceeds tol, swaps that row in with a rank-1
    update.  Both arg-max take the first index (np.argmax; in phase 2 the first flat index of the row-major B).  Every
    row is treated by elementwise operations over the columns, so bitwise-equal rows stay bitwise equal, as they do in
    the kernel.  m <= r returns arange(m), like pcx_maxvol.  `wrong_update` leaves the division by the pivot out of the
    new column j (a mistake the pivots of most matrices do not show): the generator uses it to choose a swap case whose
    pivots do."""
    A = np.array(A, dtype=np.float64)
    m, r = A.shape
    tr = MaxvolTrace()
    if m <= r:
        return np.arange(m, dtype=np.intp), tr
    work = A.copy()
    idx = np.zeros(r, dtype=np.intp)
    for k in range(r):
        s = np.zeros(m)
        for j in range(r):
            s += work[:, j] * work[:, j]
        bi, best, tie = tr._argmax(s)
        if tie:
            tr.tie_rows1.append(bi)
        idx[k] = bi
        nrm = np.sqrt(best)
        q = work[bi] / nrm if nrm > 0.0 else np.zeros(r)
        dot = np.zeros(m)
        for j in range(r):
            dot += work[:, j] * q[j]
        for j in range(r):
            work[:, j] -= dot * q[j]
        work[bi] = 0.0
    tr.phase1 = idx.copy()
    try:
        inv = np.linalg.inv(A[idx])
    except np.linalg.LinAlgError:
        return idx, tr
    B = np.zeros((m, r))
    for k in range(r):
        B += A[:, k:k + 1] * inv[k:k + 1, :]
    for _ in range(max_iters):
        f, best, tie = tr._argmax(np.abs(B).ravel(), tol)
        if not best > tol:
            tr.stopped_on_tol = True
            break
        i, j = divmod(f, r)
        if tie:
            tr.tie_rows2.append(i)
        idx[j] = i
        bij = B[i, j]
        row = B[i].copy()
        cj = B[:, j].copy()
        B -= cj[:, None] * row[None, :] / bij
        B[:, j] = cj if wrong_update else cj / bij
        tr.swaps += 1
    return idx, tr


# ---------------------------------------------------------------------------------------------- C_hat in longdouble
def chat_longdouble(U, piv):
    """U inv(U[piv]) with every operation in np.longdouble (Gauss-Jordan with partial pivoting on the transposed
    system), returned in longdouble."""
    U = np.asarray(U).astype(LD)
    r = U.shape[1]
    # solve X P = U for X, P = U[piv]:  P^T X^T = U^T
    M = np.concatenate([U[np.asarray(piv)].T, U.T], axis=1)          # r x (r + m)
    for k in range(r):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
        M[k] = M[k] / M[k, k]
        f = M[:, k].copy()
        f[k] = 0
        M -= f[:, None] * M[k][None, :]
    return M[:, r:].T


# ---------------------------------------------------------------------------------------------- the Jacobi loop, restated
def jacobi_restated(C, prescale):
    """The one-sided Jacobi loop of k_cross_step in NumPy FP64: cyclic pairs (p, q), the stop test
    |ga| <= 1e-15 sqrt(al be), at most 60 sweeps.  `prescale` multiplies by the power of two that brings max|C| into
    [1, 2) first, as the kernel does; without it this is the kernel before the prescaling.  Returns (W, sweeps)."""
    W = np.array(C, dtype=np.float64)
    m, c = W.shape
    if prescale:
        mx = float(np.max(np.abs(W)))
        if mx > 0.0:
            W = np.ldexp(W, 1 - int(np.frexp(mx)[1]))
    sweeps = 0
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        for _ in range(JACOBI_SWEEPS):
            rotated = False
            for p in range(c - 1):
                for q in range(p + 1, c):
                    wp, wq = W[:, p].copy(), W[:, q].copy()
                    al, be, ga = float(wp @ wp), float(wq @ wq), float(wp @ wq)
                    if al == 0.0 or be == 0.0:
                        continue
                    if abs(ga) <= 1e-15 * np.sqrt(np.float64(al) * np.float64(be)):
                        continue
                    rotated = True
                    zeta = (np.float64(be) - al) / (2.0 * np.float64(ga))
                    t = (1.0 if zeta >= 0.0 else -1.0) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                    cs = 1.0 / np.sqrt(1.0 + t * t)
                    sn = cs * t
                    W[:, p], W[:, q] = cs * wp - sn * wq, sn * wp + cs * wq
            sweeps += 1
            if not rotated:
                break
    return W, sweeps


def cross_step_restated(C, cap, rel_thresh=REL_THRESH, prescale=True):
    """k_cross_step in NumPy: (C_hat, pivots, rank, sweeps).  Column norms, the stable descending order, the rank rule,
    maxvol_restated, C_hat = U inv(U[pivots])."""
    W, sweeps = jacobi_restated(C, prescale)
    m, c = W.shape
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        s = np.sqrt(np.einsum("ij,ij->j", W, W))
        order = np.argsort(-s, kind="stable")
        s0 = float(np.max(s))
        eff = int(np.sum(s > rel_thresh * s0)) if s0 > 0.0 else 1
        rank = max(1, min(eff, cap, m, c))
        U = np.zeros((m, rank))
        for k in range(rank):
            if s[order[k]] > 0.0:
                U[:, k] = W[:, order[k]] / s[order[k]]
    piv = maxvol_restated(U)[0] if m > rank else np.arange(rank, dtype=np.intp)
    try:
        chat = U @ np.linalg.inv(U[piv])
    except np.linalg.LinAlgError:
        chat = U
    return chat, piv, rank, sweeps


# ---------------------------------------------------------------------------------------------- maxvol tie and swap cases
TIE_DISTANCES = (1, 63, 64, 65, 128)
TIE_M, TIE_R = 200, 4
# chosen by the generator's --search: (seed, first index) per (distance, negated, phase) such that row `first` of the
# pair wins an arg-max of that phase of the restatement on an exact tie with its copy -- in phase 2 one that swaps
TIE_SEEDS = {
    (1, False, 1): (0, 23),
    (1, False, 2): (1638, 53),
    (1, True, 1): (0, 23),
    (1, True, 2): (327, 0),
    (63, False, 1): (0, 16),
    (63, False, 2): (809, 114),
    (63, True, 1): (0, 16),
    (63, True, 2): (8280, 103),
    (64, False, 1): (1, 119),
    (64, False, 2): (11860, 65),
    (64, True, 1): (0, 16),
    (64, True, 2): (1051, 86),
    (65, False, 1): (0, 16),
    (65, False, 2): (21241, 29),
    (65, True, 1): (0, 16),
    (65, True, 2): (556, 97),
    (128, False, 1): (2, 24),
    (128, False, 2): (2395, 51),
    (128, True, 1): (0, 8),
    (128, True, 2): (1460, 41),
}
SWAP_CASE = (60, 5, 111)          # (m, r, seed): maxvol_restated(tol = 1.0) needs at least 3 swaps, and its
#                                 third depends on the update of the second being right; set by --search


def tie_matrix(distance, negated, seed, first, phase):
    """Integer-valued TIE_M x TIE_R matrix, entries -20 .. 20, whose row first + distance is a copy of row `first`
    (negated: its negative, so that |B| ties with opposite signs).  For phase 1 the pair is doubled, so that it
    competes for the first arg-max; for phase 2 it is left to be swapped in."""
    rng = np.random.default_rng([31, 100, distance, int(negated), seed, phase])
    A = rng.integers(-20, 21, (TIE_M, TIE_R)).astype(float)
    if phase == 1:
        A[first] = 2.0 * A[first]
    A[first + distance] = -A[first] if negated else A[first]
    return A


def swap_matrix(m, r, seed):
    rng = np.random.default_rng([31, 101, m, r, seed])
    return rng.standard_normal((m, r))


# ---------------------------------------------------------------------------------------------- the DCT
DCT_N = (1, 2, 3, 16, 17, 33, 63, 64)
DCT_RANKS = ((1, 1), (3, 5), (16, 16), (64, 1), (1, 64))


def dct_key(n, rl, rr):
    return f"dct_{rl}x{n}x{rr}"


@functools.lru_cache(maxsize=None)
def dct_input(n, rl, rr):
    """Value core (rl, n, rr) whose entries span six decades, both signs."""
    rng = np.random.default_rng([31, 200, n, rl, rr])
    x = rng.choice([-1.0, 1.0], (rl, n, rr)) * 10.0 ** rng.uniform(-3.0, 3.0, (rl, n, rr))
    x.setflags(write=False)
    return x


def dct_restated(x):
    """k_value_to_coeff_core in NumPy FP64."""
    x = np.asarray(x, dtype=float)
    n = x.shape[1]
    k, j = np.arange(n)[:, None], np.arange(n)[None, :]
    T = np.cos(np.pi * k * (2 * j + 1) / (2 * n))
    out = 2.0 * np.einsum("kj,ijc->ikc", T, x[:, ::-1, :]) / n
    out[:, 0, :] *= 0.5
    return out


def dct_bound(x):
    """Per output (i, k, cc): (3 pi max(k, 1) + n + 4) eps (2 / n) sum_j |x_j|.  The cosine's argument pi k (2j + 1) / (2n)
    carries three roundings (pi, the product, the quotient) of relative size eps each, at an argument below pi k: the
    cosine moves by at most 3 pi k eps; the cosine's own rounding, the n products and sums, the factor 2 / n and the
    halving are the n + 4."""
    x = np.asarray(x, dtype=float)
    n = x.shape[1]
    k = np.maximum(np.arange(n), 1)
    return ((3.0 * np.pi * k + n + 4.0) * EPS * 2.0 / n)[None, :, None] * np.sum(np.abs(x), axis=1)[:, None, :]
