"""Shared by the tests of the TT completion dense steps (csrc/tt_als_kernels.h, csrc/pcx_tt_als.hip): the case tables,
the seeded generators, the dispatch of the two contractions restated from (rank, form), a NumPy restatement of
k_tta_householder in float64 and in np.longdouble, the exact references of the integer cases, and the NumPy ALS in
projection form that tests/test_gpu_tt_completion.py compares run_completion with.  NumPy only; nothing here needs a
GPU.

A contraction case is (r, K, R): left  out (r x R) = Q^T P with Q (K x r), P (K x R); right out (R x r) = P C^T with
C = Q^T (r x K) and P^T (R x K) -- the same numbers on both sides, so one reference serves both (transposed).
"""
import functools

import numpy as np

LD = np.longdouble
EPS = 2.220446049250313e-16
THREADS = 256                   # TTA_THREADS: one lane per column (row) of the large operand in the VALU forms
WAVE_COLS = 64                  # columns (rows) of the large operand one wave owns in the MFMA forms
RED_BLOCKS = 1024               # TTA_RED_BLOCKS: the grid of k_tta_norms
MAX_RANK = 256                  # TTA_MAX_RANK
MAX_NODES = 256                 # TTA_MAX_NODES
MAX_GRID = 1 << 28              # PCX_TT_ALS_MAX_GRID
MFMA_MIN = 16                   # the switch of form 0 when PCX_TT_ALS_MFMA_MIN is unset
FORM_AUTO, FORM_VALU, FORM_MFMA = 0, 1, 2

# ---------------------------------------------------------------------------------------------- contractions
RANKS = (1, 3, 4, 5, 8, 9, 12, 13, 15, 16, 17, 31, 32, 33, 48, 64, 65, 255, 256)
KS = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65)
K_LONG = 4096                   # once, in the corner
RS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000)
PIVOT_RANKS = (5, 16, 33)       # a VALU rank, one full MFMA tile, two tiles with the second block's last tile dead
INT_BOUND = 1 << 10             # |x| <= 2^10: products <= 2^20, sums of K <= 4096 of them <= 2^32


def _contraction_cases():
    cases = [(r, 5, 65) for r in RANKS]
    cases += [(r, K, 65) for r in PIVOT_RANKS for K in KS]
    cases += [(r, 5, R) for r in PIVOT_RANKS for R in RS]
    cases += [(1, 1, 1), (256, K_LONG, 257)]
    return list(dict.fromkeys(cases))


CASES = _contraction_cases()    # (r, K, R)
ROUNDING_CASES = [(r, 777, 257) for r in (5, 16, 33, 256)]
NAN_RANKS = (5, 33)


def case_id(case):
    return "r%d_K%d_R%d" % case


def dispatch(r, form, mfma_min=MFMA_MIN):
    """What left_project / right_project launch for rank r: (form_used, accumulators or tiles, gridDim.y)."""
    if form == FORM_AUTO:
        form = FORM_MFMA if r >= mfma_min else FORM_VALU
    if form == FORM_MFMA:
        return (FORM_MFMA, 1, 1) if r <= 16 else (FORM_MFMA, 2, (r + 31) // 32)
    for rc in (4, 8, 12):
        if r <= rc:
            return FORM_VALU, rc, 1
    return FORM_VALU, 16, (r + 15) // 16


def branches(r, K, R, form):
    """The names of the paths case (r, K, R) takes in the given form: the kernel, whether the rank is tiled over
    gridDim.y, how the last rank tile ends, the K % 4 tail of the MFMA k-loop, the tail of the last wave or workgroup."""
    used, width, gy = dispatch(r, form)
    kind = "valu" if used == FORM_VALU else "mfma"
    out = {f"{kind}<{width}>", f"{kind}<{width}> gridDim.y {'> 1' if gy > 1 else '= 1'}"}
    span = width if used == FORM_VALU else 16 * width
    live = r - (gy - 1) * span                                       # rows of the last block of the rank
    out.add(f"{kind} last rank block {'full' if live == span else 'ragged'}")
    if used == FORM_MFMA:
        if width == 2 and live <= 16:
            out.add("mfma<2> second tile of the last block dead")
        out.add(f"mfma K % 4 = {K % 4}")
        if K < 4:
            out.add("mfma K < 4")
        out.add(f"mfma R % 64 {'= 0' if R % WAVE_COLS == 0 else '> 0'}")
        if R < WAVE_COLS:
            out.add("mfma R < 64")
        if R % 16 and R % WAVE_COLS:
            out.add("mfma ragged 16-column tile")
        if (R + WAVE_COLS - 1) // WAVE_COLS % 4:
            out.add("mfma idle waves in the last workgroup")
    else:
        out.add(f"valu R % 256 {'= 0' if R % THREADS == 0 else '> 0'}")
    if R > THREADS:
        out.add(f"{kind} gridDim.x > 1")
    return out


# every path the table must reach in an explicit form (tests/test_als_steps_host.py recomputes them)
REQUIRED_BRANCHES = {
    "valu<4>", "valu<8>", "valu<12>", "valu<16>", "valu<16> gridDim.y = 1", "valu<16> gridDim.y > 1",
    "valu last rank block full", "valu last rank block ragged", "valu R % 256 = 0", "valu R % 256 > 0", "valu gridDim.x > 1",
    "mfma<1>", "mfma<2>", "mfma<2> gridDim.y = 1", "mfma<2> gridDim.y > 1", "mfma last rank block full",
    "mfma last rank block ragged", "mfma<2> second tile of the last block dead", "mfma K % 4 = 0", "mfma K % 4 = 1",
    "mfma K % 4 = 2", "mfma K % 4 = 3", "mfma K < 4", "mfma R % 64 = 0", "mfma R % 64 > 0", "mfma R < 64",
    "mfma ragged 16-column tile", "mfma idle waves in the last workgroup", "mfma gridDim.x > 1",
}


@functools.lru_cache(maxsize=None)
def integer_factors(r, K, R):
    """Q (K x r) and P (K x R) with integer entries in [-2^10, 2^10], the extremes included, as float64."""
    rng = np.random.default_rng([37, r, K, R])
    Q = rng.integers(-INT_BOUND, INT_BOUND + 1, (K, r))
    P = rng.integers(-INT_BOUND, INT_BOUND + 1, (K, R))
    Q[0, 0], P[-1, -1], Q[-1, -1], P[0, 0] = INT_BOUND, INT_BOUND, -INT_BOUND, -INT_BOUND
    Q, P = Q.astype(float), P.astype(float)
    Q.setflags(write=False)
    P.setflags(write=False)
    return Q, P


@functools.lru_cache(maxsize=None)
def integer_product(r, K, R):
    """Q^T P (r x R) as int64.  Every partial sum of every element, in any order, is an integer below 2^53
    (integer_bound), so the float64 product is exact whatever order the BLAS adds in; tests/test_als_steps_host.py
    checks it against int64 and Python-integer arithmetic."""
    Q, P = integer_factors(r, K, R)
    out = (Q.T @ P).astype(np.int64)
    out.setflags(write=False)
    return out


def integer_bound(r, K, R):
    """The largest magnitude any partial sum of any output can reach, in any order: sum_k |q_k| |p_k|."""
    Q, P = integer_factors(r, K, R)
    return int((np.abs(Q).astype(np.int64).T @ np.abs(P).astype(np.int64)).max())


def sides(Q, P):
    """(side, small, big) of the two entry forms on the same numbers; the right side's output is the transpose."""
    return [(0, Q, P), (1, np.ascontiguousarray(Q.T), np.ascontiguousarray(P.T))]


@functools.lru_cache(maxsize=None)
def gaussian_factors(r, K, R):
    rng = np.random.default_rng([38, r, K, R])
    Q, P = rng.standard_normal((K, r)), rng.standard_normal((K, R))
    Q.setflags(write=False)
    P.setflags(write=False)
    return Q, P


@functools.lru_cache(maxsize=None)
def gaussian_product(r, K, R):
    """(Q^T P in longdouble, the bar K eps sum_k |q_k p_k| per element).  |fl(sum) - sum| <= gamma_K sum |q_k p_k| for
    a dot product of K terms added in ANY order, with or without fused multiply-adds (Higham, Accuracy and Stability,
    section 3.1: gamma_K = K u / (1 - K u), u = eps / 2), so K eps covers every form with a factor of two to spare; the
    longdouble reference's own error, K 2^-64 of the same sum, is 2^-11 of the bar."""
    Q, P = gaussian_factors(r, K, R)
    ref = Q.astype(LD).T @ P.astype(LD)
    bar = K * EPS * (np.abs(Q).T @ np.abs(P))
    return ref, bar


# ---------------------------------------------------------------------------------------------- Householder QR
HH_SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (7, 8), (8, 8), (9, 8), (255, 3), (256, 16), (257, 16), (64, 64), (65, 64),
             (300, 33), (700, 65), (256, 256), (512, 256), (65536, 4)]
HH_FAMILIES = ("gaussian", "flat", "dupcol", "zerocols", "zero", "triu", "graded")
WELL_CONDITIONED = ("gaussian", "flat")
SCALE_SHAPES = [(9, 4), (257, 16), (65, 64)]
SCALE_EXPONENTS = (-900, -600, -300, 0, 300, 600, 900)
_FAMILY_ID = {f: i for i, f in enumerate(HH_FAMILIES)}


def _has_family(m, c, fam):
    if fam == "dupcol":
        return c >= 2                       # a column and its copy
    if fam == "zerocols":
        return c >= 4                       # three zero columns and one that is not
    return True


HH_CASES = [(m, c, fam) for (m, c) in HH_SHAPES for fam in HH_FAMILIES if _has_family(m, c, fam)]


def hh_id(case):
    return "%dx%d_%s" % case


@functools.lru_cache(maxsize=None)
def hh_matrix(m, c, fam):
    """gaussian: standard normal entries.  flat: U diag(1 .. 0.05) V^T, cond 20.  dupcol: gaussian with the last column
    a bitwise copy of column (c - 1) // 2.  zerocols: gaussian with columns 0, c // 2 and c - 1
    exactly zero.  zero: all zeros.  triu: upper triangular with every other diagonal entry negative.  graded: gaussian
    columns times 10^(-12 j / (c - 1))."""
    rng = np.random.default_rng([39, m, c, _FAMILY_ID[fam]])
    A = rng.standard_normal((m, c))
    k = min(m, c)
    if fam == "flat":
        U, _ = np.linalg.qr(A)
        V, _ = np.linalg.qr(rng.standard_normal((c, k)))
        A = (U[:, :k] * np.linspace(1.0, 0.05, k)) @ V[:, :k].T
    elif fam == "dupcol":
        A[:, c - 1] = A[:, (c - 1) // 2]
    elif fam == "zerocols":
        A[:, [0, c // 2, c - 1]] = 0.0
    elif fam == "zero":
        A[:] = 0.0
    elif fam == "triu":
        A = np.triu(A)
        d = np.arange(k)
        A[d, d] = np.where(d % 2 == 0, -1.0, 1.0) * (0.5 + np.abs(A[d, d]))
    elif fam == "graded":
        A = A * 10.0 ** (-12.0 * np.arange(c) / max(c - 1, 1))
    A = np.ascontiguousarray(A)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def scale_matrix(m, c):
    """Gaussian entries with magnitudes clipped into [2^-4, 2^4]: times 2^e, |e| <= 900, nothing is subnormal or infinite."""
    rng = np.random.default_rng([40, m, c])
    A = rng.standard_normal((m, c))
    A = np.copysign(np.clip(np.abs(A), 2.0 ** -4, 2.0 ** 4), A)
    A.setflags(write=False)
    return A


def _exponent(mx):
    """ilogb of the column's largest magnitude, at least -1022; 0 for a zero (or non-finite) column."""
    if not (mx > 0 and np.isfinite(mx)):
        return 0
    return max(int(np.frexp(mx)[1]) - 1, -1022)


def householder(A, dtype=np.float64):
    """k_tta_householder in NumPy at the given precision: columns in their own order, each column from the diagonal
    down times 2^-ex (ex the exponent of its largest magnitude) before it is squared, beta = -copysign(norm, alpha)
    with the power of two undone, the identity reflector (tau = 0) where the scaled squares below the diagonal sum to
    zero, v_j = 1 implied, Q formed from the reflectors last to first.  Only the order inside a sum differs from the
    kernel's.  Returns (Q (m x p), R (p x c)), p = min(m, c)."""
    A = np.array(A, dtype=dtype)
    m, c = A.shape
    p = min(m, c)
    one = dtype(1.0)
    taus = np.zeros(p, dtype=dtype)
    for j in range(p):
        ex = _exponent(np.max(np.abs(A[j:, j])))
        down = np.ldexp(one, -ex)
        sub = A[j + 1:, j] * down
        sigma = np.sum(sub * sub)
        alpha = A[j, j] * down
        if sigma != 0:
            b = -np.copysign(np.sqrt(alpha * alpha + sigma), alpha)
            taus[j] = (b - alpha) / b
            A[j + 1:, j] = sub * (one / (alpha - b))
            v = np.concatenate([[one], A[j + 1:, j]]).astype(dtype)
            A[j:, j + 1:] -= np.outer(v, taus[j] * (v @ A[j:, j + 1:]))
            A[j, j] = np.ldexp(b, ex)
    R = np.triu(A[:p, :])
    Q = np.zeros((m, p), dtype=dtype)
    Q[np.arange(p), np.arange(p)] = one
    for j in range(p - 1, -1, -1):
        if taus[j] != 0:
            v = np.concatenate([[one], A[j + 1:, j]]).astype(dtype)
            Q[j:, j:] -= np.outer(v, taus[j] * (v @ Q[j:, j:]))
    return Q, R


@functools.lru_cache(maxsize=None)
def restated(m, c, fam, longdouble=False):
    Q, R = householder(hh_matrix(m, c, fam), LD if longdouble else np.float64)
    Q.setflags(write=False)
    R.setflags(write=False)
    return Q, R


def qr_figures(A, Q, R):
    """(max|Q^T Q - I|, |Q R - A|_F / |A|_F; the latter |Q R|_F itself where A = 0), measured in float64."""
    Q, R = np.asarray(Q, dtype=float), np.asarray(R, dtype=float)
    orth = float(np.max(np.abs(Q.T @ Q - np.eye(Q.shape[1]))))
    na = float(np.linalg.norm(A))
    resid = float(np.linalg.norm(Q @ R - A)) / (na if na > 0.0 else 1.0)
    return orth, resid


@functools.lru_cache(maxsize=None)
def restated_figures(m, c, fam):
    return qr_figures(hh_matrix(m, c, fam), *restated(m, c, fam))


@functools.lru_cache(maxsize=None)
def restated_distance(m, c, fam):
    """(max|Q_64 - Q_ld|, max|R_64 - R_ld|): the float64 restatement's own distance from the longdouble one."""
    (Q, R), (Ql, Rl) = restated(m, c, fam), restated(m, c, fam, True)
    return float(np.max(np.abs(Q.astype(LD) - Ql))), float(np.max(np.abs(R.astype(LD) - Rl)))


# ---------------------------------------------------------------------------------------------- norms
NORM_G = (1, 255, 256, 257, 262143, 262144, 262145, 524295)     # the last four run past the 1024 x 256 grid
NORM_BOUND = 1 << 8


@functools.lru_cache(maxsize=None)
def norm_tensors(G):
    rng = np.random.default_rng([41, G])
    t = rng.integers(-NORM_BOUND, NORM_BOUND + 1, (3, G))
    t[0, 0], t[1, 0], t[2, -1] = NORM_BOUND, -NORM_BOUND, NORM_BOUND
    t.setflags(write=False)
    return t                                                        # new, prev, target as int64


def norm_sums(tnew, tprev, target):
    """The four sums as Python integers."""
    a, b, c = (np.asarray(x, dtype=np.int64) for x in (tnew, tprev, target))
    return [int(((a - b) ** 2).sum()), int((b ** 2).sum()), int(((a - c) ** 2).sum()), int((c ** 2).sum())]


# ---------------------------------------------------------------------------------------------- end to end
E2E_MODELS = [([48, 3, 45], [1, 33, 40, 1]), ([40, 2, 3, 36], [1, 33, 34, 35, 1]), ([256, 2, 256], [1, 256, 256, 1])]
ORTH_MODEL = 1                  # orth_left / orth_right run at every position of this one


def e2e_cores(index):
    """(the cores of the exact-rank target, the random start) of model `index`, entries scaled so that the tensor's
    entries are of order one."""
    n, ranks = E2E_MODELS[index]
    rng = np.random.default_rng([42, index])
    draw = lambda: [rng.standard_normal((ranks[k], n[k], ranks[k + 1])) / np.sqrt(ranks[k]) for k in range(len(n))]
    return draw(), draw()


def numpy_als(cores, T, iters):
    """ALS in projection form: orthogonalise right to left, then carry the projected target along both half sweeps."""
    cores, n, d = [c.copy() for c in cores], T.shape, len(cores)
    for k in range(d - 1, 0, -1):
        r0, nk, r1 = cores[k].shape
        Q, R = np.linalg.qr(cores[k].reshape(r0, -1).T)
        cores[k], cores[k - 1] = Q.T.reshape(-1, nk, r1), np.einsum("anb,cb->anc", cores[k - 1], R)
    for _ in range(iters):
        P = T.reshape(1, -1)
        for k in range(d):
            rl = P.shape[0]
            C = X = P.reshape(rl * n[k], -1)
            for j in range(d - 1, k, -1):
                Cj = cores[j].reshape(cores[j].shape[0], -1)
                C = C.reshape(-1, Cj.shape[1]) @ Cj.T
            cores[k] = C.reshape(rl, n[k], -1)
            if k < d - 1:
                Q, _ = np.linalg.qr(C.reshape(rl * n[k], -1))
                cores[k], P = Q.reshape(rl, n[k], -1), Q.T @ X
        S = T.reshape(-1, 1)
        for k in range(d - 1, -1, -1):
            rr = S.shape[1]
            C = X = S.reshape(-1, n[k] * rr)
            for j in range(k):
                Qj = cores[j].reshape(-1, cores[j].shape[2])
                C = Qj.T @ C.reshape(Qj.shape[0], -1)
            cores[k] = C.reshape(-1, n[k], rr)
            if k > 0:
                Q, _ = np.linalg.qr(C.reshape(-1, n[k] * rr).T)
                cores[k], S = Q.T.reshape(-1, n[k], rr), X @ Q
    return cores


def dense(cores):
    out = cores[0]
    for c in cores[1:]:
        out = np.einsum("...i,ijk->...jk", out, c)
    return out[0, ..., 0]


def lapack_sweep(cores, side, position):
    """The reference's orthogonalisation sweep in NumPy; per orthogonalised core (m, max|Q^T Q - I| of LAPACK's factor,
    the bond)."""
    cores, figures = [c.copy() for c in cores], {}
    d = len(cores)
    order = range(position) if side == "left" else range(d - 1, position, -1)
    for k in order:
        r0, nk, r1 = cores[k].shape
        if side == "left":
            Q, R = np.linalg.qr(cores[k].reshape(r0 * nk, r1))
            cores[k + 1] = np.einsum("ij,jpk->ipk", R, cores[k + 1])
            m = r0 * nk
        else:
            Q, R = np.linalg.qr(cores[k].reshape(r0, nk * r1).T)
            cores[k - 1] = np.einsum("ipk,jk->ipj", cores[k - 1], R)
            m = nk * r1
        figures[k] = (m, float(np.max(np.abs(Q.T @ Q - np.eye(Q.shape[1])))), Q.shape[1])
    return figures
