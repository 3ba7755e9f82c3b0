"""The four device kernels of the TT-Cross dense steps (csrc/ttcross_kernels.h) called directly through the hooks of
pychebyshev_amd.tensor_train, on the case table of tests/cross_steps.py: both sides of the lane stride, one and 64
columns, m < c, m = rank + 1, the host limits, ranks cut by cap and by the 1e-12 rule, zero and duplicated columns,
exactly equal singular values, exact ties in both arg-max of maxvol, max_iters and tol away from their defaults, and
inputs scaled by 2^-900 .. 2^900.  The references are the 80-digit singular subspace of tests/golden/g31_cross_steps.npz
with the NumPy restatement of the kernel's own maxvol, a 40-digit DCT and Python integers for the grid values; every
bound is the reference's own error or a count of roundings, none is taken from the kernel."""
import functools

import numpy as np
import pytest

import cross_steps as CS
from conftest import golden
from pychebyshev_amd import tensor_train as tt_mod

pytestmark = pytest.mark.gpu

EPS = CS.EPS
RATIOS = {}                     # family -> the largest max|C_hat - C_hat_ref| / bar met


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if RATIOS:
        print("\ncross step, max|C_hat - C_hat_ref| / bar per family: " + "  ".join(f"{f} {v:.3f}" for f, v in sorted(RATIOS.items())))


@functools.lru_cache(maxsize=None)
def _fixture():
    return golden("g31_cross_steps")


def _matrix(m, c, fam, cap):
    """The matrix, after its draw passed the fixture's checksum."""
    C, draw = CS.matrix(m, c, fam, cap)
    g, key = _fixture(), CS.key(m, c, fam)
    assert CS.checksum(draw) == (float(g[key + "_sum"]), float(g[key + "_sumsq"])), (key, "the random stream changed")
    assert CS.checksum(C) == tuple(g[key + "_csum"].tolist()), (key, "the matrix is not the fixture's")
    return C


@functools.lru_cache(maxsize=None)
def _stepped(m, c, fam, cap):
    """(C_hat, pivots, rank) of the device, shared by the tests of one case; read-only."""
    chat, piv, rank = tt_mod._cross_step(_matrix(m, c, fam, cap), cap)
    chat.setflags(write=False)
    piv.setflags(write=False)
    return chat, piv, rank


# ------------------------------------------------------------------ k_cross_step
@pytest.mark.parametrize("m,c,fam,cap", CS.CASES, ids=CS.case_ids())
def test_rank_and_pivots(m, c, fam, cap):
    """The rank is the reference's rule on the 80-digit singular values (zerocols, dupcols: that of the non-degenerate
    part); the pivots are those of the restated maxvol on the 80-digit singular vectors, distinct and in range; where
    the restatement stopped on tol no entry of C_hat exceeds it."""
    g, key = _fixture(), CS.key(m, c, fam)
    chat, piv, rank = _stepped(m, c, fam, cap)
    assert rank == int(g[key + "_rank"])
    assert chat.shape == (m, rank) and piv.shape == (rank,)
    assert len(set(piv.tolist())) == rank and piv.min() >= 0 and piv.max() < m
    if fam != "equal_sigma":        # its rows tie exactly in every arg-max of phase 1: no pivot set is singled out
        assert np.array_equal(piv, g[key + "_piv"]), (piv, g[key + "_piv"])
    if bool(g[key + "_ontol"]):
        assert np.max(np.abs(chat)) <= CS.MAXVOL_TOL * (1.0 + 1e-12), np.max(np.abs(chat))


@pytest.mark.parametrize("m,c,fam,cap", CS.CASES, ids=CS.case_ids())
def test_chat_against_the_80_digit_subspace(m, c, fam, cap, oracle_mod):
    """C_hat[piv] = I to 64 eps max|C_hat|, and max|C_hat - U_top inv(U_top[piv])| <= 8 max(oracle_dev, 64 eps): eight
    times the distance of the LAPACK restatement from the same reference.  zerocols and dupcols meet it only if the
    Jacobi loop skips the zero columns and converges.  Above 256 rows (flat spectra): against oracle._cross_step at
    8 * 64 eps sigma_0 / sigma_rank.  The zero matrix: rank 1, pivot 0, C_hat = 0."""
    g, key = _fixture(), CS.key(m, c, fam)
    chat, piv, rank = _stepped(m, c, fam, cap)
    if fam == "zero":
        assert rank == 1 and piv.tolist() == [0] and chat.shape == (m, 1) and not chat.any()
        return
    top = float(np.max(np.abs(chat)))
    assert np.max(np.abs(chat[piv] - np.eye(rank))) <= 64.0 * EPS * top
    if m <= CS.U_TOP_MAX_M:
        ref = CS.chat_longdouble(g[key + "_utop"], piv)
        bar = 8.0 * max(float(g[key + "_dev"]), 64.0 * EPS)
    else:
        assert fam == "flat"
        ref, want_piv, want_rank = oracle_mod._cross_step(_matrix(m, c, fam, cap), cap)
        assert want_rank == rank and np.array_equal(want_piv[:rank], piv)
        sigma = g[key + "_sigma"]
        bar = 8.0 * 64.0 * EPS * float(sigma[0] / sigma[rank - 1])
    err = float(np.max(np.abs(chat.astype(CS.LD) - ref)))
    print(f"{key}: max|C_hat - ref| {err:.2e}, bar {bar:.2e}")
    RATIOS[fam] = max(RATIOS.get(fam, 0.0), err / bar)
    assert err <= bar, (key, err, bar)


def test_equal_singular_values_keep_the_stable_order():
    """128 x 16 Hadamard columns whose exact singular values repeat, cap = 5 between two equal ones: the kept columns are
    the first five of the stable descending order, so C_hat lies in their span and is orthogonal to the equal column
    that was cut."""
    m, c, fam, cap = 128, 16, "equal_sigma", 5
    chat, piv, rank = _stepped(m, c, fam, cap)
    s = CS.equal_sigma_scales(c)
    order = np.argsort(-s, kind="stable")
    assert rank == cap and s[order[cap - 1]] == s[order[cap]]
    H = CS.sylvester(m)
    inside = H[:, order[:cap]].T @ chat / m                     # exact products of +-1 with C_hat, up to the sum
    assert np.max(np.abs(chat - H[:, order[:cap]] @ inside)) <= 64.0 * EPS * np.max(np.abs(chat))
    assert np.max(np.abs(H[:, order[cap:]].T @ chat)) <= 64.0 * EPS * m * np.max(np.abs(chat))


def test_rel_thresh_is_the_argument():
    """The 1e-12 of the rank rule is an argument: at 1e-5 and 1e-10 the graded case keeps the values above those."""
    m, c, fam, cap = 65, 8, "graded", 8
    sigma = _fixture()[CS.key(m, c, fam) + "_sigma"]
    for thresh in (1e-5, 1e-10):
        want = int(np.sum(sigma > thresh * sigma[0]))
        assert not np.any((sigma > thresh * sigma[0] / 2) & (sigma < thresh * sigma[0] * 2))
        assert tt_mod._cross_step(_matrix(m, c, fam, cap), cap, thresh)[2] == want


@pytest.mark.parametrize("m,c,fam,cap", CS.SCALE_CASES, ids=[CS.key(m, c, f) for (m, c, f, _) in CS.SCALE_CASES])
def test_scale_free(m, c, fam, cap):
    """C 2^k for k = -900 .. 900: rank, pivots and C_hat bit for bit those of C.  They are homogeneous of degree 0, and
    the kernel works on C times an exact power of two."""
    C = _matrix(m, c, fam, cap)
    chat, piv, rank = _stepped(m, c, fam, cap)
    for k in CS.SCALE_EXPONENTS:
        Ck = np.ldexp(C, k)
        assert np.array_equal(np.ldexp(Ck, -k), C), "the scaled input must be exact"
        got_chat, got_piv, got_rank = tt_mod._cross_step(Ck, cap)
        assert got_rank == rank, (k, got_rank, rank)
        assert np.array_equal(got_piv, piv), (k, got_piv, piv)
        assert got_chat.tobytes() == chat.tobytes(), (k, float(np.max(np.abs(got_chat - chat))))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_input_is_an_error(bad):
    C = np.array(_matrix(9, 8, "flat", 8))
    C[7, 3] = bad
    with pytest.raises(ValueError, match=r"\(7, 3\).*not finite"):
        tt_mod._cross_step(C, 8)
    with pytest.raises(ValueError, match=r"\(7, 3\).*not finite"):
        tt_mod._maxvol(C)


@pytest.mark.parametrize("m,c", CS.UNSUPPORTED)
def test_beyond_the_limits_is_unsupported(m, c):
    with pytest.raises(NotImplementedError):
        tt_mod._cross_step(np.ones((m, c)), c)


# ------------------------------------------------------------------ k_maxvol
@pytest.mark.parametrize("phase", [1, 2])
@pytest.mark.parametrize("negated", [False, True])
@pytest.mark.parametrize("distance", CS.TIE_DISTANCES)
def test_maxvol_ties_go_to_the_smaller_index(distance, negated, phase):
    """Integer-valued A with row first + distance a copy (or the negative) of row first: the two tie exactly in the
    arg-max of the given phase, on lanes 1, 63, 0 (the same lane), 1 and 0 apart, and the smaller index is taken, as by
    np.argmax in the restatement."""
    seed, first = CS.TIE_SEEDS[(distance, negated, phase)]
    A = CS.tie_matrix(distance, negated, seed, first, phase)
    want, tr = CS.maxvol_restated(A)
    assert first in (tr.tie_rows1 if phase == 1 else tr.tie_rows2) and first in want and first + distance not in want
    got = tt_mod._maxvol(A)
    assert np.array_equal(got, want), (got, want)


def test_maxvol_max_iters_and_tol():
    """max_iters = k stops after exactly k swaps (tol = 1: the restatement needs at least three); tol = 1e9 returns the
    phase-1 pivots; m <= r returns arange(m)."""
    m, r, seed = CS.SWAP_CASE
    A = CS.swap_matrix(m, r, seed)
    seen = []
    for k in range(4):
        want, tr = CS.maxvol_restated(A, 1.0, k)
        assert tr.swaps == k
        got = tt_mod._maxvol(A, tol=1.0, max_iters=k)
        assert np.array_equal(got, want), (k, got, want)
        seen.append(tuple(got.tolist()))
    assert len(set(seen)) == 4
    want, tr = CS.maxvol_restated(A, 1e9)
    assert tr.swaps == 0 and np.array_equal(want, tr.phase1) and seen[0] == tuple(tr.phase1.tolist())
    assert np.array_equal(tt_mod._maxvol(A, tol=1e9), tr.phase1)
    assert np.array_equal(tt_mod._maxvol(A[:r]), np.arange(r))
    assert np.array_equal(tt_mod._maxvol(A[:r - 2]), np.arange(r - 2))


# ------------------------------------------------------------------ k_value_to_coeff_core
@pytest.mark.parametrize("rl,rr", CS.DCT_RANKS)
@pytest.mark.parametrize("n", CS.DCT_N)
def test_dct_against_40_digits(n, rl, rr):
    """Every coefficient within (3 pi max(k, 1) + n + 4) eps (2 / n) sum_j |x_j| of the 40-digit value
    (cross_steps.dct_bound), and the round trip through _coeff_core_to_value_core within that bound summed over k."""
    x = CS.dct_input(n, rl, rr)
    ref = _fixture()[CS.dct_key(n, rl, rr)]
    bound = CS.dct_bound(x)
    got = tt_mod._value_core_to_coeff_core(x)
    assert got.shape == x.shape
    worst = float(np.max(np.abs(got - ref) / bound))
    print(f"dct {rl}x{n}x{rr}: {worst:.3f} of the bound")
    assert np.all(np.abs(got - ref) <= bound), worst
    back = tt_mod._coeff_core_to_value_core(got)
    assert np.all(np.abs(back - x) <= np.sum(bound, axis=1)[:, None, :])


# ------------------------------------------------------------------ k_tt_grid_eval
GRID_TRAINS = [
    [1, 1], [1, 7, 1], [1, 64, 1], [1, 7, 7, 7, 7, 1], [1, 64, 64, 1, 1, 1],
    [1] * 13, [1] + [7] * 11 + [1], [1, 64, 1, 64, 1, 1, 2, 1, 1, 3, 1, 1, 1],
]
GRID_COUNTS = (1, 63, 64, 65, 1000)


@pytest.mark.parametrize("ranks", GRID_TRAINS, ids=lambda r: f"d{len(r) - 1}_r{max(r)}")
def test_grid_values_of_integer_trains_are_exact(ranks):
    """Integer cores with entries -3 .. 3 whose every partial sum stays below 2^53: the chain is exact in FP64 in any
    order, so the device values equal the integer ones.  Indices 0 and n - 1 occur in every dimension."""
    d = len(ranks) - 1
    n = [(4, 1, 3, 5, 2, 6)[k % 6] for k in range(d)]
    rng = np.random.default_rng([31, 300, d, max(ranks)])
    cores = [rng.integers(-3, 4, (ranks[k], n[k], ranks[k + 1])) for k in range(d)]
    bound = np.ones((1, 1), dtype=object)
    for G in cores:                                               # the largest partial sum any order can meet
        bound = bound @ np.abs(G).max(axis=1).astype(object)
        assert int(bound.max()) * max(G.shape[0], G.shape[2]) < 2 ** 53
    for count in GRID_COUNTS:
        idx = np.column_stack([rng.integers(0, n[k], count) for k in range(d)])
        idx[-1] = np.array(n) - 1
        if count > 1:
            idx[0] = 0
        v = np.ones((count, 1), dtype=np.int64)
        for k, G in enumerate(cores):
            v = np.einsum("pa,apb->pb", v, G[:, idx[:, k], :].astype(np.int64))
        got = tt_mod._tt_grid_values([G.astype(float) for G in cores], idx)
        assert np.array_equal(got, v[:, 0].astype(float)), (count, int(np.argmax(got != v[:, 0])))
