"""CPU-only checks of what tests/test_gpu_als_steps.py rests on (tests/als_steps.py): the NumPy restatement of
k_tta_householder against numpy.linalg.qr and against itself in longdouble, the exactness of the integer cases, the
coverage of the case tables recomputed from the dispatch rule, and the ABI entries.  No GPU compute here."""
import numpy as np
import pytest

import als_steps as AS
from pychebyshev_amd import _lib

EPS = AS.EPS
SMALL_SHAPES = [s for s in AS.HH_SHAPES if s[0] * s[1] <= 700 * 65]


@pytest.mark.parametrize("fam", AS.WELL_CONDITIONED)
@pytest.mark.parametrize("m,c", AS.HH_SHAPES)
def test_restatement_against_lapack(m, c, fam):
    """Up to the signs of the columns of Q (rows of R) the float64 restatement is LAPACK's factorisation: both are
    backward stable, so on a matrix of condition kappa they agree entrywise to a modest multiple of
    kappa m eps (kappa <= 20 for flat; the leading square of a Gaussian matrix is taken as it comes, with its own
    condition number measured)."""
    A = AS.hh_matrix(m, c, fam)
    p = min(m, c)
    Q, R = AS.restated(m, c, fam)
    Ql, Rl = np.linalg.qr(A)
    assert Q.shape == (m, p) and R.shape == (p, c)
    sign = np.sign(np.diag(R[:, :p])) * np.sign(np.diag(Rl[:, :p]))
    assert np.all(np.abs(sign) == 1.0)
    kappa = np.linalg.cond(A[:, :p])
    bar = 8.0 * kappa * max(m, 8) * EPS
    assert np.max(np.abs(Q * sign - Ql)) <= bar, (np.max(np.abs(Q * sign - Ql)), bar)
    assert np.max(np.abs(R * sign[:, None] - Rl)) <= bar * np.max(np.abs(Rl))
    orth, resid = AS.restated_figures(m, c, fam)
    assert orth <= 8.0 * max(m, 8) * EPS and resid <= 8.0 * max(m, 8) * EPS


HOST_CASES = [k for k in AS.HH_CASES if k[:2] in SMALL_SHAPES or k[2] == "flat"]


@pytest.mark.parametrize("m,c,fam", HOST_CASES, ids=[AS.hh_id(k) for k in HOST_CASES])
def test_restatement_float64_against_longdouble(m, c, fam):
    """The figures the GPU bars are multiples of: the float64 restatement is orthonormal and reproduces A to a few
    m eps in every family, the degenerate ones included, and on the flat family its entries lie within cond m eps of
    the longdouble restatement's."""
    A = AS.hh_matrix(m, c, fam)
    orth, resid = AS.restated_figures(m, c, fam)
    print(f"{AS.hh_id((m, c, fam))}: restated max|Q^T Q - I| {orth:.2e}, |QR - A|/|A| {resid:.2e}, m eps {m * EPS:.2e}")
    assert orth <= 8.0 * max(m, 8) * EPS and resid <= 8.0 * max(m, 8) * EPS
    Q, R = AS.restated(m, c, fam)
    assert not np.tril(R[:, :min(m, c)], -1).any()
    if fam == "flat":
        dq, dr = AS.restated_distance(m, c, fam)
        print(f"    distance from longdouble: Q {dq:.2e}, R {dr:.2e}")
        assert dq <= 20.0 * 8.0 * max(m, 8) * EPS and dr <= 20.0 * 8.0 * max(m, 8) * EPS
        Rl = AS.restated(m, c, fam, True)[1]
        assert np.array_equal(np.sign(np.diag(R)), np.sign(np.diag(Rl)).astype(float))
    if fam == "triu":
        p = min(m, c)
        assert np.array_equal(Q, np.eye(m, p)) and R.tobytes() == A[:p].tobytes()
    if fam == "zero":
        assert np.array_equal(Q, np.eye(m, min(m, c))) and not R.any()


@pytest.mark.parametrize("m,c", AS.SCALE_SHAPES)
def test_restatement_is_scale_free(m, c):
    """What the GPU scale test asserts of the kernel holds of its restatement: Q bit for bit, R = ldexp(R_0, e)."""
    A = AS.scale_matrix(m, c)
    assert np.min(np.abs(A)) >= 2.0 ** -4 and np.max(np.abs(A)) <= 2.0 ** 4
    Q0, R0 = AS.householder(A)
    for e in AS.SCALE_EXPONENTS:
        Ae = np.ldexp(A, e)
        assert np.array_equal(np.ldexp(Ae, -e), A) and np.all(np.isfinite(Ae))
        assert np.min(np.abs(Ae)) >= np.finfo(float).tiny
        Q, R = AS.householder(Ae)
        assert Q.tobytes() == Q0.tobytes(), e
        assert R.tobytes() == np.ldexp(R0, e).tobytes(), e


def test_unscaled_squares_fail_as_the_issue_states():
    """The arithmetic the kernel had before: sigma = sum a^2 on the unscaled column.  At 2^-600 sigma underflows, every
    column takes the identity reflector and QR is far from A; at 2^600 it overflows."""
    A = AS.scale_matrix(9, 4)
    for e, finite in ((-600, True), (600, False)):
        Ae = np.ldexp(A, e)
        with np.errstate(over="ignore", invalid="ignore"):
            sigma = np.array([np.sum(Ae[j + 1:, j] ** 2) for j in range(4)])
        assert np.all(sigma == 0.0) if finite else np.all(np.isinf(sigma))


@pytest.mark.parametrize("case", AS.CASES, ids=AS.case_id)
def test_integer_cases_are_exact_in_any_order(case):
    r, K, R = case
    Q, P = AS.integer_factors(r, K, R)
    assert np.array_equal(Q, np.rint(Q)) and np.array_equal(P, np.rint(P))
    assert max(np.abs(Q).max(), np.abs(P).max()) <= AS.INT_BOUND
    assert AS.integer_bound(r, K, R) < 2 ** 53 and K * AS.INT_BOUND ** 2 < 2 ** 53
    ref = AS.integer_product(r, K, R)
    assert ref.shape == (r, R) and np.array_equal(ref.astype(float).astype(np.int64), ref)
    if K * r * R <= 1 << 22:                                          # the integer matmul, which has no rounding
        assert np.array_equal(ref, Q.astype(np.int64).T @ P.astype(np.int64))
    rng = np.random.default_rng(5)                                    # Python integers, independent of NumPy's matmul
    for i, j in {(0, 0), (r - 1, R - 1)} | {(int(rng.integers(r)), int(rng.integers(R))) for _ in range(16)}:
        assert int(ref[i, j]) == sum(int(Q[k, i]) * int(P[k, j]) for k in range(K))


@pytest.mark.parametrize("G", AS.NORM_G)
def test_norm_cases_are_exact(G):
    t = AS.norm_tensors(G)
    assert t.shape == (3, G) and np.abs(t).max() <= AS.NORM_BOUND
    sums = AS.norm_sums(*t)
    assert G * (2 * AS.NORM_BOUND) ** 2 < 2 ** 53 and all(0 <= s < 2 ** 53 for s in sums)
    if G <= 257:
        a, b, c = (x.tolist() for x in t)
        assert sums == [sum((x - y) ** 2 for x, y in zip(a, b)), sum(y * y for y in b),
                        sum((x - z) ** 2 for x, z in zip(a, c)), sum(z * z for z in c)]


def test_norm_sizes_straddle_the_fixed_grid():
    full = AS.RED_BLOCKS * AS.THREADS
    assert {full - 1, full, full + 1} <= set(AS.NORM_G) and max(AS.NORM_G) > 2 * full
    assert {AS.THREADS - 1, AS.THREADS, AS.THREADS + 1, 1} <= set(AS.NORM_G)


def test_case_table_is_the_one_the_issue_sets():
    ranks = (1, 3, 4, 5, 8, 9, 12, 13, 15, 16, 17, 31, 32, 33, 48, 64, 65, 255, 256)
    ks = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65)
    rs = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000)
    cases = set(AS.CASES)
    assert {(r, 5, 65) for r in ranks} <= cases
    assert {(r, K, 65) for r in (5, 16, 33) for K in ks} <= cases
    assert {(r, 5, R) for r in (5, 16, 33) for R in rs} <= cases
    assert {(1, 1, 1), (256, 4096, 257)} <= cases
    assert sum(1 for (_, K, _) in cases if K == 4096) == 1 and len(AS.CASES) == len(cases)
    assert AS.ROUNDING_CASES == [(r, 777, 257) for r in (5, 16, 33, 256)]
    assert AS.NAN_RANKS == (5, 33)


def test_dispatch_restated():
    """The rule of left_project / right_project, spelled out at its edges."""
    V, M = AS.FORM_VALU, AS.FORM_MFMA
    assert [AS.dispatch(r, 0) for r in (1, 4, 5, 8, 9, 12, 13, 15)] == \
        [(V, 4, 1), (V, 4, 1), (V, 8, 1), (V, 8, 1), (V, 12, 1), (V, 12, 1), (V, 16, 1), (V, 16, 1)]
    assert [AS.dispatch(r, 0) for r in (16, 17, 32, 33, 256)] == [(M, 1, 1), (M, 2, 1), (M, 2, 1), (M, 2, 2), (M, 2, 8)]
    assert [AS.dispatch(r, 1) for r in (16, 17, 33, 256)] == [(V, 16, 1), (V, 16, 2), (V, 16, 3), (V, 16, 16)]
    assert [AS.dispatch(r, 2) for r in (1, 15, 16, 17)] == [(M, 1, 1), (M, 1, 1), (M, 1, 1), (M, 2, 1)]
    assert AS.dispatch(5, 0, mfma_min=1) == (M, 1, 1) and AS.dispatch(33, 0, mfma_min=999) == (V, 16, 3)


def test_case_table_reaches_every_branch():
    seen = set()
    for (r, K, R) in AS.CASES:
        for form in (AS.FORM_VALU, AS.FORM_MFMA):
            seen |= AS.branches(r, K, R, form)
    assert AS.REQUIRED_BRANCHES <= seen, sorted(AS.REQUIRED_BRANCHES - seen)
    # what the suite never ran before: mfma<1> on a ragged rank below 16, mfma<2> over gridDim.y, valu<16> at all
    assert any(r < 16 and AS.dispatch(r, 2)[1] == 1 for (r, _, _) in AS.CASES)
    assert any(AS.dispatch(r, 2)[2] > 1 for (r, _, _) in AS.CASES)
    assert any(AS.dispatch(r, 1)[1] == 16 for (r, _, _) in AS.CASES)
    # the Householder table: every family on both sides of the 256-thread stride and of m = c, and the limits
    shapes = set(AS.HH_SHAPES)
    assert {(255, 3), (256, 16), (257, 16), (7, 8), (8, 8), (9, 8), (256, 256), (512, 256), (65536, 4), (1, 1)} <= shapes
    for fam in AS.HH_FAMILIES:
        assert sum(1 for k in AS.HH_CASES if k[2] == fam) >= len(AS.HH_SHAPES) - 6, fam
    # the end-to-end models run mfma<2> over gridDim.y and touch both limits
    assert all(max(ranks) > 32 for _, ranks in AS.E2E_MODELS)
    assert max(AS.E2E_MODELS[2][0]) == AS.MAX_NODES and max(AS.E2E_MODELS[2][1]) == AS.MAX_RANK


def test_exact_rank_targets_are_recovered_by_numpy():
    """NumPy's projection ALS recovers the two smaller end-to-end targets in one iteration (the third, at the limits,
    runs with the GPU test)."""
    for index in (0, 1):
        truth, start = AS.e2e_cores(index)
        T = AS.dense(truth)
        got = AS.dense(AS.numpy_als(start, T, 1))
        assert np.linalg.norm(got - T) <= 1e-13 * np.linalg.norm(T)


def test_abi_table_has_the_diagnostic_entries():
    assert len(_lib.SIGNATURES["pcx_tt_als_project"][1]) == 10
    assert len(_lib.SIGNATURES["pcx_tt_als_qr"][1]) == 6
    assert len(_lib.SIGNATURES["pcx_tt_als_norms"][1]) == 6
    assert _lib.PCX_ERR_INTERNAL == -6
