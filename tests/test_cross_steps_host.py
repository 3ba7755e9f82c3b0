"""What the GPU tests of the TT-Cross dense steps stand on, checked without a GPU: the input conditions of
tests/cross_steps.py, the restated maxvol against the oracle's, the fixture against its seeds, and the scale
dependence of the Jacobi stop rule that the kernel's prescaling removes."""
import numpy as np
import pytest

import cross_steps as CS
from conftest import golden

SMALL = [(m, c, f, cap) for (m, c, f, cap) in CS.CASES if m * c <= 1100 and f not in ("zero", "equal_sigma")]


def test_input_conditions_of_every_case():
    """Decision margins at least 1e-6 and at least 100 oracle_dev, no singular value within a factor 2 of the 1e-12 cut,
    a ratio of at least 2 at the cap of capcut; the shapes cover what the table claims."""
    g = golden("g31_cross_steps")
    assert len(CS.CASES) == len(set(CS.case_ids())) and 30 <= len(CS.CASES) <= 40
    for (m, c, fam, cap) in CS.CASES:
        key = CS.key(m, c, fam)
        assert m <= CS.MAX_M and c <= CS.MAX_R
        sigma, rank = g[key + "_sigma"], int(g[key + "_rank"])
        assert sigma.size == min(m, c) and np.all(np.diff(sigma) <= 0) and rank == CS.expected_rank(sigma, m, c, cap)
        if fam in ("zero", "equal_sigma"):
            continue
        cut = CS.REL_THRESH * sigma[0]
        assert not np.any((sigma > cut / CS.CUT_GAP) & (sigma < cut * CS.CUT_GAP)), key
        if fam == "capcut":
            assert rank == cap and sigma[cap - 1] >= CS.CAP_GAP * sigma[cap], key
        if m > rank:
            assert float(g[key + "_margin"]) >= max(CS.MARGIN_MIN, CS.MARGIN_OVER_DEV * float(g[key + "_dev"])), key
            assert bool(g[key + "_ontol"]), key
    shapes = {(m, c) for (m, c, _, _) in CS.CASES}
    assert {m for (m, _) in shapes} >= {1, 2, 63, 64, 65, 127, 128, 129, 704, 8192}
    assert {c for (_, c) in shapes} >= {1, 2, 8, 63, 64}
    assert {(4, 8), (40, 64), (9, 8), (8, 8), (704, 64), (8192, 8)} <= shapes
    assert CS.UNSUPPORTED == [(CS.MAX_M + 1, 8), (8, CS.MAX_R + 1)]
    # a rank cut by the rule, one cut by cap, one by zero columns, one by a duplicate
    ranks = {CS.key(m, c, f): int(g[CS.key(m, c, f) + "_rank"]) for (m, c, f, _) in CS.CASES}
    assert ranks["65x8_graded"] == 7 and ranks["129x24_capcut"] == 10 and ranks["65x8_zerocols"] == 5 and ranks["65x8_dupcols"] == 7
    assert set(CS.SCALE_CASES) <= set(CS.CASES)


def test_degenerate_families_are_exactly_what_they_claim():
    C = CS.matrix(65, 8, "zerocols", 8)[0]
    assert not C[:, [0, 4, 7]].any() and np.all(np.abs(C[:, [1, 2, 3, 5, 6]]).max(axis=0) > 0)
    C = CS.matrix(65, 8, "dupcols", 8)[0]
    assert C[:, 7].tobytes() == C[:, 1].tobytes()
    for (m, c) in ((64, 8), (128, 16)):
        C = CS.matrix(m, c, "equal_sigma", c)[0]
        G = C.T @ C                                              # integers times powers of two: exact
        s = CS.equal_sigma_scales(c)
        assert np.array_equal(G, np.diag(m * s * s)) and s[2] == s[5] and len(set(s.tolist())) < c
    assert not CS.matrix(12, 3, "zero", 3)[0].any()


def test_maxvol_tie_and_swap_cases_meet_their_conditions():
    """Every tie case: the pair ties exactly at an arg-max of its phase (in phase 2 one that swaps), the smaller index
    wins, every other decision has a margin of 1e-6.  The swap case needs three swaps at tol = 1,
    and its pivots after two and three swaps depend on the rank-1 update being right."""
    for (dist, neg, phase), (seed, first) in CS.TIE_SEEDS.items():
        A = CS.tie_matrix(dist, neg, seed, first, phase)
        assert np.array_equal(A, np.rint(A)) and np.array_equal(A[first + dist], -A[first] if neg else A[first])
        piv, tr = CS.maxvol_restated(A)
        assert first in (tr.tie_rows1 if phase == 1 else tr.tie_rows2), (dist, neg, phase)
        assert first in piv and first + dist not in piv and tr.stopped_on_tol and tr.margin >= CS.MARGIN_MIN
    assert {k[0] for k in CS.TIE_SEEDS} == set(CS.TIE_DISTANCES) and len(CS.TIE_SEEDS) == 4 * len(CS.TIE_DISTANCES)
    m, r, seed = CS.SWAP_CASE
    A = CS.swap_matrix(m, r, seed)
    for k in range(4):
        piv, tr = CS.maxvol_restated(A, 1.0, k)
        assert tr.swaps == k and tr.margin >= CS.MARGIN_MIN
        if k >= 2:      # the case notices an update of column j without its division
            bad, trb = CS.maxvol_restated(A, 1.0, k, wrong_update=True)
            assert not np.array_equal(piv, bad) and trb.margin >= CS.MARGIN_MIN


def test_restated_maxvol_gives_the_oracles_pivots(oracle_mod):
    """On LAPACK's U of the 20 recorded matrices: the greedy projection of phase 1 is the column-pivoted QR of the
    oracle, and phase 2 is its swap loop."""
    g = golden("g6_primitives")
    for t in range(20):
        A = g[f"mv_A{t}"]
        piv, tr = CS.maxvol_restated(A)
        assert np.array_equal(piv, g[f"mv_p{t}"]), t
        assert np.array_equal(piv, oracle_mod.maxvol(A)), t


@pytest.mark.parametrize("m,c,fam,cap", SMALL, ids=[CS.key(m, c, f) for (m, c, f, _) in SMALL])
def test_fixture_reproduces_from_the_seeds(m, c, fam, cap):
    """The checksums of the draws and of the matrix, the rank, and -- with the whole kernel restated in NumPy, Jacobi
    loop included -- the fixture's pivots and C_hat within the GPU test's own bar."""
    g, key = golden("g31_cross_steps"), CS.key(m, c, fam)
    C, draw = CS.matrix(m, c, fam, cap)
    assert CS.checksum(draw) == (float(g[key + "_sum"]), float(g[key + "_sumsq"]))
    assert CS.checksum(C) == tuple(g[key + "_csum"].tolist())
    chat, piv, rank, sweeps = CS.cross_step_restated(C, cap)
    assert rank == int(g[key + "_rank"])
    # c > m columns cannot all be orthogonal and non-zero: there the loop may rotate rounding noise until its cap, and
    # C_hat = U inv(U) = I whatever it leaves; everywhere else it converges, zero and duplicated columns
    # included
    assert sweeps < CS.JACOBI_SWEEPS or m < c, sweeps
    assert np.array_equal(piv, g[key + "_piv"])
    ref = CS.chat_longdouble(g[key + "_utop"], piv)
    assert np.max(np.abs(chat - ref)) <= 8.0 * max(float(g[key + "_dev"]), 64.0 * CS.EPS)


def test_checksums_and_ranks_of_the_large_cases():
    g = golden("g31_cross_steps")
    for (m, c, fam, cap) in CS.CASES:
        key = CS.key(m, c, fam)
        C, draw = CS.matrix(m, c, fam, cap)
        assert CS.checksum(draw) == (float(g[key + "_sum"]), float(g[key + "_sumsq"])), key
        assert CS.checksum(C) == tuple(g[key + "_csum"].tolist()), key
        lapack = np.linalg.svd(C, compute_uv=False)
        assert CS.expected_rank(lapack, m, c, cap) == int(g[key + "_rank"]), key
        assert np.max(np.abs(lapack - g[key + "_sigma"])) <= 64.0 * CS.EPS * max(float(lapack[0]), 1e-300), key


def test_the_stop_rule_depends_on_the_scale_and_the_prescaling_removes_it():
    """40 x 8 of rank 3.  Times 2^300 the product of two squared column norms overflows, no pair is rotated and the
    kernel before the prescaling returns rank 8; times 2^-250 the product underflows for the noise columns and the loop
    runs all 60 sweeps; at 2^+-600 the squares themselves leave the range and the rank collapses to 1.  With the
    prescaling every scale gives rank 3 and the sweeps of the unscaled matrix."""
    rng = np.random.default_rng([31, 400])
    C = rng.standard_normal((40, 3)) @ rng.standard_normal((3, 8))
    _, _, rank0, sweeps0 = CS.cross_step_restated(C, 8)
    assert rank0 == 3 and sweeps0 < 20
    old = {k: CS.cross_step_restated(np.ldexp(C, k), 8, prescale=False)[2:] for k in (300, -250, 600, -600)}
    assert old[300][0] == 8 and old[300][1] == 1
    assert old[-250] == (3, CS.JACOBI_SWEEPS)
    assert old[600][0] == 1 and old[-600][0] == 1
    for k in (-900, -520, -250, 250, 300, 520, 900):
        chat, piv, rank, sweeps = CS.cross_step_restated(np.ldexp(C, k), 8)
        assert (rank, sweeps) == (rank0, sweeps0), k


def test_dct_restatement_stays_inside_the_bound():
    """The NumPy restatement against the 40-digit fixture: a small fraction of the bound the kernel is held to."""
    g = golden("g31_cross_steps")
    worst = 0.0
    for n in CS.DCT_N:
        for (rl, rr) in CS.DCT_RANKS:
            x = CS.dct_input(n, rl, rr)
            ref = g[CS.dct_key(n, rl, rr)]
            assert ref.shape == x.shape
            assert x.size <= 100 or np.log10(np.abs(x).max() / np.abs(x).min()) > 5.0
            worst = max(worst, float(np.max(np.abs(CS.dct_restated(x) - ref) / CS.dct_bound(x))))
    assert worst <= 0.5, worst                                   # 0.25 here; the summation order of another CPU moves it
    sizes = [rl * n * rr for n in CS.DCT_N for (rl, rr) in CS.DCT_RANKS]
    assert min(sizes) == 1 and any(s < 256 for s in sizes) and any(256 < s < 512 for s in sizes) and max(sizes) > 4096
