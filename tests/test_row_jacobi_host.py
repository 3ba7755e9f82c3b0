"""What the GPU tests of the row-Jacobi factorisation stand on, checked without a GPU: the NumPy restatement
against LAPACK, the fixture against the restatement, the dispatch table, and the exactness of the inputs."""
import numpy as np
import pytest

import row_jacobi as RJ
from conftest import golden

SMALL = [(m, N) for (m, N) in RJ.ALL_SHAPES if m <= 64]


@pytest.mark.parametrize("m,N", SMALL)
def test_restatement_factors_like_lapack(m, N):
    """Figures (a) .. (d) of the restatement at 1e-13 on every family, (d) against np.linalg.svd; the sweep count is
    the fixture's (to one sweep: a pair on the 1e-8 mark may fall either way with the CPU's summation order)."""
    g = golden("g30_row_jacobi")
    for fam in RJ.families_of(m, N):
        C, _ = RJ.matrix(fam, m, N)
        U, B, sweeps = RJ.restatement(C)
        assert np.max(np.abs(U @ B - C)) <= 1e-13 * max(float(np.linalg.norm(C)), 1.0), fam     # before any selection
        f = RJ.figures(C, *RJ.select(U, B))
        assert all(f[k] <= 1e-13 for k in "abcd"), (m, N, fam, f)
        assert abs(sweeps - int(g[RJ.key(m, N, fam) + "_sweeps"])) <= 1 and sweeps < RJ.MAX_SWEEPS, (m, N, fam, sweeps)


@pytest.mark.parametrize("m,N,fam", [(6, 140, "graded"), (40, 30, "lowrank"), (16, 1153, "dup"), (32, 64, "hadamard")])
def test_fixture_holds_the_restatements_figures(m, N, fam):
    g = golden("g30_row_jacobi")
    C, _ = RJ.matrix(fam, m, N)
    sref = RJ.hadamard_sigma(m, N) if fam == "hadamard" else g[RJ.key(m, N, fam) + "_sigma"] if fam == "graded" else None
    Us, Bs = RJ.select(*RJ.restatement(C)[:2])
    f = RJ.figures(C, Us, Bs, sref)
    # figures of rounding errors: another CPU's summation order moves them, not their size
    def close(got, want):
        return want / 3.0 - 1e-17 <= got <= 3.0 * want + 1e-17
    for k, want in zip("abcd", g[RJ.key(m, N, fam) + "_fig"]):
        assert close(f[k], want), (k, f[k], want)
    if sref is not None:
        assert close(RJ.relative_figure(Bs, sref, m), float(g[RJ.key(m, N, fam) + "_rel"]))


def test_the_sig2_rule_of_the_restatement_keeps_the_rank():
    """With tol > 0 the restatement skips the pairs far below the cut and still returns the fixture's rank."""
    g = golden("g30_row_jacobi")
    C, _ = RJ.matrix("graded", 17, 1085)
    sigma = g[RJ.key(17, 1085, "graded") + "_sigma"]
    for tol in RJ.RANK_TOLS:
        U, B, _ = RJ.restatement(C, tol)
        assert RJ.select(U, B, None, tol)[0].shape[1] == int(np.sum(sigma > tol * sigma[0])), tol


def test_every_listed_shape_reaches_the_path_it_is_listed_under():
    """If a threshold of rowjacobi_factor moves, restate it in row_jacobi.path_of and move the shapes: all seven paths
    stay covered, the edges next to each other."""
    reached = set()
    for path, shapes in RJ.SHAPES.items():
        for (m, N) in shapes:
            assert RJ.path_of(m, N) == path, (m, N, RJ.path_of(m, N), path)
            assert m * N < 33000
            reached.add(path)
    assert reached == set(RJ.PATHS) and len(RJ.PATHS) == 7
    for path, (m, N) in RJ.HADAMARD_SHAPES.items():
        assert RJ.path_of(m, N) == path and m & (m - 1) == 0 and N & (N - 1) == 0
    # the edges: the last shape with U in LDS and the first without, the last LDS shape and the first global one,
    # 64 and 65 pairs per step, N = 2 m and m = 100 without Gram, 16 and 17 rows with it
    assert RJ.u_in_lds(40, 459) and not RJ.u_in_lds(40, 460)
    assert RJ.u_in_lds(130, 20) and not RJ.u_in_lds(129, 140)
    assert (RJ.path_of(96, 192), RJ.path_of(96, 193)) == ("lds_hbm", "gram_graph")
    assert (RJ.path_of(127, 20), RJ.path_of(129, 20)) == ("lds_u", "lds_second")
    assert (RJ.path_of(99, 199), RJ.path_of(99, 198), RJ.path_of(100, 201)) == ("gram_graph", "nogram", "nogram")
    assert (RJ.path_of(16, 1153), RJ.path_of(17, 1085)) == ("gram_plain", "gram_graph")
    assert all(RJ.path_of(m, N) != "none" and m <= 64 for (m, N) in RJ.RANK_SHAPES)
    assert len({RJ.path_of(m, N) for (m, N) in RJ.RANK_SHAPES}) == 4


def test_hadamard_entries_are_exact():
    """Rebuilt in Python integers scaled by 2^39: every entry of the FP64 matrix is the exact sum."""
    for (m, N) in RJ.HADAMARD_SHAPES.values():
        r = RJ.hadamard_rank(m, N)
        Hm, HN = RJ.sylvester(m).tolist(), RJ.sylvester(N).tolist()
        assert all(sum(Hm[i][k] * Hm[j][k] for k in range(m)) == (m if i == j else 0) for i in range(0, m, 5) for j in range(m))
        C = RJ.matrix("hadamard", m, N)[0]
        for i in range(m):
            for j in range(0, N, 7):
                exact = sum(Hm[i][k] * HN[k][j] * 2 ** (39 - 3 * k) for k in range(r))
                assert int(C[i, j] * 2.0 ** 39) == exact and float(exact) == C[i, j] * 2.0 ** 39, (m, N, i, j)


def test_checksums_and_the_gap_of_the_rank_rule_cases():
    g = golden("g30_row_jacobi")
    for (m, N, fam) in RJ.cases():
        C, draw = RJ.matrix(fam, m, N)
        key = RJ.key(m, N, fam)
        assert RJ.checksum(draw) == (int(g[key + "_sum"]), int(g[key + "_sumsq"])), key
        assert C.shape == (m, N) and (draw.size == 0 or (draw.min() >= -64 and draw.max() <= max(64, m - 1)))
    for (m, N) in RJ.RANK_SHAPES:
        sigma = g[RJ.key(m, N, "graded") + "_sigma"]
        assert sigma.size == min(m, N) and np.all(np.diff(sigma) <= 0)
        for tol in RJ.RANK_TOLS:
            cut = tol * sigma[0]
            assert not np.any((sigma > cut / RJ.RANK_GAP) & (sigma < cut * RJ.RANK_GAP)), (m, N, tol)
        # the cuts separate something: the rank differs between the tolerances, and the last value is below 1e-12
        assert len({int(np.sum(sigma > tol * sigma[0])) for tol in RJ.RANK_TOLS}) >= 2
        assert sigma[-1] < 1e-12 * sigma[0] < sigma[-2]
