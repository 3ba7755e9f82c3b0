"""The row-Jacobi factorisation (rowjacobi_factor in csrc/pcx_ttbuild.hip, kernels of csrc/ttsvd_kernels.h) on every
path its dispatch takes, one factorisation per call through pcx_tt_svd with d = 2 (tests/row_jacobi.py).  The reference
is the NumPy restatement of the iteration, whose figures tests/golden/g30_row_jacobi.npz holds next to exact and
80-digit singular values; the bounds are the restatement's own figures times ten with floors at the last bits."""
import functools

import numpy as np
import pytest

import row_jacobi as RJ
from conftest import golden
from pychebyshev_amd import _algebra, _lib

pytestmark = pytest.mark.gpu

SHAPES = RJ.ALL_SHAPES + list(RJ.HADAMARD_SHAPES.values())
STATS = {p: {} for p in RJ.PATHS}
# one shape per iterating path for the bit-for-bit relations
METAMORPHIC_SHAPES = [(15, 300), (40, 460), (129, 140), (15, 1300), (17, 1085), (99, 198)]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for p in RJ.PATHS:
        s = STATS[p]
        if not s:
            continue
        print(f"\nrow-Jacobi, path {p}: a) {s.get('a', 0.0):.2e} ||C||_F  b) {s.get('b', 0.0):.2e}  c) {s.get('c', 0.0):.2e}  "
              f"d) {s.get('d', 0.0):.2e} sigma_0  relative, graded {s.get('rel', 0.0):.2e} (restatement "
              f"{s.get('rel_ref', 0.0):.2e}), hadamard {s.get('relh', 0.0):.2e} (restatement {s.get('relh_ref', 0.0):.2e})  "
              f"sweeps <= {int(s.get('sweeps', 0))} (restatement <= {int(s.get('sweeps_ref', 0))}, "
              f"largest excess {int(s.get('excess', -99))})")


def _worst(path, key, v):
    STATS[path][key] = max(STATS[path].get(key, -99.0), float(v))


@functools.lru_cache(maxsize=None)
def _fixture():
    return golden("g30_row_jacobi")


def _families(m, N):
    return ["hadamard"] if (m, N) in RJ.HADAMARD_SHAPES.values() else RJ.families_of(m, N)


def _matrix(fam, m, N):
    """The matrix, after its draw passed the fixture's checksum."""
    C, draw = RJ.matrix(fam, m, N)
    g, key = _fixture(), RJ.key(m, N, fam)
    assert RJ.checksum(draw) == (int(g[key + "_sum"]), int(g[key + "_sumsq"])), (key, "the random stream changed")
    return C


@functools.lru_cache(maxsize=None)
def _factored(fam, m, N):
    """(U, B, sweeps) of the device, shared by the tests of one shape; read-only."""
    U, B, sweeps = RJ.device_factor(_matrix(fam, m, N))
    U.setflags(write=False)
    B.setflags(write=False)
    return U, B, sweeps


def _sigma_ref(fam, m, N):
    """The singular values a case is held to: exact (hadamard), 80 digits (graded), else LAPACK."""
    if fam == "hadamard":
        return RJ.hadamard_sigma(m, N)
    key = RJ.key(m, N, fam) + "_sigma"
    return _fixture()[key] if key in _fixture().files else None


# ------------------------------------------------------------------ 1: the factorisation itself
@pytest.mark.parametrize("m,N", SHAPES)
def test_factorisation_invariants(m, N):
    """(a) U B = C, (b) U orthonormal, (d) the row norms are the singular values: each within
    max(10 x the restatement's figure, 1e-14); (c) kept rows mutually orthogonal to max(10 x restatement, 2 rot_tol(N)),
    the kernel's own stop rule; rows in descending order.  The zero matrix: rank 1, U[:, 0] = e_0, B = 0 exactly."""
    g, path, bad = _fixture(), RJ.path_of(m, N), []
    for fam in _families(m, N):
        C = _matrix(fam, m, N)
        U, B, _ = _factored(fam, m, N)
        assert U.shape[0] == m and B.shape == (U.shape[1], N) and 1 <= U.shape[1] <= min(m, N), (fam, U.shape, B.shape)
        assert np.all(np.isfinite(U)) and np.all(np.isfinite(B)), fam
        if fam == "zero":
            e0 = np.zeros(m)
            e0[0] = 1.0
            if not (U.shape[1] == 1 and np.array_equal(U[:, 0], e0) and np.array_equal(B, np.zeros((1, N)))):
                bad.append((fam, "rank / U / B", U.shape))
            continue
        f = RJ.figures(C, U, B, _sigma_ref(fam, m, N))
        ref = dict(zip("abcd", g[RJ.key(m, N, fam) + "_fig"]))
        print(f"{m}x{N} {fam} ({path}): " + "  ".join(f"{k}) {f[k]:.2e} (restatement {ref[k]:.2e})" for k in "abcd"))
        for k in "abcd":
            _worst(path, k, f[k])
            bound = max(10.0 * ref[k], 2.0 * RJ.rot_tol(N) if k == "c" else 1e-14)
            if not f[k] <= bound:
                bad.append((fam, k, f[k], bound))
        nrm = np.linalg.norm(B, axis=1)
        if not np.all(nrm[1:] <= nrm[:-1]):
            bad.append((fam, "row norms not descending"))
    assert not bad, (m, N, path, bad)


# ------------------------------------------------------------------ 2: convergence
@pytest.mark.parametrize("m,N", SHAPES)
def test_sweep_count_stays_next_to_the_restatement(m, N):
    """At least one sweep for m > 1, never the cap of 60; at most the restatement's count + 3 without the Gram
    preconditioner and at most the restatement's count behind it (it exists to save sweeps).  gauss behind the
    preconditioner takes exactly one sweep: k_symjacobi_lds stops after a sweep whose rotations were all within
    sqrt(1e-9) of orthogonal, which by the quadratic convergence of the cyclic iteration leaves the rows of V^T C (all
    singular values within a decade, so nothing is lost in the squares) near 1e-9 of orthogonal, below the 1e-8 mark
    that calls for another sweep of the row iteration.  A looser stop of the preconditioner shows here first."""
    g, path, bad = _fixture(), RJ.path_of(m, N), []
    for fam in _families(m, N):
        sweeps = _factored(fam, m, N)[2]
        want = int(g[RJ.key(m, N, fam) + "_sweeps"])
        print(f"{m}x{N} {fam} ({path}): {sweeps} sweeps, restatement {want}")
        _worst(path, "sweeps", sweeps)
        _worst(path, "sweeps_ref", want)
        _worst(path, "excess", sweeps - want)
        low = 1 if m > 1 else 0
        high = want if path in RJ.GRAM_PATHS else want + 3
        if path in RJ.GRAM_PATHS and fam == "gauss":
            high = 1
        if not (low <= sweeps <= high and sweeps < RJ.MAX_SWEEPS):
            bad.append((fam, sweeps, want))
    assert not bad, (m, N, path, bad)


# ------------------------------------------------------------------ 3: small singular values
RELATIVE_CASES = [(m, N, "graded") for (m, N) in RJ.ALL_SHAPES + [(64, 512)] if m >= 2] + \
                 [(m, N, "hadamard") for (m, N) in RJ.HADAMARD_SHAPES.values()]


@pytest.mark.parametrize("m,N,fam", RELATIVE_CASES)
def test_small_singular_values_keep_their_relative_accuracy(m, N, fam):
    """max|sigma_i / sigma_ref,i - 1| over sigma_ref,i > 64 eps sqrt(m) sigma_ref,0 against exact (hadamard) or
    80-digit (graded) values spanning 12 decades: within max(10 x restatement, 1e-13), behind the Gram preconditioner
    too.  Only a row-graded matrix with independent rows carries its small values to relative accuracy in FP64 at
    all: on hadamard, whose every row mixes all values, and on the tall graded shapes the restatement's own figure is
    1e-11 .. 1e-5 and the bound follows it."""
    path = RJ.path_of(m, N)
    sref = _sigma_ref(fam, m, N)
    B = RJ.device_factor(_matrix(fam, m, N))[1] if (m, N, fam) == (64, 512, "graded") else _factored(fam, m, N)[1]
    rel = RJ.relative_figure(B, sref, m)
    ref = float(_fixture()[RJ.key(m, N, fam) + "_rel"])
    print(f"{m}x{N} {fam} ({path}): relative {rel:.2e}, restatement {ref:.2e}")
    _worst(path, "rel" if fam == "graded" else "relh", rel)
    _worst(path, "rel_ref" if fam == "graded" else "relh_ref", ref)
    assert rel <= max(10.0 * ref, 1e-13), (m, N, fam, path, rel, ref)


# ------------------------------------------------------------------ 4: the rank rule
@pytest.mark.parametrize("m,N", RJ.RANK_SHAPES)
def test_rank_rule_counts_the_singular_values_above_the_cut(m, N):
    """graded: the rank at tol = 1e-6, 1e-10, 1e-12 is the count of 80-digit singular values above tol sigma_0 (none
    of which is within a factor RANK_GAP of a cut); the sig2 skip rule at up to 64 rows."""
    C = _matrix("graded", m, N)
    sigma = _fixture()[RJ.key(m, N, "graded") + "_sigma"]
    bad = []
    for tol in RJ.RANK_TOLS:
        U, B, sweeps = RJ.device_factor(C, tol=tol)
        want = int(np.sum(sigma > tol * sigma[0]))
        print(f"{m}x{N} ({RJ.path_of(m, N)}) tol {tol:g}: rank {U.shape[1]}, want {want}, {sweeps} sweeps")
        if U.shape[1] != want or not 1 <= sweeps < RJ.MAX_SWEEPS:
            bad.append((tol, U.shape[1], want, sweeps))
    assert not bad, (m, N, bad)


# ------------------------------------------------------------------ 5: metamorphic relations
@pytest.mark.parametrize("m,N", METAMORPHIC_SHAPES)
def test_power_of_two_scaling_and_repetition_are_exact(m, N):
    """Every threshold of the host code and the kernels is relative, so C 2^k (k = +-100) returns the same U bit for
    bit and B 2^k exactly; a second identical call returns equal bits."""
    bad = []
    for fam in ("gauss", "graded"):
        C = _matrix(fam, m, N)
        U, B, sweeps = _factored(fam, m, N)
        U2, B2, sweeps2 = RJ.device_factor(C)
        if not (np.array_equal(U, U2) and np.array_equal(B, B2) and sweeps == sweeps2):
            bad.append((fam, "repeat"))
        for k in (100, -100):
            Uk, Bk, sk = RJ.device_factor(C * 2.0 ** k)
            if not (Uk.shape == U.shape and np.array_equal(Uk, U) and np.array_equal(Bk, B * 2.0 ** k) and sk == sweeps):
                bad.append((fam, k, Uk.shape, U.shape, sk, sweeps))
    assert not bad, (m, N, RJ.path_of(m, N), bad)


def test_appended_zero_rows_leave_the_singular_values():
    """A 96 x 150 matrix with 1 and 44 zero rows appended (97: still LDS, U in HBM; 140: the global path): the same
    singular values within bound (d)."""
    C = _matrix("gauss", 96, 150)
    bound = max(10.0 * float(_fixture()[RJ.key(96, 150, "gauss") + "_fig"][3]), 1e-14)
    sref = np.linalg.svd(C, compute_uv=False)
    assert [RJ.path_of(r, 150) for r in (96, 97, 140)] == ["lds_hbm", "lds_hbm", "nogram"]
    for rows in (96, 97, 140):
        Cz = np.vstack([C, np.zeros((rows - 96, 150))])
        U, B, _ = RJ.device_factor(Cz)
        sig = RJ.sigma_of(B, 96)
        d = float(np.max(np.abs(sig - sref)) / sref[0])
        print(f"{rows}x150 ({RJ.path_of(rows, 150)}): d) {d:.2e}, bound {bound:.2e}")
        assert d <= bound, (rows, d, bound)
        assert np.array_equal(U[96:], np.zeros((rows - 96, U.shape[1]))), rows         # zero rows are never rotated


# ------------------------------------------------------------------ 6: the callers
def _dense(cores):
    full = cores[0]
    for c in cores[1:]:
        full = np.tensordot(full, c, axes=([-1], [0]))
    return full.reshape([c.shape[1] for c in cores])


def _train(seed, n, ranks):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((ranks[k], n[k], ranks[k + 1])) for k in range(len(n))]


# n, then the matrices orthogonalise_right factors at k = 2 and k = 1 (the bond 2 comes back at 12, the exact
# dependencies of 48 rows in 12 columns are dropped) with their paths.  In the first train the second one is 40 x 120
# and stays in LDS; the second train widens it to 40 x 480.
ROUND_TRAINS = [((12, 10, 12), [((48, 12), "lds_u"), ((40, 120), "lds_u")]),
                ((12, 40, 12), [((48, 12), "lds_u"), ((40, 480), "gram_graph")])]


@pytest.mark.parametrize("n,factored", ROUND_TRAINS)
def test_rounding_on_ranks_above_what_the_tensor_admits(n, factored):
    """tt_round of Gaussian cores with ranks (1, 40, 48, 1): exact dependencies in every factorisation.  tol = 0: the
    tensor unchanged to 1e-13 ||T||, ranks <= (12, 12), cores 0 .. d-2 left-orthonormal to 1e-13.  tol = 1e-8: the
    error at most sqrt(sum_k m_k) tol ||T||, m_k the row count of each truncated factorisation -- the sum of what
    the rule S > tol S[0] may drop."""
    for (shape, path) in factored:
        assert RJ.path_of(*shape) == path, (shape, RJ.path_of(*shape))
    cores = _train(61, n, (1, 40, 48, 1))
    T = _dense(cores)
    norm = float(np.linalg.norm(T))
    out = _algebra.tt_round(cores, 256, 0.0, _lib.default_device())
    ranks = [c.shape[2] for c in out[:-1]]
    err = float(np.max(np.abs(_dense(out) - T))) / norm
    print(f"round {n}: ranks {ranks}, max error {err:.2e} ||T||")
    assert ranks[0] <= 12 and ranks[1] <= 12, ranks
    assert err <= 1e-13, err
    for c in out[:-1]:
        q = c.reshape(-1, c.shape[2])
        assert np.max(np.abs(q.T @ q - np.eye(q.shape[1]))) <= 1e-13
    out = _algebra.tt_round(cores, 256, 1e-8, _lib.default_device())
    m_k = [40, 12]                      # the transposed unfoldings truncate_left factors: r_1 = 40 rows, then r_2 = 12
    err = float(np.linalg.norm(_dense(out) - T)) / norm
    print(f"round {n} at 1e-8: ranks {[c.shape[2] for c in out[:-1]]}, error {err:.2e} ||T||")
    assert err <= np.sqrt(sum(m_k)) * 1e-8, err


def test_swap_through_the_global_path_without_gram():
    """tt_swaps at position 1 of a train with (r_l, n_a, r_m, n_b, r_r) = (4, 20, 16, 40, 8) there: the merged matrix
    is 160 x 160.  tol = 0: the tensor with axes 1 and 2 exchanged, to 1e-13 ||T||."""
    assert RJ.path_of(4 * 40, 20 * 8) == "nogram"
    cores = _train(62, (4, 20, 40, 8), (1, 4, 16, 8, 1))
    T = _dense(cores)
    out = _algebra.tt_swaps(cores, [1], 256, 0.0, _lib.default_device())
    assert [c.shape[1] for c in out] == [4, 40, 20, 8]
    err = float(np.max(np.abs(_dense(out) - T.transpose(0, 2, 1, 3)))) / float(np.linalg.norm(T))
    print(f"swap: ranks {[c.shape[2] for c in out[:-1]]}, max error {err:.2e} ||T||")
    assert err <= 1e-13, err
