"""CPU-only checks of ChebyshevTT.fit_samples / from_samples: the properties of the NumPy restatement (tests/tt_fit.py)
that the GPU tests lean on, and the host-side contract of the two methods -- every argument error is raised before the
library is loaded, the documented start cores, the column permutation.  No GPU compute here."""
import inspect

import numpy as np
import pytest

import tt_fit as F

from pychebyshev_amd import ChebyshevTT, Domain, Ns, _lib
from pychebyshev_amd import tensor_train as tt_mod


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the HIP library fails the test: the argument checks must come first."""
    def boom(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", boom)


@pytest.fixture(scope="module")
def prototype_runs():
    """The three prototype cases from seeds 0, 1, 2, twelve iterations each: {(case, seed): (history, test error)}."""
    runs = {}
    for case, c in F.CASES.items():
        pts, y = F.samples(case)
        tp, ty = F.samples(case, 2000, seed=7)
        for seed in (0, 1, 2):
            cores, hist = F.fit(F.start_cores(c["n"], c["rank"], seed), pts, y, c["domain"], max_iter=12, tolerance=0.0)
            err = np.linalg.norm(F.evaluate(cores, tp, c["domain"]) - ty) / np.linalg.norm(ty)
            runs[case, seed] = (hist, float(err))
    return runs


# ------------------------------------------------------------------ the restatement's own properties
@pytest.mark.parametrize("case", list(F.CASES))
def test_restatement_residual_never_increases(prototype_runs, case):
    """An exact least-squares step cannot increase the residual and a QR step does not change the tensor."""
    for seed in (0, 1, 2):
        hist = prototype_runs[case, seed][0]
        assert len(hist) == 12
        for a, b in zip(hist, hist[1:]):
            assert b <= a * (1.0 + 1e-12), (case, seed, hist)


@pytest.mark.parametrize("case", list(F.CASES))
def test_restatement_seeds_end_within_a_factor_of_two(prototype_runs, case):
    finals = [prototype_runs[case, seed][0][-1] for seed in (0, 1, 2)]
    tests = [prototype_runs[case, seed][1] for seed in (0, 1, 2)]
    assert max(finals) <= 2.0 * min(finals), finals
    assert max(tests) <= 2.0 * min(tests), tests
    assert max(tests) <= 3.0 * max(finals)            # no overfit: held-out error of the order of the training residual


def test_restatement_householder_qr_and_cholesky():
    rng = np.random.default_rng(3)
    for shape in ((7, 3), (3, 7), (5, 5), (4, 1)):
        for dtype in (np.float64, np.longdouble):
            A = rng.standard_normal(shape).astype(dtype)
            Q, R = F.householder_qr(A)
            p = min(shape)
            assert Q.shape == (shape[0], p) and R.shape == (p, shape[1]) and Q.dtype == dtype
            assert np.max(np.abs(Q @ R - A)) <= 1e-14 and np.max(np.abs(Q.T @ Q - np.eye(p))) <= 1e-14
            assert np.all(np.tril(R, -1) == 0)
    M = rng.standard_normal((9, 6))
    G = M.T @ M
    b = rng.standard_normal(6)
    np.testing.assert_allclose(F.cholesky_solve(G, b), np.linalg.solve(G, b), rtol=1e-10)
    with pytest.raises(ValueError):
        F.cholesky_solve(-G, b)


def test_restatement_design_row_is_the_gradient_of_the_value():
    """TT(x_i) is linear in core k with coefficient row a_i: A c_k reproduces the evaluation, at every position."""
    rng = np.random.default_rng(4)
    n, ranks = [4, 3, 5, 2], [1, 2, 3, 2, 1]
    domain = [(-1.0, 1.0), (0.0, 2.0), (-3.0, -1.0), (0.5, 1.0)]
    cores = [rng.standard_normal((ranks[k], n[k], ranks[k + 1])) for k in range(4)]
    pts = np.column_stack([rng.uniform(a, b, 50) for a, b in domain])
    want = F.evaluate(cores, pts, domain)
    Ts = F.bases(pts, domain, n)
    for k in range(4):
        A = F.design(cores, Ts, k)
        assert A.shape == (50, cores[k].size)
        np.testing.assert_allclose(A @ cores[k].ravel(), want, rtol=0, atol=1e-13 * np.max(np.abs(want)))


# ------------------------------------------------------------------ the public surface
def test_signatures():
    sig = inspect.signature(ChebyshevTT.fit_samples)
    assert list(sig.parameters) == ["self", "points", "values", "max_iter", "tolerance", "ridge", "verbose"]
    for name, default in (("max_iter", 20), ("tolerance", 1e-10), ("ridge", 1e-12), ("verbose", False)):
        assert sig.parameters[name].default == default and sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(ChebyshevTT.from_samples)
    assert list(sig.parameters) == ["points", "values", "num_dimensions", "domain", "n_nodes", "rank", "seed", "max_iter",
                                    "tolerance", "ridge", "max_derivative_order", "descriptor"]
    assert sig.parameters["rank"].default is inspect.Parameter.empty
    assert sig.parameters["rank"].kind is inspect.Parameter.KEYWORD_ONLY
    assert ChebyshevTT.from_coeff_cores([np.ones((1, 2, 1))], [[0, 1]]).fit_info is None


def test_abi_table_has_the_fit_session():
    for name, nargs in (("pcx_tt_fit_create", 8), ("pcx_tt_fit_create_dev", 8), ("pcx_tt_fit_destroy", 1),
                        ("pcx_tt_fit_set_form", 2), ("pcx_tt_fit_normal", 8), ("pcx_tt_fit_residual", 6)):
        assert len(_lib.SIGNATURES[name][1]) == nargs


def _tt(d=3, n=4, r=2, dim_order=None):
    rng = np.random.default_rng(5)
    ranks = [1] + [r] * (d - 1) + [1]
    cores = [rng.standard_normal((ranks[k], n, ranks[k + 1])) for k in range(d)]
    return ChebyshevTT.from_coeff_cores(cores, [[-1.0, 1.0], [0.0, 2.0], [1.0, 3.0], [0.0, 1.0]][:d], dim_order=dim_order)


def _good(N=40, d=3):
    rng = np.random.default_rng(6)
    lo, hi = np.array([-1.0, 0.0, 1.0, 0.0][:d]), np.array([1.0, 2.0, 3.0, 1.0][:d])
    return lo + (hi - lo) * rng.random((N, d)), rng.standard_normal(N)


def test_fit_samples_argument_errors_come_before_the_library(no_library):
    tt = _tt()
    pts, y = _good()
    unbuilt = ChebyshevTT(lambda p, _: 0.0, 3, [[0, 1]] * 3, [3, 3, 3])
    with pytest.raises(RuntimeError, match="build"):
        unbuilt.fit_samples(pts, y)
    for bad_pts in (pts[:, :2], pts.ravel(), pts[None]):
        with pytest.raises(ValueError, match=r"points must have shape \(N, 3\)"):
            tt.fit_samples(bad_pts, y)
    for bad_y in (y[:-1], y[:, None], np.float64(1.0)):
        with pytest.raises(ValueError, match="values must have shape"):
            tt.fit_samples(pts, bad_y)
    with pytest.raises(ValueError, match="at least one sample"):
        tt.fit_samples(pts[:0], y[:0])
    with pytest.raises(TypeError, match="real numbers"):
        tt.fit_samples(pts.astype(complex), y)
    with pytest.raises(TypeError, match="real numbers"):
        tt.fit_samples(pts, np.array(["a"] * 40))
    for bad in (np.nan, np.inf, -np.inf):
        p2, y2 = pts.copy(), y.copy()
        p2[7, 1] = bad
        y2[3] = bad
        with pytest.raises(ValueError, match="points contain NaN or Inf"):
            tt.fit_samples(p2, y)
        with pytest.raises(ValueError, match="values contain NaN or Inf"):
            tt.fit_samples(pts, y2)
    for col, value in ((0, -1.0000001), (1, 2.5), (2, 0.999)):
        p2 = pts.copy()
        p2[11, col] = value
        with pytest.raises(ValueError, match=rf"points\[:, {col}\] leaves the domain"):
            tt.fit_samples(p2, y)
    for ridge in (-1e-12, np.nan, np.inf):
        with pytest.raises(ValueError, match="ridge"):
            tt.fit_samples(pts, y, ridge=ridge)
    with pytest.raises(ValueError, match="tolerance is NaN"):
        tt.fit_samples(pts, y, tolerance=np.nan)
    # ridge = 0 and fewer samples than the largest core has unknowns: position 1 (2 x 4 x 2 = 16)
    with pytest.raises(ValueError, match=r"15 samples cannot determine the 16 unknowns of position 1"):
        tt.fit_samples(pts[:15], y[:15], ridge=0.0)
    with pytest.raises(TypeError):
        tt.fit_samples(pts, y, 20)                  # keyword only
    assert tt.fit_info is None


def test_domain_edges_are_inside(no_library):
    """A coordinate exactly on lo or hi passes the checks; max_iter <= 0 then runs nothing and loads nothing."""
    tt = _tt()
    before = [c.copy() for c in tt._coeff_cores]
    pts, y = _good()
    pts[0] = [-1.0, 0.0, 1.0]
    pts[1] = [1.0, 2.0, 3.0]
    for max_iter in (0, -3):
        tt.fit_samples(pts, y, max_iter=max_iter)
        assert tt.fit_info == {"iterations": 0, "residual": [], "n_samples": 40}
        assert all(np.array_equal(a, b) for a, b in zip(before, tt._coeff_cores))


def test_points_are_checked_in_the_user_frame_and_permuted_to_storage(no_library):
    """dim_order = [2, 0, 1]: storage position 0 reads user column 2.  The domain is stored by storage position, the
    points come in the user's order: the check uses the user's frame and the session gets points[:, dim_order]."""
    tt = _tt(dim_order=[2, 0, 1])                    # storage domains (-1,1), (0,2), (1,3) -> user dims 2, 0, 1
    rng = np.random.default_rng(8)
    user_lo, user_hi = np.array([0.0, 1.0, -1.0]), np.array([2.0, 3.0, 1.0])
    pts = user_lo + (user_hi - user_lo) * rng.random((30, 3))
    y = rng.standard_normal(30)
    storage, vals, N = tt._check_samples(pts, y, 1e-12)
    assert N == 30 and storage.flags.c_contiguous and np.array_equal(vals, y)
    assert np.array_equal(storage, pts[:, [2, 0, 1]])
    for k, (a, b) in enumerate(tt.domain):
        assert storage[:, k].min() >= a and storage[:, k].max() <= b
    bad = pts.copy()
    bad[4, 0] = 2.5                                  # inside storage position 0's domain? no: user dimension 0 is [0, 2]
    with pytest.raises(ValueError, match=r"points\[:, 0\] leaves the domain \[0.0, 2.0\]"):
        tt._check_samples(bad, y, 1e-12)
    ident = _tt()
    p2, _ = _good(30)
    assert ident._check_samples(p2, y, 0.0)[0] is not None and np.array_equal(ident._check_samples(p2, y, 0.0)[0], p2)


def test_from_samples_argument_errors_come_before_the_library(no_library):
    pts, y = _good()
    dom = [[-1.0, 1.0], [0.0, 2.0], [1.0, 3.0]]
    for rank in (0, -2, 1.5):
        with pytest.raises(ValueError, match="rank must be a positive integer"):
            ChebyshevTT.from_samples(pts, y, 3, dom, [4, 4, 4], rank=rank)
    with pytest.raises(TypeError):
        ChebyshevTT.from_samples(pts, y, 3, dom, [4, 4, 4])          # rank is required
    with pytest.raises(ValueError, match="must have 3 entries"):
        ChebyshevTT.from_samples(pts, y, 3, dom[:2], [4, 4, 4], rank=2)
    with pytest.raises(ValueError, match="must have 3 entries"):
        ChebyshevTT.from_samples(pts, y, 3, dom, [4, 4], rank=2)
    with pytest.raises(ValueError, match="at least one node"):
        ChebyshevTT.from_samples(pts, y, 3, dom, [4, 0, 4], rank=2)
    with pytest.raises(ValueError, match="lo < hi"):
        ChebyshevTT.from_samples(pts, y, 3, [[-1.0, 1.0], [2.0, 0.0], [1.0, 3.0]], [4, 4, 4], rank=2)
    with pytest.raises(ValueError, match=r"points must have shape \(N, 3\)"):
        ChebyshevTT.from_samples(pts[:, :2], y, 3, dom, [4, 4, 4], rank=2)
    with pytest.raises(ValueError, match="leaves the domain"):
        ChebyshevTT.from_samples(pts + 5.0, y, 3, dom, [4, 4, 4], rank=2)
    with pytest.raises(ValueError, match="ridge"):
        ChebyshevTT.from_samples(pts, y, 3, dom, [4, 4, 4], rank=2, ridge=-1.0)


@pytest.mark.parametrize("n, rank, want", [((6, 7, 5), 2, [1, 2, 2, 1]), ((3, 7, 5), 5, [1, 3, 5, 1]),
                                            ((2, 2, 2, 2), 9, [1, 2, 4, 2, 1]), ((11,), 4, [1, 1])])
def test_from_samples_start_cores_are_the_documented_draws(no_library, n, rank, want):
    """max_iter = 0 leaves the start untouched: bonds by the caps rule, standard normals core by core from k = 0, bit
    for bit, and the object is a built model with method 'samples'."""
    d = len(n)
    rng = np.random.default_rng(1)
    pts, y = rng.random((20, d)), rng.standard_normal(20)
    for seed in (0, 1, 2):
        tt = ChebyshevTT.from_samples(pts, y, d, Domain([(0.0, 1.0)] * d), Ns(list(n)), rank=rank, seed=seed, max_iter=0,
                                      descriptor="cube")
        assert tt.tt_ranks == want
        g = np.random.default_rng(seed)
        for k in range(d):
            assert np.array_equal(tt._coeff_cores[k], g.standard_normal((want[k], n[k], want[k + 1])))
        assert [c.tobytes() for c in tt._coeff_cores] == [c.tobytes() for c in F.start_cores(list(n), rank, seed)]
        assert tt.function is None and tt.method == "samples" and tt.dim_order == list(range(d))
        assert tt.descriptor == "cube" and tt.is_construction_finished() and tt.max_rank == rank
        assert tt.fit_info == {"iterations": 0, "residual": [], "n_samples": 20}


def test_move_centre_matches_the_restatement_up_to_orientation():
    """The product's QR step (LAPACK) and the restatement's (Householder, written out) give the same tensor and the
    same bonds; the factors may differ by signs."""
    rng = np.random.default_rng(9)
    n, ranks = [3, 7, 5], [1, 5, 5, 1]               # the first unfolding holds only 3: the bond shrinks
    cores = [rng.standard_normal((ranks[k], n[k], ranks[k + 1])) for k in range(3)]
    pts = rng.uniform(-1, 1, (25, 3))
    dom = [(-1.0, 1.0)] * 3
    want = F.evaluate(cores, pts, dom)
    a, b = [c.copy() for c in cores], [c.copy() for c in cores]
    for k, to in ((2, 1), (1, 0), (0, 1), (1, 2)):
        tt_mod._fit_move_centre(a, k, to)
        F.move_centre(b, k, to)
        assert [c.shape for c in a] == [c.shape for c in b]
        np.testing.assert_allclose(F.evaluate(a, pts, dom), want, rtol=0, atol=1e-13 * np.max(np.abs(want)))
        np.testing.assert_allclose(F.evaluate(b, pts, dom), want, rtol=0, atol=1e-13 * np.max(np.abs(want)))
    assert [c.shape for c in a] == [(1, 3, 3), (3, 7, 5), (5, 5, 1)]
    with pytest.raises(ValueError):
        tt_mod._fit_move_centre(a, 0, 2)
