"""roots / minimize / maximize without a GPU: the argument rules (reference _validate_calculus_args, checked before any
device call), the batch-argument checks, and the NumPy host restatement that finishes single calls above 64 nodes
(pychebyshev_amd._calculus.roots_1d / optimize_1d) against the reference's values (golden g20)."""
import numpy as np
import pytest

from conftest import golden
import functions as F

from pychebyshev_amd import ChebyshevApproximation, ChebyshevSpline, ChebyshevTT, _calculus
from pychebyshev_amd.barycentric import chebyshev_nodes, compute_barycentric_weights, compute_differentiation_matrix

DOM2 = [[0.0, 1.0], [-2.0, 2.0]]


def _dense2():
    return ChebyshevApproximation.from_values(np.zeros((5, 6)), 2, DOM2, [5, 6])


def _tt_perm():
    g5 = golden("g5_tt_rank16")
    return ChebyshevTT.from_coeff_cores([g5[f"core{k}"] for k in range(10)], [[-1.0, 1.0]] * 9 + [[0.0, 4.0]],
                                        dim_order=[int(v) for v in g5["perm"]])


@pytest.mark.parametrize("method", ["roots", "minimize", "maximize"])
def test_unbuilt_objects_raise_call_build_first(method):
    objs = [ChebyshevApproximation(F.sin_cos_2d, 2, DOM2, [5, 6]),
            ChebyshevSpline(F.sin_cos_2d, 2, DOM2, n_nodes=[5, 6], knots=[[0.5], []]),
            ChebyshevTT(F.sin_cos_2d, 2, DOM2, [5, 6])]
    for obj in objs:
        with pytest.raises(RuntimeError, match="^Call build\\(\\) first$"):
            getattr(obj, method)(0, {1: 0.0})
    for obj in (objs[0], objs[2]):
        with pytest.raises(RuntimeError, match="^Call build\\(\\) first$"):
            getattr(obj, method + "_batch" if method != "roots" else "roots_batch")(0, np.zeros((1, 1)))


CASES = [
    (None, {1: 0.0}, "dim is required for multi-D interpolant"),
    (2, {0: 0.5}, "dim 2 out of range [0, 1]"),
    (-1, {0: 0.5}, "dim -1 out of range [0, 1]"),
    (0, None, "fixed must specify all dims except 0; missing {1}"),
    (0, {}, "fixed must specify all dims except 0; missing {1}"),
    (1, {1: 0.5}, "fixed must specify all dims except 1; missing {0}"),
    (0, {1: 2.5}, "Fixed value 2.5 for dim 1 outside domain [-2.0, 2.0]"),
    (1, {0: -0.1}, "Fixed value -0.1 for dim 0 outside domain [0.0, 1.0]"),
]


@pytest.mark.parametrize("dim,fixed,msg", CASES)
@pytest.mark.parametrize("method", ["roots", "minimize", "maximize"])
def test_validation_messages_match_the_reference(dim, fixed, msg, method):
    for obj in (_dense2(), ChebyshevSpline.from_values([np.zeros((5, 6))] * 2, 2, DOM2, [5, 6], [[0.5], []])):
        with pytest.raises(ValueError) as ei:
            getattr(obj, method)(dim, fixed)
        assert str(ei.value) == msg


def test_one_dimensional_rules():
    c = ChebyshevApproximation.from_values(np.arange(4.0), 1, [[0.0, 1.0]], [4])
    with pytest.raises(ValueError) as ei:
        c.roots(1)
    assert str(ei.value) == "dim must be 0 for 1-D interpolant, got 1"
    with pytest.raises(ValueError) as ei:
        c.minimize(0, {0: 0.5})
    assert str(ei.value) == "fixed must be empty for 1-D interpolant"


def test_tt_validates_in_its_user_frame():
    tt = _tt_perm()              # storage position 9 (domain [0, 4]) holds user dimension perm[9]
    assert tt._user_frame_domain()[tt._dim_order[-1]] == [0.0, 4.0]
    fixed = {k: 0.0 for k in range(10) if k != 0}
    user = tt._dim_order[-1]
    fixed[user] = 3.0                                         # inside [0, 4], outside [-1, 1]
    with pytest.raises(ValueError):                           # refused on the host, before any device call
        tt.minimize(0, {**fixed, user: 4.5})
    with pytest.raises(ValueError) as ei:
        tt.maximize(0, {**fixed, user: -0.5})
    assert str(ei.value) == f"Fixed value -0.5 for dim {user} outside domain [0.0, 4.0]"


def test_batch_argument_errors():
    c = _dense2()
    with pytest.raises(ValueError, match=r"fixed must have shape \(N, 1\), got \(3, 2\)"):
        c.roots_batch(0, np.zeros((3, 2)))
    with pytest.raises(ValueError, match=r"fixed must have shape \(N, 1\), got \(3,\)"):
        c.minimize_batch(1, np.zeros(3))
    with pytest.raises(ValueError, match="dim 2 out of range"):
        c.maximize_batch(2, np.zeros((3, 1)))
    with pytest.raises(TypeError):
        c.roots_batch(None, np.zeros((3, 1)))
    with pytest.raises(ValueError, match=r"Fixed value 3.0 for dim 1 outside domain \[-2.0, 2.0\] \(row 1\)"):
        c.roots_batch(0, np.array([[0.0], [3.0]]))
    big = ChebyshevApproximation.from_values(np.zeros((65, 3)), 2, DOM2, [65, 3])
    with pytest.raises(ValueError, match="65 nodes: the batched solver takes at most 64"):
        big.roots_batch(0, np.zeros((2, 1)))


# ------------------------------------------------------------------ the host restatement
@pytest.fixture(scope="module")
def g20():
    return golden("g20_calculus")


def _rand(g, n):
    import generate_golden_calculus as G
    V = G.rand_fibres(int(g["rand_seed"]), n, int(g["rand_count"]))
    assert np.array_equal(V[0, :4], g[f"rand{n}_head"]), "seeded golden fibres no longer regenerate"
    return V


@pytest.mark.parametrize("n", [8, 16, 32, 64])
def test_host_restatement_matches_reference(g20, n):
    V = _rand(g20, n)
    x = chebyshev_nodes(-1.0, 1.0, n)
    w = compute_barycentric_weights(x)
    D = compute_differentiation_matrix(x, w)
    for i in range(V.shape[0]):
        r = _calculus.roots_1d(V[i], (-1.0, 1.0))
        want = g20[f"rand{n}_roots"][i, :int(g20[f"rand{n}_count"][i])]
        assert r.shape == want.shape
        assert np.all(np.abs(r - want) <= 2e-10)
        scale = np.max(np.abs(V[i]))
        for mode in ("min", "max"):
            val, _ = _calculus.optimize_1d(V[i], x, w, D, (-1.0, 1.0), mode)
            assert abs(val - g20[f"rand{n}_{mode}"][i, 0]) <= 1e-12 * scale


def test_host_restatement_on_named_fibres(g20):
    names = sorted({k[4:-7] for k in g20.files if k.startswith("fib_") and k.endswith("_values")})
    assert len(names) == 15
    for name in names:
        v, dom = g20[f"fib_{name}_values"], tuple(g20[f"fib_{name}_domain"])
        r = _calculus.roots_1d(v, dom)
        want = g20[f"fib_{name}_roots"]
        assert r.shape == want.shape, name
        assert np.all(np.abs(r - want) <= 1e-10 * (dom[1] - dom[0])), name


def test_matrix_dct_puts_no_spurious_root_inside_the_window_for_constants():
    """The reference's FFT DCT gives exact zeros for constant data, so its series trims to degree 0; the matrix DCT
    leaves ~1e-15 coefficients whose colleague matrix has spurious eigenvalues -- just outside [-1, 1] (|t| ~ 1.036).
    The exact-zero trim is kept; this guards that the window still excludes them."""
    for n in range(1, 129):
        for c in (5.0, -1.0, 1e-3):
            assert _calculus.roots_1d(np.full(n, c), (-1.0, 1.0)).size == 0, (n, c)


@pytest.mark.parametrize("dom", [(-1.0, 1.0), (1e6, 1e6 + 1.0), (-1e-3, 1e-3), (-2.0, 3.0)])
def test_restatement_returns_the_endpoints_of_lobatto_rows_exactly(dom):
    """A root within 1e-10 of an end is that end, from either side: (1 - x^2) U_(n-3) has roots at both ends, and the
    restatement -- the host route of fibres above 64 nodes -- returns lo and hi themselves on any interval, as the
    device solver does."""
    import calc_fibres as CF

    def solve(n):
        r = _calculus.roots_1d(CF.lobatto_row(n), dom)
        return r, r.size
    missed = CF.missed_endpoints(dom, solve, list(range(4, 65)) + [65, 96, 128])
    assert not missed, missed
