"""invert_batch / roots(level=) on the host: the argument rules of the four classes, checked before any device call,
and the NumPy restatement _calculus.invert_1d on constructed fibres.  No GPU is used: the model objects are built
without a device handle and the device entry is replaced by a recorder."""
import inspect
import math

import numpy as np
import pytest

import calc_fibres as CF
import invert_fibres as IF

from pychebyshev_amd import ChebyshevApproximation, ChebyshevSlider, ChebyshevSpline, ChebyshevTT, _calculus

DOM = (-1.0, 1.0)
NS = (1, 2, 3, 17, 64)
CLASSES = (ChebyshevApproximation, ChebyshevSpline, ChebyshevSlider, ChebyshevTT)


# ------------------------------------------------------------------ argument rules
@pytest.mark.parametrize("cls", CLASSES)
def test_signatures(cls):
    r = inspect.signature(cls.roots).parameters["level"]
    assert r.kind is inspect.Parameter.KEYWORD_ONLY and r.default == 0.0
    rb = inspect.signature(cls.roots_batch).parameters["level"]
    assert rb.kind is inspect.Parameter.KEYWORD_ONLY and rb.default is None
    assert list(inspect.signature(cls.invert_batch).parameters) == ["self", "dim", "fixed", "targets"]
    for name in ("invert_batch", "roots_batch", "roots"):
        assert "level" in getattr(cls, name).__doc__ or "status" in getattr(cls, name).__doc__


def test_targets_shape_and_finiteness():
    assert np.array_equal(_calculus.validate_targets(0.5, 3), [0.5, 0.5, 0.5])
    assert _calculus.validate_targets([1.0, 2.0], 2).dtype == np.float64
    with pytest.raises(ValueError, match=r"targets must be a scalar or have shape \(3,\), got \(2,\)"):
        _calculus.validate_targets([1.0, 2.0], 3)
    with pytest.raises(ValueError, match=r"targets must be a scalar or have shape \(2,\), got \(2, 1\)"):
        _calculus.validate_targets([[1.0], [2.0]], 2)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match=r"targets must be finite, got .* \(row 1\)"):
            _calculus.validate_targets([0.0, bad], 2)
        with pytest.raises(ValueError, match=r"level must be finite, got .* \(row 0\)"):
            _calculus.validate_level(bad, 4)
    with pytest.raises(ValueError, match=r"level must be a scalar or have shape \(2,\)"):
        _calculus.validate_level([1.0, 2.0, 3.0], 2)


def test_level_zero_is_no_level():
    assert _calculus.validate_level(None, 5) is None
    assert _calculus.validate_level(0.0, 5) is None
    assert _calculus.validate_level(-0.0, 5) is None
    assert _calculus.validate_level(0, 5) is None
    assert np.array_equal(_calculus.validate_level(0.25, 2), [0.25, 0.25])
    assert np.array_equal(_calculus.validate_level([0.0, 0.0], 2), [0.0, 0.0])      # an array is a request


def _host_model(n=5):
    """A built 2-D approximation with recorders in place of its two device entries."""
    m = ChebyshevApproximation(lambda p, _: p[0] + p[1], 2, [[-1.0, 1.0], [0.0, 2.0]], [n, n])
    m.nodes = [np.zeros(n), np.zeros(n)]
    m.tensor_values = np.zeros((n, n))                      # "built", as the argument checks see it
    calls = []
    m._calculus_batch = lambda dim, rows, mode: calls.append(("calculus", dim, rows.shape, mode)) or "old"
    m._solve_batch = lambda dim, rows, t, method: calls.append(("solve", dim, rows.shape, t.copy(), method)) or "new"
    return m, calls


def test_level_zero_takes_the_path_without_a_level():
    m, calls = _host_model()
    fixed = np.array([[0.5], [1.5]])
    assert m.roots_batch(0, fixed) == "old" and m.roots_batch(0, fixed, level=None) == "old"
    assert m.roots_batch(0, fixed, level=0.0) == "old"
    assert [c[0] for c in calls] == ["calculus"] * 3 and all(c[3] == 0 for c in calls)
    assert m.roots_batch(0, fixed, level=0.3) == "new"
    assert calls[-1][0] == "solve" and np.array_equal(calls[-1][3], [0.3, 0.3]) and calls[-1][4] == 0
    assert m.invert_batch(1, np.array([[0.0]]), [1.25]) == "new"
    assert calls[-1][1] == 1 and np.array_equal(calls[-1][3], [1.25]) and calls[-1][4] == 1


def test_bad_arguments_are_refused_before_any_call():
    m, calls = _host_model()
    fixed = np.array([[0.5], [1.5]])
    with pytest.raises(ValueError, match="targets must be a scalar or have shape"):
        m.invert_batch(0, fixed, [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="targets must be finite"):
        m.invert_batch(0, fixed, [1.0, np.nan])
    with pytest.raises(ValueError, match="level must be finite"):
        m.roots_batch(0, fixed, level=np.inf)
    with pytest.raises(ValueError, match="level must be finite"):
        m.roots(0, {1: 0.5}, level=np.nan)
    with pytest.raises(ValueError, match="fixed must have shape"):
        m.invert_batch(0, np.zeros((2, 2)), 0.0)
    with pytest.raises(ValueError, match="outside domain"):
        m.invert_batch(0, np.array([[5.0]]), 0.0)
    assert not calls


def test_more_than_64_nodes_are_refused():
    m, calls = _host_model(65)
    with pytest.raises(ValueError, match="has 65 nodes: the batched solver takes at most 64"):
        m.invert_batch(0, np.array([[0.5]]), 0.0)
    with pytest.raises(ValueError, match="has 65 nodes: the batched solver takes at most 64"):
        m.roots_batch(0, np.array([[0.5]]), level=0.5)
    assert not calls


# ------------------------------------------------------------------ invert_1d on constructed fibres
def _grid(n):
    x, w, _ = CF.grid(n, *DOM)
    return x, w


@pytest.mark.parametrize("n", [n for n in NS if n >= 2])
def test_linear_fibre_has_its_closed_form_root(n):
    x, w = _grid(n)
    for slope, icpt, t in ((2.0, 0.5, 0.75), (-3.0, 1.0, -0.5), (1.0, 0.0, 0.3)):
        got, status = _calculus.invert_1d(slope * x + icpt, x, w, DOM, t)
        assert status == 1
        assert abs(got - (t - icpt) / slope) <= 1e-12 * (DOM[1] - DOM[0]), (n, got)


@pytest.mark.parametrize("n", [n for n in NS if n >= 2])
@pytest.mark.parametrize("name", ["tanh", "exp"])
def test_strictly_monotone_fibre_has_status_one(n, name):
    x, w = _grid(n)
    f = (lambda u: np.tanh(3.0 * u)) if name == "tanh" else np.exp
    v = f(x)
    for frac in (0.03, 0.31, 0.5, 0.77, 0.98):
        t = float(v[0] + frac * (v[-1] - v[0]))
        got, status = _calculus.invert_1d(v, x, w, DOM, t)
        assert status == 1, (n, name, frac, status)
        assert DOM[0] <= got <= DOM[1]
        with np.errstate(all="ignore"):
            back = _calculus._bary_rows(v[None], x, w, np.array([got]))[0]
        assert abs(back - t) <= 1e-12 * float(np.max(np.abs(v))), (n, name, frac, back - t)


@pytest.mark.parametrize("n", [n for n in NS if n >= 2])
def test_chebyshev_polynomials_at_level_0p3(n):
    """T_k = 0.3 has the k solutions cos((+-arccos 0.3 + 2 pi m) / k).  status counts crossings on the knots, so it is k
    whenever the knots separate the solutions -- every k here but a few with k close to n = 64 (k = 52 is one), where two
    solutions share a node interval and are invisible by definition: there status is the number of segments that hold
    an odd number of the closed-form solutions, still independent of the solver.  x is the lowest solution, or, where
    solutions share a segment, one of the lowest segment that holds an odd number of them."""
    x, w = _grid(n)
    knots = np.concatenate([[DOM[0]], x, [DOM[1]]])
    separated = 0
    for k in range(1, n):
        v = np.cos(k * np.arccos(x))
        got, status = _calculus.invert_1d(v, x, w, DOM, 0.3)
        th = math.acos(0.3)
        sols = np.array(sorted({math.cos(a / k) for m in range(k + 1) for a in (th + 2.0 * math.pi * m, -th + 2.0 * math.pi * m)
                                if 0.0 <= a <= k * math.pi}))
        assert sols.size == k
        per_segment = np.histogram(sols, bins=knots)[0]
        if per_segment.max() <= 1:
            separated += 1
            assert status == k, (n, k, status)
        else:
            assert status == int(np.sum(per_segment % 2 == 1)) < k, (n, k, status, per_segment)
        if per_segment.max() <= 1:
            want = sols[:1]                                             # the lowest solution
        else:                                                           # a solution of the lowest segment that brackets
            i = int(np.nonzero(per_segment % 2 == 1)[0][0])
            want = sols[(sols > knots[i]) & (sols < knots[i + 1])]
        assert np.min(np.abs(got - want)) <= 1e-12 * (DOM[1] - DOM[0]), (n, k, got, want)
    assert separated == n - 1 or n == 64, (n, separated)
    assert separated >= (n - 1) * 3 // 4


@pytest.mark.parametrize("n", NS)
def test_target_outside_the_range_is_not_reached(n):
    x, w = _grid(n)
    v = np.tanh(3.0 * x) if n > 1 else np.array([0.25])
    for t in (5.0, -5.0):
        got, status = _calculus.invert_1d(v, x, w, DOM, t)
        assert status == 0 and math.isnan(got)


@pytest.mark.parametrize("n", NS)
def test_target_equal_to_a_node_value_returns_the_node(n):
    x, w = _grid(n)
    v = np.exp(x)
    for i in sorted({0, n // 2, n - 1}):
        got, status = _calculus.invert_1d(v, x, w, DOM, float(v[i]))
        if n == 1:                                  # one node: the constant fibre equal to its target (below)
            assert got == DOM[0] and status == 3
        else:
            assert got == x[i] and status == 1, (n, i, got, status)


@pytest.mark.parametrize("n", NS)
def test_constant_equal_to_its_target(n):
    """status n + 2 and x = lo follow from the rule when the barycentric sums at the two ends return the constant
    itself: with a power of two (or zero) every product t_j c is exact and num = c den bit for bit.  Another constant
    may come back one ulp off at an end; that end then does not count, and status is n, n + 1 or n + 2 with x = lo or
    the first node.  Documented, not special-cased."""
    x, w = _grid(n)
    for c in (1.0, 0.0, 0.5, -2.0):
        got, status = _calculus.invert_1d(np.full(n, c), x, w, DOM, c)
        assert status == n + 2 and got == DOM[0], (n, c, status, got)
    got, status = _calculus.invert_1d(np.full(n, 1.5), x, w, DOM, 1.5)
    assert status in (n, n + 1, n + 2) and got in (DOM[0], x[0]), (n, status, got)


@pytest.mark.parametrize("n", NS)
def test_non_finite_fibre_or_target(n):
    x, w = _grid(n)
    v = np.exp(x)
    for bad in (np.nan, np.inf, -np.inf):
        got, status = _calculus.invert_1d(v, x, w, DOM, bad)
        assert status == -1 and math.isnan(got)
        u = v.copy()
        u[n // 2] = bad
        got, status = _calculus.invert_1d(u, x, w, DOM, 1.0)
        assert status == -1 and math.isnan(got)


@pytest.mark.parametrize("dom", [(-1.0, 1.0), (-2.0, 3.0)])
def test_solutions_at_and_next_to_zero(dom):
    """Strictly increasing fibres against t = 0, t = +-1e-15 ... +-1e-300 and t = p(0) from another summation order,
    on domains that contain 0, at every n = 2 .. 64 (even n: no node at 0; odd n: 0 is a node, and a target one step
    off its value meets the jump of the within-1e-14 rule): status 1 on every row, p(x) = t within 1e-13 max|v|, x
    within 1e-14 max(|lo|, |hi|) of 0 where the solution is there, and far fewer evaluations than the cap -- a stop relative to |x| alone never ends
    here.  The largest count is printed for DESIGN."""
    scale = max(abs(dom[0]), abs(dom[1]))
    worst = 0
    for n in range(2, 65):
        V, t = IF.near_zero(n, dom)
        x, status, iters = IF.near_zero_reference(n, dom)
        assert np.all(status == 1), (dom, n, status, t[status != 1])
        nodes, w, _ = CF.grid(n, *dom)
        with np.errstate(all="ignore"):
            back = _calculus._bary_rows(np.asarray(V), nodes, w, x)
        assert np.all(np.abs(back - t) <= 1e-13 * np.max(np.abs(V), axis=1)), (dom, n, back - t)
        last = np.arange(V.shape[0]) % (len(IF.NEAR_ZERO_TARGETS) + 1) == len(IF.NEAR_ZERO_TARGETS)
        assert np.all(np.abs(x[last]) <= 1e-14 * scale), (dom, n, x[last])         # t = p(0): the solution is 0
        if dom[0] == -dom[1]:                               # odd fibres on a symmetric grid: p is odd, every solution is near 0
            assert np.all(np.abs(x) <= 1e-14 * scale + 2.0 * np.abs(t)), (dom, n, x)
        worst = max(worst, int(iters.max()))
    print(f"\nsolutions at and next to 0 on {dom}: largest iteration count {worst} of {_calculus.INVERT_MAX_ITERS}")
    assert worst <= _calculus.INVERT_MAX_ITERS // 2


def test_the_cap_covers_three_steps_per_halving_down_to_the_floor():
    halvings = 1 + 10 + 52                                  # from 2 max(|lo|, |hi|) to 2^-10 eps max(|lo|, |hi|)
    assert _calculus.INVERT_FLOOR == 2.0 ** -10 and 3 * halvings < _calculus.INVERT_MAX_ITERS


def test_rows_do_not_depend_on_their_batch():
    n = 17
    x, w = _grid(n)
    V = CF.noise(n)[1]
    t = np.linspace(-0.5, 0.5, V.shape[0])
    X, S = _calculus.invert_rows(V, x, w, DOM, t)
    for r in (0, 7, V.shape[0] - 1):
        got, status = _calculus.invert_1d(V[r], x, w, DOM, t[r])
        assert status == S[r] and np.array_equal(got, X[r], equal_nan=True)


def test_merge_restatement():
    x = np.array([[np.nan, 0.2, 0.1, np.nan], [0.6, 0.5, np.nan, np.nan]])
    s = np.array([[0, 2, 1, -1], [1, 1, 0, 1]])
    mx, ms = _calculus.merge_inversions(x, s)
    assert np.array_equal(ms, [1, 3, 1, -1])
    assert np.array_equal(mx, [0.6, 0.2, 0.1, np.nan], equal_nan=True)
    mx, ms = _calculus.merge_inversions(np.full((2, 1), np.nan), np.zeros((2, 1), dtype=int))
    assert ms[0] == 0 and np.isnan(mx[0])
