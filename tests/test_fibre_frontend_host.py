"""The front end the four classes share for the operations along one dimension (``_calculus.FibreCalculusMixin``), without
a GPU: a host-built model of each class with recorders in place of its two device entries, as
``test_invert_host._host_model`` does for the dense class.  Every class must dispatch the same way, and must refuse bad
arguments with the same exception and message before either entry is reached.

The models are 2-D with ``n`` nodes along user dimension 0 and 5 along dimension 1, on ``[-1, 1] x [0, 2]``: the two
dimensions differ in domain and (for ``n = 65``) in node count, so a class that looked them up in the wrong frame would
refuse the wrong dimension.  The tensor train is stored with ``dim_order = [1, 0]``."""
import re

import numpy as np
import pytest

from pychebyshev_amd import ChebyshevApproximation, ChebyshevSlider, ChebyshevSpline, ChebyshevTT

DOM = [[-1.0, 1.0], [0.0, 2.0]]
KINDS = ("dense", "spline", "slider", "tt")
BATCH = ("roots_batch", "invert_batch", "minimize_batch", "maximize_batch")


def _fn(x, _=None):
    return x[0] + x[1]


def _model(kind, n=5, built=True):
    if kind == "dense":
        m = ChebyshevApproximation.from_values(np.zeros((n, 5)), 2, DOM, [n, 5]) if built else \
            ChebyshevApproximation(_fn, 2, DOM, [n, 5])
    elif kind == "spline":
        m = ChebyshevSpline.from_values([np.zeros((n, 5))] * 2, 2, DOM, [n, 5], [[0.25], []]) if built else \
            ChebyshevSpline(_fn, 2, DOM, [n, 5], knots=[[0.25], []])
    elif kind == "slider":
        m = ChebyshevSlider(_fn, 2, DOM, [n, 5], partition=[[0], [1]], pivot_point=[0.0, 1.0])
        if built:
            m.build(verbose=False)
    else:                                                   # storage position 0 holds user dimension 1
        m = ChebyshevTT.from_coeff_cores([np.zeros((1, 5, 1)), np.zeros((1, n, 1))], [DOM[1], DOM[0]], dim_order=[1, 0]) \
            if built else ChebyshevTT(_fn, 2, DOM, [n, 5])
    calls = []

    def calculus_batch(dim, rows, mode):
        calls.append(("calculus", dim, rows.shape, mode))
        return ("roots", "counts") if mode == 0 else ("values", "locations", "counts")

    def solve_batch(dim, rows, targets, method):
        calls.append(("solve", dim, rows.shape, targets.copy(), method))
        return "solved"

    m._calculus_batch, m._solve_batch = calculus_batch, solve_batch
    return m, calls


def _call(m, name, dim, fixed):
    return getattr(m, name)(dim, fixed, 0.5) if name == "invert_batch" else getattr(m, name)(dim, fixed)


# ------------------------------------------------------------------ dispatch
@pytest.mark.parametrize("kind", KINDS)
def test_roots_batch_without_a_level_is_the_calculus_entry(kind):
    m, calls = _model(kind)
    fixed = np.array([[0.5], [1.5]])
    assert m.roots_batch(0, fixed) == ("roots", "counts")
    for level in (None, 0.0, -0.0):
        assert m.roots_batch(0, fixed, level=level) == ("roots", "counts")
    assert calls == [("calculus", 0, (2, 1), 0)] * 4


@pytest.mark.parametrize("kind", KINDS)
def test_roots_batch_with_a_level_is_the_solve_entry_method_0(kind):
    m, calls = _model(kind)
    fixed = np.array([[0.5], [1.5]])
    assert m.roots_batch(0, fixed, level=0.3) == "solved"
    assert m.roots_batch(np.int64(1), np.array([[0.0], [-1.0]]), level=[0.1, -0.2]) == "solved"
    assert [c[0] for c in calls] == ["solve", "solve"]
    assert calls[0][1:3] == (0, (2, 1)) and np.array_equal(calls[0][3], [0.3, 0.3]) and calls[0][4] == 0
    assert calls[1][1:3] == (1, (2, 1)) and np.array_equal(calls[1][3], [0.1, -0.2]) and calls[1][4] == 0
    assert calls[0][3].dtype == np.float64 and type(calls[1][1]) is int


@pytest.mark.parametrize("kind", KINDS)
def test_invert_batch_is_the_solve_entry_method_1(kind):
    m, calls = _model(kind)
    assert m.invert_batch(1, np.array([[0.0], [1.0], [-1.0]]), [1.25, 0.5, 0.0]) == "solved"
    assert m.invert_batch(0, np.array([[2.0]]), 0.75) == "solved"
    assert calls[0][:3] == ("solve", 1, (3, 1)) and np.array_equal(calls[0][3], [1.25, 0.5, 0.0]) and calls[0][4] == 1
    assert calls[1][:3] == ("solve", 0, (1, 1)) and np.array_equal(calls[1][3], [0.75]) and calls[1][4] == 1


@pytest.mark.parametrize("kind", KINDS)
def test_extremum_batches_are_modes_1_and_2_without_the_counts(kind):
    m, calls = _model(kind)
    fixed = np.array([[0.5], [1.5]])
    assert m.minimize_batch(0, fixed) == ("values", "locations")
    assert m.maximize_batch(0, fixed) == ("values", "locations")
    assert calls == [("calculus", 0, (2, 1), 1), ("calculus", 0, (2, 1), 2)]


# ------------------------------------------------------------------ refusals, before either entry is reached
@pytest.mark.parametrize("name", BATCH)
@pytest.mark.parametrize("kind", KINDS)
def test_dim_type_and_range(kind, name):
    m, calls = _model(kind)
    fixed = np.array([[0.5]])
    with pytest.raises(TypeError, match=r"^dim must be an int, got float$"):
        _call(m, name, 0.0, fixed)
    with pytest.raises(TypeError, match=r"^dim must be an int, got bool$"):
        _call(m, name, True, fixed)
    with pytest.raises(TypeError, match=r"^dim must be an int, got NoneType$"):
        _call(m, name, None, fixed)
    with pytest.raises(ValueError, match=r"^dim 2 out of range \[0, 1\]$"):
        _call(m, name, 2, fixed)
    with pytest.raises(ValueError, match=r"^dim -1 out of range \[0, 1\]$"):
        _call(m, name, -1, fixed)
    assert not calls


@pytest.mark.parametrize("name", BATCH)
@pytest.mark.parametrize("kind", KINDS)
def test_fixed_shape_and_domain(kind, name):
    m, calls = _model(kind)
    with pytest.raises(ValueError, match=r"^fixed must have shape \(N, 1\), got \(2, 2\)$"):
        _call(m, name, 0, np.zeros((2, 2)))
    with pytest.raises(ValueError, match=r"^fixed must have shape \(N, 1\), got \(2,\)$"):
        _call(m, name, 0, np.zeros(2))
    # -0.5 lies in the domain of dimension 0 but not in that of dimension 1, the column of a call along 0; 1.5 the reverse
    with pytest.raises(ValueError, match=re.escape("Fixed value -0.5 for dim 1 outside domain [0.0, 2.0] (row 1)") + "$"):
        _call(m, name, 0, np.array([[0.5], [-0.5], [-0.75]]))
    with pytest.raises(ValueError, match=re.escape("Fixed value 1.5 for dim 0 outside domain [-1.0, 1.0] (row 2)") + "$"):
        _call(m, name, 1, np.array([[0.5], [-0.5], [1.5]]))
    assert not calls


@pytest.mark.parametrize("name", BATCH)
@pytest.mark.parametrize("kind", KINDS)
def test_65_nodes_are_refused_along_their_dimension_only(kind, name):
    m, calls = _model(kind, 65)
    with pytest.raises(ValueError, match=re.escape("dimension 0 has 65 nodes: the batched solver takes at most 64 "
                                                   "(the single-row calls handle more on the host)") + "$"):
        _call(m, name, 0, np.array([[0.5]]))
    assert not calls
    _call(m, name, 1, np.array([[0.5]]))                   # 5 nodes along dimension 1
    assert len(calls) == 1 and calls[0][1] == 1


@pytest.mark.parametrize("kind", KINDS)
def test_non_finite_targets_and_levels(kind):
    m, calls = _model(kind)
    fixed = np.array([[0.5], [1.5]])
    for bad, text in ((np.nan, "nan"), (np.inf, "inf"), (-np.inf, "-inf")):
        with pytest.raises(ValueError, match=rf"^targets must be finite, got {text} \(row 1\)$"):
            m.invert_batch(0, fixed, [1.0, bad])
        with pytest.raises(ValueError, match=rf"^targets must be finite, got {text} \(row 0\)$"):
            m.invert_batch(0, fixed, bad)
        with pytest.raises(ValueError, match=rf"^level must be finite, got {text} \(row 0\)$"):
            m.roots_batch(0, fixed, level=bad)
        with pytest.raises(ValueError, match=rf"^level must be finite, got {text} \(row 1\)$"):
            m.roots_batch(0, fixed, level=[0.0, bad])
        with pytest.raises(ValueError, match=rf"^level must be finite, got {text} \(row 0\)$"):
            m.roots(0, {1: 0.5}, level=bad)
    with pytest.raises(ValueError, match=r"^targets must be a scalar or have shape \(2,\), got \(3,\)$"):
        m.invert_batch(0, fixed, [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match=r"^level must be a scalar or have shape \(2,\), got \(3,\)$"):
        m.roots_batch(0, fixed, level=[1.0, 2.0, 3.0])
    assert not calls


@pytest.mark.parametrize("kind", KINDS)
def test_an_unbuilt_model_says_build_first(kind):
    m, calls = _model(kind, built=False)
    for name in BATCH:
        with pytest.raises(RuntimeError, match=r"^Call build\(\) first$"):
            _call(m, name, 0, np.array([[0.5]]))
        with pytest.raises(RuntimeError, match=r"^Call build\(\) first$"):      # before the look at dim
            _call(m, name, 7.5, np.array([[0.5]]))
    for single in (m.roots, m.minimize, m.maximize):
        with pytest.raises(RuntimeError, match=r"^Call build\(\) first$"):
            single(0, {1: 0.5})
    with pytest.raises(RuntimeError, match=r"^Call build\(\) first$"):
        m.roots(0, {1: 0.5}, level=0.25)
    assert not calls


@pytest.mark.parametrize("name", BATCH)
def test_spline_pieces_that_share_an_interval_must_share_its_grid(name):
    """The spline's own refusal, after the shared ones: 2 x 2 pieces, and the two pieces of interval 0 of dimension 0 have
    5 and 6 nodes there.  Along dimension 1 every piece has 5 nodes, so that call goes through."""
    edges = ([-1.0, 0.25, 1.0], [0.0, 1.0, 2.0])
    pieces = [ChebyshevApproximation.from_values(np.zeros((n0, 5)), 2, [[edges[0][i], edges[0][i + 1]], [edges[1][j], edges[1][j + 1]]],
                                                 [n0, 5])
              for (i, j), n0 in zip(((0, 0), (0, 1), (1, 0), (1, 1)), (5, 6, 5, 5))]
    m = ChebyshevSpline.from_pieces(pieces, 2, DOM, [[0.25], [1.0]])
    calls = []
    m._calculus_batch = lambda dim, rows, mode: calls.append(("calculus", dim)) or ("a", "b", "c")
    m._solve_batch = lambda dim, rows, t, method: calls.append(("solve", dim)) or "solved"
    with pytest.raises(ValueError, match=re.escape("pieces that share an interval of dimension 0 differ in their node counts there: "
                                                   "the batched solver needs one grid per interval (the single-row calls handle "
                                                   "this)") + "$"):
        _call(m, name, 0, np.array([[0.5]]))
    with pytest.raises(ValueError, match=r"^fixed must have shape \(N, 1\), got \(1, 2\)$"):     # the shared checks come first
        _call(m, name, 0, np.zeros((1, 2)))
    assert not calls
    _call(m, name, 1, np.array([[0.5]]))
    assert len(calls) == 1 and calls[0][1] == 1
