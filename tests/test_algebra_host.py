"""Arithmetic operators on the host side (no GPU): operand checks and their messages, the scalar rule, the
combined value tensors, the attributes of a result, persistence of a combined model, the scalar TT operators,
the d = 1 TT sum and the argument checks of ``reorder``."""
import math
import os
import pickle

import numpy as np
import pytest

import functions as F
from pychebyshev_amd import ChebyshevApproximation, ChebyshevSlider, ChebyshevSpline, ChebyshevTT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dense(seed=0, shape=(5, 6), domain=None, mdo=2):
    t = np.random.default_rng(seed).standard_normal(shape)
    domain = domain or [[-1.0, 1.0], [0.0, 2.0]][:len(shape)]
    return ChebyshevApproximation.from_values(t, len(shape), domain, list(shape), max_derivative_order=mdo)


def _spline(fn=F.kink_2d):
    case = F.SPLINE_CASES["b"]
    sp = ChebyshevSpline(fn, 2, case["domain"], n_nodes=[list(v) for v in case["n_nodes"]], knots=case["knots"])
    sp.build(verbose=False)
    return sp


def _slider(fn=F.sin_sum_3d, pivot=(0.0, 0.0, 0.0), partition=([0], [1], [2])):
    sl = ChebyshevSlider(fn, 3, [[-1.0, 1.0]] * 3, [7, 8, 9], partition=[list(g) for g in partition],
                         pivot_point=list(pivot))
    sl.build(verbose=False)
    return sl


# ------------------------------------------------------------------ compatibility checks
@pytest.mark.parametrize("other, exc, match", [
    (lambda: _dense(1, (5, 7)), ValueError, r"Node count mismatch: \[5, 6\] vs \[5, 7\]"),
    (lambda: _dense(1, (5, 6), [[-1.0, 1.0], [0.0, 3.0]]), ValueError, "Domain mismatch"),
    (lambda: _dense(1, (5,), [[-1.0, 1.0]]), ValueError, "Dimension mismatch: 2 vs 1"),
    (lambda: _dense(1, mdo=3), ValueError, "max_derivative_order mismatch: 2 vs 3"),
])
def test_dense_incompatible_operands(other, exc, match):
    a, b = _dense(0), other()
    for op in (lambda: a + b, lambda: a - b):
        with pytest.raises(exc, match=match):
            op()


def test_unbuilt_operands():
    a = _dense(0)
    raw = ChebyshevApproximation(math.sin, 2, [[-1.0, 1.0], [0.0, 2.0]], [5, 6])
    with pytest.raises(RuntimeError, match="Right operand is not built. Call build\\(\\) first."):
        a + raw
    with pytest.raises(RuntimeError, match="Left operand is not built"):
        raw + a
    sp = ChebyshevSpline(F.kink_2d, 2, [[-1.0, 1.0], [0.0, 1.0]], n_nodes=[5, 5], knots=[[0.2], [0.5]])
    with pytest.raises(RuntimeError, match="Left operand is not built"):
        sp + _spline()


def test_mixed_types_and_in_place_type_error():
    a = _dense(0)
    with pytest.raises(TypeError):
        a + _spline()
    with pytest.raises(TypeError, match="Cannot combine ChebyshevApproximation with int; operands must be the same type."):
        a += 3


def test_spline_and_slider_specific_checks():
    case = F.SPLINE_CASES["b"]
    other = ChebyshevSpline(F.kink_2d, 2, case["domain"], n_nodes=[list(v) for v in case["n_nodes"]],
                            knots=[[0.3], [0.5]])
    other.build(verbose=False)
    with pytest.raises(ValueError, match=r"Knot mismatch: \[\[0.2\], \[0.5\]\] vs \[\[0.3\], \[0.5\]\]"):
        _spline() + other
    with pytest.raises(ValueError, match="Partition mismatch"):
        _slider() + _slider(partition=([0, 1], [2]))
    with pytest.raises(ValueError, match="Pivot point mismatch"):
        _slider() - _slider(pivot=(0.1, 0.0, 0.0))


# ------------------------------------------------------------------ scalar rule
@pytest.mark.parametrize("make", [_dense, _spline, _slider])
def test_non_scalars_are_not_implemented(make):
    obj = make()
    assert obj.__mul__(np.array([2.0])) is NotImplemented      # NumPy then broadcasts the scalar product itself
    for bad in ("2", [2.0], None, 1 + 2j):
        assert obj.__mul__(bad) is NotImplemented
        assert obj.__truediv__(bad) is NotImplemented
        assert obj.__imul__(bad) is NotImplemented
        with pytest.raises(TypeError):
            obj * bad
        with pytest.raises(TypeError):
            obj / bad
    assert obj.__add__(3.0) is NotImplemented
    assert not hasattr(type(obj), "__radd__")
    with pytest.raises(TypeError):
        3.0 + obj
    with pytest.raises(ZeroDivisionError):
        obj / 0
    with pytest.raises(ZeroDivisionError):
        obj /= 0.0


def test_numpy_scalars_accepted_bit_for_bit():
    a = _dense(0)
    for s in (np.float64(1.5), np.float32(0.25), np.int64(3), np.int8(-2), 7, 0.5):
        assert np.array_equal((a * s).tensor_values, a.tensor_values * float(s))
        assert np.array_equal((s * a).tensor_values, a.tensor_values * float(s))
        assert np.array_equal((a / s).tensor_values, a.tensor_values * (1.0 / float(s)))


# ------------------------------------------------------------------ combined tensors, attributes
def test_dense_tensors_bit_for_bit():
    a, b = _dense(0), _dense(1)
    ta, tb = a.tensor_values.copy(), b.tensor_values.copy()
    assert np.array_equal((a + b).tensor_values, ta + tb)
    assert np.array_equal((a - b).tensor_values, ta - tb)
    assert np.array_equal((-a).tensor_values, ta * -1.0)
    assert np.array_equal((2.5 * a - b / 3).tensor_values, ta * 2.5 - tb * (1.0 / 3.0))
    c = _dense(0)
    before = c.tensor_values
    c += b
    c *= 0.5
    c -= b
    c /= 4
    assert c.tensor_values is not before and np.array_equal(before, ta)        # rebound, never written in place
    assert np.array_equal(c.tensor_values, (((ta + tb) * 0.5) - tb) * 0.25)
    assert np.array_equal(a.tensor_values, ta) and np.array_equal(b.tensor_values, tb)


def test_spline_and_slider_tensors_bit_for_bit():
    a, b = _spline(), _spline(lambda x, _=None: math.cos(x[0]) * x[1])
    r = a - 2 * b
    for p, q, s in zip(a._pieces, b._pieces, r._pieces):
        assert np.array_equal(s.tensor_values, p.tensor_values - q.tensor_values * 2.0)
    sa, sb = _slider(), _slider(lambda x, _=None: x[0] * x[1] + x[2] ** 2)
    r = sa + sb / 2
    for p, q, s in zip(sa.slides, sb.slides, r.slides):
        assert np.array_equal(s.tensor_values, p.tensor_values + q.tensor_values * 0.5)
    assert r.pivot_value == sa.pivot_value + sb.pivot_value * 0.5
    old = [s.tensor_values for s in sa.slides]
    pv = sa.pivot_value
    sa -= sb
    assert sa.pivot_value == pv - sb.pivot_value
    assert all(s.tensor_values is not o for s, o in zip(sa.slides, old))


def test_result_attributes():
    a, b = _dense(0), _dense(1)
    a.set_descriptor("trade a")
    a.build_time = 3.0
    a.n_evaluations = 30
    a._cached_error_estimate = 1.0
    r = a + b
    assert r.function is None and r.build_time == 0.0 and r.n_evaluations == 0 and r.descriptor == ""
    assert r._cached_error_estimate is None
    assert r.nodes is a.nodes and r.weights is a.weights and r.diff_matrices is a.diff_matrices
    a += b
    assert a._cached_error_estimate is None
    sp = _spline() * 2
    assert sp.function is None and sp.build_time == 0.0 and sp.descriptor == "" and sp.total_build_evals == 0
    sl = _slider() + _slider()
    assert sl.function is None and sl.descriptor == "" and sl._cached_error_estimate is None


def test_pickle_and_pcb_round_trips(tmp_path):
    r = 2.5 * _dense(0) - _dense(1) / 3
    r.save(tmp_path / "r.pkl")
    r.save(tmp_path / "r.pcb", format="binary")
    for path in ("r.pkl", "r.pcb"):
        back = ChebyshevApproximation.load(tmp_path / path)
        assert np.array_equal(back.tensor_values, r.tensor_values)
    sp = _spline() - _spline(lambda x, _=None: x[0] + x[1])
    back = pickle.loads(pickle.dumps(sp))
    assert all(np.array_equal(p.tensor_values, q.tensor_values) for p, q in zip(back._pieces, sp._pieces))
    sl = _slider() * 3
    back = pickle.loads(pickle.dumps(sl))
    assert back.pivot_value == sl.pivot_value


# ------------------------------------------------------------------ TT: scalars, d = 1, reorder arguments
def _tt(seed=0, shape=((1, 5, 3), (3, 6, 2), (2, 4, 1))):
    rng = np.random.default_rng(seed)
    return ChebyshevTT.from_coeff_cores([rng.standard_normal(s) for s in shape], [[-1.0, 1.0]] * len(shape))


def test_tt_scalar_operators():
    a = _tt()
    a.descriptor = "book"
    for r, s in ((a * 2.5, 2.5), (2.5 * a, 2.5), (-a, -1.0), (a / 4, 0.25)):
        assert np.array_equal(r._coeff_cores[0], a._coeff_cores[0] * s)
        assert all(np.array_equal(x, y) for x, y in zip(r._coeff_cores[1:], a._coeff_cores[1:]))
        assert r.tt_ranks == a.tt_ranks and r.descriptor == "book" and r.function is None
        assert r._build_time == 0 and r._total_build_evals == 0 and r.method == a.method
    b = a
    b *= 3
    assert b is not a and np.array_equal(b._coeff_cores[0], a._coeff_cores[0] * 3.0)
    with pytest.raises(TypeError, match="ChebyshevTT \\* str is not supported"):
        a * "x"
    with pytest.raises(TypeError, match="ChebyshevTT / list is not supported"):
        a / [1]
    with pytest.raises(ZeroDivisionError, match="division by zero"):
        a / 0
    with pytest.raises(TypeError, match="unsupported operand type for ChebyshevTT: int"):
        a + 1


def test_tt_compatibility_messages():
    a = _tt()
    with pytest.raises(ValueError, match="num_dimensions mismatch: 3 vs 2"):
        a + _tt(1, ((1, 5, 3), (3, 6, 1)))
    with pytest.raises(ValueError, match=r"n_nodes mismatch: \[5, 6, 4\] vs \[5, 6, 5\]"):
        a + _tt(1, ((1, 5, 3), (3, 6, 2), (2, 5, 1)))
    other = _tt(1)
    other.domain = [[-1.0, 1.0], [-1.0, 1.0], [0.0, 1.0]]
    with pytest.raises(ValueError, match="domain mismatch"):
        a - other
    perm = ChebyshevTT.from_coeff_cores(_tt(1)._coeff_cores, [[-1.0, 1.0]] * 3, dim_order=[2, 0, 1])
    with pytest.raises(ValueError, match=r"TT dim_order mismatch: \[0, 1, 2\] vs \[2, 0, 1\]\. Call other = "
                                         r"other\.reorder\(self\.dim_order\)"):
        a + perm
    unbuilt = ChebyshevTT(math.sin, 3, [[-1.0, 1.0]] * 3, [5, 6, 4])
    with pytest.raises(RuntimeError):
        a + unbuilt


def test_tt_one_dimensional_sum_adds_coefficients():
    a = ChebyshevTT.from_coeff_cores([np.arange(7.0).reshape(1, 7, 1)], [[0.0, 2.0]])
    b = ChebyshevTT.from_coeff_cores([np.linspace(-1, 1, 7).reshape(1, 7, 1)], [[0.0, 2.0]])
    b.max_rank = 5
    r = a + b
    assert np.array_equal(r._coeff_cores[0], a._coeff_cores[0] + b._coeff_cores[0])
    assert r.max_rank == 5 and r.tt_ranks == [1, 1]
    assert np.array_equal((a - b)._coeff_cores[0], a._coeff_cores[0] + b._coeff_cores[0] * -1.0)


def test_reorder_arguments():
    a = _tt()
    with pytest.raises(ValueError, match=r"new_order must be a permutation of range\(3\); got \[0, 1, 1\]"):
        a.reorder([0, 1, 1])
    with pytest.raises(ValueError, match="permutation"):
        a.reorder([0, 1])
    same = a.reorder((0, 1, 2))
    assert same is not a and same.dim_order == [0, 1, 2]
    assert all(np.array_equal(x, y) for x, y in zip(same._coeff_cores, a._coeff_cores))
    with pytest.raises(RuntimeError):
        ChebyshevTT(math.sin, 3, [[-1.0, 1.0]] * 3, [5, 6, 4]).reorder([2, 1, 0])


def test_golden_file_is_small_and_complete():
    path = os.path.join(ROOT, "tests", "golden", "g21_algebra.npz")
    assert os.path.getsize(path) < 1 << 20
    g = np.load(path)
    for tag in ("dense", "spline_b", "spline_c", "slider"):
        for op in ("add", "sub", "lin", "chain"):
            assert g[f"{tag}_{op}"].shape == (len(g[f"{tag}_specs"]), len(g[f"{tag}_points"]))
    for tag in ("g4", "g5", "g5b", "rand16", "rand64"):
        for op in ("add", "sub", "lin", "rev"):
            assert g[f"tt_{tag}_{op}_eval"].shape == (len(g[f"tt_{tag}_points"]),)
