"""Sobol indices on the device: ChebyshevApproximation / ChebyshevSpline .sobol_indices() (pcx_bary_sobol: d
k_mode_product coefficient passes, k_sobol_energy, k_sobol_finish) against the reference's values (golden g19),
closed forms and a NumPy restatement at sizes that take many blocks.

Bounds: indices 1e-12 absolute, variance 1e-12 relative.  The device forms the coefficients as matrix products
(the reference: an FFT DCT) and adds the energies as a tree (the reference: one by one), so the two differ in
rounding only."""
import ctypes
import math

import numpy as np
import pytest

from conftest import golden
import functions as F

from pychebyshev_amd import ChebyshevApproximation, ChebyshevSpline, ChebyshevTT, _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g19():
    return golden("g19_sobol")


def _arrays(res, d):
    assert sorted(res["first_order"]) == list(range(d)) and sorted(res["total_order"]) == list(range(d))
    assert all(type(k) is int for k in res["first_order"]) and isinstance(res["variance"], float)
    return (np.array([res["first_order"][k] for k in range(d)]), np.array([res["total_order"][k] for k in range(d)]),
            res["variance"])


def _check(res, gold, tag, d):
    first, total, var = _arrays(res, d)
    assert np.max(np.abs(first - gold[f"{tag}_first"])) <= 1e-12, tag
    assert np.max(np.abs(total - gold[f"{tag}_total"])) <= 1e-12, tag
    want = float(gold[f"{tag}_variance"])
    assert abs(var - want) <= 1e-12 * abs(want), (tag, var, want)


def _dense(tensor, domain=None):
    tensor = np.asarray(tensor, dtype=float)
    d = tensor.ndim
    domain = [[-1.0, 1.0]] * d if domain is None else [list(b) for b in domain]
    return ChebyshevApproximation.from_values(tensor, d, domain, list(tensor.shape))


def _seeded(g, tag):
    t = np.random.default_rng(int(g[f"{tag}_seed"])).standard_normal(tuple(int(v) for v in g[f"{tag}_shape"]))
    assert np.array_equal(t.ravel()[:8], g[f"{tag}_head"]), "seeded golden tensor no longer regenerates"
    return t


def _dense_input(g, tag):
    if tag == "bs5":
        return golden("g2_bs5d")["tensor"], None
    if tag == "sc2":
        return golden("g1_sincos2d")["tensor"], None
    if tag in ("rand8", "rand16"):
        return _seeded(g, tag), None
    return g[f"{tag}_tensor"], (g[f"{tag}_domain"] if f"{tag}_domain" in g.files else None)


# ------------------------------------------------------------------ reference goldens
@pytest.mark.parametrize("tag", ["bs5", "sc2", "smooth3", "one_d", "additive4", "prod2", "rand8", "rand16"])
def test_dense_sobol_matches_reference(g19, tag):
    tensor, domain = _dense_input(g19, tag)
    _check(_dense(tensor, domain).sobol_indices(), g19, tag, np.ndim(tensor))


@pytest.mark.parametrize("tag", sorted(F.SPLINE_CASES))
def test_spline_sobol_matches_reference(g19, tag):
    case = F.SPLINE_CASES[tag]
    sp = ChebyshevSpline(getattr(F, case["f"]), case["d"], case["domain"],
                         n_nodes=[list(v) if isinstance(v, list) else v for v in case["n_nodes"]], knots=case["knots"])
    sp.build(verbose=False)
    _check(sp.sobol_indices(), g19, f"spline_{tag}", case["d"])


@pytest.mark.parametrize("tag", ["sc2", "smooth3"])
def test_chebyshev_coefficients_match_reference(g19, tag):
    tensor, domain = _dense_input(g19, tag)
    got = _dense(tensor, domain)._chebyshev_coefficients()
    want = g19[f"coef_{tag}"]
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= 1e-14 * np.max(np.abs(want))


# ------------------------------------------------------------------ known answers
def test_additive_function_has_no_interactions(g19):
    first, total, _ = _arrays(_dense(g19["additive4_tensor"], g19["additive4_domain"]).sobol_indices(), 4)
    assert np.max(np.abs(first - total)) <= 1e-12
    assert abs(first.sum() - 1.0) <= 1e-12


def test_product_x0_x1_is_pure_interaction(g19):
    first, total, _ = _arrays(_dense(g19["prod2_tensor"]).sobol_indices(), 2)
    assert np.max(np.abs(first)) <= 1e-12
    assert np.max(np.abs(total - 1.0)) <= 1e-12


def test_zero_tensor_has_zero_variance_and_indices():
    res = _dense(np.zeros((4, 5, 3))).sobol_indices()
    assert res == {"first_order": {0: 0.0, 1: 0.0, 2: 0.0}, "total_order": {0: 0.0, 1: 0.0, 2: 0.0}, "variance": 0.0}


def test_constant_tensor_variance_is_rounding_noise(g19):
    c = 2.5
    t = g19["const3_tensor"]
    assert np.all(t == c)
    var = _dense(t).sobol_indices()["variance"]
    assert 0.0 <= var <= 1e-24 * c * c * math.pi ** 3      # the indices of noise are noise (so in the reference too)


def test_one_dimensional_rules():
    res = _dense(np.cos(np.arange(9.0))).sobol_indices()
    assert res["first_order"] == {0: 1.0} and res["total_order"] == {0: 1.0} and res["variance"] > 0
    res0 = _dense(np.zeros(9)).sobol_indices()
    assert res0 == {"first_order": {0: 0.0}, "total_order": {0: 0.0}, "variance": 0.0}


def test_spline_without_knots_equals_its_approximation():
    dom = [[0.0, 1.0], [-0.5, 0.5]]                      # unit volume: the spline's variance is the piece's
    sp = ChebyshevSpline(F.sin_cos_2d, 2, dom, n_nodes=[9, 11], knots=[[], []])
    sp.build(verbose=False)
    ap = ChebyshevApproximation(F.sin_cos_2d, 2, dom, [9, 11])
    ap.build(verbose=False)
    a, b = sp.sobol_indices(), ap.sobol_indices()
    assert a["variance"] == b["variance"]
    for key in ("first_order", "total_order"):
        for k in range(2):
            assert abs(a[key][k] - b[key][k]) <= 1e-15


def test_dense_of_a_tt_agrees_with_the_tt_contraction():
    g4 = golden("g4_tt_bs5d")
    tt = ChebyshevTT.from_coeff_cores([g4[f"r8_core{k}"] for k in range(5)], F.BS5_DOMAIN)
    dense = ChebyshevApproximation.from_values(tt.to_dense(), 5, F.BS5_DOMAIN, tt.n_nodes)
    a, b = dense.sobol_indices(), tt.sobol_indices()
    for key in ("first_order", "total_order"):
        for k in range(5):
            assert abs(a[key][k] - b[key][k]) <= 1e-10
    assert abs(a["variance"] - b["variance"]) <= 1e-10 * abs(b["variance"])


# ------------------------------------------------------------------ many blocks: NumPy restatement
def _numpy_sobol(T):
    """Coefficients by one tensordot per axis with the reference's per-axis DCT matrix, then masked sums of
    e = c^2 pi^d 2^-z (z = nonzero indices of the multi-index)."""
    d = T.ndim
    C = T
    for k, n in enumerate(T.shape):
        m = np.arange(n)[:, None]
        i = np.arange(n)[None, :]
        M = (2.0 / n) * np.cos(np.pi * ((m * (2 * (n - 1 - i) + 1)) % (4 * n)) / (2.0 * n))
        M[0] *= 0.5
        C = np.moveaxis(np.tensordot(M, C, axes=([1], [k])), 0, k)
    z = np.zeros(T.shape, dtype=np.int8)
    for k, n in enumerate(T.shape):
        shape = [1] * d
        shape[k] = n
        z += (np.arange(n) > 0).astype(np.int8).reshape(shape)
    E = C * C * (math.pi ** d) * np.exp2(-z.astype(float))
    var = E.sum() - E[(0,) * d]
    first, total = np.empty(d), np.empty(d)
    for k in range(d):
        line = [0] * d
        line[k] = slice(1, None)
        first[k] = E[tuple(line)].sum() / var
        total[k] = (E.sum() - E.take(0, axis=k).sum()) / var
    return first, total, var


@pytest.mark.parametrize("shape", [(64, 64, 64, 64), (65, 65, 65)])
def test_large_tensors_match_numpy_restatement(shape):
    T = np.random.default_rng(sum(shape)).standard_normal(shape) + np.linspace(0.0, 1.0, shape[-1])
    first, total, var = _arrays(_dense(T).sobol_indices(), len(shape))
    wf, wt, wv = _numpy_sobol(T)
    assert np.max(np.abs(first - wf)) <= 1e-12
    assert np.max(np.abs(total - wt)) <= 1e-12
    assert abs(var - wv) <= 1e-12 * wv


def test_results_are_bitwise_reproducible():
    T = np.random.default_rng(5).standard_normal((64, 64, 64, 64))
    a = _dense(T)
    r1, r2 = a.sobol_indices(), a.sobol_indices()
    r3 = _dense(T.copy()).sobol_indices()                 # a second handle
    assert r1 == r2 == r3


# ------------------------------------------------------------------ errors
def test_non_finite_coefficient_raises():
    ap = ChebyshevApproximation(F.sin_cos_2d, 2, [[-1.0, 1.0]] * 2, [6, 7])
    ap.build(verbose=False)
    # build() rejects non-finite callback values, so the only way to reach the kernel's non-finite flag is to edit the
    # tensor of a built model and drop its device copy
    ap.tensor_values[2, 3] = np.inf
    ap.invalidate_device_cache()
    with pytest.raises(ValueError, match="NaN or Inf"):
        ap.sobol_indices()


def test_unbuilt_spline_raises():
    sp = ChebyshevSpline(F.kink_2d, 2, [[-1.0, 1.0], [0.0, 1.0]], n_nodes=[7, 6], knots=[[0.2], [0.5]])
    with pytest.raises(RuntimeError):
        sp.sobol_indices()


def test_c_abi_argument_errors():
    ap = _dense(np.arange(12.0).reshape(3, 4))
    m = ap._model()
    lib = m.lib
    v = ctypes.c_double()
    f, t, c = np.empty(2), np.empty(2), np.empty(12)
    assert lib.pcx_bary_sobol(None, ctypes.byref(v), _lib.p_f64(f), _lib.p_f64(t)) == _lib.PCX_ERR_INVALID
    assert lib.pcx_bary_sobol(m.handle, None, _lib.p_f64(f), _lib.p_f64(t)) == _lib.PCX_ERR_INVALID
    assert lib.pcx_bary_sobol(m.handle, ctypes.byref(v), None, _lib.p_f64(t)) == _lib.PCX_ERR_INVALID
    assert lib.pcx_bary_sobol(m.handle, ctypes.byref(v), _lib.p_f64(f), None) == _lib.PCX_ERR_INVALID
    assert lib.pcx_bary_chebyshev_coefficients(None, _lib.p_f64(c)) == _lib.PCX_ERR_INVALID
    assert lib.pcx_bary_chebyshev_coefficients(m.handle, None) == _lib.PCX_ERR_INVALID
    assert b"NULL" in lib.pcx_last_error()
    _lib.check(lib.pcx_bary_sobol(m.handle, ctypes.byref(v), _lib.p_f64(f), _lib.p_f64(t)), lib)
    assert v.value > 0.0
