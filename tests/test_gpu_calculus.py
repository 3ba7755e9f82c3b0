"""roots / minimize / maximize on the device (pcx_bary_calculus_batch, pcx_tt_calculus_batch, pcx_cheb1d_calculus:
k_calc_expand, the handle's evaluation, k_cheb1d_calculus) against the reference's values (golden g20), closed
forms, the NumPy host restatement on fibres from the existing slice() path, and themselves (batch = rows, runs).

Bounds: roots 1e-10 (b - a), the reference's own de-duplication scale; values 1e-12 max|fibre|; locations 1e-8 (b - a),
because a critical point is a root of D v and D amplifies rounding by about n^2.  A location is compared only where
the optimum is well defined: a location further off must still be an equally good point (its value within the value
bound of the reference's), which is what happens at flat optima (error ~ sqrt(rounding)) and at ties (T_k, constants).
The worst errors are printed (pytest -s) for DESIGN."""
import numpy as np
import pytest

from calc_fibres import WORST, _bary, _check_opt, _check_roots
from conftest import golden
import functions as F

from pychebyshev_amd import ChebyshevApproximation, ChebyshevSpline, ChebyshevTT, _calculus
from pychebyshev_amd.barycentric import chebyshev_nodes, compute_barycentric_weights, compute_differentiation_matrix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print(f"\ncalculus worst errors: roots {WORST['root']:.2e} (b-a), values {WORST['value']:.2e} max|f|, "
          f"well-defined locations {WORST['location']:.2e} (b-a)")


@pytest.fixture(scope="module")
def g20():
    return golden("g20_calculus")


def _rand(g, n):
    import generate_golden_calculus as G
    V = G.rand_fibres(int(g["rand_seed"]), n, int(g["rand_count"]))
    assert np.array_equal(V[0, :4], g[f"rand{n}_head"]), "seeded golden fibres no longer regenerate"
    return V


def _names(g):
    return sorted({k[4:-7] for k in g.files if k.startswith("fib_") and k.endswith("_values")})


# ------------------------------------------------------------------ 1-D goldens through the public API
def test_named_fibres_match_reference(g20):
    for name in _names(g20):
        v, (a, b) = g20[f"fib_{name}_values"], tuple(g20[f"fib_{name}_domain"])
        c = ChebyshevApproximation.from_values(v, 1, [[a, b]], [v.size])
        _check_roots(c.roots(), g20[f"fib_{name}_roots"], a, b, name)
        at = _bary(v, c.nodes[0], c.weights[0])
        scale = max(float(np.max(np.abs(v))), 1e-300)
        for mode, fn in (("min", c.minimize), ("max", c.maximize)):
            _check_opt(fn(), g20[f"fib_{name}_{mode}"], scale, a, b, at, f"{name} {mode}")


@pytest.mark.parametrize("n", [8, 16, 32, 64])
def test_random_fibres_match_reference_through_cheb1d(g20, n):
    """pcx_cheb1d_calculus on the golden fibres: the solver on its own, 200 rows per call."""
    V = _rand(g20, n)
    x = chebyshev_nodes(-1.0, 1.0, n)
    w = compute_barycentric_weights(x)
    D = compute_differentiation_matrix(x, w)
    R, cnt = _calculus.cheb1d_calculus(V, x, w, None, (-1.0, 1.0), "roots")
    assert np.array_equal(cnt, g20[f"rand{n}_count"])
    for mode in ("min", "max"):
        val, loc, c2 = _calculus.cheb1d_calculus(V, x, w, D, (-1.0, 1.0), mode)
        assert np.all(c2 >= 0)
        for i in range(V.shape[0]):
            _check_opt((val[i], loc[i]), g20[f"rand{n}_{mode}"][i], np.max(np.abs(V[i])), -1.0, 1.0, _bary(V[i], x, w),
                       f"rand{n}[{i}] {mode}")
    for i in range(V.shape[0]):
        k = int(cnt[i])
        _check_roots(R[i, :k], g20[f"rand{n}_roots"][i, :k], -1.0, 1.0, f"rand{n}[{i}]")
        assert np.all(np.isnan(R[i, k:]))


@pytest.mark.parametrize("k", [5, 17, 40])
def test_chebyshev_polynomial_roots_closed_form(k):
    """T_k sampled at 64 nodes: roots cos((2j - 1) pi / 2k).  Bound 1e-11, not 1e-13: the coefficients above degree k
    are round-off, not zero, so the colleague matrix has degree 63 and last-column entries near 1e16; NumPy's own
    path (the host restatement) is off by 1.9e-13 (k = 17) and 2.5e-13 (k = 40), the device path by up to 2.7e-12."""
    n = 64
    x = chebyshev_nodes(-1.0, 1.0, n)
    c = ChebyshevApproximation.from_values(np.cos(k * np.arccos(x)), 1, [[-1.0, 1.0]], [n])
    want = np.sort(np.cos((2 * np.arange(1, k + 1) - 1) * np.pi / (2 * k)))
    got = c.roots()
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= 1e-11


# ------------------------------------------------------------------ dense, spline, TT goldens
def test_dense_goldens(g20):
    import generate_golden_calculus as G
    c1 = ChebyshevApproximation.from_values(golden("g1_sincos2d")["tensor"], 2, [[-1.0, 1.0], [-1.0, 1.0]], [12, 12])
    for k in (0, 1):
        for i, v in enumerate(G.SC2_FIXED):
            _check_roots(c1.roots(k, {1 - k: v}), g20[f"sc2_d{k}_{i}_roots"], -1.0, 1.0, f"sc2 {k} {i}")
    bs = golden("g2_bs5d")["tensor"]
    spot = ChebyshevApproximation.from_values(bs - 10.0, 5, F.BS5_DOMAIN, F.BS5_NODES)
    for i, row in enumerate(G.BS5_FIXED):
        got = spot.roots(0, {k + 1: v for k, v in enumerate(row)})
        _check_roots(got, g20[f"spot_{i}_roots"], 80.0, 120.0, f"spot {i}")
    c2 = ChebyshevApproximation.from_values(bs, 5, F.BS5_DOMAIN, F.BS5_NODES)
    full = [100.0] + G.BS5_FIXED[0]
    for k in range(5):
        fixed = {q: full[q] for q in range(5) if q != k}
        a, b = F.BS5_DOMAIN[k]
        pts = _calculus.fibre_points(5, k, _calculus.fixed_row(5, k, list(fixed.items())), c2.nodes[k])
        v = c2.vectorized_eval_batch(pts, [0] * 5)
        at = _bary(v, c2.nodes[k], c2.weights[k])
        for mode, fn in (("min", c2.minimize), ("max", c2.maximize)):
            _check_opt(fn(k, fixed), g20[f"bs5_d{k}_{mode}"], np.max(np.abs(v)), a, b, at, f"bs5 {k} {mode}")


def test_spline_goldens(g20):
    import generate_golden_calculus as G
    for name, case in F.SPLINE_CASES.items():
        sp = ChebyshevSpline(getattr(F, case["f"]), case["d"], case["domain"],
                             n_nodes=[list(v) if isinstance(v, list) else v for v in case["n_nodes"]], knots=case["knots"])
        sp.build(verbose=False)
        a, b = case["domain"][0]
        for i, row in enumerate(G.SPLINE_FIXED[name]):
            fixed = {k + 1: v for k, v in enumerate(row)} if case["d"] > 1 else None
            tag = f"spline_{name}_{i}"
            _check_roots(sp.roots(0, fixed), g20[f"{tag}_roots"], a, b, tag)

            def at(t, row=row):
                return float(sp.eval([t] + list(row)))
            scale = max(abs(float(g20[f"{tag}_min"][0])), abs(float(g20[f"{tag}_max"][0])), 1e-300)
            _check_opt(sp.minimize(0, fixed), g20[f"{tag}_min"], scale, a, b, at, tag + " min")
            _check_opt(sp.maximize(0, fixed), g20[f"{tag}_max"], scale, a, b, at, tag + " max")
    assert g20["spline_a_0_roots"].size >= 1          # case a: |x| touches zero on the knot


def test_tt_goldens(g20):
    import generate_golden_calculus as G
    g4, g5 = golden("g4_tt_bs5d"), golden("g5_tt_rank16")
    tts = {"tt4": (ChebyshevTT.from_coeff_cores([g4[f"r8_core{k}"] for k in range(5)], F.BS5_DOMAIN), G.TT4_FIXED),
           "tt5": (ChebyshevTT.from_coeff_cores([g5[f"core{k}"] for k in range(10)], [[-1.0, 1.0]] * 10,
                                                dim_order=[int(v) for v in g5["perm"]]), G.TT5_FIXED)}
    for name, (tt, fx) in tts.items():
        dom = tt._user_frame_domain()
        for k in G.TT_DIMS[name]:
            fixed = {q: fx[q] for q in range(len(fx)) if q != k}
            a, b = dom[k]
            x = chebyshev_nodes(a, b, 11)
            v = tt.eval_batch(_calculus.fibre_points(len(fx), k, _calculus.fixed_row(len(fx), k, list(fixed.items())), x))
            at = _bary(v, x, compute_barycentric_weights(x))
            for mode, fn in (("min", tt.minimize), ("max", tt.maximize)):
                _check_opt(fn(k, fixed), g20[f"{name}_d{k}_{mode}"], np.max(np.abs(v)), a, b, at, f"{name} {k} {mode}")


# ------------------------------------------------------------------ batches, rows and runs
def _bs5_minus_strike():
    return ChebyshevApproximation.from_values(golden("g2_bs5d")["tensor"] - 10.0, 5, F.BS5_DOMAIN, F.BS5_NODES)


def _rows(n, dim, seed):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(lo, hi, n) for k, (lo, hi) in enumerate(F.BS5_DOMAIN) if k != dim])


def test_batch_rows_are_bitwise_the_single_solver_and_runs_repeat():
    c = _bs5_minus_strike()
    rows = _rows(10_000, 0, 5)
    R1, n1 = c.roots_batch(0, rows)
    R2, n2 = c.roots_batch(0, rows)
    assert np.array_equal(n1, n2) and np.array_equal(R1, R2, equal_nan=True)
    v1, l1 = c.minimize_batch(2, _rows(10_000, 2, 6))
    v2, l2 = c.minimize_batch(2, _rows(10_000, 2, 6))
    assert np.array_equal(v1, v2) and np.array_equal(l1, l2)
    # any row alone through pcx_cheb1d_calculus: the same bits as inside the batch
    for r in (0, 17, 4242, 9999):
        pts = _calculus.fibre_points(5, 0, rows[r:r + 1], c.nodes[0])
        fib = c.vectorized_eval_batch(pts, [0] * 5)
        R, n = _calculus.cheb1d_calculus(fib, c.nodes[0], c.weights[0], None, tuple(F.BS5_DOMAIN[0]), "roots")
        assert n[0] == n1[r] and np.array_equal(R[0], R1[r], equal_nan=True)
        single = c.roots(0, {k + 1: float(v) for k, v in enumerate(rows[r])})
        assert np.array_equal(single, R1[r, :n1[r]])


@pytest.mark.parametrize("dim,mode", [(0, "roots"), (3, "roots"), (0, "min"), (3, "max")])
def test_bs5_batch_against_slice_and_host_restatement(dim, mode):
    """10^4 rows on the device; every 10th row checked through an independent path: the fibre from the existing
    slice() (k_contract_axis) and the NumPy restatement (chebroots)."""
    c = _bs5_minus_strike()
    rows = _rows(10_000, dim, 40 + dim)
    a, b = F.BS5_DOMAIN[dim]
    if mode == "roots":
        R, cnt = c.roots_batch(dim, rows)
    else:
        val, loc = (c.minimize_batch if mode == "min" else c.maximize_batch)(dim, rows)
    for r in range(0, rows.shape[0], 10):
        sl = c.slice([(k, float(v)) for k, v in zip([q for q in range(5) if q != dim], rows[r])])
        v = sl.tensor_values
        if mode == "roots":
            _check_roots(R[r, :cnt[r]], _calculus.roots_1d(v, (a, b)), a, b, f"row {r}")
        else:
            want = _calculus.optimize_1d(v, sl.nodes[0], sl.weights[0], sl.diff_matrices[0], (a, b), mode)
            _check_opt((val[r], loc[r]), want, np.max(np.abs(v)), a, b, _bary(v, sl.nodes[0], sl.weights[0]), f"row {r}")


def test_tt_batch_matches_single_calls():
    g4 = golden("g4_tt_bs5d")
    tt = ChebyshevTT.from_coeff_cores([g4[f"r8_core{k}"] for k in range(5)], F.BS5_DOMAIN)
    rows = _rows(500, 3, 9)
    val, loc = tt.maximize_batch(3, rows)
    for r in range(0, 500, 50):
        got = tt.maximize(3, {k: float(v) for k, v in zip([0, 1, 2, 4], rows[r])})
        assert got == (val[r], loc[r])


# ------------------------------------------------------------------ error paths
def test_nan_fibre_fails_the_row():
    t = golden("g2_bs5d")["tensor"].copy()
    c = ChebyshevApproximation.from_values(t, 5, F.BS5_DOMAIN, F.BS5_NODES)    # from_values refuses non-finite data
    t = t.copy()
    t[3, 5, 5, 5, 5] = np.nan
    c.tensor_values = t                                                      # the device copy follows tensor_values
    fx = {1: 100.0, 2: 0.5, 3: 0.25, 4: 0.03}
    R, cnt = c.roots_batch(0, np.array([[100.0, 0.5, 0.25, 0.03]]))
    assert cnt[0] == -1 and np.all(np.isnan(R[0]))
    val, loc = c.minimize_batch(0, np.array([[100.0, 0.5, 0.25, 0.03]]))
    assert np.isnan(val[0]) and np.isnan(loc[0])
    with pytest.raises(np.linalg.LinAlgError):
        c.roots(0, fx)
    with pytest.raises(np.linalg.LinAlgError):
        c.maximize(0, fx)
    x = chebyshev_nodes(-1.0, 1.0, 9)
    v = np.cos(np.arange(9.0))
    v[4] = np.inf
    R, cnt = _calculus.cheb1d_calculus(np.vstack([np.cos(np.arange(9.0)), v]), x, compute_barycentric_weights(x), None,
                                       (-1.0, 1.0), "roots")
    assert cnt[0] >= 0 and cnt[1] == -1 and np.all(np.isnan(R[1]))


def test_long_fibres_finish_on_the_host():
    n = 80
    T = np.add.outer(np.sin(3.0 * chebyshev_nodes(-1.0, 2.0, n)), np.array([0.0, 0.2, -0.3]))
    c = ChebyshevApproximation.from_values(T, 2, [[-1.0, 2.0], [0.0, 1.0]], [n, 3])
    with pytest.raises(ValueError, match="80 nodes"):
        c.roots_batch(0, np.array([[0.5]]))
    fixed = {1: 0.5}
    pts = _calculus.fibre_points(2, 0, np.array([[0.5]]), c.nodes[0])
    v = c.vectorized_eval_batch(pts, [0, 0])
    assert np.array_equal(c.roots(0, fixed), _calculus.roots_1d(v, (-1.0, 2.0)))
    assert c.minimize(0, fixed) == _calculus.optimize_1d(v, c.nodes[0], c.weights[0], c.diff_matrices[0], (-1.0, 2.0), "min")
    assert c.roots(0, fixed).size >= 1
