"""Arithmetic operators on the GPU: the reference's results (g21_algebra.npz) for dense, spline, slider and TT
combinations, the canonical form and rank handling of the device rounding, a 50-trade book, stale device
caches after in-place operators, bitwise reproducibility and the size limits of the rounding entry points."""
import ctypes

import numpy as np
import pytest

import functions as F
import generate_golden_algebra as GA
from conftest import assert_parity, golden, spec_point_tol
from pychebyshev_amd import ChebyshevApproximation, ChebyshevSlider, ChebyshevSpline, ChebyshevTT, _algebra, _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g21():
    return golden("g21_algebra")


def _combos(make_a, make_b):
    a, b = make_a(), make_b()
    out = {"add": a + b, "sub": a - b, "lin": 2.5 * a - b / 3}
    c = make_a()
    c += b
    c *= 0.5
    c -= b / 4
    out["chain"] = c
    return out


def _check(g21, tag, combos, evaluate):
    pts, specs = g21[f"{tag}_points"], g21[f"{tag}_specs"]
    for op, obj in combos.items():
        for i, spec in enumerate(specs):
            assert_parity(evaluate(obj, pts, list(spec)), g21[f"{tag}_{op}"][i], tol=1e-12,
                          point_tol=spec_point_tol(spec), what=f"algebra {tag} {op} spec {list(spec)}")


# ------------------------------------------------------------------ golden parity: dense, spline, slider
def test_dense_golden(g21):
    T = golden("g2_bs5d")["tensor"]
    combos = _combos(lambda: ChebyshevApproximation.from_values(T, 5, F.BS5_DOMAIN, F.BS5_NODES),
                     lambda: ChebyshevApproximation.from_values(np.ascontiguousarray(T[::-1]), 5, F.BS5_DOMAIN, F.BS5_NODES))
    _check(g21, "dense", combos, lambda o, p, s: o.vectorized_eval_batch(p, s))


@pytest.mark.parametrize("tag", ["b", "c"])
def test_spline_golden(g21, tag):
    case = F.SPLINE_CASES[tag]

    def build():
        sp = ChebyshevSpline(getattr(F, case["f"]), case["d"], case["domain"],
                             n_nodes=[list(v) if isinstance(v, list) else v for v in case["n_nodes"]], knots=case["knots"])
        sp.build(verbose=False)
        return sp

    def flipped():
        sp = build()
        for p in sp._pieces:
            p.tensor_values = np.ascontiguousarray(p.tensor_values[::-1])
        return sp

    _check(g21, f"spline_{tag}", _combos(build, flipped), lambda o, p, s: o.eval_batch(p, s))


def test_slider_golden(g21):
    case = F.SLIDER_CASES["b"]

    def slider(fn):
        sl = ChebyshevSlider(fn, case["d"], case["domain"], case["n_nodes"], partition=case["partition"],
                             pivot_point=case["pivot"])
        sl.build(verbose=False)
        return sl

    _check(g21, "slider", _combos(lambda: slider(F.bs_5d), lambda: slider(F.poly_5d_fixture)),
           lambda o, p, s: o.eval_batch(p, s))


# ------------------------------------------------------------------ golden parity: tensor trains
def _tt_pair(g21, tag):
    ca, cb, domain, max_rank = GA.tt_operands(tag)
    tol = float(g21[f"tt_{tag}_tol"])
    a, b = (ChebyshevTT.from_coeff_cores(c, domain) for c in (ca, cb))
    for t in (a, b):
        t.max_rank, t.tolerance = max_rank, tol
    return a, b


def _normwise(y, ref):
    return float(np.max(np.abs(y - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("tag", list(GA.TT_CASES))
def test_tt_golden(g21, tag):
    a, b = _tt_pair(g21, tag)
    pts = g21[f"tt_{tag}_points"]
    for op, res in {"add": a + b, "sub": a - b, "lin": 2.5 * a - b / 3}.items():
        assert res.tt_ranks == [int(v) for v in g21[f"tt_{tag}_{op}_ranks"]], (tag, op)
        assert res.max_rank == a.max_rank and res.tolerance == a.tolerance and res.function is None
        err = _normwise(res.eval_batch(pts), g21[f"tt_{tag}_{op}_eval"])
        assert err <= 1e-10, (tag, op, err)
    if tag == "rand64":        # its reversal is capped by max_rank on a gapless spectrum: covered by the probe, not here
        return
    d = a.num_dimensions
    rev = a.reorder(list(range(d))[::-1])
    assert rev.dim_order == list(range(d))[::-1] and max(rev.tt_ranks) <= a.max_rank
    if bool(g21[f"tt_{tag}_rev_fair"]):
        assert rev.tt_ranks == [int(v) for v in g21[f"tt_{tag}_rev_ranks"]]
        assert _normwise(rev.eval_batch(pts), g21[f"tt_{tag}_rev_eval"]) <= 1e-10


def test_tt_reorder_round_trip_keeps_the_function():
    g5b = golden("g5b_tt_mixed")
    cores = [g5b[f"core{k}"] for k in range(4)]
    dom = [[0.0, 2.0], [-3.0, -1.0], [10.0, 11.0], [-1.0, 1.0]]
    a = ChebyshevTT.from_coeff_cores(cores, dom)
    a.max_rank, a.tolerance = 64, 1e-13        # from_coeff_cores caps at the largest rank (5): a permuted order needs more
    pts = g5b["points"]
    for order in ([2, 0, 3, 1], [3, 2, 1, 0], [1, 0, 2, 3]):
        r = a.reorder(order)
        assert r.dim_order == order and r.n_nodes == [a.n_nodes[k] for k in order]
        assert _normwise(r.eval_batch(pts), g5b["out"]) <= 1e-12
        back = r.reorder([0, 1, 2, 3])
        assert _normwise(back.eval_batch(pts), g5b["out"]) <= 1e-12
        with pytest.raises(ValueError, match="mismatch"):       # n_nodes (storage order) is checked before dim_order
            a + r
        assert _normwise((back + a).eval_batch(pts), 2.0 * g5b["out"]) <= 1e-12


# ------------------------------------------------------------------ rounding: canonical form, a - a
@pytest.mark.parametrize("tag", ["g5", "rand16", "rand64"])
def test_sum_is_left_orthonormal(g21, tag):
    a, b = _tt_pair(g21, tag)
    s = a + b
    for k, c in enumerate(s._coeff_cores[:-1]):
        m = c.reshape(-1, c.shape[2])
        assert np.max(np.abs(m.T @ m - np.eye(m.shape[1]))) <= 1e-13, k


@pytest.mark.parametrize("tag", ["g4", "g5", "g5b", "rand16"])
def test_difference_with_itself_is_zero(g21, tag):
    a, _ = _tt_pair(g21, tag)
    z = a - a
    assert max(z.tt_ranks) <= a.max_rank
    pts = g21[f"tt_{tag}_points"]
    assert np.max(np.abs(z.eval_batch(pts))) <= 1e-12 * max(1.0, float(np.max(np.abs(a.eval_batch(pts)))))
    two = a + a
    assert two.tt_ranks == a.tt_ranks or max(two.tt_ranks) <= a.max_rank
    assert _normwise(two.eval_batch(pts), 2.0 * a.eval_batch(pts)) <= 1e-12


def test_rounding_is_bitwise_reproducible(g21):
    a, b = _tt_pair(g21, "rand64")
    stacked = _algebra.tt_stack(a._coeff_cores, b._coeff_cores)
    r1 = _algebra.tt_round(stacked, 128, 1e-10, 0)
    r2 = _algebra.tt_round(stacked, 128, 1e-10, 0)
    assert all(np.array_equal(x, y) for x, y in zip(r1, r2))
    s1 = _algebra.tt_swaps(a._coeff_cores, [3, 2, 3], 64, 1e-10, 0)
    s2 = _algebra.tt_swaps(a._coeff_cores, [3, 2, 3], 64, 1e-10, 0)
    assert all(np.array_equal(x, y) for x, y in zip(s1, s2))


def test_oversize_shapes_are_refused_before_any_launch():
    lib = _lib.load()
    big = [np.zeros((1, 4, 300)), np.zeros((300, 4, 1))]
    with pytest.raises(NotImplementedError, match=r"core 0 of shape \(1, 4, 300\) exceeds ranks 256"):
        _algebra.tt_round(big, 8, 1e-10, 0)
    many = [np.zeros((1, 300, 2)), np.zeros((2, 4, 1))]
    with pytest.raises(NotImplementedError, match=r"\(1, 300, 2\)"):
        _algebra.tt_swaps(many, [0], 8, 1e-10, 0)
    wide = [np.zeros((1, 64, 100)), np.zeros((100, 64, 100)), np.zeros((100, 64, 1))]
    with pytest.raises(NotImplementedError, match="TT swap at 1"):
        _algebra.tt_swaps(wide, [1], 8, 1e-10, 0)
    n = _lib.i32([4, 4])
    ranks = _lib.i32([1, 2, 1])
    out = np.empty(16)
    length = ctypes.c_int64(0)
    assert lib.pcx_tt_round(0, 2, _lib.p_i32(n), _lib.p_i32(_lib.i32([2, 2, 1])), _lib.p_f64(out), 4, 1e-10,
                            _lib.p_i32(_lib.i32([0, 0, 0])), _lib.p_f64(out), 16, ctypes.byref(length), None) == _lib.PCX_ERR_INVALID
    assert lib.pcx_tt_round(0, 2, _lib.p_i32(n), _lib.p_i32(ranks), _lib.p_f64(out), 0, 1e-10,
                            _lib.p_i32(_lib.i32([0, 0, 0])), _lib.p_f64(out), 16, ctypes.byref(length), None) == _lib.PCX_ERR_INVALID


# ------------------------------------------------------------------ a book of trades
def test_fifty_trade_book():
    rng = np.random.default_rng(50)
    domain = [[80.0, 120.0], [0.1, 1.0], [0.1, 0.5]]
    n = [11, 9, 7]
    grid = np.meshgrid(*[np.sort(0.5 * (lo + hi) + 0.5 * (hi - lo) * np.cos(np.pi * (2 * np.arange(k) + 1) / (2 * k)))
                         for (lo, hi), k in zip(domain, n)], indexing="ij")
    trades, weights = [], rng.uniform(-2.0, 2.0, 50)
    for i in range(50):
        K, q = rng.uniform(85, 115), rng.uniform(0.0, 0.05)
        vals = np.vectorize(lambda S, T, s: F.bs_call_price(S, K, T, 0.03, s, q))(*grid)
        trades.append(ChebyshevApproximation.from_values(vals, 3, domain, n))
    book = trades[0] * float(weights[0])
    for w, t in zip(weights[1:], trades[1:]):
        book = book + w * t
    pts = np.column_stack([rng.uniform(lo, hi, 100_000) for lo, hi in domain])
    specs = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0]]
    got = book.vectorized_eval_multi_batch(pts, specs)
    want = sum(w * t.vectorized_eval_multi_batch(pts, specs) for w, t in zip(weights, trades))
    for j, spec in enumerate(specs):
        assert _normwise(got[:, j], want[:, j]) <= 1e-12, spec


# ------------------------------------------------------------------ in-place operators and the device caches
def test_in_place_operators_invalidate_device_models():
    T = golden("g2_bs5d")["tensor"]
    pts = F.bs5_query_points(3000, seed=77)
    spec = [1, 0, 0, 0, 0]

    def dense(t):
        return ChebyshevApproximation.from_values(np.ascontiguousarray(t), 5, F.BS5_DOMAIN, F.BS5_NODES)

    for fan in (False, True):
        a, b = dense(T), dense(T[::-1])
        if fan:
            a.to_device(devices=[0, 0])
        a.vectorized_eval_batch(pts, spec)
        a += b
        assert np.array_equal(a.vectorized_eval_batch(pts, spec), dense(T + T[::-1]).vectorized_eval_batch(pts, spec))
        a *= 3
        assert np.array_equal(a.vectorized_eval_batch(pts, spec),
                              dense((T + T[::-1]) * 3.0).vectorized_eval_batch(pts, spec))
        if fan:
            big = np.repeat(pts, 50, axis=0)
            assert np.array_equal(a.vectorized_eval_batch(big, [0] * 5),
                                  dense((T + T[::-1]) * 3.0).vectorized_eval_batch(big, [0] * 5))

    case = F.SPLINE_CASES["c"]

    def spline():
        sp = ChebyshevSpline(F.call_payoff_3d, 3, case["domain"], n_nodes=case["n_nodes"], knots=case["knots"])
        sp.build(verbose=False)
        return sp

    sp, other = spline(), spline() * 0.5
    spts = np.column_stack([np.random.default_rng(3).uniform(lo, hi, 2000) for lo, hi in case["domain"]])
    sp.eval_batch(spts, [0, 0, 0])
    sp += other
    sp *= 2
    assert np.array_equal(sp.eval_batch(spts, [1, 0, 0]), ((spline() + spline() * 0.5) * 2).eval_batch(spts, [1, 0, 0]))

    sc = F.SLIDER_CASES["b"]

    def slider():
        sl = ChebyshevSlider(F.bs_5d, 5, sc["domain"], sc["n_nodes"], partition=sc["partition"], pivot_point=sc["pivot"])
        sl.build(verbose=False)
        return sl

    sl = slider()
    sl.eval_batch(pts, [0] * 5)
    sl -= slider() * 0.25
    sl *= 4
    want = ((slider() - slider() * 0.25) * 4).eval_multi_batch(pts, [[0] * 5, spec])
    assert np.array_equal(sl.eval_multi_batch(pts, [[0] * 5, spec]), want)
