"""The lane-per-fibre inversion (inv_block of csrc/invert_kernels.h) and the level= root finders on the device.

  a  pcx_cheb1d_solve, method 1, at n in {1, 2, 3, 16, 17, 18, 33, 34, 63, 64} and N in {1, 63, 64, 65, 200} (lane
     tails): status equals the restatement's (_calculus.invert_rows), x within 1e-13 (b - a), no row left out; the
     inputs are those of the host-pass test (invert_fibres), cycled to 200 rows; a row alone has the bits it has in
     the batch of 200; solutions at and next to 0 (t = 0, +-1e-15 ... +-1e-300, p(0) summed otherwise) have status 1
  b  truth independent of any solver: the Newton correction (p(x) - t) / p'(x) of every returned x, by Clenshaw in
     extended precision, against that of the nearest root of roots_1d(V - t): at most max(10 x, 1e-13 (b - a))
  c  method 0 equals pcx_cheb1d_calculus on V - t[:, None], bit for bit, at n in {2, 17, 34, 64}
  d  the four classes, 64 rows each, n in {11, 17, 34} along dim: invert_batch equals cheb1d_invert on the fibres the
     model evaluates, roots_batch(level=t) equals the solver on V - t, both bit for bit (the spline per piece, merged by
     the NumPy restatements of the merges); roots(dim, fixed, level=t) equals the one-row batch; on Black-Scholes prices
     in volatility (dense, spline, TT and slider models) every row has status 1, agrees with the single root of roots_batch(level=) within 1e-10 (b - a), and
     the model at the returned point gives the target within 1e-12 max|fibre|
  e  one batch across the pass size (n = 64, 2^15 + 1 rows): the rows on both sides of the edge and the last row equal
     their one-row calls bit for bit
  f  C-ABI argument errors return PCX_ERR_INVALID without a launch

The worst figures of a and b are printed (pytest -s) for DESIGN 3.16."""
import functools
import math
import os

import numpy as np
import pytest

import calc_fibres as CF
import invert_fibres as IF
import functions as F

from pychebyshev_amd import ChebyshevApproximation, ChebyshevSlider, ChebyshevSpline, ChebyshevTT, _calculus, _lib
from pychebyshev_amd.barycentric import chebyshev_nodes, compute_barycentric_weights

pytestmark = pytest.mark.gpu

DOM = (-1.0, 1.0)
SOLVER_N = (1, 2, 3, 16, 17, 18, 33, 34, 63, 64)
BATCHES = (1, 63, 64, 65, 200)
ROWS = 64
STATS = {"a": {}, "b": {"dev": 0.0, "ref": 0.0, "ratio": 0.0, "rows": 0}}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    a, b = STATS["a"], STATS["b"]
    print(f"\ninversion a) {a.get('rows', 0)} rows: worst |x - restatement| {a.get('x', 0.0):.2e} (b - a), bit for bit: "
          f"{a.get('bitwise')}; largest iteration count {a.get('iters', 0)} of {_calculus.INVERT_MAX_ITERS}; "
          f"b) {b['rows']} rows: worst Newton correction {b['dev']:.2e} (nearest eigenvalue root {b['ref']:.2e}), worst "
          f"ratio above the floor {b['ratio']:.2f}; {b.get('unconfirmed', 0)} rows without an eigenvalue root held to the "
          f"floor alone, {b.get('at_end', 0)} rows within 1e-9 of an end not checked")


@functools.lru_cache(maxsize=None)
def _cycled(n):
    """The rows of invert_fibres.inputs(n) cycled to 200, and the restatement on them (computed once per n)."""
    V, t = IF.inputs(n, DOM)
    idx = np.arange(max(BATCHES)) % V.shape[0]
    want_x, want_s, want_it = IF.reference(n, DOM)
    return V[idx], t[idx], want_x[idx], want_s[idx], int(want_it.max())


def _invert(n, V, t, dom=DOM):
    x, w, _ = CF.grid(n, *dom)
    return _calculus.cheb1d_invert(V, t, x, w, dom)


# ------------------------------------------------------------------ a: the restatement, lane tails, batch independence
@pytest.mark.parametrize("n", SOLVER_N)
def test_solver_matches_the_restatement_at_every_batch_size(n):
    V, t, want_x, want_s, iters = _cycled(n)
    STATS["a"]["iters"] = max(STATS["a"].get("iters", 0), iters)
    whole = None
    for N in BATCHES:
        x, s = _invert(n, V[:N], t[:N])
        IF.check(n, x, s, want_x[:N], want_s[:N], DOM, f"N={N}", STATS["a"])
        whole = (x, s)
    for r in (0, 62, 63, 64, 199):
        x, s = _invert(n, V[r:r + 1], t[r:r + 1])
        assert s[0] == whole[1][r] and np.array_equal(x[0], whole[0][r], equal_nan=True), (n, r, x[0], whole[0][r])


@pytest.mark.parametrize("n", [n for n in SOLVER_N if n >= 2])
def test_solver_finds_solutions_at_and_next_to_zero(n):
    """t = 0, +-1e-15 ... +-1e-300 and p(0) from another summation order on strictly increasing fibres
    (invert_fibres.near_zero): status 1 on every row, and the restatement's x."""
    V, t = IF.near_zero(n, DOM)
    want_x, want_s, want_it = IF.near_zero_reference(n, DOM)
    STATS["a"]["iters"] = max(STATS["a"].get("iters", 0), int(want_it.max()))
    x, s = _invert(n, V, t)
    assert np.all(s == 1), (n, s, t[s != 1])
    IF.check(n, x, s, want_x, want_s, DOM, "near zero", STATS["a"])


def test_solver_reports_non_finite_rows_and_leaves_their_neighbours_alone():
    n = 17
    V, t, want_x, want_s, _ = _cycled(n)
    V, t = V[:65].copy(), t[:65].copy()
    V[3, 5], V[40, 0], t[64] = np.nan, np.inf, np.inf
    x, s = _invert(n, V, t)
    bad = np.zeros(65, dtype=bool)
    bad[[3, 40, 64]] = True
    assert np.all(s[bad] == -1) and np.all(np.isnan(x[bad]))
    assert np.array_equal(s[~bad], want_s[:65][~bad]) and np.array_equal(x[~bad], want_x[:65][~bad], equal_nan=True)


# ------------------------------------------------------------------ b: Newton corrections in extended precision
@pytest.mark.parametrize("n", [n for n in SOLVER_N if n >= 2])
def test_returned_points_have_small_newton_corrections(n):
    V, t = IF.inputs(n, DOM)
    x, s = _invert(n, V, t)
    dev, ref, rows, unconfirmed, at_end = IF.newton_ratio(n, V, t, x, s, DOM)
    b = STATS["b"]
    b["dev"], b["ref"], b["rows"] = max(b["dev"], dev), max(b["ref"], ref), b["rows"] + rows
    b["unconfirmed"], b["at_end"] = b.get("unconfirmed", 0) + unconfirmed, b.get("at_end", 0) + at_end
    assert rows + unconfirmed + at_end == int(np.sum(s >= 1))
    if dev > 2e-13:
        b["ratio"] = max(b["ratio"], dev / max(ref, 1e-300))
    print(f"n={n}: Newton correction device {dev:.2e} nearest eigenvalue root {ref:.2e} ({rows} rows; {unconfirmed} more "
          f"without an eigenvalue root held to the floor alone, {at_end} within 1e-9 of an end not checked)")


# ------------------------------------------------------------------ c: method 0
@pytest.mark.parametrize("n", [2, 17, 34, 64])
def test_level_roots_equal_the_solver_on_shifted_fibres(n):
    V, t = IF.inputs(n, DOM)
    x, w, _ = CF.grid(n, *DOM)
    R, cnt = _calculus.cheb1d_level_roots(V, t, x, w, DOM)
    R0, cnt0 = _calculus.cheb1d_calculus(V - t[:, None], x, w, None, DOM, "roots")
    assert np.array_equal(cnt, cnt0) and np.array_equal(R, R0, equal_nan=True)
    assert np.any(cnt > 0)


# ------------------------------------------------------------------ d: the four classes
def _f3(x, _=None):
    return math.sin(12.0 * x[0] + 0.3) + math.cos(9.0 * x[1] + x[2]) - 0.2 * x[2]


def _f2(x, _=None):
    return math.sin(14.0 * x[0] + 0.3) * (1.0 + 0.5 * x[1]) + 0.3 * math.cos(5.0 * x[0]) - 0.1


def _fixed_rows(domain, dim, seed, rows=ROWS):
    rng = np.random.default_rng([17, seed])
    return np.column_stack([rng.uniform(lo, hi, rows) for k, (lo, hi) in enumerate(domain) if k != dim])


def _targets(fib, seed):
    """One target per row between the smallest and the largest value of the row's fibres."""
    rng = np.random.default_rng([19, seed])
    lo, hi = fib.min(axis=1), fib.max(axis=1)
    return lo + rng.uniform(0.05, 0.95, fib.shape[0]) * (hi - lo)


def _check_model(model, d, dim, rows, t, grids, fib):
    """`grids`: [(nodes, weights, (lo, hi))] per piece along dim; `fib`: the pieces' fibres, [(ROWS, n_j)]."""
    x, s = model.invert_batch(dim, rows, t)
    R, cnt = model.roots_batch(dim, rows, level=t)
    px, ps, pr, pc = [], [], [], []
    for (nd, w, pd), v in zip(grids, fib):
        xi, si = _calculus.cheb1d_invert(v, t, nd, w, pd)
        Ri, ci = _calculus.cheb1d_calculus(v - t[:, None], nd, w, None, pd, "roots")
        px.append(xi), ps.append(si), pr.append(Ri), pc.append(ci)
    if len(grids) == 1:
        want_x, want_s, want_R, want_c = px[0], ps[0], pr[0], pc[0]
    else:
        want_x, want_s = _calculus.merge_inversions(np.array(px), np.array(ps))
        dom = (grids[0][2][0], grids[-1][2][1])
        want_c = np.empty(rows.shape[0], dtype=np.int32)
        want_R = np.full(R.shape, np.nan)
        for r in range(rows.shape[0]):
            assert all(c[r] >= 0 for c in pc)
            merged = _calculus.merge_pieces("roots", [Ri[r, :ci[r]] for Ri, ci in zip(pr, pc)], dom)
            want_c[r] = merged.size
            want_R[r, :merged.size] = merged
    assert np.array_equal(s, want_s) and np.array_equal(x, want_x, equal_nan=True), (s, want_s)
    assert np.array_equal(cnt, want_c) and np.array_equal(R, want_R, equal_nan=True)
    assert np.any(s >= 1) and np.any(cnt >= 1)
    others = [k for k in range(d) if k != dim]
    for r in (0, ROWS // 2, ROWS - 1):                      # the single call is the one-row batch
        fixed = {k: float(rows[r, c]) for c, k in enumerate(others)}
        single = model.roots(dim, fixed, level=float(t[r])) if d > 1 else model.roots(level=float(t[r]))
        R1, c1 = model.roots_batch(dim, rows[r:r + 1], level=t[r:r + 1])
        assert np.array_equal(single, R1[0, :c1[0]]) and np.array_equal(R1[0], R[r], equal_nan=True) and c1[0] == cnt[r]
        x1, s1 = model.invert_batch(dim, rows[r:r + 1], t[r:r + 1])
        assert s1[0] == s[r] and np.array_equal(x1[0], x[r], equal_nan=True)


@pytest.mark.parametrize("n", [11, 17, 34])
def test_dense_model(n):
    cols = CF.noise(n)[1][:3].T
    domain = [[-2.0, 3.0], [0.0, 1.0]]
    c = ChebyshevApproximation.from_values(cols, 2, domain, list(cols.shape))
    dim, dom = 0, (-2.0, 3.0)
    rows = _fixed_rows(domain, dim, n)
    pts = np.concatenate([_calculus.fibre_points(2, dim, rows[r], c.nodes[dim]) for r in range(ROWS)])
    fib = c.vectorized_eval_batch(pts, [0, 0]).reshape(ROWS, n)
    _check_model(c, 2, dim, rows, _targets(fib, n), [(c.nodes[dim], c.weights[dim], dom)], [fib])


@pytest.mark.parametrize("n", [11, 17, 34])
def test_tt_model(n):
    rng = np.random.default_rng([13, n])
    cores = [rng.standard_normal(s) for s in ((1, 4, 3), (3, n, 3), (3, 5, 1))]
    domain = [[-1.0, 1.0], [-2.0, 3.0], [0.0, 1.0]]
    tt = ChebyshevTT.from_coeff_cores(cores, domain)
    dim, dom = 1, (-2.0, 3.0)
    rows = _fixed_rows(domain, dim, n)
    x = chebyshev_nodes(dom[0], dom[1], n)
    pts = np.concatenate([_calculus.fibre_points(3, dim, rows[r], x) for r in range(ROWS)])
    fib = tt.eval_batch(pts).reshape(ROWS, n)
    _check_model(tt, 3, dim, rows, _targets(fib, n), [(x, compute_barycentric_weights(x), dom)], [fib])


@pytest.mark.parametrize("n", [11, 17, 34])
def test_slider_model(n):
    domain = [[-1.0, 1.0], [-1.0, 1.0], [0.0, 1.0]]
    for dim, n_nodes in ((1, [5, n, 4]), (0, [n, 5, 4])):       # a two-dimensional owner, and a one-dimensional one
        sl = ChebyshevSlider(_f3, 3, domain, n_nodes, partition=[[0], [1, 2]], pivot_point=[0.1, -0.2, 0.4])
        sl.build(verbose=False)
        dom = tuple(domain[dim])
        x, w, _ = sl._owner_grid(dim)
        rows = _fixed_rows(domain, dim, n)
        pts = np.concatenate([_calculus.fibre_points(3, dim, rows[r], x) for r in range(ROWS)])
        fib = sl.eval_batch(pts, [0, 0, 0]).reshape(ROWS, n)
        _check_model(sl, 3, dim, rows, _targets(fib, n + dim), [(x, w, dom)], [fib])


@pytest.mark.parametrize("pieces,knots", [([11, 17], [0.1]), ([34, 11, 17], [-0.3, 0.4])])
def test_spline_model(pieces, knots):
    domain = [[-1.0, 1.0], [0.0, 1.0]]
    sp = ChebyshevSpline(_f2, 2, domain, n_nodes=[list(pieces), [3]], knots=[list(knots), []])
    sp.build(verbose=False)
    dim = 0
    rows = _fixed_rows(domain, dim, len(pieces))
    _, along, _ = sp._calculus_pieces(dim, {1: float(rows[0, 0])})
    assert [p.n_nodes[dim] for p in along] == list(pieces)
    grids = [(p.nodes[dim], p.weights[dim], tuple(p.domain[dim])) for p in along]
    pts = np.concatenate([_calculus.fibre_points(2, dim, rows[r], g[0]) for r in range(ROWS) for g in grids])
    vals = sp.eval_batch(pts, [0, 0]).reshape(ROWS, sum(pieces))
    fib = [np.ascontiguousarray(v) for v in np.split(vals, np.cumsum(pieces)[:-1], axis=1)]
    _check_model(sp, 2, dim, rows, _targets(vals, len(pieces)), grids, fib)


BS_DOMAIN = [[80.0, 120.0], [0.25, 1.0], [0.15, 0.35]]


def _check_monotone(model, evaluate, fibres, tag, domain=BS_DOMAIN, dim=2):
    """Black-Scholes prices rise with volatility: every target taken from the model itself is reached exactly once."""
    a, b = domain[dim]
    rows = _fixed_rows(domain, dim, 5)
    sig = np.random.default_rng(23).uniform(a + 0.01, b - 0.01, ROWS)
    t = evaluate(np.insert(rows, dim, sig, axis=1))
    x, s = model.invert_batch(dim, rows, t)
    assert np.all(s == 1), (tag, s)
    R, cnt = model.roots_batch(dim, rows, level=t)
    assert np.all(cnt == 1), (tag, cnt)
    assert np.max(np.abs(x - R[:, 0])) <= 1e-10 * (b - a), (tag, np.max(np.abs(x - R[:, 0])))
    back = evaluate(np.insert(rows, dim, x, axis=1))
    scale = np.max(np.abs(fibres(rows)), axis=1)
    worst = float(np.max(np.abs(back - t) / scale))
    print(f"{tag}: |x - root| {np.max(np.abs(x - R[:, 0])) / (b - a):.2e} (b - a), |p(x) - t| {worst:.2e} max|fibre|")
    assert worst <= 1e-12, (tag, worst)


def test_dense_black_scholes_in_volatility():
    c = ChebyshevApproximation(F.bs_3d, 3, BS_DOMAIN, [9, 7, 17])
    c.build(verbose=False)

    def fibres(rows):
        pts = np.concatenate([_calculus.fibre_points(3, 2, rows[r], c.nodes[2]) for r in range(rows.shape[0])])
        return c.vectorized_eval_batch(pts, [0, 0, 0]).reshape(rows.shape[0], -1)
    _check_monotone(c, lambda p: c.vectorized_eval_batch(p, [0, 0, 0]), fibres, "dense BS")


def test_spline_black_scholes_in_volatility():
    sp = ChebyshevSpline(F.bs_3d, 3, BS_DOMAIN, n_nodes=[[7], [5], [11, 11]], knots=[[], [], [0.25]])
    sp.build(verbose=False)
    grid = np.concatenate([chebyshev_nodes(0.15, 0.25, 11), chebyshev_nodes(0.25, 0.35, 11)])

    def fibres(rows):
        pts = np.concatenate([_calculus.fibre_points(3, 2, rows[r], grid) for r in range(rows.shape[0])])
        return sp.eval_batch(pts, [0, 0, 0]).reshape(rows.shape[0], -1)
    _check_monotone(sp, lambda p: sp.eval_batch(p, [0, 0, 0]), fibres, "spline BS")


def test_tt_black_scholes_in_volatility():
    """The 5-D rank-8 Black-Scholes train of the golden vectors, along volatility (user dimension 3, 11 nodes)."""
    g4 = np.load(os.path.join(os.path.dirname(os.path.abspath(F.__file__)), "g4_tt_bs5d.npz"))
    tt = ChebyshevTT.from_coeff_cores([g4[f"r8_core{k}"] for k in range(5)], F.BS5_DOMAIN)
    grid = chebyshev_nodes(F.BS5_DOMAIN[3][0], F.BS5_DOMAIN[3][1], 11)

    def fibres(rows):
        pts = np.concatenate([_calculus.fibre_points(5, 3, rows[r], grid) for r in range(rows.shape[0])])
        return tt.eval_batch(pts).reshape(rows.shape[0], -1)
    _check_monotone(tt, tt.eval_batch, fibres, "TT BS", F.BS5_DOMAIN, 3)


def test_slider_black_scholes_in_volatility():
    """The [[0, 1], [2], [3, 4]] Black-Scholes slider of the golden cases, along volatility (7 nodes, a 2-D owner)."""
    c = F.SLIDER_CASES["b"]
    sl = ChebyshevSlider(getattr(F, c["f"]), c["d"], c["domain"], c["n_nodes"], partition=c["partition"],
                         pivot_point=c["pivot"])
    sl.build(verbose=False)
    grid = sl._owner_grid(3)[0]

    def fibres(rows):
        pts = np.concatenate([_calculus.fibre_points(5, 3, rows[r], grid) for r in range(rows.shape[0])])
        return sl.eval_batch(pts, [0] * 5).reshape(rows.shape[0], -1)
    _check_monotone(sl, lambda p: sl.eval_batch(p, [0] * 5), fibres, "slider BS", c["domain"], 3)


# ------------------------------------------------------------------ e: a batch across the pass size
def test_rows_across_the_pass_edge_equal_their_one_row_calls():
    n, N = 64, 2 ** 15 + 1                                  # 2^21 fibre points per pass / 64 nodes = 2^15 rows
    cols = CF.noise(n)[1][:3].T
    domain = [[-1.0, 1.0], [0.0, 1.0]]
    c = ChebyshevApproximation.from_values(cols, 2, domain, list(cols.shape))
    rows = np.linspace(0.0, 1.0, N).reshape(N, 1)
    t = np.linspace(-0.4, 0.4, N)
    x, s = c.invert_batch(0, rows, t)
    R, cnt = c.roots_batch(0, rows, level=t)
    for r in (0, 2 ** 15 - 2, 2 ** 15 - 1, 2 ** 15):
        x1, s1 = c.invert_batch(0, rows[r:r + 1], t[r:r + 1])
        assert s1[0] == s[r] and np.array_equal(x1[0], x[r], equal_nan=True), (r, x1[0], x[r], s1[0], s[r])
        R1, c1 = c.roots_batch(0, rows[r:r + 1], level=t[r:r + 1])
        assert c1[0] == cnt[r] and np.array_equal(R1[0], R[r], equal_nan=True), r
    assert s[2 ** 15] >= 0 and cnt[2 ** 15] >= 0


# ------------------------------------------------------------------ f: C-ABI argument errors
def test_abi_argument_errors():
    lib = _lib.load()
    n, N = 5, 4
    x, w, _ = CF.grid(n, *DOM)
    V = _lib.f64(CF.noise(n)[1][:N])
    t = _lib.f64(np.zeros(N))
    R, cnt = np.full((N, n - 1), 7.0), np.full(N, 7, dtype=np.int32)
    xo, st = np.full(N, 7.0), np.full(N, 7, dtype=np.int32)

    def call(n_=n, method=1, targets=t, N_=N, outs=None):
        outs = (_lib.p_f64(R), _lib.p_i32(cnt), _lib.p_f64(xo), _lib.p_i32(st)) if outs is None else outs
        return lib.pcx_cheb1d_solve(0, n_, -1.0, 1.0, _lib.p_f64(x), _lib.p_f64(w), _lib.p_f64(V),
                                    _lib.p_f64(targets) if targets is not None else None, N_, method, *outs)
    assert call(targets=None) == _lib.PCX_ERR_INVALID and "targets is NULL" in _lib.last_error(lib)
    assert call(method=2) == _lib.PCX_ERR_INVALID and "method=2" in _lib.last_error(lib)
    assert call(method=-1) == _lib.PCX_ERR_INVALID
    assert call(n_=0) == _lib.PCX_ERR_INVALID and "n=0 outside [1, 64]" in _lib.last_error(lib)
    assert call(n_=65) == _lib.PCX_ERR_INVALID and "n=65 outside [1, 64]" in _lib.last_error(lib)
    assert call(N_=-1) == _lib.PCX_ERR_INVALID
    assert call(method=1, outs=(None, None, None, _lib.p_i32(st))) == _lib.PCX_ERR_INVALID
    assert call(method=0, outs=(None, _lib.p_i32(cnt), None, None)) == _lib.PCX_ERR_INVALID
    assert call(N_=0) == _lib.PCX_OK
    assert np.all(R == 7.0) and np.all(cnt == 7) and np.all(xo == 7.0) and np.all(st == 7)      # no output touched
    # a handle entry: the same checks before any launch
    cols = CF.noise(n)[1][:3].T
    c = ChebyshevApproximation.from_values(cols, 2, [[-1.0, 1.0], [0.0, 1.0]], list(cols.shape))
    m = c._model()
    lo, hi = _lib.f64([-1.0, 0.0]), _lib.f64([1.0, 1.0])
    rows = _lib.f64(np.full((N, 1), 0.5))

    def hcall(handle=m.handle, dim=0, targets=t, method=1, rws=rows):
        return m.lib.pcx_bary_solve_batch(handle, dim, _lib.p_f64(lo), _lib.p_f64(hi), _lib.p_f64(rws),
                                          _lib.p_f64(targets) if targets is not None else None, N, method,
                                          _lib.p_f64(R), _lib.p_i32(cnt), _lib.p_f64(xo), _lib.p_i32(st))
    assert hcall(handle=None) == _lib.PCX_ERR_INVALID
    assert hcall(dim=2) == _lib.PCX_ERR_INVALID
    assert hcall(targets=None) == _lib.PCX_ERR_INVALID
    assert hcall(method=3) == _lib.PCX_ERR_INVALID and "method=3" in _lib.last_error(lib)
    assert hcall(rws=_lib.f64(np.full((N, 1), 2.0))) == _lib.PCX_ERR_INVALID and "outside domain" in _lib.last_error(lib)
    assert np.all(R == 7.0) and np.all(cnt == 7) and np.all(xo == 7.0) and np.all(st == 7)
    assert hcall() == _lib.PCX_OK and np.all(st != 7)
