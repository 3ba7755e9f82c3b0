"""ChebyshevSpline batched calculus, slice and extrude on the device (pcx_spline_calculus_batch: k_spline_calc_expand, the
spline's own chunk evaluation, k_cheb1d_calculus_pieces, k_spline_calc_merge; slice through the pieces' axis contraction)
against the reference's values (golden g26), the per-piece route of the single calls restated from the pieces' public
methods, the solver on its own, and themselves (batch = rows).

Bounds as in test_gpu_calculus.py: roots 1e-10 (b - a) with equal counts in every row (the golden roots keep 1e-6 (b - a)
from every piece edge and from each other, so a count cannot hang on a last bit), values 1e-12 max|fibre|, well-defined
locations 1e-8 (b - a), a location further off must be an equally good point.  Splines: structure equal, tensors 1e-12
normwise (exactly equal for extrude, a copy, and for a slice at a node, a one-hot contraction), values at the golden
points assert_parity 1e-12."""
import numpy as np
import pytest

from conftest import assert_parity, golden

import generate_golden_spline_transforms as G
from pychebyshev_amd import ChebyshevApproximation, ChebyshevSpline, _calculus, _lib

pytestmark = pytest.mark.gpu

CALC_CHUNK_POINTS = 1 << 21          # kCalcChunkPoints of pcx_calculus.hip


@pytest.fixture(scope="module")
def g26():
    return golden("g26_spline_transforms")


def _check_roots(got, want, a, b, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, got, want)
    if want.size:
        assert float(np.max(np.abs(got - want))) / (b - a) <= 1e-10, (tag, got, want)


def _check_opt(got, want, scale, a, b, value_at, tag):
    """got / want = (value, location); value_at(x) evaluates the interpolant along the fibre."""
    assert abs(got[0] - want[0]) / scale <= 1e-12, (tag, got, want)
    if abs(got[1] - want[1]) / (b - a) > 1e-8:      # not well defined: a flat optimum or a tie -- the point found must be as good
        assert a <= got[1] <= b, (tag, got, want)
        assert abs(value_at(got[1]) - want[0]) <= 1e-12 * scale, (tag, got, want)


def _scale(own, source):
    """The scale of a bound on numbers contracted from a tensor: max|own| -- unless that is rounding noise of the data
    (below 1e-13 max|source|), then max|source|.  Case z vanishes identically on x0 = 0.2, the knot its rows and one of
    its slices sit on: the exact fibre is zero, the reference's own values there are 1e-17 next to tensors of size 1, and
    a bound relative to them would test nothing."""
    return own if own >= 1e-13 * source else source


_BUILT = {}


def _spline(case) -> ChebyshevSpline:
    if case not in _BUILT:
        _BUILT[case] = G.build(ChebyshevSpline, case)
    return _BUILT[case]


def _others(d, dim):
    return [k for k in range(d) if k != dim]


def _fixed(d, dim, row):
    return {k: float(v) for k, v in zip(_others(d, dim), row)} if d > 1 else None


def _pieces(sp, dim, row):
    """The pieces along dim that the row selects, and the fixed values as the pieces' own calls take them."""
    _, pieces, sub = sp._calculus_pieces(dim, _fixed(sp.num_dimensions, dim, row))
    return pieces, sub


def _fibres(sp, dim, row):
    """Every selected piece's fibre: the spline's evaluation at (row..., the piece's nodes along dim), one call."""
    pieces, _ = _pieces(sp, dim, row)
    d = sp.num_dimensions
    pts = np.concatenate([_calculus.fibre_points(d, dim, np.asarray(row, dtype=float), p.nodes[dim]) for p in pieces])
    vals = sp.eval_batch(pts, [0] * d)
    cuts = np.cumsum([p.n_nodes[dim] for p in pieces])[:-1]
    return pieces, np.split(vals, cuts)


def _value_at(sp, dim, row):
    def at(t):
        pt = list(row)
        pt.insert(dim, float(t))
        return float(sp.eval(pt, [0] * sp.num_dimensions))
    return at


def _parent_route(sp, dim, row, mode):
    """What the single calls did before the batch existed: every piece's own call, merged on the host."""
    pieces, sub = _pieces(sp, dim, row)
    if mode == "roots":
        return _calculus.merge_pieces("roots", [p.roots(dim, sub) for p in pieces], sp.domain[dim])
    return _calculus.merge_pieces(mode, [(p.minimize if mode == "min" else p.maximize)(dim, sub) for p in pieces])


# ------------------------------------------------------------------ reference parity
@pytest.mark.parametrize("case", sorted(G.CASES))
def test_calculus_matches_reference_single_and_batch(g26, case):
    sp = _spline(case)
    d = sp.num_dimensions
    seen = set()
    for dim in range(d):
        rows = G.calculus_rows(case, dim)
        assert np.array_equal(rows, g26[f"{case}_d{dim}_rows"]), "seeded golden rows no longer regenerate"
        a, b = sp.domain[dim]
        want_R, want_n = g26[f"{case}_d{dim}_roots"], g26[f"{case}_d{dim}_count"]
        R, cnt = sp.roots_batch(dim, rows)
        vmin, lmin = sp.minimize_batch(dim, rows)
        vmax, lmax = sp.maximize_batch(dim, rows)
        print(f"{case} dim {dim}: counts {cnt.tolist()} reference {want_n.tolist()}")
        assert R.shape == want_R.shape and R.dtype == np.float64 and cnt.dtype == np.int32 and cnt.shape == (rows.shape[0],)
        assert vmin.shape == lmin.shape == vmax.shape == lmax.shape == (rows.shape[0],)
        assert np.array_equal(cnt, want_n), (case, dim, cnt, want_n)
        seen |= set(want_n.tolist())
        for r, row in enumerate(rows):
            tag = f"{case} dim {dim} row {r}"
            fixed = _fixed(d, dim, row)
            pieces, fibres = _fibres(sp, dim, row)
            scale = _scale(float(np.max(np.abs(np.concatenate(fibres)))), max(float(np.max(np.abs(p.tensor_values))) for p in pieces))
            at = _value_at(sp, dim, row)
            k = int(want_n[r])
            _check_roots(R[r, :k], want_R[r, :k], a, b, tag + " roots_batch")
            assert np.all(np.isnan(R[r, k:])), tag
            _check_opt((vmin[r], lmin[r]), g26[f"{case}_d{dim}_min"][r], scale, a, b, at, tag + " minimize_batch")
            _check_opt((vmax[r], lmax[r]), g26[f"{case}_d{dim}_max"][r], scale, a, b, at, tag + " maximize_batch")
            _check_roots(sp.roots(dim, fixed), want_R[r, :k], a, b, tag + " roots")
            _check_opt(sp.minimize(dim, fixed), g26[f"{case}_d{dim}_min"][r], scale, a, b, at, tag + " min")
            _check_opt(sp.maximize(dim, fixed), g26[f"{case}_d{dim}_max"][r], scale, a, b, at, tag + " max")
    if case == "k":
        assert {0, 1, 2} <= seen
    if case in ("m", "o"):
        assert max(seen) >= 5
    if case == "z":       # both pieces along dimension 0 find the root on the knot; the merge returns it once
        assert np.all(g26["z_d0_count"] == 1)


# ------------------------------------------------------------------ batch = rows = the per-piece route, bit for bit
@pytest.mark.parametrize("case,dim", [("k", 0), ("k", 1), ("m", 0), ("m", 2), ("o", 0)])
def test_batch_rows_are_bitwise_the_one_row_calls_and_the_piece_route(case, dim):
    """N = 1, 67 and, for (m, 0), one N just over a pass of kCalcChunkPoints fibre points: the short rows repeated, every
    tile compared with the first, the first with one-row calls, and every row with the per-piece route.  k: nested,
    unequal pieces (one launch per piece); m: equal pieces (the one-launch evaluation); o: one dimension."""
    sp = _spline(case)
    d = sp.num_dimensions
    short = G.calculus_rows(case, dim)
    S = short.shape[0]
    F = sum(sp._dim_counts(dim))
    ones = [sp.roots_batch(dim, short[r:r + 1]) for r in range(S)]
    ones_min = [sp.minimize_batch(dim, short[r:r + 1]) for r in range(S)]
    ones_max = [sp.maximize_batch(dim, short[r:r + 1]) for r in range(S)]
    for r in range(S):
        k = int(ones[r][1][0])
        assert k >= 0
        want = _parent_route(sp, dim, short[r], "roots")
        assert np.array_equal(ones[r][0][0, :k], want) and np.all(np.isnan(ones[r][0][0, k:])), (case, dim, r)
        assert (ones_min[r][0][0], ones_min[r][1][0]) == _parent_route(sp, dim, short[r], "min"), (case, dim, r)
        assert (ones_max[r][0][0], ones_max[r][1][0]) == _parent_route(sp, dim, short[r], "max"), (case, dim, r)
        fixed = _fixed(d, dim, short[r])
        assert np.array_equal(sp.roots(dim, fixed), want)
        assert sp.minimize(dim, fixed) == (ones_min[r][0][0], ones_min[r][1][0])
        assert sp.maximize(dim, fixed) == (ones_max[r][0][0], ones_max[r][1][0])
    sizes = [1, 67] + ([CALC_CHUNK_POINTS // F + 3] if (case, dim) == ("m", 0) else [])
    for N in sizes:
        idx = np.arange(N) % S
        R, cnt = sp.roots_batch(dim, short[idx])
        val, loc = sp.minimize_batch(dim, short[idx])
        vmx, lmx = sp.maximize_batch(dim, short[idx])
        for r in range(min(S, N)):
            assert cnt[r] == ones[r][1][0] and np.array_equal(R[r], ones[r][0][0], equal_nan=True), (case, dim, N, r)
            assert val[r] == ones_min[r][0][0] and loc[r] == ones_min[r][1][0], (case, dim, N, r)
            assert vmx[r] == ones_max[r][0][0] and lmx[r] == ones_max[r][1][0], (case, dim, N, r)
        full = (N // S) * S
        if full > S:
            assert np.array_equal(cnt[:full].reshape(-1, S), np.broadcast_to(cnt[:S], (full // S, S)))
            assert np.array_equal(R[:full].reshape(full // S, S, -1), np.broadcast_to(R[:S], (full // S,) + R[:S].shape),
                                  equal_nan=True), (case, dim, N)
            for got in (val, loc, vmx, lmx):
                assert np.array_equal(got[:full].reshape(-1, S), np.broadcast_to(got[:S], (full // S, S)))
                assert np.array_equal(got[full:], got[:N - full])
            assert np.array_equal(cnt[full:], cnt[:N - full]) and np.array_equal(R[full:], R[:N - full], equal_nan=True)


@pytest.mark.parametrize("case,dim", [("k", 0), ("m", 0), ("m", 2)])
def test_batch_is_the_solver_on_the_evaluated_fibres(case, dim):
    """Each piece's fibre from eval_batch at the fibre points, solved through pcx_cheb1d_calculus and merged on the host."""
    sp = _spline(case)
    rows = G.calculus_rows(case, dim)
    R, cnt = sp.roots_batch(dim, rows)
    vmin, lmin = sp.minimize_batch(dim, rows)
    vmax, lmax = sp.maximize_batch(dim, rows)
    for r in (0, 3, rows.shape[0] - 2, rows.shape[0] - 1):
        pieces, fibres = _fibres(sp, dim, rows[r])
        found, counts, lows, highs = [], [], [], []
        for p, v in zip(pieces, fibres):
            dom = (p.domain[dim][0], p.domain[dim][1])
            Rp, n = _calculus.cheb1d_calculus(v, p.nodes[dim], p.weights[dim], None, dom, "roots")
            found.append(Rp[0, :max(int(n[0]), 0)])
            counts.append(n[0])
            lo_v, lo_x, _ = _calculus.cheb1d_calculus(v, p.nodes[dim], p.weights[dim], p.diff_matrices[dim], dom, "min")
            hi_v, hi_x, _ = _calculus.cheb1d_calculus(v, p.nodes[dim], p.weights[dim], p.diff_matrices[dim], dom, "max")
            lows.append((lo_v[0], lo_x[0]))
            highs.append((hi_v[0], hi_x[0]))
        want = _calculus.merge_pieces("roots", found, sp.domain[dim], counts=counts)
        assert cnt[r] == want.size and np.array_equal(R[r, :cnt[r]], want), (case, dim, r)
        assert (vmin[r], lmin[r]) == _calculus.merge_pieces("min", lows), (case, dim, r)
        assert (vmax[r], lmax[r]) == _calculus.merge_pieces("max", highs), (case, dim, r)


def test_a_failed_piece_fails_its_rows_only():
    good = _spline("k")
    bad = G.build(ChebyshevSpline, "k")
    broken = bad._pieces[2]                                      # piece (1, 0): x0 >= 0.2, x1 < 0.5
    broken.tensor_values = np.full_like(broken.tensor_values, np.nan)   # rebinding: the device copies follow
    rows = G.calculus_rows("k", 0)                               # column: x1; the knot row (0.5) belongs to the right piece
    hit = rows[:, 0] < 0.5
    assert hit.any() and (~hit).any()
    R0, n0 = good.roots_batch(0, rows)
    R, n = bad.roots_batch(0, rows)
    assert np.all(n[hit] == -1) and np.all(np.isnan(R[hit]))
    assert np.array_equal(n[~hit], n0[~hit]) and np.array_equal(R[~hit], R0[~hit], equal_nan=True)
    for fn_bad, fn_good in ((bad.minimize_batch, good.minimize_batch), (bad.maximize_batch, good.maximize_batch)):
        v, x = fn_bad(0, rows)
        v0, x0 = fn_good(0, rows)
        assert np.all(np.isnan(v[hit])) and np.all(np.isnan(x[hit]))
        assert np.array_equal(v[~hit], v0[~hit]) and np.array_equal(x[~hit], x0[~hit])
    r = int(np.nonzero(hit)[0][0])
    for fn in (bad.roots, bad.minimize, bad.maximize):
        with pytest.raises(np.linalg.LinAlgError):
            fn(0, {1: float(rows[r, 0])})
    # along dimension 1 the broken piece is index 0 of the rows with x0 >= 0.2
    rows1 = G.calculus_rows("k", 1)
    hit1 = rows1[:, 0] >= 0.2
    R1, n1 = bad.roots_batch(1, rows1)
    R10, n10 = good.roots_batch(1, rows1)
    assert np.all(n1[hit1] == -1) and np.all(np.isnan(R1[hit1]))
    assert np.array_equal(n1[~hit1], n10[~hit1]) and np.array_equal(R1[~hit1], R10[~hit1], equal_nan=True)


def test_long_pieces_keep_the_per_piece_route():
    """70 nodes in one piece along the dimension: the batch refuses, the single calls solve piece by piece."""
    sp = ChebyshevSpline(lambda x, _=None: np.sin(9.0 * x[0]) + 0.3 * x[1], 2, [[-1.0, 1.0], [0.0, 1.0]],
                         n_nodes=[[9, 70], [5]], knots=[[-0.5], []])
    sp.build(verbose=False)
    with pytest.raises(ValueError, match="70 nodes"):
        sp.roots_batch(0, np.array([[0.4]]))
    got = sp.roots(0, {1: 0.4})
    assert np.array_equal(got, _parent_route(sp, 0, [0.4], "roots")) and got.size >= 4
    assert sp.minimize(0, {1: 0.4}) == _parent_route(sp, 0, [0.4], "min")
    R, cnt = sp.roots_batch(1, np.array([[0.3], [-0.7]]))        # the other dimension is short: its batch runs
    assert R.shape == (2, 4) and np.all(cnt >= 0)


# ------------------------------------------------------------------ the C entry
def test_c_entry_validates_before_any_launch():
    sp = _spline("m")
    s = sp._dev()
    lib = s.lib
    lo = _lib.f64([b[0] for b in sp.domain])
    hi = _lib.f64([b[1] for b in sp.domain])
    rows = _lib.f64(G.calculus_rows("m", 0))
    N = rows.shape[0]
    R = np.full((N, 32), 7.0)
    cnt = np.full(N, 7, dtype=np.int32)
    val, loc = np.full(N, 7.0), np.full(N, 7.0)

    def call(handle, dim, mode, n, rws=rows, r=R, c=cnt, v=val, x=loc):
        return lib.pcx_spline_calculus_batch(handle, dim, _lib.p_f64(lo), _lib.p_f64(hi), _lib.p_f64(rws), n, mode,
                                             None if r is None else _lib.p_f64(r), None if c is None else _lib.p_i32(c),
                                             None if v is None else _lib.p_f64(v), None if x is None else _lib.p_f64(x))
    assert call(None, 0, 0, N) == _lib.PCX_ERR_INVALID
    assert call(s.handle, 0, 3, N) == _lib.PCX_ERR_INVALID and "mode=3" in _lib.last_error(lib)
    assert call(s.handle, 0, -1, N) == _lib.PCX_ERR_INVALID
    assert call(s.handle, 3, 0, N) == _lib.PCX_ERR_INVALID
    assert call(s.handle, -1, 0, N) == _lib.PCX_ERR_INVALID
    assert call(s.handle, 0, 0, N, r=None) == _lib.PCX_ERR_INVALID
    assert call(s.handle, 0, 0, N, c=None) == _lib.PCX_ERR_INVALID
    assert call(s.handle, 0, 1, N, v=None) == _lib.PCX_ERR_INVALID
    assert call(s.handle, 0, 2, N, x=None) == _lib.PCX_ERR_INVALID
    bad = rows.copy()
    bad[3, 0] = 0.3                                   # dimension 1 lives in [0.01, 0.25]
    assert call(s.handle, 0, 0, N, bad) == _lib.PCX_ERR_INVALID
    assert "for dim 1" in _lib.last_error(lib) and "(row 3)" in _lib.last_error(lib)
    assert call(s.handle, 0, 0, 0) == _lib.PCX_OK and call(s.handle, 2, 1, 0) == _lib.PCX_OK
    assert np.all(R == 7.0) and np.all(cnt == 7) and np.all(val == 7.0) and np.all(loc == 7.0)   # no output touched
    # and a run through ctypes equals the Python call
    assert call(s.handle, 0, 0, N) == _lib.PCX_OK
    R2, n2 = sp.roots_batch(0, rows)
    assert np.array_equal(R, R2, equal_nan=True) and np.array_equal(cnt, n2)
    mixed = G.build_mixed(ChebyshevSpline, ChebyshevApproximation)      # index 0 along dimension 0: pieces of 5 and 7 nodes
    sm = mixed._dev()
    one = _lib.f64([[0.3]])
    mlo, mhi = _lib.f64([-1.0, 0.0]), _lib.f64([1.0, 1.0])
    out6 = np.full(6, 7.0)
    assert lib.pcx_spline_calculus_batch(sm.handle, 0, _lib.p_f64(mlo), _lib.p_f64(mhi), _lib.p_f64(one), 1, 0,
                                         _lib.p_f64(out6), _lib.p_i32(cnt), None, None) == _lib.PCX_ERR_INVALID
    assert "nodes along dim 0" in _lib.last_error(lib) and np.all(out6 == 7.0)
    assert lib.pcx_spline_calculus_batch(sm.handle, 1, _lib.p_f64(mlo), _lib.p_f64(mhi), _lib.p_f64(one), 1, 0,
                                         _lib.p_f64(out6), _lib.p_i32(cnt), None, None) == _lib.PCX_OK
    assert mixed.roots(0, {1: 0.3}).size >= 1                      # the single call takes the per-piece route
    long = ChebyshevSpline(lambda x, _=None: np.sin(9.0 * x[0]), 1, [[-1.0, 1.0]], n_nodes=[[9, 70]], knots=[[-0.5]])
    long.build(verbose=False)
    sl = long._dev()
    assert lib.pcx_spline_calculus_batch(sl.handle, 0, _lib.p_f64(_lib.f64([-1.0])), _lib.p_f64(_lib.f64([1.0])), None, 1, 0,
                                         _lib.p_f64(np.empty(77)), _lib.p_i32(cnt), None, None) == _lib.PCX_ERR_INVALID


# ------------------------------------------------------------------ slice
ON_NODE = {("k", 2), ("m", 4), ("m", 6)}          # SLICE_SETS entries whose value is a node of the piece it lands in


def _lift(points, params, d):
    """Points of the sliced spline back in the source's d dimensions."""
    fixed = dict(params)
    out = np.empty((points.shape[0], d))
    col = 0
    for k in range(d):
        if k in fixed:
            out[:, k] = fixed[k]
        else:
            out[:, k] = points[:, col]
            col += 1
    return out


@pytest.mark.parametrize("case", sorted(G.SLICE_SETS))
def test_slice_matches_reference(g26, case):
    sp = _spline(case)
    sp._dev()                                                      # the result stays on the source's device index
    for i, params in enumerate(G.SLICE_SETS[case]):
        tag = f"{case}_sl{i}"
        want = G.stored_spline(g26, tag)
        got = sp.slice(params if len(params) > 1 else params[0])
        G.check_structure(got, want, sp, tag)
        source = max(float(np.max(np.abs(p.tensor_values))) for p in sp._pieces)
        scale = _scale(max(float(np.max(np.abs(t))) for t in want["tensors"]), source)
        floor = scale if scale == source else 0.0
        for piece, t in zip(got._pieces, want["tensors"]):
            if (case, i) in ON_NODE:
                assert np.array_equal(piece.tensor_values, t), tag
            assert np.max(np.abs(piece.tensor_values - t)) <= 1e-12 * scale, tag
        pts = g26[f"{tag}_points"]
        vals = got.eval_batch(pts, [0] * got.num_dimensions)
        assert_parity(vals, g26[f"{tag}_values"], 1e-12, tag, floor=floor)
        lifted = sp.eval_batch(_lift(pts, params, sp.num_dimensions), [0] * sp.num_dimensions)
        assert_parity(vals, lifted, 1e-12, tag + " against the source at the lifted points", floor=floor)
    assert sp.num_dimensions == G.CASES[case]["d"] and sp._built


@pytest.mark.parametrize("case", ["k", "m"])
def test_roots_equal_the_reference_route_on_the_new_host_code(case):
    """The reference's roots(): slice to a 1-D spline, then its roots()."""
    sp = _spline(case)
    d = sp.num_dimensions
    for dim in range(d):
        a, b = sp.domain[dim]
        for r, row in enumerate(G.calculus_rows(case, dim)):
            fixed = _fixed(d, dim, row)
            one = sp.slice(list(fixed.items()))
            assert one.num_dimensions == 1 and one._shape == (sp._shape[dim],) and one.knots == [list(sp.knots[dim])]
            _check_roots(sp.roots(dim, fixed), one.roots(), a, b, f"{case} dim {dim} row {r}")


# ------------------------------------------------------------------ extrude
@pytest.mark.parametrize("case", sorted(G.EXTRUDE_SETS))
def test_extrude_evaluates_to_the_reference_and_slices_back(g26, case):
    sp = _spline(case)
    for i, params in enumerate(G.EXTRUDE_SETS[case]):
        tag = f"{case}_ex{i}"
        got = sp.extrude(params)
        G.check_structure(got, G.stored_spline(g26, tag), sp, tag)
        pts = g26[f"{tag}_points"]
        vals = got.eval_batch(pts, [0] * got.num_dimensions)
        assert_parity(vals, g26[f"{tag}_values"], 1e-12, tag)
        for dim_idx, (lo, hi), _n in params:                       # any coordinate in a new dimension: the same value
            for x in (lo, hi, 0.5 * (lo + hi)):
                moved = pts.copy()
                moved[:, dim_idx] = x
                assert_parity(got.eval_batch(moved, [0] * got.num_dimensions), vals, 1e-12, f"{tag} new dim {dim_idx} at {x}")
        back = got.slice([(dim_idx, lo + 0.3 * (hi - lo)) for dim_idx, (lo, hi), _n in params])
        assert back.num_dimensions == sp.num_dimensions and back.knots == [list(k) for k in sp.knots]
        assert back._shape == sp._shape and back.n_nodes == sp.n_nodes
        for p, q in zip(back._pieces, sp._pieces):
            assert np.max(np.abs(p.tensor_values - q.tensor_values)) <= 1e-12 * np.max(np.abs(q.tensor_values)), tag


def test_dense_extrude_evaluates_to_the_reference(g26):
    c = G.build_dense(ChebyshevApproximation)
    for i, params in enumerate(G.DENSE_EXTRUDE_SETS):
        tag = f"dense_ex{i}"
        got = c.extrude(params)
        pts = g26[f"{tag}_points"]
        vals = got.vectorized_eval_batch(pts, [0] * got.num_dimensions)
        assert_parity(vals, g26[f"{tag}_values"], 1e-12, tag)
        for dim_idx, (lo, hi), _n in params:
            moved = pts.copy()
            moved[:, dim_idx] = lo
            assert_parity(got.vectorized_eval_batch(moved, [0] * got.num_dimensions), vals, 1e-12, f"{tag} new dim {dim_idx}")
        back = got.slice([(dim_idx, 0.5 * (lo + hi)) for dim_idx, (lo, hi), _n in params])
        assert np.max(np.abs(back.tensor_values - c.tensor_values)) <= 1e-12 * np.max(np.abs(c.tensor_values))


# ------------------------------------------------------------------ serialisation
@pytest.mark.parametrize("fmt", ["pickle", "binary"])
def test_a_sliced_spline_saves_and_loads(tmp_path, fmt):
    sp = _spline("m")
    cut = sp.slice((1, 0.1))                                       # flat n_nodes: the .pcb format takes it
    path = tmp_path / ("cut.pkl" if fmt == "pickle" else "cut.pcb")
    cut.save(str(path), format=fmt)
    back = ChebyshevSpline.load(str(path))
    assert back.num_dimensions == 2 and back.knots == cut.knots and back.n_nodes == cut.n_nodes and back._shape == cut._shape
    assert [list(b) for b in back.domain] == [list(b) for b in cut.domain]
    for p, q in zip(back._pieces, cut._pieces):
        assert np.array_equal(p.tensor_values, q.tensor_values)
    pts = G.points_in(cut.domain, [11])
    assert np.array_equal(back.eval_batch(pts, [0, 0]), cut.eval_batch(pts, [0, 0]))
    rows = G.calculus_rows("m", 0)[:, 1:]                          # the rows of (m, 0) without the sliced dimension
    R1, n1 = back.roots_batch(0, rows)
    R2, n2 = cut.roots_batch(0, rows)
    assert np.array_equal(n1, n2) and np.array_equal(R1, R2, equal_nan=True)
