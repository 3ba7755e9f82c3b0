"""ChebyshevSlider calculus, slice, extrude and box integrals on the device (pcx_slider_calculus_batch: the other slides
once per row, the owner once per fibre point or not at all, k_slider_fibre_sum, k_cheb1d_calculus; pcx_slider_box_batch:
k_slider_box_row, the slides' box launches, k_slider_box_combine) against the reference's values (golden g25), the
reference's own route restated on the new host code, and themselves (batch = rows).

Bounds as in test_gpu_calculus.py: roots 1e-10 (b - a) with equal counts, values 1e-12 max|fibre|, well-defined
locations 1e-8 (b - a), a location further off must be an equally good point.  Sliders: structure equal, pivot value and
tensors 1e-12 normwise, values at the golden points assert_parity 1e-12.  Scalars (full integrals) are compared on the
scale vol_T max_i max|slide_i tensor|, which does not depend on the code under test: case a's full-domain integral is
-5e-16 in the reference, a relative bound on it would test nothing."""
import ctypes

import numpy as np
import pytest

from conftest import assert_parity, golden

import generate_golden_slider_calculus as G
from pychebyshev_amd import ChebyshevApproximation, ChebyshevSlider, _calculus, _lib

pytestmark = pytest.mark.gpu

CALC_CHUNK_POINTS = 1 << 21          # kCalcChunkPoints of pcx_calculus.hip
BOX_CHUNK_ROWS = 1 << 20             # kSliderBoxChunk of pcx_slider_box.hip


@pytest.fixture(scope="module")
def g25():
    return golden("g25_slider_calculus")


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


def _bary(v, x, w):
    def at(t):
        d = t - x
        hit = np.nonzero(np.abs(d) < 1e-14)[0]
        if hit.size:
            return float(v[hit[0]])
        u = w / d
        return float(u @ v / u.sum())
    return at


_BUILT = {}


def _slider(case) -> ChebyshevSlider:
    if case not in _BUILT:
        _BUILT[case] = G.build(ChebyshevSlider, case)
    return _BUILT[case]


def _others(d, dim):
    return [k for k in range(d) if k != dim]


def _fibre(sl, dim, row):
    nodes, weights, _ = sl._owner_grid(dim)
    v = sl.eval_batch(_calculus.fibre_points(sl.num_dimensions, dim, np.asarray(row, dtype=float), nodes), [0] * sl.num_dimensions)
    return v, nodes, weights


def _tensor_scale(sl, vol=1.0):
    return vol * max(float(np.max(np.abs(s.tensor_values))) for s in sl.slides)


# ------------------------------------------------------------------ roots, minima, maxima
@pytest.mark.parametrize("case", sorted(G.CASES))
def test_calculus_matches_reference_single_and_batch(g25, case):
    sl = _slider(case)
    d = sl.num_dimensions
    for dim in range(d):
        rows = G.calculus_rows(case, dim)
        assert np.array_equal(rows, g25[f"{case}_d{dim}_rows"]), "seeded golden rows no longer regenerate"
        a, b = sl.domain[dim]
        want_R, want_n = g25[f"{case}_d{dim}_roots"], g25[f"{case}_d{dim}_count"]
        batch = sl.n_nodes[dim] <= _calculus.MAX_DEVICE_N
        if batch:
            R, cnt = sl.roots_batch(dim, rows)
            vmin, lmin = sl.minimize_batch(dim, rows)
            vmax, lmax = sl.maximize_batch(dim, rows)
            assert R.shape == want_R.shape and cnt.dtype == np.int32 and vmin.shape == lmax.shape == (rows.shape[0],)
            assert np.array_equal(cnt, want_n), (case, dim, cnt, want_n)
        for r, row in enumerate(rows):
            tag = f"{case} dim {dim} row {r}"
            fixed = {k: float(v) for k, v in zip(_others(d, dim), row)}
            v, nodes, weights = _fibre(sl, dim, row)
            at = _bary(v, nodes, weights)
            scale = max(float(np.max(np.abs(v))), 1e-300)
            k = int(want_n[r])
            _check_roots(sl.roots(dim, fixed), want_R[r, :k], a, b, tag + " roots")
            _check_opt(sl.minimize(dim, fixed), g25[f"{case}_d{dim}_min"][r], scale, a, b, at, tag + " min")
            _check_opt(sl.maximize(dim, fixed), g25[f"{case}_d{dim}_max"][r], scale, a, b, at, tag + " max")
            if batch:
                _check_roots(R[r, :k], want_R[r, :k], a, b, tag + " roots_batch")
                assert np.all(np.isnan(R[r, k:]))
                _check_opt((vmin[r], lmin[r]), g25[f"{case}_d{dim}_min"][r], scale, a, b, at, tag + " minimize_batch")
                _check_opt((vmax[r], lmax[r]), g25[f"{case}_d{dim}_max"][r], scale, a, b, at, tag + " maximize_batch")
    if case == "c":       # the case was chosen for fibres with 0, 1 and 2 roots
        assert {0, 1, 2} <= set(np.concatenate([g25[f"c_d{k}_count"] for k in range(4)]).tolist())
    if case == "l":
        assert g25["l_d0_count"][0] == 5


@pytest.mark.parametrize("case,dim", [("b", 4), ("a", 0), ("b", 2)])
def test_batch_rows_are_bitwise_the_one_row_calls(case, dim):
    """N = 1, 67 and one N just over a pass of kCalcChunkPoints fibre points: a short set of rows repeated, every block
    compared with the first and the first with one-row calls.  (b, 4): the dimension with the fewest nodes, owner
    [3, 4]; (a, 0) and (b, 2): one-dimensional owners, whose fibre is the slide's value tensor."""
    sl = _slider(case)
    n = sl.n_nodes[dim]
    short = G.calculus_rows(case, dim)
    S = short.shape[0]
    ones = [sl.roots_batch(dim, short[r:r + 1]) for r in range(S)]
    ones_min = [sl.minimize_batch(dim, short[r:r + 1]) for r in range(S)]
    sizes = [1, 67] + ([CALC_CHUNK_POINTS // n + 3] if (case, dim) != ("b", 2) else [])
    for N in sizes:
        idx = np.arange(N) % S
        R, cnt = sl.roots_batch(dim, short[idx])
        val, loc = sl.minimize_batch(dim, short[idx])
        for r in range(min(S, N)):
            assert cnt[r] == ones[r][1][0] and np.array_equal(R[r], ones[r][0][0], equal_nan=True), (case, dim, N, r)
            assert val[r] == ones_min[r][0][0] and loc[r] == ones_min[r][1][0], (case, dim, N, r)
        full = (N // S) * S
        if full > S:
            assert np.array_equal(cnt[:full].reshape(-1, S), np.broadcast_to(cnt[:S], (full // S, S)))
            assert np.array_equal(R[:full].reshape(full // S, S, -1), np.broadcast_to(R[:S], (full // S,) + R[:S].shape),
                                  equal_nan=True), (case, dim, N)
            assert np.array_equal(val[:full].reshape(-1, S), np.broadcast_to(val[:S], (full // S, S)))
            assert np.array_equal(loc[:full].reshape(-1, S), np.broadcast_to(loc[:S], (full // S, S)))
            assert np.array_equal(cnt[full:], cnt[:N - full]) and np.array_equal(val[full:], val[:N - full])
    # the single calls are the one-row batches, and the fibre is the evaluation's: eval_batch at the fibre points, solved
    # through pcx_cheb1d_calculus, gives the same bits
    a, b = sl.domain[dim]
    for r in (0, S - 2, S - 1):
        fixed = {k: float(v) for k, v in zip(_others(sl.num_dimensions, dim), short[r])}
        v, nodes, weights = _fibre(sl, dim, short[r])
        R1, n1 = _calculus.cheb1d_calculus(v, nodes, weights, None, (a, b), "roots")
        assert n1[0] == ones[r][1][0] and np.array_equal(R1[0], ones[r][0][0], equal_nan=True), (case, dim, r)
        assert np.array_equal(sl.roots(dim, fixed), ones[r][0][0, :ones[r][1][0]])
        assert sl.minimize(dim, fixed) == (ones_min[r][0][0], ones_min[r][1][0])


@pytest.mark.parametrize("case", ["b", "c"])
def test_roots_equal_the_reference_route_on_the_new_host_code(case):
    """The reference's roots(): slice to one dimension, evaluate at the nodes, from_values(...).roots()."""
    sl = _slider(case)
    d = sl.num_dimensions
    for dim in range(d):
        a, b = sl.domain[dim]
        for r, row in enumerate(G.calculus_rows(case, dim)):
            fixed = {k: float(v) for k, v in zip(_others(d, dim), row)}
            one = sl.slice(list(fixed.items()))
            assert one.num_dimensions == 1 and one.partition == [[0]]
            x = one.slides[0].nodes[0]
            values = one.eval_batch(x.reshape(-1, 1), [0])
            want = ChebyshevApproximation.from_values(values, 1, [[a, b]], [x.size]).roots()
            _check_roots(sl.roots(dim, fixed), want, a, b, f"{case} dim {dim} row {r}")


# ------------------------------------------------------------------ slice, extrude, integrate
def _check_slider(got, g, tag, parent):
    sizes, dims = g[f"{tag}_part_sizes"], g[f"{tag}_part_dims"].tolist()
    partition, at = [], 0
    for s in sizes:
        partition.append(dims[at:at + s])
        at += s
    assert isinstance(got, ChebyshevSlider) and got._built and got.function is None
    assert got.__dict__["_device_slider"] is None and got._device_index == parent.__dict__.get("_device_index")
    assert [list(grp) for grp in got.partition] == partition, tag
    assert got.num_dimensions == g[f"{tag}_domain"].shape[0] == len(got.pivot_point), tag
    assert np.array_equal(np.asarray(got.domain, dtype=float), g[f"{tag}_domain"]), tag
    assert list(got.n_nodes) == g[f"{tag}_n_nodes"].tolist(), tag
    assert got._dim_to_slide == {d: i for i, grp in enumerate(partition) for d in grp}
    want_pv = float(g[f"{tag}_pivot_value"])
    scale = max(max(float(np.max(np.abs(g[f"{tag}_tensor{j}"]))) for j in range(len(partition))), abs(want_pv))
    assert abs(got.pivot_value - want_pv) <= 1e-12 * scale, (tag, got.pivot_value, want_pv)
    for j, slide in enumerate(got.slides):
        want = g[f"{tag}_tensor{j}"]
        assert slide.tensor_values.shape == want.shape, (tag, j)
        assert np.max(np.abs(slide.tensor_values - want)) <= 1e-12 * scale, (tag, j)
    assert_parity(got.eval_batch(g[f"{tag}_points"], [0] * got.num_dimensions), g[f"{tag}_values"], 1e-12, tag)
    p = g[f"{tag}_points"][0]
    assert abs(got.eval(list(p), [0] * got.num_dimensions) - g[f"{tag}_values"][0]) <= 1e-12 * np.max(np.abs(g[f"{tag}_values"]))


@pytest.mark.parametrize("case", sorted(G.SLICE_SETS))
def test_slice_matches_reference(g25, case):
    sl = _slider(case)
    for i, params in enumerate(G.SLICE_SETS[case]):
        _check_slider(sl.slice(params if len(params) > 1 else params[0]), g25, f"{case}_sl{i}", sl)


@pytest.mark.parametrize("case", sorted(G.EXTRUDE_SETS))
def test_extrude_matches_reference(g25, case):
    sl = _slider(case)
    for i, params in enumerate(G.EXTRUDE_SETS[case]):
        _check_slider(sl.extrude(params if len(params) > 1 else params[0]), g25, f"{case}_ex{i}", sl)


@pytest.mark.parametrize("case", sorted(G.INT_SETS))
def test_integrate_matches_reference(g25, case):
    sl = _slider(case)
    dom = np.asarray(sl.domain, dtype=float)
    full_scale = _tensor_scale(sl, float(np.prod(dom[:, 1] - dom[:, 0])))
    got = sl.integrate()
    assert isinstance(got, float)
    print(f"{case} integrate(): {got!r} reference {float(g25[f'{case}_int_full'])!r} scale {full_scale:.3e}")
    assert abs(got - float(g25[f"{case}_int_full"])) <= 1e-12 * full_scale
    sub = np.asarray(G.SUB_BOUNDS[case])
    sub_scale = _tensor_scale(sl, float(np.prod(sub[:, 1] - sub[:, 0])))
    assert abs(sl.integrate(None, list(G.SUB_BOUNDS[case])) - float(g25[f"{case}_int_sub"])) <= 1e-12 * sub_scale
    for i, (dims, bounds) in enumerate(G.INT_SETS[case]):
        _check_slider(sl.integrate(dims, bounds), g25, f"{case}_int{i}", sl)


# ------------------------------------------------------------------ integrate_batch
@pytest.mark.parametrize("case", sorted(G.BOX_SETS))
def test_integrate_batch_matches_reference(g25, case):
    sl = _slider(case)
    d = sl.num_dimensions
    for i, dims in enumerate(G.BOX_SETS[case]):
        bounds, pts = g25[f"{case}_box{i}_bounds"], g25[f"{case}_box{i}_points"]
        gb, gp = G.box_rows(case, i)
        assert np.array_equal(bounds, gb) and np.array_equal(pts, gp), "seeded golden rows no longer regenerate"
        points = pts if len(dims) < d else None
        got = sl.integrate_batch(dims, bounds, points)
        assert got.shape == (bounds.shape[0],)
        assert_parity(got, g25[f"{case}_box{i}_values"], 1e-12, f"{case} integrate_batch dims={dims}")
        # every row alone, and the batch repeated past one block of rows
        for r in (0, 3, 7):
            assert sl.integrate_batch(dims, bounds[r:r + 1], None if points is None else points[r:r + 1])[0] == got[r]
        idx = np.arange(300) % bounds.shape[0]
        assert np.array_equal(sl.integrate_batch(dims, bounds[idx], None if points is None else points[idx]), got[idx])
        # lo == hi in one integrated dimension: exactly 0
        flat = bounds.copy()
        flat[:, -1, 1] = flat[:, -1, 0]
        zero = sl.integrate_batch(dims, flat, points)
        assert np.all(zero == 0.0), (case, dims, zero)
        # one box for every row: integrate(dims, bounds) then eval_batch
        one_box = [tuple(v) for v in bounds[2]]
        want = sl.integrate(dims, one_box)
        got_one = sl.integrate_batch(dims, bounds[2], points)
        if points is None:
            vol = float(np.prod(bounds[2, :, 1] - bounds[2, :, 0]))
            assert got_one.shape == (1,) and abs(got_one[0] - want) <= 1e-12 * _tensor_scale(sl, vol)
        else:
            assert_parity(got_one, want.eval_batch(points, [0] * want.num_dimensions), 1e-12, f"{case} integrate_batch against integrate dims={dims}")
    dom = np.asarray(sl.domain, dtype=float)
    whole = sl.integrate_batch(None)
    assert whole.shape == (1,)
    assert abs(whole[0] - sl.integrate()) <= 1e-12 * _tensor_scale(sl, float(np.prod(dom[:, 1] - dom[:, 0])))


def test_box_device_pointer_entry_equals_host_pointer_entry(g25):
    from pychebyshev_amd.device import DeviceArray
    sl = _slider("b")
    s = sl._dev()
    lo, hi = sl._domain_arrays()
    for i, dims in enumerate(G.BOX_SETS["b"]):
        bounds, pts = g25[f"b_box{i}_bounds"], g25[f"b_box{i}_points"]
        points = pts if len(dims) < 5 else None
        flags, rows = _calculus.box_rows(5, sl.domain, dims, bounds, points)
        d_rows = DeviceArray.from_host(_lib.f64(rows), s.device)
        d_out = DeviceArray.empty((rows.shape[0],), s.device)
        _lib.check(s.lib.pcx_slider_box_batch_dev(s.handle, _lib.p_i32(_lib.i32(flags)), _lib.p_f64(lo), _lib.p_f64(hi),
                                                  ctypes.c_void_p(d_rows.ptr), rows.shape[0], ctypes.c_void_p(d_out.ptr)), s.lib)
        assert np.array_equal(d_out.to_host(), sl.integrate_batch(dims, bounds, points)), dims


def test_integrate_batch_past_one_pass_of_rows(g25):
    """kSliderBoxChunk + 5 rows (two passes through the host-pointer and the device-pointer entry): the golden rows
    repeated, every block equal to the first."""
    from pychebyshev_amd.device import DeviceArray
    sl = _slider("a")
    dims = G.BOX_SETS["a"][0]
    bounds, pts = g25["a_box0_bounds"], g25["a_box0_points"]
    base = sl.integrate_batch(dims, bounds, pts)
    S, N = bounds.shape[0], BOX_CHUNK_ROWS + 5
    idx = np.arange(N) % S
    got = sl.integrate_batch(dims, bounds[idx], pts[idx])
    assert np.array_equal(got, base[idx])
    s = sl._dev()
    lo, hi = sl._domain_arrays()
    flags, rows = _calculus.box_rows(3, sl.domain, dims, bounds[idx], pts[idx])
    d_rows = DeviceArray.from_host(_lib.f64(rows), s.device)
    d_out = DeviceArray.empty((N,), s.device)
    _lib.check(s.lib.pcx_slider_box_batch_dev(s.handle, _lib.p_i32(_lib.i32(flags)), _lib.p_f64(lo), _lib.p_f64(hi),
                                              ctypes.c_void_p(d_rows.ptr), N, ctypes.c_void_p(d_out.ptr)), s.lib)
    assert np.array_equal(d_out.to_host(), got)


# ------------------------------------------------------------------ errors, raised before any launch
def test_argument_errors():
    sl = _slider("b")
    rows = G.calculus_rows("b", 0)
    bad = rows.copy()
    bad[5, 1] = 1.5                                   # dimension 2 lives in [0.25, 1]
    with pytest.raises(ValueError, match=r"Fixed value 1\.5 for dim 2 outside domain \[0\.25, 1\.0\] \(row 5\)"):
        sl.roots_batch(0, bad)
    with pytest.raises(ValueError, match=r"dim 5 out of range \[0, 4\]"):
        sl.minimize_batch(5, rows)
    with pytest.raises(ValueError, match=r"fixed must have shape \(N, 4\)"):
        sl.maximize_batch(0, rows[:, :3])
    with pytest.raises(TypeError):
        sl.roots_batch(0.0, rows)
    with pytest.raises(ValueError, match="dim is required"):
        sl.roots()
    with pytest.raises(ValueError, match="fixed must specify all dims except 0"):
        sl.roots(0, {1: 100.0})
    with pytest.raises(ValueError, match="Fixed value 200.0 for dim 1 outside domain"):
        sl.minimize(0, {1: 200.0, 2: 0.5, 3: 0.2, 4: 0.03})
    with pytest.raises(ValueError, match="points is required"):
        sl.integrate_batch([0])
    with pytest.raises(ValueError, match="outside domain"):
        sl.integrate_batch([2], [(0.0, 0.5)], np.array([[100.0, 100.0, 0.2, 0.03]]))


def test_long_fibres_finish_on_the_host(g25):
    sl = _slider("l")
    with pytest.raises(ValueError, match="70 nodes"):
        sl.roots_batch(0, np.array([[G.L_FIXED]]))
    got = sl.roots(0, {1: G.L_FIXED})
    assert got.size == 5
    _check_roots(got, g25["l_d0_roots"][0, :5], -1.0, 1.0, "l roots")
    v, nodes, weights = _fibre(sl, 0, [G.L_FIXED])
    assert np.array_equal(got, _calculus.roots_1d(v, (-1.0, 1.0)))
    assert sl.maximize(0, {1: G.L_FIXED}) == _calculus.optimize_1d(v, nodes, weights, sl.slides[0].diff_matrices[0],
                                                                  (-1.0, 1.0), "max")


def test_c_entry_validates_before_any_launch():
    sl = _slider("b")
    s = sl._dev()
    lib = s.lib
    lo, hi = sl._domain_arrays()
    rows = _lib.f64(G.calculus_rows("b", 0))
    N = rows.shape[0]
    R = np.full((N, 8), 7.0)
    cnt = np.full(N, 7, dtype=np.int32)
    val, loc = np.full(N, 7.0), np.full(N, 7.0)

    def call(handle, dim, mode, n, rws=rows):
        return lib.pcx_slider_calculus_batch(handle, dim, _lib.p_f64(lo), _lib.p_f64(hi), _lib.p_f64(rws), n, mode,
                                             _lib.p_f64(R), _lib.p_i32(cnt), _lib.p_f64(val), _lib.p_f64(loc))
    assert call(None, 0, 0, N) == _lib.PCX_ERR_INVALID
    assert call(s.handle, 0, 3, N) == _lib.PCX_ERR_INVALID and "mode=3" in _lib.last_error(lib)
    assert call(s.handle, 5, 0, N) == _lib.PCX_ERR_INVALID
    assert call(s.handle, -1, 0, N) == _lib.PCX_ERR_INVALID
    bad = rows.copy()
    bad[3, 0] = 89.0                                  # dimension 1 lives in [90, 110]
    assert call(s.handle, 0, 0, N, bad) == _lib.PCX_ERR_INVALID
    assert "for dim 1" in _lib.last_error(lib) and "(row 3)" in _lib.last_error(lib)
    assert call(s.handle, 0, 0, 0) == _lib.PCX_OK
    assert np.all(R == 7.0) and np.all(cnt == 7) and np.all(val == 7.0) and np.all(loc == 7.0)   # no output touched
    long = _slider("l")
    sd = long._dev()
    llo, lhi = long._domain_arrays()
    one = _lib.f64([[G.L_FIXED]])
    assert lib.pcx_slider_calculus_batch(sd.handle, 0, _lib.p_f64(llo), _lib.p_f64(lhi), _lib.p_f64(one), 1, 0,
                                         _lib.p_f64(np.empty(69)), _lib.p_i32(cnt), None, None) == _lib.PCX_ERR_INVALID
    # box entries: NULL handle, a flag that is neither 0 nor 1, N = 0
    flags = _lib.i32([1, 0, 0, 0, 0])
    out = np.full(1, 7.0)
    row = _lib.f64([[80.0, 120.0, 100.0, 0.5, 0.2, 0.03]])
    assert lib.pcx_slider_box_batch(None, _lib.p_i32(flags), _lib.p_f64(lo), _lib.p_f64(hi), _lib.p_f64(row), 1,
                                    _lib.p_f64(out)) == _lib.PCX_ERR_INVALID
    assert lib.pcx_slider_box_batch(s.handle, _lib.p_i32(_lib.i32([2, 0, 0, 0, 0])), _lib.p_f64(lo), _lib.p_f64(hi),
                                    _lib.p_f64(row), 1, _lib.p_f64(out)) == _lib.PCX_ERR_INVALID
    assert lib.pcx_slider_box_batch(s.handle, _lib.p_i32(flags), _lib.p_f64(lo), _lib.p_f64(hi), None, 0, None) == _lib.PCX_OK
    assert out[0] == 7.0
