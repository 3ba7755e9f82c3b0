"""Tensor-product grid evaluation of the classes built out of barycentric pieces: ``ChebyshevSpline.eval_grid``
(pcx_spline_eval_tensor_grid: one sub-grid per live piece into a packed staging buffer, then k_spline_grid_place) and
``ChebyshevSlider.eval_grid`` (pcx_slider_eval_tensor_grid: one small grid per slide, then k_slider_grid_sum).

1. golden parity: tests/golden/g32_piecewise_grid.npz holds the reference's ``ChebyshevSpline.eval_batch`` on the
   meshgrid and ``ChebyshevSlider.eval`` at every grid point; bounds 1e-12 normwise and spec_point_tol(spec) pointwise,
   with auto and with each mode-product form forced on every pass (PCX_GRID_VARIANT);
2. spline = its pieces, BIT FOR BIT: ``piece.eval_grid(sub_axes, spec)`` of every live piece, assembled on the host with
   ``np.ix_`` from a NumPy restatement of the routing;
3. slider = its slides, BIT FOR BIT: ``pivot + sum_s (G_s - pivot)`` in slide order from the slides' own ``eval_grid``,
   broadcast in NumPy; a derivative inside one slide is an exact broadcast, one across two slides is all ``+0.0``;
   2, 3 and 6 run with both forms of the assembly kernels (PCX_PIECEWISE_GRID_DECODE=1 forces the per-element decode),
   the walking form also with a single workgroup (PCX_PIECEWISE_GRID_BLOCKS=1), so that its lanes do walk these grids;
4. = the pointwise route: ``eval_batch`` on the meshgrid, both classes, every grid and spec, same bounds as 1;
5. routing edges of the spline: a coordinate on a knot gives the right-hand piece's value; an axis inside one piece
   leaves the others dead; a NaN coordinate makes exactly its hyperplane NaN and leaves every other element bit for bit
   what it is with a finite coordinate of the same (the last) piece in its place -- the same plan, so the same sums; with
   the entry REMOVED the pieces' passes may run in another order, and the rest agrees to the bounds of 1;
6. ``out=`` a DeviceArray equals the NumPy form bit for bit; a larger and then a smaller grid on the same handle are
   still right (scratch reuse); a wrong shape or device is refused with ``ChebyshevApproximation.eval_grid``'s messages;
7. argument errors of the four entry points of the C ABI."""
import ctypes

import numpy as np
import pytest

from conftest import assert_parity, golden, spec_point_tol
import generate_golden_piecewise_grid as G

from pychebyshev_amd import ChebyshevSlider, ChebyshevSpline, _lib
from pychebyshev_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

SPLINE_IDS = [G.grid_id(g) for g in G.SPLINE_GRIDS]
SLIDER_IDS = [G.grid_id(g) for g in G.SLIDER_GRIDS]
VARIANTS = pytest.mark.parametrize("variant", ["", "1", "2"], ids=["auto", "valu", "mfma"])
# the assembly kernels' two forms: the multi-index decoded once per lane and walked (up to six dimensions), or per element.
# 2048 workgroups cover these grids in one step, so the walk itself runs with ONE workgroup: 256 lanes, 256 elements apart
DECODES = pytest.mark.parametrize("decode", [("", ""), ("", "1"), ("1", "")], ids=["walk", "walk-one-workgroup", "divide"])


@pytest.fixture(scope="module")
def g32():
    return golden("g32_piecewise_grid")


@pytest.fixture(scope="module")
def splines():
    return {case: G.SP.build(ChebyshevSpline, case) for case in sorted({g["case"] for g in G.SPLINE_GRIDS})}


@pytest.fixture(scope="module")
def sliders():
    return {case: G.SL.build(ChebyshevSlider, case) for case in sorted({g["case"] for g in G.SLIDER_GRIDS})}


def _spline_grid(g32, splines, i):
    g = G.SPLINE_GRIDS[i]
    sp = splines[g["case"]]
    return sp, [g32[f"s{i}_ax{k}"] for k in range(sp.num_dimensions)], g["specs"]


def _slider_grid(g32, sliders, i):
    g = G.SLIDER_GRIDS[i]
    sl = sliders[g["case"]]
    return sl, [g32[f"l{i}_ax{k}"] for k in range(sl.num_dimensions)], g["specs"]


def _mesh(axes):
    return np.column_stack([m.ravel() for m in np.meshgrid(*axes, indexing="ij")])


def _from_pieces(sp, axes, spec):
    """The spline's grid from its pieces' own ``eval_grid``: NumPy routing, ``np.ix_`` placement."""
    d = sp.num_dimensions
    iv = [G.route(sp.knots[k], sp._shape[k], axes[k]) for k in range(d)]
    out = np.full(tuple(len(a) for a in axes), np.inf)
    live = 0
    for multi in np.ndindex(*sp._shape):
        pos = [np.flatnonzero(iv[k] == multi[k]) for k in range(d)]
        if any(p.size == 0 for p in pos):
            continue
        piece = sp._pieces[int(np.ravel_multi_index(multi, sp._shape))]
        out[np.ix_(*pos)] = piece.eval_grid([np.asarray(axes[k])[pos[k]] for k in range(d)], spec)
        live += 1
    return out, live


def _spread(sl, s, axes, sub):
    """Slide s's own grid, broadcast to the slider's grid."""
    d = sl.num_dimensions
    shape = tuple(len(a) for a in axes)
    group = list(sl.partition[s])
    g = sl.slides[s].eval_grid([axes[k] for k in group], sub)
    view = [1] * d
    for k in group:
        view[k] = shape[k]
    return np.broadcast_to(np.transpose(g, np.argsort(group)).reshape(view), shape)


def _from_slides(sl, axes, spec):
    active = sorted({s for s, group in enumerate(sl.partition) for k in group if spec[k] > 0})
    if len(active) == 1:
        return np.array(_spread(sl, active[0], axes, [spec[k] for k in sl.partition[active[0]]]))
    res = np.full(tuple(len(a) for a in axes), float(sl.pivot_value))
    for s, group in enumerate(sl.partition):
        res = res + (_spread(sl, s, axes, [0] * len(group)) - float(sl.pivot_value))
    return res


# ------------------------------------------------------------------ 1. golden parity
@VARIANTS
@pytest.mark.parametrize("i", range(len(G.SPLINE_GRIDS)), ids=SPLINE_IDS)
def test_spline_grid_matches_the_reference(g32, splines, monkeypatch, i, variant):
    monkeypatch.setenv("PCX_GRID_VARIANT", variant)
    sp, axes, specs = _spline_grid(g32, splines, i)
    for j, spec in enumerate(specs):
        ref = g32[f"s{i}_r{j}"]
        got = sp.eval_grid(axes, spec)
        assert got.shape == ref.shape == tuple(a.size for a in axes)
        assert_parity(got, ref, 1e-12, what=f"spline eval_grid {SPLINE_IDS[i]} {spec} variant '{variant}'", point_tol=spec_point_tol(spec))
    assert_parity(sp.eval_grid(axes), g32[f"s{i}_r0"], 1e-12, what=f"spline eval_grid {SPLINE_IDS[i]} without a spec")


@VARIANTS
@pytest.mark.parametrize("i", range(len(G.SLIDER_GRIDS)), ids=SLIDER_IDS)
def test_slider_grid_matches_the_reference(g32, sliders, monkeypatch, i, variant):
    monkeypatch.setenv("PCX_GRID_VARIANT", variant)
    sl, axes, specs = _slider_grid(g32, sliders, i)
    for j, spec in enumerate(specs):
        ref = g32[f"l{i}_r{j}"]
        got = sl.eval_grid(axes, spec)
        assert got.shape == ref.shape == tuple(a.size for a in axes)
        assert_parity(got, ref, 1e-12, what=f"slider eval_grid {SLIDER_IDS[i]} {spec} variant '{variant}'", point_tol=spec_point_tol(spec))
    assert_parity(sl.eval_grid(axes), g32[f"l{i}_r0"], 1e-12, what=f"slider eval_grid {SLIDER_IDS[i]} without a spec")


# ------------------------------------------------------------------ 2. / 3. the parts, bit for bit
@DECODES
@pytest.mark.parametrize("i", range(len(G.SPLINE_GRIDS)), ids=SPLINE_IDS)
def test_spline_grid_is_its_pieces_bit_for_bit(g32, splines, monkeypatch, i, decode):
    monkeypatch.setenv("PCX_PIECEWISE_GRID_DECODE", decode[0])
    monkeypatch.setenv("PCX_PIECEWISE_GRID_BLOCKS", decode[1])
    sp, axes, specs = _spline_grid(g32, splines, i)
    for spec in specs:
        want, live = _from_pieces(sp, axes, spec)
        assert np.all(np.isfinite(want)), "the pieces' blocks do not tile the grid"
        assert np.array_equal(sp.eval_grid(axes, spec), want), f"{SPLINE_IDS[i]} {spec}: {live} live pieces"
    if SPLINE_IDS[i] == "m_3x4x2":
        assert live == 6 and sp.num_pieces == 8


@DECODES
@pytest.mark.parametrize("i", range(len(G.SLIDER_GRIDS)), ids=SLIDER_IDS)
def test_slider_grid_is_its_slides_bit_for_bit(g32, sliders, monkeypatch, i, decode):
    monkeypatch.setenv("PCX_PIECEWISE_GRID_DECODE", decode[0])
    monkeypatch.setenv("PCX_PIECEWISE_GRID_BLOCKS", decode[1])
    sl, axes, specs = _slider_grid(g32, sliders, i)
    for spec in specs:
        assert np.array_equal(sl.eval_grid(axes, spec), _from_slides(sl, axes, spec)), f"{SLIDER_IDS[i]} {spec}"


def test_cross_slide_derivative_is_plus_zero(g32, sliders):
    i = SLIDER_IDS.index("c_5x3x17x2")
    sl, axes, _ = _slider_grid(g32, sliders, i)
    got = sl.eval_grid(axes, G.SLIDER_ZERO["c"])
    assert got.shape == tuple(a.size for a in axes)
    assert np.all(got == 0.0) and not np.any(np.signbit(got))
    dev = sl.eval_grid(axes, G.SLIDER_ZERO["c"], out=DeviceArray.from_host(np.full(got.shape, 7.0), sl._dev().device)).to_host()
    assert np.all(dev == 0.0) and not np.any(np.signbit(dev))


# ------------------------------------------------------------------ 4. the pointwise route
@pytest.mark.parametrize("i", range(len(G.SPLINE_GRIDS)), ids=SPLINE_IDS)
def test_spline_grid_matches_eval_batch(g32, splines, i):
    sp, axes, specs = _spline_grid(g32, splines, i)
    pts = _mesh(axes)
    for spec in specs:
        want = sp.eval_batch(pts, spec).reshape([a.size for a in axes])
        assert_parity(sp.eval_grid(axes, spec), want, 1e-12, what=f"spline eval_grid vs eval_batch {SPLINE_IDS[i]} {spec}",
                      point_tol=spec_point_tol(spec))


@pytest.mark.parametrize("i", range(len(G.SLIDER_GRIDS)), ids=SLIDER_IDS)
def test_slider_grid_matches_eval_batch(g32, sliders, i):
    sl, axes, specs = _slider_grid(g32, sliders, i)
    pts = _mesh(axes)
    for spec in specs:
        want = sl.eval_batch(pts, spec).reshape([a.size for a in axes])
        assert_parity(sl.eval_grid(axes, spec), want, 1e-12, what=f"slider eval_grid vs eval_batch {SLIDER_IDS[i]} {spec}",
                      point_tol=spec_point_tol(spec))
    if G.grid_id(G.SLIDER_GRIDS[i]) == "c_5x3x17x2":
        assert np.all(sl.eval_batch(pts, G.SLIDER_ZERO["c"]) == 0.0)


def test_derivative_id_and_scalar_axes(g32, splines, sliders):
    sp, axes, specs = _spline_grid(g32, splines, SPLINE_IDS.index("k_17x6"))
    assert np.array_equal(sp.eval_grid(axes, derivative_id=sp.get_derivative_id(specs[1])), sp.eval_grid(axes, specs[1]))
    got = sp.eval_grid([float(axes[0][0]), axes[1]])
    assert got.shape == (1, axes[1].size) and np.array_equal(got, sp.eval_grid([axes[0][:1], axes[1]]))
    sl, axes, specs = _slider_grid(g32, sliders, SLIDER_IDS.index("b_2x3x5x1x4"))
    assert np.array_equal(sl.eval_grid(axes, derivative_id=sl.get_derivative_id(specs[1])), sl.eval_grid(axes, specs[1]))


# ------------------------------------------------------------------ 5. routing edges
def test_a_coordinate_on_a_knot_takes_the_right_hand_piece(splines):
    sp = splines["k"]                                   # knots 0.2 and 0.5: the four pieces differ on them (|x - 0.2|, max(y - 0.5, 0)^2)
    right = sp._pieces[int(np.ravel_multi_index((1, 1), sp._shape))]
    left = sp._pieces[0]
    got = sp.eval_grid([[0.2], [0.5]], [1, 0])
    assert np.array_equal(got, right.eval_grid([[0.2], [0.5]], [1, 0]))
    assert got[0, 0] > 0.0 > left.eval_grid([[0.2], [0.5]], [1, 0])[0, 0], "d/dx |x - 0.2| is +e^y right of the knot, -e^y left of it"
    # just below the knots the left-hand pieces answer
    below = [[np.nextafter(0.2, -1.0)], [np.nextafter(0.5, -1.0)]]
    assert np.array_equal(sp.eval_grid(below, [1, 0]), left.eval_grid(below, [1, 0]))


def test_an_axis_inside_one_piece_leaves_the_others_dead(splines):
    sp = splines["m"]                                   # 4 x 1 x 2 pieces, knots 95, 100, 105 and 0.2
    rng = np.random.default_rng(5)
    axes = [rng.uniform(100.0, 104.9, 7), rng.uniform(0.01, 0.25, 3), np.array([0.35, 0.12, 0.2, 0.39])]
    want, live = _from_pieces(sp, axes, [0, 0, 0])
    assert live == 2
    assert np.array_equal(sp.eval_grid(axes), want)
    # every axis inside ONE piece: that piece writes the result itself
    axes[2] = np.array([0.35, 0.2, 0.39])
    want, live = _from_pieces(sp, axes, [1, 0, 0])
    assert live == 1
    assert np.array_equal(sp.eval_grid(axes, [1, 0, 0]), want)
    assert_parity(sp.eval_grid(axes, [1, 0, 0]), sp.eval_batch(_mesh(axes), [1, 0, 0]).reshape(7, 3, 3), 1e-12,
                  what="one live piece vs eval_batch", point_tol=spec_point_tol([1, 0, 0]))


@pytest.mark.parametrize("dim", [0, 1])
def test_a_nan_coordinate_spoils_exactly_its_hyperplane(g32, splines, dim):
    sp, axes, _ = _spline_grid(g32, splines, SPLINE_IDS.index("k_17x6"))
    at = 2
    bad = [a.copy() for a in axes]
    bad[dim][at] = np.nan
    got = sp.eval_grid(bad)
    expect = np.zeros(got.shape, dtype=bool)
    expect[(slice(None),) * dim + (at,)] = True
    assert np.array_equal(np.isnan(got), expect)
    # a NaN is routed to the last piece: with a finite coordinate of that piece in its place the plan is the same
    stand_in = [a.copy() for a in axes]
    stand_in[dim][at] = sp.domain[dim][1]
    assert np.array_equal(got[~expect], sp.eval_grid(stand_in)[~expect])
    removed = [np.delete(a, at) if k == dim else a for k, a in enumerate(axes)]
    assert_parity(np.delete(got, at, axis=dim), sp.eval_grid(removed), 1e-12, what=f"NaN in dimension {dim} vs the grid without it")


# ------------------------------------------------------------------ 6. device output
@DECODES
def test_device_output_and_scratch_reuse(g32, splines, sliders, monkeypatch, decode):
    monkeypatch.setenv("PCX_PIECEWISE_GRID_DECODE", decode[0])
    monkeypatch.setenv("PCX_PIECEWISE_GRID_BLOCKS", decode[1])
    for obj, axes, specs in (_spline_grid(g32, splines, SPLINE_IDS.index("m_9x1x18")), _slider_grid(g32, sliders, SLIDER_IDS.index("c_5x3x17x2"))):
        dev = obj._dev().device
        d = obj.num_dimensions
        spec = specs[1]
        small = [a[:max(1, a.size // 2)] for a in axes]
        large = [np.concatenate([a, a[::-1]]) for a in axes]
        for ax in (axes, large, small, axes):             # a larger and then a smaller grid on the same handle
            shape = tuple(a.size for a in ax)
            want = obj.eval_grid(ax, spec)
            out = DeviceArray.from_host(np.full(shape, np.nan), dev)
            res = obj.eval_grid(ax, spec, out=out)
            assert res is out and np.array_equal(out.to_host(), want)
            pts = _mesh(ax)
            assert_parity(want, obj.eval_batch(pts, spec).reshape(shape), 1e-12, what=f"{type(obj).__name__} grid {shape}",
                          point_tol=spec_point_tol(spec))
        with pytest.raises(ValueError, match="at dimension 0"):
            obj.eval_grid(axes, out=DeviceArray.empty((axes[0].size + 1,) + tuple(a.size for a in axes[1:]), dev))
        with pytest.raises(ValueError, match=f"has {d + 1} dimensions"):
            obj.eval_grid(axes, out=DeviceArray.empty(tuple(a.size for a in axes) + (1,), dev))
        with pytest.raises(ValueError):
            obj.eval_grid(axes, [9] + [0] * (d - 1))


def test_out_on_another_device_is_refused(g32, splines, sliders):
    if _lib.device_count() < 2:
        pytest.skip("needs two devices")
    for obj, axes, _ in (_spline_grid(g32, splines, 1), _slider_grid(g32, sliders, 0)):
        here = obj._dev().device
        other = DeviceArray.empty(tuple(a.size for a in axes), (here + 1) % _lib.device_count())
        with pytest.raises(ValueError, match=f"device {other.device}"):
            obj.eval_grid(axes, out=other)


# ------------------------------------------------------------------ 7. argument errors of the C ABI
def test_c_abi_argument_errors(g32, splines, sliders):
    lib = _lib.load()
    for kind, (obj, axes, _) in (("spline", _spline_grid(g32, splines, SPLINE_IDS.index("k_17x6"))),
                                 ("slider", _slider_grid(g32, sliders, SLIDER_IDS.index("a_3x17x2")))):
        host, devf = getattr(lib, f"pcx_{kind}_eval_tensor_grid"), getattr(lib, f"pcx_{kind}_eval_tensor_grid_dev")
        s = obj._dev()
        h = s.handle
        d = obj.num_dimensions
        m = _lib.i32([a.size for a in axes])
        cat = _lib.f64(np.concatenate(axes))
        out = np.empty(tuple(m))
        dout = DeviceArray.empty(tuple(m), s.device)
        pm, pc, po, pd = _lib.p_i32(m), _lib.p_f64(cat), _lib.p_f64(out), ctypes.c_void_p(dout.ptr)
        assert host(None, None, pm, pc, po) == _lib.PCX_ERR_INVALID and "handle" in _lib.last_error(lib)
        assert host(h, None, None, pc, po) == _lib.PCX_ERR_INVALID
        assert host(h, None, pm, None, po) == _lib.PCX_ERR_INVALID
        assert host(h, None, pm, pc, None) == _lib.PCX_ERR_INVALID
        assert devf(None, None, pm, pc, pd, None) == _lib.PCX_ERR_INVALID
        assert devf(h, None, None, pc, pd, None) == _lib.PCX_ERR_INVALID
        assert devf(h, None, pm, None, pd, None) == _lib.PCX_ERR_INVALID
        assert devf(h, None, pm, pc, None, None) == _lib.PCX_ERR_INVALID
        m0 = _lib.i32([m[0], 0] + list(m[2:]))
        for call in (lambda: host(h, None, _lib.p_i32(m0), pc, po), lambda: devf(h, None, _lib.p_i32(m0), pc, pd, None)):
            assert call() == _lib.PCX_ERR_INVALID
            assert "dimension 1" in _lib.last_error(lib) and "empty" in _lib.last_error(lib)
        huge = _lib.i32([1 << 21] * 2 + [1] * (d - 2))
        assert host(h, None, _lib.p_i32(huge), pc, po) == _lib.PCX_ERR_UNSUPPORTED
        assert devf(h, None, _lib.p_i32(huge), pc, pd, None) == _lib.PCX_ERR_UNSUPPORTED
        bad_spec = _lib.i32([9] + [0] * (d - 1))
        assert host(h, _lib.p_i32(bad_spec), pm, pc, po) == _lib.PCX_ERR_INVALID
        # nothing is left queued: deriv == NULL is the plain value, in both forms, straight afterwards
        assert host(h, None, pm, pc, po) == 0, _lib.last_error(lib)
        assert np.array_equal(out, obj.eval_grid(axes, [0] * d))
        assert devf(h, None, pm, pc, pd, None) == 0, _lib.last_error(lib)
        assert lib.pcx_device_synchronize(s.device) == 0
        assert np.array_equal(dout.to_host(), out)
