"""Ladders of ``ChebyshevSpline`` and ``ChebyshevSlider`` on the device (pcx_spline_ladder_batch, pcx_slider_ladder_batch:
csrc/pcx_piecewise_ladder.hip around the pieces' / slides' own fibre contraction).

1. golden parity: tests/golden/g35_piecewise_ladders*.npz hold the reference's ``ChebyshevSpline.eval_batch`` /
   ``ChebyshevSlider.eval`` at every ``(fixed..., x)`` point; bounds 1e-12 normwise and spec_point_tol(spec) pointwise on
   the cells the generator's masks keep.  Batch sizes 1, 15, 16, 17, 100 and ladder lengths 1, 16, 17, 33 are leading
   slices of the stored batch and equal it bit for bit; shared and per-row values.
2. composition, bit for bit: a spline cell is the owning piece's own ``ladder_batch`` of that row and value; a slider
   ladder is ``pivot + sum (v_s - pivot)`` formed in NumPy from the slides' own ``ladder_batch`` / ``vectorized_eval_batch``;
   the derivative cases of the slider.
3. ``fibre_batch`` is the ladder at the nodes, bit for bit, and within 1e-12 of ``eval_batch`` on the fibre points.
4. the existing route: ``eval_batch`` on the expanded points, within 1e-12 normwise, every case and dimension.
5. routing edges of the spline;  6. NaN;  7. batch independence;  8. device arrays;  9. the staging pass edge and the
   fibre-buffer chunk edge;  10. argument errors of the C ABI."""
import functools

import numpy as np
import pytest

from conftest import assert_parity, golden, parity, spec_point_tol
import generate_golden_ladders as LG
import generate_golden_piecewise_ladders as G
import generate_golden_slider_calculus as SL
import generate_golden_spline_transforms as SP
import piecewise_ladder_rule as rule

from pychebyshev_amd import ChebyshevApproximation, ChebyshevSlider, ChebyshevSpline, _lib
from pychebyshev_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

KEYS = [("s" + c, dim) for c in G.SPLINE_CASES for dim in range(SP.CASES[c]["d"])]
KEYS += [("l" + c, dim) for c in G.SLIDER_CASES for dim in range(SL.CASES[c]["d"])]
IDS = [f"{t}_dim{k}" for t, k in KEYS]
SPLINE_KEYS = [k for k in KEYS if k[0][0] == "s"]
SLIDER_KEYS = [k for k in KEYS if k[0][0] == "l"]
NS = [1, 15, 16, 17, 100]
MS = [1, 16, 17, 33]


@pytest.fixture(scope="module")
def models():
    out = {"s" + c: SP.build(ChebyshevSpline, c) for c in G.SPLINE_CASES}
    out.update({"l" + c: SL.build(ChebyshevSlider, c) for c in G.SLIDER_CASES})
    return out


@functools.lru_cache(maxsize=None)
def _gold(tag):
    return golden(G.file_of(tag))


def _specs(tag):
    return (G.SPLINE_SPECS if tag[0] == "s" else G.SLIDER_SPECS)[tag[1]]


def _batch(tag, dim):
    g = _gold(tag)
    pre = f"{tag}_k{dim}"
    return g, pre, g[f"{pre}_fixed"], g[f"{pre}_xs"], g[f"{pre}_xsrow"]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ------------------------------------------------------------------ 1. golden parity
@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_golden_parity(models, key):
    tag, dim = key
    obj = models[tag]
    g, pre, fixed, xs, xsrow = _batch(tag, dim)
    for j, spec in enumerate(_specs(tag)):
        ok, rowok = g[f"{pre}_s{j}_refok"], g[f"{pre}_s{j}_refrowok"]
        full = obj.ladder_batch(dim, fixed, xs, spec)
        assert full.shape == (fixed.shape[0], xs.size)
        assert_parity(full[:, ok], g[f"{pre}_s{j}_ref"][:, ok], tol=1e-12, what=f"{key} {spec} shared", point_tol=spec_point_tol(spec))
        row = obj.ladder_batch(dim, fixed[:xsrow.shape[0]], xsrow, spec)
        assert_parity(row[rowok], g[f"{pre}_s{j}_refrow"][rowok], tol=1e-12, what=f"{key} {spec} per row", point_tol=spec_point_tol(spec))
        for n in NS:
            assert _same_bits(obj.ladder_batch(dim, fixed[:n], xs, spec), full[:n]), f"{key} {spec} N={n}"
            if n <= xsrow.shape[0]:
                assert _same_bits(obj.ladder_batch(dim, fixed[:n], xsrow[:n], spec), row[:n]), f"{key} {spec} N={n} per row"
        for m in [v for v in MS if v <= xs.size]:
            assert _same_bits(obj.ladder_batch(dim, fixed, xs[:m], spec), full[:, :m]), f"{key} {spec} m={m}"
            assert _same_bits(obj.ladder_batch(dim, fixed[:xsrow.shape[0]], np.ascontiguousarray(xsrow[:, :m]), spec), row[:, :m])


def test_the_cross_slide_spec_is_plus_zero(models):
    sl = models["lc"]
    for dim in range(4):
        _, _, fixed, xs, xsrow = _batch("lc", dim)
        for got in (sl.ladder_batch(dim, fixed, xs, G.SLIDER_ZERO["c"]), sl.ladder_batch(dim, fixed[:17], xsrow, G.SLIDER_ZERO["c"])):
            assert np.all(got == 0.0) and not np.any(np.signbit(got))


# ------------------------------------------------------------------ 2. composition
def _spline_by_pieces(sp, dim, fixed, xs, spec):
    """every cell from the owning piece's own ladder_batch"""
    d = sp.num_dimensions
    others = [k for k in range(d) if k != dim]
    out = np.full((fixed.shape[0], xs.shape[-1]), np.nan)
    sec = [rule.route(sp.knots[k], sp._shape[k], fixed[:, c]) for c, k in enumerate(others)]
    for r in range(fixed.shape[0]):
        xr = xs if xs.ndim == 1 else xs[r]
        along = rule.route(sp.knots[dim], sp._shape[dim], xr)
        for j in np.unique(along):
            multi = [0] * d
            for c, k in enumerate(others):
                multi[k] = int(sec[c][r])
            multi[dim] = int(j)
            piece = sp._pieces[int(np.ravel_multi_index(multi, sp._shape))]
            pos = np.flatnonzero(along == j)
            out[r, pos] = piece.ladder_batch(dim, fixed[r:r + 1], xr[pos], spec)[0]
    return out


@pytest.mark.parametrize("key", SPLINE_KEYS, ids=[f"{t}_dim{k}" for t, k in SPLINE_KEYS])
def test_a_spline_cell_is_its_piece_s_own_ladder(models, key):
    tag, dim = key
    sp = models[tag]
    _, _, fixed, xs, xsrow = _batch(tag, dim)
    fixed = fixed[:24]
    for spec in _specs(tag)[:2]:
        assert _same_bits(sp.ladder_batch(dim, fixed, xs, spec), _spline_by_pieces(sp, dim, fixed, xs, spec)), f"{key} {spec}"
    assert _same_bits(sp.ladder_batch(dim, fixed[:17], xsrow), _spline_by_pieces(sp, dim, fixed[:17], xsrow, [0] * sp.num_dimensions))


def _slider_by_slides(sl, dim, fixed, xs, spec):
    """eval's rule from the slides' own ladder_batch / vectorized_eval_batch, in NumPy, slides in order"""
    d = sl.num_dimensions
    rows, m = fixed.shape[0], xs.shape[-1]
    col = {k: (k if k < dim else k - 1) for k in range(d) if k != dim}
    o = sl._dim_to_slide[dim]
    active = sorted({sl._dim_to_slide[k] for k in range(d) if spec[k] > 0})
    if len(active) > 1:
        return np.zeros((rows, m))

    def slide(s):
        g = list(sl.partition[s])
        sub = [spec[k] for k in g]
        if s == o:
            f = np.column_stack([fixed[:, col[k]] for k in g if k != dim]) if len(g) > 1 else np.empty((rows, 0))
            return sl.slides[s].ladder_batch(g.index(dim), f, xs, sub)
        pts = np.column_stack([fixed[:, col[k]] for k in g])
        return np.broadcast_to(sl.slides[s].vectorized_eval_batch(pts, sub)[:, None], (rows, m))

    if active:
        return np.array(slide(active[0]))
    res = np.full((rows, m), float(sl.pivot_value))
    for s in range(len(sl.partition)):
        res = res + (slide(s) - float(sl.pivot_value))
    return res


@pytest.mark.parametrize("key", SLIDER_KEYS, ids=[f"{t}_dim{k}" for t, k in SLIDER_KEYS])
def test_a_slider_ladder_is_the_host_composition_of_its_slides(models, key):
    tag, dim = key
    sl = models[tag]
    _, _, fixed, xs, xsrow = _batch(tag, dim)
    specs = _specs(tag) + ([G.SLIDER_ZERO[tag[1]]] if tag[1] in G.SLIDER_ZERO else [])
    for spec in specs:
        got = sl.ladder_batch(dim, fixed, xs, spec)
        assert _same_bits(got, _slider_by_slides(sl, dim, fixed, xs, spec)), f"{key} {spec} shared"
        got = sl.ladder_batch(dim, fixed[:17], xsrow, spec)
        assert _same_bits(got, _slider_by_slides(sl, dim, fixed[:17], xsrow, spec)), f"{key} {spec} per row"


# ------------------------------------------------------------------ 3. fibre_batch, 4. the existing route
def _fibre_nodes(obj, tag, dim):
    if tag[0] == "l":
        s = obj._dim_to_slide[dim]
        return np.asarray(obj.slides[s].nodes[list(obj.partition[s]).index(dim)], dtype=float)
    stride = int(np.prod(obj._shape[dim + 1:], dtype=int))
    return np.concatenate([np.asarray(obj._pieces[j * stride].nodes[dim], dtype=float) for j in range(obj._shape[dim])])


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_fibre_batch_and_the_pointwise_route(models, key):
    tag, dim = key
    obj = models[tag]
    d = obj.num_dimensions
    _, _, fixed, xs, _ = _batch(tag, dim)
    nodes = _fibre_nodes(obj, tag, dim)
    for spec in _specs(tag)[:2]:
        fib = obj.fibre_batch(dim, fixed, spec)
        assert fib.shape == (fixed.shape[0], nodes.size)
        assert _same_bits(fib, obj.ladder_batch(dim, fixed, nodes, spec)), f"{key} {spec}"
        want = obj.eval_batch(LG.expand(d, dim, fixed, nodes), spec).reshape(fib.shape)
        assert_parity(fib, want, tol=1e-12, what=f"fibre vs eval_batch {key} {spec}")
    inside = (xs >= obj.domain[dim][0]) & (xs <= obj.domain[dim][1])      # the extrapolated sums are conditioned like T_n(1.2)
    got = obj.ladder_batch(dim, fixed, xs)[:, inside]
    want = obj.eval_batch(LG.expand(d, dim, fixed, xs), [0] * d).reshape(fixed.shape[0], xs.size)[:, inside]
    e_norm, e_point = parity(got, want)
    print(f"{key}: ladder vs eval_batch E_norm {e_norm:.2e} E_point {e_point:.2e}")
    assert e_norm <= 1e-12


# ------------------------------------------------------------------ 5. routing edges of the spline
def test_spline_routing_edges(models):
    sp = models["sm"]                        # knots [95, 100, 105], [], [0.2] on [80, 120] x [0.01, 0.25] x [0.1, 0.4]
    # every row in the upper cross-section (x2 >= 0.2, the knot included): the lower one stays empty; no value in [95, 100)
    fixed = np.array([[0.13, 0.2], [0.01, 0.33], [0.25, 0.4], [0.2, 0.2], [0.07, 0.21]])
    xs = np.array([100.0, 83.7, 120.0, 105.0, 94.999, 76.0, 124.0, 95.0 - 1e-13])          # 76 and 124: 10 % outside
    got = sp.ladder_batch(0, fixed, xs)
    assert np.all(np.isfinite(got))
    pieces = np.asarray(sp._pieces, dtype=object).reshape(sp._shape)
    for x, j in ((100.0, 2), (105.0, 3), (94.999, 0), (76.0, 0), (124.0, 3), (120.0, 3)):     # a knot: the right-hand piece
        col = int(np.flatnonzero(xs == x)[0])
        assert _same_bits(got[:, col:col + 1], pieces[j, 0, 1].ladder_batch(0, fixed, [x])), x
    more = sp.ladder_batch(0, fixed, np.append(xs, 97.0))           # now the interval [95, 100) is live as well
    assert _same_bits(more[:, :-1], got)
    assert _same_bits(more[:, -1:], pieces[1, 0, 1].ladder_batch(0, fixed, [97.0]))
    want = sp.eval_batch(LG.expand(3, 0, fixed, xs), [0, 0, 0]).reshape(got.shape)
    assert_parity(got[:, :5], want[:, :5], tol=1e-12, what="routing edges vs eval_batch")
    # fixed coordinates 10 % outside their domain go to the end piece: device rows are not checked
    dev = sp._dev().device
    out_rows = np.array([[0.25 + 0.024, 0.4 + 0.03], [0.01 - 0.024, 0.1 - 0.03]])
    res = sp.ladder_batch(0, DeviceArray.from_host(out_rows, dev), xs[:4]).to_host()
    for r, sec in ((0, 1), (1, 0)):
        for col, j in enumerate((2, 0, 3, 3)):
            own = pieces[j, 0, sec].ladder_batch(0, DeviceArray.from_host(out_rows[r:r + 1], dev), xs[col:col + 1]).to_host()
            assert _same_bits(res[r:r + 1, col:col + 1], own), (r, col)


def test_the_global_histogram_path_gives_the_same_bits(models, monkeypatch):
    """PCX_SPLINE_GLOBAL_HIST=1 (read when the handle is created) forces the routing of splines with more pieces than LDS
    holds: rows counted and scattered with global atomics"""
    monkeypatch.setenv("PCX_SPLINE_GLOBAL_HIST", "1")
    sp = SP.build(ChebyshevSpline, "m")
    for dim in range(3):
        _, _, fixed, xs, xsrow = _batch("sm", dim)
        assert _same_bits(sp.ladder_batch(dim, fixed, xs), models["sm"].ladder_batch(dim, fixed, xs)), dim
        assert _same_bits(sp.ladder_batch(dim, fixed[:17], xsrow), models["sm"].ladder_batch(dim, fixed[:17], xsrow)), dim


# ------------------------------------------------------------------ 6. NaN
@pytest.mark.parametrize("tag", ["sk", "sm", "so", "la", "lb"])
def test_nan(models, tag):
    obj = models[tag]
    d = obj.num_dimensions
    for dim in range(d):
        _, _, fixed, xs, xsrow = _batch(tag, dim)
        fixed = fixed[:20]
        clean = obj.ladder_batch(dim, fixed, xs)
        xs2 = xs.copy()
        xs2[5] = np.nan
        got = obj.ladder_batch(dim, fixed, xs2)
        assert np.isnan(got[:, 5]).all()
        got[:, 5] = clean[:, 5]
        assert _same_bits(got, clean), f"{tag} dim {dim}: a NaN in xs"
        cleanrow = obj.ladder_batch(dim, fixed[:17], xsrow)
        xr = xsrow.copy()
        xr[3, 7] = np.nan
        got = obj.ladder_batch(dim, fixed[:17], xr)
        assert np.isnan(got[3, 7])
        got[3, 7] = cleanrow[3, 7]
        assert _same_bits(got, cleanrow), f"{tag} dim {dim}: a NaN in a per-row xs"
        for c in range(d - 1):               # every fixed column, the knotted ones included
            f2 = fixed.copy()
            f2[4, c] = np.nan
            got = obj.ladder_batch(dim, f2, xs)
            assert np.isnan(got[4]).all(), f"{tag} dim {dim} column {c}"
            got[4] = clean[4]
            assert _same_bits(got, clean), f"{tag} dim {dim} column {c}"


def test_nan_in_the_slider_s_derivative_cases(models):
    sl = models["lb"]                        # [[0, 1], [2], [3, 4]]
    _, _, fixed, xs, _ = _batch("lb", 2)
    fixed = fixed[:20]
    spec = [1, 0, 0, 0, 0]                   # inside slide 0, the ladder runs along slide 1's dimension: xs is not read
    clean = sl.ladder_batch(2, fixed, xs, spec)
    xs2 = xs.copy()
    xs2[3] = np.nan
    assert _same_bits(sl.ladder_batch(2, fixed, xs2, spec), clean)
    assert _same_bits(clean, np.repeat(clean[:, :1], xs.size, axis=1))
    f2 = fixed.copy()
    f2[6, 3] = np.nan                        # dimension 4 (slide 2) is not part of the derivative's slide
    assert _same_bits(sl.ladder_batch(2, f2, xs, spec), clean)
    f2[6, 0] = np.nan                        # dimension 0 is
    got = sl.ladder_batch(2, f2, xs, spec)
    assert np.isnan(got[6]).all()
    _, _, fixed, xs, _ = _batch("lb", 0)
    fixed = fixed[:20]
    clean = sl.ladder_batch(0, fixed, xs, spec)         # inside the owner: the owner's derivative ladder alone
    f2 = fixed.copy()
    f2[6, 1] = np.nan                        # dimension 2: another slide
    assert _same_bits(sl.ladder_batch(0, f2, xs, spec), clean)
    f2[6, 0] = np.nan                        # dimension 1: the owner's
    got = sl.ladder_batch(0, f2, xs, spec)
    assert np.isnan(got[6]).all()
    got[6] = clean[6]
    assert _same_bits(got, clean)


# ------------------------------------------------------------------ 7. batch independence
@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_batch_independence(models, key):
    tag, dim = key
    obj = models[tag]
    _, _, fixed, xs, _ = _batch(tag, dim)
    spec = _specs(tag)[-1]
    full = obj.ladder_batch(dim, fixed, xs, spec)
    for r in (0, 15, 16, 57, 99):
        assert _same_bits(obj.ladder_batch(dim, fixed[r:r + 1], xs, spec), full[r:r + 1]), f"{key} row {r}"
    assert _same_bits(obj.ladder_batch(dim, fixed, np.tile(xs, (fixed.shape[0], 1)), spec), full), f"{key} tiled"
    for m in (1, 5, 16):
        assert _same_bits(obj.ladder_batch(dim, fixed, xs[:m], spec), full[:, :m]), f"{key} m={m}"


# ------------------------------------------------------------------ 8. device arrays
def _device_forms(obj, device, dim, fixed, xs, xsrow, **kw):
    host = obj.ladder_batch(dim, fixed, xs, **kw)
    hostrow = obj.ladder_batch(dim, fixed[:xsrow.shape[0]], xsrow, **kw)
    dfixed = DeviceArray.from_host(fixed, device)
    got = obj.ladder_batch(dim, dfixed, xs, **kw)
    assert isinstance(got, DeviceArray) and got.shape == host.shape
    assert np.array_equal(got.to_host(), host)
    got = obj.ladder_batch(dim, DeviceArray.from_host(fixed[:xsrow.shape[0]], device), DeviceArray.from_host(xsrow, device), **kw)
    assert isinstance(got, DeviceArray) and np.array_equal(got.to_host(), hostrow)
    dout = DeviceArray.empty(host.shape, device)
    assert obj.ladder_batch(dim, fixed, xs, out=dout, **kw) is dout
    assert np.array_equal(dout.to_host(), host)
    hout = np.full(host.shape, np.nan)
    assert obj.ladder_batch(dim, fixed, xs, out=hout, **kw) is hout
    assert np.array_equal(hout, host)
    hout = np.full(host.shape, np.nan)
    assert obj.ladder_batch(dim, dfixed, xs, out=hout, **kw) is hout
    assert np.array_equal(hout, host)
    fib = obj.fibre_batch(dim, dfixed, **kw)
    assert isinstance(fib, DeviceArray) and np.array_equal(fib.to_host(), obj.fibre_batch(dim, fixed, **kw))
    empty = obj.ladder_batch(dim, dfixed, np.empty(0), **kw)
    assert isinstance(empty, DeviceArray) and empty.shape == (fixed.shape[0], 0)
    assert obj.ladder_batch(dim, fixed, np.empty(0), **kw).shape == (fixed.shape[0], 0)


@pytest.mark.parametrize("key", [("sm", 0), ("sm", 1), ("so", 0), ("sk", 1), ("la", 1), ("lb", 1), ("lc", 2), ("ll", 0)],
                         ids=lambda k: f"{k[0]}_dim{k[1]}")
def test_device_arrays(models, key):
    tag, dim = key
    obj = models[tag]
    _, _, fixed, xs, xsrow = _batch(tag, dim)
    _device_forms(obj, obj._dev().device, dim, fixed, xs, xsrow, derivative_order=_specs(tag)[min(1, len(_specs(tag)) - 1)])
    _device_forms(obj, obj._dev().device, dim, fixed, xs, xsrow)


# ------------------------------------------------------------------ 9. the two edges
def _pass_rows(width, m):
    """include/pcx.h: max(1, 2^20 / max(staged doubles per row, m)) rows per pass"""
    return max(1, (1 << 20) // max(max(1, width), m))


@pytest.mark.parametrize("tag", ["so", "la"])
@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "per_row"])
def test_batch_across_the_pass_edge(models, tag, per_row):
    obj = models[tag]
    d, m = obj.num_dimensions, 4
    P = _pass_rows(d - 1 + (m if per_row else 0), m)
    N = P + 3
    rng = np.random.default_rng(35)
    fixed = rng.uniform(-0.9, 0.9, (N, d - 1))
    xs = rng.uniform(-1.0, 1.0, (N, m)) if per_row else np.array([-0.95, 0.4, 0.1, -0.3])
    got = obj.ladder_batch(0, fixed, xs)
    assert got.shape == (N, m)
    for r in (0, P - 1, P, N - 1):
        assert _same_bits(got[r:r + 1], obj.ladder_batch(0, fixed[r:r + 1], xs[r:r + 1] if per_row else xs)), f"row {r}"


def test_batch_across_the_fibre_chunk_edge(models):
    sp = models["sm"]
    xs = np.array([85.0, 110.0])                      # live: the first and the last interval of dimension 0, 9 nodes each
    chunk = (1 << 21) // 18
    N = chunk + 3
    rng = np.random.default_rng(36)
    fixed = np.column_stack([rng.uniform(0.01, 0.25, N), rng.uniform(0.1, 0.4, N)])
    got = sp.ladder_batch(0, fixed, xs)
    for r in (0, chunk - 1, chunk, N - 1):
        assert _same_bits(got[r:r + 1], sp.ladder_batch(0, fixed[r:r + 1], xs)), f"row {r}"


# ------------------------------------------------------------------ 10. C ABI
@pytest.mark.parametrize("tag", ["sm", "lc"])
def test_abi_argument_errors(models, tag):
    lib = _lib.load()
    INV = _lib.PCX_ERR_INVALID
    obj = models[tag]
    d = obj.num_dimensions
    h = obj._dev().handle
    host = lib.pcx_spline_ladder_batch if tag[0] == "s" else lib.pcx_slider_ladder_batch
    dev = lib.pcx_spline_ladder_batch_dev if tag[0] == "s" else lib.pcx_slider_ladder_batch_dev
    _, _, gfixed, gxs, _ = _batch(tag, 1)
    fixed, xs = _lib.f64(gfixed[:4]), _lib.f64(gxs[:3])
    out = np.full((4, 3), 7.0)
    spec = _lib.i32([0] * d)
    pf, px, po, ps = _lib.p_f64(fixed), _lib.p_f64(xs), _lib.p_f64(out), _lib.p_i32(spec)
    assert host(None, 1, ps, pf, 4, px, 3, 0, po) == INV
    assert host(h, d, ps, pf, 4, px, 3, 0, po) == INV
    assert host(h, -1, ps, pf, 4, px, 3, 0, po) == INV
    assert host(h, 1, ps, pf, -1, px, 3, 0, po) == INV
    assert host(h, 1, ps, pf, 4, px, -1, 0, po) == INV
    assert host(h, 1, ps, pf, 4, px, 3, 2, po) == INV
    assert host(h, 1, ps, pf, 4, px, 3, -1, po) == INV
    assert host(h, 1, ps, None, 4, px, 3, 0, po) == INV
    assert host(h, 1, ps, pf, 4, None, 3, 0, po) == INV
    assert host(h, 1, ps, pf, 4, px, 3, 0, None) == INV
    nine = [0] * d
    nine[1] = 9
    assert host(h, 1, _lib.p_i32(_lib.i32(nine)), pf, 4, px, 3, 0, po) == INV
    nine[1] = -1
    assert host(h, 1, _lib.p_i32(_lib.i32(nine)), pf, 4, px, 3, 0, po) == INV
    assert dev(None, 1, ps, None, 4, px, 3, 0, None, None) == INV
    assert dev(h, 1, ps, None, 4, px, 3, 0, None, None) == INV
    assert dev(h, d + 2, ps, None, 0, px, 3, 0, None, None) == INV
    assert (out == 7.0).all(), "a refused call wrote results"
    assert host(h, 1, ps, pf, 0, px, 3, 0, po) == 0
    assert host(h, 1, ps, pf, 4, px, 0, 0, po) == 0
    assert dev(h, 1, ps, None, 0, px, 3, 0, None, None) == 0
    assert (out == 7.0).all()
    assert host(h, 1, None, pf, 4, px, 3, 0, po) == 0, _lib.last_error(lib)          # NULL spec: the values
    assert np.array_equal(out, obj.ladder_batch(1, fixed, xs))


def test_pieces_that_disagree_along_dim_are_refused():
    sp = SP.build_mixed(ChebyshevSpline, ChebyshevApproximation)      # index 0 along dimension 0: 5 and 7 nodes
    lib = _lib.load()
    h = sp._dev().handle
    fixed, xs = _lib.f64([[0.25], [0.75]]), _lib.f64([0.1, -0.4])
    out = np.full((2, 2), 7.0)
    rc = lib.pcx_spline_ladder_batch(h, 0, None, _lib.p_f64(fixed), 2, _lib.p_f64(xs), 2, 0, _lib.p_f64(out))
    assert rc == _lib.PCX_ERR_INVALID and "nodes along dim 0" in _lib.last_error(lib)
    assert (out == 7.0).all()
    got = sp.ladder_batch(1, np.array([[0.3], [-0.2]]), [0.25, 0.5, 0.75])          # along dimension 1 the grids agree
    want = sp.eval_batch(LG.expand(2, 1, np.array([[0.3], [-0.2]]), np.array([0.25, 0.5, 0.75])), [0, 0]).reshape(2, 3)
    assert_parity(got, want, tol=1e-12, what="mixed pieces along dimension 1")
