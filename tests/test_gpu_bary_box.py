"""Batched box integrals of the full-tensor interpolant and the spline on the device (``pcx_bary_box_batch``,
``csrc/bary_box_kernels.h``) against the reference's ``integrate(dims, bounds)`` then ``eval(point)``, row by row
(tests/golden/g24_bary_box.npz; generate_golden_bary_box.py lists the models and the rows of every group).

The MFMA form has three launch geometries, chosen by the LDS one wave needs (pcx_bary_box.hip, box_mfma_nt): two column
tiles per wave in four-wave workgroups (R1, R2, R0), one column tile in four-wave workgroups (F, W) and one wave per
workgroup with one column tile (L = 11^5, K).  ``_geometry`` restates the rule from ``pcx_bary_box_info`` and the tests
assert which one a model reaches.  F and K have no golden rows: their MFMA form is held against the rows form.

Parity is 1e-12 normwise and pointwise on the rows with |ref| >= 1e-3 max|ref| (conftest.assert_parity); every group
prints its figures before it asserts.  Measured on an MI355X: at most 8.4e-16 normwise and 2.7e-15 pointwise
(DESIGN.md section 3.10).
"""
import ctypes

import numpy as np
import pytest

from conftest import assert_parity, golden
import generate_golden_bary_box as G

from pychebyshev_amd import ChebyshevApproximation, ChebyshevSpline, _lib
from pychebyshev_amd._calculus import box_rows
from pychebyshev_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

# box_info[1:4] (k-steps, R, wide) and the launch geometry (column tiles per wave, waves per workgroup)
ROW_CODE = {"R1": ((6, 1, 0), (2, 4)), "R2": ((4, 2, 0), (2, 4)), "R0": ((4, 0, 0), (2, 4)), "W": (None, (1, 4)),
            "L": ((30, 1, 0), (1, 1)),           # five whole groups of six k-steps
            "F": ((14, 1, 0), (1, 4)),           # two groups and a remainder of two
            "K": ((56, 1, 0), (1, 1))}           # nine groups and a remainder of two
FORM_ONLY = {"F": (5, 7, 3, 19), "K": (5, 5, 15, 15)}      # no golden rows
SHAPES = {**G.MODELS, **FORM_ONLY}
GOLD = golden("g24_bary_box")


def _info(c, name, k):
    m = c._model()
    a = _lib.i32(np.zeros(k))
    _lib.check(getattr(m.lib, name)(m.handle, _lib.p_i32(a)), m.lib)
    return [int(v) for v in a]


def _set_kernel(c, variant):
    m = c._model()
    _lib.check(m.lib.pcx_bary_set_kernel(m.handle, variant), m.lib)


def _geometry(c):
    """(column tiles per wave, waves per workgroup) of the MFMA form: box_mfma_nt's rule on the LDS of one wave, its
    weight table of sum n + 2 rows and its B operands of 64 doubles per k-step, both per column tile."""
    ks = _info(c, "pcx_bary_box_info", 4)[1]
    wave = lambda nt: ((sum(c.n_nodes) + 2) * 16 * nt + ks * nt * 64) * 8
    if 4 * wave(2) <= 80 * 1024:
        return 2, 4
    return (1, 4) if 4 * wave(1) <= 80 * 1024 else (1, 1)


def _build(tag, monkeypatch):
    """Model `tag` of the golden file; the row-code models on the row-code MFMA form (variant 2, the short-plan forms
    switched off at create) as tests/test_gpu_bary_seed.py creates them."""
    shape = SHAPES[tag]
    d = len(shape)
    dom = G.domain_of(d)
    nodes = ChebyshevApproximation.nodes(d, dom, list(shape))["nodes_per_dim"]
    if tag in ROW_CODE:
        monkeypatch.setenv("PCX_BARY_GRID", "0")
        monkeypatch.setenv("PCX_BARY_KFOLD", "0")
    c = ChebyshevApproximation.from_values(G.grid_values(nodes), d, dom, list(shape))
    if tag in ROW_CODE:
        _set_kernel(c, 2)              # creates the handle: the environment is read here
        assert _info(c, "pcx_bary_grid_info", 4)[0] == 0
        box = _info(c, "pcx_bary_box_info", 4)
        assert box[0] == 1, f"{tag}: box calls do not take the MFMA form: {box}"
        if ROW_CODE[tag][0] is not None:
            assert tuple(box[1:]) == ROW_CODE[tag][0], f"{tag}: {box}"
        else:
            assert box[3] == 1, f"{tag}: not a wide plan: {box}"
        assert _geometry(c) == ROW_CODE[tag][1], f"{tag}: {box} launches as {_geometry(c)}"
    return c


def _groups(tag):
    """dims, bounds, points, ref of every group: the golden rows, or for F and K rows made by the generator's rules
    with no reference (ref is None)."""
    if tag in FORM_ONLY:
        d = len(FORM_ONLY[tag])
        dom = G.domain_of(d)
        nodes = ChebyshevApproximation.nodes(d, dom, list(FORM_ONLY[tag]))["nodes_per_dim"]
        for i, dims in enumerate(G.model_groups(d)):
            b, p = G.model_group_rows(np.random.default_rng([sum(FORM_ONLY[tag]), i]), dom, nodes, dims)
            yield dims, b, (p if p.shape[1] else None), None
        return
    all_dims = G.SPLINES[tag][2] if tag in G.SPLINES else G.model_groups(len(G.MODELS[tag]))
    for i, dims in enumerate(all_dims):
        b, p, ref = G.split_group(GOLD[f"{tag}_box{i}"], len(dims))
        yield dims, b, (p if p.shape[1] else None), ref


def _check_group(y, ref, what):
    e = np.abs(y - ref)
    big = np.abs(ref) >= 1e-3 * np.max(np.abs(ref))
    print(f"{what}: E_norm={e.max() / np.max(np.abs(ref)):.2e} E_point={np.max(e[big] / np.abs(ref[big])):.2e} "
          f"share={big.mean():.3f}")
    assert big.mean() >= 0.90, f"{what}: only {big.mean():.2f} of the rows are significant"
    assert_parity(y, ref, 1e-12, what)
    assert y[1] == 0.0, f"{what}: the row with lo == hi gives {y[1]!r}"


@pytest.mark.parametrize("tag", list(G.MODELS))
def test_groups_match_the_reference(tag, monkeypatch):
    c = _build(tag, monkeypatch)
    if tag == "S":
        assert _info(c, "pcx_bary_kernel_info", 6)[0] in (4, 5), "12 x 12 no longer prefers a lane-per-point kernel"
        assert _info(c, "pcx_bary_box_info", 4)[0] == 0
    if tag == "G":
        assert _info(c, "pcx_bary_grid_info", 4)[0] in (1, 2), "G is no grid / k-fold plan any more"
        for n in range(8, G.MODELS["G"][0]):
            smaller = ChebyshevApproximation.from_values(np.ones((n,) * 3), 3, G.domain_of(3), [n] * 3)
            assert _info(smaller, "pcx_bary_grid_info", 4)[0] == 0, f"{n}^3 has a grid / k-fold plan: G is not the smallest"
        assert _info(c, "pcx_bary_box_info", 4)[0] == 0
    for dims, b, p, ref in _groups(tag):
        _check_group(c.integrate_batch(dims, b, p), ref, f"box {tag} dims={dims}")


@pytest.mark.parametrize("tag", list(G.MODELS))
def test_full_domain_and_sub_box_scalars(tag, monkeypatch):
    c = _build(tag, monkeypatch)
    d = c.num_dimensions
    want_full, want_sub = GOLD[f"{tag}_int"][0]
    full = c.integrate_batch(list(range(d)))
    assert full.shape == (1,)
    assert abs(full[0] - want_full) <= 1e-12 * abs(want_full)
    sub = c.integrate_batch(None, GOLD[f"{tag}_int"][1:])
    assert abs(sub[0] - want_sub) <= 1e-12 * abs(want_sub)


@pytest.mark.parametrize("tag", list(ROW_CODE))
def test_rows_form_and_mfma_form_agree(tag, monkeypatch):
    c = _build(tag, monkeypatch)
    for dims, b, p, ref in _groups(tag):
        _set_kernel(c, 2)
        assert _info(c, "pcx_bary_box_info", 4)[0] == 1
        y_mfma = c.integrate_batch(dims, b, p)
        _set_kernel(c, 1)
        assert _info(c, "pcx_bary_box_info", 4) == [0, 0, 0, 0]
        y_rows = c.integrate_batch(dims, b, p)
        if ref is not None:
            _check_group(y_rows, ref, f"box {tag} dims={dims} rows form")
        e = np.abs(y_rows - y_mfma)
        print(f"box {tag} dims={dims} rows form against MFMA form: E_norm={e.max() / np.max(np.abs(y_mfma)):.2e}")
        assert_parity(y_rows, y_mfma, 1e-12, f"box {tag} dims={dims} rows form against MFMA form")
        assert y_rows[1] == 0.0 and y_mfma[1] == 0.0


def test_every_launch_geometry_of_the_mfma_form_is_reached():
    assert {geo for _, geo in ROW_CODE.values()} == {(2, 4), (1, 4), (1, 1)}


@pytest.mark.parametrize("tag", ["R1", "R2", "W", "L", "F", "K", "S", "A"])
def test_batch_sizes_and_single_rows(tag, monkeypatch):
    """A result does not depend on the batch it is part of: one workgroup walks all row tiles of its rows."""
    c = _build(tag, monkeypatch)
    forms = (2, 1) if tag in ROW_CODE else (0,)
    for dims, b, p, ref in _groups(tag):
        for variant in forms:
            _set_kernel(c, variant)
            base = c.integrate_batch(dims, b, p)
            sizes = [1, 63, 64, 65, 200] + ([66_000] if tag == "R1" and variant == 2 and len(dims) == 2 else [])
            for n in sizes:
                idx = np.arange(n) % G.ROWS
                y = c.integrate_batch(dims, b[idx], None if p is None else p[idx])
                assert np.array_equal(y, base[idx]), f"{tag} dims={dims} variant {variant} N={n}"
            for r in (0, 1, 5, 47):
                y = c.integrate_batch(dims, b[r:r + 1], None if p is None else p[r:r + 1])
                assert y.shape == (1,) and y[0] == base[r], f"{tag} dims={dims} variant {variant} row {r} alone"


@pytest.mark.parametrize("tag", ["R1", "W", "L", "S"])
def test_device_pointer_entry_equals_host_pointer_entry(tag, monkeypatch):
    c = _build(tag, monkeypatch)
    m = c._model()
    dom = np.asarray(c.domain, dtype=float)
    lo, hi = _lib.f64(dom[:, 0]), _lib.f64(dom[:, 1])
    st = ctypes.c_void_p()
    _lib.check(m.lib.pcx_bary_stream(m.handle, ctypes.byref(st)), m.lib)
    for dims, b, p, ref in _groups(tag):
        flags, rows = box_rows(c.num_dimensions, c.domain, dims, b, p)
        host = c.integrate_batch(dims, b, p)
        d_rows = DeviceArray.from_host(_lib.f64(rows), m.device)
        d_out = DeviceArray.empty((rows.shape[0],), m.device)
        _lib.check(m.lib.pcx_bary_box_batch_dev(m.handle, _lib.p_i32(_lib.i32(flags)), _lib.p_f64(lo), _lib.p_f64(hi),
                                                ctypes.c_void_p(d_rows.ptr), rows.shape[0], ctypes.c_void_p(d_out.ptr), st),
                   m.lib)
        _lib.check(m.lib.pcx_stream_synchronize(st), m.lib)
        assert np.array_equal(d_out.to_host(), host), f"{tag} dims={dims}"
    # N = 0 returns at once; a bad flag is an error code with a message, not an exception
    assert m.lib.pcx_bary_box_batch(m.handle, _lib.p_i32(_lib.i32(flags)), _lib.p_f64(lo), _lib.p_f64(hi), None, 0, None) == 0
    bad = _lib.i32(np.full(c.num_dimensions, 2))
    out = np.empty(1)
    assert m.lib.pcx_bary_box_batch(m.handle, _lib.p_i32(bad), _lib.p_f64(lo), _lib.p_f64(hi), _lib.p_f64(_lib.f64(rows)), 1,
                                    _lib.p_f64(out)) != 0


@pytest.mark.parametrize("tag", ["R1", "S", "G"])
def test_box_calls_and_evaluations_do_not_disturb_each_other(tag, monkeypatch):
    c = _build(tag, monkeypatch)
    d = c.num_dimensions
    rng = np.random.default_rng(5)
    pts = np.column_stack([rng.uniform(lo, hi, 300) for lo, hi in c.domain])
    dims, b, p, ref = list(_groups(tag))[-1]
    e0 = c.vectorized_eval_batch(pts, [0] * d)
    y0 = c.integrate_batch(dims, b, p)
    e1 = c.vectorized_eval_batch(pts, [0] * d)
    y1 = c.integrate_batch(dims, b, p)
    assert np.array_equal(e0, e1) and np.array_equal(y0, y1)
    # m = 0 would be the value: a box in one dimension shrunk onto a kept point is not, but the kept weights are the
    # evaluation's -- integrating x_0 over the whole domain at the points' other coordinates is a plain contraction
    whole = c.integrate_batch([0], None, pts[:, 1:]) if d > 1 else None
    if whole is not None:
        red = c.integrate(dims=[0])
        assert_parity(whole, red.vectorized_eval_batch(pts[:, 1:], [0] * (d - 1)), 1e-12, f"{tag}: integrate then eval")


# ------------------------------------------------------------------------------------------------- splines
def _spline(tag):
    n, knots, _ = G.SPLINES[tag]
    d = len(n)
    dom = G.domain_of(d)
    info = ChebyshevSpline.nodes(d, dom, n, knots)
    return ChebyshevSpline.from_values([G.grid_values(q["nodes_per_dim"]) for q in info["pieces"]], d, dom, n, knots)


@pytest.mark.parametrize("tag", list(G.SPLINES))
def test_spline_integrate_batch_matches_the_reference(tag):
    s = _spline(tag)
    for dims, b, p, ref in _groups(tag):
        y = s.integrate_batch(dims, b, p)
        _check_group(y, ref, f"spline box {tag} dims={dims}")
        for r in (0, 3, 5, 47):
            one = s.integrate_batch(dims, b[r:r + 1], None if p is None else p[r:r + 1])
            assert one[0] == y[r], f"spline {tag} dims={dims} row {r} alone"


@pytest.mark.parametrize("tag", list(G.SPLINES))
def test_spline_integrate_scalars_and_partials(tag):
    s = _spline(tag)
    n, knots, _ = G.SPLINES[tag]
    d = len(n)
    full, sub = (float(v) for v in GOLD[f"{tag}_int"][0])
    sub_bounds = GOLD[f"{tag}_int"][1:]
    got = s.integrate()
    assert isinstance(got, float) and abs(got - full) <= 1e-12 * abs(full)
    got = s.integrate(bounds=[tuple(v) for v in sub_bounds.tolist()])
    assert abs(got - sub) <= 1e-12 * abs(sub)
    assert abs(s.integrate_batch(None)[0] - full) <= 1e-12 * abs(full)
    assert abs(s.integrate_batch(None, sub_bounds)[0] - sub) <= 1e-12 * abs(sub)
    for i, (dims, bnds) in enumerate(G.SPLINE_PARTIALS[tag]):
        res = s.integrate(dims=dims, bounds=bnds)
        kept = [k for k in range(d) if k not in dims]
        assert isinstance(res, ChebyshevSpline) and res.num_dimensions == len(kept)
        assert np.array_equal(np.asarray(res.domain, dtype=float), GOLD[f"{tag}_part{i}_domain"])
        assert [list(map(float, k)) for k in res.knots] == [GOLD[f"{tag}_part{i}_knots{k}"].tolist() for k in range(len(kept))]
        j = 0
        while f"{tag}_part{i}_piece{j}" in GOLD.files:
            want = GOLD[f"{tag}_part{i}_piece{j}"]
            err = np.max(np.abs(res._pieces[j].tensor_values - want)) / np.max(np.abs(want))
            print(f"spline {tag} partial {i} piece {j}: {err:.2e}")
            assert err <= 1e-13, f"spline {tag} partial {i} piece {j}: {err:.2e}"
            j += 1
        assert j == len(res._pieces)
        pts = GOLD[f"{tag}_part{i}_eval"]
        assert_parity(res.eval_batch(pts[:, :-1], [0] * len(kept)), pts[:, -1], 1e-12, f"spline {tag} partial {i} eval")
