"""ChebyshevTT.integrate_batch (pcx_tt_box_batch, csrc/tt_box_kernels.h) against the reference's
``integrate(dims, bounds).eval(point)`` rows of g22_tt_transforms.npz, and sliced / extruded / integrated models
evaluated on the device.  Models A .. E run the lane-per-row form (rank caps 8, 12, 16; one and several node counts),
model F the wave-per-row form on the plain cores."""
import ctypes
import re

import numpy as np
import pytest

from conftest import assert_parity, golden
from pychebyshev_amd import ChebyshevTT, DeviceArray, _lib

pytestmark = pytest.mark.gpu

G = golden("g22_tt_transforms")
MODELS = ("A", "B", "C", "C2", "D", "E", "F")
_TT = {}


def cores_of(prefix):
    out, k = [], 0
    while f"{prefix}_core{k}" in G.files:
        out.append(G[f"{prefix}_core{k}"])
        k += 1
    return out


def model(tag):
    if tag not in _TT:
        _TT[tag] = ChebyshevTT.from_coeff_cores(cores_of(tag), G[f"{tag}_domain"].tolist(),
                                                dim_order=G[f"{tag}_order"].tolist())
    return _TT[tag]


def groups(tag):
    n = 0
    while f"{tag}_box{n}_dims" in G.files:
        n += 1
    return [f"{tag}_box{i}" for i in range(n)]


def group_args(g):
    points = G[f"{g}_points"]
    return G[f"{g}_dims"].tolist(), G[f"{g}_bounds"], (points if points.shape[1] else None)


ALL_GROUPS = [g for tag in MODELS for g in groups(tag)]


def test_every_model_has_its_groups():
    assert len(ALL_GROUPS) == 1 + 3 + 4 * 6 + 7
    for tag in MODELS:
        d = len(cores_of(tag))
        sets = [G[f"{g}_dims"].tolist() for g in groups(tag)]
        assert [0] in sets and [d - 1] in sets and list(range(d)) in sets


@pytest.mark.parametrize("g", ALL_GROUPS)
def test_integrate_batch_matches_the_reference(g):
    tt = model(g.split("_")[0])
    dims, bounds, points = group_args(g)
    ref = G[f"{g}_ref"]
    got = tt.integrate_batch(dims, bounds, points)
    assert got.shape == ref.shape and got.dtype == np.float64
    share = float(np.mean(np.abs(ref) >= 1e-3 * np.max(np.abs(ref))))
    assert share >= 0.90, f"{g}: only {share:.2f} of the rows carry the pointwise bound"
    assert_parity(got, ref, what=f"integrate_batch {g}")
    assert got[1] == 0.0                                    # row 1: lo == hi in its first integrated dimension
    assert np.array_equal(bounds[1, 0, 0], bounds[1, 0, 1])


@pytest.mark.parametrize("tag", MODELS)
def test_full_domain_over_all_dimensions_is_the_scalar_integral(tag):
    tt = model(tag)
    d = tt.num_dimensions
    want = float(G[f"{tag}_int_full"])
    got = tt.integrate_batch(list(range(d)))                # bounds None: the whole domain, one row
    assert got.shape == (1,)
    assert abs(got[0] - want) <= 1e-12 * abs(want)
    sub = tt.integrate_batch(list(range(d)), G[f"{tag}_int_sub_bounds"])
    assert abs(sub[0] - float(G[f"{tag}_int_sub"])) <= 1e-12 * abs(float(G[f"{tag}_int_sub"]))


@pytest.mark.parametrize("tag", ["C2", "D", "E", "F"])
def test_batch_sizes_and_rows_one_at_a_time(tag):
    """N around the 64-row workgroup (repeated golden rows), and a batch equal to its rows sent alone, bit for bit."""
    tt = model(tag)
    g = groups(tag)[3]                                      # a group of two integrated dimensions
    dims, bounds, points = group_args(g)
    ref = G[f"{g}_ref"]
    base = bounds.shape[0]
    whole = None
    for n in (1, 63, 64, 65, 200):
        idx = np.arange(n) % base
        got = tt.integrate_batch(dims, bounds[idx], points[idx])
        assert got.shape == (n,)
        assert_parity(got, ref[idx], what=f"integrate_batch {g} N={n}")
        whole = got
    for r in (0, 1, 5, 47):
        one = tt.integrate_batch(dims, bounds[r:r + 1], points[r:r + 1])
        assert one[0] == whole[r] == whole[r + base]


def _box_call(tt, flags, rows, out):
    t = tt._dev()
    return t.lib.pcx_tt_box_batch(t.handle, _lib.p_i32(flags), _lib.p_f64(rows), rows.shape[0], _lib.p_f64(out))


@pytest.mark.parametrize("tag", ["C", "F"])
def test_no_integrated_dimension_is_the_value(tag):
    tt = model(tag)
    d = tt.num_dimensions
    rng = np.random.default_rng(11)
    udom = tt._user_frame_domain()
    pts = np.ascontiguousarray(np.column_stack([rng.uniform(a, b, 333) for a, b in udom]))
    out = np.full(333, np.nan)
    assert _box_call(tt, np.zeros(d, dtype=np.int32), pts, out) == 0
    ref = tt.eval_batch(pts)
    assert np.max(np.abs(out - ref)) <= 1e-13 * np.max(np.abs(ref))


@pytest.mark.parametrize("tag", ["D", "F"])
def test_device_rows_equal_host_rows(tag):
    tt = model(tag)
    g = groups(tag)[3]
    dims, bounds, points = group_args(g)
    idx = np.arange(150) % bounds.shape[0]
    flags, rows = tt._box_rows(dims, bounds[idx], points[idx])
    host = tt.integrate_batch(dims, bounds[idx], points[idx])
    t = tt._dev()
    d_rows = DeviceArray.from_host(rows)
    d_out = DeviceArray.empty((rows.shape[0],), t.device)
    st = ctypes.c_void_p()
    _lib.check(t.lib.pcx_tt_stream(t.handle, ctypes.byref(st)), t.lib)
    _lib.check(t.lib.pcx_tt_box_batch_dev(t.handle, _lib.p_i32(flags), ctypes.c_void_p(d_rows.ptr), rows.shape[0],
                                          ctypes.c_void_p(d_out.ptr), st), t.lib)
    _lib.check(t.lib.pcx_stream_synchronize(st), t.lib)
    assert np.array_equal(d_out.to_host(), host)


def _result_cases():
    found = []
    for name in G.files:
        hit = re.fullmatch(r"([A-Z]\d?)_(slice|extrude|integ)(\d+)_params", name)
        if hit:
            found.append(f"{hit.group(1)}_{hit.group(2)}{hit.group(3)}")
    return sorted(found)


def _apply(tt, prefix):
    op = re.fullmatch(r"[A-Z]\d?_([a-z]+)\d+", prefix).group(1)
    params, single = G[f"{prefix}_params"], bool(int(G[f"{prefix}_single"]))
    if op == "slice":
        args = [(int(p[0]), float(p[1])) for p in params]
        return tt.slice(args[0] if single else args)
    if op == "extrude":
        args = [(int(p[0]), (float(p[1]), float(p[2])), int(p[3])) for p in params]
        return tt.extrude(args[0] if single else args)
    dims = [int(p[0]) for p in params]
    bounds = None if all(np.isnan(p[1]) for p in params) else \
        [None if np.isnan(p[1]) else (float(p[1]), float(p[2])) for p in params]
    return tt.integrate(dims[0] if single else dims, bounds=bounds)


@pytest.mark.parametrize("prefix", _result_cases())
def test_transformed_models_evaluate_on_the_device(prefix):
    res = _apply(model(prefix.split("_")[0]), prefix)
    got = res.eval_batch(G[f"{prefix}_pts"])
    assert_parity(got, G[f"{prefix}_vals"], what=f"eval of {prefix}")


def test_c_abi_argument_errors():
    tt = model("C")
    t = tt._dev()
    lib = t.lib
    flags = np.array([0, 1, 0, 0, 1], dtype=np.int32)
    rows = np.zeros((4, 7))
    out = np.full(4, 7.0)
    none_f64 = ctypes.POINTER(ctypes.c_double)()
    invalid = _lib.PCX_ERR_INVALID
    assert lib.pcx_tt_box_batch(None, _lib.p_i32(flags), _lib.p_f64(rows), 4, _lib.p_f64(out)) == invalid
    assert lib.pcx_tt_box_batch(t.handle, _lib.p_i32(flags), none_f64, 4, _lib.p_f64(out)) == invalid
    assert lib.pcx_tt_box_batch(t.handle, _lib.p_i32(flags), _lib.p_f64(rows), 4, none_f64) == invalid
    assert lib.pcx_tt_box_batch(t.handle, ctypes.POINTER(ctypes.c_int32)(), _lib.p_f64(rows), 4, _lib.p_f64(out)) == invalid
    assert lib.pcx_tt_box_batch(t.handle, _lib.p_i32(flags), _lib.p_f64(rows), -1, _lib.p_f64(out)) == invalid
    two = flags.copy()
    two[2] = 2
    assert lib.pcx_tt_box_batch(t.handle, _lib.p_i32(two), _lib.p_f64(rows), 4, _lib.p_f64(out)) == invalid
    assert lib.pcx_tt_box_batch_dev(None, _lib.p_i32(flags), None, 4, None, None) == invalid
    assert lib.pcx_tt_box_batch_dev(t.handle, _lib.p_i32(flags), None, 4, None, None) == invalid
    assert lib.pcx_tt_box_batch_dev(t.handle, _lib.p_i32(two), None, 0, None, None) == invalid
    assert np.all(out == 7.0)                               # nothing was launched
    assert lib.pcx_tt_box_batch(t.handle, _lib.p_i32(flags), _lib.p_f64(rows), 0, _lib.p_f64(out)) == 0
    assert tt.integrate_batch([1, 4], np.zeros((0, 2, 2)), np.zeros((0, 3))).shape == (0,)
