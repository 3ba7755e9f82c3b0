"""Ladders on the device: ``ladder_batch`` / ``fibre_batch`` of ``ChebyshevApproximation`` (pcx_bary_ladder_batch: the
rows form and the v_mfma_f64_16x16x4_f64 form) and ``ChebyshevTT`` (pcx_tt_ladder_batch: lane per row and wave per row).

1. golden parity: tests/golden/g34_ladders.npz holds the reference's pointwise ``vectorized_eval`` / ``eval`` at every
   ``(fixed..., x)`` point; bounds 1e-12 normwise and spec_point_tol(spec) pointwise (tests/conftest.py) on the values
   the generator found the reference itself good for (its masks: everything inside the domain, and what is outside
   where the dimension is short enough for an extrapolated FP64 sum to mean something).  Dense cases run
   on each form (auto, and rows through pcx_bary_set_kernel(h, 1)); pcx_bary_ladder_info must name the MFMA form, with
   the k-steps and column tiles of the case, wherever the case is meant for it.  Batch sizes 1, 15, 16, 17, 100 and
   ladder lengths 1, 16, 17, 33 are leading slices of the stored batch; shared and per-row values.
2. the fibre is the ladder at the nodes, bit for bit, and a value on a node returns the fibre's value bit for bit;
3. a row's bits depend neither on its batch, nor on shared / per-row values, nor on m;
4. NaN in one ``xs`` cell stays in that cell, NaN in ``fixed`` fills its row, every other bit is unchanged;
5. device arrays in, DeviceArray out, ``out=`` of both kinds: the host call's bits;
6. a batch across the host staging pass edge;
7. the existing route: ``vectorized_eval_batch`` / ``eval_batch`` on the expanded points (11^5 Black-Scholes tensor: the
   high part of the K axis has 121 entries there), within 1e-12 normwise;
8. argument errors of the C ABI."""
import ctypes

import numpy as np
import pytest

from conftest import assert_parity, golden, parity, spec_point_tol
import generate_golden_ladders as G

from pychebyshev_amd import ChebyshevApproximation, ChebyshevTT, _lib
from pychebyshev_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

DENSE_KEYS = [(i, dim) for i, c in enumerate(G.DENSE) for dim in c["dims"]]
DENSE_IDS = ["x".join(map(str, G.DENSE[i]["n"])) + f"_dim{dim}" for i, dim in DENSE_KEYS]
# (case, dim) -> (k-steps per block of 16 rows, column tiles) of the MFMA form; the 1-D case has no K axis: rows form
MFMA_GEOMETRY = {(1, 0): (2, 1), (1, 1): (2, 1), (2, 0): (17, 1), (2, 1): (6, 1), (2, 2): (11, 1), (3, 0): (2, 2),
                 (4, 0): (1, 3), (5, 0): (2, 4), (6, 1): (36, 1), (7, 0): (60, 1), (7, 1): (45, 1), (7, 2): (36, 1),
                 (7, 3): (60, 1), (7, 4): (45, 1)}
TT_TAGS = ["A", "C", "F", "G"]
NS = [1, 15, 16, 17, 100]
MS = [1, 16, 17, 33]


@pytest.fixture(scope="module")
def g34():
    return golden("g34_ladders")


@pytest.fixture(scope="module")
def dense_models(g34):
    out = {}
    for i in range(len(G.DENSE)):
        n = [int(v) for v in g34[f"d{i}_n"]]
        out[i] = ChebyshevApproximation.from_values(g34[f"d{i}_tensor"], len(n), g34[f"d{i}_domain"].tolist(), n)
    return out


@pytest.fixture(scope="module")
def tt_models(g34):
    g22 = golden("g22_tt_transforms")
    out = {}
    for tag in TT_TAGS:
        src, pre = (g34, "tG") if tag == "G" else (g22, tag)
        cores, k = [], 0
        while f"{pre}_core{k}" in src.files:
            cores.append(src[f"{pre}_core{k}"])
            k += 1
        out[tag] = ChebyshevTT.from_coeff_cores(cores, src[f"{pre}_domain"].tolist(), dim_order=[int(v) for v in g34[f"t{tag}_order"]])
    return out


def _set_rows(model, on):
    m = model._model()
    assert m.lib.pcx_bary_set_kernel(m.handle, 1 if on else 0) == 0, _lib.last_error(m.lib)


def _info(model, dim):
    m = model._model()
    info = np.zeros(3, dtype=np.int32)
    assert m.lib.pcx_bary_ladder_info(m.handle, dim, _lib.p_i32(info)) == 0, _lib.last_error(m.lib)
    return [int(v) for v in info]


WORST = {}


def _check(got, ref, spec, what):
    e_norm, e_point = parity(got, ref)
    key = what.split(" ")[0]
    w = WORST.setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], e_norm), max(w[1], e_point / spec_point_tol(spec))
    print(f"{what}: E_norm {e_norm:.2e} E_point {e_point:.2e} (worst so far for {key}: {w[0]:.2e}, {w[1]:.2f} of the pointwise bound)")
    assert_parity(got, ref, tol=1e-12, what=what, point_tol=spec_point_tol(spec))


# ------------------------------------------------------------------ 1. golden parity
@pytest.mark.parametrize("form", ["auto", "rows"])
@pytest.mark.parametrize("key", DENSE_KEYS, ids=DENSE_IDS)
def test_dense_ladder_matches_the_reference(g34, dense_models, key, form):
    i, dim = key
    model = dense_models[i]
    pre = f"d{i}_k{dim}"
    fixed, xs, xsrow = g34[f"{pre}_fixed"], g34[f"{pre}_xs"], g34[f"{pre}_xsrow"]
    _set_rows(model, form == "rows")
    try:
        info = _info(model, dim)
        if form == "auto" and key in MFMA_GEOMETRY:
            assert info == [1, *MFMA_GEOMETRY[key]], f"{DENSE_IDS[DENSE_KEYS.index(key)]}: the MFMA form did not take this case: {info}"
        else:
            assert info == [0, 0, 0]
        for j in range(int(g34[f"d{i}_nspec"])):
            spec = [int(v) for v in g34[f"d{i}_s{j}_spec"]]
            ref, refrow = g34[f"{pre}_s{j}_ref"], g34[f"{pre}_s{j}_refrow"]
            what = f"dense-{form} {DENSE_IDS[DENSE_KEYS.index(key)]} {spec}"
            full = model.ladder_batch(dim, fixed, xs, spec)
            fullrow = model.ladder_batch(dim, fixed[:xsrow.shape[0]], xsrow, spec)
            ok, rowok = g34[f"{pre}_s{j}_refok"], g34[f"{pre}_s{j}_refrowok"]      # where the reference is worth comparing with
            _check(full[:, ok], ref[:, ok], spec, what + " shared")
            _check(fullrow[rowok], refrow[rowok], spec, what + " per row")
            # the batch sizes and ladder lengths: the bits of the batch that was just held to the reference
            for N in NS:
                for m in [v for v in MS if v <= xs.size]:
                    got = model.ladder_batch(dim, fixed[:N], xs[:m], spec)
                    assert got.shape == (N, m)
                    assert np.array_equal(got, full[:N, :m]), f"{what} N={N} m={m}"
            for N in [v for v in NS if v <= xsrow.shape[0]]:
                for m in [v for v in MS if v <= xs.size]:
                    got = model.ladder_batch(dim, fixed[:N], np.ascontiguousarray(xsrow[:N, :m]), spec)
                    assert np.array_equal(got, fullrow[:N, :m]), f"{what} per row N={N} m={m}"
    finally:
        _set_rows(model, False)


@pytest.mark.parametrize("tag", TT_TAGS)
def test_tt_ladder_matches_the_reference(g34, tt_models, tag):
    tt = tt_models[tag]
    for dim in [int(v) for v in g34[f"t{tag}_dims"]]:
        pre = f"t{tag}_k{dim}"
        fixed, xs, xsrow = g34[f"{pre}_fixed"], g34[f"{pre}_xs"], g34[f"{pre}_xsrow"]
        what = f"tt-{'lpp' if tag in ('A', 'C') else 'generic'} {tag} dim {dim}"
        ok, rowok = g34[f"{pre}_refok"], g34[f"{pre}_refrowok"]
        _check(tt.ladder_batch(dim, fixed, xs)[:, ok], g34[f"{pre}_ref"][:, ok], [0], what + " shared")
        _check(tt.ladder_batch(dim, fixed[:xsrow.shape[0]], xsrow)[rowok], g34[f"{pre}_refrow"][rowok], [0], what + " per row")
        full = tt.ladder_batch(dim, fixed, xs)
        for N in NS:
            for m in [v for v in MS if v <= xs.size]:
                assert np.array_equal(tt.ladder_batch(dim, fixed[:N], xs[:m]), full[:N, :m]), f"{what} N={N} m={m}"


def test_tt_models_run_on_the_form_meant_for_them(tt_models):
    for tag in TT_TAGS:
        tt = tt_models[tag]
        small = max(tt.tt_ranks) <= 16 and max(tt.n_nodes) <= 16
        assert small == (tag in ("A", "C")), f"model {tag}: ranks {tt.tt_ranks}, nodes {tt.n_nodes}"


# ------------------------------------------------------------------ 2. fibre = ladder at the nodes
@pytest.mark.parametrize("form", ["auto", "rows"])
@pytest.mark.parametrize("key", DENSE_KEYS, ids=DENSE_IDS)
def test_dense_fibre_is_the_ladder_at_the_nodes(g34, dense_models, key, form):
    i, dim = key
    model = dense_models[i]
    fixed = g34[f"d{i}_k{dim}_fixed"][:17]
    nodes = np.asarray(model.nodes[dim], dtype=float)
    _set_rows(model, form == "rows")
    try:
        for j in range(int(g34[f"d{i}_nspec"])):
            spec = [int(v) for v in g34[f"d{i}_s{j}_spec"]]
            fib = model.fibre_batch(dim, fixed, spec)
            assert fib.shape == (17, nodes.size)
            assert np.array_equal(fib, model.ladder_batch(dim, fixed, nodes, spec))
            # values on a node, among others and out of order: the fibre's own bits
            pick = [nodes.size - 1, 0, nodes.size // 2]
            xs = np.array([nodes[pick[0]], 0.5 * (nodes[0] + nodes[-1]) + 0.123 * (nodes[-1] - nodes[0]), nodes[pick[1]], nodes[pick[2]] + 5e-15])
            got = model.ladder_batch(dim, fixed, xs, spec)
            for col, p in ((0, pick[0]), (2, pick[1]), (3, pick[2])):
                assert np.array_equal(got[:, col], fib[:, p])
    finally:
        _set_rows(model, False)


@pytest.mark.parametrize("tag", TT_TAGS)
def test_tt_fibre_is_the_ladder_at_the_nodes(g34, tt_models, tag):
    tt = tt_models[tag]
    d = tt.num_dimensions
    for dim in [int(v) for v in g34[f"t{tag}_dims"]]:
        fixed = g34[f"t{tag}_k{dim}_fixed"][:17]
        pos = tt.dim_order.index(dim)
        nodes = ChebyshevTT.nodes(d, tt.domain, tt.n_nodes)["nodes_per_dim"][pos]
        fib = tt.fibre_batch(dim, fixed)
        assert fib.shape == (17, tt.n_nodes[pos])
        assert np.array_equal(fib, tt.ladder_batch(dim, fixed, nodes))
        # the fibre against the pointwise route
        pts = G.expand(d, dim, fixed, np.asarray(nodes, dtype=float))
        assert_parity(fib, tt.eval_batch(pts).reshape(fib.shape), tol=1e-12, what=f"TT fibre vs eval_batch {tag} dim {dim}")


# ------------------------------------------------------------------ 3. batch independence
@pytest.mark.parametrize("form", ["auto", "rows"])
@pytest.mark.parametrize("key", [(2, 1), (3, 0), (5, 0), (7, 3)], ids=["4x11x6_dim1", "17x3x2_dim0", "64x5_dim0", "bs_dim3"])
def test_dense_rows_do_not_depend_on_their_batch(g34, dense_models, key, form):
    i, dim = key
    model = dense_models[i]
    fixed, xs = g34[f"d{i}_k{dim}_fixed"], g34[f"d{i}_k{dim}_xs"]
    spec = [int(v) for v in g34[f"d{i}_s{int(g34[f'd{i}_nspec']) - 1}_spec"]]
    _set_rows(model, form == "rows")
    try:
        full = model.ladder_batch(dim, fixed, xs, spec)
        for r in (0, 15, 16, 57, 99):
            assert np.array_equal(model.ladder_batch(dim, fixed[r:r + 1], xs, spec), full[r:r + 1]), f"row {r} alone"
        assert np.array_equal(model.ladder_batch(dim, fixed, np.tile(xs, (fixed.shape[0], 1)), spec), full), "shared vs tiled xs"
        for m in (1, 5, 16):
            assert np.array_equal(model.ladder_batch(dim, fixed, xs[:m], spec), full[:, :m]), f"m = {m}"
    finally:
        _set_rows(model, False)


@pytest.mark.parametrize("tag", ["C", "G"])
def test_tt_rows_do_not_depend_on_their_batch(g34, tt_models, tag):
    tt = tt_models[tag]
    dim = int(g34[f"t{tag}_dims"][1])
    fixed, xs = g34[f"t{tag}_k{dim}_fixed"], g34[f"t{tag}_k{dim}_xs"]
    full = tt.ladder_batch(dim, fixed, xs)
    for r in (0, 63, 64, 99):
        assert np.array_equal(tt.ladder_batch(dim, fixed[r:r + 1], xs), full[r:r + 1]), f"row {r} alone"
    assert np.array_equal(tt.ladder_batch(dim, fixed, np.tile(xs, (fixed.shape[0], 1))), full)


# ------------------------------------------------------------------ 4. NaN
def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@pytest.mark.parametrize("form", ["auto", "rows"])
def test_dense_nan_stays_where_it_is(g34, dense_models, form):
    i, dim = 2, 1
    model = dense_models[i]
    fixed, xs = g34[f"d{i}_k{dim}_fixed"][:40].copy(), np.tile(g34[f"d{i}_k{dim}_xs"][:17], (40, 1))
    _set_rows(model, form == "rows")
    try:
        clean = model.ladder_batch(dim, fixed, xs)
        assert np.isfinite(clean).all()
        xs2 = xs.copy()
        xs2[17, 5] = np.nan
        got = model.ladder_batch(dim, fixed, xs2)
        assert np.isnan(got[17, 5])
        got[17, 5] = clean[17, 5]
        assert _same_bits(got, clean)
        fixed2 = fixed.copy()
        fixed2[18, 1] = np.nan
        got = model.ladder_batch(dim, fixed2, xs)
        assert np.isnan(got[18]).all()
        got[18] = clean[18]
        assert _same_bits(got, clean)
    finally:
        _set_rows(model, False)


@pytest.mark.parametrize("tag", ["C", "G"])
def test_tt_nan_stays_where_it_is(g34, tt_models, tag):
    tt = tt_models[tag]
    dim = int(g34[f"t{tag}_dims"][1])
    fixed, xs = g34[f"t{tag}_k{dim}_fixed"][:70].copy(), np.tile(g34[f"t{tag}_k{dim}_xs"], (70, 1))
    clean = tt.ladder_batch(dim, fixed, xs)
    xs2 = xs.copy()
    xs2[65, 3] = np.nan
    got = tt.ladder_batch(dim, fixed, xs2)
    assert np.isnan(got[65, 3])
    got[65, 3] = clean[65, 3]
    assert _same_bits(got, clean)
    fixed2 = fixed.copy()
    fixed2[3, 0] = np.nan
    got = tt.ladder_batch(dim, fixed2, xs)
    assert np.isnan(got[3]).all()
    got[3] = clean[3]
    assert _same_bits(got, clean)


# ------------------------------------------------------------------ 5. device arrays
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


def test_dense_device_arrays(g34, dense_models):
    model = dense_models[7]
    _device_forms(model, model._model().device, 2, g34["d7_k2_fixed"], g34["d7_k2_xs"], g34["d7_k2_xsrow"], derivative_order=[1, 0, 0, 0, 0])
    one = dense_models[0]
    _device_forms(one, one._model().device, 0, g34["d0_k0_fixed"], g34["d0_k0_xs"], g34["d0_k0_xsrow"])


@pytest.mark.parametrize("tag", ["C", "G"])
def test_tt_device_arrays(g34, tt_models, tag):
    tt = tt_models[tag]
    dim = int(g34[f"t{tag}_dims"][-1])
    _device_forms(tt, tt._dev().device, dim, g34[f"t{tag}_k{dim}_fixed"], g34[f"t{tag}_k{dim}_xs"], g34[f"t{tag}_k{dim}_xsrow"])


# ------------------------------------------------------------------ 6. the host staging pass edge
def _pass_rows(width, m):
    """include/pcx.h: max(1, 2^20 / max(staged doubles per row, m)) rows per pass"""
    return max(1, (1 << 20) // max(max(1, width), m))


@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "per_row"])
def test_dense_batch_across_the_pass_edge(g34, dense_models, per_row):
    model = dense_models[1]                      # 5 x 7, dim 0: one fixed coordinate per row
    m = 4
    P = _pass_rows(1 + (m if per_row else 0), m)
    N = P + 3
    rng = np.random.default_rng(34)
    fixed = rng.uniform(0.0, 2.0, (N, 1))
    xs = rng.uniform(-1.0, 1.0, (N, m)) if per_row else g34["d1_k0_xs"][:m]
    got = model.ladder_batch(0, fixed, xs)
    assert got.shape == (N, m)
    for r in (0, P - 1, P, N - 1):
        assert np.array_equal(got[r:r + 1], model.ladder_batch(0, fixed[r:r + 1], xs[r:r + 1] if per_row else xs)), f"row {r}"


def test_tt_batch_across_the_pass_edge(g34, tt_models):
    tt = tt_models["F"]
    d = tt.num_dimensions
    dim, m = 0, 4
    P = _pass_rows(d - 1, m)
    N = P + 3
    base = g34["tF_k0_fixed"]
    fixed = base[np.random.default_rng(35).integers(0, base.shape[0], N)]
    xs = g34["tF_k0_xs"][:m]
    got = tt.ladder_batch(dim, fixed, xs)
    for r in (0, P - 1, P, N - 1):
        assert np.array_equal(got[r:r + 1], tt.ladder_batch(dim, fixed[r:r + 1], xs)), f"row {r}"


# ------------------------------------------------------------------ 7. the existing route
@pytest.fixture(scope="module")
def bs11():
    g2 = golden("g2_bs5d")
    import functions as F
    n = list(F.BS5_NODES)
    return ChebyshevApproximation.from_values(g2["tensor"], 5, F.BS5_DOMAIN, n), F


@pytest.mark.parametrize("form", ["auto", "rows"])
@pytest.mark.parametrize("dim", [0, 2, 4])
def test_ladder_matches_vectorized_eval_batch_on_the_11_5_tensor(bs11, dim, form):
    model, F = bs11
    pts = F.bs5_query_points(64, seed=34 + dim)
    fixed = np.delete(pts, dim, axis=1)
    lo, hi = F.BS5_DOMAIN[dim]
    xs = np.linspace(lo, hi, 21)
    _set_rows(model, form == "rows")
    try:
        info = _info(model, dim)
        assert info == ([1, 121 * 31, 1] if form == "auto" else [0, 0, 0])
        for spec in ([0] * 5, [1, 0, 0, 0, 0]):
            got = model.ladder_batch(dim, fixed, xs, spec)
            want = model.vectorized_eval_batch(G.expand(5, dim, fixed, xs), spec).reshape(64, 21)
            e_norm, e_point = parity(got, want)
            print(f"11^5 dim {dim} {form} {spec}: ladder vs vectorized_eval_batch E_norm {e_norm:.2e} E_point {e_point:.2e}")
            assert e_norm <= 1e-12
    finally:
        _set_rows(model, False)


# more than one column tile on the prefetching main loop (k-steps of the low part >= its group of 16 / 8 / 4 steps), and a
# high part under it: n, dim -> (k-steps, column tiles)
WIDE = [((20, 30, 9, 5), 0, (30 * 12, 2)), ((6, 40, 3), 1, (5, 3)), ((4, 5, 64), 2, (5, 4)), ((7, 19, 24), 2, (34, 2))]


@pytest.mark.parametrize("case", WIDE, ids=["x".join(map(str, c[0])) + f"_dim{c[1]}" for c in WIDE])
def test_wide_fibres_match_the_rows_form_and_the_pointwise_route(case):
    n, dim, geometry = case
    d = len(n)
    domain = [[-1.0, 1.0 + 0.25 * k] for k in range(d)]
    nodes = ChebyshevApproximation.nodes(d, domain, list(n))["nodes_per_dim"]
    grids = np.meshgrid(*nodes, indexing="ij")
    tensor = 6.0 + np.exp(-0.3 * grids[0] * grids[1]) + sum(np.sin((k + 1) * 0.7 * gk) for k, gk in enumerate(grids))
    model = ChebyshevApproximation.from_values(tensor, d, domain, list(n))
    rng = np.random.default_rng(sum(n))
    fixed = np.column_stack([rng.uniform(domain[k][0], domain[k][1], 37) for k in range(d) if k != dim])
    fixed[3, 0] = nodes[0 if dim else 1][2]                       # an exact node in a fixed dimension
    lo, hi = domain[dim]
    xs = np.concatenate([rng.uniform(lo, hi, 18), [lo, hi, nodes[dim][1], nodes[dim][-2] + 5e-15]])
    assert _info(model, dim) == [1, *geometry]
    got = model.ladder_batch(dim, fixed, xs)
    want = model.vectorized_eval_batch(G.expand(d, dim, fixed, xs), [0] * d).reshape(got.shape)
    assert_parity(got, want, tol=1e-12, what=f"wide ladder {n} dim {dim} vs vectorized_eval_batch")
    fib = model.fibre_batch(dim, fixed)
    assert np.array_equal(fib, model.ladder_batch(dim, fixed, nodes[dim]))
    assert np.array_equal(model.ladder_batch(dim, fixed[5:6], xs), got[5:6])
    _set_rows(model, True)
    try:
        assert _info(model, dim) == [0, 0, 0]
        assert_parity(got, model.ladder_batch(dim, fixed, xs), tol=1e-12, what=f"wide ladder {n} dim {dim} vs the rows form")
        assert_parity(fib, model.fibre_batch(dim, fixed), tol=1e-12, what=f"wide fibre {n} dim {dim} vs the rows form")
    finally:
        _set_rows(model, False)


@pytest.mark.parametrize("tag", TT_TAGS)
def test_tt_ladder_matches_eval_batch(g34, tt_models, tag):
    tt = tt_models[tag]
    for dim in [int(v) for v in g34[f"t{tag}_dims"]]:
        fixed, xs = g34[f"t{tag}_k{dim}_fixed"], g34[f"t{tag}_k{dim}_xs"]
        want = tt.eval_batch(G.expand(tt.num_dimensions, dim, fixed, xs)).reshape(fixed.shape[0], xs.size)
        assert_parity(tt.ladder_batch(dim, fixed, xs), want, tol=1e-12, what=f"TT ladder vs eval_batch {tag} dim {dim}")


# ------------------------------------------------------------------ 8. C ABI
def test_abi_argument_errors(g34, dense_models, tt_models):
    lib = _lib.load()
    INV = _lib.PCX_ERR_INVALID
    model = dense_models[2]
    h = model._model().handle
    fixed, xs = _lib.f64(g34["d2_k1_fixed"][:4]), _lib.f64(g34["d2_k1_xs"][:3])
    out = np.full((4, 3), 7.0)
    spec = _lib.i32([0, 0, 0])
    pf, px, po, ps = _lib.p_f64(fixed), _lib.p_f64(xs), _lib.p_f64(out), _lib.p_i32(spec)
    assert lib.pcx_bary_ladder_batch(None, 1, ps, pf, 4, px, 3, 0, po) == INV
    assert lib.pcx_bary_ladder_batch(h, 3, ps, pf, 4, px, 3, 0, po) == INV
    assert lib.pcx_bary_ladder_batch(h, -1, ps, pf, 4, px, 3, 0, po) == INV
    assert lib.pcx_bary_ladder_batch(h, 1, ps, pf, -1, px, 3, 0, po) == INV
    assert lib.pcx_bary_ladder_batch(h, 1, ps, pf, 4, px, -1, 0, po) == INV
    assert lib.pcx_bary_ladder_batch(h, 1, ps, pf, 4, px, 3, 2, po) == INV
    assert lib.pcx_bary_ladder_batch(h, 1, ps, None, 4, px, 3, 0, po) == INV
    assert lib.pcx_bary_ladder_batch(h, 1, ps, pf, 4, None, 3, 0, po) == INV
    assert lib.pcx_bary_ladder_batch(h, 1, ps, pf, 4, px, 3, 0, None) == INV
    assert lib.pcx_bary_ladder_batch(h, 1, _lib.p_i32(_lib.i32([0, 9, 0])), pf, 4, px, 3, 0, po) == INV
    assert lib.pcx_bary_ladder_batch(h, 1, _lib.p_i32(_lib.i32([0, -1, 0])), pf, 4, px, 3, 0, po) == INV
    assert lib.pcx_bary_ladder_batch_dev(h, 1, ps, None, 4, px, 3, 0, None, None) == INV
    assert lib.pcx_bary_ladder_batch_dev(h, 5, ps, None, 0, px, 3, 0, None, None) == INV
    assert lib.pcx_bary_ladder_info(h, 3, _lib.p_i32(np.zeros(3, dtype=np.int32))) == INV
    assert lib.pcx_bary_ladder_info(h, 0, None) == INV
    assert (out == 7.0).all(), "a refused call wrote results"
    assert lib.pcx_bary_ladder_batch(h, 1, ps, pf, 0, px, 3, 0, po) == 0
    assert lib.pcx_bary_ladder_batch(h, 1, ps, pf, 4, px, 0, 0, po) == 0
    assert lib.pcx_bary_ladder_batch(h, 1, None, pf, 4, px, 3, 0, po) == 0          # NULL spec: the values
    assert np.array_equal(out, model.ladder_batch(1, fixed, xs))

    tt = tt_models["F"]
    t = tt._dev().handle
    tfixed, txs = _lib.f64(g34["tF_k0_fixed"][:4]), _lib.f64(g34["tF_k0_xs"][:3])
    tout = np.full((4, 3), 7.0)
    pf, px, po = _lib.p_f64(tfixed), _lib.p_f64(txs), _lib.p_f64(tout)
    d = tt.num_dimensions
    assert lib.pcx_tt_ladder_batch(None, 0, pf, 4, px, 3, 0, po) == INV
    assert lib.pcx_tt_ladder_batch(t, d, pf, 4, px, 3, 0, po) == INV
    assert lib.pcx_tt_ladder_batch(t, -1, pf, 4, px, 3, 0, po) == INV
    assert lib.pcx_tt_ladder_batch(t, 0, pf, -1, px, 3, 0, po) == INV
    assert lib.pcx_tt_ladder_batch(t, 0, pf, 4, px, -1, 0, po) == INV
    assert lib.pcx_tt_ladder_batch(t, 0, pf, 4, px, 3, -1, po) == INV
    assert lib.pcx_tt_ladder_batch(t, 0, None, 4, px, 3, 0, po) == INV
    assert lib.pcx_tt_ladder_batch(t, 0, pf, 4, None, 3, 0, po) == INV
    assert lib.pcx_tt_ladder_batch(t, 0, pf, 4, px, 3, 0, None) == INV
    assert lib.pcx_tt_ladder_batch_dev(t, 0, None, 4, px, 3, 0, None, None) == INV
    assert (tout == 7.0).all()
    assert lib.pcx_tt_ladder_batch(t, 0, pf, 0, px, 3, 0, po) == 0
    assert lib.pcx_tt_ladder_batch(t, 0, pf, 4, px, 0, 0, po) == 0
    assert lib.pcx_tt_ladder_batch(t, 0, pf, 4, px, 3, 0, po) == 0
    assert np.array_equal(tout, tt.ladder_batch(0, tfixed, txs))
