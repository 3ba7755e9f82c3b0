"""Tensor-product grid evaluation on the device: ``ChebyshevApproximation.eval_grid`` (pcx_bary_eval_tensor_grid: d
rectangular mode products of the derivative tensor), ``ChebyshevTT.eval_grid`` (pcx_tt_tensor_grid: the chain of value
cores on the grid) and the primitive under both, ``pcx_tensor_mode_product``.

1. golden parity: tests/golden/g29_eval_grid.npz holds the reference's pointwise ``vectorized_eval`` / ``eval`` at every
   grid point; bounds 1e-12 normwise and spec_point_tol(spec) pointwise (tests/conftest.py), with auto and with each
   kernel form forced on every pass (PCX_GRID_VARIANT);
2. second route: the same grids through this library's own ``vectorized_eval_batch`` / ``eval_batch`` over the meshgrid,
   same bounds; ``out=DeviceArray`` gives the NumPy result bit for bit; the TT result has its axes in the user's order;
3. exact integers through ``pcx_tensor_mode_product``: X in [-8, 8], W in [-4, 4], every sum exact in FP64, so both
   forms must equal ``np.einsum("ji,oiq->ojq", W, X)`` EXACTLY at shapes on every tile edge; a lane map with the f32 row
   formula puts three results of four in the wrong row and fails here.  On random non-integer data the two forms agree
   BIT FOR BIT at every one of those shapes: the f64 MFMA is a k-ordered fma chain that starts from C and the k-steps
   run i ascending, so both forms sum every output in ascending i;
4. one-hot rows: a grid of exact nodes is the gather of ``tensor_values`` bit for bit, and a NaN in one tensor entry
   reaches exactly the grid points that select it (one-hot rows) or touch it (other rows) along all three axes;
5. argument errors of the C ABI and the Python API."""
import ctypes

import numpy as np
import pytest

from conftest import assert_parity, golden, spec_point_tol
import generate_golden_eval_grid as G

from pychebyshev_amd import ChebyshevApproximation, ChebyshevTT, _lib
from pychebyshev_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

DENSE_IDS = [G.case_id(i) for i in range(len(G.DENSE))]
TT_TAGS = list(G.TT_GRIDS)
# (outer, n, inner, m)
SHAPES = [(1, 1, 1, 1), (1, 3, 1, 17), (5, 4, 1, 16), (1, 7, 19, 33), (3, 11, 6, 18), (2, 64, 5, 1), (1, 8, 1, 1000),
          (1, 16, 40, 700), (37, 5, 1, 3), (2, 9, 130, 2)]


@pytest.fixture(scope="module")
def g29():
    return golden("g29_eval_grid")


@pytest.fixture(scope="module")
def dense_models(g29):
    """case number -> (model, axes, [(spec, reference grid)])"""
    out = {}
    for i in range(len(G.DENSE)):
        n = [int(v) for v in g29[f"d{i}_n"]]
        model = ChebyshevApproximation.from_values(g29[f"d{i}_tensor"], len(n), g29[f"d{i}_domain"].tolist(), n)
        axes = [g29[f"d{i}_ax{k}"] for k in range(len(n))]
        specs = [([int(v) for v in g29[f"d{i}_s{j}_spec"]], g29[f"d{i}_s{j}_ref"]) for j in range(int(g29[f"d{i}_nspec"]))]
        out[i] = (model, axes, specs)
    return out


@pytest.fixture(scope="module")
def tt_models(g29):
    """tag -> (model, axes in the user's order, reference grid)"""
    g22 = golden("g22_tt_transforms")
    out = {}
    for tag in TT_TAGS:
        cores, k = [], 0
        while f"{tag}_core{k}" in g22.files:
            cores.append(g22[f"{tag}_core{k}"])
            k += 1
        order = [int(v) for v in g29[f"t{tag}_order"]]
        tt = ChebyshevTT.from_coeff_cores(cores, g22[f"{tag}_domain"].tolist(), dim_order=order)
        out[tag] = (tt, [g29[f"t{tag}_ax{u}"] for u in range(len(cores))], g29[f"t{tag}_ref"])
    return out


def _mesh(axes):
    return np.column_stack([m.ravel() for m in np.meshgrid(*axes, indexing="ij")])


# ------------------------------------------------------------------ 1. golden parity
@pytest.mark.parametrize("variant", ["", "1", "2"], ids=["auto", "valu", "mfma"])
@pytest.mark.parametrize("i", range(len(G.DENSE)), ids=DENSE_IDS)
def test_dense_grid_matches_the_reference(dense_models, monkeypatch, i, variant):
    monkeypatch.setenv("PCX_GRID_VARIANT", variant)
    model, axes, specs = dense_models[i]
    for spec, ref in specs:
        got = model.eval_grid(axes, spec)
        assert got.shape == ref.shape
        assert_parity(got, ref, tol=1e-12, what=f"eval_grid {DENSE_IDS[i]} {spec} variant '{variant}'", point_tol=spec_point_tol(spec))
    assert_parity(model.eval_grid(axes), specs[0][1], tol=1e-12, what=f"eval_grid {DENSE_IDS[i]} without a spec")


@pytest.mark.parametrize("variant", ["", "1", "2"], ids=["auto", "valu", "mfma"])
@pytest.mark.parametrize("tag", TT_TAGS)
def test_tt_grid_matches_the_reference(tt_models, monkeypatch, tag, variant):
    monkeypatch.setenv("PCX_GRID_VARIANT", variant)
    tt, axes, ref = tt_models[tag]
    got = tt.eval_grid(axes)
    assert got.shape == ref.shape == tuple(a.size for a in axes)
    assert_parity(got, ref, tol=1e-12, what=f"TT eval_grid {tag} variant '{variant}'", point_tol=spec_point_tol([0]))


# ------------------------------------------------------------------ 2. second route
@pytest.mark.parametrize("i", range(len(G.DENSE)), ids=DENSE_IDS)
def test_dense_grid_matches_the_pointwise_route(dense_models, i):
    model, axes, specs = dense_models[i]
    pts = _mesh(axes)
    for spec, ref in specs:
        got = model.eval_grid(axes, spec)
        want = model.vectorized_eval_batch(pts, spec).reshape(ref.shape)
        assert_parity(got, want, tol=1e-12, what=f"eval_grid vs vectorized_eval_batch {DENSE_IDS[i]} {spec}", point_tol=spec_point_tol(spec))
        dev = model.eval_grid(axes, spec, out=DeviceArray.empty(ref.shape, model._model().device))
        assert isinstance(dev, DeviceArray) and dev.shape == ref.shape
        assert np.array_equal(dev.to_host(), got), "the device-resident result differs from the NumPy one"


def test_derivative_id_selects_the_spec(dense_models):
    model, axes, specs = dense_models[4]
    spec, _ = specs[1]
    assert np.array_equal(model.eval_grid(axes, derivative_id=model.get_derivative_id(spec)), model.eval_grid(axes, spec))


@pytest.mark.parametrize("tag", TT_TAGS)
def test_tt_grid_matches_eval_batch_in_user_order(tt_models, tag):
    tt, axes, ref = tt_models[tag]
    want = tt.eval_batch(_mesh(axes)).reshape(ref.shape)          # rows in the USER's order: so are the result's axes
    assert_parity(tt.eval_grid(axes), want, tol=1e-12, what=f"TT eval_grid vs eval_batch {tag}", point_tol=spec_point_tol([0]))


def test_scalar_axes_count_as_length_one(dense_models):
    model, axes, _ = dense_models[3]
    got = model.eval_grid([float(axes[0][0]), axes[1]])
    assert got.shape == (1, axes[1].size)
    assert np.array_equal(got, model.eval_grid([axes[0][:1], axes[1]]))


# ------------------------------------------------------------------ 3. the primitive
def _mode_product(X, W, variant):
    lib = _lib.load()
    outer, n, inner = X.shape
    m = W.shape[0]
    Y = np.full((outer, m, inner), np.nan)
    rc = lib.pcx_tensor_mode_product(_lib.default_device(), outer, n, inner, _lib.p_f64(X), m, _lib.p_f64(W), _lib.p_f64(Y), variant)
    assert rc == 0, _lib.last_error(lib)
    return Y


@pytest.mark.parametrize("variant", [1, 2], ids=["valu", "mfma"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_mode_product_is_exact_on_integers(shape, variant):
    outer, n, inner, m = shape
    rng = np.random.default_rng(sum(shape))
    X = rng.integers(-8, 9, (outer, n, inner)).astype(float)
    W = rng.integers(-4, 5, (m, n)).astype(float)
    assert np.array_equal(_mode_product(X, W, variant), np.einsum("ji,oiq->ojq", W, X))


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_both_forms_agree_bit_for_bit(shape):
    outer, n, inner, m = shape
    rng = np.random.default_rng(7 + sum(shape))
    X = rng.standard_normal((outer, n, inner))
    W = rng.standard_normal((m, n))
    valu, mfma, auto = (_mode_product(X, W, v) for v in (1, 2, 0))
    assert np.array_equal(valu, mfma) and np.array_equal(valu, auto)
    want = np.einsum("ji,oiq->ojq", W, X)
    assert np.max(np.abs(valu - want)) <= 4 * n * np.finfo(float).eps * np.max(np.abs(W)) * np.max(np.abs(X))


# ------------------------------------------------------------------ 4. one-hot rows
@pytest.mark.parametrize("variant", ["", "1", "2"], ids=["auto", "valu", "mfma"])
def test_node_grid_is_a_gather_and_nan_stays_where_it_belongs(monkeypatch, variant):
    monkeypatch.setenv("PCX_GRID_VARIANT", variant)
    rng = np.random.default_rng(4)
    n = (9, 17, 8)
    T = rng.standard_normal(n)
    T[0, 0, 0] = -0.0
    dom = [[-1.0, 1.0], [0.0, 3.0], [10.0, 11.0]]
    model = ChebyshevApproximation.from_values(T, 3, dom, list(n))
    pick = [np.array([3, 0, 8, 3, 5]), rng.permutation(17), np.array([7, 0, 2])]
    nodes_only = [np.asarray(model.nodes[k])[pick[k]] for k in range(3)]
    got = model.eval_grid(nodes_only)
    want = T[np.ix_(*pick)]
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
    # a NaN at (3, 11, 2): one-hot rows select it or not, every other row touches it
    Tn = T.copy()
    at = (3, 11, 2)
    Tn[at] = np.nan
    bad = ChebyshevApproximation.from_values(T, 3, dom, list(n))
    bad.tensor_values = Tn                     # from_values refuses a NaN; a replaced tensor is uploaded as it is
    axes, touches = [], []
    for k in range(3):
        x = np.asarray(bad.nodes[k])
        free = rng.uniform(dom[k][0], dom[k][1], 6)
        ax = np.concatenate([x[pick[k]], free, [x[at[k]], x[at[k]] + 5e-15]])
        perm = rng.permutation(ax.size)
        hot = np.concatenate([pick[k] == at[k], np.ones(6, bool), [True, True]])
        axes.append(ax[perm])
        touches.append(hot[perm])
    res = bad.eval_grid(axes)
    expect = touches[0][:, None, None] & touches[1][None, :, None] & touches[2][None, None, :]
    assert expect.any() and not expect.all()
    assert np.array_equal(np.isnan(res), expect)
    clean = [np.asarray(bad.nodes[k])[[i for i in range(n[k]) if i != at[k]]] for k in range(3)]
    assert np.all(np.isfinite(bad.eval_grid(clean)))
    # the finite part is what the clean model gives
    fine = model.eval_grid(axes)
    assert np.array_equal(res[~expect], fine[~expect])


# ------------------------------------------------------------------ 5. argument errors
def test_c_abi_argument_errors(dense_models):
    lib = _lib.load()
    dev = _lib.default_device()
    X, W, Y = np.ones((1, 2, 1)), np.ones((3, 2)), np.empty((1, 3, 1))
    px, pw, py = _lib.p_f64(X), _lib.p_f64(W), _lib.p_f64(Y)
    assert lib.pcx_tensor_mode_product(dev, 1, 2, 1, None, 3, pw, py, 0) == _lib.PCX_ERR_INVALID
    assert lib.pcx_tensor_mode_product(dev, 1, 2, 1, px, 3, None, py, 0) == _lib.PCX_ERR_INVALID
    assert lib.pcx_tensor_mode_product(dev, 1, 2, 1, px, 3, pw, None, 0) == _lib.PCX_ERR_INVALID
    assert lib.pcx_tensor_mode_product(dev, 1, 2, 1, px, 0, pw, py, 0) == _lib.PCX_ERR_INVALID
    assert lib.pcx_tensor_mode_product(dev, 0, 2, 1, px, 3, pw, py, 0) == _lib.PCX_ERR_INVALID
    for variant in (-1, 3):
        assert lib.pcx_tensor_mode_product(dev, 1, 2, 1, px, 3, pw, py, variant) == _lib.PCX_ERR_INVALID
        assert "variant" in _lib.last_error(lib)
    assert lib.pcx_tensor_mode_product(dev, 1 << 40, 2, 1, px, 3, pw, py, 0) == _lib.PCX_ERR_UNSUPPORTED

    model, axes, _ = dense_models[3]
    h = model._model().handle
    m = _lib.i32([a.size for a in axes])
    cat = _lib.f64(np.concatenate(axes))
    out = np.empty(tuple(m))
    assert lib.pcx_bary_eval_tensor_grid(None, None, _lib.p_i32(m), _lib.p_f64(cat), _lib.p_f64(out)) == _lib.PCX_ERR_INVALID
    assert lib.pcx_bary_eval_tensor_grid(h, None, None, _lib.p_f64(cat), _lib.p_f64(out)) == _lib.PCX_ERR_INVALID
    assert lib.pcx_bary_eval_tensor_grid(h, None, _lib.p_i32(m), None, _lib.p_f64(out)) == _lib.PCX_ERR_INVALID
    assert lib.pcx_bary_eval_tensor_grid(h, None, _lib.p_i32(m), _lib.p_f64(cat), None) == _lib.PCX_ERR_INVALID
    assert lib.pcx_bary_eval_tensor_grid_dev(h, None, _lib.p_i32(m), _lib.p_f64(cat), None, None) == _lib.PCX_ERR_INVALID
    m0 = _lib.i32([m[0], 0])
    assert lib.pcx_bary_eval_tensor_grid(h, None, _lib.p_i32(m0), _lib.p_f64(cat), _lib.p_f64(out)) == _lib.PCX_ERR_INVALID
    assert "dimension 1" in _lib.last_error(lib) and "empty" in _lib.last_error(lib)
    bad_spec = _lib.i32([9, 0])
    assert lib.pcx_bary_eval_tensor_grid(h, _lib.p_i32(bad_spec), _lib.p_i32(m), _lib.p_f64(cat), _lib.p_f64(out)) == _lib.PCX_ERR_INVALID
    # deriv == NULL is the plain value
    assert lib.pcx_bary_eval_tensor_grid(h, None, _lib.p_i32(m), _lib.p_f64(cat), _lib.p_f64(out)) == 0
    assert np.array_equal(out, model.eval_grid(axes, [0, 0]))

    cores = np.ones(3 * 2 + 2 * 4)
    mt, rk = _lib.i32([3, 4]), _lib.i32([1, 2, 1])
    res = np.empty((3, 4))
    assert lib.pcx_tt_tensor_grid(dev, 2, _lib.p_i32(mt), _lib.p_i32(rk), None, _lib.p_f64(res)) == _lib.PCX_ERR_INVALID
    assert lib.pcx_tt_tensor_grid(dev, 2, _lib.p_i32(mt), _lib.p_i32(rk), _lib.p_f64(cores), None) == _lib.PCX_ERR_INVALID
    assert lib.pcx_tt_tensor_grid(dev, 2, None, _lib.p_i32(rk), _lib.p_f64(cores), _lib.p_f64(res)) == _lib.PCX_ERR_INVALID
    assert lib.pcx_tt_tensor_grid(dev, 2, _lib.p_i32(_lib.i32([3, 0])), _lib.p_i32(rk), _lib.p_f64(cores), _lib.p_f64(res)) == _lib.PCX_ERR_INVALID
    assert "dimension 1" in _lib.last_error(lib)
    assert lib.pcx_tt_tensor_grid(dev, 2, _lib.p_i32(mt), _lib.p_i32(_lib.i32([2, 2, 1])), _lib.p_f64(cores), _lib.p_f64(res)) == _lib.PCX_ERR_INVALID
    assert lib.pcx_tt_tensor_grid(dev, 2, _lib.p_i32(mt), _lib.p_i32(rk), _lib.p_f64(cores), _lib.p_f64(res)) == 0
    assert np.array_equal(res, np.full((3, 4), 2.0))


def test_python_argument_errors(dense_models):
    model, axes, _ = dense_models[3]
    with pytest.raises(ValueError, match="2 entries"):
        model.eval_grid(axes[:1])
    with pytest.raises(ValueError, match=r"axes\[1\] is empty: dimension 1"):
        model.eval_grid([axes[0], []])
    with pytest.raises(ValueError, match="at dimension 0"):
        model.eval_grid(axes, out=DeviceArray.empty((axes[0].size + 1, axes[1].size), model._model().device))
    with pytest.raises(ValueError, match="outside"):
        model.eval_grid(axes, [9, 0])


def test_out_on_another_device_is_refused(dense_models):
    if _lib.device_count() < 2:
        pytest.skip("needs two devices")
    model, axes, _ = dense_models[3]
    here = model._model().device
    other = DeviceArray.empty(tuple(a.size for a in axes), (here + 1) % _lib.device_count())
    with pytest.raises(ValueError, match=f"device {other.device}"):
        model.eval_grid(axes, out=other)
