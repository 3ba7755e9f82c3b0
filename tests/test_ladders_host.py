"""``ladder_batch`` / ``fibre_batch`` without a GPU: the argument rules (every one is checked before the model goes to a
device), the C ABI's table, and the NumPy restatement of the fibre-then-1-D rule (tests/ladder_rule.py) against the
golden ladders of tests/golden/g34_ladders.npz to the bounds the device tests use -- the rule itself meets them."""
import re

import numpy as np
import pytest

from conftest import assert_parity, golden, spec_point_tol
import functions as F
import generate_golden_ladders as G
import ladder_rule

from pychebyshev_amd import ChebyshevApproximation, ChebyshevTT, _calculus, _lib


@pytest.fixture(scope="module")
def g34():
    return golden("g34_ladders")


@pytest.fixture(scope="module")
def dense(g34):
    n = [int(v) for v in g34["d2_n"]]
    return ChebyshevApproximation.from_values(g34["d2_tensor"], 3, g34["d2_domain"].tolist(), n)


@pytest.fixture(scope="module")
def tt(g34):
    g22 = golden("g22_tt_transforms")
    cores = [g22[f"C_core{k}"] for k in range(5)]
    return ChebyshevTT.from_coeff_cores(cores, g22["C_domain"].tolist(), dim_order=[int(v) for v in g34["tC_order"]])


def _fixed(obj, dim, N=3):
    dom = obj.domain if isinstance(obj, ChebyshevApproximation) else obj._user_frame_domain()
    return np.array([[0.5 * (dom[k][0] + dom[k][1]) for k in range(obj.num_dimensions) if k != dim]] * N)


@pytest.mark.parametrize("which", ["dense", "tt"])
def test_argument_rules(dense, tt, which):
    obj = dense if which == "dense" else tt
    d = obj.num_dimensions
    dom = obj.domain if which == "dense" else obj._user_frame_domain()
    good = _fixed(obj, 1)
    xs = np.linspace(dom[1][0], dom[1][1], 5)
    with pytest.raises(TypeError, match="dim must be an int, got float"):
        obj.ladder_batch(1.0, good, xs)
    with pytest.raises(TypeError, match="dim must be an int, got bool"):
        obj.fibre_batch(True, good)
    with pytest.raises(ValueError, match=re.escape(f"dim {d} out of range [0, {d - 1}]")):
        obj.ladder_batch(d, good, xs)
    with pytest.raises(ValueError, match=re.escape(f"dim -1 out of range [0, {d - 1}]")):
        obj.fibre_batch(-1, good)
    with pytest.raises(ValueError, match=re.escape(f"fixed must have shape (N, {d - 1}), got (3, {d})")):
        obj.ladder_batch(1, np.zeros((3, d)), xs)
    with pytest.raises(ValueError, match=re.escape(f"fixed must have shape (N, {d - 1}), got ({d - 1},)")):
        obj.ladder_batch(1, good[0], xs)
    bad = good.copy()
    bad[2, 0] = dom[0][1] + 1.0
    with pytest.raises(ValueError, match=re.escape(f"Fixed value {bad[2, 0]} for dim 0 outside domain [{dom[0][0]}, {dom[0][1]}] (row 2)")):
        obj.ladder_batch(1, bad, xs)
    bad = good.copy()
    bad[1, 1] = dom[2][0] - 1e-9
    with pytest.raises(ValueError, match=r"for dim 2 outside domain .* \(row 1\)"):
        obj.fibre_batch(1, bad)
    with pytest.raises(ValueError, match=re.escape("xs must have shape (m,) or (3, m), got (2, 5)")):
        obj.ladder_batch(1, good, np.zeros((2, 5)))
    with pytest.raises(ValueError, match=re.escape("xs must have shape (m,) or (3, m), got (3, 5, 1)")):
        obj.ladder_batch(1, good, np.zeros((3, 5, 1)))
    with pytest.raises(ValueError, match=re.escape("out.shape=(3, 4) does not match the result (3, 5)")):
        obj.ladder_batch(1, good, xs, out=np.empty((3, 4)))
    with pytest.raises(ValueError, match="out must be float64, got float32"):
        obj.ladder_batch(1, good, xs, out=np.empty((3, 5), dtype=np.float32))
    with pytest.raises(ValueError, match="out must be C-contiguous"):
        obj.ladder_batch(1, good, xs, out=np.empty((5, 3)).T)
    with pytest.raises(ValueError, match="out must be a DeviceArray, a float64 NumPy array or None"):
        obj.ladder_batch(1, good, xs, out=[[0.0] * 5] * 3)
    n_dim = obj.n_nodes[1] if which == "dense" else obj.n_nodes[obj.dim_order.index(1)]
    with pytest.raises(ValueError, match=re.escape(f"does not match the result (3, {n_dim})")):
        obj.fibre_batch(1, good, out=np.empty((3, n_dim + 1)))


def test_dense_spec_is_checked_before_any_device_call(dense):
    good = _fixed(dense, 0)
    with pytest.raises(ValueError, match="derivative_order must have 3 entries"):
        dense.ladder_batch(0, good, [0.0], [1, 0])


def test_nan_passes_the_domain_check_and_the_cap_is_gone():
    rows = np.array([[0.1, np.nan], [np.nan, 0.2]])
    out = _calculus.validate_fibre_args(3, 1, rows, [(-1, 1)] * 3)
    assert out.shape == (2, 2) and np.isnan(out[0, 1])
    n = [3, 200, 3]
    with pytest.raises(ValueError, match="at most 64"):
        _calculus.validate_batch_args(3, 1, rows[:, :2] * 0, [(-1, 1)] * 3, n)      # the solver's helper keeps its cap
    assert _calculus.validate_fibre_args(1, 0, np.empty((4, 0)), [(-1, 1)]).shape == (4, 0)
    assert _calculus.validate_fibre_args(1, 0, [], [(-1, 1)]).shape == (0, 0)


def test_xs_shapes():
    xs, m, per_row = _calculus.validate_ladder_xs(2.5, 7)
    assert xs.shape == (1,) and m == 1 and not per_row
    xs, m, per_row = _calculus.validate_ladder_xs(np.arange(6.0).reshape(2, 3), 2)
    assert xs.shape == (2, 3) and m == 3 and per_row
    xs, m, per_row = _calculus.validate_ladder_xs([], 2)
    assert m == 0 and not per_row
    xs, m, per_row = _calculus.validate_ladder_xs([np.nan, 1e300], 2)          # values are not checked
    assert m == 2


def test_unbuilt_models_say_build():
    a = ChebyshevApproximation(F.sin_cos_2d, 2, [[-1, 1], [0, 2]], [5, 7])
    t = ChebyshevTT(F.sin_sum_3d, 3, [[-1, 1]] * 3, [5, 5, 5])
    for obj, fixed in ((a, np.zeros((1, 1))), (t, np.zeros((1, 2)))):
        with pytest.raises(RuntimeError, match="build"):
            obj.ladder_batch(0, fixed, [0.0])
        with pytest.raises(RuntimeError, match="build"):
            obj.fibre_batch(0, fixed)


def test_the_abi_table_names_the_ladder_entries():
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pcx.h")) as fh:
        header = fh.read()
    for name in ("pcx_bary_ladder_batch", "pcx_bary_ladder_batch_dev", "pcx_bary_ladder_info", "pcx_tt_ladder_batch",
                 "pcx_tt_ladder_batch_dev"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\bint " + name + r"\(", header)
    assert len(_lib.SIGNATURES["pcx_bary_ladder_batch"][1]) == 9
    assert len(_lib.SIGNATURES["pcx_bary_ladder_batch_dev"][1]) == 10
    assert len(_lib.SIGNATURES["pcx_tt_ladder_batch"][1]) == 8
    assert len(_lib.SIGNATURES["pcx_tt_ladder_batch_dev"][1]) == 9


# ------------------------------------------------------------------ the rule against the golden ladders
DENSE_KEYS = [(i, dim) for i, c in enumerate(G.DENSE) for dim in c["dims"]]


@pytest.mark.parametrize("key", DENSE_KEYS, ids=["x".join(map(str, G.DENSE[i]["n"])) + f"_dim{dim}" for i, dim in DENSE_KEYS])
def test_the_dense_rule_meets_the_golden_ladders(g34, key):
    i, dim = key
    pre = f"d{i}_k{dim}"
    tensor, domain = g34[f"d{i}_tensor"], g34[f"d{i}_domain"].tolist()
    fixed, xs, xsrow = g34[f"{pre}_fixed"][:24], g34[f"{pre}_xs"], g34[f"{pre}_xsrow"]
    for j in range(int(g34[f"d{i}_nspec"])):
        spec = [int(v) for v in g34[f"d{i}_s{j}_spec"]]
        ok, rowok = g34[f"{pre}_s{j}_refok"], g34[f"{pre}_s{j}_refrowok"]
        got = ladder_rule.dense_ladder(tensor, domain, dim, fixed, xs, spec)
        assert_parity(got[:, ok], g34[f"{pre}_s{j}_ref"][:24][:, ok], tol=1e-12, what=f"rule {key} {spec} shared", point_tol=spec_point_tol(spec))
        got = ladder_rule.dense_ladder(tensor, domain, dim, fixed[:xsrow.shape[0]], xsrow, spec)
        assert_parity(got[rowok], g34[f"{pre}_s{j}_refrow"][rowok], tol=1e-12, what=f"rule {key} {spec} per row", point_tol=spec_point_tol(spec))


@pytest.mark.parametrize("tag", ["A", "C", "F", "G"])
def test_the_tt_rule_meets_the_golden_ladders(g34, tag):
    src, pre = (g34, "tG") if tag == "G" else (golden("g22_tt_transforms"), tag)
    cores, k = [], 0
    while f"{pre}_core{k}" in src.files:
        cores.append(src[f"{pre}_core{k}"])
        k += 1
    domain = src[f"{pre}_domain"].tolist()
    order = [int(v) for v in g34[f"t{tag}_order"]]
    for dim in [int(v) for v in g34[f"t{tag}_dims"]]:
        key = f"t{tag}_k{dim}"
        fixed, xs, xsrow = g34[f"{key}_fixed"][:24], g34[f"{key}_xs"], g34[f"{key}_xsrow"]
        ok, rowok = g34[f"{key}_refok"], g34[f"{key}_refrowok"]
        got = ladder_rule.tt_ladder(cores, domain, order, dim, fixed, xs)
        assert_parity(got[:, ok], g34[f"{key}_ref"][:24][:, ok], tol=1e-12, what=f"TT rule {tag} dim {dim} shared")
        got = ladder_rule.tt_ladder(cores, domain, order, dim, fixed[:xsrow.shape[0]], xsrow)
        assert_parity(got[rowok], g34[f"{key}_refrow"][rowok], tol=1e-12, what=f"TT rule {tag} dim {dim} per row")


def test_a_value_on_a_node_returns_the_fibre_itself(g34):
    tensor, domain = g34["d2_tensor"], g34["d2_domain"].tolist()
    cur, nodes, wts = ladder_rule.dense_setup(tensor, domain)
    fixed = g34["d2_k1_fixed"][:5]
    fib = ladder_rule.dense_fibres(cur, nodes, wts, 1, fixed)
    assert np.array_equal(ladder_rule.dense_ladder(tensor, domain, 1, fixed, nodes[1]), fib)
