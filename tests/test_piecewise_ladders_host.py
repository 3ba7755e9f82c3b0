"""``ChebyshevSpline`` / ``ChebyshevSlider`` ``ladder_batch`` and ``fibre_batch`` without a GPU: the argument rules (every
one is checked before the model goes to a device, with the dense ladder's messages), the C ABI's table, and the NumPy
restatement of routing, fibre, 1-D interpolant and slider sum (tests/piecewise_ladder_rule.py) against the golden ladders
of tests/golden/g35_piecewise_ladders*.npz to the bounds the device tests use -- the rule itself meets them."""
import os
import re

import numpy as np
import pytest

from conftest import assert_parity, golden, spec_point_tol
import generate_golden_piecewise_ladders as G
import generate_golden_slider_calculus as SL
import generate_golden_spline_transforms as SP
import piecewise_ladder_rule as rule

from pychebyshev_amd import ChebyshevSlider, ChebyshevSpline, _lib

RULE_ROWS = 32        # the feature rows 0 .. 23 and some interior ones: the rule is slow Python


@pytest.fixture(scope="module")
def models():
    out = {"s" + c: SP.build(ChebyshevSpline, c) for c in G.SPLINE_CASES}
    out.update({"l" + c: SL.build(ChebyshevSlider, c) for c in G.SLIDER_CASES})
    return out


def _fixed(obj, dim, N=3):
    return np.array([[0.5 * (obj.domain[k][0] + obj.domain[k][1]) for k in range(obj.num_dimensions) if k != dim]] * N)


@pytest.mark.parametrize("tag", ["sm", "lb"])
def test_argument_rules(models, tag):
    obj = models[tag]
    d, dom = obj.num_dimensions, obj.domain
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
    with pytest.raises(ValueError, match=f"derivative_order must have {d} entries"):
        obj.ladder_batch(1, good, xs, [1, 0])
    with pytest.raises(ValueError, match="not both"):
        obj.ladder_batch(1, good, xs, [0] * d, derivative_id=0)
    n_fibre = sum(SP.piece_counts("m", 1)) if tag == "sm" else obj.n_nodes[1]
    with pytest.raises(ValueError, match=re.escape(f"does not match the result (3, {n_fibre})")):
        obj.fibre_batch(1, good, out=np.empty((3, n_fibre + 1)))


def test_unbuilt_models_say_build():
    c, s = SP.CASES["k"], SL.CASES["a"]
    sp = ChebyshevSpline(c["f"], c["d"], c["domain"], n_nodes=c["n_nodes"], knots=c["knots"])
    sl = ChebyshevSlider(s["f"], s["d"], s["domain"], s["n_nodes"], partition=s["partition"], pivot_point=s["pivot"])
    for obj, fixed in ((sp, np.zeros((1, 1))), (sl, np.zeros((1, 2)))):
        with pytest.raises(RuntimeError, match="build"):
            obj.ladder_batch(0, fixed, [0.0])
        with pytest.raises(RuntimeError, match="build"):
            obj.fibre_batch(0, fixed)


def test_the_abi_table_names_the_ladder_entries():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pcx.h")) as fh:
        header = fh.read()
    for name in ("pcx_spline_ladder_batch", "pcx_slider_ladder_batch"):
        assert len(_lib.SIGNATURES[name][1]) == 9 and len(_lib.SIGNATURES[name + "_dev"][1]) == 10
        assert re.search(r"\bint " + name + r"\(", header) and re.search(r"\bint " + name + r"_dev\(", header)


def test_routing_rule():
    assert rule.route([0.2], 2, [0.1, 0.2, np.nextafter(0.2, 0.0), 5.0, -5.0, np.nan]).tolist() == [0, 1, 0, 1, 0, 1]
    assert rule.route([], 1, [0.3, np.nan]).tolist() == [0, 0]
    assert rule.route([95.0, 100.0, 105.0], 4, [100.0, 94.9, np.nan, 105.0]).tolist() == [2, 0, 3, 3]
    from generate_golden_piecewise_grid import route as grid_route
    vals = np.array([79.0, 95.0, 99.9, 100.0, 104.0, 105.0, 121.0, np.nan])
    assert np.array_equal(rule.route([95.0, 100.0, 105.0], 4, vals), grid_route([95.0, 100.0, 105.0], 4, vals))


KEYS = [("s" + c, dim) for c in G.SPLINE_CASES for dim in range(SP.CASES[c]["d"])]
KEYS += [("l" + c, dim) for c in G.SLIDER_CASES for dim in range(SL.CASES[c]["d"])]


@pytest.mark.parametrize("key", KEYS, ids=[f"{t}_dim{k}" for t, k in KEYS])
def test_the_rule_meets_the_golden_ladders(models, key):
    tag, dim = key
    g = golden(G.file_of(tag))
    obj = models[tag]
    specs = (G.SPLINE_SPECS if tag[0] == "s" else G.SLIDER_SPECS)[tag[1]]
    run = rule.spline_rule if tag[0] == "s" else rule.slider_rule
    pre = f"{tag}_k{dim}"
    fixed, xs, xsrow = g[f"{pre}_fixed"][:RULE_ROWS], g[f"{pre}_xs"], g[f"{pre}_xsrow"]
    for j, spec in enumerate(specs):
        ok, rowok = g[f"{pre}_s{j}_refok"], g[f"{pre}_s{j}_refrowok"]
        got = run(obj, dim, fixed, xs, spec)
        assert_parity(got[:, ok], g[f"{pre}_s{j}_ref"][:RULE_ROWS][:, ok], tol=1e-12, what=f"rule {key} {spec} shared",
                      point_tol=spec_point_tol(spec))
        got = run(obj, dim, fixed[:xsrow.shape[0]], xsrow, spec)
        assert_parity(got[rowok], g[f"{pre}_s{j}_refrow"][rowok], tol=1e-12, what=f"rule {key} {spec} per row",
                      point_tol=spec_point_tol(spec))


def test_the_cross_slide_spec_is_plus_zero(models):
    sl = models["lc"]
    g = golden(G.file_of("lc"))
    got = rule.slider_rule(sl, 0, g["lc_k0_fixed"][:5], g["lc_k0_xs"], G.SLIDER_ZERO["c"])
    assert np.all(got == 0.0) and not np.any(np.signbit(got))
