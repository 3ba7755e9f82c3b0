"""ChebyshevSlider slice / extrude / integrate / calculus: what needs no device.  Argument rules and messages, the index
remapping, and -- with the two device primitives the host code calls (the axis contraction and a slide's evaluation)
replaced by NumPy -- the structure and numbers of slice / integrate against the reference (golden g25), and the box
formula of pcx_slider_box_batch restated on the host against the reference's integrate(dims, bounds).eval(point)."""
import numpy as np
import pytest

from conftest import golden

import generate_golden_slider_calculus as G
from pychebyshev_amd import ChebyshevApproximation, ChebyshevSlider, _calculus


@pytest.fixture(scope="module")
def g25():
    return golden("g25_slider_calculus")


@pytest.fixture
def host_primitives(monkeypatch):
    """tensor x_axis vec and a slide's value, in NumPy."""
    def contract(self, tensor, axis, vec):
        return np.tensordot(tensor, vec, axes=([axis], [0]))

    def value(self, point, derivative_order=None, *, derivative_id=None):
        t = np.asarray(self.tensor_values, dtype=float)
        for k in range(self.num_dimensions - 1, -1, -1):
            diff = point[k] - self.nodes[k]
            j = int(np.argmin(np.abs(diff)))
            if abs(diff[j]) < 1e-14:
                t = np.take(t, j, axis=k)
            else:
                u = self.weights[k] / diff
                t = np.tensordot(t, u / u.sum(), axes=([k], [0]))
        return float(t)
    monkeypatch.setattr(ChebyshevApproximation, "_contract", contract)
    monkeypatch.setattr(ChebyshevApproximation, "vectorized_eval", value)


_BUILT = {}


def _slider(case) -> ChebyshevSlider:
    if case not in _BUILT:
        _BUILT[case] = G.build(ChebyshevSlider, case)
    return _BUILT[case]


def _partition(g, tag):
    dims, out, at = g[f"{tag}_part_dims"].tolist(), [], 0
    for s in g[f"{tag}_part_sizes"]:
        out.append(dims[at:at + s])
        at += s
    return out


def _check_slider(got, g, tag):
    partition = _partition(g, tag)
    assert got._built and got.function is None and got.__dict__["_device_slider"] is None
    assert [list(grp) for grp in got.partition] == partition, tag
    assert got.num_dimensions == len(got.pivot_point) == g[f"{tag}_domain"].shape[0]
    assert np.array_equal(np.asarray(got.domain, dtype=float), g[f"{tag}_domain"]), tag
    assert list(got.n_nodes) == g[f"{tag}_n_nodes"].tolist(), tag
    assert got._dim_to_slide == {d: i for i, grp in enumerate(partition) for d in grp}
    for slide, grp in zip(got.slides, partition):
        assert slide.num_dimensions == len(grp) and slide.n_nodes == [got.n_nodes[d] for d in grp]
        assert [list(b) for b in slide.domain] == [list(got.domain[d]) for d in grp]
    want_pv = float(g[f"{tag}_pivot_value"])
    scale = max(max(float(np.max(np.abs(g[f"{tag}_tensor{j}"]))) for j in range(len(partition))), abs(want_pv))
    assert abs(got.pivot_value - want_pv) <= 1e-12 * scale, tag
    for j, slide in enumerate(got.slides):
        assert np.max(np.abs(slide.tensor_values - g[f"{tag}_tensor{j}"])) <= 1e-12 * scale, (tag, j)


def test_unbuilt_slider_refuses():
    c = G.CASES["a"]
    sl = ChebyshevSlider(c["f"], c["d"], c["domain"], c["n_nodes"], partition=c["partition"], pivot_point=c["pivot"])
    calls = [lambda: sl.slice((0, 0.1)), lambda: sl.extrude((0, (0.0, 1.0), 3)), lambda: sl.integrate(),
             lambda: sl.integrate_batch([0], None, np.zeros((1, 2))), lambda: sl.roots(0, {1: 0.0, 2: 0.0}),
             lambda: sl.minimize(0, {1: 0.0, 2: 0.0}), lambda: sl.maximize(0, {1: 0.0, 2: 0.0}),
             lambda: sl.roots_batch(0, np.zeros((1, 2))), lambda: sl.minimize_batch(0, np.zeros((1, 2))),
             lambda: sl.maximize_batch(0, np.zeros((1, 2)))]
    for call in calls:
        with pytest.raises(RuntimeError, match=r"Call build\(\) first"):
            call()


def test_extrude_matches_reference_and_validates(g25):
    for case, sets in G.EXTRUDE_SETS.items():
        sl = _slider(case)
        for i, params in enumerate(sets):
            got = sl.extrude(params)
            _check_slider(got, g25, f"{case}_ex{i}")
            for (k, (lo, hi), n) in params:
                assert got.pivot_point[k] == 0.5 * (lo + hi)
                j = got._dim_to_slide[k]
                assert got.partition[j] == [k] and np.array_equal(got.slides[j].tensor_values, np.full(n, sl.pivot_value))
            assert got.slides[:len(sl.slides)] == sl.slides and got.pivot_value == sl.pivot_value
    sl = _slider("a")
    assert sl.extrude((3, (0.0, 1.0), 4)).partition == [[0], [1], [2], [3]]
    assert sl.extrude((0, (0.0, 1.0), 4)).partition == [[1], [2], [3], [0]]
    assert sl.extrude([(1, (0.0, 1.0), 4), (3, (0.0, 1.0), 2)]).partition == [[0], [2], [4], [1], [3]]
    assert sl.partition == [[0], [1], [2]]                       # the source is untouched
    with pytest.raises(TypeError, match="dim_index must be int, got float"):
        sl.extrude([(1.0, (0.0, 1.0), 4)])
    with pytest.raises(ValueError, match=r"dim_index 4 out of range \[0, 3\]"):
        sl.extrude((4, (0.0, 1.0), 4))
    with pytest.raises(ValueError, match="Duplicate dim_index 1"):
        sl.extrude([(1, (0.0, 1.0), 4), (1, (0.0, 1.0), 4)])
    with pytest.raises(ValueError, match="Domain bounds must satisfy lo < hi"):
        sl.extrude((1, (1.0, 1.0), 4))
    with pytest.raises(ValueError, match="n_nodes must be int >= 2, got 1"):
        sl.extrude((1, (0.0, 1.0), 1))


def test_slice_matches_reference_and_validates(g25, host_primitives):
    for case, sets in G.SLICE_SETS.items():
        sl = _slider(case)
        for i, params in enumerate(sets):
            _check_slider(sl.slice(params), g25, f"{case}_sl{i}")
    sl = _slider("b")
    assert sl.slice((2, 0.5)).partition == [[0, 1], [2, 3]]          # a one-dimension group goes
    assert sl.slice((0, 100.0)).partition == [[0], [1], [2, 3]]      # a multi-dimension group shrinks
    assert sl.slice([(4, 0.03), (1, 100.0), (2, 0.5)]).partition == [[0], [1]]
    one = sl.slice((2, 0.5))
    assert one.pivot_value == sl.slides[1].vectorized_eval([0.5], [0]) and one.pivot_point == [100.0, 100.0, 0.25, 0.04]
    delta = one.pivot_value - sl.pivot_value
    assert np.array_equal(one.slides[0].tensor_values, sl.slides[0].tensor_values + delta)
    with pytest.raises(ValueError, match=r"Cannot slice all 5 dimensions"):
        sl.slice([(k, sl.pivot_point[k]) for k in range(5)])
    with pytest.raises(TypeError, match="dim_index must be int"):
        sl.slice([("0", 100.0)])
    with pytest.raises(ValueError, match=r"dim_index 5 out of range \[0, 4\]"):
        sl.slice((5, 0.0))
    with pytest.raises(ValueError, match="Duplicate dim_index 2"):
        sl.slice([(2, 0.5), (2, 0.6)])
    with pytest.raises(ValueError, match=r"Slice value 2.0 for dim 2 is outside domain \[0.25, 1.0\]"):
        sl.slice((2, 2.0))


def test_integrate_matches_reference_and_validates(g25, host_primitives):
    for case, sets in G.INT_SETS.items():
        sl = _slider(case)
        dom = np.asarray(sl.domain, dtype=float)
        scale = float(np.prod(dom[:, 1] - dom[:, 0])) * max(float(np.max(np.abs(s.tensor_values))) for s in sl.slides)
        assert abs(sl.integrate() - float(g25[f"{case}_int_full"])) <= 1e-12 * scale
        assert abs(sl.integrate(None, list(G.SUB_BOUNDS[case])) - float(g25[f"{case}_int_sub"])) <= 1e-12 * scale
        for i, (dims, bounds) in enumerate(sets):
            _check_slider(sl.integrate(dims, bounds), g25, f"{case}_int{i}")
    sl = _slider("b")
    assert sl.integrate(0).partition == [[0], [1], [2, 3]] and sl.integrate([2]).partition == [[0, 1], [2, 3]]
    assert sl.integrate([4, 0, 0]).partition == [[0], [1], [2]]
    assert isinstance(sl.integrate([0, 1, 2, 3, 4]), float)
    with pytest.raises(ValueError, match=r"dim 5 out-of-range \[0, 4\]"):
        sl.integrate([5])
    with pytest.raises(ValueError, match="bounds length 2 != dims length 1"):
        sl.integrate([0], [(80.0, 90.0), (90.0, 100.0)])
    with pytest.raises(ValueError, match=r"bounds lo=110.0 > hi=90.0 for dim 0"):
        sl.integrate([0], [(110.0, 90.0)])
    with pytest.raises(ValueError, match=r"outside domain \[0.25, 1.0\] for dim 2"):
        sl.integrate([0, 2], [None, (0.0, 0.5)])


def test_box_formula_on_the_host_matches_reference(g25, host_primitives):
    """out = pv vol_T + sum_i vol(T \\ G_i) (I_i - pv vol(T n G_i)), as k_slider_box_combine forms it from the rows that
    box_rows lays out, with I_i from the slide's own integrate / evaluation."""
    for case, sets in G.BOX_SETS.items():
        sl = _slider(case)
        d = sl.num_dimensions
        for i, dims in enumerate(sets):
            bounds, pts = g25[f"{case}_box{i}_bounds"], g25[f"{case}_box{i}_points"]
            flags, rows = _calculus.box_rows(d, sl.domain, dims, bounds, pts if len(dims) < d else None)
            assert flags.tolist() == [int(u in dims) for u in range(d)] and rows.shape == (bounds.shape[0], d + len(dims))
            off = [u + int(np.sum(flags[:u])) for u in range(d)]
            got = np.empty(rows.shape[0])
            for r, row in enumerate(rows):
                width = {u: row[off[u] + 1] - row[off[u]] for u in dims}
                vol_t = float(np.prod([width[u] for u in dims]))
                acc = sl.pivot_value * vol_t
                for slide, grp in zip(sl.slides, sl.partition):
                    local = [k for k, u in enumerate(grp) if flags[u]]
                    part = slide.integrate(local, [(row[off[grp[k]]], row[off[grp[k]] + 1]) for k in local]) if local else slide
                    kept = [row[off[u]] for u in grp if not flags[u]]
                    I = part.vectorized_eval(kept, [0] * len(kept)) if kept else float(part)
                    vin = float(np.prod([width[u] for u in dims if u in grp]))
                    vout = float(np.prod([width[u] for u in dims if u not in grp]))
                    acc += vout * (I - sl.pivot_value * vin)
                got[r] = acc
            want = g25[f"{case}_box{i}_values"]
            assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (case, dims)
    sl = _slider("b")
    with pytest.raises(ValueError, match="points is required: 4 dimensions are kept"):
        sl.integrate_batch([0])
    with pytest.raises(ValueError, match="out-of-range index"):
        sl.integrate_batch([7], None, np.zeros((1, 4)))
    with pytest.raises(ValueError, match=r"bounds lo=100.0 > hi=90.0 for dim 0 \(row 0\)"):
        sl.integrate_batch([0], [(100.0, 90.0)], np.array([[100.0, 0.5, 0.2, 0.03]]))


def test_calculus_argument_rules():
    sl = _slider("b")
    with pytest.raises(ValueError, match="dim is required for multi-D interpolant"):
        sl.roots()
    with pytest.raises(ValueError, match=r"dim 7 out of range \[0, 4\]"):
        sl.minimize(7, {})
    with pytest.raises(ValueError, match="fixed must specify all dims except 1"):
        sl.maximize(1, {0: 100.0})
    with pytest.raises(ValueError, match=r"Fixed value 70.0 for dim 0 outside domain \[80.0, 120.0\]"):
        sl.roots(1, {0: 70.0, 2: 0.5, 3: 0.2, 4: 0.03})
    with pytest.raises(ValueError, match=r"fixed must have shape \(N, 4\), got \(3, 2\)"):
        sl.roots_batch(0, np.zeros((3, 2)))
    with pytest.raises(ValueError, match=r"outside domain \[90.0, 110.0\] \(row 1\)"):
        sl.minimize_batch(0, np.array([[100.0, 0.5, 0.2, 0.03], [111.0, 0.5, 0.2, 0.03]]))
    with pytest.raises(ValueError, match="70 nodes"):
        _slider("l").roots_batch(0, np.array([[0.4]]))
    nodes, weights, diff = sl._owner_grid(4)
    assert nodes is sl.slides[2].nodes[1] and diff is sl.slides[2].diff_matrices[1] and weights.shape == (5,)
