"""ChebyshevSpline slice / extrude / batched calculus and ChebyshevApproximation.extrude: what needs no device.  Argument
rules with the reference's messages and types, extrude (a host copy: tensors exactly equal) against the reference (golden
g26) in structure and in the form of ``n_nodes``, the batch argument checks, and the host merge of the pieces' results
(``_calculus.merge_pieces``, the restatement of k_spline_calc_merge) on the reference's own per-piece roots."""
import numpy as np
import pytest

from conftest import golden

import generate_golden_spline_transforms as G
from pychebyshev_amd import ChebyshevApproximation, ChebyshevSpline, _calculus


@pytest.fixture(scope="module")
def g26():
    return golden("g26_spline_transforms")


_BUILT = {}


def _spline(case) -> ChebyshevSpline:
    if case not in _BUILT:
        _BUILT[case] = G.build(ChebyshevSpline, case)
    return _BUILT[case]


# ------------------------------------------------------------------ unbuilt objects, argument errors
def test_unbuilt_objects_refuse():
    sp = ChebyshevSpline(G.f_z, 2, [[-1.0, 1.0], [0.0, 1.0]], n_nodes=[8, 5], knots=[[0.2], []])
    calls = [lambda: sp.slice((1, 0.3)), lambda: sp.extrude((0, (0.0, 1.0), 3)), lambda: sp.roots_batch(0, np.array([[0.3]])),
             lambda: sp.minimize_batch(0, np.array([[0.3]])), lambda: sp.maximize_batch(0, np.array([[0.3]]))]
    ap = ChebyshevApproximation(G.f_z, 2, [[-1.0, 1.0], [0.0, 1.0]], [8, 5])
    calls.append(lambda: ap.extrude((0, (0.0, 1.0), 3)))
    for call in calls:
        with pytest.raises(RuntimeError, match=r"Call build\(\) first"):
            call()


@pytest.mark.parametrize("make", [lambda: _spline("k"), lambda: G.build_dense(ChebyshevApproximation)], ids=["spline", "dense"])
def test_extrude_argument_errors(make):
    obj = make()                                                   # two dimensions
    with pytest.raises(TypeError, match="dim_index must be int, got float"):
        obj.extrude([(0.0, (0.0, 1.0), 3)])
    with pytest.raises(TypeError, match="dim_index must be int, got str"):
        obj.extrude([("0", (0.0, 1.0), 3)])
    with pytest.raises(ValueError, match=r"dim_index 3 out of range \[0, 2\]"):
        obj.extrude((3, (0.0, 1.0), 3))
    with pytest.raises(ValueError, match=r"dim_index -1 out of range \[0, 3\]"):
        obj.extrude([(0, (0.0, 1.0), 3), (-1, (0.0, 1.0), 3)])
    with pytest.raises(ValueError, match="Duplicate dim_index 1"):
        obj.extrude([(1, (0.0, 1.0), 3), (1, (0.0, 2.0), 4)])
    with pytest.raises(ValueError, match=r"Domain bounds must satisfy lo < hi, got \[1.0, 1.0\]"):
        obj.extrude((0, (1.0, 1.0), 3))
    with pytest.raises(ValueError, match="n_nodes must be int >= 2, got 1"):
        obj.extrude((0, (0.0, 1.0), 1))
    with pytest.raises(ValueError, match="n_nodes must be int >= 2, got 3.0"):
        obj.extrude((0, (0.0, 1.0), 3.0))


def test_slice_argument_errors():
    sp = _spline("m")
    with pytest.raises(TypeError, match="dim_index must be int, got float"):
        sp.slice([(1.0, 0.1)])
    with pytest.raises(ValueError, match=r"dim_index 3 out of range \[0, 2\]"):
        sp.slice((3, 0.1))
    with pytest.raises(ValueError, match="Duplicate dim_index 2"):
        sp.slice([(2, 0.3), (2, 0.2)])
    with pytest.raises(ValueError, match=r"Cannot slice all 3 dimensions \(would produce 0D result\)"):
        sp.slice([(0, 100.0), (1, 0.1), (2, 0.3)])
    with pytest.raises(ValueError, match=r"Slice value 79.0 for dim 0 is outside domain \[80.0, 120.0\]"):
        sp.slice((0, 79.0))
    with pytest.raises(ValueError, match=r"Slice value 0.5 for dim 2 is outside domain \[0.1, 0.4\]"):
        sp.slice([(1, 0.1), (2, 0.5)])
    with pytest.raises(ValueError, match=r"Cannot slice all 1 dimensions"):
        _spline("o").slice((0, 0.1))


def test_batch_argument_errors():
    sp = _spline("m")
    rows = G.calculus_rows("m", 0)
    for fn in (sp.roots_batch, sp.minimize_batch, sp.maximize_batch):
        with pytest.raises(TypeError, match="dim must be an int, got float"):
            fn(0.0, rows)
        with pytest.raises(TypeError, match="dim must be an int, got bool"):
            fn(True, rows)
        with pytest.raises(ValueError, match=r"dim 3 out of range \[0, 2\]"):
            fn(3, rows)
        with pytest.raises(ValueError, match=r"fixed must have shape \(N, 2\), got \(12, 1\)"):
            fn(0, rows[:, :1])
        bad = rows.copy()
        bad[7, 1] = 0.45                                          # dimension 2 lives in [0.1, 0.4]
        with pytest.raises(ValueError, match=r"Fixed value 0\.45 for dim 2 outside domain \[0\.1, 0\.4\] \(row 7\)"):
            fn(0, bad)
    with pytest.raises(ValueError, match=r"fixed must have shape \(N, 0\)"):
        _spline("o").roots_batch(0, np.zeros((3, 1)))
    # more than 64 nodes in one piece along the dimension: refused as by the other classes; other dimensions are not
    long = ChebyshevSpline(lambda x, _=None: np.sin(5.0 * x[0]) + x[1], 2, [[-1.0, 1.0], [0.0, 1.0]],
                           n_nodes=[[5, 70], [4]], knots=[[0.0], []])
    long.build(verbose=False)
    with pytest.raises(ValueError, match="dimension 0 has 70 nodes: the batched solver takes at most 64"):
        long.roots_batch(0, np.array([[0.5]]))
    with pytest.raises(ValueError, match="dimension 0 has 70 nodes"):
        long.maximize_batch(0, np.array([[0.5]]))
    assert long._dim_counts(0) == [5, 70] and long._dim_counts(1) == [4]


# ------------------------------------------------------------------ extrude: a copy
@pytest.mark.parametrize("case", sorted(G.EXTRUDE_SETS))
def test_spline_extrude_equals_reference_exactly(g26, case):
    sp = _spline(case)
    for i, params in enumerate(G.EXTRUDE_SETS[case]):
        tag = f"{case}_ex{i}"
        want = G.stored_spline(g26, tag)
        got = sp.extrude(params if len(params) > 1 else params[0])
        G.check_structure(got, want, sp, tag)
        for piece, t in zip(got._pieces, want["tensors"]):
            assert np.array_equal(piece.tensor_values, t), tag
        assert got._n_nodes_nested == isinstance(G.CASES[case]["n_nodes"][0], list)        # flat stays flat, nested nested
        for k, (dim_idx, (lo, hi), n) in enumerate(sorted(params)):
            assert got.knots[dim_idx] == [] and got._shape[dim_idx] == 1 and got.domain[dim_idx] == [lo, hi]
            assert got.n_nodes[dim_idx] == ([n] if got._n_nodes_nested else n)
            for piece in got._pieces:
                assert piece.n_nodes[dim_idx] == n and piece.nodes[dim_idx].shape == (n,)
    assert sp.num_dimensions == G.CASES[case]["d"]               # the source is untouched


def test_dense_extrude_equals_reference_exactly(g26):
    from pychebyshev_amd.barycentric import chebyshev_nodes, compute_barycentric_weights, compute_differentiation_matrix
    c = G.build_dense(ChebyshevApproximation)
    for i, params in enumerate(G.DENSE_EXTRUDE_SETS):
        tag = f"dense_ex{i}"
        got = c.extrude(params if len(params) > 1 else params[0])
        assert isinstance(got, ChebyshevApproximation) and got.function is None and got.build_time == 0.0
        assert got.max_derivative_order == c.max_derivative_order and got._device_model is None
        assert np.array_equal(np.asarray(got.domain, dtype=float), g26[f"{tag}_domain"])
        assert list(got.n_nodes) == g26[f"{tag}_n_nodes"].tolist() == list(got.tensor_values.shape)
        assert np.array_equal(got.tensor_values, g26[f"{tag}_tensor"])
        for dim_idx, (lo, hi), n in params:
            x = chebyshev_nodes(lo, hi, n)
            w = compute_barycentric_weights(x)
            assert np.array_equal(got.nodes[dim_idx], x) and np.array_equal(got.weights[dim_idx], w)
            assert np.array_equal(got.diff_matrices[dim_idx], compute_differentiation_matrix(x, w))
            assert np.array_equal(np.take(got.tensor_values, 0, axis=dim_idx), np.take(got.tensor_values, n - 1, axis=dim_idx))
    assert c.num_dimensions == 2 and c.tensor_values.shape == (7, 6)


# ------------------------------------------------------------------ the merge of the pieces
def test_merge_turns_the_reference_piece_roots_into_its_rows(g26):
    seen = set()
    for case, c in G.CASES.items():
        for k in range(c["d"]):
            PR, pc = g26[f"{case}_d{k}_proots"], g26[f"{case}_d{k}_pcount"]
            R, cnt = g26[f"{case}_d{k}_roots"], g26[f"{case}_d{k}_count"]
            assert R.shape[1] == sum(max(n - 1, 1) for n in G.piece_counts(case, k))
            for r in range(R.shape[0]):
                found = [PR[r, j, :pc[r, j]] for j in range(PR.shape[1])]
                got = _calculus.merge_pieces("roots", found, c["domain"][k], counts=pc[r])
                assert got.size == cnt[r] and np.array_equal(got, R[r, :cnt[r]]), (case, k, r)
                assert np.all(np.isnan(R[r, cnt[r]:]))
            seen |= set(cnt.tolist())
    assert {0, 1} <= seen and max(seen) >= 5
    assert np.all(g26["z_d0_count"] == 1) and np.all(g26["z_d0_pcount"] == 1)     # both pieces find 0.2, the merge keeps one
    assert np.all(np.abs(g26["z_d0_roots"][:, 0] - 0.2) <= 1e-10 * 2.0)


def test_merge_rules():
    dom = (0.0, 9.0)                                            # tolerance 1e-10 (9 + 1) = 1e-9
    merge = _calculus.merge_pieces
    # the predecessor is the immediate one, kept or not: 1 + 0.8e-9 is dropped, and 1 + 1.6e-9 is compared with it
    got = merge("roots", [np.array([1.0]), np.array([1.0 + 0.8e-9, 1.0 + 1.6e-9]), np.array([]), np.array([5.0])], dom)
    assert np.array_equal(got, [1.0, 5.0])
    assert np.array_equal(merge("roots", [np.array([1.0]), np.array([1.0 + 2e-9])], dom), [1.0, 1.0 + 2e-9])
    assert merge("roots", [], dom).size == 0 and merge("roots", [np.array([]), np.array([])], dom).size == 0
    assert merge("roots", [np.array([]), np.array([2.0])], dom).tolist() == [2.0]
    # extrema: strictly better replaces, so the first of equal pieces wins; the start is (+-inf, 0.0)
    assert merge("min", [(1.0, 0.1), (0.5, 0.2), (0.5, 0.3), (0.7, 0.4)]) == (0.5, 0.2)
    assert merge("max", [(1.0, 0.1), (1.0, 0.2), (0.7, 0.4)]) == (1.0, 0.1)
    assert merge("min", [(np.inf, 0.3)]) == (np.inf, 0.0) and merge("max", [(-np.inf, 0.3)]) == (-np.inf, 0.0)
    assert merge("min", [(np.nan, 0.3), (2.0, 0.4)]) == (2.0, 0.4)
    assert merge("min", []) == (np.inf, 0.0)
    for mode, found in (("roots", [np.array([1.0]), np.array([])]), ("min", [(1.0, 0.1), (np.nan, np.nan)])):
        with pytest.raises(np.linalg.LinAlgError):
            merge(mode, found, dom, counts=[1, -1])


def test_pieces_of_one_interval_with_different_grids_are_refused_by_the_batch():
    """Pieces that share an index along the dimension but not their node count there (auto-N pieces may): the batch, which
    takes one grid per index, refuses; the other dimension's batch arguments pass."""
    sp = G.build_mixed(ChebyshevSpline, ChebyshevApproximation)
    assert sp._dim_counts(0) is None and sp._dim_counts(1) == [4, 4]
    for fn in (sp.roots_batch, sp.minimize_batch, sp.maximize_batch):
        with pytest.raises(ValueError, match="pieces that share an interval of dimension 0 differ in their node counts"):
            fn(0, np.array([[0.3]]))
    assert sp._calculus_rows(1, np.array([[0.3]])).shape == (1, 1)
