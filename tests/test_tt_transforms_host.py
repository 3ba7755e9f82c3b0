"""ChebyshevTT.slice / extrude / integrate / inner_product against the reference's results (g22_tt_transforms.npz,
written by tests/golden/generate_golden_tt_transforms.py), their exceptions, and the argument validation of
integrate_batch.  Host NumPy only: no GPU."""
import pickle
import re

import numpy as np
import pytest

from conftest import golden
from pychebyshev_amd import ChebyshevTT

G = golden("g22_tt_transforms")
TRANSFORM_MODELS = ("A", "B", "C", "D")
IP_MODELS = ("B", "C", "D")


def cores_of(prefix):
    out, k = [], 0
    while f"{prefix}_core{k}" in G.files:
        out.append(G[f"{prefix}_core{k}"])
        k += 1
    return out


def model(tag):
    return ChebyshevTT.from_coeff_cores(cores_of(tag), G[f"{tag}_domain"].tolist(), dim_order=G[f"{tag}_order"].tolist())


def cases(op):
    found = []
    for name in G.files:
        hit = re.fullmatch(rf"([A-Z]\d?)_{op}(\d+)_params", name)
        if hit and hit.group(1) in TRANSFORM_MODELS:
            found.append((hit.group(1), int(hit.group(2))))
    return sorted(found)


def apply(tt, op, params, single):
    if op == "slice":
        args = [(int(p[0]), float(p[1])) for p in params]
        return tt.slice(args[0] if single else args)
    if op == "extrude":
        args = [(int(p[0]), (float(p[1]), float(p[2])), int(p[3])) for p in params]
        return tt.extrude(args[0] if single else args)
    dims = [int(p[0]) for p in params]
    if all(np.isnan(p[1]) for p in params):
        bounds = None
    else:
        bounds = [None if np.isnan(p[1]) else (float(p[1]), float(p[2])) for p in params]
    return tt.integrate(dims[0] if single else dims, bounds=bounds)


ALL_CASES = [(op, tag, i) for op in ("slice", "extrude", "integ") for tag, i in cases(op)]


def test_the_golden_file_holds_every_kind_of_case():
    ops = {op for op, _, _ in ALL_CASES}
    assert ops == {"slice", "extrude", "integ"}
    assert {tag for _, tag, _ in ALL_CASES} == set(TRANSFORM_MODELS)
    assert any(int(G[f"{tag}_{op}{i}_single"]) for op, tag, i in ALL_CASES)


@pytest.mark.parametrize("op,tag,i", ALL_CASES, ids=[f"{t}-{o}{i}" for o, t, i in ALL_CASES])
def test_result_matches_the_reference(op, tag, i):
    prefix = f"{tag}_{op}{i}"
    res = apply(model(tag), op, G[f"{prefix}_params"], bool(int(G[f"{prefix}_single"])))
    want = cores_of(prefix)
    assert isinstance(res, ChebyshevTT)
    assert res.num_dimensions == len(want)
    assert res.dim_order == G[f"{prefix}_order"].tolist()
    assert list(res.n_nodes) == G[f"{prefix}_n"].tolist()
    np.testing.assert_allclose(np.asarray(res.domain, dtype=float), G[f"{prefix}_domain"], rtol=0, atol=0)
    assert res.tt_ranks == [1] + [c.shape[2] for c in want]
    for k, (got, ref) in enumerate(zip(res._coeff_cores, want)):
        assert got.shape == ref.shape
        scale = float(np.max(np.abs(ref)))
        assert np.max(np.abs(got - ref)) <= 1e-13 * scale, f"{prefix} core {k}"


def test_results_carry_the_source_settings():
    tt = model("D")
    tt.max_rank, tt.tolerance, tt.max_sweeps, tt.max_derivative_order = 23, 3e-9, 7, 1
    tt.descriptor, tt.additional_data, tt.method = "desk model", {"k": 1}, "svd"
    for res in (tt.slice((0, -1.1)), tt.extrude((1, (0.0, 1.0), 3)), tt.integrate([2])):
        assert (res.max_rank, res.tolerance, res.max_sweeps, res.max_derivative_order) == (23, 3e-9, 7, 1)
        assert (res.descriptor, res.additional_data, res.method) == ("desk model", {"k": 1}, "svd")
        assert res.function is None and res.is_construction_finished()


@pytest.mark.parametrize("tag", ["A", "B", "C", "C2", "D", "E", "F"])
def test_scalar_integrate(tag):
    tt = model(tag)
    full = tt.integrate()
    assert isinstance(full, float)
    assert abs(full - float(G[f"{tag}_int_full"])) <= 1e-13 * abs(float(G[f"{tag}_int_full"]))
    sub = tt.integrate(None, bounds=[tuple(r) for r in G[f"{tag}_int_sub_bounds"].tolist()])
    assert abs(sub - float(G[f"{tag}_int_sub"])) <= 1e-13 * abs(float(G[f"{tag}_int_sub"]))
    # all dimensions named one by one is the same number
    assert tt.integrate(list(range(tt.num_dimensions))) == full


@pytest.mark.parametrize("tag", IP_MODELS)
def test_inner_product(tag):
    tt = model(tag)
    other = ChebyshevTT.from_coeff_cores(cores_of(f"{tag}_other"), G[f"{tag}_domain"].tolist(),
                                         dim_order=G[f"{tag}_order"].tolist())
    total = ChebyshevTT.from_coeff_cores(cores_of(f"{tag}_sum"), G[f"{tag}_domain"].tolist(),
                                         dim_order=G[f"{tag}_order"].tolist())
    for got, key in ((tt.inner_product(tt), "ip_self"), (tt.inner_product(other), "ip_other"),
                     (total.inner_product(tt), "ip_sum")):
        ref = float(G[f"{tag}_{key}"])
        assert isinstance(got, float)
        assert abs(got - ref) <= 1e-13 * abs(ref), key
    assert other.inner_product(tt) == pytest.approx(tt.inner_product(other), rel=1e-14)


def test_inner_product_errors():
    tt = model("D")
    with pytest.raises(ValueError, match="other must be a ChebyshevTT, got int"):
        tt.inner_product(3)
    wide = ChebyshevTT.from_coeff_cores(cores_of("D"), [[0.0, 9.0]] * 4, dim_order=G["D_order"].tolist())
    with pytest.raises(ValueError, match="requires matching domains"):
        tt.inner_product(wide)
    padded = cores_of("D")
    padded[0] = np.concatenate([padded[0], np.zeros((1, 1, 12))], axis=1)          # 8 coefficients where tt has 7
    with pytest.raises(ValueError, match="requires matching n_nodes"):
        tt.inner_product(ChebyshevTT.from_coeff_cores(padded, G["D_domain"].tolist(), dim_order=G["D_order"].tolist()))
    plain = ChebyshevTT.from_coeff_cores(cores_of("D"), G["D_domain"].tolist())
    with pytest.raises(ValueError, match="requires matching _dim_order"):
        tt.inner_product(plain)
    unbuilt = ChebyshevTT(None, 4, G["D_domain"].tolist(), [7, 16, 5, 9])
    with pytest.raises(RuntimeError, match="build"):
        tt.inner_product(unbuilt)


def test_slice_errors():
    tt = model("D")                    # user domains: dim 0 = [-2, -0.25], 1 = [0.5, 3], 2 = [10, 14], 3 = [-1, 1]
    with pytest.raises(ValueError, match=r"Cannot slice all 4 dimensions \(would produce 0D result\)"):
        tt.slice([(0, -1.0), (1, 1.0), (2, 11.0), (3, 0.0)])
    with pytest.raises(ValueError, match="Duplicate dim_index 1"):
        tt.slice([(1, 1.0), (1, 2.0)])
    with pytest.raises(ValueError, match=r"dim_index 4 out of range \[0, 3\]"):
        tt.slice((4, 0.0))
    with pytest.raises(ValueError, match=r"dim_index -1 out of range \[0, 3\]"):
        tt.slice((-1, 0.0))
    with pytest.raises(TypeError, match="dim_index must be int, got float"):
        tt.slice([(1.0, 0.0)])
    with pytest.raises(ValueError, match=r"Slice value 9.5 for dim 2 is outside domain \[10.0, 14.0\]"):
        tt.slice((2, 9.5))
    with pytest.raises(ValueError, match=r"Slice value 1.5 for dim 3 is outside domain \[-1.0, 1.0\]"):
        tt.slice([(0, -1.0), (3, 1.5)])


def test_slice_exactly_at_a_node_picks_the_value():
    from pychebyshev_amd.barycentric import chebyshev_nodes
    from pychebyshev_amd.tensor_train import _coeff_core_to_value_core
    tt = model("C")
    nodes = chebyshev_nodes(*tt.domain[2], tt.n_nodes[2])
    res = tt.slice((2, float(nodes[4])))
    picked = _coeff_core_to_value_core(tt._coeff_cores[2])[:, 4, :]
    np.testing.assert_array_equal(res._coeff_cores[2], np.einsum("lr,rjs->ljs", picked, tt._coeff_cores[3]))
    near = tt.slice((2, float(nodes[4]) + 1e-9))           # off the node: the barycentric weights, nearly the same cores
    assert np.max(np.abs(near._coeff_cores[2] - res._coeff_cores[2])) < 1e-6
    assert not np.array_equal(near._coeff_cores[2], res._coeff_cores[2])


def test_value_core_is_the_inverse_of_the_coefficient_transform():
    from numpy.polynomial import chebyshev as C
    from pychebyshev_amd.tensor_train import _coeff_core_to_value_core
    rng = np.random.default_rng(5)
    core = rng.standard_normal((3, 9, 2))
    vals = _coeff_core_to_value_core(core)
    x = np.sort(C.chebpts1(9))
    for a in range(3):
        for b in range(2):
            np.testing.assert_allclose(vals[a, :, b], C.chebval(x, core[a, :, b]), rtol=0, atol=1e-14)


def test_extrude_errors_and_core():
    tt = model("B")
    with pytest.raises(ValueError, match=r"dim_index 3 out of range \[0, 2\]"):
        tt.extrude((3, (0.0, 1.0), 4))
    with pytest.raises(ValueError, match="Duplicate dim_index 0"):
        tt.extrude([(0, (0.0, 1.0), 4), (0, (0.0, 1.0), 4)])
    with pytest.raises(ValueError, match=r"Domain bounds must satisfy lo < hi, got \[1.0, 1.0\]"):
        tt.extrude((0, (1.0, 1.0), 4))
    with pytest.raises(ValueError, match="n_nodes must be int >= 2, got 1"):
        tt.extrude((0, (0.0, 1.0), 1))
    with pytest.raises(TypeError, match="dim_index must be int, got str"):
        tt.extrude([("0", (0.0, 1.0), 4)])
    # identity order: the core goes to its storage position, keeps the rank and holds c_0 = 1 only
    ident = model("C").extrude((2, (0.0, 1.0), 4))
    core = ident._coeff_cores[2]
    assert core.shape == (8, 4, 8) and ident.dim_order == list(range(6))
    np.testing.assert_array_equal(core[:, 0, :], np.eye(8))
    assert not core[:, 1:, :].any()
    # a storage order: appended at the storage end, placed by dim_order
    moved = tt.extrude((1, (0.0, 1.0), 4))
    assert moved._coeff_cores[-1].shape == (1, 4, 1) and moved.dim_order == [2, 0, 1]


def test_integrate_errors():
    tt = model("D")
    with pytest.raises(ValueError, match=r"dims contains out-of-range index \(num_dimensions=4, dims=\[1, 4\]\)"):
        tt.integrate([4, 1])
    with pytest.raises(ValueError, match="bounds length 1 != dims length 2"):
        tt.integrate([0, 1], bounds=[(0.0, 1.0)])
    with pytest.raises(ValueError, match="bounds lo=0.5 > hi=0.0 for dim 3"):
        tt.integrate(3, bounds=(0.5, 0.0))
    with pytest.raises(ValueError, match=r"bounds \(9.0, 12.0\) outside domain \[10.0, 14.0\] for dim 2"):
        tt.integrate([2], bounds=[(9.0, 12.0)])


def test_pickle_round_trip_of_a_result():
    tt = model("D")
    for res in (tt.slice((1, 1.25)), tt.extrude((4, (0.0, 1.0), 3)), tt.integrate([0, 3])):
        back = pickle.loads(pickle.dumps(res))
        assert back.dim_order == res.dim_order and back.n_nodes == res.n_nodes and back.domain == res.domain
        for a, b in zip(back._coeff_cores, res._coeff_cores):
            np.testing.assert_array_equal(a, b)
        assert back.integrate() == res.integrate()


def test_methods_need_a_built_model():
    tt = ChebyshevTT(None, 2, [[0.0, 1.0]] * 2, [4, 4])
    for call in (lambda: tt.slice((0, 0.5)), lambda: tt.extrude((0, (0.0, 1.0), 3)), lambda: tt.integrate(),
                 lambda: tt.inner_product(tt), lambda: tt.integrate_batch([0], points=[[0.5]])):
        with pytest.raises(RuntimeError, match="build"):
            call()


def test_build_method_als_still_raises():
    tt = ChebyshevTT(lambda x, _: x[0], 2, [[0.0, 1.0]] * 2, [4, 4])
    with pytest.raises(NotImplementedError):
        tt.build(verbose=False, method="als")


# ------------------------------------------------------------------------------------------------ integrate_batch arguments
def test_integrate_batch_rows_follow_the_user_dimensions():
    tt = model("D")                    # user domains: dim 0 = [-2, -0.25], 1 = [0.5, 3], 2 = [10, 14], 3 = [-1, 1]
    bounds = np.array([[[-1.5, -1.0], [11.0, 12.0]], [[-2.0, -0.25], [10.0, 10.0]]])
    points = np.array([[1.0, 0.5], [3.0, -1.0]])
    flags, rows = tt._box_rows([2, 0], bounds, points)
    assert flags.tolist() == [1, 0, 1, 0] and flags.dtype == np.int32
    assert rows.shape == (2, 6)        # d + m
    np.testing.assert_array_equal(rows, [[-1.5, -1.0, 1.0, 11.0, 12.0, 0.5], [-2.0, -0.25, 3.0, 10.0, 10.0, -1.0]])
    # one (m, 2) block, one (2,) pair and None serve every row
    _, rows = tt._box_rows([0, 2], [(-1.5, -1.0), (11.0, 12.0)], points)
    np.testing.assert_array_equal(rows[:, [0, 1, 3, 4]], [[-1.5, -1.0, 11.0, 12.0]] * 2)
    _, rows = tt._box_rows(3, (-0.5, 0.5), np.zeros((3, 3)) + [-1.0, 1.0, 11.0])
    assert rows.shape == (3, 5)
    np.testing.assert_array_equal(rows[:, 3:], [[-0.5, 0.5]] * 3)
    _, rows = tt._box_rows([0, 1, 2, 3], None, None)
    np.testing.assert_array_equal(rows, [[-2.0, -0.25, 0.5, 3.0, 10.0, 14.0, -1.0, 1.0]])
    # an overshoot of the domain within 1e-14 is clipped, as integrate() does
    _, rows = tt._box_rows(3, (-1.0 - 5e-15, 1.0), np.zeros((1, 3)) + [-1.0, 1.0, 11.0])
    assert rows[0, 3] == -1.0


def test_integrate_batch_argument_errors():
    tt = model("D")
    pts2 = np.array([[1.0, 0.5], [3.0, -1.0]])
    ok = np.array([[[-1.5, -1.0], [11.0, 12.0]]] * 2)
    with pytest.raises(ValueError, match=r"dims contains out-of-range index \(num_dimensions=4, dims=\[0, 4\]\)"):
        tt.integrate_batch([0, 4], ok, pts2)
    with pytest.raises(ValueError, match="at least one dimension"):
        tt.integrate_batch([], None, np.zeros((1, 4)))
    with pytest.raises(ValueError, match=r"bounds must broadcast to \(N, 2, 2\), got shape \(2, 3, 2\)"):
        tt.integrate_batch([0, 2], np.zeros((2, 3, 2)), pts2)
    with pytest.raises(ValueError, match=r"bounds must broadcast to \(N, 2, 2\)"):
        tt.integrate_batch([0, 2], (-1.5, -1.0), pts2)
    with pytest.raises(ValueError, match=r"points must have shape \(N, 2\), got \(2, 3\)"):
        tt.integrate_batch([0, 2], ok, np.zeros((2, 3)))
    with pytest.raises(ValueError, match="points is required: 2 dimensions are kept"):
        tt.integrate_batch([0, 2], ok)
    with pytest.raises(ValueError, match="bounds has 2 rows but points has 3"):
        tt.integrate_batch([0, 2], ok, np.array([[1.0, 0.5]] * 3))
    bad = ok.copy()
    bad[1, 1] = (12.0, 11.0)
    with pytest.raises(ValueError, match=r"bounds lo=12.0 > hi=11.0 for dim 2 \(row 1\)"):
        tt.integrate_batch([0, 2], bad, pts2)
    bad = ok.copy()
    bad[1, 0] = (-2.5, -1.0)
    with pytest.raises(ValueError, match=r"bounds \(-2.5, -1.0\) outside domain \[-2.0, -0.25\] for dim 0 \(row 1\)"):
        tt.integrate_batch([0, 2], bad, pts2)
    off = pts2.copy()
    off[1, 1] = 1.5
    with pytest.raises(ValueError, match=r"point value 1.5 for dim 3 is outside domain \[-1.0, 1.0\] \(row 1\)"):
        tt.integrate_batch([0, 2], ok, off)
    many = np.tile(ok[:1], (5, 1, 1))
    many[3, 0, 1] = 0.0                                 # rows 3 and 4 are both wrong: the first one is named
    many[4, 1, 0] = 9.0
    with pytest.raises(ValueError, match=r"outside domain \[-2.0, -0.25\] for dim 0 \(row 3\)"):
        tt.integrate_batch([0, 2], many, np.tile(pts2[:1], (5, 1)))
