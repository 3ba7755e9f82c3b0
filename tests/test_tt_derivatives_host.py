"""ChebyshevTT.differentiate against the long-double chain of g28_tt_derivatives.npz (written by
tests/golden/generate_golden_tt_derivatives.py), what it keeps of the model, and the argument validation of
differentiate and of the ``method`` keyword of eval_multi / eval_multi_batch.  Host NumPy only: no GPU."""
import pickle

import numpy as np
import pytest

from conftest import assert_parity, golden, spec_point_tol
from pychebyshev_amd import ChebyshevTT, _lib

G22 = golden("g22_tt_transforms")
G = golden("g28_tt_derivatives")
MODELS = ("A", "B", "C", "C2", "D", "E", "F")


def cores_of(tag):
    out, k = [], 0
    while f"{tag}_core{k}" in G22.files:
        out.append(G22[f"{tag}_core{k}"])
        k += 1
    return out


def model(tag):
    return ChebyshevTT.from_coeff_cores(cores_of(tag), G22[f"{tag}_domain"].tolist(), dim_order=G22[f"{tag}_order"].tolist())


GROUPS = [f"{tag}_s{i}" for tag in MODELS for i in range(int(G[f"{tag}_nspec"]))]


def value_chain(tt, pts):
    """The plain evaluation chain of a model in float64 NumPy: T_j by the forward recurrence, points in the user frame."""
    v = np.ones((pts.shape[0], 1))
    for k, core in enumerate(tt._coeff_cores):
        a, b = tt.domain[k]
        s = (pts[:, tt._dim_order[k]] - a) * (2.0 / (b - a)) - 1.0
        n = core.shape[1]
        T = np.ones((n, s.size))
        if n > 1:
            T[1] = s
        for j in range(2, n):
            T[j] = 2.0 * s * T[j - 1] - T[j - 2]
        v = np.einsum("na,nab->nb", v, np.einsum("jn,ajb->nab", T, core))
    return v[:, 0]


def test_the_golden_file_holds_every_kind_of_spec():
    assert len(GROUPS) == 3 + 8 + 13 + 13 + 12 + 12 + 10
    for tag in MODELS:
        d = len(cores_of(tag))
        specs = [G[f"{tag}_s{i}_spec"].tolist() for i in range(int(G[f"{tag}_nspec"]))]
        assert [0] * d in specs
        for u in range(d):
            for o in (1, 2):
                assert [o if v == u else 0 for v in range(d)] in specs
        if d >= 2:
            assert [1] + [0] * (d - 2) + [1] in specs and [2, 1] + [0] * (d - 2) in specs
        if d <= 4:
            assert [2] * d in specs
    for g in GROUPS:
        tag = g.split("_")[0]
        dom = model(tag)._user_frame_domain()
        pts = G[f"{g}_pts"]
        assert pts.shape == (48, len(dom))
        assert np.array_equal(pts[0], [a for a, _ in dom]) and np.array_equal(pts[1], [b for _, b in dom])
        assert (f"{g}_ref" in G.files) == (sum(G[f"{g}_spec"]) <= 2 and bool(np.any(G[f"{g}_ld"] != 0)))


@pytest.mark.parametrize("g", GROUPS)
def test_differentiated_cores_match_the_long_double_chain(g):
    tt = model(g.split("_")[0])
    spec = G[f"{g}_spec"].tolist()
    ld = G[f"{g}_ld"]
    got = value_chain(tt.differentiate(spec), G[f"{g}_pts"])
    if not np.any(ld):                              # an order reaches the node count: the zero model
        assert np.all(got == 0.0)
        return
    assert_parity(got, ld, tol=1e-12, point_tol=spec_point_tol(spec), what=f"differentiate {g} {spec}")


@pytest.mark.parametrize("tag", MODELS)
def test_order_zero_returns_equal_cores(tag):
    tt = model(tag)
    res = tt.differentiate([0] * tt.num_dimensions)
    assert res is not tt and len(res._coeff_cores) == tt.num_dimensions
    for mine, theirs in zip(res._coeff_cores, tt._coeff_cores):
        assert mine is not theirs and np.array_equal(mine, theirs)


def test_shape_domain_and_dim_order_are_kept():
    tt = model("D")
    tt.error_estimate()
    assert tt._cached_error_estimate is not None
    res = tt.differentiate([1, 0, 2, 3])
    assert res.function is None and res._cached_error_estimate is None
    assert res.dim_order == tt.dim_order == [3, 1, 0, 2]
    assert res.domain == tt.domain and res.n_nodes == tt.n_nodes and res.tt_ranks == tt.tt_ranks
    assert [c.shape for c in res._coeff_cores] == [c.shape for c in tt._coeff_cores]
    # storage position k holds user dimension dim_order[k]: order p zeroes the top p coefficients of that core
    for pos, p in enumerate([3, 0, 1, 2]):
        core = res._coeff_cores[pos]
        assert np.all(core[:, core.shape[1] - p:, :] == 0.0) if p else np.array_equal(core, tt._coeff_cores[pos])
    assert tt._cached_error_estimate is not None                 # the source model is untouched


def test_orders_compose_and_high_orders_vanish():
    tt = model("D")
    twice = tt.differentiate([1, 0, 0, 0]).differentiate([1, 0, 1, 0])
    once = tt.differentiate([2, 0, 1, 0])
    for a, b in zip(twice._coeff_cores, once._coeff_cores):
        assert np.allclose(a, b, rtol=1e-13, atol=1e-13 * np.max(np.abs(b)))
    gone = model("B").differentiate([0, 2])                      # user dimension 1 is stored first, with 2 nodes
    assert np.all(gone._coeff_cores[0] == 0.0) and np.array_equal(gone._coeff_cores[1], model("B")._coeff_cores[1])
    assert np.all(model("C").differentiate([0, 0, 11, 0, 0])._coeff_cores[2] == 0.0)


def test_the_result_pickles():
    res = model("C2").differentiate([0, 1, 0, 0, 2])
    back = pickle.loads(pickle.dumps(res))
    assert back.dim_order == res.dim_order and back.domain == res.domain and back.function is None
    for a, b in zip(back._coeff_cores, res._coeff_cores):
        assert np.array_equal(a, b)


def test_differentiate_validation():
    tt = model("C")
    with pytest.raises(ValueError, match="derivative_order needs 5 orders, got 4"):
        tt.differentiate([1, 0, 0, 0])
    with pytest.raises(ValueError, match=r"Derivative order -1 not supported \(use an integer >= 0\)"):
        tt.differentiate([0, -1, 0, 0, 0])
    with pytest.raises(ValueError, match=r"Derivative order 1.5 not supported \(use an integer >= 0\)"):
        tt.differentiate([0, 0, 1.5, 0, 0])
    with pytest.raises(RuntimeError, match="build"):
        ChebyshevTT(lambda p, _: 0.0, 2, [[0, 1], [0, 1]], [4, 4]).differentiate([1, 0])


def test_method_keyword_validation():
    tt = model("C")
    pts = G["C_s0_pts"]
    for bad in ("exact", "FD", None):
        with pytest.raises(ValueError, match="method must be 'fd' or 'analytic'"):
            tt.eval_multi_batch(pts, [[1, 0, 0, 0, 0]], method=bad)
        with pytest.raises(ValueError, match="method must be 'fd' or 'analytic'"):
            tt.eval_multi(pts[0], [[1, 0, 0, 0, 0]], method=bad)
    # orders and lengths are validated as on the finite-difference path, before anything reaches the device
    with pytest.raises(ValueError, match=r"Derivative order 3 not supported \(use 1 or 2\)"):
        tt.eval_multi_batch(pts, [[0, 3, 0, 0, 0]], method="analytic")
    with pytest.raises(ValueError, match="each derivative spec needs 5 orders, got 4"):
        tt.eval_multi_batch(pts, [[1, 0, 0, 0]], method="analytic")
    with pytest.raises(ValueError, match=r"Derivative order 3 not supported \(use 1 or 2\)"):
        tt.eval_multi(pts[0], [[0, 3, 0, 0, 0]], method="analytic")
    assert tt.eval_multi_batch(pts, [], method="analytic").shape == (48, 0)


def test_the_library_exports_the_entry_points():
    lib = _lib.load()
    assert lib.pcx_tt_deriv_batch is not None and lib.pcx_tt_deriv_batch_dev is not None
