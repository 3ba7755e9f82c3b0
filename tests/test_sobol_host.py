"""ChebyshevTT.sobol_indices(): the coefficient-core contraction on the host (no GPU), against the
reference's values (golden g19) and closed forms."""
import math
import os

import numpy as np
import pytest

from pychebyshev_amd import ChebyshevTT

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def _g(name):
    return np.load(os.path.join(GOLD, name))


def _check(res, gold, tag, d, keys=None):
    keys = list(range(d)) if keys is None else keys
    assert sorted(res["first_order"]) == sorted(keys) and sorted(res["total_order"]) == sorted(keys)
    assert all(type(k) is int for k in res["first_order"])
    first = np.array([res["first_order"][k] for k in range(d)])
    total = np.array([res["total_order"][k] for k in range(d)])
    assert np.max(np.abs(first - gold[f"{tag}_first"])) <= 1e-12
    assert np.max(np.abs(total - gold[f"{tag}_total"])) <= 1e-12
    want = float(gold[f"{tag}_variance"])
    assert isinstance(res["variance"], float)
    assert abs(res["variance"] - want) <= 1e-12 * abs(want)


def _tt(cores, order=None):
    return ChebyshevTT.from_coeff_cores(cores, [[-1.0, 1.0]] * len(cores), dim_order=order)


@pytest.mark.parametrize("tag,src,prefix,d", [
    ("tt_g4r8", "g4_tt_bs5d.npz", "r8_core", 5),
    ("tt_g5", "g5_tt_rank16.npz", "core", 10),
    ("tt_g5b", "g5b_tt_mixed.npz", "core", 4),
])
def test_tt_sobol_matches_reference(tag, src, prefix, d):
    g = _g(src)
    res = _tt([g[f"{prefix}{k}"] for k in range(d)]).sobol_indices()
    _check(res, _g("g19_sobol.npz"), tag, d)


def test_tt_sobol_keys_are_user_dimensions_under_a_dim_order():
    g5 = _g("g5_tt_rank16.npz")
    cores = [g5[f"core{k}"] for k in range(10)]
    perm = [int(v) for v in g5["perm"]]
    res = _tt(cores, perm).sobol_indices()
    _check(res, _g("g19_sobol.npz"), "tt_g5perm", 10)
    plain = _tt(cores).sobol_indices()
    for s, user in enumerate(perm):          # storage position s holds user dimension perm[s]
        assert res["first_order"][user] == plain["first_order"][s]
        assert res["total_order"][user] == plain["total_order"][s]
    assert res["variance"] == plain["variance"]


def test_tt_sobol_rank_one_separable_closed_form():
    # f = prod_k (a_k + b_k T_1(x_k)): under the Chebyshev measure the factor k has mean part a_k^2 pi and
    # fluctuating part b_k^2 pi / 2, so V = prod(pi a^2 + pi b^2 / 2) - prod(pi a^2),
    # S_k = (pi b_k^2 / 2) prod_{j != k} pi a_j^2 / V and T_k = (pi b_k^2 / 2) prod_{j != k} (pi a_j^2 + pi b_j^2 / 2) / V
    a = np.array([1.0, 0.5, 2.0])
    b = np.array([0.3, 1.0, 0.7])
    cores = []
    for ak, bk in zip(a, b):
        c = np.zeros((1, 4, 1))
        c[0, 0, 0], c[0, 1, 0] = ak, bk
        cores.append(c)
    res = _tt(cores).sobol_indices()
    mean = math.pi * a ** 2
    fluc = math.pi * b ** 2 / 2
    V = np.prod(mean + fluc) - np.prod(mean)
    assert abs(res["variance"] - V) <= 1e-13 * V
    for k in range(3):
        others = [j for j in range(3) if j != k]
        assert abs(res["first_order"][k] - fluc[k] * np.prod(mean[others]) / V) <= 1e-13
        assert abs(res["total_order"][k] - fluc[k] * np.prod((mean + fluc)[others]) / V) <= 1e-13


def test_tt_sobol_of_a_constant_is_zero():
    cores = [np.zeros((1, 3, 1)) for _ in range(3)]
    for c in cores:
        c[0, 0, 0] = 1.5
    res = _tt(cores).sobol_indices()
    assert res == {"first_order": {0: 0.0, 1: 0.0, 2: 0.0}, "total_order": {0: 0.0, 1: 0.0, 2: 0.0}, "variance": 0.0}


def test_tt_sobol_unbuilt_raises():
    tt = ChebyshevTT(lambda x, _: 0.0, 2, [[-1.0, 1.0]] * 2, [4, 4])
    with pytest.raises(RuntimeError, match="build"):
        tt.sobol_indices()


def test_unbuilt_dense_and_spline_raise_without_a_gpu():
    from pychebyshev_amd import ChebyshevApproximation, ChebyshevSpline
    ap = ChebyshevApproximation(None, 2, [[-1.0, 1.0]] * 2, [4, 5], defer_build=True)
    with pytest.raises(RuntimeError, match="build"):
        ap.sobol_indices()
    sp = ChebyshevSpline(None, 1, [[-1.0, 1.0]], n_nodes=[5], knots=[[0.0]], defer_build=True)
    with pytest.raises(RuntimeError, match="build"):
        sp.sobol_indices()


def test_slider_has_no_sobol_indices():
    # the reference's ChebyshevSlider has none either
    from pychebyshev_amd import ChebyshevSlider
    assert not hasattr(ChebyshevSlider, "sobol_indices")
