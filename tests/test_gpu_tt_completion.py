"""ChebyshevTT.run_completion / orth_left / orth_right on the device (pcx_tt_als, pcx_tt_orth) against the reference's
golden vectors (tests/golden/g23_tt_completion.npz), an independent NumPy ALS in projection form, an exactly
representable target, and LAPACK's orthogonality on the same unfoldings."""
import numpy as np
import pytest
from numpy.polynomial.chebyshev import chebpts1

from als_steps import dense as _dense, lapack_sweep as _lapack_sweep, numpy_als as _numpy_als
from conftest import assert_parity, golden

from pychebyshev_amd import ChebyshevTT

pytestmark = pytest.mark.gpu

MODELS = ("M1", "M2", "M3", "M4", "M16", "M5")
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def g23():
    return golden("g23_tt_completion")


def _start(g, tag):
    d = len(g[f"{tag}_n"])
    cores = [g[f"{tag}_start_core{k}"] for k in range(d)]
    return ChebyshevTT.from_coeff_cores(cores, g[f"{tag}_domain"].tolist(), dim_order=[int(v) for v in g[f"{tag}_order"]])


def _target(g, tag):
    """The stored target; M5's is not stored (file size) and comes from the generator's closed form again."""
    if f"{tag}_T" in g.files:
        return g[f"{tag}_T"]
    import generate_golden_tt_completion as gen
    return gen.target_tensor(g[f"{tag}_domain"].tolist(), [int(v) for v in g[f"{tag}_n"]])


def _lookup(T, domain):
    """A callback that returns the stored grid values exactly: the node's index by searchsorted on each grid."""
    grids = [np.sort(0.5 * (a + b) + 0.5 * (b - a) * chebpts1(n)) for (a, b), n in zip(domain, T.shape)]

    def f(point, _data):
        return float(T[tuple(min(int(np.searchsorted(g, x)), len(g) - 1) for g, x in zip(grids, point))])
    return f


def _check_history(info, want, m):
    assert info["iterations"] == m and len(info["rel_change"]) == m
    for got, ref in zip(info["rel_change"], want[:m]):
        if ref >= 1e-6:
            assert abs(got - ref) <= 1e-8 * ref, (info["rel_change"], want)


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("tag", MODELS)
def test_golden_parity_both_entry_points(g23, tag, m):
    T = _target(g23, tag)
    by_values = _start(g23, tag)
    by_values.run_completion(tolerance=0.0, max_iter=m, values=T)
    by_callback = _start(g23, tag)
    by_callback.function = _lookup(T, by_callback.domain)
    by_callback.run_completion(tolerance=0.0, max_iter=m)
    for a, b in zip(by_values._coeff_cores, by_callback._coeff_cores):
        assert np.array_equal(a, b), "the two entry points differ"
    assert by_values.completion_info == by_callback.completion_info
    print(f"{tag} m={m}: ranks {by_values.tt_ranks} info {by_values.completion_info}")
    assert_parity(by_values.to_dense(), g23[f"{tag}_dense_m{m}"], tol=1e-12, what=f"{tag} to_dense m={m}")
    assert_parity(by_values.eval_batch(g23[f"{tag}_pts"]), g23[f"{tag}_eval_m{m}"], tol=1e-12, what=f"{tag} eval m={m}")
    _check_history(by_values.completion_info, g23[f"{tag}_rel_change"], m)
    assert by_values.tt_ranks == [1] + [c.shape[2] for c in by_values._coeff_cores]
    if tag == "M3":
        assert by_values.tt_ranks == [1, 6, 7, 1]
    resid = np.linalg.norm(by_values.to_dense() - T) / np.linalg.norm(T)
    assert abs(by_values.completion_info["grid_residual"] - resid) <= 1e-10 + 1e-6 * resid


@pytest.mark.parametrize("m", [1, 3])
def test_golden_parity_behind_a_storage_order(g23, m):
    tt = _start(g23, "M4o")
    assert tt.dim_order == [2, 0, 3, 1] and tt.function is None
    tt.run_completion(tolerance=0.0, max_iter=m, values=g23["M4o_T"])
    assert_parity(tt.to_dense(), g23[f"M4o_dense_m{m}"], tol=1e-12, what=f"M4o to_dense m={m}")
    assert_parity(tt.eval_batch(g23["M4o_pts"]), g23[f"M4o_eval_m{m}"], tol=1e-12, what=f"M4o eval m={m}")
    _check_history(tt.completion_info, g23["M4o_rel_change"], m)


def test_tolerance_stops_at_the_stored_iteration(g23, capsys):
    tt = _start(g23, "M4")
    tt.run_completion(tolerance=float(g23["M4_tol"]), max_iter=50, verbose=True, values=g23["M4_T"])
    iters = int(g23["M4_tol_iters"])
    assert tt.completion_info["iterations"] == iters
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("  ALS iter ")]
    assert len(lines) == iters and lines[0].startswith("  ALS iter 1: rel_change = ")
    assert_parity(tt.to_dense(), g23["M4_tol_dense"], tol=1e-12, what="M4 tolerance-stopped run")


def test_max_iter_zero_runs_no_sweep(g23):
    tt = _start(g23, "M4")
    before = tt.to_dense()
    tt.run_completion(max_iter=0, values=g23["M4_T"])
    assert tt.completion_info["iterations"] == 0 and tt.completion_info["rel_change"] == []
    assert_parity(tt.to_dense(), before, tol=1e-12, what="max_iter=0")
    resid = np.linalg.norm(before - g23["M4_T"]) / np.linalg.norm(g23["M4_T"])
    assert abs(tt.completion_info["grid_residual"] - resid) <= 1e-10


# ------------------------------------------------------------------ independent of the reference
def _smooth_target(n, domain):
    grids = [np.sort(0.5 * (a + b) + 0.5 * (b - a) * chebpts1(nk)) for (a, b), nk in zip(domain, n)]
    mesh = np.meshgrid(*grids, indexing="ij")
    q = 1.0 + sum(c * x * x for c, x in zip([0.9, 0.35, 0.6, 1.1], mesh))
    s = sum(c * x for c, x in zip([1.3, 0.7, -0.9, 1.7], mesh))
    return 1.5 + 1.0 / q + 0.25 * np.sin(s)


def test_against_numpy_projection_als():
    from pychebyshev_amd.tensor_train import _coeff_core_to_value_core
    n, ranks = (12, 11, 13, 10), [1, 5, 5, 5, 1]
    domain = [[-1.0, 1.0], [0.5, 3.0], [-2.0, -0.25], [0.0, 1.0]]
    T = _smooth_target(n, domain)
    rng = np.random.default_rng(41)
    start = [rng.standard_normal((ranks[k], n[k], ranks[k + 1])) * 0.6 ** np.arange(n[k])[None, :, None] for k in range(4)]
    tt = ChebyshevTT.from_coeff_cores(start, domain)
    want = _dense(_numpy_als([_coeff_core_to_value_core(c) for c in start], T, 3))
    tt.run_completion(tolerance=0.0, max_iter=3, values=T)
    print("numpy ALS:", tt.completion_info, "max|got - want| / max|want| =",
          np.max(np.abs(tt.to_dense() - want)) / np.max(np.abs(want)))
    assert_parity(tt.to_dense(), want, tol=1e-12, what="(12,11,13,10) rank 5 vs NumPy projection ALS")


def test_exact_low_rank_target_is_recovered_in_one_iteration():
    rng = np.random.default_rng(77)
    n, ranks = [16] * 5, [1, 6, 6, 6, 6, 1]
    T = _dense([rng.standard_normal((ranks[k], n[k], ranks[k + 1])) for k in range(5)])
    start = [rng.standard_normal((ranks[k], n[k], ranks[k + 1])) for k in range(5)]
    tt = ChebyshevTT.from_coeff_cores(start, [[-1.0, 1.0]] * 5)
    tt.run_completion(max_iter=1, values=T)
    print("exact rank-6 target:", tt.completion_info)
    assert tt.completion_info["iterations"] == 1
    assert tt.completion_info["grid_residual"] <= 1e-12


def test_two_identical_calls_give_equal_bits(g23):
    runs = []
    for _ in range(2):
        tt = _start(g23, "M16")
        tt.run_completion(tolerance=0.0, max_iter=2, values=g23["M16_T"])
        runs.append(tt)
    for a, b in zip(runs[0]._coeff_cores, runs[1]._coeff_cores):
        assert np.array_equal(a, b)
    assert runs[0].completion_info == runs[1].completion_info


# ------------------------------------------------------------------ orthogonalisation
def _rank_deficient_cores():
    rng = np.random.default_rng(9)
    n, ranks = [5, 6, 4, 7], [1, 4, 5, 4, 1]
    cores = [rng.standard_normal((ranks[k], n[k], ranks[k + 1])) for k in range(4)]
    cores[0][:, :, 3] = cores[0][:, :, 1]            # duplicated columns of the left unfoldings
    cores[1][:, :, 4] = cores[1][:, :, 0]
    cores[2][2] = cores[2][0]                        # duplicated rows of the right unfoldings
    cores[3][3] = cores[3][1]
    return cores, [[-1.0, 1.0], [0.0, 2.0], [-3.0, -1.0], [1.0, 4.0]]


def _orth_models(g):
    cores, domain = _rank_deficient_cores()
    return {"M16": ([g[f"M16_start_core{k}"] for k in range(4)], g["M16_domain"].tolist()), "deficient": (cores, domain)}


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("name", ["M16", "deficient"])
def test_orthogonalisation_every_position(g23, name, side):
    cores, domain = _orth_models(g23)[name]
    d = len(cores)
    rng = np.random.default_rng(3)
    pts = np.column_stack([rng.uniform(a, b, 64) for a, b in domain])
    before = ChebyshevTT.from_coeff_cores(cores, domain).eval_batch(pts)
    for position in (range(1, d) if side == "left" else range(0, d - 1)):
        tt = ChebyshevTT.from_coeff_cores(cores, domain)
        getattr(tt, f"orth_{side}")(position)
        figures = _lapack_sweep(cores, side, position)
        for k, (m, e_lapack, bond) in figures.items():
            c = tt._coeff_cores[k]
            U = c.reshape(-1, c.shape[2]) if side == "left" else c.reshape(c.shape[0], -1).T
            assert U.shape[1] == bond
            err = float(np.max(np.abs(U.T @ U - np.eye(bond))))
            print(f"{name} orth_{side}({position}) core {k}: {err:.2e} (LAPACK {e_lapack:.2e}, m eps {m * EPS:.2e})")
            assert err <= max(8.0 * e_lapack, m * EPS)
        untouched = range(position + 1, d) if side == "left" else range(0, position)
        for k in untouched:
            assert np.array_equal(tt._coeff_cores[k], cores[k]), f"core {k} beyond the pivot changed"
        assert tt.tt_ranks == [1] + [c.shape[2] for c in tt._coeff_cores]
        assert_parity(tt.eval_batch(pts), before, tol=1e-12, what=f"{name} orth_{side}({position})")


def test_wide_core_shrinks_its_bond(g23):
    cores = [g23[f"M3_start_core{k}"] for k in range(3)]            # (1, 6, 8), (8, 5, 8), (8, 7, 1)
    domain = g23["M3_domain"].tolist()
    pts = np.column_stack([np.random.default_rng(4).uniform(a, b, 64) for a, b in domain])
    before = ChebyshevTT.from_coeff_cores(cores, domain).eval_batch(pts)
    left = ChebyshevTT.from_coeff_cores(cores, domain)
    left.orth_left(1)
    assert left.tt_ranks == [1, 6, 8, 1] and left._coeff_cores[1].shape == (6, 5, 8)
    assert_parity(left.eval_batch(pts), before, tol=1e-12, what="M3 orth_left(1)")
    right = ChebyshevTT.from_coeff_cores(cores, domain)
    right.orth_right(0)
    assert right.tt_ranks == [1, 8, 7, 1]
    assert_parity(right.eval_batch(pts), before, tol=1e-12, what="M3 orth_right(0)")


def test_device_handle_is_dropped_by_the_mutators(g23):
    tt = _start(g23, "M4")
    tt.to_device(0)
    pts = g23["M4_pts"]
    y0 = tt.eval_batch(pts)
    assert tt.error_estimate() == tt._cached_error_estimate
    tt.run_completion(tolerance=0.0, max_iter=1, values=g23["M4_T"])
    assert tt._device_tt is None and tt._cached_error_estimate is None
    y1 = tt.eval_batch(pts)
    fresh = ChebyshevTT.from_coeff_cores(tt._coeff_cores, tt.domain)
    assert np.array_equal(y1, fresh.eval_batch(pts)) and not np.array_equal(y1, y0)
    tt.error_estimate()
    tt.orth_left(2)
    assert tt._device_tt is None and tt._cached_error_estimate is None
    y2 = tt.eval_batch(pts)
    assert np.array_equal(y2, ChebyshevTT.from_coeff_cores(tt._coeff_cores, tt.domain).eval_batch(pts))
    assert_parity(y2, y1, tol=1e-12, what="orth_left after completion")
