"""ChebyshevTT.fit_samples / from_samples end to end on the device, against the NumPy restatement (tests/tt_fit.py).

Parity rule: after m = 1, 2, 3 outer iterations from the same start, ``to_dense()`` and ``eval_batch`` on 500 fresh
points are compared normwise (2-norm) with the float64 restatement.  ALS amplifies rounding by the conditioning of each
solve, so the tolerance is not a constant: it is 8 x the restatement's own float64-against-longdouble deviation on
exactly these inputs, measured here on the CPU (the device orders its sums differently and orients its QR differently;
both numbers per case are in DESIGN.md section 5)."""
import functools

import numpy as np
import pytest

import tt_fit as F

from pychebyshev_amd import ChebyshevTT
from pychebyshev_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

PARITY_FACTOR = 8.0


def _f1d(x):
    return np.exp(x[:, 0]) * np.sin(3.0 * x[:, 0])


ONE_D = dict(f=_f1d, domain=[(-1.0, 2.0)], n=[9], rank=1, N=50)
ORDER5 = [2, 0, 4, 1, 3]


def _norm_dev(a, b):
    a, b = np.asarray(a, dtype=np.longdouble).ravel(), np.asarray(b, dtype=np.longdouble).ravel()
    return float(np.sqrt(np.sum((a - b) ** 2)) / np.sqrt(np.sum(b ** 2)))


def _uniform(domain, N, seed):
    rng = np.random.default_rng(seed)
    lo, hi = np.array([a for a, _ in domain]), np.array([b for _, b in domain])
    return lo + (hi - lo) * rng.random((N, len(domain)))


@functools.lru_cache(maxsize=None)
def _setup(case):
    """(model factory, user-order samples, storage-order samples, storage domain, start cores, ridge)."""
    ridge = 1e-12
    if case == "one_d":
        c = ONE_D
        pts = _uniform(c["domain"], c["N"], 100)
        start = F.start_cores(c["n"], 1, 0)
        make = lambda: ChebyshevTT.from_coeff_cores(start, c["domain"])          # noqa: E731
        return make, pts, c["f"](pts), pts, c["domain"], start, ridge, c["f"]
    if case == "reordered_5d":
        c = F.CASES["rank3_5d"]
        base = ChebyshevTT.from_coeff_cores(F.start_cores(c["n"], c["rank"], 0), c["domain"])
        moved = base.reorder(ORDER5, max_rank=c["rank"], tolerance=0.0)
        assert moved.dim_order == ORDER5
        start = [np.array(k) for k in moved._coeff_cores]
        sdomain = [tuple(b) for b in moved.domain]
        pts, y = F.samples("rank3_5d")                                          # user order
        make = lambda: ChebyshevTT.from_coeff_cores(start, sdomain, dim_order=ORDER5)      # noqa: E731
        return make, pts, y, np.ascontiguousarray(pts[:, ORDER5]), sdomain, start, ridge, c["f"]
    if case == "ridge_1e-8":
        c = F.CASES["sincos3d"]
        pts, y = F.samples("sincos3d", 20)                                      # 20 samples, 2 x 7 x 2 = 28 unknowns
        start = F.start_cores(c["n"], c["rank"], 0)
        make = lambda: ChebyshevTT.from_coeff_cores(start, c["domain"])          # noqa: E731
        return make, pts, y, pts, c["domain"], start, 1e-8, c["f"]
    c = F.CASES[case]
    pts, y = F.samples(case)
    start = F.start_cores(c["n"], c["rank"], 0)
    make = lambda: ChebyshevTT.from_coeff_cores(start, c["domain"])              # noqa: E731
    return make, pts, y, pts, c["domain"], start, ridge, c["f"]


@functools.lru_cache(maxsize=None)
def _restated(case):
    """The restatement after 1, 2, 3 iterations in float64 and longdouble: per m, (dense64, fresh64, deviation of the
    dense tensors, deviation on the fresh points); the fresh points in user and storage order."""
    _, _, y, spts, sdomain, start, ridge, _ = _setup(case)
    n = [c.shape[1] for c in start]
    snaps = {}
    for dtype in (np.float64, np.longdouble):
        snaps[dtype] = []
        F.fit(start, spts, y, sdomain, max_iter=3, tolerance=0.0, ridge=ridge, dtype=dtype, snapshots=snaps[dtype])
        # tolerance 0 still stops an iteration that repeats its residual bit for bit (d = 1: one solve is the optimum)
        assert 2 <= len(snaps[dtype]) <= 3
        snaps[dtype] += snaps[dtype][-1:] * (3 - len(snaps[dtype]))
    grid = F.grid_points(sdomain, n)
    fresh = _uniform(sdomain, 500, 77)
    out = []
    for m in range(3):
        d64, dld = F.evaluate(snaps[np.float64][m], grid, sdomain), F.evaluate(snaps[np.longdouble][m], grid, sdomain, np.longdouble)
        f64, fld = F.evaluate(snaps[np.float64][m], fresh, sdomain), F.evaluate(snaps[np.longdouble][m], fresh, sdomain, np.longdouble)
        out.append((d64, f64, _norm_dev(d64, dld), _norm_dev(f64, fld)))
    return out, fresh


def _storage_to_user(tt, pts_storage):
    out = np.empty_like(pts_storage)
    out[:, tt.dim_order] = pts_storage
    return out


PARITY_CASES = ["sincos3d", "rank4_3d", "rank3_5d", "reordered_5d", "one_d", "ridge_1e-8"]


@pytest.mark.parametrize("case", PARITY_CASES)
def test_parity_with_the_restatement_after_one_two_three_iterations(case):
    make, pts, y, _, sdomain, start, ridge, _ = _setup(case)
    ref, fresh = _restated(case)
    for m in (1, 2, 3):
        tt = make()
        tt.fit_samples(pts, y, max_iter=m, tolerance=0.0, ridge=ridge)
        assert tt.fit_info["iterations"] == (m if tt.num_dimensions > 1 else min(m, 2)) and tt.fit_info["n_samples"] == len(y)
        d64, f64, dev_dense, dev_fresh = ref[m - 1]
        dense = tt.to_dense()
        if tt.dim_order != list(range(tt.num_dimensions)):
            dense = np.transpose(dense, tt.dim_order)          # user axes -> storage axes, the restatement's frame
        got_dense = _norm_dev(dense.ravel(), d64)
        got_fresh = _norm_dev(tt.eval_batch(_storage_to_user(tt, fresh)), f64)
        print(f"{case} m={m}: restatement float64 vs longdouble {dev_dense:.3e} (dense) {dev_fresh:.3e} (fresh); "
              f"device vs float64 restatement {got_dense:.3e} (dense) {got_fresh:.3e} (fresh)")
        assert got_dense <= PARITY_FACTOR * dev_dense, (case, m, got_dense, dev_dense)
        assert got_fresh <= PARITY_FACTOR * dev_fresh, (case, m, got_fresh, dev_fresh)


@pytest.mark.parametrize("case", ["sincos3d", "rank4_3d", "rank3_5d", "reordered_5d", "one_d"])
def test_residual_is_monotone_and_the_fit_generalises(case):
    make, pts, y, spts, sdomain, start, ridge, f = _setup(case)
    tt = make()
    tt.fit_samples(pts, y, max_iter=12, tolerance=0.0)
    hist = tt.fit_info["residual"]
    assert len(hist) == tt.fit_info["iterations"] == (12 if tt.num_dimensions > 1 else 2)      # d = 1 repeats its residual
    for a, b in zip(hist, hist[1:]):
        assert b <= a * (1.0 + 1e-12), hist
    cores, ref_hist = F.fit(start, spts, y, sdomain, max_iter=12, tolerance=0.0)
    held = _uniform(sdomain, 2000, 55)                       # storage order
    truth = f(_storage_to_user(tt, held))
    err_ref = np.linalg.norm(F.evaluate(cores, held, sdomain) - truth) / np.linalg.norm(truth)
    err_dev = np.linalg.norm(tt.eval_batch(_storage_to_user(tt, held)) - truth) / np.linalg.norm(truth)
    print(f"{case}: residual {hist[-1]:.3e} (restatement {ref_hist[-1]:.3e}), held-out {err_dev:.3e} (restatement {err_ref:.3e})")
    assert err_dev <= 2.0 * err_ref
    assert hist[-1] <= 2.0 * ref_hist[-1]


def test_tolerance_stops_the_iterations_and_verbose_prints(capsys):
    make, pts, y, *_ = _setup("sincos3d")
    tt = make()
    tt.fit_samples(pts, y, max_iter=40, tolerance=1e-3, verbose=True)
    info = tt.fit_info
    hist = info["residual"]
    assert 2 <= info["iterations"] < 40 and len(hist) == info["iterations"]
    assert abs(hist[-2] - hist[-1]) <= 1e-3 * hist[-2]
    assert all(abs(a - b) > 1e-3 * a for a, b in zip(hist[:-2], hist[1:-1]))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "fit_samples iter" in ln]
    assert len(lines) == info["iterations"]
    assert tt._device_tt is None                             # dropped through _set_cores
    assert tt.error_estimate() == float(sum(np.max(np.abs(c[:, -1, :])) for c in tt._coeff_cores))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_from_samples_reaches_the_restatements_residual(seed, tmp_path):
    c = F.CASES["sincos3d"]
    pts, y = F.samples("sincos3d")
    tt = ChebyshevTT.from_samples(pts, y, 3, c["domain"], c["n"], rank=c["rank"], seed=seed, max_iter=12, tolerance=0.0)
    _, ref_hist = F.fit(F.start_cores(c["n"], c["rank"], seed), pts, y, c["domain"], max_iter=12, tolerance=0.0)
    assert tt.fit_info["residual"][-1] <= 2.0 * ref_hist[-1], (tt.fit_info["residual"][-1], ref_hist[-1])
    assert tt.method == "samples" and tt.function is None and tt.tt_ranks == [1, 2, 2, 1]
    # the result behaves like every other built model
    fresh = _uniform(c["domain"], 64, 9)
    vals = tt.eval_batch(fresh)
    path = tmp_path / "fitted.pkl"
    tt.save(str(path))
    back = ChebyshevTT.load(str(path))
    assert np.array_equal(back.eval_batch(fresh), vals) and back.method == "samples"
    two = tt + tt
    np.testing.assert_allclose(two.eval_batch(fresh), 2.0 * vals, rtol=0, atol=1e-12 * np.max(np.abs(vals)))
    value, grad = tt.gradient_batch(fresh)
    assert np.array_equal(value, vals) or np.max(np.abs(value - vals)) <= 1e-13 * np.max(np.abs(vals))
    h = 1e-6
    moved = fresh.copy()
    moved[:, 0] = np.minimum(moved[:, 0] + h, c["domain"][0][1])
    fd = (tt.eval_batch(moved) - vals) / np.where(moved[:, 0] - fresh[:, 0] == 0, 1.0, moved[:, 0] - fresh[:, 0])
    assert np.max(np.abs(fd - grad[:, 0])) <= 1e-4 * max(1.0, np.max(np.abs(grad[:, 0])))


def test_a_bond_the_unfolding_cannot_hold_shrinks():
    rng = np.random.default_rng(3)
    n, dom = [3, 7, 5], [(-1.0, 1.0)] * 3
    pts = rng.uniform(-1, 1, (400, 3))
    y = np.sin(pts[:, 0] + pts[:, 1]) * pts[:, 2]
    tt = ChebyshevTT.from_samples(pts, y, 3, dom, n, rank=5, seed=0, max_iter=2)
    assert tt.tt_ranks == [1, 3, 5, 1]
    wide = ChebyshevTT.from_coeff_cores([rng.standard_normal(s) for s in ((1, 3, 5), (5, 7, 5), (5, 5, 1))], dom)
    assert wide.tt_ranks == [1, 5, 5, 1]
    wide.fit_samples(pts, y, max_iter=2)
    assert wide.tt_ranks == [1, 3, 5, 1] and [c.shape for c in wide._coeff_cores] == [(1, 3, 3), (3, 7, 5), (5, 5, 1)]
    assert np.isfinite(wide.eval_batch(pts[:10])).all()


@pytest.mark.parametrize("case", ["sincos3d", "reordered_5d"])
def test_device_arrays_give_the_bits_of_host_arrays(case):
    make, pts, y, *_ = _setup(case)
    host, dev = make(), make()
    host.fit_samples(pts, y, max_iter=2, tolerance=0.0)
    d_pts, d_y = DeviceArray.from_host(pts), DeviceArray.from_host(y)
    dev.fit_samples(d_pts, d_y, max_iter=2, tolerance=0.0)
    assert [c.tobytes() for c in host._coeff_cores] == [c.tobytes() for c in dev._coeff_cores]
    assert host.fit_info == dev.fit_info
    assert np.array_equal(d_pts.to_host(), pts) and np.array_equal(d_y.to_host(), y)
    mixed = make()
    mixed.fit_samples(d_pts, y, max_iter=2, tolerance=0.0)              # device points, host values
    assert [c.tobytes() for c in host._coeff_cores] == [c.tobytes() for c in mixed._coeff_cores]


def test_bad_samples_on_the_device_raise_value_error():
    make, pts, y, *_ = _setup("sincos3d")
    for bad, what in ((np.nan, "NaN or Inf"), (np.inf, "NaN or Inf"), (1.0 + 1e-9, "outside its domain")):
        p2 = pts.copy()
        p2[17, 0] = bad                                     # dimension 0 is [-1, 1]
        tt = make()
        before = [c.copy() for c in tt._coeff_cores]
        with pytest.raises(ValueError, match=what):
            tt.fit_samples(DeviceArray.from_host(p2), DeviceArray.from_host(y))
        with pytest.raises(ValueError):
            tt.fit_samples(p2, y)                           # the host check says the same
        assert all(np.array_equal(a, b) for a, b in zip(before, tt._coeff_cores)) and tt.fit_info is None
    y2 = y.copy()
    y2[3] = np.nan
    with pytest.raises(ValueError, match="values contain NaN or Inf"):
        make().fit_samples(DeviceArray.from_host(pts), DeviceArray.from_host(y2))
    with pytest.raises(ValueError, match=r"shape \(N, 3\)"):
        make().fit_samples(DeviceArray.from_host(pts[:, :2]), DeviceArray.from_host(y))
    with pytest.raises(ValueError, match="values must have shape"):
        make().fit_samples(DeviceArray.from_host(pts), DeviceArray.from_host(y[:-1]))


def test_ridge_zero_needs_enough_samples_and_a_ridge_makes_it_solvable():
    make, pts, y, *_ = _setup("ridge_1e-8")                  # 20 samples, the middle core has 28 unknowns
    with pytest.raises(ValueError, match=r"20 samples cannot determine the 28 unknowns of position 1"):
        make().fit_samples(pts, y, ridge=0.0)
    tt = make()
    tt.fit_samples(pts, y, ridge=1e-8, max_iter=3, tolerance=0.0)       # parity with the restatement: the case above
    assert tt.fit_info["iterations"] == 3 and np.isfinite(tt.fit_info["residual"]).all()


def test_a_system_that_is_not_positive_definite_names_its_position():
    """Every sample at the midpoint of a one-dimensional model: T_1(0) = 0, so column 1 of the design matrix and the
    pivot G[1][1] are exactly zero."""
    tt = ChebyshevTT.from_coeff_cores([np.ones((1, 3, 1))], [(-1.0, 1.0)])
    pts, y = np.zeros((5, 1)), np.arange(5.0)
    with pytest.raises(ValueError, match=r"position 0 .*not\s+positive definite.*ridge"):
        tt.fit_samples(pts, y, ridge=0.0)
    assert tt.fit_info is None and np.array_equal(tt._coeff_cores[0], np.ones((1, 3, 1)))
    tt.fit_samples(pts, y, ridge=1e-6, max_iter=1)           # the ridge makes the same call solvable
    assert tt.fit_info["iterations"] == 1
