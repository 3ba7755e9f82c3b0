"""The normal equations of one ALS position on scattered samples, directly through pcx_tt_fit_normal, in both forced
forms of the Gram kernel (csrc/tt_fit_kernels.h: k_ttf_interface, k_ttf_gram_valu / k_ttf_gram_mfma, k_ttf_reduce).

Reference: the longdouble restatement (tests/tt_fit.py).  Bound, derived and not measured: entrywise
    |G - G_ld| <= gamma G_abs,    |b - b_ld| <= gamma b_abs,    gamma = (N + 4 sum_k (n_k + r_k) + 8) 2^-52,
G_abs / b_abs the same formulas with every core entry, basis value and y replaced by its absolute value: the running
error bound of a sum of N products of chain values, the slack constant covering the recurrence.

Shapes: the smallest at which each body can go wrong -- N on both sides of a k-step (4), a wave (64) and a chunk (256),
P on both sides of a 16-tile and a 64-block of the augmented (P + 1)-wide Gram and of 256, every position, unequal
ranks, ranks 1 .. 33, rows at the domain's corners (t = -1 and +1 exactly).  P = 257 does not exist (a prime above the
256 a rank or a node count may be): 258 and 260 stand in for it, and at P = 256 the augmented Gram is 257 wide."""
import ctypes

import numpy as np
import pytest

import tt_fit as F

from pychebyshev_amd import ChebyshevTT, _lib
from pychebyshev_amd import tensor_train as tt_mod
from pychebyshev_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

GUARD = 64
VALU, MFMA = 1, 2


def _model(n, ranks, seed, domain=None):
    rng = np.random.default_rng(seed)
    d = len(n)
    cores = [rng.standard_normal((ranks[k], n[k], ranks[k + 1])) for k in range(d)]
    domain = domain or [(-1.0 - 0.25 * k, 0.5 + k) for k in range(d)]
    return cores, domain


def _samples(domain, N, seed, corners=True):
    """Uniform points; with corners the first rows are the all-lo corner, the all-hi corner and an alternating one."""
    rng = np.random.default_rng(seed)
    lo = np.array([a for a, _ in domain])
    hi = np.array([b for _, b in domain])
    pts = lo + (hi - lo) * rng.random((N, len(domain)))
    if corners:
        special = [lo, hi, np.where(np.arange(len(lo)) % 2 == 0, lo, hi)]
        for i in range(min(N - 1, 3)):
            pts[i] = special[i]
    return np.ascontiguousarray(pts), rng.standard_normal(N)


def _session(cores, domain, pts, y):
    tt = ChebyshevTT.from_coeff_cores(cores, domain)
    return tt_mod._FitSession(tt, pts, y, pts.shape[0])


def _normal_raw(session, cores, k):
    """pcx_tt_fit_normal into host buffers that start as a NaN pattern with a guard tail."""
    n = _lib.i32([c.shape[1] for c in cores])
    ranks = _lib.i32([1] + [c.shape[2] for c in cores])
    cat = _lib.f64(np.concatenate([c.ravel() for c in cores]))
    P = cores[k].size
    G = np.full(P * P + GUARD, np.nan)
    b = np.full(P + GUARD, np.nan)
    G.view(np.uint64)[:] = ~np.uint64(0)
    b.view(np.uint64)[:] = ~np.uint64(0)
    rc = session.lib.pcx_tt_fit_normal(session.handle, len(cores), _lib.p_i32(n), _lib.p_i32(ranks), _lib.p_f64(cat), k,
                                       _lib.p_f64(G), _lib.p_f64(b))
    assert rc == 0, _lib.last_error(session.lib)
    assert np.all(G.view(np.uint64)[P * P:] == ~np.uint64(0)) and np.all(b.view(np.uint64)[P:] == ~np.uint64(0)), "overrun"
    assert not np.isnan(G[:P * P]).any() and not np.isnan(b[:P]).any(), "an element was not written"
    return G[:P * P].reshape(P, P), b[:P]


def _gamma(cores, N):
    return (N + 4 * sum(c.shape[1] + c.shape[2] for c in cores) + 8) * 2.0 ** -52


def _reference(cores, domain, pts, y, k):
    G_ld, b_ld = F.normal(cores, pts, y, domain, k, np.longdouble)
    G_abs, b_abs = F.normal(cores, pts, y, domain, k, np.longdouble, absolute=True)
    return G_ld, b_ld, G_abs, b_abs


def _check_position(cores, domain, pts, y, k, forms=(VALU, MFMA)):
    N = pts.shape[0]
    G_ld, b_ld, G_abs, b_abs = _reference(cores, domain, pts, y, k)
    gamma = np.longdouble(_gamma(cores, N))
    session = _session(cores, domain, pts, y)
    try:
        for form in forms:
            session.set_form(form)
            G, b = _normal_raw(session, cores, k)
            G2, b2 = _normal_raw(session, cores, k)
            assert G.tobytes() == G2.tobytes() and b.tobytes() == b2.tobytes(), "two identical calls differ"
            assert np.array_equal(G, G.T), "the two triangles differ"
            eg = np.abs(G.astype(np.longdouble) - G_ld) - gamma * G_abs
            eb = np.abs(b.astype(np.longdouble) - b_ld) - gamma * b_abs
            worst_g = float(np.max(np.abs(G.astype(np.longdouble) - G_ld) / np.maximum(G_abs, np.finfo(float).tiny)) / gamma)
            worst_b = float(np.max(np.abs(b.astype(np.longdouble) - b_ld) / np.maximum(b_abs, np.finfo(float).tiny)) / gamma)
            print(f"form {form} k {k} P {b.size} N {N}: |G - G_ld| / (gamma G_abs) <= {worst_g:.3f}, b: {worst_b:.3f}")
            assert np.all(eg <= 0), f"form {form}, position {k}: G misses its bound by a factor {worst_g:.2f}"
            assert np.all(eb <= 0), f"form {form}, position {k}: b misses its bound by a factor {worst_b:.2f}"
    finally:
        session.close()


# (n, ranks, positions, N): P of each position in the comment
CASES = {
    "d1_n2_N1": ([2], [1, 1], [0], 1),                                            # P = 2
    "d1_n15_N3": ([15], [1, 1], [0], 3),                                          # 15: one 16-tile with the y column
    "d1_n16_N63": ([16], [1, 1], [0], 63),                                        # 16: the y column opens a second tile
    "d1_n17_N65": ([17], [1, 1], [0], 65),                                        # 17
    "d2_rank5_N64": ([3, 11], [1, 5, 1], [0, 1], 64),                             # 15, 55
    "d2_rank3_N4099": ([3, 11], [1, 3, 1], [0, 1], 4099),                         # 9, 33: 17 chunks, the last of 3 samples
    "d3_ranks23_N259": ([2, 3, 11], [1, 2, 3, 1], [0, 1, 2], 259),                # 4, 18, 33: two chunks
    "d3_P63_N65": ([3, 7, 3], [1, 3, 3, 1], [1], 65),                             # 63: the augmented Gram fills one 64-block
    "d3_P64_N63": ([2, 16, 2], [1, 2, 2, 1], [1], 63),                            # 64: a second 64-block for the y column
    "d2_P65_N64": ([5, 13], [1, 5, 1], [1], 64),                                  # 65
    "d3_P255_N65": ([5, 3, 17], [1, 5, 17, 1], [0, 1, 2], 65),                    # 25, 255, 289; ranks 5 | 17
    "d3_P256_N259": ([8, 2, 16], [1, 8, 16, 1], [1], 259),                        # 256; ranks 8 | 16
    "d3_P258_N63": ([2, 3, 43], [1, 2, 43, 1], [1], 63),                          # 258
    "d3_P260_N3": ([2, 10, 13], [1, 2, 13, 1], [1], 3),                           # 260
    "d3_bond33_N64": ([11, 2, 3], [1, 33, 2, 1], [0, 1], 64),                     # 363, 132: a bond wider than a wave's half
    "d3_ranks15_16_N65": ([2, 2, 2], [1, 15, 16, 1], [1, 2], 65),                 # 480, 32
    "d3_ranks17_8_N3": ([3, 2, 2], [1, 17, 8, 1], [0, 1, 2], 3),                  # 51, 272, 16
    "d5_N4099": ([2, 3, 2, 3, 2], [1, 2, 3, 5, 2, 1], [0, 2, 4], 4099),           # 4, 30, 4
    "d5_rank1_N259": ([2, 3, 2, 3, 2], [1, 1, 1, 1, 1, 1], [1, 3], 259),          # 3, 3: rank 1 throughout
}


@pytest.mark.parametrize("name", list(CASES))
def test_normal_equations_meet_the_running_error_bound(name):
    n, ranks, positions, N = CASES[name]
    cores, domain = _model(n, ranks, seed=len(name))
    pts, y = _samples(domain, N, seed=N)
    for k in positions:
        _check_position(cores, domain, pts, y, k)


def test_rows_at_every_corner_of_the_domain():
    """All 2^3 corners: every t is -1 or +1 exactly, every T_j is +-1."""
    cores, domain = _model([11, 16, 3], [1, 3, 2, 1], seed=2, domain=[(-2.0, 1.0), (0.5, 0.75), (1.0, 9.0)])
    corners = np.array([[domain[k][(i >> k) & 1] for k in range(3)] for i in range(8)])
    y = np.random.default_rng(0).standard_normal(8)
    for k in range(3):
        _check_position(cores, domain, corners, y, k)


def test_the_automatic_form_switches_at_sixteen_unknowns():
    """form 0: VALU below P = 16, MFMA from there on -- each gives the bits of the forced form."""
    for n, want in ((15, VALU), (16, MFMA)):
        cores, domain = _model([n], [1, 1], seed=1)
        pts, y = _samples(domain, 70, seed=3)
        session = _session(cores, domain, pts, y)
        try:
            got = {}
            for form in (0, VALU, MFMA):
                session.set_form(form)
                got[form] = _normal_raw(session, cores, 0)
            assert got[0][0].tobytes() == got[want][0].tobytes() and got[0][1].tobytes() == got[want][1].tobytes()
        finally:
            session.close()


def test_host_and_device_samples_give_equal_bits():
    cores, domain = _model([3, 11, 2], [1, 3, 5, 1], seed=7)
    pts, y = _samples(domain, 259, seed=8)
    host = _session(cores, domain, pts, y)
    d_pts, d_y = DeviceArray.from_host(pts), DeviceArray.from_host(y)
    dev = _session(cores, domain, d_pts, d_y)
    try:
        for form in (VALU, MFMA):
            for k in range(3):
                host.set_form(form)
                dev.set_form(form)
                Gh, bh = _normal_raw(host, cores, k)
                Gd, bd = _normal_raw(dev, cores, k)
                assert Gh.tobytes() == Gd.tobytes() and bh.tobytes() == bd.tobytes()
        assert host.sumsq(cores).tobytes() == dev.sumsq(cores).tobytes()
    finally:
        host.close()
        dev.close()
    assert np.array_equal(d_pts.to_host(), pts)           # adopted, not written


def _chain_abs(cores, pts, domain):
    """The chain with every core entry and basis value replaced by its absolute value (longdouble)."""
    cs = [np.abs(np.asarray(c, dtype=np.longdouble)) for c in cores]
    Ts = F.bases(pts, domain, [c.shape[1] for c in cs], np.longdouble, absolute=True)
    L = np.ones((pts.shape[0], 1), dtype=np.longdouble)
    for m in range(len(cs)):
        L = np.einsum("ia,ij,ajb->ib", L, Ts[m], cs[m])
    return L[:, 0]


def test_residual_sums():
    """sum (TT - y)^2 and sum y^2 against the longdouble restatement.  A device value is f_ld + e with |e| <= g f_abs,
    g = (4 sum_k (n_k + r_k) + 8) 2^-52 (the chain's part of the bound above); a square then carries 2 |f_ld - y| |e| +
    e^2, and the sum of N of them (N + 4) 2^-52 of itself."""
    for n, ranks, N in (([3, 11, 2], [1, 3, 5, 1], 4099), ([17], [1, 1], 3), ([2, 3, 2, 3, 2], [1, 2, 3, 5, 2, 1], 259)):
        cores, domain = _model(n, ranks, seed=11)
        pts, y = _samples(domain, N, seed=12)
        session = _session(cores, domain, pts, y)
        try:
            got = session.sumsq(cores)
            assert got.tobytes() == session.sumsq(cores).tobytes()
        finally:
            session.close()
        eps = np.longdouble(2.0 ** -52)
        f_ld = F.evaluate(cores, pts, domain, np.longdouble)
        y_ld = y.astype(np.longdouble)
        e = np.longdouble(_gamma(cores, 0)) * _chain_abs(cores, pts, domain)
        r = np.abs(f_ld - y_ld)
        want = np.array([np.sum(r ** 2), np.sum(y_ld ** 2)])
        slack0 = np.sum(2 * r * e + e * e) + (N + 4) * eps * np.sum((r + e) ** 2)
        slack1 = (N + 4) * eps * want[1]
        print(f"n {n} N {N}: sum (f - y)^2 off by {float(abs(got[0] - want[0]) / slack0):.3f} of its bound, "
              f"sum y^2 by {float(abs(got[1] - want[1]) / slack1):.3f}")
        assert abs(np.longdouble(got[0]) - want[0]) <= slack0, (float(got[0]), float(want[0]), float(slack0))
        assert abs(np.longdouble(got[1]) - want[1]) <= slack1


def test_the_largest_position_runs():
    """P = 4096 (16 x 16 x 16), the documented limit, on the automatic form; 48 rows of G are checked against the bound."""
    cores, domain = _model([2, 16, 2], [1, 16, 16, 1], seed=5)
    pts, y = _samples(domain, 5, seed=6)
    session = _session(cores, domain, pts, y)
    try:
        G, b = _normal_raw(session, cores, 1)
    finally:
        session.close()
    assert G.shape == (4096, 4096) and np.array_equal(G, G.T)
    rows = np.random.default_rng(1).choice(4096, 48, replace=False)
    gamma = np.longdouble(_gamma(cores, 5))
    for absolute in (False, True):
        cs = [np.abs(c) for c in cores] if absolute else cores
        yy = np.abs(y) if absolute else y
        Ts = F.bases(pts, domain, [2, 16, 2], np.longdouble, absolute)
        A = F.design([np.asarray(c, dtype=np.longdouble) for c in cs], Ts, 1)
        if absolute:
            G_abs, b_abs = A[:, rows].T @ A, A.T @ yy.astype(np.longdouble)
        else:
            G_ld, b_ld = A[:, rows].T @ A, A.T @ yy.astype(np.longdouble)
    assert np.all(np.abs(G[rows].astype(np.longdouble) - G_ld) <= gamma * G_abs)
    assert np.all(np.abs(b.astype(np.longdouble) - b_ld) <= gamma * b_abs)


def test_c_abi_argument_errors_return_codes():
    lib = _lib.load()
    cores, domain = _model([3, 4, 2], [1, 2, 3, 1], seed=1)
    pts, y = _samples(domain, 20, seed=2)
    lo, hi = _lib.f64([a for a, _ in domain]), _lib.f64([b for _, b in domain])
    h = ctypes.c_void_p()
    P, Y, LO, HI = _lib.p_f64(pts), _lib.p_f64(y), _lib.p_f64(lo), _lib.p_f64(hi)
    INV, UNS = _lib.PCX_ERR_INVALID, _lib.PCX_ERR_UNSUPPORTED
    assert lib.pcx_tt_fit_create(0, 3, LO, HI, P, Y, 20, None) == INV
    for args in ((0, 0, LO, HI, P, Y, 20), (0, 17, LO, HI, P, Y, 20), (0, 3, None, HI, P, Y, 20), (0, 3, LO, None, P, Y, 20),
                 (0, 3, LO, HI, None, Y, 20), (0, 3, LO, HI, P, None, 20), (0, 3, LO, HI, P, Y, 0), (0, 3, LO, HI, P, Y, -5),
                 (0, 3, HI, LO, P, Y, 20), (0, 3, LO, LO, P, Y, 20)):
        assert lib.pcx_tt_fit_create(*args, ctypes.byref(h)) == INV and not h.value, args
        assert _lib.last_error(lib)
    assert lib.pcx_tt_fit_create(0, 3, LO, HI, P, Y, (1 << 28) + 1, ctypes.byref(h)) == UNS and not h.value
    assert lib.pcx_tt_fit_create(99, 3, LO, HI, P, Y, 20, ctypes.byref(h)) == _lib.PCX_ERR_NO_DEVICE and not h.value
    for bad in (np.nan, np.inf):
        p2, y2 = pts.copy(), y.copy()
        p2[3, 2] = bad
        y2[19] = bad
        assert lib.pcx_tt_fit_create(0, 3, LO, HI, _lib.p_f64(p2), Y, 20, ctypes.byref(h)) == INV and not h.value
        assert "points contain NaN or Inf" in _lib.last_error(lib)
        assert lib.pcx_tt_fit_create(0, 3, LO, HI, P, _lib.p_f64(y2), 20, ctypes.byref(h)) == INV and not h.value
        assert "values contain NaN or Inf" in _lib.last_error(lib)
        d2, dy2 = DeviceArray.from_host(p2), DeviceArray.from_host(y2)
        dp, dy = DeviceArray.from_host(pts), DeviceArray.from_host(y)
        assert lib.pcx_tt_fit_create_dev(0, 3, LO, HI, ctypes.c_void_p(d2.ptr), ctypes.c_void_p(dy.ptr), 20, ctypes.byref(h)) == INV
        assert "points contain NaN or Inf" in _lib.last_error(lib) and not h.value
        assert lib.pcx_tt_fit_create_dev(0, 3, LO, HI, ctypes.c_void_p(dp.ptr), ctypes.c_void_p(dy2.ptr), 20, ctypes.byref(h)) == INV
        assert "values contain NaN or Inf" in _lib.last_error(lib) and not h.value
    p2 = pts.copy()
    p2[5, 1] = domain[1][1] + 1e-9
    assert lib.pcx_tt_fit_create(0, 3, LO, HI, _lib.p_f64(p2), Y, 20, ctypes.byref(h)) == INV
    assert "storage dimension 1 lies outside" in _lib.last_error(lib)
    d2 = DeviceArray.from_host(p2)
    assert lib.pcx_tt_fit_create_dev(0, 3, LO, HI, ctypes.c_void_p(d2.ptr), ctypes.c_void_p(dy.ptr), 20, ctypes.byref(h)) == INV
    assert "storage dimension 1 lies outside" in _lib.last_error(lib) and not h.value
    assert lib.pcx_tt_fit_create_dev(0, 3, LO, HI, None, ctypes.c_void_p(dy.ptr), 20, ctypes.byref(h)) == INV

    assert lib.pcx_tt_fit_create(0, 3, LO, HI, P, Y, 20, ctypes.byref(h)) == 0 and h.value
    try:
        n, ranks = _lib.i32([3, 4, 2]), _lib.i32([1, 2, 3, 1])
        cat = _lib.f64(np.concatenate([c.ravel() for c in cores]))
        G, b, s2 = np.empty(24 * 24), np.empty(24), np.empty(2)
        NN, RR, CC, GG, BB = _lib.p_i32(n), _lib.p_i32(ranks), _lib.p_f64(cat), _lib.p_f64(G), _lib.p_f64(b)
        assert lib.pcx_tt_fit_normal(None, 3, NN, RR, CC, 1, GG, BB) == INV
        for args in ((3, None, RR, CC, 1, GG, BB), (3, NN, None, CC, 1, GG, BB), (3, NN, RR, None, 1, GG, BB),
                     (3, NN, RR, CC, 1, None, BB), (3, NN, RR, CC, 1, GG, None), (3, NN, RR, CC, -1, GG, BB),
                     (3, NN, RR, CC, 3, GG, BB), (2, NN, RR, CC, 1, GG, BB), (4, NN, RR, CC, 1, GG, BB)):
            assert lib.pcx_tt_fit_normal(h, *args) == INV, args
        for bad_ranks in ([2, 2, 3, 1], [1, 2, 3, 2], [1, 0, 3, 1]):
            assert lib.pcx_tt_fit_normal(h, 3, NN, _lib.p_i32(_lib.i32(bad_ranks)), CC, 1, GG, BB) == INV
        assert lib.pcx_tt_fit_normal(h, 3, _lib.p_i32(_lib.i32([3, 0, 2])), RR, CC, 1, GG, BB) == INV
        # outside the kernels' range: refused before anything runs (the core buffer is never read)
        assert lib.pcx_tt_fit_normal(h, 3, NN, _lib.p_i32(_lib.i32([1, 257, 3, 1])), CC, 1, GG, BB) == UNS
        assert lib.pcx_tt_fit_normal(h, 3, _lib.p_i32(_lib.i32([3, 257, 2])), RR, CC, 1, GG, BB) == UNS
        assert lib.pcx_tt_fit_normal(h, 3, NN, _lib.p_i32(_lib.i32([1, 64, 33, 1])), CC, 1, GG, BB) == UNS      # P = 8448
        assert "more than 4096" in _lib.last_error(lib)
        assert lib.pcx_tt_fit_residual(None, 3, NN, RR, CC, _lib.p_f64(s2)) == INV
        assert lib.pcx_tt_fit_residual(h, 3, NN, RR, CC, None) == INV
        assert lib.pcx_tt_fit_residual(h, 2, NN, RR, CC, _lib.p_f64(s2)) == INV
        assert lib.pcx_tt_fit_set_form(None, 1) == INV
        for form in (-1, 3):
            assert lib.pcx_tt_fit_set_form(h, form) == INV
        # the session still works after all of that
        assert lib.pcx_tt_fit_normal(h, 3, NN, RR, CC, 1, GG, BB) == 0 and np.isfinite(G).all()
        assert lib.pcx_tt_fit_residual(h, 3, NN, RR, CC, _lib.p_f64(s2)) == 0 and np.isfinite(s2).all()
    finally:
        assert lib.pcx_tt_fit_destroy(h) == 0
    assert lib.pcx_tt_fit_destroy(None) == 0
