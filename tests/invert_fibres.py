"""Shared by the inversion tests: the fibres of calc_fibres with a target per row, the comparison with the NumPy
restatement (pychebyshev_amd._calculus.invert_rows) and the extended-precision Newton check.  Plain NumPy, no GPU.

Targets are drawn per row, uniformly between the fibre's smallest and largest value (default_rng([11, n])); a row
whose values are all equal has no such interval and draws from [v - 1, v + 1].  A target is redrawn until neither end
value is marginal, |p(lo) - t| and |p(hi) - t| >= 1e-6 max|v| (p at the ends by the restatement's own barycentric sum),
so no row has to be left out of a comparison."""
import functools

import numpy as np

import calc_fibres as CF

from pychebyshev_amd import ChebyshevApproximation, _calculus

X_TOL = 1e-13                 # of (b - a): the floor DESIGN 3.6 uses between two correct solvers
MAX_SKIPPED = 0


@functools.lru_cache(maxsize=None)
def inputs(n, dom=(-1.0, 1.0)):
    """(values (rows, n), targets (rows,)) of one fibre length: every family row of calc_fibres.families(n)."""
    V = CF.families(n)[0]
    x, w, _ = CF.grid(n, *dom)
    rng = np.random.default_rng([11, n])
    ends = np.stack([_calculus._bary_rows(V, x, w, np.full(V.shape[0], e)) for e in dom], axis=1)
    t = np.empty(V.shape[0])
    for r, v in enumerate(V):
        lo, hi = float(v.min()), float(v.max())
        if lo == hi:
            lo, hi = lo - 1.0, hi + 1.0
        scale = float(np.max(np.abs(v)))
        for _ in range(1000):
            t[r] = rng.uniform(lo, hi)
            if np.all(np.abs(ends[r] - t[r]) >= 1e-6 * scale):
                break
        else:
            raise AssertionError(f"n={n} row {r}: no target with both end values clear of it")
    t.setflags(write=False)
    return V, t


@functools.lru_cache(maxsize=None)
def reference(n, dom=(-1.0, 1.0)):
    """The restatement on inputs(n): (x, status, iterations), computed once."""
    V, t = inputs(n, dom)
    x, w, _ = CF.grid(n, *dom)
    out = _calculus.invert_rows(V, x, w, dom, t, return_iterations=True)
    for o in out:
        o.setflags(write=False)
    return out


NEAR_ZERO_TARGETS = (0.0,) + tuple(s * 10.0 ** -e for e in (15, 17, 20, 25, 50, 100, 200, 300) for s in (1.0, -1.0))


@functools.lru_cache(maxsize=None)
def near_zero(n, dom=(-1.0, 1.0)):
    """(values, targets) whose solution lies at or next to x = 0 inside a domain that contains 0, where a stop relative
    to |x| alone would never be reached: the strictly increasing fibres tanh(3x), x + 0.3 x^3 and 2 sin(x / 2) at the n >= 2
    nodes of `dom`, each against t = 0, t = +-1e-15 ... +-1e-300, and t = p(0) summed in another order (np.sum, not
    the sequential sum; the middle node's value where 0 is a node).  Every row has exactly one solution: status 1."""
    x, w, _ = CF.grid(n, *dom)
    rows, targets = [], []
    for f in (lambda u: np.tanh(3.0 * u), lambda u: u + 0.3 * u ** 3, lambda u: 2.0 * np.sin(0.5 * u)):
        v = f(x)
        hit = np.nonzero(np.abs(x) < 1e-14)[0]
        if hit.size:
            p0 = float(v[hit[0]])
        else:
            q = w / (0.0 - x)
            p0 = float(np.sum(q * v) / np.sum(q))
        for t in NEAR_ZERO_TARGETS + (p0,):
            rows.append(v)
            targets.append(t)
    V, t = np.array(rows), np.array(targets)
    V.setflags(write=False)
    t.setflags(write=False)
    return V, t


@functools.lru_cache(maxsize=None)
def near_zero_reference(n, dom=(-1.0, 1.0)):
    """The restatement on near_zero(n): (x, status, iterations), computed once."""
    V, t = near_zero(n, dom)
    x, w, _ = CF.grid(n, *dom)
    out = _calculus.invert_rows(V, x, w, dom, t, return_iterations=True)
    for o in out:
        o.setflags(write=False)
    return out


def check(n, got_x, got_status, want_x, want_status, dom, tag, stats):
    """status equal, x within X_TOL (b - a) and NaN exactly where the restatement's is; stats collects the worst
    difference and whether every x was the restatement's bit for bit."""
    got_x, got_status = np.asarray(got_x), np.asarray(got_status)
    assert got_x.shape == want_x.shape and got_status.shape == want_status.shape, (tag, got_x.shape, want_x.shape)
    assert np.array_equal(got_status, want_status), (tag, n, got_status, want_status)
    assert np.array_equal(np.isnan(got_x), np.isnan(want_x)), (tag, n, got_x, want_x)
    ok = ~np.isnan(want_x)
    err = float(np.max(np.abs(got_x[ok] - want_x[ok]), initial=0.0)) / (dom[1] - dom[0])
    stats["x"] = max(stats.get("x", 0.0), err)
    stats["bitwise"] = stats.get("bitwise", True) and bool(np.array_equal(got_x, want_x, equal_nan=True))
    stats["rows"] = stats.get("rows", 0) + got_x.size
    assert err <= X_TOL, (tag, n, err)


def newton_ratio(n, V, t, x, status, dom=(-1.0, 1.0)):
    """For every returned x with status >= 1: the Newton correction (p(x) - t) / p'(x) by Clenshaw on the row's own
    coefficients in extended precision, in units of the reference frame [-1, 1].  Where x lies inside
    (|u| < 1 - 1e-9) and roots_1d(V - t) has a root, the correction is at most max(10 x that of the nearest such root,
    1e-13 (b - a)); a returned point that the eigenvalue solver does not confirm (it finds no root) is held to the floor
    1e-13 (b - a) alone.  A point within 1e-9 of an end is not checked (p' need not be resolved there) and is counted.
    -> (worst device correction, worst restatement correction, rows compared with a root, rows held to the floor alone,
    rows at an end)."""
    a, b = dom
    floor = 2e-13               # corrections are in [-1, 1] units: half of (b - a) per unit, so 1e-13 (b - a) is 2e-13 there
    worst_dev = worst_ref = 0.0
    rows = unconfirmed = at_end = 0
    for r in range(V.shape[0]):
        if status[r] < 1:
            continue
        u = (2.0 * x[r] - (a + b)) / (b - a)
        if not abs(u) < 1.0 - 1e-9:
            at_end += 1
            continue
        shifted = V[r] - t[r]
        coef = ChebyshevApproximation._chebyshev_coefficients_1d(shifted)
        dev = abs(float(CF.hp_newton(coef, [u])[0]))
        worst_dev = max(worst_dev, dev)
        ref = CF.ref_roots(shifted, dom)
        if ref is None or not ref.size:
            unconfirmed += 1
            assert dev <= floor, (n, r, dev, x[r])
            continue
        near = ref[np.argmin(np.abs(ref - x[r]))]
        rf = abs(float(CF.hp_newton(coef, [(2.0 * near - (a + b)) / (b - a)])[0]))
        rows += 1
        worst_ref = max(worst_ref, rf)
        assert dev <= max(10.0 * rf, floor), (n, r, dev, rf, x[r], near)
    return worst_dev, worst_ref, rows, unconfirmed, at_end
