"""Roots, minima and maxima of an interpolant along one dimension: argument rules, the batch driver and the host
restatement (reference ``_calculus.py:198-355``).

Every fibre of at most :data:`MAX_DEVICE_N` nodes is solved on the device (``pcx_*_calculus_batch``,
``csrc/calculus_kernels.h``).  Longer fibres still come from the device, and the single calls then finish here with
:func:`roots_1d` / :func:`optimize_1d`, NumPy's ``chebroots`` on the coefficients of
``ChebyshevApproximation._chebyshev_coefficients_1d``; the batch calls refuse them.
"""
from __future__ import annotations

import numpy as np

from . import _lib

MAX_DEVICE_N = 64
_MODES = {"roots": 0, "min": 1, "max": 2}


def validate_calculus_args(ndim: int, dim, fixed, domain):
    """The reference's ``_validate_calculus_args``: ``(dim, [(dim_index, value), ...])`` with the same exceptions
    and messages.  ``fixed`` names every dimension but ``dim``; a value outside its dimension's domain is an error."""
    if ndim == 1:
        dim = 0 if dim is None else dim
        if dim != 0:
            raise ValueError(f"dim must be 0 for 1-D interpolant, got {dim}")
        if fixed and len(fixed) > 0:
            raise ValueError("fixed must be empty for 1-D interpolant")
        return dim, []
    if dim is None:
        raise ValueError("dim is required for multi-D interpolant")
    if dim < 0 or dim >= ndim:
        raise ValueError(f"dim {dim} out of range [0, {ndim - 1}]")
    fixed = {} if fixed is None else fixed
    expected = set(range(ndim)) - {dim}
    if set(fixed.keys()) != expected:
        raise ValueError(f"fixed must specify all dims except {dim}; missing {expected - set(fixed.keys())}")
    params = []
    for k, v in fixed.items():
        lo, hi = domain[k]
        if v < lo or v > hi:
            raise ValueError(f"Fixed value {v} for dim {k} outside domain [{lo}, {hi}]")
        params.append((k, v))
    return dim, params


def fixed_row(ndim: int, dim: int, params) -> np.ndarray:
    """The validated ``(dim_index, value)`` pairs as one batch row: the values in increasing dimension order."""
    vals = dict(params)
    return np.array([[float(vals[k]) for k in range(ndim) if k != dim]], dtype=float).reshape(1, ndim - 1)


def validate_batch_args(ndim: int, dim, fixed, domain, n_nodes) -> np.ndarray:
    """The ``(N, ndim - 1)`` float64 rows of a batch call along ``dim`` (``n_nodes`` and ``domain`` by dimension),
    checked on the host before any launch."""
    if isinstance(dim, bool) or not isinstance(dim, (int, np.integer)):
        raise TypeError(f"dim must be an int, got {type(dim).__name__}")
    if dim < 0 or dim >= ndim:
        raise ValueError(f"dim {dim} out of range [0, {ndim - 1}]")
    n = int(n_nodes[dim])
    if n > MAX_DEVICE_N:
        raise ValueError(f"dimension {dim} has {n} nodes: the batched solver takes at most {MAX_DEVICE_N} "
                         f"(the single-row calls handle more on the host)")
    rows = np.ascontiguousarray(np.asarray(fixed, dtype=np.float64))
    if ndim == 1 and rows.ndim == 1 and rows.size == 0:
        rows = rows.reshape(0, 0)
    if rows.ndim != 2 or rows.shape[1] != ndim - 1:
        raise ValueError(f"fixed must have shape (N, {ndim - 1}), got {rows.shape}")
    others = [k for k in range(ndim) if k != dim]
    for c, k in enumerate(others):
        lo, hi = domain[k]
        bad = np.nonzero((rows[:, c] < lo) | (rows[:, c] > hi))[0]
        if bad.size:
            r = int(bad[0])
            raise ValueError(f"Fixed value {rows[r, c]} for dim {k} outside domain [{lo}, {hi}] (row {r})")
    return rows


def run_batch(call, lib, n: int, N: int, mode: int):
    """Run one ``pcx_*_calculus_batch`` entry (``call(roots, counts, val, loc)`` -> rc) and shape its outputs:
    mode 0 ``(roots (N, max(n-1, 1)), counts)``, modes 1 and 2 ``(values, locations, counts)``."""
    W = max(n - 1, 1)
    counts = np.empty(N, dtype=np.int32)
    if mode == 0:
        roots = np.empty((N, W))
        _lib.check(call(_lib.p_f64(roots), _lib.p_i32(counts), None, None), lib)
        return roots, counts
    val, loc = np.empty(N), np.empty(N)
    _lib.check(call(None, _lib.p_i32(counts), _lib.p_f64(val), _lib.p_f64(loc)), lib)
    return val, loc, counts


def cheb1d_calculus(values, nodes, weights, diff, domain, mode: str, device: int | None = None):
    """``pcx_cheb1d_calculus`` on given fibres: ``values`` (N, n) at the ascending ``nodes`` of ``domain``.  Mode
    ``"roots"`` returns ``(roots, counts)``, ``"min"`` / ``"max"`` ``(values, locations, counts)``."""
    lib = _lib.load()
    v = _lib.f64(np.atleast_2d(values))
    N, n = v.shape
    m = _MODES[mode]
    nd, wt = _lib.f64(nodes), _lib.f64(weights)
    D = _lib.f64(diff) if diff is not None else None
    dev = _lib.default_device() if device is None else int(device)

    def call(r, c, va, lo_):
        return lib.pcx_cheb1d_calculus(dev, n, float(domain[0]), float(domain[1]), _lib.p_f64(nd), _lib.p_f64(wt),
                                       _lib.p_f64(D) if D is not None else None, _lib.p_f64(v), N, m, r, c, va, lo_)
    return run_batch(call, lib, n, N, m)


def single_roots(roots: np.ndarray, counts: np.ndarray) -> np.ndarray:
    if counts[0] < 0:
        raise np.linalg.LinAlgError("fibre is not finite or the eigenvalue iteration did not converge")
    return roots[0, :int(counts[0])].copy()


def single_extremum(val: np.ndarray, loc: np.ndarray, counts: np.ndarray):
    if counts[0] < 0:
        raise np.linalg.LinAlgError("fibre is not finite or the eigenvalue iteration did not converge")
    return float(val[0]), float(loc[0])


# ---------------------------------------------------------------------------------------------- host restatement
def roots_1d(values: np.ndarray, domain) -> np.ndarray:
    """Real roots in ``domain`` of the interpolant through ``values`` at ascending type-I nodes (reference
    ``_roots_1d``): ``chebroots`` of the coefficients, |imag| < 1e-10, inside [-1, 1] up to 1e-10, clipped, mapped,
    sorted, near-duplicates (``1e-10 (b - a + 1)``) dropped."""
    from numpy.polynomial.chebyshev import chebroots

    from .barycentric import ChebyshevApproximation
    coeffs = ChebyshevApproximation._chebyshev_coefficients_1d(values)
    raw = chebroots(coeffs)
    tol = 1e-10
    keep = [np.clip(r.real, -1.0, 1.0) for r in np.atleast_1d(raw)
            if abs(r.imag) < tol and -1.0 - tol <= r.real <= 1.0 + tol]
    if not keep:
        return np.array([], dtype=float)
    a, b = domain
    physical = np.sort(0.5 * (a + b) + 0.5 * (b - a) * np.array(keep))
    if len(physical) > 1:
        physical = physical[np.concatenate([[True], np.diff(physical) > 1e-10 * (b - a + 1)])]
    return physical


def optimize_1d(values, nodes, weights, diff, domain, mode: str = "min"):
    """Minimum or maximum of the interpolant (reference ``_optimize_1d``): the roots of ``D @ values`` are the
    critical points; the candidates ``[a, critical..., b]`` are evaluated barycentrically (a node within 1e-14 gives
    its value) and the first best one is returned as ``(value, location)``."""
    values = np.asarray(values, dtype=float)
    nodes = np.asarray(nodes, dtype=float)
    a, b = domain
    cand = np.concatenate([[a], roots_1d(np.asarray(diff) @ values, domain), [b]]).astype(float)
    dx = cand[:, None] - nodes[None, :]
    exact = np.abs(dx) < 1e-14
    wod = np.asarray(weights)[None, :] / np.where(exact, 1.0, dx)
    vals = (wod * values[None, :]).sum(axis=1) / wod.sum(axis=1)
    hit = exact.any(axis=1)
    if hit.any():
        vals = np.where(hit, values[exact.argmax(axis=1)], vals)
    idx = int(np.argmin(vals) if mode == "min" else np.argmax(vals))
    return float(vals[idx]), float(cand[idx])


def fibre_points(ndim: int, dim: int, row: np.ndarray, nodes) -> np.ndarray:
    """The n points ``(fixed..., x_j)`` of one fibre, columns in dimension order."""
    nodes = np.asarray(nodes, dtype=float)
    pts = np.empty((nodes.size, ndim))
    pts[:, [k for k in range(ndim) if k != dim]] = row.reshape(1, -1)
    pts[:, dim] = nodes
    return pts


def run_single(fibre_fn, batch_fn, n: int, mode: str, nodes, weights, diff, domain):
    """A single call: the device solver (``batch_fn(mode)``: one row) up to :data:`MAX_DEVICE_N` nodes, else the
    host restatement on the device-evaluated fibre (``fibre_fn()``)."""
    if n <= MAX_DEVICE_N:
        out = batch_fn(_MODES[mode])
        return single_roots(*out) if mode == "roots" else single_extremum(*out)
    values = fibre_fn()
    if mode == "roots":
        return roots_1d(values, domain)
    return optimize_1d(values, nodes, weights, diff, domain, mode)

