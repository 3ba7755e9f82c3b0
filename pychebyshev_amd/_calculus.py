"""Roots, minima and maxima of an interpolant along one dimension: argument rules, the batch driver, the front end the
four model classes share (:class:`FibreCalculusMixin`) and the host restatement (reference ``_calculus.py:198-355``).

Every fibre of at most :data:`MAX_DEVICE_N` nodes is solved on the device (``pcx_*_calculus_batch``,
``csrc/calculus_kernels.h``).  Longer fibres still come from the device, and the single calls then finish here with
:func:`roots_1d` / :func:`optimize_1d`, NumPy's ``chebroots`` on the coefficients of
``ChebyshevApproximation._chebyshev_coefficients_1d``; the batch calls refuse them.

With a target per row (``pcx_*_solve_batch``): ``roots(level=)`` / ``roots_batch(level=)`` subtract the row's level from
its fibre on the device before the same solver, and ``invert_batch`` solves one bracketed scalar equation per fibre, a
device lane each (``csrc/invert_kernels.h``); :func:`invert_rows` / :func:`invert_1d` restate that routine in NumPy.
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


def validate_dim(ndim: int, dim) -> None:
    """``dim`` of a batch call: an int (no bool) in ``[0, ndim)``."""
    if isinstance(dim, bool) or not isinstance(dim, (int, np.integer)):
        raise TypeError(f"dim must be an int, got {type(dim).__name__}")
    if dim < 0 or dim >= ndim:
        raise ValueError(f"dim {dim} out of range [0, {ndim - 1}]")


def validate_batch_args(ndim: int, dim, fixed, domain, n_nodes) -> np.ndarray:
    """The ``(N, ndim - 1)`` float64 rows of a batch call along ``dim`` (``n_nodes`` and ``domain`` by dimension),
    checked on the host before any launch: ``dim``, the 64-node cap of the solver along it, then the rows."""
    validate_dim(ndim, dim)
    n = int(n_nodes[dim])
    if n > MAX_DEVICE_N:
        raise ValueError(f"dimension {dim} has {n} nodes: the batched solver takes at most {MAX_DEVICE_N} "
                         f"(the single-row calls handle more on the host)")
    return _host_rows(ndim, dim, fixed, domain)


def validate_fibre_args(ndim: int, dim, fixed, domain):
    """The rows of the calls that need no solver (``ladder_batch`` / ``fibre_batch``): :func:`validate_batch_args`'s
    checks and messages without the 64-node cap along ``dim``.  NaN passes the domain check (it makes its row NaN).
    ``fixed`` may be a device array: its shape is checked here, its values are not (they would have to come to the
    host first); it is returned as the ``DeviceArray``."""
    from .device import as_device_array
    validate_dim(ndim, dim)
    dev = as_device_array(fixed)
    if dev is not None:
        if dev.ndim != 2 or dev.shape[1] != ndim - 1:
            raise ValueError(f"fixed must have shape (N, {ndim - 1}), got {dev.shape}")
        return dev
    return _host_rows(ndim, dim, fixed, domain)


def _host_rows(ndim: int, dim: int, fixed, domain) -> np.ndarray:
    """Host ``fixed`` as ``(N, ndim - 1)`` float64 rows, every value inside its dimension's domain (NaN passes)."""
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


def validate_ladder_xs(xs, N: int):
    """The values of a ladder: ``(xs, m, per_row)``.  Shape ``(m,)`` (a scalar counts as ``(1,)``) is shared by all rows
    and comes back as a host array; ``(N, m)`` is one set per row, a host array or a ``DeviceArray``.  The values are not
    checked: points outside the domain extrapolate, as in evaluation, and a NaN gives NaN in its own cell."""
    from .device import as_device_array
    dev = as_device_array(xs)
    if dev is not None:
        if dev.ndim == 2 and dev.shape[0] == N:
            return dev, dev.shape[1], True
        if dev.ndim == 1:
            return np.ascontiguousarray(dev.to_host()), dev.shape[0], False       # shared values enter from the host
        raise ValueError(f"xs must have shape (m,) or ({N}, m), got {dev.shape}")
    arr = np.asarray(xs, dtype=np.float64)
    if arr.ndim == 0:
        arr = arr.reshape(1)
    if arr.ndim == 1:
        return np.ascontiguousarray(arr), arr.shape[0], False
    if arr.ndim == 2 and arr.shape[0] == N:
        return np.ascontiguousarray(arr), arr.shape[1], True
    raise ValueError(f"xs must have shape (m,) or ({N}, m), got {arr.shape}")


def validate_ladder_out(out, shape):
    """``out=`` of a ladder call: ``None``, a ``DeviceArray`` or a C-contiguous float64 NumPy array of the result's shape.
    Returns ``(host_out, dev_out)``, at most one of them set.  Needs no device."""
    from .device import as_device_array
    if out is None:
        return None, None
    if isinstance(out, np.ndarray):
        if out.dtype != np.float64:
            raise ValueError(f"out must be float64, got {out.dtype}")
        if out.shape != tuple(shape):
            raise ValueError(f"out.shape={out.shape} does not match the result {tuple(shape)}")
        if not out.flags.c_contiguous:
            raise ValueError("out must be C-contiguous")
        return out, None
    dev = as_device_array(out)
    if dev is None:
        raise ValueError("out must be a DeviceArray, a float64 NumPy array or None")
    if dev.shape != tuple(shape):
        raise ValueError(f"out.shape={dev.shape} does not match the result {tuple(shape)}")
    return None, dev


def run_ladder(lib, device: int, stream, call_host, call_dev, rows, xs, m: int, per_row: bool, out):
    """Drive one ``pcx_*_ladder_batch`` / ``_dev`` pair over validated arguments.  ``call_host(fixed, N, xs, m, per_row,
    out)`` and ``call_dev(d_fixed, N, xs, m, per_row, d_out, stream)`` return the entry's code.  All-host arguments go
    through the host entry; a device array among ``rows``, a per-row ``xs`` or ``out`` sends the call through the device
    entry, host pieces uploaded first.  The result is ``out`` when given, a ``DeviceArray`` (complete on return) when
    ``rows`` is one, else a NumPy array."""
    import ctypes

    from .device import DeviceArray, is_device_array
    N = rows.shape[0]
    host_out, dev_out = validate_ladder_out(out, (N, m))
    rows_dev, xs_dev = is_device_array(rows), per_row and is_device_array(xs)
    for name, arr in (("fixed", rows if rows_dev else None), ("xs", xs if xs_dev else None), ("out", dev_out)):
        if arr is not None and arr.size and arr.device != device:
            raise ValueError(f"{name} lives on device {arr.device} but the model is on device {device}; "
                             f"call to_device({arr.device}) on the model first")
    if not (rows_dev or xs_dev or dev_out is not None):
        res = np.empty((N, m)) if host_out is None else host_out
        if N and m:
            _lib.check(call_host(_lib.p_f64(rows), N, _lib.p_f64(xs), m, 1 if per_row else 0, _lib.p_f64(res)), lib)
        return res
    res = DeviceArray.empty((N, m), device) if dev_out is None else dev_out
    if N and m:
        d_rows = rows if rows_dev else DeviceArray.from_host(rows, device)
        if per_row:
            d_xs = xs if xs_dev else DeviceArray.from_host(xs, device)
            xs_arg = ctypes.c_void_p(d_xs.ptr)
        else:
            xs_arg = xs.ctypes.data_as(ctypes.c_void_p)
        _lib.check(call_dev(ctypes.c_void_p(d_rows.ptr), N, xs_arg, m, 1 if per_row else 0, ctypes.c_void_p(res.ptr), stream), lib)
        _lib.check(lib.pcx_stream_synchronize(stream), lib)
    if host_out is not None:
        if res.size:
            host_out[...] = res.to_host()
        return host_out
    if dev_out is not None:
        return out
    return res if rows_dev else res.to_host()


def validate_targets(targets, N: int, name: str = "targets") -> np.ndarray:
    """The ``(N,)`` float64 targets of an ``invert_batch`` call (a scalar serves every row), checked on the host before
    any launch: one finite value per row."""
    t = np.asarray(targets, dtype=np.float64)
    if t.ndim == 0:
        t = np.full(N, float(t))
    if t.shape != (N,):
        raise ValueError(f"{name} must be a scalar or have shape ({N},), got {t.shape}")
    bad = np.nonzero(~np.isfinite(t))[0]
    if bad.size:
        r = int(bad[0])
        raise ValueError(f"{name} must be finite, got {t[r]} (row {r})")
    return np.ascontiguousarray(t)


def validate_level(level, N: int):
    """The ``level=`` keyword of ``roots`` / ``roots_batch``: None for ``None`` and for the scalar 0.0 (today's path,
    the same launches and bits), else the ``(N,)`` finite float64 levels."""
    if level is None:
        return None
    if np.ndim(level) == 0 and not isinstance(level, (bool, np.bool_)):
        lv = float(level)
        if lv == 0.0:
            return None
    return validate_targets(level, N, "level")


def run_solve(call, lib, n: int, N: int, method: int, width: int | None = None):
    """Run one ``pcx_*_solve_batch`` entry (``call(roots, counts, x, status)`` -> rc) and shape its outputs: method 0
    ``(roots (N, max(n-1, 1)), counts)`` as :func:`run_batch`, method 1 ``(x (N,) float64, status (N,) int32)``."""
    if method == 0:
        W = max(n - 1, 1) if width is None else int(width)
        roots, counts = np.empty((N, W)), np.empty(N, dtype=np.int32)
        _lib.check(call(_lib.p_f64(roots), _lib.p_i32(counts), None, None), lib)
        return roots, counts
    x, status = np.empty(N), np.empty(N, dtype=np.int32)
    _lib.check(call(None, None, _lib.p_f64(x), _lib.p_i32(status)), lib)
    return x, status


def _cheb1d_solve(values, targets, nodes, weights, domain, method: int, device):
    lib = _lib.load()
    v = _lib.f64(np.atleast_2d(values))
    N, n = v.shape
    t = _lib.f64(np.broadcast_to(np.asarray(targets, dtype=np.float64), (N,)))
    nd, wt = _lib.f64(nodes), _lib.f64(weights)
    dev = _lib.default_device() if device is None else int(device)

    def call(r, c, x, s):
        return lib.pcx_cheb1d_solve(dev, n, float(domain[0]), float(domain[1]), _lib.p_f64(nd), _lib.p_f64(wt),
                                    _lib.p_f64(v), _lib.p_f64(t), N, method, r, c, x, s)
    return run_solve(call, lib, n, N, method)


def cheb1d_level_roots(values, levels, nodes, weights, domain, device: int | None = None):
    """``pcx_cheb1d_solve``, method 0, on given fibres: ``(roots, counts)`` of ``values - levels[:, None]``, the
    subtraction made on the device."""
    return _cheb1d_solve(values, levels, nodes, weights, domain, 0, device)


def cheb1d_invert(values, targets, nodes, weights, domain, device: int | None = None):
    """``pcx_cheb1d_solve``, method 1, on given fibres: ``values`` (N, n) at the ascending ``nodes`` of ``domain``,
    one target per row -> ``(x (N,), status (N,))`` as :func:`invert_1d` defines them."""
    return _cheb1d_solve(values, targets, nodes, weights, domain, 1, device)


def merge_inversions(x, status):
    """Join the inversions of the pieces of a spline along one dimension (the NumPy restatement of
    ``k_spline_invert_merge``): ``x`` and ``status`` are ``(P, N)``, piece by piece in order.  The lowest ``x`` of the
    pieces with ``status > 0`` and the sum of their statuses; a -1 in any piece makes the row -1 and NaN; no piece
    with a solution gives ``(NaN, 0)``."""
    x, status = np.atleast_2d(np.asarray(x, dtype=float)), np.atleast_2d(np.asarray(status))
    found = status > 0
    out_s = np.where(found, status, 0).sum(axis=0).astype(np.int32)
    with np.errstate(invalid="ignore"):
        out_x = np.where(found, x, np.inf).min(axis=0)
    out_x = np.where(out_s > 0, out_x, np.nan)
    failed = (status < 0).any(axis=0)
    return np.where(failed, np.nan, out_x), np.where(failed, np.int32(-1), out_s).astype(np.int32)


def run_batch(call, lib, n: int, N: int, mode: int, width: int | None = None):
    """Run one ``pcx_*_calculus_batch`` entry (``call(roots, counts, val, loc)`` -> rc) and shape its outputs:
    mode 0 ``(roots (N, max(n-1, 1)), counts)``, modes 1 and 2 ``(values, locations, counts)``.  ``width`` replaces the
    roots' column count where it is not that of one fibre (a spline: the sum over its pieces)."""
    W = max(n - 1, 1) if width is None else int(width)
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


def merge_pieces(mode: str, found, domain=None, counts=None):
    """Join the results of the pieces of a spline along one dimension, given in piece order (reference
    spline.py:1762-1910; the NumPy restatement of ``k_spline_calc_merge``).  ``counts``, when given, holds each piece's
    solver count: a -1 raises ``LinAlgError``, as the piece's own single call does.

    ``"roots"``: ``found`` holds one ascending array per piece.  The arrays are concatenated -- the pieces are ordered and
    a piece's roots lie in its own interval -- and an element is kept when it is the first or exceeds its immediate
    predecessor, kept or not, by more than ``1e-10 (|b - a| + 1)`` (``domain = (a, b)`` of the spline along the
    dimension).  ``"min"`` / ``"max"``: ``found`` holds one ``(value, location)`` per piece; the result starts at
    ``(+-inf, 0.0)`` and a piece replaces it only when strictly better, so the first of equal pieces wins."""
    if counts is not None and any(int(c) < 0 for c in counts):
        raise np.linalg.LinAlgError("fibre is not finite or the eigenvalue iteration did not converge")
    if mode == "roots":
        out = np.concatenate([np.asarray(r, dtype=float).ravel() for r in found]) if len(found) else np.array([], dtype=float)
        if out.size > 1:
            scale = abs(domain[1] - domain[0]) + 1
            out = out[np.concatenate([[True], np.diff(out) > 1e-10 * scale])]
        return out
    best = (float("inf") if mode == "min" else float("-inf"), 0.0)
    for val, loc in found:
        if (val < best[0]) if mode == "min" else (val > best[0]):
            best = (float(val), float(loc))
    return best


# ---------------------------------------------------------------------------------------------- host restatement
def roots_1d(values: np.ndarray, domain) -> np.ndarray:
    """Real roots in ``domain`` of the interpolant through ``values`` at ascending type-I nodes (reference
    ``_roots_1d``): ``chebroots`` of the coefficients, |imag| < 1e-10, inside [-1, 1] up to 1e-10, mapped, sorted,
    near-duplicates (``1e-10 (b - a + 1)``) dropped.  An eigenvalue within 1e-10 of +-1, on either side, is that end
    and gives exactly ``a`` or ``b``; the reference clips only from outside, which leaves a root at an end a few ulp
    inside it as often as not."""
    from numpy.polynomial.chebyshev import chebroots

    from .barycentric import ChebyshevApproximation
    coeffs = ChebyshevApproximation._chebyshev_coefficients_1d(values)
    raw = chebroots(coeffs)
    tol = 1e-10
    keep = np.array([r.real for r in np.atleast_1d(raw)
                     if abs(r.imag) < tol and -1.0 - tol <= r.real <= 1.0 + tol], dtype=float)
    if not keep.size:
        return np.array([], dtype=float)
    a, b = domain
    physical = 0.5 * (a + b) + 0.5 * (b - a) * keep
    physical[keep >= 1.0 - tol] = b
    physical[keep <= tol - 1.0] = a
    physical = np.sort(physical)
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


INVERT_MAX_ITERS = 192       # INV_MAX_ITERS of csrc/invert_kernels.h: 3 steps per halving, 63 halvings to the floor
INVERT_FLOOR = 2.0 ** -10    # INV_FLOOR: the bracket stops at INVERT_FLOOR eps max(|lo|, |hi|)


def _bary_rows(V, nodes, weights, x):
    """p_r(x_r) for the rows of ``V`` (R, n): the barycentric formula as ``inv_eval`` forms it -- a sequential sum over
    j = 0 .. n-1, the first node within 1e-14 gives its value.  Vectorised over rows only, so every row sees the
    operations of the scalar routine in their order."""
    R, n = V.shape
    num, den = np.zeros(R), np.zeros(R)
    exact = np.full(R, -1)
    for j in range(n):
        dx = x - nodes[j]
        hit = np.abs(dx) < 1e-14
        exact = np.where(hit & (exact < 0), j, exact)
        t = weights[j] / np.where(hit, 1.0, dx)
        num = np.where(hit, num, num + t * V[:, j])
        den = np.where(hit, den, den + t)
    return np.where(exact >= 0, V[np.arange(R), np.maximum(exact, 0)], num / den)


def invert_rows(values, nodes, weights, domain, targets, return_iterations: bool = False):
    """The NumPy restatement of ``inv_solve`` (``csrc/invert_kernels.h``) on the rows of ``values`` (R, n), one target
    per row -> ``(x (R,) float64, status (R,) int32)``, and the evaluations each row spent inside its bracket when
    ``return_iterations``.  Every row goes through the scalar routine's operations in their order (explicit sequential
    sums; rows are independent lanes of the vector statements), so ``status`` and ``x`` are the device's.

    Knots ``s_0 = lo, s_1 .. s_n`` the ascending nodes, ``s_(n+1) = hi``; ``g_i = p(s_i) - t`` (the values themselves
    at the nodes).  Segment ``i`` brackets when ``g_i == 0`` or ``g_i`` and ``g_(i+1)`` have opposite signs; a
    ``g_(n+1) == 0`` counts as one more.  ``status`` is the number of bracketing segments (0: the target is not
    reached on the knots, ``x`` NaN; > 1: ``x`` is the lowest), -1 with ``x`` NaN when the fibre or the target is not
    finite or the iteration cap :data:`INVERT_MAX_ITERS` was reached.  ``x = s_i`` exactly when ``g_i == 0``, else the
    root inside the lowest bracketing segment: Illinois secant steps kept ``4 eps max(|a|, |b|)`` inside the bracket,
    a midpoint when the bracket is narrower than twice that or two steps in a row failed to halve it, until
    ``g(x) == 0`` or the bracket's ends are adjacent doubles (then the end with the smaller ``|g|``).  Stop and
    distance carry the floor ``flo = INVERT_FLOOR eps max(|lo|, |hi|)``: the bracket also stops at ``b - a <= flo``, so
    a root at or near 0 in a domain that contains 0 does not ask for a bracket down to the subnormals; a root with
    ``|x| >= 2^-9 max(|lo|, |hi|)`` still ends at adjacent doubles.  A constant fibre equal to its target gives
    ``status = n + 2`` and ``x = lo`` when the barycentric sums at the two ends return the constant itself (a power of
    two or zero; another constant may round there, and status is then n to n + 2 with ``x = lo`` or the first node)."""
    V = np.atleast_2d(np.asarray(values, dtype=float))
    R, n = V.shape
    nodes, weights = np.asarray(nodes, dtype=float), np.asarray(weights, dtype=float)
    t = np.broadcast_to(np.asarray(targets, dtype=float), (R,)).copy()
    lo, hi = float(domain[0]), float(domain[1])
    eps = float(np.finfo(float).eps)
    flo = INVERT_FLOOR * eps * max(abs(lo), abs(hi))
    x_out = np.full(R, np.nan)
    iters = np.zeros(R, dtype=np.int32)
    with np.errstate(all="ignore"):
        finite = np.isfinite(t) & np.isfinite(V).all(axis=1)
        count = np.zeros(R, dtype=np.int32)
        exact = np.zeros(R, dtype=bool)
        a, b, ga, gb = np.zeros(R), np.zeros(R), np.zeros(R), np.zeros(R)
        sp, gp = np.full(R, lo), _bary_rows(V, nodes, weights, np.full(R, lo)) - t
        for i in range(n + 1):
            sn = np.full(R, nodes[i] if i < n else hi)
            gn = V[:, i] - t if i < n else _bary_rows(V, nodes, weights, np.full(R, hi)) - t
            zero = gp == 0.0
            br = zero | ((gp < 0.0) & (gn > 0.0)) | ((gp > 0.0) & (gn < 0.0))
            first = br & (count == 0)
            a, b, ga, gb = np.where(first, sp, a), np.where(first, sn, b), np.where(first, gp, ga), np.where(first, gn, gb)
            exact = np.where(first, zero, exact)
            count = count + br
            sp, gp = sn, gn
        endz = gp == 0.0
        first = endz & (count == 0)
        a = np.where(first, sp, a)
        exact = np.where(first, True, exact)
        count = count + endz
        status = np.where(finite, count, -1).astype(np.int32)
        found = finite & (count > 0)
        x_out = np.where(found & exact, a, x_out)
        idx = np.nonzero(found & ~exact)[0]
        if idx.size:
            Vi, ti = V[idx], t[idx]
            a, b, ga, gb = a[idx], b[idx], ga[idx], gb[idx]
            fa, fb = ga.copy(), gb.copy()
            side, slow, creep = (np.zeros(idx.size, dtype=int) for _ in range(3))
            live = np.ones(idx.size, dtype=bool)
            xo, its = np.full(idx.size, np.nan), np.zeros(idx.size, dtype=np.int32)
            for _ in range(INVERT_MAX_ITERS):
                if not live.any():
                    break
                w = b - a
                m = a + 0.5 * w
                adj = live & (~((a < m) & (m < b)) | ~(w > flo))
                xo = np.where(adj, np.where(np.abs(ga) <= np.abs(gb), a, b), xo)
                live = live & ~adj
                tol = np.ldexp(np.maximum(4.0 * eps * np.maximum(np.abs(a), np.abs(b)), flo), creep)
                xc = b - fb * (w / (fb - fa))
                bis = (slow >= 2) | ~(w > 2.0 * tol)
                near_a, near_b = ~(xc > a + tol), ~(xc < b - tol)
                xc = np.where(near_a, a + tol, xc)
                near_b = near_b & ~near_a
                xc = np.where(near_b, b - tol, xc)
                inside = (a < xc) & (xc < b)
                xn = np.where(bis | ~inside, m, xc)
                pushed = np.where(bis | ~inside, 0, np.where(near_a, -1, np.where(near_b, 1, 0)))
                slow = np.where(bis, 0, slow)
                gx = _bary_rows(Vi, nodes, weights, xn) - ti
                its = its + live
                hit = live & (gx == 0.0)
                xo = np.where(hit, xn, xo)
                live = live & ~hit
                left = live & ((gx < 0.0) == (ga < 0.0))
                right = live & ~left
                fb = np.where(left & (side == -1), fb * 0.5, fb)
                fa = np.where(right & (side == 1), fa * 0.5, fa)
                a, ga, fa = np.where(left, xn, a), np.where(left, gx, ga), np.where(left, gx, fa)
                b, gb, fb = np.where(right, xn, b), np.where(right, gx, gb), np.where(right, gx, fb)
                side = np.where(left, -1, np.where(right, 1, side))
                crept = (left & (pushed == -1)) | (right & (pushed == 1))
                creep = np.where(live, np.where(crept, creep + 1, np.where(pushed == 0, creep, 0)), creep)
                slow = np.where(live, np.where((b - a) > 0.5 * w, slow + 1, 0), slow)
            x_out[idx] = np.where(live, np.nan, xo)
            status[idx] = np.where(live, -1, status[idx])
            iters[idx] = its
    if return_iterations:
        return x_out, status, iters
    return x_out, status


def invert_1d(values, nodes, weights, domain, target):
    """One fibre: ``(x, status)`` of :func:`invert_rows` as a float and an int."""
    x, status = invert_rows(np.asarray(values, dtype=float)[None, :], nodes, weights, domain, [target])
    return float(x[0]), int(status[0])


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


def run_single_level(fibre_fn, solve_fn, n: int, level: np.ndarray, domain):
    """``roots(level=)`` as a single call: the one-row ``pcx_*_solve_batch`` (``solve_fn()``, method 0) up to
    :data:`MAX_DEVICE_N` nodes, else the host restatement on the device-evaluated fibre minus the level."""
    if n <= MAX_DEVICE_N:
        return single_roots(*solve_fn())
    return roots_1d(np.asarray(fibre_fn(), dtype=float) - float(level[0]), domain)


# ---------------------------------------------------------------------------------------------- the front end
class FibreCalculusMixin:
    """The operations along one dimension of the four model classes: ``roots`` / ``minimize`` / ``maximize``, their
    ``_batch`` forms, ``invert_batch``, ``fibre_batch`` and the driver of ``ladder_batch``.  Needs ``num_dimensions``,
    ``domain``, ``n_nodes`` and ``_built`` on the host class, and:

    * ``_fibre_prefix``: the prefix of the class's C entries (``"pcx_bary"``, ``"pcx_spline"``, ``"pcx_slider"``,
      ``"pcx_tt"``); ``_ladder_own_stream``: whether its ladder runs on the stream ``<prefix>_stream`` reports (dense,
      TT) or on the handle's own streams (the composites: the null stream is passed);
    * ``_fibre_grid(dim)`` -> ``(nodes, weights, diff, (a, b))`` of a dimension and ``_fibre_values(points)``, the model
      without a derivative at ``(n, d)`` points -- what a single call above 64 nodes finishes on the host with.

    A class overrides, where its own differ: ``_fibre_check_built()`` (default: ``_built``), ``_fibre_domain()`` and
    ``_fibre_counts()`` (domain and node counts by user dimension; default ``domain`` / ``n_nodes``),
    ``_fibre_handle()`` (default ``_dev()``), ``_domain_arrays()`` (what the two solver entries take between ``dim``
    and the rows; default the domain's ends) and ``_fibre_shape(dim)`` (``(n, width)`` of the batch results).  The
    public methods reach the device through ``self._calculus_batch`` / ``self._solve_batch`` only."""

    _ladder_own_stream = False

    # ------------------------------------------------------------ hooks
    def _fibre_check_built(self) -> None:
        if not self._built:
            raise RuntimeError("Call build() first")

    def _fibre_domain(self):
        return self.domain

    def _fibre_counts(self):
        return self.n_nodes

    def _fibre_handle(self):
        return self._dev()

    def _domain_arrays(self):
        """The leading arguments of the two solver entries, between ``dim`` and the rows: the domain's lower and upper
        ends by dimension; empty for the TT, whose handle knows its domain."""
        dom = np.asarray(self.domain, dtype=float)
        return _lib.f64(dom[:, 0]), _lib.f64(dom[:, 1])

    def _fibre_shape(self, dim: int):
        return int(self._fibre_counts()[dim]), None

    def _fibre_nodes(self, dim: int) -> np.ndarray:
        """The values ``fibre_batch`` takes the ladder at."""
        return np.asarray(self._fibre_grid(dim)[0], dtype=float)

    # ------------------------------------------------------------ the two device entries
    def _calculus_batch(self, dim: int, rows: np.ndarray, mode: int):
        """``<prefix>_calculus_batch`` over validated rows (see :func:`run_batch`)."""
        n, width = self._fibre_shape(dim)
        h = self._fibre_handle()
        entry = getattr(h.lib, self._fibre_prefix + "_calculus_batch")
        lead = self._domain_arrays()
        rows = _lib.f64(rows)
        N = rows.shape[0]

        def call(r, c, v, loc):
            return entry(h.handle, int(dim), *map(_lib.p_f64, lead), _lib.p_f64(rows), N, mode, r, c, v, loc)
        return run_batch(call, h.lib, n, N, mode, width=width)

    def _solve_batch(self, dim: int, rows: np.ndarray, targets: np.ndarray, method: int):
        """``<prefix>_solve_batch`` over validated rows and targets (see :func:`run_solve`)."""
        n, width = self._fibre_shape(dim)
        h = self._fibre_handle()
        entry = getattr(h.lib, self._fibre_prefix + "_solve_batch")
        lead = self._domain_arrays()
        rows, targets = _lib.f64(rows), _lib.f64(targets)
        N = rows.shape[0]

        def call(r, c, x, s):
            return entry(h.handle, int(dim), *map(_lib.p_f64, lead), _lib.p_f64(rows), _lib.p_f64(targets), N, method,
                         r, c, x, s)
        return run_solve(call, h.lib, n, N, method, width=width)

    # ------------------------------------------------------------ single calls
    def _single_args(self, dim, fixed):
        """A single call's validated ``dim``, its one batch row, the node count along ``dim``, the device-evaluated
        fibre for the host finish (a callable) and that dimension's grid."""
        self._fibre_check_built()
        d = self.num_dimensions
        dim, params = validate_calculus_args(d, dim, fixed, self._fibre_domain())
        row = fixed_row(d, dim, params)
        grid = self._fibre_grid(dim)
        return dim, row, int(self._fibre_counts()[dim]), lambda: self._fibre_values(fibre_points(d, dim, row, grid[0])), grid

    def _calculus(self, dim, fixed, mode: str):
        dim, row, n, fibre, grid = self._single_args(dim, fixed)
        return run_single(fibre, lambda m: self._calculus_batch(dim, row, m), n, mode, *grid)

    def _level_roots(self, dim, fixed, level: np.ndarray) -> np.ndarray:
        dim, row, n, fibre, grid = self._single_args(dim, fixed)
        return run_single_level(fibre, lambda: self._solve_batch(dim, row, level, 0), n, level, grid[3])

    def roots(self, dim=None, fixed=None, *, level=0.0) -> np.ndarray:
        """Sorted real roots along ``dim`` with every other dimension fixed (``fixed = {dim_index: value}``) by the
        colleague-matrix method.  The fibre is evaluated and solved on the device; above 64 nodes the solve runs on the
        host (NumPy ``chebroots``).  A non-finite fibre raises ``numpy.linalg.LinAlgError``.  Unlike the reference, which
        clips from outside only, a root within ``1e-10`` (of the half-width) of an end of the domain along ``dim``, on
        either side of it, is returned as exactly that end; the batched forms and the critical points of
        :meth:`minimize` / :meth:`maximize` follow the same rule.

        ``level`` (keyword only, a finite scalar) asks for the solutions of ``p = level`` instead: the level is
        subtracted from the fibre on the device, one rounding per value, before the same solver.  ``None`` or ``0.0``
        is the call without a level, the same launches and bits."""
        lv = validate_level(level, 1)
        if lv is None:
            return self._calculus(dim, fixed, "roots")
        return self._level_roots(dim, fixed, lv)

    def minimize(self, dim=None, fixed=None):
        """``(value, location)`` of the minimum along ``dim``: the roots of the derivative series and the two ends are
        the candidates, the first smallest value wins.  A critical point within ``1e-10`` of an end is that end (see
        :meth:`roots`)."""
        return self._calculus(dim, fixed, "min")

    def maximize(self, dim=None, fixed=None):
        """``(value, location)`` of the maximum along ``dim``, as :meth:`minimize`."""
        return self._calculus(dim, fixed, "max")

    # ------------------------------------------------------------ batches
    def _calculus_rows(self, dim, fixed) -> np.ndarray:
        self._fibre_check_built()
        return validate_batch_args(self.num_dimensions, dim, fixed, self._fibre_domain(), self._fibre_counts())

    def roots_batch(self, dim: int, fixed, *, level=None):
        """Roots along ``dim`` for every row of ``fixed`` (host float64 ``(N, d-1)``: the other dimensions in
        increasing order), in one device pass (extension).  Returns ``(roots, counts)``: ``roots`` float64
        ``(N, max(n_dim-1, 1))`` ascending and NaN-padded, ``counts`` int32 ``(N,)``, -1 where the fibre was not finite
        or the eigenvalue iteration failed.  At most 64 nodes along ``dim``.

        ``level`` (keyword only, a finite scalar or an ``(N,)`` array, one level per row) asks for the solutions of
        ``p = level`` instead: the level is subtracted from the fibre on the device, one rounding per value, before the
        same solver.  ``None`` or ``0.0`` is the call without a level, the same launches and bits."""
        rows = self._calculus_rows(dim, fixed)
        lv = validate_level(level, rows.shape[0])
        if lv is None:
            return self._calculus_batch(int(dim), rows, 0)
        return self._solve_batch(int(dim), rows, lv, 0)

    def invert_batch(self, dim: int, fixed, targets):
        """The value of dimension ``dim`` at which the model equals each row's target (extension; the class's
        ``pcx_bary_solve_batch`` / ``pcx_spline_solve_batch`` / ``pcx_slider_solve_batch`` / ``pcx_tt_solve_batch``,
        method 1): ``fixed`` as in :meth:`roots_batch`, ``targets`` a finite scalar or ``(N,)`` array.  Returns
        ``(x (N,) float64, status (N,) int32)``.  On the knots ``[lo, nodes..., hi]`` of the fibre
        a segment brackets when the value at its lower knot equals the target or ``p - target`` changes sign across it;
        ``status`` is the number of bracketing segments: ``0`` the target is not reached on the knots (``x`` NaN),
        ``1`` unique on the knots, ``> 1`` not unique (``x`` is the lowest), ``-1`` the fibre is not finite or the
        solver's fixed iteration cap was reached (``x`` NaN).  ``x`` is the knot itself where the value equals the
        target there, else the root inside the lowest bracketing segment, down to adjacent doubles.  A constant fibre
        equal to its target gives ``status = n + 2`` and ``x = lo`` when the sums at the two ends return the constant
        itself (a power of two, zero), else n to n + 2.  A root closer to 0 than ``2^-9 max(|lo|, |hi|)`` is returned to
        within ``2^-10 eps max(|lo|, |hi|)``, not to adjacent doubles.  Only crossings between knots are seen: two
        solutions inside one node interval are invisible here, and ``roots_batch(level=)`` finds them.  At most 64
        nodes along ``dim``.  One device lane solves one row (``csrc/invert_kernels.h``)."""
        rows = self._calculus_rows(dim, fixed)
        return self._solve_batch(int(dim), rows, validate_targets(targets, rows.shape[0]), 1)

    def minimize_batch(self, dim: int, fixed):
        """``(values, locations)``, float64 ``(N,)``, of the minimum along ``dim`` for every row of ``fixed``
        (extension; arguments as :meth:`roots_batch`).  NaN where a row failed."""
        rows = self._calculus_rows(dim, fixed)
        val, loc, _ = self._calculus_batch(int(dim), rows, 1)
        return val, loc

    def maximize_batch(self, dim: int, fixed):
        """``(values, locations)`` of the maximum along ``dim`` for every row of ``fixed`` (extension)."""
        rows = self._calculus_rows(dim, fixed)
        val, loc, _ = self._calculus_batch(int(dim), rows, 2)
        return val, loc

    # ------------------------------------------------------------ ladders and fibres
    def _ladder_orders(self, derivative_order, derivative_id):
        """The derivative orders of a ladder call: no spec at all is the value."""
        if derivative_order is None and derivative_id is None:
            return [0] * self.num_dimensions
        return self._resolve_derivative_args(derivative_order, derivative_id)

    def _ladder(self, dim, fixed, xs, out, orders=None):
        """``ladder_batch`` over resolved derivative ``orders`` (None: the class's entries take no spec): every check
        before the model goes to a device, then ``<prefix>_ladder_batch`` / ``_dev`` through :func:`run_ladder`."""
        import ctypes
        self._fibre_check_built()
        d = self.num_dimensions
        rows = validate_fibre_args(d, dim, fixed, self._fibre_domain())
        spec = ()
        if orders is not None:
            arr = np.asarray(orders)
            if arr.shape != (d,):
                raise ValueError(f"derivative_order must have {d} entries, got {list(np.shape(orders))}")
            arr = _lib.i32(arr)
            spec = (_lib.p_i32(arr),)
        xv, m, per_row = validate_ladder_xs(xs, rows.shape[0])
        validate_ladder_out(out, (rows.shape[0], m))                    # refused before the model goes to a device
        s = self._fibre_handle()
        lib, h, dim = s.lib, s.handle, int(dim)
        st = ctypes.c_void_p()                                          # null: the composites run on their handle's streams
        if self._ladder_own_stream:
            _lib.check(getattr(lib, self._fibre_prefix + "_stream")(h, ctypes.byref(st)), lib)
        host, dev = (getattr(lib, self._fibre_prefix + name) for name in ("_ladder_batch", "_ladder_batch_dev"))
        return run_ladder(
            lib, s.device, st,
            lambda f, N, x, mm, pr, o: host(h, dim, *spec, f, N, x, mm, pr, o),
            lambda f, N, x, mm, pr, o, stream: dev(h, dim, *spec, f, N, x, mm, pr, o, stream),
            rows, xv, m, per_row, out)

    def fibre_batch(self, dim: int, fixed, derivative_order=None, *, derivative_id=None, out=None):
        """Every row's restriction to ``dim`` at that dimension's own nodes (ascending), ``(N, n_dim)``:
        :meth:`ladder_batch` at those nodes, bit for bit."""
        self._fibre_check_built()
        validate_dim(self.num_dimensions, dim)
        return self.ladder_batch(dim, fixed, self._fibre_nodes(int(dim)), derivative_order, derivative_id=derivative_id,
                                 out=out)


# ---------------------------------------------------------------------------------------------- box integrals
def box_rows(d: int, domain, dims, bounds, points):
    """Validated arguments of an ``integrate_batch`` call on a ``d``-dimensional model over ``domain`` -> (flags by
    dimension, rows ``(N, d + m)``): ``bounds`` broadcast to ``(N, m, 2)`` and clipped to the domain, ``points``
    ``(N, d - m)``, both in increasing dimension order.  A row holds, per dimension, the coordinate of a kept
    dimension or ``lo, hi`` of an integrated one (``pcx_bary_box_batch`` / ``pcx_tt_box_batch``).  Raises before any
    device call."""
    if dims is None:
        dims = list(range(d))
    elif isinstance(dims, (int, np.integer)):
        dims = [int(dims)]
    else:
        dims = sorted(set(int(v) for v in dims))
    if any(u < 0 or u >= d for u in dims):
        raise ValueError(f"dims contains out-of-range index (num_dimensions={d}, dims={dims})")
    m = len(dims)
    if m < 1:
        raise ValueError("dims must name at least one dimension")
    udom = np.asarray(domain, dtype=float)
    kept = [u for u in range(d) if u not in dims]
    n_rows = []
    if bounds is None:
        bnd = udom[dims][None, :, :]
    else:
        bnd = np.asarray(bounds, dtype=float)
        if m == 1 and bnd.ndim == 1:
            bnd = bnd[None, :]
        if bnd.ndim == 2 and bnd.shape == (m, 2):
            bnd = bnd[None, :, :]
        elif m == 1 and bnd.ndim == 2 and bnd.shape[1] == 2:
            bnd = bnd[:, None, :]
        if bnd.ndim != 3 or bnd.shape[1:] != (m, 2):
            raise ValueError(f"bounds must broadcast to (N, {m}, 2), got shape {np.shape(bounds)}")
        if bnd.shape[0] != 1:
            n_rows.append(("bounds", bnd.shape[0]))
    if points is None:
        if kept:
            raise ValueError(f"points is required: {len(kept)} dimensions are kept")
        pts = None
    else:
        pts = np.asarray(points, dtype=float)
        if pts.ndim != 2 or pts.shape[1] != len(kept):
            raise ValueError(f"points must have shape (N, {len(kept)}), got {pts.shape}")
        n_rows.append(("points", pts.shape[0]))
    if len(n_rows) == 2 and n_rows[0][1] != n_rows[1][1]:
        raise ValueError(f"bounds has {n_rows[0][1]} rows but points has {n_rows[1][1]}")
    N = n_rows[0][1] if n_rows else 1
    bnd = np.broadcast_to(bnd, (N, m, 2))
    lo, hi = bnd[:, :, 0], bnd[:, :, 1]
    a, b = udom[dims, 0][None, :], udom[dims, 1][None, :]
    bad = (lo > hi) | (lo < a - 1e-14) | (hi > b + 1e-14) | ~np.isfinite(lo) | ~np.isfinite(hi)
    if bad.any():
        r = int(np.argmax(bad.any(axis=1)))
        j = int(np.argmax(bad[r]))
        if lo[r, j] > hi[r, j]:
            raise ValueError(f"bounds lo={lo[r, j]} > hi={hi[r, j]} for dim {dims[j]} (row {r})")
        raise ValueError(f"bounds ({lo[r, j]}, {hi[r, j]}) outside domain [{udom[dims[j], 0]}, {udom[dims[j], 1]}] "
                         f"for dim {dims[j]} (row {r})")
    if pts is not None and pts.size:
        pa, pb = udom[kept, 0][None, :], udom[kept, 1][None, :]
        bad = ~((pts >= pa) & (pts <= pb))
        if bad.any():
            r = int(np.argmax(bad.any(axis=1)))
            j = int(np.argmax(bad[r]))
            raise ValueError(f"point value {pts[r, j]} for dim {kept[j]} is outside domain "
                             f"[{udom[kept[j], 0]}, {udom[kept[j], 1]}] (row {r})")
    flags = np.zeros(d, dtype=np.int32)
    flags[dims] = 1
    rows = np.empty((N, d + m))
    col = 0
    for u in range(d):
        if flags[u]:
            j = dims.index(u)
            rows[:, col] = np.maximum(lo[:, j], a[0, j])         # clipped to the domain, as integrate() does
            rows[:, col + 1] = np.minimum(hi[:, j], b[0, j])
            col += 2
        else:
            rows[:, col] = pts[:, kept.index(u)]
            col += 1
    return flags, rows


def box_quadrature_matrix(n: int) -> np.ndarray:
    """``Q_n`` of the device box integrals (``csrc/bary_box_kernels.h``): ``Q_n @ mu`` are the sub-interval Fejer-1
    weights at the ``n`` ascending type-I nodes for the moments ``mu_q`` of ``T_q`` over the sub-interval --
    ``Q[j, 0] = 1 / n``, ``Q[j, q] = (2 / n) cos(pi q (2 (n - 1 - j) + 1) / (2 n))`` (the reference's DCT-III,
    reversed)."""
    j = np.arange(n)[:, None]
    q = np.arange(n)[None, :]
    Q = (2.0 / n) * np.cos(np.pi * q * (2 * (n - 1 - j) + 1) / (2.0 * n))
    Q[:, 0] = 1.0 / n
    return Q


def box_moments(n: int, t_lo: float, t_hi: float) -> np.ndarray:
    """``mu_q = F_q(t_hi) - F_q(t_lo)`` for ``q < n`` with the antiderivatives ``F_0 = t``, ``F_1 = t^2 / 2``,
    ``F_q = (T_{q+1} / (q + 1) - T_{q-1} / (q - 1)) / 2``: every ``F_q`` by the same operations at both ends, as the
    device forms them, so ``t_lo == t_hi`` gives exactly zeros."""
    mu = np.zeros(n)
    mu[0] = t_hi - t_lo
    if n > 1:
        mu[1] = 0.5 * (t_hi * t_hi) - 0.5 * (t_lo * t_lo)
    am, ac = t_lo, 2.0 * t_lo * t_lo - 1.0
    bm, bc = t_hi, 2.0 * t_hi * t_hi - 1.0
    for q in range(2, n):
        ap, bp = 2.0 * t_lo * ac - am, 2.0 * t_hi * bc - bm
        c1, c2 = 1.0 / (q + 1), 1.0 / (q - 1)
        mu[q] = 0.5 * (bp * c1 - bm * c2) - 0.5 * (ap * c1 - am * c2)
        am, ac = ac, ap
        bm, bc = bc, bp
    return mu


def box_weights(n: int, a: float, b: float, lo: float, hi: float) -> np.ndarray:
    """Host restatement of ``box_weights_1d``: the weight vector of an integrated dimension with ``n`` nodes on
    ``[a, b]`` for the sub-interval ``[lo, hi]``, ``(b - a) / 2 . Q_n mu``."""
    scale = 2.0 / (b - a)
    return 0.5 * (b - a) * (box_quadrature_matrix(n) @ box_moments(n, (lo - a) * scale - 1.0, (hi - a) * scale - 1.0))
