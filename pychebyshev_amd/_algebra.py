"""Arithmetic on interpolants: the operand checks shared by the operators of the four classes, the operators
of the three classes that hold value tensors (:class:`ValueAlgebraMixin`), the block-diagonal stacking of two
tensor trains, and the device calls that round a tensor train (``pcx_tt_round``) or swap its storage axes
(``pcx_tt_reorder``).

Dense, spline and slider operators combine value tensors with NumPy on the host: the result is a new
interpolant whose device model is built on its first evaluation, so the intermediate results of a chain
never reach the GPU.  A tensor-train sum has ranks ``r_a + r_b`` until it is rounded; the rounding runs
on the device.
"""
from __future__ import annotations

import ctypes
import itertools
import operator

import numpy as np

from . import _lib


def is_scalar(value) -> bool:
    """Python and NumPy integers and floats count as scalars; nothing else does."""
    return isinstance(value, (int, float, np.integer, np.floating))


def check_compatible(a, b) -> None:
    """Raise unless ``a`` and ``b`` can be added: same type, both built, same dimensions, node counts,
    domain (to ``allclose``) and ``max_derivative_order``."""
    if type(a) is not type(b):
        raise TypeError(f"Cannot combine {type(a).__name__} with {type(b).__name__}; "
                        f"operands must be the same type.")
    for side, obj in (("Left", a), ("Right", b)):
        if getattr(obj, "tensor_values", None) is None and not getattr(obj, "_built", False):
            raise RuntimeError(f"{side} operand is not built. Call build() first.")
    if a.num_dimensions != b.num_dimensions:
        raise ValueError(f"Dimension mismatch: {a.num_dimensions} vs {b.num_dimensions}")
    if not np.array_equal(np.asarray(a.n_nodes, dtype=int), np.asarray(b.n_nodes, dtype=int)):
        raise ValueError(f"Node count mismatch: {a.n_nodes} vs {b.n_nodes}")
    if not np.allclose(np.asarray(a.domain, dtype=float), np.asarray(b.domain, dtype=float)):
        raise ValueError(f"Domain mismatch: {a.domain} vs {b.domain}")
    if a.max_derivative_order != b.max_derivative_order:
        raise ValueError(f"max_derivative_order mismatch: {a.max_derivative_order} vs {b.max_derivative_order}")


def leaves(other, attr: str):
    """What pairs with a composite's leaves in an operator: ``other``'s own leaves (``attr``), or the scalar itself
    for each."""
    return getattr(other, attr) if hasattr(other, attr) else itertools.repeat(other)


class ValueAlgebraMixin:
    """The ten arithmetic operators of the classes that hold value tensors (dense, spline, slider; reference
    barycentric.py:2433-2500, spline.py:1912-2010, slider.py:1285-1390).  The host class supplies

    * ``_check_operand(other)``: its compatibility check (default :func:`check_compatible`);
    * ``_leafwise(op, other)``: a new object with ``op(a, b)`` on every value tensor ``a`` -- ``b`` is the matching
      tensor of ``other``, or ``other`` itself when it is a float;
    * ``_leafwise_inplace(op, other)``: the same in place.  It rebinds ``tensor_values`` to a new array and clears
      ``_cached_error_estimate`` on the leaves and the owner: the device copies recognise staleness by the identity of
      that array, so it is never modified in place.

    ``op`` is ``operator.add``, ``operator.sub`` or ``operator.mul`` (with ``float(scalar)``)."""

    _check_operand = check_compatible

    def __add__(self, other):
        if type(self) is not type(other):
            return NotImplemented
        self._check_operand(other)
        return self._leafwise(operator.add, other)

    def __sub__(self, other):
        if type(self) is not type(other):
            return NotImplemented
        self._check_operand(other)
        return self._leafwise(operator.sub, other)

    def __mul__(self, scalar):
        if not is_scalar(scalar):
            return NotImplemented
        return self._leafwise(operator.mul, float(scalar))

    def __rmul__(self, scalar):
        return self.__mul__(scalar)

    def __truediv__(self, scalar):
        if not is_scalar(scalar):
            return NotImplemented
        return self.__mul__(1.0 / float(scalar))

    def __neg__(self):
        return self.__mul__(-1.0)

    def __iadd__(self, other):
        self._check_operand(other)
        self._leafwise_inplace(operator.add, other)
        return self

    def __isub__(self, other):
        self._check_operand(other)
        self._leafwise_inplace(operator.sub, other)
        return self

    def __imul__(self, scalar):
        if not is_scalar(scalar):
            return NotImplemented
        self._leafwise_inplace(operator.mul, float(scalar))
        return self

    def __itruediv__(self, scalar):
        if not is_scalar(scalar):
            return NotImplemented
        return self.__imul__(1.0 / float(scalar))


# --------------------------------------------------------------------------------------
# tensor trains
# --------------------------------------------------------------------------------------

def tt_stack(cores_a, cores_b):
    """Cores of ``a + b``, exact: the first cores side by side along the right rank, the last ones stacked along the
    left rank, the inner ones block-diagonal.  A single core has both boundary ranks 1, so for ``d == 1`` the
    coefficients are added instead."""
    d = len(cores_a)
    if d == 1:
        return [np.asarray(cores_a[0], dtype=float) + np.asarray(cores_b[0], dtype=float)]
    out = []
    for k, (a, b) in enumerate(zip(cores_a, cores_b)):
        if k == 0:
            out.append(np.concatenate([a, b], axis=2))
        elif k == d - 1:
            out.append(np.concatenate([a, b], axis=0))
        else:
            c = np.zeros((a.shape[0] + b.shape[0], a.shape[1], a.shape[2] + b.shape[2]))
            c[:a.shape[0], :, :a.shape[2]] = a
            c[a.shape[0]:, :, a.shape[2]:] = b
            out.append(c)
    return out


def _shape_args(cores):
    n = _lib.i32([c.shape[1] for c in cores])
    ranks = _lib.i32([1] + [c.shape[2] for c in cores])
    cat = _lib.f64(np.concatenate([np.asarray(c, dtype=float).ravel() for c in cores]))
    return n, ranks, cat


def _split(flat, n, ranks):
    cores, off = [], 0
    for k in range(len(n)):
        size = int(ranks[k]) * int(n[k]) * int(ranks[k + 1])
        cores.append(flat[off:off + size].reshape(int(ranks[k]), int(n[k]), int(ranks[k + 1])).copy())
        off += size
    return cores


def tt_round(cores, max_rank: int, tol: float, device: int):
    """Round a tensor train on the device (``pcx_tt_round``): right-to-left orthogonalisation, then a
    left-to-right truncated-SVD sweep with the reference's rank rule.  Returns the new cores; cores
    ``0 .. d-2`` are left-orthonormal."""
    lib = _lib.load()
    n, ranks, cat = _shape_args(cores)
    out = np.empty(cat.size)
    ranks_out = np.empty(len(cores) + 1, dtype=np.int32)
    length, sweeps = ctypes.c_int64(0), ctypes.c_int32(0)
    _lib.check(lib.pcx_tt_round(int(device), len(cores), _lib.p_i32(n), _lib.p_i32(ranks), _lib.p_f64(cat),
                                int(max_rank), float(tol), _lib.p_i32(ranks_out), _lib.p_f64(out), out.size,
                                ctypes.byref(length), ctypes.byref(sweeps)), lib)
    return _split(out, n, ranks_out)


def tt_swaps(cores, positions, max_rank: int, tol: float, device: int):
    """Apply adjacent swaps of storage axes on the device (``pcx_tt_reorder``): swap ``p`` exchanges axes
    ``p`` and ``p + 1`` through one truncated SVD of the merged pair.  Returns the new cores."""
    lib = _lib.load()
    d = len(cores)
    n, ranks, cat = _shape_args(cores)
    # capacity: a bond's rank never exceeds max(its rank now, min(max_rank, the node counts on either side))
    big = sorted((int(v) for v in n), reverse=True)
    bound = [1] * (d + 1)
    for k in range(1, d):
        side = min(int(np.prod(big[:k], dtype=float)), int(np.prod(big[:d - k], dtype=float)))
        bound[k] = max(int(ranks[k]), min(int(max_rank), side))
    cap = sum(bound[k] * big[0] * bound[k + 1] for k in range(d))
    out = np.empty(max(cap, cat.size))
    n_out = np.empty(d, dtype=np.int32)
    ranks_out = np.empty(d + 1, dtype=np.int32)
    swaps = _lib.i32(list(positions) or [0])
    length, sweeps = ctypes.c_int64(0), ctypes.c_int32(0)
    _lib.check(lib.pcx_tt_reorder(int(device), d, _lib.p_i32(n), _lib.p_i32(ranks), _lib.p_f64(cat), len(positions),
                                  _lib.p_i32(swaps), int(max_rank), float(tol), _lib.p_i32(n_out), _lib.p_i32(ranks_out),
                                  _lib.p_f64(out), out.size, ctypes.byref(length), ctypes.byref(sweeps)), lib)
    return _split(out, n_out, ranks_out)
