"""``ChebyshevTT`` -- Chebyshev interpolant in tensor-train format, evaluated and built
with MI355X kernels through ``libpcx_hip.so``.

Host-side mirror of the reference class (``/root/reference/src/pychebyshev/tensor_train.py``,
v0.21.1) for the hot path:

    build(method="cross") -> _tt_cross                    (:1140-1289, :123-540)
    eval / eval_batch / eval_multi (+ finite differences)  (:2127-2463)
    tt_ranks / compression_ratio / total_build_evals / dim_order, pickle, repr

Division of labour in the TT-Cross build: the Python callback, the evaluation cache,
the NumPy RNG draws (their order defines the result for a given seed) and the index-set
bookkeeping stay on the host, as in the reference; every dense step -- SVD-rank,
maxvol, ``U inv(U[piv])``, the TT chain of the convergence check and the value->coefficient
DCT -- runs on the device (``pcx_tt_cross_step``, ``pcx_tt_grid_eval``,
``pcx_tt_value_to_coeff_core``).  Evaluation (single, batch, finite-difference stencils)
is always a ``pcx_tt_eval_batch`` launch; there is no CPU fallback.

``sobol_indices`` contracts the coefficient cores on the host (NumPy, O(d n r^2): no hot path).
``roots`` / ``minimize`` / ``maximize`` and their batched forms evaluate the fibres and solve them on the device
(``pcx_tt_calculus_batch``).

``+`` / ``-`` stack the cores block-diagonally and round them back on the device (``pcx_tt_round``);
``reorder`` runs its adjacent swaps on the device (``pcx_tt_reorder``); scalars scale core 0 on the host.

``slice`` / ``extrude`` / ``integrate`` / ``inner_product`` contract the coefficient cores on the host (NumPy: a few
``einsum`` calls over cores of a few kilobytes).  ``integrate_batch`` -- the integral over a box that differs per row, at
the row's coordinates in the kept dimensions -- is one launch of the TT chain with the antiderivative basis in the
integrated dimensions (``pcx_tt_box_batch``, ``csrc/tt_box_kernels.h``).

``eval_multi`` / ``eval_multi_batch`` take ``method="analytic"`` for the exact derivatives of the interpolant in place
of the reference's finite differences (the default, unchanged): the same chain with ``T_j``, ``T'_j`` or ``T''_j`` as the
basis of a differentiated dimension, one launch for all rows and specs (``pcx_tt_deriv_batch``,
``csrc/tt_deriv_kernels.h``).  ``differentiate`` returns the derivative as a model: the coefficient-derivative
recurrence on the host cores.  ``gradient_batch`` / ``gradient`` give the value, every first partial derivative and,
on request, every dimension's own second derivative from one forward-backward pass per row (``pcx_tt_grad_batch``,
``csrc/tt_grad_kernels.h``) instead of one chain per spec; ``hessian_batch`` / ``hessian`` add every mixed second
partial from the same sweeps (``pcx_tt_hess_batch``, ``csrc/tt_hess_kernels.h``).

``orth_left`` / ``orth_right`` run their Householder QR sweep on the device (``pcx_tt_orth``).  ``run_completion`` --
fixed-rank alternating least squares against the values on the whole grid -- runs all its outer iterations in one
device call (``pcx_tt_als``, ``csrc/tt_als_kernels.h``): with the neighbouring cores orthonormal each core's solve is
the projection ``C_k = L^T T R^T``, two chains of tall-skinny contractions over the target tensor, in place of the
reference's dense ``lstsq``.  Its ``values=`` keyword passes the target as a tensor instead of through the callback.

``fit_samples`` / ``from_samples`` fit the cores to samples at ARBITRARY points (extension: every other builder needs the
function on the Chebyshev grid): alternating least squares over the coefficient cores, one position at a time.  The
samples live on the device for the whole fit (a ``pcx_tt_fit`` session); per position the device accumulates the normal
equations ``G = A^T A``, ``b = A^T y`` of the design matrix ``a_i = L_i (x) T (x) R_i`` without ever forming it
(``pcx_tt_fit_normal``, ``csrc/tt_fit_kernels.h``: the N P^2 work of a step), and per outer iteration the residual on the
samples (``pcx_tt_fit_residual``: the evaluation kernels on the resident points); the P x P solve and the QR steps that
move the orthogonality centre are host NumPy on core-sized arrays.

Out of scope in this tier: the ``method='als'`` builder (raises ``NotImplementedError``) and ``with_auto_order``.
"""
from __future__ import annotations

import ctypes
import pickle
import time
import warnings
from typing import Callable, List, Sequence, Tuple

import numpy as np
from numpy.polynomial.chebyshev import chebpts1

from . import _calculus, _lib
from ._calculus import FibreCalculusMixin
from ._ergonomics import ErgonomicsMixin
from ._version import __version__

__all__ = ["ChebyshevTT"]


# --------------------------------------------------------------------------------------
# device-backed dense steps
# --------------------------------------------------------------------------------------

def _device() -> int:
    return _lib.default_device()


def _cross_step(C: np.ndarray, cap: int, rel_thresh: float = 1e-12):
    """SVD-rank + maxvol + cross interpolation of one unfolding on the device
    (reference tensor_train.py:332-362).  Returns (C_hat (m, rank), pivots (rank,), rank)."""
    lib = _lib.load()
    C = _lib.f64(C)
    m, c = C.shape
    chat = np.empty(m * c)
    piv = np.zeros(c, dtype=np.int64)
    rank = ctypes.c_int32(0)
    _lib.check(lib.pcx_tt_cross_step(_device(), _lib.p_f64(C), m, c, int(cap), float(rel_thresh),
                                     _lib.p_f64(chat), _lib.p_i64(piv), ctypes.byref(rank)), lib)
    r = int(rank.value)
    return chat[: m * r].reshape(m, r).copy(), piv[:r].astype(np.intp), r


def _maxvol(A: np.ndarray, tol: float = 1.05, max_iters: int = 100) -> np.ndarray:
    """Rows of an (m, r) matrix with approximately maximal volume
    (reference tensor_train.py:38-120), computed on the device."""
    lib = _lib.load()
    A = _lib.f64(A)
    m, r = A.shape
    idx = np.zeros(min(m, r) if m <= r else r, dtype=np.int64)
    _lib.check(lib.pcx_maxvol(_device(), _lib.p_f64(A), m, r, float(tol), int(max_iters),
                              _lib.p_i64(idx)), lib)
    return idx.astype(np.intp)


def _als_project(side: int, small: np.ndarray, big: np.ndarray, form: int = 0):
    """One contraction of the completion sweeps on the device (diagnostic, ``pcx_tt_als_project``).  side 0:
    ``small.T @ big`` with small (K, r), big (K, R); side 1: ``big @ small.T`` with small (r, K), big (R, K).
    form 0 is the sweeps' dispatch, 1 the VALU form, 2 the MFMA form.  Returns (out, form_used)."""
    lib = _lib.load()
    small, big = _lib.f64(small), _lib.f64(big)
    if side == 0:
        (K, r), (K2, R) = small.shape, big.shape
        out = np.empty((r, R))
    else:
        (r, K), (R, K2) = small.shape, big.shape
        out = np.empty((R, r))
    if K != K2:
        raise ValueError(f"contraction lengths differ: {K} and {K2}")
    used = ctypes.c_int32(0)
    _lib.check(lib.pcx_tt_als_project(_device(), int(side), int(form), _lib.p_f64(small), _lib.p_f64(big), _lib.p_f64(out),
                                      K, r, R, ctypes.byref(used)), lib)
    return out, int(used.value)


def _als_qr(A: np.ndarray):
    """The Householder QR of the completion sweeps and of ``orth_left`` / ``orth_right`` on the device (diagnostic,
    ``pcx_tt_als_qr``): (Q (m, p), R (p, c)), p = min(m, c)."""
    lib = _lib.load()
    A = _lib.f64(A)
    m, c = A.shape
    p = min(m, c)
    Q, R = np.empty((m, p)), np.empty((p, c))
    _lib.check(lib.pcx_tt_als_qr(_device(), _lib.p_f64(A), m, c, _lib.p_f64(Q), _lib.p_f64(R)), lib)
    return Q, R


def _als_norms(tnew: np.ndarray, tprev: np.ndarray, target: np.ndarray) -> np.ndarray:
    """The four convergence sums of one outer iteration on the device (diagnostic, ``pcx_tt_als_norms``):
    |new - prev|^2, |prev|^2, |new - target|^2, |target|^2."""
    lib = _lib.load()
    a, b, c = (_lib.f64(x).ravel() for x in (tnew, tprev, target))
    if not a.size == b.size == c.size:
        raise ValueError("the three tensors differ in size")
    out = np.empty(4)
    _lib.check(lib.pcx_tt_als_norms(_device(), _lib.p_f64(a), _lib.p_f64(b), _lib.p_f64(c), a.size, _lib.p_f64(out)), lib)
    return out


def _value_core_to_coeff_core(value_core: np.ndarray) -> np.ndarray:
    """Values at type-I nodes -> Chebyshev coefficients along axis 1
    (reference tensor_train.py:997-1016), DCT-II evaluated on the device."""
    lib = _lib.load()
    vc = _lib.f64(value_core)
    rl, n, rr = vc.shape
    out = np.empty_like(vc)
    _lib.check(lib.pcx_tt_value_to_coeff_core(_device(), _lib.p_f64(vc), rl, n, rr,
                                              _lib.p_f64(out)), lib)
    return out


def _tt_grid_values(cores: Sequence[np.ndarray], idx: np.ndarray) -> np.ndarray:
    """TT value at integer grid index tuples through the chain of value cores
    (reference ``_eval_tt``, tensor_train.py:223-228), batched on the device."""
    lib = _lib.load()
    d = len(cores)
    n = _lib.i32([c.shape[1] for c in cores])
    ranks = _lib.i32([1] + [c.shape[2] for c in cores])
    cat = _lib.f64(np.concatenate([np.asarray(c, dtype=float).ravel() for c in cores]))
    ii = _lib.i32(idx).reshape(-1, d)
    out = np.empty(ii.shape[0])
    _lib.check(lib.pcx_tt_grid_eval(_device(), d, _lib.p_i32(n), _lib.p_i32(ranks), _lib.p_f64(cat),
                                    _lib.p_i32(ii), ii.shape[0], _lib.p_f64(out)), lib)
    return out


def _coeff_core_to_value_core(coeff_core: np.ndarray) -> np.ndarray:
    """Chebyshev coefficients along axis 1 -> values at the type-I nodes in ascending order: the inverse of
    :func:`_value_core_to_coeff_core` (reference tensor_train.py:1019-1043, an inverse DCT there).  Host NumPy:
    ``value[:, i, :] = sum_j T_j(x_i) coeff[:, j, :]`` with ``T_j(x_i) = cos(j theta_i)`` -- the cores are small."""
    c = np.asarray(coeff_core, dtype=float)
    n = c.shape[1]
    theta = np.pi * (2.0 * np.arange(n - 1, -1, -1) + 1.0) / (2.0 * n)      # ascending nodes x_i = cos(theta_i)
    basis = np.cos(np.outer(theta, np.arange(n)))
    return np.einsum("ij,rjs->ris", basis, c)


def _check_derivative_method(method) -> None:
    if method not in ("fd", "analytic"):
        raise ValueError(f"method must be 'fd' or 'analytic', got {method!r}")


def _entry_list(params, arity: int) -> list:
    """A ``slice`` (arity 2: ``(dim, value)``) or ``extrude`` (arity 3: ``(dim, (lo, hi), n_nodes)``) argument as a list
    of tuples: one entry may come alone."""
    alone = isinstance(params, tuple) and len(params) == arity and isinstance(params[0], (int, np.integer))
    return [tuple(params)] if alone else [tuple(entry) for entry in params]


def _checked_entries(entries: list, arity: int, upper: int) -> list:
    """The entries of :func:`_entry_list`, validated.  Every entry leads with a dimension index, an integer in
    ``[0, upper)`` that no other entry repeats; an extrude entry also needs ``lo < hi`` and an integer ``n_nodes >= 2``.
    The checks run over all entries at once; what is reported is the first entry that fails anything and, within it,
    type before range before repetition before bounds before node count -- the order a caller of the reference sees
    (_extrude_slice.py:9-63), with its messages."""
    count = len(entries)
    if count == 0:
        return entries
    heads = [entry[0] for entry in entries]
    is_index = np.fromiter((isinstance(h, (int, np.integer)) for h in heads), dtype=bool, count=count)
    index = np.array([int(h) if ok else -1 for h, ok in zip(heads, is_index)], dtype=np.int64)
    outside = (index < 0) | (index >= upper)
    first_use = np.unique(index, return_index=True)[1]
    repeats = np.ones(count, dtype=bool)
    repeats[first_use] = False                                   # True where an earlier entry has the same index
    failures = [(~is_index, TypeError, lambda e: f"dim_index must be int, got {type(e[0]).__name__}"),
                (outside, ValueError, lambda e: f"dim_index {e[0]} out of range [0, {upper - 1}]"),
                (repeats, ValueError, lambda e: f"Duplicate dim_index {e[0]}")]
    if arity == 3:
        empty = np.fromiter((not entry[1][0] < entry[1][1] for entry in entries), dtype=bool, count=count)
        few = np.fromiter((not isinstance(entry[2], (int, np.integer)) or entry[2] < 2 for entry in entries),
                          dtype=bool, count=count)
        failures += [(empty, ValueError, lambda e: f"Domain bounds must satisfy lo < hi, got [{e[1][0]}, {e[1][1]}]"),
                     (few, ValueError, lambda e: f"n_nodes must be int >= 2, got {e[2]}")]
    failed = np.logical_or.reduce([mask for mask, _, _ in failures])
    if failed.any():
        at = int(np.argmax(failed))
        for mask, kind, text in failures:
            if mask[at]:
                raise kind(text(entries[at]))
    return [(int(entry[0]),) + entry[1:] for entry in entries]


def _slice_params(params, ndim: int) -> list:
    """``(dim, value)`` pairs of a ``slice`` call; at least one dimension has to stay."""
    entries = _entry_list(params, 2)
    if len(entries) >= ndim:
        raise ValueError(f"Cannot slice all {ndim} dimensions (would produce 0D result)")
    return _checked_entries(entries, 2, ndim)


def _extrude_params(params, ndim: int) -> list:
    """``(dim, (lo, hi), n_nodes)`` triples of an ``extrude`` call, ascending by the index each takes in the result."""
    entries = _entry_list(params, 3)
    entries = _checked_entries(entries, 3, ndim + len(entries))
    return sorted(((k, (b[0], b[1]), int(n)) for k, b, n in entries), key=lambda entry: entry[0])


def _renumbered(kept_user_dims: Sequence[int], ndim: int, removed) -> List[int]:
    """``dim_order`` of a result that lost the user dimensions ``removed``: the surviving user dimensions, listed by
    storage position in ``kept_user_dims``, renumbered 0 .. in increasing order (reference :1664-1679, :2093-2104)."""
    survivors = [u for u in range(ndim) if u not in removed]
    new_index = {u: i for i, u in enumerate(survivors)}
    return [new_index[u] for u in kept_user_dims]


def _sobol_from_coeff_cores(cores: Sequence[np.ndarray]):
    """Variance, first- and total-order Sobol indices of a TT in Chebyshev coefficient space, as arrays by
    storage position (the reference's TT sensitivity, _sensitivity.py:143-270, restated).

    Under the Chebyshev measure a coefficient c_a carries the energy c_a^2 prod_k g(a_k), g(0) = pi and
    g(m > 0) = pi / 2.  With G_k[i, j] the Gram chains of the cores weighted by g (``gram[k]`` covers the
    dimensions before k, ``tail[k]`` those from k on), the total energy is gram[d], the variance is that minus the
    constant term's share c_0^2 pi^d, the part of it with a_j = 0 is gram[j] (x) pi C_j0 (x) C_j0 (x) tail[j+1],
    and the first-order part of dimension j is the squared line of coefficients c(0, .., m, .., 0), m >= 1, times
    pi^(d-1) pi / 2.  Cost O(d n r^2)."""
    d = len(cores)
    g = []
    for c in cores:
        gk = np.full(c.shape[1], np.pi / 2.0)
        gk[0] = np.pi
        g.append(gk)

    def step_left(M, A, w):        # sum_p w[p] A[:, p, :]^T M A[:, p, :]
        return np.einsum("ipa,ipb->ab", np.einsum("ij,jpb->ipb", M, A), A * w[None, :, None])

    def step_right(M, A, w):       # sum_p w[p] A[:, p, :] M A[:, p, :]^T
        return np.einsum("ipa,jpa->ij", np.einsum("ipb,ab->ipa", A, M), A * w[None, :, None])

    gram = [np.ones((1, 1))]
    for A, w in zip(cores, g):
        gram.append(step_left(gram[-1], A, w))
    tail = [np.ones((1, 1))]
    for A, w in zip(reversed(cores), reversed(g)):
        tail.append(step_right(tail[-1], A, w))
    tail.reverse()                 # tail[k]: dimensions k .. d-1, tail[d] = 1

    # degree-0 chains: lo[k] = C_00 ... C_(k-1)0 (a row), hi[k] = C_k0 ... C_(d-1)0 (a column)
    lo = [np.ones(1)]
    for A in cores:
        lo.append(lo[-1] @ A[:, 0, :])
    hi = [np.ones(1)]
    for A in reversed(cores):
        hi.append(A[:, 0, :] @ hi[-1])
    hi.reverse()

    energy = float(gram[d][0, 0])
    variance = energy - float(lo[d][0]) ** 2 * np.pi ** d
    if variance <= 0:
        return np.zeros(d), np.zeros(d), float(max(variance, 0.0))
    first, total = np.empty(d), np.empty(d)
    for j, A in enumerate(cores):
        line = np.einsum("i,ima,a->m", lo[j], A[:, 1:, :], hi[j + 1])
        first[j] = float(line @ line) * ((np.pi / 2.0) * np.pi ** (d - 1))
        A0 = A[:, 0, :]
        total[j] = energy - np.pi * float(np.sum((gram[j] @ A0) * (A0 @ tail[j + 1])))
    return first / variance, total / variance, float(variance)


def _tt_svd_from_tensor(tensor: np.ndarray, max_rank: int, tol: float) -> List[np.ndarray]:
    """TT-SVD of a dense value tensor (reference tensor_train.py:638-690): value cores
    ``(r_{k-1}, n_k, r_k)``.  Every unfolding is factored on the device (one-sided Jacobi on
    its rows, ``pcx_tt_svd``); the rank rule is the reference's."""
    lib = _lib.load()
    t = _lib.f64(np.asarray(tensor, dtype=np.float64))
    n = [int(v) for v in t.shape]
    d = len(n)
    if d == 1:
        return [t.reshape(1, n[0], 1).copy()]
    cap = 0
    r_prev, rest = 1, int(np.prod(n))
    for k in range(d):
        rest //= n[k]
        r = 1 if k == d - 1 else min(int(max_rank), r_prev * n[k], rest)
        cap += r_prev * n[k] * r
        r_prev = r
    cores_cat = np.empty(cap)
    ranks = np.zeros(d + 1, dtype=np.int32)
    used = ctypes.c_int64(0)
    sweeps = ctypes.c_int32(0)
    _lib.check(lib.pcx_tt_svd(_device(), d, _lib.p_i32(_lib.i32(n)), _lib.p_f64(t.ravel()), int(max_rank),
                              float(tol), _lib.p_i32(ranks), _lib.p_f64(cores_cat), cap,
                              ctypes.byref(used), ctypes.byref(sweeps)), lib)
    cores, off = [], 0
    for k in range(d):
        cnt = int(ranks[k]) * n[k] * int(ranks[k + 1])
        cores.append(cores_cat[off: off + cnt].reshape(int(ranks[k]), n[k], int(ranks[k + 1])).copy())
        off += cnt
    return cores


def _tt_svd(func, grids, max_rank, tol, verbose):
    """Full-grid evaluation through the Python callback (C order, as the reference's
    ``np.ndindex`` loop, :594-599) followed by the device TT-SVD (reference :543-635)."""
    n = [len(g) for g in grids]
    full = int(np.prod(n))
    if verbose:
        print(f"  Building full tensor ({full:,} evaluations)...")
    T = np.empty(n)
    d = len(n)
    for idx in np.ndindex(*n):
        T[idx] = func([float(grids[k][idx[k]]) for k in range(d)], None)
    cores = _tt_svd_from_tensor(T, max_rank, tol)
    if verbose:
        print(f"  TT-SVD ranks: {[1] + [c.shape[2] for c in cores]}")
    return cores, full


# --------------------------------------------------------------------------------------
# TT-Cross (host orchestration; reference tensor_train.py:123-540)
# --------------------------------------------------------------------------------------

class _CrossBuilder:
    """Alternating left-to-right / right-to-left cross approximation with maxvol pivots.

    State: left/right multi-index sets per dimension, the evaluation cache, the best cores
    seen so far.  The RNG is drawn in the reference's order: first the right index sets
    (one ``integers`` call per column, :252-263), then one call per dimension for every
    convergence check (:289-291).
    """

    def __init__(self, func: Callable, grids: List[np.ndarray], max_rank: int, tol: float,
                 max_sweeps: int, verbose, seed):
        self.func = func
        self.grids = grids
        self.d = len(grids)
        self.n = [len(g) for g in grids]
        self.tol = tol
        self.max_sweeps = max_sweeps
        self.verbose = verbose
        self.rng = np.random.default_rng(seed)
        self.cache: dict = {}
        d, n = self.d, self.n
        self.caps = [1] * (d + 1)
        for k in range(1, d):
            self.caps[k] = min(max_rank, int(np.prod(n[:k])), int(np.prod(n[k:])))
        start_rank = [1] * (d + 1)
        for k in range(1, d):
            start_rank[k] = min(self.caps[k], n[k - 1], n[k])
        self.right = [None] * d
        for k in range(d - 1):
            cols = [self.rng.integers(0, n[k + 1 + j], size=start_rank[k + 1]) for j in range(d - k - 1)]
            self.right[k] = np.column_stack(cols)
        self.right[d - 1] = np.zeros((1, 0), dtype=np.intp)
        self.left = [None] * d
        self.left[0] = np.zeros((1, 0), dtype=np.intp)
        self.cores = [None] * d
        self.n_test = min(20, max(5, d))
        self.best_err = float("inf")
        self.best_cores = None
        self.stale = 0

    # -- function values through the cache (key = grid index tuple, :215-221)
    def value(self, index) -> float:
        key = tuple(int(i) for i in index)
        hit = self.cache.get(key)
        if hit is None:
            hit = self.func([float(self.grids[k][key[k]]) for k in range(self.d)], None)
            self.cache[key] = hit
        return hit

    def unfolding(self, k: int) -> np.ndarray:
        """Values f(left[a], i, right[b]) as an array of shape (r_left, n_k, r_right)."""
        L, R = self.left[k], self.right[k]
        out = np.empty((L.shape[0], self.n[k], R.shape[0]))
        for a, lrow in enumerate(L):
            head = list(lrow)
            for i in range(self.n[k]):
                mid = head + [i]
                for b, rrow in enumerate(R):
                    out[a, i, b] = self.value(mid + list(rrow))
        return out

    def check(self) -> float:
        """Relative error of the TT at n_test random grid points (:287-297)."""
        pts = np.column_stack([self.rng.integers(0, self.n[k], size=self.n_test) for k in range(self.d)])
        approx = _tt_grid_values(self.cores, pts)
        exact = np.array([self.value(p) for p in pts])
        ref = np.linalg.norm(exact)
        err = np.linalg.norm(approx - exact)
        return float(err / ref) if ref > 0 else float(err)

    def note(self, err: float, label: str) -> bool:
        """Best-cores bookkeeping and stop rules (:403-422, :515-534).  True = stop."""
        if err < self.best_err * 0.9:
            self.best_err = err
            self.best_cores = [c.copy() for c in self.cores]
            self.stale = 0
        else:
            self.stale += 1
        if err < self.tol:
            if self.verbose:
                print(f"    Converged after {label}")
            return True
        if self.stale >= 3 and self.best_err < 1e-3:
            if self.verbose:
                print(f"    No improvement in {self.stale} checks (best = {self.best_err:.2e}) — stopping")
            return True
        return False

    def sweep_left_to_right(self) -> None:
        d, n = self.d, self.n
        for k in range(d - 1):
            T = self.unfolding(k)
            rl, nk, rr = T.shape
            chat, piv, rank = _cross_step(T.reshape(rl * nk, rr), self.caps[k + 1])
            self.cores[k] = chat.reshape(rl, nk, rank)
            new_left = np.empty((rank, k + 1), dtype=np.intp)
            for t, p in enumerate(piv):
                a, ik = divmod(int(p), nk)
                a = min(a, rl - 1)
                new_left[t, :k] = self.left[k][a]
                new_left[t, k] = ik
            self.left[k + 1] = new_left
        T = self.unfolding(d - 1)          # right set is the empty tuple: shape (r, n, 1)
        self.cores[d - 1] = T.reshape(T.shape[0], n[d - 1], 1).copy()

    def sweep_right_to_left(self) -> None:
        d, n = self.d, self.n
        for k in range(d - 1, 0, -1):
            T = self.unfolding(k)
            rl, nk, rr = T.shape
            Ct = T.reshape(rl, nk * rr).T                    # rows = (node, right index)
            chat_t, piv, rank = _cross_step(np.ascontiguousarray(Ct), self.caps[k])
            self.cores[k] = chat_t.T.reshape(rank, nk, rr).copy()
            new_right = np.empty((rank, d - k), dtype=np.intp)
            span = max(rr, 1)
            for t, p in enumerate(piv):
                ik, b = divmod(int(p), span)
                ik = min(ik, nk - 1)
                b = min(b, span - 1)
                new_right[t, 0] = ik
                new_right[t, 1:] = self.right[k][b]
            self.right[k - 1] = new_right
        T = self.unfolding(0)              # left set is the empty tuple: shape (1, n, r)
        self.cores[0] = T.copy()

    def run(self):
        for sweep in range(self.max_sweeps):
            self.sweep_left_to_right()
            err = self.check()
            if self.verbose:
                ranks = [1] + [c.shape[2] for c in self.cores]
                print(f"    Sweep {sweep + 1} L->R: rel error = {err:.2e}, "
                      f"unique evals = {len(self.cache):,}, ranks = {ranks}")
            if self.note(err, f"{sweep + 1} sweeps (L->R)"):
                break
            self.sweep_right_to_left()
            err = self.check()
            if self.verbose:
                print(f"    Sweep {sweep + 1} R->L: rel error = {err:.2e}, "
                      f"unique evals = {len(self.cache):,}")
            if self.note(err, f"{sweep + 1} sweeps"):
                break
        cores = self.best_cores if self.best_cores is not None else self.cores
        return cores, len(self.cache)


def _tt_cross(func, grids, max_rank, tol, max_sweeps, verbose, seed=None):
    """TT value cores from a callable via alternating TT-Cross (reference :123-540)."""
    return _CrossBuilder(func, grids, max_rank, tol, max_sweeps, verbose, seed).run()


# --------------------------------------------------------------------------------------
# ChebyshevTT
# --------------------------------------------------------------------------------------

# --------------------------------------------------------------------------------------
# fitting to scattered samples: the host side of ChebyshevTT.fit_samples
# --------------------------------------------------------------------------------------

def _checked_sample_points(points, d: int) -> np.ndarray:
    arr = np.asarray(points)
    if arr.dtype.kind not in "fiu":
        raise TypeError(f"points must be real numbers, got dtype {arr.dtype}")
    if arr.ndim != 2 or arr.shape[1] != d:
        raise ValueError(f"points must have shape (N, {d}), got {arr.shape}")
    return _lib.f64(arr)


def _checked_sample_values(values) -> np.ndarray:
    arr = np.asarray(values)
    if arr.dtype.kind not in "fiu":
        raise TypeError(f"values must be real numbers, got dtype {arr.dtype}")
    if arr.ndim != 1:
        raise ValueError(f"values must have shape (N,), got {arr.shape}")
    return _lib.f64(arr)


def _fit_start_ranks(n: Sequence[int], rank: int) -> List[int]:
    """The bonds of ``from_samples``' start: ``_CrossBuilder``'s caps, ``min(rank, prod(n[:k]), prod(n[k:]))``."""
    d = len(n)
    return [1] + [min(rank, int(np.prod(n[:k], dtype=np.int64)), int(np.prod(n[k:], dtype=np.int64)))
                  for k in range(1, d)] + [1]


def _fit_move_centre(cores: List[np.ndarray], k: int, to: int) -> None:
    """Move the orthogonality centre from core ``k`` to its neighbour ``to`` in place: a reduced QR of core ``k``'s
    unfolding, the triangular factor absorbed into the neighbour; the tensor is unchanged, the bond becomes
    ``min(rows, columns)`` of the unfolding."""
    rl, n, rr = cores[k].shape
    if to == k + 1:
        Q, R = np.linalg.qr(cores[k].reshape(rl * n, rr))
        cores[k] = Q.reshape(rl, n, Q.shape[1])
        nxt = cores[k + 1]
        cores[k + 1] = (R @ nxt.reshape(rr, -1)).reshape(R.shape[0], nxt.shape[1], nxt.shape[2])
    elif to == k - 1:
        Q, R = np.linalg.qr(cores[k].reshape(rl, n * rr).T)
        cores[k] = np.ascontiguousarray(Q.T).reshape(Q.shape[1], n, rr)
        prv = cores[k - 1]
        cores[k - 1] = (prv.reshape(-1, rl) @ R.T).reshape(prv.shape[0], prv.shape[1], R.shape[0])
    else:
        raise ValueError(f"the centre moves to a neighbour, not from {k} to {to}")


class _FitSession:
    """Owner of one ``pcx_tt_fit`` session: the samples of one ``fit_samples`` call, resident on the device."""

    def __init__(self, tt: "ChebyshevTT", pts, vals, N: int, device: int | None = None):
        from .device import DeviceArray
        lib = _lib.load()
        d = tt.num_dimensions
        lo = _lib.f64([float(b[0]) for b in tt.domain])
        hi = _lib.f64([float(b[1]) for b in tt.domain])
        handle = ctypes.c_void_p()
        self.handle, self._keep = None, None
        if isinstance(pts, DeviceArray):
            dev = pts.device
            self._keep = (pts, vals)            # adopted, not copied: alive as long as the session
            rc = lib.pcx_tt_fit_create_dev(dev, d, _lib.p_f64(lo), _lib.p_f64(hi), ctypes.c_void_p(pts.ptr),
                                           ctypes.c_void_p(vals.ptr), N, ctypes.byref(handle))
        else:
            dev = device if device is not None else (_lib.default_device() if tt._device_index is None else tt._device_index)
            rc = lib.pcx_tt_fit_create(int(dev), d, _lib.p_f64(lo), _lib.p_f64(hi), _lib.p_f64(pts), _lib.p_f64(vals), N,
                                       ctypes.byref(handle))
        _lib.check(rc, lib)
        self.lib, self.handle, self.device, self.d = lib, handle, int(dev), d

    def set_form(self, form: int) -> None:
        _lib.check(self.lib.pcx_tt_fit_set_form(self.handle, int(form)), self.lib)

    def normal(self, cores, k: int):
        """``(G, b)`` of position ``k`` for ``cores``."""
        from . import _algebra
        n, ranks, cat = _algebra._shape_args(cores)
        P = cores[k].size
        G, b = np.empty((P, P)), np.empty(P)
        _lib.check(self.lib.pcx_tt_fit_normal(self.handle, self.d, _lib.p_i32(n), _lib.p_i32(ranks), _lib.p_f64(cat), int(k),
                                              _lib.p_f64(G), _lib.p_f64(b)), self.lib)
        return G, b

    def sumsq(self, cores) -> np.ndarray:
        """``[sum (TT(x_i) - y_i)^2, sum y_i^2]`` for ``cores``."""
        from . import _algebra
        n, ranks, cat = _algebra._shape_args(cores)
        out = np.empty(2)
        _lib.check(self.lib.pcx_tt_fit_residual(self.handle, self.d, _lib.p_i32(n), _lib.p_i32(ranks), _lib.p_f64(cat),
                                                _lib.p_f64(out)), self.lib)
        return out

    def residual(self, cores) -> float:
        """``||TT(x) - y|| / ||y||``; 0 for an exact fit of all-zero values, inf for any other fit of them."""
        s = self.sumsq(cores)
        if s[1] > 0.0:
            return float(np.sqrt(s[0]) / np.sqrt(s[1]))
        return float("inf") if s[0] > 0.0 else 0.0

    def close(self) -> None:
        if self.handle:
            self.lib.pcx_tt_fit_destroy(self.handle)
            self.handle = None
        self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DeviceTT:
    """Owner of one ``pcx_tt`` handle (freed on garbage collection)."""

    def __init__(self, tt: "ChebyshevTT", device: int):
        lib = _lib.load()
        cores = tt._coeff_cores
        d = tt.num_dimensions
        n = _lib.i32([c.shape[1] for c in cores])
        ranks = _lib.i32([cores[0].shape[0]] + [c.shape[2] for c in cores])
        lo = _lib.f64([float(b[0]) for b in tt.domain])
        hi = _lib.f64([float(b[1]) for b in tt.domain])
        cat = _lib.f64(np.concatenate([np.asarray(c, dtype=float).ravel() for c in cores]))
        order = _lib.i32(tt._dim_order)
        handle = ctypes.c_void_p()
        _lib.check(lib.pcx_tt_create(device, d, _lib.p_i32(n), _lib.p_i32(ranks), _lib.p_f64(lo),
                                     _lib.p_f64(hi), _lib.p_f64(cat), _lib.p_i32(order),
                                     ctypes.byref(handle)), lib)
        self.lib = lib
        self.handle = handle
        self.device = device
        self.key = (id(cores), tuple(id(c) for c in cores), tuple(tt._dim_order))

    def __del__(self):
        try:
            if self.handle:
                self.lib.pcx_tt_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class ChebyshevTT(ErgonomicsMixin, FibreCalculusMixin):
    """Chebyshev interpolation in tensor-train format (signature: reference :1088-1100)."""

    def __init__(self, function: Callable, num_dimensions: int,
                 domain: Sequence[Tuple[float, float]], n_nodes: Sequence[int], max_rank: int = 10,
                 tolerance: float = 1e-6, max_sweeps: int = 10, additional_data: object = None, *,
                 max_derivative_order: int = 2):
        from . import Domain, Ns
        if isinstance(domain, Domain):
            domain = list(domain.bounds)
        if isinstance(n_nodes, Ns):
            n_nodes = list(n_nodes.counts)
        if len(domain) != num_dimensions:
            raise ValueError(f"domain has {len(domain)} entries but num_dimensions={num_dimensions}")
        if len(n_nodes) != num_dimensions:
            raise ValueError(f"n_nodes has {len(n_nodes)} entries but num_dimensions={num_dimensions}")
        self.function = function
        self.num_dimensions = num_dimensions
        self.domain = domain
        self.n_nodes = n_nodes
        self.max_rank = max_rank
        self.tolerance = tolerance
        self.max_sweeps = max_sweeps
        self.max_derivative_order = max_derivative_order
        self._coeff_cores: List[np.ndarray] | None = None
        self._built = False
        self.descriptor = ""
        self.additional_data = additional_data
        self._tt_ranks: List[int] | None = None
        self._build_time = 0.0
        self._total_build_evals = 0
        self._cached_error_estimate = None
        self.method: str | None = None
        self._dim_order: List[int] = list(range(num_dimensions))
        self._device_tt: _DeviceTT | None = None
        self._device_index: int | None = None

    # ---------------------------------------------------------------- build
    def build(self, verbose: bool | int = True, seed: int | None = None, method: str = "cross") -> None:
        """TT-Cross build then value->coefficient conversion (reference :1140-1289)."""
        if method not in ("cross", "svd", "als"):
            raise ValueError(f"method must be 'cross', 'svd', or 'als', got {method!r}")
        if method == "als":
            raise NotImplementedError("method='als' (alternating least squares sweeps around LAPACK "
                                      "solves in the reference) is outside this build's scope; "
                                      "use 'cross' or 'svd'")
        self.method = method
        start = time.time()
        self._cached_error_estimate = None
        full = int(np.prod(self.n_nodes))
        if verbose:
            print(f"Building {self.num_dimensions}D ChebyshevTT (max_rank={self.max_rank}, method={method!r})...")
            print(f"  Full tensor would need {full:,} evaluations")
        grids = [np.sort(0.5 * (a + b) + 0.5 * (b - a) * chebpts1(n))
                 for (a, b), n in zip(self.domain, self.n_nodes)]
        data, raw = self.additional_data, self.function

        def with_data(point, _unused):
            return raw(point, data)

        if method == "cross":
            if verbose:
                print("  Running TT-Cross...")
            value_cores, n_evals = _tt_cross(with_data, grids, self.max_rank, self.tolerance,
                                             self.max_sweeps, verbose, seed)
        else:
            value_cores, n_evals = _tt_svd(with_data, grids, self.max_rank, self.tolerance, verbose)
        self._total_build_evals = n_evals
        self._coeff_cores = [_value_core_to_coeff_core(c) for c in value_cores]
        self._tt_ranks = [1] + [c.shape[2] for c in self._coeff_cores]
        self._build_time = time.time() - start
        self._built = True
        self._device_tt = None
        if verbose:
            storage = sum(c.size for c in self._coeff_cores)
            print(f"  Built in {self._build_time:.3f}s ({n_evals:,} function evaluations)")
            print(f"  TT ranks: {self._tt_ranks}")
            print(f"  Compression: {full:,} -> {storage:,} elements ({full / storage:.1f}x)")

    @classmethod
    def from_values(cls, tensor_values, num_dimensions: int, domain, n_nodes,
                    max_rank: int | None = None, tolerance: float = 1e-6,
                    max_derivative_order: int = 2, additional_data=None,
                    descriptor: str = "") -> "ChebyshevTT":
        """TT interpolant from a precomputed dense tensor of node values by TT-SVD
        (reference :2871-2965); the compression runs on the device."""
        from . import Domain, Ns
        if isinstance(domain, Domain):
            domain = list(domain.bounds)
        if isinstance(n_nodes, Ns):
            n_nodes = list(n_nodes.counts)
        arr = np.asarray(tensor_values, dtype=np.float64)
        expected_shape = tuple(n_nodes)
        if arr.shape != expected_shape:
            raise ValueError(f"tensor_values shape {arr.shape} does not match expected {expected_shape}")
        if not np.isfinite(arr).all():
            raise ValueError("tensor_values contains NaN or Inf — all values must be finite")
        if max_rank is None:
            max_rank = max(n_nodes)
        value_cores = _tt_svd_from_tensor(arr, max_rank=max_rank, tol=tolerance)
        obj = cls(None, num_dimensions, list(domain), list(n_nodes), max_rank=max_rank,
                  tolerance=tolerance, max_derivative_order=max_derivative_order,
                  additional_data=additional_data)
        obj.descriptor = descriptor
        obj.method = "svd"
        obj._coeff_cores = [_value_core_to_coeff_core(c) for c in value_cores]
        obj._tt_ranks = [c.shape[0] for c in obj._coeff_cores] + [obj._coeff_cores[-1].shape[2]]
        obj._built = True
        return obj

    @classmethod
    def from_coeff_cores(cls, coeff_cores: Sequence[np.ndarray], domain, dim_order=None,
                         max_derivative_order: int = 2) -> "ChebyshevTT":
        """Wrap existing Chebyshev coefficient cores ``(r_{k-1}, n_k, r_k)`` (extension; the
        reference builds such objects through its ``object.__new__`` factory pattern, :2946-2965)."""
        cores = [np.array(c, dtype=float) for c in coeff_cores]
        d = len(cores)
        obj = cls(None, d, [list(b) for b in domain], [c.shape[1] for c in cores],
                  max_rank=max(c.shape[2] for c in cores), max_derivative_order=max_derivative_order)
        for k in range(d - 1):
            if cores[k].shape[2] != cores[k + 1].shape[0]:
                raise ValueError(f"core {k} right rank {cores[k].shape[2]} != core {k + 1} left rank {cores[k + 1].shape[0]}")
        if cores[0].shape[0] != 1 or cores[-1].shape[2] != 1:
            raise ValueError("boundary TT ranks must be 1")
        obj._coeff_cores = cores
        obj._tt_ranks = [1] + [c.shape[2] for c in cores]
        obj._built = True
        obj.method = "cross"
        if dim_order is not None:
            if sorted(dim_order) != list(range(d)):
                raise ValueError("dim_order must be a permutation of range(num_dimensions)")
            obj._dim_order = [int(v) for v in dim_order]
        return obj

    def _check_built(self) -> None:
        if not self._built:
            raise RuntimeError("Call build() before using this method.")

    # ---------------------------------------------------------------- device plumbing
    def to_device(self, device: int | None = None, *, devices=None, pin: bool = False) -> "ChebyshevTT":
        """Upload the cores to GPU ``device``; ``devices`` (list or ``"all"``; default ``PCX_DEVICES``) replicates
        them on several GPUs of this process, and large host-pointer batches are split into one contiguous row
        block per device (``pcx_tt_group_eval_batch``), as ``ChebyshevApproximation.to_device`` describes."""
        self._check_built()
        if devices is None and device is None:
            devices = _lib.fanout_devices()
        if isinstance(devices, str):
            if devices.lower() != "all":
                raise ValueError("devices must be a list of device indices or 'all'")
            devices = list(range(max(1, _lib.device_count())))
        if devices is not None:
            devices = [int(v) for v in devices]
            if not devices:
                raise ValueError("devices is empty")
            device = devices[0]
        dev = _lib.default_device() if device is None else int(device)
        self._device_index = dev
        self._device_tt = _DeviceTT(self, dev)
        self._fanout = [self._device_tt] + [_DeviceTT(self, g) for g in (devices or [])[1:]]
        self._fanout_devices = list(devices) if devices else None
        # fan-out only.  pin=False (default since round 4): fan out over arrays the caller page-locked itself (pcx_host_register,
        # held for the arrays' lifetime) and send everything else through the first device.  pin=True: page-lock the caller's
        # arrays for the duration of each call (hipHostRegister over the points and the result, released afterwards) -- copies
        # at PCIe rate, but a heap range that was registered and released has three times ended a LATER call over the same
        # addresses in a GPU memory access fault (tools/soak.py --pin): opt-in, for processes that keep their arrays
        self._fanout_pin = bool(pin)
        return self

    def invalidate_device_cache(self) -> None:
        self._device_tt = None
        self._fanout = []

    def _dev(self) -> _DeviceTT:
        t = self._device_tt
        key = (id(self._coeff_cores), tuple(id(c) for c in self._coeff_cores), tuple(self._dim_order))
        if t is None or t.key != key:
            fan = getattr(self, "_fanout_devices", None)
            if fan:
                self.to_device(devices=fan)
            else:
                self.to_device(self._device_index)    # None: PCX_DEVICES, if set, replicates the cores
            t = self._device_tt
        return t

    def _eval_user_points(self, pts: np.ndarray) -> np.ndarray:
        """Points in the USER's dimension order; the device applies ``_dim_order``."""
        t = self._dev()
        from .device import DeviceArray, as_device_array, check_points
        dev_pts = as_device_array(pts)
        if dev_pts is not None:       # device-resident batch: result stays in HBM, complete on return
            n = check_points(dev_pts, self.num_dimensions, t.device)
            dout = DeviceArray.empty((n,), t.device)
            if n:
                st = ctypes.c_void_p()
                _lib.check(t.lib.pcx_tt_stream(t.handle, ctypes.byref(st)), t.lib)
                _lib.check(t.lib.pcx_tt_eval_batch_dev(t.handle, ctypes.c_void_p(dev_pts.ptr), n, ctypes.c_void_p(dout.ptr), st), t.lib)
                _lib.check(t.lib.pcx_stream_synchronize(st), t.lib)
            return dout
        pts = _lib.f64(pts)
        if pts.ndim != 2 or pts.shape[1] != self.num_dimensions:
            raise ValueError(f"points must have shape (N, {self.num_dimensions}), got {pts.shape}")
        out = np.empty(pts.shape[0])
        group = [g for g in getattr(self, "_fanout", []) if g.key == t.key]
        use = max(1, min(len(group), pts.shape[0] // _lib.FANOUT_MIN_ROWS_PER_DEVICE)) if group and group[0] is t else 1
        if use > 1:
            harr, keep = _lib.handle_array([g.handle for g in group[:use]])
            _lib.check(t.lib.pcx_tt_group_eval_batch(harr, use, _lib.p_f64(pts), pts.shape[0], _lib.p_f64(out),
                                                     1 if getattr(self, "_fanout_pin", False) else 0), t.lib)
        else:
            _lib.check(t.lib.pcx_tt_eval_batch(t.handle, _lib.p_f64(pts), pts.shape[0], _lib.p_f64(out)), t.lib)
        return out

    def _storage_to_user(self, pts_storage: np.ndarray) -> np.ndarray:
        """Rows in storage frame -> rows in user frame (inverse of points[:, _dim_order])."""
        if self._dim_order == list(range(self.num_dimensions)):
            return pts_storage
        out = np.empty_like(pts_storage)
        out[:, self._dim_order] = pts_storage
        return out

    # ---------------------------------------------------------------- evaluation API
    def eval(self, point) -> float:
        """Value at one point (reference :2127-2170)."""
        self._check_built()
        return float(self._eval_user_points(np.asarray([list(point)], dtype=float))[0])

    def eval_batch(self, points) -> np.ndarray:
        """Values at ``(N, num_dimensions)`` points (reference :2217-2265)."""
        self._check_built()
        from .device import is_device_array
        return self._eval_user_points(points if is_device_array(points) else np.asarray(points))

    def eval_multi(self, point, derivative_orders, *, method: str = "fd") -> List[float]:
        """Value and central-finite-difference derivatives at one point (reference
        :2267-2463).  All stencil points of all specs go to the device in ONE batch; the
        stencil arithmetic (h = 1e-4 (b - a), boundary nudge 1.5 h, 2/3/4-point and nested
        rules) is then replayed on the host in the reference's order.  ``method="analytic"`` (extension): the exact
        derivatives of the interpolant, row 0 of a one-row :meth:`eval_multi_batch` with that method."""
        self._check_built()
        _check_derivative_method(method)
        if method == "analytic":
            row = self.eval_multi_batch(np.asarray([list(point)], dtype=float), derivative_orders, method="analytic")
            return [float(v) for v in row[0]]
        d = self.num_dimensions
        order = self._dim_order
        if order != list(range(d)):
            pt = [point[order[k]] for k in range(d)]
            specs = [[s[order[k]] for k in range(d)] for s in derivative_orders]
        else:
            pt = list(point)
            specs = [list(s) for s in derivative_orders]

        pending: list = []

        def run(value_of):
            return [self._fd_spec(pt, spec, value_of) for spec in specs]

        def record(p):
            pending.append(list(p))
            return 0.0

        run(record)                                   # pass 1: collect stencil points
        vals = self._eval_user_points(self._storage_to_user(np.asarray(pending, dtype=float)))
        it = iter(vals)
        return run(lambda p: float(next(it)))         # pass 2: same traversal, real values

    def eval_multi_batch(self, points, derivative_orders, *, chunk: int = 1 << 18, method: str = "fd"):
        """Batched :meth:`eval_multi` (extension; the reference evaluates one point per call): ``(N, d)``
        points x ``m`` specs -> ``(N, m)``.  The finite-difference rules of the reference
        (``tensor_train.py:2322-2463``) run ON THE DEVICE (``pcx_tt_eval_multi_batch``, ``csrc/tt_fd_kernels.h``):
        every stencil point is formed from the query row in registers and evaluated by the model's own chain, so
        row i equals ``eval_multi(points[i], derivative_orders)`` bit for bit and no stencil batch crosses PCIe.
        A device array in gives a device array out.  Specs with more than three differenced dimensions (27+
        stencil points) keep the host-side traversal (``_eval_multi_batch_host``).

        ``method="analytic"``: the exact derivatives of the interpolant instead (``pcx_tt_deriv_batch``,
        ``csrc/tt_deriv_kernels.h``) -- one chain per (row, spec) with ``T_j``, ``T'_j`` or ``T''_j`` as the basis of a
        dimension.  No step size, no nudge at a domain end, any number of differentiated dimensions, host or device
        arrays; ``chunk`` is not used."""
        self._check_built()
        _check_derivative_method(method)
        d = self.num_dimensions
        specs_user = [[int(v) for v in s] for s in derivative_orders]
        for spec in specs_user:
            if len(spec) != d:
                raise ValueError(f"each derivative spec needs {d} orders, got {len(spec)}")
            for o in spec:
                if o not in (0, 1, 2):
                    raise ValueError(f"Derivative order {o} not supported (use 1 or 2)")
        m = len(specs_user)
        from .device import DeviceArray, as_device_array, check_points, is_device_array
        on_device = is_device_array(points)
        if m == 0:
            n0 = int(points.shape[0]) if hasattr(points, "shape") else len(points)
            return np.empty((n0, 0))
        analytic = method == "analytic"
        if not analytic and any(sum(1 for o in spec if o) > 3 for spec in specs_user):
            if on_device:
                raise NotImplementedError("specs with more than three differenced dimensions need host arrays")
            return self._eval_multi_batch_host(points, specs_user, chunk=chunk)
        t = self._dev()
        host_entry = t.lib.pcx_tt_deriv_batch if analytic else t.lib.pcx_tt_eval_multi_batch
        dev_entry = t.lib.pcx_tt_deriv_batch_dev if analytic else t.lib.pcx_tt_eval_multi_batch_dev
        block = _lib.i32(np.asarray(specs_user).reshape(-1))
        if on_device:
            dev_pts = as_device_array(points)
            n = check_points(dev_pts, d, t.device)
            dout = DeviceArray.empty((n, m), t.device)
            if n:
                st = ctypes.c_void_p()
                _lib.check(t.lib.pcx_tt_stream(t.handle, ctypes.byref(st)), t.lib)
                _lib.check(dev_entry(t.handle, ctypes.c_void_p(dev_pts.ptr), n, _lib.p_i32(block), m,
                                     ctypes.c_void_p(dout.ptr), st), t.lib)
                _lib.check(t.lib.pcx_stream_synchronize(st), t.lib)
            return dout
        pts = _lib.f64(np.asarray(points, dtype=float))
        if pts.ndim != 2 or pts.shape[1] != d:
            raise ValueError(f"points must have shape (N, {d}), got {pts.shape}")
        out = np.empty((pts.shape[0], m))
        if pts.shape[0]:
            _lib.check(host_entry(t.handle, _lib.p_f64(pts), pts.shape[0], _lib.p_i32(block), m, _lib.p_f64(out)), t.lib)
        return out

    def _sweep_batch(self, points, out, C, entry, arg):
        """The ``(N, C)`` result of ``gradient_batch`` / ``hessian_batch``: the argument checks, then ``entry`` on host
        points (or ``entry + "_dev"`` when the points or ``out=`` are on the device) with the integer ``arg`` between N
        and the result.  A NumPy array or a :class:`~pychebyshev_amd.device.DeviceArray`, ``out`` itself when given."""
        self._check_built()
        from .device import DeviceArray, as_device_array, check_points, is_device_array
        d = self.num_dimensions
        t = self._dev()
        if is_device_array(points):
            dev_pts, pts = as_device_array(points), None
            n = check_points(dev_pts, d, t.device)
        else:
            pts = _lib.f64(np.asarray(points, dtype=float))
            if pts.ndim != 2 or pts.shape[1] != d:
                raise ValueError(f"points must have shape (N, {d}), got {pts.shape}")
            dev_pts, n = None, pts.shape[0]
        host_out, dev_out = _calculus.validate_ladder_out(out, (n, C))
        if dev_out is not None and dev_out.size and dev_out.device != t.device:
            raise ValueError(f"out lives on device {dev_out.device} but the model is on device {t.device}; "
                             f"call to_device({dev_out.device}) on the model first")
        if dev_pts is None and dev_out is None:
            res = np.empty((n, C)) if host_out is None else host_out
            if n:
                _lib.check(getattr(t.lib, entry)(t.handle, _lib.p_f64(pts), n, arg, _lib.p_f64(res)), t.lib)
        else:
            res = DeviceArray.empty((n, C), t.device) if dev_out is None else dev_out
            if n:
                d_pts = dev_pts if dev_pts is not None else DeviceArray.from_host(pts, t.device)
                st = ctypes.c_void_p()
                _lib.check(t.lib.pcx_tt_stream(t.handle, ctypes.byref(st)), t.lib)
                _lib.check(getattr(t.lib, entry + "_dev")(t.handle, ctypes.c_void_p(d_pts.ptr), n, arg,
                                                          ctypes.c_void_p(res.ptr), st), t.lib)
                _lib.check(t.lib.pcx_stream_synchronize(st), t.lib)
            if host_out is not None:              # device points, host out=
                if n:
                    host_out[...] = res.to_host()
                res = host_out
        return res

    def gradient_batch(self, points, *, second: bool = False, out=None):
        """Value and every first partial derivative of the interpolant at ``(N, d)`` points, exact as
        ``eval_multi_batch(..., method="analytic")`` (extension): ``(values (N,), grad (N, d))``, and with
        ``second=True`` ``(values, grad, diag (N, d))``, ``diag[:, u]`` the second derivative along dimension ``u``
        (the Hessian's diagonal).  Columns are the user's dimensions.

        One forward-backward pass per row (``pcx_tt_grad_batch``, ``csrc/tt_grad_kernels.h``): a right sweep keeps every
        partial product ``R_k``, a left sweep folds each core with ``T_j``, ``T'_j`` and ``T''_j`` from the same core
        loads -- three chains' worth of folds for value and gradient (one for the right sweep, two for the left), four
        with the diagonal, whatever ``d`` is, where the analytic ``eval_multi_batch`` walks one chain per (row, spec):
        ``d + 1`` / ``2 d + 1`` of them.

        The returns are views of one ``(N, C)`` result, ``C = 1 + d`` or ``1 + 2 d``: column 0 the value, ``1 + u`` the
        gradient, ``1 + d + u`` the diagonal.  Host points give NumPy arrays; a device array in gives device arrays out
        (strided :class:`~pychebyshev_amd.device.DeviceColumns` of one :class:`~pychebyshev_amd.device.DeviceArray`,
        complete on return; ``to_host()`` of a view downloads the whole result, so for all parts on the host download
        ``view.parent`` once and slice it).  ``out=`` is that ``(N, C)`` result preallocated, a C-contiguous float64 NumPy array or
        a device array; the views are then of ``out``."""
        self._check_built()
        from .device import DeviceColumns
        d = self.num_dimensions
        second = bool(second)
        C = 1 + (2 if second else 1) * d
        res = self._sweep_batch(points, out, C, "pcx_tt_grad_batch", int(second))
        if isinstance(res, np.ndarray):
            parts = (res[:, 0], res[:, 1:1 + d]) + ((res[:, 1 + d:],) if second else ())
        else:
            parts = (DeviceColumns(res, 0, 1, squeeze=True), DeviceColumns(res, 1, 1 + d)) \
                + ((DeviceColumns(res, 1 + d, C),) if second else ())
        return parts

    def gradient(self, point, *, second: bool = False):
        """Value and gradient at one point, ``(float, (d,) array)``, and with ``second=True`` the second derivatives
        along each dimension as a third ``(d,)`` array: row 0 of a one-row :meth:`gradient_batch`."""
        parts = self.gradient_batch(np.asarray([list(point)], dtype=float), second=second)
        return (float(parts[0][0]),) + tuple(np.array(p[0]) for p in parts[1:])

    def hessian_batch(self, points, *, out=None):
        """Value, gradient and the full Hessian of the interpolant at ``(N, d)`` points, exact as
        ``eval_multi_batch(..., method="analytic")`` (extension): ``(values (N,), grad (N, d), hess (N, d, d))``,
        ``hess[:, u, v]`` the second partial derivative along the user's dimensions ``u`` and ``v``; both triangles hold
        the one computed number.

        The sweeps of :meth:`gradient_batch` (``pcx_tt_hess_batch``, ``csrc/tt_hess_kernels.h``): the vector the left
        sweep forms for ``grad[:, i]`` is kept and carried to the right beside the left partial product, and at every
        later position two vector-matrix products with folds the sweep holds anyway give the mixed partial -- where the
        analytic ``eval_multi_batch`` walks one chain per (row, spec), ``1 + 2 d + d (d - 1) / 2`` of them.  The carried
        vectors live in LDS, so the left sweep runs in as many passes as the model needs; a row's bits depend neither on
        that nor on the batch, and the value, the gradient and ``diag(hess)`` are ``gradient_batch(points, second=True)``'s
        bit for bit.

        The returns are views of one ``(N, C)`` result, ``C = 1 + d + d * d``: column 0 the value, ``1 + u`` the
        gradient, ``1 + d + u * d + v`` the Hessian.  Host points give NumPy arrays, ``hess = res[:, 1 + d:].reshape(N,
        d, d)``; a device array in, or a device ``out=``, gives :class:`~pychebyshev_amd.device.DeviceColumns` of one
        :class:`~pychebyshev_amd.device.DeviceArray`, complete on return, ``hess`` then ``(N, d * d)``, row-major in
        ``(u, v)``.  ``out=`` is the ``(N, C)`` result preallocated, as in :meth:`gradient_batch`."""
        self._check_built()
        from .device import DeviceColumns
        d = self.num_dimensions
        C = 1 + d + d * d
        res = self._sweep_batch(points, out, C, "pcx_tt_hess_batch", 0)      # block = 0: the planner's
        if isinstance(res, np.ndarray):
            return res[:, 0], res[:, 1:1 + d], res[:, 1 + d:].reshape(res.shape[0], d, d)
        return DeviceColumns(res, 0, 1, squeeze=True), DeviceColumns(res, 1, 1 + d), DeviceColumns(res, 1 + d, C)

    def hessian(self, point):
        """Value, gradient and Hessian at one point, ``(float, (d,) array, (d, d) array)``: row 0 of a one-row
        :meth:`hessian_batch`."""
        value, grad, hess = self.hessian_batch(np.asarray([list(point)], dtype=float))
        return float(value[0]), np.array(grad[0]), np.array(hess[0])

    def _eval_multi_batch_host(self, points, derivative_orders, *, chunk: int = 1 << 18) -> np.ndarray:
        """The finite-difference rules on NumPy columns -- the same record / replay traversal as :meth:`eval_multi`
        with columns in place of floats; all stencil points of a chunk of rows go to the device in one batch.
        Kept for specs the device rules do not take (more than three differenced dimensions) and as the
        row-by-row cross-check of the device path in the tests."""
        self._check_built()
        d = self.num_dimensions
        pts = np.asarray(points, dtype=float)
        if pts.ndim != 2 or pts.shape[1] != d:
            raise ValueError(f"points must have shape (N, {d}), got {pts.shape}")
        order = self._dim_order
        specs = [[int(s[order[k]]) for k in range(d)] for s in derivative_orders]
        for spec in specs:
            for o in spec:
                if o not in (0, 1, 2):
                    raise ValueError(f"Derivative order {o} not supported (use 1 or 2)")
        out = np.empty((pts.shape[0], len(specs)))
        if pts.shape[0] == 0:
            return out
        # stencil points per row: one dry traversal with scalars
        n_stencil = [0]

        def count(_q):
            n_stencil[0] += 1
            return 0.0
        for spec in specs:
            self._fd_spec([float(v) for v in pts[0, order]], spec, count)
        for start in range(0, pts.shape[0], max(1, int(chunk))):
            block = pts[start:start + chunk]
            n = block.shape[0]
            cols = [np.ascontiguousarray(block[:, order[k]]) for k in range(d)]       # storage frame
            # all stencil points of the block, written straight into the batch the device gets (user frame:
            # storage dimension k is user column order[k])
            batch = np.empty((n_stencil[0] * n, d))
            filled = [0]

            def run(value_of):
                return [self._fd_spec(cols, spec, value_of) for spec in specs]

            def record(q):
                lo = filled[0] * n
                for k in range(d):
                    batch[lo:lo + n, order[k]] = q[k]
                filled[0] += 1
                return 0.0

            run(record)                               # pass 1: collect the stencil columns
            vals = self._eval_user_points(batch)
            it = iter(np.split(vals, n_stencil[0]))
            res = run(lambda q: next(it))             # pass 2: same traversal, real values
            for j, r in enumerate(res):
                out[start:start + n, j] = r
        return out

    def to_dense(self) -> np.ndarray:
        """Full tensor of values on the Chebyshev grid, axes in the user's dimension order
        (reference :1874-1917).  One device batch over all ``prod(n_nodes)`` grid points
        replaces the reference's einsum chain over value cores."""
        self._check_built()
        d = self.num_dimensions
        grids = [np.sort(0.5 * (a + b) + 0.5 * (b - a) * chebpts1(n))
                 for (a, b), n in zip(self.domain, self.n_nodes)]          # storage frame
        mesh = np.meshgrid(*grids, indexing="ij")
        pts_storage = np.column_stack([m.ravel() for m in mesh])
        vals = self._eval_user_points(self._storage_to_user(pts_storage))
        dense = vals.reshape(tuple(self.n_nodes))
        if self._dim_order != list(range(d)):
            inv = [0] * d
            for pos, orig in enumerate(self._dim_order):
                inv[orig] = pos
            dense = np.transpose(dense, axes=inv)
        return dense

    def eval_grid(self, axes) -> np.ndarray:
        """The interpolant on the tensor-product grid ``axes[0] x ... x axes[d-1]`` (extension): ``axes`` in the USER's
        dimension order, ``result[i_0, ..., i_{d-1}] = eval([axes[0][i_0], ...])``, a NumPy array of shape
        ``(m_0, ..., m_{d-1})`` with its axes in the user's order too.

        The host forms the value cores on the grid, ``G_k[a, i, b] = sum_j T_j(t_k(x_i)) coeff_core_k[a, j, b]`` with
        ``x = axes[dim_order[k]]`` (tiny), the device multiplies the chain out into the dense tensor
        (``pcx_tt_tensor_grid``: d - 1 mode products), and the host transposes storage order to user order as
        :meth:`to_dense` does.  ``sum_k m_k r_k r_{k+1} n_k`` plus about ``2 r prod m`` flops, where ``eval_batch``
        over the meshgrid pays the whole chain per point."""
        self._check_built()
        from numpy.polynomial.chebyshev import chebvander
        from .barycentric import _grid_axes
        d = self.num_dimensions
        ax = _grid_axes(axes, d)
        grid_cores = []
        for k, core in enumerate(self._coeff_cores):
            a, b = self.domain[k]
            t = 2.0 * (ax[self._dim_order[k]] - a) / (b - a) - 1.0
            basis = chebvander(t, core.shape[1] - 1)                       # (m_k, n_k)
            grid_cores.append(np.einsum("ij,ajb->aib", basis, core))
        m = _lib.i32([g.shape[1] for g in grid_cores])
        ranks = _lib.i32([1] + [g.shape[2] for g in grid_cores])
        cat = _lib.f64(np.concatenate([g.ravel() for g in grid_cores]))
        dense = np.empty(tuple(int(v) for v in m))
        lib = _lib.load()
        dev = _lib.default_device() if self._device_index is None else self._device_index
        _lib.check(lib.pcx_tt_tensor_grid(int(dev), d, _lib.p_i32(m), _lib.p_i32(ranks), _lib.p_f64(cat), _lib.p_f64(dense)), lib)
        if self._dim_order != list(range(d)):
            inv = [0] * d
            for pos, orig in enumerate(self._dim_order):
                inv[orig] = pos
            dense = np.transpose(dense, axes=inv)
        return dense

    # finite-difference rules, all in storage frame (reference :2322-2463)
    def _fd_step(self, k: int) -> float:
        a, b = self.domain[k]
        return (b - a) * 1e-4

    def _nudge(self, p, k: int, h: float):
        """``p`` is a point (list of floats) or, for the batched rules, a list of ``(N,)`` columns."""
        p = list(p)
        a, b = self.domain[k]
        need = h * 1.5
        if isinstance(p[k], np.ndarray):
            x = np.where(p[k] - a < need, a + need, p[k])
            p[k] = np.where(b - x < need, b - need, x)
            return p
        if p[k] - a < need:
            p[k] = a + need
        if b - p[k] < need:
            p[k] = b - need
        return p

    @staticmethod
    def _moved(p, k, delta):
        q = list(p)
        q[k] = q[k] + delta
        return q

    def _fd_nested(self, p, active, value_of):
        if not active:
            return value_of(p)
        (k, o), rest = active[0], active[1:]
        h = self._fd_step(k)
        p = self._nudge(p, k, h)
        if o == 1:
            up = self._fd_nested(self._moved(p, k, h), rest, value_of)
            dn = self._fd_nested(self._moved(p, k, -h), rest, value_of)
            return (up - dn) / (2.0 * h)
        if o == 2:
            up = self._fd_nested(self._moved(p, k, h), rest, value_of)
            mid = self._fd_nested(p, rest, value_of)
            dn = self._fd_nested(self._moved(p, k, -h), rest, value_of)
            return (up - 2.0 * mid + dn) / (h * h)
        raise ValueError(f"Derivative order {o} not supported (use 1 or 2)")

    def _fd_spec(self, pt, spec, value_of):
        active = [(k, o) for k, o in enumerate(spec) if o > 0]
        if len(active) == 2 and active[0][1] == 1 and active[1][1] == 1:
            (k1, _), (k2, _) = active
            h1, h2 = self._fd_step(k1), self._fd_step(k2)
            p = self._nudge(self._nudge(pt, k1, h1), k2, h2)

            def at(s1, s2):
                q = list(p)
                q[k1] = q[k1] + s1 * h1               # not +=: the batched rules pass NumPy columns
                q[k2] = q[k2] + s2 * h2
                return value_of(q)
            f_pp, f_pm, f_mp, f_mm = at(+1, +1), at(+1, -1), at(-1, +1), at(-1, -1)
            return (f_pp - f_pm - f_mp + f_mm) / (4.0 * h1 * h2)
        return self._fd_nested(pt, active, value_of)

    # ---------------------------------------------------------------- properties
    @property
    def tt_ranks(self) -> List[int]:
        self._check_built()
        return list(self._tt_ranks)

    @property
    def compression_ratio(self) -> float:
        self._check_built()
        return int(np.prod(self.n_nodes)) / sum(c.size for c in self._coeff_cores)

    @property
    def total_build_evals(self) -> int:
        return self._total_build_evals

    @property
    def dim_order(self) -> List[int]:
        return list(self._dim_order)

    def is_construction_finished(self) -> bool:
        return self._built

    def get_used_ns(self) -> List[int]:
        return list(self.n_nodes)

    def get_num_evaluation_points(self) -> int:
        """Size of the full tensor grid (what a dense build would evaluate)."""
        return int(np.prod(self.n_nodes))

    def get_evaluation_points(self) -> np.ndarray:
        """Full Cartesian grid of the storage-frame nodes, rows in C order over the storage
        dimensions, columns in the user's frame (reference :2775-2800)."""
        per_dim = [np.sort(0.5 * (a + b) + 0.5 * (b - a) * chebpts1(n))
                   for (a, b), n in zip(self.domain, self.n_nodes)]
        grids = np.meshgrid(*per_dim, indexing="ij")
        cols = [grids[self._dim_order.index(u)] for u in range(self.num_dimensions)]
        return np.stack([g.ravel() for g in cols], axis=-1).astype(np.float64)

    @staticmethod
    def nodes(num_dimensions: int, domain, n_nodes) -> dict:
        """Per-dimension type-I nodes a ``from_values`` tensor must be sampled at (reference :3122-3156)."""
        from . import Domain, Ns
        from .barycentric import chebyshev_nodes
        if isinstance(domain, Domain):
            domain = list(domain.bounds)
        if isinstance(n_nodes, Ns):
            n_nodes = list(n_nodes.counts)
        if len(domain) != num_dimensions or len(n_nodes) != num_dimensions:
            raise ValueError(f"domain and n_nodes must have length {num_dimensions}")
        return {"nodes_per_dim": [chebyshev_nodes(domain[k][0], domain[k][1], n_nodes[k])
                                  for k in range(num_dimensions)]}

    def sobol_indices(self) -> dict:
        """First- and total-order Sobol indices by contracting the coefficient cores (reference
        tensor_train.py:2823-2870): ``{"first_order": {dim: index}, "total_order": {dim: index},
        "variance": float}``, keyed by the user's dimensions through ``dim_order``.  Host NumPy, cost
        O(d n r^2): the cores are small and there is no dense tensor."""
        if not self._built:
            raise RuntimeError("Call build() first")
        first, total, variance = _sobol_from_coeff_cores(self._coeff_cores)
        user = self._dim_order                  # storage position s holds user dimension user[s]
        return {"first_order": {user[s]: float(first[s]) for s in range(self.num_dimensions)},
                "total_order": {user[s]: float(total[s]) for s in range(self.num_dimensions)},
                "variance": variance}

    # ---------------------------------------------------------------- calculus
    def _user_frame_domain(self) -> list:
        """``domain`` indexed by user dimension: user dimension u lives at storage position ``_dim_order.index(u)``."""
        return [self.domain[self._dim_order.index(u)] for u in range(self.num_dimensions)]

    # _calculus.FibreCalculusMixin's methods over these hooks: ``dim``, ``fixed`` and the rows' columns are in the
    # user's frame, the handle applies ``dim_order``; below, what this class adds to their docstrings.
    _fibre_prefix = "pcx_tt"
    _ladder_own_stream = True
    _fibre_domain = _user_frame_domain

    def _fibre_counts(self):
        return [self.n_nodes[self._dim_order.index(u)] for u in range(self.num_dimensions)]

    def _domain_arrays(self):
        return ()                                   # the handle knows its domain: the entries take no lo / hi

    def _fibre_grid(self, dim: int):
        """The grid of user dimension ``dim``, built only where a single call finishes on the host (above 64 nodes)."""
        from .barycentric import chebyshev_nodes, compute_barycentric_weights, compute_differentiation_matrix
        pos = self._dim_order.index(dim)
        n, (a, b) = int(self.n_nodes[pos]), self.domain[pos]
        if n <= _calculus.MAX_DEVICE_N:
            return None, None, None, (a, b)
        nodes = chebyshev_nodes(a, b, n)
        weights = compute_barycentric_weights(nodes)
        return nodes, weights, compute_differentiation_matrix(nodes, weights), (a, b)

    def _fibre_values(self, points) -> np.ndarray:
        return self.eval_batch(points)

    def roots(self, dim=None, fixed=None, *, level=0.0) -> np.ndarray:
        """:meth:`FibreCalculusMixin.roots <pychebyshev_amd._calculus.FibreCalculusMixin.roots>`, ``level`` included,
        along user dimension ``dim`` (reference tensor_train.py:1749-1790): the fibre is the TT's values at the nodes of
        ``dim``.  ``dim`` and ``fixed`` are in the user's frame."""
        return super().roots(dim, fixed, level=level)

    def minimize(self, dim=None, fixed=None):
        """:meth:`FibreCalculusMixin.minimize <pychebyshev_amd._calculus.FibreCalculusMixin.minimize>` along user
        dimension ``dim`` (reference tensor_train.py:1792-1831)."""
        return super().minimize(dim, fixed)

    def maximize(self, dim=None, fixed=None):
        """:meth:`FibreCalculusMixin.maximize <pychebyshev_amd._calculus.FibreCalculusMixin.maximize>` along user
        dimension ``dim`` (reference tensor_train.py:1833-1872)."""
        return super().maximize(dim, fixed)

    def roots_batch(self, dim: int, fixed, *, level=None):
        """:meth:`FibreCalculusMixin.roots_batch <pychebyshev_amd._calculus.FibreCalculusMixin.roots_batch>`, ``level``
        included, along user dimension ``dim`` (extension; columns = the other user dimensions in increasing order)."""
        return super().roots_batch(dim, fixed, level=level)

    def ladder_batch(self, dim: int, fixed, xs, *, out=None):
        """The model along user dimension ``dim`` at ``m`` values for every row of ``fixed`` (extension; as
        ``ChebyshevApproximation.ladder_batch``): ``result[r, x] = eval(point)`` at the point whose coordinate along
        ``dim`` is the row's x-th value and whose other coordinates are ``fixed[r]`` (``(N, d-1)``, the other user
        dimensions in increasing order), shape ``(N, m)``.  ``xs`` is ``(m,)`` shared or ``(N, m)`` per row and is not
        checked against the domain; ``fixed`` is (``ValueError`` before any device call); NaN in ``fixed`` makes its
        row NaN, in ``xs`` its own cell.  ``fixed``, a per-row ``xs`` and ``out=`` may be device arrays, as there.

        The row's left and right chains and the ``n`` Chebyshev coefficients of its restriction to ``dim`` are formed
        once (``pcx_tt_ladder_batch``), each value is then that series: about one evaluation per row plus ``n`` FMAs
        per value, where ``eval_batch`` on the ``N m`` points walks the whole train ``m`` times per row.

        The call takes no derivative spec: a Greek ladder is ``tt.differentiate(spec).ladder_batch(...)``."""
        return self._ladder(dim, fixed, xs, out)

    def fibre_batch(self, dim: int, fixed, *, out=None):
        """Every row's restriction to user dimension ``dim`` at that dimension's ascending nodes (the grid
        :meth:`nodes` gives), ``(N, n_dim)``: :meth:`ladder_batch` at those nodes, bit for bit.  No derivative spec:
        ``tt.differentiate(spec).fibre_batch(...)``."""
        from .barycentric import chebyshev_nodes
        self._fibre_check_built()
        _calculus.validate_dim(self.num_dimensions, dim)
        pos = self._dim_order.index(int(dim))
        a, b = self.domain[pos]
        return self.ladder_batch(dim, fixed, chebyshev_nodes(a, b, int(self.n_nodes[pos])), out=out)

    def invert_batch(self, dim: int, fixed, targets):
        """:meth:`FibreCalculusMixin.invert_batch <pychebyshev_amd._calculus.FibreCalculusMixin.invert_batch>`
        (``status`` as there).  ``dim`` and the columns of ``fixed`` are in the user's frame."""
        return super().invert_batch(dim, fixed, targets)

    def minimize_batch(self, dim: int, fixed):
        """:meth:`FibreCalculusMixin.minimize_batch <pychebyshev_amd._calculus.FibreCalculusMixin.minimize_batch>`
        along user dimension ``dim``."""
        return super().minimize_batch(dim, fixed)

    def maximize_batch(self, dim: int, fixed):
        """:meth:`FibreCalculusMixin.maximize_batch <pychebyshev_amd._calculus.FibreCalculusMixin.maximize_batch>`
        along user dimension ``dim``."""
        return super().maximize_batch(dim, fixed)

    def error_estimate(self) -> float:
        """Sum over dimensions of the largest last Chebyshev coefficient (reference :2469-2504)."""
        self._check_built()
        if self._cached_error_estimate is None:
            self._cached_error_estimate = float(sum(np.max(np.abs(c[:, -1, :])) for c in self._coeff_cores))
        return self._cached_error_estimate

    # ---------------------------------------------------------------- orthogonalisation and completion
    # Reference tensor_train.py:1296-1436.  Both act in place; every argument check runs before the library is loaded.
    def _set_cores(self, cores) -> None:
        """New cores in place: the ranks follow the cores' bonds, the device handle and the cached error estimate go."""
        self._coeff_cores = cores
        self._tt_ranks = [c.shape[0] for c in cores] + [cores[-1].shape[2]]
        self._cached_error_estimate = None
        self.invalidate_device_cache()

    def _orth(self, side: int, position: int) -> None:
        from . import _algebra
        lib = _lib.load()
        n, ranks, cat = _algebra._shape_args(self._coeff_cores)
        out = np.empty(cat.size)
        ranks_out = np.empty(self.num_dimensions + 1, dtype=np.int32)
        length = ctypes.c_int64(0)
        dev = _lib.default_device() if self._device_index is None else self._device_index
        _lib.check(lib.pcx_tt_orth(int(dev), self.num_dimensions, _lib.p_i32(n), _lib.p_i32(ranks), _lib.p_f64(cat),
                                   int(side), int(position), _lib.p_i32(ranks_out), _lib.p_f64(out), out.size,
                                   ctypes.byref(length)), lib)
        self._set_cores(_algebra._split(out, n, ranks_out))

    def orth_left(self, position: int) -> None:
        """Left-orthogonalise cores ``[0 .. position-1]`` in place (reference :1296-1325): each, unfolded as
        ``(r_k n_k, r_{k+1})``, gets orthonormal columns, the R factors move right into ``core[position]``; the tensor
        is unchanged.  Householder QR on the device (``pcx_tt_orth``).  An unfolding wider than tall comes back with
        the smaller bond, and ``tt_ranks`` follows."""
        self._check_built()
        d = self.num_dimensions
        if not (1 <= position < d):
            raise ValueError(f"position must be in [1, {d - 1}] for orth_left, got {position}")
        self._orth(0, position)

    def orth_right(self, position: int) -> None:
        """Right-orthogonalise cores ``[position+1 .. d-1]`` in place (reference :1327-1356): each, unfolded as
        ``(r_k, n_k r_{k+1})``, gets orthonormal rows, the factors move left; the tensor is unchanged."""
        self._check_built()
        d = self.num_dimensions
        if not (0 <= position < d - 1):
            raise ValueError(f"position must be in [0, {d - 2}] for orth_right, got {position}")
        self._orth(1, position)

    completion_info = None      # set by run_completion: {"iterations", "rel_change", "grid_residual"}

    def run_completion(self, tolerance: float = 1e-8, max_iter: int = 50, verbose: bool = False, *, values=None) -> None:
        """Refine the TT at its current rank by alternating least squares against the function's values on the whole
        tensor grid (reference :1358-1436).  All outer iterations run in one device call (``pcx_tt_als``): with the
        neighbouring cores orthonormal each core's solve is a projection of the target, see DESIGN.md.

        ``values`` (extension, keyword only): the target as a dense tensor of shape ``tuple(self.n_nodes)`` in the
        storage frame, in ``from_values``' node order, instead of the callback -- so a TT without ``function``
        (``from_values``, ``reorder``, algebra results, loaded models) can be completed.  Without it the grid is filled
        through ``self.function(point, additional_data)`` as ``build(method="svd")`` fills it.

        Stops when ``||T_new - T_old||_F / ||T_old||_F < tolerance`` after an outer iteration, or after ``max_iter``
        of them (``max_iter <= 0``: none).  ``self.completion_info`` records the iterations run, the ``rel_change``
        history and ``grid_residual = ||TT - T||_F / ||T||_F`` of the final cores."""
        self._check_built()
        n = [int(v) for v in self.n_nodes]
        d = self.num_dimensions
        if values is None:
            if self.function is None:
                raise RuntimeError("run_completion requires self.function to be callable; "
                                   "the TT was loaded from a source without the original function.")
            grids = [np.sort(0.5 * (a + b) + 0.5 * (b - a) * chebpts1(nk)) for (a, b), nk in zip(self.domain, n)]
            data, raw = self.additional_data, self.function
            target = np.empty(n)
            for idx in np.ndindex(*n):
                target[idx] = raw([float(grids[k][idx[k]]) for k in range(d)], data)
        else:
            target = np.asarray(values, dtype=np.float64)
            if target.shape != tuple(n):
                raise ValueError(f"values shape {target.shape} does not match expected {tuple(n)}")
            if not np.isfinite(target).all():
                raise ValueError("values contains NaN or Inf — all values must be finite")
        from . import _algebra
        lib = _lib.load()
        value_cores = [_coeff_core_to_value_core(c) for c in self._coeff_cores]
        nn, ranks, cat = _algebra._shape_args(value_cores)
        target = _lib.f64(target)
        out = np.empty(cat.size)
        ranks_out = np.empty(d + 1, dtype=np.int32)
        length, iters, resid = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_double(0.0)
        history = np.zeros(max(int(max_iter), 1))
        dev = _lib.default_device() if self._device_index is None else self._device_index
        _lib.check(lib.pcx_tt_als(int(dev), d, _lib.p_i32(nn), _lib.p_i32(ranks), _lib.p_f64(cat), _lib.p_f64(target.ravel()),
                                  float(tolerance), int(max_iter), _lib.p_i32(ranks_out), _lib.p_f64(out), out.size,
                                  ctypes.byref(length), ctypes.byref(iters), _lib.p_f64(history), ctypes.byref(resid)), lib)
        refined = _algebra._split(out, nn, ranks_out)
        self._set_cores([_value_core_to_coeff_core(c) for c in refined])
        rel = [float(v) for v in history[: int(iters.value)]]
        if verbose:
            for i, x in enumerate(rel):
                print(f"  ALS iter {i + 1}: rel_change = {x:.3e}")
        self.completion_info = {"iterations": int(iters.value), "rel_change": rel, "grid_residual": float(resid.value)}

    # ---------------------------------------------------------------- fitting to scattered samples
    fit_info = None             # set by fit_samples: {"iterations", "residual", "n_samples"}

    def _check_samples(self, points, values, ridge):
        """The argument checks of ``fit_samples``, before the library is loaded for host arrays: ``(points in STORAGE
        column order, values, N)``, both NumPy arrays or both device arrays."""
        from .device import is_device_array
        d = self.num_dimensions
        ridge = float(ridge)
        if not (ridge >= 0.0) or not np.isfinite(ridge):
            raise ValueError(f"ridge must be finite and >= 0, got {ridge!r}")
        identity = self._dim_order == list(range(d))
        if is_device_array(points) or is_device_array(values):
            from .device import DeviceArray, as_device_array
            dp = as_device_array(points) if is_device_array(points) else DeviceArray.from_host(_checked_sample_points(points, d))
            dv = as_device_array(values) if is_device_array(values) else DeviceArray.from_host(_checked_sample_values(values))
            if dp.ndim != 2 or dp.shape[1] != d:
                raise ValueError(f"points must have shape (N, {d}), got {dp.shape}")
            if dv.ndim != 1 or dv.shape[0] != dp.shape[0]:
                raise ValueError(f"values must have shape ({dp.shape[0]},), got {dv.shape}")
            if dp.shape[0] < 1:
                raise ValueError("at least one sample is needed")
            if dp.device != dv.device:
                raise ValueError(f"points live on device {dp.device} but values on device {dv.device}")
            if not identity:       # the session takes storage-order columns: a permuted model stages the points through the host
                dp = DeviceArray.from_host(dp.to_host()[:, self._dim_order], dp.device)
            return dp, dv, dp.shape[0]
        pts = _checked_sample_points(points, d)
        vals = _checked_sample_values(values)
        if vals.shape[0] != pts.shape[0]:
            raise ValueError(f"values must have shape ({pts.shape[0]},), got {vals.shape}")
        if pts.shape[0] < 1:
            raise ValueError("at least one sample is needed")
        if not np.isfinite(vals).all():
            raise ValueError("values contain NaN or Inf — every sample must be finite")
        if not np.isfinite(pts).all():
            raise ValueError("points contain NaN or Inf — every sample must be finite")
        user_domain = self._user_frame_domain()
        for u, (a, b) in enumerate(user_domain):
            col = pts[:, u]
            if col.min() < a or col.max() > b:
                raise ValueError(f"points[:, {u}] leaves the domain [{a}, {b}] of dimension {u}: a Chebyshev basis "
                                 "extrapolates explosively, drop or clip those samples")
        if not identity:
            pts = np.ascontiguousarray(pts[:, self._dim_order])
        return pts, vals, pts.shape[0]

    def fit_samples(self, points, values, *, max_iter: int = 20, tolerance: float = 1e-10, ridge: float = 1e-12,
                    verbose: bool = False) -> None:
        """Least-squares fit of the TT, at its current ranks and in place, to samples at arbitrary points (extension):
        minimises ``sum_i (TT(x_i) - y_i)^2`` by alternating least squares over the coefficient cores.

        ``points`` is ``(N, d)`` in the user's dimension order and ``values`` ``(N,)``; NumPy arrays, or device arrays
        (:class:`~pychebyshev_amd.device.DeviceArray` or anything with ``__cuda_array_interface__``), which the fit
        reads where they are.  Every coordinate must be finite and inside its dimension's domain and every value finite.

        The algorithm: (1) cores ``d-1 .. 1`` are right-orthogonalised (QR of the unfoldings); (2) one outer iteration
        visits the positions ``0, 1, .., d-1, d-2, .., 1``; (3) at position ``k`` the design row of sample ``i`` is
        ``a_i = L_i (x) T(t_k(x_ik)) (x) R_i`` in the core's own C order, ``L_i`` / ``R_i`` the partial products of the
        chain on either side; (4) ``G = A^T A``, ``b = A^T y`` are accumulated on the device (``pcx_tt_fit_normal``,
        ``csrc/tt_fit_kernels.h``: the ``N x P`` matrix is never formed in memory) and ``lam = ridge trace(G) / P``;
        (5) ``(G + lam I) c = b`` is solved on the host (a Cholesky factorisation tests that it is positive definite) and
        becomes core ``k``; (6) the orthogonality
        centre moves one step towards the next position (a QR of the core's unfolding, the factor absorbed into the
        neighbour; a bond shrinks where the unfolding cannot hold it); (7) after each outer iteration ``res =
        ||TT(x) - y|| / ||y||`` on the samples (``pcx_tt_fit_residual``) and the loop stops when ``|res_prev - res| <=
        tolerance res_prev``, when ``res == 0`` or after ``max_iter`` iterations (``max_iter <= 0``: none).

        ``self.fit_info`` records ``iterations``, the ``residual`` history and ``n_samples``.  With ``ridge == 0``
        ``N`` must be at least the largest number of unknowns of a position.  A system that is not positive definite
        raises ``ValueError`` naming the position.  The samples are uploaded (or adopted) once per call."""
        self._check_built()
        pts, vals, N = self._check_samples(points, values, ridge)
        ridge, tolerance, max_iter = float(ridge), float(tolerance), int(max_iter)
        if tolerance != tolerance:
            raise ValueError("tolerance is NaN")
        d = self.num_dimensions
        cores = [np.array(c, dtype=np.float64) for c in self._coeff_cores]
        sizes = [c.size for c in cores]
        if ridge == 0.0 and N < max(sizes):
            k = int(np.argmax(sizes))
            raise ValueError(f"{N} samples cannot determine the {sizes[k]} unknowns of position {k} "
                             f"(core shape {cores[k].shape}) with ridge = 0: pass more samples, lower the rank or set ridge > 0")
        history: List[float] = []
        if max_iter > 0:
            session = _FitSession(self, pts, vals, N)
            try:
                for k in range(d - 1, 0, -1):
                    _fit_move_centre(cores, k, k - 1)
                order = list(range(d)) + list(range(d - 2, 0, -1))
                for it in range(max_iter):
                    for i, k in enumerate(order):
                        G, b = session.normal(cores, k)
                        P = b.size
                        lam = ridge * float(np.trace(G)) / P
                        if lam:
                            G[np.diag_indices(P)] += lam
                        try:
                            chol = np.linalg.cholesky(G)
                        except np.linalg.LinAlgError:
                            raise ValueError(f"the normal equations of position {k} ({P} unknowns, {N} samples) are not "
                                             f"positive definite: the samples do not determine this core; raise ridge "
                                             f"(now {ridge:g}), lower the rank or pass more samples") from None
                        del chol                                   # the factorisation is the definiteness test; LAPACK's
                        c = np.linalg.solve(G, b)                  # solver (NumPy has no triangular one) gives the solution
                        cores[k] = c.reshape(cores[k].shape)
                        nxt = order[(i + 1) % len(order)]
                        if nxt != k:
                            _fit_move_centre(cores, k, nxt)
                    res = session.residual(cores)
                    history.append(res)
                    if verbose:
                        print(f"  fit_samples iter {it + 1}: residual = {res:.6e}")
                    if res == 0.0 or (it > 0 and abs(history[-2] - res) <= tolerance * history[-2]):
                        break
            finally:
                session.close()
            self._set_cores(cores)
        self.fit_info = {"iterations": len(history), "residual": history, "n_samples": int(N)}

    @classmethod
    def from_samples(cls, points, values, num_dimensions: int, domain, n_nodes, *, rank: int, seed=None,
                     max_iter: int = 20, tolerance: float = 1e-10, ridge: float = 1e-12, max_derivative_order: int = 2,
                     descriptor: str = "") -> "ChebyshevTT":
        """A TT of fixed ``rank`` fitted to samples ``(points (N, d), values (N,))`` at arbitrary points of ``domain``
        (extension).  The start is random: ``np.random.default_rng(seed).standard_normal((r_l, n_k, r_r))`` core by core
        from ``k = 0``, every interior bond ``min(rank, prod(n[:k]), prod(n[k:]))``; then :meth:`fit_samples`.  The result
        has ``function = None``, ``method = "samples"`` and the identity ``dim_order``."""
        from . import Domain, Ns
        if isinstance(domain, Domain):
            domain = list(domain.bounds)
        if isinstance(n_nodes, Ns):
            n_nodes = list(n_nodes.counts)
        d = int(num_dimensions)
        if int(rank) != rank or int(rank) < 1:
            raise ValueError(f"rank must be a positive integer, got {rank!r}")
        n = [int(v) for v in n_nodes]
        if len(domain) != d or len(n) != d:
            raise ValueError(f"domain and n_nodes must have {d} entries, got {len(domain)} and {len(n)}")
        if min(n) < 1:
            raise ValueError(f"every dimension needs at least one node, got {n}")
        for k, (a, b) in enumerate(domain):
            if not (np.isfinite(a) and np.isfinite(b) and a < b):
                raise ValueError(f"domain of dimension {k} must be finite with lo < hi, got {(a, b)}")
        bonds = _fit_start_ranks(n, int(rank))
        obj = cls(None, d, [list(b) for b in domain], n, max_rank=int(rank), tolerance=float(tolerance),
                  max_derivative_order=max_derivative_order)
        obj.descriptor = descriptor
        obj.method = "samples"
        rng = np.random.default_rng(seed)
        obj._coeff_cores = [rng.standard_normal((bonds[k], n[k], bonds[k + 1])) for k in range(d)]
        obj._tt_ranks = list(bonds)
        obj._built = True
        start = time.time()
        obj.fit_samples(points, values, max_iter=max_iter, tolerance=tolerance, ridge=ridge)
        obj._build_time = time.time() - start
        return obj

    # ---------------------------------------------------------------- algebra
    # Reference tensor_train.py:3287-3458 and :2575-2676.  Scalars scale core 0 on the host; a sum stacks the cores
    # block-diagonally (ranks r_a + r_b) and rounds them back on the device (pcx_tt_round); reorder runs its adjacent
    # swaps on the device (pcx_tt_reorder).  Every result is a new object: the in-place forms rebind the name.
    def _derived(self, cores, *, max_rank=None, domain=None, n_nodes=None, dim_order=None) -> "ChebyshevTT":
        obj = self.__class__.__new__(self.__class__)
        obj.function = None
        obj.num_dimensions = len(cores)
        obj.domain = list(self.domain if domain is None else domain)
        obj.n_nodes = list(self.n_nodes if n_nodes is None else n_nodes)
        obj.max_rank = self.max_rank if max_rank is None else max_rank
        obj.tolerance = self.tolerance
        obj.max_sweeps = self.max_sweeps
        obj.max_derivative_order = self.max_derivative_order
        obj.additional_data = self.additional_data
        obj.descriptor = self.descriptor
        obj.method = self.method
        obj._coeff_cores = cores
        obj._tt_ranks = [c.shape[0] for c in cores] + [cores[-1].shape[2]]
        obj._built = True
        obj._build_time = 0.0
        obj._total_build_evals = 0
        obj._cached_error_estimate = None
        obj._dim_order = list(self._dim_order if dim_order is None else dim_order)
        obj._device_tt = None
        obj._device_index = self._device_index
        return obj

    def _check_compatible_tt(self, other) -> None:
        if not isinstance(other, ChebyshevTT):
            raise TypeError(f"unsupported operand type for ChebyshevTT: {type(other).__name__}")
        self._check_built()
        other._check_built()
        if self.num_dimensions != other.num_dimensions:
            raise ValueError(f"num_dimensions mismatch: {self.num_dimensions} vs {other.num_dimensions}")
        if list(self.n_nodes) != list(other.n_nodes):
            raise ValueError(f"n_nodes mismatch: {self.n_nodes} vs {other.n_nodes}")
        if not np.allclose(np.asarray(self.domain, dtype=float), np.asarray(other.domain, dtype=float)):
            raise ValueError(f"domain mismatch: {self.domain} vs {other.domain}")
        if self._dim_order != other._dim_order:
            raise ValueError(f"TT dim_order mismatch: {self._dim_order} vs {other._dim_order}. "
                             "Call other = other.reorder(self.dim_order) (or self = "
                             "self.reorder(other.dim_order)) to align before adding/subtracting.")

    def __add__(self, other: "ChebyshevTT") -> "ChebyshevTT":
        """Sum: block-diagonal stacking, then rounding on the device to ``max(self.max_rank, other.max_rank)``
        with ``self.tolerance`` as the relative singular-value cutoff."""
        from . import _algebra
        self._check_compatible_tt(other)
        target = max(self.max_rank, other.max_rank)
        stacked = _algebra.tt_stack(self._coeff_cores, other._coeff_cores)
        if self.num_dimensions > 1:
            dev = _lib.default_device() if self._device_index is None else self._device_index
            stacked = _algebra.tt_round(stacked, target, self.tolerance, dev)
        return self._derived(stacked, max_rank=target)

    def __sub__(self, other: "ChebyshevTT") -> "ChebyshevTT":
        return self + (-other)

    def __neg__(self) -> "ChebyshevTT":
        return self._scaled(-1.0)

    def _scaled(self, s: float) -> "ChebyshevTT":
        self._check_built()
        cores = [c.copy() for c in self._coeff_cores]
        cores[0] = cores[0] * s
        return self._derived(cores)

    def __mul__(self, scalar) -> "ChebyshevTT":
        from . import _algebra
        if not _algebra.is_scalar(scalar):
            raise TypeError(f"ChebyshevTT * {type(scalar).__name__} is not supported "
                            "(only scalar multiplication is defined for TT)")
        return self._scaled(float(scalar))

    def __rmul__(self, scalar) -> "ChebyshevTT":
        return self.__mul__(scalar)

    def __truediv__(self, scalar) -> "ChebyshevTT":
        from . import _algebra
        if not _algebra.is_scalar(scalar):
            raise TypeError(f"ChebyshevTT / {type(scalar).__name__} is not supported")
        if float(scalar) == 0.0:
            raise ZeroDivisionError("division by zero")
        return self.__mul__(1.0 / float(scalar))

    def __iadd__(self, other) -> "ChebyshevTT":
        return self + other

    def __isub__(self, other) -> "ChebyshevTT":
        return self - other

    def __imul__(self, scalar) -> "ChebyshevTT":
        return self * scalar

    def __itruediv__(self, scalar) -> "ChebyshevTT":
        return self / scalar

    def reorder(self, new_order, *, max_rank=None, tolerance=None) -> "ChebyshevTT":
        """New TT whose storage order is ``new_order`` (reference :2575-2676): the current order is bubble-sorted into
        ``new_order`` by adjacent swaps, each one truncated SVD of the merged pair on the device, capped at
        ``max_rank`` (default ``self.max_rank``) with relative cutoff ``tolerance`` (default ``self.tolerance``)."""
        from . import _algebra
        self._check_built()
        new_order = list(new_order)
        d = self.num_dimensions
        if sorted(new_order) != list(range(d)):
            raise ValueError(f"new_order must be a permutation of range({d}); got {new_order!r}")
        if new_order == self._dim_order:
            return self.clone()
        eff_rank = self.max_rank if max_rank is None else max_rank
        eff_tol = self.tolerance if tolerance is None else tolerance
        current, n_nodes, domain = list(self._dim_order), list(self.n_nodes), list(self.domain)
        swaps = []
        for k in range(d):
            j = current.index(new_order[k])
            while j > k:
                swaps.append(j - 1)
                for lst in (current, n_nodes, domain):
                    lst[j - 1], lst[j] = lst[j], lst[j - 1]
                j -= 1
        dev = _lib.default_device() if self._device_index is None else self._device_index
        cores = _algebra.tt_swaps(self._coeff_cores, swaps, eff_rank, eff_tol, dev)
        return self._derived(cores, domain=domain, n_nodes=n_nodes, dim_order=new_order)

    # ---------------------------------------------------------------- slice / extrude / integrate / inner product
    # Reference tensor_train.py:1438-1702 and :1919-2125.  Host NumPy on the coefficient cores; dimensions in the
    # arguments are the USER's, the cores are walked by storage position.
    def slice(self, params) -> "ChebyshevTT":
        """Fix one or more user dimensions at given values (reference :2013-2125): ``(dim, value)`` or a list of
        them.  The core goes to value space and is contracted with the normalised barycentric weights -- or picked
        exactly when the value is within 1e-14 of a node -- and the matrix is absorbed into the right neighbour
        (the left one for the last core)."""
        from .barycentric import chebyshev_nodes, compute_barycentric_weights
        self._check_built()
        d = self.num_dimensions
        params = _slice_params(params, d)
        for dim_idx, value in params:
            lo, hi = self.domain[self._dim_order.index(dim_idx)]
            if value < lo or value > hi:
                raise ValueError(f"Slice value {value} for dim {dim_idx} is outside domain [{lo}, {hi}]")
        cores = list(self._coeff_cores)
        domain, n_nodes, live = list(self.domain), list(self.n_nodes), list(self._dim_order)
        placed = sorted(((self._dim_order.index(k), v) for k, v in params), reverse=True)
        for pos, value in placed:                     # from the back: earlier positions stay valid
            lo, hi = domain[pos]
            nodes = chebyshev_nodes(lo, hi, n_nodes[pos])
            values = _coeff_core_to_value_core(cores[pos])
            gap = value - nodes
            nearest = int(np.argmin(np.abs(gap)))
            if abs(gap[nearest]) < 1e-14:
                M = values[:, nearest, :]
            else:
                u = compute_barycentric_weights(nodes) / gap
                M = np.einsum("rjs,j->rs", values, u / np.sum(u))
            if pos < len(cores) - 1:
                cores[pos + 1] = np.einsum("lr,rjs->ljs", M, cores[pos + 1])
            else:
                cores[pos - 1] = np.einsum("ijs,sr->ijr", cores[pos - 1], M)
            for lst in (cores, domain, n_nodes, live):
                del lst[pos]
        order = _renumbered(live, d, {k for k, _ in params})
        return self._derived(cores, domain=domain, n_nodes=n_nodes, dim_order=order)

    def extrude(self, params) -> "ChebyshevTT":
        """Add dimensions along which the function is constant (reference :1919-2011): ``(dim, (lo, hi), n_nodes)``
        or a list of them, ``dim`` being the new dimension's index in the result.  The new core keeps the rank and
        holds 1 in its c_0 slot only.  With the identity ``dim_order`` it is inserted at that storage position;
        otherwise it is appended at the storage end and ``dim_order`` records where the user sees it."""
        self._check_built()
        params = _extrude_params(params, self.num_dimensions)
        identity = self._dim_order == list(range(self.num_dimensions))
        cores = list(self._coeff_cores)
        domain, n_nodes, order = list(self.domain), list(self.n_nodes), list(self._dim_order)
        for dim_idx, (lo, hi), n_new in params:
            pos = dim_idx if identity else len(cores)
            rank = 1 if pos == 0 or pos == len(cores) else cores[pos - 1].shape[2]
            core = np.zeros((rank, n_new, rank))
            core[np.arange(rank), 0, np.arange(rank)] = 1.0
            cores.insert(pos, core)
            domain.insert(pos, [lo, hi])
            n_nodes.insert(pos, n_new)
            if identity:
                order = list(range(len(cores)))
            else:
                order = [u if u < dim_idx else u + 1 for u in order] + [dim_idx]
        return self._derived(cores, domain=domain, n_nodes=n_nodes, dim_order=order)

    def _integrated_dims(self, dims) -> List[int]:
        if dims is None:
            dims = list(range(self.num_dimensions))
        elif isinstance(dims, (int, np.integer)):
            dims = [int(dims)]
        else:
            dims = sorted(set(int(v) for v in dims))
        if any(u < 0 or u >= self.num_dimensions for u in dims):
            raise ValueError(f"dims contains out-of-range index (num_dimensions={self.num_dimensions}, dims={dims})")
        return dims

    def integrate(self, dims=None, bounds=None):
        """Integrate over the user dimensions ``dims`` (all by default; reference :1505-1702): each integrated core
        goes to value space and is contracted with the Fejer-1 weights -- the sub-interval weights where ``bounds``
        gives ``(lo, hi)`` -- times ``(b - a) / 2``.  A float when no dimension is left, else a lower-dimensional
        TT with the matrices absorbed into the next kept core (the last kept core for trailing ones)."""
        from .barycentric import _integration_bounds, fejer1_weights, sub_interval_weights
        self._check_built()
        d = self.num_dimensions
        dims = self._integrated_dims(dims)
        per_dim = _integration_bounds(dims, bounds, self._user_frame_domain())
        matrices = {}
        for u, bd in zip(dims, per_dim):
            pos = self._dim_order.index(u)
            n = self.n_nodes[pos]
            a, b = self.domain[pos]
            if bd is None:
                quad = fejer1_weights(n)
            else:
                quad = sub_interval_weights(n, 2.0 * (bd[0] - a) / (b - a) - 1.0, 2.0 * (bd[1] - a) / (b - a) - 1.0)
            matrices[pos] = np.einsum("rjs,j->rs", _coeff_core_to_value_core(self._coeff_cores[pos]),
                                      quad * ((b - a) / 2.0))
        if len(dims) == d:
            total = matrices[0]
            for pos in range(1, d):
                total = total @ matrices[pos]
            return float(total.ravel()[0])
        cores, pending = [], None
        for pos in range(d):
            if pos in matrices:
                pending = matrices[pos] if pending is None else pending @ matrices[pos]
                continue
            core = self._coeff_cores[pos].copy()
            if pending is not None:
                core = np.einsum("lr,rjs->ljs", pending, core)
                pending = None
            cores.append(core)
        if pending is not None:
            cores[-1] = np.einsum("ljs,sr->ljr", cores[-1], pending)
        kept = [pos for pos in range(d) if pos not in matrices]
        return self._derived(cores, domain=[self.domain[pos] for pos in kept],
                             n_nodes=[self.n_nodes[pos] for pos in kept],
                             dim_order=_renumbered([self._dim_order[pos] for pos in kept], d, set(dims)))

    def inner_product(self, other: "ChebyshevTT") -> float:
        """Frobenius inner product of the two Chebyshev coefficient tensors, contracted core by core
        (reference :1438-1503)."""
        self._check_built()
        if not isinstance(other, ChebyshevTT):
            raise ValueError(f"other must be a ChebyshevTT, got {type(other).__name__}")
        other._check_built()
        same_box = np.allclose(np.asarray(self.domain, dtype=float), np.asarray(other.domain, dtype=float))
        for what, same, mine, theirs in (("domains", same_box, self.domain, other.domain),
                                         ("n_nodes", list(self.n_nodes) == list(other.n_nodes), self.n_nodes, other.n_nodes)):
            if not same:
                raise ValueError(f"inner_product requires matching {what}; got {mine} vs {theirs}")
        if list(self._dim_order) != list(other._dim_order):
            raise ValueError(f"inner_product requires matching _dim_order: {self._dim_order} vs {other._dim_order}. "
                             "Call other = other.reorder(self._dim_order) (or self = self.reorder(other._dim_order)) "
                             "to align before computing inner_product.")
        # gram[a, b] pairs the left ranks of the two trains over the dimensions walked so far: fold it into this
        # train's core, then sum that against the other's core over (its left rank, the coefficient index)
        gram = np.ones((1, 1))
        for mine, theirs in zip(self._coeff_cores, other._coeff_cores):
            folded = np.tensordot(gram, mine, axes=(0, 0))                        # (r_other, n, r_self')
            gram = np.tensordot(folded, theirs, axes=((0, 1), (0, 1)))            # (r_self', r_other')
        return float(gram[0, 0])

    def _box_rows(self, dims, bounds, points):
        """Validated arguments of :meth:`integrate_batch` -> (flags by user dimension, rows ``(N, d + m)``)."""
        from ._calculus import box_rows
        return box_rows(self.num_dimensions, self._user_frame_domain(), self._integrated_dims(dims), bounds, points)

    def integrate_batch(self, dims, bounds=None, points=None) -> np.ndarray:
        """Box integrals for a batch of rows (extension; the reference computes one with ``integrate(dims, bounds)``
        and then ``eval(point)``): ``out[r]`` is the integral over ``bounds[r]`` in the user dimensions ``dims`` at
        ``points[r]`` in the others.  ``bounds`` broadcasts to ``(N, m, 2)`` with the integrated dimensions in
        increasing order (``(m, 2)``, or ``(2,)`` for one dimension, serves every row; ``None`` is the whole domain);
        ``points`` is ``(N, d - m)``, the kept dimensions in increasing order as in :meth:`roots_batch`, and may be
        ``None`` only when every dimension is integrated.  One launch on the device (``pcx_tt_box_batch``): the TT
        chain with the antiderivatives of the Chebyshev polynomials as the basis in the integrated dimensions.
        Host arrays only."""
        self._check_built()
        flags, rows = self._box_rows(dims, bounds, points)
        t = self._dev()
        rows = _lib.f64(rows)
        out = np.empty(rows.shape[0])
        if rows.shape[0]:
            _lib.check(t.lib.pcx_tt_box_batch(t.handle, _lib.p_i32(flags), _lib.p_f64(rows), rows.shape[0],
                                              _lib.p_f64(out)), t.lib)
        return out

    def differentiate(self, derivative_order) -> "ChebyshevTT":
        """The partial derivative as a model of its own (extension): ``derivative_order`` gives an order >= 0 per user
        dimension, and each differentiated core goes through the Chebyshev coefficient-derivative recurrence along
        axis 1 (``c'_{j-1} = c'_{j+1} + 2 j c_j``, the constant halved) that many times, scaled by ``2 / (b - a)`` per
        order.  Host NumPy on cores of a few kilobytes, as :meth:`slice` and :meth:`integrate`.  Node counts, domain and
        ``dim_order`` are kept (the top coefficients of a differentiated core are zero); an order that reaches a
        dimension's node count gives the zero model.  ``function`` is ``None``.  The result evaluates, slices,
        integrates and goes through ``roots`` / ``minimize`` like any other model -- the zeros of a delta are
        ``tt.differentiate(spec).roots(...)`` -- and its ``eval_batch`` is a second route to
        ``eval_multi_batch(points, [spec], method="analytic")``."""
        from numpy.polynomial.chebyshev import chebder
        self._check_built()
        d = self.num_dimensions
        spec = list(derivative_order)
        if len(spec) != d:
            raise ValueError(f"derivative_order needs {d} orders, got {len(spec)}")
        for o in spec:
            if not isinstance(o, (int, np.integer)) or isinstance(o, bool) or o < 0:
                raise ValueError(f"Derivative order {o!r} not supported (use an integer >= 0)")
        cores = []
        for pos, core in enumerate(self._coeff_cores):
            p = int(spec[self._dim_order[pos]])
            new = np.array(core, dtype=float)
            if p:
                a, b = self.domain[pos]
                der = chebder(new, m=p, scl=2.0 / (b - a), axis=1)      # p >= n: one zero coefficient
                new = np.zeros_like(new)
                new[:, :der.shape[1], :] = der
            cores.append(new)
        return self._derived(cores)


    # ---------------------------------------------------------------- persistence
    def __getstate__(self) -> dict:
        state = self.__dict__.copy()
        state["function"] = None
        state.pop("_device_tt", None)
        state.pop("_device_index", None)
        state.pop("_fanout", None)
        state.pop("_fanout_devices", None)
        state["_pychebyshev_version"] = __version__
        return state

    def __setstate__(self, state: dict) -> None:
        saved = state.pop("_pychebyshev_version", None)
        if saved is not None and saved != __version__:
            warnings.warn(f"This object was saved with pychebyshev {saved}, but you are loading it "
                          f"with {__version__}. Evaluation results may differ if internal data "
                          f"layout changed.", UserWarning, stacklevel=2)
        self.__dict__.update(state)
        self.function = None
        for key, val in (("_cached_error_estimate", None), ("additional_data", None),
                         ("descriptor", ""), ("max_derivative_order", 2)):
            if not hasattr(self, key):
                setattr(self, key, val)
        if not hasattr(self, "_dim_order"):
            self._dim_order = list(range(self.num_dimensions))
        self._device_tt = None
        self._device_index = None

    def save(self, path) -> None:
        self._check_built()
        with open(path, "wb") as f:
            pickle.dump(self, f, protocol=pickle.HIGHEST_PROTOCOL)

    @classmethod
    def load(cls, path) -> "ChebyshevTT":
        with open(path, "rb") as f:
            obj = pickle.load(f)  # noqa: S301 - same trust model as the reference
        if not isinstance(obj, cls):
            raise TypeError(f"Expected a {cls.__name__} instance, got {type(obj).__name__}")
        return obj

    def __repr__(self) -> str:
        return (f"ChebyshevTT(dims={self.num_dimensions}, nodes={self.n_nodes}, "
                f"max_rank={self.max_rank}, built={self._built})")

    def __str__(self) -> str:
        """Multi-line summary in the reference's layout (:3235-3281)."""
        shown = 6
        ns, dom = list(self.n_nodes), list(self.domain)
        if self.num_dimensions > shown:
            nodes_txt = "[" + ", ".join(str(n) for n in ns[:shown]) + ", ...]"
            dom_txt = " x ".join(f"[{lo}, {hi}]" for lo, hi in dom[:shown]) + " x ..."
        else:
            nodes_txt = str(ns)
            dom_txt = " x ".join(f"[{lo}, {hi}]" for lo, hi in dom)
        out = [f"ChebyshevTT ({self.num_dimensions}D, {'built' if self._built else 'not built'})",
               f"  Nodes:       {nodes_txt}"]
        if self._built:
            full = int(np.prod(ns))
            stored = sum(c.size for c in self._coeff_cores)
            out += [f"  TT ranks:    {self._tt_ranks}",
                    f"  Compression: {full:,} -> {stored:,} elements ({full / stored:.1f}x)",
                    f"  Build:       {self._build_time:.3f}s ({self._total_build_evals:,} function evals)",
                    f"  Domain:      {dom_txt}",
                    f"  Error est:   {self.error_estimate():.2e}"]
        else:
            out.append(f"  Domain:      {dom_txt}")
        return "\n".join(out)
