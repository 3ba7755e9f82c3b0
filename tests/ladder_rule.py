"""NumPy restatement of the rule ``ladder_batch`` / ``fibre_batch`` compute (csrc/bary_ladder_kernels.h,
csrc/tt_ladder_kernels.h): the row's fibre along ``dim`` first, then its 1-D interpolant at the row's values.  No GPU;
tests/test_ladders_host.py holds it to the golden ladders, which shows that the RULE, not only the kernels, meets them.
"""
from __future__ import annotations

import numpy as np

from pychebyshev_amd.barycentric import (chebyshev_nodes, compute_barycentric_weights,
                                         compute_differentiation_matrix)


def bary_weights_1d(x, nodes, wts):
    """Normalised barycentric weights of one coordinate: one-hot at the first node within 1e-14"""
    diff = x - nodes
    exact = np.nonzero(np.abs(diff) < 1e-14)[0]
    if exact.size:
        out = np.zeros(nodes.size)
        out[exact[0]] = 1.0
        return out
    u = wts / diff
    return u / u.sum()


def interp_1d(x, nodes, wts, F):
    """ladder_interp_1d: F at the first node within 1e-14 of x, else sum u F / sum u"""
    if np.isnan(x):
        return np.nan
    diff = x - nodes
    exact = np.nonzero(np.abs(diff) < 1e-14)[0]
    if exact.size:
        return F[exact[0]]
    u = wts / diff
    with np.errstate(divide="ignore", invalid="ignore"):      # far outside a long dimension the weights cancel to 0
        return float(np.dot(u, F) / u.sum())


def dense_setup(tensor, domain, spec=None):
    """(derived tensor, nodes, weights) of a dense model: the D passes by dimension, descending, as the handle makes them"""
    cur = np.asarray(tensor, dtype=float)
    d = cur.ndim
    nodes = [chebyshev_nodes(domain[k][0], domain[k][1], cur.shape[k]) for k in range(d)]
    wts = [compute_barycentric_weights(x) for x in nodes]
    if spec is not None:
        for k in range(d - 1, -1, -1):
            if spec[k]:
                D = compute_differentiation_matrix(nodes[k], wts[k])
                for _ in range(int(spec[k])):
                    cur = np.moveaxis(np.tensordot(D, cur, axes=([1], [k])), 0, k)
    return cur, nodes, wts


def dense_fibres(cur, nodes, wts, dim, fixed):
    """(N, n_dim): F[r, j] = sum over the other dimensions of T . (their weights at the row's coordinates)"""
    d = cur.ndim
    others = [k for k in range(d) if k != dim]
    out = np.empty((fixed.shape[0], cur.shape[dim]))
    moved = np.moveaxis(cur, dim, 0)
    for r in range(fixed.shape[0]):
        fib = moved
        for c in reversed(range(len(others))):
            k = others[c]
            fib = np.tensordot(fib, bary_weights_1d(fixed[r, c], nodes[k], wts[k]), axes=([fib.ndim - 1], [0]))
        out[r] = fib
    return out


def dense_ladder(tensor, domain, dim, fixed, xs, spec=None):
    cur, nodes, wts = dense_setup(tensor, domain, spec)
    F = dense_fibres(cur, nodes, wts, dim, np.asarray(fixed, dtype=float))
    xs = np.asarray(xs, dtype=float)
    out = np.empty((F.shape[0], xs.shape[-1]))
    for r in range(F.shape[0]):
        xr = xs if xs.ndim == 1 else xs[r]
        out[r] = [interp_1d(x, nodes[dim], wts[dim], F[r]) for x in xr]
    return out


def cheb_basis(s, n):
    T = np.empty(n)
    T[0] = 1.0
    if n > 1:
        T[1] = s
    for j in range(2, n):
        T[j] = 2.0 * s * T[j - 1] - T[j - 2]
    return T


def tt_ladder(cores, domain, order, dim, fixed, xs):
    """cores and domain by storage position, ``order[k]`` = the user dimension at storage position k; dim, fixed and xs
    in the user's frame: left chain, right chain, the n coefficients at dim's position, then the series per value"""
    d = len(cores)
    p = list(order).index(dim)
    fixed = np.asarray(fixed, dtype=float)
    xs = np.asarray(xs, dtype=float)
    out = np.empty((fixed.shape[0], xs.shape[-1]))

    def mat(k, x):
        a, b = domain[k]
        s = (x - a) * (2.0 / (b - a)) - 1.0
        return np.tensordot(cores[k], cheb_basis(s, cores[k].shape[1]), axes=([1], [0]))

    for r in range(fixed.shape[0]):
        coord = {u: fixed[r, u if u < dim else u - 1] for u in range(d) if u != dim}
        L = np.ones(1)
        for k in range(p):
            L = L @ mat(k, coord[order[k]])
        R = np.ones(1)
        for k in range(d - 1, p, -1):
            R = mat(k, coord[order[k]]) @ R
        c = np.einsum("a,aib,b->i", L, cores[p], R)
        a, b = domain[p]
        xr = xs if xs.ndim == 1 else xs[r]
        out[r] = [float(np.dot(c, cheb_basis((x - a) * (2.0 / (b - a)) - 1.0, c.size))) for x in xr]
    return out
