"""NumPy restatement of ``ChebyshevTT.fit_samples`` (helper, no tests): ALS regression of a tensor train on scattered
samples, step by step as the method's docstring states it, in float64 or -- ``dtype=np.longdouble`` -- in the extended
format, where nothing goes through LAPACK (NumPy has no longdouble ``qr`` / ``cholesky``): the Householder QR and the
Cholesky solve are written out here and used for both formats.  It is the reference of tests/test_tt_fit_host.py,
tests/test_gpu_tt_fit_steps.py and tests/test_gpu_tt_fit.py; the code under test is never its own reference.

Points are in STORAGE order (column k belongs to core k) everywhere in this file."""
from __future__ import annotations

import numpy as np
from numpy.polynomial.chebyshev import chebpts1


def basis(x, lo, hi, n, dtype=np.float64):
    """``T_j(t)``, ``j < n``, at ``t = 2 (x - lo) / (hi - lo) - 1`` by the recurrence: ``(N, n)``."""
    x = np.asarray(x, dtype=dtype)
    lo, hi = dtype(lo), dtype(hi)
    t = dtype(2) * (x - lo) / (hi - lo) - dtype(1)
    T = np.empty((x.shape[0], n), dtype=dtype)
    T[:, 0] = 1
    if n > 1:
        T[:, 1] = t
    for j in range(2, n):
        T[:, j] = dtype(2) * t * T[:, j - 1] - T[:, j - 2]
    return T


def bases(points, domain, n_nodes, dtype=np.float64, absolute=False):
    Ts = [basis(np.asarray(points)[:, k], domain[k][0], domain[k][1], n_nodes[k], dtype) for k in range(len(n_nodes))]
    return [np.abs(T) for T in Ts] if absolute else Ts


def interfaces(cores, Ts, k):
    """``L`` (N, r_k) and ``R`` (N, r_{k+1}): the partial products of the chain left and right of position ``k``."""
    N, dtype = Ts[0].shape[0], Ts[0].dtype
    L = np.ones((N, 1), dtype=dtype)
    for m in range(k):
        L = np.einsum("ia,ij,ajb->ib", L, Ts[m], cores[m])
    R = np.ones((N, 1), dtype=dtype)
    for m in range(len(cores) - 1, k, -1):
        R = np.einsum("ajb,ij,ib->ia", cores[m], Ts[m], R)
    return L, R


def design(cores, Ts, k):
    """The design matrix of position ``k``: row i = ``L_i (x) T(t_k) (x) R_i`` in C order (a, j, b)."""
    L, R = interfaces(cores, Ts, k)
    return np.einsum("ia,ij,ib->iajb", L, Ts[k], R).reshape(Ts[0].shape[0], -1)


def normal(cores, points, values, domain, k, dtype=np.float64, absolute=False):
    """``G = A^T A`` and ``b = A^T y`` of position ``k``; ``absolute``: every core entry, basis value and y replaced by
    its absolute value (the magnitude the rounding errors of the sums scale with)."""
    cs = [np.asarray(c, dtype=dtype) for c in cores]
    y = np.asarray(values, dtype=dtype)
    if absolute:
        cs, y = [np.abs(c) for c in cs], np.abs(y)
    Ts = bases(points, domain, [c.shape[1] for c in cs], dtype, absolute)
    A = design(cs, Ts, k)
    return A.T @ A, A.T @ y


def evaluate(cores, points, domain, dtype=np.float64):
    cs = [np.asarray(c, dtype=dtype) for c in cores]
    Ts = bases(points, domain, [c.shape[1] for c in cs], dtype)
    L, _ = interfaces(cs + [np.ones((1, 1, 1), dtype=dtype)], Ts + [np.ones((Ts[0].shape[0], 1), dtype=dtype)], len(cs))
    return L[:, 0]


def grid_points(domain, n_nodes):
    """The Chebyshev grid of ``to_dense()``, C order, as rows."""
    grids = [np.sort(0.5 * (a + b) + 0.5 * (b - a) * chebpts1(n)) for (a, b), n in zip(domain, n_nodes)]
    return np.column_stack([m.ravel() for m in np.meshgrid(*grids, indexing="ij")])


def householder_qr(A):
    """Reduced QR of ``A`` (m x c) in A's own dtype: Q (m x p), R (p x c), p = min(m, c)."""
    A = np.array(A)
    dtype = A.dtype.type
    m, c = A.shape
    p = min(m, c)
    R = A.copy()
    vs = []
    for j in range(p):
        x = R[j:, j].copy()
        nx = np.sqrt(x @ x)
        v = x
        if nx > 0:
            v[0] += nx if x[0] >= 0 else -nx
            v = v / np.sqrt(v @ v)
            R[j:, j:] -= dtype(2) * np.outer(v, v @ R[j:, j:])
        else:
            v = np.zeros_like(x)
        vs.append(v)
    Q = np.eye(m, p, dtype=A.dtype)
    for j in range(p - 1, -1, -1):
        v = vs[j]
        Q[j:, :] -= dtype(2) * np.outer(v, v @ Q[j:, :])
    return Q, np.triu(R[:p, :])


def move_centre(cores, k, to):
    rl, n, rr = cores[k].shape
    if to == k + 1:
        Q, R = householder_qr(cores[k].reshape(rl * n, rr))
        cores[k] = Q.reshape(rl, n, Q.shape[1])
        nxt = cores[k + 1]
        cores[k + 1] = (R @ nxt.reshape(rr, -1)).reshape(R.shape[0], nxt.shape[1], nxt.shape[2])
    else:
        assert to == k - 1
        Q, R = householder_qr(cores[k].reshape(rl, n * rr).T)
        cores[k] = np.ascontiguousarray(Q.T).reshape(Q.shape[1], n, rr)
        prv = cores[k - 1]
        cores[k - 1] = (prv.reshape(-1, rl) @ R.T).reshape(prv.shape[0], prv.shape[1], R.shape[0])


def cholesky_solve(G, b):
    """``G c = b`` by Cholesky in G's own dtype; ``ValueError`` when G is not positive definite."""
    P = G.shape[0]
    Lc = np.zeros_like(G)
    for j in range(P):
        s = G[j, j] - Lc[j, :j] @ Lc[j, :j]
        if not s > 0:
            raise ValueError("not positive definite")
        Lc[j, j] = np.sqrt(s)
        Lc[j + 1:, j] = (G[j + 1:, j] - Lc[j + 1:, :j] @ Lc[j, :j]) / Lc[j, j]
    z = np.zeros_like(b)
    for j in range(P):
        z[j] = (b[j] - Lc[j, :j] @ z[:j]) / Lc[j, j]
    c = np.zeros_like(b)
    for j in range(P - 1, -1, -1):
        c[j] = (z[j] - Lc[j + 1:, j] @ c[j + 1:]) / Lc[j, j]
    return c


def residual(cores, Ts, y):
    L, _ = interfaces(list(cores) + [np.ones((1, 1, 1), dtype=y.dtype)], Ts + [np.ones((y.shape[0], 1), dtype=y.dtype)], len(cores))
    return float(np.sqrt(np.sum((L[:, 0] - y) ** 2)) / np.sqrt(np.sum(y ** 2)))


def fit(cores, points, values, domain, max_iter=20, tolerance=1e-10, ridge=1e-12, dtype=np.float64, snapshots=None):
    """``fit_samples`` restated: ``(cores, residual history)``.  ``snapshots``: a list that receives a copy of the cores
    after every outer iteration."""
    cores = [np.array(c, dtype=dtype) for c in cores]
    y = np.asarray(values, dtype=dtype)
    d = len(cores)
    Ts = bases(points, domain, [c.shape[1] for c in cores], dtype)
    history = []
    if max_iter <= 0:
        return cores, history
    for k in range(d - 1, 0, -1):
        move_centre(cores, k, k - 1)
    order = list(range(d)) + list(range(d - 2, 0, -1))
    for it in range(max_iter):
        for i, k in enumerate(order):
            A = design(cores, Ts, k)
            G, b = A.T @ A, A.T @ y
            P = b.size
            lam = dtype(ridge) * np.trace(G) / dtype(P)
            c = cholesky_solve(G + lam * np.eye(P, dtype=dtype), b)
            cores[k] = c.reshape(cores[k].shape)
            nxt = order[(i + 1) % len(order)]
            if nxt != k:
                move_centre(cores, k, nxt)
        res = residual(cores, Ts, y)
        history.append(res)
        if snapshots is not None:
            snapshots.append([c.copy() for c in cores])
        if res == 0.0 or (it > 0 and abs(history[-2] - res) <= tolerance * history[-2]):
            break
    return cores, history


def start_cores(n_nodes, rank, seed):
    """``from_samples``' documented start: bonds min(rank, prod(n[:k]), prod(n[k:])), standard normals core by core."""
    d = len(n_nodes)
    bonds = [1] + [min(rank, int(np.prod(n_nodes[:k])), int(np.prod(n_nodes[k:]))) for k in range(1, d)] + [1]
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((bonds[k], n_nodes[k], bonds[k + 1])) for k in range(d)]


# ---- the prototype cases -------------------------------------------------------------------------------------------
def _case_a(x):
    return np.sin(x[:, 0]) + np.cos(x[:, 1]) * x[:, 2]


def _case_b(x):          # rank 4 in three dimensions
    return np.exp(-x[:, 0] * x[:, 1]) * np.sin(x[:, 2] + x[:, 0]) + x[:, 1] * np.cos(2.0 * x[:, 2])


def _case_c(x):          # five dimensions, fitted at rank 3
    return np.sin(x[:, 0] + x[:, 1] + x[:, 2] + x[:, 3] + x[:, 4]) + x[:, 0] * x[:, 4]


CASES = {
    "sincos3d": dict(f=_case_a, domain=[(-1.0, 1.0), (0.0, 2.0), (-1.0, 0.5)], n=[6, 7, 5], rank=2, N=600),
    "rank4_3d": dict(f=_case_b, domain=[(-1.0, 1.0), (0.0, 1.0), (-0.5, 1.5)], n=[8, 7, 9], rank=4, N=4000),
    "rank3_5d": dict(f=_case_c, domain=[(-1.0, 1.0), (0.0, 1.0), (-1.0, 0.0), (0.0, 0.5), (-0.5, 0.5)], n=[5, 4, 5, 4, 5], rank=3, N=6000),
}


def samples(case, N=None, seed=100):
    """``N`` uniform points of the case's domain (storage order) and the function there."""
    c = CASES[case]
    rng = np.random.default_rng(seed)
    lo = np.array([a for a, _ in c["domain"]])
    hi = np.array([b for _, b in c["domain"]])
    pts = lo + (hi - lo) * rng.random((N or c["N"], len(lo)))
    return pts, c["f"](pts)
