"""The blocked carried association of ``ChebyshevTT.hessian_batch`` (csrc/tt_hess_kernels.h) restated with the
elementwise steps of tests/tt_chain.py: the right sweep that keeps every ``R_k`` and a left sweep in passes of ``block``
sources.  Pass 0 is the gradient's left sweep (tests/tt_grad_chain.py); at a source position i the vector
``D_i = L_i M1_i`` is kept, and at every later position k

    H_ik = sum_b (D_i M1_k)[b] R_{k+1}[b],    D_i <- D_i M_k

A pass p >= 1 folds ``L`` alone up to its first source p * block.  Every sum is ``tt_chain._step``, so in float64 the
result is the same bits on every machine and for every block.  In exact arithmetic the columns are ``Chain.value()``
and ``Chain.deriv`` of the column's spec: (1, 1) in dimensions u and v off the diagonal, 2 in u on it.  Plain NumPy."""
import numpy as np

import tt_chain as C


def columns(d):
    """[(column, spec, family)] of the N x C result, C = 1 + d + d^2: the value, the gradient, then the Hessian
    row-major in the USER's (u, v)."""
    out = [(0, [0] * d, "value")]
    for u in range(d):
        out.append((1 + u, [int(v == u) for v in range(d)], "order1"))
    for u in range(d):
        for v in range(d):
            spec = [2 * int(w == u) if u == v else int(w in (u, v)) for w in range(d)]
            out.append((1 + d + u * d + v, spec, C.family_of(spec)))
    return out


def forward_backward(chain, block):
    """(N, 1 + d + d^2) in ``chain``'s dtype at block size ``block``, 1 <= block <= max(1, d - 1)."""
    d, N = chain.d, chain.pts.shape[0]
    assert 1 <= block <= max(1, d - 1)
    one = np.ones((N, 1), dtype=chain.dt)
    R = [None] * d + [one]
    for k in range(d - 1, 0, -1):
        R[k] = C._step(R[k + 1], chain.fold(k, 0)[0].transpose(0, 2, 1))
    out = np.zeros((N, 1 + d + d * d), dtype=chain.dt)
    H = out[:, 1 + d:].reshape(N, d, d)
    assert np.shares_memory(H, out)
    first = 0
    while first == 0 or first < d - 1:
        last = min(first + block, d - 1)
        L = one
        D = {}
        for k in range(d):
            v = chain.order[k]
            if k >= first:
                if first == 0:
                    out[:, 1 + v] = C._step(C._step(L, chain.fold(k, 1)[0]), R[k + 1][:, :, None])[:, 0]
                    H[:, v, v] = C._step(C._step(L, chain.fold(k, 2)[0]), R[k + 1][:, :, None])[:, 0]
                for i in sorted(D):
                    u = chain.order[i]
                    H[:, u, v] = H[:, v, u] = C._step(C._step(D[i], chain.fold(k, 1)[0]), R[k + 1][:, :, None])[:, 0]
                    D[i] = C._step(D[i], chain.fold(k, 0)[0])
                if k < last:
                    D[k] = C._step(L, chain.fold(k, 1)[0])
            L = C._step(L, chain.fold(k, 0)[0])
        if first == 0:
            out[:, 0] = L[:, 0]
        first += block
    return out


def reference(built):
    """[(column, family, values, amplitudes)] in long double: ``Chain.value()`` and ``Chain.deriv`` of every column's
    spec (a symmetric pair shares one computation)."""
    ld = C.Chain(built.cores, built.domain, built.order, built.pts, C.LD)
    out, seen = [], {}
    for col, spec, family in columns(len(built.cores)):
        key = tuple(spec)
        if key not in seen:
            seen[key] = ld.value() if family == "value" else ld.deriv(spec)
        out.append((col, family) + tuple(seen[key]))
    return out


def worst_ratios(got, ref):
    """{"value", "order1" (the gradient), "order2" (the diagonal), "cross" (the off-diagonals)}: worst
    |got - ref| / (eps A_row) of an (N, C) result against ``reference``'s columns.  The off-diagonals' family is
    "order1"; they are reported apart from the gradient."""
    d = int(round((-1 + np.sqrt(1 + 4 * (len(ref) - 1))) / 2))
    worst = {}
    for col, family, val, amp in ref:
        name = "cross" if col >= 1 + d and family == "order1" else family
        worst[name] = max(worst.get(name, 0.0), float(np.max(C.ratios(got[:, col], val, amp))))
    return worst
