"""The forward-backward association of ``ChebyshevTT.gradient_batch`` (csrc/tt_grad_kernels.h) restated with the
elementwise steps of tests/tt_chain.py: a right sweep that keeps every ``R_k``, then a left sweep that takes, at storage
position k,

    g_k = sum_b (L_k M1_k)[b] R_{k+1}[b],    h_k = sum_b (L_k M2_k)[b] R_{k+1}[b],    L_{k+1} = L_k M_k

with ``M_k``, ``M1_k``, ``M2_k`` the core folded with ``T_j``, ``sc T'_j`` and ``sc^2 T''_j`` (``Chain.fold(k, p)``).  Every
sum is ``tt_chain._step``: the rank index ascending, no matrix product, no FMA -- in float64 the same bits on every
machine.  In exact arithmetic the columns are ``Chain.value()`` and ``Chain.deriv`` of the single-dimension specs; the
host test holds the float64 restatement to those in long double, the GPU test holds the kernels to them.  Plain NumPy."""
import numpy as np

import tt_chain as C


def columns(d, second=True):
    """[(column, spec, family)] of the N x C result: the value, then order 1 and (``second``) order 2 per USER dimension."""
    out = [(0, [0] * d, "value")]
    for o, family in ((1, "order1"), (2, "order2"))[:2 if second else 1]:
        for u in range(d):
            out.append((1 + (o - 1) * d + u, [o if v == u else 0 for v in range(d)], family))
    return out


def forward_backward(chain, second=True):
    """(N, C) in ``chain``'s dtype, C = 1 + d or 1 + 2 d: value, gradient and diagonal in the USER's dimension order."""
    d, N = chain.d, chain.pts.shape[0]
    one = np.ones((N, 1), dtype=chain.dt)
    R = [None] * d + [one]
    for k in range(d - 1, 0, -1):
        R[k] = C._step(R[k + 1], chain.fold(k, 0)[0].transpose(0, 2, 1))            # R_k[a] = sum_b M[a][b] R_{k+1}[b]
    out = np.zeros((N, 1 + (2 if second else 1) * d), dtype=chain.dt)
    L = one
    for k in range(d):
        u = chain.order[k]
        for o in (1, 2)[:2 if second else 1]:
            out[:, 1 + (o - 1) * d + u] = C._step(C._step(L, chain.fold(k, o)[0]), R[k + 1][:, :, None])[:, 0]
        L = C._step(L, chain.fold(k, 0)[0])
    out[:, 0] = L[:, 0]
    return out


def reference(built, second=True):
    """[(column, family, values, amplitudes)] in long double: ``Chain.value()`` and ``Chain.deriv`` of every column's spec."""
    ld = C.Chain(built.cores, built.domain, built.order, built.pts, C.LD)
    out = []
    for col, spec, family in columns(len(built.cores), second):
        val, amp = ld.value() if family == "value" else ld.deriv(spec)
        out.append((col, family, val, amp))
    return out


def worst_ratios(got, ref):
    """{family: worst |got - ref| / (eps A_row)} of an (N, C) result against ``reference``'s columns."""
    worst = {}
    for col, family, val, amp in ref:
        worst[family] = max(worst.get(family, 0.0), float(np.max(C.ratios(got[:, col], val, amp))))
    return worst
