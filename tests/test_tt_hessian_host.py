"""ChebyshevTT.hessian_batch on the host: the blocked carried association of csrc/tt_hess_kernels.h restated in float64
(tests/tt_hess_chain.py) against the long-double chain of tests/tt_chain.py, and the entry points the library and the
class gained.  Host NumPy only: no GPU.

The off-diagonal columns are the (1, 1) specs, family "order1".  Over the 292 models of the sweep, the tail model and
the edge models the float64 restatement of the carried association measures, worst |y - ref| / (eps A_row) of those
columns, sweep 0.4328 and edge 0.3694 -- equal to the last bit to the left-to-right ``Chain.deriv`` of the same specs,
measured beside it -- so K_of(worst) is 8 and 8 where tt_chain.K["sweep" / "edge"]["order1"] is 8 and 32: the
off-diagonals take K["order1"], the diagonal K["order2"], the value and the gradient their own K, and the Hessian
kernels need no constant of their own.  Value, gradient and diagonal are tests/tt_grad_chain.py's, bit for bit."""
import numpy as np
import pytest

import tt_chain as C
import tt_grad_chain as GC
import tt_hess_chain as HC
from pychebyshev_amd import ChebyshevTT, _lib

ALL = C.sweep_models() + C.edge_models() + (C.tail_model(),)


def test_the_columns_are_the_value_the_gradient_and_every_pair():
    assert HC.columns(2) == [(0, [0, 0], "value"), (1, [1, 0], "order1"), (2, [0, 1], "order1"),
                             (3, [2, 0], "order2"), (4, [1, 1], "order1"), (5, [1, 1], "order1"), (6, [0, 2], "order2")]
    cols = HC.columns(5)
    assert [c for c, _, _ in cols] == list(range(1 + 5 + 25))
    assert cols[1 + 5 + 1 * 5 + 3][1] == [0, 1, 0, 1, 0] and cols[1 + 5 + 3 * 5 + 1][1] == [0, 1, 0, 1, 0]
    assert cols[1 + 5 + 2 * 5 + 2][1:] == ([0, 0, 2, 0, 0], "order2")


@pytest.mark.parametrize("number", [0, 37, 160, 287, 288, 290, 291])
def test_the_carried_association_is_the_chain_in_long_double(number):
    """Every column within 2^-60 of the amplitude of the plain chain with that column's spec (permuted dim_order, edge
    and tail models among them), at block 1 and at d - 1; in float64 block = 1, 2 and d - 1 give the same bits."""
    b = C.build(ALL[number])
    d = len(b.cores)
    top = max(1, d - 1)
    chain = C.Chain(b.cores, b.domain, b.order, b.pts, C.LD)
    ref = HC.reference(b)
    for block in sorted({1, top}):
        got = HC.forward_backward(chain, block)
        assert got.shape == (b.model.rows, 1 + d + d * d)
        for col, family, val, amp in ref:
            assert np.all(np.abs(got[:, col] - val) <= 2.0 ** -60 * amp), (b.model.name, block, col, family)
    f64 = C.Chain(b.cores, b.domain, b.order, b.pts, np.float64)
    one = HC.forward_backward(f64, 1)
    assert one.dtype == np.float64
    for block in sorted({min(2, top), top}):
        assert np.array_equal(HC.forward_backward(f64, block), one), (b.model.name, block)
    H = one[:, 1 + d:].reshape(-1, d, d)
    assert np.array_equal(H, H.transpose(0, 2, 1))


def test_the_restatement_of_the_pairs_stays_within_the_left_to_right_figures():
    """The float64 restatement's (1, 1) columns against the long-double chain on all 292 models: the worst ratio per
    list does not exceed the left-to-right ``Chain.deriv`` figure of the same specs computed beside it, and its K_of is
    within tt_chain.K[list]["order1"].  Measured: sweep 0.4328, edge 0.3694, the two associations equal to the last
    bit (in long double every pair of every model is within 2^-60 A_row of the chain; the test above asserts that on
    seven models).  The value, gradient and diagonal columns equal tt_grad_chain.forward_backward exactly."""
    assert len(ALL) == 292
    worst = {"sweep": 0.0, "edge": 0.0}
    left_to_right = dict(worst)
    for m in ALL:
        b = C.build(m)
        d = len(b.cores)
        group = C.group_of(m)
        f64 = C.Chain(b.cores, b.domain, b.order, b.pts, np.float64)
        ld = C.Chain(b.cores, b.domain, b.order, b.pts, C.LD)
        got = HC.forward_backward(f64, max(1, d - 1))
        grad = GC.forward_backward(f64)
        assert np.array_equal(got[:, :1 + d], grad[:, :1 + d]), m.name
        assert np.array_equal(got[:, 1 + d:].reshape(-1, d, d)[:, np.arange(d), np.arange(d)], grad[:, 1 + d:]), m.name
        for u in range(d):
            for v in range(u + 1, d):
                spec = [int(w in (u, v)) for w in range(d)]
                val, amp = ld.deriv(spec)
                col = 1 + d + u * d + v
                worst[group] = max(worst[group], float(np.max(C.ratios(got[:, col], val, amp))))
                left_to_right[group] = max(left_to_right[group], float(np.max(C.ratios(f64.deriv(spec)[0], val, amp))))
    print("carried", {g: round(r, 4) for g, r in worst.items()}, "left to right", {g: round(r, 4) for g, r in left_to_right.items()})
    for group, r in worst.items():
        assert r > 0.0
        assert r <= left_to_right[group], (group, r, left_to_right[group])
        assert C.K_of(r) <= C.K[group]["order1"], (group, r)


def test_exact_zeros_of_short_dimensions():
    """n = 1: the Hessian's row and column exactly zero; n = 2: the diagonal entry -- in the restatement as in the
    chain (amplitude zero) -- and nothing else is."""
    for short in (1, 2):
        m = next(m for m in C.sweep_models() if m.mode == "mixed" and short in m.n)
        b = C.build(m)
        d = len(m.n)
        got = HC.forward_backward(C.Chain(b.cores, b.domain, b.order, b.pts, np.float64), 2)
        H = got[:, 1 + d:].reshape(-1, d, d)
        user_n = [m.n[C.storage_position(b, u)] for u in range(d)]
        for u in range(d):
            assert np.all(H[:, u, u] == 0.0) == (user_n[u] <= 2), (m.name, u)
            for v in range(d):
                if u != v:
                    assert np.all(H[:, u, v] == 0.0) == (1 in (user_n[u], user_n[v])), (m.name, u, v)


def test_the_library_exports_the_entry_points():
    lib = _lib.load()
    assert lib.pcx_tt_hess_batch is not None and lib.pcx_tt_hess_batch_dev is not None and lib.pcx_tt_hess_info is not None
    assert len(_lib.SIGNATURES["pcx_tt_hess_batch"][1]) == 5
    assert len(_lib.SIGNATURES["pcx_tt_hess_batch_dev"][1]) == 6
    assert len(_lib.SIGNATURES["pcx_tt_hess_info"][1]) == 2
    assert callable(ChebyshevTT.hessian_batch) and callable(ChebyshevTT.hessian)
