"""ChebyshevTT.gradient_batch on the host: the forward-backward association of csrc/tt_grad_kernels.h restated in float64
(tests/tt_grad_chain.py) against the long-double chain of tests/tt_chain.py, and the entry points the library and the
class gained.  Host NumPy only: no GPU.

The restatement keeps every R_k of a right sweep and takes g_k = sum_b (L_k M1_k)[b] R_{k+1}[b] on the way back; the
long-double reference is the plain left-to-right chain, ``Chain.value()`` and ``Chain.deriv`` of each single-dimension
spec.  Worst |y - ref| / (eps A_row) over all 292 models comes out where the left-to-right restatement's does
(tt_chain.RESTATEMENT_WORST: sweep 0.270 / 0.405 / 0.467, edge 1.842 / 1.812 / 3.244 for value / order 1 / order 2), so
the K of tt_chain.K holds for the gradient kernels as it stands: no constant of their own."""
import numpy as np
import pytest

import tt_chain as C
import tt_grad_chain as GC
from pychebyshev_amd import ChebyshevTT, _lib

FAMILIES = ("value", "order1", "order2")


def test_the_columns_are_the_single_dimension_specs():
    assert GC.columns(3) == [(0, [0, 0, 0], "value"), (1, [1, 0, 0], "order1"), (2, [0, 1, 0], "order1"),
                             (3, [0, 0, 1], "order1"), (4, [2, 0, 0], "order2"), (5, [0, 2, 0], "order2"),
                             (6, [0, 0, 2], "order2")]
    assert GC.columns(2, second=False) == [(0, [0, 0], "value"), (1, [1, 0], "order1"), (2, [0, 1], "order1")]


@pytest.mark.parametrize("number", [0, 37, 160, 287, 288, 290, 291])
def test_forward_backward_is_the_chain_in_long_double(number):
    """Associating the product around each core changes nothing beyond long-double rounding: every column within
    2^-60 of the amplitude of the plain chain with that column's spec (permuted dim_order, edge and tail models among
    them), and the first 1 + d columns do not depend on ``second``."""
    b = C.build((C.sweep_models() + C.edge_models() + (C.tail_model(),))[number])
    chain = C.Chain(b.cores, b.domain, b.order, b.pts, C.LD)
    got = GC.forward_backward(chain)
    d = len(b.cores)
    assert got.shape == (b.model.rows, 1 + 2 * d)
    for col, family, val, amp in GC.reference(b):
        assert np.all(np.abs(got[:, col] - val) <= 2.0 ** -60 * amp), (b.model.name, col, family)
    assert np.array_equal(GC.forward_backward(chain, second=False), got[:, :1 + d])


def test_the_restatement_stays_within_the_left_to_right_figures():
    """The float64 forward-backward restatement against the long-double chain on every model of the sweep, the tail
    model and the edge models: the worst ratio per list and family does not exceed the left-to-right restatement's,
    measured here unrounded on the same models and specs (tt_chain.deriv_specs, as tt_chain.restatement_ratios takes
    them).  tt_chain.RESTATEMENT_WORST records those left-to-right figures to three decimals (0.2703 as 0.270), and
    they are held to it as tests/test_tt_chain_host.py holds them; the two associations come out equal to the last
    bit here (sweep 0.27035 / 0.40452 / 0.46678, edge 1.84208 / 1.81163 / 3.24363)."""
    groups = ("sweep", "edge")                      # the lists measured here; C.K also holds the MFMA forms' lists
    worst = {group: dict.fromkeys(FAMILIES, 0.0) for group in groups}
    left_to_right = {group: dict.fromkeys(FAMILIES, 0.0) for group in groups}
    for m in C.sweep_models() + C.edge_models() + (C.tail_model(),):
        b = C.build(m)
        group = C.group_of(m)
        chain = C.Chain(b.cores, b.domain, b.order, b.pts, np.float64)
        f64 = GC.forward_backward(chain)
        assert f64.dtype == np.float64
        for family, r in GC.worst_ratios(f64, GC.reference(b)).items():
            worst[group][family] = max(worst[group][family], r)
        ld = C.Chain(b.cores, b.domain, b.order, b.pts, C.LD)
        for spec in C.deriv_specs(m):
            val, amp = ld.deriv(spec)
            family = C.family_of(spec)
            left_to_right[group][family] = max(left_to_right[group][family], float(np.max(C.ratios(chain.deriv(spec)[0], val, amp))))
    for group, fam in worst.items():
        print(group, {f: round(r, 5) for f, r in fam.items()}, "left to right", {f: round(r, 5) for f, r in left_to_right[group].items()})
    for group, fam in worst.items():
        for family, r in fam.items():
            assert r <= left_to_right[group][family], (group, family, r, left_to_right[group][family])
            assert left_to_right[group][family] == pytest.approx(C.RESTATEMENT_WORST[group][family], rel=5e-3), (group, family)


def test_zero_columns_of_short_dimensions():
    """n = 1: gradient and second derivative exactly zero, n = 2: the second derivative -- in the restatement as in
    the chain (amplitude zero)."""
    for short in (1, 2):
        m = next(m for m in C.sweep_models() if m.mode == "mixed" and short in m.n)
        b = C.build(m)
        d = len(m.n)
        got = GC.forward_backward(C.Chain(b.cores, b.domain, b.order, b.pts, np.float64))
        for k, n in enumerate(m.n):
            u = k if b.order is None else b.order[k]
            assert np.all(got[:, 1 + u] == 0.0) == (n == 1), (m.name, k)
            assert np.all(got[:, 1 + d + u] == 0.0) == (n <= 2), (m.name, k)


def test_the_library_exports_the_entry_points():
    lib = _lib.load()
    assert lib.pcx_tt_grad_batch is not None and lib.pcx_tt_grad_batch_dev is not None
    assert len(_lib.SIGNATURES["pcx_tt_grad_batch"][1]) == 5
    assert len(_lib.SIGNATURES["pcx_tt_grad_batch_dev"][1]) == 6
    assert callable(ChebyshevTT.gradient_batch) and callable(ChebyshevTT.gradient)
