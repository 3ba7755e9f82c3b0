"""Every rank and node-count body of the lane-per-row tensor-train kernels -- k_tt_eval_lpp, k_tt_fd_lpp, k_tt_box_lpp,
k_tt_deriv_lpp and k_tt_ladder_lpp (csrc/tt_lpp_kernels.h, tt_fd_kernels.h, tt_box_kernels.h, tt_deriv_kernels.h,
tt_ladder_kernels.h) -- against the long-double chain of tests/tt_chain.py.

The sweep is tt_chain.sweep_models(): 288 seeded models whose dimensions reach all 16 x (8 + 12 + 16) x 2 = 1,152
(rank cap, uniform or mixed node counts, left rank, node count) bodies of each kernel and every node-count body of the
ladder kernel's left, right and core steps (tests/test_tt_chain_host.py asserts that from the list alone).  One case
per model: the model is built, the five kernels run on it, and its handle is dropped.  Then the wave-per-row forms on
three models that make their lane loops take one, two and three trips, and the batch tails of the lane kernels.

Bounds against the long-double chain, per call:
  normwise    max |got - ref| <= 1e-12 max |ref|, the project's bar
  row by row  |got - ref| <= K eps A_row, A_row the row's amplitude (tt_chain.py) and K = tt_chain.K: 16 times the
              worst ratio of the float64 restatement of the chain, per family, at most 64
The row bound is the real check: a row that cancels is held to its own terms, not to the largest row of the batch.
A pointwise relative bound cannot be 1e-12 here (the restatement alone reaches 3e-12 on |ref| >= 1e-3 max |ref|).

Worst |got - ref| / (eps A_row) measured on MI355X / the restatement's figure / K:
    sweep  eval 0.21 / 0.27 / 8, deriv order 0: 0.21 / 0.27 / 8, order 1: 0.28 / 0.41 / 8, order 2: 0.38 / 0.47 / 8,
           box 0.52 / 0.74 / 16, ladder 0.48 / 0.37 / 8
    edge   eval 1.86 / 1.84 / 32, deriv order 0: 1.86 / 1.84 / 32, order 1: 1.46 / 1.81 / 32, order 2: 2.60 / 3.24 / 64,
           box 2.08 / 2.91 / 64, ladder 2.69 / 2.80 / 64"""
import functools

import numpy as np
import pytest

import tt_chain as C
from pychebyshev_amd import _lib
from tt_rows import check, model as _model, set_kernel as _set_kernel

pytestmark = pytest.mark.gpu

SWEEP = C.sweep_models()
EDGE = C.edge_models()
WORST = {}
_check = functools.partial(check, WORST)      # tests/tt_rows.py: the normwise bar, then every row against its amplitude


def _kept(b, dims):
    kept = [u for u in range(len(b.model.n)) if u not in dims]
    return np.ascontiguousarray(b.pts[:, kept]) if kept else None


def _run_deriv(tt, b, chain, group):
    m = b.model
    specs = C.deriv_specs(m)
    got = tt.eval_multi_batch(b.pts, specs, method="analytic")            # <= 14 specs: one launch
    assert got.shape == (m.rows, len(specs))
    un = [m.n[C.storage_position(b, u)] for u in range(len(m.n))]
    for i, spec in enumerate(specs):
        if any(p >= un[u] for u, p in enumerate(spec)):                  # an order reaches the node count: exactly 0.0
            assert np.all(got[:, i] == 0.0), f"{m.name} deriv {spec}"
        _check(got[:, i], chain.deriv(spec), group, "deriv", C.family_of(spec), f"{m.name} deriv {spec}")
    return got


def _run_box(tt, b, chain, group):
    out = []
    for dims, bounds in C.box_cases(b):
        got = tt.integrate_batch(dims, bounds, _kept(b, dims))
        _check(got, chain.box(dims, bounds), group, "box", "box", f"{b.model.name} box {dims}")
        assert got[1] == 0.0, f"{b.model.name} box {dims}: row 1 has lo == hi"
        out.append(got)
    return out


def _run_ladder(tt, b, chain, group):
    out = []
    for dim, xs in C.ladder_cases(b):
        got = tt.ladder_batch(dim, np.delete(b.pts, dim, axis=1), xs)
        _check(got, chain.ladder(dim, xs), group, "ladder", "ladder",
               f"{b.model.name} ladder dim {dim} {'per row' if xs.ndim == 2 else 'shared'}")
        out.append(got)
    return out


def _box_without_an_integrated_dimension(tt, b):
    """The C entry with every flag zero is the value: equal to eval_batch to 1e-13 normwise."""
    t = tt._dev()
    out = np.full(b.model.rows, np.nan)
    flags = np.zeros(len(b.model.n), dtype=np.int32)
    assert t.lib.pcx_tt_box_batch(t.handle, _lib.p_i32(flags), _lib.p_f64(b.pts), b.pts.shape[0], _lib.p_f64(out)) == 0
    ref = tt.eval_batch(b.pts)
    assert np.max(np.abs(out - ref)) <= 1e-13 * np.max(np.abs(ref)), b.model.name


@pytest.mark.parametrize("model", SWEEP, ids=[m.name for m in SWEEP])
def test_lane_bodies(model):
    b = C.build(model)
    tt = _model(b)
    chain = C.Chain(b.cores, b.domain, b.order, b.pts)
    # eval: the lane kernel forced, then auto (a rank-16 bond sends auto to the MFMA form)
    for variant in (4, 0):
        _set_kernel(tt, variant)
        _check(tt.eval_batch(b.pts), chain.value(), "sweep", "eval", "value", f"{model.name} eval variant {variant}")
    # fd on the lane kernel (variant 4: also where auto would not take it): the host traversal's bits, and column 0
    # the evaluation's
    _set_kernel(tt, 4)
    specs = C.fd_specs(model)
    fd = tt.eval_multi_batch(b.pts, specs)
    assert fd.shape == (model.rows, 4)
    assert np.array_equal(fd, tt._eval_multi_batch_host(b.pts, specs)), f"{model.name} fd {specs}"
    assert np.array_equal(fd[:, 0], tt.eval_batch(b.pts)), f"{model.name} fd column 0"
    _set_kernel(tt, 0)
    _run_deriv(tt, b, chain, "sweep")
    _run_box(tt, b, chain, "sweep")
    _box_without_an_integrated_dimension(tt, b)
    _run_ladder(tt, b, chain, "sweep")


@pytest.mark.parametrize("model", EDGE, ids=[m.name for m in EDGE])
def test_wave_per_row_lane_loops(model):
    """k_tt_box_generic, k_tt_deriv_generic, k_tt_ladder_generic: `for (b = lane; b < rr; b += 64)` with one, two and
    three trips, and the model that is generic only because n > 16.  130 rows: 32 blocks of four waves and two rows."""
    b = C.build(model)
    tt = _model(b)
    chain = C.Chain(b.cores, b.domain, b.order, b.pts)
    _check(tt.eval_batch(b.pts), chain.value(), "edge", "eval", "value", f"{model.name} eval")
    _run_deriv(tt, b, chain, "edge")
    _run_box(tt, b, chain, "edge")
    _box_without_an_integrated_dimension(tt, b)
    _run_ladder(tt, b, chain, "edge")


def test_batch_tails_are_the_leading_rows():
    """deriv, box and ladder at N = 1, 63, 64, 65, 127, 128 against the N = 129 call, bit for bit: a lane past the batch
    works on row N - 1 and stores nothing."""
    b = C.build(C.tail_model())
    tt = _model(b)
    chain = C.Chain(b.cores, b.domain, b.order, b.pts)
    full = (_run_deriv(tt, b, chain, "sweep"), _run_box(tt, b, chain, "sweep"), _run_ladder(tt, b, chain, "sweep"))
    specs, boxes, ladders = C.deriv_specs(b.model), C.box_cases(b), C.ladder_cases(b)
    for N in C.TAIL_NS:
        pts = np.ascontiguousarray(b.pts[:N])
        assert np.array_equal(tt.eval_multi_batch(pts, specs, method="analytic"), full[0][:N]), f"deriv N = {N}"
        for (dims, bounds), want in zip(boxes, full[1]):
            kept = _kept(b, dims)
            got = tt.integrate_batch(dims, bounds[:N], None if kept is None else kept[:N])
            assert np.array_equal(got, want[:N]), f"box {dims} N = {N}"
        for (dim, xs), want in zip(ladders, full[2]):
            got = tt.ladder_batch(dim, np.delete(pts, dim, axis=1), xs if xs.ndim == 1 else np.ascontiguousarray(xs[:N]))
            assert np.array_equal(got, want[:N]), f"ladder dim {dim} N = {N}"


def test_worst_rows_stay_in_the_restatements_range():
    """Runs last: the worst row of every kernel family over the cases that ran in this session, next to the
    restatement's figure (the numbers DESIGN.md section 5 quotes)."""
    for key in sorted(WORST):
        group, _, family = key.split(" ")
        print(f"{key}: worst {WORST[key]:.3f} eps A_row, restatement {C.RESTATEMENT_WORST[group][family]:.3f}, K {C.K[group][family]}")
        assert WORST[key] <= C.K[group][family]
