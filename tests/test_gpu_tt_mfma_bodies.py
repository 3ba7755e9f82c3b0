"""Every body of the three MFMA forms of ChebyshevTT.eval_batch -- k_tt_eval_mfma (16x16x4 direct form, variant 1),
k_tt_eval_wfirst (W-first, variant 2) and k_tt_eval_d4 (4x4x4, variant 3), csrc/tt_kernels.h -- against the long-double
chain of tests/tt_chain.py.

The list is tt_chain.mfma_models(): 220 seeded models of 96 rows (both domain corners among them, every third model
behind a permuted dim_order).  tests/test_tt_chain_host.py proves from the list and tests/tt_plan_rule.py alone that it
reaches
  83 bodies of the direct form    the six instantiations <1|2|3|4, 1, 4>, <8, 2, 2>, <16, 4, 1>, each with d >= 3, the
                                  node loop of dimension 0 and of a middle dimension ending in every way (no pair, one
                                  pair, pair + peeled node, several pairs, several + peel; the plain loop of ranks > 16
                                  likewise), the last core read from its LDS copy and from global memory; d = 1; d = 2
  48 of the W-first form          <R, KS, NT> for R = 4, 8, 12 and KS = 1 .. 8, a middle dimension that spreads v' and
                                  the one that does not; from KS = 2 on beside a dimension whose last k-step is all zero rows
  108 of the 4x4x4 form           RA = 1, 2, 3 x (k-steps 1 .. 4 of dimension 0, NJ = 1 .. 16 of tt_d4_mid and tt_d4_last)
and which variants each model's plan offers.  One case per model: every offered variant of (1, 2, 3) is forced, then
auto; a variant the plan does not offer is refused with PCX_ERR_UNSUPPORTED.  Then the batch tails of one model per kernel
family, a second and third trip of the persistent batch loops, the finite-difference Greeks on the materialising path.

Bounds against the long-double chain, per call (tests/tt_rows.py):
  normwise    max |got - ref| <= 1e-12 max |ref|
  row by row  |got - ref| <= K eps A_row, K = 16 times the worst ratio of the float64 restatement of the chain, rounded up
              to a power of two, at most 64.  d <= 2: A_row also holds the row's first-order change under one eps of s
              (tt_chain.RESTATEMENT_WORST says why)

Worst |got - ref| / (eps A_row) measured on MI355X / the restatement's figure / K:
    mfma       variant 1: 1.72 / 1.21 / 32, variant 2: 1.11 / 1.21 / 32, variant 3: 1.22 / 1.21 / 32, auto: 1.22 / 1.21 / 32
    mfma-lowd  variant 1: 0.54 / 0.63 / 16, variant 2: 0.61 / 0.63 / 16, variant 3: 0.54 / 0.63 / 16, auto: 0.61 / 0.63 / 16
233 cases, 3 s wall."""
import ctypes
import functools

import numpy as np
import pytest

import tt_chain as C
from pychebyshev_amd import _lib
from pychebyshev_amd.device import DeviceArray
from tt_rows import check, model as _model, set_kernel as _set_kernel

pytestmark = pytest.mark.gpu

MODELS = C.mfma_models()
WORST = {}
_check = functools.partial(check, WORST)


def _eval(tt, variant, pts):
    _set_kernel(tt, variant)
    return tt.eval_batch(pts)


@pytest.mark.parametrize("model", MODELS, ids=[m.name for m in MODELS])
def test_mfma_bodies(model):
    b = C.build(model)
    tt = _model(b)
    group = C.group_of(model)
    pair = C.value_pair(C.Chain(b.cores, b.domain, b.order, b.pts), group)
    offered = C.offered(model)
    t = tt._dev()
    for variant in (1, 2, 3):
        if variant not in offered:
            assert t.lib.pcx_tt_set_kernel(t.handle, variant) == _lib.PCX_ERR_UNSUPPORTED, f"{model.name} variant {variant}"
    for variant in offered + (0,):
        _check(_eval(tt, variant, b.pts), pair, group, f"variant{variant}", "value", f"{model.name} variant {variant}")


TAILS = C.mfma_tail_models()


@pytest.mark.parametrize("model,variant", TAILS, ids=[m.name for m, _ in TAILS])
def test_batch_tails_are_the_leading_rows(model, variant):
    """N = 1 .. 257 around every multiple of a wave's 16 NT points and a workgroup's 64 NT, against the N = 300 call, bit
    for bit: a lane past the batch reads zeros and stores nothing."""
    b = C.build(model)
    tt = _model(b)
    full = _eval(tt, variant, b.pts)
    _check(full, C.Chain(b.cores, b.domain, b.order, b.pts).value(), "mfma", f"variant{variant}", "value", model.name)
    for N in C.MFMA_TAIL_NS:
        got = tt.eval_batch(np.ascontiguousarray(b.pts[:N]))
        assert got.shape == (N,) and np.array_equal(got, full[:N]), f"{model.name} N = {N}"


def _compute_units(t):
    cus = ctypes.c_int()
    _lib.check(t.lib.pcx_device_info(t.device, None, 0, ctypes.byref(cus), None), t.lib)
    return cus.value


PERSISTENT = C.persistent_models()


@pytest.mark.parametrize("model,variant,per_batch", PERSISTENT, ids=[f"{m.name}-variant{v}" for m, v, _ in PERSISTENT])
def test_the_persistent_batch_loop_takes_further_trips(model, variant, per_batch):
    """The launchers start at most 4 x resident workgroups, and no more than floor(160 KiB / launch LDS) are resident on
    a CU: with 3 x 4 x r x CUs batches and a ragged one, some workgroup walks at least three batches and prefetches the
    rows of two.  Every row equals the same row of the 96-row call, bit for bit."""
    b = C.build(model)
    tt = _model(b)
    small = _eval(tt, variant, b.pts)
    _check(small, C.Chain(b.cores, b.domain, b.order, b.pts).value(), "mfma", f"variant{variant}", "value", model.name)
    r, cus = C.CU_LDS_BYTES // C.launch_lds(model, variant), _compute_units(tt._dev())
    workgroups = 4 * r * cus
    N = 3 * workgroups * per_batch + 777
    batches = -(-N // per_batch)
    print(f"{model.name}: {cus} CUs x {r} resident, at most {workgroups} workgroups for {batches} batches, N = {N}")
    assert r >= 1 and cus >= 1 and batches > 2 * workgroups, "the busiest workgroup would take fewer than three trips"
    assert N * len(model.n) * 8 < 120e6
    reps = -(-N // model.rows)
    # a device array: one launch over all N rows (a host batch of this size is cut into pieces of 65,536 rows and up)
    rows = DeviceArray.from_host(np.ascontiguousarray(np.tile(b.pts, (reps, 1))[:N]), tt._dev().device)
    got = tt.eval_batch(rows).to_host()
    rows.free()
    want = np.tile(small, reps)[:N]
    differ = np.flatnonzero(got != want)
    assert differ.size == 0, f"{model.name}: {differ.size} rows differ, the first at {differ[0]} (batch {differ[0] // per_batch})"


FD = (next(m for m in MODELS if m.name == "large1-uniform-n5"), next(m for m in MODELS if m.name == "large2-uniform-n4"),
      C.edge_models()[0])


@pytest.mark.parametrize("model", FD, ids=[m.name for m in FD])
def test_fd_on_the_materialising_path(model):
    """k_tt_fd_points / k_tt_fd_combine around the model's own kernel (<8, 2, 2>, <16, 4, 1>, generic): a value, a first
    order, a second order and a mixed spec on rows that include both domain corners equal the host traversal, and column
    0 equals eval_batch, bit for bit."""
    assert (max(model.ranks) > 64) == (model.mode == "generic") and max(model.ranks) in (32, 64, 65)
    b = C.build(model)
    tt = _model(b)
    specs = C.fd_specs(model)
    assert [sum(s) for s in specs] == [0, 1, 2, 2] and max(specs[3]) == 1
    fd = tt.eval_multi_batch(b.pts, specs)
    assert fd.shape == (model.rows, 4)
    assert np.array_equal(fd, tt._eval_multi_batch_host(b.pts, specs)), f"{model.name} fd {specs}"
    assert np.array_equal(fd[:, 0], tt.eval_batch(b.pts)), f"{model.name} fd column 0"


def test_worst_rows_stay_in_the_restatements_range():
    """Runs last: the worst row per group and variant over the cases that ran in this session, next to the
    restatement's figure (the numbers DESIGN.md section 5 quotes)."""
    for key in sorted(WORST):
        group, _, family = key.split(" ")
        print(f"{key}: worst {WORST[key]:.3f} eps A_row, restatement {C.RESTATEMENT_WORST[group][family]:.3f}, K {C.K[group][family]}")
        assert WORST[key] <= C.K[group][family]
