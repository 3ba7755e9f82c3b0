"""Every body of the row-code MFMA barycentric kernels -- k_bary_mfma<KS, NT, WIDE, NF, false, R> and
k_bary_mfma4<KS, R> (csrc/bary_kernels.h), as launch_mfma_nf and launch_mfma4 (csrc/bary_mfma_launch.h) launch them --
against the long-double reference of tests/bary_ld.py.

The lists are bary_mfma_ld.rowcode_models() (616: every (KS 1 .. 32, nf2 / nf3 / nf4 / wide, R 0 / 1 / 2), the R = 0
bodies once by K = 4 KS and once by K = 4 KS - 1; 36 .. 64 in every class and R; 42 seeded), tile_models() (60: the five
tile loops at 1, 2, 3, 4, 7, 8, 9 row tiles, three- and four-dimensional tails) and mfma4_models() (89);
tests/test_bary_mfma_ld_host.py asserts from the lists and the GPU-free planner which bodies they reach.  One case per
model: the handle is created with the grid and k-fold forms off, its calls run, and it is dropped.

Per model, variant 2 forced (a refusal fails the case), on 96 rows -- corners, a grid point, rows on a node of a head or
of a tail dimension only, rows 3e-15 beside a node, uniform rows:
  plan        pcx_bary_kernel_info / _grid_info / _tail_info equal the list: MT, KS, split, points per workgroup, chunks
  normwise    max |got - ref| <= 1e-12 max |ref|
  row by row  |got - ref| <= K eps A_row, K = bary_mfma_ld.K (128: 16 times the float64 restatement's worst row)
  grid point  the tensor entry exactly
  three specs [value, d/dx_last, d/dx_first] in one launch (grid.z, frag_tab[z]): column 0 the single call bit for bit,
              the derivative columns against the long-double sum over the derived tensor read back from the device
  batches     the 96 rows tiled to 40,000 points (one column tile per wave, unsplit or tail-split) and to 65,536 + 777
              (two column tiles wherever the plan has them): every row the 96-row call's bit for bit -- which ran as a
              split launch through k_bary_reduce -- so the NT = 2 bodies are held to the reference through NT = 1
  seed        a seeded model equals its PCX_BARY_SEED=0 handle bit for bit: (KS or KS + 1, R = 0), zero-padded columns
  tail split  every eighth model again on a PCX_BARY_TAIL=2 handle at the large batch, bit for bit
  variant 3   where the plan offers it, bit for bit variant 2; where it does not, PCX_ERR_UNSUPPORTED

Worst |got - ref| / (eps A_row), the restatement's figure -> measured on MI355X (K):
    k_bary_mfma   value 5.63 -> 5.29 (128); first derivative 6.25 -> 6.25 (128)
    k_bary_mfma4  value 5.63 -> 5.42 (128); first derivative 6.25 -> 4.05 (128)
The tiled batches, the unseeded handles and the other variant are those rows bit for bit."""
import numpy as np
import pytest

import bary_ld as B
import bary_mfma_ld as M
from conftest import assert_parity, spec_point_tol
from pychebyshev_amd import ChebyshevApproximation, _lib

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not B.LD_OK, reason="np.longdouble is no wider than float64 here")]

ROWCODE, TILES, MFMA4 = M.rowcode_models(), M.tile_models(), M.mfma4_models()
WORST = {}


def _check(got, pair, family, order, group, what):
    B.check(WORST, got, pair, family, order, group, what, k=M.K[order])


def _info(c, fn, n):
    m = c._model()
    info = _lib.i32(np.zeros(n))
    _lib.check(getattr(m.lib, fn)(m.handle, _lib.p_i32(info)), m.lib)
    return [int(v) for v in info]


def _set_kernel(c, variant):
    """A refusal raises: a failure of the case, not a skip."""
    m = c._model()
    _lib.check(m.lib.pcx_bary_set_kernel(m.handle, variant), m.lib)


def _handle(monkeypatch, b, seed=True, tail=1):
    """A fresh model of the list entry on the row-code form: the environment is read when the handle is created."""
    for name, value in M.ENV_OFF.items():
        monkeypatch.setenv(name, value)
    monkeypatch.setenv("PCX_BARY_SEED", "1" if seed else "0")
    monkeypatch.setenv("PCX_BARY_TAIL", str(tail))
    shape = b.model.shape
    c = ChebyshevApproximation.from_values(b.c.tensor_values, len(shape), b.c.domain, list(shape))
    _set_kernel(c, 2)
    return c


def _plans_as_listed(c, m, seeded=True):
    ki, gi, ti = _info(c, "pcx_bary_kernel_info", 6), _info(c, "pcx_bary_grid_info", 4), _info(c, "pcx_bary_tail_info", 6)
    assert gi[0] == 0, f"{m.name}: a grid or k-fold plan {gi}"
    assert (ki[1], ki[2], ki[5]) == (m.MT, m.KS if seeded else m.KS0, m.split), f"{m.name}: kernel_info {ki}"
    assert ti[2] == -(-m.MT // 4) and 1 <= ti[0] <= 512, f"{m.name}: tail_info {ti}"
    if seeded:
        assert ki[4] == ti[1] == 64 * m.nt, f"{m.name}: points per workgroup {ki} {ti}"


def _derived(c, spec):
    """The derived tensor the device contracts, and it is the oracle's bit for bit."""
    if not any(spec):
        return c.tensor_values
    m = c._model()
    got = np.empty(c.tensor_values.shape)
    _lib.check(m.lib.pcx_bary_derivative_tensor(m.handle, _lib.p_i32(_lib.i32(spec)), _lib.p_f64(got)), m.lib)
    assert np.array_equal(got, B.derived_tensor(c, spec)), spec
    return got


def _tiled(pts, n):
    idx = np.arange(n) % len(pts)
    return np.ascontiguousarray(pts[idx]), idx


def _bounds(c, b, variant, group):
    """The 96-row (tile models: 130-row) calls of one variant against the reference: (value column, multi-spec block)."""
    m, pts, d = b.model, b.pts, len(b.model.shape)
    _set_kernel(c, variant)
    pair = B.reference(c.nodes, c.weights, c.tensor_values, pts)
    got = c.vectorized_eval_batch(pts, [0] * d)
    _check(got, pair, m.family, "value", group, f"{m.name} value, variant {variant}")
    assert got[b.grid_row] == c.tensor_values[b.grid_idx], f"{m.name}: the grid-point row is not the tensor entry"
    specs = M.specs_of(m.shape)
    multi = c.vectorized_eval_multi_batch(pts, specs)
    assert multi.shape == (m.rows, len(specs))
    assert np.array_equal(multi[:, 0], got), f"{m.name}: column 0 of the multi-spec launch"
    for j, spec in enumerate(specs[1:], start=1):
        pj = B.reference(c.nodes, c.weights, _derived(c, spec), pts)
        _check(multi[:, j], pj, m.family, "order1", group, f"{m.name} {spec}, variant {variant}")
        assert_parity(multi[:, j], pj[0].astype(np.float64), 1e-12, f"{m.name} {spec}", spec_point_tol(spec))
    return got, multi


def _run_rowcode(monkeypatch, m, index):
    b = M.build(m)
    c = _handle(monkeypatch, b)
    _plans_as_listed(c, m)
    value = [0] * len(m.shape)
    got, multi = _bounds(c, b, 2, "rows")
    for n in (M.BATCH_NT1, M.BATCH_NT2):
        big, idx = _tiled(b.pts, n)
        assert np.array_equal(c.vectorized_eval_batch(big, value), got[idx]), f"{m.name}: N = {n} differs from the {m.rows}-row call"
    m_ = c._model()
    if m.mfma4:                                # k_bary_mfma4 on the same handle: the same bits
        _set_kernel(c, 3)
        assert np.array_equal(c.vectorized_eval_batch(b.pts, value), got), f"{m.name}: variant 3 differs from variant 2"
        _set_kernel(c, 2)
    else:
        assert m_.lib.pcx_bary_set_kernel(m_.handle, 3) == _lib.PCX_ERR_UNSUPPORTED, f"{m.name}: variant 3 was not refused"
        _set_kernel(c, 2)
    if m.R > 0:                                # the unseeded form: every column in the k-loop, (KS or KS + 1, R = 0)
        c0 = _handle(monkeypatch, b, seed=False)
        _plans_as_listed(c0, m, seeded=False)
        assert np.array_equal(c0.vectorized_eval_batch(b.pts, value), got), f"{m.name}: the unseeded handle differs"
        assert np.array_equal(c0.vectorized_eval_multi_batch(b.pts, M.specs_of(m.shape)), multi), f"{m.name}: the unseeded handle differs, multi-spec"
        big, idx = _tiled(b.pts, M.BATCH_NT2)
        assert np.array_equal(c0.vectorized_eval_batch(big, value), got[idx]), f"{m.name}: the unseeded handle differs, N = {len(big)}"
    if index % 8 == 0:                         # the tail split wherever the geometry allows
        c2 = _handle(monkeypatch, b, tail=2)
        big, idx = _tiled(b.pts, M.BATCH_NT2)
        assert np.array_equal(c2.vectorized_eval_batch(big, value), got[idx]), f"{m.name}: PCX_BARY_TAIL=2 differs"
    return b, c, got, multi


@pytest.mark.parametrize("i", range(len(ROWCODE)), ids=[m.name for m in ROWCODE])
def test_rowcode_bodies(i, monkeypatch):
    """k_bary_mfma<KS, 1 and nt, WIDE, NF, false, R> of the model's body."""
    _run_rowcode(monkeypatch, ROWCODE[i], i)


@pytest.mark.parametrize("i", range(len(TILES)), ids=[m.name for m in TILES])
def test_tile_loop_edges(i, monkeypatch):
    """The five tile loops at 1, 2, 3, 4, 7, 8, 9 row tiles and the four-field tail weights: the bounds of the body cases,
    and the batch tails N = 1 .. 129 against the leading rows of the 130-row call, bit for bit."""
    m = TILES[i]
    b, c, got, multi = _run_rowcode(monkeypatch, m, i)
    specs = M.specs_of(m.shape)
    for n in M.TAIL_NS:
        pts = np.ascontiguousarray(b.pts[:n])
        assert np.array_equal(c.vectorized_eval_batch(pts, specs[0]), got[:n]), f"{m.name} N = {n}"
        assert np.array_equal(c.vectorized_eval_multi_batch(pts, specs), multi[:n]), f"{m.name} N = {n}, {len(specs)} specs"


@pytest.mark.parametrize("i", range(len(MFMA4)), ids=[m.name for m in MFMA4])
def test_mfma4_bodies(i, monkeypatch):
    """k_bary_mfma4<KS, R>: the bounds at 96 rows, bit for bit variant 2 on the same handle, the tiled 65,536 + 777 batch."""
    m = MFMA4[i]
    b = M.build(m)
    c = _handle(monkeypatch, b)
    _plans_as_listed(c, m)
    value = [0] * len(m.shape)
    got, multi = _bounds(c, b, 3, "rows")
    big, idx = _tiled(b.pts, M.BATCH_NT2)
    assert np.array_equal(c.vectorized_eval_batch(big, value), got[idx]), f"{m.name}: N = {len(big)} differs from the 96-row call"
    _set_kernel(c, 2)
    assert np.array_equal(c.vectorized_eval_batch(b.pts, value), got), f"{m.name}: variant 2 differs from variant 3"
    assert np.array_equal(c.vectorized_eval_multi_batch(b.pts, M.specs_of(m.shape)), multi), f"{m.name}: variant 2 differs, multi-spec"
    if m.R > 0:
        c0 = _handle(monkeypatch, b, seed=False)
        _set_kernel(c0, 3 if M.plan_of(m.shape, m.split, False)[5] else 2)         # one k-step more may not fit variant 3's LDS
        assert np.array_equal(c0.vectorized_eval_batch(b.pts, value), got), f"{m.name}: the unseeded handle differs"


def test_worst_rows_stay_in_the_restatements_range():
    """Runs last: the worst row per (family, spec order) over the cases that ran in this session, next to the
    restatement's figure (the numbers DESIGN.md section 5 quotes).  The 40,000- and 66,313-point batches are the 96-row
    calls bit for bit, so their worst rows are these."""
    for key in sorted(WORST):
        _, order, _ = key.split(" ")
        print(f"{key} (and the tiled batches, bit-identical): worst {WORST[key]:.3f} eps A_row, restatement {M.RESTATEMENT_WORST[order]:.3f}, K {M.K[order]}")
        assert WORST[key] <= M.K[order]
