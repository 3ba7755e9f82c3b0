"""Every reachable body of the grid and k-fold MFMA barycentric kernels -- k_bary_mfma_grid<KS, NT, WPB, AF>
(csrc/bary_grid_kernels.h, launch_grid_nt of csrc/pcx_bary_grid.hip) and k_bary_mfma_kfold<MT, KS2, NT, STR, SM>
(csrc/bary_kfold_kernels.h, launch_kfold_t of csrc/pcx_bary_kfold.hip) -- against the long-double reference of
tests/bary_ld.py.

The lists are bary_gk_ld.grid_models() (193: every (KS 1 .. 32, WPB 1 / 4, AF) of the switch, 63 plans that take every
run-time path -- RA x outer dimensions x tail dimensions, padded A / B, one to three tiles along A and B, a ragged split
-- on either side of the WHOLE switch, two domains of unusual width) and bary_gk_ld.kfold_models() (105: the 54
reachable (MT, KS2, STR), the straddled ones with an even and an odd loop dimension, the six role assignments at one to
four row tiles, loop dimensions of 65 .. 80 nodes, the straddled shapes on padded bodies, two domains);
tests/test_bary_gk_ld_host.py asserts from the lists and the GPU-free planner which bodies they reach.  One case per
model: the handle is created with PCX_BARY_GRID=2 and PCX_BARY_KFOLD=0 (grid) or PCX_BARY_KFOLD_EFF=1 (k-fold), its
calls run, and it is dropped.

Per model, variant 2 forced (a refusal fails the case), on 96 rows -- corners, a grid point, per role of the form a row
on a node, a row 3e-15 and a row 4e-14 beside one, uniform rows; the grid form runs them as a split launch through
k_bary_grid_reduce, the k-fold form of two row tiles or more on the split-M kernel:
  plan        pcx_bary_kernel_info and pcx_bary_grid_info equal the list
  normwise    max |got - ref| <= 1e-12 max |ref|
  row by row  |got - ref| <= K eps A_row, K = bary_gk_ld.K (16 times the float64 restatement's worst row, at most 128)
  grid point  the tensor entry exactly
  three specs [value, d/dx_last, d/dx_first] in one launch: column 0 the single call bit for bit, the derivative columns
              against the long-double sum over the derived tensor read back from the device
  batches     the 96 rows tiled to 40,000 points (unsplit, one column tile per wave; k-fold: the four-wave kernel) and
              to 65,536 + 777 (two column tiles wherever the plan has them): every row the 96-row call's bit for bit
  second handles, every eighth model: PCX_BARY_GRID_PROD=0 (weights by division) against the reference with the
              division rule's K; grid models: a batch that splits the chunks raggedly, bit for bit
Two splines per form with buckets of 0, 1, 63, 64, 65 and 129 rows (the perm path), each piece against its own
reference; one model per form with NaN coordinates.

Worst |got - ref| / (eps A_row), the restatement's figure -> measured on MI355X (K):
    k_bary_mfma_grid   product weights: value 3.48 -> 3.55 (64); first derivative 4.02 -> 4.65 (128)
                       by division:     value 4.51 -> 4.65 (128); first derivative 6.06 -> 6.06 (128)
    k_bary_mfma_kfold  product weights: value 5.74 -> 5.74 (128); first derivative 6.86 -> 6.86 (128)
                       by division:     value 6.85 -> 6.31 (128); first derivative 6.28 -> 6.28 (128)
The tiled batches and the ragged splits are those rows bit for bit."""
import numpy as np
import pytest

import bary_gk_ld as G
import bary_ld as B
from conftest import assert_parity, spec_point_tol
from pychebyshev_amd import ChebyshevApproximation, _lib

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not B.LD_OK, reason="np.longdouble is no wider than float64 here")]

GRID, KFOLD, SPLINES = G.grid_models(), G.kfold_models(), G.spline_models()
WORST = {}


def _check(got, pair, m, order, rule, what):
    B.check(WORST, got, pair, m.form, order, rule, what, k=G.K[m.form][rule][order])


def _info(c, fn, n):
    h = c._model()
    info = _lib.i32(np.zeros(n))
    _lib.check(getattr(h.lib, fn)(h.handle, _lib.p_i32(info)), h.lib)
    return tuple(int(v) for v in info)


def _set_kernel(c, variant):
    """A refusal raises: a failure of the case, not a skip."""
    h = c._model()
    _lib.check(h.lib.pcx_bary_set_kernel(h.handle, variant), h.lib)


def _setenv(monkeypatch, m, grid_prod=True):
    """The environment is read when a handle is created."""
    for name, value in G.ENVS[m.env].items():
        monkeypatch.setenv(name, value)
    for name, value in (("PCX_BARY_GRID_PROD", "1" if grid_prod else "0"), ("PCX_BARY_SEED", "1"), ("PCX_BARY_TAIL", "1")):
        monkeypatch.setenv(name, value)


def _plans_as_listed(c, m):
    ki, gi = _info(c, "pcx_bary_kernel_info", 6), _info(c, "pcx_bary_grid_info", 4)
    assert gi == m.grid_info and gi[0] == (1 if m.form == "grid" else 2), f"{m.name}: grid_info {gi}, listed {m.grid_info}"
    assert ki == m.kernel_info, f"{m.name}: kernel_info {ki}, listed {m.kernel_info}"


def _handle(monkeypatch, b, grid_prod=True):
    """A fresh model of the list entry on the form of its list, variant 2 forced."""
    m = b.model
    _setenv(monkeypatch, m, grid_prod)
    c = ChebyshevApproximation.from_values(b.c.tensor_values, len(m.shape), b.c.domain, list(m.shape))
    _set_kernel(c, 2)
    _plans_as_listed(c, m)
    return c


def _derived(c, spec):
    """The derived tensor the device contracts, and it is the oracle's bit for bit."""
    if not any(spec):
        return c.tensor_values
    h = c._model()
    got = np.empty(c.tensor_values.shape)
    _lib.check(h.lib.pcx_bary_derivative_tensor(h.handle, _lib.p_i32(_lib.i32(spec)), _lib.p_f64(got)), h.lib)
    assert np.array_equal(got, B.derived_tensor(c, spec)), spec
    return got


def _tiled(pts, n):
    idx = np.arange(n) % len(pts)
    return np.ascontiguousarray(pts[idx]), idx


def _bounds(c, b, pairs, rule):
    """The 96-row calls of one handle against the reference: (value column, multi-spec block)."""
    m, pts, d = b.model, b.pts, len(b.model.shape)
    got = c.vectorized_eval_batch(pts, [0] * d)
    _check(got, pairs[0], m, "value", rule, f"{m.name} value, {rule}")
    assert got[b.grid_row] == c.tensor_values[b.grid_idx], f"{m.name}: the grid-point row is not the tensor entry"
    specs = G.specs_of(m.shape)
    multi = c.vectorized_eval_multi_batch(pts, specs)
    assert multi.shape == (m.rows, len(specs))
    assert np.array_equal(multi[:, 0], got), f"{m.name}: column 0 of the multi-spec launch"
    for j, spec in enumerate(specs[1:], start=1):
        _check(multi[:, j], pairs[j], m, "order1", rule, f"{m.name} {spec}, {rule}")
        assert_parity(multi[:, j], pairs[j][0].astype(np.float64), 1e-12, f"{m.name} {spec}", spec_point_tol(spec))
    return got, multi


def _run(monkeypatch, m, index):
    b = G.build(m)
    c = _handle(monkeypatch, b)
    value = [0] * len(m.shape)
    # the reference once per model and spec: the tiled batches and the second handles reuse it
    pairs = [B.reference(c.nodes, c.weights, _derived(c, spec), b.pts) for spec in G.specs_of(m.shape)]
    got, multi = _bounds(c, b, pairs, G.rule_of(m))
    for n in (G.BATCH_NT1, G.BATCH_NT2):
        big, idx = _tiled(b.pts, n)
        assert np.array_equal(c.vectorized_eval_batch(big, value), got[idx]), f"{m.name}: N = {n} differs from the {m.rows}-row call"
    if G.second_handle(index):
        if m.form == "grid":
            n = G.ragged_batch(m.body[1], m.claim[6])
            if n is not None:                  # 1 < nsplit < nchunks, the last part shorter than the others
                big, idx = _tiled(b.pts, n)
                assert np.array_equal(c.vectorized_eval_batch(big, value), got[idx]), f"{m.name}: the ragged split at N = {n} differs"
        if m.grid_prod:                        # weights by division: its own rounding, held to the reference
            c0 = _handle(monkeypatch, b, grid_prod=False)
            got0, _ = _bounds(c0, b, pairs, "div")
            big, idx = _tiled(b.pts, G.BATCH_NT2)
            assert np.array_equal(c0.vectorized_eval_batch(big, value), got0[idx]), f"{m.name}: by division, N = {len(big)}"
    return b, c, got


@pytest.mark.parametrize("i", range(len(GRID)), ids=[m.name for m in GRID])
def test_grid_bodies(i, monkeypatch):
    """k_bary_mfma_grid<KS, 1 and nt, WPB, AF> of the model's body: split (96 rows, k_bary_grid_reduce) and unsplit."""
    _run(monkeypatch, GRID[i], i)


@pytest.mark.parametrize("i", range(len(KFOLD)), ids=[m.name for m in KFOLD])
def test_kfold_bodies(i, monkeypatch):
    """k_bary_mfma_kfold<MT, KS2, 1 and nt, STR> of the model's body, and <MT, KS2, 1, STR, SM> at 96 rows for MT >= 2."""
    _run(monkeypatch, KFOLD[i], i)


@pytest.mark.parametrize("m", SPLINES, ids=[m.name for m in SPLINES])
def test_bucket_edges(m, monkeypatch):
    """Six pieces along dimension 0 whose buckets hold 0, 1, 63, 64, 65 and 129 rows, in shuffled order: the perm path of
    both kernels.  Every piece against its own reference, and equal to the same rows evaluated one piece at a time."""
    _setenv(monkeypatch, m)
    b = B.build_spline(m, B.BUCKETS)
    sp, pts = b.sp, b.pts
    for piece in sp._pieces:                    # the spline handle holds the pieces' own handles
        _set_kernel(piece, 2)
        _plans_as_listed(piece, m)
    assert np.array_equal(sp.piece_indices(pts), b.ids)
    assert sorted(np.bincount(b.ids, minlength=6).tolist()) == sorted(B.BUCKETS)
    specs = B.piece_specs_of(m.shape)
    pairs = [B.spline_reference(sp, [_derived(p, spec) for p in sp._pieces], pts, b.ids) for spec in specs]
    got = sp.eval_batch(pts, specs[0])
    multi = sp.eval_multi_batch(pts, specs)
    _check(got, pairs[0], m, "value", G.rule_of(m), f"{m.name} value")
    _check(multi[:, 1], pairs[1], m, "order1", G.rule_of(m), f"{m.name} {specs[1]}")
    assert np.array_equal(multi[:, 0], got)
    for p in np.unique(b.ids):
        rows = np.nonzero(b.ids == p)[0]
        sub = np.ascontiguousarray(pts[rows])
        assert np.array_equal(sp.eval_batch(sub, specs[0]), got[rows]), f"{m.name}: piece {p} alone"
        assert np.array_equal(sp._pieces[int(p)].vectorized_eval_batch(sub, specs[0]), got[rows]), f"{m.name}: piece {p}'s own handle"


@pytest.mark.parametrize("m", [GRID[40], KFOLD[20]], ids=lambda m: m.name)
def test_nan_rows(m, monkeypatch):
    """A NaN coordinate gives NaN in that row and nowhere else: 96 rows and the 65,536 + 777 batch."""
    b = G.build(m)
    c = _handle(monkeypatch, b)
    d = len(m.shape)
    got = c.vectorized_eval_batch(b.pts, [0] * d)
    pts = b.pts.copy()
    bad = [20 + 7 * k for k in range(d)] + [95]
    for r, k in zip(bad, list(range(d)) + [0]):
        pts[r, k] = np.nan
    pts[95, :] = np.nan
    for n in (m.rows, G.BATCH_NT2):
        big, idx = _tiled(pts, n)
        y = c.vectorized_eval_batch(big, [0] * d)
        isbad = np.isin(idx, bad)
        assert np.all(np.isnan(y[isbad])), f"{m.name}: a NaN row is finite, N = {n}"
        assert np.array_equal(y[~isbad], got[idx][~isbad]), f"{m.name}: a NaN row changed another row, N = {n}"


def test_worst_rows_stay_in_the_restatements_range():
    """Runs last: the worst row per (form, spec order, weight rule) over the cases that ran in this session, next to the
    restatement's figure (the numbers DESIGN.md section 5 quotes).  The tiled batches and ragged splits are the 96-row
    calls bit for bit, so their worst rows are these."""
    for key in sorted(WORST):
        form, order, rule = key.split(" ")
        k = G.K[form][rule][order]
        print(f"{key} (and the tiled batches, bit-identical): worst {WORST[key]:.3f} eps A_row, restatement {G.RESTATEMENT_WORST[form][rule][order]:.3f}, K {k}")
        assert WORST[key] <= k
