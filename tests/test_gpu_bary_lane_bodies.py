"""Every body of the lane-per-point barycentric kernels -- k_bary_small<DOUT, NLP>, k_bary_sq<NL, LEAD>,
k_bary_small_pieces<DOUT, NLP> and k_bary_sq_pieces<NL, LEAD> (csrc/bary_kernels.h), as the four switches of
csrc/pcx_bary.hip launch them -- against the long-double reference of tests/bary_ld.py.

The lists are bary_ld.small_models() (d = 1 .. 4 x last-dimension node count 1 .. 64: 256 models), sq_models() (25 NL x 3
LEAD) and piece_models() (171 splines of two to six equal-shape pieces); tests/test_bary_ld_host.py asserts from the
lists alone that they reach all 76 + 75 bodies of either pair of switches, both EXACT branches and every padded n.  One
case per model: the model is created, its calls run, and its handle is dropped.  Then two six-piece splines whose
buckets hold 0, 1, 63, 64, 65 and 129 rows, and the batch tails of seven models.

Bounds against the reference, per call:
  normwise    max |got - ref| <= 1e-12 max |ref|, the project's bar
  row by row  |got - ref| <= K eps A_row, A_row = sum_i |T_i| prod_k |b_k,i_k| the row's amplitude and K = bary_ld.K:
              16 times the worst ratio of the float64 restatement of the kernels, per family and spec order, <= 128
The row bound is the real check: a row that cancels is held to its own terms, not to the largest row of the batch.
Derivative columns are held to the same sum over the derived tensor (read back from the device, and equal to the
oracle's derivative passes bit for bit), with that tensor's own amplitude.

Worst |got - ref| / (eps A_row), the restatement's figure -> measured on MI355X (K):
    small  value 4.77 -> single 4.62, auto 4.68, pieces 3.95 (128); first derivative 5.53 -> 6.14, 6.14, 3.75 (128)
    sq     value 3.94 -> single 3.70, auto 2.98, pieces 3.30 (64);  first derivative 4.45 -> 3.40, 3.55, 3.55 (128)"""
import functools

import numpy as np
import pytest

import bary_ld as B
from pychebyshev_amd import _lib

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not B.LD_OK, reason="np.longdouble is no wider than float64 here")]

SMALL, SQ, PIECES = B.small_models(), B.sq_models(), B.piece_models()
WORST = {}
_check = functools.partial(B.check, WORST)      # the normwise bar, then every row against its amplitude


def _set_kernel(c, variant):
    """A refusal raises: a failure of the case, not a skip."""
    m = c._model()
    _lib.check(m.lib.pcx_bary_set_kernel(m.handle, variant), m.lib)


def _derived(c, spec):
    """The derived tensor the device contracts, and it is the oracle's bit for bit."""
    if not any(spec):
        return c.tensor_values
    m = c._model()
    got = np.empty(c.tensor_values.shape)
    _lib.check(m.lib.pcx_bary_derivative_tensor(m.handle, _lib.p_i32(_lib.i32(spec)), _lib.p_f64(got)), m.lib)
    assert np.array_equal(got, B.derived_tensor(c, spec)), spec
    return got


def _run_single(model):
    b = B.build(model)
    c, pts, d, fam = b.c, b.pts, len(model.shape), model.family
    value = [0] * d
    _set_kernel(c, B.variant_of(model))
    pair = B.reference(c.nodes, c.weights, c.tensor_values, pts)
    got = c.vectorized_eval_batch(pts, value)
    _check(got, pair, fam, "value", "single", f"{model.name} value")
    assert got[b.grid_row] == c.tensor_values[b.grid_idx], f"{model.name}: the grid-point row is not the tensor entry"
    # one launch for all specs: the T_tab branch with m > 1 (m = 1 where no dimension has two nodes)
    specs = B.specs_of(model.shape)
    multi = c.vectorized_eval_multi_batch(pts, specs)
    assert multi.shape == (model.rows, len(specs))
    assert np.array_equal(multi[:, 0], got), f"{model.name}: column 0 of the multi-spec launch"
    pairs = [pair]
    for j, spec in enumerate(specs[1:], start=1):
        pairs.append(B.reference(c.nodes, c.weights, _derived(c, spec), pts))
        _check(multi[:, j], pairs[j], fam, "order1", "single", f"{model.name} {spec}")
    # whatever auto picks on the same handle
    _set_kernel(c, 0)
    _check(c.vectorized_eval_batch(pts, value), pair, fam, "value", "auto", f"{model.name} value, auto")
    auto = c.vectorized_eval_multi_batch(pts, specs)
    for j, spec in enumerate(specs):
        _check(auto[:, j], pairs[j], fam, B.order_of(spec), "auto", f"{model.name} {spec}, auto")


@pytest.mark.parametrize("model", SMALL, ids=[m.name for m in SMALL])
def test_small_bodies(model):
    """k_bary_small<d - 1, NLP>: the EXACT branch at n = NLP, the padded one at every other n."""
    _run_single(model)


@pytest.mark.parametrize("model", SQ, ids=[m.name for m in SQ])
def test_sq_bodies(model):
    """k_bary_sq<NL, d - 2>."""
    _run_single(model)


def _set_pieces(sp, variant):
    for piece in sp._pieces:                    # the spline handle holds the pieces' own handles
        _set_kernel(piece, variant)


def _piece_pairs(b, specs):
    return [B.spline_reference(b.sp, [_derived(p, spec) for p in b.sp._pieces], b.pts, b.ids) for spec in specs]


@pytest.mark.parametrize("i", range(len(PIECES)), ids=[m.name for m in PIECES])
def test_piece_bodies(i, monkeypatch):
    """k_bary_small_pieces / k_bary_sq_pieces: every row on its own piece, routed by the searchsorted rule; for every
    eighth model a launch per piece (PCX_SPLINE_FUSED=0) gives the same bits."""
    model = PIECES[i]
    b = B.build_spline(model)
    sp, pts, fam = b.sp, b.pts, model.family
    _set_pieces(sp, B.variant_of(model))
    assert np.array_equal(sp.piece_indices(pts), b.ids), f"{model.name}: routing"
    specs = B.piece_specs_of(model.shape)
    pairs = _piece_pairs(b, specs)
    got = sp.eval_batch(pts, specs[0])
    _check(got, pairs[0], fam, "value", "pieces", f"{model.name} value")
    for row, p, idx in b.grid_rows:
        assert got[row] == sp._pieces[p].tensor_values[idx], f"{model.name}: grid-point row {row} of piece {p}"
    multi = sp.eval_multi_batch(pts, specs)
    assert multi.shape == (model.rows, 2)
    assert np.array_equal(multi[:, 0], got), f"{model.name}: column 0 of the two-spec launch"
    _check(multi[:, 1], pairs[1], fam, B.order_of(specs[1]), "pieces", f"{model.name} {specs[1]}")
    if i % 8 == 0:
        monkeypatch.setenv("PCX_SPLINE_FUSED", "0")
        sp.to_device(sp._dev().device)          # a second spline handle, created under the override, on the same piece handles
        assert np.array_equal(sp.eval_batch(pts, specs[0]), got), f"{model.name}: launch per piece, value"
        assert np.array_equal(sp.eval_multi_batch(pts, specs), multi), f"{model.name}: launch per piece, two specs"


@pytest.mark.parametrize("model", B.bucket_models(), ids=[m.name for m in B.bucket_models()])
def test_bucket_edges(model):
    """Six pieces along dimension 0 whose buckets hold 0, 1, 63, 64, 65 and 129 rows, in shuffled order: blk_first,
    piece_end and the `valid` test of the piece kernels at their edges.  Every row within bounds, and equal to the same
    row evaluated one piece at a time (through the spline, and on the piece's own handle)."""
    b = B.build_spline(model, B.BUCKETS)
    sp, pts, fam = b.sp, b.pts, model.family
    _set_pieces(sp, B.variant_of(model))
    assert np.array_equal(sp.piece_indices(pts), b.ids)
    assert sorted(np.bincount(b.ids, minlength=6).tolist()) == sorted(B.BUCKETS)
    specs = B.piece_specs_of(model.shape)
    pairs = _piece_pairs(b, specs)
    got = sp.eval_batch(pts, specs[0])
    multi = sp.eval_multi_batch(pts, specs)
    _check(got, pairs[0], fam, "value", "pieces", f"{model.name} value")
    _check(multi[:, 1], pairs[1], fam, "order1", "pieces", f"{model.name} {specs[1]}")
    assert np.array_equal(multi[:, 0], got)
    for p in np.unique(b.ids):
        rows = np.nonzero(b.ids == p)[0]
        sub = np.ascontiguousarray(pts[rows])
        assert np.array_equal(sp.eval_batch(sub, specs[0]), got[rows]), f"{model.name}: piece {p} alone"
        assert np.array_equal(sp.eval_multi_batch(sub, specs), multi[rows]), f"{model.name}: piece {p} alone, two specs"
        assert np.array_equal(sp._pieces[int(p)].vectorized_eval_batch(sub, specs[0]), got[rows]), f"{model.name}: piece {p}'s own handle"


@pytest.mark.parametrize("model", B.tail_models(), ids=[m.name for m in B.tail_models()])
def test_batch_tails(model):
    """N = 1, 63, 64, 65, 127, 128, 129 against the leading rows of the 130-row call, bit for bit: a lane past the batch
    computes on a node and stores nothing."""
    b = B.build(model)
    c, fam = b.c, model.family
    _set_kernel(c, B.variant_of(model))
    specs = B.specs_of(model.shape)
    full = c.vectorized_eval_batch(b.pts, specs[0])
    full_multi = c.vectorized_eval_multi_batch(b.pts, specs)
    _check(full, B.reference(c.nodes, c.weights, c.tensor_values, b.pts), fam, "value", "single", f"{model.name} value")
    for j, spec in enumerate(specs[1:], start=1):
        _check(full_multi[:, j], B.reference(c.nodes, c.weights, _derived(c, spec), b.pts), fam, "order1", "single", f"{model.name} {spec}")
    for N in B.TAIL_NS:
        pts = np.ascontiguousarray(b.pts[:N])
        assert np.array_equal(c.vectorized_eval_batch(pts, specs[0]), full[:N]), f"{model.name} N = {N}"
        assert np.array_equal(c.vectorized_eval_multi_batch(pts, specs), full_multi[:N]), f"{model.name} N = {N}, {len(specs)} specs"


def test_worst_rows_stay_in_the_restatements_range():
    """Runs last: the worst row per (family, spec order, single / auto / pieces) over the cases that ran in this session,
    next to the restatement's figure (the numbers DESIGN.md section 5 quotes)."""
    for key in sorted(WORST):
        family, order, _ = key.split(" ")
        print(f"{key}: worst {WORST[key]:.3f} eps A_row, restatement {B.RESTATEMENT_WORST[family][order]:.3f}, K {B.K[family][order]}")
        assert WORST[key] <= B.K[family][order]
