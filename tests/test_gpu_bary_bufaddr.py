"""The pipelined tile loop of k_bary_mfma (12 k-steps or more): buffer-resource loads and the deferred hand-over.

Loads: fragments, row codes / offsets and seeds go through buffer resources -- per table a window from the tile being
read to the table's end, rebased per tile with scalar arithmetic, the lane's part of the address a loop-invariant offset.
Hand-over (narrow plans of at most 64 B-operand doubles per lane): two accumulator sets alternate per tile, the seed of
tile t+1 is formed into the idle set, and tile t's epilogue -- its cs FMAs, the chunk-end fold, the split store -- runs at
k-step 1 of tile t+1; one flush behind the loop finishes the last tile.

Same loads, same arithmetic, same order: every result below is compared BIT FOR BIT with the same model on k_bary_mfma4
(variant 3), which keeps its pointer loads and its one accumulator set and is specified as bit-identical; plans that
variant 3 does not run (wide codes, more than 32 k-steps) and dim-0 group launches are compared with the CPU oracle.
Shapes are the smallest that take the paths in question; each plan is asserted through pcx_bary_kernel_info (row tiles,
k-steps, head dimensions) so that a planner change cannot empty a case silently.

Row-tile counts 1, 2, 4 and 5: the prefetch of "the next tile" re-reads the only one and nothing but the flush finishes
it; one hand-over; exactly a chunk of four; a chunk plus one (an odd count: the flush reads the other set).  Batches 1,
31, 33, 129 and 1,000 run one column tile per wave and split the chunks over grid.y (deferred split stores); 66,000 runs
two column tiles per wave.
"""
import numpy as np
import pytest

from conftest import assert_parity, golden, spec_point_tol
import functions as F

from pychebyshev_amd import ChebyshevApproximation, ChebyshevSpline, _lib

pytestmark = pytest.mark.gpu

SMALL_BATCHES = (1, 31, 33, 129, 1000)
BIG = 66_000


def _info(c, fn, n):
    m = c._model()
    info = _lib.i32(np.zeros(n))
    _lib.check(getattr(m.lib, fn)(m.handle, _lib.p_i32(info)), m.lib)
    return [int(v) for v in info]


def _set_kernel(c, variant):
    m = c._model()
    _lib.check(m.lib.pcx_bary_set_kernel(m.handle, variant), m.lib)


def _row_code_model(monkeypatch, T, dom, tail=1):
    """The model on the row-code MFMA form (the short-plan forms switched off at create)."""
    monkeypatch.setenv("PCX_BARY_GRID", "0")
    monkeypatch.setenv("PCX_BARY_KFOLD", "0")
    monkeypatch.setenv("PCX_BARY_TAIL", str(tail))
    c = ChebyshevApproximation.from_values(T, T.ndim, dom, list(T.shape))
    _set_kernel(c, 2)              # creates the handle: the environment is read here
    assert _info(c, "pcx_bary_grid_info", 4)[0] == 0
    return c


def _dom(d):
    return [[-1.0, 1.0], [0.0, 2.0], [2.0, 5.0], [-3.0, -1.0], [0.5, 1.5], [-2.0, 0.0], [1.0, 3.0]][:d]


def _points(c, dom, n, seed):
    rng = np.random.default_rng(seed)
    pts = np.column_stack([rng.uniform(lo, hi, n) for lo, hi in dom])
    d = len(dom)
    for r in range(6):             # exact nodes at both ends of the batch; rows 0 and 1 are the first and the last node
        idx = [0] * d if r == 0 else [len(c.nodes[k]) - 1 for k in range(d)] if r == 1 else \
              [int(rng.integers(0, len(c.nodes[k]))) for k in range(d)]
        pts[r] = [c.nodes[k][i] for k, i in enumerate(idx)]
        pts[n - 1 - r] = pts[r]
    return pts


def _mixed(d):
    return [1] + [0] * (d - 2) + [1]


# shape, row tiles, k-steps, head dimensions (NF: at most two read two fields), seed columns R
PLANS = [
    ((4, 4, 7, 7), 1, 12, 2, 1),            # one tile: the next tile's prefetch re-reads it
    ((4, 8, 7, 7), 2, 12, 2, 1),            # one hand-over
    ((8, 8, 7, 7), 4, 12, 2, 1),            # exactly a chunk
    ((8, 10, 7, 7), 5, 12, 2, 1),           # a chunk plus one
    ((5, 5, 8, 6), 2, 12, 2, 0),            # no seed; 25 rows: the last tile is ragged
    ((6, 6, 5, 10), 3, 12, 2, 2),           # two seed columns
    ((9,) * 4, 6, 20, 2, 1),
    ((7,) * 5, 22, 12, 3, 1),               # three head dimensions: both offset words
    ((3, 3, 3, 4, 5, 10), 7, 12, 4, 2),     # four head dimensions, two seed columns
]


def _seed_columns(shape, split):
    K = int(np.prod(shape[split:]))
    return K % 4 if K > 4 and K % 4 in (1, 2) else 0


@pytest.mark.parametrize("shape,mt,ks,split,r", PLANS)
def test_pipelined_loop_matches_the_4x4x4_form(monkeypatch, shape, mt, ks, split, r):
    d = len(shape)
    rng = np.random.default_rng(700 + sum(shape) + d)
    T = rng.standard_normal(shape)
    dom = _dom(d)
    c = _row_code_model(monkeypatch, T, dom)
    kinfo = _info(c, "pcx_bary_kernel_info", 6)
    assert (kinfo[1], kinfo[2], kinfo[5]) == (mt, ks, split) and ks >= 12, f"{shape}: plan {kinfo}"
    assert _seed_columns(shape, split) == r
    pts = _points(c, dom, BIG, 13 + d)
    specs = [[0] * d, _mixed(d)]
    big = {}
    for variant in (2, 3):
        _set_kernel(c, variant)
        for s in specs:
            big[variant, tuple(s)] = c.vectorized_eval_batch(pts, s)
        big[variant, "multi"] = c.vectorized_eval_multi_batch(pts[:1000], specs)        # grid.z = 2: one resource per z
    _set_kernel(c, 2)
    for s in specs:
        y = big[2, tuple(s)]
        assert np.isfinite(y).all()
        assert np.array_equal(y, big[3, tuple(s)]), f"{shape} {s} N={BIG}: the two MFMA forms differ"
        assert np.array_equal(y[BIG - 6:], y[:6][::-1])            # the same nodes at both ends of the batch
        for n in SMALL_BATCHES:
            assert np.array_equal(c.vectorized_eval_batch(pts[:n], s), y[:n]), \
                f"{shape} {s} N={n}: differs from the same rows of the large batch"
    assert np.array_equal(big[2, "multi"], big[3, "multi"]), f"{shape}: multi-spec launch, the two MFMA forms differ"
    for j, s in enumerate(specs):
        assert np.array_equal(big[2, "multi"][:, j], big[2, tuple(s)][:1000]), f"{shape}: multi-spec column {s}"
    y = big[2, tuple(specs[0])]                                     # grid points return the tensor entry exactly
    assert y[0] == T[(0,) * d] and y[1] == T[tuple(n - 1 for n in shape)]


@pytest.mark.parametrize("shape,nchunks", [((7,) * 5, 6), ((8, 10, 7, 7), 2)])
def test_tail_pieces_meet_the_pipelined_loop(monkeypatch, shape, nchunks):
    """One batch just over `slots` workgroups: under PCX_BARY_TAIL=2 its last block is walked in pieces (split stores
    from inside the pipelined loop, k_bary_reduce finishes), under =0 by one workgroup; both against variant 3."""
    d = len(shape)
    rng = np.random.default_rng(900 + sum(shape))
    T = rng.standard_normal(shape)
    dom = _dom(d)
    c2 = _row_code_model(monkeypatch, T, dom, 2)
    c0 = _row_code_model(monkeypatch, T, dom, 0)
    ti = _info(c2, "pcx_bary_tail_info", 6)
    slots, per_wg = ti[0], ti[1]
    assert 1 <= slots <= 512 and per_wg == 128 and ti[2] == nchunks and ti[3] == 2, ti
    n = slots * per_wg + 128 + 5                                    # two tail blocks, the last one ragged
    pts = _points(c2, dom, n, 21 + d)
    spec = [0] * d
    y2 = c2.vectorized_eval_batch(pts, spec)
    got = _info(c2, "pcx_bary_tail_info", 6)
    assert got[4] == nchunks and got[5] == 2, f"{shape}: launch geometry {got}"
    y0 = c0.vectorized_eval_batch(pts, spec)
    assert _info(c0, "pcx_bary_tail_info", 6)[4] == 0
    _set_kernel(c0, 3)
    y3 = c0.vectorized_eval_batch(pts, spec)
    assert np.array_equal(y2, y3), f"{shape}: tail pieces differ from the 4x4x4 form"
    assert np.array_equal(y0, y3), f"{shape}: one workgroup per block differs from the 4x4x4 form"
    assert np.array_equal(c2.vectorized_eval_batch(pts[:1000], spec), y2[:1000])


# shape, row tiles, k-steps, head dimensions
ORACLE_PLANS = [
    ((2, 2, 2, 2, 3, 9, 9), 3, 20, 5),      # five head dimensions: row codes with a second word (WIDE)
    ((4, 8, 12, 12), 2, 36, 2),             # 36 k-steps: two column tiles per wave keep the one-set hand-over, one takes two sets
]


@pytest.mark.parametrize("shape,mt,ks,split", ORACLE_PLANS)
def test_plans_without_a_4x4x4_form_match_the_oracle(oracle_mod, monkeypatch, shape, mt, ks, split):
    d = len(shape)
    rng = np.random.default_rng(sum(shape))
    T = rng.standard_normal(shape)
    dom = _dom(d)
    c = _row_code_model(monkeypatch, T, dom)
    kinfo = _info(c, "pcx_bary_kernel_info", 6)
    assert (kinfo[1], kinfo[2], kinfo[5]) == (mt, ks, split), kinfo
    m = c._model()
    assert m.lib.pcx_bary_set_kernel(m.handle, 3) != 0
    pts = _points(c, dom, BIG, 5)
    om = oracle_mod.BaryModel(c.nodes, c.weights, c.diff_matrices, c.tensor_values)
    sub = np.r_[0:300, BIG - 300:BIG]
    for s in ([0] * d, _mixed(d)):
        y = c.vectorized_eval_batch(pts, s)
        assert_parity(y[sub], oracle_mod.bary_eval_batch(om, pts[sub], s), 1e-12, f"bufaddr {shape} {s}", spec_point_tol(s),
                      floor=float(np.max(np.abs(T))))
        for n in SMALL_BATCHES:
            assert np.array_equal(c.vectorized_eval_batch(pts[:n], s), y[:n]), f"{shape} {s} N={n}"


def test_dim0_group_launch_matches_the_oracle(oracle_mod):
    """Price + delta of the 11^5 model in one two-spec call at a batch large enough for a dim-0 group: the slab-packed
    image, its seed array and the group's row codes, each through its own resource."""
    T = golden("g2_bs5d")["tensor"]
    c = ChebyshevApproximation.from_values(T, 5, F.BS5_DOMAIN, F.BS5_NODES)
    m = c._model()
    assert _info(c, "pcx_bary_kernel_info", 6)[1:3] == [84, 30]
    n = 66_480
    pts = F.bs5_query_points(n, seed=31)
    specs = [[0, 0, 0, 0, 0], [1, 0, 0, 0, 0]]
    gem = _lib.i32(np.zeros(1))
    _lib.check(m.lib.pcx_bary_count_gemms(m.handle, _lib.p_i32(_lib.i32(np.asarray(specs).ravel())), 2, n, _lib.p_i32(gem)), m.lib)
    assert int(gem[0]) == 1, "the call formed no dim-0 group"
    got = c.vectorized_eval_multi_batch(pts, specs)
    om = oracle_mod.BaryModel(c.nodes, c.weights, c.diff_matrices, c.tensor_values)
    sub = np.r_[0:300, n - 300:n]
    for j, s in enumerate(specs):
        assert_parity(got[sub, j], oracle_mod.bary_eval_batch(om, pts[sub], s), 1e-12, f"bufaddr g0 {s}", spec_point_tol(s))


def test_spline_buckets_match_the_4x4x4_form(monkeypatch):
    """Two (8, 10, 7, 7) pieces: each bucket's launch covers the rows perm names."""
    shape = (8, 10, 7, 7)
    dom = _dom(4)
    knots = [[0.25], [], [], []]
    rng = np.random.default_rng(41)
    vals = [rng.standard_normal(shape) for _ in range(2)]
    n = 3001
    pts = np.column_stack([rng.uniform(lo, hi, n) for lo, hi in dom])
    res = {}
    for variant in (2, 3):
        monkeypatch.setenv("PCX_BARY_GRID", "0")
        monkeypatch.setenv("PCX_BARY_KFOLD", "0")
        sp = ChebyshevSpline.from_values(vals, 4, dom, list(shape), knots)
        for piece in sp._pieces:
            assert _info(piece, "pcx_bary_kernel_info", 6)[1:3] == [5, 12]
            _set_kernel(piece, variant)
        res[variant] = sp.eval_batch(pts, [0] * 4)
    assert np.isfinite(res[2]).all() and np.array_equal(res[2], res[3])
