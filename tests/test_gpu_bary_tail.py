"""The last round of a large k_bary_mfma launch inside the same launch, and the row offsets of its pipelined loop.

Tail split: a launch of more workgroups than the device holds at once (`slots`, pcx_bary_tail_info) whose last round is
at most half full walks every point block of that round with P workgroups, each a contiguous range of row-tile chunks,
and k_bary_reduce adds the chunk sums -- the additions of a small-batch split launch in the same order.  Every result
below is compared BIT FOR BIT with a handle created under PCX_BARY_TAIL=0, which keeps one workgroup per point block;
the geometry each launch took is read back from pcx_bary_tail_info.  By default the split is taken only where a
workgroup's row-tile walk is long enough to pay for the finishing kernel (the 11^5 headline model: tested on the
default handle); the small tensors here are split under PCX_BARY_TAIL=2, which takes it wherever the geometry allows.

Row offsets: the pipelined loop (12 k-steps or more, narrow codes) reads its head-weight rows through pre-scaled 16-bit
LDS offsets and prologue 2 reads only the live fields of a two-dimensional tail; k_bary_mfma4 (variant 3) keeps the
8-bit row codes and four-field k codes and is specified as bit-identical to k_bary_mfma.

4^6 as a shape plans a TWO-dimensional head (K = 4^4 = 256 in 64 k-steps is priced below M = 256 rows of K = 16), which
variant 3 does not cover: it is compared with the oracle, and (4, 4, 4, 17, 4, 4) -- a tail of 16 columns, the next
fold being 272 > 256 -- supplies the four-dimensional head (NF = 4) against variant 3.
"""
import numpy as np
import pytest

from conftest import assert_parity, golden
import functions as F

from pychebyshev_amd import ChebyshevApproximation, ChebyshevSpline, _lib

pytestmark = pytest.mark.gpu


def _info(c, fn, n):
    m = c._model()
    info = _lib.i32(np.zeros(n))
    _lib.check(getattr(m.lib, fn)(m.handle, _lib.p_i32(info)), m.lib)
    return [int(v) for v in info]


def _tail_info(c):
    return _info(c, "pcx_bary_tail_info", 6)


def _row_code_model(monkeypatch, T, dom, tail=2, variant=2):
    """The model on the row-code MFMA form (the short-plan forms switched off at create); tail: PCX_BARY_TAIL (0 never
    splits, 1 the default rule, 2 wherever the geometry allows)."""
    monkeypatch.setenv("PCX_BARY_GRID", "0")
    monkeypatch.setenv("PCX_BARY_KFOLD", "0")
    monkeypatch.setenv("PCX_BARY_TAIL", str(tail))
    c = ChebyshevApproximation.from_values(T, T.ndim, dom, list(T.shape))
    m = c._model()                 # creates the handle: the environment is read here
    _lib.check(m.lib.pcx_bary_set_kernel(m.handle, variant), m.lib)
    assert _info(c, "pcx_bary_grid_info", 4)[0] == 0
    return c


def _points(c, dom, n, seed):
    rng = np.random.default_rng(seed)
    pts = np.column_stack([rng.uniform(lo, hi, n) for lo, hi in dom])
    d = len(dom)
    for r in range(6):             # a few exact nodes, at both ends of the batch (the far end lies in the tail blocks)
        idx = [int(rng.integers(0, len(c.nodes[k]))) for k in range(d)]
        pts[r] = [c.nodes[k][i] for k, i in enumerate(idx)]
        pts[n - 1 - r] = pts[r]
    return pts


def _dom(d):
    return [[-1.0, 1.0], [0.0, 2.0], [2.0, 5.0], [-3.0, -1.0], [0.5, 1.5], [-2.0, 0.0]][:d]


# shape, k-steps, row tiles, chunks
TAIL_CASES = [
    ((7,) * 5, 12, 22, 6),         # R = 1, the shortest pipelined loop; the last chunk is partial
    ((9,) * 4, 20, 6, 2),
    ((5,) * 4, 6, 2, 1),           # a single chunk: nothing to split, the launch must decline
]


def _expected_P(blocks, slots, nchunks):
    tail = blocks % slots
    if blocks <= slots or tail == 0 or 2 * tail > slots or nchunks < 2:
        return 0
    P = min(nchunks, slots // tail)
    cpp = -(-nchunks // P)
    P = -(-nchunks // cpp)
    return P if P > 1 else 0


@pytest.mark.parametrize("shape,ks,mt,nchunks", TAIL_CASES)
def test_tail_split_matches_the_one_workgroup_per_block_geometry(monkeypatch, shape, ks, mt, nchunks):
    d = len(shape)
    rng = np.random.default_rng(300 + sum(shape) + d)
    T = rng.standard_normal(shape)
    dom = _dom(d)
    c = _row_code_model(monkeypatch, T, dom, 2)
    c0 = _row_code_model(monkeypatch, T, dom, 0)
    kinfo = _info(c, "pcx_bary_kernel_info", 6)
    assert (kinfo[1], kinfo[2]) == (mt, ks), f"{shape}: plan {kinfo}"
    ti, ti0 = _tail_info(c), _tail_info(c0)
    slots, per_wg = ti[0], ti[1]
    assert 1 <= slots <= 512 and per_wg == 128 and ti[2] == nchunks and ti[3] == 2, ti
    assert ti0[:4] == [slots, per_wg, nchunks, 0], ti0
    S = slots * per_wg
    batches = [S + 128, S + 133 * 128 - 37, S + S // 2, 2 * S - 3 * 128, 3 * S + 17]
    pts = _points(c, dom, max(batches), 7 + d)
    spec = [0] * d
    mixed = [1] + [0] * (d - 2) + [1]
    small = c.vectorized_eval_batch(pts[:1000], spec)          # one column tile per wave, split over grid.y
    for n in batches:
        blocks = -(-n // per_wg)
        want_P = _expected_P(blocks, slots, nchunks)
        if n == 2 * S - 3 * 128:
            assert want_P == 0                                   # the tail is too full
        elif nchunks > 1:
            assert want_P > 1
        p = pts[:n].copy()
        p[n - 6:] = pts[:6]                                      # exact nodes in the ragged end of every batch
        y = c.vectorized_eval_batch(p, spec)
        got = _tail_info(c)
        assert (got[4], got[5]) == (want_P, blocks % slots if want_P else 0), f"{shape} N={n}: launch geometry {got}"
        y0 = c0.vectorized_eval_batch(p, spec)
        assert _tail_info(c0)[4] == 0
        assert np.array_equal(y, y0), f"{shape} N={n}: the tail split changes bits"
        assert np.array_equal(y[:1000], small), f"{shape} N={n}: the first 1,000 points differ from the small batch"
        assert np.array_equal(y[n - 6:], y[:6])                  # the same nodes in a whole block and in a tail block
    for r in range(6):                                           # grid points return the tensor entry exactly
        idx = tuple(int(np.argmin(np.abs(np.asarray(c.nodes[k]) - pts[r, k]))) for k in range(d))
        assert small[r] == T[idx]
    # a derivative spec and a multi-spec call (grid.z = 2 keeps one workgroup per block) at a batch the value spec splits
    n = batches[1]
    ym = c.vectorized_eval_batch(pts[:n], mixed)
    assert np.array_equal(ym, c0.vectorized_eval_batch(pts[:n], mixed))
    multi = c.vectorized_eval_multi_batch(pts[:n], [spec, mixed])
    assert np.array_equal(multi, c0.vectorized_eval_multi_batch(pts[:n], [spec, mixed]))
    assert np.array_equal(multi[:, 0], c.vectorized_eval_batch(pts[:n], spec)) and np.array_equal(multi[:, 1], ym)


def test_tail_split_of_a_spline_bucket(monkeypatch):
    """Two 7^5 pieces; the first one's bucket exceeds `slots` workgroups with a last round a quarter full: the launch
    goes through perm (the bucket's rows of the batch) and splits."""
    shape = (7,) * 5
    dom = _dom(5)
    knots = [[0.25], [], [], [], []]
    rng = np.random.default_rng(77)
    vals = [rng.standard_normal(shape) for _ in range(2)]
    res = {}
    for tail_on in (True, False):
        monkeypatch.setenv("PCX_BARY_GRID", "0")
        monkeypatch.setenv("PCX_BARY_KFOLD", "0")
        monkeypatch.setenv("PCX_BARY_TAIL", "2" if tail_on else "0")
        sp = ChebyshevSpline.from_values(vals, 5, dom, list(shape), knots)
        for piece in sp._pieces:
            m = piece._model()
            _lib.check(m.lib.pcx_bary_set_kernel(m.handle, 2), m.lib)
        ti = _tail_info(sp._pieces[0])
        S = ti[0] * ti[1]
        n0, n1 = S + 133 * 128 - 37, 5000
        if tail_on:
            pts = np.column_stack([rng.uniform(lo, hi, n0 + n1) for lo, hi in dom])
            pts[:, 0] = np.r_[rng.uniform(-1.0, 0.2, n0), rng.uniform(0.3, 1.0, n1)]
            pts = pts[rng.permutation(n0 + n1)]
        res[tail_on] = sp.eval_batch(pts, [0] * 5)
        got = _tail_info(sp._pieces[0])
        assert (got[4], got[5]) == ((_expected_P(-(-n0 // 128), ti[0], 6), 133) if tail_on else (0, 0)), got
    assert np.array_equal(res[True], res[False])
    left = pts[:, 0] < 0.25
    piece0 = _row_code_model(monkeypatch, vals[0], [[-1.0, 0.25]] + dom[1:], 2)
    assert np.array_equal(res[True][left][:1000], piece0.vectorized_eval_batch(pts[left][:1000], [0] * 5))


def test_default_handle_splits_the_headline_model_and_not_a_short_walk(monkeypatch):
    """The default rule (PCX_BARY_TAIL unset): 11^5 (84 row tiles of 30 k-steps) splits its ragged last round, 9^4
    (6 tiles of 20) keeps one workgroup per block; both give the bits of a PCX_BARY_TAIL=0 handle."""
    monkeypatch.delenv("PCX_BARY_TAIL", raising=False)
    T = golden("g2_bs5d")["tensor"]
    c = ChebyshevApproximation.from_values(T, 5, F.BS5_DOMAIN, F.BS5_NODES)
    ti = _tail_info(c)
    assert ti[2:4] == [21, 1], ti
    n = ti[0] * ti[1] + 133 * 128 - 37
    pts = F.bs5_query_points(n, seed=29)
    y = c.vectorized_eval_batch(pts, [0] * 5)
    got = _tail_info(c)
    assert (got[4], got[5]) == (_expected_P(-(-n // 128), ti[0], 21), 133) and got[4] > 1, got
    c0 = _row_code_model(monkeypatch, T, F.BS5_DOMAIN, 0)
    assert np.array_equal(y, c0.vectorized_eval_batch(pts, [0] * 5))
    assert np.array_equal(y[:1000], c.vectorized_eval_batch(pts[:1000], [0] * 5))
    monkeypatch.delenv("PCX_BARY_TAIL", raising=False)
    rng = np.random.default_rng(94)
    T4 = rng.standard_normal((9,) * 4)
    monkeypatch.setenv("PCX_BARY_GRID", "0")
    c4 = ChebyshevApproximation.from_values(T4, 4, _dom(4), [9] * 4)
    m4 = c4._model()
    _lib.check(m4.lib.pcx_bary_set_kernel(m4.handle, 2), m4.lib)
    p4 = _points(c4, _dom(4), n, 5)
    y4 = c4.vectorized_eval_batch(p4, [0] * 4)
    assert _tail_info(c4)[3:5] == [1, 0], _tail_info(c4)
    assert np.array_equal(y4, _row_code_model(monkeypatch, T4, _dom(4), 2).vectorized_eval_batch(p4, [0] * 4))


# shape, live row-code fields (head dimensions)
OFFSET_CASES = [
    ((7,) * 5, 3),
    ((9,) * 4, 2),
    ((4, 4, 4, 17, 4, 4), 4),
    ((4,) * 6, 2),                 # two-dimensional head, 64 k-steps: no variant 3, compared with the oracle
]


@pytest.mark.parametrize("shape,nf", OFFSET_CASES)
def test_default_kernel_matches_the_row_code_4x4x4_form(oracle_mod, monkeypatch, shape, nf):
    d = len(shape)
    rng = np.random.default_rng(500 + sum(shape) + d)
    T = rng.standard_normal(shape)
    dom = _dom(d)
    c = _row_code_model(monkeypatch, T, dom, 1)
    assert _info(c, "pcx_bary_kernel_info", 6)[5] == nf
    m = c._model()
    pts = _points(c, dom, 66_000, 11 + d)
    have3 = m.lib.pcx_bary_set_kernel(m.handle, 3) == 0
    assert have3 == (shape != (4,) * 6)
    for n in (66_000, 4_096):      # two column tiles per wave; one
        p = pts[:n]
        for spec in ([0] * d, [1] + [0] * (d - 2) + [1]):
            _lib.check(m.lib.pcx_bary_set_kernel(m.handle, 2), m.lib)
            y = c.vectorized_eval_batch(p, spec)
            assert np.isfinite(y).all()
            if have3:
                _lib.check(m.lib.pcx_bary_set_kernel(m.handle, 3), m.lib)
                assert np.array_equal(c.vectorized_eval_batch(p, spec), y), f"{shape} {spec} N={n}: the two MFMA forms differ"
            else:
                om = oracle_mod.BaryModel(c.nodes, c.weights, c.diff_matrices, c.tensor_values)
                sub = np.r_[0:300, n - 300:n]
                assert_parity(y[sub], oracle_mod.bary_eval_batch(om, p[sub], spec), 1e-12, f"tail {shape} {spec}",
                              1e-12 * 10.0 ** sum(spec), floor=float(np.max(np.abs(T))))


def test_wide_plan_keeps_its_row_codes_and_matches_the_oracle(oracle_mod, monkeypatch):
    shape = (3,) * 10
    rng = np.random.default_rng(sum(shape))
    T = rng.standard_normal(shape)
    dom = [[-1.0, 1.0]] * 10
    c = _row_code_model(monkeypatch, T, dom, 1)
    pts = _points(c, dom, 777, 3)
    om = oracle_mod.BaryModel(c.nodes, c.weights, c.diff_matrices, c.tensor_values)
    for spec in ([0] * 10, [1] + [0] * 9, [0] * 9 + [2]):
        assert_parity(c.vectorized_eval_batch(pts, spec), oracle_mod.bary_eval_batch(om, pts, spec), 1e-12,
                      f"wide {spec}", 1e-12 * 10.0 ** sum(spec), floor=float(np.max(np.abs(T))))
