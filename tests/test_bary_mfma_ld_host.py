"""The lists of tests/bary_mfma_ld.py on a CPU: what tests/test_gpu_bary_mfma_bodies.py runs on the device reaches
every body of the three row-code switches of csrc/bary_mfma_launch.h (launch_mfma_nf's KS 1 .. 32 and its long counts,
launch_mfma4) that the planner can reach, the float64 restatement of k_bary_mfma sets K, and the long-double reference
agrees with the C oracle.  No GPU is used.

1. Every list entry plans as the list claims, seeded and under PCX_BARY_SEED=0, by the GPU-free planner
   (tests/host/bary_plan_main.cpp --kfold=0 with the grid switch off): variant 2 offered on the row-code form, split,
   K, MT, KS, R, column tiles, points per workgroup, chunks, variant 3.
2. Coverage.  launch_mfma_nf: all 32 x 4 x 3 short bodies, each R = 0 body three ways (K = 4 KS, K = 4 KS - 1, the
   unseeded handles of the R > 0 shapes; KS = 1 two ways: no plan of four columns or fewer is seeded), every one also on
   a plan of two column tiles; 36 .. 64 in every class and R at
   one column tile, 36 / 40 narrow at two; 42 in the seeded sets.  (42, R = 0) is not instantiated and pick_ks never
   returns it: asserted over every K <= 256.  launch_mfma4: 89 of the 96 (KS, R); the other seven cannot be planned,
   by mfma4_lds_bytes <= 160 KiB: asserted over every ordering of every factorisation of their K (below).
3. The restatement stays within K / 16 of the reference on every model, and K <= 128.
4. On one shape per code class the reference agrees with the oracle's bary_eval_batch to 1e-13 normwise."""
import itertools

import numpy as np
import pytest

import bary_ld as B
import bary_mfma_ld as M

needs_ld = pytest.mark.skipif(not B.LD_OK, reason="np.longdouble is no wider than float64 here")

ROWCODE, TILES, MFMA4 = M.rowcode_models(), M.tile_models(), M.mfma4_models()
# k_bary_mfma4<KS, R> the planner cannot reach: K = 4 KS + R is a prime (one tail dimension of K nodes) or 2 x 61
MFMA4_UNREACHABLE = ((18, 1), (22, 1), (24, 1), (25, 1), (27, 1), (28, 1), (30, 2))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    exe = M.build_planner(tmp_path_factory.mktemp("bary_mfma_plan"))
    if exe is None:
        pytest.skip("hipcc not found")
    return exe


@pytest.fixture(scope="module")
def planned(exe):
    """shape -> (seeded record, PCX_BARY_SEED=0 record) for every list entry."""
    shapes = sorted({m.shape for m in M.all_models()})
    return dict(zip(shapes, zip(M.plan(exe, shapes, True), M.plan(exe, shapes, False))))


def test_the_lists_have_the_sizes_the_search_gave():
    assert len(ROWCODE) == 32 * 4 * 4 + 9 * 4 * 3 - 4 == 616
    assert len(TILES) == 8 * 7 + 4 == 60 and len(MFMA4) == 96 - len(MFMA4_UNREACHABLE) == 89
    names = [m.name for m in M.all_models()]
    assert len(set(names)) == len(names) == 765
    assert all(m.rows == 96 for m in ROWCODE + MFMA4) and all(m.rows == 130 for m in TILES)
    assert max(int(np.prod(m.shape)) for m in M.all_models()) < 50_000


def test_every_model_plans_as_the_list_claims(planned):
    for m in M.all_models():
        on, off = planned[m.shape]
        narrow = m.cls != "wide"
        assert on.ok and off.ok, m.name                                            # variant 2, no grid and no k-fold form
        assert (on.split, on.K, on.MT, on.KS, on.R, on.nt, on.wide, on.mfma4) == (m.split, m.K, m.MT, m.KS, m.R, m.nt, not narrow, m.mfma4), (m, on)
        assert (off.split, off.K, off.MT, off.KS, off.R, off.wide) == (m.split, m.K, m.MT, m.KS0, 0, not narrow), (m, off)
        assert M.class_of(on.split, len(m.shape)) == m.cls and m.R == M.seed_columns(m.K) and m.KS == M.pick_ks(m.K, m.R)
        assert (on.per_wg, on.nchunks) == (64 * m.nt, -(-m.MT // 4)), (m, on)      # pcx_bary_tail_info[1], [2]
        assert on.kernel_info[1:3] == (m.MT, m.KS) and on.kernel_info[4:] == (64 * m.nt, m.split), (m, on)
        if m.R > 0:                                                                # the unseeded handle: R = 0 by zero-padded columns
            assert m.KS0 in (m.KS, m.KS + 1) or m.KS0 > 32, m
            assert 1 <= 4 * m.KS0 - m.K <= 3 or m.KS0 > 32, m
        # what the rule of the variant-3 offer rests on (the unreachable bodies below)
        assert on.mfma4 == (narrow and m.KS <= 32 and M.mfma4_budget(sum(m.shape), m.KS)), m
    for m in ROWCODE:
        M_rows = int(np.prod(m.shape[:m.split]))
        assert M_rows % 16 != 0 and m.MT >= 5, m                                    # a ragged last tile; two chunks or more
        pre = m.shape[:m.split - 1]
        if m.cls == "wide":                                                         # the all-ones prefix, or (1, 1, 1, a) where a long prime K
            assert pre[:3] == (1, 1, 1), m                                              # needs a short n0 to keep two column tiles
        else:
            assert pre.count(1) <= 1, m
        if m.way:
            assert m.R == 0 and m.K == 4 * m.KS - (m.way == "4ks-1"), m


def test_the_lists_reach_every_body_of_launch_mfma_nf():
    short = {(ks, cls, r) for ks in M.KS_SHORT for cls in M.CLASSES for r in range(3)}
    long_ = {(ks, cls, r) for ks in M.KS_LONG for cls in M.CLASSES for r in range(3) if ks != 42 or r > 0}
    assert len(short) == 384 and len(long_) == 104
    assert {m.body for m in ROWCODE} == short | long_
    for ks in M.KS_SHORT:                      # R = 0 three ways: K = 4 KS, K = 4 KS - 1, the unseeded handles
        for cls in M.CLASSES:
            ways = {m.way for m in ROWCODE if m.body == (ks, cls, 0)}
            assert ways == {"4ks", "4ks-1"}, (ks, cls, ways)
            unseeded = [m for m in ROWCODE if m.cls == cls and m.R > 0 and m.KS0 == ks]
            if ks == 1:                        # a seeded plan has K > 4 columns: its unseeded handle runs two k-steps or more
                assert not unseeded and all(M.seed_columns(K) == 0 for K in range(1, 5))
                continue
            assert {4 * ks - m.K for m in unseeded} == {2, 3}, (ks, cls)       # two and three zero-padded columns
    # NT = 2: every model runs the one-column-tile body (40,000 points); those of nt = 2 the other one too (66,313 points)
    nt2 = {m.body for m in ROWCODE if m.nt == 2}
    assert short <= nt2
    assert {(ks, cls, r) for ks in (36, 40) for cls in M.CLASSES[:3] for r in range(3)} == {b for b in nt2 if b[0] > 32}
    assert all(m.nt == 1 for m in ROWCODE if m.KS > 40 or (m.KS > 32 and m.cls == "wide"))      # not instantiated, not planned
    # KS 42 exists in the seeded sets only, and pick_ks gives it to a seeded plan only: every K a plan may fold
    for K in range(1, 257):
        for seed in (True, False):
            R = M.seed_columns(K, seed)
            assert (M.pick_ks(K, R) == 42) == (R > 0 and 161 <= K - R <= 168), (K, seed)       # 41 or 42 whole k-steps
            assert M.pick_ks(K, R) in M.KS_SHORT + M.KS_LONG
    assert {m.K for m in ROWCODE if m.KS == 42} <= {165, 166, 169, 170}


def test_the_tile_list_reaches_the_five_loops_at_every_tile_count():
    by = {}
    for m in TILES[:56]:
        for nt in {1, m.nt}:
            by.setdefault((M.loop_of(m, nt), m.R > 0), set()).add(m.MT)
    for key in (("plain", False), ("plain", True), ("defer", False), ("defer", True), ("nodefer", False), ("wide", False), ("carry", True)):
        assert by[key] == set(M.TILE_MT), (key, by.get(key))
    carry = {(m.cls, nt) for m in TILES[:56] for nt in {1, m.nt} if M.loop_of(m, nt) == "carry"}
    assert carry == {("wide", 1), ("wide", 2), ("nf2", 2)}                      # the carried seed in both loops that have it
    assert all(m.nt == 2 for m in TILES)
    tails = sorted((len(m.shape) - m.split, m.KS >= 12, m.R) for m in TILES[56:])
    assert tails == [(3, False, 0), (3, False, 1), (4, False, 0), (4, True, 2)]
    assert {len(m.shape) - m.split for m in ROWCODE if m.cls != "wide"} >= {1, 2, 3}


def _orderings(K, most):
    return sorted({p for f in M.factorisations(K, most) for p in itertools.permutations(f)})


def test_the_mfma4_list_reaches_every_body_the_planner_can_plan(exe, planned):
    every = {(ks, r) for ks in M.KS_SHORT for r in range(3)}
    assert {(m.KS, m.R) for m in MFMA4} == every - set(MFMA4_UNREACHABLE) and set(MFMA4_UNREACHABLE) < every
    assert all(planned[m.shape][0].mfma4 for m in MFMA4)
    # The rule: variant 3 is offered to narrow plans of KS <= 32 whose mfma4_lds_bytes(sum_n, KS) fits 160 KiB (asserted
    # for every list entry above, and for every shape planned here).  A seeded (KS, R > 0) is K = 4 KS + R exactly.  Every
    # ordering of every factorisation of that K into at most eight tail dimensions of two nodes or more: more than four
    # are a wide plan; of the others none leaves a row for a head or a unit dimension (each adds one to sum_n), so the
    # tensor would be the tail alone -- and where that fits at all (2 x 61) the planner folds one dimension only.
    shapes = []
    for ks, r in MFMA4_UNREACHABLE:
        K = 4 * ks + r
        assert M.seed_columns(K) == r and M.pick_ks(K, r) == ks
        assert [k for k in range(1, 257) if M.seed_columns(k) == r and M.pick_ks(k, r) == ks] == [K]
        for tail in _orderings(K, 8):
            if len(tail) > 4:
                continue
            assert not M.mfma4_budget(sum(tail) + 1, ks), (ks, r, tail)          # no room for one more row
            if M.mfma4_budget(sum(tail), ks):
                shapes.append((ks, r, tail))
    assert sorted(s for _, _, s in shapes) == [(2, 61), (61, 2)]
    for (ks, r, tail), rec in zip(shapes, M.plan(exe, [s for _, _, s in shapes])):
        assert rec.ok and rec.K != 4 * ks + r and (rec.KS, rec.R) != (ks, r), (tail, rec)
        assert rec.mfma4 == (not rec.wide and rec.KS <= 32 and M.mfma4_budget(sum(tail), rec.KS))


@needs_ld
def test_every_kind_of_row_is_where_the_list_says():
    """Corners, a grid point, a row on a node of a tail dimension only, one on a node of a head dimension only, two rows
    2e-15 .. 5e-15 beside a node (tail, head), uniform rows."""
    for m in (ROWCODE[5], ROWCODE[14], ROWCODE[300], ROWCODE[-1], TILES[9], MFMA4[40]):
        b = M.build(m)
        nodes, d, s = b.c.nodes, len(m.shape), m.split
        gap = [np.min(np.abs(b.pts[:, k, None] - nodes[k][None, :]), axis=1) for k in range(d)]
        assert len(b.pts) == m.rows
        assert np.array_equal(b.pts[0], [lo for lo, _ in b.c.domain]) and np.array_equal(b.pts[1], [hi for _, hi in b.c.domain])
        assert all(gap[k][b.grid_row] == 0 for k in range(d))
        assert b.c.tensor_values[b.grid_idx] == M.restatement(nodes, b.c.weights, b.c.tensor_values, b.pts, s)[b.grid_row]
        assert gap[d - 1][3] == 0 and all(gap[k][3] > 1e-9 for k in range(d - 1))
        assert 2e-15 <= gap[d - 1][5] <= 5e-15 and all(gap[k][5] > 1e-9 for k in range(d - 1))
        if any(v >= 2 for v in m.shape[:s]):
            assert sum(gap[k][4] == 0 for k in range(s)) == 1 and all(gap[k][4] > 1e-9 for k in range(s, d))
            assert sum(2e-15 <= gap[k][6] <= 5e-15 for k in range(s)) == 1 and all(gap[k][6] > 1e-9 for k in range(s, d))


@needs_ld
def test_the_restatement_sets_K():
    """The float64 restatement against the long-double reference on every list entry, value and first-derivative specs:
    the worst |y - ref| / (eps A_row) is the figure bary_mfma_ld.RESTATEMENT_WORST records, below 8, and K is 16 times
    it, rounded up to a power of two, <= 128."""
    worst = dict.fromkeys(M.K, 0.0)
    for m in M.all_models():
        for order, r in M.restatement_ratios(m).items():
            assert r <= M.K[order] / 16.0, (m.name, order, r)
            worst[order] = max(worst[order], r)
    print({o: round(r, 4) for o, r in worst.items()}, "K", M.K)
    for order, r in worst.items():
        assert r == pytest.approx(M.RESTATEMENT_WORST[order], rel=5e-3), (order, r)
        k = M.K[order]
        assert r <= 8.0 and k == B.K_of(r) and k / 2 < 16.0 * r <= k <= B.K_CAP == 128, (order, r, k)


@needs_ld
@pytest.mark.parametrize("name", ["ks9-nf2-r1", "ks20-nf3-r2", "ks32-nf4-r0-4ks", "ks32-wide-r2"])
def test_the_reference_agrees_with_the_oracle(oracle_mod, name):
    """bary_eval_batch of the C oracle against the long-double reference, node-rule rows included: 1e-13 normwise."""
    m = next(m for m in ROWCODE if m.name == name)
    b = M.build(m)
    om = oracle_mod.BaryModel(b.c.nodes, b.c.weights, b.c.diff_matrices, b.c.tensor_values)
    for spec in M.specs_of(m.shape):
        ref, _ = B.reference(b.c.nodes, b.c.weights, B.derived_tensor(b.c, spec), b.pts)
        want = oracle_mod.bary_eval_batch(om, b.pts, spec)
        err = float(np.max(np.abs(want.astype(B.LD) - ref)) / np.max(np.abs(ref)))
        print(f"{name} {spec}: oracle against the reference {err:.2e}")
        assert err <= 1e-13, (name, spec, err)
