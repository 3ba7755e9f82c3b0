"""The lists of tests/bary_gk_ld.py on a CPU: what tests/test_gpu_bary_gk_bodies.py runs on the device reaches every
body of launch_grid_nt (csrc/pcx_bary_grid.hip) and launch_kfold_t (csrc/pcx_bary_kfold.hip) that the planner can reach,
the float64 restatements of k_bary_mfma_grid and k_bary_mfma_kfold set K, and the long-double reference agrees with the
C oracle.  No GPU is used.

1. Every list entry plans as the list claims, by the GPU-free planner (tests/host/bary_plan_main.cpp) under the switches
   of the entry's environment (--kfold=0 with the grid switch 2; --kfold-eff=1; --kfold-eff=1 --kfold-straddle=0): form
   and grid_info, kernel_info, nt, WPB, AF, RA, the tile and chunk counts, MT, KS2, STR, the roles, grid_prod.
2. Coverage.  launch_grid_nt: all 128 (KS 1 .. 32, WPB, AF) are reached, 127 of them on a plan of two column tiles, every
   one on a plan of two chunks or more; the run-time paths bary_gk_ld.all_path_props() names are all taken.
   launch_kfold_t: 54 of its 61 (MT, KS2, STR); the other seven are KFOLD_UNREACHABLE below with the rule that excludes
   them, asserted from the planner over every node count of the body, sixteen lengths of the third dimension and the six
   placements.
3. Every kind of row is where the list says it is.
4. The restatements stay within K / 16 of the reference on every model and rule, and K <= 128.
5. On a handful of entries the reference agrees with the oracle's bary_eval_batch to 1e-13 normwise."""
import itertools

import numpy as np
import pytest

import bary_gk_ld as G
import bary_ld as B
import bary_mfma_ld as M

needs_ld = pytest.mark.skipif(not B.LD_OK, reason="np.longdouble is no wider than float64 here")

GRID, KFOLD = G.grid_models(), G.kfold_models()
# launch_grid_nt: every instantiation is reached.
GRID_UNREACHABLE = ()
# launch_kfold_t: (MT, KS2, STR) no plan has.  With MT = 2 (3) row tiles of n0 = 17 .. 32 (33 .. 48) rows and n2 > 40 (56)
# columns the swapped roles -- rows = the n2 dimension in three or four row tiles, b2 = the n0 dimension in 5 .. 12
# operands -- are eligible, pad n0 to a multiple of 4 instead of 16, and their row tiles weigh more (kfold_tile_weight):
# bary_plan_kfold takes them.  KS2 = 13 at two row tiles (n2 = 49 .. 52: 64 rows swapped, 52 columns here) and KS2 <= 10 stay.
KFOLD_UNREACHABLE = {(2, 11, 0): "swapped roles", (2, 12, 0): "swapped roles", (2, 14, 0): "swapped roles", (2, 15, 0): "swapped roles",
                     (2, 16, 0): "swapped roles", (3, 15, 0): "swapped roles", (3, 16, 0): "swapped roles"}
THIRD = (1, 2, 3, 5, 8, 16, 17, 31, 32, 33, 48, 63, 64, 65, 100, 200)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    exe = M.build_planner(tmp_path_factory.mktemp("bary_gk_plan"))
    if exe is None:
        pytest.skip("hipcc not found")
    return exe


@pytest.fixture(scope="module")
def planned(exe):
    """(env, shape) -> the planner's record, for every list entry."""
    out = {}
    for env in G.PLANNER:
        shapes = sorted({m.shape for m in G.all_models() + G.spline_models() if m.env == env})
        out.update({(env, s): p for s, p in zip(shapes, G.plan(exe, shapes, env))})
    return out


def test_the_lists_have_the_sizes_the_search_gave():
    assert len(G.GRID_BODIES) == 128 and len(G.GRID_PATHS) == 63 and len(GRID) == 193
    assert len(G.KFOLD_BODIES) == 54 + 10 and len(G.KFOLD_ROLES) == 16 and len(G.KFOLD_MORE) == 4 and len(G.KFOLD_PADDED) == 19
    assert len(KFOLD) == 105
    names = [m.name for m in G.all_models() + G.spline_models()]
    assert len(set(names)) == len(names) == 302
    assert all(m.rows == 96 for m in G.all_models()) and all(m.rows == sum(B.BUCKETS) for m in G.spline_models())
    assert max(int(np.prod(m.shape)) for m in G.all_models()) <= 210_000 and min(min(m.shape) for m in G.all_models()) >= 2
    for form in ("grid", "kfold"):                 # two domains of unusual width per form
        assert sorted(m.dom for m in G.all_models() if m.form == form and m.dom) == ["narrow", "wide"]
    assert G.DOMAINS["narrow"][1] - G.DOMAINS["narrow"][0] == 2.0 ** -7 and G.DOMAINS["narrow"][0] > 1 and G.DOMAINS["wide"] == (-8.0, 8.0)


def test_every_model_plans_as_the_list_claims(planned, exe):
    for m in G.all_models() + G.spline_models():
        p = planned[(m.env, m.shape)]
        assert p is not None, m.name                                               # variant 2 is offered
        assert (p["kernel_info"], p["grid_info"]) == (m.kernel_info, m.grid_info), (m.name, p)
        assert bool(p["grid_prod"]) == m.grid_prod and p["nt"] == m.nt, (m.name, p)
        if m.form == "grid":
            assert p["grid_ok"] and not p["kfold_ok"] and m.grid_info[0] == 1, m.name
            assert G.grid_body(p) == m.body and G.grid_claim(p) == m.claim, (m.name, p)
            s, (ks, wpb, af) = m.split, m.body
            _, nt, RA, TA, TB, nouter, nchunks, MT, trows = m.claim
            assert (p["gp.nA"], p["gp.nB"], p["plan.K"]) == (m.shape[s - 2], m.shape[s - 1], int(np.prod(m.shape[s:]))), m.name
            assert p["plan.R"] == 0 and ks == M.pick_ks(p["plan.K"]) and 2 <= s <= 4 and 1 <= len(m.shape) - s <= 4 and nouter == s - 2, m.name
            assert (TA, TB) == (-(-p["gp.nA"] // RA), -(-p["gp.nB"] // (16 // RA))) and af == (TB * ks >= 48), m.name
            assert nchunks == int(np.prod(m.shape[:s - 2])) * TA >= 2 and MT == nchunks * TB, m.name
            assert m.grid_info == (1, RA, MT, nchunks) and m.kernel_info[1:] == (MT, ks, wpb * trows * 16 * nt * 8, 64 * nt, s), m.name
        else:
            assert p["kfold_ok"] and not p["grid_ok"] and m.grid_info[0] == 2, m.name
            assert G.kfold_body(p) == m.body and G.kfold_claim(p) == m.claim, (m.name, p)
            (mt, ks2, st), (roles, nt, nbody, P, trows) = m.body, m.claim
            n0, n1, n2 = (m.shape[k] for k in roles)
            assert sorted(roles) == [0, 1, 2] and (p["kf.n0"], p["kf.n1"], p["kf.n2"]) == (n0, n1, n2), m.name
            assert (mt, ks2) == (-(-n0 // 16), -(-n2 // 4)) and n0 <= 64 and n2 <= 64 and mt * ks2 >= 8, m.name
            assert (P, nbody) == ((2 * ks2 - 1, (n1 + 1) // 2) if st else (ks2, n1)) and nbody >= 3, m.name
            assert trows == max(16 * mt, n1 + 1, 4 * ks2) and nt == (1 if 4 * trows * 32 * 8 > 72 * 1024 else 2), m.name
            assert m.grid_info == (2, 0, mt, ks2) and m.kernel_info[1:5] == (mt, nbody * P, 4 * trows * 16 * nt * 8, 64 * nt), m.name
            if st:
                assert n2 == 4 * ks2 - 2 and m.env == "kfold", m.name
    # the weights of a PCX_BARY_GRID_PROD=0 handle: the same plan, grid_prod off
    second = [m for ms in (GRID, KFOLD) for i, m in enumerate(ms) if G.second_handle(i) and m.grid_prod]
    for env in G.PLANNER:
        ms = [m for m in second if m.env == env]
        for m, p in zip(ms, G.plan(exe, [m.shape for m in ms], env, grid_prod=False)):
            assert not p["grid_prod"] and (p["kernel_info"], p["grid_info"]) == (m.kernel_info, m.grid_info), m.name


def test_the_grid_list_reaches_every_body_and_run_time_path(planned):
    bodies = [m for m in GRID if m.name.startswith("grid-ks")]
    assert {m.body for m in bodies} == G.all_grid_bodies() - set(GRID_UNREACHABLE) and len(G.all_grid_bodies()) == 128
    assert [m.body for m in bodies if m.nt != 2] == [(1, 4, 1)]                    # NT = 2: the 65,536 + 777 batch of all but one
    assert all(int(np.prod(m.shape[m.split:])) in (4 * m.body[0] - 3, 4 * m.body[0]) for m in bodies)      # K at an edge of the body
    props = {}
    for m in GRID:
        for prop in G.path_props(m.shape, planned[("grid", m.shape)]):
            props.setdefault(prop, []).append(m)
    assert set(props) >= G.all_path_props() and len(G.all_path_props()) == 2 * (36 + 4 + 6 + 1)
    # a ragged split among the second handles of the device test
    assert sum(G.second_handle(i) and G.ragged_batch(m.body[1], m.claim[6]) is not None for i, m in enumerate(GRID)) >= 10
    for wpb, nchunks, n in ((4, 15, None), (4, 3, None), (1, 7, None)):            # ragged_batch is launch_grid_t's rule
        n = G.ragged_batch(wpb, nchunks)
        blocks, want = -(-n // (16 * wpb)), 2048 // wpb
        nsplit = min(nchunks, -(-want // blocks))
        cps = -(-nchunks // nsplit)
        assert blocks < want and 1 < -(-nchunks // cps) < nchunks and nchunks % cps and n % G.ROWS == 0 and n <= G.BATCH_NT1
    assert G.ragged_batch(4, 2) is None
    # both node-count limits of the division-free weights, and a dimension beyond them
    assert {64, 65} <= {v for m in GRID for v in m.shape}


def test_the_kfold_list_reaches_every_body_the_planner_can_plan(exe):
    every = G.all_kfold_bodies()
    assert len(every) == 61 and set(KFOLD_UNREACHABLE) < every
    assert {m.body for m in KFOLD if m.env == "kfold"} == every - set(KFOLD_UNREACHABLE)
    bodies = [m for m in KFOLD if m.name.startswith("kfold-mt")]
    for key in every - set(KFOLD_UNREACHABLE):
        ms = [m for m in bodies if m.body == key]
        assert len(ms) == (2 if key[2] else 1), key
        if key[2]:                                                                 # straddled: an even and an odd loop dimension
            assert sorted(m.shape[m.claim[0][1]] % 2 for m in ms) == [0, 1], key
        for m in ms:                                                               # node counts at the edges of the body
            n0, n2 = m.shape[m.claim[0][0]], m.shape[m.claim[0][2]]
            assert n0 in (16 * key[0] - 15, 16 * key[0]) + ((4, 8, 12) if key[0] == 1 else ()), m
            assert n2 in ((4 * key[1] - 2,) if key[2] else (4 * key[1] - 3, 4 * key[1])), m
    assert {m.shape[m.claim[0][0]] for m in bodies} >= {16, 17, 32, 33, 48, 49, 64}
    assert {m.shape[m.claim[0][2]] for m in bodies} >= {8, 9, 61 + 3, 57}
    assert {(m.claim[0], m.body[0]) for m in KFOLD} == {(r, mt) for r in G.PERMS for mt in range(1, 5)}     # six role assignments x MT
    loops = {m.shape[m.claim[0][1]]: m for m in KFOLD if m.name.startswith("kfold-loop")}
    assert sorted(loops) == [65, 71, 72, 80] and not any(m.grid_prod for m in loops.values())
    assert [loops[n].nt for n in (65, 71, 72, 80)] == [2, 2, 1, 1]
    padded = [m for m in KFOLD if m.env == "kfold-padded"]
    assert sorted(m.shape for m in padded) == sorted(m.shape for m in bodies if m.body[2] and m.grid_prod) and not any(m.body[2] for m in padded)
    assert [m.name for m in bodies if m.body[2] and not m.grid_prod] == ["kfold-mt1-ks8-str-n1odd"]      # bary_gk_ld.emit: no padded twin
    # the unreachable bodies: every node count of the body, every placement
    for (mt, ks2, st), why in KFOLD_UNREACHABLE.items():
        shapes = sorted({s for n0 in range(16 * mt - 15, 16 * mt + 1) for n2 in range(4 * ks2 - 3, 4 * ks2 + 1) for n1 in THIRD
                         for s in itertools.permutations((n0, n1, n2))})
        seen = 0
        for shape, p in zip(shapes, G.plan(exe, shapes, "kfold")):
            body = G.kfold_body(p)
            assert body != (mt, ks2, st) and body not in KFOLD_UNREACHABLE, (shape, body)
            seen += body is not None
        assert seen > 1000, (mt, ks2, seen)


@needs_ld
def test_every_kind_of_row_is_where_the_list_says():
    """Corners, a grid point, and per role a row on a node of that dimension only, a row 2e-15 .. 5e-15 beside one and a
    row 3e-14 .. 5e-14 beside one; the restatement returns the tensor entry exactly on the grid point."""
    picks = (GRID[3], GRID[77], GRID[127], GRID[150], GRID[-1], GRID[-2], KFOLD[0], KFOLD[30], KFOLD[70], KFOLD[-1], KFOLD[-2])
    for m in picks:
        b = G.build(m)
        nodes, d = b.c.nodes, len(m.shape)
        gap = [np.min(np.abs(b.pts[:, k, None] - nodes[k][None, :]), axis=1) for k in range(d)]
        assert len(b.pts) == m.rows
        assert np.array_equal(b.pts[0], [lo for lo, _ in b.c.domain]) and np.array_equal(b.pts[1], [hi for _, hi in b.c.domain])
        assert all(gap[k][b.grid_row] == 0 for k in range(d))
        assert b.c.tensor_values[b.grid_idx] == G.restatement(m, nodes, b.c.weights, b.c.tensor_values, b.pts)[b.grid_row]
        roles = m.roles
        assert len(roles) == (4 if m.form == "grid" else 3) and (roles[0] is None) == (m.form == "grid" and m.split == 2)
        for r, k in enumerate(roles):
            if k is None:
                continue
            for kind, (lo, hi) in zip(G.KINDS, ((0, 0), (2e-15, 5e-15), (3e-14, 5e-14))):
                row = b.where[(kind, r)]
                assert lo <= gap[k][row] <= hi, (m.name, kind, r)
                assert all(gap[u][row] > 1e-9 for u in range(d) if u != k), (m.name, kind, r)
        assert len(b.where) == 3 * sum(k is not None for k in roles) and max(b.where.values()) < 16
    if any(m.dom for m in picks):
        dom = G.build(GRID[-2]).c.domain
        assert all(tuple(v) == G.DOMAINS["narrow"] for v in dom)


@needs_ld
def test_the_restatements_set_every_K():
    """The float64 restatements against the long-double reference on every list entry, value and first-derivative specs,
    by the plan's weight rule and -- every eighth entry of a form's list, as the device test's second handles -- by
    division: the worst |y - ref| / (eps A_row) is the figure bary_gk_ld.RESTATEMENT_WORST records, at most 8, and K is 16
    times it, rounded up to a power of two, <= 128."""
    worst = {form: {rule: dict.fromkeys(("value", "order1"), 0.0) for rule in ("prod", "div")} for form in ("grid", "kfold")}
    for form, ms in (("grid", GRID), ("kfold", KFOLD)):
        for i, m in enumerate(ms):
            runs = [(G.rule_of(m), None)] + ([("div", False)] if G.second_handle(i) and m.grid_prod else [])
            for rule, prod in runs:
                for order, r in G.restatement_ratios(m, prod).items():
                    assert r <= G.K[form][rule][order] / 16.0, (m.name, rule, order, r)
                    worst[form][rule][order] = max(worst[form][rule][order], r)
    print(worst, "K", G.K)
    for form, rules in worst.items():
        for rule, orders in rules.items():
            for order, r in orders.items():
                assert r == pytest.approx(G.RESTATEMENT_WORST[form][rule][order], rel=5e-3), (form, rule, order, r)
                k = G.K[form][rule][order]
                assert r <= 8.0 and k == B.K_of(r) and k / 2 < 16.0 * r <= k <= B.K_CAP == 128, (form, rule, order, r, k)


@needs_ld
@pytest.mark.parametrize("name", ["grid-ks8-w4-af0", "grid-ks20-w1-af1", "grid-narrow-domain", "kfold-mt2-ks8-str-n1odd", "kfold-loop72-mt2-ks4",
                                  "kfold-wide-domain"])
def test_the_reference_agrees_with_the_oracle(oracle_mod, name):
    """bary_eval_batch of the C oracle against the long-double reference, node-rule rows included: 1e-13 normwise."""
    m = next(m for m in G.all_models() if m.name == name)
    b = G.build(m)
    om = oracle_mod.BaryModel(b.c.nodes, b.c.weights, b.c.diff_matrices, b.c.tensor_values)
    for spec in G.specs_of(m.shape):
        ref, _ = B.reference(b.c.nodes, b.c.weights, B.derived_tensor(b.c, spec), b.pts)
        want = oracle_mod.bary_eval_batch(om, b.pts, spec)
        err = float(np.max(np.abs(want.astype(B.LD) - ref)) / np.max(np.abs(ref)))
        print(f"{name} {spec}: oracle against the reference {err:.2e}")
        assert err <= 1e-13, (name, spec, err)
