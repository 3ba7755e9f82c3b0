"""tests/tt_chain.py on the host: the long-double chain against the three golden files that hold such chains already,
the coverage of the lane-body sweep and of the MFMA forms' list computed from the model lists (and tests/tt_plan_rule.py)
alone, and the measurement behind every K of the row bound in tests/test_gpu_tt_lane_bodies.py and
tests/test_gpu_tt_mfma_bodies.py.  Host NumPy only: no GPU."""
import numpy as np
import pytest

from conftest import assert_parity, golden, spec_point_tol
import tt_chain as C
import tt_plan_rule as R

G22 = golden("g22_tt_transforms")
G28 = golden("g28_tt_derivatives")
MODELS = ("A", "B", "C", "C2", "D", "E", "F")


def g22_model(tag, src=G22):
    cores, k = [], 0
    while f"{tag}_core{k}" in src.files:
        cores.append(src[f"{tag}_core{k}"])
        k += 1
    return cores, src[f"{tag}_domain"].tolist()


# ------------------------------------------------------------------------------------------------ the stored chains
@pytest.mark.parametrize("tag", MODELS)
def test_the_derivative_chain_reproduces_g28(tag):
    """The _ld columns were computed in long double by the same recurrences: equal to 1e-15 after rounding to float64."""
    cores, domain = g22_model(tag)
    order = G22[f"{tag}_order"].tolist()
    for i in range(int(G28[f"{tag}_nspec"])):
        g = f"{tag}_s{i}"
        spec, want = G28[f"{g}_spec"].tolist(), G28[f"{g}_ld"]
        val, amp = C.Chain(cores, domain, order, G28[f"{g}_pts"]).deriv(spec)
        got = val.astype(np.float64)
        if not np.any(want):
            assert np.all(got == 0.0) and np.all(amp == 0), g
            continue
        assert np.all(np.abs(got - want) <= 1e-15 * np.maximum(np.abs(want), 1e-3 * np.max(np.abs(want)))), \
            (g, spec, float(np.max(np.abs(got - want) / np.abs(want))))
        assert np.all(amp >= np.abs(val))


def _box_groups(tag):
    i = 0
    while f"{tag}_box{i}_dims" in G22.files:
        yield f"{tag}_box{i}"
        i += 1


@pytest.mark.parametrize("tag", MODELS)
def test_the_box_chain_reproduces_g22(tag):
    """The _ref rows are the reference's float64 integrate(dims, bounds).eval(point): the bound of
    test_gpu_tt_transforms.py::test_integrate_batch_matches_the_reference (assert_parity's defaults)."""
    cores, domain = g22_model(tag)
    order = G22[f"{tag}_order"].tolist()
    d = len(cores)
    udom = [domain[order.index(u)] for u in range(d)]
    groups = list(_box_groups(tag))
    assert groups
    for g in groups:
        dims, bounds, points = G22[f"{g}_dims"].tolist(), G22[f"{g}_bounds"], G22[f"{g}_points"]
        pts = np.empty((bounds.shape[0], d))
        kept = [u for u in range(d) if u not in dims]
        pts[:, kept] = points
        pts[:, dims] = [udom[u][0] for u in dims]              # not read: these dimensions are integrated
        val, amp = C.Chain(cores, domain, order, pts).box(dims, bounds)
        assert_parity(val.astype(np.float64), G22[f"{g}_ref"], what=f"long-double box chain {g}")
        assert val[1] == 0 and amp[1] > 0                       # row 1: lo == hi; the amplitude does not cancel
        assert np.all(amp >= np.abs(val))


@pytest.mark.parametrize("tag", ["A", "C", "F", "G"])
def test_the_ladder_chain_reproduces_g34(tag):
    """The TT rows of g34 are the reference's float64 eval at every (fixed..., x): the bounds of
    test_gpu_ladders.py::test_tt_ladder_matches_the_reference, over the file's own masks."""
    g34 = golden("g34_ladders")
    cores, domain = g22_model("tG", g34) if tag == "G" else g22_model(tag)
    order = [int(v) for v in g34[f"t{tag}_order"]]
    for dim in [int(v) for v in g34[f"t{tag}_dims"]]:
        pre = f"t{tag}_k{dim}"
        fixed, xs, xsrow = g34[f"{pre}_fixed"], g34[f"{pre}_xs"], g34[f"{pre}_xsrow"]
        ok, rowok = g34[f"{pre}_refok"], g34[f"{pre}_refrowok"]
        val, _ = C.Chain(cores, domain, order, C.with_column(fixed, dim)).ladder(dim, xs)
        assert_parity(val.astype(np.float64)[:, ok], g34[f"{pre}_ref"][:, ok], tol=1e-12, point_tol=spec_point_tol([0]),
                      what=f"long-double ladder {pre} shared")
        val, _ = C.Chain(cores, domain, order, C.with_column(fixed[:xsrow.shape[0]], dim)).ladder(dim, xsrow)
        assert_parity(val.astype(np.float64)[rowok], g34[f"{pre}_refrow"][rowok], tol=1e-12, point_tol=spec_point_tol([0]),
                      what=f"long-double ladder {pre} per row")


@pytest.mark.parametrize("number", [0, 37, 160, 287, 289])
def test_the_ladder_is_the_value_chain_at_the_expanded_points(number):
    """Associating the product around the ladder's core changes nothing beyond long-double rounding: against the plain
    chain at every (fixed..., x), within 2^-60 of the amplitude, and the amplitudes agree as closely."""
    b = C.build((C.sweep_models() + C.edge_models())[number])
    d = len(b.model.n)
    chain = C.Chain(b.cores, b.domain, b.order, b.pts)
    for dim, xs in C.ladder_cases(b):
        val, amp = chain.ladder(dim, xs)
        pts = C.expand(d, dim, np.delete(b.pts, dim, axis=1), xs)
        v2, a2 = C.Chain(b.cores, b.domain, b.order, pts).value()
        assert np.all(np.abs(val.ravel() - v2) <= 2.0 ** -60 * a2)
        assert np.all(np.abs(amp.ravel() - a2) <= 2.0 ** -60 * a2)


# ------------------------------------------------------------------------------------------------ coverage
def test_the_sweep_reaches_every_lane_body():
    """Computed from the model list alone: (rank cap, uniform or mixed, left rank, node count) over the dimensions of
    the sweep is the full set of 16 x (8 + 12 + 16) x 2 = 1,152 bodies of each of eval, fd, box and deriv."""
    models = C.sweep_models()
    assert len(models) == 288 and [m.number for m in models] == list(range(288))
    want = C.all_lane_bodies()
    assert len(want) == 1152
    assert want == {(cap, uni, rl, n) for cap, top in ((8, 8), (12, 12), (16, 16)) for uni in (True, False)
                    for rl in range(1, top + 1) for n in range(1, 17)}
    assert C.lane_bodies(models) == want
    for m in models:
        d = len(m.n)
        assert len(m.ranks) == d + 1 and m.ranks[0] == m.ranks[-1] == 1 and 4 <= d <= 6 and m.rows == 96
        assert C.rank_cap(m) == m.cap == (8 if max(m.ranks) <= 8 else 12 if max(m.ranks) <= 12 else 16)
        assert C.is_uniform(m) == (m.mode == "uniform")
        assert m.cap != 16 or 16 in m.ranks                 # auto takes the MFMA form there: variant 4 reaches the lane bodies
    assert len(C.rank_chains()) == 9


def test_the_ladder_sweep_reaches_every_node_count_on_every_side():
    assert C.ladder_positions(C.sweep_models()) == {(side, n) for side in ("left", "at", "right") for n in range(1, 17)}


def test_models_rows_and_cases_are_what_the_sweep_says():
    models = C.sweep_models()
    for m in models[:12] + models[150:156] + C.edge_models() + (C.tail_model(),):
        b = C.build(m)
        d = len(m.n)
        assert (b.order is not None) == (m.number % 3 == 0)
        assert [c.shape for c in b.cores] == [(m.ranks[k], m.n[k], m.ranks[k + 1]) for k in range(d)]
        assert b.pts.shape == (m.rows, d)
        assert b.pts[0].tolist() == [a for a, _ in b.udom] and b.pts[1].tolist() == [hi for _, hi in b.udom]
        again = C.build(m)
        assert np.array_equal(again.pts, b.pts) and all(np.array_equal(x, y) for x, y in zip(again.cores, b.cores))
        specs = C.deriv_specs(m)
        assert len(specs) == 2 * d + 2 <= 64 and specs[0] == [0] * d and sorted(specs[-1]) == [0] * (d - 2) + [1, 2]
        fd = C.fd_specs(m)
        assert fd[0] == [0] * d and [sorted(s, reverse=True)[:2] for s in fd[1:]] == [[1, 0], [2, 0], [1, 1]]
        assert [sum(s) for s in fd] == [0, 1, 2, 2]
        boxes = C.box_cases(b)
        assert [dims for dims, _ in boxes] == [[u] for u in range(d)] + [list(range(d))]
        for dims, bounds in boxes:
            assert bounds[1, 0, 0] == bounds[1, 0, 1]
            for j, u in enumerate(dims):
                lo, hi = b.udom[u]
                w = (bounds[2:, j, 1] - bounds[2:, j, 0]) / (hi - lo)
                assert np.all(bounds[:, j, 0] >= lo) and np.all(bounds[:, j, 1] <= hi) and np.all((w >= 0.0499) & (w <= 1.0))
                assert bounds[0, j].tolist() == [lo, hi]
        ladders = C.ladder_cases(b)
        assert [dim for dim, _ in ladders] == [u for u in sorted({0, d // 2, d - 1}) for _ in range(2)]
        assert all(np.shape(xs) in ((C.LADDER_M,), (m.rows, C.LADDER_M)) for _, xs in ladders)
    # the fd dimensions rotate: over a chain's 32 models every dimension is differenced at each order
    for first in range(0, 288, 32):
        d = len(models[first].n)
        specs = [C.fd_specs(m) for m in models[first:first + 32]]
        for col in (1, 2):
            assert {int(np.argmax(s[col])) for s in specs} == set(range(d))
    edge = C.edge_models()
    assert [(m.ranks, m.n, m.rows) for m in edge] == [((1, 64, 65, 1), (3, 4, 17), 130), ((1, 130, 1), (2, 9), 130),
                                                     ((1, 1, 1), (17, 1), 130)]
    assert all(C.rank_cap(m) == 0 for m in edge)
    tail = C.tail_model()
    assert tail.cap == 12 and tail.mode == "mixed" and not C.is_uniform(tail) and tail.rows == max(C.TAIL_NS) == 129


def test_the_mfma_list_is_what_its_docstring_says():
    models = C.mfma_models()
    first = C.tail_model().number + 1
    assert first == 292 and [m.number for m in models] == list(range(first, first + 220))
    assert len({m.name for m in models}) == 220 and all(m.rows == 96 for m in models)
    assert sum(m.number % 3 == 0 for m in models) in (73, 74)              # every third behind a permuted dim_order
    for c, ranks in enumerate(C.SMALL_CHAINS):
        top = max(ranks)
        assert len(ranks) == 5 and 4 * c < top <= 4 * c + 4 and any(r % 4 for r in ranks[1:-1])
        mine = [m for m in models if m.ranks == ranks and m.mode != "mfma-global"]
        assert [m.n for m in mine if m.mode == "mfma-uniform"] == [(n,) * 4 for n in range(1, 33)]
        mixed = [m.n for m in mine if m.mode == "mfma-mixed"]
        assert [max(n) for n in mixed] == list(range(2, 33)) and all(n.count(max(n)) == 1 for n in mixed)
        where = [n.index(max(n)) for n in mixed]
        assert {0, 3} < set(where) == {0, 1, 2, 3} and all(a != b for a, b in zip(where, where[1:]))
        for n in mixed:                    # from two k-steps on, a dimension whose last k-step holds zero rows only
            ks = -(-max(n) // 4)
            assert ks == 1 or min(n) <= 4 * ks - 4
    # d = 4 is the largest d whose W-first image fits at R = 12, KS = 8
    fits = [R.plan(d, [32] * d, [1] + [12] * (d - 1) + [1], [0.0] * d, [1.0] * d, None)["plan"]["wR"] for d in (4, 5)]
    assert fits == [12, 0]
    large = [m for m in models if m.ranks in C.LARGE_CHAINS]
    assert [(max(r), 1 in r[1:-1], 64 in r) for r in C.LARGE_CHAINS] == [(16, False, False), (32, True, False), (64, False, True)]
    assert {m.ranks[k] % 4 for m in large for k in range(len(m.n))} == {0, 1, 2, 3}              # left ranks
    assert {1, 15, 16, 17} <= {m.ranks[k + 1] for m in large for k in range(len(m.n))}           # right ranks
    for ranks in C.LARGE_CHAINS:
        assert [m.n for m in large if m.ranks == ranks and m.mode == "mfma-uniform"] == [(n,) * (len(ranks) - 1) for n in C.DIRECT_NS]
    # the last core just past its LDS copy: one node fewer and the planner keeps the copy
    glob = [m for m in models if m.mode == "mfma-global"]
    assert [m.ranks for m in glob] == list(C.SMALL_CHAINS + C.LARGE_CHAINS)
    for m in glob:
        assert C.plan_of(m)["last_lds_doubles"] == 0 and max(m.n[:-1]) <= 3
        assert C.plan_of(m._replace(n=m.n[:-1] + (m.n[-1] - 1,)))["last_lds_doubles"] == C.plan_of(m)["last_rows"] * (m.n[-1] - 1)
    assert [(m.ranks, m.n) for m in models if m.mode == "mfma-lowd"] == list(C.LOWD)
    assert [(max(r), n) for r, n in C.LOWD] == [(1, (1,)), (1, (7,)), (1, (32,)), (4, (5, 3)), (12, (7, 10)), (16, (6, 5)), (64, (4, 9))]
    for m in models[:3] + models[-3:] + C.mfma_extra_models():
        b, again = C.build(m), C.build(m)
        assert (b.order is not None) == (m.number % 3 == 0) and b.pts.shape == (m.rows, len(m.n))
        assert b.pts[0].tolist() == [a for a, _ in b.udom] and b.pts[1].tolist() == [hi for _, hi in b.udom]
        assert np.array_equal(again.pts, b.pts) and all(np.array_equal(x, y) for x, y in zip(again.cores, b.cores))


def test_the_mfma_list_reaches_every_body_of_the_three_forms():
    """Computed from the model list and tests/tt_plan_rule.py's restatement of the planner alone."""
    models = C.mfma_models()
    want = C.all_direct_bodies()
    assert len(want) == 11 + 6 * 2 * 5 + 6 * 2 == 83
    assert {b[1] for b in want} == {1, 2, 3, 4, 8, 16}
    assert {b[3] for b in want if b[0] == "nodes" and b[2] == "mid"} == {"ping-pong", "plain"}
    assert {b[1] for b in want if b[0] == "nodes" and b[3] == "plain"} == {8, 16}
    assert C.direct_bodies(models) == want
    want = C.all_wfirst_bodies()
    assert len(want) == 3 * 8 * 2 == 48
    assert C.wfirst_bodies(models) == want
    want = C.all_d4_bodies()
    assert len(want) == 3 * (4 + 16 + 16) == 108
    assert C.d4_bodies(models) == want
    # the bodies are reached on the variant that owns them: which variants a model's plan offers
    for m in models:
        small, nmax = max(m.ranks) <= 12, max(m.n)
        assert C.offered(m) == (1,) + ((2,) if small and nmax <= 32 else ()) + ((3,) if small and nmax <= 16 else ()), m.name
        p = C.plan_of(m)
        auto = R.auto_variant(p, 0)
        assert auto == (4 if max(m.ranks) <= 15 and nmax <= 16 else 3 if 3 in C.offered(m) else 2 if 2 in C.offered(m) else 1), m.name
    # every W-first instantiation of 5 .. 8 k-steps, the range where auto takes the form, runs on auto too
    assert {(C.plan_of(m)["wR"], C.plan_of(m)["wplan.ks"]) for m in models if R.auto_variant(C.plan_of(m), 0) == 2} \
        == {(r, ks) for r in (4, 8, 12) for ks in range(5, 9)}


def test_the_tail_and_persistent_models_run_the_kernels_their_tests_name():
    tails = C.mfma_tail_models()
    assert [(C.plan_of(m)["cls"], C.plan_of(m)["wR"], v) for m, v in tails] == [(0, 0, 1), (1, 0, 1), (2, 0, 1), (0, 4, 2), (0, 12, 2), (0, 8, 3)]
    assert all(m.rows == 300 > max(C.MFMA_TAIL_NS) and v in C.offered(m) for m, v in tails)
    assert tails[0][0].number == C.mfma_models()[-1].number + 1
    (wide, v0, p0), (w12, v1, p1), (d4, v2, p2) = C.persistent_models()
    assert (v0, p0, C.plan_of(wide)["wR"]) == (2, 256, 4) and (v1, p1, C.plan_of(w12)["wR"]) == (2, 64, 12) and (v2, p2) == (3, 64)
    assert C.plan_of(d4)["d4RA"] == 3 and wide.number == tails[-1][0].number + 1
    # residency by LDS alone, and the host array of 3 x 4 x resident x CUs batches on a device of 256 CUs
    assert [C.CU_LDS_BYTES // C.launch_lds(m, v) for m, v, _ in C.persistent_models()] == [1, 1, 2]
    for m, v, per in C.persistent_models():
        assert (3 * 4 * (C.CU_LDS_BYTES // C.launch_lds(m, v)) * 256 * per + 777) * len(m.n) * 8 < 100e6
    assert C.launch_lds(wide._replace(ranks=wide.ranks[:-2] + (1,), n=wide.n[:-1]), 2) <= C.CU_LDS_BYTES // 2     # d = 11: two resident


# ------------------------------------------------------------------------------------------------ the tolerance
def test_the_restatement_sets_every_K():
    """The float64 restatement against the long-double chain on every case of every model, per list and family: the
    worst |y - ref| / (eps A_row) is the figure tt_chain.RESTATEMENT_WORST records (the arithmetic is a fixed sequence
    of elementwise operations: the same bits everywhere), and K is 16 times it, rounded up to a power of two, <= 64.
    The MFMA forms' lists are lists of eval_batch: their value rows alone."""
    worst = {group: dict.fromkeys(fam, 0.0) for group, fam in C.K.items()}
    for m in C.sweep_models() + C.edge_models() + (C.tail_model(),):
        for family, r in C.restatement_ratios(C.build(m)).items():
            w = worst[C.group_of(m)]
            w[family] = max(w[family], r)
    for m in C.mfma_models() + C.mfma_extra_models():
        w = worst[C.group_of(m)]
        w["value"] = max(w["value"], C.restatement_value_ratio(C.build(m)))
    assert set(worst["mfma"]) == set(worst["mfma-lowd"]) == {"value"}
    for group, fam in worst.items():
        print(group, {f: round(r, 4) for f, r in fam.items()}, "K", C.K[group])
        for family, r in fam.items():
            assert r == pytest.approx(C.RESTATEMENT_WORST[group][family], rel=5e-3), (group, family, r)
            k = C.K[group][family]
            assert k == C.K_of(r) and k / 2 < 16.0 * r <= k <= C.K_CAP, (group, family, r, k)
