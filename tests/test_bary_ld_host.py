"""The lists of tests/bary_ld.py on a CPU: what tests/test_gpu_bary_lane_bodies.py runs on the device reaches every
body of the four lane-per-point switches of csrc/pcx_bary.hip (launch_small, launch_sq, bary_launch_small_pieces,
bary_launch_sq_pieces), the float64 restatement of the kernels sets K, and the long-double reference agrees with the
C oracle.  No GPU is used.

1. Planner coverage, from the lists alone and the GPU-free planner (tests/host/bary_plan_main.cpp with
   csrc/pcx_bary_plan.hip, built here without sanitizer flags; tests/test_bary_plan_host.py runs the sanitized build):
   every model of small_models() is offered variant 4 with the small_nlp the list claims, every model of sq_models()
   variant 5 with its sq_nl; the union of bodies is all 4 x 19 (DOUT, NLP), both EXACT branches of every NLP that has a
   padded one, every padded n in every DOUT, and all 25 x 3 (NL, LEAD).  The piece list reaches every (DOUT, NLP) and
   (NL, LEAD) again; the pieces of a spline share one shape, so they plan identically (pcx_spline_create's fused_ok).
2. The restatement stays within K of the reference on every model, and K <= 128.
3. On six shapes over d = 1 .. 4 the reference agrees with the oracle's bary_eval_batch to 1e-13 normwise."""
import json
import os
import subprocess

import numpy as np
import pytest

import bary_ld as B
from pychebyshev_amd import _build

HERE = os.path.dirname(os.path.abspath(__file__))

needs_ld = pytest.mark.skipif(not B.LD_OK, reason="np.longdouble is no wider than float64 here")


def _hipcc():
    try:
        return _build.hipcc_path()
    except RuntimeError:
        return None


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """shape -> the planner's record, from one child process over every shape of every list."""
    if _hipcc() is None:
        pytest.skip("hipcc not found")
    tmp = tmp_path_factory.mktemp("bary_ld_plan")
    exe, src = str(tmp / "bary_plan_main"), str(tmp / "cases.txt")
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O1", "-I", _build.CSRC, "-o", exe, os.path.join(HERE, "host", "bary_plan_main.cpp"),
           os.path.join(_build.CSRC, "pcx_bary_plan.hip")]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, "hipcc failed:\n" + res.stdout
    shapes = sorted({m.shape for m in B.small_models() + B.sq_models() + B.piece_models() + B.bucket_models() + B.tail_models()})
    with open(src, "w") as fh:
        fh.write("\n".join(" ".join(map(str, [len(s), *s, 1, 1, 1, 1, 1])) for s in shapes) + "\n")
    run = subprocess.run([exe, src], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and not run.stderr, f"exit {run.returncode}\n{run.stderr[-4000:]}"
    lines = run.stdout.splitlines()
    assert len(lines) == len(shapes)
    return {s: json.loads(line) for s, line in zip(shapes, lines)}


def _offers(rec, model):
    """The planner offers the model's variant with the width the list claims, inside the limits the launch code relies on."""
    assert rec["rc"] == 0, model.name
    shape, p = model.shape, rec["plan"]
    assert int(np.prod(shape)) <= 1 << 22 and len(shape) <= 4, model.name
    if model.family == "small":
        assert sum(shape[:-1]) <= 128, model.name                               # the outer weights table: 64 KB of LDS
        assert rec["set_kernel"][2] == 1 and p["small_nlp"] == B.nlp_of(shape[-1]), (model.name, p["small_nlp"])
    else:
        assert shape[-1] == shape[-2] and sum(shape[:-2]) <= 96, model.name
        assert rec["set_kernel"][3] == 1 and p["sq_nl"] == shape[-1], (model.name, p["sq_nl"])
        assert p["small_nlp"] == B.nlp_of(shape[-1]), model.name               # pcx_spline_create compares both widths


ALL_SMALL = {(dout, nlp) for dout in range(4) for nlp in B.NLP_LIST}
ALL_SQ = {(nl, lead) for nl in B.SQ_LIST for lead in range(3)}


def test_the_lists_are_the_sizes_the_issue_sets():
    small, sq, pieces = B.small_models(), B.sq_models(), B.piece_models()
    assert len(small) == 256 and len(sq) == 75 and len(pieces) == 4 * (19 + 5) + 75
    assert len({m.name for m in small + sq + pieces + B.bucket_models() + B.tail_models()}) == len(small) + len(sq) + len(pieces) + 2 + 7
    assert all(m.rows == B.ROWS == 96 for m in small + sq + pieces)
    outer = [v for m in small for v in m.shape[:-1]]
    assert 1 in outer and 2 in outer and len(set(outer)) == 7
    lead = [v for m in sq for v in m.shape[:-2]]
    assert set(lead) == {1, 2, 3, 4, 5}
    assert any(len(m.shape) == 4 and 1 in m.shape[:2] for m in sq)              # a LEAD = 2 model with a leading count of 1
    for m in pieces:
        n_pieces = int(np.prod([len(k) + 1 for k in m.knots]))
        assert len(m.knots[0]) in (1, 2) and n_pieces in (2, 3, 4, 6), m.name
    for i, m in enumerate(pieces):             # for d >= 2 every fourth model has a second knot in another dimension
        assert sum(len(k) for k in m.knots[1:]) == int(len(m.shape) >= 2 and i % 4 == 3), m.name
    assert {len(m.shape) - 1 - [bool(k) for k in m.knots][::-1].index(True) for m in pieces if any(m.knots[1:])} == {1, 2, 3}
    assert sorted(len(m.shape) for m in B.tail_models() if m.family == "small") == [1, 2, 3, 4]
    assert sorted(len(m.shape) for m in B.tail_models() if m.family == "sq") == [2, 3, 4]
    for m in B.bucket_models():
        assert len(m.knots[0]) == 5 and not any(m.knots[1:]) and m.rows == sum(B.BUCKETS) == 322


def test_the_single_model_lists_reach_every_body(planned):
    small, sq = B.small_models(), B.sq_models()
    for m in small + sq + B.tail_models():
        _offers(planned[m.shape], m)
    bodies = {B.small_body(m) for m in small}
    assert {(dout, nlp) for dout, nlp, _, _ in bodies} == ALL_SMALL and len(ALL_SMALL) == 76
    for dout in range(4):
        for nlp in B.NLP_LIST:
            assert (dout, nlp, True, nlp) in bodies                              # bary_weights_reg<NLP, true>
        padded = {n for do, _, exact, n in bodies if do == dout and not exact}   # bary_weights_reg<NLP, false>: every j < n test
        assert padded == set(B.PADDED_N) and len(padded) == 1 + 7 + 7 + 15 + 15, dout
        assert {nlp for do, nlp, exact, _ in bodies if do == dout and not exact} == {2, 24, 32, 48, 64}
    assert {B.sq_body(m) for m in sq} == ALL_SQ and len(ALL_SQ) == 75


def test_the_piece_list_reaches_every_body_of_the_piece_switches(planned):
    pieces = B.piece_models()
    for m in pieces + B.bucket_models():
        _offers(planned[m.shape], m)           # one shape per spline: every piece plans as this record does (fused_ok)
    small = {B.small_body(m) for m in pieces if m.family == "small"}
    assert {(dout, nlp) for dout, nlp, _, _ in small} == ALL_SMALL
    for dout in range(4):
        assert {(nlp, n) for do, nlp, exact, n in small if do == dout and exact} == {(v, v) for v in B.NLP_LIST}
        assert {(nlp, n) for do, nlp, exact, n in small if do == dout and not exact} == {(2, 1), (24, 19), (32, 27), (48, 41), (64, 57)}
    assert {B.sq_body(m) for m in pieces if m.family == "sq"} == ALL_SQ


@needs_ld
def test_every_kind_of_row_is_where_the_list_says():
    """The rows of a model: corners, a grid point, on a node of the last and of an outer dimension only, next to a node
    (2e-15 .. 5e-15 away) in each, uniform rows; in a spline inside every piece, and one row on the knot, which the
    searchsorted rule gives to the right-hand piece."""
    for m in (B.small_models()[64 + 8], B.small_models()[3 * 64 + 40], B.sq_models()[5]):
        b = B.build(m)
        nodes, d = b.c.nodes, len(m.shape)
        gap = [np.min(np.abs(b.pts[:, k, None] - nodes[k][None, :]), axis=1) for k in range(d)]
        assert np.array_equal(b.pts[0], [lo for lo, _ in b.c.domain]) and np.array_equal(b.pts[1], [hi for _, hi in b.c.domain])
        assert all(gap[k][b.grid_row] == 0 for k in range(d))
        assert b.c.tensor_values[b.grid_idx] == B.restatement(nodes, b.c.weights, b.c.tensor_values, b.pts)[b.grid_row]
        assert gap[d - 1][3] == 0 and all(gap[k][3] > 1e-9 for k in range(d - 1))
        assert b.pts[3, d - 1] == nodes[d - 1][-1 if m.seed % 2 else 0]
        assert sum(gap[k][4] == 0 for k in range(d - 1)) == 1 and gap[d - 1][4] > 1e-9
        assert 2e-15 <= gap[d - 1][5] <= 5e-15 and all(gap[k][5] > 1e-9 for k in range(d - 1))
        assert sum(2e-15 <= gap[k][6] <= 5e-15 for k in range(d - 1)) == 1 and gap[d - 1][6] > 1e-9
        assert all(np.all(g[7:] > 1e-12) for g in gap)
    for m in (B.piece_models()[30], B.piece_models()[-1]):
        b = B.build_spline(m)
        n_pieces = len(b.sp._pieces)
        assert sorted(p for _, p, _ in b.grid_rows) == list(range(n_pieces))
        for row, p, idx in b.grid_rows:
            assert b.ids[row] == p and np.array_equal(b.pts[row], [b.sp._pieces[p].nodes[k][i] for k, i in enumerate(idx)])
        on_knot = np.nonzero(b.pts[:, 0] == b.sp.knots[0][0])[0]
        assert len(on_knot) >= 1 and np.all(np.unravel_index(b.ids[on_knot], b.sp._shape)[0] == 1)
        assert np.all(np.bincount(b.ids, minlength=n_pieces) >= 5)
    for m in B.bucket_models():
        b = B.build_spline(m, B.BUCKETS)
        assert sorted(np.bincount(b.ids, minlength=6).tolist()) == sorted(B.BUCKETS)
        assert np.any(np.diff(b.ids) < 0)                                         # shuffled, not bucket by bucket


@needs_ld
def test_the_restatement_sets_every_K():
    """The float64 restatement against the long-double reference on every list entry, value and first-derivative specs,
    per kernel family: the worst |y - ref| / (eps A_row) is the figure bary_ld.RESTATEMENT_WORST records (a fixed
    sequence of elementwise operations: the same bits everywhere), below 8, and K is 16 times it, rounded up to a power
    of two, <= 128."""
    for family, orders in B.K.items():
        worst = dict.fromkeys(orders, 0.0)
        for m in B.family_models(family):
            for order, r in B.restatement_ratios(m).items():
                worst[order] = max(worst[order], r)
        print(family, {o: round(r, 4) for o, r in worst.items()}, "K", B.K[family])
        for order, r in worst.items():
            assert r == pytest.approx(B.RESTATEMENT_WORST[family][order], rel=5e-3), (family, order, r)
            k = B.K[family][order]
            assert r <= 8.0 and k == B.K_of(r) and k / 2 < 16.0 * r <= k <= B.K_CAP == 128, (family, order, r, k)


@needs_ld
@pytest.mark.parametrize("name", ["small-d1-n23", "small-d2-n64", "small-d3-n9", "small-d4-n41", "sq-n13-lead1", "sq-n6-lead2"])
def test_the_reference_agrees_with_the_oracle(oracle_mod, name):
    """bary_eval_batch of the C oracle (float64 in the reference's order, the node rule applied literally) against the
    long-double reference, node-rule rows included: 1e-13 normwise, value and first-derivative specs."""
    m = next(m for m in B.small_models() + B.sq_models() if m.name == name)
    b = B.build(m)
    om = oracle_mod.BaryModel(b.c.nodes, b.c.weights, b.c.diff_matrices, b.c.tensor_values)
    for spec in B.specs_of(m.shape):
        ref, _ = B.reference(b.c.nodes, b.c.weights, B.derived_tensor(b.c, spec), b.pts)
        want = oracle_mod.bary_eval_batch(om, b.pts, spec)
        err = float(np.max(np.abs(want.astype(B.LD) - ref)) / np.max(np.abs(ref)))
        print(f"{name} {spec}: oracle against the reference {err:.2e}")
        assert err <= 1e-13, (name, spec, err)
