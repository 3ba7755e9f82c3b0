"""The planner of ``ChebyshevSpline.eval_grid`` (csrc/spline_grid_plan.h) on a CPU, and the argument checks of the
spline's and the slider's ``eval_grid`` that need no device.

tests/host/spline_grid_plan_main.cpp is compiled with hipcc under the address and undefined-behaviour sanitizers (host
side) and run once as a child process over every spline grid of tests/golden/g32_piecewise_grid.npz plus the edges: all
entries of an axis in one interval, an axis of length 1 on a knot, a NaN entry, and d = 16 with m = 1 everywhere.
Asserted:

1. intervals equal ``np.searchsorted(knots, x, side="right")`` clipped to the last piece, a NaN in the last piece;
2. the list of every interval holds exactly its entries in ascending position (stable), ranks are positions in it;
3. a piece has a block exactly when every one of its d lists is non-empty; blocks lie back to back in ascending piece
   order, C order each, and tile ``prod m`` doubles exactly; a block's sub-axes are the coordinates of its lists;
4. every grid index maps to exactly one (block, local index) through the tables the placement kernel reads, and what
   lies there is the block's own element for that index;
5. an empty axis is PCX_ERR_INVALID and names the dimension; the sanitizers report nothing.
No GPU is used."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import golden
import generate_golden_piecewise_grid as G

from pychebyshev_amd import ChebyshevSlider, ChebyshevSpline, _build, _lib

HERE = os.path.dirname(os.path.abspath(__file__))
SAN_FLAGS = ["--offload-arch=gfx950", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
             "-fno-sanitize-recover=undefined"]
PCX_ERR_INVALID = -1


def _hipcc():
    try:
        return _build.hipcc_path()
    except RuntimeError:
        return None


needs_hipcc = pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")


def _cases():
    """id -> (knots per dimension, axes per dimension)"""
    g = golden("g32_piecewise_grid")
    out = {}
    for i, grid in enumerate(G.SPLINE_GRIDS):
        knots = G.SP.CASES[grid["case"]]["knots"]
        out[G.grid_id(grid)] = (knots, [g[f"s{i}_ax{k}"] for k in range(len(knots))])
    rng = np.random.default_rng(32)
    out["one_interval"] = ([[0.0, 1.0], [0.5]], [rng.uniform(0.1, 0.9, 7), rng.uniform(-1.0, 2.0, 5)])    # dimension 0 in [0, 1) only
    out["on_a_knot"] = ([[0.25, 0.5], [0.5]], [np.array([0.5]), np.array([0.7, 0.5, 0.2, 0.5])])
    out["nan"] = ([[0.0], [1.0, 2.0]], [np.array([0.3, np.nan, -0.3, 0.0]), np.array([2.5, 0.5, np.nan, 1.0, 1.5])])
    out["d16"] = ([[0.5], []] * 8, [np.array([v]) for v in rng.uniform(0.0, 1.0, 16)])
    out["repeats"] = ([[-1.0, -1.0, 3.0]], [np.array([3.0, -1.0, 5.0, -2.0, -1.0, 0.0, 3.0])])           # a double knot: an interval nothing can reach
    out["no_knots"] = ([[], []], [rng.uniform(0.0, 1.0, 3), rng.uniform(0.0, 1.0, 4)])
    return out


CASES = _cases()


def _hex(values):
    return " ".join(float(v).hex() for v in np.asarray(values, dtype=float).ravel())


def _line(knots, m, axes):
    toks = ["S", str(len(knots)), *[str(len(k)) for k in knots], *map(str, m)]
    toks += [t for t in (_hex(np.concatenate([np.asarray(k, dtype=float) for k in knots])), _hex(np.concatenate(axes)) if sum(m) else "") if t]
    return " ".join(toks)


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """(records by id, the bad case's record) from ONE sanitized child."""
    tmp = tmp_path_factory.mktemp("spline_grid_plan")
    exe, src = str(tmp / "spline_grid_plan_main"), str(tmp / "cases.txt")
    cmd = [_hipcc()] + SAN_FLAGS + ["-I", _build.CSRC, "-o", exe, os.path.join(HERE, "host", "spline_grid_plan_main.cpp")]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, "hipcc failed:\n" + res.stdout
    lines = [_line(knots, [a.size for a in axes], axes) for knots, axes in CASES.values()]
    bad = _line([[0.5], []], [3, 0], [np.array([0.1, 0.6, 0.5]), np.array([])])
    with open(src, "w") as fh:
        fh.write("\n".join(lines + [bad]) + "\n")
    run = subprocess.run([exe, src], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and not run.stderr, f"exit {run.returncode} (sanitizer report?)\n{run.stderr[-4000:]}"
    recs = [json.loads(line) for line in run.stdout.splitlines()]
    assert len(recs) == len(lines) + 1
    return dict(zip(CASES, recs[:-1])), recs[-1]


def _per_dim(rec, name, off):
    return [np.array(rec[name][rec[off][k]:rec[off][k + 1]], dtype=np.int64) for k in range(len(rec[off]) - 1)]


@needs_hipcc
@pytest.mark.parametrize("cid", list(CASES))
def test_intervals_lists_and_ranks(planned, cid):
    knots, axes = CASES[cid]
    rec = planned[0][cid]
    assert rec["rc"] == 0, rec
    d = len(knots)
    shape = [len(k) + 1 for k in knots]
    assert rec["total"] == int(np.prod([a.size for a in axes])) and rec["n_pieces"] == int(np.prod(shape))
    iv, rk, ls = _per_dim(rec, "interval", "axis_off"), _per_dim(rec, "rank", "axis_off"), _per_dim(rec, "list", "axis_off")
    cnt, loff = _per_dim(rec, "count", "cnt_off"), _per_dim(rec, "list_off", "cnt_off")
    for k in range(d):
        want = G.route(knots[k], shape[k], axes[k])
        assert np.array_equal(iv[k], want), (cid, k)
        assert np.all(iv[k][np.isnan(axes[k])] == shape[k] - 1), "a NaN belongs to the last piece"
        assert cnt[k].size == shape[k] and np.array_equal(cnt[k], np.bincount(want, minlength=shape[k]))
        for j in range(shape[k]):
            start = loff[k][j] - rec["axis_off"][k]
            members = ls[k][start:start + cnt[k][j]]
            assert np.array_equal(members, np.flatnonzero(want == j)), f"{cid}: the list of interval {j} of dimension {k} is not stable"
            assert np.array_equal(rk[k][members], np.arange(members.size))


@needs_hipcc
@pytest.mark.parametrize("cid", list(CASES))
def test_blocks_tile_the_grid_and_every_index_has_one_home(planned, cid):
    knots, axes = CASES[cid]
    rec = planned[0][cid]
    d = len(knots)
    shape = [len(k) + 1 for k in knots]
    m = [a.size for a in axes]
    iv, rk = _per_dim(rec, "interval", "axis_off"), _per_dim(rec, "rank", "axis_off")
    cnt = _per_dim(rec, "count", "cnt_off")
    sub = np.array([float.fromhex(v) for v in rec["sub_axes"]])
    # live pieces: every list non-empty; in ascending flat order, back to back
    live = [int(np.ravel_multi_index(multi, shape)) for multi in np.ndindex(*shape) if all(cnt[k][multi[k]] for k in range(d))]
    assert [b[0] for b in rec["blocks"]] == live
    block_off = np.array(rec["block_off"])
    assert block_off.size == rec["n_pieces"] and np.all(block_off[[p for p in range(rec["n_pieces"]) if p not in set(live)]] == -1)
    at = a_at = 0
    stage = np.full(rec["total"], -1, dtype=np.int64)         # the grid index each staged element belongs to
    flat = np.arange(rec["total"]).reshape(m)
    for piece, offset, count, axes_off, *bm in rec["blocks"]:
        multi = np.unravel_index(piece, shape)
        assert offset == at == block_off[piece] and axes_off == a_at
        assert bm == [int(cnt[k][multi[k]]) for k in range(d)] and count == int(np.prod(bm))
        pos = [np.flatnonzero(iv[k] == multi[k]) for k in range(d)]
        want_axes = np.concatenate([axes[k][pos[k]] for k in range(d)])
        assert np.array_equal(sub[a_at:a_at + sum(bm)], want_axes, equal_nan=True), f"{cid}: sub-axes of piece {piece}"
        stage[offset:offset + count] = flat[np.ix_(*pos)].ravel()
        at += count
        a_at += sum(bm)
    assert at == rec["total"] and a_at == sub.size, "the blocks do not tile prod m exactly"
    assert np.array_equal(np.sort(stage), np.arange(rec["total"])), "an element is staged twice or never"
    # the placement kernel's arithmetic: piece from the intervals, local index from the ranks and the counts
    grids = np.meshgrid(*[np.arange(mk) for mk in m], indexing="ij")
    piece = np.zeros(m, dtype=np.int64)
    local = np.zeros(m, dtype=np.int64)
    for k in range(d):
        piece = piece * shape[k] + iv[k][grids[k]]
        local = local * cnt[k][iv[k][grids[k]]] + rk[k][grids[k]]
    src = block_off[piece] + local
    assert np.all(block_off[piece] >= 0)
    assert np.array_equal(stage[src], flat), f"{cid}: a grid index does not find its own element"


@needs_hipcc
def test_edges(planned):
    recs = planned[0]
    one = recs["one_interval"]
    assert one["count"][:3] == [0, 7, 0] and one["n_pieces"] == 6                   # intervals 0 and 2 of dimension 0 are dead
    assert len(one["blocks"]) == len(set(one["interval"][7:])) and all(b[0] in (2, 3) for b in one["blocks"])
    assert recs["on_a_knot"]["interval"][0] == 2, "a coordinate on a knot belongs to the right-hand piece"
    assert len(recs["d16"]["blocks"]) == 1 and recs["d16"]["total"] == 1 and recs["d16"]["n_pieces"] == 256
    assert recs["repeats"]["count"][1] == 0, "nothing lies between the two equal knots"
    assert len(recs["no_knots"]["blocks"]) == 1 and recs["no_knots"]["blocks"][0][:3] == [0, 0, 12]
    m_live = recs["m_3x4x2"]
    assert len(m_live["blocks"]) == 6 and m_live["n_pieces"] == 8


@needs_hipcc
def test_planner_rejects_an_empty_axis(planned):
    bad = planned[1]
    assert bad["rc"] == PCX_ERR_INVALID and "dimension 1" in bad["error"] and "empty" in bad["error"]


# ---------------------------------------------------------------- Python-side argument checks (no device is touched)
def _spline(built=True):
    sp = ChebyshevSpline(lambda x, _: abs(x[0]) + x[1], 2, [[-1.0, 1.0], [0.0, 1.0]], [4, 3], knots=[[0.0], []])
    if built:
        sp.build(verbose=False)
    return sp


def _slider(built=True):
    sl = ChebyshevSlider(lambda x, _: x[0] + x[1] * x[2], 3, [[-1.0, 1.0]] * 3, [3, 4, 3], partition=[[0], [1, 2]], pivot_point=[0.0] * 3)
    if built:
        sl.build(verbose=False)
    return sl


@pytest.mark.parametrize("make", [_spline, _slider], ids=["spline", "slider"])
def test_eval_grid_argument_errors(make):
    obj = make()
    d = obj.num_dimensions
    ax = [[0.1, 0.2]] * d
    with pytest.raises(RuntimeError, match="build"):
        make(built=False).eval_grid(ax)
    with pytest.raises(ValueError, match=f"{d} entries"):
        obj.eval_grid(ax[:-1])
    with pytest.raises(ValueError, match=f"sequence of {d}"):
        obj.eval_grid(0.5)
    with pytest.raises(ValueError, match=r"axes\[0\] is empty: dimension 0"):
        obj.eval_grid([[]] + ax[1:])
    with pytest.raises(ValueError, match=r"axes\[1\].*dimension 1"):
        obj.eval_grid([ax[0], np.zeros((2, 2))] + ax[2:])
    with pytest.raises(ValueError, match="not both"):
        obj.eval_grid(ax, [0] * d, derivative_id=0)
    with pytest.raises(ValueError, match=f"derivative_order must have {d} entries"):
        obj.eval_grid(ax, [0] * (d + 1))
    # a wrong `out` is refused before the model goes to a device: a borrowed DeviceArray over no memory serves
    from pychebyshev_amd.device import DeviceArray
    with pytest.raises(ValueError, match="at dimension 1"):
        obj.eval_grid(ax, out=DeviceArray(4096, (2, 3) + (2,) * (d - 2), 0, owns=False))
    with pytest.raises(ValueError, match="has 1 dimensions"):
        obj.eval_grid(ax, out=DeviceArray(4096, (2 ** d,), 0, owns=False))
    with pytest.raises(ValueError, match="DeviceArray"):
        obj.eval_grid(ax, out=np.empty((2,) * d))


def test_the_library_exports_the_entry_points():
    lib = _lib.load()
    for name in ("pcx_spline_eval_tensor_grid", "pcx_spline_eval_tensor_grid_dev", "pcx_slider_eval_tensor_grid",
                 "pcx_slider_eval_tensor_grid_dev"):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == (6 if name.endswith("_dev") else 5)
