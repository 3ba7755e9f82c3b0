"""The launch planner of the barycentric handle (csrc/bary_plan.h, csrc/pcx_bary_plan.hip) on a CPU.

tests/host/bary_plan_main.cpp is compiled with hipcc together with the planner unit, under the address and
undefined-behaviour sanitizers (host side), and run once as a child process over every case of
tests/golden/g27_bary_plans.npz -- plan signatures recorded on an MI355X before the planner was split from
pcx_bary_create -- and a few more shapes at the limits (d = 16, one node, 4096 nodes).  Asserted:

1. the signature the planner gives (what pcx_bary_kernel_info, _grid_info, _tail_info[1..3] and _set_kernel report,
   through the functions those entry points call) equals the recorded one field for field; the shape no kernel covers
   fails with the recorded code and text;
2. the tables' structure: every row-code field below tail_base, every k-code field at most rows - 1 - tail_base, rows at
   or beyond M and columns at or beyond K on the all-ones row, row offsets = row codes x 16 nt 8, and the lengths
   pcx_bary_create uploads;
3. the sanitizers report nothing.
No GPU is used."""
import json
import os
import subprocess

import numpy as np
import pytest

import generate_golden_bary_plans as G

from pychebyshev_amd import _build

HERE = os.path.dirname(os.path.abspath(__file__))
SAN_FLAGS = ["--offload-arch=gfx950", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
             "-fno-sanitize-recover=undefined"]
EXTRA_SHAPES = [(2,) * 16, (1,), (1, 1, 1), (16, 4096), (4096, 2), (5, 255), (3, 7, 11, 13)]
CODE_FIELDS = 4


def _hipcc():
    try:
        return _build.hipcc_path()
    except RuntimeError:
        return None


pytestmark = pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")


def _line(shape, env):
    sw = [int(env.get("PCX_BARY_SEED", "1") != "0"), int(env.get("PCX_BARY_TAIL", "1")), int(env.get("PCX_BARY_SQ", "1") != "0"),
          int(env.get("PCX_BARY_GRID", "1")), int(env.get("PCX_BARY_GRID_PROD", "1") != "0")]
    return " ".join(map(str, [len(shape), *shape, *sw]))


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """id -> (shape, the program's record), from one sanitized child over all cases."""
    tmp = tmp_path_factory.mktemp("bary_plan")
    exe, src = str(tmp / "bary_plan_main"), str(tmp / "cases.txt")
    cmd = [_hipcc()] + SAN_FLAGS + ["-I", _build.CSRC, "-o", exe, os.path.join(HERE, "host", "bary_plan_main.cpp"),
                                    os.path.join(_build.CSRC, "pcx_bary_plan.hip")]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, "hipcc failed:\n" + res.stdout
    cases = [(G.case_id(c), tuple(c["shape"]), c["env"]) for c in G.CASES]
    cases += [("x".join(map(str, s)), s, {}) for s in EXTRA_SHAPES]
    with open(src, "w") as fh:
        fh.write("\n".join(_line(s, e) for _, s, e in cases) + "\n")
    run = subprocess.run([exe, "--tables", src], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and not run.stderr, f"exit {run.returncode} (sanitizer report?)\n{run.stderr[-4000:]}"
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases)
    return {cid: (shape, json.loads(line)) for (cid, shape, _), line in zip(cases, lines)}


@pytest.fixture(scope="module")
def recorded():
    return G.load()


def test_every_case_of_the_generator_is_in_the_fixture(recorded):
    assert sorted(recorded) == sorted(G.case_id(c) for c in G.CASES)


@pytest.mark.parametrize("cid", [G.case_id(c) for c in G.CASES])
def test_planner_gives_the_recorded_signature(planned, recorded, cid):
    want, (_, got) = recorded[cid], planned[cid]
    assert got["rc"] == want["rc"]
    if want["rc"] != 0:
        assert got["error"] == want["error"]
        return
    for key in ("kernel_info", "grid_info", "tail_info"):
        assert got[key] == want[key], key
    assert [bool(v) for v in got["set_kernel"]] == want["set_kernel"]


def _fields(words):
    """(..., 4) array of the 8-bit fields of code words."""
    w = np.asarray(words, dtype=np.uint32)
    return np.stack([(w >> (8 * i)) & 255 for i in range(CODE_FIELDS)], axis=-1).astype(np.int64)


def _rows_in_order(lane_ordered):
    """Undo the lane order: entry (4 t + g) * 4 + j holds row 16 t + g + 4 j."""
    v = np.asarray(lane_ordered, dtype=np.uint32).reshape(-1, 4, 4)          # [t][g][j]
    return v.transpose(0, 2, 1).reshape(-1)                                   # [t][j][g] -> row 16 t + 4 j + g


def _table(rec, name):
    t = rec["tables"][name]
    assert len(t["data"]) == t["len"]
    return np.asarray(t["data"])


def test_tables_keep_their_structure(planned):
    checked = 0
    for cid, (shape, rec) in planned.items():
        if rec["rc"] != 0:
            continue
        p, tabs, d, sum_n = rec["plan"], rec["tables"], len(shape), sum(shape)
        rowcode_form = p["mfma_ok"] and not p["grid_ok"] and not p["kfold_ok"]
        want = set()
        if p["small_nlp"]:
            want.add("snodes")
            assert tabs["snodes"]["len"] == sum_n
        if p["grid_ok"] or p["kfold_ok"]:
            want.add("gsnodes")
            assert tabs["gsnodes"]["len"] == sum_n + 16
            scales = _table(rec, "gsnodes")[sum_n:sum_n + d]
            assert np.all(np.frexp(scales)[0] == 0.5), f"{cid}: scales are powers of two"
        if p["mfma_ok"]:
            want |= {"rowcode", "kcode"}
            if p["wide"]:
                want |= {"rowcode_hi", "kcode_hi"}
            # the row offsets serve the pipelined loop of the narrow row-code kernel only
            if rowcode_form and not p["wide"] and p["plan.KS"] >= 12:
                want |= {"rowoff1", "rowoff2"}
            if p["g0_ok"]:
                want.add("rowcode_g0")
        assert set(tabs) == want, cid
        if not p["mfma_ok"]:
            continue
        checked += 1
        M, K, MT, KS, R, split = (p["plan." + k] for k in ("M", "K", "MT", "KS", "R", "split"))
        tail_base, rows = p["plan.tail_base"], p["plan.rows"]
        ones_h, ones_t = tail_base - 1, rows - 1 - tail_base
        assert MT == (M + 15) // 16 and 4 * KS >= K - R and rows == sum_n + 2 and tail_base == sum(shape[:split]) + 1, cid
        offs = np.concatenate([[0], np.cumsum(shape)])
        for word, name in enumerate(["rowcode", "rowcode_hi"][:2 if p["wide"] else 1]):
            f = _fields(_rows_in_order(_table(rec, name)))
            assert f.shape == (MT * 16, CODE_FIELDS), cid
            assert f.max() < tail_base, f"{cid}: a row-code field at or beyond tail_base"
            assert np.all(f[M:] == ones_h), f"{cid}: rows beyond M are not all ones"
            idx = np.array(np.unravel_index(np.arange(M), shape[:split])).T.reshape(M, split) if split else np.zeros((M, 0), int)
            for i in range(CODE_FIELDS):
                k = CODE_FIELDS * word + i
                assert np.array_equal(f[:M, i], offs[k] + idx[:, k] if k < split else np.full(M, ones_h)), (cid, name, i)
        for word, name in enumerate(["kcode", "kcode_hi"][:2 if p["wide"] else 1]):
            f = _fields(_table(rec, name))
            assert f.shape == (4 * KS + R, CODE_FIELDS), cid
            assert f.max() <= ones_t, f"{cid}: a k-code field beyond the tail part"
            col = np.concatenate([R + np.arange(4 * KS), np.arange(R)])
            assert np.all(f[col >= K] == ones_t), f"{cid}: columns beyond K are not all ones"
            live = col < K
            idx = np.array(np.unravel_index(col[live], shape[split:])).T
            for i in range(CODE_FIELDS):
                k = split + CODE_FIELDS * word + i
                want_f = offs[k] - offs[split] + idx[:, k - split] if k < d else np.full(live.sum(), ones_t)
                assert np.array_equal(f[live, i], want_f), (cid, name, i)
        if "rowoff1" in tabs:
            code = _fields(_table(rec, "rowcode")).reshape(-1, 4, CODE_FIELDS)                   # [q][j][field]
            for nt in (1, 2):
                sc = 16 * nt * 8
                off = _table(rec, f"rowoff{nt}").astype(np.int64).reshape(-1, 2, 4)             # [q][half][j]
                assert off.shape[0] == MT * 4, cid
                for half in (0, 1):
                    assert np.array_equal(off[:, half, :], code[:, :, 2 * half] * sc | (code[:, :, 2 * half + 1] * sc) << 16), (cid, nt)
        if p["g0_ok"]:
            n0, tps, M1 = shape[0], p["g0_tps"], M // shape[0]
            f = _fields(_rows_in_order(_table(rec, "rowcode_g0"))).reshape(n0, tps * 16, CODE_FIELDS)
            assert tps == (M1 + 15) // 16 and p["g0_nf"] == max(2, split - 1), cid
            assert f.max() < tail_base and np.all(f[:, M1:] == ones_h), cid
            idx = np.array(np.unravel_index(np.arange(M1), shape[1:split])).T
            for i in range(CODE_FIELDS):
                want_f = offs[i + 1] + idx[:, i] if i + 1 < split else np.full(M1, ones_h)
                assert np.all(f[:, :M1, i] == want_f), (cid, i)
    assert checked >= 50
