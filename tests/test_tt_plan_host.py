"""The planner of the tensor-train handle (csrc/tt_plan.h, csrc/pcx_tt_plan.hip) on a CPU.

tests/host/tt_plan_main.cpp is compiled with hipcc together with the planner unit, under the address and
undefined-behaviour sanitizers (host side), and run once as a child process over one or more tiny models per branch of
handle creation (at most 10^5 core entries each) and every validation error.  Asserted:

1. the plan -- every scalar and array of TTPlan, the five LDS sizes, tt_auto_variant for every requested variant with all
   images uploaded and with the lane-per-point image missing -- equals the independent rule mirror tests/tt_plan_rule.py
   field for field; a refused model fails with the mirror's code and text;
2. the host-built tables (padded last core, 4x4x4 image, lane-per-point image and table) equal their stated layouts,
   computed in numpy from the same seeded cores;
3. the child's stderr is empty and its exit status 0: the sanitizers report nothing.
No GPU is used."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import tt_plan_rule as R

from pychebyshev_amd import _build

HERE = os.path.dirname(os.path.abspath(__file__))
SAN_FLAGS = ["--offload-arch=gfx950", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
             "-fno-sanitize-recover=undefined"]
KIB = 1024


def _hipcc():
    try:
        return _build.hipcc_path()
    except RuntimeError:
        return None


pytestmark = pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")


def _m(name, n, ranks, order=None, d=None, bad=0):
    """one model: `d` is what the planner is told (default: the arrays' length), `bad` as tt_plan_main.cpp reads it"""
    return {"id": name, "n": list(n), "ranks": list(ranks), "order": list(order) if order else list(range(len(n))),
            "d": len(n) if d is None else d, "bad": bad}


def _u(d, n, r):
    return [n] * d, [1] + [r] * (d - 1) + [1]


def _d4_bytes(d, n=16, RA=3, NMP=4):
    """LDS of the 4x4x4 form for d dimensions of n nodes at ranks 9 .. 12, from the rule as the issue states it"""
    total = -(-n // 4) * 16 * NMP + (d - 2) * n * RA * 16 * NMP + 4 * RA * n
    return (total + 2 * 16 * d + 4 * (16 * d + 96)) * 8


D4_EDGE = max(d for d in range(3, 17) if _d4_bytes(d) <= 72 * KIB)       # rank 12, n = 16: the last d inside 72 KiB

MODELS = (
    [_m("d1", [7], [1, 1]), _m("d16_n2", *_u(16, 2, 2))]
    + [_m(f"rmax{r}", *_u(3, 5, r)) for r in (1, 4, 5, 8, 9, 12, 13, 15, 16, 17, 32, 33, 64, 65)]
    + [_m("generic_lds_over", [5, 5], [1, 2558, 1]), _m("generic_lds_under", [4, 4], [1, 2558, 1]), _m("rmax4097", [1, 1], [1, 4097, 1])]
    + [_m(f"nmax{n}", *_u(3, n, 3)) for n in (1, 16, 17, 32, 33)]
    + [_m("mixed_nodes", [5, 9, 4, 7], [1, 3, 5, 2, 1]), _m("mixed_order", [5, 9, 4, 7], [1, 3, 5, 2, 1], order=[2, 0, 3, 1]),
       _m("mixed_r20", [3, 18, 6], [1, 20, 7, 1], order=[1, 2, 0]), _m("no_dim_order", [6, 3, 6], [1, 4, 2, 1], bad=5),
       _m("last_core_past_16k", [4, 600], [1, 3, 1])]
    + [_m("r12_n32_d3", *_u(3, 32, 12)), _m("r12_n32_d5", *_u(5, 32, 12))]
    + [_m("r12_n16_d4_in", *_u(D4_EDGE, 16, 12)), _m("r12_n16_d4_out", *_u(D4_EDGE + 1, 16, 12))]
    + [_m("r8_n11", *_u(5, 11, 8)), _m("r12_n12", *_u(4, 12, 12))]
    # every validation error, in the order the checks run
    + [_m("d0", [4], [1, 1], d=0), _m("d17", [2] * 16, [1] + [2] * 15 + [1], d=17)]
    + [_m(f"null{b}", [4, 4], [1, 3, 1], bad=b) for b in (1, 2, 3, 4)]
    + [_m("boundary_left", [4, 4], [2, 3, 1]), _m("boundary_right", [4, 4], [1, 3, 2]),
       _m("n_zero", [4, 0], [1, 3, 1]), _m("n_4097", [4097, 4], [1, 3, 1]), _m("rank_zero", [4, 4, 4], [1, 0, 3, 1]),
       _m("lo_is_hi", [4, 4], [1, 3, 1], bad=11), _m("order_repeats", [4, 4], [1, 3, 1], order=[1, 1]),
       _m("order_past_d", [4, 4], [1, 3, 1], order=[0, 2]), _m("order_negative", [4, 4], [1, 3, 1], order=[-1, 0]),
       _m("rank_before_domain", [4, 4], [1, 0, 1], bad=10), _m("domain_before_order", [4, 4], [1, 3, 1], order=[1, 1], bad=10)]
)
IDS = [m["id"] for m in MODELS]


def _seed(m):
    return int.from_bytes(hashlib.sha256(m["id"].encode()).digest()[:4], "little")


def _line(m):
    return " ".join(map(str, [m["d"], len(m["n"]), *m["n"], *m["ranks"], *m["order"], _seed(m), m["bad"]]))


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """id -> the program's record, from one sanitized child over all models"""
    tmp = tmp_path_factory.mktemp("tt_plan")
    exe, src = str(tmp / "tt_plan_main"), str(tmp / "models.txt")
    cmd = [_hipcc()] + SAN_FLAGS + ["-I", _build.CSRC, "-o", exe, os.path.join(HERE, "host", "tt_plan_main.cpp"),
                                    os.path.join(_build.CSRC, "pcx_tt_plan.hip")]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, "hipcc failed:\n" + res.stdout
    with open(src, "w") as fh:
        fh.write("\n".join(_line(m) for m in MODELS) + "\n")
    run = subprocess.run([exe, src], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and not run.stderr, f"exit {run.returncode} (sanitizer report?)\n{run.stderr[-4000:]}"
    lines = run.stdout.splitlines()
    assert len(lines) == len(MODELS)
    return {m["id"]: json.loads(line) for m, line in zip(MODELS, lines)}


def _mirror(m):
    k = len(m["n"])
    lo = [-1.0 - 0.125 * i for i in range(k)]
    hi = [1.0 + 0.25 * i for i in range(k)]
    if m["bad"] >= 10:
        hi[m["bad"] - 10] = lo[m["bad"] - 10]
    arrays = [None if m["bad"] == b else a for b, a in ((1, m["n"]), (2, m["ranks"]), (3, lo), (4, hi), (5, m["order"]))]
    return R.plan(m["d"], *arrays)


@pytest.mark.parametrize("m", MODELS, ids=IDS)
def test_plan_equals_the_rule_mirror(planned, m):
    got, want = planned[m["id"]], _mirror(m)
    assert got["rc"] == want["rc"]
    if want["rc"] != 0:
        assert got["error"] == want["error"]
        return
    p = want["plan"]
    assert sorted(got["plan"]) == sorted(p)
    for key in p:
        assert got["plan"][key] == p[key], key
    assert got["lds"] == R.lds(p)
    assert got["auto_all"] == [R.auto_variant(p, v) for v in range(5)]
    assert got["auto_nolpp"] == [R.auto_variant(p, v, lpp=False) for v in range(5)]


def _same(table, want):
    want = np.ascontiguousarray(want, dtype=np.float64)
    if table["len"] != want.size:
        return False
    if "data" in table:
        return np.array_equal(np.asarray(table["data"], dtype=np.float64), want)
    return table["sha256"] == hashlib.sha256(want.tobytes()).hexdigest()


@pytest.mark.parametrize("m", [m for m in MODELS if _mirror(m)["rc"] == 0], ids=lambda m: m["id"])
def test_tables_equal_their_layouts(planned, m):
    tabs, p = planned[m["id"]]["tables"], _mirror(m)["plan"]
    c = R.cores(_seed(m), p["core_total"])
    want = set()
    if not p["generic"]:
        want.add("last")
        assert _same(tabs["last"], R.last_core(p, c))
    if p["d4RA"]:
        want.add("d4")
        assert tabs["d4"]["len"] == p["d4plan.total"] and _same(tabs["d4"], R.d4_image(p, c))
    if p["lppCap"]:
        want |= {"lpp", "lpp_tab"}
        assert tabs["lpp"]["len"] == p["core_total"] + 64 and _same(tabs["lpp"], R.lpp_image(p, c))
        assert tabs["lpp_tab"] == R.lpp_table(p)
    assert set(tabs) == want


def test_the_models_reach_the_branches_they_are_named_for(planned):
    """on the program's own output, so that a mirror and a planner wrong in the same way cannot pass every case above"""
    plan = {cid: r["plan"] for cid, r in planned.items() if r["rc"] == 0}
    auto = {cid: r["auto_all"][0] for cid, r in planned.items() if r["rc"] == 0}
    assert [plan[f"rmax{r}"]["cls"] for r in (16, 17, 32, 33, 64)] == [0, 1, 1, 2, 2]
    assert [plan[f"rmax{r}"]["lppCap"] for r in (8, 9, 12, 13, 16, 17)] == [8, 12, 12, 16, 16, 0]
    assert [auto[f"rmax{r}"] for r in (1, 12, 13, 15, 16, 17, 64, 65)] == [4, 4, 4, 4, 1, 1, 1, 0]
    assert plan["rmax65"]["generic"] and plan["generic_lds_under"]["generic"]
    assert planned["generic_lds_over"]["rc"] == planned["rmax4097"]["rc"] == R.UNSUPPORTED
    assert plan["r12_n32_d3"]["wR"] == 12 and plan["r12_n32_d5"]["wR"] == 0 and plan["r12_n32_d5"]["wplan.total"] * 8 > 96 * KIB
    assert auto["r12_n32_d3"] == 2 and auto["r12_n32_d5"] == 1
    assert plan["r12_n16_d4_in"]["d4RA"] == 3 and plan["r12_n16_d4_out"]["d4RA"] == 0
    assert plan["r8_n11"]["d4_preferred"] == 1 and planned["r8_n11"]["auto_nolpp"][0] == 3
    assert plan["r12_n12"]["d4_preferred"] == 0 and planned["r12_n12"]["auto_nolpp"][0] == 2
    assert [plan[f"nmax{n}"]["wR"] for n in (16, 17, 32, 33)] == [4, 4, 4, 0]
    assert [plan[f"nmax{n}"]["d4RA"] for n in (16, 17)] == [1, 0] and [plan[f"nmax{n}"]["lppCap"] for n in (16, 17)] == [8, 0]
    assert plan["mixed_nodes"]["lpp_nodes"] == 0 and plan["nmax16"]["lpp_nodes"] == 16
    assert plan["mixed_order"]["col"] == [2, 0, 3, 1] and plan["no_dim_order"]["col"] == [0, 1, 2]
    assert plan["last_core_past_16k"]["last_lds_doubles"] == 0 and plan["nmax33"]["last_lds_doubles"] == 4 * 33
    refused = [planned[m["id"]]["error"] for m in MODELS if planned[m["id"]]["rc"] == R.INVALID]
    # d = 0 and 17, NULL array, boundary ranks, n / rank at dims 0 and 1, domain at dims 0 and 1, dim_order
    assert len(set(refused)) == 9
