"""The planner of tensor-product grid evaluation (csrc/grid_plan.h) on a CPU, and the argument checks of ``eval_grid``
that need no device.

tests/host/grid_plan_main.cpp is compiled with hipcc under the address and undefined-behaviour sanitizers (host side)
and run once as a child process over every dense case of tests/golden/g29_eval_grid.npz plus shapes at the limits
(d = 16, n = 1, m = 1 everywhere, n = 4096).  Asserted:

1. W_k equals a NumPy restatement of the reference's rule (barycentric.py:941-947: one-hot within 1e-14 of a node, else
   w / diff / np.sum(w / diff)) to 1 ulp; one-hot rows are exactly one-hot, at the FIRST matching node, and the plan's
   ``hot`` column says so; rows sum to 1 within 4 n ulp;
2. the order is ascending m_k / n_k, compared in integers, ties to the higher dimension first; each pass carries the
   outer / inner sizes of the tensor as the passes before it left it; the reported intermediate size is the maximum
   over the passes that are not the last;
3. the tensor-train chain runs from the side with the smaller largest intermediate;
4. an empty axis is PCX_ERR_INVALID and names the dimension; the sanitizers report nothing.
No GPU is used."""
import json
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import golden
import generate_golden_eval_grid as G

from pychebyshev_amd import ChebyshevApproximation, ChebyshevTT, _build
from pychebyshev_amd.barycentric import chebyshev_nodes, compute_barycentric_weights
from pychebyshev_amd.device import DeviceArray

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


def _axis(rng, nodes, lo, hi, m):
    """interior points, both ends, exact nodes, a point 5e-15 from a node, a repeat; shuffled"""
    n = nodes.size
    feats = [lo, hi, nodes[0], nodes[n // 2], nodes[(n // 3) % n] + 5e-15, 0.3 * lo + 0.7 * hi, 0.3 * lo + 0.7 * hi]
    ax = np.array((feats + list(rng.uniform(lo, hi, max(0, m - len(feats)))))[:m])
    return ax[rng.permutation(m)]


def _cases():
    """id -> (n, m, nodes per dim, weights per dim, axes per dim)"""
    g = golden("g29_eval_grid")
    out = {}
    for i in range(len(G.DENSE)):
        n = [int(v) for v in g[f"d{i}_n"]]
        dom = g[f"d{i}_domain"]
        nodes = [chebyshev_nodes(dom[k][0], dom[k][1], n[k]) for k in range(len(n))]
        axes = [g[f"d{i}_ax{k}"] for k in range(len(n))]
        out[G.case_id(i)] = (n, [a.size for a in axes], nodes, [compute_barycentric_weights(x) for x in nodes], axes)
    rng = np.random.default_rng(29)
    extra = {"d16": ([2, 3] * 8, [3, 2, 1, 4] * 4), "n1": ([1, 1, 5], [4, 1, 7]), "m1": ([3, 9, 4, 6], [1, 1, 1, 1]),
             "n4096": ([4096, 3], [5, 9]), "ties": ([4, 8, 2, 6], [6, 12, 3, 9]), "shrink": ([16, 16, 16], [4, 40, 16])}
    for name, (n, m) in extra.items():
        nodes = [chebyshev_nodes(-1.0 - k, 2.0 + k, nk) for k, nk in enumerate(n)]
        wts = [compute_barycentric_weights(x) if x.size <= 64 else (-1.0) ** np.arange(x.size) *
               np.sin(np.pi * (2 * np.arange(x.size)[::-1] + 1) / (2 * x.size)) for x in nodes]
        axes = [_axis(rng, x, -1.0 - k, 2.0 + k, mk) for k, (x, mk) in enumerate(zip(nodes, m))]
        out[name] = (n, m, nodes, wts, axes)
    return out


CASES = _cases()
TT_CASES = {"left": ([5, 6, 7, 8], [1, 3, 4, 2, 1]), "right": ([8, 7, 6, 5], [1, 2, 4, 9, 1]), "tie": ([4, 4], [1, 3, 1]),
            "d1": ([9], [1, 1]), "one": ([1, 1, 1], [1, 2, 2, 1]), "wide": ([30, 2, 2, 30], [1, 2, 16, 2, 1])}


def _hex(values):
    return " ".join(float(v).hex() for v in np.asarray(values, dtype=float).ravel())


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """(grid records by id, TT records by id, bad-case records) from ONE sanitized child."""
    tmp = tmp_path_factory.mktemp("grid_plan")
    exe, src = str(tmp / "grid_plan_main"), str(tmp / "cases.txt")
    cmd = [_hipcc()] + SAN_FLAGS + ["-I", _build.CSRC, "-o", exe, os.path.join(HERE, "host", "grid_plan_main.cpp")]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, "hipcc failed:\n" + res.stdout
    lines = []
    for n, m, nodes, wts, axes in CASES.values():
        lines.append(" ".join(["G", str(len(n)), *map(str, n), *map(str, m), _hex(np.concatenate(nodes)), _hex(np.concatenate(wts)),
                               _hex(np.concatenate(axes))]))
    for m, r in TT_CASES.values():
        lines.append(" ".join(["T", str(len(m)), *map(str, m), *map(str, r)]))
    bad = ["G 2 3 4 5 0 " + _hex(np.arange(7)) + " " + _hex(np.ones(7)) + " " + _hex(np.zeros(5)), "T 2 3 0 1 2 1", "T 2 3 3 2 2 1"]
    with open(src, "w") as fh:
        fh.write("\n".join(lines + bad) + "\n")
    run = subprocess.run([exe, src], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and not run.stderr, f"exit {run.returncode} (sanitizer report?)\n{run.stderr[-4000:]}"
    recs = [json.loads(line) for line in run.stdout.splitlines()]
    assert len(recs) == len(lines) + len(bad)
    ng = len(CASES)
    return (dict(zip(CASES, recs[:ng])), dict(zip(TT_CASES, recs[ng:ng + len(TT_CASES)])), recs[ng + len(TT_CASES):])


def _reference_row(x, nodes, wts):
    diff = x - nodes
    exact = np.where(np.abs(diff) < 1e-14)[0]
    if len(exact) > 0:
        row = np.zeros(nodes.size)
        row[exact[0]] = 1.0
        return row, int(exact[0])
    w_over_diff = wts / diff
    return w_over_diff / np.sum(w_over_diff), -1


@needs_hipcc
@pytest.mark.parametrize("cid", list(CASES))
def test_weight_matrices_follow_the_reference_rule(planned, cid):
    n, m, nodes, wts, axes = CASES[cid]
    rec = planned[0][cid]
    assert rec["rc"] == 0, rec
    W = np.array([float.fromhex(v) for v in rec["W"]])
    assert W.size == sum(a * b for a, b in zip(m, n)) and len(rec["hot"]) == sum(m)
    off = hoff = 0
    n_hot = 0
    for k in range(len(n)):
        Wk = W[off:off + m[k] * n[k]].reshape(m[k], n[k])
        for r, x in enumerate(axes[k]):
            want, at = _reference_row(x, nodes[k], wts[k])
            assert rec["hot"][hoff + r] == at, (cid, k, r)
            if at >= 0:
                n_hot += 1
                assert np.array_equal(Wk[r], want), f"{cid}: dimension {k} row {r} is not one-hot at the first matching node"
            else:
                assert np.all(np.abs(Wk[r] - want) <= np.spacing(np.abs(want))), f"{cid}: dimension {k} row {r} beyond 1 ulp"
            assert abs(Wk[r].sum() - 1.0) <= 4 * n[k] * np.finfo(float).eps, (cid, k, r)
        off += m[k] * n[k]
        hoff += m[k]
    if cid not in ("d0_3_to_1", "m1"):
        assert n_hot > 0, f"{cid}: the axes were meant to hold exact nodes"


@needs_hipcc
@pytest.mark.parametrize("cid", list(CASES))
def test_order_and_intermediates(planned, cid):
    n, m, *_ = CASES[cid]
    d = len(n)
    rec = planned[0][cid]
    # ascending m_k / n_k as exact fractions, ties to the higher dimension first
    want_order = sorted(range(d), key=lambda k: (Fraction(m[k], n[k]), -k))
    assert [p[0] for p in rec["passes"]] == want_order
    cur, w_off, sizes = list(n), np.concatenate([[0], np.cumsum([a * b for a, b in zip(m, n)])]), []
    for dim, outer, nk, inner, mk, woff, out_count in rec["passes"]:
        assert (outer, nk, inner, mk) == (int(np.prod(cur[:dim], dtype=np.int64)), n[dim], int(np.prod(cur[dim + 1:], dtype=np.int64)), m[dim])
        assert woff == w_off[dim] and out_count == outer * mk * inner
        cur[dim] = mk
        sizes.append(out_count)
    assert cur == list(m)
    assert rec["max_intermediate"] == max(sizes[:-1], default=0)


@needs_hipcc
def test_shrinking_dimensions_go_first(planned):
    rec = planned[0]["shrink"]                       # n = 16^3, m = (4, 40, 16): dimension 0 shrinks, 2 keeps, 1 grows
    assert [p[0] for p in rec["passes"]] == [0, 2, 1]
    assert rec["max_intermediate"] == 4 * 16 * 16
    assert [p[0] for p in planned[0]["ties"]["passes"]] == [3, 2, 1, 0]       # every ratio 3 / 2


@needs_hipcc
@pytest.mark.parametrize("tid", list(TT_CASES))
def test_tt_chain_direction(planned, tid):
    m, r = TT_CASES[tid]
    d = len(m)
    rec = planned[1][tid]
    assert rec["rc"] == 0 and rec["total"] == int(np.prod(m))

    def inter(from_right):
        mm, rr = (m[::-1], r[::-1]) if from_right else (m, r)
        run, sizes = mm[0], []
        for k in range(1, d):
            run *= mm[k]
            sizes.append(run * rr[k + 1])
        return max(sizes[:-1], default=0)
    left, right = inter(False), inter(True)
    assert rec["from_right"] == int(right < left)
    assert rec["max_intermediate"] == min(left, right)
    assert len(rec["steps"]) == d - 1
    if d > 1:
        assert rec["steps"][-1][5] == rec["total"]
        assert [s[0] for s in rec["steps"]] == (list(range(d - 2, -1, -1)) if rec["from_right"] else list(range(1, d)))
    assert {"left": 0, "right": 1, "tie": 0}.get(tid, rec["from_right"]) == rec["from_right"]


@needs_hipcc
def test_planner_rejects_empty_axes_and_bad_ranks(planned):
    g, t0, t1 = planned[2]
    assert g["rc"] == PCX_ERR_INVALID and "dimension 1" in g["error"] and "empty" in g["error"]
    assert t0["rc"] == PCX_ERR_INVALID and "dimension 1" in t0["error"]
    assert t1["rc"] == PCX_ERR_INVALID and "boundary ranks" in t1["error"]


# ---------------------------------------------------------------- Python-side argument checks (no device is touched)
def _model():
    return ChebyshevApproximation.from_values(np.arange(12.0).reshape(3, 4), 2, [[0, 1], [0, 1]], [3, 4])


def test_eval_grid_argument_errors_dense():
    c = _model()
    with pytest.raises(ValueError, match="2 entries"):
        c.eval_grid([[0.1, 0.2]])
    with pytest.raises(ValueError, match=r"axes\[1\].*dimension 1"):
        c.eval_grid([[0.1], [[0.1, 0.2], [0.3, 0.4]]])
    with pytest.raises(ValueError, match=r"axes\[0\] is empty: dimension 0"):
        c.eval_grid([[], [0.5]])
    with pytest.raises(ValueError, match="sequence of 2"):
        c.eval_grid(0.5)
    with pytest.raises(ValueError, match="derivative_order must have 2 entries"):
        c.eval_grid([[0.1], [0.2]], [1, 0, 0])
    with pytest.raises(ValueError, match="not both"):
        c.eval_grid([[0.1], [0.2]], [1, 0], derivative_id=0)
    # a wrong `out` is refused before the model goes to a device: a borrowed DeviceArray over no memory serves
    with pytest.raises(ValueError, match="at dimension 1"):
        c.eval_grid([[0.1, 0.2], [0.3, 0.4, 0.5]], out=DeviceArray(4096, (2, 4), 0, owns=False))
    with pytest.raises(ValueError, match="has 1 dimensions"):
        c.eval_grid([[0.1, 0.2], [0.3, 0.4, 0.5]], out=DeviceArray(4096, (6,), 0, owns=False))
    with pytest.raises(ValueError, match="DeviceArray"):
        c.eval_grid([[0.1, 0.2], [0.3]], out=np.empty((2, 1)))


def test_eval_grid_argument_errors_tt():
    tt = ChebyshevTT.from_coeff_cores([np.ones((1, 3, 2)), np.ones((2, 4, 1))], [[0, 1], [0, 1]])
    with pytest.raises(ValueError, match="2 entries"):
        tt.eval_grid([[0.1]])
    with pytest.raises(ValueError, match=r"axes\[1\] is empty: dimension 1"):
        tt.eval_grid([[0.1], []])
    with pytest.raises(ValueError, match=r"axes\[0\].*dimension 0"):
        tt.eval_grid([np.zeros((2, 2)), [0.1]])


def test_the_library_exports_the_entry_points():
    from pychebyshev_amd import _lib
    lib = _lib.load()
    for name in ("pcx_tensor_mode_product", "pcx_bary_eval_tensor_grid", "pcx_bary_eval_tensor_grid_dev", "pcx_tt_tensor_grid"):
        assert hasattr(lib, name)
    assert len(_lib.SIGNATURES["pcx_tensor_mode_product"][1]) == 9
