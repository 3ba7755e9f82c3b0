"""ChebyshevTT.gradient_batch / gradient (pcx_tt_grad_batch, csrc/tt_grad_kernels.h: k_tt_grad_lpp and
k_tt_grad_generic) against the long-double chain of tests/tt_chain.py.

Every column of the N x C result is held to ``Chain.value()`` (column 0) or to ``Chain.deriv`` of the column's
single-dimension spec, row by row: |got - ref| <= K eps A_row with A_row the row's amplitude and K = tt_chain.K of the
model's list (sweep 8 / 8 / 8, edge 32 / 32 / 64 for value / order 1 / order 2) -- the bound of
tests/test_gpu_tt_lane_bodies.py.  tests/test_tt_gradient_host.py shows that the forward-backward association, restated in
float64, sits where the left-to-right chain does, so the table needs no constant for it.

The degenerate shapes take the same table, no constant of their own: the two models whose every rank is 1 (one
dimension; four dimensions of rank 1) the edge K, the list tt_chain.py keeps for exactly that reason -- a model of
rank 1 does not dilute the rounding of s = (x - lo) sc - 1 (there, at RESTATEMENT_WORST; its own rank-1 model is
edge-n17-rank1) -- and the other two (n = 1 and 2 with ranks 3 and 4; d = 16 with ranks 16) the sweep K.

Worst |got - ref| / (eps A_row) measured on MI355X, value / order 1 / order 2 (K beside it):
    sweep 0.21 / 0.30 / 0.38 (8 / 8 / 8), edge 1.86 / 1.46 / 2.60 (32 / 32 / 64), golden D and F 0.14 / 0.21 / 0.29,
    derived models 0.12 / 0.34 / 0.18; one dimension 0.92 / 4.08 / 6.24 and every rank 1 2.25 / 2.50 / 3.93 (32 / 32 / 64),
    n = 1 and 2 0.40 / 0.60 / 0.91 (8 / 8 / 8), d = 16 below 0.001 (8 / 8 / 8; its rows cancel by nine orders of magnitude, so
    eps A_row is far above the rounding of the result and still orders below the result itself)."""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import ROOT, assert_parity, golden, spec_point_tol
import tt_chain as C
import tt_grad_chain as GC
from pychebyshev_amd import ChebyshevTT, DeviceArray, _lib
from pychebyshev_amd.device import is_device_array

pytestmark = pytest.mark.gpu

SWEEP = C.sweep_models()
EDGE = C.edge_models()
G22 = golden("g22_tt_transforms")
G28 = golden("g28_tt_derivatives")


def _model(b):
    return ChebyshevTT.from_coeff_cores(b.cores, b.domain, dim_order=b.order)


def _matrix(parts):
    if is_device_array(parts[0]):                          # views of one device result: one download
        assert all(p.parent is parts[0].parent for p in parts)
        whole = parts[0].parent.to_host()
        assert whole.shape[1] == 1 + sum(p.shape[1] for p in parts[1:])
        assert np.array_equal(parts[-1].to_host(), whole[:, -parts[-1].shape[1]:]) and np.array_equal(parts[0].to_host(), whole[:, 0])
        return whole
    return np.column_stack([np.asarray(p.to_host() if is_device_array(p) else p).reshape(parts[0].shape[0], -1) for p in parts])


def _check(got, ref, K, what):
    """(N, C) against [(column, family, values, amplitudes)]: each row of each column within K[family] eps A_row."""
    assert got.dtype == np.float64 and got.shape[1] == len(ref), what
    for col, family, val, amp in ref:
        r = C.ratios(got[:, col], val, amp)                # asserts an exact zero where the amplitude is zero
        worst = float(np.max(r))
        print(f"{what} column {col} ({family}): worst row {worst:.3f} eps A_row (K = {K[family]})")
        assert worst <= K[family], f"{what} column {col} ({family}): row {int(np.argmax(r))}: {worst:.3g} eps A_row > K = {K[family]}"


def _exact_zero_columns(got, b):
    d = len(b.cores)
    for k, core in enumerate(b.cores):
        u = k if b.order is None else b.order[k]
        n = core.shape[1]
        if n == 1:
            assert np.all(got[:, 1 + u] == 0.0), (k, "gradient of a one-node dimension")
        if n <= 2:
            assert np.all(got[:, 1 + d + u] == 0.0), (k, "second derivative of a dimension with at most two nodes")


def _run(b, group_K, what):
    tt = _model(b)
    parts = tt.gradient_batch(b.pts, second=True)
    d = len(b.cores)
    assert [p.shape for p in parts] == [(b.pts.shape[0],), (b.pts.shape[0], d), (b.pts.shape[0], d)]
    got = _matrix(parts)
    _check(got, GC.reference(b), group_K, what)
    _exact_zero_columns(got, b)
    return tt, got


@pytest.mark.parametrize("model", SWEEP, ids=[m.name for m in SWEEP])
def test_every_body_of_both_sweeps(model):
    """96 rows (rows 0 and 1 on the domain ends; every third model a permuted dim_order), second=True: each model's
    dimensions reach their (cap, uniform / mixed, left rank, node count) bodies of the right and the left sweep."""
    _run(C.build(model), C.K["sweep"], model.name)


@pytest.mark.parametrize("model", EDGE, ids=[m.name for m in EDGE])
def test_wave_per_row(model):
    """k_tt_grad_generic: lane loops of one, two and three trips, and the model that is generic only because n > 16."""
    b = C.build(model)
    tt, got = _run(b, C.K["edge"], model.name)
    first = _matrix(tt.gradient_batch(b.pts))
    assert np.array_equal(first, got[:, :1 + len(b.cores)])


DEGENERATE = [
    C.Model(1000, "one-dimension", 8, "uniform", (1, 1), (7,), 70),
    C.Model(1001, "one-and-two-nodes", 8, "mixed", (1, 3, 4, 1), (5, 1, 2), 70),
    C.Model(1002, "every-rank-1", 8, "mixed", (1, 1, 1, 1, 1), (4, 1, 16, 3), 70),
    C.Model(1003, "d16-rank16-n2", 16, "uniform", (1,) + (16,) * 15 + (1,), (2,) * 16, 65),
]


@pytest.mark.parametrize("model", DEGENERATE, ids=[m.name for m in DEGENERATE])
def test_degenerate_shapes(model):
    """d = 1 (no R is stored); n = 1 and n = 2 (exact zeros); every rank 1; d = 16 with ranks 16: the 128 KiB LDS launch."""
    b = C.build(model)
    tt, got = _run(b, C.K["edge" if max(model.ranks) == 1 else "sweep"], model.name)
    assert C.rank_cap(model) != 0
    if model.name == "d16-rank16-n2":
        assert (sum(model.ranks[1:-1]) + max(model.ranks)) * 64 * 8 == 128 * 1024
        # the LDS limit of an instantiation is lifted at its first large launch only: a second one gives the same bits
        assert np.array_equal(_matrix(tt.gradient_batch(b.pts, second=True)), got)
    first = _matrix(tt.gradient_batch(b.pts))
    assert np.array_equal(first, got[:, :1 + len(model.n)])


def test_bit_for_bit():
    """tail_model(): a batch of N rows equals its rows sent one at a time; the host- and the device-pointer entry agree;
    out= is the returned arrays; gradient(point) is row 0; second=True's first 1 + d columns are second=False's."""
    b = C.build(C.tail_model())
    tt = _model(b)
    d = len(b.cores)
    rows = [_matrix(tt.gradient_batch(b.pts[r:r + 1], second=True))[0] for r in range(b.pts.shape[0])]
    for N in (1, 63, 64, 65, 129):
        pts = np.ascontiguousarray(b.pts[:N])
        parts = tt.gradient_batch(pts, second=True)
        got = _matrix(parts)
        assert got.shape == (N, 1 + 2 * d)
        assert np.array_equal(got, np.array(rows[:N])), f"N = {N}: rows alone"
        assert parts[0].base is parts[1].base is parts[2].base and parts[0].base.shape == (N, 1 + 2 * d)
        dev = tt.gradient_batch(DeviceArray.from_host(pts), second=True)
        assert all(is_device_array(p) for p in dev) and [p.shape for p in dev] == [(N,), (N, d), (N, d)]
        assert np.array_equal(_matrix(dev), got), f"N = {N}: device entry"
        assert np.array_equal(_matrix(tt.gradient_batch(pts)), got[:, :1 + d]), f"N = {N}: second=False"
        assert np.array_equal(_matrix(tt.gradient_batch(DeviceArray.from_host(pts))), got[:, :1 + d]), f"N = {N}: second=False, device"
        out = np.full((N, 1 + 2 * d), np.nan)
        views = tt.gradient_batch(pts, second=True, out=out)
        assert np.array_equal(out, got) and all(np.shares_memory(v, out) for v in views)
        dout = DeviceArray.empty((N, 1 + 2 * d))
        dviews = tt.gradient_batch(pts, second=True, out=dout)
        assert np.array_equal(dout.to_host(), got) and np.array_equal(_matrix(dviews), got)
    value, grad, diag = tt.gradient(b.pts[0], second=True)
    assert isinstance(value, float) and grad.shape == diag.shape == (d,)
    assert np.array_equal(np.concatenate([[value], grad, diag]), rows[0])
    value, grad = tt.gradient(b.pts[0])
    assert np.array_equal(np.concatenate([[value], grad]), rows[0][:1 + d])
    with pytest.raises(ValueError, match="does not match the result"):
        tt.gradient_batch(b.pts, out=np.empty((b.pts.shape[0], 1 + 2 * d)))
    with pytest.raises(ValueError, match=r"points must have shape"):
        tt.gradient_batch(b.pts[:, :-1])


def _golden(tag):
    cores, k = [], 0
    while f"{tag}_core{k}" in G22.files:
        cores.append(G22[f"{tag}_core{k}"])
        k += 1
    pts = np.concatenate([G28[f"{tag}_s{i}_pts"] for i in range(3)])[:130]
    return C.Built(None, cores, G22[f"{tag}_domain"].tolist(), G22[f"{tag}_order"].tolist(), None, np.ascontiguousarray(pts))


@pytest.mark.parametrize("tag, group", [("D", "sweep"), ("F", "edge")])
def test_against_the_chain_per_spec_kernel(tag, group):
    """D: a storage order and mixed node counts on the lane-per-row form; F: the wave-per-row form.  gradient_batch and
    eval_multi_batch(method="analytic") with the same 2 d + 1 specs both stay within K of the long-double chain (the
    association differs: no equality of bits); differentiate(e_u).eval_batch is a third route for one u."""
    b = _golden(tag)
    tt, got = _run(b, C.K[group], f"golden {tag}")
    d = len(b.cores)
    lane_image = max(tt.tt_ranks) <= 16 and max(c.shape[1] for c in b.cores) <= C.MAX_N
    assert lane_image == (group == "sweep")
    specs = [spec for _, spec, _ in GC.columns(d)]
    per_spec = tt.eval_multi_batch(b.pts, specs, method="analytic")
    _check(per_spec, GC.reference(b), C.K[group], f"golden {tag} eval_multi_batch")
    u = d - 1
    spec = specs[1 + u]
    third = tt.differentiate(spec).eval_batch(b.pts)
    assert_parity(third, got[:, 1 + u], tol=1e-12, point_tol=spec_point_tol(spec), what=f"tt differentiate vs gradient_batch {tag} {spec}")


def test_derived_models_are_ordinary_handles():
    """A differentiated, a sliced, an extruded, a summed and a reordered model: gradient_batch on each against the
    long-double chain of the model's own cores (the row bound is the sweep's; the cores are what the transform left)."""
    src = next(m for m in SWEEP if m.cap == 8 and m.mode == "uniform" and m.n[0] == 6)
    b = C.build(src._replace(rows=70))
    tt = _model(b)
    d = len(b.cores)
    derived = {
        "differentiate": tt.differentiate([1] + [0] * (d - 1)),
        "slice": tt.slice([(1, float(b.udom[1][0] + 0.25 * (b.udom[1][1] - b.udom[1][0])))]),
        "extrude": tt.extrude([(1, [-1.0, 2.0], 5)]),
        "sum": tt + tt * 0.5,
        "reorder": tt.reorder(list(range(d))[::-1]),
    }
    rng = np.random.default_rng(77)
    for name, m in derived.items():
        dom = [m.domain[m.dim_order.index(u)] for u in range(m.num_dimensions)]           # user frame
        pts = np.column_stack([rng.uniform(lo, hi, 70) for lo, hi in dom])
        built = C.Built(None, m._coeff_cores, [list(map(float, ab)) for ab in m.domain], list(m.dim_order), None, pts)
        got = _matrix(m.gradient_batch(pts, second=True))
        _check(got, GC.reference(built), C.K["sweep"], f"derived {name}")
    assert derived["reorder"].dim_order != list(range(d))


def test_c_abi_argument_errors():
    b = C.build(C.tail_model())
    tt = _model(b)
    t = tt._dev()
    lib = t.lib
    invalid = _lib.PCX_ERR_INVALID
    d = len(b.cores)
    pts = np.ascontiguousarray(b.pts[:4])
    out = np.full((4, 1 + 2 * d), 7.0)
    none_f64 = ctypes.POINTER(ctypes.c_double)()
    assert lib.pcx_tt_grad_batch(None, _lib.p_f64(pts), 4, 1, _lib.p_f64(out)) == invalid
    assert lib.pcx_tt_grad_batch(t.handle, _lib.p_f64(pts), 4, 2, _lib.p_f64(out)) == invalid
    assert "second" in lib.pcx_last_error().decode()
    assert lib.pcx_tt_grad_batch(t.handle, _lib.p_f64(pts), 4, -1, _lib.p_f64(out)) == invalid
    assert lib.pcx_tt_grad_batch(t.handle, _lib.p_f64(pts), -1, 1, _lib.p_f64(out)) == invalid
    assert lib.pcx_tt_grad_batch(t.handle, none_f64, 4, 1, _lib.p_f64(out)) == invalid
    assert lib.pcx_tt_grad_batch(t.handle, _lib.p_f64(pts), 4, 1, none_f64) == invalid
    assert lib.pcx_tt_grad_batch(t.handle, _lib.p_f64(pts), 0, 2, _lib.p_f64(out)) == invalid
    assert lib.pcx_tt_grad_batch_dev(None, None, 4, 1, None, None) == invalid
    assert lib.pcx_tt_grad_batch_dev(t.handle, None, 4, 1, None, None) == invalid
    assert lib.pcx_tt_grad_batch_dev(t.handle, None, 0, 2, None, None) == invalid
    assert lib.pcx_tt_grad_batch_dev(t.handle, None, -1, 0, None, None) == invalid
    assert np.all(out == 7.0)                               # nothing was launched
    assert lib.pcx_tt_grad_batch(t.handle, _lib.p_f64(pts), 0, 1, _lib.p_f64(out)) == 0
    assert lib.pcx_tt_grad_batch(t.handle, none_f64, 0, 0, none_f64) == 0
    assert lib.pcx_tt_grad_batch_dev(t.handle, None, 0, 1, None, None) == 0
    assert np.all(out == 7.0)
    empty = tt.gradient_batch(np.zeros((0, d)), second=True)
    assert [p.shape for p in empty] == [(0,), (0, d), (0, d)]
    assert lib.pcx_tt_grad_batch(t.handle, _lib.p_f64(pts), 4, 1, _lib.p_f64(out)) == 0
    assert np.array_equal(out, _matrix(tt.gradient_batch(pts, second=True)))


def test_torch_tensor_in_device_arrays_out():
    """A ROCm PyTorch tensor as the batch, in a child process (torch brings its own copy of the HIP runtime)."""
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        import numpy as np
        import torch
        from pychebyshev_amd import ChebyshevTT
        from pychebyshev_amd.device import DeviceArray, is_device_array
        g = np.load({os.path.join(ROOT, "tests", "golden", "g22_tt_transforms.npz")!r})
        v = np.load({os.path.join(ROOT, "tests", "golden", "g28_tt_derivatives.npz")!r})
        tt = ChebyshevTT.from_coeff_cores([g[f"D_core{{k}}"] for k in range(4)], g["D_domain"].tolist(),
                                          dim_order=g["D_order"].tolist())
        pts = v["D_s0_pts"]
        t = torch.as_tensor(pts, device="cuda:0") * 1.0
        value, grad, diag = tt.gradient_batch(t, second=True)
        assert all(is_device_array(p) and isinstance(p, DeviceArray) for p in (value, grad, diag))
        assert value.shape == (48,) and grad.shape == diag.shape == (48, 4)
        hv, hg, hd = tt.gradient_batch(pts, second=True)
        back = torch.as_tensor(grad, device="cuda:0")
        assert back.data_ptr() == grad.ptr and tuple(back.stride()) == (9, 1)
        assert np.array_equal(back.cpu().numpy(), hg)
        assert np.array_equal(torch.as_tensor(value, device="cuda:0").cpu().numpy(), hv)
        assert np.array_equal(diag.to_host(), hd)
        out = torch.full((48, 9), float("nan"), dtype=torch.float64, device="cuda:0")
        tt.gradient_batch(t, second=True, out=out)
        assert np.array_equal(out.cpu().numpy(), np.column_stack([hv, hg, hd]))
        print("torch-interop-ok")
    """)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "torch-interop-ok" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
