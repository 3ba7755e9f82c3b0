"""ChebyshevTT.hessian_batch / hessian (pcx_tt_hess_batch, csrc/tt_hess_kernels.h: k_tt_hess_lpp and
k_tt_hess_generic) against the long-double chain of tests/tt_chain.py.

Every column of the N x C result, C = 1 + d + d^2, is held to ``Chain.value()`` (column 0) or to ``Chain.deriv`` of the
column's spec, row by row: |got - ref| <= K eps A_row with K = tt_chain.K of the model's list and the column's family:
the gradient and the off-diagonals (the (1, 1) specs) "order1", the diagonal "order2".  tests/test_tt_hessian_host.py
shows that the carried association, restated in float64, sits where the left-to-right chain does, so the table needs no
constant for it.  The two models whose every rank is 1 take the edge K, as in tests/test_gpu_tt_gradient.py: the float64
restatement itself measures 3.70 and 4.12 eps A_row there (the undiluted rounding of s, tt_chain.RESTATEMENT_WORST), so
K = 32 leaves 8x, not 16x.

Worst |got - ref| / (eps A_row) measured on MI355X, value / gradient / diagonal / off-diagonals (K beside it; the
off-diagonals take the gradient's):
    sweep 0.21 / 0.30 / 0.38 / 0.54 (8 / 8 / 8), edge 1.86 / 1.46 / 2.60 / 0.30 (32 / 32 / 64), golden D and F
    0.14 / 0.21 / 0.29 / 0.22, derived models 0.15 / 0.22 / 0.23 / 0.21; one dimension 0.92 / 4.08 / 6.24 / none, every
    rank 1 2.25 / 2.50 / 3.93 / 3.66 and the 4-D rank-1 n = 9 model 2.46 / 2.45 / 2.13 / 3.11 (32 / 32 / 64; the float64
    restatement's off-diagonals: 3.70 and 4.12), n = 1 and 2 0.40 / 0.60 / 0.91 / 0.35 (8 / 8 / 8), d = 16 below 0.001.
The first three figures of every list are tests/test_gpu_tt_gradient.py's: the columns are the same bits."""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import ROOT, assert_parity, golden, spec_point_tol
import tt_chain as C
import tt_hess_chain as HC
from pychebyshev_amd import ChebyshevTT, DeviceArray, _lib
from pychebyshev_amd.device import is_device_array

pytestmark = pytest.mark.gpu

SWEEP = C.sweep_models()
EDGE = C.edge_models()
G22 = golden("g22_tt_transforms")
G28 = golden("g28_tt_derivatives")
LDS_MAX = 160 * 1024


def _model(b):
    return ChebyshevTT.from_coeff_cores(b.cores, b.domain, dim_order=b.order)


def _matrix(parts):
    """The (N, C) result behind the three returns."""
    N = parts[0].shape[0]
    if is_device_array(parts[0]):                          # views of one device result: one download
        assert all(p.parent is parts[0].parent for p in parts)
        whole = parts[0].parent.to_host()
        assert whole.shape[1] == 1 + parts[1].shape[1] + parts[2].shape[1]
        assert np.array_equal(parts[2].to_host(), whole[:, -parts[2].shape[1]:]) and np.array_equal(parts[0].to_host(), whole[:, 0])
        return whole
    return np.column_stack([np.asarray(p).reshape(N, -1) for p in parts])


def _root(a):
    """The array a NumPy view is a view of."""
    return a if a.base is None else _root(a.base)


def _info(tt):
    t = tt._dev()
    info = np.zeros(4, dtype=np.int32)
    _lib.check(t.lib.pcx_tt_hess_info(t.handle, _lib.p_i32(info)), t.lib)
    return [int(v) for v in info]


def _forced(tt, pts, block):
    """pcx_tt_hess_batch at a forced block: (rc, the (N, C) result)."""
    t = tt._dev()
    d = pts.shape[1]
    out = np.full((pts.shape[0], 1 + d + d * d), np.nan)
    rc = t.lib.pcx_tt_hess_batch(t.handle, _lib.p_f64(np.ascontiguousarray(pts)), pts.shape[0], block, _lib.p_f64(out))
    return rc, out


def _check(got, ref, K, what):
    """(N, C) against [(column, family, values, amplitudes)]: each row of each column within K[family] eps A_row."""
    assert got.dtype == np.float64 and got.shape[1] == len(ref), what
    for col, family, val, amp in ref:
        r = C.ratios(got[:, col], val, amp)                # asserts an exact zero where the amplitude is zero
        worst = float(np.max(r))
        assert worst <= K[family], f"{what} column {col} ({family}): row {int(np.argmax(r))}: {worst:.3g} eps A_row > K = {K[family]}"
    print(f"{what}: worst rows, eps A_row:", {f: round(r, 3) for f, r in HC.worst_ratios(got, ref).items()},
          "K", {f: K[f] for f in ("value", "order1", "order2")})


def _exact_zeros(got, b):
    d = len(b.cores)
    H = got[:, 1 + d:].reshape(-1, d, d)
    for k, core in enumerate(b.cores):
        u = k if b.order is None else b.order[k]
        n = core.shape[1]
        if n == 1:
            assert np.all(H[:, u, :] == 0.0) and np.all(H[:, :, u] == 0.0), (k, "Hessian row and column of a one-node dimension")
        if n <= 2:
            assert np.all(H[:, u, u] == 0.0), (k, "diagonal entry of a dimension with at most two nodes")


def _run(b, group_K, what):
    tt = _model(b)
    parts = tt.hessian_batch(b.pts)
    d, N = len(b.cores), b.pts.shape[0]
    assert [p.shape for p in parts] == [(N,), (N, d), (N, d, d)]
    got = _matrix(parts)
    _check(got, HC.reference(b), group_K, what)
    _exact_zeros(got, b)
    assert np.array_equal(parts[2], parts[2].transpose(0, 2, 1))
    return tt, got


@pytest.mark.parametrize("model", SWEEP, ids=[m.name for m in SWEEP])
def test_every_body(model):
    """96 rows (rows 0 and 1 on the domain ends; every third model a permuted dim_order) at the planner's block: each
    model's dimensions reach their (cap, uniform / mixed, left rank, node count) bodies of the right sweep, of the
    left sweep with carried vectors; block = 1 then takes every later pass's bodies (the plain fold up to its source, the
    two-basis fold from there) to the same bits."""
    b = C.build(model)
    tt, got = _run(b, C.K["sweep"], model.name)
    rc, one = _forced(tt, b.pts, 1)
    assert rc == 0 and np.array_equal(one, got)


@pytest.mark.parametrize("model", EDGE, ids=[m.name for m in EDGE])
def test_wave_per_row(model):
    """k_tt_hess_generic: lane loops of one, two and three trips, and the model that is generic only because n > 16."""
    b = C.build(model)
    tt, _ = _run(b, C.K["edge"], model.name)
    assert _info(tt)[0] == 2


DEGENERATE = [
    C.Model(1000, "one-dimension", 8, "uniform", (1, 1), (7,), 70),
    C.Model(1001, "one-and-two-nodes", 8, "mixed", (1, 3, 4, 1), (5, 1, 2), 70),
    C.Model(1002, "every-rank-1", 8, "mixed", (1, 1, 1, 1, 1), (4, 1, 16, 3), 70),
    C.Model(1003, "d16-rank16-n2", 16, "uniform", (1,) + (16,) * 15 + (1,), (2,) * 16, 65),
    C.Model(1004, "rank-1-4d-n9", 8, "uniform", (1, 1, 1, 1, 1), (9,) * 4, 130),
]


@pytest.mark.parametrize("model", DEGENERATE, ids=[m.name for m in DEGENERATE])
def test_degenerate_shapes(model):
    """d = 1 (C = 3, hess is the diagonal); n = 1 and n = 2 (exact zeros); every rank 1 (edge K); d = 16 with ranks 16:
    the launch above R and L's 128 KiB."""
    b = C.build(model)
    tt, got = _run(b, C.K["edge" if max(model.ranks) == 1 else "sweep"], model.name)
    assert C.rank_cap(model) != 0
    info = _info(tt)
    assert info[0] == 1
    if model.name == "one-dimension":
        assert got.shape[1] == 3 and info[1] == info[3] == 1
        assert np.array_equal(got[:, 2], _second(tt, b.pts)[:, 2])
    if model.name == "d16-rank16-n2":
        assert info[2] <= LDS_MAX and info[3] >= 1 and 1 <= info[1] <= info[3]
        assert info[2] > 128 * 1024
        # the LDS limit of an instantiation is lifted at its first large launch only: a second one gives the same bits
        assert np.array_equal(_matrix(tt.hessian_batch(b.pts)), got)


def _second(tt, pts):
    """gradient_batch(second=True) as one (N, 1 + 2 d) array."""
    v, g, h = tt.gradient_batch(pts, second=True)
    return np.column_stack([v, g, h])


def _uniform(cap):
    return next(m for m in SWEEP if m.cap == cap and m.mode == "uniform" and m.n[0] == 6)


BLOCK_MODELS = [_uniform(8), next(m for m in SWEEP if m.cap == 12 and m.mode == "mixed" and m.name.endswith("t3")), _uniform(16),
                EDGE[0], DEGENERATE[3]]


@pytest.mark.parametrize("model", BLOCK_MODELS, ids=[m.name for m in BLOCK_MODELS])
def test_the_block_does_not_matter(model):
    """block = 1, 2, the planner's and the largest that fits give the same bits; one above the largest that fits is
    PCX_ERR_UNSUPPORTED where it is a block at all, PCX_ERR_INVALID where it is not."""
    b = C.build(model)
    tt = _model(b)
    d = len(b.cores)
    form, plan, lds, fits = _info(tt)
    assert form == (2 if model.mode == "generic" else 1)
    assert 1 <= plan <= fits <= max(1, d - 1) and 0 < lds <= LDS_MAX
    got = _matrix(tt.hessian_batch(b.pts))
    for block in sorted({1, min(2, fits), plan, fits}):
        rc, out = _forced(tt, b.pts, block)
        assert rc == 0, (model.name, block, _lib.last_error(tt._dev().lib))
        assert np.array_equal(out, got), (model.name, block)
    rc, out = _forced(tt, b.pts, fits + 1)
    assert rc == (_lib.PCX_ERR_UNSUPPORTED if fits + 1 <= max(1, d - 1) else _lib.PCX_ERR_INVALID), (model.name, fits)
    assert np.all(np.isnan(out))
    if model.name == "d16-rank16-n2":
        assert fits < d - 1                                # the model the blocks exist for


def test_bit_for_bit():
    """tail_model(): a batch of N rows equals its rows sent one at a time; the host- and the device-pointer entry agree;
    out= is the returned arrays; hessian(point) is row 0; the Hessian is symmetric; value, gradient and diagonal are
    gradient_batch(second=True)'s."""
    b = C.build(C.tail_model())
    tt = _model(b)
    d = len(b.cores)
    Cc = 1 + d + d * d
    rows = np.array([_matrix(tt.hessian_batch(b.pts[r:r + 1]))[0] for r in range(b.pts.shape[0])])
    diag = 1 + d + np.arange(d) * (d + 1)
    for N in C.TAIL_NS:
        pts = np.ascontiguousarray(b.pts[:N])
        parts = tt.hessian_batch(pts)
        got = _matrix(parts)
        assert got.shape == (N, Cc)
        assert np.array_equal(got, rows[:N]), f"N = {N}: rows alone"
        assert _root(parts[0]) is _root(parts[1]) is _root(parts[2]) and _root(parts[0]).shape == (N, Cc)
        assert np.array_equal(parts[2], parts[2].transpose(0, 2, 1))
        dev = tt.hessian_batch(DeviceArray.from_host(pts))
        assert all(is_device_array(p) for p in dev) and [p.shape for p in dev] == [(N,), (N, d), (N, d * d)]
        assert np.array_equal(_matrix(dev), got), f"N = {N}: device entry"
        second = _second(tt, pts)
        assert np.array_equal(got[:, :1 + d], second[:, :1 + d]) and np.array_equal(got[:, diag], second[:, 1 + d:]), f"N = {N}: gradient_batch"
        out = np.full((N, Cc), np.nan)
        views = tt.hessian_batch(pts, out=out)
        assert np.array_equal(out, got) and all(np.shares_memory(v, out) for v in views)
        dout = DeviceArray.empty((N, Cc))
        dviews = tt.hessian_batch(pts, out=dout)
        assert np.array_equal(dout.to_host(), got) and np.array_equal(_matrix(dviews), got)
    value, grad, hess = tt.hessian(b.pts[0])
    assert isinstance(value, float) and grad.shape == (d,) and hess.shape == (d, d)
    assert np.array_equal(np.concatenate([[value], grad, hess.ravel()]), rows[0])
    with pytest.raises(ValueError, match="does not match the result"):
        tt.hessian_batch(b.pts, out=np.empty((b.pts.shape[0], 1 + 2 * d)))
    with pytest.raises(ValueError, match=r"points must have shape"):
        tt.hessian_batch(b.pts[:, :-1])


def test_a_host_batch_in_three_pieces():
    """A 2-D rank-3 model and a host batch one row longer than two staging pieces ((1 + 2 d) / C of 2^18 rows, rounded
    down to a multiple of 64) against the device-pointer entry, bit for bit."""
    m = C.Model(1100, "two-dimensions-rank-3", 8, "mixed", (1, 3, 1), (5, 4), 2)
    b = C.build(m)
    tt = _model(b)
    piece = ((1 << 18) * 5 // 7) // 64 * 64
    N = 2 * piece + 1
    rng = np.random.default_rng(11)
    pts = np.column_stack([rng.uniform(lo, hi, N) for lo, hi in b.udom])
    host = _matrix(tt.hessian_batch(pts))
    dev = _matrix(tt.hessian_batch(DeviceArray.from_host(pts)))
    assert host.shape == (N, 7) and np.array_equal(host, dev)
    assert np.array_equal(host[[0, piece - 1, piece, 2 * piece - 1, 2 * piece]],
                          _matrix(tt.hessian_batch(pts[[0, piece - 1, piece, 2 * piece - 1, 2 * piece]])))


def _golden(tag):
    cores, k = [], 0
    while f"{tag}_core{k}" in G22.files:
        cores.append(G22[f"{tag}_core{k}"])
        k += 1
    pts = np.concatenate([G28[f"{tag}_s{i}_pts"] for i in range(3)])[:130]
    return C.Built(None, cores, G22[f"{tag}_domain"].tolist(), G22[f"{tag}_order"].tolist(), None, np.ascontiguousarray(pts))


@pytest.mark.parametrize("tag, group", [("D", "sweep"), ("F", "edge")])
def test_against_the_chain_per_spec_kernel(tag, group):
    """D: a storage order and mixed node counts on the lane-per-row form; F: the wave-per-row form.  hessian_batch and
    eval_multi_batch(method="analytic") with every column's spec both stay within K of the long-double chain, and within
    spec_point_tol of each other (the association differs: no equality of bits)."""
    b = _golden(tag)
    tt, got = _run(b, C.K[group], f"golden {tag}")
    d = len(b.cores)
    assert _info(tt)[0] == (1 if group == "sweep" else 2)
    cols = HC.columns(d)
    per_spec = tt.eval_multi_batch(b.pts, [spec for _, spec, _ in cols], method="analytic")
    _check(per_spec, HC.reference(b), C.K[group], f"golden {tag} eval_multi_batch")
    for col, spec, _ in cols:
        assert_parity(got[:, col], per_spec[:, col], tol=1e-12, point_tol=spec_point_tol(spec), what=f"tt hessian_batch vs analytic {tag} {spec}")


def test_derived_models_are_ordinary_handles():
    """A differentiated, a reordered and a summed model: hessian_batch on each against the long-double chain of the
    model's own cores."""
    src = next(m for m in SWEEP if m.cap == 8 and m.mode == "uniform" and m.n[0] == 6)
    b = C.build(src._replace(rows=70))
    tt = _model(b)
    d = len(b.cores)
    derived = {
        "differentiate": tt.differentiate([1] + [0] * (d - 1)),
        "sum": tt + tt * 0.5,
        "reorder": tt.reorder(list(range(d))[::-1]),
    }
    rng = np.random.default_rng(77)
    for name, m in derived.items():
        dom = [m.domain[m.dim_order.index(u)] for u in range(m.num_dimensions)]           # user frame
        pts = np.column_stack([rng.uniform(lo, hi, 70) for lo, hi in dom])
        built = C.Built(None, m._coeff_cores, [list(map(float, ab)) for ab in m.domain], list(m.dim_order), None, pts)
        got = _matrix(m.hessian_batch(pts))
        _check(got, HC.reference(built), C.K["sweep"], f"derived {name}")
    assert derived["reorder"].dim_order != list(range(d))


def test_c_abi_argument_errors():
    b = C.build(C.tail_model())
    tt = _model(b)
    t = tt._dev()
    lib = t.lib
    invalid = _lib.PCX_ERR_INVALID
    d = len(b.cores)
    pts = np.ascontiguousarray(b.pts[:4])
    out = np.full((4, 1 + d + d * d), 7.0)
    none_f64 = ctypes.POINTER(ctypes.c_double)()
    assert lib.pcx_tt_hess_batch(None, _lib.p_f64(pts), 4, 0, _lib.p_f64(out)) == invalid
    assert lib.pcx_tt_hess_batch(t.handle, _lib.p_f64(pts), 4, d, _lib.p_f64(out)) == invalid
    assert "block" in lib.pcx_last_error().decode()
    assert lib.pcx_tt_hess_batch(t.handle, _lib.p_f64(pts), 4, -1, _lib.p_f64(out)) == invalid
    assert lib.pcx_tt_hess_batch(t.handle, _lib.p_f64(pts), -1, 0, _lib.p_f64(out)) == invalid
    assert lib.pcx_tt_hess_batch(t.handle, none_f64, 4, 0, _lib.p_f64(out)) == invalid
    assert lib.pcx_tt_hess_batch(t.handle, _lib.p_f64(pts), 4, 0, none_f64) == invalid
    assert lib.pcx_tt_hess_batch(t.handle, _lib.p_f64(pts), 0, d, _lib.p_f64(out)) == invalid
    assert lib.pcx_tt_hess_batch_dev(None, None, 4, 0, None, None) == invalid
    assert lib.pcx_tt_hess_batch_dev(t.handle, None, 4, 0, None, None) == invalid
    assert lib.pcx_tt_hess_batch_dev(t.handle, None, 0, d, None, None) == invalid
    assert lib.pcx_tt_hess_batch_dev(t.handle, None, -1, 0, None, None) == invalid
    assert lib.pcx_tt_hess_info(None, _lib.p_i32(np.zeros(4, dtype=np.int32))) == invalid
    assert lib.pcx_tt_hess_info(t.handle, None) == invalid
    assert np.all(out == 7.0)                               # nothing was launched
    assert lib.pcx_tt_hess_batch(t.handle, _lib.p_f64(pts), 0, 1, _lib.p_f64(out)) == 0
    assert lib.pcx_tt_hess_batch(t.handle, none_f64, 0, 0, none_f64) == 0
    assert lib.pcx_tt_hess_batch_dev(t.handle, None, 0, d - 1, None, None) == 0
    assert np.all(out == 7.0)
    empty = tt.hessian_batch(np.zeros((0, d)))
    assert [p.shape for p in empty] == [(0,), (0, d), (0, d, d)]
    assert lib.pcx_tt_hess_batch(t.handle, _lib.p_f64(pts), 4, 1, _lib.p_f64(out)) == 0
    assert np.array_equal(out, _matrix(tt.hessian_batch(pts)))


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
        value, grad, hess = tt.hessian_batch(t)
        assert all(is_device_array(p) and isinstance(p, DeviceArray) for p in (value, grad, hess))
        assert value.shape == (48,) and grad.shape == (48, 4) and hess.shape == (48, 16)
        hv, hg, hh = tt.hessian_batch(pts)
        back = torch.as_tensor(hess, device="cuda:0")
        assert back.data_ptr() == hess.ptr and tuple(back.stride()) == (21, 1)
        assert np.array_equal(back.cpu().numpy().reshape(48, 4, 4), hh)
        assert np.array_equal(torch.as_tensor(value, device="cuda:0").cpu().numpy(), hv)
        assert np.array_equal(grad.to_host(), hg)
        out = torch.full((48, 21), float("nan"), dtype=torch.float64, device="cuda:0")
        tt.hessian_batch(t, out=out)
        assert np.array_equal(out.cpu().numpy(), np.column_stack([hv, hg, hh.reshape(48, 16)]))
        print("torch-interop-ok")
    """)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "torch-interop-ok" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
