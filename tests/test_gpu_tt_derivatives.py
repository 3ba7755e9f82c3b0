"""ChebyshevTT.eval_multi_batch(..., method="analytic") (pcx_tt_deriv_batch, csrc/tt_deriv_kernels.h) against the
long-double chain and the reference's dense analytic route of g28_tt_derivatives.npz, against the closed forms of the
differentiated basis, and against ``differentiate`` as a second route.  Models A .. E run the lane-per-row form (rank
caps 8, 12, 16; one and several node counts), model F the wave-per-row form on the plain cores."""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
from numpy.polynomial import chebyshev as npcheb

from conftest import ROOT, assert_parity, golden, spec_point_tol
from pychebyshev_amd import ChebyshevTT, DeviceArray, _lib

pytestmark = pytest.mark.gpu

G22 = golden("g22_tt_transforms")
G = golden("g28_tt_derivatives")
MODELS = ("A", "B", "C", "C2", "D", "E", "F")
_TT = {}
_GOT = {}


def model(tag):
    if tag not in _TT:
        cores, k = [], 0
        while f"{tag}_core{k}" in G22.files:
            cores.append(G22[f"{tag}_core{k}"])
            k += 1
        _TT[tag] = ChebyshevTT.from_coeff_cores(cores, G22[f"{tag}_domain"].tolist(), dim_order=G22[f"{tag}_order"].tolist())
    return _TT[tag]


def specs_of(tag):
    return [G[f"{tag}_s{i}_spec"].tolist() for i in range(int(G[f"{tag}_nspec"]))]


def analytic(g):
    """The device's column for one golden group, computed once for the tests that compare it."""
    if g not in _GOT:
        got = model(g.split("_")[0]).eval_multi_batch(G[f"{g}_pts"], [G[f"{g}_spec"].tolist()], method="analytic")
        assert got.shape == (48, 1) and got.dtype == np.float64
        _GOT[g] = got[:, 0].copy()
    return _GOT[g]


GROUPS = [f"{tag}_s{i}" for tag in MODELS for i in range(int(G[f"{tag}_nspec"]))]
ZERO_GROUPS = [g for g in GROUPS if not np.any(G[f"{g}_ld"])]
REF_GROUPS = [g for g in GROUPS if f"{g}_ref" in G.files]


@pytest.mark.parametrize("g", [g for g in GROUPS if g not in ZERO_GROUPS])
def test_analytic_matches_the_long_double_chain(g):
    spec = G[f"{g}_spec"].tolist()
    assert_parity(analytic(g), G[f"{g}_ld"], tol=1e-12, point_tol=1e-12, what=f"tt analytic order {sum(spec)} vs ld {g} {spec}")


@pytest.mark.parametrize("g", REF_GROUPS)
def test_analytic_matches_the_reference_dense_route(g):
    spec = G[f"{g}_spec"].tolist()
    assert_parity(analytic(g), G[f"{g}_ref"], tol=1e-12, point_tol=spec_point_tol(spec),
                  what=f"tt analytic order {sum(spec)} vs ref {g} {spec}")


def test_an_order_that_reaches_the_node_count_is_exactly_zero():
    assert ZERO_GROUPS and all(g.startswith("B_") for g in ZERO_GROUPS)
    assert [G[f"{g}_spec"].tolist() for g in ZERO_GROUPS] == [[0, 2], [2, 2]]              # model B: user dimension 1 has 2 nodes
    for g in ZERO_GROUPS:
        got = analytic(g)
        assert np.all(got == 0.0) and not np.any(np.signbit(got) & (got != 0.0))
    c = model("C")
    mixed = c.eval_multi_batch(G["C_s0_pts"], [[0] * 5, [2, 0, 0, 0, 1]], method="analytic")
    assert np.all(mixed[:, 0] != 0.0)


@pytest.mark.parametrize("j", range(16))
def test_basis_closed_forms(j):
    """A 1-D model whose core is the unit vector e_j is sc^p T_j^(p)(s): at s = +-1, T'_j = (+-1)^(j+1) j^2 and
    T''_j = (+-1)^j j^2 (j^2 - 1) / 3; at s = 0 against numpy.polynomial.chebyshev.  The domain [1, 5] has
    sc = 2 / (b - a) = 0.5 and maps its ends and its middle to s = -1, 1, 0 exactly."""
    core = np.zeros((1, 16, 1))
    core[0, j, 0] = 1.0
    tt = ChebyshevTT.from_coeff_cores([core], [[1.0, 5.0]])
    sc = 0.5
    got = tt.eval_multi_batch(np.array([[1.0], [5.0], [3.0]]), [[0], [1], [2]], method="analytic")
    for row, sign in ((0, -1.0), (1, 1.0)):
        want = [sign ** j, sign ** (j + 1) * j * j * sc, sign ** j * j * j * (j * j - 1) / 3.0 * sc * sc]
        for p in range(3):
            assert abs(got[row, p] - want[p]) <= 1e-13 * abs(want[p]), (j, row, p, got[row, p], want[p])
    for p in range(3):
        want = float(npcheb.chebval(0.0, npcheb.chebder(core[0, :, 0], m=p))) * sc ** p if p else float(npcheb.chebval(0.0, core[0, :, 0]))
        assert abs(got[2, p] - want) <= 1e-13 * max(abs(want), sc ** p), (j, p, got[2, p], want)


@pytest.mark.parametrize("tag", ["D", "F"])
def test_differentiate_is_a_second_route(tag):
    """D: a storage order and mixed node counts on the lane-per-row form; F: the wave-per-row form."""
    tt = model(tag)
    for i, spec in enumerate(specs_of(tag)):
        pts = G[f"{tag}_s{i}_pts"]
        fused = analytic(f"{tag}_s{i}")
        res = tt.differentiate(spec)
        assert res.dim_order == tt.dim_order
        assert_parity(res.eval_batch(pts), fused, tol=1e-12, point_tol=spec_point_tol(spec),
                      what=f"tt differentiate order {sum(spec)} vs analytic {tag} {spec}")


@pytest.mark.parametrize("tag", ["C", "D", "F"])
def test_batch_sizes_rows_alone_and_the_device_entry(tag):
    """N around the 64-row workgroup; a batch equals its rows sent one at a time, and the device-pointer entry the
    host-pointer one, bit for bit."""
    tt = model(tag)
    specs = specs_of(tag)
    base = np.concatenate([G[f"{tag}_s0_pts"], G[f"{tag}_s1_pts"], G[f"{tag}_s2_pts"]])[:130]
    whole = tt.eval_multi_batch(base, specs, method="analytic")
    assert whole.shape == (130, len(specs))
    for n in (1, 63, 64, 65):
        assert np.array_equal(tt.eval_multi_batch(base[:n], specs, method="analytic"), whole[:n]), n
    for r in range(130):
        assert np.array_equal(tt.eval_multi_batch(base[r:r + 1], specs, method="analytic")[0], whole[r]), r
    for n in (1, 65, 130):
        dev = tt.eval_multi_batch(DeviceArray.from_host(base[:n]), specs, method="analytic")
        assert isinstance(dev, DeviceArray) and dev.shape == (n, len(specs))
        assert np.array_equal(dev.to_host(), whole[:n]), n
    assert tt.eval_multi(base[0], specs, method="analytic") == whole[0].tolist()
    # every column is the single-spec launch the parity tests look at
    assert np.array_equal(whole[:48, 0], analytic(f"{tag}_s0"))


@pytest.mark.parametrize("tag", ["C", "F"])
def test_more_specs_than_one_launch_takes(tag):
    """65 specs: 64 on the first launch's blockIdx.y and one on a second; equal to the same specs in two calls."""
    tt = model(tag)
    own = specs_of(tag)
    specs = [own[i % len(own)] for i in range(65)]
    pts = np.concatenate([G[f"{tag}_s0_pts"], G[f"{tag}_s1_pts"], G[f"{tag}_s2_pts"]])[:130]
    once = tt.eval_multi_batch(pts, specs, method="analytic")
    assert once.shape == (130, 65)
    twice = np.hstack([tt.eval_multi_batch(pts, specs[:40], method="analytic"),
                       tt.eval_multi_batch(pts, specs[40:], method="analytic")])
    assert np.array_equal(once, twice)
    for i in range(len(own), 65):
        assert np.array_equal(once[:, i], once[:, i % len(own)])
    dev = tt.eval_multi_batch(DeviceArray.from_host(pts), specs, method="analytic")
    assert np.array_equal(dev.to_host(), once)


def test_four_differenced_dimensions_on_a_device_array():
    tt = model("D")
    spec = [1, 1, 1, 1]
    pts = G["D_s0_pts"]
    d_pts = DeviceArray.from_host(pts)
    with pytest.raises(NotImplementedError, match="more than three differenced dimensions"):
        tt.eval_multi_batch(d_pts, [spec])
    got = tt.eval_multi_batch(d_pts, [spec], method="analytic")
    assert isinstance(got, DeviceArray) and got.shape == (48, 1)
    want = tt.differentiate(spec).eval_batch(pts)
    assert_parity(got.to_host()[:, 0], want, tol=1e-12, point_tol=spec_point_tol(spec), what="tt analytic order 4 vs differentiate D")


def test_default_method_is_still_the_finite_differences():
    tt = model("C")
    pts = G["C_s0_pts"]
    specs = [[0] * 5, [1, 0, 0, 0, 0], [0, 0, 2, 0, 0]]
    fd = tt.eval_multi_batch(pts, specs)
    assert np.array_equal(fd, tt.eval_multi_batch(pts, specs, method="fd"))
    assert np.array_equal(fd, tt._eval_multi_batch_host(pts, specs))
    assert tt.eval_multi(pts[5], specs) == tt.eval_multi(pts[5], specs, method="fd") == fd[5].tolist()
    an = tt.eval_multi_batch(pts, specs, method="analytic")
    assert not np.array_equal(an[:, 1:], fd[:, 1:])
    # the finite differences carry O(h^2) truncation error and, in the two corner rows, the nudge of 1.5 h = 3e-4 in s:
    # by Markov's inequality a derivative of a degree-10 polynomial moves by at most n^2 = 121 times that, 3.6e-2
    assert np.max(np.abs(an - fd)) <= 5e-2 * np.max(np.abs(an))


def test_torch_tensor_in_device_array_out():
    """A ROCm PyTorch tensor as the batch, in a child process (torch brings its own copy of the HIP runtime)."""
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        import numpy as np
        import torch
        from pychebyshev_amd import ChebyshevTT, DeviceArray
        g = np.load({os.path.join(ROOT, "tests", "golden", "g22_tt_transforms.npz")!r})
        v = np.load({os.path.join(ROOT, "tests", "golden", "g28_tt_derivatives.npz")!r})
        tt = ChebyshevTT.from_coeff_cores([g[f"D_core{{k}}"] for k in range(4)], g["D_domain"].tolist(),
                                          dim_order=g["D_order"].tolist())
        pts = v["D_s0_pts"]
        specs = [[0, 0, 0, 0], [1, 0, 0, 1], [1, 1, 1, 1]]
        t = torch.as_tensor(pts, device="cuda:0") * 1.0
        out = tt.eval_multi_batch(t, specs, method="analytic")
        assert isinstance(out, DeviceArray) and out.shape == (48, 3)
        back = torch.as_tensor(out, device="cuda:0")
        assert back.data_ptr() == out.ptr
        assert np.array_equal(back.cpu().numpy(), tt.eval_multi_batch(pts, specs, method="analytic"))
        print("torch-interop-ok")
    """)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "torch-interop-ok" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


def test_c_abi_argument_errors():
    tt = model("C")
    t = tt._dev()
    lib = t.lib
    invalid = _lib.PCX_ERR_INVALID
    pts = np.ascontiguousarray(G["C_s0_pts"][:4])
    out = np.full((4, 2), 7.0)
    ok = np.array([[1, 0, 0, 0, 0], [0, 0, 2, 0, 0]], dtype=np.int32)
    none_f64 = ctypes.POINTER(ctypes.c_double)()
    none_i32 = ctypes.POINTER(ctypes.c_int32)()
    assert lib.pcx_tt_deriv_batch(None, _lib.p_f64(pts), 4, _lib.p_i32(ok), 2, _lib.p_f64(out)) == invalid
    assert lib.pcx_tt_deriv_batch(t.handle, none_f64, 4, _lib.p_i32(ok), 2, _lib.p_f64(out)) == invalid
    assert lib.pcx_tt_deriv_batch(t.handle, _lib.p_f64(pts), 4, _lib.p_i32(ok), 2, none_f64) == invalid
    assert lib.pcx_tt_deriv_batch(t.handle, _lib.p_f64(pts), 4, none_i32, 2, _lib.p_f64(out)) == invalid
    assert lib.pcx_tt_deriv_batch(t.handle, _lib.p_f64(pts), -1, _lib.p_i32(ok), 2, _lib.p_f64(out)) == invalid
    assert lib.pcx_tt_deriv_batch(t.handle, _lib.p_f64(pts), 4, _lib.p_i32(ok), -1, _lib.p_f64(out)) == invalid
    for bad_order in (3, -1):
        bad = ok.copy()
        bad[1, 4] = bad_order
        assert lib.pcx_tt_deriv_batch(t.handle, _lib.p_f64(pts), 4, _lib.p_i32(bad), 2, _lib.p_f64(out)) == invalid
        assert "not supported" in lib.pcx_last_error().decode()
        assert lib.pcx_tt_deriv_batch_dev(t.handle, None, 0, _lib.p_i32(bad), 2, None, None) == invalid
    assert lib.pcx_tt_deriv_batch_dev(None, None, 4, _lib.p_i32(ok), 2, None, None) == invalid
    assert lib.pcx_tt_deriv_batch_dev(t.handle, None, 4, _lib.p_i32(ok), 2, None, None) == invalid
    assert lib.pcx_tt_deriv_batch_dev(t.handle, None, 4, none_i32, 2, None, None) == invalid
    assert np.all(out == 7.0)                               # nothing was launched
    assert lib.pcx_tt_deriv_batch(t.handle, _lib.p_f64(pts), 0, _lib.p_i32(ok), 2, _lib.p_f64(out)) == 0
    assert lib.pcx_tt_deriv_batch(t.handle, _lib.p_f64(pts), 4, none_i32, 0, _lib.p_f64(out)) == 0
    assert lib.pcx_tt_deriv_batch_dev(t.handle, None, 0, _lib.p_i32(ok), 2, None, None) == 0
    assert np.all(out == 7.0)
    assert tt.eval_multi_batch(np.zeros((0, 5)), ok.tolist(), method="analytic").shape == (0, 2)
