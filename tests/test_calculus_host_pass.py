"""The host compilation pass of calc_row (csrc/calculus_kernels.h: "written once for both compilation passes") under the
address and undefined-behaviour sanitizers, on a CPU.

tests/host/calc_host_main.cpp is compiled with hipcc (both passes compile; the sanitizers instrument the host side only)
and run as child processes, one per mode, over every fibre length n = 1 .. 64: the families of calc_fibres and its
metamorphic inputs.  The program keeps the solver's LDS on the heap, exactly as large as the kernels' __shared__ array
of the fibre's class, filled with NaN bit patterns before every row: an index past it (the 4n-entry cosine table, the
n + 1 candidates, the MP + 1 row stride at m == MP) ends the child with a sanitizer report, and a slot read before it
is written shows as a wrong result.  The outputs must match the NumPy restatement as the device tests ask (counts equal,
roots 1e-10 (b - a), values 1e-12 max|fibre|) and satisfy the metamorphic relations bit for bit.  No GPU is used."""
import os
import struct
import subprocess

import numpy as np
import pytest

import calc_fibres as CF

from pychebyshev_amd import _build

HERE = os.path.dirname(os.path.abspath(__file__))
DOM = (-1.0, 1.0)
SAN_FLAGS = ["--offload-arch=gfx950", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
             "-fno-sanitize-recover=undefined"]


def _hipcc():
    try:
        return _build.hipcc_path()
    except RuntimeError:
        return None


pytestmark = pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")


def _inputs(n):
    """name -> rows of one fibre length: the families, then the metamorphic inputs."""
    inp = {"families": CF.families(n)[0]}
    inp.update(CF.metamorphic_inputs(n))
    return inp


def _write_cases(path, mode):
    """Every input of every n as one case each -> [(n, name, rows)] in file order."""
    cases = [(n, name, V) for n in range(1, 65) for name, V in _inputs(n).items()]
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", len(cases)))
        for n, name, V in cases:
            fh.write(struct.pack("<4i2d", n, V.shape[0], CF.MODES.index(mode), 0, *DOM))
            for arr in CF.grid(n, *DOM) + (V,):
                fh.write(np.ascontiguousarray(arr, dtype="<f8").tobytes())
    return [(n, name, V.shape[0]) for n, name, V in cases]


def _read_cases(path, mode, cases):
    """(n, name) -> the outputs in the shape cheb1d_calculus returns them."""
    with open(path, "rb") as fh:
        buf = fh.read()
    out, at = {}, 0
    for n, name, rows in cases:
        cnt = np.frombuffer(buf, "<i4", rows, at)
        at += 4 * rows
        if mode == "roots":
            W = max(n - 1, 1)
            out[n, name] = (np.frombuffer(buf, "<f8", rows * W, at).reshape(rows, W), cnt)
            at += 8 * rows * W
        else:
            out[n, name] = (np.frombuffer(buf, "<f8", rows, at), np.frombuffer(buf, "<f8", rows, at + 8 * rows), cnt)
            at += 16 * rows
    assert at == len(buf), "the program wrote more than the cases hold"
    return out


@pytest.fixture(scope="module")
def host_pass(tmp_path_factory):
    """Build the program and run it once per mode (three children side by side) -> results[mode][n, name]."""
    tmp = tmp_path_factory.mktemp("calc_host")
    exe = str(tmp / "calc_host_main")
    cmd = [_hipcc()] + SAN_FLAGS + ["-I", _build.CSRC, "-o", exe, os.path.join(HERE, "host", "calc_host_main.cpp")]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, "hipcc failed:\n" + res.stdout
    procs = {}
    for mode in CF.MODES:
        src, dst = str(tmp / f"{mode}.in"), str(tmp / f"{mode}.out")
        cases = _write_cases(src, mode)
        procs[mode] = (subprocess.Popen([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True),
                       dst, cases)
    results = {}
    for mode, (proc, dst, cases) in procs.items():
        log = proc.communicate()[0]
        assert proc.returncode == 0, f"mode {mode}: exit {proc.returncode}\n{log[-4000:]}"
        results[mode] = _read_cases(dst, mode, cases)
    return results


@pytest.mark.parametrize("mp", sorted(CF.LDS_CLASSES))
def test_host_pass_matches_the_restatement(host_pass, mp):
    stats = {}
    for n in CF.LDS_CLASSES[mp]:
        V, kinds = CF.families(n)
        for mode in CF.MODES:
            skipped = CF.check_rows(n, V, kinds, DOM, mode, host_pass[mode][n, "families"], f"host n={n} {mode}", stats)
            assert skipped <= CF.MAX_FRAGILE * CF.NOISE_ROWS, (n, skipped)
    print(f"\nhost pass, LDS class {mp}: worst root difference {stats.get('root', 0.0):.2e} (b - a), "
          f"worst value difference {stats.get('value', 0.0):.2e} max|f|")


def test_host_pass_returns_the_endpoints_of_lobatto_rows_exactly(host_pass):
    def solve(n):
        R, cnt = host_pass["roots"][n, "families"]
        i = CF.families(n)[1].index("lobatto")
        return R[i], cnt[i]
    missed = CF.missed_endpoints(DOM, solve, range(4, 65))
    assert not missed, missed


@pytest.mark.parametrize("mp", sorted(CF.LDS_CLASSES))
def test_host_pass_metamorphic_relations_hold_bitwise(host_pass, mp):
    for n in CF.LDS_CLASSES[mp]:
        out = {name: {mode: host_pass[mode][n, name] for mode in CF.MODES} for name in CF.metamorphic_inputs(n)}
        CF.check_metamorphic(n, DOM, out, f"host n={n}")
