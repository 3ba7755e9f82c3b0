"""The host compilation pass of inv_block (csrc/invert_kernels.h: written once for both compilation passes) under the
address and undefined-behaviour sanitizers, on a CPU.

tests/host/invert_host_main.cpp is compiled with hipcc (both passes compile; the sanitizers instrument the host side
only) and run as one child process over every fibre length n = 1 .. 64: the families of calc_fibres with the targets of
invert_fibres.  The program keeps the solver's LDS tile on the heap, exactly as large as the kernel's __shared__ array of
the fibre's class, filled with NaN bit patterns before every block of 64 rows: an index past it ends the child with a
sanitizer report, and a slot read before it is written shows as a wrong result.  status must equal the NumPy
restatement's (_calculus.invert_rows) exactly and x lie within 1e-13 (b - a) of it, with no row left out; the printed
summary says whether x was in fact the restatement's bit for bit, and the largest iteration count.  No GPU is used."""
import os
import struct
import subprocess

import numpy as np
import pytest

import calc_fibres as CF
import invert_fibres as IF

from pychebyshev_amd import _build, _calculus

HERE = os.path.dirname(os.path.abspath(__file__))
DOM = (-1.0, 1.0)
SAN_FLAGS = ["--offload-arch=gfx950", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
             "-fno-sanitize-recover=undefined"]
NS = range(1, 65)
ZERO_NS = range(2, 65)          # invert_fibres.near_zero: solutions at and next to 0


def _hipcc():
    try:
        return _build.hipcc_path()
    except RuntimeError:
        return None


pytestmark = pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")


@pytest.fixture(scope="module")
def host_pass(tmp_path_factory):
    """Build the program and run it once -> {n: (x, status, iterations)}."""
    tmp = tmp_path_factory.mktemp("invert_host")
    exe = str(tmp / "invert_host_main")
    cmd = [_hipcc()] + SAN_FLAGS + ["-I", _build.CSRC, "-o", exe, os.path.join(HERE, "host", "invert_host_main.cpp")]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, "hipcc failed:\n" + res.stdout
    src, dst = str(tmp / "cases.in"), str(tmp / "cases.out")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<i", len(NS) + len(ZERO_NS)))
        for n, (V, t) in [(n, IF.inputs(n, DOM)) for n in NS] + [(n, IF.near_zero(n, DOM)) for n in ZERO_NS]:
            fh.write(struct.pack("<2i2d", n, V.shape[0], *DOM))
            for arr in CF.grid(n, *DOM)[:2] + (V, t):
                fh.write(np.ascontiguousarray(arr, dtype="<f8").tobytes())
    run = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout[-4000:]}"
    with open(dst, "rb") as fh:
        buf = fh.read()
    out, at = {}, 0
    for key, rows in [(n, IF.inputs(n, DOM)[0].shape[0]) for n in NS] + [(("zero", n), IF.near_zero(n, DOM)[0].shape[0]) for n in ZERO_NS]:
        x = np.frombuffer(buf, "<f8", rows, at)
        st = np.frombuffer(buf, "<i4", rows, at + 8 * rows)
        it = np.frombuffer(buf, "<i4", rows, at + 12 * rows)
        at += 16 * rows
        out[key] = (x, st, it)
    assert at == len(buf), "the program wrote more than the cases hold"
    return out


def test_host_pass_matches_the_restatement(host_pass):
    stats = {}
    iters = 0
    for n in NS:
        want_x, want_status, want_it = IF.reference(n, DOM)
        x, st, it = host_pass[n]
        IF.check(n, x, st, want_x, want_status, DOM, "host", stats)
        assert np.array_equal(it, want_it), (n, it, want_it)
        assert np.all(st >= 0), (n, st)                     # finite fibres: the cap is never reached
        iters = max(iters, int(it.max()))
    skipped = 0
    assert skipped <= IF.MAX_SKIPPED
    print(f"\nhost pass, n = 1 .. 64, {stats['rows']} rows, {skipped} left out: worst |x - restatement| "
          f"{stats['x']:.2e} (b - a), bit for bit: {stats['bitwise']}; largest iteration count {iters} of "
          f"{_calculus.INVERT_MAX_ITERS}")


def test_host_pass_solutions_at_and_next_to_zero(host_pass):
    stats = {}
    iters = 0
    for n in ZERO_NS:
        want_x, want_status, want_it = IF.near_zero_reference(n, DOM)
        x, st, it = host_pass["zero", n]
        IF.check(n, x, st, want_x, want_status, DOM, "host, near zero", stats)
        assert np.array_equal(it, want_it), (n, it, want_it)
        assert np.all(st == 1), (n, st)
        iters = max(iters, int(it.max()))
    print(f"\nhost pass, solutions at and next to 0, n = 2 .. 64, {stats['rows']} rows: status 1 everywhere, worst "
          f"|x - restatement| {stats['x']:.2e} (b - a), bit for bit: {stats['bitwise']}; largest iteration count {iters}")


def test_host_pass_statuses_cover_no_one_and_several_solutions(host_pass):
    """The inputs exercise every outcome but -1: noise rows cross their targets several times, the line once."""
    seen = set()
    for n in NS:
        seen.update(int(s) for s in host_pass[n][1])
    assert 1 in seen and max(seen) > 1, seen
