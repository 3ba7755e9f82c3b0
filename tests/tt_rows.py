"""Shared by the tensor-train body tests on the GPU (tests/test_gpu_tt_lane_bodies.py, tests/test_gpu_tt_mfma_bodies.py):
a model of tests/tt_chain.py on the device, and one call held to the long-double chain."""
import numpy as np

import tt_chain as C
from pychebyshev_amd import ChebyshevTT, _lib


def model(b):
    return ChebyshevTT.from_coeff_cores(b.cores, b.domain, dim_order=b.order)


def set_kernel(tt, variant):
    t = tt._dev()
    _lib.check(t.lib.pcx_tt_set_kernel(t.handle, variant), t.lib)


def check(seen, got, pair, group, kernel, family, what):
    """One call against the long-double chain: the normwise bar, then every row against its own amplitude.  ``seen``
    collects the worst row per (group, kernel, family) of the calling module."""
    ref, amp = pair
    got = np.asarray(got)
    assert got.shape == ref.shape and got.dtype == np.float64, what
    err = np.abs(got.astype(C.LD) - ref)
    scale = float(np.max(np.abs(ref)))
    r = C.ratios(got, ref, amp)                      # asserts an exact zero where the amplitude is zero
    worst = float(np.max(r))
    key = f"{group} {kernel} {family}"
    seen[key] = max(seen.get(key, 0.0), worst)
    print(f"{what}: E_norm {float(np.max(err)) / scale if scale else 0.0:.2e}, worst row {worst:.3f} eps A_row "
          f"(K = {C.K[group][family]})")
    assert float(np.max(err)) <= 1e-12 * scale, f"{what}: E_norm {float(np.max(err)) / scale:.3e}"
    at = np.unravel_index(int(np.argmax(r)), r.shape)
    assert worst <= C.K[group][family], \
        f"{what}: row {at}: |got - ref| = {worst:.3g} eps A_row > K = {C.K[group][family]} (got {got[at]!r}, ref {float(ref[at])!r})"
