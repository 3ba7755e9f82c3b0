"""roots(dim, fixed, level=t) against the reference's roots of its own model of f - t (tests/golden/
g33_level_inversion.npz, written by generate_golden_level_inversion.py): a 3-D approximation, the 1-D and 3-D golden
splines and a slider, three levels each, a dozen fixed rows.  The model here is built from f itself and asked for the
level; the counts must be equal and the roots agree within 1e-10 (b - a), the project's bar for roots.  The generator
asserts that every stored root is 1e-8 (b - a) clear of its neighbours and of the ends, so no row is left out.  The batch
form with one level per row must return what the single calls return, bit for bit."""
import os

import numpy as np
import pytest

import generate_golden_level_inversion as G

from pychebyshev_amd import ChebyshevApproximation, ChebyshevSlider, ChebyshevSpline

pytestmark = pytest.mark.gpu

CLASSES = {"approx": ChebyshevApproximation, "spline": ChebyshevSpline, "slider": ChebyshevSlider}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(G.__file__)), "g33_level_inversion.npz"))


@pytest.mark.parametrize("case", sorted(G.CASES))
def test_level_roots_match_the_reference_model_of_f_minus_t(golden, case):
    c = G.CASES[case]
    dim = c["dim"]
    a, b = c["domain"][dim]
    rows = G.fixed_rows(case)
    assert np.array_equal(rows, golden[f"{case}_rows"]) and np.array_equal(c["levels"], golden[f"{case}_levels"])
    model = G.build(CLASSES, case)
    worst = 0.0
    for i, t in enumerate(c["levels"]):
        want_R, want_c = golden[f"{case}_L{i}_roots"], golden[f"{case}_L{i}_count"]
        R, cnt = model.roots_batch(dim, rows, level=np.full(rows.shape[0], t))
        for r, row in enumerate(rows):
            got = model.roots(dim, G.fixed_dict(case, row), level=t)
            assert got.size == want_c[r], (case, t, r, got, want_R[r])
            if got.size:
                err = float(np.max(np.abs(got - want_R[r, :got.size]))) / (b - a)
                worst = max(worst, err)
                assert err <= 1e-10, (case, t, r, got, want_R[r])
            assert cnt[r] == got.size and np.array_equal(R[r, :cnt[r]], got), (case, t, r)
    print(f"{case}: worst |root - reference| {worst:.2e} (b - a)")


def test_one_batch_takes_a_level_per_row(golden):
    case = "approx"
    c = G.CASES[case]
    rows = G.fixed_rows(case)
    model = G.build(CLASSES, case)
    levels = np.resize(np.array(c["levels"]), rows.shape[0])
    R, cnt = model.roots_batch(c["dim"], rows, level=levels)
    for r in range(rows.shape[0]):
        i = r % len(c["levels"])
        assert cnt[r] == golden[f"{case}_L{i}_count"][r]
        assert np.max(np.abs(R[r, :cnt[r]] - golden[f"{case}_L{i}_roots"][r, :cnt[r]]), initial=0.0) <= 1e-10 * 2.0
