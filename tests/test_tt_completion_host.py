"""CPU-only checks of ChebyshevTT.orth_left / orth_right / run_completion: the public surface, the argument errors
(all raised before the library is touched) and the golden file's own rel_change bookkeeping.  No GPU compute here."""
import inspect

import numpy as np
import pytest

from conftest import golden

from pychebyshev_amd import ChebyshevTT, _lib

SMALL = ("M1", "M2", "M3", "M4")


def _tt(d=3):
    rng = np.random.default_rng(5)
    ranks = [1] + [2] * (d - 1) + [1]
    cores = [rng.standard_normal((ranks[k], 4, ranks[k + 1])) for k in range(d)]
    return ChebyshevTT.from_coeff_cores(cores, [[-1.0, 1.0]] * d)


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the HIP library fails the test: the argument checks must come first."""
    def boom(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", boom)


def test_methods_exist_with_the_reference_signatures():
    for name in ("orth_left", "orth_right"):
        sig = inspect.signature(getattr(ChebyshevTT, name))
        assert list(sig.parameters) == ["self", "position"]
    sig = inspect.signature(ChebyshevTT.run_completion)
    assert list(sig.parameters) == ["self", "tolerance", "max_iter", "verbose", "values"]
    assert sig.parameters["tolerance"].default == 1e-8
    assert sig.parameters["max_iter"].default == 50
    assert sig.parameters["verbose"].default is False
    assert sig.parameters["values"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["values"].default is None


def test_completion_info_is_none_on_a_fresh_object():
    assert _tt().completion_info is None
    assert ChebyshevTT(lambda p, _: 0.0, 2, [[0, 1]] * 2, [3, 3]).completion_info is None


def test_unbuilt_object_raises_runtime_error(no_library):
    tt = ChebyshevTT(lambda p, _: 0.0, 3, [[0, 1]] * 3, [3, 3, 3])
    for call in (lambda: tt.orth_left(1), lambda: tt.orth_right(0), lambda: tt.run_completion(),
                 lambda: tt.run_completion(values=np.zeros((3, 3, 3)))):
        with pytest.raises(RuntimeError, match="build"):
            call()


@pytest.mark.parametrize("position", [0, -1, 3, 7])
def test_orth_left_position_out_of_range(no_library, position):
    with pytest.raises(ValueError, match=rf"position must be in \[1, 2\] for orth_left, got {position}"):
        _tt(3).orth_left(position)


@pytest.mark.parametrize("position", [-1, 2, 5])
def test_orth_right_position_out_of_range(no_library, position):
    with pytest.raises(ValueError, match=rf"position must be in \[0, 1\] for orth_right, got {position}"):
        _tt(3).orth_right(position)


def test_one_dimensional_tt_has_no_valid_position(no_library):
    tt = _tt(1)
    with pytest.raises(ValueError):
        tt.orth_left(0)
    with pytest.raises(ValueError):
        tt.orth_right(0)


def test_run_completion_without_function_or_values(no_library):
    with pytest.raises(RuntimeError, match="run_completion requires self.function to be callable"):
        _tt().run_completion()


def test_run_completion_values_are_checked(no_library):
    tt = _tt()
    with pytest.raises(ValueError, match="shape"):
        tt.run_completion(values=np.zeros((4, 4)))
    with pytest.raises(ValueError, match="shape"):
        tt.run_completion(values=np.zeros((4, 4, 5)))
    bad = np.zeros((4, 4, 4))
    bad[1, 2, 3] = np.nan
    with pytest.raises(ValueError, match="NaN or Inf"):
        tt.run_completion(values=bad)
    bad[1, 2, 3] = np.inf
    with pytest.raises(ValueError, match="NaN or Inf"):
        tt.run_completion(values=bad)
    with pytest.raises(TypeError):
        tt.run_completion(1e-8, 50, False, np.zeros((4, 4, 4)))       # keyword only


def test_build_method_als_still_raises():
    tt = ChebyshevTT(lambda p, _: 0.0, 2, [[0, 1]] * 2, [3, 3])
    with pytest.raises(NotImplementedError):
        tt.build(verbose=False, method="als")


def test_abi_table_has_the_two_entry_points():
    assert len(_lib.SIGNATURES["pcx_tt_orth"][1]) == 11
    assert len(_lib.SIGNATURES["pcx_tt_als"][1]) == 15
    assert len(_lib.SIGNATURES["pcx_tt_als_project"][1]) == 10
    assert len(_lib.SIGNATURES["pcx_tt_als_qr"][1]) == 6
    assert len(_lib.SIGNATURES["pcx_tt_als_norms"][1]) == 6


@pytest.mark.parametrize("tag", SMALL)
def test_golden_rel_change_matches_numpy_on_the_stored_tensors(tag):
    g = golden("g23_tt_completion")
    tensors = [g[f"{tag}_dense_m{m}"] for m in range(3)]
    want = [np.linalg.norm(tensors[i + 1] - tensors[i]) / (np.linalg.norm(tensors[i]) + 1e-30) for i in range(2)]
    np.testing.assert_allclose(g[f"{tag}_rel_change"][:2], want, rtol=1e-12, atol=0.0)
    assert g[f"{tag}_rel_change"].shape == (3,)
    assert g[f"{tag}_T"].shape == tuple(int(v) for v in g[f"{tag}_n"])


def test_golden_tolerance_run_has_its_margin():
    g = golden("g23_tt_completion")
    hist, tol, iters = g["M4_tol_history"], float(g["M4_tol"]), int(g["M4_tol_iters"])
    assert np.all(hist[:iters - 1] >= 10.0 * tol) and hist[iters - 1] <= tol / 10.0
