"""The dense device steps of TT completion (csrc/tt_als_kernels.h) called one at a time through the diagnostic hooks of
pychebyshev_amd.tensor_train (pcx_tt_als_project, pcx_tt_als_qr, pcx_tt_als_norms), on the tables of
tests/als_steps.py: both contractions in the VALU and in the MFMA form at every rank class, K % 4 tail and R tail,
exact on integers, within the dot-product bound on Gaussians, and with a NaN that must stay in its column; the
Householder QR on every shape class and seven matrix families, and on inputs scaled by 2^-900 .. 2^900; the four
convergence sums on integers past the fixed grid; and run_completion / orth_left / orth_right above rank 32 and at the
limits of 256.  Every bar is exact equality, a derived rounding bound, or a stated multiple of the NumPy restatement's
own error; none is taken from the kernel."""
import ctypes
import functools
import os

import numpy as np
import pytest

import als_steps as AS
from conftest import assert_parity, parity
from pychebyshev_amd import ChebyshevTT, _lib
from pychebyshev_amd import tensor_train as tt_mod

pytestmark = pytest.mark.gpu

EPS = AS.EPS
FORMS = (AS.FORM_VALU, AS.FORM_MFMA, AS.FORM_AUTO)
FORM_NAME = {AS.FORM_VALU: "valu", AS.FORM_MFMA: "mfma", AS.FORM_AUTO: "auto"}
SWITCH_MOVED = "PCX_TT_ALS_MFMA_MIN" in os.environ
RATIOS = {}                     # what -> the largest figure / bar met


def _note(what, ratio):
    RATIOS[what] = max(RATIOS.get(what, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if RATIOS:
        print("\nALS steps, worst figure / bar: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(RATIOS.items())))


# ------------------------------------------------------------------ contractions
@pytest.mark.parametrize("case", AS.CASES, ids=AS.case_id)
def test_contractions_of_integers_are_exact(case):
    """Integers up to 2^10: every product and every partial sum is exact in any order, so all three forms on both sides
    return the int64 product bit for bit -- every element written (the buffer starts as NaN), none beyond (the guard
    behind it).  form 0 runs the VALU form below rank 16 and the MFMA form from 16 on."""
    r, K, R = case
    want = AS.integer_product(r, K, R).astype(float)
    for side, small, big in AS.sides(*AS.integer_factors(r, K, R)):
        ref = want if side == 0 else want.T
        for form in FORMS:
            got, used = tt_mod._als_project(side, small, big, form)
            assert got.shape == ref.shape
            bad = np.argwhere(got != ref)
            assert bad.size == 0, (side, FORM_NAME[form], len(bad), bad[:4].tolist())
            if form != AS.FORM_AUTO:
                assert used == form
            elif not SWITCH_MOVED:
                assert used == AS.dispatch(r, AS.FORM_AUTO)[0] == (AS.FORM_MFMA if r >= 16 else AS.FORM_VALU)


@pytest.mark.parametrize("case", AS.ROUNDING_CASES, ids=AS.case_id)
def test_contractions_of_gaussians_within_the_dot_product_bound(case):
    """Per element |out - ref| <= K eps sum_k |a_k b_k| against the longdouble product: the bound of a K-term dot product
    in any summation order (als_steps.gaussian_product)."""
    r, K, R = case
    ref, bar = AS.gaussian_product(r, K, R)
    for side, small, big in AS.sides(*AS.gaussian_factors(r, K, R)):
        for form in FORMS:
            got, _ = tt_mod._als_project(side, small, big, form)
            got = got if side == 0 else got.T
            worst = float(np.max(np.abs(got.astype(AS.LD) - ref) / bar))
            print(f"{AS.case_id(case)} side {side} {FORM_NAME[form]}: {worst:.4f} of the bound")
            _note(f"contraction/{FORM_NAME[form]}", worst)
            assert worst <= 1.0, (side, FORM_NAME[form], worst)


@pytest.mark.parametrize("form", [AS.FORM_VALU, AS.FORM_MFMA], ids=["valu", "mfma"])
@pytest.mark.parametrize("r", AS.NAN_RANKS)
def test_one_nan_stays_in_its_column(r, form):
    """One NaN in the large operand at (k, j): exactly output column j (left) or row j (right) is NaN, everything else
    is the exact integer product.  A zero-padded lane that multiplied it, or a tile read past its edge, would spread it."""
    K, R = 7, 65
    Q, P = AS.integer_factors(r, K, R)
    want = AS.integer_product(r, K, R).astype(float)
    for (k, j) in ((0, 0), (K - 1, R - 1), (3, 16), (4, 63), (6, 64)):
        Pn = np.array(P)
        Pn[k, j] = np.nan
        for side, small, big in AS.sides(Q, Pn):
            got, _ = tt_mod._als_project(side, small, big, form)
            got = got if side == 0 else got.T
            assert np.all(np.isnan(got[:, j])), (side, k, j)
            keep = np.arange(R) != j
            assert np.array_equal(got[:, keep], want[:, keep]), (side, k, j, np.argwhere(got[:, keep] != want[:, keep])[:4].tolist())


def test_projection_arguments_are_checked():
    one = np.ones((1, 1))
    lib = _lib.load()
    used = ctypes.c_int32(0)
    out = np.zeros(4)
    call = lambda side, form, K, r, R: lib.pcx_tt_als_project(0, side, form, _lib.p_f64(out), _lib.p_f64(out), _lib.p_f64(out),
                                                               K, r, R, ctypes.byref(used))
    assert call(2, 0, 1, 1, 1) == _lib.PCX_ERR_INVALID and call(0, 3, 1, 1, 1) == _lib.PCX_ERR_INVALID
    assert call(0, 0, 0, 1, 1) == _lib.PCX_ERR_INVALID and call(0, 0, 1, 0, 1) == _lib.PCX_ERR_INVALID
    assert call(1, 0, 1, 1, 0) == _lib.PCX_ERR_INVALID
    assert call(0, 1, 1, AS.MAX_RANK + 1, 1) == _lib.PCX_ERR_UNSUPPORTED
    assert call(1, 2, 2, 1, AS.MAX_GRID // 2 + 1) == _lib.PCX_ERR_UNSUPPORTED
    got, used_form = tt_mod._als_project(0, one, one, 2)
    assert got.tolist() == [[1.0]] and used_form == 2


# ------------------------------------------------------------------ Householder QR
@functools.lru_cache(maxsize=None)
def _factored(m, c, fam):
    Q, R = tt_mod._als_qr(AS.hh_matrix(m, c, fam))
    Q.setflags(write=False)
    R.setflags(write=False)
    return Q, R


@pytest.mark.parametrize("m,c,fam", AS.HH_CASES, ids=[AS.hh_id(k) for k in AS.HH_CASES])
def test_householder_families(m, c, fam):
    """Q (m x p) orthonormal and QR = A to 8 times the figures of the float64 restatement (floor m eps), R exactly zero
    below the diagonal; flat: entrywise against the longdouble restatement at 8 times the float64 restatement's distance
    from it, with its diagonal signs; triu and zero: the identity and the input, bit for bit."""
    A = AS.hh_matrix(m, c, fam)
    p = min(m, c)
    Q, R = _factored(m, c, fam)
    assert Q.shape == (m, p) and R.shape == (p, c)
    assert not np.tril(R[:, :p], -1).any(), "R has a nonzero below its diagonal"
    assert np.all(np.isfinite(Q)) and np.all(np.isfinite(R))
    orth, resid = AS.qr_figures(A, Q, R)
    orth_ref, resid_ref = AS.restated_figures(m, c, fam)
    bars = max(8.0 * orth_ref, m * EPS), max(8.0 * resid_ref, m * EPS)
    print(f"{AS.hh_id((m, c, fam))}: max|Q^T Q - I| {orth:.2e} (restated {orth_ref:.2e}), |QR - A|/|A| {resid:.2e} "
          f"(restated {resid_ref:.2e}), m eps {m * EPS:.2e}")
    _note("qr/orthogonality", orth / bars[0])
    _note("qr/residual", resid / bars[1])
    assert orth <= bars[0] and resid <= bars[1]
    if fam == "flat":
        Ql, Rl = AS.restated(m, c, fam, True)
        dq, dr = AS.restated_distance(m, c, fam)
        eq, er = float(np.max(np.abs(Q.astype(AS.LD) - Ql))), float(np.max(np.abs(R.astype(AS.LD) - Rl)))
        print(f"    against longdouble: Q {eq:.2e} (restated {dq:.2e}), R {er:.2e} (restated {dr:.2e})")
        if dq > 0.0:
            _note("qr/Q entrywise", eq / (8.0 * dq))
        if dr > 0.0:
            _note("qr/R entrywise", er / (8.0 * dr))
        assert eq <= 8.0 * dq and er <= 8.0 * dr
        assert np.array_equal(np.sign(np.diag(R)), np.sign(np.diag(Rl)).astype(float))
    if fam == "triu":
        assert Q.tobytes() == np.eye(m, p).tobytes() and R.tobytes() == A[:p].tobytes()
    if fam == "zero":
        assert Q.tobytes() == np.eye(m, p).tobytes() and not R.any()


@pytest.mark.parametrize("m,c,fam", [(257, 16, "gaussian"), (65, 64, "dupcol"), (7, 8, "flat"), (512, 256, "graded")])
def test_householder_twice_gives_equal_bits(m, c, fam):
    Q, R = _factored(m, c, fam)
    Q2, R2 = tt_mod._als_qr(AS.hh_matrix(m, c, fam))
    assert Q.tobytes() == Q2.tobytes() and R.tobytes() == R2.tobytes()


@pytest.mark.parametrize("m,c", AS.SCALE_SHAPES)
def test_householder_is_scale_free(m, c):
    """A 2^e for e = -900 .. 900: Q bit for bit that of A, R = ldexp(R_0, e) bit for bit.  Q is homogeneous of degree 0
    and R of degree 1, and the kernel squares each column times an exact power of two."""
    A = AS.scale_matrix(m, c)
    Q0, R0 = tt_mod._als_qr(A)
    for e in AS.SCALE_EXPONENTS:
        Ae = np.ldexp(A, e)
        assert np.array_equal(np.ldexp(Ae, -e), A), "the scaled input must be exact"
        Q, R = tt_mod._als_qr(Ae)
        want = np.ldexp(R0, e)
        with np.errstate(invalid="ignore"):
            print(f"{m}x{c} e = {e}: max|Q - Q_0| {np.max(np.abs(Q - Q0)):.2e}, "
                  f"max|R 2^-e - R_0| / max|R_0| {np.max(np.abs(np.ldexp(R, -e) - R0)) / np.max(np.abs(R0)):.2e}")
        assert Q.tobytes() == Q0.tobytes(), e
        assert R.tobytes() == want.tobytes(), e


def test_qr_arguments_are_checked():
    lib = _lib.load()
    buf = np.zeros(4)
    call = lambda m, c: lib.pcx_tt_als_qr(0, _lib.p_f64(buf), m, c, _lib.p_f64(buf), _lib.p_f64(buf))
    assert call(0, 1) == _lib.PCX_ERR_INVALID and call(1, 0) == _lib.PCX_ERR_INVALID
    assert call(1, AS.MAX_RANK + 1) == _lib.PCX_ERR_UNSUPPORTED and call(AS.MAX_GRID // 2 + 1, 2) == _lib.PCX_ERR_UNSUPPORTED


# ------------------------------------------------------------------ norms
@pytest.mark.parametrize("G", AS.NORM_G)
def test_norms_of_integer_tensors_are_exact(G):
    """Integers up to 2^8: the four sums are exact in any order and equal the Python-integer sums bit for bit, on one
    block, on both sides of a full block, and past the 1024 x 256 grid where a thread takes a second element."""
    tnew, tprev, target = AS.norm_tensors(G)
    got = tt_mod._als_norms(tnew, tprev, target)
    assert got.tolist() == [float(s) for s in AS.norm_sums(tnew, tprev, target)]
    same = tt_mod._als_norms(tnew, tnew, tnew)
    s = float(AS.norm_sums(tnew, tnew, tnew)[1])
    assert same.tolist() == [0.0, s, 0.0, s]
    zero = tt_mod._als_norms(tnew, tprev, np.zeros(G))
    want = AS.norm_sums(tnew, tprev, np.zeros(G, dtype=np.int64))
    assert zero.tolist() == [float(v) for v in want] and zero[3] == 0.0 and zero[2] == float(int((tnew ** 2).sum())) > 0.0


# ------------------------------------------------------------------ end to end above rank 32 and at the limits
@functools.lru_cache(maxsize=None)
def _model(index):
    truth, start = AS.e2e_cores(index)
    T = AS.dense(truth)
    T.setflags(write=False)
    return T, start


@pytest.mark.parametrize("index", range(len(AS.E2E_MODELS)), ids=["r40", "r35", "r256"])
def test_exact_rank_target_above_rank_32(index):
    """One outer iteration from a random start recovers an exact-rank target: grid residual <= 1e-12, and the dense
    tensor equals that of NumPy's projection ALS from the same start at the project's 1e-12 normwise bar,
    max|got - want| / max|want|.  (An entry here is a sum of up to 65536 signed products that cancel, so the pointwise
    relative figure of assert_parity, printed below, is not bounded by the normwise one.)"""
    n, ranks = AS.E2E_MODELS[index]
    T, start = _model(index)
    tt = ChebyshevTT.from_coeff_cores(start, [[-1.0, 1.0]] * len(n))
    want = AS.dense(AS.numpy_als([tt_mod._coeff_core_to_value_core(c) for c in start], T, 1))
    print(f"n {n} ranks {ranks}: NumPy ALS |got - T|/|T| = {np.linalg.norm(want - T) / np.linalg.norm(T):.2e}")
    tt.run_completion(max_iter=1, values=T)
    print(f"    device: {tt.completion_info}, ranks {tt.tt_ranks}")
    assert tt.completion_info["iterations"] == 1 and tt.tt_ranks == ranks
    assert tt.completion_info["grid_residual"] <= 1e-12
    e_norm, e_point = parity(tt.to_dense(), want)
    print(f"    to_dense vs NumPy projection ALS: normwise {e_norm:.2e}, pointwise on the significant entries {e_point:.2e}")
    _note("end to end/to_dense normwise", e_norm / 1e-12)
    assert e_norm <= 1e-12


@pytest.mark.parametrize("side", ["left", "right"])
def test_orthogonalisation_above_rank_32(side):
    """orth_left / orth_right at every position of the rank 33 / 34 / 35 model, with the assertions of
    test_gpu_tt_completion.test_orthogonalisation_every_position."""
    n, ranks = AS.E2E_MODELS[AS.ORTH_MODEL]
    cores = _model(AS.ORTH_MODEL)[1]
    d = len(cores)
    domain = [[-1.0, 1.0]] * d
    pts = np.random.default_rng(3).uniform(-1.0, 1.0, (64, d))
    before = ChebyshevTT.from_coeff_cores(cores, domain).eval_batch(pts)
    for position in (range(1, d) if side == "left" else range(0, d - 1)):
        tt = ChebyshevTT.from_coeff_cores(cores, domain)
        getattr(tt, f"orth_{side}")(position)
        for k, (m, e_lapack, bond) in AS.lapack_sweep(cores, side, position).items():
            c = tt._coeff_cores[k]
            U = c.reshape(-1, c.shape[2]) if side == "left" else c.reshape(c.shape[0], -1).T
            assert U.shape[1] == bond
            err = float(np.max(np.abs(U.T @ U - np.eye(bond))))
            print(f"orth_{side}({position}) core {k}: {err:.2e} (LAPACK {e_lapack:.2e}, m eps {m * EPS:.2e})")
            assert err <= max(8.0 * e_lapack, m * EPS)
        untouched = range(position + 1, d) if side == "left" else range(0, position)
        for k in untouched:
            assert np.array_equal(tt._coeff_cores[k], cores[k]), f"core {k} beyond the pivot changed"
        assert tt.tt_ranks == [1] + [c.shape[2] for c in tt._coeff_cores]
        assert_parity(tt.eval_batch(pts), before, tol=1e-12, what=f"orth_{side}({position})")


@pytest.mark.parametrize("n,ranks", [([2, 2], [1, 257, 1]), ([257, 2], [1, 2, 1]), ([2, 257], [1, 2, 1]),
                                     ([256, 256, 256, 17], [1, 1, 1, 1, 1])], ids=["rank257", "nodes257", "nodes257_last", "grid"])
def test_beyond_the_limits_is_unsupported(n, ranks):
    """A rank or a node count of 257, and a grid above 2^28 points, come back as PCX_ERR_UNSUPPORTED from correctly
    sized zero buffers (the target of the last is never touched: its pages are never mapped)."""
    lib = _lib.load()
    d = len(n)
    size = sum(ranks[k] * n[k] * ranks[k + 1] for k in range(d))
    nn, rr = _lib.i32(n), _lib.i32(ranks)
    cores, out = np.zeros(size), np.zeros(size)
    ranks_out = np.zeros(d + 1, dtype=np.int32)
    length, iters, resid = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_double(0.0)
    history = np.zeros(1)
    target = np.zeros(int(np.prod(n, dtype=np.int64)))
    rc = lib.pcx_tt_als(0, d, _lib.p_i32(nn), _lib.p_i32(rr), _lib.p_f64(cores), _lib.p_f64(target), 0.0, 1,
                        _lib.p_i32(ranks_out), _lib.p_f64(out), out.size, ctypes.byref(length), ctypes.byref(iters),
                        _lib.p_f64(history), ctypes.byref(resid))
    assert rc == _lib.PCX_ERR_UNSUPPORTED, (rc, _lib.last_error(lib))
    assert not out.any() and length.value == 0
    if int(np.prod(n, dtype=np.int64)) <= AS.MAX_GRID:
        rc = lib.pcx_tt_orth(0, d, _lib.p_i32(nn), _lib.p_i32(rr), _lib.p_f64(cores), 0, 1, _lib.p_i32(ranks_out),
                             _lib.p_f64(out), out.size, ctypes.byref(length))
        assert rc == _lib.PCX_ERR_UNSUPPORTED, (rc, _lib.last_error(lib))
