"""The device root solver on its own (calc_row of csrc/calculus_kernels.h through pcx_cheb1d_calculus) at every fibre
length n = 1 .. 64, by LDS class -- MP = 16 (n <= 17), 32 (n <= 33), 64 -- so that every class is filled (m = MP at
n = 17, 33) and left by one (n = 18, 34), and the callers on top of it at those lengths.

  a  parity with the NumPy restatement on the families of calc_fibres: counts equal, roots 1e-10 (b - a), exact NaN
     padding, extrema through _check_opt (1e-12 max|fibre|, 1e-8 (b - a)); constants and the zero fibre have no root
  b  T_(n-1) and (1 - x^2) U_(n-3) against their closed-form roots in extended precision: with E_ref the restatement's
     own worst error at that n, the device's is at most max(10 E_ref, 1e-13 (b - a)) -- two backward-stable eigenvalue
     solvers round differently (10 x), and where the reference lands on the last bit the ratio means nothing (the floor,
     1000 x under the project's 1e-10)
  c  every device root of a noise row with |t| < 1 - 1e-9: the Newton correction p / p' by Clenshaw on the row's own
     coefficients in extended precision, at most max(10 x the restatement's worst at that n, 1e-13); no eigenvalue
     solver and no count decision enters
  d  metamorphic relations, bit for bit (calc_fibres.check_metamorphic)
  e  a and b on the T rows over other intervals; on (0, 1e-9) the de-duplication scale 1e-10 (b - a + 1) merges roots by
     design, so there only the restatement is compared
  f  dense, TT, slider and spline batches with n in {17, 18, 33, 34, 64} along `dim`: every row against the restatement
     on the fibre the model itself evaluates.  The fragility predicate, which the families apply to noise rows only, is
     applied to these fibres too: a fragile row keeps its extremum check and loses its count and roots check, at most
     2 % of a batch's 64 rows (one row); the report prints how many were left out

The worst figures of a, b and c per class are printed (pytest -s) for DESIGN 3.6."""
import functools
import math

import numpy as np
import pytest

import calc_fibres as CF
from calc_fibres import _bary, _check_opt, _check_roots

from pychebyshev_amd import ChebyshevApproximation, ChebyshevSlider, ChebyshevSpline, ChebyshevTT, _calculus
from pychebyshev_amd.barycentric import chebyshev_nodes, compute_barycentric_weights, compute_differentiation_matrix

pytestmark = pytest.mark.gpu

DOM = (-1.0, 1.0)
CLASSES = sorted(CF.LDS_CLASSES)
STATS = {mp: {} for mp in CLASSES}
CALLERS = {}                          # worst figures of the caller tests (f)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for mp, s in STATS.items():
        print(f"\nsolver, LDS class {mp} (n = {CF.LDS_CLASSES[mp][0]} .. {CF.LDS_CLASSES[mp][-1]}): "
              f"a) roots {s.get('root', 0.0):.2e} (b-a), values {s.get('value', 0.0):.2e} max|f|; "
              f"b) closed form {s.get('closed', 0.0):.2e} (restatement {s.get('closed_ref', 0.0):.2e}); "
              f"c) Newton {s.get('newton', 0.0):.2e} (restatement {s.get('newton_ref', 0.0):.2e})")
    print(f"callers at the class boundaries: roots {CALLERS.get('root', 0.0):.2e} (b-a), values "
          f"{CALLERS.get('value', 0.0):.2e} max|f|, well-defined locations {CALLERS.get('location', 0.0):.2e} (b-a); "
          f"{CALLERS.get('skipped', 0)} of {CALLERS.get('rows', 0)} rows left out of the roots check as fragile")


def _worst(mp, key, v):
    STATS[mp][key] = max(STATS[mp].get(key, 0.0), float(v))


def _solve(n, V, mode, dom=DOM):
    x, w, D = CF.grid(n, *dom)
    return _calculus.cheb1d_calculus(V, x, w, None if mode == "roots" else D, dom, mode)


@functools.lru_cache(maxsize=None)
def _device_families(n, mode):
    """One call per n and mode: every family row."""
    return _solve(n, CF.families(n)[0], mode)


# ------------------------------------------------------------------ a: the restatement at every n
@pytest.mark.parametrize("mp", CLASSES)
def test_every_length_matches_the_restatement(mp):
    for n in CF.LDS_CLASSES[mp]:
        V, kinds = CF.families(n)
        for mode in CF.MODES:
            skipped = CF.check_rows(n, V, kinds, DOM, mode, _device_families(n, mode), f"n={n} {mode}", STATS[mp])
            assert skipped <= CF.MAX_FRAGILE * CF.NOISE_ROWS, (n, skipped)


# ------------------------------------------------------------------ b: closed forms
def _closed_form(n, dom, R, cnt, V, kinds, tag):
    """-> (device worst, restatement worst) against the exact roots of the T and lobatto rows, in units of b - a."""
    a, b = dom
    dev = ref = 0.0
    for kind in ("T", "lobatto"):
        if kind not in kinds:
            continue
        i = kinds.index(kind)
        exact = CF.exact_roots(kind, n, dom)
        want = CF.ref_roots(V[i], dom)
        assert cnt[i] == n - 1 == want.size, (tag, kind, int(cnt[i]), want.size)        # the roots row is full
        dev = max(dev, CF.hp_max_abs_diff(R[i], exact))
        ref = max(ref, CF.hp_max_abs_diff(want, exact))
    print(f"{tag}: closed form device {dev / (b - a):.2e} restatement {ref / (b - a):.2e} (b-a)")
    assert dev <= max(10.0 * ref, 1e-13 * (b - a)), (tag, dev, ref)
    return dev / (b - a), ref / (b - a)


@pytest.mark.parametrize("mp", CLASSES)
def test_closed_form_roots_within_ten_times_the_restatement(mp):
    for n in CF.LDS_CLASSES[mp]:
        if n < 2:
            continue
        V, kinds = CF.families(n)
        R, cnt = _device_families(n, "roots")
        dev, ref = _closed_form(n, DOM, R, cnt, V, kinds, f"n={n}")
        _worst(mp, "closed", dev)
        _worst(mp, "closed_ref", ref)


def test_lobatto_rows_return_the_endpoints_exactly():
    """The roots at +-1 of (1 - x^2) U_(n-3) come back as exactly lo and hi: an eigenvalue within 1e-10 of an end, on
    either side of it, is that end.  With the reference's one-sided clip an eigenvalue a few ulp inside [-1, 1] passed
    unchanged, and 44 of these 61 rows missed an endpoint on the device (39 in NumPy's chebroots), by up to 2.8e-15."""
    def solve(n):
        R, cnt = _device_families(n, "roots")
        i = CF.families(n)[1].index("lobatto")
        return R[i], cnt[i]
    missed = CF.missed_endpoints(DOM, solve, range(4, 65))
    assert not missed, missed


@pytest.mark.parametrize("dom", [(1e6, 1e6 + 1.0), (-1e-3, 1e-3), (-2.0, 3.0)])
def test_lobatto_rows_return_the_endpoints_exactly_on_other_intervals(dom):
    """lo and hi themselves, not 0.5 (lo + hi) +- 0.5 (hi - lo), which rounds (one ulp of 1e6 on the first interval)."""
    def solve(n):
        R, cnt = _solve(n, CF.lobatto_row(n)[None], "roots", dom)
        return R[0], cnt[0]
    missed = CF.missed_endpoints(dom, solve, CF.BOUNDARY_N)
    assert not missed, missed


# ------------------------------------------------------------------ c: Newton corrections in extended precision
def _interior(r):
    return r[np.abs(r) < 1.0 - 1e-9]


@pytest.mark.parametrize("mp", CLASSES)
def test_noise_roots_have_small_newton_corrections(mp):
    for n in CF.LDS_CLASSES[mp]:
        if n < 2:
            continue
        coef, V = CF.noise(n)
        R, cnt = _device_families(n, "roots")
        dev = ref = 0.0
        for i in range(CF.NOISE_ROWS):
            assert cnt[i] >= 0, (n, i)
            d = CF.hp_newton(coef[i], _interior(R[i, :cnt[i]]))
            r = CF.hp_newton(coef[i], _interior(CF.ref_roots(V[i], DOM)))
            dev = max(dev, float(np.max(np.abs(d), initial=0.0)))
            ref = max(ref, float(np.max(np.abs(r), initial=0.0)))
        print(f"n={n}: Newton correction device {dev:.2e} restatement {ref:.2e}")
        _worst(mp, "newton", dev)
        _worst(mp, "newton_ref", ref)
        assert dev <= max(10.0 * ref, 1e-13), (n, dev, ref)


# ------------------------------------------------------------------ d: metamorphic relations
@pytest.mark.parametrize("mp", CLASSES)
def test_metamorphic_relations_hold_bitwise(mp):
    for n in CF.LDS_CLASSES[mp]:
        out = {name: {mode: _solve(n, V, mode) for mode in CF.MODES} for name, V in CF.metamorphic_inputs(n).items()}
        CF.check_metamorphic(n, DOM, out, f"n={n}")


# ------------------------------------------------------------------ e: other intervals
@pytest.mark.parametrize("dom", [(1e6, 1e6 + 1.0), (-1e-3, 1e-3), (-2.0, 3.0)])
def test_boundary_lengths_on_other_intervals(dom):
    for n in CF.BOUNDARY_N:
        V, kinds = CF.t_row(n)[None], ("T",)
        for mode in CF.MODES:
            got = _solve(n, V, mode, dom)
            CF.check_rows(n, V, kinds, dom, mode, got, f"n={n} {dom} {mode}")
            if mode == "roots":
                _closed_form(n, dom, got[0], got[1], V, kinds, f"n={n} {dom}")


def test_boundary_lengths_on_a_tiny_interval():
    dom = (0.0, 1e-9)
    for n in CF.BOUNDARY_N:
        V = CF.t_row(n)[None]
        with np.errstate(all="ignore"):         # the barycentric weights overflow on this interval; roots do not read them
            CF.grid(n, *dom)
        CF.check_rows(n, V, ("T",), dom, "roots", _solve(n, V, "roots", dom), f"n={n} {dom}")


# ------------------------------------------------------------------ f: the callers at the class boundaries
ROWS = 64


def _f3(x, _=None):
    return math.sin(12.0 * x[0] + 0.3) + math.cos(9.0 * x[1] + x[2]) - 0.2 * x[2]


def _f2(x, _=None):
    return math.sin(14.0 * x[0] + 0.3) * (1.0 + 0.5 * x[1]) + 0.3 * math.cos(5.0 * x[0]) - 0.1


def _fixed_rows(domain, dim, seed):
    rng = np.random.default_rng([11, seed])
    return np.column_stack([rng.uniform(lo, hi, ROWS) for k, (lo, hi) in enumerate(domain) if k != dim])


def _check_callers(tag, dim, dom, grids, rows, fibres, value_at, roots_batch, minimize_batch):
    """Every row of a roots_batch and a minimize_batch call against the restatement.  `grids`: [(nodes, weights, D,
    (lo, hi))] per piece along dim (one entry unless the model is a spline), `fibres(r)`: the pieces' fibres of row r."""
    a, b = dom
    R, cnt = roots_batch(dim, rows)
    val, loc = minimize_batch(dim, rows)
    skipped = 0
    for r in range(rows.shape[0]):
        fib = fibres(r)
        scale = max(float(np.max(np.abs(np.concatenate(fib)))), 1e-300)
        found = [_calculus.optimize_1d(v, x, w, D, pd, "min") for v, (x, w, D, pd) in zip(fib, grids)]
        want = found[0] if len(grids) == 1 else _calculus.merge_pieces("min", found)
        _check_opt((val[r], loc[r]), want, scale, a, b, value_at(r), f"{tag} row {r} min", CALLERS)
        if any(CF.fragile(v) for v in fib):
            skipped += 1
            continue
        found = [_calculus.roots_1d(v, pd) for v, (x, w, D, pd) in zip(fib, grids)]
        want = found[0] if len(grids) == 1 else _calculus.merge_pieces("roots", found, dom)
        assert cnt[r] == want.size, (tag, r, int(cnt[r]), want.size)
        _check_roots(R[r, :cnt[r]], want, a, b, f"{tag} row {r}", CALLERS)
        assert np.all(np.isnan(R[r, cnt[r]:])), (tag, r)
    CALLERS["rows"] = CALLERS.get("rows", 0) + rows.shape[0]
    CALLERS["skipped"] = CALLERS.get("skipped", 0) + skipped
    assert skipped <= CF.MAX_FRAGILE * ROWS, (tag, skipped)


def _one_grid(x, dom):
    w = compute_barycentric_weights(x)
    return [(x, w, compute_differentiation_matrix(x, w), dom)]


@pytest.mark.parametrize("n", CF.BOUNDARY_N)
def test_dense_batches_at_the_class_boundaries(n):
    cols = CF.noise(n)[1][:3].T                      # (n, 3): every fibre along the long dimension is noise-like
    for dim, T in ((0, cols), (1, np.ascontiguousarray(cols.T))):
        domain = [[-1.0, 1.0], [0.0, 1.0]] if dim == 0 else [[0.0, 1.0], [-2.0, 3.0]]
        c = ChebyshevApproximation.from_values(T, 2, domain, list(T.shape))
        rows = _fixed_rows(domain, dim, n)
        dom = tuple(domain[dim])
        pts = np.concatenate([_calculus.fibre_points(2, dim, rows[r], c.nodes[dim]) for r in range(ROWS)])
        fib = c.vectorized_eval_batch(pts, [0, 0]).reshape(ROWS, n)
        _check_callers(f"dense n={n} dim={dim}", dim, dom, [(c.nodes[dim], c.weights[dim], c.diff_matrices[dim], dom)], rows,
                       lambda r: [fib[r]], lambda r: _bary(fib[r], c.nodes[dim], c.weights[dim]), c.roots_batch, c.minimize_batch)


@pytest.mark.parametrize("n", CF.BOUNDARY_N)
def test_tt_batches_at_the_class_boundaries(n):
    rng = np.random.default_rng([13, n])
    cores = [rng.standard_normal(s) for s in ((1, 4, 3), (3, n, 3), (3, 5, 1))]
    domain = [[-1.0, 1.0], [-2.0, 3.0], [0.0, 1.0]]
    tt = ChebyshevTT.from_coeff_cores(cores, domain)
    dim, dom = 1, (-2.0, 3.0)
    rows = _fixed_rows(domain, dim, n)
    x = chebyshev_nodes(dom[0], dom[1], n)
    grids = _one_grid(x, dom)
    pts = np.concatenate([_calculus.fibre_points(3, dim, rows[r], x) for r in range(ROWS)])
    fib = tt.eval_batch(pts).reshape(ROWS, n)
    _check_callers(f"tt n={n}", dim, dom, grids, rows, lambda r: [fib[r]], lambda r: _bary(fib[r], x, grids[0][1]),
                   tt.roots_batch, tt.minimize_batch)


@pytest.mark.parametrize("n", CF.BOUNDARY_N)
def test_slider_batches_at_the_class_boundaries(n):
    domain = [[-1.0, 1.0], [-1.0, 1.0], [0.0, 1.0]]
    for dim, n_nodes in ((1, [5, n, 4]), (0, [n, 5, 4])):       # a two-dimensional owner, and a one-dimensional one
        sl = ChebyshevSlider(_f3, 3, domain, n_nodes, partition=[[0], [1, 2]], pivot_point=[0.1, -0.2, 0.4])
        sl.build(verbose=False)
        dom = tuple(domain[dim])
        x, w, D = sl._owner_grid(dim)
        rows = _fixed_rows(domain, dim, n)
        pts = np.concatenate([_calculus.fibre_points(3, dim, rows[r], x) for r in range(ROWS)])
        fib = sl.eval_batch(pts, [0, 0, 0]).reshape(ROWS, n)
        _check_callers(f"slider n={n} dim={dim}", dim, dom, [(x, w, D, dom)], rows, lambda r: [fib[r]],
                       lambda r: _bary(fib[r], x, w), sl.roots_batch, sl.minimize_batch)


@pytest.mark.parametrize("pieces,knots", [([17, 18], [0.1]), ([33, 34, 64], [-0.3, 0.4])])
def test_spline_batches_mix_fibre_lengths_in_one_launch(pieces, knots):
    domain = [[-1.0, 1.0], [0.0, 1.0]]
    sp = ChebyshevSpline(_f2, 2, domain, n_nodes=[list(pieces), [3]], knots=[list(knots), []])
    sp.build(verbose=False)
    dim, dom = 0, (-1.0, 1.0)
    rows = _fixed_rows(domain, dim, len(pieces))
    _, along, _ = sp._calculus_pieces(dim, {1: float(rows[0, 0])})
    assert [p.n_nodes[dim] for p in along] == list(pieces)
    grids = [(p.nodes[dim], p.weights[dim], p.diff_matrices[dim], tuple(p.domain[dim])) for p in along]
    pts = np.concatenate([_calculus.fibre_points(2, dim, rows[r], g[0]) for r in range(ROWS) for g in grids])
    vals = sp.eval_batch(pts, [0, 0]).reshape(ROWS, sum(pieces))
    cuts = np.cumsum(pieces)[:-1]

    def value_at(r):
        return lambda t: float(sp.eval([float(t), float(rows[r, 0])], [0, 0]))
    _check_callers(f"spline {pieces}", dim, dom, grids, rows, lambda r: np.split(vals[r], cuts), value_at,
                   sp.roots_batch, sp.minimize_batch)
