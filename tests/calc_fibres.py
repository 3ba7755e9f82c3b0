"""Shared by the calculus tests: the result checks, seeded fibre families for the root solver (calc_row of
csrc/calculus_kernels.h), their closed-form roots in extended precision and the comparison with the NumPy restatement
(pychebyshev_amd._calculus.roots_1d / optimize_1d).  Plain NumPy, no GPU.

A fibre is the row of n values of a 1-D interpolant at its n ascending type-I nodes; the families are value rows in the
reference frame (the nodes chebyshev_nodes(-1, 1, n)), so the same row serves every physical interval:

  noise     NOISE_ROWS rows chebval(t, standard_normal(n)) from default_rng([7, n]): no decay, up to 48 real roots at 64
  T         T_(n-1) at n nodes (n >= 2): the roots row is full, roots cos((2j - 1) pi / 2(n - 1))
  lobatto   (1 - t^2) U_(n-3)(t) (n >= 4): full row again, roots cos(j pi / (n - 2)), both endpoints among them
  specials  the constants 5, -1, 1e-3, the zero fibre and the exact line t - 0.25

Two correct eigenvalue solvers may decide differently on a row whose raw eigenvalues sit on one of the solver's
thresholds; `fragile` names those rows from the restatement's own raw chebroots output, and the comparison leaves their
counts and roots out.  Only noise rows can be left out, and at most MAX_FRAGILE of them per n."""
import contextlib
import decimal
import functools

import numpy as np
from numpy.polynomial.chebyshev import chebroots, chebval

from pychebyshev_amd import ChebyshevApproximation, _calculus
from pychebyshev_amd.barycentric import chebyshev_nodes, compute_barycentric_weights, compute_differentiation_matrix

WORST = {"root": 0.0, "value": 0.0, "location": 0.0}


def _check_roots(got, want, a, b, tag, worst=WORST):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, got, want)
    if want.size:
        err = float(np.max(np.abs(got - want))) / (b - a)
        worst["root"] = max(worst.get("root", 0.0), err)
        assert err <= 1e-10, (tag, got, want)


def _check_opt(got, want, scale, a, b, value_at, tag, worst=WORST):
    """got / want = (value, location); value_at(x) evaluates the interpolant along the fibre."""
    ev = abs(got[0] - want[0]) / scale
    worst["value"] = max(worst.get("value", 0.0), ev)
    assert ev <= 1e-12, (tag, got, want)
    el = abs(got[1] - want[1]) / (b - a)
    if el <= 1e-8:
        worst["location"] = max(worst.get("location", 0.0), el)
    else:       # not well defined: a flat optimum or a tie -- the point found must be as good
        assert a <= got[1] <= b, (tag, got, want)
        assert abs(value_at(got[1]) - want[0]) <= 1e-12 * scale, (tag, got, want)


def _bary(v, x, w):
    def at(t):
        d = t - x
        hit = np.nonzero(np.abs(d) < 1e-14)[0]
        if hit.size:
            return float(v[hit[0]])
        u = w / d
        return float(u @ v / u.sum())
    return at


# ---------------------------------------------------------------------------------------------- the families
NOISE_ROWS = 30
MAX_FRAGILE = 0.02                    # of the noise rows of one n
MODES = ("roots", "min", "max")
LDS_CLASSES = {16: range(1, 18), 32: range(18, 34), 64: range(34, 65)}     # MP -> the fibre lengths n with n - 1 <= MP
BOUNDARY_N = (17, 18, 33, 34, 64)     # a full class, the first length of the next one, the longest fibre


@functools.lru_cache(maxsize=None)
def grid(n, lo=-1.0, hi=1.0):
    """Nodes, barycentric weights and differentiation matrix of n type-I nodes on [lo, hi], as the models build them."""
    x = chebyshev_nodes(lo, hi, n)
    w = compute_barycentric_weights(x)
    return x, w, compute_differentiation_matrix(x, w)


@functools.lru_cache(maxsize=None)
def noise(n):
    """(coefficients, values), NOISE_ROWS x n each."""
    coef = np.random.default_rng([7, n]).standard_normal((NOISE_ROWS, n))
    t = grid(n)[0]
    return coef, np.array([chebval(t, c) for c in coef])


def t_row(n):
    return np.cos((n - 1) * np.arccos(grid(n)[0]))


def lobatto_row(n):
    th = np.arccos(grid(n)[0])
    return np.sin(th) * np.sin((n - 2) * th)


def specials(n):
    return np.array([np.full(n, 5.0), np.full(n, -1.0), np.full(n, 1e-3), np.zeros(n), grid(n)[0] - 0.25])


@functools.lru_cache(maxsize=None)
def families(n):
    """(values (rows, n), kinds): noise, then T (n >= 2), lobatto (n >= 4), the three constants, zero, the line."""
    rows, kinds = [noise(n)[1]], ["noise"] * NOISE_ROWS
    if n >= 2:
        rows.append(t_row(n)[None])
        kinds.append("T")
    if n >= 4:
        rows.append(lobatto_row(n)[None])
        kinds.append("lobatto")
    rows.append(specials(n))
    kinds += ["const", "const", "const", "zero", "line"]
    V = np.concatenate(rows)
    V.setflags(write=False)
    return V, tuple(kinds)


def mixed_batch(n):
    """Rows of every kind in one launch: zero, constant, line, T, noise, a NaN row, a +-inf row, noise."""
    v = noise(n)[1]
    nan_row, inf_row = v[2].copy(), v[3].copy()
    nan_row[n // 2] = np.nan
    inf_row[0] = np.inf
    inf_row[n - 1] = -np.inf if n > 1 else np.inf
    sp = specials(n)
    return np.array([sp[3], sp[0], sp[4], t_row(n), v[0], nan_row, inf_row, v[1]]), (5, 6)


# ---------------------------------------------------------------------------------------------- fragile rows
def raw_eigenvalues(values):
    """What the restatement's chebroots returns before any filter (empty below degree 1)."""
    return np.atleast_1d(chebroots(ChebyshevApproximation._chebyshev_coefficients_1d(values))).astype(complex)


def _memo(fn):
    """Cache fn(values, *key) by the row's bytes: the tests of one module ask for the same reference more than once."""
    cache = {}

    @functools.wraps(fn)
    def cached(values, *key):
        k = (np.asarray(values, dtype=float).tobytes(),) + key
        if k not in cache:
            out = cache[k] = fn(values, *key)
            if isinstance(out, np.ndarray):
                out.setflags(write=False)
        return cache[k]
    return cached


@_memo
def fragile(values):
    """True when a count or a kept root of this row hangs on a threshold of the filter: an eigenvalue with
    |re| <= 1 + 1e-6 and 1e-13 < |imag| < 1e-7 (the 1e-10 cut on |imag|), two kept roots closer than 1e-7 (a nearly
    double root, and the de-duplication), or an eigenvalue within 1e-7 of the cut-off +-(1 + 1e-10) itself."""
    ev = raw_eigenvalues(values)
    if not ev.size:
        return False
    near = np.abs(ev.real) <= 1.0 + 1e-6
    if np.any(near & (np.abs(ev.imag) > 1e-13) & (np.abs(ev.imag) < 1e-7)):
        return True
    kept = np.sort(ev.real[(np.abs(ev.imag) < 1e-10) & (np.abs(ev.real) <= 1.0 + 1e-10)])
    if kept.size > 1 and np.min(np.diff(kept)) < 1e-7:
        return True
    cut = 1.0 + 1e-10
    return bool(np.any(np.minimum(np.abs(ev - cut), np.abs(ev + cut)) < 1e-7))


# ---------------------------------------------------------------------------------------------- the restatement
@_memo
def ref_roots(values, dom):
    """roots_1d, or None where it raises (a fibre that is not finite): the device's count -1."""
    try:
        with np.errstate(invalid="ignore", divide="ignore"):
            return _calculus.roots_1d(values, dom)
    except np.linalg.LinAlgError:
        return None


@_memo
def ref_opt(values, n, dom, mode):
    x, w, D = grid(n, *dom)
    try:
        with np.errstate(invalid="ignore", divide="ignore"):
            return _calculus.optimize_1d(values, x, w, D, dom, mode)
    except np.linalg.LinAlgError:
        return None


def check_rows(n, V, kinds, dom, mode, got, tag, stats=None):
    """One call's outputs (`got`: (roots, counts) or (values, locations, counts)) on the rows V against the restatement:
    counts equal, roots within 1e-10 (b - a), the NaN padding exact, extrema through _check_opt; constants and the zero
    fibre have no root.  A fibre the restatement refuses has count -1 and NaN outputs.  Returns the noise rows left
    out as fragile; `stats` collects the worst figures (root, value, location) of these rows alone."""
    a, b = dom
    x, w, _ = grid(n, a, b)
    stats = {} if stats is None else stats
    skipped = 0
    if mode == "roots":
        R, cnt = got
        assert R.shape == (V.shape[0], max(n - 1, 1)) and cnt.shape == (V.shape[0],)
        for i, kind in enumerate(kinds):
            want = ref_roots(V[i], dom)
            if want is None:
                assert cnt[i] == -1 and np.all(np.isnan(R[i])), (tag, i, kind, cnt[i], R[i])
                continue
            if kind in ("const", "zero"):
                assert cnt[i] == 0 and want.size == 0, (tag, i, kind, cnt[i], R[i], want)
            if kind == "noise" and fragile(V[i]):
                skipped += 1
                continue
            assert cnt[i] == want.size, (tag, i, kind, int(cnt[i]), want.size, R[i], want)
            _check_roots(R[i, :cnt[i]], want, a, b, (tag, i, kind), stats)
            assert np.all(np.isnan(R[i, cnt[i]:])), (tag, i, kind, R[i])
        return skipped
    val, loc, cnt = got
    assert val.shape == loc.shape == cnt.shape == (V.shape[0],)
    for i, kind in enumerate(kinds):
        want = ref_opt(V[i], n, dom, mode)
        if want is None:
            assert cnt[i] == -1 and np.isnan(val[i]) and np.isnan(loc[i]), (tag, i, kind, cnt[i], val[i], loc[i])
            continue
        if not np.isfinite(want[0]):     # n <= 2: no matrix; NaN wins the extremum at the first candidate, an inf stays
            assert cnt[i] >= 0 and loc[i] == want[1], (tag, i, kind, cnt[i], loc[i], want)
            assert np.array_equal(val[i], want[0], equal_nan=True), (tag, i, kind, val[i], want)
            continue
        assert cnt[i] >= 0, (tag, i, kind, cnt[i])
        scale = max(float(np.max(np.abs(V[i]))), 1e-300)
        _check_opt((val[i], loc[i]), want, scale, a, b, _bary(V[i], x, w), (tag, i, kind), stats)
    return skipped


def missed_endpoints(dom, solve, ns):
    """The n of `ns` at which the lobatto row's roots -- `solve(n)` -> (roots (n - 1,), count) -- are not a full row
    that starts at exactly lo and ends at exactly hi: [(n, count, first - lo, last - hi)]."""
    missed = []
    for n in ns:
        r, cnt = solve(n)
        if not (cnt == n - 1 and r[0] == dom[0] and r[n - 2] == dom[1]):
            missed.append((n, int(cnt), float(r[0] - dom[0]), float(r[n - 2] - dom[1])))
    print(f"{dom}: lobatto rows whose first / last root is not exactly lo / hi: {len(missed)} of {len(ns)}")
    return missed


# ---------------------------------------------------------------------------------------------- metamorphic relations
MIXED_KINDS = ("zero", "const", "line", "T", "noise", "nan", "inf", "noise")


def metamorphic_inputs(n):
    """name -> rows.  "stack": a base of six noise rows, T, lobatto and the specials, then the base times 2^200, times
    2^-200 and negated, four blocks in one call; "mixed": mixed_batch(n); "mixed<r>": its row r alone, for
    each of its eight rows."""
    V, _ = families(n)
    base = np.concatenate([V[:6], V[NOISE_ROWS:]])
    inp = {"stack": np.concatenate([base, base * 2.0 ** 200, base * 2.0 ** -200, -base]), "mixed": mixed_batch(n)[0]}
    for r in range(inp["mixed"].shape[0]):
        inp[f"mixed{r}"] = inp["mixed"][r:r + 1]
    return inp


def check_metamorphic(n, dom, out, tag):
    """out[name][mode] = one call's outputs on metamorphic_inputs(n)[name].  Every relation holds bit for bit, because
    a power of two and a sign pass through the DCT, the ratios c_q / c_m and the barycentric quotient unchanged, and a
    row's result depends on its own fibre only:
      scaling    the same roots and counts; extrema scaled exactly, at the same locations
      negation   the same roots; minimize(-v) = (-maximize(v).value, the same location) and the converse
      batch      a row alone = the same row inside the mixed batch, NaN and inf rows among its neighbours
    and the mixed batch itself follows the restatement: a NaN or inf row has count -1 and NaN outputs from n = 3 on
    (below there is no matrix: count 0, and a NaN wins the extremum)."""
    def same(x, y):
        return np.array_equal(x, y, equal_nan=True)
    blocks = {mode: [np.split(o, 4) for o in out["stack"][mode]] for mode in MODES}      # [output][block]
    base, up, down, neg = ({mode: [o[k] for o in blocks[mode]] for mode in MODES} for k in range(4))
    for name, got, f in (("up", up, 2.0 ** 200), ("down", down, 2.0 ** -200)):
        assert same(got["roots"][0], base["roots"][0]) and same(got["roots"][1], base["roots"][1]), (tag, name)
        for mode in ("min", "max"):
            val, loc, cnt = got[mode]
            assert same(val, base[mode][0] * f) and same(loc, base[mode][1]) and same(cnt, base[mode][2]), (tag, name, mode)
    assert same(neg["roots"][0], base["roots"][0]) and same(neg["roots"][1], base["roots"][1]), (tag, "neg")
    for mode, other in (("min", "max"), ("max", "min")):
        val, loc, cnt = neg[mode]
        assert same(val, -base[other][0]) and same(loc, base[other][1]) and same(cnt, base[other][2]), (tag, "neg", mode)
    mixed = out["mixed"]
    alone_rows = sorted(int(name[5:]) for name in out if name.startswith("mixed") and name != "mixed")
    assert alone_rows == list(range(len(MIXED_KINDS)))
    for mode in MODES:
        for r in alone_rows:
            for whole, alone in zip(mixed[mode], out[f"mixed{r}"][mode]):
                assert alone.shape[0] == 1 and same(whole[r], alone[0]), (tag, "mixed", mode, r, whole[r], alone[0])
        check_rows(n, metamorphic_inputs(n)["mixed"], MIXED_KINDS, dom, mode, mixed[mode], (tag, "mixed", mode))
        if n >= 3:
            for r in mixed_batch(n)[1]:
                assert mixed[mode][-1][r] == -1 and all(np.isnan(o[r]).all() for o in mixed[mode][:-1]), (tag, mode, r)


# ---------------------------------------------------------------------------------------------- extended precision
# np.longdouble where it carries more than 60 bits (x87: eps 1.1e-19), else `decimal` at 40 digits in object arrays.
HP_LONGDOUBLE = bool(np.finfo(np.longdouble).eps < 1e-18)
_PI50 = "3.14159265358979323846264338327950288419716939937510"


def hp_context():
    if HP_LONGDOUBLE:
        return contextlib.nullcontext()
    return decimal.localcontext(decimal.Context(prec=40))


def hp_array(x):
    x = np.atleast_1d(np.asarray(x, dtype=float))
    if HP_LONGDOUBLE:
        return x.astype(np.longdouble)
    return np.array([decimal.Decimal(float(v)) for v in x.ravel()], dtype=object).reshape(x.shape)


def _decimal_cos(x):
    s = term = decimal.Decimal(1)
    x2, k = x * x, 0
    while abs(term) > decimal.Decimal("1e-45"):
        k += 2
        term = -term * x2 / (k * (k - 1))
        s += term
    return s


def hp_cos_pi(num, den):
    """cos(pi num / den) for the integers `num` (array) and `den`."""
    num = np.asarray(num)
    if HP_LONGDOUBLE:
        pi = 4.0 * np.arctan(np.longdouble(1.0))
        return np.cos(pi * num.astype(np.longdouble) / np.longdouble(den))
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        pi = decimal.Decimal(_PI50)
        return np.array([+_decimal_cos(pi * int(k) / int(den)) for k in num], dtype=object)


def exact_roots(kind, n, dom=(-1.0, 1.0)):
    """The closed-form roots of the T / lobatto row of n nodes on `dom`, ascending, in extended precision."""
    with hp_context():
        if kind == "T":
            t = hp_cos_pi(2 * np.arange(n - 1, 0, -1) - 1, 2 * (n - 1))
        else:
            t = hp_cos_pi(np.arange(n - 2, -1, -1), n - 2)
        a, b = hp_array(dom[0])[0], hp_array(dom[1])[0]
        return (a + b) / 2 + (b - a) / 2 * t


def hp_max_abs_diff(got, exact):
    """max |got - exact| as a float, the difference formed in extended precision."""
    with hp_context():
        d = hp_array(got) - exact
        return float(max(abs(v) for v in d)) if d.size else 0.0


def hp_newton(coef, t):
    """The Newton corrections p(t) / p'(t) of the Chebyshev series `coef` at the points t (reference frame): series
    and derivative by Clenshaw in extended precision.  Independent of any eigenvalue solver."""
    t = np.atleast_1d(np.asarray(t, dtype=float))
    if not t.size:
        return np.zeros(0)
    with hp_context():
        c, x = hp_array(coef), hp_array(t)
        n = c.size
        zero = c[0] * 0
        d = [zero] * (n + 1)            # p' = sum d_k T_k: d_(k-1) = d_(k+1) + 2 k c_k, d_0 halved
        for k in range(n - 1, 0, -1):
            d[k - 1] = d[k + 1] + 2 * k * c[k]
        d[0] = d[0] / 2

        def clenshaw(s, m):
            b1 = b2 = x * 0
            for k in range(m - 1, 0, -1):
                b1, b2 = 2 * x * b1 - b2 + s[k], b1
            return x * b1 - b2 + s[0]
        delta = clenshaw(c, n) / clenshaw(d, n - 1) if n > 1 else x * 0
        return np.array([float(v) for v in delta])
