"""The lane-per-point barycentric kernels -- k_bary_small, k_bary_sq, k_bary_small_pieces, k_bary_sq_pieces
(csrc/bary_kernels.h) -- on a CPU: a long-double reference with the row's amplitude, a float64 restatement of the
kernels' own arithmetic, and the seeded model lists whose shapes reach every template body the four switches of
csrc/pcx_bary.hip can launch.  Not a test module: tests/test_bary_ld_host.py inspects the lists and sets K from the
restatement; tests/test_gpu_bary_lane_bodies.py runs the lists on the device.  Plain NumPy and the package's host code
(nodes, weights, differentiation matrices); no GPU.

Reference, per dimension k and row, in np.longdouble:
    b_k,j = (w_j / (x_k - x_j)) / sum_i (w_i / (x_k - x_i))
with the reference's node rule applied literally: the first j with |x_k - x_j| < 1e-14, the difference taken in
float64, makes b_k one-hot.  Then y = sum_i T_i prod_k b_k,i_k and the row's amplitude
A_row = sum_i |T_i| prod_k |b_k,i_k|; a row is held to |got - y| <= K eps A_row.

Restatement (bary_weights_reg / bary_weights_prod, then bary_small_nest): t_j = x 2^e - (x_j 2^e) -- x 2^e and x_j 2^e
are exact, so the one rounding of the subtraction is the kernels' fma(x, 2^e, -snodes_j) bit for bit --, prefix products
times w_j, suffix products, one reciprocal of the sum, the node rule on |t_j| < 1e-14 2^e, and the contraction in the
kernels' nesting order, last dimension innermost, every sum one ascending chain.  It is what K is taken from, never the
code under test."""
from typing import NamedTuple, Optional, Tuple

import numpy as np

from pychebyshev_amd import ChebyshevApproximation, ChebyshevSpline

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
LD_OK = float(np.finfo(LD).eps) < 2e-19          # an 80-bit (or wider) long double; otherwise the tests skip
ROWS = 96                                        # one full 64-lane workgroup and a ragged one
NLP_LIST = (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 24, 32, 48, 64)     # k_bary_small<DOUT, NLP>
SQ_LIST = tuple(range(4, 25)) + (26, 28, 30, 32)                                    # k_bary_sq<NL, LEAD>
PADDED_N = (1,) + tuple(range(17, 24)) + tuple(range(25, 32)) + tuple(range(33, 48)) + tuple(range(49, 64))
PIECE_PADDED_N = (1, 19, 27, 41, 57)             # the five padded classes once more in the piece list
TAIL_ROWS = 130
TAIL_NS = (1, 63, 64, 65, 127, 128, 129)
BUCKETS = (0, 1, 63, 64, 65, 129)                # rows per piece of the bucket-edge splines


class Model(NamedTuple):
    name: str
    family: str                                  # "small" (variant 4) or "sq" (variant 5)
    shape: Tuple[int, ...]
    seed: int
    knots: Optional[Tuple[Tuple[float, ...], ...]] = None     # splines: per dimension, fractions of the domain
    rows: int = ROWS


def nlp_of(n_last):
    """The padded last-dimension width plan_lane_per_point gives n_last nodes."""
    return next(v for v in NLP_LIST if v >= n_last)


def variant_of(model):
    return 4 if model.family == "small" else 5


def small_body(model):
    """(DOUT, NLP, EXACT, n_last) of a variant-4 launch of the model."""
    n = model.shape[-1]
    return len(model.shape) - 1, nlp_of(n), n == nlp_of(n), n


def sq_body(model):
    """(NL, LEAD) of a variant-5 launch of the model."""
    return model.shape[-1], len(model.shape) - 2


# ---------------------------------------------------------------------------------------------------- the lists
def _outer(d, n, shift=0):
    return tuple(1 + (3 * k + n + shift) % 7 for k in range(d - 1))


def small_models():
    """d = 1 .. 4 x last-dimension node count 1 .. 64: every (DOUT, NLP), both EXACT branches, every padded n."""
    return tuple(Model(f"small-d{d}-n{n}", "small", _outer(d, n) + (n,), 1000 * d + n)
                 for d in range(1, 5) for n in range(1, 65))


def _sq_lead(nl, lead, seed):
    if lead == 2 and nl == 4:
        return (1, 3)                            # the one LEAD = 2 model with a leading count of 1
    return tuple(int(v) for v in np.random.default_rng(seed).integers(1, 6, size=lead))


def sq_models():
    """Every NL of launch_sq's list x LEAD 0, 1, 2; leading node counts from 1 .. 5."""
    return tuple(Model(f"sq-n{nl}-lead{lead}", "sq", _sq_lead(nl, lead, 7000 + 10 * nl + lead) + (nl, nl), 5000 + 10 * nl + lead)
                 for nl in SQ_LIST for lead in range(3))


def _piece_knots(i, d):
    """Two or three pieces along dimension 0; for d >= 2 every fourth model a knot in another dimension as well."""
    knots = [()] * d
    knots[0] = (0.4,) if i % 2 else (0.3, 0.65)
    if d >= 2 and i % 4 == 3:
        knots[1 + (i // 4) % (d - 1)] = (0.55,)
    return tuple(knots)


def piece_models():
    """Splines of equal-shape pieces: every (DOUT, NLP) of the small list at n = NLP, the five padded classes once more,
    and every (NL, LEAD) of the square list."""
    out = []
    for d in range(1, 5):
        for n in NLP_LIST + PIECE_PADDED_N:
            i = len(out)
            out.append(Model(f"pieces-small-d{d}-n{n}", "small", _outer(d, n, 2) + (n,), 20000 + 100 * d + n, _piece_knots(i, d)))
    for nl in SQ_LIST:
        for lead in range(3):
            i = len(out)
            out.append(Model(f"pieces-sq-n{nl}-lead{lead}", "sq", _sq_lead(nl, lead, 9000 + 10 * nl + lead) + (nl, nl),
                             30000 + 10 * nl + lead, _piece_knots(i, lead + 2)))
    return tuple(out)


def bucket_models():
    """One spline per form with six pieces along dimension 0 (test_bucket_edges)."""
    six = (0.15, 0.3, 0.5, 0.7, 0.85)
    return (Model("buckets-small", "small", (5, 7), 41, (six, ()), sum(BUCKETS)),
            Model("buckets-sq", "sq", (3, 6, 6), 42, (six, (), ()), sum(BUCKETS)))


def tail_models():
    """One model per (kernel, d) for the batch tails."""
    return (Model("tail-small-d1", "small", (13,), 51, None, TAIL_ROWS), Model("tail-small-d2", "small", (4, 21), 52, None, TAIL_ROWS),
            Model("tail-small-d3", "small", (3, 2, 9), 53, None, TAIL_ROWS), Model("tail-small-d4", "small", (2, 3, 2, 5), 54, None, TAIL_ROWS),
            Model("tail-sq-d2", "sq", (7, 7), 55, None, TAIL_ROWS), Model("tail-sq-d3", "sq", (3, 5, 5), 56, None, TAIL_ROWS),
            Model("tail-sq-d4", "sq", (2, 3, 4, 4), 57, None, TAIL_ROWS))


# ---------------------------------------------------------------------------------------------------- models and rows
def _domain(rng, d):
    """As tests/test_gpu_bary.py::test_lane_per_point_kernel_for_small_tensors draws it, the upper end capped at 8:
    |node| <= 8 keeps node +- 3e-15 a whole number of ulps between 2e-15 and 5e-15 away."""
    return [[float(a), float(min(a + w, 8.0))] for a, w in zip(rng.uniform(-5, 5, d), rng.uniform(0.5, 5, d))]


def _next_to(node, sign):
    """node +- 3e-15, rounded: k ulp with 2e-15 <= k ulp <= 5e-15 for |node| <= 8 -- well inside the 1e-14 rule and
    never within a factor of two of it, so reference and kernel agree about the side of the rule."""
    x = float(node) + sign * 3e-15
    assert abs(node) <= 8.0 and 2e-15 <= abs(x - node) <= 5e-15
    return x


def _special_rows(rng, nodes, dom, seed, head=None):
    """The fixed kinds of rows inside one box: (rows, position of the grid-point row, its multi-index).  head (the
    row-code MFMA models of tests/bary_mfma_ld.py): the "outer" dimension of rows 4 and 6 is drawn from the head
    dimensions [0, head) that have two nodes or more, where there is one; None draws it from all but the last."""
    d = len(nodes)
    shape = [len(x) for x in nodes]
    pool = [k for k in range(head or 0) if shape[k] >= 2]

    def outer():
        return pool[int(rng.integers(0, len(pool)))] if pool else int(rng.integers(0, d - 1))

    def uniform():
        return [rng.uniform(lo, hi) for lo, hi in dom]
    rows = [[lo for lo, _ in dom], [hi for _, hi in dom]]                       # both domain corners
    idx = tuple(int(rng.integers(0, v)) for v in shape)
    rows.append([nodes[k][idx[k]] for k in range(d)])                           # a full grid point
    r = uniform()
    r[d - 1] = nodes[d - 1][-1 if seed % 2 else 0]                              # on a node of the register dimension only:
    rows.append(r)                                                              # the prefix / suffix products end there
    if d >= 2:
        r, k = uniform(), outer()
        r[k] = nodes[k][int(rng.integers(0, shape[k]))]                         # on a node of an outer (LDS) dimension only
        rows.append(r)
    r = uniform()
    r[d - 1] = _next_to(nodes[d - 1][int(rng.integers(0, shape[d - 1]))], 1 if seed % 4 < 2 else -1)
    rows.append(r)                                                              # next to a node, last dimension
    if d >= 2:
        r, k = uniform(), outer()
        r[k] = _next_to(nodes[k][int(rng.integers(0, shape[k]))], -1 if seed % 4 < 2 else 1)
        rows.append(r)                                                          # next to a node, an outer dimension
    return rows, 2, idx


class Built(NamedTuple):
    model: Model
    c: ChebyshevApproximation
    pts: np.ndarray
    grid_row: int
    grid_idx: Tuple[int, ...]


def build(model, head=None):
    """The single model of a list entry on the host (no device call) and its rows (head: see _special_rows)."""
    assert model.knots is None
    rng = np.random.default_rng(model.seed)
    d = len(model.shape)
    T = rng.standard_normal(model.shape)
    dom = _domain(rng, d)
    c = ChebyshevApproximation.from_values(T, d, dom, list(model.shape))
    rows, at, idx = _special_rows(rng, c.nodes, dom, model.seed, head)
    pts = np.column_stack([rng.uniform(lo, hi, model.rows) for lo, hi in dom])
    pts[:len(rows)] = rows
    return Built(model, c, np.ascontiguousarray(pts), at, idx)


class BuiltSpline(NamedTuple):
    model: Model
    sp: ChebyshevSpline
    pts: np.ndarray
    ids: np.ndarray                              # the searchsorted rule's piece of every row
    grid_rows: Tuple[Tuple[int, int, Tuple[int, ...]], ...]     # (row, piece, multi-index): rows on a full grid point


def piece_ids(sp, pts):
    """The reference's routing: searchsorted(knots, x, side="right") per dimension, capped at the last interval."""
    multi = [np.minimum(np.searchsorted(np.asarray(kn, dtype=float), pts[:, k], side="right"), len(kn)) if len(kn)
             else np.zeros(len(pts), dtype=np.int64) for k, kn in enumerate(sp.knots)]
    return np.ravel_multi_index(multi, sp._shape).astype(np.int32)


def build_spline(model, counts=None):
    """The spline of a list entry and its rows: every kind of row inside every piece, one row exactly on the first knot
    of dimension 0 (it belongs to the right-hand piece), the rest uniform in the domain.  counts: instead, that many
    uniform rows inside each piece of dimension 0 (the bucket-edge splines), in shuffled order."""
    rng = np.random.default_rng(model.seed)
    d = len(model.shape)
    dom = _domain(rng, d)
    knots = [[lo + f * (hi - lo) for f in fr] for fr, (lo, hi) in zip(model.knots, dom)]
    n_pieces = int(np.prod([len(k) + 1 for k in knots]))
    values = [rng.standard_normal(model.shape) for _ in range(n_pieces)]
    sp = ChebyshevSpline.from_values(values, d, dom, list(model.shape), knots)
    grid_rows = []
    if counts is None:
        rows = []
        for p, piece in enumerate(sp._pieces):
            special, at, idx = _special_rows(rng, piece.nodes, piece.domain, model.seed + p)
            grid_rows.append((len(rows) + at, p, idx))
            rows += special
        r = [rng.uniform(lo, hi) for lo, hi in dom]
        r[0] = knots[0][0]
        rows.append(r)
        pts = np.column_stack([rng.uniform(lo, hi, model.rows) for lo, hi in dom])
        assert len(rows) < model.rows
        pts[:len(rows)] = rows
    else:
        assert len(counts) == n_pieces == len(knots[0]) + 1 and sum(counts) == model.rows
        parts = []
        for p, cnt in enumerate(counts):
            lo0, hi0 = sp._pieces[p].domain[0]
            x0 = lo0 + (hi0 - lo0) * rng.uniform(0.01, 0.99, cnt)              # strictly inside the piece
            parts.append(np.column_stack([x0] + [rng.uniform(lo, hi, cnt) for lo, hi in dom[1:]]))
        pts = np.concatenate(parts)[rng.permutation(model.rows)]
    pts = np.ascontiguousarray(pts)
    return BuiltSpline(model, sp, pts, piece_ids(sp, pts), tuple(grid_rows))


# ---------------------------------------------------------------------------------------------------- long-double reference
def _weights_ld(nodes, wts, x):
    """(rows, n) normalised weights in long double; the node rule decides in float64, as the reference does."""
    hit = np.abs(x[:, None] - nodes[None, :]) < 1e-14
    diff = x.astype(LD)[:, None] - nodes.astype(LD)[None, :]
    u = wts.astype(LD)[None, :] / np.where(diff == 0, LD(1), diff)             # diff == 0 only where the rule hits
    b = u / u.sum(axis=1, keepdims=True)
    on = hit.any(axis=1)
    b[on] = 0
    b[on, hit.argmax(axis=1)[on]] = 1
    return b


def reference(nodes, weights, T, pts):
    """(ref, amp) of the rows of one model, long double: ref = sum_i T_i prod_k b_k,i_k, amp the same over absolute values."""
    d, rows = len(nodes), len(pts)
    R = np.asarray(T).astype(LD)[None]
    A = np.abs(R)
    for k in range(d - 1, -1, -1):
        b = _weights_ld(np.asarray(nodes[k], dtype=float), np.asarray(weights[k], dtype=float), pts[:, k])
        b = b.reshape((rows,) + (1,) * k + (b.shape[1],))
        R, A = (R * b).sum(axis=-1), (A * np.abs(b)).sum(axis=-1)
    return R, A


def spline_reference(sp, tensors, pts, ids):
    """(ref, amp), every row on its own piece; tensors: one (derived) tensor per piece."""
    ref, amp = np.zeros(len(pts), dtype=LD), np.zeros(len(pts), dtype=LD)
    for p in np.unique(ids):
        rows = np.nonzero(ids == p)[0]
        piece = sp._pieces[int(p)]
        ref[rows], amp[rows] = reference(piece.nodes, piece.weights, tensors[int(p)], pts[rows])
    return ref, amp


# ---------------------------------------------------------------------------------------------------- float64 restatement
def node_scale(nodes):
    """pcx_bary_plan.hip's node_scale: the power of two 2^e ~ 2 / (node span); 0.5 for a single node."""
    span = float(nodes[-1] - nodes[0])
    e = int(np.frexp(2.0 / span)[1]) if span > 0.0 and np.isfinite(span) else 0
    return float(np.ldexp(1.0, e - 1))


def _weights_f64(nodes, wts, x):
    """bary_weights_reg / bary_weights_prod in float64, one row per point."""
    scale = node_scale(nodes)
    t = (x * scale)[:, None] - (nodes * scale)[None, :]                        # = fma(x, 2^e, -snodes_j): one rounding
    n = len(nodes)
    b = np.empty_like(t)
    run = np.ones(len(x))
    for j in range(n):                                                          # b_j <- w_j prefix_j
        b[:, j] = wts[j] * run
        run = run * t[:, j]
    run, su = np.ones(len(x)), np.zeros(len(x))
    for j in range(n - 1, -1, -1):                                              # b_j <- b_j suffix_j
        b[:, j] = b[:, j] * run
        su = su + b[:, j]
        run = run * t[:, j]
    with np.errstate(divide="ignore", invalid="ignore"):                       # on a node su is 0 or tiny: the rule rewrites the row
        b = b * (1.0 / su)[:, None]
    hit = np.abs(t) < 1e-14 * scale
    on = hit.any(axis=1)
    b[on] = 0.0
    b[on, hit.argmax(axis=1)[on]] = 1.0
    return b


def restatement(nodes, weights, T, pts):
    """The kernels' value of every row in float64: last dimension innermost, every sum one ascending chain."""
    d, rows = len(nodes), len(pts)
    R = np.asarray(T, dtype=float)[None]
    for k in range(d - 1, -1, -1):
        b = _weights_f64(np.asarray(nodes[k], dtype=float), np.asarray(weights[k], dtype=float), pts[:, k])
        s = np.zeros((rows,) + R.shape[1:-1])
        for j in range(b.shape[1]):
            s = s + R[..., j] * b[:, j].reshape((rows,) + (1,) * k)
        R = s
    return R


# ---------------------------------------------------------------------------------------------------- derivative specs
def specs_of(shape):
    """[value, d/dx_last, d/dx_0] without the derivatives of a dimension of fewer than 2 nodes; d = 1: they coincide."""
    d = len(shape)
    specs = [[0] * d]
    for k in (d - 1, 0):
        s = [int(u == k) for u in range(d)]
        if shape[k] >= 2 and s not in specs:
            specs.append(s)
    return specs


def piece_specs_of(shape):
    """[value, first derivative] of a spline call: along the last dimension, else the first one with 2 nodes or more;
    none: the value twice (still a two-tensor launch)."""
    d = len(shape)
    for k in (d - 1,) + tuple(range(d - 1)):
        if shape[k] >= 2:
            return [[0] * d, [int(u == k) for u in range(d)]]
    return [[0] * d, [0] * d]


def derived_tensor(c, spec):
    """The derivative passes of the CPU oracle (float64; the device tensor is bit-identical to it)."""
    import ctypes

    import oracle
    if not any(spec):
        return c.tensor_values
    om = oracle.BaryModel(c.nodes, c.weights, c.diff_matrices, c.tensor_values)
    lib = oracle._lib()
    lib.pcxo_apply_derivative_passes.restype = ctypes.POINTER(ctypes.c_double)
    s = np.ascontiguousarray(spec, dtype=np.int32)
    ptr = lib.pcxo_apply_derivative_passes(ctypes.c_int(om.d), om.n.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                           om.diff_cat.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                           om.tensor.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                           s.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    out = np.ctypeslib.as_array(ptr, shape=(c.tensor_values.size,)).reshape(c.tensor_values.shape).copy()
    ctypes.CDLL(None).free(ptr)
    return out


def order_of(spec):
    return ("value", "order1")[max(int(v) for v in spec)]


# ---------------------------------------------------------------------------------------------------- K
def ratios(got, ref, amp):
    """|got - ref| / (eps A_row), elementwise; 0 where the amplitude is 0 (then got must be exactly 0 as well)."""
    got, ref, amp = np.asarray(got), np.asarray(ref), np.asarray(amp)
    err = np.abs(got.astype(LD) - ref)
    assert not np.any((amp == 0) & (err != 0)), "a row of amplitude zero is not exactly zero"
    return np.where(amp > 0, err / (LD(EPS) * np.where(amp > 0, amp, 1)), 0).astype(np.float64)


def restatement_ratios(model):
    """{order: worst ratio} of the float64 restatement against the long-double reference on one list entry."""
    worst = {"value": 0.0, "order1": 0.0}

    def note(nodes, weights, T, pts, order):
        ref, amp = reference(nodes, weights, T, pts)
        worst[order] = max(worst[order], float(np.max(ratios(restatement(nodes, weights, T, pts), ref, amp))))
    if model.knots is None:
        b = build(model)
        for spec in specs_of(model.shape):
            note(b.c.nodes, b.c.weights, derived_tensor(b.c, spec), b.pts, order_of(spec))
    else:
        b = build_spline(model, BUCKETS if model.name.startswith("buckets") else None)
        for spec in piece_specs_of(model.shape):
            for p in np.unique(b.ids):
                piece = b.sp._pieces[int(p)]
                note(piece.nodes, piece.weights, derived_tensor(piece, spec), b.pts[b.ids == p], order_of(spec))
    return worst


def family_models(family):
    """Every list entry whose rows are held to K[family]."""
    return tuple(m for m in small_models() + sq_models() + piece_models() + bucket_models() + tail_models() if m.family == family)


# Worst |y - ref| / (eps A_row) of the float64 restatement over family_models(), per kernel family and spec order,
# measured by tests/test_bary_ld_host.py::test_the_restatement_sets_every_K (which asserts these figures), and the row
# bound's factor K: 16 times that, rounded up to a power of two.  The 16 covers what the kernels do differently from
# the restatement: FMA contraction, k_bary_sq's four row chains and two partial sums per block.  K <= 128 keeps the
# bound honest: a dropped node of a 64-node row is of the order of A_row / 64 = 2^46 eps A_row.
# The figures sit at 4 .. 5.5 rather than below 1 because a product-form weight is a product of n - 1 rounded factors:
# its relative error grows with n (d = 1: 1.1 at 2 nodes, 1.4 at 16, 2.9 at 32, 4.3 at 48; worst models: 54 and 56 nodes
# in the last dimension), and A_row does not count n.
RESTATEMENT_WORST = {
    "small": {"value": 4.769, "order1": 5.535},          # small-d3-n54, small-d3-n56
    "sq": {"value": 3.939, "order1": 4.452},             # pieces-sq-n19-lead0, pieces-sq-n18-lead1
}
K_CAP = 128


def K_of(worst):
    return 2 ** int(np.ceil(np.log2(16.0 * worst))) if worst > 0 else 1


K = {family: {order: K_of(w) for order, w in orders.items()} for family, orders in RESTATEMENT_WORST.items()}


def check(seen, got, pair, family, order, group, what, k=None):
    """One call against the long-double reference: the normwise bar, then every row against its own amplitude
    (tests/tt_rows.check for these models).  ``seen`` collects the worst row per (family, order, group).  k: the row
    bound's factor of a family whose K lives elsewhere (tests/bary_mfma_ld.py); None: K[family][order]."""
    ref, amp = pair
    got = np.asarray(got)
    assert got.shape == ref.shape and got.dtype == np.float64, what
    err = np.abs(got.astype(LD) - ref)
    scale = float(np.max(np.abs(ref)))
    r = ratios(got, ref, amp)
    worst = float(np.max(r))
    key = f"{family} {order} {group}"
    seen[key] = max(seen.get(key, 0.0), worst)
    k = K[family][order] if k is None else k
    print(f"{what}: E_norm {float(np.max(err)) / scale if scale else 0.0:.2e}, worst row {worst:.3f} eps A_row (K = {k})")
    assert float(np.max(err)) <= 1e-12 * scale, f"{what}: E_norm {float(np.max(err)) / scale:.3e}"
    at = int(np.argmax(r))
    assert worst <= k, f"{what}: row {at}: |got - ref| = {worst:.3g} eps A_row > K = {k} (got {got[at]!r}, ref {float(ref[at])!r})"
