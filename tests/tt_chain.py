"""Shared by the tensor-train body tests: the TT chain  v <- v . (sum_j q_j G_k[:, j, :])  in ``np.longdouble`` with
the four bases the device kernels use, the amplitude of every row, the same chain restated in float64, and the seeded
model lists: the sweep of the lane-per-row kernels (tests/test_gpu_tt_lane_bodies.py runs it) and mfma_models(), the
list of the three MFMA forms of eval_batch (tests/test_gpu_tt_mfma_bodies.py; 220 models that reach 83 + 48 + 108
bodies of the 16x16x4, W-first and 4x4x4 forms; worst rows on MI355X 1.72 eps A_row against the restatement's 1.21,
K = 32, and 0.61 against 0.63, K = 16, for d <= 2).  tests/test_tt_chain_host.py inspects both lists.  Plain NumPy, no
GPU, nothing from the reference checkout.

Frames: ``cores`` and ``domain`` are indexed by STORAGE position k; ``dim_order[k]`` is the user dimension stored there;
rows (``pts``), specs, ``dims``, ``bounds`` and ``xs`` are in the USER's frame, as the public calls take them.

Bases of storage position k on [lo, hi], with  s = (x - lo) (2 / (hi - lo)) - 1  and  sc = 2 / (hi - lo):

  value        q_j = T_j(s):  T_0 = 1, T_1 = s, T_{j+1} = 2 s T_j - T_{j-1}
  derivative   q_j = sc^p T_j^(p)(s), p = 0, 1, 2, by the three recurrences of generate_golden_tt_derivatives.py run
               together:  T'_{j+1} = 2 T_j + 2 s T'_j - T'_{j-1},  T''_{j+1} = 4 T'_j + 2 s T''_j - T''_{j-1}
  box          q_j = (hi - lo) / 2 (F_j(t_hi) - F_j(t_lo)),  F_0 = t, F_1 = t^2 / 2,
               F_j = (T_{j+1} / (j + 1) - T_{j-1} / (j - 1)) / 2
  ladder       the value chain at every (fixed..., x) of a ladder row.  The product is associated around the ladder's
               core -- left chain, right chain, the n coefficients of the row's restriction, then the series at each x --
               which is the same number in exact arithmetic and costs one chain per row instead of m
               (test_tt_chain_host.py holds it to the plain value chain at the expanded points)

Every result comes with the row's AMPLITUDE A_row: the same chain with |G| in place of G and |q_j| in place of q_j; for
an integrated dimension  (hi - lo) / 2 (|F_j(t_hi)| + |F_j(t_lo)|)  -- the difference cancels for a narrow box, the
rounding error of its two terms does not.  eps A_row is the size of one rounding error of the row's sum, so
|got - ref| / (eps A_row) is a row's error in units that do not depend on how much the row cancels.

A contraction is a fixed sequence of elementwise multiplications and additions (j ascending, then the left rank
ascending; no matrix product, no FMA), so the float64 restatement gives the same bits on every machine and the ratios
measured from it (RESTATEMENT_WORST below) can be asserted."""
import collections
import functools

import numpy as np

import tt_plan_rule as plan_rule

LD = np.longdouble
# a platform whose long double is float64 would compare double with double: refuse to import
assert np.finfo(LD).eps <= 2.0 ** -63, f"np.longdouble carries no extended precision here (eps {np.finfo(LD).eps})"
EPS = float(np.finfo(np.float64).eps)


# ---------------------------------------------------------------------------------------------- bases
def _recurrences(s, n):
    """T, T', T'' of shape (n + 1, N) in s's dtype (index n is T_n, which the antiderivatives need)."""
    T = np.zeros((n + 1, s.size), dtype=s.dtype)
    U = np.zeros_like(T)
    W = np.zeros_like(T)
    T[0] = 1
    T[1] = s
    U[1] = 1
    for j in range(1, n):
        T[j + 1] = 2 * s * T[j] - T[j - 1]
        U[j + 1] = 2 * T[j] + 2 * s * U[j] - U[j - 1]
        W[j + 1] = 4 * U[j] + 2 * s * W[j] - W[j - 1]
    return T, U, W


def deriv_basis(s, n, p, sc):
    """(N, n): sc^p T_j^(p)(s), j < n."""
    return (_recurrences(s, n)[p][:n] * sc ** p).T


def _antiderivatives(t, n):
    """(n, N): F_j(t), j < n."""
    T = _recurrences(t, n)[0]
    F = np.empty((n, t.size), dtype=t.dtype)
    F[0] = t
    if n > 1:
        F[1] = t * t / 2
    for j in range(2, n):
        F[j] = (T[j + 1] / (j + 1) - T[j - 1] / (j - 1)) / 2
    return F


def box_basis(ta, tb, n, half):
    """(q, |q|-bound), (N, n) each: half (F_j(tb) - F_j(ta)) and half (|F_j(tb)| + |F_j(ta)|)."""
    Fa, Fb = _antiderivatives(ta, n), _antiderivatives(tb, n)
    return (half * (Fb - Fa)).T, (half * (np.abs(Fb) + np.abs(Fa))).T


# ---------------------------------------------------------------------------------------------- the chain
def _fold(core, q):
    """(N, rl, rr): sum_j q[:, j] core[:, j, :], j ascending."""
    M = q[:, 0, None, None] * core[None, :, 0, :]
    for j in range(1, core.shape[1]):
        M = M + q[:, j, None, None] * core[None, :, j, :]
    return M


def _step(v, M):
    """(N, rr): sum_a v[:, a] M[:, a, :], a ascending."""
    out = v[:, 0, None] * M[:, 0, :]
    for a in range(1, M.shape[1]):
        out = out + v[:, a, None] * M[:, a, :]
    return out


class Chain:
    """One model on one batch of rows, in ``dtype`` (np.longdouble: the reference; np.float64: the restatement).
    Every method returns (values, amplitudes) in ``dtype``; the folded cores of a dimension are formed once per basis."""

    def __init__(self, cores, domain, dim_order, pts, dtype=LD):
        self.dt = np.dtype(dtype).type
        self.d = len(cores)
        self.order = list(range(self.d)) if dim_order is None else [int(v) for v in dim_order]
        self.G = [np.asarray(c).astype(self.dt) for c in cores]
        self.absG = [np.abs(g) for g in self.G]
        self.n = [g.shape[1] for g in self.G]
        self.lo = [self.dt(a) for a, _ in domain]
        self.hi = [self.dt(b) for _, b in domain]
        self.sc = [self.dt(2) / (b - a) for a, b in zip(self.lo, self.hi)]
        self.pts = np.asarray(pts, dtype=np.float64)
        self._folds = {}

    def s(self, k, x):
        return (np.asarray(x).astype(self.dt) - self.lo[k]) * self.sc[k] - self.dt(1)

    def _pair(self, k, q, qabs):
        return _fold(self.G[k], q), _fold(self.absG[k], qabs)

    def fold(self, k, p):
        """(M, |M|-bound) of storage position k at the rows' own coordinate, derivative order p."""
        if (k, p) not in self._folds:
            q = deriv_basis(self.s(k, self.pts[:, self.order[k]]), self.n[k], p, self.sc[k])
            self._folds[k, p] = self._pair(k, q, np.abs(q))
        return self._folds[k, p]

    def _run(self, folds):
        v = a = np.ones((self.pts.shape[0], 1), dtype=self.dt)
        for M, Mabs in folds:
            v, a = _step(v, M), _step(a, Mabs)
        return v[:, 0], a[:, 0]

    def value(self):
        return self._run([self.fold(k, 0) for k in range(self.d)])

    def value_s(self):
        """The value with the amplitude  A_row + sum_k A_k:  A_k is the chain on |G| with |T_j'(s_k)| in place of
        |T_j(s_k)| at storage position k -- the first-order size of the row's change under an absolute error of one eps
        in s_k (see RESTATEMENT_WORST on why A_row alone cannot see it)."""
        val, amp = self.value()
        one = np.ones((self.pts.shape[0], 1), dtype=self.dt)
        for k in range(self.d):
            q1 = np.abs(deriv_basis(self.s(k, self.pts[:, self.order[k]]), self.n[k], 1, self.dt(1)))
            a = one
            for i in range(self.d):
                a = _step(a, _fold(self.absG[k], q1) if i == k else self.fold(i, 0)[1])
            amp = amp + a[:, 0]
        return val, amp

    def deriv(self, spec):
        """spec: an order 0, 1 or 2 per USER dimension."""
        return self._run([self.fold(k, int(spec[self.order[k]])) for k in range(self.d)])

    def box(self, dims, bounds):
        """dims: the integrated user dimensions, ascending; bounds (N, len(dims), 2); the kept coordinates are the rows'."""
        dims = [int(u) for u in dims]
        folds = []
        for k in range(self.d):
            u = self.order[k]
            if u not in dims:
                folds.append(self.fold(k, 0))
                continue
            b = np.asarray(bounds)[:, dims.index(u), :]
            half = (self.hi[k] - self.lo[k]) / 2
            folds.append(self._pair(k, *box_basis(self.s(k, b[:, 0]), self.s(k, b[:, 1]), self.n[k], half)))
        return self._run(folds)

    def ladder(self, dim, xs):
        """Along user dimension ``dim`` at xs (m,) shared or (N, m) per row; the other coordinates are the rows' (the
        rows' own column ``dim`` is not read).  (N, m) values and amplitudes."""
        N = self.pts.shape[0]
        p = self.order.index(int(dim))
        one = np.ones((N, 1), dtype=self.dt)
        L, La = one, one
        for k in range(p):
            M, Mabs = self.fold(k, 0)
            L, La = _step(L, M), _step(La, Mabs)
        R, Ra = one, one
        for k in range(self.d - 1, p, -1):
            M, Mabs = self.fold(k, 0)
            R, Ra = _step(R, M.transpose(0, 2, 1)), _step(Ra, Mabs.transpose(0, 2, 1))
        xs = np.broadcast_to(np.asarray(xs, dtype=np.float64), (N, np.shape(xs)[-1]))
        T = np.stack([deriv_basis(self.s(p, xs[:, i]), self.n[p], 0, self.sc[p]) for i in range(xs.shape[1])], axis=1)
        out = []
        for G, l, r, t in ((self.G[p], L, R, T), (self.absG[p], La, Ra, np.abs(T))):
            c = np.stack([_step(_step(l, G[None, :, j, :]), r[:, :, None])[:, 0] for j in range(self.n[p])], axis=1)
            out.append(_step(c, t.transpose(0, 2, 1)))
        return out[0], out[1]


def expand(d, dim, fixed, xs):
    """(N * m, d) points of a ladder batch, row by row: the plain points ``ladder_batch`` stands for."""
    N, m = fixed.shape[0], np.shape(xs)[-1]
    pts = np.empty((N, m, d))
    for c, u in enumerate([u for u in range(d) if u != dim]):
        pts[:, :, u] = fixed[:, c][:, None]
    pts[:, :, dim] = np.broadcast_to(xs, (N, m))
    return pts.reshape(N * m, d)


def with_column(fixed, dim, value=0.0):
    """(N, d) rows from a ladder's ``fixed`` (N, d - 1): column ``dim`` put in (Chain.ladder does not read it)."""
    return np.insert(np.asarray(fixed, dtype=np.float64), dim, value, axis=1)


# ---------------------------------------------------------------------------------------------- the sweep's models
DECAY = 0.55                  # the g22 goldens' recipe: normal * DECAY^j / sqrt(r_left) keeps derivative rows comparable
CAPS = (8, 12, 16)            # the rank-cap instantiations of the lane kernels
MAX_N = 16
ROWS = 96                     # one full 64-row workgroup and a ragged one
LADDER_M = 5
TAIL_ROWS = 129
TAIL_NS = (1, 63, 64, 65, 127, 128, 129)

Model = collections.namedtuple("Model", "number name cap mode ranks n rows")


def rank_chains():
    """(cap, ranks): 2 .. cap in groups of four, each between rank-1 ends and followed by the cap itself (which makes
    the model run on that cap's instantiation) where the group does not hold it.  9 chains, d <= 6."""
    out = []
    for cap in CAPS:
        inner = list(range(2, cap + 1))
        for i in range(0, len(inner), 4):
            group = inner[i:i + 4]
            out.append((cap, [1] + group + ([] if cap in group else [cap]) + [1]))
    return out


@functools.lru_cache(maxsize=None)
def sweep_models():
    """Every rank chain with every node count 1 .. 16 in every dimension (uniform: the kernels' one-level switch) and
    with n_k = 1 + (4 k + t) % 16, t = 0 .. 15 (mixed: the two-level switch; d >= 4, so the counts do differ)."""
    out = []
    for c, (cap, ranks) in enumerate(rank_chains()):
        d = len(ranks) - 1
        for n in range(1, MAX_N + 1):
            out.append(Model(len(out), f"cap{cap}-chain{c}-uniform-n{n}", cap, "uniform", tuple(ranks), (n,) * d, ROWS))
        for t in range(MAX_N):
            out.append(Model(len(out), f"cap{cap}-chain{c}-mixed-t{t}", cap, "mixed", tuple(ranks),
                             tuple(1 + (4 * k + t) % MAX_N for k in range(d)), ROWS))
    return tuple(out)


def edge_models():
    """The wave-per-row forms: lane loops of exactly one and of two trips; rank > 16 alone, three trips; generic only
    because n > 16, every rank 1.  130 rows: 32 blocks of four waves and a ragged one."""
    first = len(sweep_models())
    shapes = [("edge-r64-r65", (1, 64, 65, 1), (3, 4, 17)), ("edge-r130", (1, 130, 1), (2, 9)), ("edge-n17-rank1", (1, 1, 1), (17, 1))]
    return tuple(Model(first + i, name, 0, "generic", ranks, n, 130) for i, (name, ranks, n) in enumerate(shapes))


def tail_model():
    """One mixed-mode cap-12 model with TAIL_ROWS rows, for the batch tails."""
    src = next(m for m in sweep_models() if m.cap == 12 and m.mode == "mixed" and m.name.endswith("t5"))
    return src._replace(number=len(sweep_models()) + len(edge_models()), name="tail-" + src.name, rows=TAIL_ROWS)


def rank_cap(model):
    """The instantiation the launchers pick: from the model's largest rank (0: no lane-per-row image)."""
    r = max(model.ranks)
    if r > 16 or max(model.n) > MAX_N:
        return 0
    return 8 if r <= 8 else (12 if r <= 12 else 16)


def is_uniform(model):
    return len(set(model.n)) == 1


def lane_bodies(models):
    """{(cap, uniform?, left rank, node count)} over the dimensions of the lane-per-row models of ``models``."""
    return {(rank_cap(m), is_uniform(m), m.ranks[k], m.n[k]) for m in models if rank_cap(m) for k in range(len(m.n))}


def all_lane_bodies():
    """The 1,152 reachable bodies: left ranks 1 .. cap under each cap that holds them, n = 1 .. 16, both modes."""
    return {(cap, uni, rl, n) for cap in CAPS for uni in (True, False) for rl in range(1, cap + 1) for n in range(1, MAX_N + 1)}


# ---------------------------------------------------------------------------------------------- the MFMA forms' models
# The list of tests/test_gpu_tt_mfma_bodies.py: the 16x16x4 direct form (variant 1), the W-first form (2) and the 4x4x4
# form (3) of ChebyshevTT.eval_batch.  Which body a model runs is read off tests/tt_plan_rule.py's restatement of the
# planner, so tests/test_tt_chain_host.py proves the coverage below without a GPU.
SMALL_CHAINS = ((1, 2, 4, 3, 1), (1, 5, 8, 7, 1), (1, 9, 12, 11, 1))        # largest rank in (0, 4], (4, 8], (8, 12]; d = 4
LARGE_CHAINS = ((1, 14, 16, 15, 1), (1, 17, 1, 32, 21, 1), (1, 33, 64, 50, 1))   # 13 .. 16; 17 .. 32, a rank-1 bond inside; 33 .. 64
DIRECT_NS = (1, 2, 3, 4, 5, 8)     # the ping-pong loop: no pair, one pair, pair + peel, two pairs, two + peel, four pairs
DIRECT_RCS = (1, 2, 3, 4, 8, 16)   # k_tt_eval_mfma<RC, RT, NT>: <1|2|3|4, 1, 4>, <8, 2, 2>, <16, 4, 1>
W_MAX_N = 32
D4_MAX_N = 16
LOWD = (((1, 1), (1,)), ((1, 1), (7,)), ((1, 1), (32,)),
        ((1, 4, 1), (5, 3)), ((1, 12, 1), (7, 10)), ((1, 16, 1), (6, 5)), ((1, 64, 1), (4, 9)))
MFMA_TAIL_ROWS = 300
MFMA_TAIL_NS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257)
CU_LDS_BYTES = 160 * 1024


@functools.lru_cache(maxsize=None)
def _plan(ranks, n):
    d = len(n)
    made = plan_rule.plan(d, list(n), list(ranks), [0.0] * d, [1.0] * d, None)
    assert made["rc"] == 0, made
    return made["plan"]


def plan_of(model):
    """The planner's decisions about a model (tests/tt_plan_rule.py); none of those read here depends on the domain."""
    return _plan(tuple(model.ranks), tuple(model.n))


def offered(model):
    """The forced variants among (1, 2, 3) the model's plan offers (every image uploaded)."""
    p = plan_of(model)
    return tuple(v for v in (1, 2, 3) if plan_rule.auto_variant(p, v) == v)


def first_global_last(ranks, head):
    """The smallest last node count whose padded last core the direct form no longer copies to LDS
    (last_lds_doubles == 0), behind the node counts ``head``."""
    return next(n for n in range(1, 4097) if not _plan(tuple(ranks), tuple(head) + (n,))["last_lds_doubles"])


def mixed_counts(m):
    """d = 4 node counts whose largest, m >= 2, stands alone at position m % 4.  The others: 4 KS - 4 (KS = ceil(m / 4);
    from KS = 2 on, the W-first image of that dimension ends in a whole k-step of zero rows), m - 1 and m // 2, rotated."""
    ks = -(-m // 4)
    others = [max(1, 4 * (ks - 1)), m - 1, max(1, m // 2)]
    turn = (m // 4) % 3
    others = others[turn:] + others[:turn]
    return tuple(others[:m % 4] + [m] + others[m % 4:])


@functools.lru_cache(maxsize=None)
def mfma_models():
    """220 models of ROWS rows, numbered behind tail_model():
      small chains   SMALL_CHAINS x (every uniform node count 1 .. 32, and mixed_counts(m), m = 2 .. 32: m = 1 leaves no
                     smaller count for the other dimensions, the uniform n = 1 model is that case)
      large chains   LARGE_CHAINS x uniform n in DIRECT_NS
      global last    every chain with small leading node counts and the first last node count that the direct form reads
                     from global memory instead of its LDS copy
      low dimension  LOWD: d = 1 with n = 1, 7, 32; d = 2 with largest rank 4, 12, 16, 64"""
    first = tail_model().number + 1
    out = []

    def add(name, mode, ranks, n):
        out.append(Model(first + len(out), name, 0, mode, tuple(ranks), tuple(n), ROWS))
    for c, ranks in enumerate(SMALL_CHAINS):
        for n in range(1, W_MAX_N + 1):
            add(f"small{c}-uniform-n{n}", "mfma-uniform", ranks, (n,) * 4)
        for m in range(2, W_MAX_N + 1):
            add(f"small{c}-mixed-max{m}", "mfma-mixed", ranks, mixed_counts(m))
    for c, ranks in enumerate(LARGE_CHAINS):
        for n in DIRECT_NS:
            add(f"large{c}-uniform-n{n}", "mfma-uniform", ranks, (n,) * (len(ranks) - 1))
    for c, ranks in enumerate(SMALL_CHAINS + LARGE_CHAINS):
        head = tuple(2 + k % 2 for k in range(len(ranks) - 2))
        add(f"{'small' if c < 3 else 'large'}{c % 3}-global-last", "mfma-global", ranks, head + (first_global_last(ranks, head),))
    for ranks, n in LOWD:
        add(f"lowd-d{len(n)}-r{max(ranks)}-n{'x'.join(map(str, n))}", "mfma-lowd", ranks, n)
    return tuple(out)


def _mfma(name):
    return next(m for m in mfma_models() if m.name == name)


@functools.lru_cache(maxsize=None)
def mfma_tail_models():
    """((model of MFMA_TAIL_ROWS rows, forced variant), ...): one per kernel family -- direct NT = 4, 2, 1, W-first
    NT = 4 (R = 4) and NT = 1 (R = 12), 4x4x4.  Numbered behind mfma_models()."""
    picks = (("large0-uniform-n5", 1), ("large1-uniform-n5", 1), ("large2-uniform-n3", 1),
             ("small0-mixed-max19", 2), ("small2-mixed-max22", 2), ("small1-mixed-max13", 3))
    first = mfma_models()[-1].number + 1
    return tuple((_mfma(name)._replace(number=first + i, name="tail-" + name, rows=MFMA_TAIL_ROWS), variant)
                 for i, (name, variant) in enumerate(picks))


@functools.lru_cache(maxsize=None)
def persistent_models():
    """((model, forced variant, points per batch of a workgroup), ...) for the persistent batch loops of k_tt_eval_wfirst
    and k_tt_eval_d4.  Launch LDS above half (a third) of a CU's 160 KiB: at most one (two) workgroups resident per CU,
    so 3 x 4 x resident x CUs batches stay a host array of under 80 MB.  The R = 4 model is the list's only 12-D one: the
    smallest d at which the NT = 4 launch (image + 6 x 64 d query-row doubles) passes 80 KiB."""
    wide = Model(mfma_tail_models()[-1][0].number + 1, "persistent-r4-d12", 0, "mfma-mixed",
                 (1, 2, 4, 3, 4, 1, 3, 4, 2, 4, 3, 2, 1), tuple(32 - k % 4 for k in range(12)), ROWS)
    return ((wide, 2, 256), (_mfma("small2-uniform-n32"), 2, 64), (_mfma("small2-uniform-n16"), 3, 64))


def mfma_extra_models():
    """The models of the tail and persistent-loop tests that are not in mfma_models() themselves."""
    return tuple(m for m, _ in mfma_tail_models()) + (persistent_models()[0][0],)


def launch_lds(model, variant):
    """Dynamic LDS bytes of the model's launch on a forced variant (tests/tt_plan_rule.py)."""
    p = plan_of(model)
    lds = plan_rule.lds(p)
    if variant == 3:
        return lds["d4"]
    if variant == 2:
        return lds["wfirst"][1 if p["wR"] == 4 else 0]                # R = 4 runs NT = 4, R = 8 and 12 NT = 1
    return lds["direct"][(2, 1, 0)[p["cls"]]]                         # NT = 4, 2, 1 by rank class


def n_class(n):
    """How the direct form's two-node loop ends: (pairs, capped at 2; a peeled odd node)."""
    return min(n // 2, 2), n % 2


N_CLASSES = ((0, 1), (1, 0), (1, 1), (2, 0), (2, 1))


def direct_bodies(models):
    """Of k_tt_eval_mfma<RC, RT, NT>, RC naming the instantiation:
      ("shape", RC, "d1" | "d2" | "d3+")                             the d == 1 branch, no middle dimension, the loop over k
      ("nodes", RC, "dim0" | "mid", "ping-pong" | "plain", n class)  tt_mfma_nodes<1 | RC, RT, NT>: F = RCX RT <= 8 or not
      ("last", RC, "lds" | "global")                                 where the last core is read from"""
    out = set()
    for m in models:
        p = plan_of(m)
        if p["generic"]:
            continue
        d, RC, RT = p["d"], p["last_rows"] // 4, p["rk.rt"][0]
        out.add(("shape", RC, "d1" if d == 1 else "d2" if d == 2 else "d3+"))
        for k in range(d - 1):
            out.add(("nodes", RC, "mid" if k else "dim0", "ping-pong" if p["rk.rc"][k] * RT <= 8 else "plain", n_class(m.n[k])))
        out.add(("last", RC, "lds" if p["last_lds_doubles"] else "global"))
    return out


def all_direct_bodies():
    """83: the d = 1 model has rank 1 and the d = 2 models largest rank 4, 12, 16, 64; 6 x 2 x 5 node loops; 6 x 2 last cores."""
    out = {("shape", 1, "d1")} | {("shape", rc, "d2") for rc in (1, 3, 4, 16)} | {("shape", rc, "d3+") for rc in DIRECT_RCS}
    for rc in DIRECT_RCS:
        rt = max(1, rc // 4)
        for cls in N_CLASSES:
            out.add(("nodes", rc, "dim0", "ping-pong", cls))
            out.add(("nodes", rc, "mid", "ping-pong" if rc * rt <= 8 else "plain", cls))
        out |= {("last", rc, "lds"), ("last", rc, "global")}
    return out


def wfirst_bodies(models):
    """{(R, KS, "spread" | "none")}: the k_tt_eval_wfirst<R, KS, NT> instantiation and its middle dimensions, k < d - 2
    (v' is spread to every lane) and k = d - 2 (it is not)."""
    out = set()
    for m in models:
        p = plan_of(m)
        if p["wR"]:
            out |= {(p["wR"], p["wplan.ks"], "spread" if k < p["d"] - 2 else "none") for k in range(1, p["d"] - 1)}
    return out


def all_wfirst_bodies():
    return {(R, ks, pos) for R in (4, 8, 12) for ks in range(1, 9) for pos in ("spread", "none")}


def d4_bodies(models):
    """{("ks0", RA, k-steps of dimension 0), ("mid", RA, NJ), ("last", RA, NJ)} of k_tt_eval_d4<RA>."""
    out = set()
    for m in models:
        p = plan_of(m)
        RA, d = p["d4RA"], p["d"]
        if RA:
            if d > 1:
                out.add(("ks0", RA, -(-m.n[0] // 4)))
            out |= {("mid", RA, m.n[k]) for k in range(1, d - 1)} | {("last", RA, m.n[-1])}
    return out


def all_d4_bodies():
    return ({("ks0", RA, s) for RA in (1, 2, 3) for s in range(1, 5)}
            | {(part, RA, n) for part in ("mid", "last") for RA in (1, 2, 3) for n in range(1, D4_MAX_N + 1)})


Built = collections.namedtuple("Built", "model cores domain order udom pts")


def build(model):
    """Seeded cores, storage-frame domain, dim_order (every third model: a permutation; else None) and the rows: row 0
    on every lower domain end, row 1 on every upper end, the rest uniform.  A pure function of the model."""
    rng = np.random.default_rng([2031, model.number])
    d = len(model.n)
    cores = [rng.standard_normal((model.ranks[k], nk, model.ranks[k + 1])) * (DECAY ** np.arange(nk))[None, :, None]
             / np.sqrt(model.ranks[k]) for k, nk in enumerate(model.n)]
    domain = [[float(a), float(a + w)] for a, w in zip(rng.uniform(-5, 5, d), rng.uniform(0.1, 10, d))]
    order = [int(v) for v in rng.permutation(d)] if model.number % 3 == 0 else None
    udom = domain if order is None else [domain[order.index(u)] for u in range(d)]
    pts = np.column_stack([rng.uniform(a, b, model.rows) for a, b in udom])
    pts[0] = [a for a, _ in udom]
    if model.rows > 1:
        pts[1] = [b for _, b in udom]
    return Built(model, cores, domain, order, udom, np.ascontiguousarray(pts))


def storage_position(built, u):
    return u if built.order is None else built.order.index(u)


def deriv_specs(model):
    """The zero spec, order 1 and order 2 in every dimension in turn, one mixed pair that rotates with the model."""
    d = len(model.n)
    specs = [[0] * d]
    for u in range(d):
        for o in (1, 2):
            specs.append([o if v == u else 0 for v in range(d)])
    a, b = model.number % d, (model.number + 1) % d
    specs.append([1 if v == a else (2 if v == b else 0) for v in range(d)])
    return specs


def fd_specs(model):
    """The zero spec, one first order, one second order, one mixed pair; the dimensions rotate with the model."""
    d = len(model.n)
    a, b, c = model.number % d, (model.number + 1) % d, (model.number + 2) % d
    if c == a:
        c = b
    return [[0] * d, [int(v == a) for v in range(d)], [2 * int(v == b) for v in range(d)],
            [int(v in (a, c)) for v in range(d)]]


def box_cases(built):
    """[(dims, bounds (N, m, 2))]: every single dimension in turn, then all of them.  Widths 5 % - 100 % of the domain;
    row 0 is the whole domain, row 1 has lo == hi in its first integrated dimension."""
    m = built.model
    d, N = len(m.n), m.rows
    rng = np.random.default_rng([2032, m.number])
    out = []
    for dims in [[u] for u in range(d)] + [list(range(d))]:
        bounds = np.empty((N, len(dims), 2))
        for j, u in enumerate(dims):
            a, b = built.udom[u]
            w = rng.uniform(0.05, 1.0, N) * (b - a)
            lo = a + rng.uniform(0.0, 1.0, N) * ((b - a) - w)
            bounds[:, j, 0] = np.clip(lo, a, b)
            bounds[:, j, 1] = np.clip(lo + w, a, b)
            bounds[0, j] = (a, b)
        if N > 1:
            bounds[1, 0, 1] = bounds[1, 0, 0]
        out.append((dims, bounds))
    return out


def ladder_cases(built):
    """[(dim, xs)]: the first, a middle and the last user dimension, each with LADDER_M shared values (both domain
    ends among them) and with LADDER_M values per row."""
    m = built.model
    d = len(m.n)
    rng = np.random.default_rng([2033, m.number])
    out = []
    for dim in sorted({0, d // 2, d - 1}):
        a, b = built.udom[dim]
        out.append((dim, np.concatenate([[a, b], rng.uniform(a, b, LADDER_M - 2)])))
        out.append((dim, rng.uniform(a, b, (m.rows, LADDER_M))))
    return out


def ladder_positions(models):
    """{(side, n)}: the node counts left of, at and right of the ladder dimensions of ladder_cases, by storage position."""
    seen = set()
    for m in models:
        b = build(m)
        d = len(m.n)
        for dim in sorted({0, d // 2, d - 1}):
            p = storage_position(b, dim)
            seen |= {("left", m.n[k]) for k in range(p)} | {("at", m.n[p])} | {("right", m.n[k]) for k in range(p + 1, d)}
    return seen


# ---------------------------------------------------------------------------------------------- bounds
FAMILIES = ("value", "order1", "order2", "box", "ladder")


def family_of(spec):
    """A derivative spec's family: by its highest order (the mixed pair holds an order 2)."""
    return ("value", "order1", "order2")[max(int(v) for v in spec)]


def ratios(got, ref, amp):
    """|got - ref| / (eps A_row), elementwise; 0 where the amplitude is 0 (then ref and got must both be 0)."""
    got, ref, amp = np.asarray(got), np.asarray(ref), np.asarray(amp)
    err = np.abs(got.astype(LD) - ref)
    assert not np.any((amp == 0) & (err != 0)), "a row of amplitude zero is not exactly zero"
    return np.where(amp > 0, err / (LD(EPS) * np.where(amp > 0, amp, 1)), 0).astype(np.float64)


def restatement_ratios(built):
    """{family: worst ratio} of the float64 restatement against the long-double chain on one model's cases."""
    ld = Chain(built.cores, built.domain, built.order, built.pts, LD)
    f64 = Chain(built.cores, built.domain, built.order, built.pts, np.float64)
    worst = dict.fromkeys(FAMILIES, 0.0)

    def note(family, pair, refpair):
        worst[family] = max(worst[family], float(np.max(ratios(pair[0], refpair[0], refpair[1]))))
    for spec in deriv_specs(built.model):
        note(family_of(spec), f64.deriv(spec), ld.deriv(spec))
    for dims, bounds in box_cases(built):
        note("box", f64.box(dims, bounds), ld.box(dims, bounds))
    for dim, xs in ladder_cases(built):
        note("ladder", f64.ladder(dim, xs), ld.ladder(dim, xs))
    return worst


def restatement_value_ratio(built):
    """The worst ratio of the float64 restatement's value chain alone (the MFMA forms' lists: eval_batch only)."""
    ref = value_pair(Chain(built.cores, built.domain, built.order, built.pts, LD), group_of(built.model))
    got = Chain(built.cores, built.domain, built.order, built.pts, np.float64).value()
    return float(np.max(ratios(got[0], ref[0], ref[1])))


def value_pair(chain, group):
    """(values, amplitudes) a group's value rows are held to: "mfma-lowd" counts the one-eps error of s (Chain.value_s)."""
    return chain.value_s() if group == "mfma-lowd" else chain.value()


# Worst |y - ref| / (eps A_row) of the float64 restatement, measured by
# test_tt_chain_host.py::test_the_restatement_sets_every_K (which asserts these figures), and the row bound's factor K
# per family: 16 times that, rounded up to a power of two.  The 16 covers what the kernels do differently from the
# restatement: two partial sums from RL = 4 on, FMA contraction, the basis scale folded into q.  K <= 64: a rigorous
# running-error bound for d <= 6, n <= 16, r <= 16 is about 100 eps; above 64 the row bound no longer separates a
# dropped term from rounding.
#
# Two lists, each with the K of its own measurement.  "sweep": sweep_models() and tail_model().  "edge": edge_models().
# The edge list sits higher for a reason the amplitude does not see: s = (x - lo) sc - 1 carries an absolute error of up
# to one eps (the rounding of sc times t <= 2, then the subtraction), whatever the size of s, and that error enters the
# row as eps |c_1| while A_row holds only |c_1| |s|.  In a 2-D model of rank 1 nothing dilutes it (worst rows: s near 0);
# in the sweep's 4-D and 6-D models the rank sums' amplitudes do.  The kernels form s by the same rule, so this is the
# restatement's own error, not slack: stronger decay does not move it (0.55 -> 0.25: 1.8 .. 3.2 -> 2.4 .. 3.4).
#
# "mfma": mfma_models() of d >= 3 and mfma_extra_models(), value rows only (the MFMA forms are forms of eval_batch).
# Higher than the sweep: node counts up to 32 (513 in a last dimension) against 16, and rank sums of up to 64 terms.
#
# "mfma-lowd": mfma_models() of d <= 2.  Against A_row alone this list measures 4.02 (K would be 128): the d = 1,
# n = 32 model has a row at s = 0.95, and towards the ends |T_j'| grows to j^2, so the one-eps error of s described
# above enters as eps sum_j |c_j T_j'(s)| -- 5.7 times that row's A_row = sum_j |c_j T_j(s)| -- and a 1-D model has
# nothing to dilute it (its n = 7 model: 1.79).
# The mechanism is a property of the argument, not of the sum, so this group's amplitude states it: Chain.value_s adds to
# A_row the chain with |T_j'(s_k)| at position k, for every k -- the row's first-order change under one eps in s_k.  In
# those units the restatement's worst is 0.63 and K = 16: tighter than K = 128 on A_row for every row away from the
# ends, and still eps times sums of the row's own terms.  The device forms derive s by x - lo and one FMA, or (W-first)
# by the reference's division: at most the same one eps.
RESTATEMENT_WORST = {
    "sweep": {"value": 0.270, "order1": 0.405, "order2": 0.467, "box": 0.735, "ladder": 0.366},
    "edge": {"value": 1.842, "order1": 1.812, "order2": 3.244, "box": 2.908, "ladder": 2.797},
    "mfma": {"value": 1.208},
    "mfma-lowd": {"value": 0.628},
}
K_CAP = 64


def K_of(worst):
    return 2 ** int(np.ceil(np.log2(16.0 * worst)))


K = {group: {family: K_of(w) for family, w in fam.items()} for group, fam in RESTATEMENT_WORST.items()}


def group_of(model):
    if model.mode.startswith("mfma"):
        return "mfma" if len(model.n) >= 3 else "mfma-lowd"
    return "edge" if model.mode == "generic" else "sweep"
