"""K-remainder columns as the accumulators' seed in the row-code MFMA kernels (k_bary_mfma, k_bary_mfma4).

A plan whose folded tail has K = 1 or 2 (mod 4) columns keeps its first R = K mod 4 columns out of the fragment image
and the k-loop: they enter as the MFMA C operand, formed by R vector FMAs onto +0.0 per accumulator register.  The
f64 MFMA is a k-ordered FMA chain that starts from C, so the seeded form performs the operations of the padded form
in the same order: every result below is compared BIT FOR BIT with a handle created under PCX_BARY_SEED=0, which plans,
packs and launches the unseeded form.

Shapes are chosen by their planned tail: the dimension in front of the tail makes a three-dimensional tail longer
than the 256 columns a plan may fold, so the planner takes the last two dimensions; split and k-step count are
asserted through pcx_bary_kernel_info.
"""
import numpy as np
import pytest

from conftest import assert_parity, golden, spec_point_tol
import functions as F

from pychebyshev_amd import ChebyshevApproximation, _lib

pytestmark = pytest.mark.gpu

BATCHES = (1, 31, 33, 777, 66_000)       # one column tile per wave and split launches; a ragged last wave; two column tiles, unsplit


def _kernel_info(c):
    m = c._model()
    info = _lib.i32(np.zeros(6))
    _lib.check(m.lib.pcx_bary_kernel_info(m.handle, _lib.p_i32(info)), m.lib)
    return [int(v) for v in info]


def _grid_kind(c):
    m = c._model()
    info = _lib.i32(np.zeros(4))
    _lib.check(m.lib.pcx_bary_grid_info(m.handle, _lib.p_i32(info)), m.lib)
    return int(info[0])


def _set_kernel(c, variant):
    m = c._model()
    _lib.check(m.lib.pcx_bary_set_kernel(m.handle, variant), m.lib)


def _row_code_model(monkeypatch, T, dom, shape, seed_on):
    """The model on the row-code MFMA form (variant 2, the short-plan forms switched off at create), seeded or not."""
    monkeypatch.setenv("PCX_BARY_GRID", "0")
    monkeypatch.setenv("PCX_BARY_KFOLD", "0")
    monkeypatch.setenv("PCX_BARY_SEED", "1" if seed_on else "0")
    c = ChebyshevApproximation.from_values(T, len(shape), dom, list(shape))
    _set_kernel(c, 2)              # creates the handle: the environment is read here
    assert _grid_kind(c) == 0
    return c


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# shape, k-steps with the seed, k-steps without; the last two dimensions are the planned tail (split = 2)
CASES = [
    ((7, 11, 5, 5), 6, 7),          # K = 25, R = 1: plain tile loop, 5 row tiles (the last one ragged), 2 chunks
    ((9, 11, 7, 7), 12, 13),        # K = 49, R = 1: the shortest pipelined loop (12 k-steps)
    ((5, 15, 6, 3), 4, 5),          # K = 18, R = 2: two seed columns
    ((6, 11, 13, 13), 42, 44),      # K = 169, R = 1: exactly 42 k-steps (43 unseeded, which has no instantiation: 44)
    ((4, 18, 5, 3), 4, 4),          # control, K = 15: a remainder of 3 stays a k-step
    ((5, 17, 4, 4), 4, 4),          # control, K = 16: no remainder
]


def _check_model(oracle_mod, monkeypatch, T, dom, shape, ks_seed, ks_plain, split, pts, mixed, floor):
    d = len(shape)
    c = _row_code_model(monkeypatch, T, dom, shape, True)
    c0 = _row_code_model(monkeypatch, T, dom, shape, False)
    info, info0 = _kernel_info(c), _kernel_info(c0)
    assert (info[2], info[5]) == (ks_seed, split), f"{shape}: seeded plan {info}"
    assert (info0[2], info0[5]) == (ks_plain, split), f"{shape}: unseeded plan {info0}"
    n_big = BATCHES[-1]
    assert len(pts) == n_big
    # rows with every coordinate on a node: the node whose column is the seed (index 0 of both tail dimensions), the one
    # behind it, the last one, and a random one
    rng = np.random.default_rng(sum(shape))
    node_rows = [[0] * d, [0] * (d - 1) + [1], [0] * (d - 2) + [1, 0], [n - 1 for n in shape], [int(rng.integers(0, n)) for n in shape],
                 [int(rng.integers(0, n)) for n in shape[:-2]] + [0, 0]]
    for r, idx in enumerate(node_rows):
        pts[r] = [c.nodes[k][i] for k, i in enumerate(idx)]
        pts[n_big - 1 - r] = pts[r]                      # ... and in the ragged end of the large batch
    pts[20, d - 1] = np.nan                              # one row with a NaN coordinate (in every batch but the first)
    om = oracle_mod.BaryModel(c.nodes, c.weights, c.diff_matrices, c.tensor_values)
    specs = [[0] * d, mixed]
    sub = np.r_[0:20, 21:300, n_big - 300:n_big]         # the oracle's rows (finite ones)
    big = {}
    for s in specs:
        y = c.vectorized_eval_batch(pts, s)
        big[tuple(s)] = y
        assert np.isnan(y[20]) and np.isfinite(np.delete(y, 20)).all()
        # (a) against the oracle
        assert_parity(y[sub], oracle_mod.bary_eval_batch(om, pts[sub], s), 1e-12, f"seed {shape} {s}", spec_point_tol(s), floor=floor)
        for n in BATCHES:
            got = y if n == n_big else c.vectorized_eval_batch(pts[:n], s)
            # (d) a small batch equals the same rows of the large one
            assert _same(got, y[:n]), f"{shape} {s} N={n}: differs from the same rows of the large batch"
            # (b) the unseeded form gives the same bits
            assert _same(c0.vectorized_eval_batch(pts[:n], s), got), f"{shape} {s} N={n}: seeded and unseeded forms differ"
    # (c) grid points return the tensor entry exactly
    for r, idx in enumerate(node_rows):
        assert big[tuple(specs[0])][r] == T[tuple(idx)] == big[tuple(specs[0])][n_big - 1 - r], (shape, idx)
    # a multi-spec call (one launch, grid.z = 2; dim-0 groups do not apply to these specs)
    for n in (777, n_big):
        multi = c.vectorized_eval_multi_batch(pts[:n], specs)
        for j, s in enumerate(specs):
            assert _same(multi[:, j], big[tuple(s)][:n]), f"{shape} multi-spec column {s} N={n}"
        assert _same(c0.vectorized_eval_multi_batch(pts[:n], specs), multi), f"{shape} multi-spec N={n}: forms differ"


@pytest.mark.parametrize("shape,ks_seed,ks_plain", CASES)
def test_seeded_plans_match_oracle_and_unseeded_form(oracle_mod, monkeypatch, shape, ks_seed, ks_plain):
    rng = np.random.default_rng(1000 + sum(shape))
    T = rng.standard_normal(shape)
    dom = [[0.0, 1.0], [-1.0, 1.0], [2.0, 5.0], [-3.0, -1.0]]
    pts = np.column_stack([rng.uniform(lo, hi, BATCHES[-1]) for lo, hi in dom])
    _check_model(oracle_mod, monkeypatch, T, dom, shape, ks_seed, ks_plain, 2, pts, [1, 0, 0, 1], float(np.max(np.abs(T))))


def test_seeded_bs5d_matches_oracle_and_unseeded_form(oracle_mod, monkeypatch):
    """The headline model (golden g2): tail 11 x 11, K = 121 = 1 + 4 x 30, the pipelined loop."""
    T = golden("g2_bs5d")["tensor"]
    pts = F.bs5_query_points(BATCHES[-1], seed=17)
    _check_model(oracle_mod, monkeypatch, T, F.BS5_DOMAIN, tuple(F.BS5_NODES), 30, 31, 3, pts, [1, 0, 0, 1, 0], 0.0)


def test_both_mfma_forms_stay_bit_identical_with_the_seed(monkeypatch):
    """k_bary_mfma4 (variant 3) takes the same seed from the same array: its accumulator of row group rg is register
    j = rg of the 16x16x4 kernel's D layout."""
    T = golden("g2_bs5d")["tensor"]
    pts = F.bs5_query_points(70_000, seed=5)
    pts[7] = [120.0, 90.0, 1.0, 0.15, 0.08]
    res = {}
    for seed_on in (True, False):
        monkeypatch.setenv("PCX_BARY_SEED", "1" if seed_on else "0")
        c = ChebyshevApproximation.from_values(T, 5, F.BS5_DOMAIN, F.BS5_NODES)
        for variant in (2, 3):
            _set_kernel(c, variant)
            assert _kernel_info(c)[2] == (30 if seed_on else 31)
            res[seed_on, variant] = [c.vectorized_eval_batch(pts, s) for s in ([0] * 5, [1, 0, 0, 1, 0])]
    for key, val in res.items():
        for a, b in zip(val, res[True, 2]):
            assert np.array_equal(a, b), f"seed {key[0]} variant {key[1]} differs from the seeded 16x16x4 form"


def test_dim0_group_launch_is_bit_identical_with_the_seed(monkeypatch):
    """Price + delta + gamma in one multi-spec call at a batch large enough for dim-0 groups: the slab-packed launch
    (its own fragment image and seed array, packed per i0) gives the bits of the unseeded one."""
    T = golden("g2_bs5d")["tensor"]
    pts = F.bs5_query_points(66_480, seed=23)
    specs = [[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [2, 0, 0, 0, 0]]
    res = {}
    for seed_on in (True, False):
        monkeypatch.setenv("PCX_BARY_SEED", "1" if seed_on else "0")
        c = ChebyshevApproximation.from_values(T, 5, F.BS5_DOMAIN, F.BS5_NODES)
        m = c._model()
        assert _kernel_info(c)[2] == (30 if seed_on else 31)
        res[seed_on] = c.vectorized_eval_multi_batch(pts, specs)
        gem = _lib.i32(np.zeros(1))
        flat = _lib.i32(np.asarray(specs).ravel())
        _lib.check(m.lib.pcx_bary_count_gemms(m.handle, _lib.p_i32(flat), len(specs), len(pts), _lib.p_i32(gem)), m.lib)
        assert int(gem[0]) < len(specs), "the call formed no dim-0 group"
    assert np.array_equal(res[True], res[False])
