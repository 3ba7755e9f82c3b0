"""Host side of the batched box integrals (``integrate_batch`` of ChebyshevApproximation and ChebyshevSpline,
``ChebyshevSpline.integrate``): the arithmetic the device kernels restate, the argument rules -- every error is raised
before any device call, so these run without a GPU -- and the layout of the golden file."""
import os

import numpy as np
import pytest

from conftest import golden
import generate_golden_bary_box as G

from pychebyshev_amd import ChebyshevApproximation, ChebyshevSpline
from pychebyshev_amd._calculus import box_moments, box_quadrature_matrix, box_rows, box_weights
from pychebyshev_amd.barycentric import sub_interval_weights


def _model(shape=(5, 7, 6)):
    d = len(shape)
    dom = G.domain_of(d)
    nodes = ChebyshevApproximation.nodes(d, dom, list(shape))["nodes_per_dim"]
    return ChebyshevApproximation.from_values(G.grid_values(nodes), d, dom, list(shape))


def _spline(tag="Q"):
    n, knots, _ = G.SPLINES[tag]
    d = len(n)
    dom = G.domain_of(d)
    info = ChebyshevSpline.nodes(d, dom, n, knots)
    return ChebyshevSpline.from_values([G.grid_values(p["nodes_per_dim"]) for p in info["pieces"]], d, dom, n, knots)


# ------------------------------------------------------------------------------------------------- arithmetic
@pytest.mark.parametrize("n", [2, 3, 5, 11, 16, 33, 64])
def test_quadrature_matrix_times_moments_is_the_sub_interval_rule(n):
    """Q_n . mu against barycentric.sub_interval_weights (the reference's DCT-III of the moments): 1e-13 of the largest
    weight; measured 3e-15 on sub-intervals of 5 % of [-1, 1] and wider."""
    rng = np.random.default_rng(n)
    Q = box_quadrature_matrix(n)
    worst = 0.0
    for _ in range(100):
        w = rng.uniform(0.1, 2.0)
        lo = rng.uniform(-1.0, 1.0 - w)
        got = Q @ box_moments(n, lo, lo + w)
        ref = sub_interval_weights(n, lo, lo + w)
        worst = max(worst, float(np.max(np.abs(got - ref)) / np.max(np.abs(ref))))
    print(f"n={n}: worst {worst:.2e}")
    assert worst <= 1e-13
    for t in (-1.0, -0.3, 0.0, 0.77, 1.0):
        assert not box_moments(n, t, t).any()
        assert not (Q @ box_moments(n, t, t)).any()


def test_box_weights_integrate_the_interpolant():
    """(b - a) / 2 . Q_n mu integrates polynomials of degree < n exactly over [lo, hi]."""
    a, b, lo, hi = 0.5, 3.0, 0.9, 2.2
    for n in (3, 6, 11):
        nodes = ChebyshevApproximation.nodes(1, [[a, b]], [n])["nodes_per_dim"][0]
        w = box_weights(n, a, b, lo, hi)
        for deg in range(n):
            exact = (hi ** (deg + 1) - lo ** (deg + 1)) / (deg + 1)
            assert abs(w @ nodes ** deg - exact) <= 1e-13 * abs(exact)
    assert not box_weights(7, a, b, 1.25, 1.25).any()


def test_box_rows_layout_and_clipping():
    dom = [[0.0, 1.0], [2.0, 3.0], [-1.0, 1.0]]
    flags, rows = box_rows(3, dom, [2, 0], [[[0.0 - 5e-15, 0.5], [-0.5, 1.0 + 5e-15]]], [[2.5], [2.75]])
    assert flags.tolist() == [1, 0, 1]
    assert rows.tolist() == [[0.0, 0.5, 2.5, -0.5, 1.0], [0.0, 0.5, 2.75, -0.5, 1.0]]
    flags, rows = box_rows(1, [[0.0, 1.0]], 0, None, None)
    assert flags.tolist() == [1] and rows.tolist() == [[0.0, 1.0]]
    flags, rows = box_rows(2, dom[:2], [1], (2.25, 2.5), [[0.1], [0.2], [0.3]])
    assert rows.shape == (3, 3) and rows[:, 1].tolist() == [2.25] * 3


# ------------------------------------------------------------------------------------------------- argument rules
BATCH_ERRORS = [
    (dict(dims=[3], points=[[0.0, 1.0, -1.0]]), r"dims contains out-of-range index \(num_dimensions=3, dims=\[3\]\)"),
    (dict(dims=[-1], points=[[0.0, 1.0, -1.0]]), r"dims contains out-of-range index"),
    (dict(dims=[], points=[[0.0, 1.0, -1.0]]), r"dims must name at least one dimension"),
    (dict(dims=[0, 2], bounds=[[0.0, 0.5]], points=[[1.0]]), r"bounds must broadcast to \(N, 2, 2\), got shape \(1, 2\)"),
    (dict(dims=[0], bounds=[[0.0, 0.5, 0.7]], points=[[1.0, -1.0]]), r"bounds must broadcast to \(N, 1, 2\)"),
    (dict(dims=[0]), r"points is required: 2 dimensions are kept"),
    (dict(dims=[0], points=[[1.0]]), r"points must have shape \(N, 2\), got \(1, 1\)"),
    (dict(dims=[0], points=[1.0, -1.0]), r"points must have shape \(N, 2\), got \(2,\)"),
    (dict(dims=[0], bounds=[[0.0, 0.5], [0.1, 0.5], [0.2, 0.5]], points=[[1.0, -1.0], [1.0, -1.0]]),
     r"bounds has 3 rows but points has 2"),
    (dict(dims=[0], bounds=[[0.0, 0.5], [0.5, 0.25]], points=[[1.0, -1.0], [1.0, -1.0]]),
     r"bounds lo=0.5 > hi=0.25 for dim 0 \(row 1\)"),
    (dict(dims=[1], bounds=[0.25, 2.0], points=[[0.0, -1.0]]),
     r"bounds \(0.25, 2.0\) outside domain \[0.5, 3.0\] for dim 1 \(row 0\)"),
    (dict(dims=[1], bounds=[1.0, np.nan], points=[[0.0, -1.0]]), r"outside domain \[0.5, 3.0\] for dim 1 \(row 0\)"),
    (dict(dims=[0], points=[[1.0, -1.0], [3.5, -1.0]]),
     r"point value 3.5 for dim 1 is outside domain \[0.5, 3.0\] \(row 1\)"),
    (dict(dims=[0], points=[[1.0, np.nan]]), r"point value nan for dim 2 is outside domain \[-2.0, -0.25\] \(row 0\)"),
]


@pytest.mark.parametrize("kwargs,message", BATCH_ERRORS)
def test_approximation_integrate_batch_errors(kwargs, message):
    with pytest.raises(ValueError, match=message):
        _model().integrate_batch(**kwargs)


@pytest.mark.parametrize("kwargs,message", BATCH_ERRORS)
def test_spline_integrate_batch_errors(kwargs, message):
    with pytest.raises(ValueError, match=message):
        _spline("Q").integrate_batch(**kwargs)


def test_unbuilt_models_refuse():
    f = lambda x, _: float(sum(x))                                        # noqa: E731
    c = ChebyshevApproximation(f, 2, [[0.0, 1.0], [0.0, 1.0]], [4, 4])
    with pytest.raises(RuntimeError, match=r"Call build\(\) first"):
        c.integrate_batch([0], points=[[0.5]])
    s = ChebyshevSpline(f, 2, [[0.0, 1.0], [0.0, 1.0]], [4, 4], [[0.5], []])
    with pytest.raises(RuntimeError, match=r"Call build\(\) first"):
        s.integrate_batch([0], points=[[0.5]])
    with pytest.raises(RuntimeError, match=r"Call build\(\) first"):
        s.integrate()


def test_empty_batches_need_no_device():
    assert _model().integrate_batch([0], points=np.zeros((0, 2))).shape == (0,)
    assert _spline("P").integrate_batch([1], points=np.zeros((0, 1))).shape == (0,)


@pytest.mark.parametrize("kwargs,message", [
    (dict(dims=[3]), r"dim 3 out of range \[0, 2\]"),
    (dict(dims=-1), r"dim -1 out of range \[0, 2\]"),
    (dict(dims=[0, 1], bounds=[(0.0, 0.5)]), r"bounds length 1 != dims length 2"),
    (dict(dims=[0], bounds=[(0.5, 0.25)]), r"bounds lo=0.5 > hi=0.25 for dim 0"),
    (dict(dims=[1], bounds=(0.25, 2.0)), r"bounds \(0.25, 2.0\) outside domain \[0.5, 3.0\] for dim 1"),
    (dict(bounds=[(-1.0, 1.0), (0.5, 3.5), None]), r"bounds \(0.5, 3.5\) outside domain \[0.5, 3.0\] for dim 1"),
])
def test_spline_integrate_errors(kwargs, message):
    with pytest.raises(ValueError, match=message):
        _spline("Q").integrate(**kwargs)


# ------------------------------------------------------------------------------------------------- golden file
def test_golden_file_has_the_groups():
    g = golden("g24_bary_box")
    for tag, shape in G.MODELS.items():
        d = len(shape)
        assert tuple(g[f"{tag}_shape"]) == tuple(shape)
        groups = G.model_groups(d)
        assert f"{tag}_box{len(groups)}" not in g.files
        for i, dims in enumerate(groups):
            m = len(dims)
            assert g[f"{tag}_box{i}"].shape == (G.ROWS, 2 * m + (d - m) + 1)
            b, p, ref = G.split_group(g[f"{tag}_box{i}"], m)
            dom = np.asarray(G.domain_of(d))
            assert np.array_equal(b[0], dom[dims])                            # row 0: the whole domain
            assert b[1, 0, 0] == b[1, 0, 1] and ref[1] == 0.0                 # row 1: an empty box
            assert (b[:, :, 0] >= dom[dims, 0]).all() and (b[:, :, 1] <= dom[dims, 1]).all()
            width = (b[:, :, 1] - b[:, :, 0]) / (dom[dims, 1] - dom[dims, 0])[None, :]
            if d > m:
                kept0 = [k for k in range(d) if k not in dims][0]
                assert p[2, 0] == dom[kept0, 0] and p[3, 0] == dom[kept0, 1]
                nodes = ChebyshevApproximation.nodes(d, dom.tolist(), list(shape))["nodes_per_dim"][kept0]
                assert np.min(np.abs(nodes - p[4, 0])) < 1e-14
            rest = np.delete(width, 1, axis=0)
            if m <= 2:
                assert (np.sum(rest < 0.06, axis=0) >= 4).all() and rest.min() > 0.04
            else:
                assert rest.min() >= 0.39
            assert np.mean(np.abs(ref) >= 1e-3 * np.max(np.abs(ref))) >= G.MIN_SHARE
        assert g[f"{tag}_int"].shape == (d + 1, 2) and np.isfinite(g[f"{tag}_int"]).all()
    for tag, (n, knots, groups) in G.SPLINES.items():
        d = len(n)
        assert tuple(g[f"{tag}_shape"]) == tuple(n)
        assert f"{tag}_box{len(groups)}" not in g.files
        for i, dims in enumerate(groups):
            m = len(dims)
            assert g[f"{tag}_box{i}"].shape == (G.ROWS, 2 * m + (d - m) + 1)
            b, p, ref = G.split_group(g[f"{tag}_box{i}"], m)
            assert ref[1] == 0.0
            knotted = [j for j, k in enumerate(dims) if knots[k]]
            if knotted:
                j, kn = knotted[0], knots[dims[knotted[0]]]
                assert b[2, j, 1] < kn[0]                                             # inside the first piece
                assert b[3, j, 0] < kn[0] < b[3, j, 1] and (len(kn) == 1 or b[3, j, 1] < kn[1])
                assert b[4, j, 0] < kn[0] and kn[-1] < b[4, j, 1]                     # across every knot
                assert b[5, j, 0] == kn[0] and b[6, j, 1] == kn[-1]                   # an edge on a knot
            for c, k in enumerate([k for k in range(d) if k not in dims]):
                for v in knots[k]:
                    assert np.min(np.abs(p[:, c] - v)) >= 0.05
            assert np.mean(np.abs(ref) >= 1e-3 * np.max(np.abs(ref))) >= G.MIN_SHARE
        assert g[f"{tag}_int"].shape == (d + 1, 2)
        for i, (dims, _) in enumerate(G.SPLINE_PARTIALS[tag]):
            assert f"{tag}_part{i}_piece0" in g.files and g[f"{tag}_part{i}_eval"].shape == (G.ROWS, d - len(dims) + 1)
    # tens of kilobytes: one array per group (an archive member costs about 250 bytes) and inputs on a grid of 2^-8
    assert os.path.getsize(os.path.join(os.path.dirname(G.__file__), "g24_bary_box.npz")) < 80 * 1024
