"""``ChebyshevSpline`` -- piecewise Chebyshev interpolant (knots at kinks), evaluated on an
MI355X through ``libpcx_hip.so``.

Host-side mirror of the reference class (``/root/reference/src/pychebyshev/spline.py``,
v0.21.1) for the evaluation path, the direct caller of the barycentric hot path:

    __init__ / build (one ChebyshevApproximation per sub-domain)        (:106-412)
    _find_piece / _check_knot_boundary                                   (:414-446, :519-550)
    eval / eval_multi / eval_batch                                       (:552-704)
    get_derivative_id, num_pieces, total_build_evals, build_time, pickle, repr

``eval_batch`` in the reference buckets the points with ``np.searchsorted`` and calls each
piece's ``vectorized_eval_batch``.  Here routing, bucketing and the per-piece barycentric
launches all run on the device (``pcx_spline_eval_batch``: ``k_spline_piece_id`` ->
``k_spline_scatter`` -> one ``k_bary_mfma`` launch per non-empty piece on its bucket).

Auto-N pieces (``error_threshold``) build through the pieces' own doubling loop; ``.pcb`` files
(class tag 2) are read and written byte-compatibly.  ``sobol_indices`` aggregates the pieces' device-side indices
on the host as the reference does.  ``roots_batch`` / ``minimize_batch`` / ``maximize_batch`` expand every row into the
fibre points of all pieces along the dimension, evaluate them with the spline's own routing and kernels, solve every fibre
and merge the pieces of a row on the device (``pcx_spline_calculus_batch``); ``roots`` / ``minimize`` / ``maximize`` are
the one-row batch, or, above 64 nodes in a piece, the pieces' own calls merged on the host.  ``slice`` picks the pieces
that contain the value and slices each on the device; ``extrude`` repeats every piece's tensor on the host.  ``+``, ``-``, ``*`` and ``/`` combine the pieces' value tensors on the host.
``integrate`` contracts each piece on the device and sums the pieces along the integrated dimensions;
``integrate_batch`` is the box integral with another box per row: one ``pcx_bary_box_batch`` launch per piece on the
rows whose box reaches it.  ``eval_grid`` (extension) evaluates a tensor-product grid without routing a single point:
the intervals of the axis entries split the grid into one sub-grid per piece, every piece that holds a point runs its own
grid evaluation (``d`` mode products) into its block of a packed staging buffer, and ``k_spline_grid_place`` copies the
blocks into the result (``pcx_spline_eval_tensor_grid``; the planner is ``csrc/spline_grid_plan.h``).  Not provided:
auto_knots.
"""
from __future__ import annotations

import ctypes
import itertools
import pickle
import time
import warnings
from typing import Callable, List, Sequence, Tuple

import numpy as np

from . import _algebra, _calculus, _lib
from ._algebra import ValueAlgebraMixin
from ._calculus import FibreCalculusMixin
from ._derivative_ids import DerivativeIdMixin
from ._ergonomics import ErgonomicsMixin
from ._version import __version__
from .barycentric import ChebyshevApproximation

__all__ = ["ChebyshevSpline"]


def _is_nested(n_nodes) -> bool:
    return any(isinstance(x, (list, tuple)) for x in n_nodes)


class _DeviceSpline:
    """Owner of one ``pcx_spline`` handle; keeps the piece device models alive."""

    def __init__(self, spline: "ChebyshevSpline", device: int):
        lib = _lib.load()
        d = spline.num_dimensions
        self.models = []
        for piece in spline._pieces:
            piece._device_index = device
            self.models.append(piece._model())
        n_knots = _lib.i32([len(k) for k in spline.knots])
        flat = [float(v) for k in spline.knots for v in k]
        knots = _lib.f64(flat if flat else [0.0])
        arr = (ctypes.c_void_p * len(self.models))(*[m.handle for m in self.models])
        handle = ctypes.c_void_p()
        _lib.check(lib.pcx_spline_create(device, d, _lib.p_i32(n_knots), _lib.p_f64(knots),
                                         ctypes.cast(arr, _lib.c_vpp), len(self.models),
                                         ctypes.byref(handle)), lib)
        self.lib = lib
        self.handle = handle
        self.device = device
        self.tensors = [p.tensor_values for p in spline._pieces]      # the arrays themselves, not their ids

    def matches(self, spline: "ChebyshevSpline") -> bool:
        return (len(self.tensors) == len(spline._pieces)
                and all(a is p.tensor_values for a, p in zip(self.tensors, spline._pieces)))

    def __del__(self):
        try:
            if self.handle:
                self.lib.pcx_spline_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class ChebyshevSpline(ErgonomicsMixin, DerivativeIdMixin, FibreCalculusMixin, ValueAlgebraMixin):
    """Piecewise Chebyshev interpolation with user-specified knots (signature: reference
    spline.py:106-123)."""

    def __init__(self, function: Callable, num_dimensions: int,
                 domain: Sequence[Tuple[float, float]], n_nodes=None, knots=None,
                 max_derivative_order: int = 2, error_threshold: float | None = None, max_n: int = 64,
                 additional_data: object = None, *, defer_build: bool = False,
                 n_workers: int | None = None):
        from . import Domain, Ns
        if isinstance(domain, Domain):
            domain = list(domain.bounds)
        if isinstance(n_nodes, Ns):
            n_nodes = list(n_nodes.counts)
        self.function = function
        self.num_dimensions = num_dimensions
        self.domain = domain
        self.error_threshold = error_threshold
        if max_n < 3:
            raise ValueError(f"max_n must be at least 3 (the initial N of the doubling loop), "
                             f"got max_n={max_n}. For a grid smaller than 3 per dimension, pass "
                             f"n_nodes explicitly instead of using error-threshold auto-calibration.")
        self.max_n = max_n
        self.n_workers = n_workers
        if n_nodes is None:
            if error_threshold is None:
                raise ValueError("Must provide either n_nodes (explicit) or error_threshold "
                                 "(auto-N). Got neither.")
            n_nodes = [None] * num_dimensions
        else:
            n_nodes = list(n_nodes)
            if any(n is None for n in n_nodes) and error_threshold is None:
                raise ValueError("None entries in n_nodes require error_threshold to be set "
                                 "(auto-N mode).")
        self._n_nodes_nested = _is_nested(n_nodes)
        if self._n_nodes_nested and not all(isinstance(x, (list, tuple)) for x in n_nodes):
            raise ValueError("n_nodes must be fully nested (all dims as lists) when any "
                             "dim is nested; got mixed form")
        self.n_nodes = n_nodes
        if knots is None:
            knots = [[] for _ in range(num_dimensions)]
        self.knots = knots
        self.max_derivative_order = max_derivative_order
        self.additional_data = additional_data
        self._derivative_id_registry: dict = {}
        self._derivative_id_to_orders: list = []
        self.descriptor = ""

        for d in range(num_dimensions):
            lo, hi = domain[d]
            for k in knots[d]:
                if not (lo < k < hi):
                    raise ValueError(f"Knot {k} for dimension {d} is not strictly "
                                     f"inside domain [{lo}, {hi}]")
            if list(knots[d]) != sorted(knots[d]):
                raise ValueError(f"Knots for dimension {d} must be sorted")

        self._intervals: List[List[Tuple[float, float]]] = []
        for d in range(num_dimensions):
            lo, hi = domain[d]
            edges = [lo] + list(knots[d]) + [hi]
            self._intervals.append([(edges[i], edges[i + 1]) for i in range(len(edges) - 1)])
        self._shape = tuple(len(iv) for iv in self._intervals)

        if self._n_nodes_nested:
            for d in range(num_dimensions):
                expected = len(knots[d]) + 1
                if len(n_nodes[d]) != expected:
                    raise ValueError(f"n_nodes[{d}] must have {expected} entries "
                                     f"(one per sub-interval); got {len(n_nodes[d])}")
                inner = list(n_nodes[d])
                if any(x is None for x in inner) and error_threshold is None:
                    raise ValueError("None entries in nested n_nodes require error_threshold "
                                     "to be set (auto-N mode).")
                n_nodes[d] = inner
            self.n_nodes = n_nodes

        self._pieces: List[ChebyshevApproximation | None] = [None] * int(np.prod(self._shape))
        self._built = False
        self._build_time = 0.0
        self._cached_error_estimate = None
        self._device_spline: _DeviceSpline | None = None
        self._device_index: int | None = None

        if defer_build:
            if function is not None:
                raise ValueError("defer_build=True requires function=None (the deferred-construction "
                                 "workflow expects values to be supplied via "
                                 "set_original_function_values() later)")
            for flat, multi in enumerate(itertools.product(*[range(s) for s in self._shape])):
                self._pieces[flat] = ChebyshevApproximation(
                    None, num_dimensions, self._piece_domain(multi), self._piece_nodes(multi),
                    max_derivative_order=max_derivative_order, additional_data=additional_data,
                    defer_build=True, n_workers=n_workers)

    # ---------------------------------------------------------------- pieces
    def _piece_domain(self, multi):
        return [list(self._intervals[d][multi[d]]) for d in range(self.num_dimensions)]

    def _piece_nodes(self, multi):
        if self._n_nodes_nested:
            return [self.n_nodes[d][multi[d]] for d in range(self.num_dimensions)]
        return list(self.n_nodes)

    def set_original_function_values(self, per_piece_values) -> None:
        """Fill a ``defer_build=True`` spline: one value tensor per piece, C order over the
        per-dimension intervals (reference spline.py:269-323)."""
        if self._built:
            raise RuntimeError("spline is already constructed; "
                               "set_original_function_values() is for defer_build=True objects")
        if len(per_piece_values) != len(self._pieces):
            raise ValueError(f"expected {len(self._pieces)} per-piece tensors, got {len(per_piece_values)}")
        for piece, vals in zip(self._pieces, per_piece_values):
            piece.set_original_function_values(vals)
        self.function = None
        self._built = True
        self._device_spline = None

    def build(self, verbose: bool | int = True) -> None:
        """Build every piece on its sub-domain (reference spline.py:325-412)."""
        if self.function is None:
            raise RuntimeError("Cannot build: no function assigned. "
                               "This object was created via from_values() or load().")
        start = time.time()
        self._cached_error_estimate = None
        total_pieces = int(np.prod(self._shape))
        if verbose:
            print(f"Building {self.num_dimensions}D Chebyshev Spline ({total_pieces} pieces, "
                  f"{self.total_build_evals:,} total evaluations)...")
        for flat, multi in enumerate(itertools.product(*[range(s) for s in self._shape])):
            sub_domain = self._piece_domain(multi)
            piece = ChebyshevApproximation(
                self.function, self.num_dimensions, sub_domain, self._piece_nodes(multi),
                max_derivative_order=self.max_derivative_order, error_threshold=self.error_threshold,
                max_n=self.max_n, additional_data=self.additional_data, n_workers=self.n_workers)
            piece.build(verbose=False)
            self._pieces[flat] = piece
            if verbose:
                print(f"  Piece {flat + 1}/{total_pieces}: domain {sub_domain}, n_nodes={piece.n_nodes}")
        self._build_time = time.time() - start
        self._built = True
        self._device_spline = None
        if verbose:
            print(f"Build complete in {self._build_time:.3f}s")

    @staticmethod
    def _validated_intervals(num_dimensions: int, domain, knots):
        """Per-dimension sub-intervals after the checks ``nodes`` and ``from_values`` share."""
        for d in range(num_dimensions):
            lo, hi = domain[d]
            if lo >= hi:
                raise ValueError(f"domain[{d}]: lo={lo} must be strictly less than hi={hi}")
            for k in knots[d]:
                if not (lo < k < hi):
                    raise ValueError(f"Knot {k} for dimension {d} is not strictly "
                                     f"inside domain [{lo}, {hi}]")
            if list(knots[d]) != sorted(knots[d]):
                raise ValueError(f"Knots for dimension {d} must be sorted")
            if len(knots[d]) != len(set(knots[d])):
                raise ValueError(f"Knots for dimension {d} contain duplicates")
        out = []
        for d in range(num_dimensions):
            edges = [domain[d][0]] + list(knots[d]) + [domain[d][1]]
            out.append([(edges[i], edges[i + 1]) for i in range(len(edges) - 1)])
        return out

    @staticmethod
    def nodes(num_dimensions: int, domain, n_nodes, knots) -> dict:
        """Where ``from_values`` expects its samples: one grid per piece, pieces in C order over the
        per-dimension intervals (reference spline.py:1105-1216)."""
        if _is_nested(n_nodes):
            raise NotImplementedError("ChebyshevSpline.nodes() accepts only flat n_nodes "
                                      "(one int per dim, shared across pieces).")
        intervals = ChebyshevSpline._validated_intervals(num_dimensions, domain, knots)
        shape = tuple(len(iv) for iv in intervals)
        pieces = []
        for multi in itertools.product(*[range(n) for n in shape]):
            sub = [intervals[d][multi[d]] for d in range(num_dimensions)]
            info = ChebyshevApproximation.nodes(num_dimensions, [list(b) for b in sub], n_nodes)
            pieces.append({"piece_index": multi, "sub_domain": sub, "nodes_per_dim": info["nodes_per_dim"],
                           "full_grid": info["full_grid"], "shape": info["shape"]})
        return {"pieces": pieces, "num_pieces": int(np.prod(shape)), "piece_shape": shape}

    @classmethod
    def from_values(cls, piece_values, num_dimensions: int, domain, n_nodes, knots,
                    max_derivative_order: int = 2) -> "ChebyshevSpline":
        """Spline from precomputed value tensors, one per piece in C order over the
        per-dimension intervals, all of shape ``tuple(n_nodes)`` (reference spline.py:1218-1358).
        The result has ``function=None`` and is fully built."""
        if _is_nested(n_nodes):
            raise NotImplementedError("ChebyshevSpline.from_values() accepts only flat n_nodes "
                                      "(one int per dim, shared across pieces).")
        cls._validated_intervals(num_dimensions, domain, knots)
        obj = cls(None, num_dimensions, [list(b) for b in domain], n_nodes=list(n_nodes),
                  knots=[list(k) for k in knots], max_derivative_order=max_derivative_order)
        if len(piece_values) != len(obj._pieces):
            raise ValueError(f"Expected {len(obj._pieces)} piece_values, got {len(piece_values)}")
        want = tuple(n_nodes)
        for flat, pv in enumerate(piece_values):
            if np.asarray(pv).shape != want:
                raise ValueError(f"piece_values[{flat}] has shape {np.asarray(pv).shape}, expected {want}")
        for flat, multi in enumerate(itertools.product(*[range(n) for n in obj._shape])):
            obj._pieces[flat] = ChebyshevApproximation.from_values(
                piece_values[flat], num_dimensions, obj._piece_domain(multi), list(n_nodes),
                max_derivative_order=max_derivative_order)
        obj._built = True
        return obj

    @classmethod
    def from_pieces(cls, pieces: Sequence[ChebyshevApproximation], num_dimensions: int, domain, knots,
                    max_derivative_order: int = 2) -> "ChebyshevSpline":
        """Assemble a spline from already-built pieces in C order over the intervals
        (extension; the reference's internal ``_from_pieces``, spline.py:1364-1389)."""
        n_nodes = [[None] * (len(k) + 1) for k in knots]
        obj = cls(None, num_dimensions, domain, n_nodes=n_nodes, knots=knots,
                  max_derivative_order=max_derivative_order, error_threshold=0.0)
        if len(pieces) != len(obj._pieces):
            raise ValueError(f"expected {len(obj._pieces)} pieces, got {len(pieces)}")
        for multi, piece in zip(itertools.product(*[range(s) for s in obj._shape]), pieces):
            for d in range(num_dimensions):
                obj.n_nodes[d][multi[d]] = piece.n_nodes[d]
        obj.error_threshold = None
        obj._pieces = list(pieces)
        obj._built = True
        return obj

    # ---------------------------------------------------------------- device plumbing
    def to_device(self, device: int | None = None) -> "ChebyshevSpline":
        if not self._built:
            raise RuntimeError("Call build() first")
        dev = _lib.default_device() if device is None else int(device)
        self._device_index = dev
        self._device_spline = _DeviceSpline(self, dev)
        return self

    def _dev(self) -> _DeviceSpline:
        s = self._device_spline
        if s is None or not s.matches(self):
            self.to_device(self._device_index)
            s = self._device_spline
        return s

    def _points(self, points) -> np.ndarray:
        pts = _lib.f64(points)
        if pts.ndim != 2 or pts.shape[1] != self.num_dimensions:
            raise ValueError(f"points must have shape (N, {self.num_dimensions}), got {pts.shape}")
        return pts

    # ---------------------------------------------------------------- evaluation API
    def _find_piece(self, point) -> Tuple[int, ChebyshevApproximation]:
        """Piece containing ``point``: ``searchsorted(knots, x, side='right')`` per dimension,
        clamped (reference spline.py:414-446)."""
        multi = []
        for d in range(self.num_dimensions):
            if len(self.knots[d]) == 0:
                multi.append(0)
            else:
                idx = int(np.searchsorted(self.knots[d], point[d], side="right"))
                multi.append(min(idx, self._shape[d] - 1))
        flat = int(np.ravel_multi_index(multi, self._shape))
        return flat, self._pieces[flat]

    def _check_knot_boundary(self, point, derivative_order) -> None:
        """Derivatives are undefined exactly at a knot (reference spline.py:519-550)."""
        if all(o == 0 for o in derivative_order):
            return
        for d in range(self.num_dimensions):
            if derivative_order[d] > 0:
                for k in self.knots[d]:
                    if abs(point[d] - k) < 1e-14:
                        raise ValueError(f"Derivative w.r.t. dimension {d} is not defined at knot "
                                         f"x[{d}]={k}. The left and right derivatives may differ "
                                         f"at this point.")

    def eval(self, point, derivative_order=None, *, derivative_id=None) -> float:
        """Value/derivative at one point (reference spline.py:552-595)."""
        if not self._built:
            raise RuntimeError("Call build() before eval().")
        derivative_order = self._resolve_derivative_args(derivative_order, derivative_id)
        self._check_knot_boundary(point, derivative_order)
        return float(self.eval_batch(np.asarray([list(point)], dtype=float), derivative_order)[0])

    def eval_multi(self, point, derivative_orders) -> List[float]:
        """Several derivative specs at one point (reference spline.py:597-631)."""
        if not self._built:
            raise RuntimeError("Call build() before eval_multi().")
        for spec in derivative_orders:
            self._check_knot_boundary(point, spec)
        out = self.eval_multi_batch(np.asarray([list(point)], dtype=float), derivative_orders)
        return [float(v) for v in out[0]]

    def eval_batch(self, points, derivative_order=None, *, derivative_id=None) -> np.ndarray:
        """Values at ``(N, d)`` points, routed and bucketed per piece on the device
        (reference spline.py:633-704)."""
        if not self._built:
            raise RuntimeError("Call build() before eval_batch().")
        derivative_order = self._resolve_derivative_args(derivative_order, derivative_id)
        spec = _lib.i32(derivative_order)
        if spec.shape != (self.num_dimensions,):
            raise ValueError(f"derivative_order must have {self.num_dimensions} entries")
        from .device import as_device_array
        dev_pts = as_device_array(points)
        if dev_pts is not None:
            return self._eval_dev(dev_pts, spec.reshape(1, -1), True)
        pts = self._points(np.asarray(points, dtype=float))
        s = self._dev()
        out = np.empty(pts.shape[0])
        _lib.check(s.lib.pcx_spline_eval_batch(s.handle, _lib.p_f64(pts), pts.shape[0], _lib.p_i32(spec),
                                               _lib.p_f64(out)), s.lib)
        return out

    def eval_multi_batch(self, points, derivative_orders) -> np.ndarray:
        """Batched ``eval_multi``: ``(N, d)`` points x ``m`` specs -> ``(N, m)`` (extension)."""
        if not self._built:
            raise RuntimeError("Call build() before eval_multi_batch().")
        specs = _lib.i32(np.asarray(derivative_orders).reshape(-1, self.num_dimensions))
        from .device import as_device_array
        dev_pts = as_device_array(points)
        if dev_pts is not None:
            return self._eval_dev(dev_pts, specs, False)
        pts = self._points(np.asarray(points, dtype=float))
        s = self._dev()
        out = np.empty((pts.shape[0], specs.shape[0]))
        _lib.check(s.lib.pcx_spline_eval_multi_batch(s.handle, _lib.p_f64(pts), pts.shape[0], _lib.p_i32(specs),
                                                     specs.shape[0], _lib.p_f64(out)), s.lib)
        return out

    def _eval_dev(self, dev_pts, specs: np.ndarray, flat: bool):
        """Device-resident batch (:mod:`pychebyshev_amd.device`): ``(N,)`` / ``(N, m)`` ``DeviceArray``;
        specs go in groups of 64 (one ``pcx_spline_eval_multi_batch_dev`` call each)."""
        from .device import DeviceArray, check_points
        s = self._dev()
        n = check_points(dev_pts, self.num_dimensions, s.device)
        m = specs.shape[0]
        out = DeviceArray.empty((n,) if flat else (n, m), s.device)
        if n == 0:
            return out
        # any number of specs: the library evaluates them in groups of 64 (as it does for host-pointer batches)
        _lib.check(s.lib.pcx_spline_eval_multi_batch_dev(s.handle, ctypes.c_void_p(dev_pts.ptr), n, _lib.p_i32(specs), m,
                                                         ctypes.c_void_p(out.ptr)), s.lib)
        return out

    def eval_grid(self, axes, derivative_order=None, *, derivative_id=None, out=None):
        """The spline on the tensor-product grid ``axes[0] x ... x axes[d-1]`` (extension; what the reference's
        ``plot_1d`` / ``plot_2d_surface`` and a risk ladder over a kinked payoff evaluate point by point):
        ``result[i_0, ..., i_{d-1}] = eval_batch(meshgrid)[...]``, shape ``(m_0, ..., m_{d-1})`` -- ``eval_batch``'s
        rule, not ``eval``'s: a coordinate on a knot belongs to the right-hand piece, one outside the domain to the end
        piece, and a derivative spec is not checked against the knots.

        ``axes``, ``derivative_order`` / ``derivative_id`` and ``out`` as in ``ChebyshevApproximation.eval_grid``.
        Piece routing is separable per dimension, so the grid falls apart into one sub-grid per piece: every piece
        that holds a grid point evaluates its own small tensor grid (``d`` mode products) and one kernel places the
        blocks into the result (``pcx_spline_eval_tensor_grid``); no point is routed, counted or bucketed."""
        from .barycentric import _composite_eval_grid
        return _composite_eval_grid(self, "pcx_spline_eval_tensor_grid", axes, derivative_order, derivative_id, out)

    def piece_indices(self, points) -> np.ndarray:
        """Flat piece index of every point, computed on the device (diagnostic)."""
        pts = self._points(np.asarray(points, dtype=float))
        s = self._dev()
        ids = np.zeros(pts.shape[0], dtype=np.int32)
        _lib.check(s.lib.pcx_spline_piece_ids(s.handle, _lib.p_f64(pts), pts.shape[0], _lib.p_i32(ids)), s.lib)
        return ids

    # ---------------------------------------------------------------- sensitivity
    def sobol_indices(self) -> dict:
        """Sobol indices of the piecewise interpolant (reference spline.py:735-800): each piece's variance and
        indices come from the device (``pcx_bary_sobol`` on its handle); a piece weighs ``volume * variance``, so
        the spline's variance is the sum of the weights and each index the weight-averaged piece index."""
        if not self._built:
            raise RuntimeError("Call build() first")
        d = self.num_dimensions
        results = [(float(np.prod([hi - lo for lo, hi in p.domain])), p.sobol_indices())
                   for p in self._pieces if p is not None]
        weight = np.array([vol * res["variance"] for vol, res in results])
        variance = float(weight.sum()) if results else 0.0
        if variance == 0:
            return {"first_order": {k: 0.0 for k in range(d)}, "total_order": {k: 0.0 for k in range(d)},
                    "variance": 0.0}
        out = {"variance": variance}
        for key in ("first_order", "total_order"):
            idx = np.array([[res[key][k] for k in range(d)] for _, res in results])
            out[key] = {k: float(v) for k, v in enumerate(weight @ idx / variance)}
        return {"first_order": out["first_order"], "total_order": out["total_order"], "variance": variance}

    # ---------------------------------------------------------------- calculus
    def _calculus_pieces(self, dim, fixed):
        """The validated ``dim`` and, along it, each piece selected by the fixed values (``searchsorted(knots, v,
        side="right")`` capped at the last interval, as the reference's ``slice``) with its own ``fixed``."""
        self._fibre_check_built()
        d = self.num_dimensions
        dim, params = _calculus.validate_calculus_args(d, dim, fixed, self.domain)
        vals = dict(params)
        ranges = []
        for k in range(d):
            if k == dim:
                ranges.append(range(self._shape[k]))
            elif len(self.knots[k]) == 0:
                ranges.append([0])
            else:
                ranges.append([min(int(np.searchsorted(self.knots[k], vals[k], side="right")), self._shape[k] - 1)])
        sub = {k: v for k, v in vals.items()} if d > 1 else None
        pieces = [self._pieces[int(np.ravel_multi_index(multi, self._shape))] for multi in itertools.product(*ranges)]
        return dim, pieces, sub

    def _dim_counts(self, dim: int):
        """Node counts along ``dim`` of the pieces with index 0, 1, ... there, or None when pieces that share an index
        differ (auto-N pieces may): the device batch takes the nodes of index j from one piece."""
        along = np.array([p.n_nodes[dim] for p in self._pieces], dtype=int).reshape(self._shape)
        along = np.moveaxis(along, dim, 0).reshape(self._shape[dim], -1)
        if np.any(along != along[:, :1]):
            return None
        return [int(v) for v in along[:, 0]]

    _fibre_prefix = "pcx_spline"

    def _fibre_counts(self):
        """The largest node count over the pieces, by dimension: what the 64-node cap sees."""
        return [max(int(p.n_nodes[k]) for p in self._pieces) for k in range(self.num_dimensions)]

    def _fibre_shape(self, dim: int):
        """The batch results' ``n`` is the longest piece's, their width the sum over the pieces along ``dim``."""
        counts = self._dim_counts(dim)
        return max(counts), sum(max(n - 1, 1) for n in counts)

    def _fibre_nodes(self, dim: int) -> np.ndarray:
        stride = int(np.prod(self._shape[dim + 1:], dtype=int))
        return np.concatenate([np.asarray(self._pieces[j * stride].nodes[dim], dtype=float) for j in range(self._shape[dim])])

    def _calculus(self, dim, fixed, mode: str):
        """A single call: the one-row batch when every piece along ``dim`` has at most 64 nodes (one device call for all
        pieces), else every piece on its own (their single calls finish long fibres on the host) and the host merge."""
        dim, pieces, sub = self._calculus_pieces(dim, fixed)
        counts = self._dim_counts(dim)
        if counts is not None and max(counts) <= _calculus.MAX_DEVICE_N:
            row = _calculus.fixed_row(self.num_dimensions, dim, list((sub or {}).items()))
            out = self._calculus_batch(dim, row, _calculus._MODES[mode])
            return _calculus.single_roots(*out) if mode == "roots" else _calculus.single_extremum(*out)
        if mode == "roots":
            return _calculus.merge_pieces("roots", [p.roots(dim, sub) for p in pieces], self.domain[dim])
        return _calculus.merge_pieces(mode, [(p.minimize if mode == "min" else p.maximize)(dim, sub) for p in pieces])

    def _level_roots(self, dim, fixed, level: np.ndarray) -> np.ndarray:
        """As :meth:`_calculus` for the roots at a level: the one-row batch, or every piece on its own and the host
        merge."""
        dim, pieces, sub = self._calculus_pieces(dim, fixed)
        counts = self._dim_counts(dim)
        if counts is not None and max(counts) <= _calculus.MAX_DEVICE_N:
            row = _calculus.fixed_row(self.num_dimensions, dim, list((sub or {}).items()))
            return _calculus.single_roots(*self._solve_batch(dim, row, level, 0))
        return _calculus.merge_pieces("roots", [p.roots(dim, sub, level=float(level[0])) for p in pieces], self.domain[dim])

    def roots(self, dim=None, fixed=None, *, level=0.0) -> np.ndarray:
        """Sorted roots along ``dim`` (reference spline.py:1762-1820): every piece along ``dim`` is solved on its own
        interval, the roots are concatenated in piece order and near-duplicates at the knots (``1e-10 (|domain[dim]| +
        1)``) dropped -- in one device call (the one-row :meth:`roots_batch`) up to 64 nodes per piece.  The end rule of
        :meth:`FibreCalculusMixin.roots <pychebyshev_amd._calculus.FibreCalculusMixin.roots>` holds per piece: a root
        within ``1e-10`` (of the half-width) of an end of its piece's interval, on either side of it, is returned as
        exactly that end, a knot included, and so is a critical point of :meth:`minimize` / :meth:`maximize` (the
        reference clips from outside only).  ``level`` as there; every piece's fibre takes the level."""
        return super().roots(dim, fixed, level=level)

    def minimize(self, dim=None, fixed=None):
        """:meth:`FibreCalculusMixin.minimize <pychebyshev_amd._calculus.FibreCalculusMixin.minimize>` over the pieces
        in order, strictly smaller wins (reference spline.py:1822-1865)."""
        return super().minimize(dim, fixed)

    def maximize(self, dim=None, fixed=None):
        """:meth:`FibreCalculusMixin.maximize <pychebyshev_amd._calculus.FibreCalculusMixin.maximize>` over the pieces
        (reference spline.py:1867-1910)."""
        return super().maximize(dim, fixed)

    def _calculus_rows(self, dim, fixed) -> np.ndarray:
        rows = super()._calculus_rows(dim, fixed)
        if self._dim_counts(int(dim)) is None:
            raise ValueError(f"pieces that share an interval of dimension {dim} differ in their node counts there: "
                             f"the batched solver needs one grid per interval (the single-row calls handle this)")
        return rows

    def roots_batch(self, dim: int, fixed, *, level=None):
        """:meth:`FibreCalculusMixin.roots_batch <pychebyshev_amd._calculus.FibreCalculusMixin.roots_batch>` over the
        pieces (``pcx_spline_calculus_batch``): the fibre points of every piece along ``dim`` go through the spline's own
        evaluation, one launch solves all rows and pieces, a last kernel merges the pieces of a row as :meth:`roots`
        does.  ``roots`` is ``(N, W)`` with ``W`` the sum of ``max(n_j - 1, 1)`` over the pieces along ``dim``; ``counts``
        is -1 where a piece's fibre was not finite or its eigenvalue iteration failed.  At most 64 nodes per piece.
        Every ``(row, piece)`` fibre takes its row's ``level``."""
        return super().roots_batch(dim, fixed, level=level)

    def invert_batch(self, dim: int, fixed, targets):
        """:meth:`FibreCalculusMixin.invert_batch <pychebyshev_amd._calculus.FibreCalculusMixin.invert_batch>` per
        piece: every piece along ``dim`` is solved as its own fibre on its own interval and nodes; ``x`` is the lowest
        over the pieces with ``status > 0`` and ``status`` the sum of the pieces' statuses, so a solution exactly on an
        interior knot is counted by both pieces that find it; a ``-1`` in any piece makes the row ``-1``."""
        return super().invert_batch(dim, fixed, targets)

    def ladder_batch(self, dim: int, fixed, xs, derivative_order=None, *, derivative_id=None, out=None):
        """The spline along ``dim`` at ``m`` values for every row of ``fixed`` (extension; a spot ladder over a kinked
        payoff): ``result[r, x] = eval_batch(point, derivative_order)`` at the point whose coordinate along ``dim`` is the
        row's x-th value and whose other coordinates are ``fixed[r]``, shape ``(N, m)`` -- ``eval_batch``'s rule, not
        ``eval``'s, as in :meth:`eval_grid`: a coordinate on a knot belongs to the right-hand piece, one outside the
        domain to the end piece, a NaN to the last piece, and a derivative spec is not checked against the knots.

        ``fixed``, ``xs``, ``derivative_order`` / ``derivative_id``, ``out`` and device arrays exactly as in
        ``ChebyshevApproximation.ladder_batch``: host ``fixed`` outside its domain raises ``ValueError`` before any
        device call, ``xs`` is never checked, a NaN in ``xs`` gives NaN in its own cell, a NaN in ``fixed`` its row;
        ``m = 0`` returns ``(N, 0)`` without a launch.

        Rows, not points, are routed (``pcx_spline_ladder_batch``): ``fixed[r]`` selects the row's piece index in every
        dimension but ``dim``, the rows are bucketed by that cross-section, every piece of a non-empty cross-section
        whose interval along ``dim`` holds a value of the call contracts its fibres once per row (its own
        ``ladder_batch`` launch at its own nodes), and one kernel interpolates each cell on the fibre of the piece its
        value falls into.  ``result[r, x]`` is bit for bit what that piece's own ``ladder_batch`` gives for the row and
        value, and depends neither on the batch, nor on ``m``, nor on whether ``xs`` is shared.  Pieces that share an
        interval of ``dim`` must have the same node count there."""
        return self._ladder(dim, fixed, xs, out, self._ladder_orders(derivative_order, derivative_id))

    def fibre_batch(self, dim: int, fixed, derivative_order=None, *, derivative_id=None, out=None):
        """Every row's fibres along ``dim``, ``(N, sum_j n_j)``: the fibres of the pieces along ``dim`` in piece order,
        nodes ascending -- the values the calculus batches expand into points, from one contraction per row and piece.
        Type-1 nodes never sit on a knot, so this is :meth:`ladder_batch` at the concatenated nodes, bit for bit (see
        :meth:`FibreCalculusMixin.fibre_batch <pychebyshev_amd._calculus.FibreCalculusMixin.fibre_batch>`)."""
        return super().fibre_batch(dim, fixed, derivative_order, derivative_id=derivative_id, out=out)

    # ---------------------------------------------------------------- extrude / slice
    def _reshaped(self, pieces, domain, knots, n_nodes) -> "ChebyshevSpline":
        """A built spline over other dimensions than this one's: ``function=None``, no device handle yet, the form of
        ``n_nodes`` (flat or nested), ``max_derivative_order`` and the device index kept."""
        obj = self._with_pieces(pieces)
        obj.num_dimensions = len(domain)
        obj.domain = domain
        obj.knots = knots
        obj.n_nodes = n_nodes
        obj._intervals = []
        for (lo, hi), kn in zip(domain, knots):
            edges = [lo] + list(kn) + [hi]
            obj._intervals.append([(edges[i], edges[i + 1]) for i in range(len(edges) - 1)])
        obj._shape = tuple(len(iv) for iv in obj._intervals)
        return obj

    def extrude(self, params) -> "ChebyshevSpline":
        """Add dimensions along which the function is constant (reference spline.py:1391-1473).  ``params`` is one
        ``(dim_index, (lo, hi), n_nodes)`` or a list of them, ``dim_index`` being the position in the result.  Every
        piece is extruded (:meth:`ChebyshevApproximation.extrude`); a new dimension has no knots, one interval, and the
        ``n_nodes`` entry ``[n]`` when the spline's ``n_nodes`` is nested, ``n`` when it is flat."""
        if not self._built:
            raise RuntimeError("Call build() first")
        from .tensor_train import _extrude_params
        sorted_params = _extrude_params(params, self.num_dimensions)
        domain = [list(b) for b in self.domain]
        knots = [list(k) for k in self.knots]
        n_nodes = [list(v) if isinstance(v, list) else v for v in self.n_nodes]
        for dim_idx, (lo, hi), n in sorted_params:
            domain.insert(dim_idx, [lo, hi])
            knots.insert(dim_idx, [])
            n_nodes.insert(dim_idx, [n] if self._n_nodes_nested else n)
        # a new dimension has shape 1: the C order of the pieces stays
        return self._reshaped([piece.extrude(sorted_params) for piece in self._pieces], domain, knots, n_nodes)

    def slice(self, params) -> "ChebyshevSpline":
        """Fix one or more dimensions (reference spline.py:1475-1575): ``params`` is one ``(dim_index, value)`` or a list.
        Along a sliced dimension only the pieces of interval ``min(searchsorted(knots, value, "right"), shape - 1)``
        survive -- a value on a knot belongs to the piece on its right -- and each is sliced on the device
        (:meth:`ChebyshevApproximation.slice`).  Returns a new, lower-dimensional built spline."""
        if not self._built:
            raise RuntimeError("Call build() first")
        from .tensor_train import _slice_params
        sorted_params = sorted(_slice_params(params, self.num_dimensions), key=lambda p: p[0], reverse=True)
        for dim_idx, value in sorted_params:
            lo, hi = self.domain[dim_idx]
            if value < lo or value > hi:
                raise ValueError(f"Slice value {value} for dim {dim_idx} is outside domain [{lo}, {hi}]")
        domain = [list(b) for b in self.domain]
        knots = [list(k) for k in self.knots]
        n_nodes = [list(v) if isinstance(v, list) else v for v in self.n_nodes]
        grid = np.empty(len(self._pieces), dtype=object)
        grid[:] = self._pieces
        grid = grid.reshape(self._shape)
        for dim_idx, value in sorted_params:                       # descending: the lower indices stay valid
            at = min(int(np.searchsorted(knots[dim_idx], value, side="right")), grid.shape[dim_idx] - 1) if knots[dim_idx] else 0
            grid = np.take(grid, at, axis=dim_idx)
            rest = grid.shape
            flat = grid.reshape(-1)
            for i in range(flat.size):
                flat[i] = flat[i].slice((dim_idx, value))
            grid = flat.reshape(rest)
            del domain[dim_idx], knots[dim_idx], n_nodes[dim_idx]
        return self._reshaped(list(grid.reshape(-1)), domain, knots, n_nodes)

    # ---------------------------------------------------------------- integration
    def integrate(self, dims=None, bounds=None):
        """Integrate over ``dims`` (all by default; reference spline.py:1581-1760).  Over all dimensions: the sum
        of the pieces' integrals over their part of ``bounds``, a float.  Otherwise every piece is integrated along
        the dimension (on the device, ``ChebyshevApproximation.integrate``) over its part of the bounds, the pieces
        along that axis are summed, and the result is a lower-dimensional spline.  Bounds that equal a piece's
        interval within 1e-14 integrate the whole piece."""
        from .barycentric import _integration_bounds
        if not self._built:
            raise RuntimeError("Call build() first")
        if dims is None:
            dims = list(range(self.num_dimensions))
        elif isinstance(dims, (int, np.integer)):
            dims = [int(dims)]
        dims = sorted(set(dims))
        for d in dims:
            if d < 0 or d >= self.num_dimensions:
                raise ValueError(f"dim {d} out of range [0, {self.num_dimensions - 1}]")
        per_dim = dict(zip(dims, _integration_bounds(dims, bounds, self.domain)))

        def part(bd, interval):
            """What a piece over ``interval`` integrates of ``bd``: "skip", None (the whole piece) or (lo, hi)."""
            if bd is None:
                return None
            lo, hi = max(bd[0], interval[0]), min(bd[1], interval[1])
            if lo >= hi:
                return "skip"
            if abs(lo - interval[0]) < 1e-14 and abs(hi - interval[1]) < 1e-14:
                return None
            return (lo, hi)

        pieces = np.empty(self._shape, dtype=object)
        for multi, piece in zip(itertools.product(*[range(n) for n in self._shape]), self._pieces):
            pieces[multi] = piece
        if len(dims) == self.num_dimensions:
            total = 0.0
            for multi in np.ndindex(*self._shape):
                parts = [part(per_dim[d], self._intervals[d][multi[d]]) for d in range(self.num_dimensions)]
                if any(isinstance(b, str) for b in parts):
                    continue
                if all(b is None for b in parts):
                    total += pieces[multi].integrate()
                else:
                    total += pieces[multi].integrate(bounds=parts)
            return total

        knots = [list(k) for k in self.knots]
        intervals = [list(iv) for iv in self._intervals]
        domain = [list(b) for b in self.domain]
        for d in sorted(dims, reverse=True):
            rest = tuple(n for i, n in enumerate(pieces.shape) if i != d)
            summed = np.empty(rest, dtype=object)
            for idx in np.ndindex(*rest):
                along = pieces[idx[:d] + (slice(None),) + idx[d:]]
                terms = []
                for i, p in enumerate(along):
                    b = part(per_dim[d], intervals[d][i])
                    if isinstance(b, str):
                        continue
                    terms.append(p.integrate(dims=[d]) if b is None else p.integrate(dims=[d], bounds=[b]))
                if not terms:                       # the bounds reach no piece: a zero piece
                    terms.append(along[0].integrate(dims=[d]) * 0.0)
                acc = terms[0]
                for other in terms[1:]:
                    acc = acc + other
                summed[idx] = acc
            pieces = summed
            del knots[d], intervals[d], domain[d]
        out = ChebyshevSpline.from_pieces(list(pieces.ravel()), self.num_dimensions - len(dims), domain, knots,
                                          max_derivative_order=self.max_derivative_order)
        out._device_index = self._device_index
        return out

    def integrate_batch(self, dims, bounds=None, points=None) -> np.ndarray:
        """Box integrals for a batch of rows (extension; arguments as ``ChebyshevApproximation.integrate_batch``):
        ``out[r]`` is the integral over ``bounds[r]`` in the dimensions ``dims`` at ``points[r]`` in the others.  The
        kept coordinates route a row to one piece index per kept dimension as :meth:`eval_batch` does; every piece
        then takes, in one ``pcx_bary_box_batch`` launch, the rows routed to it whose box overlaps its interval in
        every integrated dimension, with their bounds clipped to it, and the results are added up per row.  A row
        whose box overlaps no piece is 0.  Host arrays only."""
        from ._calculus import box_rows
        if not self._built:
            raise RuntimeError("Call build() first")
        d = self.num_dimensions
        flags, rows = box_rows(d, self.domain, dims, bounds, points)
        N = rows.shape[0]
        out = np.zeros(N)
        if N == 0:
            return out
        self._dev()                      # every piece's device model on the spline's device
        col = np.concatenate([[0], np.cumsum(1 + flags)[:-1]]).astype(int)
        kept = [k for k in range(d) if not flags[k]]
        routed = np.zeros((d, N), dtype=np.int64)
        if kept:
            full = np.empty((N, d))
            for k in range(d):
                full[:, k] = self.domain[k][0] if flags[k] else rows[:, col[k]]
            routed = np.asarray(np.unravel_index(self.piece_indices(full).astype(np.int64), self._shape))
        for multi, piece in zip(itertools.product(*[range(n) for n in self._shape]), self._pieces):
            take = np.ones(N, dtype=bool)
            for k in range(d):
                if flags[k]:
                    lo, hi = self._intervals[k][multi[k]]
                    take &= np.maximum(rows[:, col[k]], lo) < np.minimum(rows[:, col[k] + 1], hi)
                else:
                    take &= routed[k] == multi[k]
            if not take.any():
                continue
            sub = rows[take].copy()
            for k in range(d):
                if flags[k]:
                    lo, hi = self._intervals[k][multi[k]]
                    sub[:, col[k]] = np.maximum(sub[:, col[k]], lo)
                    sub[:, col[k] + 1] = np.minimum(sub[:, col[k] + 1], hi)
            out[take] += piece._box_batch(flags, sub)
        return out

    # ---------------------------------------------------------------- algebra
    # Reference spline.py:1912-2010; the operators are _algebra.ValueAlgebraMixin's: piece by piece on the host
    # (the pieces' own hooks), the result a new spline over the same knots.  The in-place forms rebind every
    # piece's tensor_values, which is how the device copy (_DeviceSpline.matches) sees that it is stale.
    def _check_spline_compatible(self, other) -> None:
        _algebra.check_compatible(self, other)
        if self.knots != other.knots:
            raise ValueError(f"Knot mismatch: {self.knots} vs {other.knots}")

    def _with_pieces(self, pieces) -> "ChebyshevSpline":
        obj = object.__new__(ChebyshevSpline)
        obj.function = None
        obj.num_dimensions = self.num_dimensions
        obj.domain = [list(b) for b in self.domain]
        obj.error_threshold = None
        obj.max_n = self.max_n
        obj.n_workers = None
        obj._n_nodes_nested = self._n_nodes_nested
        obj.n_nodes = [list(v) if isinstance(v, list) else v for v in self.n_nodes]
        obj.knots = [list(k) for k in self.knots]
        obj.max_derivative_order = self.max_derivative_order
        obj.additional_data = None
        obj._derivative_id_registry = {}
        obj._derivative_id_to_orders = []
        obj.descriptor = ""
        obj._intervals = self._intervals
        obj._shape = self._shape
        obj._pieces = pieces
        obj._built = True
        obj._build_time = 0.0
        obj._cached_error_estimate = None
        obj._device_spline = None
        obj._device_index = self._device_index
        return obj

    _check_operand = _check_spline_compatible

    def _leafwise(self, op, other) -> "ChebyshevSpline":
        return self._with_pieces([p._leafwise(op, q) for p, q in zip(self._pieces, _algebra.leaves(other, "_pieces"))])

    def _leafwise_inplace(self, op, other) -> None:
        for p, q in zip(self._pieces, _algebra.leaves(other, "_pieces")):
            p._leafwise_inplace(op, q)
        self._cached_error_estimate = None

    # ---------------------------------------------------------------- properties
    @property
    def num_pieces(self) -> int:
        return int(np.prod(self._shape))

    @property
    def total_build_evals(self) -> int:
        if self._built:
            return sum(int(p.n_evaluations) for p in self._pieces)
        total = 0
        for multi in itertools.product(*[range(s) for s in self._shape]):
            piece_n = self._piece_nodes(multi)
            if any(n is None for n in piece_n):
                return 0
            total += int(np.prod(piece_n))
        return total

    @property
    def build_time(self) -> float:
        return self._build_time

    def is_construction_finished(self) -> bool:
        return self._built

    def get_used_ns(self) -> list:
        return [list(v) if isinstance(v, list) else v for v in self.n_nodes]

    def get_error_threshold(self):
        return self.error_threshold

    def get_num_evaluation_points(self) -> int:
        return int(sum(int(np.prod(p.n_nodes)) for p in self._pieces))

    def get_evaluation_points(self) -> np.ndarray:
        """The pieces' grids, piece after piece (reference spline.py:974-987)."""
        return np.concatenate([p.get_evaluation_points() for p in self._pieces], axis=0)

    def get_special_points(self):
        return [list(k) for k in self.knots]

    # ---------------------------------------------------------------- persistence
    def __getstate__(self) -> dict:
        state = self.__dict__.copy()
        state["function"] = None
        state.pop("_device_spline", None)
        state.pop("_device_index", None)
        state["_pychebyshev_version"] = __version__
        return state

    def __setstate__(self, state: dict) -> None:
        saved = state.pop("_pychebyshev_version", None)
        if saved is not None and saved != __version__:
            warnings.warn(f"This object was saved with pychebyshev {saved}, but you are loading it "
                          f"with {__version__}. Evaluation results may differ if internal data "
                          f"layout changed.", UserWarning, stacklevel=2)
        self.__dict__.update(state)
        self.function = None
        self._device_spline = None
        self._device_index = None

    def save(self, path, format: str = "pickle") -> None:
        if not self._built:
            raise RuntimeError("Cannot save an unbuilt ChebyshevSpline. Call build() first.")
        if format == "pickle":
            with open(path, "wb") as f:
                pickle.dump(self, f, protocol=pickle.HIGHEST_PROTOCOL)
        elif format == "binary":
            from . import _binary
            with open(path, "wb") as f:
                _binary.write_spline(f, self)
        else:
            raise ValueError(f"format must be 'pickle' or 'binary', got {format!r}")

    @classmethod
    def load(cls, path) -> "ChebyshevSpline":
        """Pickle or ``.pcb`` (detected by the magic bytes; reference spline.py:1064-1108)."""
        from . import _binary
        if _binary.detect_format(path) == "binary":
            with open(path, "rb") as f:
                return _binary.read_spline(f)
        with open(path, "rb") as f:
            obj = pickle.load(f)  # noqa: S301 - same trust model as the reference
        if not isinstance(obj, cls):
            raise TypeError(f"Expected a {cls.__name__} instance, got {type(obj).__name__}")
        return obj

    def error_estimate(self) -> float:
        """Largest per-piece estimate: a point lies in exactly one piece (reference spline.py:702-733)."""
        if not self._built:
            raise RuntimeError("Call build() before error_estimate().")
        if self._cached_error_estimate is None:
            self._cached_error_estimate = max(p.error_estimate() for p in self._pieces)
        return self._cached_error_estimate

    def __str__(self) -> str:
        """Multi-line summary in the reference's layout (spline.py:2013-2074)."""
        shown = 6
        if self.num_dimensions > shown:
            nodes_txt = "[" + ", ".join(str(n) for n in self.n_nodes[:shown]) + ", ...]"
            knots_txt = "[" + ", ".join(str(k) for k in self.knots[:shown]) + ", ...]"
            dom_txt = " x ".join(f"[{lo}, {hi}]" for lo, hi in self.domain[:shown]) + " x ..."
        else:
            nodes_txt, knots_txt = str(self.n_nodes), str(self.knots)
            dom_txt = " x ".join(f"[{lo}, {hi}]" for lo, hi in self.domain)
        out = [f"ChebyshevSpline ({self.num_dimensions}D, {'built' if self._built else 'not built'})",
               f"  Nodes:       {nodes_txt} per piece",
               f"  Knots:       {knots_txt}",
               f"  Pieces:      {self.num_pieces} ({' x '.join(str(n) for n in self._shape)})"]
        if self._built:
            out.append(f"  Build:       {self._build_time:.3f}s ({self.total_build_evals:,} function evals)")
        out.append(f"  Domain:      {dom_txt}")
        if self._built:
            out.append(f"  Error est:   {self.error_estimate():.2e}")
        return "\n".join(out)

    def __repr__(self) -> str:
        return (f"ChebyshevSpline(dims={self.num_dimensions}, pieces={self.num_pieces}, "
                f"shape={self._shape}, built={self._built})")
