"""``ChebyshevSlider`` -- additive "sliding" decomposition around a pivot point: a sum of
low-dimensional barycentric interpolants, each evaluated on an MI355X.

Host-side mirror of the reference class (``/root/reference/src/pychebyshev/slider.py``,
v0.21.1) for the evaluation path:

    __init__ / build (one ChebyshevApproximation per partition group)   (:80-199)
    eval / eval_multi   f(x) ~ f(z) + sum_i [ s_i(x_i) - f(z) ]          (:247-341)
    get_derivative_id, total_build_evals, pickle, repr

``eval_batch`` / ``eval_multi_batch`` are extensions (the reference has no batch method):
``pcx_slider_eval_multi_batch`` uploads the points once, every slide evaluates its column
group of the whole batch in one device launch and a last kernel adds the slide results in
the reference's order.

``+``, ``-``, ``*`` and ``/`` combine the slides' value tensors and the pivot value on the host.

    extrude / slice                                                       (:621-875)
    integrate(dims, bounds)   scalar, or a slider over the kept dimensions  (:881-1136)
    roots / minimize / maximize(dim, fixed)                               (:1178-1283)

``roots_batch`` / ``minimize_batch`` / ``maximize_batch`` and ``integrate_batch`` are extensions.  Along one
dimension only the slide that owns it varies, so ``pcx_slider_calculus_batch`` evaluates every other slide once per
row and the owner once per fibre point (not at all when the owner is one-dimensional: its value tensor is the fibre),
adds them in ``eval``'s order and solves every fibre on the device; the single calls are one-row batches up to 64
nodes and the host restatement of ``_calculus`` above.  ``pcx_slider_box_batch`` sums the slides' own per-row box
integrals scaled by the row's box widths.

``eval_grid`` (extension) evaluates a tensor-product grid as a broadcast sum: every slide evaluates the small grid of
its own group of dimensions (``d_s`` mode products) and ``k_slider_grid_sum`` writes ``pivot + sum_s (G_s - pivot)`` over
the whole grid in one pass, in ``eval``'s order of operations (``pcx_slider_eval_tensor_grid``); a derivative inside one
slide is that slide's grid broadcast, one across slides is ``+0.0``.

Out of scope in this tier: plotting.
"""
from __future__ import annotations

import ctypes
import pickle
import time
import warnings
from typing import Callable, List, Sequence, Tuple

import numpy as np

from . import _algebra, _calculus, _lib
from ._algebra import ValueAlgebraMixin
from ._calculus import FibreCalculusMixin
from ._version import __version__
from ._derivative_ids import DerivativeIdMixin
from ._ergonomics import ErgonomicsMixin
from .barycentric import ChebyshevApproximation, _integration_bounds

__all__ = ["ChebyshevSlider"]


def _partition_intersect(group, integrate_dims):
    """The reference's ``_slider_partition_intersect``: a slide group against the integrated dimensions -> ``"full"``
    (every dimension integrated), ``"partial"`` or ``"none"``, and the group's dimensions that are kept."""
    overlap = set(group) & set(integrate_dims)
    if not overlap:
        return "none", list(group)
    if overlap == set(group):
        return "full", []
    return "partial", [d for d in group if d not in overlap]


class _DeviceSlider:
    """Owner of one ``pcx_slider`` handle; keeps the slides' device models alive."""

    def __init__(self, slider: "ChebyshevSlider", device: int):
        lib = _lib.load()
        self.models = []
        for slide in slider.slides:
            slide._device_index = device
            self.models.append(slide._model())
        sizes = _lib.i32([len(g) for g in slider.partition])
        dims = _lib.i32([d for g in slider.partition for d in g])
        arr = (ctypes.c_void_p * len(self.models))(*[m.handle for m in self.models])
        handle = ctypes.c_void_p()
        _lib.check(lib.pcx_slider_create(device, slider.num_dimensions, len(self.models),
                                         ctypes.cast(arr, _lib.c_vpp), _lib.p_i32(sizes), _lib.p_i32(dims),
                                         float(slider.pivot_value), ctypes.byref(handle)), lib)
        self.lib = lib
        self.handle = handle
        self.device = device
        self.tensors = [s.tensor_values for s in slider.slides]      # the arrays themselves, not their ids
        self.pivot_value = float(slider.pivot_value)

    def matches(self, slider: "ChebyshevSlider") -> bool:
        return (len(self.tensors) == len(slider.slides) and self.pivot_value == float(slider.pivot_value)
                and all(a is s.tensor_values for a, s in zip(self.tensors, slider.slides)))

    def __del__(self):
        try:
            if self.handle:
                self.lib.pcx_slider_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class ChebyshevSlider(ErgonomicsMixin, DerivativeIdMixin, FibreCalculusMixin, ValueAlgebraMixin):
    """Sum of low-dimensional slides around ``pivot_point`` (signature: reference slider.py:80-90)."""

    def __init__(self, function: Callable, num_dimensions: int,
                 domain: Sequence[Tuple[float, float]], n_nodes: Sequence[int],
                 partition: Sequence[Sequence[int]], pivot_point: Sequence[float],
                 max_derivative_order: int = 2, additional_data: object = None):
        from . import Domain, Ns
        if isinstance(domain, Domain):
            domain = list(domain.bounds)
        if isinstance(n_nodes, Ns):
            n_nodes = list(n_nodes.counts)
        self.function = function
        self.num_dimensions = num_dimensions
        self.domain = domain
        self.n_nodes = n_nodes
        self.partition = partition
        self.pivot_point = list(pivot_point)
        self.max_derivative_order = max_derivative_order
        self.descriptor = ""
        self.additional_data = additional_data
        covered = sorted(d for group in partition for d in group)
        if covered != list(range(num_dimensions)):
            raise ValueError(f"Partition must cover all dimensions 0..{num_dimensions - 1} "
                             f"exactly once. Got dimensions: {covered}")
        self._dim_to_slide = {d: i for i, group in enumerate(partition) for d in group}
        self.slides: List[ChebyshevApproximation] = []
        self.pivot_value = 0.0
        self._built = False
        self._cached_error_estimate = None
        self._derivative_id_registry: dict = {}
        self._derivative_id_to_orders: list = []
        self._device_slider = None
        self._device_index = None

    # ---------------------------------------------------------------- device plumbing
    def to_device(self, device: int | None = None) -> "ChebyshevSlider":
        if not self._built:
            raise RuntimeError("Call build() first")
        dev = _lib.default_device() if device is None else int(device)
        self._device_index = dev
        self._device_slider = _DeviceSlider(self, dev)
        return self

    def _dev(self) -> _DeviceSlider:
        s = self.__dict__.get("_device_slider")
        if s is None or not s.matches(self):
            self.to_device(self.__dict__.get("_device_index"))
            s = self._device_slider
        return s

    # ---------------------------------------------------------------- build
    def build(self, verbose: bool | int = True) -> None:
        """Build every slide with the other coordinates frozen at the pivot
        (reference slider.py:128-199)."""
        start = time.time()
        self._cached_error_estimate = None
        self.pivot_value = self.function(self.pivot_point, self.additional_data)
        if verbose:
            print(f"Building {self.num_dimensions}D Chebyshev Slider ({len(self.partition)} slides, "
                  f"{self.total_build_evals:,} evaluations vs {int(np.prod(self.n_nodes)):,} for full tensor)...")
        self.slides = []
        for idx, group in enumerate(self.partition):
            def restricted(sub_point, data, _group=tuple(group), _pivot=tuple(self.pivot_point)):
                full = list(_pivot)
                for local, dim in enumerate(_group):
                    full[dim] = sub_point[local]
                return self.function(full, data)

            slide = ChebyshevApproximation(restricted, len(group), [self.domain[d] for d in group],
                                           [self.n_nodes[d] for d in group],
                                           max_derivative_order=self.max_derivative_order,
                                           additional_data=self.additional_data)
            slide.build(verbose=False)
            self.slides.append(slide)
            if verbose:
                print(f"  Slide {idx + 1}/{len(self.partition)}: dims {group}, "
                      f"{int(np.prod(slide.n_nodes)):,} evals")
        if verbose:
            print(f"Build complete in {time.time() - start:.3f}s")
        self._built = True

    # ---------------------------------------------------------------- evaluation
    def _active_slides(self, derivative_order):
        return {self._dim_to_slide[d] for d, o in enumerate(derivative_order) if o > 0}

    def eval(self, point, derivative_order=None, *, derivative_id=None) -> float:
        """Reference slider.py:247-318 (Ruiz & Zeron eq. 7.5); a derivative involves only the
        slide that owns the differentiated dimensions, cross-slide mixed partials are 0."""
        if not self._built:
            raise RuntimeError("Call build() before eval().")
        derivative_order = self._resolve_derivative_args(derivative_order, derivative_id)
        active = self._active_slides(derivative_order)
        if active:
            if len(active) > 1:
                return 0.0
            idx = active.pop()
            group = self.partition[idx]
            return self.slides[idx].vectorized_eval([point[d] for d in group],
                                                    [derivative_order[d] for d in group])
        result = self.pivot_value
        for idx, group in enumerate(self.partition):
            val = self.slides[idx].vectorized_eval([point[d] for d in group], [0] * len(group))
            result += val - self.pivot_value
        return result

    def eval_multi(self, point, derivative_orders) -> List[float]:
        """Reference slider.py:320-341: one ``eval`` per spec."""
        return [self.eval(point, spec) for spec in derivative_orders]

    def eval_batch(self, points, derivative_order=None, *, derivative_id=None) -> np.ndarray:
        """Batched :meth:`eval` (extension): points uploaded once, one launch per slide, summed on the device."""
        if not self._built:
            raise RuntimeError("Call build() before eval_batch().")
        derivative_order = self._resolve_derivative_args(derivative_order, derivative_id)
        out = self.eval_multi_batch(points, [list(derivative_order)])
        if isinstance(out, np.ndarray):
            return out[:, 0]
        out.shape = (out.shape[0],)           # (N, 1) device result: same memory as (N,)
        return out

    def eval_multi_batch(self, points, derivative_orders) -> np.ndarray:
        """``(N, d)`` points x ``m`` specs -> ``(N, m)`` (extension); value specs share the slides' values."""
        if not self._built:
            raise RuntimeError("Call build() before eval_multi_batch().")
        specs = _lib.i32(np.asarray(derivative_orders).reshape(-1, self.num_dimensions))
        from .device import DeviceArray, as_device_array, check_points
        dev_pts = as_device_array(points)
        if dev_pts is not None:           # device-resident batch: the result stays in HBM
            s = self._dev()
            n = check_points(dev_pts, self.num_dimensions, s.device)
            dout = DeviceArray.empty((n, specs.shape[0]), s.device)
            if n:
                _lib.check(s.lib.pcx_slider_eval_multi_batch_dev(s.handle, ctypes.c_void_p(dev_pts.ptr), n, _lib.p_i32(specs),
                                                                 specs.shape[0], ctypes.c_void_p(dout.ptr)), s.lib)
            return dout
        pts = _lib.f64(points)
        if pts.ndim != 2 or pts.shape[1] != self.num_dimensions:
            raise ValueError(f"points must have shape (N, {self.num_dimensions}), got {pts.shape}")
        s = self._dev()
        out = np.empty((pts.shape[0], specs.shape[0]))
        _lib.check(s.lib.pcx_slider_eval_multi_batch(s.handle, _lib.p_f64(pts), pts.shape[0], _lib.p_i32(specs),
                                                     specs.shape[0], _lib.p_f64(out)), s.lib)
        return out

    def eval_grid(self, axes, derivative_order=None, *, derivative_id=None, out=None):
        """The slider on the tensor-product grid ``axes[0] x ... x axes[d-1]`` (extension; what the reference's
        ``plot_2d_surface`` and a risk ladder over a high-dimensional book evaluate point by point):
        ``result[i_0, ..., i_{d-1}] = eval([axes[0][i_0], ...], derivative_order)``, shape ``(m_0, ..., m_{d-1})``.

        ``axes``, ``derivative_order`` / ``derivative_id`` and ``out`` as in ``ChebyshevApproximation.eval_grid``.
        Every slide depends on its own group of dimensions only: each evaluates the small grid of its group and one
        kernel writes ``pivot + sum_s (G_s - pivot)``, slides in order, over the whole grid
        (``pcx_slider_eval_tensor_grid``).  A derivative inside one slide is that slide's derivative grid, broadcast
        over the other dimensions; one that spans two slides or more is ``+0.0`` everywhere."""
        from .barycentric import _composite_eval_grid
        return _composite_eval_grid(self, "pcx_slider_eval_tensor_grid", axes, derivative_order, derivative_id, out)

    # ---------------------------------------------------------------- algebra
    # Reference slider.py:1285-1390; the operators are _algebra.ValueAlgebraMixin's: slide by slide on the host
    # (the slides' own hooks), pivot_value combined the same way.  The in-place forms rebind every slide's
    # tensor_values and pivot_value, which is how the device copy (_DeviceSlider.matches) sees that it is stale.
    def _check_slider_compatible(self, other) -> None:
        _algebra.check_compatible(self, other)
        if self.partition != other.partition:
            raise ValueError(f"Partition mismatch: {self.partition} vs {other.partition}")
        if self.pivot_point != other.pivot_point:
            raise ValueError(f"Pivot point mismatch: {self.pivot_point} vs {other.pivot_point}")

    def _with_slides(self, slides, pivot_value) -> "ChebyshevSlider":
        obj = object.__new__(ChebyshevSlider)
        obj.function = None
        obj.num_dimensions = self.num_dimensions
        obj.domain = [list(b) for b in self.domain]
        obj.n_nodes = list(self.n_nodes)
        obj.partition = [list(g) for g in self.partition]
        obj.pivot_point = list(self.pivot_point)
        obj.max_derivative_order = self.max_derivative_order
        obj.descriptor = ""
        obj.additional_data = None
        obj._dim_to_slide = self._dim_to_slide
        obj.slides = slides
        obj.pivot_value = pivot_value
        obj._built = True
        obj._cached_error_estimate = None
        obj._derivative_id_registry = {}
        obj._derivative_id_to_orders = []
        obj._device_slider = None
        obj._device_index = self.__dict__.get("_device_index")
        return obj

    _check_operand = _check_slider_compatible

    def _leafwise(self, op, other) -> "ChebyshevSlider":
        return self._with_slides([s._leafwise(op, t) for s, t in zip(self.slides, _algebra.leaves(other, "slides"))],
                                 op(self.pivot_value, getattr(other, "pivot_value", other)))

    def _leafwise_inplace(self, op, other) -> None:
        for s, t in zip(self.slides, _algebra.leaves(other, "slides")):
            s._leafwise_inplace(op, t)
        self.pivot_value = op(self.pivot_value, getattr(other, "pivot_value", other))
        self._cached_error_estimate = None

    # ---------------------------------------------------------------- extrude / slice
    def _assembled(self, num_dimensions, domain, n_nodes, partition, pivot_point, slides, pivot_value) -> "ChebyshevSlider":
        """A built slider over other dimensions than this one's (``function=None``, no device handle yet)."""
        obj = self._with_slides(slides, pivot_value)
        obj.num_dimensions = num_dimensions
        obj.domain = domain
        obj.n_nodes = n_nodes
        obj.partition = partition
        obj.pivot_point = pivot_point
        obj._dim_to_slide = {d: i for i, group in enumerate(partition) for d in group}
        return obj

    def extrude(self, params) -> "ChebyshevSlider":
        """Add dimensions along which the function is constant (reference slider.py:621-739).  ``params`` is one
        ``(dim_index, (lo, hi), n_nodes)`` or a list of them, ``dim_index`` being the position in the result.  Each
        new dimension is a one-dimensional slide of its own whose tensor is ``np.full(n, pivot_value)`` -- it adds
        ``s(x) - pivot_value = 0`` to the sum -- appended to the partition; the existing groups are renumbered and
        the new pivot coordinate is the midpoint."""
        if not self._built:
            raise RuntimeError("Call build() first")
        from .tensor_train import _extrude_params
        sorted_params = _extrude_params(params, self.num_dimensions)
        domain = [list(b) for b in self.domain]
        n_nodes = list(self.n_nodes)
        pivot_point = list(self.pivot_point)
        partition = [list(g) for g in self.partition]
        slides = list(self.slides)
        for dim_idx, (lo, hi), n in sorted_params:
            partition = [[d + 1 if d >= dim_idx else d for d in group] for group in partition]
            slide = ChebyshevApproximation.from_values(np.full(n, self.pivot_value), 1, [[lo, hi]], [n],
                                                       max_derivative_order=self.max_derivative_order)
            slide._device_index = self.__dict__.get("_device_index")
            partition.append([dim_idx])
            slides.append(slide)
            domain.insert(dim_idx, [lo, hi])
            n_nodes.insert(dim_idx, n)
            pivot_point.insert(dim_idx, 0.5 * (lo + hi))
        return self._assembled(self.num_dimensions + len(sorted_params), domain, n_nodes, partition, pivot_point,
                               slides, self.pivot_value)

    def slice(self, params) -> "ChebyshevSlider":
        """Fix one or more dimensions (reference slider.py:741-875): ``params`` is one ``(dim_index, value)`` or a
        list.  A dimension of a multi-dimension group is sliced out of its slide (``ChebyshevApproximation.slice``); a
        one-dimension group is evaluated to ``s_val``, ``delta = s_val - pivot_value`` goes into every remaining
        slide's tensor, ``pivot_value`` becomes ``s_val`` and the group is dropped.  Indices are renumbered."""
        if not self._built:
            raise RuntimeError("Call build() first")
        from .tensor_train import _slice_params
        sorted_params = sorted(_slice_params(params, self.num_dimensions), key=lambda p: p[0], reverse=True)
        for dim_idx, value in sorted_params:
            lo, hi = self.domain[dim_idx]
            if value < lo or value > hi:
                raise ValueError(f"Slice value {value} for dim {dim_idx} is outside domain [{lo}, {hi}]")
        domain = [list(b) for b in self.domain]
        n_nodes = list(self.n_nodes)
        pivot_point = list(self.pivot_point)
        partition = [list(g) for g in self.partition]
        slides = list(self.slides)
        pivot_value = self.pivot_value
        for dim_idx, value in sorted_params:                       # descending
            slide_idx = next(i for i, group in enumerate(partition) if dim_idx in group)
            if len(partition[slide_idx]) > 1:
                slides[slide_idx] = slides[slide_idx].slice((partition[slide_idx].index(dim_idx), value))
                partition[slide_idx].remove(dim_idx)
            else:
                s_val = slides[slide_idx].vectorized_eval([value], [0])
                delta = s_val - pivot_value
                slides = [s._combined(s.tensor_values + delta) for i, s in enumerate(slides) if i != slide_idx]
                pivot_value = s_val
                del partition[slide_idx]
            partition = [[d - 1 if d > dim_idx else d for d in group] for group in partition]
            del domain[dim_idx]
            del n_nodes[dim_idx]
            del pivot_point[dim_idx]
        return self._assembled(self.num_dimensions - len(sorted_params), domain, n_nodes, partition, pivot_point,
                               slides, pivot_value)

    # ---------------------------------------------------------------- integration
    def integrate(self, dims=None, bounds=None):
        """Integrate over ``dims`` (all by default; ``bounds``: one ``(lo, hi)`` or ``None`` per integrated dimension)
        by the closed form of the sliding sum (reference slider.py:881-1136).  A slide whose group is integrated in
        full goes into the new pivot value ``pv' = pv vol_T + sum vol(T \\ G_i) (I_i - pv vol(G_i))``; every other
        slide keeps its surviving dimensions with the tensor ``scale . source + (pv' - pv vol_T)``, ``source`` its own
        partial integral (scale ``vol(T \\ G_i)``) or, where none of its dimensions is integrated, its tensor (scale
        ``vol_T``).  Returns a float when no dimension is left, else a slider over the surviving dimensions."""
        if not self._built:
            raise RuntimeError("Call build() first")
        if dims is None:
            dims_sorted = list(range(self.num_dimensions))
        elif isinstance(dims, (int, np.integer)):
            dims_sorted = [int(dims)]
        else:
            dims_sorted = sorted(set(dims))
        for d in dims_sorted:
            if d < 0 or d >= self.num_dimensions:
                raise ValueError(f"dim {d} out-of-range [0, {self.num_dimensions - 1}]")
        bounds_for_dim = dict(zip(dims_sorted, _integration_bounds(dims_sorted, bounds, self.domain)))
        widths = {d: (self.domain[d][1] - self.domain[d][0]) if bd is None else bd[1] - bd[0]
                  for d, bd in bounds_for_dim.items()}
        vol_T = 1.0
        for d in dims_sorted:
            vol_T *= widths[d]

        def vol_outside(group):
            v = 1.0
            for d in dims_sorted:
                if d not in group:
                    v *= widths[d]
            return v

        def slide_integral(slide, group):
            local = [(i, bounds_for_dim[g]) for i, g in enumerate(group) if g in bounds_for_dim]
            local_dims, local_bounds = [i for i, _ in local], [b for _, b in local]
            if all(b is None for b in local_bounds):
                return slide.integrate(dims=local_dims)
            return slide.integrate(dims=local_dims, bounds=local_bounds)

        kinds = [_partition_intersect(group, dims_sorted) for group in self.partition]
        pv_new = self.pivot_value * vol_T
        for slide, group, (kind, _) in zip(self.slides, self.partition, kinds):
            if kind != "full":
                continue
            I_i = float(slide_integral(slide, group))
            vol_group = 1.0
            for d in group:
                vol_group *= widths[d]
            pv_new += vol_outside(group) * (I_i - self.pivot_value * vol_group)
        if len(dims_sorted) == self.num_dimensions:
            return float(pv_new)

        survive = [d for d in range(self.num_dimensions) if d not in bounds_for_dim]
        old_to_new = {old: new for new, old in enumerate(survive)}
        shift = pv_new - self.pivot_value * vol_T
        new_partition, new_slides = [], []
        for slide, group, (kind, kept) in zip(self.slides, self.partition, kinds):
            if kind == "full":
                continue
            if kind == "none":
                new_slides.append(slide._combined(vol_T * slide.tensor_values + shift))
            else:
                reduced = slide_integral(slide, group)
                new_slides.append(reduced._combined(vol_outside(group) * reduced.tensor_values + shift))
            new_partition.append([old_to_new[d] for d in kept])
        obj = self._assembled(len(survive), [list(self.domain[d]) for d in survive], [self.n_nodes[d] for d in survive],
                              new_partition, [self.pivot_point[d] for d in survive], new_slides, pv_new)
        obj.descriptor = self.descriptor
        obj.additional_data = self.additional_data
        return obj

    def integrate_batch(self, dims, bounds=None, points=None) -> np.ndarray:
        """Box integrals for a batch of rows (extension; the reference computes one with ``integrate(dims, bounds)``
        and then ``eval(point)``).  Arguments and the ``(N,)`` result as
        :meth:`ChebyshevApproximation.integrate_batch`.  On the device every slide takes its own box integral of the
        row and a last kernel sums them scaled by the row's box widths (``pcx_slider_box_batch``).  Host arrays only."""
        if not self._built:
            raise RuntimeError("Call build() first")
        flags, rows = _calculus.box_rows(self.num_dimensions, self.domain, dims, bounds, points)
        rows = _lib.f64(rows)
        out = np.empty(rows.shape[0])
        if rows.shape[0]:
            s = self._dev()
            lo, hi = self._domain_arrays()
            _lib.check(s.lib.pcx_slider_box_batch(s.handle, _lib.p_i32(_lib.i32(flags)), _lib.p_f64(lo), _lib.p_f64(hi),
                                                  _lib.p_f64(rows), rows.shape[0], _lib.p_f64(out)), s.lib)
        return out

    # ---------------------------------------------------------------- calculus
    # _calculus.FibreCalculusMixin's methods over these hooks; below, what this class adds to their docstrings.
    _fibre_prefix = "pcx_slider"

    def _owner_grid(self, dim: int):
        """Nodes, weights and differentiation matrix of ``dim``: those of the slide that owns it."""
        idx = self._dim_to_slide[dim]
        local = list(self.partition[idx]).index(dim)
        slide = self.slides[idx]
        return slide.nodes[local], slide.weights[local], slide.diff_matrices[local]

    def _fibre_grid(self, dim: int):
        return (*self._owner_grid(dim), (self.domain[dim][0], self.domain[dim][1]))

    def _fibre_values(self, points) -> np.ndarray:
        return self.eval_batch(points, [0] * self.num_dimensions)

    def roots(self, dim=None, fixed=None, *, level=0.0) -> np.ndarray:
        """:meth:`FibreCalculusMixin.roots <pychebyshev_amd._calculus.FibreCalculusMixin.roots>`, ``level`` included
        (reference slider.py:1178-1224, which slices to one dimension and re-interpolates at the nodes): here the fibre
        is formed and solved on the device."""
        return super().roots(dim, fixed, level=level)

    def minimize(self, dim=None, fixed=None):
        """:meth:`FibreCalculusMixin.minimize <pychebyshev_amd._calculus.FibreCalculusMixin.minimize>` (reference
        slider.py:1226-1264)."""
        return super().minimize(dim, fixed)

    def maximize(self, dim=None, fixed=None):
        """:meth:`FibreCalculusMixin.maximize <pychebyshev_amd._calculus.FibreCalculusMixin.maximize>` (reference
        slider.py:1266-1283)."""
        return super().maximize(dim, fixed)

    def ladder_batch(self, dim: int, fixed, xs, derivative_order=None, *, derivative_id=None, out=None):
        """The slider along ``dim`` at ``m`` values for every row of ``fixed`` (extension; a spot or vol ladder over a
        wide book): ``result[r, x] = eval(point, derivative_order)`` at the point whose coordinate along ``dim`` is the
        row's x-th value and whose other coordinates are ``fixed[r]``, shape ``(N, m)``.

        ``fixed``, ``xs``, ``derivative_order`` / ``derivative_id``, ``out`` and device arrays exactly as in
        ``ChebyshevApproximation.ladder_batch``: host ``fixed`` outside its domain raises ``ValueError`` before any
        device call, ``xs`` is never checked, a NaN in ``xs`` gives NaN in its own cell; ``m = 0`` returns ``(N, 0)``
        without a launch.

        Only the slide that owns ``dim`` varies along a ladder (``pcx_slider_ladder_batch``): it runs its own
        ``ladder_batch`` launch, one contraction per row; every other slide is evaluated once per row, not ``m`` times,
        and one kernel forms ``pivot + sum_s (v_s - pivot)``, slides in order, so the result is bit for bit the host
        composition of the slides' own ``ladder_batch`` / ``vectorized_eval_batch`` results.  A NaN in ``fixed`` makes
        its row NaN.  Derivatives follow :meth:`eval`: a spec inside the owner slide is the owner's derivative ladder
        alone (a NaN among the other slides' coordinates then does not show); one inside another slide is that slide's
        derivative at the row, at every value (``xs`` is then not read: a NaN there does not show); one that spans two
        slides or more is ``+0.0`` everywhere."""
        return self._ladder(dim, fixed, xs, out, self._ladder_orders(derivative_order, derivative_id))

    def fibre_batch(self, dim: int, fixed, derivative_order=None, *, derivative_id=None, out=None):
        """:meth:`FibreCalculusMixin.fibre_batch <pychebyshev_amd._calculus.FibreCalculusMixin.fibre_batch>` at the
        nodes of the slide that owns ``dim``."""
        return super().fibre_batch(dim, fixed, derivative_order, derivative_id=derivative_id, out=out)

    # ---------------------------------------------------------------- misc
    @property
    def total_build_evals(self) -> int:
        return sum(int(np.prod([self.n_nodes[d] for d in group])) for group in self.partition)

    def is_construction_finished(self) -> bool:
        return self._built

    def get_used_ns(self) -> list:
        return list(self.n_nodes)

    def get_num_evaluation_points(self) -> int:
        return int(self.total_build_evals)

    def get_evaluation_points(self) -> np.ndarray:
        """Every slide's grid embedded at the pivot in the other dimensions, slide after slide
        (reference slider.py:479-500)."""
        pivot = np.array(self.pivot_point, dtype=np.float64)
        rows = []
        for slide, group in zip(self.slides, self.partition):
            grid = slide.get_evaluation_points()
            full = np.tile(pivot, (len(grid), 1))
            full[:, list(group)] = grid
            rows.append(full)
        return np.concatenate(rows, axis=0)

    def error_estimate(self) -> float:
        """Sum of the slides' estimates: every slide contributes at every point (reference :343-350)."""
        if not self._built:
            raise RuntimeError("Call build() before error_estimate().")
        if self._cached_error_estimate is None:
            self._cached_error_estimate = sum(s.error_estimate() for s in self.slides)
        return self._cached_error_estimate

    def __getstate__(self) -> dict:
        state = self.__dict__.copy()
        state["function"] = None
        state["_device_slider"] = None
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

    def save(self, path) -> None:
        if not self._built:
            raise RuntimeError("Cannot save an unbuilt ChebyshevSlider. Call build() first.")
        with open(path, "wb") as f:
            pickle.dump(self, f, protocol=pickle.HIGHEST_PROTOCOL)

    @classmethod
    def load(cls, path) -> "ChebyshevSlider":
        with open(path, "rb") as f:
            obj = pickle.load(f)  # noqa: S301 - same trust model as the reference
        if not isinstance(obj, cls):
            raise TypeError(f"Expected a {cls.__name__} instance, got {type(obj).__name__}")
        return obj

    def __repr__(self) -> str:
        return (f"ChebyshevSlider(dims={self.num_dimensions}, slides={len(self.partition)}, "
                f"partition={self.partition}, built={self._built})")
