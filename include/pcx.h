/*
 * pcx.h -- C ABI of libpcx_hip.so: MI355X (gfx950) batched evaluation of Chebyshev
 * interpolants, the drop-in for PyChebyshev's evaluation hot path.
 *
 * The reference (PyChebyshev v0.21.1) is pure Python/NumPy and has NO FFI seam; the
 * seam is its Python class surface.  Each entry point below therefore names the
 * reference *method* (file:line under /root/reference/src/pychebyshev/) whose work it
 * replaces.  The Python classes in pychebyshev_amd/ are the only intended callers;
 * INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++/torch types cross the boundary.
 *   - return 0 (PCX_OK) or a negative PCX_ERR_* code; never throws: every entry point catches what its C++ body may
 *     raise (std::bad_alloc -> PCX_ERR_NOMEM, anything else -> PCX_ERR_HIP; csrc/pcx_internal.h, PCX_API_BEGIN / _END).
 *     pcx_last_error() returns a thread-local description of the last failure on the calling thread.
 *   - all floating point is IEEE float64; tensors are C-order (last index fastest);
 *     `pts` is an (N, d) row-major array, exactly the ndarray the reference takes.
 *   - the library copies model data at create; callers keep ownership of every buffer
 *     they pass.  Handles are immutable after create except for an internal cache of
 *     derivative-transformed tensors (mutex-protected); one handle may be used from
 *     several host threads.
 *   - one handle lives on ONE device (one process per GPU; shard batches across
 *     processes/handles -- the path has no cross-device exchange).
 *   - "_dev" variants take DEVICE pointers and only enqueue work on the given HIP
 *     stream (NULL = the handle's own stream); they do not synchronize.
 */
#ifndef PCX_H
#define PCX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCX_ABI_VERSION 1

#define PCX_OK 0
#define PCX_ERR_INVALID (-1)     /* bad argument (shape, NULL, range)               */
#define PCX_ERR_NO_DEVICE (-2)   /* no usable HIP device / device index out of range */
#define PCX_ERR_HIP (-3)         /* a HIP runtime call failed                        */
#define PCX_ERR_UNSUPPORTED (-4) /* valid request outside what the kernels cover     */
#define PCX_ERR_NOMEM (-5)
#define PCX_ERR_INTERNAL (-6)    /* a self-check of the library failed (diagnostic entry points) */

#define PCX_MAX_DIMS 16

typedef struct pcx_bary pcx_bary; /* device-resident ChebyshevApproximation state */
typedef struct pcx_tt pcx_tt;     /* device-resident ChebyshevTT coefficient cores */
typedef struct pcx_spline pcx_spline; /* knots + piece handles of a ChebyshevSpline   */
typedef struct pcx_slider pcx_slider; /* partition + slide handles of a ChebyshevSlider */

/* ---- library / device ------------------------------------------------------ */
int pcx_abi_version(void);
const char *pcx_last_error(void);
int pcx_device_count(int *n);
int pcx_device_info(int device, char *name, int name_len, int *compute_units, int64_t *hbm_bytes);
/* PCI bus id of the device ("0000:05:00.0"): lets a multi-rank run prove that its ranks sat on distinct GPUs */
int pcx_device_pci_bus_id(int device, char *buf, int len);

/* Device-memory plumbing for callers that keep query batches resident in HBM
 * (bench.py, multi-GPU drivers).  `stream` arguments are hipStream_t passed as void*. */
int pcx_dev_malloc(int device, size_t bytes, void **dptr);
int pcx_dev_free(int device, void *dptr);
/* The device a pointer lives on (hipPointerGetAttributes); PCX_ERR_INVALID for host or
 * unknown memory.  Lets a host that received a device array from another library
 * (`__cuda_array_interface__`) check it before handing it to a `_dev` entry point.    */
int pcx_pointer_device(const void *ptr, int *device);
int pcx_memcpy_h2d(int device, void *dst, const void *src, size_t bytes);
int pcx_memcpy_d2h(int device, void *dst, const void *src, size_t bytes);
int pcx_device_synchronize(int device);
int pcx_event_create(int device, void **event);
int pcx_event_record(void *event, void *stream);
int pcx_event_elapsed_ms(void *start, void *stop, float *ms); /* synchronizes on `stop` */
int pcx_event_destroy(void *event);
/* Streams and asynchronous copies for drivers that overlap the gather / download of one
 * step with the kernel of the next (bench.py, pychebyshev_amd/distributed.py).  A stream
 * belongs to the device it was created on.  pcx_host_register pins an existing host range
 * (e.g. a POSIX shared-memory result buffer every rank downloads its block into) so that
 * device-to-host copies into it run at full PCIe rate and asynchronously.               */
int pcx_stream_create(int device, void **stream);
int pcx_stream_destroy(void *stream);
int pcx_stream_synchronize(void *stream);
int pcx_stream_wait_event(void *stream, void *event);
int pcx_memcpy_h2d_async(void *dst, const void *src, size_t bytes, void *stream);
int pcx_memcpy_d2h_async(void *dst, const void *src, size_t bytes, void *stream);
int pcx_host_register(int device, void *ptr, size_t bytes);
int pcx_host_unregister(void *ptr);

/* ---- barycentric full-tensor interpolant ----------------------------------- */
/* State of ChebyshevApproximation (barycentric.py:401-414): per-dimension nodes,
 * barycentric weights and differentiation matrices (concatenated: sum n_d, sum n_d,
 * sum n_d^2 doubles, each D_d row-major) and tensor_values (prod n_d doubles, C-order).
 * Built by the host exactly as barycentric.py:440-452, :30-49, :52-77 do.            */
int pcx_bary_create(int device, int d, const int32_t *n_nodes, const double *nodes_cat,
                    const double *weights_cat, const double *diffmat_cat, const double *tensor,
                    pcx_bary **out);
int pcx_bary_destroy(pcx_bary *h);

/* Load a ChebyshevApproximation from a .pcb v1 file (reference _binary.py:208-283;
 * examples/binary_reader/reader.c there is the reference's C reader) straight into a
 * device handle.  Nodes / weights / differentiation matrices are rebuilt on the host
 * with the formulas of barycentric.py:440-452, :30-49, :52-77.  For C/C++ callers.    */
int pcx_bary_create_from_pcb(int device, const char *path, pcx_bary **out);
/* The write side of the same format (_binary.py:208-283): header, d, domain bounds, n_nodes
 * and the untransformed tensor (copied back from the device), little-endian, byte-identical
 * to what the reference writes for the same model.  lo / hi (d doubles each) give the domain;
 * both may be NULL for a handle that came from pcx_bary_create_from_pcb (it remembers its own). */
int pcx_bary_save_pcb(pcx_bary *h, const char *path, const double *lo, const double *hi);
/* Shape of a handle: d (may be NULL) and n_nodes (PCX_MAX_DIMS ints, may be NULL).   */
int pcx_bary_shape(pcx_bary *h, int32_t *d_out, int32_t *n_nodes_out);

/* vectorized_eval_batch (barycentric.py:992-1047): _apply_derivative_passes
 * (:951-990) once for `deriv` (d orders, NULL = all zero; cached per handle), then per
 * point the exact-node test |x - node| < 1e-14 / (T . w/diff) / sum(w/diff) reduction
 * over all dimensions.  Host-pointer form: copies pts in, result out, synchronizes.   */
int pcx_bary_eval_batch(pcx_bary *h, const double *pts, int64_t N, const int32_t *deriv,
                        double *out);
int pcx_bary_eval_batch_dev(pcx_bary *h, const double *d_pts, int64_t N, const int32_t *deriv,
                            double *d_out, void *stream);

/* vectorized_eval_multi (barycentric.py:1049-1112) batched over points: m derivative
 * specs (m x d orders) at each of N points; out is (N, m) row-major.                  */
int pcx_bary_eval_multi_batch(pcx_bary *h, const double *pts, int64_t N, const int32_t *derivs,
                              int m, double *out);
/* The same over SEVERAL handles of one process (the same model created on several devices -- the
 * "devices[] list" of a drop-in create): handle g evaluates the contiguous row
 * block [g ceil(N/G), ...) on its own device from its own host thread, every download lands in its slice of
 * `out`; no collective.  The blocks run concurrently only over PAGE-LOCKED arrays: pin != 0 registers the caller's
 * arrays for the call (arrays the caller has page-locked itself -- pcx_host_register -- are taken as they are);
 * with pin = 0 and pageable arrays, or when the registration fails, the whole batch goes through handles[0]
 * (several host threads never copy to or from one pageable allocation; PCX_FANOUT_LOG=1 reports the fallback).
 * Prefer pin = 0 over arrays registered ONCE (pcx_host_register, for the arrays' lifetime): a heap range registered and
 * released per call has ended later calls over the same addresses in a GPU memory access fault; the
 * Python layer passes pin = 0 unless asked (to_device(devices=..., pin=True)).
 * Replaces the reference's single-process vectorized_eval_batch (barycentric.py:992) when the process sees more
 * than one GPU.                                                                                              */
int pcx_bary_group_eval_multi_batch(pcx_bary *const *handles, int n_handles, const double *pts, int64_t N,
                                    const int32_t *derivs, int m, double *out, int pin);
/* Device-resident form: d_pts (N x d) and d_out (N x m) in HBM; enqueues on `stream`
 * (NULL = the handle's own) and returns without synchronizing.                         */
int pcx_bary_eval_multi_batch_dev(pcx_bary *h, const double *d_pts, int64_t N,
                                  const int32_t *derivs, int m, double *d_out, void *stream);

/* The derivative-transformed tensor of _apply_derivative_passes (:951-990), copied to
 * the host (prod n_d doubles) -- lets tests check kernel K3 on its own.               */
int pcx_bary_derivative_tensor(pcx_bary *h, const int32_t *deriv, double *tensor_out);

/* Chebyshev coefficient tensor of the handle's values (reference _sensitivity.py:14-49: per
 * dimension reverse, DCT-II, / n, halve c_0), C order, prod n_d doubles: d mode products
 * on the device.                                                                        */
int pcx_bary_chebyshev_coefficients(pcx_bary *h, double *coeffs_out);

/* First- and total-order Sobol indices and the variance of the handle's interpolant
 * (reference _sensitivity.py:67-140), including its rules: d = 1 -> both indices 1.0 when
 * variance > 0; variance == 0 -> all indices 0.0; any non-finite coefficient ->
 * PCX_ERR_INVALID with "coefficients contain NaN or Inf" in pcx_last_error().
 * first_out and total_out hold d doubles each.                                           */
int pcx_bary_sobol(pcx_bary *h, double *variance_out, double *first_out, double *total_out);

/* Contract axis `axis` of a C-order tensor (d dims, n_nodes) with `vec` (n_nodes[axis]
 * doubles): out has the remaining d-1 dims.  The device half of
 * ChebyshevApproximation.slice (barycentric.py:2064-2154, _extrude_slice.py:79-92).   */
int pcx_tensor_contract_axis(int device, int d, const int32_t *n_nodes, const double *tensor,
                             int axis, const double *vec, double *out);

/* Rectangular mode product of host arrays, the companion of pcx_tensor_contract_axis and the pass of a tensor-product
 * grid evaluation:   Y[o, j, q] = sum_i W[j, i] * X[o, i, q],   o < outer, i < n, j < m, q < inner   (C order, FP64).
 * variant: 0 = auto, 1 = any-shape VALU form (one fma chain per output, i ascending), 2 = v_mfma_f64_16x16x4_f64 form
 * (the same chain per output: both forms agree bit for bit, whatever the tile an output falls in).  Any other variant:
 * PCX_ERR_INVALID; more than 2^40 elements in X or Y: PCX_ERR_UNSUPPORTED.  A row of W that is one-hot (a single 1.0,
 * zeros elsewhere) is a gather of X, not a sum: identical on finite data, and it keeps a NaN or Inf elsewhere in the
 * fibre out of that output.                                                                                        */
int pcx_tensor_mode_product(int device, int64_t outer, int n, int64_t inner, const double *X, int m, const double *W,
                            double *Y, int variant);

/* The interpolant (or its derivative `deriv`, NULL = plain values) on the tensor-product grid x_0 x ... x x_{d-1}:
 * out[i_0, ..., i_{d-1}] (C order, prod m_k doubles) = the value at (x_0[i_0], ..., x_{d-1}[i_{d-1}]).  m holds the d
 * axis lengths (each >= 1: an empty axis is PCX_ERR_INVALID), axes_cat the sum m_k coordinates, dimension 0 first,
 * always on the HOST.  Axes may be unsorted, repeat values and leave the domain; they are not checked.
 *   Weights: per axis the m_k x n_k matrix W_k of the reference's pointwise rule (barycentric.py:941-947): a
 *     coordinate within 1e-14 of a node gives a one-hot row at the FIRST such node (a gather of the tensor, bit for
 *     bit); otherwise (w_i / (x - node_i)) / sum_i (w_i / (x - node_i)).
 *   Order: d mode products of the handle's derivative tensor, dimensions by ascending m_k / n_k (compared exactly as
 *     m_a n_b < m_b n_a in 64-bit integers; ties: the higher dimension first), so the intermediates stay small; they
 *     ping-pong between two scratch buffers of the handle and the last pass writes the result.
 * Parity with pointwise evaluation (pcx_bary_eval_batch on the meshgrid: 1e-12 normwise) holds for FINITE tensors: the
 * two routes sum in different orders and spread a NaN or Inf differently.  Every allocation precedes the first launch.
 * The _dev form writes d_out in HBM, enqueues on `stream` (NULL = the handle's own) and returns without synchronizing. */
int pcx_bary_eval_tensor_grid(pcx_bary *h, const int32_t *deriv, const int32_t *m, const double *axes_cat, double *out);
int pcx_bary_eval_tensor_grid_dev(pcx_bary *h, const int32_t *deriv, const int32_t *m, const double *axes_cat,
                                  double *d_out, void *stream);

/* Kernel selection and introspection.  variant: 0 = auto, 1 = row-parallel VALU kernel
 * (any shape), 2 = MFMA kernel (v_mfma_f64_16x16x4_f64), 3 = the same contraction on
 * v_mfma_f64_4x4x4_4b_f64 with LDS-staged tiles (bit-identical to 2; opt-in, never picked
 * by auto), 5 = lane-per-point kernel for mid-size tensors whose last two dimensions have the same node count
 * (4 .. 24 or 32; d <= 4: both trailing weight vectors in registers, what auto picks there above 4096 elements),
 * 4 = lane-per-point kernel for small tensors (d <= 4, last dimension <= 64 nodes;
 * what auto picks up to 4096 elements; it sums in the reference's own nesting order and
 * forms the barycentric weights from prefix / suffix products, one division per dimension).
 * PCX_ERR_UNSUPPORTED when the shape is not covered.  info_out receives
 * {variant used by auto, row tiles, k-steps, lds bytes, points per workgroup, split}.  */
int pcx_bary_set_kernel(pcx_bary *h, int variant);
/* Multi-spec batches (pcx_bary_eval_multi_batch[_dev], N >= 65,536 on the MFMA kernel): a spec and the spec ONE order
 * below it along any one dimension q (n_q <= 16) may share ONE contraction of the other dimensions, finished with D_q
 * on the per-node partial sums -- the order of operations of the reference's vectorized_eval_multi
 * (barycentric.py:1098-1110).  That rounds differently from the reference's batch path (which differentiates the
 * tensor first) by a data-dependent amount, so every candidate pair is MEASURED once per handle: a probe batch of
 * 2,048 points (domain corners, edges, interior) goes through the shared launch and through the spec's own GEMM, and
 * the pair is formed only when the two agree to `tol` of the batch's scale -- default 3e-13 (PCX_BARY_GROUP_TOL), a
 * factor of three inside the 1e-12 parity bar.  5-D Black-Scholes: delta out of the price tensor 1e-13 and gamma out
 * of the delta tensor 1e-13 (shared), vega 7e-13, dV/dT 1e-12, rho 1e-12 (own GEMMs unless tol is raised).
 * q > 0 runs on a copy of the model with q in front, built on first use (tensors up to 2^24 elements; launches on
 * the handle's own streams only).  PCX_BARY_PROBE_LOG=1 prints every measurement.
 * pcx_bary_set_group_span: 1 = the above (default; PCX_BARY_G0_SPAN overrides it at load); 2 first lets specs up to
 * two dim-0 orders apart share without a probe (price / delta / gamma in one GEMM: gamma then 4e-12 from the
 * reference's batch path); 0: every spec its own GEMM.
 * pcx_bary_count_gemms: the number of GEMM launches a call with these specs and N would execute.                 */
int pcx_bary_count_gemms(pcx_bary *h, const int32_t *derivs, int m, int64_t N, int32_t *gemms_out);
int pcx_bary_set_group_tolerance(pcx_bary *h, double tol);
int pcx_bary_set_group_span(pcx_bary *h, int span);
int pcx_bary_kernel_info(pcx_bary *h, int32_t *info_out /* 6 ints; [2] = k-steps of the MFMA plan, not counting seeded columns */);
/* Short MFMA plans (3-D tensors of 17 .. 65 nodes, 64^4: spline pieces, auto-N builds) lay their row tiles over the last two
 * head dimensions instead of taking 16 consecutive rows, so the head weights need no row codes (k_bary_mfma_grid).
 * info_out: {1 when the handle's MFMA plan is of that kind else 0, rows of the first tiled dimension per tile (1, 2, 4),
 * row tiles, chunks}.  PCX_BARY_GRID=0 in the environment keeps every handle on the row-code form.
 * 3-D tensors one of whose dimensions fills row tiles well (25 .. 32, 44 .. 48, 59 .. 64 nodes, or whatever prices ahead of the
 * grid plan by the measured rule of DESIGN.md 3.1f) keep that dimension in the accumulators and fold the other two into K
 * with the B operand formed per k-step (k_bary_mfma_kfold): info_out = {2, 0, row tiles, k-steps per index of the loop
 * dimension}.  PCX_BARY_KFOLD=0 switches
 * that form off. */
int pcx_bary_grid_info(pcx_bary *h, int32_t *info_out /* 4 ints */);
/* The row-code MFMA form's launch geometry for large batches: [0] workgroups the device holds at once, [1] points per
 * workgroup, [2] chunks of row tiles, [3] whether a launch whose last round of workgroups is at most half full splits
 * that round over the idle ones (1: where the row-tile walk is long enough to pay for the finishing kernel, the default;
 * PCX_BARY_TAIL=0 at create: 0, never; =2: 2, wherever the geometry allows), [4] workgroups per tail block in the latest such
 * launch (0: it kept one workgroup per block), [5] its tail blocks.  All zero when launches take another form. */
int pcx_bary_tail_info(pcx_bary *h, int32_t *info_out /* 6 ints */);
int pcx_bary_stream(pcx_bary *h, void **stream);
/* Box integrals, batched (the reference's integrate(dims, bounds) then vectorized_eval(point), one row per call there):
 * out[r] = integral of the interpolant over [lo, hi] in every integrated dimension of row r, at the row's coordinates in
 * the kept ones.  flags = d entries (0 kept, 1 integrated; anything else is PCX_ERR_INVALID); lo / hi = the model's domain,
 * d each (a handle does not know it; lo < hi, else PCX_ERR_INVALID).  rows is N x (d + m) row-major, m = number of flags
 * set: for dimensions 0 .. d-1 in order one double (the coordinate) for a kept dimension, two (lo, hi) for an integrated
 * one.  m = 0 is the value.  A kept coordinate within 1e-14 of a node takes that node's slice, as an evaluation does; an
 * integrated dimension takes the sub-interval Fejer-1 weights of its (lo, hi), and a row with lo == hi gives exactly 0.
 * Rows are not checked against the domain.  N = 0 returns PCX_OK without a launch.  One launch per piece of the batch and
 * one workgroup per block of rows: a result does not depend on the batch size.  Handles whose fragment image is the
 * row-code packing run v_mfma_f64_16x16x4_f64 on that image (k_bary_box_mfma); every other handle, a handle whose
 * evaluation prefers a lane-per-point kernel while no variant is set, and every handle after pcx_bary_set_kernel(h, 1)
 * run the any-shape form on the plain tensor (k_bary_box_rows).  The _dev form takes device
 * rows and results and queues on `stream` (NULL: the handle's); it returns without waiting. */
int pcx_bary_box_batch(pcx_bary *h, const int32_t *flags, const double *lo, const double *hi, const double *rows,
                       int64_t N, double *out);
int pcx_bary_box_batch_dev(pcx_bary *h, const int32_t *flags, const double *lo, const double *hi, const double *d_rows,
                           int64_t N, double *d_out, void *stream);
/* The form a box call takes now: [0] 1 = MFMA form, 0 = rows form; [1] k-steps per row tile; [2] seed columns R;
 * [3] 1 = wide codes (more than four head or tail dimensions).  [1] .. [3] are 0 for the rows form. */
int pcx_bary_box_info(pcx_bary *h, int32_t *info_out /* 4 ints */);
/* Ladders, batched: out[r * m + x] = the interpolant (its derivative `deriv`: d orders as pcx_bary_eval_batch takes them,
 * NULL = the values) at the point whose coordinate along `dim` is the x-th value of row r and whose other coordinates
 * are fixed[r * (d - 1) + ...], the dimensions but dim in increasing order.  xs_per_row = 0: the m values of xs are shared
 * by all rows; 1: xs is N x m.  The row's fibre F[j] = sum over the other dimensions of T . (their normalised barycentric
 * weights, the one-hot rule within 1e-14 of a node included) is formed once, on the spec's derived tensor, and the
 * ladder is its 1-D barycentric interpolant: a value within 1e-14 of a node of dim returns F at that node itself, so
 * xs = the nodes of dim gives the fibre.  Neither fixed nor xs is checked against a domain; a NaN in fixed makes the row
 * NaN, a NaN in xs its own cell.  A NULL handle or pointer, dim outside [0, d), m < 0, N < 0, xs_per_row outside {0, 1}
 * and a derivative order outside [0, 8] are PCX_ERR_INVALID before any launch; N = 0 or m = 0 returns PCX_OK after these
 * checks without a launch.  Handles with at least two dimensions, at most 64 nodes along dim and tables within 64 KB
 * of LDS run v_mfma_f64_16x16x4_f64 on an image of the tensor with dim innermost, packed on the first call per
 * (deriv, dim) and kept with the derived tensor (k_bary_ladder_mfma); every other handle, and every handle after
 * pcx_bary_set_kernel(h, 1), runs the any-shape form on the plain tensor (k_bary_ladder_rows).  One workgroup per block
 * of rows: a row's result depends neither on the batch nor on m.  The host form stages d - 1 (+ m when xs is per row,
 * at least 1) doubles per row in passes of max(1, 2^20 / max(that width, m)) rows through the driver the evaluation
 * entries share.  The _dev form takes device rows, device xs when they are per row (HOST xs when shared: it then
 * returns after its kernel has finished) and device results, and queues on `stream` (NULL: the handle's). */
int pcx_bary_ladder_batch(pcx_bary *h, int dim, const int32_t *deriv, const double *fixed, int64_t N, const double *xs,
                          int m, int xs_per_row, double *out);
int pcx_bary_ladder_batch_dev(pcx_bary *h, int dim, const int32_t *deriv, const double *d_fixed, int64_t N,
                              const double *xs, int m, int xs_per_row, double *d_out, void *stream);
/* The form a ladder along dim takes now: [0] 1 = MFMA form, 0 = rows form; [1] k-steps per block of 16 rows; [2] column
 * tiles of 16 fibre nodes.  [1] and [2] are 0 for the rows form. */
int pcx_bary_ladder_info(pcx_bary *h, int dim, int32_t *info_out /* 3 ints */);

/* ---- piecewise (spline) interpolant ---------------------------------------- */
/* ChebyshevSpline (spline.py:35-700): per-dimension sorted interior knots (concatenated)
 * and one pcx_bary handle per piece in C order over the per-dimension intervals
 * (n_pieces = prod(n_knots[k] + 1)).  The spline handle BORROWS the piece handles: they
 * must outlive it and live on the same device.                                        */
int pcx_spline_create(int device, int d, const int32_t *n_knots, const double *knots_cat,
                      pcx_bary *const *pieces, int n_pieces, pcx_spline **out);
int pcx_spline_destroy(pcx_spline *h);
/* eval_batch (spline.py:633-700): piece = searchsorted(knots, x, side='right') clipped,
 * points bucketed per piece on the device, one barycentric launch per non-empty piece. */
int pcx_spline_eval_batch(pcx_spline *h, const double *pts, int64_t N, const int32_t *deriv,
                          double *out);
int pcx_spline_eval_multi_batch(pcx_spline *h, const double *pts, int64_t N, const int32_t *derivs,
                                int m, double *out);
/* The piece index of every point (spline.py:414-446, _find_piece) -- for tests/tools.  */
int pcx_spline_piece_ids(pcx_spline *h, const double *pts, int64_t N, int32_t *ids_out);
/* Device-resident points (N x d) and results (N, or N x m) on the handle's device.  Routing needs
 * the per-piece counts on the host, so these calls are synchronous: all work is done on return;
 * m <= 64. */
int pcx_spline_eval_batch_dev(pcx_spline *h, const double *d_pts, int64_t N, const int32_t *deriv,
                              double *d_out);
int pcx_spline_eval_multi_batch_dev(pcx_spline *h, const double *d_pts, int64_t N,
                                    const int32_t *derivs, int m, double *d_out);
/* The piecewise interpolant (or its derivative `deriv`, NULL = plain values) on the tensor-product grid
 * x_0 x ... x x_{d-1}: out[i_0, ..., i_{d-1}] (C order, prod m_k doubles) = pcx_spline_eval_batch at
 * (x_0[i_0], ..., x_{d-1}[i_{d-1}]).  m, axes_cat (always on the HOST) and their errors as for pcx_bary_eval_tensor_grid:
 * an empty axis is PCX_ERR_INVALID and names the dimension, more than 2^40 grid points are PCX_ERR_UNSUPPORTED, a NULL
 * handle or buffer is PCX_ERR_INVALID.  Axes may be unsorted, repeat values and leave the domain.
 *   Routing: per dimension, the interval of a coordinate is the number of knots <= it (searchsorted side='right', clipped
 *     to the last piece): a coordinate on a knot belongs to the right-hand piece, one outside the domain to the end piece,
 *     which extrapolates, a NaN to the last piece.  There is no knot check for derivative specs (eval_batch has none).
 *   Evaluation: a piece is live when every dimension has an axis entry in its interval.  Every live piece runs
 *     pcx_bary_eval_tensor_grid_dev on the entries of its intervals (ascending position) into its block of a packed
 *     staging buffer -- bit for bit what the piece's own grid evaluation returns --, on the stream or round-robin on the
 *     handle's side streams, without a host synchronization in between; one kernel then copies every element from its
 *     block to its place.  With a single live piece the piece writes the result itself.
 * Every allocation of the handle precedes its first launch of the call.  The _dev form writes d_out in HBM, enqueues on
 * `stream` (NULL = the handle's own) and returns without synchronizing.                                                */
int pcx_spline_eval_tensor_grid(pcx_spline *h, const int32_t *deriv, const int32_t *m, const double *axes_cat, double *out);
int pcx_spline_eval_tensor_grid_dev(pcx_spline *h, const int32_t *deriv, const int32_t *m, const double *axes_cat,
                                    double *d_out, void *stream);
/* Ladders, batched: out[r * m + x] = pcx_spline_eval_batch (spec `deriv`, NULL = the values) at the point whose
 * coordinate along `dim` is the x-th value of row r and whose other coordinates are fixed[r * (d - 1) + ...].  Arguments,
 * checks (a NULL handle or pointer, dim outside [0, d), m < 0, N < 0, xs_per_row outside {0, 1}, an order outside [0, 8]:
 * PCX_ERR_INVALID before any launch; N = 0 or m = 0: PCX_OK after them) and host staging as pcx_bary_ladder_batch.
 *   Routing: pcx_spline_eval_tensor_grid's rule per dimension (knots <= x counted, clipped; a knot belongs to the
 *     right-hand piece, outside the domain to the end piece, NaN to the last piece; no knot check for derivative specs).
 *     fixed[r] selects the row's cross-section (the piece index in every dimension but dim), each value the index along dim.
 *   Evaluation: rows are bucketed by cross-section; every piece (non-empty cross-section, live index j along dim) runs its
 *     own ladder (pcx_bary_ladder_batch_dev's launch) on the bucket's rows at its own nodes along dim, which gives the
 *     bucket's fibres; one kernel then interpolates every cell on the fibre of the piece its value falls into, by the dense
 *     ladder's 1-D rule: out[r * m + x] is bit for bit what that piece's own ladder gives for the row and value.  An index
 *     along dim is live when a value of the call falls into it (found on the host; with device per-row xs all are live).
 *     Pieces that share an index along dim must share the node count there (else PCX_ERR_INVALID); more than 65535 pieces
 *     along dim are PCX_ERR_UNSUPPORTED.  Rows go in chunks of 2^21 / (sum of the live node counts along dim).
 * The _dev form takes device rows, device xs when they are per row (HOST xs when shared) and device results; the work
 * runs on the handle's stream and side streams and is complete on return (`stream` may be NULL and is not used). */
int pcx_spline_ladder_batch(pcx_spline *h, int dim, const int32_t *deriv, const double *fixed, int64_t N, const double *xs,
                            int m, int xs_per_row, double *out);
int pcx_spline_ladder_batch_dev(pcx_spline *h, int dim, const int32_t *deriv, const double *d_fixed, int64_t N,
                                const double *xs, int m, int xs_per_row, double *d_out, void *stream);

/* ---- slider: sum of low-dimensional slides around a pivot -------------------- */
/* State of ChebyshevSlider (slider.py:80-341): the slides are barycentric handles over the
 * dimension groups of `partition` (group_sizes[s] entries of group_dims_cat each, every
 * dimension exactly once), pivot_value = f(pivot_point).  The slides are BORROWED: they must
 * outlive the slider handle.  Evaluation (slider.py:247-318, eq. 7.5 of Ruiz & Zeron):
 *   value:       pivot + sum_s (slide_s(x_group_s) - pivot), summed in slide order;
 *   derivative:  all differentiated dimensions in one slide -> that slide's derivative;
 *                spread over more than one slide -> 0.
 * The reference evaluates one point per call; these evaluate N points with one launch per
 * slide (plus a column gather and the sum), points uploaded once for all m specs. */
int pcx_slider_create(int device, int d, int n_slides, pcx_bary *const *slides,
                      const int32_t *group_sizes, const int32_t *group_dims_cat,
                      double pivot_value, pcx_slider **out);
int pcx_slider_destroy(pcx_slider *h);
int pcx_slider_eval_batch(pcx_slider *h, const double *pts, int64_t N, const int32_t *deriv,
                          double *out);
int pcx_slider_eval_multi_batch(pcx_slider *h, const double *pts, int64_t N,
                                const int32_t *derivs, int m, double *out /* N x m */);
/* Device-resident points and results; synchronous on return. */
int pcx_slider_eval_multi_batch_dev(pcx_slider *h, const double *d_pts, int64_t N,
                                    const int32_t *derivs, int m, double *d_out);
/* Box integrals, batched (the reference's integrate(dims, bounds) then eval(point), slider.py:881-1136, one row per call
 * there).  flags, lo / hi (the slider's domain, d each) and the N x (d + m) rows are those of pcx_bary_box_batch over the
 * slider's dimensions: the column of dimension u is u + the number of flags set below u; m = 0 is the value.  Per slide a
 * gather writes the slide's own box row, pcx_bary_box_batch_dev on the slider's stream gives its box integral I_i (its
 * value where none of its dimensions is integrated), and a last kernel forms, slides in partition order,
 *     out = pv vol_T + sum_i vol(T \ G_i) (I_i - pv vol(T n G_i)),
 * vol(S) the product of the row's hi - lo over the integrated dimensions in S (1 for none).  Volumes are products, never
 * quotients: a row with lo == hi in an integrated dimension gives exactly 0.  Rows are not checked against the domain.
 * N = 0 returns PCX_OK without a launch.  The _dev form takes device rows and results and is synchronous on return. */
int pcx_slider_box_batch(pcx_slider *h, const int32_t *flags, const double *lo, const double *hi, const double *rows,
                         int64_t N, double *out);
int pcx_slider_box_batch_dev(pcx_slider *h, const int32_t *flags, const double *lo, const double *hi, const double *d_rows,
                             int64_t N, double *d_out);
/* The slider (or its derivative `deriv`, NULL = plain values) on the tensor-product grid x_0 x ... x x_{d-1}:
 * out[i_0, ..., i_{d-1}] (C order, prod m_k doubles) = pcx_slider_eval_batch at (x_0[i_0], ..., x_{d-1}[i_{d-1}]).  m,
 * axes_cat (always on the HOST) and the errors as for pcx_spline_eval_tensor_grid.
 *   value:       every slide runs pcx_bary_eval_tensor_grid_dev on the axes of its own group (the group's order) into the
 *                handle's scratch, G_s; one kernel writes r = pivot; r += G_s[i restricted to group s] - pivot, slides in
 *                order -- the operations of pcx_slider_eval_batch in their order, G_s broadcast over the other dimensions;
 *   derivative:  all differentiated dimensions in one slide -> that slide's derivative grid, broadcast by the same kernel
 *                (no pivot terms); spread over more than one slide -> +0.0 everywhere (a memset).
 * Every allocation of the handle precedes its first launch of the call.  The _dev form writes d_out in HBM, enqueues on
 * `stream` (NULL = the handle's own) and returns without synchronizing.                                                */
int pcx_slider_eval_tensor_grid(pcx_slider *h, const int32_t *deriv, const int32_t *m, const double *axes_cat, double *out);
int pcx_slider_eval_tensor_grid_dev(pcx_slider *h, const int32_t *deriv, const int32_t *m, const double *axes_cat,
                                    double *d_out, void *stream);
/* Ladders, batched: out[r * m + x] = pcx_slider_eval_batch (spec `deriv`, NULL = the values) at the point whose coordinate
 * along `dim` is the x-th value of row r and whose other coordinates are fixed[r * (d - 1) + ...].  Arguments, checks and
 * host staging as pcx_spline_ladder_batch.
 *   value:       every slide but the owner of dim is evaluated once per row; the owner runs its own ladder
 *                (pcx_bary_ladder_batch_dev's launch) along dim's place in its group, at the row's coordinates of the
 *                group's other dimensions, into the result, and one kernel forms r = pivot; r += v_s - pivot, slides in
 *                order, in place.  A one-dimensional owner with shared xs runs its ladder for ONE row (its fibre is its
 *                tensor: the same m values for every row) and the kernel broadcasts it.
 *   derivative:  inside the owner -> the owner's derivative ladder alone; inside another slide -> that slide's derivative
 *                at the row, at every value (xs is not read); spread over more than one slide -> +0.0 everywhere.
 * Rows go in chunks of 2^21 / m.  The _dev form as pcx_spline_ladder_batch_dev: on the handle's stream, complete on return. */
int pcx_slider_ladder_batch(pcx_slider *h, int dim, const int32_t *deriv, const double *fixed, int64_t N, const double *xs,
                            int m, int xs_per_row, double *out);
int pcx_slider_ladder_batch_dev(pcx_slider *h, int dim, const int32_t *deriv, const double *d_fixed, int64_t N,
                                const double *xs, int m, int xs_per_row, double *d_out, void *stream);

/* ---- tensor-train interpolant ---------------------------------------------- */
/* State of ChebyshevTT (tensor_train.py:1117-1138): Chebyshev COEFFICIENT cores
 * (r_{k-1}, n_k, r_k) C-order concatenated, ranks (d+1, ranks[0]=ranks[d]=1), domain,
 * and dim_order (storage position k reads user column dim_order[k]; NULL = identity). */
int pcx_tt_create(int device, int d, const int32_t *n_nodes, const int32_t *ranks,
                  const double *lo, const double *hi, const double *coeff_cores_cat,
                  const int32_t *dim_order, pcx_tt **out);
int pcx_tt_destroy(pcx_tt *h);

/* eval_batch (tensor_train.py:2217-2265): per storage dim scale to [-1,1], Chebyshev
 * polynomials T_0..T_{n-1}, contract with the core, chain-multiply.                   */
int pcx_tt_eval_batch(pcx_tt *h, const double *pts, int64_t N, double *out);
/* eval_batch fanned out over several handles (one per device), as pcx_bary_group_eval_multi_batch
 * (reference entry point: tensor_train.py:2217).                                            */
int pcx_tt_group_eval_batch(pcx_tt *const *handles, int n_handles, const double *pts, int64_t N, double *out, int pin);
int pcx_tt_eval_batch_dev(pcx_tt *h, const double *d_pts, int64_t N, double *d_out, void *stream);
/* eval_multi batched (tensor_train.py:2267-2463; the reference evaluates one point per call): value and central
 * finite-difference derivatives, out[p * m + s] for spec s.  derivs = m x d orders (0, 1 or 2; anything else is
 * PCX_ERR_INVALID, "... not supported ...") in the USER's dimension order.  The reference's rules in its order of
 * operations: h = (b - a) 1e-4, the coordinate nudged so that 1.5 h stays inside the domain, 2-point / 3-point rules
 * nested over the differenced dimensions, the 4-point rule for a mixed (1, 1) partial.  Every stencil point is formed
 * and evaluated on the device (for lane-per-point models in registers: no stencil batch in HBM); a spec with more
 * than three differenced dimensions is PCX_ERR_UNSUPPORTED.  Row p equals the per-point stencil evaluated through
 * pcx_tt_eval_batch bit for bit. */
int pcx_tt_eval_multi_batch(pcx_tt *h, const double *pts, int64_t N, const int32_t *derivs, int m, double *out);
int pcx_tt_eval_multi_batch_dev(pcx_tt *h, const double *d_pts, int64_t N, const int32_t *derivs, int m, double *d_out,
                                void *stream);
int pcx_tt_stream(pcx_tt *h, void **stream);
/* Box integrals, batched (the reference's integrate(dims, bounds) then eval(point), tensor_train.py:1505-1702, one row
 * per call there): out[r] = integral of the model over [lo, hi] in every integrated dimension of row r, at the row's
 * coordinates in the kept ones.  integrated = d flags (0 or 1; anything else is PCX_ERR_INVALID) in the USER's dimension
 * order.  rows is N x (d + m) row-major, m = number of flags set: for user dimensions 0 .. d-1 in order one double (the
 * coordinate) for a kept dimension, two (lo, hi) for an integrated one.  m = 0 is the value, as pcx_tt_eval_batch.  A row
 * with lo == hi gives exactly 0.  The domain is not checked.  N = 0 returns PCX_OK without a launch.  Models with a
 * lane-per-point image (ranks <= 16, n <= 16) run one row per lane, every other model one row per wave on the plain
 * cores. */
int pcx_tt_box_batch(pcx_tt *h, const int32_t *integrated, const double *rows, int64_t N, double *out);
int pcx_tt_box_batch_dev(pcx_tt *h, const int32_t *integrated, const double *d_rows, int64_t N, double *d_out,
                         void *stream);
/* Ladders, batched, as pcx_bary_ladder_batch[_dev] without a derivative spec: out[r * m + x] = the model at the point
 * whose coordinate along `dim` (the USER's dimension order, as the columns of fixed) is the x-th value of row r.  The
 * row's left and right chains and the n Chebyshev coefficients of its restriction to dim are formed once; each value is
 * then that series by the evaluation's recurrence.  Arguments, checks and staging as there.  Models with a lane-per-point
 * image (ranks <= 16, n <= 16) run one row per lane, every other model one row per wave on the plain cores. */
int pcx_tt_ladder_batch(pcx_tt *h, int dim, const double *fixed, int64_t N, const double *xs, int m, int xs_per_row,
                        double *out);
int pcx_tt_ladder_batch_dev(pcx_tt *h, int dim, const double *d_fixed, int64_t N, const double *xs, int m, int xs_per_row,
                            double *d_out, void *stream);
/* Analytic derivatives, batched: out[p * m + s] = the partial derivative of the interpolant with the orders of spec s at
 * point p.  Arguments as pcx_tt_eval_multi_batch[_dev]: derivs = m x d orders (0, 1 or 2; anything else is
 * PCX_ERR_INVALID, "... not supported ...") in the USER's dimension order, out is N x m.  One chain per (point, spec)
 * with T_j, T'_j or T''_j (times (2 / (b - a))^order) as the basis of a dimension: no stencil, no truncation error, any
 * number of differentiated dimensions; an order that reaches a dimension's node count gives exactly 0.  N = 0 or m = 0
 * returns PCX_OK without a launch (after the argument checks).  More than 64 specs are split over launches.  Models with
 * a lane-per-point image (ranks <= 16, n <= 16) run one point per lane, every other model one point per wave on the
 * plain cores. */
int pcx_tt_deriv_batch(pcx_tt *h, const double *pts, int64_t N, const int32_t *derivs, int m, double *out);
int pcx_tt_deriv_batch_dev(pcx_tt *h, const double *d_pts, int64_t N, const int32_t *derivs, int m, double *d_out,
                           void *stream);
/* Value, gradient and Hessian diagonal, batched, in one forward-backward pass per point: out is N x C row-major with
 * C = 1 + d (second = 0) or 1 + 2 d (second = 1); column 0 is the value, column 1 + u the first and column 1 + d + u the
 * second partial derivative along dimension u of the USER's dimension order.  One right sweep keeps every right partial
 * product, one left sweep folds each core with T_j, T'_j and T''_j from the same core loads: about four (second = 0:
 * three) chains' work whatever d is, against d + 1 / 2 d + 1 chains of pcx_tt_deriv_batch, and as exact.  A dimension
 * with one node has both derivatives exactly 0, one with two nodes second derivative exactly 0.  second outside {0, 1},
 * N < 0 or a NULL buffer with N > 0 is PCX_ERR_INVALID before any launch; N = 0 returns PCX_OK without one.  Staging,
 * the two kernel forms and PCX_ERR_UNSUPPORTED (a wave-per-row model beyond the LDS of a workgroup) as
 * pcx_tt_deriv_batch[_dev]. */
int pcx_tt_grad_batch(pcx_tt *h, const double *pts, int64_t N, int second, double *out);
int pcx_tt_grad_batch_dev(pcx_tt *h, const double *d_pts, int64_t N, int second, double *d_out, void *stream);
/* Value, gradient and the full Hessian, batched: out is N x C row-major with C = 1 + d + d * d; column 0 is the value,
 * column 1 + u the first partial derivative and column 1 + d + u * d + v the second partial derivative along
 * dimensions u and v of the USER's dimension order (both triangles are written from the one computed number; u = v is
 * the diagonal of pcx_tt_grad_batch).  The sweeps of pcx_tt_grad_batch, with the vector D_i = L_i M1_i that its left sweep
 * forms at storage position i kept and carried to the right beside L: at every later position k two vector-matrix
 * products with folds the sweep holds anyway give D_i M_k and the mixed partial (D_i M1_k) . R_{k+1}.  A carried vector
 * takes LDS, so the left sweep runs in passes of `block` sources each (pass 0 is the gradient's sweep; a later pass
 * repeats the one-basis fold up to its first source): block = 0 takes the planner's choice, 1 .. max(1, d - 1) forces
 * one, a forced block whose launch does not fit the LDS of a workgroup is PCX_ERR_UNSUPPORTED, any other block
 * PCX_ERR_INVALID.  A row's bits depend neither on block nor on the batch; the first 1 + d columns and the diagonal are
 * pcx_tt_grad_batch's, bit for bit.  The Hessian row and column of a one-node dimension and the diagonal entry of a
 * two-node dimension are exactly 0.  N < 0 or a NULL buffer with N > 0 is PCX_ERR_INVALID; every check comes before any
 * launch; N = 0 returns PCX_OK without one.  Staging and the two kernel forms as pcx_tt_grad_batch[_dev], the host
 * entry's pieces shortened by (1 + 2 d) / C.
 * pcx_tt_hess_info: info_out[0] = the form (1 lane-per-row, 2 wave-per-row), [1] = the planner's block, [2] = the
 * dynamic LDS bytes of a workgroup at that block, [3] = the largest block that fits (0: none, every call is
 * PCX_ERR_UNSUPPORTED; [1] is then 0 and [2] the bytes at block 1). */
int pcx_tt_hess_batch(pcx_tt *h, const double *pts, int64_t N, int block, double *out);
int pcx_tt_hess_batch_dev(pcx_tt *h, const double *d_pts, int64_t N, int block, double *d_out, void *stream);
int pcx_tt_hess_info(pcx_tt *h, int32_t *info_out);
/* Kernel selection: 0 = auto, 1 = direct form on v_mfma_f64_16x16x4 (one GEMM over (node, left
 * rank) per dimension; ranks <= 64), 2 = small-rank "W first" form (ranks <= 12, cores in LDS),
 * 3 = small-rank direct form on v_mfma_f64_4x4x4_4b (ranks <= 12, n <= 16, cores in LDS),
 * 4 = lane-per-point VALU form (ranks <= 16, n <= 16: one point per lane, core elements as scalar
 * operands of v_fma_f64; what auto picks for ranks <= 15 since round 3).
 * PCX_ERR_UNSUPPORTED when the model is outside a form's range.
 * Models with a rank above 64 always run on a generic wave-per-point kernel.            */
int pcx_tt_set_kernel(pcx_tt *h, int variant);

/* ---- roots, minimum and maximum along one dimension -------------------------- */
/* The device half of roots() / minimize() / maximize() (reference _calculus.py:198-297) over a batch of N fibres of
 * n <= 64 nodes (PCX_ERR_INVALID above): mode 0 roots, 1 minimize, 2 maximize.  All pointers are host pointers.
 * roots_out: N x max(n-1, 1), ascending within a row, NaN-padded (mode 0); val_out / loc_out: N (modes 1, 2);
 * counts_out: N always, the roots (mode 0) or critical points (modes 1, 2) found, -1 where the colleague matrix was
 * not finite or its QR iteration did not converge (that row's roots / value / location are NaN).
 * pcx_cheb1d_calculus solves given fibres: values N x n at the ascending nodes of [lo, hi], barycentric weights,
 * and the n x n row-major differentiation matrix diff (modes 1, 2; may be NULL for mode 0).                        */
int pcx_cheb1d_calculus(int device, int n, double lo, double hi, const double *nodes, const double *weights,
                        const double *diff, const double *values, int64_t N, int mode, double *roots_out,
                        int32_t *counts_out, double *val_out, double *loc_out);
/* The fibres of a handle along dimension `dim`: row r of `fixed` (N x (d-1)) holds the values of the other
 * dimensions in increasing order; every value must lie in its dimension's domain (lo / hi: d doubles each, the
 * handle's domain), else PCX_ERR_INVALID before any launch.  The fibres are the handle's values at its own nodes of
 * `dim` and never leave the device.                                                                                */
int pcx_bary_calculus_batch(pcx_bary *h, int dim, const double *lo, const double *hi, const double *fixed, int64_t N,
                            int mode, double *roots_out, int32_t *counts_out, double *val_out, double *loc_out);
/* The same for a tensor train: `dim` and the columns of `fixed` are in the user's frame (dim_order applied on the
 * device), the domain is the handle's own; the fibre's nodes, weights and differentiation matrix are built as
 * chebyshev_nodes / compute_barycentric_weights / compute_differentiation_matrix build them.                      */
int pcx_tt_calculus_batch(pcx_tt *h, int dim, const double *fixed, int64_t N, int mode, double *roots_out,
                          int32_t *counts_out, double *val_out, double *loc_out);
/* The same for a slider (reference slider.py:1178-1283 slices to one dimension and re-interpolates): `dim` and the
 * columns of `fixed` are the slider's dimensions, lo / hi its domain (d doubles each; a handle does not know it).  Every
 * argument is checked before any launch: NULL handle, dim, mode, the node count of `dim` (<= 64) and the fixed values
 * against their dimensions' domains (NaN passes), each PCX_ERR_INVALID.  Along `dim` only the slide that owns it varies:
 * every other slide is evaluated once per row at its columns of `fixed`, the owner at the n fibre points of its own
 * group -- or, when its group is `dim` alone, not at all: its value tensor is the fibre.  Element (r, j) of the fibre is
 * pivot, then += v_i - pivot for the slides in partition order, the evaluation's order of operations, so it equals
 * pcx_slider_eval_batch at (fixed..., x_j).  The solver, its outputs, the NaN padding and counts = -1 are those of
 * pcx_bary_calculus_batch, with the owner slide's nodes, weights and differentiation matrix of `dim`.  Passes of at most
 * 2^21 fibre points, one download.  N = 0 returns PCX_OK and touches no output.                                       */
int pcx_slider_calculus_batch(pcx_slider *h, int dim, const double *lo, const double *hi, const double *fixed, int64_t N,
                              int mode, double *roots_out, int32_t *counts_out, double *val_out, double *loc_out);
/* The same for a spline (reference spline.py:1762-1910: slice to one dimension, solve every piece, merge): `dim` and the
 * columns of `fixed` are the spline's dimensions, lo / hi its domain (d doubles each; a handle does not know it).  Along
 * `dim` there are P pieces over [e_j, e_j+1], edges = [lo[dim], knots..., hi[dim]], piece j with n_j nodes (those of the
 * piece whose other indices are 0).  Every argument is checked before any launch: NULL handle, dim, mode, a node count
 * above 64 in any piece along `dim`, pieces that share an index along `dim` but differ in their node count there (one
 * grid serves an index), the fixed values against their dimensions' domains (NaN passes) and NULL outputs for
 * the mode, each PCX_ERR_INVALID.  A pass of rows expands every row into the F = sum n_j points (fixed..., x_ji), x_ji
 * piece j's own node values, and sends them through the spline's own evaluation (pcx_spline_eval_batch's routing,
 * bucketing and per-piece kernels: the other indices of a row's pieces are searchsorted(knots, v, "right") capped at the
 * last interval), solves the rows x P fibres in one launch with the solver of pcx_bary_calculus_batch on each piece's
 * interval, and merges the pieces of every row on the device:
 *   roots_out  N x W, W = sum_j max(n_j - 1, 1): the pieces' roots in piece order, an element kept when it is the first
 *              or exceeds its immediate predecessor in that sequence (kept or not) by more than
 *              1e-10 (|hi[dim] - lo[dim]| + 1); ascending, NaN-padded
 *   counts_out N, always written: roots kept (mode 0), the sum of the pieces' critical points (modes 1, 2), -1 when any
 *              piece of the row failed -- the row is then NaN everywhere
 *   val_out, loc_out   N each (modes 1, 2): the first piece, in order, that is strictly best
 * More than 65535 pieces along `dim`, or more than 2^23 fibre points in one row, are PCX_ERR_UNSUPPORTED.
 * Passes of at most 2^21 fibre points, one download.  N = 0 returns PCX_OK and touches no output.                      */
int pcx_spline_calculus_batch(pcx_spline *h, int dim, const double *lo, const double *hi, const double *fixed, int64_t N,
                              int mode, double *roots_out, int32_t *counts_out, double *val_out, double *loc_out);

/* ---- solutions of p = target along one dimension, a target per row ----------- */
/* The entries above with `targets` (N host doubles, one per row) and a method:
 *   method 0   all roots of p - targets[r]: the row's target is subtracted from its fibre on the device, one rounding per
 *              value, and the solver of mode 0 runs on the result; roots_out / counts_out as in mode 0 (the spline's
 *              widths and merge included), bit for bit what pcx_cheb1d_calculus returns on values - targets[:, None]
 *   method 1   bracketed inversion, one lane per fibre: on the knots [lo, nodes..., hi] a segment brackets when the
 *              value at its lower knot equals the target or p - target changes sign across it (a value equal to the
 *              target at hi counts as one more).  status_out (N) = the number of bracketing segments: 0 not reached on
 *              the knots (x NaN), 1 unique on the knots, > 1 not unique (x the lowest), -1 when the fibre or the target
 *              is not finite or the fixed iteration cap was reached (x NaN).  x_out (N) = the knot itself where the
 *              value equals the target there, else the root inside the lowest bracketing segment, found without leaving
 *              it, down to adjacent doubles (to within 2^-10 eps max(|lo|, |hi|) where the root is closer to 0 than
 *              2^-9 max(|lo|, |hi|)).  Two solutions between two neighbouring knots are not seen; method 0 finds
 *              them.  A spline solves every piece along `dim` on its own interval and nodes: x is the lowest over the
 *              pieces with status > 0, status the sum of the pieces' (a solution exactly on an interior knot is counted
 *              by both pieces that find it), -1 when any piece is -1.
 * The outputs of the other method may be NULL.  Checked before any launch, each PCX_ERR_INVALID: everything the
 * calculus entries check, n outside [1, 64], a method other than 0 or 1, NULL targets with N > 0, NULL outputs of the
 * method.  A target that is not finite is not an argument error: its row gets status -1 (method 1) or, its fibre no
 * longer being finite, counts -1 (method 0).  N = 0 returns PCX_OK and touches no output.                             */
int pcx_cheb1d_solve(int device, int n, double lo, double hi, const double *nodes, const double *weights,
                     const double *values, const double *targets, int64_t N, int method, double *roots_out,
                     int32_t *counts_out, double *x_out, int32_t *status_out);
int pcx_bary_solve_batch(pcx_bary *h, int dim, const double *lo, const double *hi, const double *fixed,
                         const double *targets, int64_t N, int method, double *roots_out, int32_t *counts_out,
                         double *x_out, int32_t *status_out);
int pcx_tt_solve_batch(pcx_tt *h, int dim, const double *fixed, const double *targets, int64_t N, int method,
                       double *roots_out, int32_t *counts_out, double *x_out, int32_t *status_out);
int pcx_slider_solve_batch(pcx_slider *h, int dim, const double *lo, const double *hi, const double *fixed,
                           const double *targets, int64_t N, int method, double *roots_out, int32_t *counts_out,
                           double *x_out, int32_t *status_out);
int pcx_spline_solve_batch(pcx_spline *h, int dim, const double *lo, const double *hi, const double *fixed,
                           const double *targets, int64_t N, int method, double *roots_out, int32_t *counts_out,
                           double *x_out, int32_t *status_out);

/* ---- TT-Cross build steps (tensor_train.py:123-540) ------------------------- */
/* One unfolding step of _tt_cross (:332-362 and :449-474): thin SVD of the m x c cross
 * matrix C (row-major), rank = max(1, min(cap, #{S > rel_thresh*S0}, min(m,c))), maxvol
 * rows of U[:, :rank] when m > rank, C_hat = U inv(U[piv]).  Outputs: chat (m x rank
 * row-major), pivots (rank), rank.  Runs on `device` (single-workgroup HIP kernels).
 * The result does not depend on the scale of C (any finite FP64 magnitudes).  m <= 8192 and
 * c <= 64, else PCX_ERR_UNSUPPORTED; an entry that is not finite is PCX_ERR_INVALID.      */
int pcx_tt_cross_step(int device, const double *C, int m, int c, int cap, double rel_thresh,
                      double *chat, int64_t *pivots, int32_t *rank_out);

/* _maxvol (:38-120) on a row-major m x r matrix; idx_out receives r row indices (m <= r:
 * 0 .. m-1).  Same limits; an entry that is not finite is PCX_ERR_INVALID.              */
int pcx_maxvol(int device, const double *A, int m, int r, double tol, int max_iters,
               int64_t *idx_out);

/* _value_core_to_coeff_core (:997-1016): DCT-II along the node axis, /n, c_0 halved.  */
int pcx_tt_value_to_coeff_core(int device, const double *value_core, int rl, int n, int rr,
                               double *coeff_core);

/* _eval_tt (:223-228) batched: TT value at `count` integer grid index tuples
 * (count x d int32, row-major) through the chain of VALUE cores (same layout as
 * coeff_cores_cat).  Used by the convergence check (:287-297).                        */
int pcx_tt_grid_eval(int device, int d, const int32_t *n_nodes, const int32_t *ranks,
                     const double *value_cores_cat, const int32_t *idx, int count, double *out);

/* The dense tensor of a tensor train on a tensor-product grid (stateless, like pcx_tt_round): grid_cores_cat holds the
 * value cores ON THE GRID, G_k of shape (r_k, m_k, r_{k+1}) with ranks[0] = ranks[d] = 1, C order, concatenated; out
 * receives prod m_k doubles, C order, dimensions in storage order.  The chain
 *   P_{k+1} = reshape(P_k, (m_0 .. m_{k-1}, r_k)) . reshape(G_k, (r_k, m_k r_{k+1}))
 * runs on the device as d - 1 mode products (pcx_tensor_mode_product with outer = 1), from the left or from the right,
 * whichever has the smaller largest intermediate (a tie: from the left).  An empty axis is PCX_ERR_INVALID.  (Not to
 * be confused with pcx_tt_grid_eval above, which evaluates integer grid INDEX tuples for TT-Cross.)                   */
int pcx_tt_tensor_grid(int device, int d, const int32_t *m, const int32_t *ranks, const double *grid_cores_cat, double *out);

/* TT-SVD compression of a dense C-order value tensor (d dims, n_nodes): replaces
 * _tt_svd_from_tensor (tensor_train.py:638-690), used by ChebyshevTT.from_values (:2871-2965)
 * and build(method="svd") (:1235-1243).  Each unfolding is factored on the device by a
 * one-sided Jacobi iteration on its rows; the rank rule is the reference's (cap at
 * max_rank, drop singular values <= tol * sigma_max, at least 1).  Outputs: ranks_out[d+1];
 * the VALUE cores (r_{k-1}, n_k, r_k), C order, concatenated in cores_out (capacity
 * cores_cap doubles, used length in *cores_len); sweeps_out (optional) = Jacobi sweeps run. */
int pcx_tt_svd(int device, int d, const int32_t *n_nodes, const double *tensor, int max_rank,
               double tol, int32_t *ranks_out, double *cores_out, int64_t cores_cap,
               int64_t *cores_len, int32_t *sweeps_out);

/* TT rounding (reference _algebra.py::_tt_round_cores), used by ChebyshevTT + and -: a right-to-left
 * orthogonalisation sweep, then a left-to-right truncated-SVD sweep, every factorisation a one-sided
 * Jacobi iteration on the device.  Input: d coefficient cores (r_{k-1}, n_k, r_k), C order,
 * concatenated, ranks[d+1] with ranks[0] = ranks[d] = 1.  The rank rule is the reference's (cap at
 * max_rank, drop singular values <= tol * sigma_max when sigma_max > 0, at least 1).  Ranks above 256
 * or more than 256 nodes are PCX_ERR_UNSUPPORTED before anything runs.  Outputs: ranks_out[d+1]; the
 * rounded cores, cores 0..d-2 left-orthonormal, concatenated in cores_out (capacity cores_cap
 * doubles -- the input length always suffices -- used length in *cores_len); sweeps_out (optional)
 * = Jacobi sweeps run.                                                                          */
int pcx_tt_round(int device, int d, const int32_t *n_nodes, const int32_t *ranks, const double *cores,
                 int max_rank, double tol, int32_t *ranks_out, double *cores_out, int64_t cores_cap,
                 int64_t *cores_len, int32_t *sweeps_out);

/* Core orthogonalisation in place of ChebyshevTT.orth_left / orth_right (reference tensor_train.py:1296-1356,
 * helpers :697-735).  side 0: cores 0 .. position-1 become left-orthonormal (position in [1, d-1]), each R factor
 * multiplied into the next core; side 1: cores position+1 .. d-1 become row-orthonormal (position in [0, d-2]), each
 * factor multiplied into the core before.  Every factorisation is a Householder QR of one unfolding in one workgroup,
 * columns in their own order; a column that is zero below its diagonal takes the identity reflector, so the factor is
 * orthonormal on rank-deficient input too.  An unfolding wider than tall gives the smaller bond, min(r_l n, r_r), as
 * numpy.linalg.qr does.  Layout and limits of pcx_tt_round: cores concatenated in C order, ranks[0] = ranks[d] = 1,
 * ranks or node counts above 256 are PCX_ERR_UNSUPPORTED before anything runs.  The input length always suffices as
 * cores_cap.  The cores on the far side of `position` come back bit for bit.                                      */
int pcx_tt_orth(int device, int d, const int32_t *n_nodes, const int32_t *ranks, const double *cores, int side,
                int position, int32_t *ranks_out, double *cores_out, int64_t cores_cap, int64_t *cores_len);

/* Fixed-rank completion by alternating least squares against the values on the whole tensor grid
 * (ChebyshevTT.run_completion, reference tensor_train.py:1358-1436 and _als_fixed_rank_sweeps :738-876).  value_cores:
 * the VALUE cores in pcx_tt_round's layout; target: host, prod(n) doubles, C order.  With the neighbouring cores in
 * orthonormal form the solve of core k is the projection C_k = L^T T R^T; one outer iteration is a left-to-right and
 * a right-to-left half sweep that carry the projected target along and read it about four times.  After each outer
 * iteration the dense tensor of the cores is formed on the device and rel_change = ||T_new - T_prev||_F /
 * (||T_prev||_F + 1e-30) goes to rel_change_out[i]; the loop stops when it falls below `tolerance` (the reference's
 * rule) or after max_iter iterations; *iters_out = iterations run.  max_iter <= 0 runs none and returns the cores as
 * given (rel_change_out may be NULL).  *grid_residual_out = ||TT - target||_F / ||target||_F of the returned cores.
 * Bonds shrink where an unfolding cannot hold them (ranks_out).  Every sum runs in a fixed order: equal input gives
 * equal bits.  Limits: those of pcx_tt_round, and a grid of at most PCX_TT_ALS_MAX_GRID points (the device holds the
 * target, two reconstructions and the projection buffers, about 4 prod(n) doubles), else PCX_ERR_UNSUPPORTED before
 * anything runs.                                                                                                    */
#define PCX_TT_ALS_MAX_GRID (1LL << 28)
int pcx_tt_als(int device, int d, const int32_t *n_nodes, const int32_t *ranks, const double *value_cores,
               const double *target, double tolerance, int max_iter, int32_t *ranks_out, double *cores_out,
               int64_t cores_cap, int64_t *cores_len, int32_t *iters_out, double *rel_change_out,
               double *grid_residual_out);

/* Diagnostic: the dense steps of pcx_tt_als / pcx_tt_orth one at a time (tests/test_gpu_als_steps.py).  Host pointers,
 * the null stream; each is an upload, one call of the internal step and a download.
 *
 * One contraction.  side 0: out (r x R) = small^T big with small = Q (K x r), big = P (K x R); side 1: out (R x r) =
 * big small^T with small = C (r x K), big = P (R x K); all row-major.  form 0: the dispatch pcx_tt_als uses (MFMA from
 * rank 16 on, or from PCX_TT_ALS_MFMA_MIN); 1: the VALU form of this rank (4, 8, 12 accumulators, above 12 sixteen,
 * tiled over the rank); 2: the MFMA form (one 16-row tile up to rank 16, two above, tiled over the rank).  *form_used
 * = 1 or 2.  The device output starts as a NaN pattern and is followed by 256 doubles of it: an element the kernel
 * did not write comes back NaN, a disturbed tail is PCX_ERR_INTERNAL.  1 <= r <= 256 (above: PCX_ERR_UNSUPPORTED),
 * K >= 1, R >= 1, K R <= PCX_TT_ALS_MAX_GRID (above: PCX_ERR_UNSUPPORTED).                                          */
int pcx_tt_als_project(int device, int side, int form, const double *small, const double *big, double *out, int K,
                       int r, int64_t R, int32_t *form_used);

/* Diagnostic: the Householder QR of A (m x c row-major, c <= 256, m c <= PCX_TT_ALS_MAX_GRID, else
 * PCX_ERR_UNSUPPORTED): Q (m x p) and R (p x c), p = min(m, c).  Q does not depend on the scale of A and R follows it
 * exactly, for any finite FP64 magnitudes.                                                                          */
int pcx_tt_als_qr(int device, const double *A, int64_t m, int c, double *Q, double *R);

/* Diagnostic: out4 = |tnew - tprev|^2, |tprev|^2, |tnew - target|^2, |target|^2 over G elements
 * (1 <= G <= PCX_TT_ALS_MAX_GRID), the convergence sums of one outer iteration.  The squares are not scaled.        */
int pcx_tt_als_norms(int device, const double *tnew, const double *tprev, const double *target, int64_t G, double *out4);

/* Least-squares fitting of a tensor train to scattered samples (ChebyshevTT.fit_samples / from_samples; extension: the
 * reference has no builder for data off the grid).  A fit session holds N samples on the device for the whole of one
 * fit: points N x d row-major in STORAGE order (column k belongs to storage position k: the caller permutes) and N
 * values.  pcx_tt_fit_create copies host arrays; pcx_tt_fit_create_dev adopts device pointers without a copy (they must
 * outlive the session).  lo / hi = the domain by storage position, d each, lo < hi.  Checked at creation, each
 * PCX_ERR_INVALID: d in [1, PCX_MAX_DIMS], N >= 1, NULL, a value or coordinate that is not finite, a coordinate outside
 * its dimension's domain (host arrays: a loop on the host before any launch; device arrays: one small kernel).  More
 * than PCX_TT_FIT_MAX_SAMPLES samples are PCX_ERR_UNSUPPORTED.
 *
 * pcx_tt_fit_normal: the normal equations of position k (0 <= k < d) for the given COEFFICIENT cores (pcx_tt_create's
 * layout, ranks[0] = ranks[d] = 1).  With the design row of sample i
 *     a_i = L_i (x) T(t_k(x_ik)) (x) R_i          C order (a, j, b), the core's own layout, P = r_k n_k r_{k+1} entries,
 * L_i / R_i the left / right partial products of the chain at x_i and T the n_k Chebyshev polynomials at
 * t = 2 (x - lo) / (hi - lo) - 1 (-1 and +1 exactly at the domain's ends), G_out (host, P x P, both triangles, exactly symmetric) = sum_i a_i a_i^T and b_out
 * (host, P) = sum_i y_i a_i.  Two kernels: one wave per sample forms (L_i, T, R_i), r_k + n_k + r_{k+1} numbers a sample;
 * the Gram kernel forms the P-wide rows in registers from them (the N x P matrix never exists in memory) and adds the
 * products over fixed chunks of samples, v_mfma_f64_16x16x4_f64 with the samples as K from P = 16 on, one output per
 * lane on the VALU below; a third kernel adds the chunks' partial sums in ascending order.  No atomics: equal input
 * gives equal bits.  pcx_tt_fit_set_form forces the Gram kernel: 0 the rule above, 1 VALU, 2 MFMA, each at any P
 * (anything else: PCX_ERR_INVALID).  The device outputs start as a NaN pattern followed by 256 doubles of it: an
 * element no kernel wrote comes back NaN, a disturbed tail is PCX_ERR_INTERNAL.
 * Limits, each PCX_ERR_UNSUPPORTED before anything runs: ranks or node counts above 256, P > PCX_TT_FIT_MAX_P.
 *
 * pcx_tt_fit_residual: sumsq_out[0] = sum_i (TT(x_i) - y_i)^2, sumsq_out[1] = sum_i y_i^2 for the given cores: the
 * evaluation kernels of pcx_tt_eval_batch_dev on the resident points, then a fixed-grid, fixed-tree reduction.  The
 * squares are not scaled.
 *
 * pcx_tt_fit_times: ms_out[0 .. 2] = the device time in milliseconds of the three kernels of the session's last
 * pcx_tt_fit_normal (interface vectors, Gram, reduction), from events recorded around each; zeros before the first.  */
#define PCX_TT_FIT_MAX_P 4096
#define PCX_TT_FIT_MAX_SAMPLES (1LL << 28)
typedef struct pcx_tt_fit pcx_tt_fit;
int pcx_tt_fit_create(int device, int d, const double *lo, const double *hi, const double *pts, const double *values,
                      int64_t N, pcx_tt_fit **out);
int pcx_tt_fit_create_dev(int device, int d, const double *lo, const double *hi, const double *d_pts,
                          const double *d_values, int64_t N, pcx_tt_fit **out);
int pcx_tt_fit_destroy(pcx_tt_fit *s);
int pcx_tt_fit_set_form(pcx_tt_fit *s, int form);
int pcx_tt_fit_normal(pcx_tt_fit *s, int d, const int32_t *n_nodes, const int32_t *ranks, const double *coeff_cores,
                      int k, double *G_out, double *b_out);
int pcx_tt_fit_residual(pcx_tt_fit *s, int d, const int32_t *n_nodes, const int32_t *ranks, const double *coeff_cores,
                        double *sumsq_out);
int pcx_tt_fit_times(pcx_tt_fit *s, float *ms_out);

/* A sequence of adjacent swaps of storage axes (reference _algebra.py::_tt_swap_adjacent, driven by
 * ChebyshevTT.reorder): swap s exchanges axes swaps[s] and swaps[s] + 1 by one truncated SVD of the
 * merged pair (same rank rule).  Same input layout and limits as pcx_tt_round; a merged pair of more
 * than 4096 rows (r_{i-1} n_{i+1}) or 2^24 elements is PCX_ERR_UNSUPPORTED.  Outputs: n_nodes_out[d]
 * (the permuted node counts), ranks_out[d+1], the cores in cores_out as above (capacity: the caller
 * bounds the new ranks), sweeps_out (optional).                                                 */
int pcx_tt_reorder(int device, int d, const int32_t *n_nodes, const int32_t *ranks, const double *cores,
                   int n_swaps, const int32_t *swaps, int max_rank, double tol, int32_t *n_nodes_out,
                   int32_t *ranks_out, double *cores_out, int64_t cores_cap, int64_t *cores_len,
                   int32_t *sweeps_out);

/* ---- multi-GPU: the final gather of the per-rank result blocks ----------------- */
/* The reference has no multi-device path (docs/roadmap.md:245); SURVEY.md 8(e) defines
 * it: query rows are sharded in contiguous blocks over one process per GPU, the model is
 * replicated, and the ONLY exchange is the gather of the result blocks on one rank --
 * here grouped ncclSend/ncclRecv of RCCL over xGMI (one direct link per peer, no ring).
 * RCCL (librccl.so.1 of the ROCm this library was built with) is dlopen'ed on the first
 * pcx_comm_* call: single-GPU users never load it.  No PyTorch anywhere.
 *
 * Bootstrap: rank 0 calls pcx_comm_unique_id and hands the PCX_COMM_ID_BYTES opaque bytes
 * to the other ranks by any host channel (pychebyshev_amd.distributed.HostGroup uses a
 * shared-memory file); every rank then calls pcx_comm_create (collective, blocking).      */
#define PCX_COMM_ID_BYTES 128
typedef struct pcx_comm pcx_comm;
int pcx_comm_unique_id(void *id_out /* PCX_COMM_ID_BYTES */);
int pcx_comm_create(int device, int rank, int world, const void *id, pcx_comm **out);
int pcx_comm_destroy(pcx_comm *c);
/* rank, world, device, RCCL version code (any pointer may be NULL)                      */
int pcx_comm_info(pcx_comm *c, int32_t *rank, int32_t *world, int32_t *device, int32_t *rccl_version);
/* Gather blocks of doubles on `root`: rank r contributes counts[r] doubles from d_send,
 * which land at d_recv + offsets[r] on root (d_recv is ignored elsewhere; counts/offsets
 * have `world` entries and must be identical on every rank).  Enqueues on `stream`
 * (NULL = the communicator's own stream) and returns without synchronizing: ordered
 * behind the kernel that produced d_send when that ran on the same stream.              */
int pcx_comm_gatherv_dev(pcx_comm *c, const double *d_send, double *d_recv, const int64_t *counts,
                         const int64_t *offsets, int root, void *stream);
/* Host-level helpers for drivers: max over ranks of one double (the benchmark's
 * max-over-ranks step time) and a barrier; both synchronize the communicator's stream.  */
int pcx_comm_allreduce_max(pcx_comm *c, double *value_inout);
int pcx_comm_barrier(pcx_comm *c);
int pcx_comm_stream(pcx_comm *c, void **stream);

#ifdef __cplusplus
}
#endif
#endif /* PCX_H */
