// pcx_internal.h -- host-side internals shared by the translation units of libpcx_hip.so (not part of the ABI).
#pragma once

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <deque>
#include <exception>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "pcx_common.h"

#define PCX_HIDDEN __attribute__((visibility("hidden")))

// ---------------------------------------------------------------------------------
// errors: one thread-local message buffer for the whole library (defined in pcx_core.hip)
// ---------------------------------------------------------------------------------
#define PCX_ERR_LEN 512
PCX_HIDDEN char *pcx_err_buf() noexcept;        // the calling thread's message buffer (PCX_ERR_LEN bytes)

static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(pcx_err_buf(), PCX_ERR_LEN, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(PCX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                               \
    } while (0)

static int use_device(int device) {
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess || cnt <= 0)
        return fail(PCX_ERR_NO_DEVICE, "no HIP device available (%s)", hipGetErrorString(e));
    if (device < 0 || device >= cnt)
        return fail(PCX_ERR_NO_DEVICE, "device %d out of range [0, %d)", device, cnt);
    HIP_TRY(hipSetDevice(device));
    return PCX_OK;
}

// ---------------------------------------------------------------------------------
// No C++ exception crosses the C ABI (include/pcx.h: "never throws"): every extern "C" body runs inside
// PCX_API_BEGIN / PCX_API_END.  std::bad_alloc (a std::vector, std::map node or handle that could not be
// allocated) becomes PCX_ERR_NOMEM, anything else (std::system_error from a thread that could not start, ...)
// PCX_ERR_HIP, both with pcx_last_error() set.  PCX_FAULT_INJECT=<entry point name> makes that entry point
// throw std::bad_alloc at its start: the CPU-side test of this guard (tests/test_host_logic.py).
// ---------------------------------------------------------------------------------
PCX_HIDDEN int pcx_guard_caught(const char *fn) noexcept;     // call inside a catch (...) block only
PCX_HIDDEN void pcx_fault_inject(const char *fn);             // throws when the environment names fn

#define PCX_API_BEGIN try { pcx_fault_inject(__func__);
#define PCX_API_END } catch (...) { return pcx_guard_caught(__func__); }

// grow-only device scratch used by the host-pointer entry points
struct Scratch {
    void *ptr = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return PCX_OK;
        if (ptr) { (void)hipFree(ptr); ptr = nullptr; cap = 0; }
        hipError_t e = hipMalloc(&ptr, bytes);
        if (e != hipSuccess) { ptr = nullptr; return fail(PCX_ERR_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); }
        cap = bytes;
        return PCX_OK;
    }
    void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; cap = 0; }
};

// RAII device buffer: freed on every exit path unless release() hands the pointer on
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) {
        hipError_t e = hipMalloc(&p, bytes ? bytes : 8);
        if (e != hipSuccess) { p = nullptr; return fail(PCX_ERR_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); }
        return PCX_OK;
    }
    template <typename T> T *as() { return (T *)p; }
    template <typename T> T *release() { T *q = (T *)p; p = nullptr; return q; }
};

// typed view of memory somebody else owns (a Scratch)
struct DevView {
    void *p;
    template <typename T> T *as() { return (T *)p; }
};

// Host-pointer batches are processed in chunks so the staging buffers stay bounded.
static const int64_t kChunkPoints = 1 << 23;
// ... and, from two such pieces on, in 256 Ki-point pieces alternating between two streams
static const int64_t kPipeChunkPoints = 1 << 18;

// Small host-pointer batches skip the H2D/D2H copies: the points are memcpy'd into a pinned,
// device-mapped buffer the kernel reads directly over PCIe, and the results land in a second
// pinned buffer (coherent host memory: visible after the stream sync).  Two API calls fewer
// per query; this is the single-query latency path.
static const size_t kPinnedBytes = 512 * 1024;
struct Pinned {
    void *in = nullptr, *out = nullptr;
    bool tried = false;
    bool ready() {
        if (!tried) {
            tried = true;
            if (hipHostMalloc(&in, kPinnedBytes, hipHostMallocMapped) != hipSuccess) in = nullptr;
            if (hipHostMalloc(&out, kPinnedBytes, hipHostMallocMapped) != hipSuccess) out = nullptr;
            (void)hipGetLastError();
        }
        return in && out;
    }
    void release() {
        if (in) (void)hipHostFree(in);
        if (out) (void)hipHostFree(out);
        in = out = nullptr;
    }
};

// A copy from or to PAGEABLE caller memory blocks the calling thread until it is done, so a single host thread runs a
// piece's upload and the previous piece's download one after the other (40 + 8 bytes per TT point at the pageable rate:
// the whole host-pointer path).  The downloads of a pipelined batch therefore go to a helper thread: it issues each one
// on the piece's own stream -- behind that piece's kernel -- while the caller's thread is inside the next upload.  The
// two threads touch different allocations (points / results).  Jobs are issued in order; the caller's thread waits for
// job i to have been ISSUED before it queues anything else on that stream or frees its source buffer.
struct Downloader {
    struct Job { void *dst; const void *src; size_t bytes; hipStream_t st; };
    int device;
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Job> q;
    long pushed = 0, issued = 0;
    bool stop = false;
    int rc = PCX_OK;
    std::string err;
    explicit Downloader(int dev) : device(dev) {}
    Downloader(const Downloader &) = delete;
    Downloader &operator=(const Downloader &) = delete;
    void run() {
        (void)hipSetDevice(device);
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || !q.empty(); });
                if (q.empty()) return;
                j = q.front();
                q.pop_front();
            }
            hipError_t e = hipSuccess;
            if (rc == PCX_OK) e = hipMemcpyAsync(j.dst, j.src, j.bytes, hipMemcpyDeviceToHost, j.st);
            {
                std::lock_guard<std::mutex> lk(mu);
                if (e != hipSuccess && rc == PCX_OK) { rc = PCX_ERR_HIP; err = std::string("download: ") + hipGetErrorString(e); }
                ++issued;
            }
            cv.notify_all();
        }
    }
    void push(void *dst, const void *src, size_t bytes, hipStream_t st) {
        {
            std::lock_guard<std::mutex> lk(mu);
            q.push_back(Job{dst, src, bytes, st});
            ++pushed;
        }
        if (!th.joinable()) th = std::thread([this] { run(); });
        cv.notify_all();
    }
    void wait_issued(long count) {               // until the first `count` jobs have been issued
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return issued >= count; });
    }
    int finish() {                               // every job issued, the thread gone; the streams are the caller's to drain
        if (th.joinable()) {
            wait_issued(pushed);
            { std::lock_guard<std::mutex> lk(mu); stop = true; }
            cv.notify_all();
            th.join();
        }
        return rc == PCX_OK ? PCX_OK : fail(rc, "%s", err.c_str());
    }
    ~Downloader() { (void)finish(); }
};

// Staging of one handle's host-pointer batches (stage_host_batch): two slots of device scratch, the second slot's stream
// and the zero-copy window.  Guarded by the handle's mutex.
struct HostStage {
    hipStream_t second = nullptr;    // the second slot's stream, created on the first two-slot batch
    Scratch pts[2], out[2];
    Pinned pin;
    void release() {                 // at destroy, after the handle's own stream has drained
        if (second) { (void)hipStreamSynchronize(second); (void)hipStreamDestroy(second); second = nullptr; }
        for (int i = 0; i < 2; ++i) { pts[i].release(); out[i].release(); }
        pin.release();
    }
};

// How a host-pointer batch is cut: the first piece, every later piece, whether the pieces alternate between two slots
// (the handle's stream and HostStage::second), and whether a batch that fits kPinnedBytes takes the zero-copy window.
struct StagePlan { int64_t first, piece; bool two_slots, zero_copy; };

// N points (pts, N x d) into out (N x m) through launch(slot, stream, d_pts, cnt, d_out) -> rc, which queues the evaluation
// of cnt device-resident points on `stream` (slot 1: the second slot's stream).  One slot: upload, launch, download and
// drain, piece by piece.  Two slots: the upload of piece i + 1 overlaps the kernel of piece i and the download of piece
// i - 1.  The copies read and write the CALLER's arrays: whatever happens, the Downloader is joined and both streams are
// drained before this returns.  Caller holds the handle's mutex.
template <typename Launch>
static int stage_host_batch(HostStage &s, int device, hipStream_t main, const double *pts, int64_t N, int d, int m,
                            double *out, const StagePlan &plan, Launch &&launch) {
    const size_t in_row = (size_t)d * sizeof(double), out_row = (size_t)m * sizeof(double);
    if (plan.zero_copy && N > 0 && N * in_row <= kPinnedBytes && N * out_row <= kPinnedBytes && s.pin.ready()) {
        memcpy(s.pin.in, pts, N * in_row);
        const int rc = launch(0, main, (const double *)s.pin.in, (long)N, (double *)s.pin.out);
        const hipError_t e = hipStreamSynchronize(main);
        if (rc) return rc;
        HIP_TRY(e);
        memcpy(out, s.pin.out, N * out_row);
        return PCX_OK;
    }
    if (plan.two_slots && !s.second) HIP_TRY(hipStreamCreateWithFlags(&s.second, hipStreamNonBlocking));
    Downloader dl(device);
    auto pipeline = [&]() -> int {
        long piece_no = 0;
        for (int64_t start = 0, step = plan.first; start < N; start += step, step = plan.piece, ++piece_no) {
            const long cnt = (long)std::min<int64_t>(step, N - start);
            const int slot = plan.two_slots ? (int)(piece_no & 1) : 0;
            hipStream_t st = slot ? s.second : main;
            if (plan.two_slots && piece_no >= 2) dl.wait_issued(piece_no - 1);     // this slot's last download is behind its kernel
            int rc = s.pts[slot].reserve(cnt * in_row);
            if (rc) return rc;
            if ((rc = s.out[slot].reserve(cnt * out_row))) return rc;
            double *dp = (double *)s.pts[slot].ptr, *dout = (double *)s.out[slot].ptr;
            HIP_TRY(hipMemcpyAsync(dp, pts + (size_t)start * d, cnt * in_row, hipMemcpyHostToDevice, st));
            if ((rc = launch(slot, st, (const double *)dp, cnt, dout))) return rc;
            if (plan.two_slots) {
                dl.push(out + (size_t)start * m, dout, cnt * out_row, st);
                continue;
            }
            HIP_TRY(hipMemcpyAsync(out + (size_t)start * m, dout, cnt * out_row, hipMemcpyDeviceToHost, st));
            if (start + cnt < N) HIP_TRY(hipStreamSynchronize(st));    // single slot: drained before its buffers are reused
        }
        return PCX_OK;
    };
    const int rc_pipe = pipeline();
    const int rc_dl = dl.finish();
    const hipError_t e1 = hipStreamSynchronize(main);
    const hipError_t e2 = s.second ? hipStreamSynchronize(s.second) : hipSuccess;
    if (rc_pipe) return rc_pipe;
    if (rc_dl) return rc_dl;
    HIP_TRY(e1);
    HIP_TRY(e2);
    return PCX_OK;
}

// ---------------------------------------------------------------------------------
// What the four pcx_*_ladder_batch / _dev pairs share (pcx_bary_ladder.hip, pcx_tt_ladder.hip, pcx_piecewise_ladder.hip)
// ---------------------------------------------------------------------------------
// The argument checks of a ladder entry on a model of d dimensions, in the entries' order; a class's own checks go in
// front or behind.  deriv may be NULL (a class without a spec, or the plain values).
static int ladder_check(const void *h, int d, int dim, const int32_t *deriv, const void *fixed, int64_t N, const void *xs, int m,
                        int xs_per_row, const void *out) {
    if (!h) return fail(PCX_ERR_INVALID, "handle is NULL");
    if (N < 0) return fail(PCX_ERR_INVALID, "N < 0");
    if (m < 0) return fail(PCX_ERR_INVALID, "m < 0");
    if (xs_per_row != 0 && xs_per_row != 1) return fail(PCX_ERR_INVALID, "xs_per_row = %d is neither 0 nor 1", xs_per_row);
    if (dim < 0 || dim >= d) return fail(PCX_ERR_INVALID, "dim %d out of range [0, %d]", dim, d - 1);
    if (deriv)
        for (int k = 0; k < d; ++k)
            if (deriv[k] < 0 || deriv[k] > 8)
                return fail(PCX_ERR_INVALID, "derivative order %d at dim %d outside [0, 8]", (int)deriv[k], k);
    if (N > 0 && d > 1 && !fixed) return fail(PCX_ERR_INVALID, "fixed is NULL");
    if (m > 0 && (xs_per_row ? N > 0 : true) && !xs) return fail(PCX_ERR_INVALID, "xs is NULL");
    if (N > 0 && m > 0 && !out) return fail(PCX_ERR_INVALID, "out is NULL");
    return PCX_OK;
}

// The m values all rows share, from the host into a buffer of the call's (DevBuf) or of the handle's (Scratch): queued
// on st, or with a blocking copy; *d_xs: where they are on the device.
static int ladder_upload_xs(void *p, const double *xs, int m, bool queued, hipStream_t st, const double **d_xs) {
    if (queued) HIP_TRY(hipMemcpyAsync(p, xs, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
    else HIP_TRY(hipMemcpy(p, xs, (size_t)m * sizeof(double), hipMemcpyHostToDevice));
    *d_xs = (const double *)p;
    return PCX_OK;
}
static int ladder_shared_xs(DevBuf &buf, const double *xs, int m, bool queued, hipStream_t st, const double **d_xs) {
    const int rc = buf.alloc((size_t)m * sizeof(double));
    return rc ? rc : ladder_upload_xs(buf.p, xs, m, queued, st, d_xs);
}
static int ladder_shared_xs(Scratch &buf, const double *xs, int m, bool queued, hipStream_t st, const double **d_xs) {
    const int rc = buf.reserve((size_t)m * sizeof(double));
    return rc ? rc : ladder_upload_xs(buf.ptr, xs, m, queued, st, d_xs);
}

// doubles of the wider side (rows in, ladders out) one pass of a host-pointer ladder stages: 8 MB, an eighth of a
// kChunkPoints piece of pcx_bary_eval_batch
static const int64_t kLadderPassDoubles = (int64_t)1 << 20;

// A staged row is the nq fixed coordinates, then the row's m values when xs is per row -- at least one double: a
// one-dimensional model with shared values stages one unused double per row.
static int ladder_row_width(int nq, int m, int xs_per_row) { return std::max(1, nq + (xs_per_row ? m : 0)); }
// rows per pass
static int64_t ladder_pass_rows(int nq, int m, int xs_per_row) {
    return std::max<int64_t>(1, kLadderPassDoubles / std::max(ladder_row_width(nq, m, xs_per_row), m));
}

// The host-pointer form of every ladder: the rows are packed (shared values and nq > 0: the caller's `fixed` is the
// staged array already) and go through stage_host_batch in passes of ladder_pass_rows rows.
// run(d_fixed, fstride, d_xs, xstride, cnt, d_out, st) queues cnt device-resident rows on st, the stage's stream of the
// pass (`main`: one slot); d_shared: the shared values on the device.  Caller holds the handle's mutex.
template <typename Run>
static int ladder_host_passes(HostStage &stage, int device, hipStream_t main, int nq, const double *fixed, int64_t N,
                              const double *xs, const double *d_shared, int m, int xs_per_row, double *out, Run &&run) {
    const int w = ladder_row_width(nq, m, xs_per_row);
    const int64_t pass = ladder_pass_rows(nq, m, xs_per_row);
    const bool direct = !xs_per_row && nq > 0;
    std::vector<double> rows;
    for (int64_t start = 0; start < N; start += pass) {
        const int64_t cnt = std::min<int64_t>(pass, N - start);
        const double *src = fixed + (size_t)start * nq;
        if (!direct) {
            rows.assign((size_t)cnt * w, 0.0);
            for (int64_t r = 0; r < cnt; ++r) {
                double *dst = rows.data() + (size_t)r * w;
                if (nq) memcpy(dst, fixed + (size_t)(start + r) * nq, (size_t)nq * sizeof(double));
                if (xs_per_row) memcpy(dst + nq, xs + (size_t)(start + r) * m, (size_t)m * sizeof(double));
            }
            src = rows.data();
        }
        int rc = stage_host_batch(stage, device, main, src, cnt, w, m, out + (size_t)start * m, StagePlan{cnt, cnt, false, true},
                                  [&](int, hipStream_t st, const double *dp, long c, double *dout) {
                                      return xs_per_row ? run(dp, (long)w, dp + nq, (long)w, c, dout, st)
                                                        : run(dp, (long)w, d_shared, 0L, c, dout, st);
                                  });
        if (rc) return rc;
    }
    return PCX_OK;
}

// true when the runtime reports [p, p + bytes), bytes > 0, as page-locked host memory at both ends and up to 14 interior
// points (two separate registrations could cover just the ends)
static bool host_range_locked(const void *p, size_t bytes) {
    bool locked = true;
    const size_t probes = bytes > (size_t)16 ? 16 : 2;
    for (size_t i = 0; i < probes && locked; ++i) {
        const size_t off = i + 1 == probes ? bytes - 1 : (bytes / (probes - 1)) * i;
        hipPointerAttribute_t at{};
        locked = hipPointerGetAttributes(&at, (const char *)p + off) == hipSuccess && at.type == hipMemoryTypeHost;
    }
    (void)hipGetLastError();
    return locked;
}

struct HostPin {
    void *a = nullptr, *b = nullptr;
    // true when [p, p + bytes) is page-locked afterwards: registered here (released by the destructor) or already
    // page-locked by the caller (pcx_host_register, hipHostMalloc)
    bool pin(const void *p, size_t bytes, void **slot) {
        if (!p || !bytes) return true;
        // Ask the runtime about the range FIRST, register only what is not page-locked yet.  (Round 4 tried the other order
        // -- always attempt hipHostRegister and read "already registered" off the error -- and tools/soak.py --pin ended in
        // the GPU memory access fault of round 3 again, at a host address, in the single-handle call FOLLOWING a fan-out call
        // over the same arrays: a heap range registered, unregistered and then copied from as pageable memory.  With the
        // query in front the same soak has run clean since round 3; why that is enough is still not established.)
        if (host_range_locked(p, bytes)) return true;
        if (hipHostRegister(const_cast<void *>(p), bytes, hipHostRegisterPortable) == hipSuccess) {
            *slot = const_cast<void *>(p);
            return true;
        }
        (void)hipGetLastError();
        return false;
    }
    ~HostPin() {
        for (void *p : {a, b})
            if (p && hipHostUnregister(p) != hipSuccess) {
                (void)hipGetLastError();
                fprintf(stderr, "libpcx_hip: hipHostUnregister(%p) failed -- the range stays page-locked\n", p);
            }
    }
};

// Several host threads may copy between ONE pageable allocation and their devices only when that allocation is
// page-locked as a whole.  From pageable memory the runtime page-locks each copy's range on the fly, rounded to pages;
// two threads working on adjacent row blocks then share the boundary page, and a copy that found the neighbour's
// lock went on past its end: a GPU memory access fault in the middle of the caller's result array (found by
// tools/soak.py --pin, round 3: barycentric value, 2^19 rows over two handles).  So the fan-out runs only over
// page-locked arrays: `pin` registers them for the call; when that is declined or fails, the whole batch goes
// through the first handle.
static bool fanout_arrays_locked(HostPin &hp, int pin, const void *in, size_t in_bytes, void *out, size_t out_bytes) {
    if (!pin) return host_range_locked(in, in_bytes) && host_range_locked(out, out_bytes);
    const bool ok_in = hp.pin(in, in_bytes, &hp.a);
    const bool ok_out = hp.pin(out, out_bytes, &hp.b);
    static const bool log = getenv("PCX_FANOUT_LOG") != nullptr;
    if (log && !(ok_in && ok_out))
        fprintf(stderr, "[pcx] fan-out: could not page-lock the caller's arrays (points %d, results %d): one handle takes the batch\n",
                (int)ok_in, (int)ok_out);
    return ok_in && ok_out;
}

template <typename Fn>
static int fan_out(int n_handles, int64_t N, Fn &&block_call) {
    const int64_t per = (N + n_handles - 1) / n_handles;
    std::vector<int> rcs(n_handles, PCX_OK);
    std::vector<std::string> errs(n_handles);
    std::vector<std::thread> th;
    for (int g = 0; g < n_handles; ++g) {
        const int64_t lo = std::min<int64_t>(N, (int64_t)g * per), hi = std::min<int64_t>(N, lo + per);
        if (hi <= lo) continue;
        th.emplace_back([&, g, lo, hi] {
            rcs[g] = block_call(g, lo, hi - lo);
            if (rcs[g]) errs[g] = pcx_err_buf();    // the buffer is thread-local: carry the message to the caller's thread
        });
    }
    for (auto &t : th) t.join();
    for (int g = 0; g < n_handles; ++g)
        if (rcs[g]) return fail(rcs[g], "device block %d: %s", g, errs[g].c_str());
    return PCX_OK;
}

// The tail of the *_group_eval_* entry points, after each has validated its handles: row blocks over the handles when the
// caller's arrays are page-locked (fanout_arrays_locked), else the whole batch through handle 0.  eval(g, lo, cnt)
// evaluates rows [lo, lo + cnt) on handle g.
template <typename Fn>
static int fan_out_host(int n_handles, int device0, int pin, int64_t N, const void *in, size_t in_bytes, void *out,
                        size_t out_bytes, Fn &&eval) {
    if (n_handles == 1 || N == 0) return eval(0, (int64_t)0, N);
    HostPin hp;
    HIP_TRY(hipSetDevice(device0));
    if (!fanout_arrays_locked(hp, pin, in, in_bytes, out, out_bytes)) return eval(0, (int64_t)0, N);
    return fan_out(n_handles, N, eval);
}

// pcx_tt.hip: what pcx_calculus.hip reads of a tensor-train handle (its device, shape and domain by storage position,
// and its stream)
PCX_HIDDEN int tt_handle_view(pcx_tt *h, int *device, TTDims *dims, hipStream_t *stream);

// pcx_tt.hip: what pcx_tt_box.hip, _deriv, _grad and _ladder read of a tensor-train handle -- its plan (tt_plan.h), the
// lane-per-point image and table when the handle holds them (d_lpp_img != NULL), else the plain cores, and the mutex and
// staging buffers their entry points share with pcx_tt_eval_batch.  The pointers live as long as the handle.
struct TTPlan;
struct TTBoxView {
    int device;
    hipStream_t stream;
    const TTPlan *plan;
    const double *d_lpp_img;
    const TTLppDim *d_lpp_tab;   // [d]
    const double *d_cores;
    double **d_rinv;             // the handle's table of 1 / j (NULL until the wave-per-row box kernel first runs); freed with the handle
    std::mutex *mu;
    HostStage *stage;
};
PCX_HIDDEN int tt_box_view(pcx_tt *h, TTBoxView *v);
