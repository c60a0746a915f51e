#pragma once
// sbe_unit.hip.h -- what the host code of the side units shares (every .hip file that includes this header: each an opaque
// handle type of its own behind a C header of its own): the handle's common members, error reporting, the HIP check,
// create, destroy, device buffers that only grow, launches in grid chunks, the row store's lanes and its piece loop, the
// bit store with the host checks of a sample store's shape and bytes, the timed region of a compute call and the copies back.  Host code only and nothing of the engine: a unit that includes
// this header compiles no kernels but its own (the device side is sbe_unit_device.hip.h, taken from here for its launch
// limit).  sbe_engine_internal.hip.h takes HIPCHK and div_up from here.  The helpers live in an unnamed namespace, as the
// engine's do: every unit compiles its own copy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <vector>

#include "sbe_unit_device.hip.h"
#include "../../include/sbe_engine.h"

// What every unit's handle starts with.  The unit's struct derives from it and adds `std::vector<void*> buffers() const`,
// the device pointers it owns (null ones included).
struct sbe_unit_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};       // around the kernels of the unit's last compute call
    float last_kernel_ms = 0.0f;
    std::string last_error;
};

// the message of a unit's last failed call without a handle (sbe_<unit>_last_error(NULL)): one object per handle type
template <class H>
inline thread_local std::string g_unit_error;

namespace {

// Records a printf-style message in the handle, if there is one, and in its unit's g_unit_error; returns `code`.  The
// pointer's static type names the unit: a call without a handle passes a typed null (the unit's kNoHandle).
template <class H>
int fail(H* h, int code, const char* fmt, ...) {
    using Unit = std::remove_const_t<H>;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_unit_error<Unit> = buf;
    if (h) const_cast<Unit*>(h)->last_error = buf;
    return code;
}

// (a macro: the message names the failing call and its place)
#define HIPCHK(h, call)                                                                                    \
    do {                                                                                                   \
        hipError_t _err = (call);                                                                          \
        if (_err != hipSuccess)                                                                            \
            return fail(h, SBE_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_err), __FILE__, __LINE__); \
    } while (0)

// `text`: the unit's wording for a null handle
#define CHECK_HANDLE(h, text) \
    if (!(h)) return fail(h, SBE_ERR_ARG, "%s", text)

inline int div_up(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

template <class H>
const char* unit_last_error(const H* h) { return h ? h->last_error.c_str() : g_unit_error<H>.c_str(); }

template <class H>
int unit_last_kernel_ms(const H* h, float* ms_out, const char* null_text) {
    CHECK_HANDLE(h, null_text);
    if (!ms_out) return fail(h, SBE_ERR_ARG, "null pointer argument: ms_out");
    *ms_out = h->last_kernel_ms;
    return SBE_OK;
}

// the handle and everything it holds (the caller has made the handle's device current)
template <class H>
void unit_free(H* h) {
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (void* p : h->buffers())
        if (p) (void)hipFree(p);
    for (hipEvent_t ev : h->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

template <class H>
int unit_destroy(H* h, const char* null_text) {
    CHECK_HANDLE(h, null_text);
    (void)hipSetDevice(h->device);
    unit_free(h);
    return SBE_OK;
}

// A create that fails at a HIP call: the caller gets no handle, so the message goes to the unit's g_unit_error alone, and
// the handle is freed with what it holds so far.  `who`: "sbe_<unit>_create"; `shape`: the unit's own end of the message.
template <class H>
int unit_create_failed(H* h, const char* who, const char* what, hipError_t err, const char* shape) {
    fail((H*)nullptr, SBE_ERR_HIP, "%s: %s failed: %s%s", who, what, hipGetErrorString(err), shape);
    unit_free(h);
    return SBE_ERR_HIP;
}

// The device part of a create, after the unit's own argument checks: is there a GPU and is `device` one, then a new
// handle on it with its stream and events in `h`.  The unit's allocations follow (on failure: unit_create_failed).
template <class H>
int unit_open(H*& h, int device, const char* who, const char* shape) {
    constexpr H* none = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return fail(none, SBE_ERR_NODEVICE, "no usable GPU (hipGetDeviceCount reports none); there is no CPU fallback");
    if (device >= count) return fail(none, SBE_ERR_ARG, "device %d out of range [0,%d)", device, count);
    H* made = new H();
    made->device = device;
    hipError_t err;
    if ((err = hipSetDevice(device)) != hipSuccess) return unit_create_failed(made, who, "hipSetDevice", err, shape);
    if ((err = hipStreamCreateWithFlags(&made->stream, hipStreamNonBlocking)) != hipSuccess)
        return unit_create_failed(made, who, "hipStreamCreate", err, shape);
    for (hipEvent_t& ev : made->ev)
        if ((err = hipEventCreate(&ev)) != hipSuccess) return unit_create_failed(made, who, "hipEventCreate", err, shape);
    h = made;
    return SBE_OK;
}

// The whole body of a create that takes only a device.  `who`: "sbe_<unit>_create".
template <class H>
int unit_create_on_device(H** out, int device, const char* who) {
    constexpr H* none = nullptr;
    if (!out) return fail(none, SBE_ERR_ARG, "null pointer argument: out");
    *out = nullptr;
    if (device < 0) return fail(none, SBE_ERR_ARG, "device %d out of range", device);
    return unit_open(*out, device, who, "");
}

// A device buffer that only grows: afterwards p holds at least `want` bytes (what it held before is not kept).  A failure
// leaves p null and `have` 0, so the next call tries again.
template <class H, class T>
int unit_ensure(H* h, T*& p, size_t& have, size_t want) {
    if (have >= want) return SBE_OK;
    if (p) HIPCHK(h, hipFree(p));
    p = nullptr;
    have = 0;
    HIPCHK(h, hipMalloc((void**)&p, want));
    have = want;
    return SBE_OK;
}

// ... one whose size never changes: allocated on first use
template <class H, class T>
int unit_ensure(H* h, T*& p, size_t bytes) {
    size_t have = p ? bytes : 0;
    return unit_ensure(h, p, have, bytes);
}

// fn(first, count) for consecutive chunks of [0, total) with count <= kMaxGridBlocks (one launch each, `first` its offset);
// returns the first non-zero code
template <class Fn>
int unit_for_grid_chunks(int64_t total, Fn fn) {
    for (int64_t first = 0; first < total; first += kMaxGridBlocks) {
        const int rc = fn(first, std::min(kMaxGridBlocks, total - first));
        if (rc) return rc;
    }
    return SBE_OK;
}

// ---- the row store: host rows go to the device in pieces through a staging buffer -------------------------------------
constexpr int64_t kStageBytes = (int64_t)64 << 20;    // host rows are moved in pieces of at most 64 MiB

// rows per piece: at most kStageBytes, at most the store's capacity, at least one row
inline int64_t unit_piece_rows(int64_t row_bytes, int64_t cap) {
    return std::max<int64_t>(1, std::min<int64_t>(cap, kStageBytes / row_bytes));
}

// n_rows > 0 host rows of row_bytes each into a store of `cap` rows: per piece the copy into `stage` (grown to one piece),
// the unit's launch(piece rows, row offset of the piece within `rows`) and a wait for the stream
template <class H, class Launch>
int unit_append_pieces(H* h, void*& stage, size_t& stage_bytes, const void* rows, int64_t n_rows, int64_t row_bytes, int64_t cap,
                       Launch launch) {
    const int64_t piece = unit_piece_rows(row_bytes, cap);
    int rc = unit_ensure(h, stage, stage_bytes, (size_t)piece * (size_t)row_bytes);
    for (int64_t r = 0; !rc && r < n_rows; r += piece) {
        const int64_t k = std::min(piece, n_rows - r);
        HIPCHK(h, hipMemcpyAsync(stage, (const char*)rows + r * row_bytes, (size_t)k * (size_t)row_bytes, hipMemcpyHostToDevice, h->stream));
        if ((rc = launch(k, r))) break;
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return rc;
}

// The lanes of a row store (the chains of sbe_diag, the runs of sbe_align): rows held per lane and the capacity of each.
// No lane: the store has no shape yet.  `noun` names a lane in the messages, `reset`: the call that shapes the store.
struct unit_lanes {
    std::vector<int64_t> rows;
    int64_t cap = 0;
    int count() const { return (int)rows.size(); }

    template <class H>
    int check_shaped(H* h, const char* reset) const {
        return rows.empty() ? fail(h, SBE_ERR_STATE, "the store has no shape yet (%s)", reset) : SBE_OK;
    }
    // <prefix>_rows
    template <class H>
    int get(H* h, const char* noun, int lane, int64_t* n_rows_out) const {
        if (!n_rows_out) return fail(h, SBE_ERR_ARG, "null pointer argument: n_rows_out");
        if (lane < 0 || lane >= count()) return fail(h, SBE_ERR_ARG, "%s %d out of range [0,%d)", noun, lane, count());
        *n_rows_out = rows[(size_t)lane];
        return SBE_OK;
    }
    // the argument checks of <prefix>_append_rows
    template <class H>
    int check_append(H* h, const char* noun, const char* reset, int lane, const void* src, int64_t n_rows) const {
        if (const int rc = check_shaped(h, reset)) return rc;
        if (lane < 0 || lane >= count()) return fail(h, SBE_ERR_ARG, "%s %d out of range [0,%d)", noun, lane, count());
        if (n_rows < 0) return fail(h, SBE_ERR_ARG, "n_rows=%lld is negative", (long long)n_rows);
        if (n_rows > 0 && !src) return fail(h, SBE_ERR_ARG, "null pointer argument: rows");
        if (rows[(size_t)lane] + n_rows > cap)
            return fail(h, SBE_ERR_ARG, "store overflow: %s %d holds %lld rows, %lld more exceed the capacity of %lld rows", noun, lane,
                        (long long)rows[(size_t)lane], (long long)n_rows, (long long)cap);
        return SBE_OK;
    }
};

// the most a unit's bit store may be shaped to; objects_why: the unit's reason for max_objects, in parentheses
struct unit_store_limits {
    int max_runs, max_clusters;
    int64_t max_objects, max_rows, max_bytes;
    const char* objects_why;
};

// A bit store: runs of cluster samples, host rows [n][K][N] of 0 / 1 bytes, held as bit words [runs][cap][K][W] with
// W = ceil(N / 32).  A unit's handle derives from it beside sbe_unit_handle and lists d_bits and d_stage in its buffers().
struct unit_bit_store {
    unit_lanes runs;                    // (empty: no shape yet)
    int K = 0;
    int64_t N = 0, W = 0;
    uint32_t* d_bits = nullptr;         // [runs][cap][K][W]
    size_t bits_bytes = 0;
    void* d_stage = nullptr;            // host rows in flight
    size_t stage_bytes = 0;
    static constexpr int kPackBlock = 256;

    // d_bits for a shape; set_shape follows once the unit's other allocations stand
    template <class H>
    int alloc_bits(H* h, int n_runs, int n_clusters, int64_t n_objects, int64_t cap) {
        return unit_ensure(h, d_bits, bits_bytes, (size_t)n_runs * (size_t)cap * (size_t)n_clusters * (size_t)((n_objects + 31) / 32) * sizeof(uint32_t));
    }
    void set_shape(int n_runs, int n_clusters, int64_t n_objects, int64_t cap) {
        K = n_clusters;
        N = n_objects;
        W = (n_objects + 31) / 32;
        runs.cap = cap;
        runs.rows.assign((size_t)n_runs, 0);
    }
    uint32_t* at(int run, int64_t row) const { return d_bits + ((int64_t)run * runs.cap + row) * K * W; }

    // The range checks of <prefix>_reset against the unit's limits.  report = false records no message: shape_ok, by which
    // <prefix>_image_bytes decides whether there is a size to state
    static bool shape_ok(const unit_store_limits& lim, int n_runs, int n_clusters, int64_t n_objects, int64_t cap) {
        return check_shape((sbe_unit_handle*)nullptr, lim, n_runs, n_clusters, n_objects, cap, false) == SBE_OK;
    }
    template <class H>
    static int check_shape(H* h, const unit_store_limits& lim, int n_runs, int n_clusters, int64_t n_objects, int64_t cap, bool report = true) {
        auto refuse = [&](const char* fmt, auto... a) { return report ? fail(h, SBE_ERR_ARG, fmt, a...) : (int)SBE_ERR_ARG; };
        if (n_runs < 1 || n_runs > lim.max_runs) return refuse("n_runs=%d out of range [1, %d]", n_runs, lim.max_runs);
        if (n_clusters < 1 || n_clusters > lim.max_clusters) return refuse("n_clusters=%d out of range [1, %d]", n_clusters, lim.max_clusters);
        if (n_objects < 1 || n_objects > lim.max_objects)
            return refuse("n_objects=%lld out of range [1, %lld] %s", (long long)n_objects, (long long)lim.max_objects, lim.objects_why);
        if (cap < 1 || cap > lim.max_rows) return refuse("capacity_rows=%lld out of range [1, %lld]", (long long)cap, (long long)lim.max_rows);
        return SBE_OK;
    }
    // ... and of what a shape that passed them takes on the device, `bytes` by the unit's count
    template <class H>
    static int check_device_bytes(H* h, const unit_store_limits& lim, int n_runs, int n_clusters, int64_t n_objects, int64_t cap, int64_t bytes) {
        if (bytes <= lim.max_bytes) return SBE_OK;
        return fail(h, SBE_ERR_ARG, "a store of %d runs x %lld rows x %d clusters x %lld objects takes %lld bytes on the device, the limit is %lld", n_runs,
                    (long long)cap, n_clusters, (long long)n_objects, (long long)bytes, (long long)lim.max_bytes);
    }

    // The samples [s0, s0 + n) of a call's host rows [.][K][N] hold only 0 and 1: else the first other byte, by its place in
    // the call.  (Blocks: the common case is one OR per byte.)
    template <class H>
    int check_binary(H* h, const uint8_t* rows, int64_t s0, int64_t n) const {
        const int64_t row_bytes = (int64_t)K * N, end = (s0 + n) * row_bytes;
        for (int64_t q0 = s0 * row_bytes; q0 < end; q0 += 4096) {
            const int64_t q1 = std::min(end, q0 + 4096);
            uint8_t any = 0;
            for (int64_t q = q0; q < q1; ++q) any |= rows[q];
            if (any <= 1) continue;
            int64_t q = q0;
            while (rows[q] <= 1) ++q;
            return fail(h, SBE_ERR_DATA, "rows[%lld][%lld][%lld]=%d is neither 0 nor 1", (long long)(q / row_bytes), (long long)(q % row_bytes / N),
                        (long long)(q % N), (int)rows[q]);
        }
        return SBE_OK;
    }

    // The whole of <prefix>_append_rows: the argument checks, the handle's device, the pieces.
    template <class H, class Hook>
    int append(H* h, const char* noun, const char* reset, int run, const uint8_t* rows, int64_t n_rows, Hook before_piece) {
        const int rc = runs.check_append(h, noun, reset, run, rows, n_rows);
        if (rc || n_rows == 0) return rc;
        HIPCHK(h, hipSetDevice(h->device));
        return append_pieces(h, run, rows, n_rows, before_piece);
    }

    // ... its device part, for a unit that has work of its own between the two: the arguments have passed check_append,
    // n_rows > 0 and the handle's device is current.  Per piece of the host rows the unit's before_piece(piece rows, the row
    // of the run where the piece goes) -- the store changes from there on, and a non-zero code ends the call -- and the pack
    // kernel; the run's row count moves once every piece is in.  What a failed piece leaves behind is the unit's to say.
    template <class H, class Hook>
    int append_pieces(H* h, int run, const uint8_t* rows, int64_t n_rows, Hook before_piece) {
        const int64_t have = runs.rows[(size_t)run];
        const int rc = unit_append_pieces(h, d_stage, stage_bytes, rows, n_rows, (int64_t)K * N, runs.cap, [&](int64_t k, int64_t r) {
            if (const int hooked = before_piece(k, have + r)) return hooked;
            const int64_t lines = k * K;
            uint32_t* out = at(run, have + r);
            return unit_for_grid_chunks(lines, [&](int64_t l0, int64_t n) {
                k_unit_pack_bits<kPackBlock><<<dim3((unsigned)n, (unsigned)div_up(N, kPackBlock)), kPackBlock, 0, h->stream>>>((const uint8_t*)d_stage, lines,
                                                                                                                             (int)N, (int)W, out, l0);
                HIPCHK(h, hipGetLastError());
                return SBE_OK;
            });
        });
        if (rc) return rc;
        runs.rows[(size_t)run] = have + n_rows;
        return SBE_OK;
    }
};

// ---- a compute call: the launches between the handle's two events, the copies back, then the wait -----------------------
template <class H, class Fn>
int unit_timed(H* h, Fn launches) {
    HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
    if (const int rc = launches()) return rc;
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    return SBE_OK;
}

// outs[q] <- d[q * n .. (q + 1) * n), on the handle's stream
template <class H, class T>
int unit_copy_back(H* h, const T* d, size_t n, std::initializer_list<T*> outs) {
    for (T* out : outs) {
        HIPCHK(h, hipMemcpyAsync(out, d, n * sizeof(T), hipMemcpyDeviceToHost, h->stream));
        d += n;
    }
    return SBE_OK;
}

// the wait for the stream (the copies back have arrived), then last_kernel_ms from the events
template <class H>
int unit_sync_timed(H* h) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipEventElapsedTime(&h->last_kernel_ms, h->ev[0], h->ev[1]));
    return SBE_OK;
}

}  // namespace
