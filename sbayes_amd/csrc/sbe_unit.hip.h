#pragma once
// sbe_unit.hip.h -- what the host code of the side units shares (sbe_elpd.hip, sbe_em.hip, sbe_assoc.hip, sbe_geo.hip, sbe_diag.hip, sbe_align.hip: each an opaque
// handle type of its own behind a C header of its own): the handle's common members, error reporting, the HIP check, the
// device part of create, destroy, and device buffers that only grow.  Host code only and nothing of the engine: a unit
// that includes this header alone compiles no kernels but its own.  sbe_engine_internal.hip.h takes HIPCHK and div_up
// from here.  The helpers live in an unnamed namespace, as the engine's do: every unit compiles its own copy.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

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

}  // namespace
