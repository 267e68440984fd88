// What the C-ABI units (hhuff_capi.hip and hhuff_capi_{blocks,string,host,multi}.hip) share: the error string and the
// return codes made from it, the per-thread device context, the argument checks several call families make, the
// pinned-pointer query, the connection map of a stateful call, the slot-layout launch of either direction and the
// handle of the resident per-string service.  Host code only: no unit gets a kernel or a device variable from here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <mutex>

#include "hhuff.h"
#include "hhuff_hostplan.h"
#include "hhuff_launch.h"
#include "hhuff_slots.h"

#define HHUFF_API extern "C" __attribute__((visibility("default")))

namespace hhuff {

extern thread_local char t_err[256];  // hhuff_last_error_string(); defined in hhuff_capi.hip

inline int hip_fail(hipError_t e, const char* where) {
    snprintf(t_err, sizeof(t_err), "%s: %s (%d)", where, hipGetErrorString(e), (int)e);
    return HHUFF_EHIP;
}

inline int arg_fail(const char* what) {
    snprintf(t_err, sizeof(t_err), "invalid argument: %s", what);
    return HHUFF_EINVAL;
}

// a call's return code from its last HIP call
inline int hip_rc(hipError_t e, const char* where) { return e == hipSuccess ? HHUFF_OK : hip_fail(e, where); }

#define HIP_TRY(call, where)                         \
    do {                                             \
        hipError_t e_ = (call);                      \
        if (e_ != hipSuccess) return hip_fail(e_, where); \
    } while (0)

// Per-thread device context: a stream on the chosen device plus growable device / pinned buffers.
// bind() never changes the calling thread's current device for good: the per-string symbols run on the
// thread's current device (h2o's worker threads may have set one), the host batch calls on their `device`
// argument with the caller's current device restored on return (DeviceGuard).
struct Ctx {
    int dev = -1;
    hipStream_t stream = nullptr;
    uint8_t* d = nullptr;
    size_t dcap = 0;
    uint8_t* h = nullptr;  // pinned, device-visible (the per-string kernel reads and writes it in place)
    size_t hcap = 0;
    ~Ctx() {
        // thread exit: release what this thread allocated (ignore errors at process teardown); a one-string
        // kernel whose result was taken early (wait_one) may still be retiring
        if (stream) (void)hipStreamSynchronize(stream);
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        if (stream) (void)hipStreamDestroy(stream);
    }
    // make `device` (-1: the thread's current device) this context's device; the caller's current device is
    // the one left current (the stream of a device can be used with another device current)
    int bind(int device) {
        int cur = 0;
        HIP_TRY(hipGetDevice(&cur), "hipGetDevice");
        if (device < 0) device = cur;
        if (dev != device) {
            if (stream) (void)hipStreamSynchronize(stream);
            if (d) (void)hipFree(d), d = nullptr, dcap = 0;
            if (h) (void)hipHostFree(h), h = nullptr, hcap = 0;
            if (stream) (void)hipStreamDestroy(stream), stream = nullptr;
            if (device != cur) HIP_TRY(hipSetDevice(device), "hipSetDevice");
            const hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
            if (device != cur) (void)hipSetDevice(cur);
            if (e != hipSuccess) return hip_fail(e, "hipStreamCreate");
            dev = device;
        }
        return HHUFF_OK;
    }
    int reserve(size_t dneed, size_t hneed) {
        if (dneed > dcap) {
            if (d) (void)hipFree(d), d = nullptr, dcap = 0;
            size_t cap = dneed < (1u << 20) ? (1u << 20) : dneed + dneed / 4;
            HIP_TRY(hipMalloc(&d, cap), "hipMalloc");
            dcap = cap;
        }
        if (hneed > hcap) {
            if (h) (void)hipStreamSynchronize(stream), (void)hipHostFree(h), h = nullptr, hcap = 0;  // (wait_one)
            size_t cap = hneed < (1u << 16) ? (1u << 16) : hneed + hneed / 4;
            // coherent (fine-grained): the per-string kernel reads and writes it in place across PCIe
            HIP_TRY(hipHostMalloc(&h, cap, hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc");
            hcap = cap;
        }
        return HHUFF_OK;
    }
};
// defined in hhuff_capi.hip.  A plain extern: a unit reaches it through the thread-local wrapper, which costs the
// per-string C caller nothing measurable
extern thread_local Ctx t_ctx;

// Makes `device` current for the scope of a host batch call, restoring the caller's device on exit.
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (device >= 0 && device != prev) err = hipSetDevice(device);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// p is not a multiple of `bytes` (a power of two); NULL is aligned
inline bool misaligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

inline int check_batch(const uint8_t* in, const uint32_t* in_off, uint32_t n, const uint8_t* out, const uint32_t* out_len) {
    if (n == 0) return HHUFF_OK;
    if (!in || !in_off || !out || !out_len) return arg_fail("NULL array");
    if (misaligned(in, 16)) return arg_fail("`in` must be 16-byte aligned");
    if (misaligned(out, 16)) return arg_fail("`out` must be 16-byte aligned");
    if (n > 0xFFFFFFFEu) return arg_fail("n too large");
    return HHUFF_OK;
}

// a host-array or multi-device batch call lacks one of its arrays (an encode may go without status)
inline bool null_array(bool decode, const void* in, const void* in_off, const void* out, const void* out_len, const void* status) {
    return !in || !in_off || !out || !out_len || (decode && !status);
}

// the contiguous layout with implicit output slots (hhuff_hostplan.h implicit_refusal; in_end = in_off[n]), checked
// before any device call
inline int check_implicit(bool decode, uint64_t in_size, uint64_t in_end, uint64_t out_size) {
    const char* bad = implicit_refusal(decode, in_size, in_end, out_size);
    return bad ? arg_fail(bad) : HHUFF_OK;
}

// The device address of a caller's host array the device can reach (pinned or registered); NULL for a NULL, a
// pageable or a device pointer.
inline void* pinned_dev_ptr(const void* p) {
    if (!p) return nullptr;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return a.type == hipMemoryTypeHost ? a.devicePointer : nullptr;
}

// The slot-layout launch of either direction: in_size and sel_bytes as launch_decode / launch_encode take them
// (hhuff_launch.h), in_len and out_off NULL for the contiguous layout; an encode takes no names and may go
// without status.
inline hipError_t launch_slots(bool decode, const uint8_t* in, uint64_t in_size, const uint32_t* in_off, const uint32_t* in_len,
                               uint32_t n, const uint32_t* names, uint8_t* out, const uint32_t* out_off, uint32_t* out_len,
                               uint8_t* status, hipStream_t stream, uint64_t sel_bytes = 0) {
    return decode ? hhuff::launch_decode(in, in_size, in_off, in_len, n, names, out, out_off, out_len, status, stream, sel_bytes)
                  : hhuff::launch_encode(in, in_size, in_off, in_len, n, out, out_off, out_len, status, stream, sel_bytes);
}

// A stateful call's connection map (include/hhuff.h (2h)): made on the call's stream before its kernels,
// released behind them.  Without slots it holds nothing and launches nothing.
struct ConnMap {
    uint32_t* cmap = nullptr;
    hipStream_t stream;
    explicit ConnMap(hipStream_t s) : stream(s) {}
    hipError_t make(const hhuff_conn_slots_t* slots, uint32_t nconn) {
        return hhuff::conn_map_make(slots, nconn, stream, &cmap);
    }
    ~ConnMap() {
        if (cmap) (void)hipFreeAsync(cmap, stream);
    }
};
// the end of every stateful call: make the map, hand it to the call struct, launch(call, stream), release the map
template <class Call, class Launch>
int launch_mapped(const hhuff_conn_slots_t* slots, Call& call, void* stream, Launch launch, const char* where) {
    ConnMap map((hipStream_t)stream);
    const hipError_t e = map.make(slots, call.nconn);
    if (e != hipSuccess) return hip_fail(e, "connection slots");
    call.cmap = map.cmap;
    return hip_rc(launch(call, (hipStream_t)stream), where);
}

// The host half of the resident per-string service (hhuff_capi_string.hip), one per device.
struct Service {
    std::mutex mu;
    bool ready = false, broken = false;
    hipStream_t stream = nullptr;
    hhuff::SvcSlot* slots = nullptr;  // host view (pinned, mapped, coherent)
    hhuff::SvcSlot* d_slots = nullptr;
    hhuff::SvcCtrl* ctrl = nullptr;
    hhuff::SvcCtrl* d_ctrl = nullptr;
    uint32_t seq[hhuff::kSvcSlots] = {};
    std::mutex slot_mu[hhuff::kSvcSlots];
};
extern Service g_svc[64];  // defined in hhuff_capi_string.hip
// stop a ready service's grid and wait for it; the caller holds S.mu, so no per-string call relaunches it meanwhile
inline void svc_stop(Service& S) {
    __atomic_store_n(&S.ctrl->stop, 1u, __ATOMIC_RELEASE);
    (void)hipStreamSynchronize(S.stream);  // the wave polls stop: it exits within a poll
}

// shard_bounds_kernel (hhuff_capi.hip) for a batch in device memory: the cut of ns <= kMaxDev shards at kShardAlign
// and the byte offsets at the cut, b[0 .. ns] and in_off[b[k]] at b[ns + 1 + k]; b: device-visible host memory
constexpr int kMaxDev = 64;
hipError_t launch_shard_bounds(const uint32_t* in_off, uint32_t n, uint32_t ns, uint32_t* b, hipStream_t stream);

// the chunked host pipeline (hhuff_capi_host.hip); hhuff_capi_multi.hip runs a shard of host arrays through it
int pipelined(bool decode, const uint8_t* in, uint64_t in_size, const uint32_t* in_off, uint32_t n,
              const uint32_t* is_name_bits, uint8_t* out, uint64_t out_size, uint32_t* out_len, uint8_t* status,
              int device, uint64_t chunk_bytes);

}  // namespace hhuff
