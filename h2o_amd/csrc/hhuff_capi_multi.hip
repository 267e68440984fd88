// ---------------------------------------------------------------------------------------------------
// (3d) multi-device batch: one batch over several GPUs of this process (include/hhuff.h (3d)).  Offsets stay
// absolute, so a shard is just a sub-range of in_off with `in` / `out` (and, for a shard copied to another
// device, its scratch shifted back by the shard's base) -- the same addressing as the chunked host pipeline.
// ---------------------------------------------------------------------------------------------------
#include <stdlib.h>
#include <string.h>

#include <condition_variable>
#include <functional>
#include <string>
#include <thread>

#include "hhuff_host.h"

using namespace hhuff;

namespace {

// HHUFF_MULTI_COPY=1: shards on the source device go through the copy path too (a device-to-device copy there):
// the peer path's addressing, tested on a one-GPU box
bool force_copy() {
    const char* v = getenv("HHUFF_MULTI_COPY");  // read per call (tests switch it within one process)
    return v && v[0] == '1';
}

int check_devices(int ndev, const int* devices, int* dv) {
    if (ndev < 1 || ndev > kMaxDev) return arg_fail("ndev must be in [1, 64]");
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count), "hipGetDeviceCount");
    for (int k = 0; k < ndev; ++k) {
        dv[k] = devices ? devices[k] : k;
        if (dv[k] < 0 || dv[k] >= count) return arg_fail("device id out of range");
    }
    return HHUFF_OK;
}

// host arrays: one persistent library thread per device (its thread-local stream, scratch and pinned staging
// persist across calls), each running its shard through the host path
struct DevWorker {
    std::mutex mu;
    std::condition_variable cv;
    std::function<void()> job;
    bool has = false, done = false;
    DevWorker() {
        std::thread([this] {
            for (;;) {
                std::function<void()> j;
                {
                    std::unique_lock<std::mutex> l(mu);
                    cv.wait(l, [this] { return has; });
                    j = std::move(job);
                    has = false;
                }
                j();
                {
                    std::lock_guard<std::mutex> l(mu);
                    done = true;
                }
                cv.notify_all();
            }
        }).detach();
    }
    void post(std::function<void()> f) {
        {
            std::lock_guard<std::mutex> l(mu);
            job = std::move(f);
            has = true;
            done = false;
        }
        cv.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> l(mu);
        cv.wait(l, [this] { return done; });
    }
};
std::mutex g_multi_mu;                       // one multi-device host call at a time (each uses every device)
DevWorker* g_workers[kMaxDev] = {};          // created on first use, never destroyed (detached threads)

int multi_host(bool decode, int ndev, const int* dv, const uint8_t* in, uint64_t in_size, const uint32_t* in_off,
               uint32_t n, const uint32_t* names, uint8_t* out, uint64_t out_size, uint32_t* out_len, uint8_t* status) {
    const int bad = check_implicit(decode, in_size, in_off[n], out_size);
    if (bad) return bad;
    std::vector<uint32_t> b(ndev + 1);
    for (int k = 0; k <= ndev; ++k) b[k] = shard_bound(in_off, n, (uint32_t)k, (uint32_t)ndev, kShardAlign);
    std::lock_guard<std::mutex> g(g_multi_mu);
    std::vector<int> rc(ndev, HHUFF_OK);
    std::vector<std::string> err(ndev);
    std::vector<int> posted;
    for (int k = 0; k < ndev; ++k) {
        const uint32_t lo = b[k], m = b[k + 1] - b[k];
        if (m == 0) continue;
        DevWorker*& w = g_workers[k];
        if (!w) w = new DevWorker();
        const int dev = dv[k];
        w->post([=, &rc, &err] {
            rc[k] = pipelined(decode, in, in_size, in_off + lo, m, names ? names + lo / 32 : nullptr, out, out_size,
                              out_len + lo, status ? status + lo : nullptr, dev, 0);
            if (rc[k]) err[k] = t_err;
        });
        posted.push_back(k);
    }
    for (int k : posted) g_workers[k]->wait();
    for (int k = 0; k < ndev; ++k)
        if (rc[k]) {
            snprintf(t_err, sizeof(t_err), "shard %d (device %d): %s", k, dv[k], err[k].c_str());
            return rc[k];
        }
    return HHUFF_OK;
}

// device arrays on src: per calling thread, one stream per device and the mapped words the cut comes back in
struct MultiCtx {
    hipStream_t s[kMaxDev] = {};
    uint32_t* hb = nullptr;  // mapped host memory: 2 (kMaxDev + 1) words
    bool peer[kMaxDev][kMaxDev] = {};
    ~MultiCtx() {
        for (auto& x : s)
            if (x) (void)hipStreamDestroy(x);
        if (hb) (void)hipHostFree(hb);
    }
};
thread_local MultiCtx t_multi;

int multi_device(bool decode, int ndev, const int* dv, int src, const uint8_t* in, uint64_t in_size,
                 const uint32_t* in_off, uint32_t n, const uint32_t* names, uint8_t* out, uint64_t out_size,
                 uint32_t* out_len, uint8_t* status, hipStream_t stream) {
    DeviceGuard guard(src);
    if (guard.err != hipSuccess) return hip_fail(guard.err, "hipSetDevice");
    MultiCtx& X = t_multi;
    if (!X.hb) HIP_TRY(hipHostMalloc(&X.hb, 8 * (kMaxDev + 1), hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc");
    uint32_t* d_hb = nullptr;
    HIP_TRY(hipHostGetDevicePointer((void**)&d_hb, X.hb, 0), "hipHostGetDevicePointer");
    HIP_TRY(launch_shard_bounds(in_off, n, (uint32_t)ndev, d_hb, stream), "shard bounds launch");
    HIP_TRY(hipStreamSynchronize(stream), "sync (the cut)");
    uint32_t b[kMaxDev + 1], boff[kMaxDev + 1];  // (ndev <= kMaxDev: check_devices)
    memcpy(b, X.hb, ((size_t)ndev + 1) * 4);
    memcpy(boff, X.hb + ndev + 1, ((size_t)ndev + 1) * 4);
    if (const int bad = check_implicit(decode, in_size, boff[ndev], out_size)) return bad;
    hipEvent_t ready;
    HIP_TRY(hipEventCreateWithFlags(&ready, hipEventDisableTiming), "hipEventCreate");
    std::vector<hipEvent_t> fin;
    int rc = HHUFF_OK;
    auto fail = [&](hipError_t e, const char* where) {
        if (rc == HHUFF_OK) rc = hip_fail(e, where);
    };
    hipError_t e = hipEventRecord(ready, stream);
    if (e != hipSuccess) fail(e, "hipEventRecord");
    for (int k = 0; k < ndev && rc == HHUFF_OK; ++k) {
        const uint32_t lo = b[k], m = b[k + 1] - b[k];
        if (m == 0) continue;
        const int dev = dv[k];
        const uint64_t s0 = boff[k], e0 = boff[k + 1];
        if (dev == src && !force_copy()) {  // in place, on the caller's stream
            e = launch_slots(decode, in, in_size, in_off + lo, nullptr, m, names ? names + lo / 32 : nullptr, out, nullptr,
                             out_len + lo, status ? status + lo : nullptr, stream, e0 - s0);
            if (e != hipSuccess) fail(e, "shard launch (source device)");
            continue;
        }
        if ((e = hipSetDevice(dev)) != hipSuccess) {
            fail(e, "hipSetDevice");
            break;
        }
        if (!X.s[dev] && (e = hipStreamCreateWithFlags(&X.s[dev], hipStreamNonBlocking)) != hipSuccess) {
            fail(e, "hipStreamCreate");
            break;
        }
        if (dev != src && !X.peer[dev][src]) {  // direct xGMI reads / writes of src's memory where the link allows it
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, dev, src) == hipSuccess && can) {
                const hipError_t pe = hipDeviceEnablePeerAccess(src, 0);
                if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) {
                    fail(pe, "hipDeviceEnablePeerAccess");
                    break;
                }
                (void)hipGetLastError();
            }
            X.peer[dev][src] = true;
        }
        hipStream_t ms = X.s[dev];
        // the shard's layout on its device: that of one chunk of the host pipeline (hhuff_hostplan.h ChunkLayout).
        // (ohi: in_off comes from device memory and is not known to ascend, so the range that goes back is held
        // inside `out` here)
        const ChunkLayout L = chunk_layout(decode, s0, e0, m, names != nullptr);
        const uint64_t base = L.base, nbytes = L.nbytes, olo = L.olo, ohi = std::min<uint64_t>(L.ohi, out_size), obase = L.obase;
        const size_t nw = L.nw, o_off = L.o_off, o_nm = L.o_nm, o_out = L.o_out, o_len = L.o_len, o_st = L.o_st;
        uint8_t* d = nullptr;
        if ((e = hipStreamWaitEvent(ms, ready, 0)) != hipSuccess || (e = hhuff::work_alloc((void**)&d, L.need, ms)) != hipSuccess) {
            fail(e, "shard scratch");
            break;
        }
        uint32_t* d_off = reinterpret_cast<uint32_t*>(d + o_off);
        uint32_t* d_nm = nw ? reinterpret_cast<uint32_t*>(d + o_nm) : nullptr;
        uint32_t* d_len = reinterpret_cast<uint32_t*>(d + o_len);
        uint8_t* d_st = d + o_st;
        if ((e = hipMemcpyPeerAsync(d, dev, in + base, src, nbytes, ms)) != hipSuccess ||
            (e = hipMemcpyPeerAsync(d_off, dev, in_off + lo, src, ((size_t)m + 1) * 4, ms)) != hipSuccess ||
            (nw && (e = hipMemcpyPeerAsync(d_nm, dev, names + lo / 32, src, nw * 4, ms)) != hipSuccess)) {
            fail(e, "peer copy in");
            break;
        }
        e = launch_slots(decode, d - base, e0, d_off, nullptr, m, d_nm, d + o_out - obase, nullptr, d_len,
                         status ? d_st : nullptr, ms, e0 - s0);
        if (e != hipSuccess) {
            fail(e, "shard launch (peer device)");
            break;
        }
        if ((ohi > olo && (e = hipMemcpyPeerAsync(out + olo, src, d + o_out + (olo - obase), dev, ohi - olo, ms)) != hipSuccess) ||
            (e = hipMemcpyPeerAsync(out_len + lo, src, d_len, dev, (size_t)m * 4, ms)) != hipSuccess ||
            (status && (e = hipMemcpyPeerAsync(status + lo, src, d_st, dev, m, ms)) != hipSuccess)) {
            fail(e, "peer copy out");
            break;
        }
        if ((e = hipFreeAsync(d, ms)) != hipSuccess) {
            fail(e, "hipFreeAsync");
            break;
        }
        hipEvent_t f;
        if ((e = hipEventCreateWithFlags(&f, hipEventDisableTiming)) != hipSuccess || (e = hipEventRecord(f, ms)) != hipSuccess) {
            fail(e, "hipEventRecord");
            break;
        }
        fin.push_back(f);
    }
    (void)hipSetDevice(src);
    for (hipEvent_t f : fin) {  // the caller's stream goes on once every shard is back
        e = hipStreamWaitEvent(stream, f, 0);
        if (e != hipSuccess) fail(e, "hipStreamWaitEvent");
        (void)hipEventDestroy(f);  // released once it completes
    }
    (void)hipEventDestroy(ready);
    return rc;
}

int batch_multi(bool decode, int ndev, const int* devices, int src, const uint8_t* in, uint64_t in_size,
                const uint32_t* in_off, uint32_t n, const uint32_t* names, uint8_t* out, uint64_t out_size, uint32_t* out_len,
                uint8_t* status, void* stream) {
    int dv[kMaxDev];
    int rc = check_devices(ndev, devices, dv);
    if (rc) return rc;
    if (n == 0) return HHUFF_OK;
    if (null_array(decode, in, in_off, out, out_len, status)) return arg_fail("NULL array");
    if (src == HHUFF_HOST_MEMORY)
        return multi_host(decode, ndev, dv, in, in_size, in_off, n, names, out, out_size, out_len, status);
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count), "hipGetDeviceCount");
    if (src < 0 || src >= count) return arg_fail("src_device out of range");
    return multi_device(decode, ndev, dv, src, in, in_size, in_off, n, names, out, out_size, out_len, status,
                        static_cast<hipStream_t>(stream));
}

}  // namespace

HHUFF_API int hhuff_decode_batch_multi(int ndev, const int* devices, int src_device, const uint8_t* in, uint64_t in_size,
                                       const uint32_t* in_off, uint32_t n, const uint32_t* is_name_bits, uint8_t* out,
                                       uint64_t out_size, uint32_t* out_len, uint8_t* status, void* stream) {
    return batch_multi(true, ndev, devices, src_device, in, in_size, in_off, n, is_name_bits, out, out_size, out_len,
                       status, stream);
}

HHUFF_API int hhuff_encode_batch_multi(int ndev, const int* devices, int src_device, const uint8_t* in, uint64_t in_size,
                                       const uint32_t* in_off, uint32_t n, uint8_t* out, uint64_t out_size, uint32_t* out_len,
                                       uint8_t* status, void* stream) {
    return batch_multi(false, ndev, devices, src_device, in, in_size, in_off, n, nullptr, out, out_size, out_len, status,
                       stream);
}

HHUFF_API int hhuff_shard_bounds(const uint32_t* in_off, uint32_t n, uint32_t nshards, uint32_t align, uint32_t* bounds) {
    if (!in_off || !bounds) return arg_fail("NULL array");
    if (nshards < 1) return arg_fail("nshards must be >= 1");
    for (uint32_t k = 0; k <= nshards; ++k) bounds[k] = shard_bound(in_off, n, k, nshards, align);
    return HHUFF_OK;
}
