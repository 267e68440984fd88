// ---------------------------------------------------------------------------------------------------
// (1) h2o per-string symbols: one string per launch on the thread's stream, synchronously.
// Strings up to kOneMax bytes go through one_string_kernel on a pinned, device-visible buffer
// [u32 len, is_name, result, status][input][output] (no copies: one launch, one synchronisation); longer
// ones through the batch kernels with device copies.  A HIP failure (no GPU, a lost device) never aborts
// the caller: decode returns SIZE_MAX -- h2o's decode_string then reports H2O_HTTP2_ERROR_COMPRESSION for
// that literal (hpack.c:241-242) and the connection closes --, encode returns SIZE_MAX -- every caller then
// emits the string raw (hpack.c:836, qpack.c:1046-1051), which is a correct encoding; the reason is in
// hhuff_last_error_string().
// ---------------------------------------------------------------------------------------------------
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <immintrin.h>

#include "hhuff_host.h"

using namespace hhuff;

Service hhuff::g_svc[64];

namespace {
constexpr size_t kMeta = 32;
#ifndef HHUFF_LONG_ENC_DEFAULT
#define HHUFF_LONG_ENC_DEFAULT 1
#endif
uint64_t g_per_string_calls = 0;  // process-wide, atomic adds (hhuff_per_string_calls)

// ---- the resident per-string service (service_kernel, hhuff_kernels.hip), one grid per device ----
// A call posts its string in its thread's mailbox (slot = thread number mod kSvcSlots, a mutex per slot for
// more threads than slots), raises the slot's request counter and spins on the slot's done counter.  The
// grid has service_waves() waves (default 16), wave g serving mailboxes g, g + G, ..., so calls from up to G
// threads are coded at once.  It exits after kSvcIdle without a request to any wave; a call that finds its
// request unserved and the grid gone (ctrl->alive 0, the service stream idle) launches it again.  atexit stops every service before the HIP
// runtime goes away.  HHUFF_NO_SERVICE=1 in the environment keeps the launch-per-string path.
constexpr uint64_t kSvcIdle = 200000;      // real-time counter ticks (100 MHz): 2 ms without a request
constexpr uint64_t kSvcLife = 1000000000;  // 10 s in all, then a fresh launch
std::atomic<uint32_t> g_svc_threads{0};  // (Service, g_svc: hhuff_host.h -- hhuff_pool_trim stops the grid too)
thread_local int t_svc_slot = -1;

void svc_shutdown() {
    for (auto& S : g_svc) {
        std::lock_guard<std::mutex> g(S.mu);
        if (!S.ready) continue;
        svc_stop(S);
        S.ready = false;
    }
}

bool svc_enabled() {
    static const bool on = [] {
        const char* e = getenv("HHUFF_NO_SERVICE");
        return !(e && *e && *e != '0');
    }();
    return on;
}

// make sure device dev's service is set up and running (stream idle -> launch); caller holds nothing
int svc_kick(Service& S, int dev) {
    std::lock_guard<std::mutex> g(S.mu);
    if (S.broken) return HHUFF_EHIP;
    if (!S.ready) {
        int cur = 0;
        HIP_TRY(hipGetDevice(&cur), "hipGetDevice");
        if (cur != dev) HIP_TRY(hipSetDevice(dev), "hipSetDevice");
        hipError_t e = hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking);
        void* h = nullptr;
        const size_t bytes = sizeof(hhuff::SvcSlot) * hhuff::kSvcSlots + sizeof(hhuff::SvcCtrl);
        if (e == hipSuccess) e = hipHostMalloc(&h, bytes, hipHostMallocMapped | hipHostMallocCoherent);
        void* d = nullptr;
        if (e == hipSuccess) {
            memset(h, 0, bytes);
            e = hipHostGetDevicePointer(&d, h, 0);
        }
        if (cur != dev) (void)hipSetDevice(cur);
        if (e != hipSuccess) {
            S.broken = true;
            return hip_fail(e, "per-string service setup");
        }
        S.slots = static_cast<hhuff::SvcSlot*>(h);
        S.d_slots = static_cast<hhuff::SvcSlot*>(d);
        S.ctrl = reinterpret_cast<hhuff::SvcCtrl*>(S.slots + hhuff::kSvcSlots);
        S.d_ctrl = reinterpret_cast<hhuff::SvcCtrl*>(S.d_slots + hhuff::kSvcSlots);
        static std::once_flag once;
        std::call_once(once, [] { atexit(svc_shutdown); });
        S.ready = true;
    }
    const hipError_t q = hipStreamQuery(S.stream);
    if (q == hipErrorNotReady) return HHUFF_OK;  // running (or starting)
    if (q != hipSuccess) return hip_fail(q, "per-string service query");
    // a fresh grid: no quit, no wave gone yet, alive from the launch on (the stream tells a finished grid)
    for (uint32_t g = 0; g < hhuff::kSvcMaxWaves; ++g) S.ctrl->gone[g] = 0u;
    S.ctrl->quit = 0u;
    S.ctrl->waves = hhuff::service_waves();
    __atomic_store_n(&S.ctrl->stop, 0u, __ATOMIC_RELEASE);
    __atomic_store_n(&S.ctrl->alive, 1u, __ATOMIC_RELEASE);
    const hipError_t e = hhuff::launch_service(S.d_slots, S.d_ctrl, kSvcIdle, kSvcLife, S.stream);
    return hip_rc(e, "per-string service launch");
}

// 1: served (result in *res), 0: not taken (the caller uses the launch path), -1: HIP failure
int svc_call(int dev, bool encode, const uint8_t* src, size_t len, int is_name, uint8_t* dst, uint32_t* res,
             uint32_t* status) {
    if (dev < 0 || dev >= 64 || len > hhuff::kSvcMax || !svc_enabled()) return 0;
    Service& S = g_svc[dev];
    if (S.broken) return 0;
    if (!S.ready && svc_kick(S, dev) != HHUFF_OK) return S.broken ? 0 : -1;
    if (t_svc_slot < 0) t_svc_slot = (int)(g_svc_threads.fetch_add(1) % hhuff::kSvcSlots);
    const int k = t_svc_slot;
    std::lock_guard<std::mutex> g(S.slot_mu[k]);
    hhuff::SvcSlot* sl = S.slots + k;
    const uint32_t n = ++S.seq[k];
    // chunks first, each one 16-B store {n, 12 bytes}; then the header, one 16-B store (see SvcSlot)
    for (size_t i = 0; 12 * i < len; ++i) {
        uint32_t w[4] = {n, 0u, 0u, 0u};
        memcpy(&w[1], src + 12 * i, len - 12 * i < 12 ? len - 12 * i : 12);
        _mm_store_si128(reinterpret_cast<__m128i*>(sl->chunk[i]), _mm_loadu_si128(reinterpret_cast<const __m128i*>(w)));
    }
    __atomic_thread_fence(__ATOMIC_RELEASE);
    const uint32_t h[4] = {n, encode ? 1u : 0u, (uint32_t)len, is_name ? 1u : 0u};
    _mm_store_si128(reinterpret_cast<__m128i*>(&sl->req), _mm_loadu_si128(reinterpret_cast<const __m128i*>(h)));
    // spin for the result.  While the wave is alive nothing else is done; a wave that is gone (idle exit,
    // or exiting just as this request arrived) is launched again -- checked every 64 spins, so a wave that
    // is still starting up is not launched twice (svc_kick sees its stream busy)
    // a grid that is gone is launched again; once the service is broken (another thread's 5-s timeout, a
    // failed setup) this call is not a Huffman error but a request for the launch path
    auto revive = [&]() -> int {
        if (__atomic_load_n(&S.ctrl->alive, __ATOMIC_ACQUIRE) != 0u) return 1;
        if (svc_kick(S, dev) == HHUFF_OK) return 1;
        return S.broken ? 0 : -1;
    };
    if (const int rv = revive(); rv <= 0) return rv;
    uint64_t spins = 0;
    const auto t0 = std::chrono::steady_clock::now();
    // {done, result, status} arrive as one 16-B store: one 16-B load sees them together
    auto load16 = [](const void* q, uint32_t (&w)[4]) {
        __asm__ volatile("" ::: "memory");  // re-read the device-written line on every try
        _mm_storeu_si128(reinterpret_cast<__m128i*>(w), _mm_load_si128(reinterpret_cast<const __m128i*>(q)));
    };
    uint32_t res4[4];
    for (load16(&sl->done, res4); res4[0] != n; load16(&sl->done, res4)) {
        ++spins;
        if ((spins & 63u) == 0u) {
            if (const int rv = revive(); rv <= 0) return rv;
            if ((spins & 4095u) == 0u && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) {
                // a busy device (a long batch kernel ahead of the wave) is not a HIP failure: this call and
                // the later ones take the launch path, so a valid string is still coded
                snprintf(t_err, sizeof(t_err), "per-string service: no answer in 5 s (launch path from now on)");
                std::lock_guard<std::mutex> gg(S.mu);
                S.broken = true;
                return 0;
            }
        }
        __builtin_ia32_pause();
    }
    const uint32_t r = res4[1];
    *res = r;
    *status = res4[2];
    if (r != HHUFF_FAIL_LEN) {
        for (uint32_t i = 0; 12u * i < r; ++i) {  // each chunk once it carries this request's number
            uint32_t c4[4];
            for (uint64_t k = 0;; ++k) {  // stored with the result: here within microseconds
                load16(sl->outc[i], c4);
                if (c4[0] == n) break;
                if ((k & 4095u) == 4095u && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) {
                    snprintf(t_err, sizeof(t_err), "per-string service: output chunk %u never arrived", i);
                    return -1;
                }
                __builtin_ia32_pause();
            }
            memcpy(dst + 12u * i, &c4[1], r - 12u * i < 12u ? r - 12u * i : 12u);
        }
    }
    return 1;
}

// The one-string kernel stores its result length last (system scope, after every output word): spin on it
// instead of waiting for the launch's completion signal, for up to 2 ms, then synchronise the stream as before
// (which also reports a failed launch).  HHUFF_ONE_SYNC=1: always synchronise.
// A result taken early is complete (every output word precedes the length's release store), but an error the
// kernel raises after that store -- nothing in it runs after the store but the exit -- would surface at the
// next synchronisation of this thread's stream, i.e. be reported against the thread's next call.
constexpr uint32_t kOnePending = 0xFFFFFFFEu;  // never a result: lengths stay below 2^16, failures are ~0u
static hipError_t wait_one(Ctx& c, const uint32_t* meta) {
    static const bool sync_only = [] {
        const char* v = getenv("HHUFF_ONE_SYNC");
        return v && v[0] == '1';
    }();
    if (!sync_only) {
        const auto t0 = std::chrono::steady_clock::now();
        for (uint64_t k = 0;; ++k) {
            if (__atomic_load_n(&meta[2], __ATOMIC_ACQUIRE) != kOnePending) return hipSuccess;
            if ((k & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
            __builtin_ia32_pause();
        }
    }
    return hipStreamSynchronize(c.stream);
}

// Per-string encode past kOneMax: one block over the string (encode_long_kernel) with HHUFF_LONG_ENC=1 (or a
// build default of 1), else the batch kernels on a batch of one (one lane: ~8 ms for 64 KB)
static bool long_encode_block() {
    static const bool on = [] {
        const char* v = getenv("HHUFF_LONG_ENC");
        return v ? v[0] != '0' : HHUFF_LONG_ENC_DEFAULT != 0;
    }();
    return on;
}

size_t per_string(bool encode, uint8_t* dst, const uint8_t* src, size_t len, int is_name, unsigned* soft_errors) {
    __atomic_fetch_add(&g_per_string_calls, 1, __ATOMIC_RELAXED);
    Ctx& c = t_ctx;
    if (len > 0x1FFFFFFFu) {
        snprintf(t_err, sizeof(t_err), "string of %zu bytes exceeds the per-string limit", len);
        return SIZE_MAX;
    }
    if (c.bind(-1)) return SIZE_MAX;
    {
        uint32_t r = 0, st = 0;
        const int sv = svc_call(c.dev, encode, src, len, is_name, dst, &r, &st);
        if (sv < 0) return SIZE_MAX;
        if (sv > 0) {
            if (r == HHUFF_FAIL_LEN) return SIZE_MAX;
            if (!encode) *soft_errors |= st & 3u;
            return r;
        }
    }
    const size_t in_cap = up16(len ? len : 1);
    if (len <= hhuff::kOneMax) {
        const size_t out_cap = up16(len * 8 / 5 + 4);
        if (c.reserve(0, 16 + in_cap + out_cap)) return SIZE_MAX;
        uint32_t* meta = reinterpret_cast<uint32_t*>(c.h);
        meta[0] = (uint32_t)len;
        meta[1] = is_name ? 1u : 0u;
        __atomic_store_n(&meta[2], kOnePending, __ATOMIC_RELAXED);
        memcpy(c.h + 16, src, len);
        hipError_t e = hhuff::launch_one(c.h, (uint32_t)len, (uint32_t)in_cap, is_name != 0, encode, c.stream);
        if (e == hipSuccess) e = wait_one(c, meta);
        if (e != hipSuccess) return hip_fail(e, encode ? "encode (one string)" : "decode (one string)"), SIZE_MAX;
        const uint32_t r = __atomic_load_n(&meta[2], __ATOMIC_ACQUIRE);
        if (r == HHUFF_FAIL_LEN) return SIZE_MAX;
        memcpy(dst, c.h + 16 + in_cap, r);
        if (!encode) *soft_errors |= meta[3] & 3u;
        return r;
    }
    // long strings: the batch kernels on a batch of one, device copies
    const size_t out_cap = up16(len * 8 / 5 + 4);
    if (c.reserve(kMeta + in_cap + out_cap, kMeta + in_cap + out_cap)) return SIZE_MAX;
    uint32_t* meta = reinterpret_cast<uint32_t*>(c.h);
    meta[0] = 0;
    meta[1] = (uint32_t)len;
    meta[2] = 0;
    meta[3] = is_name ? 1u : 0u;
    memcpy(c.h + kMeta, src, len);
    uint32_t* d_meta = reinterpret_cast<uint32_t*>(c.d);
    uint8_t* d_in = c.d + kMeta;
    uint8_t* d_out = c.d + kMeta + in_cap;
    uint8_t* h_out = c.h + kMeta + in_cap;
    hipError_t e = hipMemcpyAsync(c.d, c.h, kMeta + len, hipMemcpyHostToDevice, c.stream);
    if (e == hipSuccess)
        e = encode && long_encode_block()
                ? hhuff::launch_encode_long(d_in, (uint32_t)len, d_out, d_meta + 2, c.stream)
                : launch_slots(!encode, d_in, len, d_meta, nullptr, 1, d_meta + 3, d_out, nullptr, d_meta + 2,
                               encode ? nullptr : reinterpret_cast<uint8_t*>(d_meta + 4), c.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c.h, c.d, kMeta, hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_out, d_out, out_cap, hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) return hip_fail(e, encode ? "encode (long string)" : "decode (long string)"), SIZE_MAX;
    const uint32_t r = meta[2];
    if (r == HHUFF_FAIL_LEN) return SIZE_MAX;
    memcpy(dst, h_out, r);
    if (!encode) *soft_errors |= *reinterpret_cast<const uint8_t*>(meta + 4);
    return r;
}
}  // namespace

HHUFF_API size_t h2o_hpack_decode_huffman(char* dst, unsigned* soft_errors, const uint8_t* src, size_t len, int is_name,
                                          const char** err_desc) {
    (void)err_desc;  // never written, as in the reference (hpack.c:142-144 is unreachable)
    return per_string(false, reinterpret_cast<uint8_t*>(dst), src, len, is_name, soft_errors);
}

HHUFF_API size_t h2o_hpack_encode_huffman(uint8_t* dst, const uint8_t* src, size_t len) {
    return per_string(true, dst, src, len, 0, nullptr);
}

HHUFF_API uint64_t hhuff_per_string_calls(void) { return __atomic_load_n(&g_per_string_calls, __ATOMIC_RELAXED); }

HHUFF_API int hhuff_service_stamps(uint32_t* out4) {
    int dev = 0;
    if (!out4 || hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return HHUFF_EINVAL;
    const Service& S = g_svc[dev];
    if (!S.ready || t_svc_slot < 0) return HHUFF_EINVAL;
    const hhuff::SvcSlot* sl = S.slots + t_svc_slot;
    out4[0] = sl->t_seen, out4[1] = sl->t_data, out4[2] = sl->t_coded, out4[3] = sl->t_out;
    return HHUFF_OK;
}
