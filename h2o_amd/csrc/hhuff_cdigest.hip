// Cache digests on the device (include/hhuff.h (2m), hhuff_cdigest.h).
//   cd_load_kernel<FIELDS>   one wave (a workgroup of 64) per request.  The element / attribute walk of hhuff_cdigest.h
//                      runs wave-uniform: every lane holds the same iterator and only runs of plain bytes are skipped
//                      64 at a time by a ballot.  A digest is checked (alphabet, tail) by the whole wave, then decoded in
//                      rounds of 4,096 bits:
//                        a. the round's 512 bytes and 8 of look-ahead are decoded from base64 into LDS, a quad a lane;
//                        b. lane L takes bits 64 L .. 64 L + 63 as a window, MSB first, so clz finds the next 1;
//                        c. every lane fills its window's table entry offset -> offset at which the search enters the
//                           next window (a backward pass over its 64 offsets, in LDS: a terminator at t hands the search
//                           to t + pbits + 1 <= 95, so the exit is below 32 and the table composes window by window);
//                        d. the wave follows the chain through the 64 tables (64 dependent LDS reads, every lane reads
//                           the same byte) and lane L keeps the offset at which the search enters its window;
//                        e. every lane walks the terminators of its window: q from the distance to the search position
//                           before (the round's carry or the nearest earlier lane's, by a max scan, for its first one),
//                           the remainder from its and its neighbour's window; key counts and sums of q << pbits | r
//                           plus one are prefix-summed over the wave (saturating, so the drop decision key >= 2^capacity_bits
//                           is exact at any length), and a second walk puts the keys into an LDS stage that is
//                           stored 64 lanes x 8 bytes at a time.
//                      The search position, the running minimum and the key count carry into the next round; an unfinished
//                      unary run is just a search position that lies rounds back.  The frame header is written when the
//                      digest is complete and fits (append only: a dropped digest leaves the write position alone).
//   cd_lookup_kernel   one lane per query: the segments' bytes by aligned dword loads and shifts into SHA-256's
//                      16-word window (registers; no LDS, no scratch), then the checked frame walk with a bisection
//                      a frame.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_cdigest.h"

#define HHUFF_API extern "C" __attribute__((visibility("default")))

namespace hhuff {
namespace {
using namespace cd;

constexpr uint32_t kWave = 64;
constexpr uint32_t kRoundBits = 4096, kRoundBytes = kRoundBits / 8u;
constexpr uint32_t kBufBytes = kRoundBytes + 8u;  // a remainder of up to 31 bits behind bit 4095, and lane 63's neighbour
constexpr uint32_t kStage = 512;                  // keys an LDS stage holds: a round has at most 4,096, commonly a few hundred
constexpr uint32_t kNone = 0xFFFFFFFFu;

struct LoadArgs {
    const uint8_t* in;
    uint64_t in_size;
    const uint32_t* val_off;
    const uint32_t* val_len;
    const uint32_t* first;
    const uint32_t* nfields;  // FIELDS
    const int32_t* token;     // FIELDS
    int32_t want;             // FIELDS
    uint32_t nslots;          // FIELDS
    uint8_t* dig;
    const uint64_t* dig_off;
    int32_t* status;
};

struct DevSrc {
    const uint8_t* in;
    uint32_t lane;
    __device__ __forceinline__ uint8_t byte(uint64_t i) const { return in[i]; }
    // called by the whole wave with equal arguments
    __device__ __forceinline__ uint64_t skip_plain(uint64_t cur, uint64_t end) const {
        for (; cur < end; cur += kWave) {
            bool stop = true;  // (a lane at or past the end stops the run)
            if (cur + lane < end) {
                const uint8_t c = in[cur + lane];
                stop = c == ' ' || c == '\t' || c == ';' || c == ',' || c == '=';
            }
            const uint64_t m = __ballot(stop);
            if (m) return cur + (uint32_t)__builtin_ctzll(m);
        }
        return end;
    }
};

template <class T, class Op>
__device__ __forceinline__ T wave_scan(T v, uint32_t lane, Op op) {  // inclusive
#pragma unroll
    for (uint32_t d = 1; d < kWave; d <<= 1) {
        const T o = __shfl_up(v, d);
        if (lane >= d) v = op(o, v);
    }
    return v;
}

// The terminators of one window from entry offset e on: f(q, r) for every complete value, q counted from the search
// position inside the window (the caller adds what lies before the window to the first).  Returns the search position
// behind the last terminator, relative to the window, or kNone without one.
template <class F>
__device__ __forceinline__ uint32_t walk(uint64_t w, uint64_t wn, uint32_t e, uint32_t pbits, uint64_t base, uint64_t nbits, F&& f) {
    uint32_t p = e;
    bool any = false;
    while (p < 64u) {
        const uint64_t m = w & (~0ull >> p);
        if (!m) break;
        const uint32_t t = (uint32_t)__builtin_clzll(m), s = t + 1u;
        any = true;
        const uint32_t q = t - p;
        p = s + pbits;
        if (base + t + pbits >= nbits) break;  // the remainder is cut short: no key, and nothing behind it
        const uint64_t x = s == 64u ? wn : (w << s) | (wn >> (64u - s));
        f(q, pbits ? x >> (64u - pbits) : 0ull);
    }
    return any ? p : kNone;
}

struct WaveSink {
    const uint8_t* in;
    uint8_t* img;
    uint64_t size;
    uint32_t lane;
    uint32_t* buf;    // kBufBytes
    uint8_t* tab;     // [64 offsets][64 lanes]
    uint64_t* stage;  // kStage
    uint64_t pos = kHeaderBytes;
    uint32_t nframes = 0, flags = 0;
    int32_t status = 0;

    __device__ __forceinline__ void reset() { pos = kHeaderBytes, nframes = 0, flags = 0; }
    __device__ __forceinline__ bool stopped() const { return status != 0; }
    __device__ __forceinline__ uint64_t be64(uint32_t word) const {
        return (uint64_t)__builtin_bswap32(buf[word]) << 32 | __builtin_bswap32(buf[word + 1u]);
    }

    __device__ void digest(uint64_t start, uint64_t c, bool validators, bool complete) {
        if (c % 4u == 1u) return;
        bool ok = true;
        for (uint64_t i = lane; i < c; i += kWave) ok = ok && b64_val(in[start + i]) != 0xFFu;
        if (__ballot(!ok)) return;
        const uint64_t nbytes = c * 3u / 4u, nbits = 8u * nbytes;
        if (nbits < 10u) return;
        const bool head = size >= pos + kFrameBytes;
        uint64_t* const keys = reinterpret_cast<uint64_t*>(img + (head ? pos + kFrameBytes : 0u));
        const uint64_t room = head ? (size - pos - kFrameBytes) / 8u : 0u;  // keys are stored while they fit
        uint32_t pbits = 0, cap = 0;
        uint64_t limit = 0, p_in = 10, next_min = 0, nkeys = 0;
        uint8_t* const bytes = reinterpret_cast<uint8_t*>(buf);
        for (uint64_t R = 0; R < nbits && p_in < nbits; R += kRoundBits) {
            // a. base64 -> the round's bytes (zeros behind the digest's last byte)
            const uint64_t byte0 = R / 8u;
            __syncthreads();
            for (uint64_t j = byte0 / 3u + lane; 3u * j < byte0 + kBufBytes; j += kWave) {
                uint32_t v = 0;
#pragma unroll
                for (uint32_t i = 0; i < 4u; ++i) v = v << 6 | (4u * j + i < c ? b64_val(in[start + 4u * j + i]) : 0u);
#pragma unroll
                for (uint32_t i = 0; i < 3u; ++i) {
                    const uint64_t b = 3u * j + i;
                    if (b >= byte0 && b < byte0 + kBufBytes) bytes[b - byte0] = b < nbytes ? (uint8_t)(v >> (16u - 8u * i)) : (uint8_t)0;
                }
            }
            __syncthreads();
            // b. windows
            const uint64_t w = be64(2u * lane);
            const uint64_t up = __shfl_down(w, 1u);
            const uint64_t wn = lane == kWave - 1u ? be64(2u * kWave) : up;
            if (R == 0) {
                const uint64_t w0 = __shfl(w, 0);
                pbits = (uint32_t)(w0 >> 54) & 31u, cap = ((uint32_t)(w0 >> 59) & 31u) + pbits, limit = 1ull << cap;
            }
            // c. the window's table
            uint32_t x = 0;
            for (int e = 63; e >= 0; --e) {
                if ((w >> (63 - e)) & 1u) {
                    const uint32_t nxt = (uint32_t)e + pbits + 1u;
                    x = nxt >= 64u ? nxt - 64u : tab[nxt * kWave + lane];
                }
                tab[(uint32_t)e * kWave + lane] = (uint8_t)x;
            }
            __syncthreads();
            // d. the chain through the windows
            uint32_t e = p_in > R ? (uint32_t)(p_in - R) : 0u, mine = 0;  // (p_in - R < 32)
            for (uint32_t L = 0; L < kWave; ++L) {
                if (lane == L) mine = e;
                e = tab[e * kWave + L];
            }
            // e. values: first walk, counts and sums
            const uint64_t base = R + 64u * lane;
            uint32_t cnt = 0;
            uint64_t sum = 0;
            const uint32_t pe = walk(w, wn, mine, pbits, base, nbits, [&](uint32_t q, uint64_t r) {
                ++cnt, sum = sat_add(sum, sat_add(sat_value(q, r, pbits), 1u));
            });
            const uint64_t lastp = wave_scan(pe == kNone ? 0ull : base + pe, lane, [](uint64_t a, uint64_t b) { return a > b ? a : b; });
            uint64_t before = __shfl_up(lastp, 1u);
            before = lane == 0 || before < p_in ? p_in : before;          // the search position in front of this window's first
            const uint64_t qfix = sat_shl(base + mine - before, pbits);  // what its unary run holds outside the window
            if (cnt) sum = sat_add(sum, qfix);
            const uint32_t cinc = wave_scan(cnt, lane, [](uint32_t a, uint32_t b) { return a + b; });
            const uint64_t sinc = wave_scan(sum, lane, [](uint64_t a, uint64_t b) { return sat_add(a, b); });
            const uint32_t total = (uint32_t)__shfl((int)cinc, (int)(kWave - 1u));
            const uint64_t next_out = sat_add(next_min, __shfl(sinc, (int)(kWave - 1u)));
            if (total != 0 && next_out - 1u >= limit) return;  // the round's last key: the digest is dropped
            uint64_t sbefore = __shfl_up(sinc, 1u);
            sbefore = lane == 0 ? 0ull : sbefore;
            // second walk: the keys, through the stage
            for (uint32_t s0 = 0; s0 < total; s0 += kStage) {
                uint32_t idx = cinc - cnt - s0;  // (wraps below the stage's start: not stored)
                uint64_t run = sat_add(next_min, sbefore), fix = qfix;
                walk(w, wn, mine, pbits, base, nbits, [&](uint32_t q, uint64_t r) {
                    const uint64_t key = sat_add(run, sat_add(sat_value(q, r, pbits), fix));
                    if (idx < kStage) stage[idx] = key;
                    run = key + 1u, fix = 0, ++idx;
                });
                __syncthreads();
                const uint32_t n = total - s0 < kStage ? total - s0 : kStage;
                for (uint32_t j = lane; j < n; j += kWave)
                    if (nkeys + s0 + j < room) keys[nkeys + s0 + j] = stage[j];
                __syncthreads();
            }
            nkeys += total, next_min = next_out;
            const uint64_t plast = __shfl(lastp, (int)(kWave - 1u));
            p_in = plast > p_in ? plast : p_in;
        }
        if (nkeys > 0xFFFFFFFFull || pos + kFrameBytes + 8u * nkeys > size) {
            status = HHUFF_CD_SPACE;
            return;
        }
        if (lane == 0) {
            uint32_t* f = reinterpret_cast<uint32_t*>(img + pos);
            f[0] = cap | (validators ? 1u : 0u) << 8, f[1] = (uint32_t)nkeys, f[2] = 0, f[3] = 0;
        }
        pos += kFrameBytes + 8u * nkeys, ++nframes, flags = kPresent | (complete ? kComplete : 0u);
    }
};

template <bool FIELDS>
__global__ __launch_bounds__(kWave) void cd_load_kernel(LoadArgs A) {
    __shared__ uint32_t buf[kBufBytes / 4u];
    __shared__ uint8_t tab[64u * kWave];
    __shared__ uint64_t stage[kStage];
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    const uint64_t d0 = A.dig_off[r], d1 = A.dig_off[r + 1u];
    if ((d0 & 15u) != 0 || d1 < d0) {  // no region to write to
        if (lane == 0) A.status[r] = HHUFF_CD_EINVAL;
        return;
    }
    const uint64_t size = d1 - d0 < 0xFFFFFFF0ull ? d1 - d0 : 0xFFFFFFF0ull;  // (`bytes` is a u32)
    const DevSrc S{A.in, lane};
    WaveSink K{A.in, A.dig + d0, size, lane, buf, tab, stage};
    uint32_t s0 = A.first[r], s1 = FIELDS ? A.nfields[r] : A.first[r + 1u];
    if (FIELDS) s1 = (uint64_t)s0 + s1 < A.nslots ? s0 + s1 : A.nslots;
    for (uint64_t sb = s0; sb < s1 && !K.stopped(); sb += kWave) {
        const uint64_t s = sb + lane;
        uint64_t m = __ballot(s < s1 && (!FIELDS || A.token[s] == A.want));
        for (; m && !K.stopped(); m &= m - 1u) {
            const uint64_t v = sb + (uint32_t)__builtin_ctzll(m);
            const uint64_t off = A.val_off[v], len = A.val_len[v];
            if (off + len > A.in_size) K.status = HHUFF_CD_EINVAL;
            else load_value(S, off, len, K);
        }
    }
    if (K.status != 0) K.reset();
    if (lane == 0) {
        A.status[r] = size < kHeaderBytes && K.status == 0 ? HHUFF_CD_SPACE : K.status;
        if (size >= kHeaderBytes) {
            uint32_t* h = reinterpret_cast<uint32_t*>(K.img);
            h[0] = kMagic, h[1] = kVersion | K.flags << 16, h[2] = K.nframes, h[3] = (uint32_t)K.pos;
        }
    }
}

// ---- lookup ----
constexpr uint32_t kLookupThreads = 256;

struct LookupArgs {
    const uint8_t* dig;
    const uint64_t* dig_off;
    uint32_t nreq;
    const uint8_t* in;
    uint64_t in_size;
    const uint32_t* queries;  // 12 dwords a query
    uint32_t nq;
    int32_t* state;
    uint64_t* hash_out;
};

struct DevChunks {  // the aligned dword that holds in[pos], from that byte on
    const uint8_t* in;
    __device__ __forceinline__ uint32_t chunk(uint64_t pos, uint32_t rem, uint32_t* k) const {
        const uintptr_t a = (uintptr_t)(in + pos);
        const uint32_t r = (uint32_t)(a & 3u), n = 4u - r < rem ? 4u - r : rem;
        const uint32_t d = *reinterpret_cast<const uint32_t*>(a - r);
        *k = n;
        return (__builtin_bswap32(d) << (8u * r)) & (0xFFFFFFFFu << (32u - 8u * n));
    }
};

struct DevImage {
    const uint32_t* p;
    __device__ __forceinline__ uint32_t word(uint64_t i) const { return p[i]; }
    __device__ __forceinline__ uint64_t key(uint64_t i) const { return reinterpret_cast<const uint64_t*>(p)[i]; }
};

__global__ __launch_bounds__(kLookupThreads) void cd_lookup_kernel(LookupArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * kLookupThreads + threadIdx.x;
    if (i >= A.nq) return;
    const uint32_t* q = A.queries + 12u * i;
    const uint32_t req = q[0], qflags = q[1];
    bool ok = req < A.nreq && (qflags & ~HHUFF_CDQ_ETAG) == 0;
    for (uint32_t k = 0; k < 5u; ++k) ok = ok && (q[7u + k] == 0 || (uint64_t)q[2u + k] + q[7u + k] <= A.in_size);
    if (!ok) {
        A.state[i] = HHUFF_CD_EINVAL;
        return;
    }
    const DevChunks S{A.in};
    SegWords<DevChunks> M(S, q + 2, q + 7);
    const uint64_t hash = sha256_first8(M, M.nwords / 16u);
    if (A.hash_out) A.hash_out[i] = hash;
    const uint64_t d0 = A.dig_off[req], d1 = A.dig_off[req + 1u];
    int32_t st = HHUFF_CD_EFORMAT;
    if ((d0 & 15u) == 0 && d1 >= d0) st = lookup(DevImage{reinterpret_cast<const uint32_t*>(A.dig + d0)}, d1 - d0, qflags & 1u, hash);
    A.state[i] = st;
}

hipError_t launch_load(const LoadArgs& A, uint32_t n, bool fields, hipStream_t stream) {
    if (fields) hipLaunchKernelGGL(cd_load_kernel<true>, dim3(n), dim3(kWave), 0, stream, A);
    else hipLaunchKernelGGL(cd_load_kernel<false>, dim3(n), dim3(kWave), 0, stream, A);
    return hipGetLastError();
}
}  // namespace
}  // namespace hhuff

HHUFF_API int hhuff_cache_digests_load(const uint8_t* in, uint64_t in_size, const uint32_t* val_off, const uint32_t* val_len,
                                       const uint32_t* first, uint32_t nreq, uint8_t* dig, const uint64_t* dig_off,
                                       int32_t* status, void* stream) {
    if (nreq == 0) return HHUFF_OK;
    if (!in || !val_off || !val_len || !first || !dig || !dig_off || !status || ((uintptr_t)dig & 15u) != 0) return HHUFF_EINVAL;
    hhuff::LoadArgs A{};
    A.in = in, A.in_size = in_size, A.val_off = val_off, A.val_len = val_len, A.first = first;
    A.dig = dig, A.dig_off = dig_off, A.status = status;
    return hhuff::launch_load(A, nreq, false, (hipStream_t)stream) == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}

HHUFF_API int hhuff_cache_digests_load_fields(const uint8_t* arena, uint64_t arena_size, const uint32_t* value_off,
                                              const uint32_t* value_len, const uint32_t* first, const uint32_t* nfields,
                                              uint32_t nblk, uint32_t nslots, const int32_t* token, int32_t cache_digest_token,
                                              uint8_t* dig, const uint64_t* dig_off, int32_t* status, void* stream) {
    if (nblk == 0) return HHUFF_OK;
    if (!arena || !value_off || !value_len || !first || !nfields || !token || !dig || !dig_off || !status ||
        ((uintptr_t)dig & 15u) != 0)
        return HHUFF_EINVAL;
    hhuff::LoadArgs A{};
    A.in = arena, A.in_size = arena_size, A.val_off = value_off, A.val_len = value_len, A.first = first, A.nfields = nfields;
    A.token = token, A.want = cache_digest_token, A.nslots = nslots, A.dig = dig, A.dig_off = dig_off, A.status = status;
    return hhuff::launch_load(A, nblk, true, (hipStream_t)stream) == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}

HHUFF_API int hhuff_cache_digests_lookup(const uint8_t* dig, const uint64_t* dig_off, uint32_t nreq, const uint8_t* in,
                                         uint64_t in_size, const hhuff_cd_query_t* queries, uint32_t nq, int32_t* state,
                                         uint64_t* hash_out, void* stream) {
    if (nq == 0) return HHUFF_OK;
    if (!dig || !dig_off || !in || !queries || !state || ((uintptr_t)dig & 15u) != 0) return HHUFF_EINVAL;
    hhuff::LookupArgs A{dig, dig_off, nreq, in, in_size, reinterpret_cast<const uint32_t*>(queries), nq, state, hash_out};
    const uint32_t grid = (nq + hhuff::kLookupThreads - 1u) / hhuff::kLookupThreads;
    hipLaunchKernelGGL(hhuff::cd_lookup_kernel, dim3(grid), dim3(hhuff::kLookupThreads), 0, (hipStream_t)stream, A);
    return hipGetLastError() == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}
