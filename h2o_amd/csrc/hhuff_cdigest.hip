// Cache digests on the device (include/hhuff.h (2m), hhuff_cdigest.h).
//   cd_load_kernel<FIELDS>   one wave (a workgroup of 64) per request.  The element / attribute walk of hhuff_cdigest.h
//                      runs wave-uniform: every lane holds the same iterator and only runs of plain bytes are skipped
//                      64 at a time by a ballot.  A digest is checked (alphabet, tail) and decoded by the whole wave
//                      in rounds of 4,096 bits: hhuff_gcswave.h, which the CASPER kernel runs too.  The keys go to the
//                      image 64 lanes x 8 bytes at a time while they fit.  The frame header is written when the
//                      digest is complete and fits (append only: a dropped digest leaves the write position alone).
//   cd_lookup_kernel   one lane per query: the segments' bytes by aligned dword loads and shifts into SHA-256's
//                      16-word window (registers; no LDS, no scratch), then the checked frame walk with a bisection
//                      a frame.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_cdigest.h"
#include "hhuff_gcswave.h"

#define HHUFF_API extern "C" __attribute__((visibility("default")))

namespace hhuff {
namespace {
using namespace cd;

using gcsw::kWave;

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

struct WaveSink {
    const uint8_t* in;
    uint8_t* img;
    uint64_t size;
    uint32_t lane;
    gcsw::Lds lds;
    uint64_t pos = kHeaderBytes;
    uint32_t nframes = 0, flags = 0;
    int32_t status = 0;

    __device__ __forceinline__ void reset() { pos = kHeaderBytes, nframes = 0, flags = 0; }
    __device__ __forceinline__ bool stopped() const { return status != 0; }

    __device__ void digest(uint64_t start, uint64_t c, bool validators, bool complete) {
        const bool head = size >= pos + kFrameBytes;
        uint64_t* const keys = reinterpret_cast<uint64_t*>(img + (head ? pos + kFrameBytes : 0u));
        const uint64_t room = head ? (size - pos - kFrameBytes) / 8u : 0u;  // keys are stored while they fit
        uint32_t cap = 0;
        uint64_t nkeys = 0;
        if (!gcsw::decode<true>(in, start, c, lane, lds, 0u, 0ull, &cap, &nkeys, [&](uint64_t i, uint64_t k) {
                if (i < room) keys[i] = k;
            }))
            return;
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
    __shared__ uint32_t buf[gcsw::kBufBytes / 4u];
    __shared__ uint8_t tab[64u * kWave];
    __shared__ uint64_t stage[gcsw::kStage];
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    const uint64_t d0 = A.dig_off[r], d1 = A.dig_off[r + 1u];
    if ((d0 & 15u) != 0 || d1 < d0) {  // no region to write to
        if (lane == 0) A.status[r] = HHUFF_CD_EINVAL;
        return;
    }
    const uint64_t size = d1 - d0 < 0xFFFFFFF0ull ? d1 - d0 : 0xFFFFFFF0ull;  // (`bytes` is a u32)
    const DevSrc S{A.in, lane};
    WaveSink K{A.in, A.dig + d0, size, lane, {buf, tab, stage}};
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
    const gcsw::DevChunks S{A.in};
    SegWords<gcsw::DevChunks> M(S, q + 2, q + 7);
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
