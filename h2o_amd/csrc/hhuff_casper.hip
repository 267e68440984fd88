// CASPER on the device (include/hhuff.h (2n), hhuff_casper.h).
//   casper_step_kernel   one wave (a workgroup of 64) per connection; the op list is walked wave-uniformly.
//     The set lives in LDS for the whole list: loaded once behind the header check, stored once at the end if it
//     changed.  Dynamic LDS, sized from max_keys: the set A and a cookie's keys B (max_keys each), then the decoder's
//     buffers, the cookie's bit tile and the hashes.
//     Hashes ahead of the walk: a path's key before masking does not depend on the state, so at every 64th LOOKUP /
//     MARK op the wave looks ahead, lane j takes the j-th such op from there and runs its SHA-1 (bytes by aligned dword
//     loads and shifts, a rolling 16-word schedule: registers only); the walk masks with the capacity_bits current at
//     the op.
//     LOOKUP / MARK: the first key >= k by a bisection over 64-key blocks and one ballot; an insert shifts the tail by
//     lanes from the top, 64 keys a step.
//     CONSUME: name and alphabet by the wave, the Golomb decode by the rounds of hhuff_gcswave.h into B (the count goes
//     on past the room).  The union is rank-based: every key of B finds its rank in A by bisection and the fresh ones
//     are compacted with their final positions (a ballot's prefix count); if they fit, A's keys move up by their rank in
//     the fresh keys, 64 a step from the top, and the fresh keys drop into the gaps.  No serial merge; A is not touched
//     before the fit is known.
//     COOKIE: keys 64 a round, lane i one key: the delta from the neighbour (__shfl_up, the round's carry for lane 0),
//     its bit count (delta >> r) + 1 + r, a wave scan for the bit positions.  A first pass gives the length, so
//     HHUFF_CSP_SPACE is decided before any store.  The second ORs every one-and-remainder (at most two dwords) into a
//     zeroed LDS tile of 3,072 bits = 512 characters -- unary zeros cost nothing, a run longer than a tile leaves whole
//     tiles of 'A' -- and every finished tile is written as base64url, eight characters a lane.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_casper.h"
#include "hhuff_gcswave.h"

#define HHUFF_API extern "C" __attribute__((visibility("default")))

namespace hhuff {
namespace {
using namespace csp;
using gcsw::kWave;
using gcsw::wave_scan;

constexpr uint32_t kTileBits = 3072, kTileWords = kTileBits / 32u, kTileChars = kTileBits / 6u;
constexpr uint32_t kBufWords = (gcsw::kBufBytes + 15u) / 16u * 4u;
constexpr uint32_t kTabBytes = 64u * kWave;  // also the fresh keys' positions: u16 [HHUFF_CSP_MAX_KEYS]
static_assert(2u * HHUFF_CSP_MAX_KEYS <= kTabBytes, "the positions share the decoder's table");
constexpr uint32_t kFixedLds = 8u * gcsw::kStage + kTabBytes + 4u * (kBufWords + kTileWords + 2u * kWave);

struct StepArgs {
    uint8_t* scratch;
    uint32_t nslots, max_keys;
    const uint32_t* slot;
    const uint32_t* ops;  // 4 dwords an op
    const uint32_t* op_first;
    const uint8_t* in;
    uint64_t in_size;
    const uint32_t* value_off;
    const uint32_t* value_len;
    const int32_t* token;
    uint32_t nfslots;
    int32_t cookie_token;
    uint8_t* out;
    const uint32_t* out_off;
    uint32_t* res;  // 4 dwords an op
};

__device__ __forceinline__ uint32_t below(uint64_t m, uint32_t lane) { return (uint32_t)__popcll(m & ((1ull << lane) - 1u)); }

struct Conn {  // every member is wave-uniform
    const StepArgs& G;
    uint32_t lane;
    uint64_t* A;  // the set
    uint64_t* B;  // a cookie's keys
    gcsw::Lds lds;
    uint32_t* tile;
    uint32_t* hkey;  // the round's 64 keys before masking
    uint32_t* hop;   // their ops
    bool valid = false, dirty = false;
    uint32_t cap = 0, rem = 0, na = 0;
    uint32_t wpos = 0, rend = 0;

    // the first index with A[i] >= k, by the wave
    __device__ uint32_t find(uint64_t k) const {
        const uint32_t nblk = (na + kWave - 1u) / kWave;
        uint32_t lo = 0, hi = nblk;  // the first block whose last key is >= k
        while (lo < hi) {
            const uint32_t mid = (lo + hi) / 2u, last = kWave * mid + kWave - 1u;
            if (A[last < na ? last : na - 1u] < k) lo = mid + 1u;
            else hi = mid;
        }
        if (lo == nblk) return na;
        const uint32_t i = kWave * lo + lane;
        const uint64_t m = __ballot(i < na && A[i] >= k);
        const uint32_t end = kWave * lo + kWave < na ? kWave * lo + kWave : na;  // (no bit: only in a damaged set)
        return m ? kWave * lo + (uint32_t)__builtin_ctzll(m) : end;
    }

    // lane j hashes the j-th LOOKUP / MARK op from op o on
    __device__ void hash_round(uint32_t o, uint32_t o1) {
        uint32_t n = 0;
        for (uint32_t ob = o; ob < o1 && n < kWave; ob += kWave) {
            const uint32_t oi = ob + lane;
            const uint32_t kind = oi < o1 ? G.ops[4u * oi] : 0u;
            const bool path = kind == HHUFF_CSP_LOOKUP || kind == HHUFF_CSP_MARK;
            const uint64_t m = __ballot(path);
            const uint32_t j = n + below(m, lane);
            if (path && j < kWave) hop[j] = oi;
            n += (uint32_t)__popcll(m);
        }
        __syncthreads();
        if (lane < n) {
            const uint32_t a = G.ops[4u * hop[lane] + 1u], b = G.ops[4u * hop[lane] + 2u];
            if ((uint64_t)a + b <= G.in_size) hkey[lane] = path_key(gcsw::DevChunks{G.in}, a, b);
        }
        __syncthreads();
    }

    __device__ int32_t lookup(uint32_t h, bool set, uint32_t* value) {
        const uint64_t k = h & ((1u << cap) - 1u);
        const uint32_t p = find(k);
        if (p < na && A[p] == k) {
            *value = 1;
            return 0;
        }
        if (!set) return 0;
        if (na == G.max_keys) return HHUFF_CSP_SPACE;
        for (uint32_t hi = na; hi > p;) {  // the tail moves up by one, from the top
            const uint32_t lo = hi - p > kWave ? hi - kWave : p, i = lo + lane;
            const uint64_t v = i < hi ? A[i] : 0u;
            __syncthreads();
            if (i < hi) A[i + 1u] = v;
            __syncthreads();
            hi = lo;
        }
        if (lane == 0) A[p] = k;
        __syncthreads();
        ++na, dirty = true;
        return 0;
    }

    __device__ int32_t consume(uint64_t off, uint64_t len, uint32_t* value) {
        if (off + len > G.in_size) return HHUFF_CSP_EINVAL;
        if (len <= kNameLen) return 0;
        if (__ballot(lane < kNameLen && G.in[off + lane] != name_byte(lane))) return 0;
        uint32_t unused;
        uint64_t nb;
        uint64_t* const Bk = B;
        const uint32_t room = G.max_keys;
        // (a key whose successor reaches 2^63 drops the cookie)
        if (!gcsw::decode<false>(G.in, off + kNameLen, len - kNameLen, lane, lds, rem, kSat - 1u, &unused, &nb, [=](uint64_t i, uint64_t k) {
                if (i < room) Bk[i] = k;
            }))
            return 0;
        __syncthreads();
        if (nb > ((1ull << cap) > 128u ? 1ull << cap : 128u)) return 0;
        *value += (uint32_t)nb;
        if (nb > room) return HHUFF_CSP_SPACE;
        // ranks in A; the fresh keys are compacted in B with their final positions
        uint16_t* const pos16 = reinterpret_cast<uint16_t*>(lds.tab);
        uint32_t nf = 0;
        for (uint32_t j0 = 0; j0 < (uint32_t)nb; j0 += kWave) {
            const uint32_t j = j0 + lane;
            const bool has = j < (uint32_t)nb;
            const uint64_t b = has ? B[j] : 0u;
            const uint32_t ra = has ? lower_bound(A, na, b) : 0u;
            const bool fresh = has && !(ra < na && A[ra] == b);
            const uint64_t m = __ballot(fresh);
            const uint32_t idx = nf + below(m, lane);
            __syncthreads();
            if (fresh) B[idx] = b, pos16[idx] = (uint16_t)(ra + idx);
            __syncthreads();
            nf += (uint32_t)__popcll(m);
        }
        if (na + nf > room) return HHUFF_CSP_SPACE;
        if (nf == 0) return 0;
        for (uint32_t hi = na; hi > 0;) {  // A's keys move up by their rank in the fresh keys, from the top
            const uint32_t lo = hi > kWave ? hi - kWave : 0u, i = lo + lane;
            const uint64_t v = i < hi ? A[i] : 0u;
            const uint32_t t = i < hi ? i + lower_bound(B, nf, v) : 0u;
            __syncthreads();
            if (i < hi) A[t] = v;
            __syncthreads();
            hi = lo;
        }
        for (uint32_t j = lane; j < nf; j += kWave) A[pos16[j]] = B[j];
        __syncthreads();
        na += nf, dirty = true;
        return 0;
    }

    __device__ int32_t consume_fields(uint32_t a, uint32_t b, uint32_t* value) {
        if (!G.value_off || !G.value_len || !G.token || (uint64_t)a + b > G.nfslots) return HHUFF_CSP_EINVAL;
        const uint64_t s1 = (uint64_t)a + b;
        for (uint64_t sb = a; sb < s1; sb += kWave) {
            const uint64_t s = sb + lane;
            for (uint64_t m = __ballot(s < s1 && G.token[s] == G.cookie_token); m; m &= m - 1u) {
                const uint64_t v = sb + (uint32_t)__builtin_ctzll(m);
                const int32_t st = consume(G.value_off[v], G.value_len[v], value);
                if (st != 0) return st;
            }
        }
        return 0;
    }

    // one round of the encoder: lane i's key of A[r0 ..), its bits, and the inclusive scan of the bit counts
    struct Round {
        bool has;
        uint64_t delta, bits, inc;
    };
    __device__ Round round(uint32_t r0, uint64_t* next_min) const {
        Round r;
        const uint32_t i = r0 + lane;
        r.has = i < na;
        const uint64_t k = r.has ? A[i] : 0u, up = __shfl_up(k, 1u);
        r.delta = k - (lane == 0 ? *next_min : up + 1u);
        r.bits = r.has ? sat_add(r.delta >> rem, 1u + rem) : 0u;
        r.inc = wave_scan(r.bits, lane, [](uint64_t a, uint64_t b) { return sat_add(a, b); });
        *next_min = __shfl(k, (int)(na - r0 < kWave ? na - r0 - 1u : kWave - 1u)) + 1u;
        return r;
    }

    // `count` characters of the tile to dst, eight a lane
    __device__ void flush(uint8_t* dst, uint32_t count) const {
        __syncthreads();
        if (8u * lane < count) {
            const uint32_t d = 3u * lane / 2u, sh = (lane & 1u) * 16u;
            const uint64_t x = (((uint64_t)tile[d] << 32 | tile[d + 1u]) << sh) >> 16;  // 48 bits
            uint64_t pack = 0;
#pragma unroll
            for (uint32_t i = 0; i < 8u; ++i) pack |= (uint64_t)b64url_char((uint32_t)(x >> (42u - 6u * i)) & 63u) << (8u * i);
            uint8_t* p = dst + 8u * lane;
            const uint32_t n = count - 8u * lane;
            if (n >= 8u && ((uintptr_t)p & 7u) == 0) *reinterpret_cast<uint64_t*>(p) = pack;
            else
                for (uint32_t i = 0; i < 8u && i < n; ++i) p[i] = (uint8_t)(pack >> (8u * i));
        }
        __syncthreads();
        for (uint32_t i = lane; i < kTileWords; i += kWave) tile[i] = 0;
        __syncthreads();
    }

    __device__ int32_t cookie(uint32_t* value) {
        if (na == 0) return 0;
        uint64_t total = 0, next_min = 0;
        for (uint32_t r0 = 0; r0 < na; r0 += kWave) total = sat_add(total, __shfl(round(r0, &next_min).inc, (int)(kWave - 1u)));
        const uint64_t len = cookie_length(total);
        if (len > rend - wpos) return HHUFF_CSP_SPACE;
        const uint32_t nchars = (uint32_t)len - kNameLen - kAttrLen;
        uint8_t* const dst = G.out + wpos + kNameLen;
        if (lane < kNameLen) G.out[wpos + lane] = name_byte(lane);
        if (lane < kAttrLen) dst[nchars + lane] = attr_byte(lane);
        for (uint32_t i = lane; i < kTileWords; i += kWave) tile[i] = 0;
        __syncthreads();
        uint64_t pos = 0, T = 0;  // the round's first bit; the tile being filled
        next_min = 0;
        for (uint32_t r0 = 0; r0 < na; r0 += kWave) {
            const Round r = round(r0, &next_min);
            // the one and the remainder, MSB first from bit s: the upper dword at s / 32, the lower behind it
            const uint64_t s = pos + r.inc - (1u + rem);
            const uint64_t piece = (1ull << rem | (r.delta & ((1ull << rem) - 1u))) << (63u - rem) >> (s & 31u);
            const uint64_t end = pos + __shfl(r.inc, (int)(kWave - 1u));
            for (;;) {
                const uint64_t d = s / 32u - T * kTileWords;  // (wraps below the tile)
                if (r.has && d < kTileWords) atomicOr(&tile[d], (uint32_t)(piece >> 32));
                if (r.has && d + 1u < kTileWords && (uint32_t)piece) atomicOr(&tile[d + 1u], (uint32_t)piece);
                if (end < (T + 1u) * kTileBits) break;
                flush(dst + T * kTileChars, kTileChars);  // every bit of the tile is known
                ++T;
            }
            pos = end;
        }
        if (nchars > T * kTileChars) flush(dst + T * kTileChars, nchars - (uint32_t)(T * kTileChars));
        wpos += (uint32_t)len, *value = (uint32_t)len;
        return 0;
    }
};

__global__ __launch_bounds__(kWave) void casper_step_kernel(StepArgs G) {
    extern __shared__ uint64_t lds64[];
    const uint32_t c = blockIdx.x, lane = threadIdx.x, mk = G.max_keys;
    uint64_t* const stage = lds64 + 2u * mk;
    uint8_t* const tab = reinterpret_cast<uint8_t*>(stage + gcsw::kStage);
    uint32_t* const buf = reinterpret_cast<uint32_t*>(tab + kTabBytes);
    Conn K{G, lane, lds64, lds64 + mk, {buf, tab, stage}, buf + kBufWords, buf + kBufWords + kTileWords, buf + kBufWords + kTileWords + kWave};
    const uint32_t o0 = G.op_first[c], o1 = G.op_first[c + 1u];
    const uint32_t s = G.slot ? G.slot[c] : c;
    const bool bad_slot = s >= G.nslots;
    uint8_t* const slab = G.scratch + (bad_slot ? 0u : s * slab_bytes(mk));
    uint64_t* const keys = reinterpret_cast<uint64_t*>(slab + kHeaderBytes);
    if (!bad_slot) {
        const uint32_t* h = reinterpret_cast<const uint32_t*>(slab);
        K.valid = header_ok(h[0], h[1], h[2], h[3], mk);
        if (K.valid) {
            K.cap = (h[1] >> 16) & 0xFFu, K.rem = h[1] >> 24, K.na = h[2];
            for (uint32_t i = lane; i < K.na; i += kWave) K.A[i] = keys[i];
        }
    }
    K.wpos = G.out_off[c], K.rend = G.out_off[c + 1u] > K.wpos ? G.out_off[c + 1u] : K.wpos;
    __syncthreads();
    uint32_t npath = 0;
    for (uint32_t o = o0; o < o1; ++o) {
        const uint32_t kind = G.ops[4u * o], a = G.ops[4u * o + 1u], b = G.ops[4u * o + 2u];
        const bool path = kind == HHUFF_CSP_LOOKUP || kind == HHUFF_CSP_MARK, fields = kind == HHUFF_CSP_CONSUME_FIELDS;
        if (path && npath++ % kWave == 0) K.hash_round(o, o1);
        int32_t st = 0;
        uint32_t value = 0, at = 0;
        if (bad_slot || G.ops[4u * o + 3u] != 0 || kind < HHUFF_CSP_INIT || kind > HHUFF_CSP_COOKIE) st = HHUFF_CSP_EINVAL;
        else if (kind == HHUFF_CSP_INIT) {
            if (a < 1u || a > 30u || b > 31u) st = HHUFF_CSP_EINVAL;
            else K.valid = K.dirty = true, K.cap = a, K.rem = b, K.na = 0;
        } else if (!K.valid) st = HHUFF_CSP_EFORMAT;
        else if (kind == HHUFF_CSP_CONSUME) st = K.consume(a, b, &value);
        else if (fields) st = K.consume_fields(a, b, &value);
        else if (path) st = (uint64_t)a + b > G.in_size ? HHUFF_CSP_EINVAL : K.lookup(K.hkey[(npath - 1u) % kWave], kind == HHUFF_CSP_MARK, &value);
        else at = K.wpos, st = K.cookie(&value);
        if (st != 0 && !(st == HHUFF_CSP_SPACE && (kind == HHUFF_CSP_CONSUME || fields))) value = 0;
        if (lane == 0) {
            uint32_t* r = G.res + 4u * o;
            r[0] = (uint32_t)st, r[1] = value, r[2] = K.valid && !bad_slot ? K.na : 0u, r[3] = at;
        }
    }
    if (K.valid && K.dirty && !bad_slot) {
        __syncthreads();
        for (uint32_t i = lane; i < K.na; i += kWave) keys[i] = K.A[i];
        if (lane == 0) {
            uint32_t* h = reinterpret_cast<uint32_t*>(slab);
            h[0] = kMagic, h[1] = header_word1(K.cap, K.rem), h[2] = K.na, h[3] = mk;
        }
    }
}
}  // namespace
}  // namespace hhuff

HHUFF_API int hhuff_casper_step(void* scratch, uint32_t nslots, uint32_t max_keys, const uint32_t* slot, const hhuff_casper_op_t* ops,
                                const uint32_t* op_first, uint32_t nconn, const uint8_t* in, uint64_t in_size,
                                const uint32_t* value_off, const uint32_t* value_len, const int32_t* token, uint32_t nfslots,
                                int32_t cookie_token, uint8_t* out, const uint32_t* out_off, hhuff_casper_result_t* res, void* stream) {
    if (nconn == 0) return HHUFF_OK;
    if (!scratch || !ops || !op_first || !in || !out || !out_off || !res || ((uintptr_t)scratch & 15u) != 0 || max_keys == 0 ||
        max_keys > HHUFF_CSP_MAX_KEYS)
        return HHUFF_EINVAL;
    const hhuff::StepArgs A{(uint8_t*)scratch, nslots, max_keys, slot, reinterpret_cast<const uint32_t*>(ops), op_first, in, in_size,
                            value_off, value_len, token, nfslots, cookie_token, out, out_off, reinterpret_cast<uint32_t*>(res)};
    const uint32_t lds = 16u * max_keys + hhuff::kFixedLds;
    hipLaunchKernelGGL(hhuff::casper_step_kernel, dim3(nconn), dim3(hhuff::kWave), lds, (hipStream_t)stream, A);
    return hipGetLastError() == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}
