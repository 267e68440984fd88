// The wave-parallel decoder of Golomb-coded sets in base64url: the one definition that hhuff_cdigest.hip (a digest with
// its 5 + 5 bits of nbits and pbits in front) and hhuff_casper.hip (a cookie: no header, the connection's
// remainder_bits) both run.  Device only; called by every lane of a workgroup of one wave with equal arguments.
// A set is decoded in rounds of 4,096 bits:
//   a. the round's 512 bytes and 8 of look-ahead are decoded from base64 into LDS, a quad a lane;
//   b. lane L takes bits 64 L .. 64 L + 63 as a window, MSB first, so clz finds the next 1;
//   c. every lane fills its window's table entry offset -> offset at which the search enters the next window (a
//      backward pass over its 64 offsets, in LDS: a terminator at t hands the search to t + pbits + 1 <= 95, so the
//      exit is below 32 and the table composes window by window);
//   d. the wave follows the chain through the 64 tables (64 dependent LDS reads, every lane reads the same byte) and
//      lane L keeps the offset at which the search enters its window;
//   e. every lane walks the terminators of its window: q from the distance to the search position before (the round's
//      carry or the nearest earlier lane's, by a max scan, for its first one), the remainder from its and its
//      neighbour's window; key counts and sums of q << pbits | r plus one are prefix-summed over the wave (saturating,
//      so the drop decision key >= limit is exact at any length), and a second walk puts the keys into an LDS stage
//      that is handed to the caller's sink 64 keys at a time.
// The search position, the running minimum and the key count carry into the next round; an unfinished unary run is
// just a search position that lies rounds back.
#ifndef HHUFF_GCSWAVE_H
#define HHUFF_GCSWAVE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff_cdigest.h"

namespace hhuff {
namespace gcsw {
using namespace cd;

constexpr uint32_t kWave = 64;
constexpr uint32_t kRoundBits = 4096, kRoundBytes = kRoundBits / 8u;
constexpr uint32_t kBufBytes = kRoundBytes + 8u;  // a remainder of up to 31 bits behind bit 4095, and lane 63's neighbour
constexpr uint32_t kStage = 512;                  // keys an LDS stage holds: a round has at most 4,096, commonly a few hundred
constexpr uint32_t kNone = 0xFFFFFFFFu;

struct Lds {
    uint32_t* buf;    // kBufBytes
    uint8_t* tab;     // [64 offsets][64 lanes]
    uint64_t* stage;  // kStage
};

// (a message source of cd::SegWords, shared by the two units' hashes)
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

// The set in the c characters in[start ..): false = dropped (a tail of one character, a foreign byte, fewer bits than
// the header, a key at or above the limit).  HEADER: pbits and the limit 2^(nbits + pbits) are the set's first 10
// bits (*cap = nbits + pbits) and the values begin behind them; else they begin at bit 0 with the caller's pbits and
// limit.  put(i, key), i ascending from 0, is called by one lane a key and may refuse to store; *nkeys counts all.
template <bool HEADER, class Put>
__device__ bool decode(const uint8_t* in, uint64_t start, uint64_t c, uint32_t lane, const Lds& M, uint32_t pbits, uint64_t limit,
                       uint32_t* cap_out, uint64_t* nkeys_out, Put&& put) {
    if (c % 4u == 1u) return false;
    bool ok = true;
    for (uint64_t i = lane; i < c; i += kWave) ok = ok && b64_val(in[start + i]) != 0xFFu;
    if (__ballot(!ok)) return false;
    const uint64_t nbytes = c * 3u / 4u, nbits = 8u * nbytes;
    uint64_t p_in = HEADER ? 10u : 0u, next_min = 0, nkeys = 0;
    if (nbits < p_in) return false;
    uint32_t cap = 0;
    uint8_t* const bytes = reinterpret_cast<uint8_t*>(M.buf);
    uint8_t* const tab = M.tab;
    auto be64 = [&](uint32_t word) { return (uint64_t)__builtin_bswap32(M.buf[word]) << 32 | __builtin_bswap32(M.buf[word + 1u]); };
    for (uint64_t R = 0; R < nbits && p_in < nbits; R += kRoundBits) {
        // a. base64 -> the round's bytes (zeros behind the set's last byte)
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
        if (HEADER && R == 0) {
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
        if (total != 0 && next_out - 1u >= limit) return false;  // the round's last key: the set is dropped
        uint64_t sbefore = __shfl_up(sinc, 1u);
        sbefore = lane == 0 ? 0ull : sbefore;
        // second walk: the keys, through the stage
        for (uint32_t s0 = 0; s0 < total; s0 += kStage) {
            uint32_t idx = cinc - cnt - s0;  // (wraps below the stage's start: not stored)
            uint64_t run = sat_add(next_min, sbefore), fix = qfix;
            walk(w, wn, mine, pbits, base, nbits, [&](uint32_t q, uint64_t r) {
                const uint64_t key = sat_add(run, sat_add(sat_value(q, r, pbits), fix));
                if (idx < kStage) M.stage[idx] = key;
                run = key + 1u, fix = 0, ++idx;
            });
            __syncthreads();
            const uint32_t n = total - s0 < kStage ? total - s0 : kStage;
            for (uint32_t j = lane; j < n; j += kWave) put(nkeys + s0 + j, M.stage[j]);
            __syncthreads();
        }
        nkeys += total, next_min = next_out;
        const uint64_t plast = __shfl(lastp, (int)(kWave - 1u));
        p_in = plast > p_in ? plast : p_in;
    }
    *cap_out = cap, *nkeys_out = nkeys;
    return true;
}
}  // namespace gcsw
}  // namespace hhuff
#endif
