// What the header encoders of both protocols share (hhuff_hpenc.hip: HPACK, hhuff_qpenc.hip: QPACK): the
// prefix-integer and string lengths, the string hash, prep's per-pair step, the register-sink writers, the
// long-string lists with the two launches that serve them, and the launchers' workspace and launch helpers.
// The Huffman code tables are hhuff_devtables.h's.  One object is built per .hip and the units share no device
// symbols, so the tables have internal linkage: one copy per unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_device.h"
#include "hhuff_devtables.h"
#include "hhuff_launch.h"

namespace hhuff {
// Strings too long for one lane: their hash / code bits (long_bits_kernel) and their payloads
// (long_payload_kernel) are done by a wave each.
struct LongWork {
    uint32_t* bits;  // [1 + cap]: count, then item << 1 | which (0 name, 1 value)
    uint4* jobs;     // payloads {source offset, length, destination address lo, hi | Huffman << 31}
    uint32_t* njobs;
    uint32_t cap, jcap;
};

// The two launches of the long-string kernels (hhuff_hpenc.hip).  launch_long_bits: rec[item].z / .w get the
// code bits of the listed names / values and, with `hash`, .x / .y their hashes.
hipError_t launch_long_bits(bool hash, const uint8_t* in, const hhuff_hpack_header_t* hdr, uint32_t nhdr, uint32_t server_off,
                            uint32_t server_len, uint4* rec, const LongWork& L, hipStream_t stream);
hipError_t launch_long_payload(const uint8_t* in, const LongWork& L, hipStream_t stream);

// The long lists of a call out of its workspace; the capacities are the launcher's (it derives them and
// refuses those past 32 bits)
inline LongWork long_ws(Carve& cv, uint64_t bits, uint64_t jobs) {
    LongWork L;
    L.jobs = cv.take<uint4>(jobs);
    L.bits = cv.take<uint32_t>(1 + bits);
    L.njobs = cv.take<uint32_t>(1);
    L.cap = (uint32_t)bits;
    L.jcap = (uint32_t)jobs;
    return L;
}

// One line per kernel in a launcher: launched if all went well so far, `e` then holds the launch's error
#define HHUFF_LAUNCH(e, kernel, grid, block, stream, ...)                                         \
    do {                                                                                          \
        if ((e) == hipSuccess) {                                                                  \
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, __VA_ARGS__);          \
            (e) = hipGetLastError();                                                              \
        }                                                                                         \
    } while (0)

namespace {
__device__ const uint8_t __attribute__((aligned(16))) e_server[16] = {'s', 'e', 'r', 'v', 'e', 'r'};

constexpr uint32_t kLongStr = 256;     // strings longer than this are hashed / coded by a whole wave
constexpr uint32_t kOpSkip = 1u << 31; // op code of a field that writes nothing

__device__ __forceinline__ uint32_t int_len(uint32_t v, uint32_t p) {  // h2o_hpack_encode_int's length (hpack.c:757-772)
    const uint32_t pmax = (1u << p) - 1u;
    if (v < pmax) return 1;
    v -= pmax;
    uint32_t n = 2;
    while (v >= 128) {
        v >>= 7;
        ++n;
    }
    return n;
}

__device__ __forceinline__ bool huff_wins(uint32_t len, uint32_t bits) {  // hpack.c:789-791, :799-800
    return len != 0 && bits <= 8u * len - 8u;
}

__device__ __forceinline__ uint32_t str_len(uint32_t len, uint32_t bits) {  // h2o_hpack_encode_string's length
    if (huff_wins(len, bits)) {
        const uint32_t hb = (bits + 7u) >> 3;
        return int_len(hb, 7) + hb;
    }
    return int_len(len, 7) + len;
}

// String hash: sum over the 4-byte words w_k (bytes 4k .. 4k+3, zero past the end) of mix(w_k, k), mixed with
// the length -- a function of the bytes alone that any split of the words computes alike, so one lane and a
// whole wave agree.  Used as a prefilter only: the bytes of a candidate are always compared.
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint32_t word_term(uint32_t w, uint32_t k) { return mix32(w ^ (k * 0x9E3779B9u)); }
__device__ __forceinline__ uint32_t hash_final(uint32_t sum, uint32_t len) { return mix32(sum ^ (len * 0x85EBCA6Bu)); }

// the 4 bytes of word k of string p (length len), zero past the end; code bits of its bytes
__device__ __forceinline__ uint32_t string_word(const uint8_t* p, uint32_t len, uint32_t k, const uint8_t* nbits, uint32_t& bits) {
    uint32_t w = 0;
    const uint32_t a = 4u * k;
    if (a + 4u <= len) {
        __builtin_memcpy(&w, p + a, 4);
        bits = nbits[w & 0xFFu] + nbits[(w >> 8) & 0xFFu] + nbits[(w >> 16) & 0xFFu] + nbits[w >> 24];
    } else {
        bits = 0;
        for (uint32_t j = 0; j < 4; ++j)
            if (a + j < len) {
                const uint32_t b = p[a + j];
                w |= b << (8 * j);
                bits += nbits[b];
            }
    }
    return w;
}

__device__ __forceinline__ void hash_bits_lane(const uint8_t* p, uint32_t len, const uint8_t* nbits, uint32_t& h, uint32_t& bits) {
    uint32_t sum = 0;
    bits = 0;
    for (uint32_t k = 0; 4u * k < len; ++k) {
        uint32_t b;
        sum += word_term(string_word(p, len, k, nbits, b), k);
        bits += b;
    }
    h = hash_final(sum, len);
}

__device__ __forceinline__ bool lit_eq(const uint8_t* a, const char* lit, uint32_t n) {
    for (uint32_t k = 0; k < n; ++k)
        if (a[k] != (uint8_t)lit[k]) return false;
    return true;
}

// byte equality without an early exit: 16-byte loads issue back to back, one wait covers them
__device__ __forceinline__ bool bytes_eq(const uint8_t* a, const uint8_t* b, uint32_t n) {
    uint32_t diff = 0, k = 0;
    for (; k + 16u <= n; k += 16u) {
        uint4 x, y;
        __builtin_memcpy(&x, a + k, 16);
        __builtin_memcpy(&y, b + k, 16);
        diff |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
    }
    for (; k < n; ++k) diff |= (uint32_t)(a[k] ^ b[k]);
    return diff == 0;
}

__device__ __forceinline__ void push_long_bits(const LongWork& L, uint32_t item, uint32_t which) {
    const uint32_t j = atomicAdd(L.bits, 1u);
    if (j < L.cap) L.bits[1 + j] = item << 1 | which;
}

// prep's step for the string pair of `item`: the rec word {name hash, value hash, name code bits, value code
// bits}, each string hashed and counted in this lane or -- longer than kLongStr -- left to long_bits_kernel
__device__ __forceinline__ uint4 prep_pair(const LongWork& L, uint32_t item, const uint8_t* n, uint32_t nl, const uint8_t* v,
                                           uint32_t vl, const uint8_t* nbits) {
    uint32_t nh, vh, nb = 0, vb = 0;
    if (nl > kLongStr) {
        push_long_bits(L, item, 0);
        nh = 0;
    } else {
        hash_bits_lane(n, nl, nbits, nh, nb);
    }
    if (vl > kLongStr) {
        push_long_bits(L, item, 1);
        vh = 0;
    } else {
        hash_bits_lane(v, vl, nbits, vh, vb);
    }
    return make_uint4(nh, vh, nb, vb);
}

__device__ __forceinline__ void sink_int(RegSink& sink, uint32_t first, uint32_t v, uint32_t p) {  // hpack.c:757-772
    const uint32_t pmax = (1u << p) - 1u;
    if (v < pmax) {
        sink.put1(first | v);
        return;
    }
    sink.put1(first | pmax);
    v -= pmax;
    while (v >= 128) {
        sink.put1(0x80u | (v & 127u));
        v >>= 7;
    }
    sink.put1(v);
}

__device__ __forceinline__ void sink_raw(RegSink& sink, const GlobalSource& src, uint32_t s, uint32_t len) {
    uint32_t a = s & ~3u, rem = len, skip = s & 3u;
    while (rem) {
        const uint32_t w = src.word(a) >> (8 * skip);
        const uint32_t k = min(4u - skip, rem);
        sink.push(w, k);
        rem -= k;
        a += 4;
        skip = 0;
    }
}

// The payload of a string literal: written here, or -- longer than kLongStr -- handed to
// long_payload_kernel while the sink steps over its bytes.
__device__ __forceinline__ void sink_payload(RegSink& sink, const GlobalSource& src, uint32_t s, uint32_t len, bool huff,
                                             uint32_t hb, const uint2* enc, const LongWork& L) {
    if (len > kLongStr) {
        sink.finish();
        const uint64_t d = (uint64_t)sink.p;
        const uint32_t j = atomicAdd(L.njobs, 1u);
        if (j < L.jcap) L.jobs[j] = make_uint4(s, len, (uint32_t)d, (uint32_t)(d >> 32) | (huff ? 0x80000000u : 0u));
        sink.init(sink.p + (huff ? hb : len));
    } else if (huff) {
        encode_core(src, s, len, sink, enc);  // flushes the sink
    } else {
        sink_raw(sink, src, s, len);
    }
}

// h2o_hpack_encode_string (hpack.c:816-837) of in[s .. s + len) whose code is `bits` long
__device__ __forceinline__ void sink_string(RegSink& sink, const GlobalSource& src, uint32_t s, uint32_t len, uint32_t bits,
                                            const uint2* enc, const LongWork& L) {
    const bool huff = huff_wins(len, bits);
    const uint32_t hb = (bits + 7u) >> 3;
    sink_int(sink, huff ? 0x80u : 0u, huff ? hb : len, 7);
    sink_payload(sink, src, s, len, huff, hb, enc, L);
}
}  // namespace
}  // namespace hhuff
