// The HPACK / QPACK prefix integer on the receive side: h2o_hpack_decode_int (lib/http2/hpack.c:52-83), the one
// definition the header-block decoders (hhuff_blocks.hip, hhuff_qpack.hip), the literal kernels (hhuff_literals.hip),
// the QPACK encoder sessions' decoder stream (hhuff_qpenc.hip) and the host program tools/int_host.cpp run.  It reads
// bytes[p .. end) and nothing else.
#ifndef HHUFF_INT_H
#define HHUFF_INT_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HHUFF_INT_HD __host__ __device__ static  // (no inline hint: the compiler decides, as for the copies it replaces)
#else
#define HHUFF_INT_HD inline
#endif

namespace hhuff {

constexpr int64_t kIntIncomplete = -255, kIntBad = -9;  // H2O_HTTP2_ERROR_INCOMPLETE, _COMPRESSION

// The integer with a prefix of prefix_bits bits at bytes[p], bounded by end: its value (p then stands behind it),
// kIntIncomplete when the bytes end inside it, kIntBad when it passes 2^63 - 1 or goes on behind its tenth octet.
HHUFF_INT_HD int64_t hpack_int(const uint8_t* bytes, uint64_t& p, uint64_t end, uint32_t prefix_bits) {
    if (p >= end) return kIntIncomplete;
    const uint64_t pmax = (1u << prefix_bits) - 1u;
    uint64_t v = bytes[p++] & pmax;
    if (v != pmax) return (int64_t)v;
    uint32_t shift = 0;
    for (; shift < 56; shift += 7) {
        if (p == end) return kIntIncomplete;
        const uint32_t b = bytes[p++];
        v += (uint64_t)(b & 127u) << shift;
        if (!(b & 128u)) return (int64_t)v;
    }
    if (p == end) return kIntIncomplete;  // the ninth octet after the prefix (hpack.c:75-81)
    if (bytes[p] & 128u) return kIntBad;
    v += (uint64_t)(bytes[p++] & 127u) << shift;
    if (v > 0x7FFFFFFFFFFFFFFFull) return kIntBad;
    return (int64_t)v;
}

}  // namespace hhuff
#endif
