// HTTP/3 bodies (include/hhuff.h (2l') and (2l'')): what handle_input_expect_data_payload (lib/http3/server.c:1388-1409)
// appends to req_body with the content-length test of handle_input_expect_data (server.c:1431-1438), and the DATA frame
// header of flatten_data_frame_header (server.c:1694-1709).  The device kernels (hhuff_h3bodies.hip) and the host
// program (tools/h3bodies_host.cpp) run this very code.
//   Cnt           what a slot or a send record adds to the scans: bytes (64 bits: hostile payloads may overlap), DATA
//                 slots, bad slots
//   slot_count    one frame record's counts
//   varint_size, hdr_len, hdr_byte, hdr_of_size   the DATA header: a type byte 0 and the shortest QUIC varint
//   over, first_true   the content-length test as a monotone predicate over a stream's slots, and its bisection
//   write_line    one 16-byte line of the packed output (cut by address), whatever segments lie in it: one writer a line
#ifndef HHUFF_H3BODIES_H
#define HHUFF_H3BODIES_H
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_linecopy.h"

namespace hhuff {
namespace h3b {

constexpr uint32_t kBadSrc = 0xFFFFFFFFu;  // a segment whose source is not read (in_size <= 2^32 - 3: no payload begins there)

struct Cnt {  // 16 bytes
    uint64_t bytes;
    uint32_t data, bad;
};
static_assert(sizeof(Cnt) == 16, "workspace layout");
HHUFF_LC_HD Cnt vadd(Cnt a, Cnt b) { return Cnt{a.bytes + b.bytes, a.data + b.data, a.bad + b.bad}; }

// A DATA slot is bad when its payload leaves in[0 .. in_size) or avail > length; a bad slot adds no bytes.
HHUFF_LC_HD Cnt slot_count(const hhuff_h3_frame_t& F, uint64_t in_size) {
    if (F.type != 0) return Cnt{0, 0, 0};
    const bool bad = F.avail > F.length || (uint64_t)F.payload_off + F.avail > in_size;
    return Cnt{bad ? 0u : F.avail, 1u, bad ? 1u : 0u};
}

HHUFF_LC_HD uint32_t varint_size(uint64_t v) { return v < 64u ? 1u : (v < 16384u ? 2u : (v < (1u << 30) ? 4u : 8u)); }
HHUFF_LC_HD uint32_t hdr_len(uint64_t len) { return len != 0 ? 1u + varint_size(len) : 0u; }  // payload_size != 0 guards the header
// byte i of the h header bytes of a payload of len bytes: the type, then quicly_encodev's big-endian varint
HHUFF_LC_HD uint32_t hdr_byte(uint64_t len, uint32_t h, uint32_t i) {
    if (i == 0) return 0u;
    const uint32_t n = h - 1u;  // 1, 2, 4, 8
    const uint64_t tag = n == 1u ? 0u : (n == 2u ? 1u : (n == 4u ? 2u : 3u));
    return (uint32_t)(((len | (tag << (8u * n - 2u))) >> (8u * (n - i))) & 0xffu);
}
// the header bytes of a frame of sz bytes in all: sz = hdr_len(len) + len has one solution
HHUFF_LC_HD uint32_t hdr_of_size(uint64_t sz) {
    return sz == 0 ? 0u : (sz <= 63u + 2u ? 2u : (sz <= 16383u + 3u ? 3u : (sz <= (1u << 30) + 4u ? 5u : 9u)));
}

// server.c:1431: content_length - req_body_bytes_received < frame.length, with P of the stream's bytes of this step in
// front of the slot and room = content_length - received on entry.  hl: the length of a DATA slot that has a header, 0
// for any other slot.  Every DATA frame but a stream's last in a step is complete, so P + hl never decreases along a
// stream the de-framer listed, and the first slot that is over is a bisection.
HHUFF_LC_HD bool over(uint64_t room, uint64_t P, uint64_t hl) { return P > room || room - P < hl; }
HHUFF_LC_HD uint64_t header_length(const hhuff_h3_frame_t& F) { return F.type == 0 && F.hdr_off != F.payload_off ? F.length : 0u; }
template <class Pred>
HHUFF_LC_HD uint32_t first_true(uint32_t n, Pred pred) {  // the first k < n with pred(k), n when there is none
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (pred(mid))
            hi = mid;
        else
            lo = mid + 1u;
    }
    return lo;
}

// A segment of the packed output: out[s0 .. s1), first its header (kHdr: hdr_of_size(s1 - s0) bytes), then its payload
// from src[seg.src ..); kBadSrc: its bytes are left 0.
struct Seg {
    uint32_t s0, s1, src;
};

// The line at address `line`, whose byte 0 is out[o0] (o0 < 0 in the first line of an `out` that is not aligned), of an
// output of `limit` bytes.  find(x) -> the segment that holds out[x].  A line inside one payload is aligned source
// dwords, funnel-shifted, and one 16-byte store; else the segments that touch it are walked and the line assembled in
// registers, and stored once -- in part only where the line leaves out[0 .. limit).
template <bool kHdr, class Find>
HHUFF_LC_HD void write_line(uint64_t src_addr, uint64_t line, int64_t o0, uint32_t limit, Find& find) {
    const int b0 = o0 < 0 ? (int)-o0 : 0;
    const int b1 = (int64_t)limit - o0 < 16 ? (int)((int64_t)limit - o0) : 16;
    uint8_t* d = reinterpret_cast<uint8_t*>((uintptr_t)line);
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    for (int p = b0; p < b1;) {
        const uint32_t x = (uint32_t)(o0 + p);
        const Seg S = find(x);
        if (x < S.s0 || x >= S.s1) {  // (never, whatever the records hold, unless they change under the call)
            ++p;
            continue;
        }
        const uint32_t sz = S.s1 - S.s0, h = kHdr ? hdr_of_size(sz) : 0u;
        const int e = (int64_t)S.s1 - o0 < b1 ? (int)((int64_t)S.s1 - o0) : b1;  // the segment has the line's bytes [p, e)
        const int64_t pay = (int64_t)S.s0 + h - o0;                             // where its payload begins in the line
        const int pl = pay > p ? (pay < e ? (int)pay : e) : p;
        if (pl < e && S.src != kBadSrc) {
            uint32_t w[4];
            lc::load16(src_addr + S.src - (uint64_t)pay, pl, e, w);  // (modulo 2^64 where the payload begins behind byte 0)
            if (pl == 0 && e == 16) {
                lc::store16(d, w);
                return;
            }
            HHUFF_LC_UNROLL
            for (int q = 0; q < 4; ++q) v[q] |= w[q] & lc::mask32(q, pl, e);
        }
        if (kHdr && p < pl) {
            HHUFF_LC_UNROLL
            for (int i = 0; i < 16; ++i)
                if (i >= p && i < pl) v[i >> 2] |= hdr_byte(sz - h, h, (uint32_t)(o0 + i - S.s0)) << (8 * (i & 3));
        }
        p = e;
    }
    if (b0 == 0 && b1 == 16)
        lc::store16(d, v);
    else
        lc::store_part(d, v, b0, b1);
}

}  // namespace h3b
}  // namespace hhuff
#endif
