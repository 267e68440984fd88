// HTTP/2 frames on the receive side (include/hhuff.h (2k)): the rules of h2o_http2_decode_frame,
// h2o_http2_decode_headers_payload (lib/http2/frame.c:130-224) and of the HEADERS -> CONTINUATION sequencing
// (lib/http2/connection.c:757-803, 1023-1095, 1288-1325; lib/common/http2client.c:448-491, 607-659, 873-925) as
// plain functions over a byte span.  The device kernels (hhuff_frames.hip) and the host program
// (tools/frames_host.cpp) run this very code; it reads p[0 .. len) and nothing else.
//   frame_header     rules 1-3: the 9-byte header, the size limit, completeness
//   headers_payload  rule 5: stream id, padding, priority, the fragment
//   promise_payload  rule 7 with HHUFF_H2F_ACCEPT_PUSH (RFC 9113 6.6): stream id, padding, the promised id
//   walk             one connection: rules 1-9 in h2o's order.  A unit is one frame that is no header frame, or a
//                    whole header block (HEADERS / PUSH_PROMISE and its CONTINUATIONs).  A unit is first validated
//                    to its end without output -- so an error, a missing byte or a missing frame slot anywhere in
//                    it leaves nothing of it behind --, then walked again to hand its frames and its block to the
//                    sink.  `consumed` is the end of the last unit handed over.
#ifndef HHUFF_FRAMES_H
#define HHUFF_FRAMES_H
#include <stdint.h>

#include "hhuff.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HHUFF_FRM_HD __host__ __device__ __forceinline__
#else
#define HHUFF_FRM_HD inline
#endif

namespace hhuff {
namespace frm {

enum : uint32_t { kData = 0, kHeaders = 1, kPushPromise = 5, kContinuation = 9 };
enum : uint32_t { kEndStream = 0x1, kEndHeaders = 0x4, kPadded = 0x8, kPriority = 0x20 };
constexpr uint32_t kHeaderSize = 9;
constexpr int32_t kProtocol = -1, kFrameSize = -6;  // H2O_HTTP2_ERROR_PROTOCOL, _FRAME_SIZE
constexpr uint32_t kNoBlock = 0xFFFFFFFFu;

struct Hdr {
    uint32_t length, stream_id;
    uint32_t type, flags;
};

// h2o_http2_decode_frame: the frame's whole size (9 + length), 0 for incomplete, or -6.  The size limit is tested
// before completeness, as h2o tests it.
HHUFF_FRM_HD int64_t frame_header(const uint8_t* p, uint64_t avail, uint32_t max_frame_size, Hdr& h) {
    if (avail < kHeaderSize) return 0;
    h.length = ((uint32_t)p[0] << 16) | ((uint32_t)p[1] << 8) | p[2];
    h.type = p[3], h.flags = p[4];
    h.stream_id = (((uint32_t)p[5] << 24) | ((uint32_t)p[6] << 16) | ((uint32_t)p[7] << 8) | p[8]) & 0x7fffffffu;
    if (h.length > max_frame_size) return kFrameSize;
    if (avail < (uint64_t)kHeaderSize + h.length) return 0;
    return (int64_t)kHeaderSize + h.length;
}

struct Payload {
    uint32_t frag_off, frag_len;  // inside the payload
    uint32_t exclusive, dependency, weight;
    uint32_t promised;
    uint32_t err;  // HHUFF_H2F_ERR_*
};

// The pad byte of a PADDED frame: false when it is missing or longer than what follows it.
HHUFF_FRM_HD bool strip_padding(const uint8_t* pay, const Hdr& h, uint32_t& at, uint32_t& end) {
    at = 0, end = h.length;
    if ((h.flags & kPadded) == 0) return true;
    if (end == 0) return false;
    const uint32_t padlen = pay[at++];
    if (end - at < padlen) return false;
    end -= padlen;
    return true;
}

// h2o_http2_decode_headers_payload and handle_headers_frame's test of the stream id's parity: 0 or -1.  (The result
// is put together in locals and stored once: with a store of `err` at every return the compiler kept it in scratch.)
HHUFF_FRM_HD int32_t headers_payload(const uint8_t* pay, const Hdr& h, Payload& o) {
    uint32_t err = HHUFF_H2F_ERR_NONE, at = 0, end = 0, exclusive = 0, dependency = 0, weight = 16;  // h2o_http2_default_priority
    if (h.stream_id == 0) {
        err = HHUFF_H2F_ERR_HEADERS_STREAM_ID;
    } else if (!strip_padding(pay, h, at, end)) {
        err = HHUFF_H2F_ERR_HEADERS_FRAME;
    } else {
        if ((h.flags & kPriority) != 0) {
            if (end - at < 5) {
                err = HHUFF_H2F_ERR_HEADERS_PRIORITY;
            } else {
                const uint32_t u4 = ((uint32_t)pay[at] << 24) | ((uint32_t)pay[at + 1] << 16) | ((uint32_t)pay[at + 2] << 8) | pay[at + 3];
                exclusive = u4 >> 31, dependency = u4 & 0x7fffffffu, weight = (uint32_t)pay[at + 4] + 1u;
                at += 5;
            }
        }
        if (err == HHUFF_H2F_ERR_NONE && (h.stream_id & 1u) == 0) err = HHUFF_H2F_ERR_HEADERS_STREAM_ID;
    }
    const bool ok = err == HHUFF_H2F_ERR_NONE;
    o = Payload{ok ? at : 0u, ok ? end - at : 0u, exclusive, dependency, weight, 0u, err};
    return ok ? 0 : kProtocol;
}

HHUFF_FRM_HD int32_t promise_payload(const uint8_t* pay, const Hdr& h, Payload& o) {
    uint32_t err = HHUFF_H2F_ERR_NONE, at = 0, end = 0, promised = 0;
    if (h.stream_id == 0) {
        err = HHUFF_H2F_ERR_PROMISE_STREAM_ID;
    } else if (!strip_padding(pay, h, at, end) || end - at < 4) {
        err = HHUFF_H2F_ERR_PROMISE_FRAME;
    } else {
        promised = (((uint32_t)pay[at] << 24) | ((uint32_t)pay[at + 1] << 16) | ((uint32_t)pay[at + 2] << 8) | pay[at + 3]) & 0x7fffffffu;
        at += 4;
    }
    const bool ok = err == HHUFF_H2F_ERR_NONE;
    o = Payload{ok ? at : 0u, ok ? end - at : 0u, 0u, 0u, 16u, promised, err};
    return ok ? 0 : kProtocol;
}

struct Params {
    uint32_t max_frame_size, max_block_bytes, flags;
    uint32_t frame_cap;  // frame slots of this connection
};

struct Result {
    uint32_t nframes, nblocks, block_bytes, consumed;
    int32_t status;
    uint32_t err;
};

// A sink that keeps nothing: the counting walk.
struct NoSink {
    HHUFF_FRM_HD void frame(uint32_t, const hhuff_h2_frame_t&, uint32_t) {}
    HHUFF_FRM_HD void block(uint32_t, const hhuff_h2_block_t&, uint32_t) {}
};

// One connection, p[0 .. len).  The sink receives
//   frame(i, rec, dst)  frame i of the connection; offsets in rec are relative to p, rec.block is the block's number
//                       within the connection (kNoBlock: no header frame); dst = where the fragment goes, relative to
//                       the connection's first block byte
//   block(b, rec, off)  block b of the connection, complete; rec.first_frame is relative to the connection's first
//                       frame; off = the block's first byte, relative as dst
template <class Sink>
HHUFF_FRM_HD void walk(const uint8_t* p, uint32_t len, const Params& P, Sink& sink, Result& R) {
    R = Result{0, 0, 0, 0, 0, HHUFF_H2F_ERR_NONE};
    uint32_t pos = 0;
    for (;;) {
        Hdr h;
        const int64_t r = frame_header(p + pos, len - pos, P.max_frame_size, h);
        if (r <= 0) {
            R.status = (int32_t)r;
            return;
        }
        const uint32_t pay = pos + kHeaderSize;
        if (h.type != kHeaders && h.type != kPushPromise && h.type != kContinuation) {  // rule 8
            if (R.nframes == P.frame_cap) {
                R.status = HHUFF_H2F_FRAMES;
                return;
            }
            const hhuff_h2_frame_t f{pay, h.length, h.stream_id, (uint8_t)h.type, (uint8_t)h.flags, 0, 0, 0, kNoBlock, 0};
            sink.frame(R.nframes, f, 0);
            ++R.nframes, pos += (uint32_t)r, R.consumed = pos;
            continue;
        }
        if (h.type == kContinuation) {  // rule 6
            R.status = kProtocol, R.err = HHUFF_H2F_ERR_INVALID_CONTINUATION;
            return;
        }
        Payload pl;
        int32_t e;
        if (h.type == kPushPromise) {  // rule 7
            if ((P.flags & HHUFF_H2F_ACCEPT_PUSH) == 0) {
                R.status = kProtocol, R.err = HHUFF_H2F_ERR_PUSH_PROMISE;
                return;
            }
            e = promise_payload(p + pay, h, pl);
        } else {
            e = headers_payload(p + pay, h, pl);  // rule 5
        }
        if (e != 0) {
            R.status = e, R.err = pl.err;
            return;
        }
        // rule 4, without output: the CONTINUATIONs up to END_HEADERS
        uint32_t nfr = 1, size = pl.frag_len, q = pos + (uint32_t)r, end_stream_id = h.stream_id;
        if ((h.flags & kEndHeaders) == 0) {
            for (;;) {
                Hdr c;
                const int64_t rc = frame_header(p + q, len - q, P.max_frame_size, c);
                if (rc <= 0) {
                    R.status = (int32_t)rc;
                    return;
                }
                if (c.type != kContinuation) {
                    R.status = kProtocol, R.err = HHUFF_H2F_ERR_EXPECTED_CONTINUATION;
                    return;
                }
                if (P.max_block_bytes != 0 && (uint64_t)size + c.length > P.max_block_bytes) {
                    R.status = HHUFF_H2F_REFUSED;
                    return;
                }
                size += c.length, ++nfr, q += (uint32_t)rc, end_stream_id = c.stream_id;
                if ((c.flags & kEndHeaders) != 0) break;
            }
        }
        if (nfr > P.frame_cap - R.nframes) {  // rule 9
            R.status = HHUFF_H2F_FRAMES;
            return;
        }
        // the unit stands: hand it over
        hhuff_h2_block_t b{};
        b.stream_id = h.stream_id, b.end_stream_id = end_stream_id;
        b.flags = (h.type == kPushPromise ? HHUFF_H2B_PROMISE : (h.flags & kEndStream) ? HHUFF_H2B_END_STREAM : 0u) |
                  (nfr > 1 ? HHUFF_H2B_CONTINUED : 0u);
        if (h.type == kHeaders && (h.flags & kPriority) != 0)
            b.flags |= HHUFF_H2B_PRIORITY | (pl.exclusive ? HHUFF_H2B_EXCLUSIVE : 0u) |
                       (pl.dependency == h.stream_id ? HHUFF_H2B_SELF_DEPENDENCY : 0u);
        b.dependency = pl.dependency, b.weight = pl.weight, b.promised_stream_id = pl.promised;
        b.first_frame = R.nframes, b.nframes = nfr;
        const uint32_t boff = R.block_bytes;
        {
            const hhuff_h2_frame_t f{pay, h.length, h.stream_id, (uint8_t)h.type, (uint8_t)h.flags, 0, pay + pl.frag_off, pl.frag_len,
                                     R.nblocks, 0};
            sink.frame(R.nframes, f, R.block_bytes);
            ++R.nframes, R.block_bytes += pl.frag_len, pos += (uint32_t)r;
        }
        for (uint32_t k = 1; k < nfr; ++k) {
            Hdr c;
            const int64_t rc = frame_header(p + pos, len - pos, P.max_frame_size, c);  // (> 0: validated above)
            const hhuff_h2_frame_t f{pos + kHeaderSize, c.length, c.stream_id, (uint8_t)c.type, (uint8_t)c.flags, 0,
                                     pos + kHeaderSize, c.length, R.nblocks, 0};
            sink.frame(R.nframes, f, R.block_bytes);
            ++R.nframes, R.block_bytes += c.length, pos += (uint32_t)rc;
        }
        sink.block(R.nblocks, b, boff);
        ++R.nblocks, R.consumed = pos;
    }
}

}  // namespace frm
}  // namespace hhuff
#endif
