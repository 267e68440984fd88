// HTTP/2 control frames (include/hhuff.h (2k')): the payload rules of h2o_http2_decode_data_payload,
// _priority_payload, _rst_stream_payload, _ping_payload, _goaway_payload, _window_update_payload and
// h2o_http2_update_peer_settings (lib/http2/frame.c:37-66, 152-177, 226-310), h2o_http2_window_update
// (include/h2o/http2_common.h:234-241) and the stream-free parts of the frame handlers of both h2o sides
// (lib/http2/connection.c:976-989, 1097-1108, 1151-1261; lib/common/http2client.c:662-871) as plain functions over a
// byte span.  The device kernel (hhuff_h2ctl.hip) and the host program (tools/h2ctl_host.cpp) run this very code; a
// payload function reads p[0 .. F.length) and nothing else, byte by byte.
//   *_payload             one h2o decoder each: the record's a and b, or the error
//   update_peer_settings  the SETTINGS pairs onto a hhuff_h2_peer_t
//   step                  one frame against the connection's state: the record, the new state, the reply owed
//   walk                  one connection: its frame records in wire order, the first failure stops it
#ifndef HHUFF_H2CTL_H
#define HHUFF_H2CTL_H
#include <stdint.h>

#include "hhuff.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HHUFF_CTL_HD __host__ __device__ __forceinline__
#else
#define HHUFF_CTL_HD inline
#endif

namespace hhuff {
namespace h2c {

enum : uint32_t { kData = 0, kHeaders = 1, kPriority = 2, kRstStream = 3, kSettings = 4, kPushPromise = 5, kPing = 6, kGoaway = 7,
                  kWindowUpdate = 8, kContinuation = 9 };
enum : uint32_t { kAck = 0x1, kPadded = 0x8 };
// H2O_HTTP2_ERROR_PROTOCOL, _FLOW_CONTROL, _FRAME_SIZE
constexpr int32_t kProtocol = -1, kFlowControl = -3, kFrameSize = -6;
constexpr uint32_t kHeaderSize = 9, kMaxReply = 17;
constexpr int64_t kInt32Max = 0x7fffffff;

struct Frame {  // of the frame record
    uint32_t payload_off, length, stream_id, type, flags;
};

struct Verdict {
    uint32_t a, b;
    int32_t status;
    uint32_t err, flags;
};

// A reply frame: the 9-byte header and up to two big-endian words of payload (len = 9, 13 or 17; 0: none).
struct Reply {
    uint32_t len, type, flags, stream_id, w0, w1;
};

HHUFF_CTL_HD uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// (Every rule puts its result together in locals and builds the record's content once, at its end: with a store into
// the caller's struct at every return the compiler kept the struct in scratch.)
HHUFF_CTL_HD Verdict refused(int32_t status, uint32_t err, uint32_t a = 0) { return Verdict{a, 0, status, err, 0}; }
HHUFF_CTL_HD Verdict passed(uint32_t a, uint32_t b, uint32_t flags) { return Verdict{a, b, 0, HHUFF_H2C_ERR_NONE, flags}; }
HHUFF_CTL_HD Verdict verdict(uint32_t err, int32_t status, uint32_t a, uint32_t b, uint32_t flags) {
    return err == HHUFF_H2C_ERR_NONE ? passed(a, b, flags) : refused(status, err);
}

// h2o_http2_decode_data_payload: a = the data's offset inside the payload, b = its length
HHUFF_CTL_HD Verdict data_payload(const uint8_t* p, const Frame& F) {
    uint32_t err = HHUFF_H2C_ERR_NONE, a = 0, b = F.length;
    if (F.stream_id == 0) {
        err = HHUFF_H2C_ERR_DATA_STREAM_ID;
    } else if ((F.flags & kPadded) != 0) {
        if (F.length < 1) {
            err = HHUFF_H2C_ERR_DATA_FRAME;
        } else {
            const uint32_t pad = p[0];
            if (F.length < 1u + pad) err = HHUFF_H2C_ERR_DATA_FRAME;
            a = 1, b = F.length - (1u + pad);
        }
    }
    return verdict(err, kProtocol, a, b, HHUFF_H2R_NEEDS_STREAM);
}

// h2o_http2_decode_priority_payload and the handlers' "stream cannot depend on itself"
HHUFF_CTL_HD Verdict priority_payload(const uint8_t* p, const Frame& F) {
    if (F.stream_id == 0) return refused(kProtocol, HHUFF_H2C_ERR_PRIORITY_STREAM_ID);
    if (F.length != 5) return refused(kFrameSize, HHUFF_H2C_ERR_PRIORITY_FRAME);
    const uint32_t u4 = be32(p);
    return verdict((u4 & 0x7fffffffu) == F.stream_id ? HHUFF_H2C_ERR_SELF_DEPENDENCY : HHUFF_H2C_ERR_NONE, kProtocol, u4,
                   (uint32_t)p[4] + 1u, HHUFF_H2R_NEEDS_STREAM);
}

HHUFF_CTL_HD Verdict rst_stream_payload(const uint8_t* p, const Frame& F) {
    if (F.stream_id == 0) return refused(kProtocol, HHUFF_H2C_ERR_RST_STREAM_STREAM_ID);
    if (F.length != 4) return refused(kFrameSize, HHUFF_H2C_ERR_RST_STREAM_FRAME);
    return passed(be32(p), 0, HHUFF_H2R_NEEDS_STREAM);
}

HHUFF_CTL_HD Verdict ping_payload(const uint8_t* p, const Frame& F) {
    if (F.stream_id != 0) return refused(kProtocol, HHUFF_H2C_ERR_PING_FRAME);
    if (F.length != 8) return refused(kFrameSize, HHUFF_H2C_ERR_PING_FRAME);
    return passed(be32(p), be32(p + 4), (F.flags & kAck) != 0 ? HHUFF_H2R_ACK : 0u);
}

HHUFF_CTL_HD Verdict goaway_payload(const uint8_t* p, const Frame& F) {
    if (F.stream_id != 0) return refused(kProtocol, HHUFF_H2C_ERR_GOAWAY_STREAM_ID);
    if (F.length < 8) return refused(kFrameSize, HHUFF_H2C_ERR_GOAWAY_FRAME);
    return passed(be32(p) & 0x7fffffffu, be32(p + 4), 0);
}

// h2o_http2_decode_window_update_payload: a = the increment; stream_level as h2o's *err_is_stream_level
HHUFF_CTL_HD Verdict window_update_payload(const uint8_t* p, const Frame& F, bool& stream_level) {
    stream_level = false;
    if (F.length != 4) return refused(kFrameSize, HHUFF_H2C_ERR_WINDOW_UPDATE_FRAME);
    const uint32_t increment = be32(p) & 0x7fffffffu;
    stream_level = increment == 0 && F.stream_id != 0;
    return verdict(increment == 0 ? HHUFF_H2C_ERR_WINDOW_UPDATE_FRAME : HHUFF_H2C_ERR_NONE, kProtocol, increment, 0, 0);
}

// h2o_http2_update_peer_settings on S's five settings: 0 or the error; pairs = those read without error.  What an
// earlier pair set stays set.
HHUFF_CTL_HD int32_t update_peer_settings(hhuff_h2_peer_t& S, const uint8_t* p, uint32_t len, uint32_t& pairs, uint32_t& err) {
    pairs = 0, err = HHUFF_H2C_ERR_NONE;
    for (; len >= 6; len -= 6, p += 6, ++pairs) {
        const uint32_t id = ((uint32_t)p[0] << 8) | p[1], value = be32(p + 2);
        int32_t bad = 0;
        switch (id) {
            case 1: S.header_table_size = value; break;
            case 2:
                if (value > 1u) bad = kProtocol; else S.enable_push = value;
                break;
            case 3: S.max_concurrent_streams = value; break;
            case 4:
                if (value > 0x7fffffffu) bad = kFlowControl; else S.initial_window_size = value;
                break;
            case 5:
                if (value < 16384u || value > 16777215u) bad = kProtocol; else S.max_frame_size = value;
                break;
            default: break;  // unknown identifiers are ignored (RFC 9113 6.5.2)
        }
        if (bad != 0) {
            err = HHUFF_H2C_ERR_SETTINGS_FRAME;
            return bad;
        }
    }
    if (len != 0) {
        err = HHUFF_H2C_ERR_SETTINGS_SIZE;
        return kFrameSize;
    }
    return 0;
}

// h2o_http2_window_update for an increment of at most 2^31 - 1
HHUFF_CTL_HD int32_t window_update(int64_t& avail, uint32_t increment) {
    if (avail > kInt32Max - (int64_t)increment) return -1;
    avail += increment;
    return 0;
}

struct Params {
    uint32_t flags;             // HHUFF_H2C_*
    uint32_t recv_window_size;  // <= INT32_MAX
};

// One frame, payload p[0 .. F.length), against the state S: v is the record's content, rp the reply owed (len 0:
// none).  Returns the connection-level status: 0, or h2o's error, with S then as h2o leaves its connection.
HHUFF_CTL_HD int32_t step(const uint8_t* p, const Frame& F, const Params& P, hhuff_h2_peer_t& S, Verdict& out, Reply& reply) {
    Verdict v = passed(0, 0, 0);  // HEADERS, PUSH_PROMISE, CONTINUATION are (2k)'s; expect_default ignores types from 10 on
    Reply rp{0, 0, 0, 0, 0, 0};
    bool fatal = true;  // a status other than 0 ends the connection
    if (F.type == kData) {
        v = data_payload(p, F);
        if (v.status == 0) {
            v.a += F.payload_off;
            if (P.recv_window_size != 0 && (P.flags & HHUFF_H2C_CLIENT) == 0) {  // connection.c:986-989
                S.recv_window -= (int64_t)F.length;
                if (S.recv_window <= (int64_t)(P.recv_window_size / 2u)) {
                    rp = Reply{13, kWindowUpdate, 0, 0, (uint32_t)(uint64_t)((int64_t)P.recv_window_size - S.recv_window), 0};
                    S.recv_window = P.recv_window_size;
                    v.flags |= HHUFF_H2R_WINDOW_UPDATE;
                }
            }
        }
    } else if (F.type == kPriority) {
        v = priority_payload(p, F);
    } else if (F.type == kRstStream) {
        v = rst_stream_payload(p, F);
    } else if (F.type == kSettings) {
        if (F.stream_id != 0) {
            v = refused(kProtocol, HHUFF_H2C_ERR_SETTINGS_STREAM_ID);
        } else if ((F.flags & kAck) != 0) {
            v = F.length != 0 ? refused(kFrameSize, HHUFF_H2C_ERR_SETTINGS_ACK) : passed(0, 0, HHUFF_H2R_ACK);
        } else {
            const uint32_t before = S.initial_window_size;
            uint32_t pairs, err;
            const int32_t r = update_peer_settings(S, p, F.length, pairs, err);
            if (r != 0) {
                v = refused(r, err, pairs);
            } else {
                const uint32_t delta = S.initial_window_size - before;  // connection.c:1178-1179: the int32 difference's bits
                v = passed(pairs, delta, delta != 0 ? HHUFF_H2R_WINDOW_DELTA : 0u);
                S.flags |= HHUFF_H2P_SETTINGS;
                rp = Reply{9, kSettings, kAck, 0, 0, 0};
            }
        }
    } else if (F.type == kPing) {
        v = ping_payload(p, F);
        if (v.status == 0 && (F.flags & kAck) == 0) rp = Reply{17, kPing, kAck, 0, v.a, v.b};
    } else if (F.type == kGoaway) {
        v = goaway_payload(p, F);
        if (v.status == 0) S.flags |= HHUFF_H2P_GOAWAY;
    } else if (F.type == kWindowUpdate) {
        bool stream_level;
        v = window_update_payload(p, F, stream_level);
        if (stream_level) {  // stream_send_error(conn, stream_id, ret); the connection goes on
            fatal = false;
            rp = Reply{13, kRstStream, 0, F.stream_id, (uint32_t)-v.status, 0};
            v.flags = HHUFF_H2R_STREAM_ERROR | HHUFF_H2R_NEEDS_STREAM;
        } else if (v.status == 0) {
            if (F.stream_id != 0)
                v.flags = HHUFF_H2R_NEEDS_STREAM;
            else if (window_update(S.send_window, v.a) != 0)
                v = refused(kFlowControl, HHUFF_H2C_ERR_FLOW_CONTROL);
        }
    }
    out = v, reply = rp;
    return fatal ? v.status : 0;
}

// The reply's bytes (frame.c:68-122) to dst[0 .. rp.len).
HHUFF_CTL_HD void emit(uint8_t* dst, const Reply& rp) {
    if (rp.len == 0) return;
    const uint32_t n = rp.len - kHeaderSize;
    dst[0] = 0, dst[1] = 0, dst[2] = (uint8_t)n, dst[3] = (uint8_t)rp.type, dst[4] = (uint8_t)rp.flags;
    dst[5] = (uint8_t)(rp.stream_id >> 24), dst[6] = (uint8_t)(rp.stream_id >> 16), dst[7] = (uint8_t)(rp.stream_id >> 8);
    dst[8] = (uint8_t)rp.stream_id;
    if (n >= 4) dst[9] = (uint8_t)(rp.w0 >> 24), dst[10] = (uint8_t)(rp.w0 >> 16), dst[11] = (uint8_t)(rp.w0 >> 8), dst[12] = (uint8_t)rp.w0;
    if (n >= 8) dst[13] = (uint8_t)(rp.w1 >> 24), dst[14] = (uint8_t)(rp.w1 >> 16), dst[15] = (uint8_t)(rp.w1 >> 8), dst[16] = (uint8_t)rp.w1;
}

struct Result {
    uint32_t nctl, rep_len;
    int32_t status;
    uint32_t err;
};

HHUFF_CTL_HD hhuff_h2_ctl_t record_of(const Verdict& v, uint32_t reply_len) {
    return hhuff_h2_ctl_t{v.a, v.b, v.status, (uint16_t)v.err, (uint8_t)v.flags, (uint8_t)reply_len};
}

// One connection: its n frame records fr[0 .. n) (offsets in in[0 .. in_size)), its state S (in and out), its reply
// region rep[0 .. rep_cap).  sink.record(i, rec) receives frame i's record.  A frame is first handled on a copy of
// the state, so that a reply that does not fit leaves nothing of it behind.
template <class Sink>
HHUFF_CTL_HD void walk(const uint8_t* in, uint64_t in_size, const hhuff_h2_frame_t* fr, uint32_t n, const Params& P,
                       hhuff_h2_peer_t& S, uint8_t* rep, uint32_t rep_cap, Sink& sink, Result& R) {
    R = Result{0, 0, 0, HHUFF_H2C_ERR_NONE};
    if (n == 0) return;
    // (the next record is loaded before this one's stores are issued: a lane's chain of loads does not wait on them)
    Frame next{fr[0].payload_off, fr[0].length, fr[0].stream_id, fr[0].type, fr[0].flags};
    for (uint32_t i = 0; i < n; ++i) {
        const Frame F = next;
        const uint32_t j = i + 1u < n ? i + 1u : i;
        next = Frame{fr[j].payload_off, fr[j].length, fr[j].stream_id, fr[j].type, fr[j].flags};
        if ((uint64_t)F.payload_off + F.length > in_size) {
            R.status = HHUFF_H2C_EINVAL;
            return;
        }
        hhuff_h2_peer_t T = S;
        Verdict v;
        Reply rp;
        const int32_t r = step(in + F.payload_off, F, P, T, v, rp);
        if (r != 0) {  // what the handler changed before it failed stands (a SETTINGS frame's earlier pairs)
            S = T;
            sink.record(i, record_of(v, 0));
            R.status = r, R.err = v.err;
            return;
        }
        if (rp.len > rep_cap - R.rep_len) {
            R.status = HHUFF_H2C_SPACE;
            return;
        }
        S = T;
        emit(rep + R.rep_len, rp);
        R.rep_len += rp.len;
        sink.record(i, record_of(v, rp.len));
        ++R.nctl;
    }
}

}  // namespace h2c
}  // namespace hhuff
#endif
