// HTTP/3 frames on the receive side (include/hhuff.h (2l)): the rules of h2o_http3_read_frame
// (lib/http3/common.c:1057-1145), of the request-stream handlers of h2o's server (lib/http3/server.c:1367-1453,
// 1499-1536) and client (lib/common/http3client.c:438-540), of unknown_type_handle_input and
// control_stream_handle_input (common.c:365-439), of h2o_http3_handle_settings_frame (common.c:1422-1473) and of
// h2o_http3_decode_priority_update_frame / _goaway_frame (lib/http3/frame.c:40-98) as plain functions over a byte
// span.  The device kernels (hhuff_h3frames.hip) and the host program (tools/h3frames_host.cpp) run this very code;
// it reads p[0 .. len) and nothing else.
//   varint                   ptls_decode_quicint: 1, 2, 4 or 8 bytes by the first byte's top bits, any width for any
//                            value
//   read_frame               rule 1: two varints, the size limit, completeness, the type table
//   settings_payload         rule 13: id / value pairs, the last value of an id stands
//   priority_update_payload  rule 13: the element id and its kind
//   goaway_payload           rule 13: one varint and nothing behind it
//   walk                     one stream: rules 1-14 in h2o's order.  A frame is handed to the sink only when every
//                            rule has passed it, so an error, a missing byte or a missing frame slot leaves nothing
//                            of it behind; `consumed` is the end of the last frame handed over (or of the bytes a
//                            stream without frames gives away).
#ifndef HHUFF_H3FRAMES_H
#define HHUFF_H3FRAMES_H
#include <stdint.h>

#include "hhuff.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HHUFF_H3F_HD __host__ __device__ __forceinline__
#else
#define HHUFF_H3F_HD inline
#endif

namespace hhuff {
namespace h3f {

enum : uint64_t {
    kData = 0,
    kHeaders = 1,
    kCancelPush = 3,
    kSettings = 4,
    kPushPromise = 5,
    kGoaway = 7,
    kMaxPushId = 13,
    kPriorityUpdateRequest = 0xF0700,
    kPriorityUpdatePush = 0xF0701
};
enum : uint64_t { kStreamControl = 0, kStreamQpackEncoder = 2, kStreamQpackDecoder = 3 };
enum : uint64_t {
    kSetQpackMaxTableCapacity = 1,
    kSetMaxFieldSectionSize = 6,
    kSetQpackBlockedStreams = 7,
    kSetH3Datagram = 0x33,
    kSetH3DatagramDraft03 = 0x276
};
// H2O_HTTP3_ERROR_* (include/h2o/http3_common.h:56-77) as QUICLY_ERROR_FROM_APPLICATION_ERROR_CODE makes them
constexpr int32_t kGeneralProtocol = 0x30101, kFrameUnexpected = 0x30105, kFrame = 0x30106, kExcessiveLoad = 0x30107;
constexpr int32_t kIncomplete = -1;  // H2O_HTTP3_ERROR_INCOMPLETE: the walk reports it as status 0
constexpr uint32_t kNoSection = 0xFFFFFFFFu;
constexpr uint64_t kNone = ~0ull;

// ptls_decode_quicint: the bytes taken, 0 when the varint is cut short.
HHUFF_H3F_HD uint32_t varint(const uint8_t* p, uint64_t avail, uint64_t& v) {
    if (avail == 0) return 0;
    const uint32_t b = p[0];
    const uint32_t n = 1u << (b >> 6);
    if (avail < n) return 0;
    uint64_t x = b & 0x3fu;
    for (uint32_t i = 1; i < n; ++i) x = (x << 8) | p[i];
    v = x;
    return n;
}

struct Frame {
    uint64_t type, length;
    uint32_t hdr;  // bytes of the two varints
    uint32_t err;  // HHUFF_H3F_ERR_*
};

// The frame-type table of common.c:1096-1140.  control == false: a request stream.
HHUFF_H3F_HD bool type_allowed(uint64_t type, bool is_client, bool control) {
    switch (type) {
    case kData:
    case kHeaders:
        return !control;
    case kCancelPush:
    case kSettings:
    case kGoaway:
        return control;
    case kPushPromise:
        return !control && is_client;
    case kMaxPushId:
    case kPriorityUpdateRequest:
    case kPriorityUpdatePush:
        return control && !is_client;
    default:
        return true;
    }
}

// h2o_http3_read_frame: 0, kIncomplete, kGeneralProtocol (too large) or kFrameUnexpected.  On 0 the frame's bytes
// are p[0 .. F.hdr + F.length), for DATA p[0 .. F.hdr).  F.type is valid whenever the type varint was whole
// (F.hdr != 0 or the result is not kIncomplete), as handle_input_expect_headers needs it.
HHUFF_H3F_HD int32_t read_frame(const uint8_t* p, uint64_t avail, uint64_t max_frame_payload_size, bool is_client, bool control,
                                Frame& F) {
    F.type = kNone, F.length = 0, F.hdr = 0, F.err = HHUFF_H3F_ERR_NONE;
    uint64_t type = 0, length = 0;
    const uint32_t n1 = varint(p, avail, type);
    if (n1 == 0) return kIncomplete;
    const uint32_t n2 = varint(p + n1, avail - n1, length);
    if (n2 == 0) return kIncomplete;
    F.type = type, F.length = length, F.hdr = n1 + n2;
    if (type != kData) {
        if (length > max_frame_payload_size) {
            F.err = HHUFF_H3F_ERR_FRAME_TOO_LARGE;
            return kGeneralProtocol;
        }
        if (avail - F.hdr < length) return kIncomplete;
    }
    return type_allowed(type, is_client, control) ? 0 : kFrameUnexpected;
}

struct Settings {
    uint64_t max_field_section_size;  // kNone: the frame has none
    uint64_t max_table_capacity, max_blocked;
    uint32_t h3_datagram;
};

// h2o_http3_handle_settings_frame: 0 or kFrame ("malformed SETTINGS frame").
HHUFF_H3F_HD int32_t settings_payload(const uint8_t* p, uint64_t len, bool peer_datagrams, Settings& S) {
    uint64_t mfss = kNone, cap = 0, blocked = 0, pos = 0;
    uint32_t dgram = 0;
    bool bad = false;
    while (pos != len && !bad) {
        uint64_t id = 0, value = 0;
        const uint32_t n1 = varint(p + pos, len - pos, id);
        const uint32_t n2 = n1 ? varint(p + pos + n1, len - pos - n1, value) : 0u;
        if (n2 == 0) {
            bad = true;
        } else {
            pos += n1 + n2;
            if (id == kSetMaxFieldSectionSize) {
                mfss = value;
            } else if (id == kSetQpackMaxTableCapacity) {
                cap = value;
            } else if (id == kSetQpackBlockedStreams) {
                blocked = value;
            } else if (id == kSetH3Datagram || id == kSetH3DatagramDraft03) {
                if (value == 1 && peer_datagrams)
                    dgram = 1;
                else if (value != 0)
                    bad = true;
            }
        }
    }
    S = Settings{mfss, cap, blocked, dgram};
    return bad ? kFrame : 0;
}

// h2o_http3_decode_priority_update_frame: 0 or kFrame, never with an err_desc.  h2o assigns quicly_decodev's result to
// the 63-bit field frame->element before it compares with UINT64_MAX (frame.c:49), so its "invalid PRIORITY frame"
// branch is never taken: an element id cut short reads as 2^63 - 1 -- a server-initiated unidirectional stream, which
// the kind test below refuses for PRIORITY_UPDATE_REQUEST and accepts for _PUSH -- with the one byte
// ptls_decode_quicint had taken as the id's bytes.  idlen = the bytes of the element id.
HHUFF_H3F_HD int32_t priority_update_payload(const uint8_t* p, uint64_t len, bool is_push, uint32_t& idlen, uint32_t& err) {
    idlen = 0, err = HHUFF_H3F_ERR_NONE;
    if (len == 0) return kFrame;
    uint64_t element = 0;
    uint32_t n = varint(p, len, element);
    if (n == 0) element = 0x7fffffffffffffffull, n = 1;
    // quicly_stream_is_client_initiated: (id & 1) == 0; quicly_stream_is_unidirectional: (id & 2) != 0
    const bool client_initiated = (element & 1u) == 0, uni = (element & 2u) != 0;
    if (is_push ? !(!client_initiated && uni) : !(client_initiated && !uni)) return kFrame;
    idlen = n;
    return 0;
}

// h2o_http3_decode_goaway_frame: 0 or kFrame ("Invalid GOAWAY frame").
HHUFF_H3F_HD int32_t goaway_payload(const uint8_t* p, uint64_t len, uint32_t& idlen, uint32_t& err) {
    uint64_t id = 0;
    const uint32_t n = varint(p, len, id);
    const bool ok = n != 0 && n == len;
    idlen = ok ? n : 0u, err = ok ? HHUFF_H3F_ERR_NONE : HHUFF_H3F_ERR_INVALID_GOAWAY;
    return ok ? 0 : kFrame;
}

struct Params {
    uint64_t max_frame_payload_size;
    uint32_t is_client;
    uint32_t frame_cap;  // frame slots of this stream
};

struct Result {
    uint32_t nframes, consumed;
    int32_t status;
    uint32_t err;
    uint32_t nsec, sec_bytes, enc_bytes, got_settings;  // nsec and got_settings are 0 or 1
    uint64_t data_left;
    uint32_t kind, phase;
};

// A sink that keeps nothing: the counting walk.
struct NoSink {
    HHUFF_H3F_HD void frame(uint32_t, const hhuff_h3_frame_t&) {}
    HHUFF_H3F_HD void section(uint32_t, uint32_t) {}
    HHUFF_H3F_HD void encoder(uint32_t, uint32_t) {}
    HHUFF_H3F_HD void settings(const Settings&) {}
};

HHUFF_H3F_HD bool state_valid(const hhuff_h3_stream_t& st, bool is_client) {
    bool ok = (st.flags & ~(HHUFF_H3S_WALK_ON | HHUFF_H3S_TUNNEL | HHUFF_H3S_PEER_DATAGRAMS)) == 0;
    for (int i = 0; i < 13; ++i) ok = ok && st.rsv[i] == 0;
    if (st.kind == HHUFF_H3K_REQUEST)
        ok = ok && (st.phase == HHUFF_H3P_HEADERS || st.phase == HHUFF_H3P_DATA || st.phase == HHUFF_H3P_DATA_PAYLOAD ||
                    (st.phase == HHUFF_H3P_POST_TRAILERS && !is_client));
    else if (st.kind == HHUFF_H3K_CONTROL)
        ok = ok && (st.phase == HHUFF_H3P_SETTINGS || st.phase == HHUFF_H3P_OPEN);
    else
        ok = ok && st.kind <= HHUFF_H3K_DISCARD && st.phase == 0;
    const bool payload = st.kind == HHUFF_H3K_REQUEST && st.phase == HHUFF_H3P_DATA_PAYLOAD;
    return ok && (payload ? st.data_left != 0 : st.data_left == 0);
}

// One stream, p[0 .. len), in the state st.  The sink receives
//   frame(i, rec)       frame i of the stream; hdr_off and payload_off are relative to p; a HEADERS frame that is a
//                       section has aux 0 (the stream's only section), every other HEADERS frame kNoSection
//   section(off, n)     the stream's section: p[off .. off + n)
//   encoder(off, n)     a QPACK encoder stream's bytes
//   settings(S)         the SETTINGS frame the control stream passed
// R.kind, R.phase and R.data_left are the state to present next time.
template <class Sink>
HHUFF_H3F_HD void walk(const uint8_t* p, uint32_t len, const hhuff_h3_stream_t& st, const Params& P, Sink& sink, Result& R) {
    R = Result{0, 0, 0, HHUFF_H3F_ERR_NONE, 0, 0, 0, 0, st.data_left, st.kind, st.phase};
    const bool is_client = P.is_client != 0;
    if (!state_valid(st, is_client)) {
        R.status = HHUFF_H3F_EINVAL;
        return;
    }
    uint32_t pos = 0, kind = st.kind, phase = st.phase;
    uint64_t data_left = st.data_left;
    int32_t status = 0;
    uint32_t err = HHUFF_H3F_ERR_NONE;
    if (kind == HHUFF_H3K_UNI) {  // rule 8
        uint64_t type = 0;
        const uint32_t n = varint(p, len, type);
        if (n == 0) return;
        pos = n;
        kind = type == kStreamControl        ? HHUFF_H3K_CONTROL
               : type == kStreamQpackEncoder ? HHUFF_H3K_QPACK_ENCODER
               : type == kStreamQpackDecoder ? HHUFF_H3K_QPACK_DECODER
                                             : HHUFF_H3K_DISCARD;
        phase = kind == HHUFF_H3K_CONTROL ? HHUFF_H3P_SETTINGS : 0u;
    }
    if (kind == HHUFF_H3K_QPACK_ENCODER) {  // rule 9
        if (len != pos) sink.encoder(pos, len - pos);
        R.enc_bytes = len - pos, pos = len;
    } else if (kind == HHUFF_H3K_DISCARD) {  // rule 11; rule 10 (the decoder stream) keeps its bytes
        pos = len;
    } else if (kind == HHUFF_H3K_CONTROL) {
        while (pos != len) {
            Frame F;
            status = read_frame(p + pos, len - pos, P.max_frame_payload_size, is_client, true, F);  // rule 12
            err = F.err;
            if (status != 0) break;
            if ((phase == HHUFF_H3P_OPEN) == (F.type == kSettings)) {  // common.c:384-388 (DATA never passes the table)
                status = kFrameUnexpected;
                break;
            }
            const uint8_t* pay = p + pos + F.hdr;
            uint32_t aux = 0;
            Settings S{};
            if (F.type == kSettings)  // rule 13
                status = settings_payload(pay, F.length, (st.flags & HHUFF_H3S_PEER_DATAGRAMS) != 0, S),
                err = status ? HHUFF_H3F_ERR_MALFORMED_SETTINGS : HHUFF_H3F_ERR_NONE;
            else if (!is_client && (F.type == kPriorityUpdateRequest || F.type == kPriorityUpdatePush))
                status = priority_update_payload(pay, F.length, F.type == kPriorityUpdatePush, aux, err);
            else if (is_client && F.type == kGoaway)
                status = goaway_payload(pay, F.length, aux, err);
            if (status != 0) break;
            if (R.nframes == P.frame_cap) {  // rule 14
                status = HHUFF_H3F_FRAMES;
                break;
            }
            sink.frame(R.nframes, hhuff_h3_frame_t{F.type, pos, pos + F.hdr, F.length, (uint32_t)F.length, aux});
            ++R.nframes, pos += F.hdr + (uint32_t)F.length;
            if (F.type == kSettings) {
                sink.settings(S);
                R.got_settings = 1, phase = HHUFF_H3P_OPEN;
            }
        }
    } else if (kind == HHUFF_H3K_REQUEST) {
        const bool tunnel = (st.flags & HHUFF_H3S_TUNNEL) != 0;
        while (pos != len) {
            if (phase == HHUFF_H3P_DATA_PAYLOAD) {  // handle_input_expect_data_payload / handle_input_data_payload
                if (R.nframes == P.frame_cap) {
                    status = HHUFF_H3F_FRAMES;
                    break;
                }
                const uint32_t take = data_left < len - pos ? (uint32_t)data_left : len - pos;
                sink.frame(R.nframes, hhuff_h3_frame_t{kData, pos, pos, data_left, take, 0u});
                ++R.nframes, pos += take, data_left -= take;
                if (data_left == 0) phase = HHUFF_H3P_DATA;
                continue;
            }
            Frame F;
            status = read_frame(p + pos, len - pos, P.max_frame_payload_size, is_client, false, F);  // rule 1
            err = F.err;
            if (status == kIncomplete) break;
            if (phase == HHUFF_H3P_HEADERS) {
                if (status != 0) {
                    if (is_client)  // rule 6
                        status = kExcessiveLoad, err = HHUFF_H3F_ERR_RESPONSE_TOO_LARGE;
                    else if (err == HHUFF_H3F_ERR_FRAME_TOO_LARGE && F.type == kHeaders)  // rule 2
                        status = HHUFF_H3F_REJECTED;
                    break;
                }
                if (F.type == kData) {
                    status = kFrameUnexpected, err = is_client ? HHUFF_H3F_ERR_DATA_BEFORE_HEADERS : HHUFF_H3F_ERR_NONE;
                    break;
                }
            } else {
                if (status != 0) break;
                if (F.type == kHeaders && (phase == HHUFF_H3P_POST_TRAILERS || tunnel)) {  // rules 4, 5, 7
                    status = kFrameUnexpected;
                    err = phase == HHUFF_H3P_DATA && !is_client ? HHUFF_H3F_ERR_UNEXPECTED_TYPE : HHUFF_H3F_ERR_NONE;
                    break;
                }
                if (F.type == kData && phase == HHUFF_H3P_POST_TRAILERS) {
                    status = kFrameUnexpected;
                    break;
                }
            }
            if (R.nframes == P.frame_cap) {  // rule 14
                status = HHUFF_H3F_FRAMES;
                break;
            }
            if (F.type == kData) {  // phase _DATA: the bytes present are taken at once
                const uint64_t here = len - pos - F.hdr;
                const uint32_t take = F.length < here ? (uint32_t)F.length : (uint32_t)here;
                sink.frame(R.nframes, hhuff_h3_frame_t{kData, pos, pos + F.hdr, F.length, take, 0u});
                ++R.nframes, pos += F.hdr + take, data_left = F.length - take;
                if (data_left != 0) phase = HHUFF_H3P_DATA_PAYLOAD;
                continue;
            }
            const bool section = F.type == kHeaders && phase == HHUFF_H3P_HEADERS;  // rules 3, 6
            sink.frame(R.nframes, hhuff_h3_frame_t{F.type, pos, pos + F.hdr, F.length, (uint32_t)F.length,
                                                   F.type == kHeaders && !section ? kNoSection : 0u});
            ++R.nframes;
            if (section) {
                sink.section(pos + F.hdr, (uint32_t)F.length);
                R.nsec = 1, R.sec_bytes = (uint32_t)F.length, phase = HHUFF_H3P_DATA;
            } else if (F.type == kHeaders && !is_client) {
                phase = HHUFF_H3P_POST_TRAILERS;  // trailers (server.c:1428-1430); the client ignores them
            }
            pos += F.hdr + (uint32_t)F.length;
            if (section && (st.flags & HHUFF_H3S_WALK_ON) == 0) break;
        }
    }
    R.consumed = pos, R.status = status == kIncomplete ? 0 : status, R.err = status == kIncomplete ? HHUFF_H3F_ERR_NONE : err;
    R.data_left = data_left, R.kind = kind, R.phase = phase;
}

// The state record to present next time.
HHUFF_H3F_HD hhuff_h3_stream_t next_state(const hhuff_h3_stream_t& st, const Result& R) {
    if (R.status == HHUFF_H3F_EINVAL) return st;
    hhuff_h3_stream_t o{};
    o.stream_id = st.stream_id, o.data_left = R.data_left;
    o.kind = (uint8_t)R.kind, o.phase = (uint8_t)R.phase, o.flags = st.flags;
    return o;
}

}  // namespace h3f
}  // namespace hhuff
#endif
