// HTTP/2 stream table (include/hhuff.h (2k''')): h2o's server-side stream rules -- handle_headers_frame,
// handle_incoming_request, handle_trailing_headers, expect_continuation_of_headers, handle_data_frame,
// handle_request_body_chunk, update_stream_input_window, handle_priority_frame, handle_rst_stream_frame,
// handle_window_update_frame, the stream half of handle_settings_frame and handle_goaway_frame
// (lib/http2/connection.c:49-52, 451-460, 470-481, 518-607, 618-820, 976-1138, 1151-1286), h2o_http2_stream_open /
// _close / _reset (lib/http2/stream.c:36-105) and h2o_http2_stream_prepare_for_request
// (include/h2o/http2_internal.h:428-445) -- as plain functions over a connection's slab.  The device kernel
// (hhuff_h2streams.hip) and the host program (tools/h2streams_host.cpp) run this very code.
//   find / insert / remove       the table: open addressing, linear probes, deletion by backward shift
//   stream_open, stream_leave    h2o_http2_stream_open, and the counters of h2o_http2_stream_close
//   update_stream_input_window, request_body_chunk, data_frame, headers_open, incoming_request, trailing_headers,
//   priority_frame, rst_stream_frame, window_update_frame, apply_op      one h2o function each, on a copy of the state
//   step                         one frame against that copy: the event, the replies owed, what becomes of the entry
//   walk                         one connection: its ops, then its frames in wire order; the first failure stops it
#ifndef HHUFF_H2STREAMS_H
#define HHUFF_H2STREAMS_H
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_h2ctl.h"

namespace hhuff {
namespace h2s {

using h2c::Reply;

// H2O_HTTP2_ERROR_STREAM_CLOSED, _REFUSED_STREAM, _ENHANCE_YOUR_CALM, _INVALID_HEADER_CHAR (http2_common.h)
constexpr int32_t kProtocol = -1, kFlowControl = -3, kStreamClosed = -5, kRefusedStream = -7, kEnhanceYourCalm = -11;
constexpr int32_t kInvalidHeaderChar = -254;
constexpr uint32_t kHostStreamWindow = 65535;  // H2O_HTTP2_SETTINGS_HOST_STREAM_INITIAL_WINDOW_SIZE
constexpr uint32_t kMaxOwnReply = 26;          // a DATA frame: two WINDOW_UPDATEs, or one and a RST_STREAM
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kMaxEntries = 1u << 24;
constexpr uint64_t kNoLength = ~0ull;  // SIZE_MAX

// h2o_http2_stream_state_t up to the point where the request is the application's; h2o_http2_req_body_state_t
enum : uint8_t { kIdle = 0, kRecvHeaders = 1, kRecvBody = 2, kHanded = 3 };
enum : uint8_t { kBodyNone = 0, kBodyBeforeFirst = 1, kBodyOpen = 2, kBodyCloseDelivered = 3 };
enum : uint8_t { kTunnel = 1, kHasBody = 2 /* req_body.buf != NULL */, kStreamed = 4 /* req_body.streamed */, kPush = 8 };

struct Head {  // 32 bytes, the slab's first
    uint32_t pull_max_open, push_max_open;  // conn->pull_stream_ids.max_open, push_stream_ids.max_open
    uint32_t pull_open, priority_open;      // conn->num_streams.pull.open, .priority.open
    uint32_t count;                         // entries in the table
    uint32_t fill_epoch;                    // of the last hhuff_h2_streams_fill_sends
    uint32_t rsv[2];
};
struct Entry {  // 48 bytes; stream_id 0: the slot is free
    uint32_t stream_id;
    uint8_t state, body, flags, rsv;
    uint32_t bytes_unnotified;  // input_window.bytes_unnotified (below 2^32: see update_stream_input_window)
    uint32_t mark;              // the fill_epoch that listed it
    int64_t output_window, input_window;
    uint64_t received, content_length;  // req.req_body_bytes_received, req.content_length
};
static_assert(sizeof(Head) == 32 && sizeof(Entry) == 48, "slab layout");

// The table of max_entries streams has the smallest power of two of slots that is at least twice that, so a probe
// always meets a free slot.
HHUFF_CTL_HD uint32_t table_cap(uint32_t max_entries) {
    uint32_t cap = 4;
    while (cap < 2u * max_entries) cap <<= 1;
    return cap;
}
HHUFF_CTL_HD uint64_t slab_size(uint32_t max_entries) { return sizeof(Head) + (uint64_t)table_cap(max_entries) * sizeof(Entry); }

struct Table {
    Head* head;
    Entry* ent;
    uint32_t mask, max_entries;
};
HHUFF_CTL_HD Table table_at(uint8_t* slab, uint32_t max_entries) {
    return Table{reinterpret_cast<Head*>(slab), reinterpret_cast<Entry*>(slab + sizeof(Head)), table_cap(max_entries) - 1u, max_entries};
}
HHUFF_CTL_HD uint32_t home(const Table& T, uint32_t id) { return ((id * 0x9E3779B1u) >> 7) & T.mask; }

HHUFF_CTL_HD void clear(const Table& T) {
    *T.head = Head{0, 0, 0, 0, 0, 0, {0, 0}};
    for (uint32_t i = 0; i <= T.mask; ++i) T.ent[i].stream_id = 0;
}
// The slot of stream id, or kNone.  (Every loop over the table is bounded by its size, whatever a slab holds.)
HHUFF_CTL_HD uint32_t find(const Table& T, uint32_t id) {
    uint32_t i = home(T, id);
    for (uint32_t n = 0; n <= T.mask; ++n, i = (i + 1u) & T.mask) {
        const uint32_t s = T.ent[i].stream_id;
        if (s == id) return i;
        if (s == 0) break;
    }
    return kNone;
}
// E goes to the first free slot of its probe sequence; the caller has checked count < max_entries.
HHUFF_CTL_HD void insert(const Table& T, const Entry& E) {
    uint32_t i = home(T, E.stream_id);
    for (uint32_t n = 0; n <= T.mask; ++n, i = (i + 1u) & T.mask) {
        if (T.ent[i].stream_id == 0) {
            T.ent[i] = E;
            return;
        }
    }
}
// Slot i becomes free, and every entry behind it that a probe from its home would no longer reach moves up.
HHUFF_CTL_HD void remove(const Table& T, uint32_t i) {
    T.ent[i].stream_id = 0;
    uint32_t j = i;
    for (uint32_t n = 0; n < T.mask; ++n) {
        j = (j + 1u) & T.mask;
        const uint32_t s = T.ent[j].stream_id;
        if (s == 0) return;
        const uint32_t k = home(T, s);
        const bool stays = i <= j ? (i < k && k <= j) : (i < k || k <= j);  // its home lies in (i, j], cyclically
        if (stays) continue;
        T.ent[i] = T.ent[j];
        T.ent[j].stream_id = 0;
        i = j;
    }
}

struct Cfg {  // hhuff_h2_streams_params_t, checked
    uint32_t max_streams, max_streams_for_priority;
    uint32_t window_ext;  // active_stream_window_size - H2O_HTTP2_SETTINGS_HOST_STREAM_INITIAL_WINDOW_SIZE
    uint32_t flags, max_entries;
    uint64_t max_request_entity_size;
};

struct Event {
    uint32_t stream_id, a;
    int32_t status;
    uint32_t err, flags;
};
HHUFF_CTL_HD hhuff_h2_sev_t record_of(const Event& e) {
    return hhuff_h2_sev_t{e.stream_id, e.a, (int16_t)e.status, (uint16_t)e.err, e.flags};
}

// What a step works on: copies of the connection's counters and of the stream's entry (have: there is one), and the
// replies it owes.  Nothing reaches the slab before the walk knows that the replies fit.
struct Work {
    Head H;
    Entry E;
    bool have;
    Reply r0, r1;
};
HHUFF_CTL_HD void owe(Work& W, const Reply& r) {
    if (W.r0.len == 0)
        W.r0 = r;
    else
        W.r1 = r;
}
HHUFF_CTL_HD Reply rst_stream(uint32_t id, int32_t err) { return Reply{13, h2c::kRstStream, 0, id, (uint32_t)-err, 0}; }
HHUFF_CTL_HD Reply window_update_of(uint32_t id, uint32_t delta) { return Reply{13, h2c::kWindowUpdate, 0, id, delta, 0}; }

// h2o_http2_stream_open: an IDLE stream, counted in num_streams.priority
HHUFF_CTL_HD void stream_open(Work& W, uint32_t id, uint32_t initial_window_size) {
    W.E = Entry{id, kIdle, kBodyNone, 0, 0, 0, 0, (int64_t)initial_window_size, (int64_t)kHostStreamWindow, 0, kNoLength};
    W.have = true;
    ++W.H.priority_open;
}
// h2o_http2_stream_close (and _reset, which here is always a close: DESIGN.md (c)): the entry leaves its counter
HHUFF_CTL_HD void stream_leave(Work& W) {
    if ((W.E.flags & kPush) == 0) {
        uint32_t& n = W.E.state == kIdle ? W.H.priority_open : W.H.pull_open;
        if (n != 0) --n;
    }
    W.have = false;
}
// stream_send_error + h2o_http2_stream_reset
HHUFF_CTL_HD void reset_stream(Work& W, int32_t err, Event& ev) {
    owe(W, rst_stream(W.E.stream_id, err));
    stream_leave(W);
    ev.status = err, ev.flags |= HHUFF_H2SE_RESET_SENT;
}
HHUFF_CTL_HD int32_t refuse(Event& ev, int32_t status, uint32_t err) {
    ev.status = status, ev.err = err;
    return status;
}

// update_stream_input_window (connection.c:813-820).  h2o compares the size_t bytes_unnotified with the ssize_t
// window as unsigned numbers, so a window the peer has overdrawn owes nothing.  bytes_unnotified stays below the
// window, which is at most INT32_MAX, and delta is at most INT32_MAX: the sum fits 32 bits; h2o asserts that the
// increment sent is at most INT32_MAX, here it is cut to that.
HHUFF_CTL_HD void update_stream_input_window(Work& W, uint32_t delta, Event& ev) {
    const uint64_t unnotified = (uint64_t)W.E.bytes_unnotified + delta;
    if (unnotified >= (uint64_t)W.E.input_window) {
        const uint32_t inc = unnotified > (uint64_t)h2c::kInt32Max ? (uint32_t)h2c::kInt32Max : (uint32_t)unnotified;
        owe(W, window_update_of(W.E.stream_id, inc));
        (void)h2c::window_update(W.E.input_window, inc);
        W.E.bytes_unnotified = 0;
        ev.flags |= HHUFF_H2SE_WINDOW_UPDATE_SENT;
    } else {
        W.E.bytes_unnotified = (uint32_t)unnotified;
    }
}

// handle_request_body_chunk (connection.c:518-607) on a stream whose body is OPEN*
HHUFF_CTL_HD void request_body_chunk(Work& W, const Cfg& P, uint32_t len, bool end_stream, Event& ev) {
    const bool first = W.E.body == kBodyBeforeFirst;
    W.E.body = kBodyOpen;
    W.E.received += len;
    if (W.E.received > P.max_request_entity_size) return reset_stream(W, kRefusedStream, ev);
    if (W.E.content_length != kNoLength && (end_stream ? W.E.received != W.E.content_length : W.E.received > W.E.content_length))
        return reset_stream(W, kProtocol, ev);
    ev.a = len, ev.flags |= HHUFF_H2SE_BODY;
    if (end_stream) {
        if (W.E.state < kHanded) W.E.state = kHanded;
        W.E.body = kBodyCloseDelivered;
        ev.flags |= HHUFF_H2SE_REQUEST_COMPLETE;
    }
    if ((W.E.flags & kStreamed) != 0) return;
    if (first && !end_stream) {
        if ((P.flags & HHUFF_H2SP_STREAM_BODIES) != 0)
            W.E.flags |= kStreamed;  // execute_or_enqueue_request_core: the request is the caller's from here on
        else
            update_stream_input_window(W, P.window_ext, ev);
    }
}

// handle_data_frame behind the connection window (connection.c:991-1020); length is the frame's, data_len the
// payload's without padding
HHUFF_CTL_HD int32_t data_frame(Work& W, const Cfg& P, uint32_t id, uint32_t length, uint32_t data_len, bool end_stream, Event& ev) {
    if (!W.have) {
        if (id > W.H.pull_max_open) return refuse(ev, kProtocol, HHUFF_H2ST_ERR_DATA_FRAME);
        owe(W, rst_stream(id, kStreamClosed));
        ev.status = kStreamClosed, ev.flags |= HHUFF_H2SE_RESET_SENT;
        return 0;
    }
    if (!(W.E.body == kBodyBeforeFirst || W.E.body == kBodyOpen)) {
        reset_stream(W, kStreamClosed, ev);
        return 0;
    }
    W.E.input_window -= (int64_t)length;
    if (length != data_len) update_stream_input_window(W, length - data_len, ev);
    if (data_len != 0 || end_stream) request_body_chunk(W, P, data_len, end_stream, ev);
    return 0;
}

// handle_headers_frame up to the point where the block is complete (connection.c:1032-1080): 0, or the failure.
// Afterwards W.E.state tells what the block is: RECV_HEADERS a request head, else trailers.
HHUFF_CTL_HD int32_t headers_open(Work& W, const Cfg& P, uint32_t id, uint32_t block_flags, uint32_t initial_window_size, Event& ev) {
    if ((id & 1u) == 0) return refuse(ev, kProtocol, HHUFF_H2ST_ERR_HEADERS_STREAM_ID);
    if (id <= W.H.pull_max_open) {
        if (!W.have) return refuse(ev, kStreamClosed, HHUFF_H2ST_ERR_HEADERS_CLOSED);
        if (!(W.E.body == kBodyBeforeFirst || W.E.body == kBodyOpen)) return refuse(ev, kProtocol, HHUFF_H2ST_ERR_HEADERS_STREAM_ID);
        if ((W.E.flags & kTunnel) != 0) return refuse(ev, kProtocol, HHUFF_H2ST_ERR_TUNNEL_TRAILERS);
        if ((block_flags & HHUFF_H2B_END_STREAM) == 0) return refuse(ev, kProtocol, HHUFF_H2ST_ERR_TRAILERS_END_STREAM);
        return 0;
    }
    if ((block_flags & HHUFF_H2B_SELF_DEPENDENCY) != 0) return refuse(ev, kProtocol, HHUFF_H2ST_ERR_SELF_DEPENDENCY);
    if (!W.have) {
        if (W.H.count >= P.max_entries) return refuse(ev, HHUFF_H2ST_EFULL, HHUFF_H2ST_ERR_NONE);
        stream_open(W, id, initial_window_size);
    }
    // h2o_http2_stream_prepare_for_request
    W.H.pull_max_open = id;
    if (W.E.state == kIdle) {
        if (W.H.priority_open != 0) --W.H.priority_open;
        ++W.H.pull_open;
    }
    W.E.state = kRecvHeaders;
    W.E.output_window = initial_window_size;
    if ((block_flags & HHUFF_H2B_END_STREAM) == 0) W.E.flags |= kHasBody;
    return 0;
}

struct Bytes {
    const uint8_t* p;  // NULL: h2o's iovec has no base
    uint32_t len;
};
HHUFF_CTL_HD bool bytes_are(const Bytes& s, const char* lit, uint32_t n) {
    if (s.p == nullptr || s.len != n) return false;
    for (uint32_t i = 0; i < n; ++i)
        if (s.p[i] != (uint8_t)lit[i]) return false;
    return true;
}

// handle_incoming_request (connection.c:618-740) behind h2o_hpack_parse_request: bstatus is its return value,
// exists_map and content_length what it left, method and path the bytes of those fields
HHUFF_CTL_HD int32_t incoming_request(Work& W, const Cfg& P, int32_t bstatus, uint32_t exists_map, uint64_t content_length,
                                      const Bytes& method, const Bytes& path, uint32_t block, Event& ev) {
    if (bstatus != 0 && bstatus != kInvalidHeaderChar) return refuse(ev, bstatus, HHUFF_H2ST_ERR_HEADER_BLOCK);
    constexpr uint32_t kMethod = 1, kScheme = 2, kPath = 4, kAuthority = 8, kProtocolExists = 16;  // hpack.h:81-85
    bool is_connect = false, ok = true;
    uint32_t must, may = 0;
    if (bytes_are(method, "CONNECT", 7)) {
        is_connect = true;
        must = kMethod | kAuthority;
        if ((exists_map & kProtocolExists) != 0) must |= kScheme | kPath | kProtocolExists;
    } else if (bytes_are(method, "CONNECT-UDP", 11)) {
        ok = (exists_map & kProtocolExists) == 0 && bytes_are(path, "/", 1);
        is_connect = true;
        must = kMethod | kScheme | kAuthority | kPath;
    } else {
        must = kMethod | kScheme | kPath;
        may = kAuthority;
    }
    if (!(ok && (exists_map & must) == must && (exists_map & ~(must | may)) == 0)) {
        reset_stream(W, kProtocol, ev);
        return 0;
    }
    if (W.H.pull_open > P.max_streams) {
        reset_stream(W, kRefusedStream, ev);
        return 0;
    }
    ev.a = block, ev.flags |= HHUFF_H2SE_OPENED;
    W.E.content_length = content_length;
    if (bstatus != 0) {  // send_invalid_request_error: the 400 is the caller's
        W.E.state = kHanded;
        ev.flags |= HHUFF_H2SE_INVALID_HEADER_CHAR;
        return 0;
    }
    if (is_connect) {
        if (content_length != kNoLength || (W.E.flags & kHasBody) == 0) {
            W.E.state = kHanded;
            ev.flags |= HHUFF_H2SE_BAD_CONNECT;
            return 0;
        }
        // ProcessImmediately: process_request with proceed_req set extends the window at once (connection.c:180-182)
        W.E.flags |= kTunnel | kStreamed;
        W.E.state = kRecvBody, W.E.body = kBodyOpen;
        update_stream_input_window(W, P.window_ext, ev);
        return 0;
    }
    if ((W.E.flags & kHasBody) == 0) {
        W.E.state = kHanded;
        ev.flags |= HHUFF_H2SE_REQUEST_COMPLETE;
    } else {
        W.E.state = kRecvBody, W.E.body = kBodyBeforeFirst;
    }
    return 0;
}

// handle_trailing_headers (connection.c:742-755).  h2o parses trailers with NULL pseudo-header pointers
// (hpack.c:533-586, 601): the first pseudo-header is "invalid pseudo header" and a host field falls through to the
// connection-specific refusal, both in front of whatever the head rules found later in the block; any other
// non-zero return, the soft -254 included, is the connection's.  has_host: the record's authority came from a host
// field (exists_map has no authority bit).
HHUFF_CTL_HD int32_t trailing_headers(Work& W, const Cfg& P, int32_t bstatus, uint32_t exists_map, bool has_host, Event& ev) {
    if (exists_map != 0) return refuse(ev, kProtocol, HHUFF_H2ST_ERR_TRAILERS_PSEUDO_HEADER);
    if (has_host) return refuse(ev, kProtocol, HHUFF_H2ST_ERR_TRAILERS_HOST);
    if (bstatus != 0) return refuse(ev, bstatus, HHUFF_H2ST_ERR_HEADER_BLOCK);
    ev.flags |= HHUFF_H2SE_TRAILERS;
    request_body_chunk(W, P, 0, true, ev);
    if ((ev.flags & HHUFF_H2SE_RESET_SENT) == 0) ev.flags &= ~HHUFF_H2SE_BODY, ev.a = 0;  // (an empty chunk delivers nothing)
    return 0;
}

// handle_priority_frame behind its payload rules (connection.c:1110-1137); the tree is the caller's
HHUFF_CTL_HD int32_t priority_frame(Work& W, const Cfg& P, uint32_t id, uint32_t initial_window_size, Event& ev) {
    if (W.have) {
        ev.flags |= HHUFF_H2SE_PRIORITY;
        return 0;
    }
    if ((id & 1u) == 0 || id <= W.H.pull_max_open) {
        ev.flags |= HHUFF_H2SE_IGNORED;
        return 0;
    }
    if (W.H.priority_open >= P.max_streams_for_priority) return refuse(ev, kEnhanceYourCalm, HHUFF_H2ST_ERR_TOO_MANY_IDLE);
    if (W.H.count >= P.max_entries) return refuse(ev, HHUFF_H2ST_EFULL, HHUFF_H2ST_ERR_NONE);
    stream_open(W, id, initial_window_size);
    ev.flags |= HHUFF_H2SE_PRIORITY_ONLY_OPENED;
    return 0;
}

HHUFF_CTL_HD bool is_idle_stream_id(const Head& H, uint32_t id) { return ((id & 1u) == 0 ? H.push_max_open : H.pull_max_open) < id; }

// handle_rst_stream_frame (connection.c:1271-1285)
HHUFF_CTL_HD int32_t rst_stream_frame(Work& W, uint32_t id, Event& ev) {
    if (is_idle_stream_id(W.H, id)) return refuse(ev, kProtocol, HHUFF_H2ST_ERR_RST_STREAM_STREAM_ID);
    if (W.have) {
        stream_leave(W);
        ev.flags |= HHUFF_H2SE_RESET_BY_PEER;
    } else {
        ev.flags |= HHUFF_H2SE_IGNORED;
    }
    return 0;
}

// update_stream_output_window (connection.c:470-481): false when the window would pass INT32_MAX
HHUFF_CTL_HD bool update_stream_output_window(Entry& E, int64_t delta, bool& opened) {
    const int64_t cur = E.output_window;
    opened = false;
    if (cur + delta > h2c::kInt32Max) return false;
    E.output_window = cur + delta;
    opened = cur <= 0 && E.output_window > 0;
    return true;
}

// handle_window_update_frame on a stream (connection.c:1194-1226); stream_error: the control record's STREAM_ERROR
// (increment 0: its RST_STREAM is among the control replies)
HHUFF_CTL_HD int32_t window_update_frame(Work& W, uint32_t id, uint32_t increment, bool stream_error, Event& ev) {
    if (stream_error) {
        if (W.have) stream_leave(W);
        ev.status = kProtocol, ev.flags |= HHUFF_H2SE_RESET_SENT;
        return 0;
    }
    if (is_idle_stream_id(W.H, id)) return refuse(ev, kProtocol, HHUFF_H2ST_ERR_WINDOW_UPDATE_STREAM_ID);
    if (!W.have) {
        ev.flags |= HHUFF_H2SE_IGNORED;
        return 0;
    }
    bool opened;
    if (!update_stream_output_window(W.E, increment, opened)) {
        const uint32_t sid = W.E.stream_id;
        stream_leave(W);
        owe(W, rst_stream(sid, kFlowControl));
        ev.status = kFlowControl, ev.flags |= HHUFF_H2SE_RESET_SENT;
    } else if (opened) {
        ev.flags |= HHUFF_H2SE_SEND_WINDOW_OPENED;
    }
    return 0;
}

// What the application side does to a stream between steps: the op's own status (0, HHUFF_H2ST_EINVAL / _ENOENT /
// _EFULL), never the connection's
HHUFF_CTL_HD int32_t apply_op(Work& W, const Cfg& P, const hhuff_h2_stream_op_t& op, uint32_t initial_window_size, Event& ev) {
    if (op.stream_id == 0 || op.stream_id > 0x7fffffffu || op.rsv != 0) return HHUFF_H2ST_EINVAL;
    if (op.op == HHUFF_H2O_CLOSE) {
        if (!W.have) return HHUFF_H2ST_ENOENT;
        stream_leave(W);
        return 0;
    }
    if (op.op == HHUFF_H2O_CREDIT) {
        if (!W.have) return HHUFF_H2ST_ENOENT;
        if (op.arg > 0x7fffffffu) return HHUFF_H2ST_EINVAL;
        update_stream_input_window(W, op.arg, ev);
        return 0;
    }
    if (op.op == HHUFF_H2O_OPEN_PUSH) {  // h2o_http2_conn_push_path: no push once the ids run out or GOAWAY has come
        if ((op.stream_id & 1u) != 0 || W.have || W.H.push_max_open >= 0x7ffffff0u) return HHUFF_H2ST_EINVAL;
        if (W.H.count >= P.max_entries) return HHUFF_H2ST_EFULL;
        W.E = Entry{op.stream_id, kHanded, kBodyNone, kPush, 0, 0, 0, (int64_t)initial_window_size, (int64_t)kHostStreamWindow, 0, kNoLength};
        W.have = true;
        if (W.H.push_max_open < op.stream_id) W.H.push_max_open = op.stream_id;
        return 0;
    }
    return HHUFF_H2ST_EINVAL;
}

// The SETTINGS sweep (connection.c:1178-1183): delta on every stream's send window; a stream whose sum would pass
// INT32_MAX keeps its window.  Returns the streams whose window opened.
HHUFF_CTL_HD uint32_t sweep_output_windows(const Table& T, int32_t delta) {
    uint32_t n = 0;
    for (uint32_t i = 0; i <= T.mask; ++i) {
        if (T.ent[i].stream_id == 0) continue;
        Entry E = T.ent[i];
        bool opened;
        if (update_stream_output_window(E, delta, opened)) T.ent[i].output_window = E.output_window;
        n += opened ? 1u : 0u;
    }
    return n;
}

// One connection's arrays (the call's, as they are) and the ranges of them that are its own.
struct Conn {
    const uint8_t* in;
    uint64_t in_size;
    const hhuff_h2_frame_t* frames;  // the whole array: block records name absolute indices
    const hhuff_h2_ctl_t* ctl;
    uint32_t f0, n;                  // its frame slots f0 .. f0 + n - 1 are walked
    const uint8_t* ctl_rep;          // its control replies ctl_rep[0 .. ctl_rep_len)
    uint32_t ctl_rep_len;
    const hhuff_h2_block_t* blocks;
    const int32_t* bstatus;
    const hhuff_request_t* req;
    uint32_t b0, b1;                 // its blocks, below frm_cap
    const uint8_t* arena;
    uint64_t arena_size;
    const uint32_t* blk_off;
    const uint32_t* value_off;
    const uint32_t* value_len;
    uint32_t initial_window_size;    // peers[c].initial_window_size: the peer's setting behind the step's last frame
    const hhuff_h2_stream_op_t* ops; // its ops ops[0 .. nops)
    uint32_t nops;
    hhuff_h2_sev_t* sev;             // the whole array
    hhuff_h2_sev_t* op_sev;          // its first
    uint8_t* rep;                    // its region rep[0 .. rep_cap)
    uint32_t rep_cap;
};
struct Result {
    uint32_t nstr, rep_len;
    int32_t status;
    uint32_t err;
};

// the bytes of field `field` of block b (a request record's method or path), or false when they leave the arrays
HHUFF_CTL_HD bool field_value(const Conn& C, uint32_t b, int32_t field, Bytes& out) {
    out = Bytes{nullptr, 0};
    if (field < 0) return true;
    const uint64_t slot = (uint64_t)C.blk_off[b] + (uint32_t)field;
    if (slot >= C.blk_off[b + 1] || slot >= C.in_size) return false;
    const uint64_t off = C.value_off[slot], len = C.value_len[slot];
    if (off + len > C.arena_size) return false;
    out = Bytes{C.arena + off, (uint32_t)len};
    return true;
}

// handle_incoming_request or handle_trailing_headers for block b, as expect_continuation_of_headers picks
// (connection.c:784-790)
HHUFF_CTL_HD int32_t block_end(Work& W, const Cfg& P, const Conn& C, uint32_t b, Event& ev) {
    const int32_t bst = C.bstatus[b];
    const hhuff_request_t R = C.req[b];
    if (W.E.state != kRecvHeaders) return trailing_headers(W, P, bst, R.exists_map, (R.exists_map & 8u) == 0 && R.authority >= 0, ev);
    Bytes method, path;
    if (!field_value(C, b, R.method, method) || !field_value(C, b, R.path, path)) return refuse(ev, HHUFF_H2ST_EINVAL, HHUFF_H2ST_ERR_NONE);
    return incoming_request(W, P, bst, R.exists_map, R.content_length, method, path, b, ev);
}

// One frame (slot i, absolute) against the copy W: the connection-level status -- 0, h2o's error, or
// HHUFF_H2ST_EINVAL / _EFULL with nothing of W to be kept.  key: the stream the frame is about (0: none); W has
// been loaded for it.
HHUFF_CTL_HD uint32_t key_of(const Conn& C, const hhuff_h2_frame_t& F, const hhuff_h2_ctl_t& K, bool& bad) {
    bad = false;
    if (F.type == h2c::kHeaders || F.type == h2c::kContinuation) {
        if (F.block < C.b0 || F.block >= C.b1) {
            bad = true;
            return 0;
        }
        return C.blocks[F.block].stream_id;
    }
    if (F.type == h2c::kData || F.type == h2c::kPriority || F.type == h2c::kRstStream) return F.stream_id;
    if (F.type == h2c::kWindowUpdate && (K.flags & HHUFF_H2R_NEEDS_STREAM) != 0) return F.stream_id;
    return 0;
}

HHUFF_CTL_HD int32_t step(Work& W, const Cfg& P, const Conn& C, uint32_t iws, uint32_t i, const hhuff_h2_frame_t& F, const hhuff_h2_ctl_t& K,
                          Event& ev) {
    if (F.type == h2c::kData) {
        if (K.b > F.length) return refuse(ev, HHUFF_H2ST_EINVAL, HHUFF_H2ST_ERR_NONE);
        return data_frame(W, P, F.stream_id, F.length, K.b, (F.flags & 1u) != 0, ev);
    }
    if (F.type == h2c::kHeaders || F.type == h2c::kContinuation) {
        const hhuff_h2_block_t B = C.blocks[F.block];
        const bool inside = i >= B.first_frame && i - B.first_frame < B.nframes;
        const bool first = i == B.first_frame, last = inside && i - B.first_frame == B.nframes - 1u;
        if (!inside || (B.flags & HHUFF_H2B_PROMISE) != 0 || first != (F.type == h2c::kHeaders) || B.stream_id == 0)
            return refuse(ev, HHUFF_H2ST_EINVAL, HHUFF_H2ST_ERR_NONE);
        if (first) {
            const int32_t r = headers_open(W, P, B.stream_id, B.flags, iws, ev);
            if (r != 0) return r;
        } else {
            if (F.stream_id != B.stream_id) return refuse(ev, kProtocol, HHUFF_H2ST_ERR_CONTINUATION_STREAM_ID);
            if (!W.have) return refuse(ev, HHUFF_H2ST_EINVAL, HHUFF_H2ST_ERR_NONE);  // (no opener was walked)
        }
        return last ? block_end(W, P, C, F.block, ev) : 0;
    }
    if (F.type == h2c::kPriority) return priority_frame(W, P, F.stream_id, iws, ev);
    if (F.type == h2c::kRstStream) return rst_stream_frame(W, F.stream_id, ev);
    if (F.type == h2c::kWindowUpdate && (K.flags & HHUFF_H2R_NEEDS_STREAM) != 0)
        return window_update_frame(W, F.stream_id, K.a, (K.flags & HHUFF_H2R_STREAM_ERROR) != 0, ev);
    if (F.type == h2c::kGoaway) W.H.push_max_open = 0x7ffffffeu;  // stop opening new push streams (connection.c:1242)
    return 0;
}

// What W says became of the entry goes to the table, the counters to the slab's copy.
HHUFF_CTL_HD void commit(const Table& T, Head& H, const Work& W, uint32_t slot) {
    H = W.H;
    if (slot != kNone) {
        if (W.have) {
            T.ent[slot] = W.E;
        } else {
            remove(T, slot);
            --H.count;
        }
    } else if (W.have) {
        insert(T, W.E);
        ++H.count;
    }
}

// One connection: the table T (fresh: it starts empty), its ops and then its frames.  The replies are the merged
// stream: per frame the control call's bytes, then this call's own.  A frame is stepped on a copy, so that a reply
// that does not fit leaves nothing of it behind.
HHUFF_CTL_HD void walk(const Conn& C, const Cfg& P, const Table& T, bool fresh, Result& R) {
    R = Result{0, 0, 0, HHUFF_H2ST_ERR_NONE};
    if (fresh) clear(T);
    Head H = *T.head;
    if (H.count > P.max_entries) H.count = P.max_entries;  // (a slab that was never this family's)
    const Reply none{0, 0, 0, 0, 0, 0};
    // h2o opens a stream with the setting of that moment: the setting in front of the step's first frame is the one
    // behind its last less every change the control call recorded, and each SETTINGS frame moves it on
    uint32_t iws = C.initial_window_size;
    for (uint32_t i = C.f0; i < C.f0 + C.n; ++i)
        if (C.frames[i].type == h2c::kSettings && (C.ctl[i].flags & HHUFF_H2R_WINDOW_DELTA) != 0) iws -= C.ctl[i].b;
    for (uint32_t k = 0; k < C.nops; ++k) {
        const hhuff_h2_stream_op_t op = C.ops[k];
        Work W{H, Entry{}, false, none, none};
        const uint32_t slot = op.stream_id != 0 ? find(T, op.stream_id) : kNone;
        if (slot != kNone) W.E = T.ent[slot], W.have = true;
        Event ev{op.stream_id, 0, 0, HHUFF_H2ST_ERR_NONE, 0};
        const int32_t r = apply_op(W, P, op, iws, ev);
        if (r != 0) {
            C.op_sev[k] = record_of(Event{op.stream_id, 0, r, HHUFF_H2ST_ERR_NONE, 0});
            continue;
        }
        if (W.r0.len > C.rep_cap - R.rep_len) {
            *T.head = H;
            R.status = HHUFF_H2ST_SPACE;
            return;
        }
        h2c::emit(C.rep + R.rep_len, W.r0);
        R.rep_len += W.r0.len;
        commit(T, H, W, slot);
        C.op_sev[k] = record_of(ev);
    }
    uint32_t ctl_pos = 0;
    if (C.n != 0) {
        // (the next records are loaded before this frame's stores are issued: a lane's chain of loads does not wait)
        hhuff_h2_frame_t Fn = C.frames[C.f0];
        hhuff_h2_ctl_t Kn = C.ctl[C.f0];
        for (uint32_t i = C.f0; i < C.f0 + C.n; ++i) {
            const hhuff_h2_frame_t F = Fn;
            const hhuff_h2_ctl_t K = Kn;
            const uint32_t j = i + 1u < C.f0 + C.n ? i + 1u : i;
            Fn = C.frames[j], Kn = C.ctl[j];
            bool bad;
            const uint32_t key = key_of(C, F, K, bad);
            if (bad || K.reply_len > C.ctl_rep_len - ctl_pos) {
                R.status = HHUFF_H2ST_EINVAL;
                break;
            }
            Work W{H, Entry{}, false, none, none};
            const uint32_t slot = key != 0 ? find(T, key) : kNone;
            if (slot != kNone) W.E = T.ent[slot], W.have = true;
            Event ev{key, 0, 0, HHUFF_H2ST_ERR_NONE, 0};
            const int32_t r = step(W, P, C, iws, i, F, K, ev);
            if (r == HHUFF_H2ST_EINVAL || r == HHUFF_H2ST_EFULL) {
                R.status = r;
                break;
            }
            const uint32_t own = r != 0 ? 0u : W.r0.len + W.r1.len;
            if ((uint64_t)K.reply_len + own > C.rep_cap - R.rep_len) {
                R.status = HHUFF_H2ST_SPACE;
                break;
            }
            for (uint32_t q = 0; q < K.reply_len; ++q) C.rep[R.rep_len + q] = C.ctl_rep[ctl_pos + q];
            R.rep_len += K.reply_len, ctl_pos += K.reply_len;
            if (r == 0) {
                h2c::emit(C.rep + R.rep_len, W.r0);
                h2c::emit(C.rep + R.rep_len + W.r0.len, W.r1);
                R.rep_len += own;
            }
            commit(T, H, W, slot);  // (after a failure too: the connection is left as h2o leaves its own)
            if (r == 0 && F.type == h2c::kSettings && (K.flags & HHUFF_H2R_WINDOW_DELTA) != 0) {
                ev.a = sweep_output_windows(T, (int32_t)K.b);
                iws += K.b;
                if (ev.a != 0) ev.flags |= HHUFF_H2SE_SEND_WINDOW_OPENED;
            }
            C.sev[i] = record_of(ev);
            if (r != 0) {
                R.status = r, R.err = ev.err;
                break;
            }
            ++R.nstr;
        }
    }
    *T.head = H;
}

// hhuff_h2_streams_fill_sends for one connection: sends[0 .. n), miss[0 .. n)
HHUFF_CTL_HD void fill_sends(const Table& T, hhuff_h2_send_t* sends, uint32_t n, uint8_t* miss) {
    uint32_t epoch = T.head->fill_epoch + 1u;
    if (epoch == 0) epoch = 1;
    T.head->fill_epoch = epoch;
    for (uint32_t r = 0; r < n; ++r) {
        const uint32_t id = sends[r].stream_id;
        const uint32_t slot = id != 0 ? find(T, id) : kNone;
        int32_t window = 0;
        uint8_t m = 1;
        if (slot != kNone) {
            if (T.ent[slot].mark == epoch) {
                m = 2;
            } else {
                const int64_t w = T.ent[slot].output_window;
                window = w > h2c::kInt32Max ? (int32_t)h2c::kInt32Max : (w < -h2c::kInt32Max ? (int32_t)-h2c::kInt32Max : (int32_t)w);
                T.ent[slot].mark = epoch;
                m = 0;
            }
        }
        sends[r].window = window, miss[r] = m;
    }
}
// hhuff_h2_streams_commit_sent: a stream the last fill listed pays what its record sent, once
HHUFF_CTL_HD void commit_sent(const Table& T, const hhuff_h2_send_t* sends, const hhuff_h2_sent_t* sent, uint32_t n) {
    const uint32_t epoch = T.head->fill_epoch;
    for (uint32_t r = 0; r < n; ++r) {
        const uint32_t id = sends[r].stream_id;
        const uint32_t slot = id != 0 ? find(T, id) : kNone;
        if (slot == kNone || epoch == 0 || T.ent[slot].mark != epoch) continue;
        T.ent[slot].output_window -= (int64_t)sent[r].sent;
        T.ent[slot].mark = 0;
    }
}

}  // namespace h2s
}  // namespace hhuff
#endif
