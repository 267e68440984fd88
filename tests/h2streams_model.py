"""A plain model of the HTTP/2 stream table (include/hhuff.h (2k''')), written from h2o's lib/http2/connection.c:49-52,
451-460, 470-481, 518-607, 618-820, 976-1138, 1151-1286, lib/http2/stream.c:36-105 and include/h2o/http2_internal.h:320-445
-- not from h2o_amd/csrc/hhuff_h2streams.h.  One function per h2o function; a connection is a dict, a stream a dict in
conn["streams"].  DEFECTS names deliberate mistakes a corpus has to tell from the rules.

A step's input is what the three calls in front leave, in Python form (build() makes the calls' arrays of it):
    frames   [dict(type, flags, stream_id, length, ctl=(a, b, flags), ctl_reply=bytes, block=index or None)]
    blocks   [dict(stream_id, flags, first_frame, nframes, bstatus, exists_map, content_length, method, path, host)]
             first_frame within the connection; method / path: bytes or None; host: authority came from a host field
    ops      [(stream_id, op, arg)]
"""
import numpy as np

DATA, HEADERS, PRIORITY, RST_STREAM, SETTINGS, PUSH_PROMISE, PING, GOAWAY, WINDOW_UPDATE, CONTINUATION = range(10)
PROTOCOL, FLOW_CONTROL, STREAM_CLOSED, REFUSED_STREAM, ENHANCE_YOUR_CALM, INVALID_HEADER_CHAR = -1, -3, -5, -7, -11, -254
SPACE, EINVAL, EFULL, ENOENT, ESLOT = -315, -316, -317, -318, -319
INT32_MAX = 0x7fffffff
NO_LENGTH = (1 << 64) - 1
HOST_STREAM_WINDOW = 65535
CONTINUE, STREAM_BODIES = 1, 1
OP_CLOSE, OP_CREDIT, OP_OPEN_PUSH = 1, 2, 3
# event flags
(OPENED, BODY, REQUEST_COMPLETE, TRAILERS, RESET_BY_PEER, RESET_SENT, WINDOW_UPDATE_SENT, IGNORED, PRIORITY_ONLY_OPENED,
 SEND_WINDOW_OPENED, BAD_CONNECT, INVALID_HEADER, PRIORITY_EV) = (1 << i for i in range(13))
ALL_EVENT_FLAGS = tuple(1 << i for i in range(13))
# control record flags and block flags the rules read
R_NEEDS_STREAM, R_STREAM_ERROR, R_WINDOW_DELTA = 2, 4, 8
B_END_STREAM, B_PROMISE, B_SELF_DEPENDENCY = 1, 16, 32
M_METHOD, M_SCHEME, M_PATH, M_AUTHORITY, M_PROTOCOL = 1, 2, 4, 8, 16
(E_NONE, E_HEADERS_STREAM_ID, E_HEADERS_CLOSED, E_TUNNEL_TRAILERS, E_TRAILERS_END_STREAM, E_SELF_DEPENDENCY,
 E_CONTINUATION_STREAM_ID, E_DATA_FRAME, E_TOO_MANY_IDLE, E_RST_STREAM_STREAM_ID, E_WINDOW_UPDATE_STREAM_ID,
 E_TRAILERS_PSEUDO_HEADER, E_TRAILERS_HOST, E_HEADER_BLOCK) = range(14)
ERR_TEXT = {E_NONE: None, E_HEADERS_STREAM_ID: "invalid stream id in HEADERS frame",
            E_HEADERS_CLOSED: "closed stream id in HEADERS frame", E_TUNNEL_TRAILERS: "trailer cannot be used in a CONNECT request",
            E_TRAILERS_END_STREAM: "trailing HEADERS frame MUST have END_STREAM flag set",
            E_SELF_DEPENDENCY: "stream cannot depend on itself", E_CONTINUATION_STREAM_ID: "unexpected stream id in CONTINUATION frame",
            E_DATA_FRAME: "invalid DATA frame", E_TOO_MANY_IDLE: "too many streams in idle/closed state",
            E_RST_STREAM_STREAM_ID: "unexpected stream id in RST_STREAM frame",
            E_WINDOW_UPDATE_STREAM_ID: "invalid stream id in WINDOW_UPDATE frame", E_TRAILERS_PSEUDO_HEADER: "invalid pseudo header",
            E_TRAILERS_HOST: "found an unexpected connection-specific header", E_HEADER_BLOCK: None}
ALL_ERR = tuple(range(14))
# stream states, body states
IDLE, RECV_HEADERS, RECV_BODY, HANDED = range(4)
BODY_NONE, BODY_BEFORE_FIRST, BODY_OPEN, BODY_CLOSE_DELIVERED = range(4)

DEFECTS = ("trailers_without_end_stream", "closed_headers_is_protocol", "max_streams_inclusive", "priority_limit_exclusive",
           "end_length_unchecked", "entity_limit_inclusive", "padding_not_credited", "signed_window_compare", "no_first_frame_extension",
           "window_overflow_inclusive", "delta_overflow_resets", "rst_idle_ignores_parity", "goaway_keeps_push_ids",
           "own_reply_first", "space_applies", "data_on_idle_is_closed", "connect_needs_no_authority",
           "tunnel_trailers", "credit_missing_stream_ok", "no_window_opened_event", "soft_trailers_pass")


def params(max_streams=100, max_streams_for_priority=16, active_stream_window_size=HOST_STREAM_WINDOW, max_entries=None,
           max_request_entity_size=1 << 30, flags=0):
    if max_entries is None:
        max_entries = max_streams + 1 + max_streams_for_priority + 4
    return dict(max_streams=max_streams, max_streams_for_priority=max_streams_for_priority,
                active_stream_window_size=active_stream_window_size, max_entries=max_entries,
                max_request_entity_size=max_request_entity_size, flags=flags)


def new_conn():
    return dict(pull_max_open=0, push_max_open=0, pull_open=0, priority_open=0, streams={})


def be32(v):
    return int(v & 0xffffffff).to_bytes(4, "big")


def frame_bytes(typ, flags, sid, payload):
    return len(payload).to_bytes(3, "big") + bytes([typ, flags]) + be32(sid) + payload


def rst_stream_bytes(sid, err):
    return frame_bytes(RST_STREAM, 0, sid, be32(-err))


def window_update_bytes(sid, inc):
    return frame_bytes(WINDOW_UPDATE, 0, sid, be32(inc))


class Fail(Exception):
    def __init__(self, status, err=E_NONE):
        self.status, self.err = status, err


class Step:
    """one frame or op against the connection: the event and the bytes owed"""

    def __init__(self, conn, P, iws, defects):
        self.conn, self.P, self.iws, self.defects = conn, P, iws, defects
        self.out = b""
        self.a = self.status = self.flags = 0

    # h2o_http2_stream_open
    def stream_open(self, sid):
        if len(self.conn["streams"]) >= self.P["max_entries"]:
            raise Fail(EFULL)
        s = dict(id=sid, state=IDLE, body=BODY_NONE, tunnel=False, has_body=False, streamed=False, push=False,
                 output_window=self.iws, input_window=HOST_STREAM_WINDOW, bytes_unnotified=0, received=0, content_length=NO_LENGTH)
        self.conn["streams"][sid] = s
        self.conn["priority_open"] += 1
        return s

    # h2o_http2_stream_close: the counters
    def stream_close(self, s):
        if not s["push"]:
            self.conn["priority_open" if s["state"] == IDLE else "pull_open"] -= 1
        del self.conn["streams"][s["id"]]

    # stream_send_error + h2o_http2_stream_reset
    def reset(self, s, err):
        self.out += rst_stream_bytes(s["id"], err)
        self.stream_close(s)
        self.status, self.flags = err, self.flags | RESET_SENT

    def update_stream_input_window(self, s, delta):
        s["bytes_unnotified"] += delta
        window = s["input_window"]
        if "signed_window_compare" not in self.defects:
            window &= (1 << 64) - 1  # size_t >= ssize_t compares unsigned
        if s["bytes_unnotified"] >= window:
            inc = min(s["bytes_unnotified"], INT32_MAX)
            self.out += window_update_bytes(s["id"], inc)
            if s["input_window"] + inc <= INT32_MAX:
                s["input_window"] += inc
            s["bytes_unnotified"] = 0
            self.flags |= WINDOW_UPDATE_SENT

    def handle_request_body_chunk(self, s, n, end_stream):
        first = s["body"] == BODY_BEFORE_FIRST
        s["body"] = BODY_OPEN
        s["received"] += n
        limit = self.P["max_request_entity_size"]
        if s["received"] > limit or ("entity_limit_inclusive" in self.defects and s["received"] == limit):
            return self.reset(s, REFUSED_STREAM)
        if s["content_length"] != NO_LENGTH:
            if end_stream:
                bad = s["received"] != s["content_length"] and "end_length_unchecked" not in self.defects
            else:
                bad = s["received"] > s["content_length"]
            if bad:
                return self.reset(s, PROTOCOL)
        self.a, self.flags = n, self.flags | BODY
        if end_stream:
            s["state"] = max(s["state"], HANDED)
            s["body"] = BODY_CLOSE_DELIVERED
            self.flags |= REQUEST_COMPLETE
        if s["streamed"]:
            return
        if first and not end_stream:
            if self.P["flags"] & STREAM_BODIES:
                s["streamed"] = True
            elif "no_first_frame_extension" not in self.defects:
                self.update_stream_input_window(s, self.P["active_stream_window_size"] - HOST_STREAM_WINDOW)

    def handle_data_frame(self, sid, length, data_len, end_stream):
        s = self.conn["streams"].get(sid)
        if s is None:
            if sid <= self.conn["pull_max_open"] or "data_on_idle_is_closed" in self.defects:
                self.out += rst_stream_bytes(sid, STREAM_CLOSED)
                self.status, self.flags = STREAM_CLOSED, self.flags | RESET_SENT
                return
            raise Fail(PROTOCOL, E_DATA_FRAME)
        if s["body"] not in (BODY_BEFORE_FIRST, BODY_OPEN):
            return self.reset(s, STREAM_CLOSED)
        s["input_window"] -= length
        if length != data_len and "padding_not_credited" not in self.defects:
            self.update_stream_input_window(s, length - data_len)
        if data_len or end_stream:
            self.handle_request_body_chunk(s, data_len, end_stream)

    def handle_headers_frame(self, sid, bflags):
        """up to the block's completion: the stream"""
        c = self.conn
        if sid % 2 == 0:
            raise Fail(PROTOCOL, E_HEADERS_STREAM_ID)
        s = c["streams"].get(sid)
        if sid <= c["pull_max_open"]:
            if s is None:
                raise Fail(PROTOCOL if "closed_headers_is_protocol" in self.defects else STREAM_CLOSED, E_HEADERS_CLOSED)
            if s["body"] not in (BODY_BEFORE_FIRST, BODY_OPEN):
                raise Fail(PROTOCOL, E_HEADERS_STREAM_ID)
            if s["tunnel"] and "tunnel_trailers" not in self.defects:
                raise Fail(PROTOCOL, E_TUNNEL_TRAILERS)
            if not bflags & B_END_STREAM and "trailers_without_end_stream" not in self.defects:
                raise Fail(PROTOCOL, E_TRAILERS_END_STREAM)
            return s
        if bflags & B_SELF_DEPENDENCY:
            raise Fail(PROTOCOL, E_SELF_DEPENDENCY)
        if s is None:
            s = self.stream_open(sid)
        # h2o_http2_stream_prepare_for_request
        c["pull_max_open"] = max(c["pull_max_open"], sid)
        if s["state"] == IDLE:
            c["priority_open"] -= 1
            c["pull_open"] += 1
        s["state"] = RECV_HEADERS
        s["output_window"] = self.iws
        s["has_body"] = not bflags & B_END_STREAM
        return s

    def handle_incoming_request(self, s, b, index):
        ret, exists = b["bstatus"], b["exists_map"]
        if ret not in (0, INVALID_HEADER_CHAR):
            raise Fail(ret, E_HEADER_BLOCK)
        ok, may = True, 0
        if b["method"] == b"CONNECT":
            is_connect, must = True, M_METHOD | M_AUTHORITY
            if "connect_needs_no_authority" in self.defects:
                must = M_METHOD
            if exists & M_PROTOCOL:
                must |= M_SCHEME | M_PATH | M_PROTOCOL
        elif b["method"] == b"CONNECT-UDP":
            ok = not exists & M_PROTOCOL and b["path"] == b"/"
            is_connect, must = True, M_METHOD | M_SCHEME | M_AUTHORITY | M_PATH
        else:
            is_connect, must, may = False, M_METHOD | M_SCHEME | M_PATH, M_AUTHORITY
        if not (ok and exists & must == must and exists & ~(must | may) == 0):
            return self.reset(s, PROTOCOL)
        over = self.conn["pull_open"] > self.P["max_streams"]
        if "max_streams_inclusive" in self.defects:
            over = self.conn["pull_open"] >= self.P["max_streams"]
        if over:
            return self.reset(s, REFUSED_STREAM)
        self.a, self.flags = index, self.flags | OPENED
        s["content_length"] = b["content_length"]
        if ret != 0:
            s["state"] = HANDED
            self.flags |= INVALID_HEADER
            return
        if is_connect:
            if s["content_length"] != NO_LENGTH or not s["has_body"]:
                s["state"] = HANDED
                self.flags |= BAD_CONNECT
                return
            s["tunnel"] = s["streamed"] = True
            s["state"], s["body"] = RECV_BODY, BODY_OPEN
            return self.update_stream_input_window(s, self.P["active_stream_window_size"] - HOST_STREAM_WINDOW)  # process_request
        if not s["has_body"]:
            s["state"] = HANDED
            self.flags |= REQUEST_COMPLETE
        else:
            s["state"], s["body"] = RECV_BODY, BODY_BEFORE_FIRST

    def handle_trailing_headers(self, s, b):
        if b["exists_map"]:
            raise Fail(PROTOCOL, E_TRAILERS_PSEUDO_HEADER)
        if b["host"]:
            raise Fail(PROTOCOL, E_TRAILERS_HOST)
        if b["bstatus"] and not (b["bstatus"] == INVALID_HEADER_CHAR and "soft_trailers_pass" in self.defects):
            raise Fail(b["bstatus"], E_HEADER_BLOCK)
        self.flags |= TRAILERS
        self.handle_request_body_chunk(s, 0, True)
        if not self.flags & RESET_SENT:
            self.flags &= ~BODY

    def handle_priority_frame(self, sid):
        c = self.conn
        if sid in c["streams"]:
            self.flags |= PRIORITY_EV
        elif sid % 2 == 0 or sid <= c["pull_max_open"]:
            self.flags |= IGNORED
        else:
            limit = self.P["max_streams_for_priority"]
            if c["priority_open"] >= limit + ("priority_limit_exclusive" in self.defects):
                raise Fail(ENHANCE_YOUR_CALM, E_TOO_MANY_IDLE)
            self.stream_open(sid)
            self.flags |= PRIORITY_ONLY_OPENED

    def is_idle_stream_id(self, sid):
        if "rst_idle_ignores_parity" in self.defects:
            return self.conn["pull_max_open"] < sid
        return (self.conn["push_max_open"] if sid % 2 == 0 else self.conn["pull_max_open"]) < sid

    def handle_rst_stream_frame(self, sid):
        if self.is_idle_stream_id(sid):
            raise Fail(PROTOCOL, E_RST_STREAM_STREAM_ID)
        s = self.conn["streams"].get(sid)
        if s is None:
            self.flags |= IGNORED
        else:
            self.stream_close(s)
            self.flags |= RESET_BY_PEER

    def update_stream_output_window(self, s, delta):
        cur = s["output_window"]
        if cur + delta > INT32_MAX - ("window_overflow_inclusive" in self.defects):
            return -1, False
        s["output_window"] = cur + delta
        return 0, cur <= 0 < s["output_window"] and "no_window_opened_event" not in self.defects

    def handle_window_update_frame(self, sid, increment, stream_error):
        s = self.conn["streams"].get(sid)
        if stream_error:
            if s is not None:
                self.stream_close(s)
            self.status, self.flags = PROTOCOL, self.flags | RESET_SENT
            return
        if self.is_idle_stream_id(sid):
            raise Fail(PROTOCOL, E_WINDOW_UPDATE_STREAM_ID)
        if s is None:
            self.flags |= IGNORED
            return
        ret, opened = self.update_stream_output_window(s, increment)
        if ret != 0:
            self.stream_close(s)
            self.out += rst_stream_bytes(sid, FLOW_CONTROL)
            self.status, self.flags = FLOW_CONTROL, self.flags | RESET_SENT
        elif opened:
            self.flags |= SEND_WINDOW_OPENED

    def handle_settings_delta(self, delta):
        n = 0
        for s in self.conn["streams"].values():
            ret, opened = self.update_stream_output_window(s, delta)
            if ret != 0 and "delta_overflow_resets" in self.defects:
                s["output_window"] = INT32_MAX
            n += opened
        self.a = n
        if n:
            self.flags |= SEND_WINDOW_OPENED

    def handle_goaway_frame(self):
        if "goaway_keeps_push_ids" not in self.defects:
            self.conn["push_max_open"] = 0x7ffffffe

    def apply_op(self, sid, op, arg):
        """the op's own status"""
        c = self.conn
        if sid == 0 or sid > INT32_MAX:
            return EINVAL
        s = c["streams"].get(sid)
        if op == OP_CLOSE:
            if s is None:
                return ENOENT
            self.stream_close(s)
        elif op == OP_CREDIT:
            if s is None:
                return 0 if "credit_missing_stream_ok" in self.defects else ENOENT
            if arg > INT32_MAX:
                return EINVAL
            self.update_stream_input_window(s, arg)
        elif op == OP_OPEN_PUSH:
            if sid % 2 or s is not None or c["push_max_open"] >= 0x7ffffff0:
                return EINVAL
            if len(c["streams"]) >= self.P["max_entries"]:
                return EFULL
            s = self.stream_open(sid)
            c["priority_open"] -= 1  # h2o_http2_stream_prepare_for_request moves it to num_streams.push
            s.update(state=HANDED, push=True)
            c["push_max_open"] = max(c["push_max_open"], sid)
        else:
            return EINVAL
        return 0


def copy_conn(conn):
    c = dict(conn)
    c["streams"] = {k: dict(v) for k, v in conn["streams"].items()}
    return c


def step_frame(conn, P, iws, i, f, blocks, defects=()):
    """frame i of the connection: (ret, event, own bytes); conn changes as h2o's connection does"""
    st = Step(conn, P, iws, defects)
    typ, sid = f["type"], f["stream_id"]
    a, b, cflags = f["ctl"]
    key = 0
    try:
        if typ == DATA:
            key = sid
            st.handle_data_frame(sid, f["length"], b, bool(f["flags"] & 1))
        elif typ in (HEADERS, CONTINUATION):
            blk = blocks[f["block"]]
            key = blk["stream_id"]
            first = i == blk["first_frame"]
            last = i == blk["first_frame"] + blk["nframes"] - 1
            if first:
                s = st.handle_headers_frame(key, blk["flags"])
            else:
                if sid != key:
                    raise Fail(PROTOCOL, E_CONTINUATION_STREAM_ID)
                s = conn["streams"][key]
            if last:
                if s["state"] == RECV_HEADERS:
                    st.handle_incoming_request(s, blk, f["block"])
                else:
                    st.handle_trailing_headers(s, blk)
        elif typ == PRIORITY:
            key = sid
            st.handle_priority_frame(sid)
        elif typ == RST_STREAM:
            key = sid
            st.handle_rst_stream_frame(sid)
        elif typ == WINDOW_UPDATE and cflags & R_NEEDS_STREAM:
            key = sid
            st.handle_window_update_frame(sid, a, bool(cflags & R_STREAM_ERROR))
        elif typ == SETTINGS and cflags & R_WINDOW_DELTA:
            d = b - (1 << 32) if b & 0x80000000 else b
            st.handle_settings_delta(d)
        elif typ == GOAWAY:
            st.handle_goaway_frame()
    except Fail as e:
        return e.status, (key, 0, e.status, e.err, 0), b""
    return 0, (key, st.a, st.status, E_NONE, st.flags), st.out


def walk(conn, P, iws, frames, blocks, ops=(), rep_cap=None, nctl=None, defects=()):
    """One connection's step: dict(status, err, nstr, events [(stream_id, a, status, err, flags)], op_events, replies).
    conn is changed in place, as h2o changes its connection.  iws: the peer's SETTINGS_INITIAL_WINDOW_SIZE behind the
    step's last frame, as hhuff_h2_control leaves it; each stream is opened with the setting of its own moment."""
    for f in frames[:len(frames) if nctl is None else nctl]:
        if f["type"] == SETTINGS and f["ctl"][2] & R_WINDOW_DELTA:
            iws = (iws - f["ctl"][1]) & 0xffffffff
    n = len(frames) if nctl is None else min(nctl, len(frames))
    cap = 43 * len(frames) + 13 * len(ops) if rep_cap is None else rep_cap
    out = dict(status=0, err=E_NONE, nstr=0, events=[], op_events=[], replies=b"")
    for sid, op, arg in ops:
        trial = copy_conn(conn)
        st = Step(trial, P, iws, defects)
        r = st.apply_op(sid, op, arg)
        if r != 0:
            out["op_events"].append((sid, 0, r, E_NONE, 0))
            continue
        if len(out["replies"]) + len(st.out) > cap:
            out["status"] = SPACE
            return out
        conn.clear()
        conn.update(trial)
        out["replies"] += st.out
        out["op_events"].append((sid, 0, 0, E_NONE, st.flags))
    for i in range(n):
        f = frames[i]
        trial = copy_conn(conn)
        try:
            ret, ev, own = step_frame(trial, P, iws, i, f, blocks, defects)
        except Fail as e:  # EFULL
            out["status"] = e.status
            return out
        if ret == EFULL:
            out["status"] = EFULL
            return out
        need = len(f["ctl_reply"]) + len(own)
        if len(out["replies"]) + need > cap:
            out["status"] = SPACE
            if "space_applies" in defects:
                conn.clear()
                conn.update(trial)
            return out
        conn.clear()
        conn.update(trial)
        if f["type"] == SETTINGS and f["ctl"][2] & R_WINDOW_DELTA:
            iws = (iws + f["ctl"][1]) & 0xffffffff
        out["replies"] += own + f["ctl_reply"] if "own_reply_first" in defects else f["ctl_reply"] + own
        out["events"].append(ev)
        if ret != 0:
            out["status"], out["err"] = ret, ev[3]
            return out
        out["nstr"] += 1
    return out


def snapshot(conn):
    """the state a test compares: the counters and every live stream, by id"""
    keys = ("state", "body", "tunnel", "output_window", "input_window", "bytes_unnotified", "received", "content_length")
    return ((conn["pull_max_open"], conn["push_max_open"], conn["pull_open"], conn["priority_open"]),
            tuple((sid, tuple(int(s[k]) for k in keys)) for sid, s in sorted(conn["streams"].items())))


def fill_sends(conn, records):
    """[(stream_id)] -> [(window, miss)]; marks what it listed in conn["listed"]"""
    listed, out = set(), []
    for sid in records:
        s = conn["streams"].get(sid)
        if s is None:
            out.append((0, 1))
        elif sid in listed:
            out.append((0, 2))
        else:
            listed.add(sid)
            out.append((max(-INT32_MAX, min(INT32_MAX, s["output_window"])), 0))
    conn["listed"] = listed
    return out


def commit_sent(conn, records, sent):
    listed = conn.pop("listed", set())
    for sid, n in zip(records, sent):
        if sid in listed and sid in conn["streams"]:
            conn["streams"][sid]["output_window"] -= n
            listed.discard(sid)


# ---- the calls' arrays of a batch of connections (what hhuff_h2_deframe, hhuff_h2_control and hhuff_hpack_parse_requests
# would leave), for the host program and the GPU tests

FRAME_DTYPE = np.dtype([("payload_off", "<u4"), ("length", "<u4"), ("stream_id", "<u4"), ("type", "u1"), ("flags", "u1"), ("rsv", "<u2"),
                        ("frag_off", "<u4"), ("frag_len", "<u4"), ("block", "<u4"), ("rsv2", "<u4")])
BLOCK_DTYPE = np.dtype([("stream_id", "<u4"), ("end_stream_id", "<u4"), ("flags", "<u4"), ("dependency", "<u4"), ("weight", "<u4"),
                        ("promised_stream_id", "<u4"), ("first_frame", "<u4"), ("nframes", "<u4")])
CTL_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("status", "<i4"), ("err", "<u2"), ("flags", "u1"), ("reply_len", "u1")])
REQ_DTYPE = np.dtype([("content_length", "<u8"), ("method", "<i4"), ("scheme", "<i4"), ("authority", "<i4"), ("path", "<i4"),
                      ("protocol", "<i4"), ("expect", "<i4"), ("exists_map", "<u4"), ("nheaders", "<u4"), ("err", "<u4"),
                      ("scheme_kind", "<u4")])
SEV_DTYPE = np.dtype([("stream_id", "<u4"), ("a", "<u4"), ("status", "<i2"), ("err", "<u2"), ("flags", "<u4")])
OP_DTYPE = np.dtype([("stream_id", "<u4"), ("op", "<u4"), ("arg", "<u4"), ("rsv", "<u4")])


def build(conns, slack=0):
    """conns: [dict(frames, blocks, ops, nctl (None: all), rep_cap (None: the bound))] -> the arrays of one call.  Every
    block gets two field slots: its method and its path."""
    nconn = len(conns)
    nfr = [len(c["frames"]) for c in conns]
    frm_first = np.concatenate([[0], np.cumsum([n + slack for n in nfr])]).astype(np.uint32)
    frm_cap = int(frm_first[-1])
    frames = np.zeros(max(frm_cap, 1), FRAME_DTYPE)
    frames["block"] = 0xFFFFFFFF
    ctl = np.zeros(max(frm_cap, 1), CTL_DTYPE)
    blocks = np.zeros(max(frm_cap, 1), BLOCK_DTYPE)
    bstatus = np.zeros(max(frm_cap, 1), np.int32)
    req = np.zeros(max(frm_cap, 1), REQ_DTYPE)
    blk_off = np.zeros(frm_cap + 1, np.uint32)
    conn_first = np.zeros(nconn + 1, np.uint32)
    ctl_rep_off = np.zeros(nconn + 1, np.uint32)
    rep_off = np.zeros(nconn + 1, np.uint32)
    op_first = np.zeros(nconn + 1, np.uint32)
    ctl_rep, arena, ops = b"", b"", []
    value_off, value_len = [], []
    nb = 0
    for c, cn in enumerate(conns):
        f0 = int(frm_first[c])
        for i, f in enumerate(cn["frames"]):
            r = frames[f0 + i]
            r["length"], r["stream_id"], r["type"], r["flags"] = f["length"], f["stream_id"], f["type"], f["flags"]
            if f["block"] is not None:
                r["block"] = nb + f["block"]
            k = ctl[f0 + i]
            k["a"], k["b"], k["flags"] = f["ctl"]
            k["reply_len"] = len(f["ctl_reply"])
            ctl_rep += f["ctl_reply"]
        for b in cn["blocks"]:
            r = blocks[nb]
            r["stream_id"] = r["end_stream_id"] = b["stream_id"]
            r["flags"], r["first_frame"], r["nframes"] = b["flags"], f0 + b["first_frame"], b["nframes"]
            bstatus[nb] = b["bstatus"]
            q = req[nb]
            q["content_length"], q["exists_map"] = b["content_length"], b["exists_map"]
            for name in ("method", "scheme", "authority", "path", "protocol", "expect"):
                q[name] = -1
            blk_off[nb] = len(value_off)
            for name in ("method", "path"):
                if b[name] is not None:
                    q[name] = len(value_off) - int(blk_off[nb])
                    value_off.append(len(arena))
                    value_len.append(len(b[name]))
                    arena += b[name]
            if b["host"] or b["exists_map"] & M_AUTHORITY:
                q["authority"] = 0
            while len(value_off) - int(blk_off[nb]) < 2:  # (block bytes: at least two, so that two fields fit)
                value_off.append(0)
                value_len.append(0)
            nb += 1
        conn_first[c + 1] = nb
        ctl_rep_off[c + 1] = len(ctl_rep)
        cap = cn.get("rep_cap")
        rep_off[c + 1] = rep_off[c] + (43 * (nfr[c] + slack) + 13 * len(cn.get("ops", ())) if cap is None else cap)
        for sid, op, arg in cn.get("ops", ()):
            ops.append((sid, op, arg, 0))
        op_first[c + 1] = len(ops)
    blk_off[nb:] = len(value_off)
    nframes = np.array(nfr, np.uint32)
    nctl = np.array([n if cn.get("nctl") is None else cn["nctl"] for n, cn in zip(nfr, conns)], np.uint32)
    return dict(nconn=nconn, frm_cap=frm_cap, frames=frames, ctl=ctl, blocks=blocks, bstatus=bstatus, req=req, blk_off=blk_off,
                conn_first=conn_first, frm_first=frm_first, nframes=nframes, nctl=nctl,
                ctl_rep=np.frombuffer(ctl_rep + b"\0", np.uint8).copy(), ctl_rep_size=len(ctl_rep), ctl_rep_off=ctl_rep_off,
                arena=np.frombuffer(arena + b"\0", np.uint8).copy(), arena_size=len(arena),
                value_off=np.array(value_off + [0], np.uint32), value_len=np.array(value_len + [0], np.uint32),
                in_size=len(value_off), ops=np.array(ops, np.uint32).reshape(-1, 4), op_first=op_first,
                rep_off=rep_off, rep_size=int(rep_off[-1]))
