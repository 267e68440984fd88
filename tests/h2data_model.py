"""A model of HTTP/2 DATA framing on the send side (include/hhuff.h (2k'')), written from h2o's lib/http2/stream.c and
include/h2o/http2_internal.h: one plain function per h2o function, frame by frame; separately the closed form of a
record; the call's batch semantics on top of the frame-by-frame functions; and switchable defects, each a mistake a
port could make, so that the tests can show that their cases tell a wrong framer from a right one."""
import numpy as np

from h2o_amd import codec as C

HEADER = 9  # H2O_HTTP2_FRAME_HEADER_SIZE
FINAL, TRAILERS = 1, 2
END_STREAM, DONE, STREAM_WINDOW, ROOM, CONN_WINDOW, MAX_FRAMES = 1, 2, 4, 8, 16, 32
STOPS = (DONE, STREAM_WINDOW, ROOM, CONN_WINDOW, MAX_FRAMES)
EINVAL = -314

DEFECTS = (
    "room_counts_no_header",     # get_buffer_window without its "- H2O_HTTP2_FRAME_HEADER_SIZE"
    "room_needs_two_bytes",      # the room test off by one: a header and one byte of room are not enough
    "stream_window_ignored",     # calc_max_payload_size without the stream's window
    "conn_window_ignored",       # get_buffer_window without the connection's window
    "conn_window_not_consumed",  # commit_data_header leaves conn->_write.window alone
    "end_stream_despite_trailers",
    "end_stream_on_every_frame",  # send_data without its "bufcnt != 0 -> IN_PROGRESS"
    "empty_frame_without_final",  # commit_data_header writing a header for length 0 in progress
    "no_empty_final_frame",      # ... and never writing the one of an empty FINAL body
    "length_in_16_bits",         # the frame header's length without its high byte
    "stream_id_little_endian",
    "max_frame_size_16384",      # the peer's MAX_FRAME_SIZE never taken up
    "conn_window_before_room",   # the stop reasons' order
)


# ---------------------------------------------------------------------------------------------------
# h2o's functions, one each.  conn: m (peer_settings.max_frame_size), window (_write.window), room (capacity - size of
# _write.buf), buf (the bytes queued); stream: data, pos, stream_id, window (output_window), final, trailers.
# ---------------------------------------------------------------------------------------------------
def conn_get_buffer_window(conn, D=()):
    """h2o_http2_conn_get_buffer_window, latency optimisation off: -> (ret, the reason for 0)"""
    ret = conn["room"]
    if ret < HEADER or ("room_needs_two_bytes" in D and ret <= HEADER + 1):
        return 0, ROOM
    if "room_counts_no_header" not in D:
        ret -= HEADER
    if ret <= 0:
        return 0, ROOM
    if "conn_window_ignored" not in D:
        if conn["window"] <= 0:
            return 0, CONN_WINDOW
        ret = min(ret, conn["window"])
    return ret, 0


def calc_max_payload_size(conn, stream, D=()):
    if "conn_window_before_room" in D and conn["window"] <= 0 and conn["room"] <= HEADER:
        return 0, CONN_WINDOW
    conn_max, why = conn_get_buffer_window(conn, D)
    if why:
        return 0, why
    m = 16384 if "max_frame_size_16384" in D else conn["m"]
    if "stream_window_ignored" in D:
        return min(conn_max, m), 0
    if stream["window"] <= 0:
        return 0, STREAM_WINDOW
    return min(conn_max, stream["window"], m), 0


def encode_frame_header(length, typ, flags, stream_id, D=()):
    """h2o_http2_encode_frame_header"""
    ln = (length & 0xFFFF if "length_in_16_bits" in D else length).to_bytes(3, "big")
    sid = stream_id.to_bytes(4, "little" if "stream_id_little_endian" in D else "big")
    return ln + bytes([typ, flags]) + sid


def commit_data_header(conn, stream, payload, final, D=()):
    """commit_data_header without H2O_SEND_STATE_ERROR: -> whether a frame was written"""
    is_end_stream = final and (not stream["trailers"] or "end_stream_despite_trailers" in D)
    length = len(payload)
    write = length != 0 or is_end_stream
    if "empty_frame_without_final" in D:
        write = True
    if "no_empty_final_frame" in D and length == 0:
        write = False
    if not write:
        return False
    conn["buf"] += encode_frame_header(length, 0, END_STREAM if is_end_stream else 0, stream["stream_id"], D) + payload
    conn["frames"].append((length, int(is_end_stream)))
    if "conn_window_not_consumed" not in D:
        conn["window"] -= length
    stream["window"] -= length
    conn["room"] -= length + HEADER
    return True


def send_data(conn, stream, D=()):
    """send_data over the one vector stream["data"][pos:]: -> (the reason nothing could be sent or 0, frame written)"""
    max_payload_size, why = calc_max_payload_size(conn, stream, D)
    if max_payload_size == 0:
        return why or ROOM, False
    left = len(stream["data"]) - stream["pos"]
    fill = min(max_payload_size, left)
    payload = stream["data"][stream["pos"]:stream["pos"] + fill]
    stream["pos"] += fill
    final = stream["final"]
    if stream["pos"] != len(stream["data"]) and "end_stream_on_every_frame" not in D:
        final = False  # bufcnt != 0: send_state = H2O_SEND_STATE_IN_PROGRESS
    wrote = False
    if fill != 0 or stream["final"]:
        wrote = commit_data_header(conn, stream, payload, final, D)
    return 0, wrote


def stream_send_pending_data(conn, stream, D=()):
    """h2o_http2_stream_send_pending_data: -> (the reason it sent nothing or 0, frame written)"""
    if stream["window"] <= 0 and "stream_window_ignored" not in D:
        return STREAM_WINDOW, False
    return send_data(conn, stream, D)


# ---------------------------------------------------------------------------------------------------
# a record, frame by frame, and its closed form
# ---------------------------------------------------------------------------------------------------
def new_conn(m=16384, window=65535, room=0):
    return dict(m=m, window=window, room=room, buf=bytearray(), frames=[])


def visit(conn, data, stream_id, window, flags, max_frames, D=()):
    """one send record against conn, frame by frame: -> (sent, nframes, flags, the stream's window afterwards)"""
    stream = dict(data=data, pos=0, stream_id=stream_id, window=window, final=bool(flags & FINAL), trailers=bool(flags & TRAILERS))
    nframes = calls = 0
    end = 0
    while True:
        before = len(conn["frames"])
        why, wrote = stream_send_pending_data(conn, stream, D)
        calls += 1
        if wrote:
            nframes += 1
            end |= conn["frames"][before][1]
        if why:
            break
        if stream["pos"] == len(data):
            why = DONE
            break
        if max_frames and calls >= max_frames:
            why = MAX_FRAMES
            break
    return stream["pos"], nframes, why | (END_STREAM if end else 0), stream["window"]


def closed_form(m, R, Wc, Ws, L, final, trailers, max_frames=0):
    """the record without a loop over frames: -> (full frames of m bytes, bytes of the one frame behind them, whether
    that frame is the empty END_STREAM one, flags)"""
    def stop(R, Wc, Ws):
        return STREAM_WINDOW if Ws <= 0 else ROOM if R <= HEADER else CONN_WINDOW if Wc <= 0 else 0

    L = max(L, 0)
    es = END_STREAM if final and not trailers else 0
    why = stop(R, Wc, Ws)
    if why:
        return 0, 0, False, why
    if L == 0:
        return 0, 0, bool(es), DONE | es
    cap = min(Wc, Ws)
    by_room = (R - HEADER - m) // (m + HEADER) + 1 if R - HEADER - m >= 0 else 0
    K = min(L // m, cap // m, by_room)
    tail = 0
    if max_frames and K >= max_frames:
        K = max_frames
    else:
        tail = max(0, min(L - K * m, cap - K * m, R - HEADER - K * (m + HEADER)))
    n, k = K * m + tail, K + (tail > 0)
    if n == L:
        return K, tail, False, DONE | es
    if max_frames and k >= max_frames:
        return K, tail, False, MAX_FRAMES
    return K, tail, False, stop(R - n - HEADER * k, Wc - n, Ws - n)


# ---------------------------------------------------------------------------------------------------
# the call
# ---------------------------------------------------------------------------------------------------
def send_rec(body_off, body_len, stream_id, window=65535, flags=0, max_frames=0):
    return (body_off, body_len, stream_id, window, flags, max_frames)


def record_ok(s, body_size):
    return s[0] + s[1] <= body_size and 1 <= s[2] <= 0x7FFFFFFF and not (s[4] & ~(FINAL | TRAILERS))


def connection(body, sends, m, window, room, start=0, D=()):
    """one connection's records in order, frame by frame: -> dict(status, sent [(sent, nframes, out_off, flags, window)],
    buf, window, frames [(length, end_stream)])"""
    conn = new_conn(m, window, room)
    out = dict(status=0, sent=[])
    if not 16384 <= m <= 16777215:
        out["status"] = EINVAL
    else:
        for s in sends:
            if not record_ok(s, len(body)):
                out["status"] = EINVAL
                break
            at = start + len(conn["buf"])
            n, k, fl, w = visit(conn, body[s[0]:s[0] + s[1]], s[2], s[3], s[4], s[5], D)
            out["sent"].append((n, k, at, fl, w))
    out.update(buf=bytes(conn["buf"]), window=conn["window"], frames=conn["frames"])
    return out


def clamp_ranges(first, cap):
    """(2k')'s clamp of a running sum that may be none: -> [(lo, hi)]"""
    r = []
    for a, b in zip(first[:-1], first[1:]):
        lo = min(int(a), cap)
        r.append((lo, max(lo, min(int(b), cap))))
    return r


def peers_array(peers):
    """[(max_frame_size, send_window)] or full H2_PEER_DTYPE tuples -> records (the other fields HHUFF_H2_PEER_INIT's)"""
    p = np.empty(len(peers), C.H2_PEER_DTYPE)
    for i, v in enumerate(peers):
        if len(v) == 2:
            t = list(C.H2_PEER_INIT)
            t[4], t[6] = v
            v = tuple(t)
        p[i] = v
    return p


def batch(body, conns, peers, out_off=None, rooms=None, send_first=None, nsend=None, out_size=None, fill=0xA5, D=()):
    """The call on conns = [[send records]] with peers = [(max_frame_size, send_window)]: the input arrays and every
    output as the call must leave it over buffers filled with `fill`.  rooms: each region's size (default: exactly what
    its frames take without the room's cut, plus 10 -- h2o's room test wants more than a header left -- so that the
    room never cuts); out_off / send_first / nsend / out_size override the arrays built from them
    (hostile ones)."""
    recs = [s for c in conns for s in c]
    if send_first is None:
        send_first = np.cumsum([0] + [len(c) for c in conns])
    nconn = len(send_first) - 1
    assert len(peers) == nconn
    nsend = len(recs) if nsend is None else nsend
    if out_off is None:
        if rooms is None:
            rooms = []
            for c, (m, w) in zip(conns, peers):
                r = connection(body, c, m, w, 1 << 40, 0, D)
                rooms.append(len(r["buf"]) + HEADER + 1)
        out_off = np.cumsum([0] + list(rooms))
    out_size = int(out_off[-1]) if out_size is None else out_size
    sends = np.zeros(max(nsend, len(recs)), C.H2_SEND_DTYPE)
    for i, s in enumerate(recs):
        sends[i] = tuple(int(v) for v in s)
    pin = peers_array(peers)
    e = dict(body=np.frombuffer(bytes(body), np.uint8), sends=sends, send_first=np.asarray(send_first, np.uint32), nsend=nsend,
             out_off=np.asarray(out_off, np.uint32), out_size=out_size, peers_in=pin, peers_out=pin.copy(),
             out=np.full(out_size, fill, np.uint8), out_used=np.zeros(out_size, bool),
             sent=np.zeros(nsend, C.H2_SENT_DTYPE), sent_used=np.zeros(nsend, bool),
             out_len=np.zeros(nconn, np.uint32), cstatus=np.zeros(nconn, np.int32), frames=[])
    for c, ((s0, s1), (o0, o1)) in enumerate(zip(clamp_ranges(send_first, nsend), clamp_ranges(out_off, out_size))):
        m, w = int(pin["max_frame_size"][c]), int(pin["send_window"][c])
        r = connection(body, [tuple(int(v) for v in sends[i]) for i in range(s0, s1)], m, w, o1 - o0, o0, D)
        n = len(r["buf"])
        e["out"][o0:o0 + n] = np.frombuffer(r["buf"], np.uint8)
        e["out_used"][o0:o0 + n] = True
        for i, t in enumerate(r["sent"]):
            e["sent"][s0 + i] = t + (0,)
            e["sent_used"][s0 + i] = True
        e["out_len"][c], e["cstatus"][c] = n, r["status"]
        e["peers_out"]["send_window"][c] = r["window"]
        e["frames"].append(r["frames"])
    return e


def split_frames(buf):
    """the frames of a byte string: [(length, type, flags, stream_id, payload)]"""
    out, pos = [], 0
    while pos < len(buf):
        n = int.from_bytes(buf[pos:pos + 3], "big")
        out.append((n, buf[pos + 3], buf[pos + 4], int.from_bytes(buf[pos + 5:pos + 9], "big"), bytes(buf[pos + 9:pos + 9 + n])))
        pos += 9 + n
    assert pos == len(buf)
    return out
