"""Hand-built connections for the HTTP/2 stream table (include/hhuff.h (2k''')) with literal expectations, on both sides of
every rule's edge.  A case is one connection:
    P, iws     the server's parameters (h2streams_model.params) and the peer's SETTINGS_INITIAL_WINDOW_SIZE behind each step
    steps      [S]: the calls made for it, in order; S.frames / S.blocks / S.ops / S.rep_cap / S.nctl as h2streams_model takes them,
               S.sends what the send side booked in front of the step
    status, err, nstr, events, op_events, replies     of the LAST step: events [(flags, status, a)] per frame written
    counters   (pull max_open, push max_open, pull.open, priority.open) behind the last step
    streams    {id: (state, body state, output_window, input_window, bytes_unnotified)} behind the last step
The expectations are worked out from lib/http2/connection.c by hand, not taken from the model or the code under test."""
import h2streams_model as M
from h2streams_model import (B_END_STREAM, B_SELF_DEPENDENCY, BAD_CONNECT, BODY, BODY_BEFORE_FIRST, BODY_CLOSE_DELIVERED, BODY_NONE,
                             BODY_OPEN, CONTINUATION, DATA, E_CONTINUATION_STREAM_ID, E_DATA_FRAME, E_HEADER_BLOCK, E_HEADERS_CLOSED,
                             E_HEADERS_STREAM_ID, E_NONE, E_RST_STREAM_STREAM_ID, E_SELF_DEPENDENCY, E_TOO_MANY_IDLE,
                             E_TRAILERS_END_STREAM, E_TRAILERS_HOST, E_TRAILERS_PSEUDO_HEADER, E_TUNNEL_TRAILERS,
                             E_WINDOW_UPDATE_STREAM_ID, EFULL, EINVAL, ENOENT, GOAWAY, HANDED, HEADERS, IDLE, IGNORED, INT32_MAX,
                             INVALID_HEADER, NO_LENGTH, OP_CLOSE, OP_CREDIT, OP_OPEN_PUSH, OPENED, PING, PRIORITY, PRIORITY_EV,
                             PRIORITY_ONLY_OPENED, R_NEEDS_STREAM, R_STREAM_ERROR, R_WINDOW_DELTA, RECV_BODY, REQUEST_COMPLETE,
                             RESET_BY_PEER, RESET_SENT, RST_STREAM, SEND_WINDOW_OPENED, SETTINGS, SPACE, STREAM_BODIES, TRAILERS,
                             WINDOW_UPDATE, WINDOW_UPDATE_SENT, frame_bytes, params, rst_stream_bytes, window_update_bytes)

GET = 1 | 2 | 4            # :method, :scheme, :path
RC = REQUEST_COMPLETE
WUS = WINDOW_UPDATE_SENT
RST = rst_stream_bytes
WU = window_update_bytes
ACK = frame_bytes(SETTINGS, 1, 0, b"")


class S:
    """one step of one connection"""

    def __init__(self, rep_cap=None, nctl=None, sends=()):
        """sends: [(stream_id, bytes sent)] that hhuff_h2_streams_fill_sends and _commit_sent book in front of the step"""
        self.frames, self.blocks, self.ops, self.rep_cap, self.nctl, self.sends = [], [], [], rep_cap, nctl, list(sends)

    def _frame(self, typ, flags, sid, length, ctl=(0, 0, 0), ctl_reply=b"", block=None):
        self.frames.append(dict(type=typ, flags=flags, stream_id=sid, length=length, ctl=ctl, ctl_reply=ctl_reply, block=block))
        return self

    def headers(self, sid, end_stream=False, method=b"GET", exists=GET, cl=NO_LENGTH, path=b"/", bstatus=0, host=False,
                self_dep=False, cont=0, cont_sid=None):
        flags = (B_END_STREAM if end_stream else 0) | (B_SELF_DEPENDENCY if self_dep else 0)
        self.blocks.append(dict(stream_id=sid, flags=flags, first_frame=len(self.frames), nframes=1 + cont, bstatus=bstatus,
                                exists_map=exists, content_length=cl, method=method, path=path, host=host))
        b = len(self.blocks) - 1
        self._frame(HEADERS, (1 if end_stream else 0) | (0 if cont else 4), sid, 10, block=b)
        for k in range(cont):
            self._frame(CONTINUATION, 4 if k == cont - 1 else 0, sid if cont_sid is None else cont_sid, 3, block=b)
        return self

    def trailers(self, sid, end_stream=True, exists=0, **kw):
        return self.headers(sid, end_stream=end_stream, method=None, path=None, exists=exists, **kw)

    def data(self, sid, n, pad=0, end_stream=False, ctl_reply=b""):
        """pad: the padding's bytes, the pad-length byte included"""
        return self._frame(DATA, (1 if end_stream else 0) | (8 if pad else 0), sid, n + pad, (100, n, R_NEEDS_STREAM), ctl_reply)

    def priority(self, sid):
        return self._frame(PRIORITY, 0, sid, 5, (0, 16, R_NEEDS_STREAM))

    def rst(self, sid):
        return self._frame(RST_STREAM, 0, sid, 4, (8, 0, R_NEEDS_STREAM))

    def wu(self, sid, inc):
        if inc == 0:  # the control call's stream-level error: its RST_STREAM is among the control replies
            return self._frame(WINDOW_UPDATE, 0, sid, 4, (0, 0, R_NEEDS_STREAM | R_STREAM_ERROR), RST(sid, -1))
        return self._frame(WINDOW_UPDATE, 0, sid, 4, (inc, 0, R_NEEDS_STREAM))

    def settings(self, delta):
        return self._frame(SETTINGS, 0, 0, 6, (1, delta & 0xffffffff, R_WINDOW_DELTA if delta else 0), ACK)

    def goaway(self):
        return self._frame(GOAWAY, 0, 0, 8, (0, 0, 0))

    def ping(self):
        return self._frame(PING, 0, 0, 8, (1, 2, 0), frame_bytes(PING, 1, 0, b"\0\0\0\1\0\0\0\2"))

    def op(self, sid, op, arg=0):
        self.ops.append((sid, op, arg))
        return self


CASES = []


def case(name, steps, status=0, err=E_NONE, nstr=None, events=(), op_events=(), replies=b"", counters=None, streams=None, P=None,
         iws=65535):
    steps = steps if isinstance(steps, list) else [steps]
    if P is None:
        P = params(max_streams=4, max_streams_for_priority=2, max_request_entity_size=1 << 20)
    if not isinstance(iws, list):
        iws = [iws] * len(steps)
    CASES.append(dict(name=name, P=P, iws=iws, steps=steps, status=status, err=err,
                      nstr=len(steps[-1].frames) if nstr is None else nstr, events=list(events), op_events=list(op_events),
                      replies=replies, counters=counters, streams=streams or {}))


W0 = 65535

# ---- HEADERS: ids around max_open, parity, self-dependency
case("get_end_stream", S().headers(1, True), events=[(OPENED | RC, 0, 0)], counters=(1, 0, 1, 0),
     streams={1: (HANDED, BODY_NONE, W0, W0, 0)})
case("headers_at_max_open_on_a_finished_stream", S().headers(3, True).headers(3, True), status=-1, err=E_HEADERS_STREAM_ID, nstr=1,
     events=[(OPENED | RC, 0, 0), (0, -1, 0)], counters=(3, 0, 1, 0), streams={3: (HANDED, BODY_NONE, W0, W0, 0)})
case("headers_below_max_open_closed", S().headers(3, True).headers(1, True), status=-5, err=E_HEADERS_CLOSED, nstr=1,
     events=[(OPENED | RC, 0, 0), (0, -5, 0)], counters=(3, 0, 1, 0), streams={3: (HANDED, BODY_NONE, W0, W0, 0)})
case("headers_at_max_open_plus_2", S().headers(3, True).headers(5, True), events=[(OPENED | RC, 0, 0), (OPENED | RC, 0, 1)],
     counters=(5, 0, 2, 0), streams={3: (HANDED, BODY_NONE, W0, W0, 0), 5: (HANDED, BODY_NONE, W0, W0, 0)})
case("headers_even_id", S().headers(2, True), status=-1, err=E_HEADERS_STREAM_ID, nstr=0, events=[(0, -1, 0)], counters=(0, 0, 0, 0))
case("headers_self_dependency", S().headers(1, True, self_dep=True), status=-1, err=E_SELF_DEPENDENCY, nstr=0, events=[(0, -1, 0)],
     counters=(0, 0, 0, 0))
case("continuation_of_the_block", S().headers(1, True, cont=2), events=[(0, 0, 0), (0, 0, 0), (OPENED | RC, 0, 0)],
     counters=(1, 0, 1, 0), streams={1: (HANDED, BODY_NONE, W0, W0, 0)})
case("continuation_names_another_stream", S().headers(1, True, cont=1, cont_sid=3), status=-1, err=E_CONTINUATION_STREAM_ID, nstr=1,
     events=[(0, 0, 0), (0, -1, 0)], counters=(1, 0, 1, 0), streams={1: (1, BODY_NONE, W0, W0, 0)})

# ---- the head: pseudo-header maps, max_streams, the 400s
case("get_without_path", S().headers(1, True, exists=1 | 2), events=[(RESET_SENT, -1, 0)], replies=RST(1, -1), counters=(1, 0, 0, 0))
case("get_with_authority", S().headers(1, True, exists=GET | 8), events=[(OPENED | RC, 0, 0)], counters=(1, 0, 1, 0),
     streams={1: (HANDED, BODY_NONE, W0, W0, 0)})
case("get_with_protocol", S().headers(1, True, exists=GET | 16), events=[(RESET_SENT, -1, 0)], replies=RST(1, -1),
     counters=(1, 0, 0, 0))
case("no_method_at_all", S().headers(1, True, method=None, exists=2 | 4), events=[(RESET_SENT, -1, 0)], replies=RST(1, -1),
     counters=(1, 0, 0, 0))
case("connect", S().headers(1, method=b"CONNECT", exists=1 | 8, path=None), events=[(OPENED, 0, 0)], counters=(1, 0, 1, 0),
     streams={1: (RECV_BODY, BODY_OPEN, W0, W0, 0)})
case("connect_without_authority", S().headers(1, method=b"CONNECT", exists=1, path=None), events=[(RESET_SENT, -1, 0)],
     replies=RST(1, -1), counters=(1, 0, 0, 0))
case("connect_with_path", S().headers(1, method=b"CONNECT", exists=1 | 8 | 4), events=[(RESET_SENT, -1, 0)], replies=RST(1, -1),
     counters=(1, 0, 0, 0))
case("extended_connect", S().headers(1, method=b"CONNECT", exists=31), events=[(OPENED, 0, 0)], counters=(1, 0, 1, 0),
     streams={1: (RECV_BODY, BODY_OPEN, W0, W0, 0)})
case("extended_connect_without_scheme", S().headers(1, method=b"CONNECT", exists=31 - 2), events=[(RESET_SENT, -1, 0)],
     replies=RST(1, -1), counters=(1, 0, 0, 0))
case("connect_udp", S().headers(1, method=b"CONNECT-UDP", exists=15), events=[(OPENED, 0, 0)], counters=(1, 0, 1, 0),
     streams={1: (RECV_BODY, BODY_OPEN, W0, W0, 0)})
case("connect_udp_other_path", S().headers(1, method=b"CONNECT-UDP", exists=15, path=b"/x"), events=[(RESET_SENT, -1, 0)],
     replies=RST(1, -1), counters=(1, 0, 0, 0))
case("connect_udp_with_protocol", S().headers(1, method=b"CONNECT-UDP", exists=31), events=[(RESET_SENT, -1, 0)], replies=RST(1, -1),
     counters=(1, 0, 0, 0))
case("connect_with_end_stream", S().headers(1, True, method=b"CONNECT", exists=9, path=None), events=[(OPENED | BAD_CONNECT, 0, 0)],
     counters=(1, 0, 1, 0), streams={1: (HANDED, BODY_NONE, W0, W0, 0)})
case("connect_with_content_length", S().headers(1, method=b"CONNECT", exists=9, path=None, cl=0), events=[(OPENED | BAD_CONNECT, 0, 0)],
     counters=(1, 0, 1, 0), streams={1: (HANDED, BODY_NONE, W0, W0, 0)})
case("connect_extends_the_window_at_once", S().headers(1, method=b"CONNECT", exists=9, path=None), events=[(OPENED | WUS, 0, 0)],
     replies=WU(1, W0), counters=(1, 0, 1, 0), streams={1: (RECV_BODY, BODY_OPEN, W0, 2 * W0, 0)},
     P=params(max_streams=4, active_stream_window_size=2 * W0))
case("soft_error_head", S().headers(1, bstatus=-254), events=[(OPENED | INVALID_HEADER, 0, 0)], counters=(1, 0, 1, 0),
     streams={1: (HANDED, BODY_NONE, W0, W0, 0)})
case("soft_error_head_without_path", S().headers(1, bstatus=-254, exists=3), events=[(RESET_SENT, -1, 0)], replies=RST(1, -1),
     counters=(1, 0, 0, 0))
case("compression_error_head", S().ping().headers(1, bstatus=-9), status=-9, err=E_HEADER_BLOCK, nstr=1,
     events=[(0, 0, 0), (0, -9, 0)], replies=S().ping().frames[0]["ctl_reply"], counters=(1, 0, 1, 0),
     streams={1: (1, BODY_NONE, W0, W0, 0)})
P2 = params(max_streams=2, max_streams_for_priority=2)
case("pull_open_at_max_streams", S().headers(1).headers(3), events=[(OPENED, 0, 0), (OPENED, 0, 1)], counters=(3, 0, 2, 0), P=P2,
     streams={1: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0), 3: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0)})
case("pull_open_above_max_streams", S().headers(1).headers(3).headers(5).headers(7, True),
     events=[(OPENED, 0, 0), (OPENED, 0, 1), (RESET_SENT, -7, 0), (RESET_SENT, -7, 0)], replies=RST(5, -7) + RST(7, -7),
     counters=(7, 0, 2, 0), P=P2,
     streams={1: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0), 3: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0)})
case("table_full", S().headers(1).headers(3), status=EFULL, nstr=1, events=[(OPENED, 0, 0)], counters=(1, 0, 1, 0),
     P=params(max_streams=4, max_entries=1), streams={1: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0)})

# ---- trailers
case("trailers", S().headers(1).data(1, 5).trailers(1), events=[(OPENED, 0, 0), (BODY, 0, 5), (TRAILERS | RC, 0, 0)],
     counters=(1, 0, 1, 0), streams={1: (HANDED, BODY_CLOSE_DELIVERED, W0, W0 - 5, 0)})
case("trailers_without_data", S().headers(1).trailers(1), events=[(OPENED, 0, 0), (TRAILERS | RC, 0, 0)], counters=(1, 0, 1, 0),
     streams={1: (HANDED, BODY_CLOSE_DELIVERED, W0, W0, 0)})
case("trailers_without_end_stream", S().headers(1).trailers(1, end_stream=False), status=-1, err=E_TRAILERS_END_STREAM, nstr=1,
     events=[(OPENED, 0, 0), (0, -1, 0)], counters=(1, 0, 1, 0), streams={1: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0)})
case("trailers_with_a_pseudo_header", S().headers(1).trailers(1, exists=1), status=-1, err=E_TRAILERS_PSEUDO_HEADER, nstr=1,
     events=[(OPENED, 0, 0), (0, -1, 0)], counters=(1, 0, 1, 0), streams={1: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0)})
case("trailers_with_a_pseudo_header_and_a_later_error", S().headers(1).trailers(1, exists=1, bstatus=-9), status=-1,
     err=E_TRAILERS_PSEUDO_HEADER, nstr=1, events=[(OPENED, 0, 0), (0, -1, 0)], counters=(1, 0, 1, 0),
     streams={1: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0)})
case("trailers_with_host", S().headers(1).trailers(1, host=True), status=-1, err=E_TRAILERS_HOST, nstr=1,
     events=[(OPENED, 0, 0), (0, -1, 0)], counters=(1, 0, 1, 0), streams={1: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0)})
case("trailers_with_a_soft_error", S().headers(1).trailers(1, bstatus=-254), status=-254, err=E_HEADER_BLOCK, nstr=1,
     events=[(OPENED, 0, 0), (0, -254, 0)], counters=(1, 0, 1, 0), streams={1: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0)})
case("trailers_on_a_tunnel", S().headers(1, method=b"CONNECT", exists=9, path=None).trailers(1), status=-1, err=E_TUNNEL_TRAILERS,
     nstr=1, events=[(OPENED, 0, 0), (0, -1, 0)], counters=(1, 0, 1, 0), streams={1: (RECV_BODY, BODY_OPEN, W0, W0, 0)})
case("trailers_ignore_self_dependency", S().headers(1).trailers(1, self_dep=True), events=[(OPENED, 0, 0), (TRAILERS | RC, 0, 0)],
     counters=(1, 0, 1, 0), streams={1: (HANDED, BODY_CLOSE_DELIVERED, W0, W0, 0)})
case("trailers_short_of_content_length", S().headers(1, cl=6).data(1, 5).trailers(1),
     events=[(OPENED, 0, 0), (BODY, 0, 5), (TRAILERS | RESET_SENT, -1, 0)], replies=RST(1, -1), counters=(1, 0, 0, 0))

# ---- DATA
case("post", S().headers(1).data(1, 10).data(1, 5, end_stream=True), events=[(OPENED, 0, 0), (BODY, 0, 10), (BODY | RC, 0, 5)],
     counters=(1, 0, 1, 0), streams={1: (HANDED, BODY_CLOSE_DELIVERED, W0, W0 - 15, 0)})
case("empty_data_without_end_stream", S().headers(1).data(1, 0), events=[(OPENED, 0, 0), (0, 0, 0)], counters=(1, 0, 1, 0),
     streams={1: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0)})
case("empty_data_with_end_stream", S().headers(1).data(1, 0, end_stream=True), events=[(OPENED, 0, 0), (BODY | RC, 0, 0)],
     counters=(1, 0, 1, 0), streams={1: (HANDED, BODY_CLOSE_DELIVERED, W0, W0, 0)})
case("data_on_an_idle_id", S().headers(1).data(3, 5, ctl_reply=WU(0, 40000)), status=-1, err=E_DATA_FRAME, nstr=1,
     events=[(OPENED, 0, 0), (0, -1, 0)], replies=WU(0, 40000), counters=(1, 0, 1, 0),
     streams={1: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0)})
case("data_on_an_idle_id_without_a_control_reply", S().headers(1).data(3, 5), status=-1, err=E_DATA_FRAME, nstr=1,
     events=[(OPENED, 0, 0), (0, -1, 0)], counters=(1, 0, 1, 0), streams={1: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0)})
case("data_on_a_closed_id", S().headers(3, True).data(1, 5).data(2, 5).ping(),
     events=[(OPENED | RC, 0, 0), (RESET_SENT, -5, 0), (RESET_SENT, -5, 0), (0, 0, 0)],
     replies=RST(1, -5) + RST(2, -5) + S().ping().frames[0]["ctl_reply"], counters=(3, 0, 1, 0),
     streams={3: (HANDED, BODY_NONE, W0, W0, 0)})
case("control_reply_goes_in_front_of_the_frames_own", S().headers(3, True).data(1, 5, ctl_reply=WU(0, 40000)),
     events=[(OPENED | RC, 0, 0), (RESET_SENT, -5, 0)], replies=WU(0, 40000) + RST(1, -5), counters=(3, 0, 1, 0),
     streams={3: (HANDED, BODY_NONE, W0, W0, 0)})
case("data_behind_end_stream", S().headers(1).data(1, 5, end_stream=True).data(1, 5),
     events=[(OPENED, 0, 0), (BODY | RC, 0, 5), (RESET_SENT, -5, 0)], replies=RST(1, -5), counters=(1, 0, 0, 0))
case("body_at_content_length", S().headers(1, cl=10).data(1, 4).data(1, 6, end_stream=True),
     events=[(OPENED, 0, 0), (BODY, 0, 4), (BODY | RC, 0, 6)], counters=(1, 0, 1, 0),
     streams={1: (HANDED, BODY_CLOSE_DELIVERED, W0, W0 - 10, 0)})
case("body_one_over_content_length", S().headers(1, cl=10).data(1, 4).data(1, 7),
     events=[(OPENED, 0, 0), (BODY, 0, 4), (RESET_SENT, -1, 0)], replies=RST(1, -1), counters=(1, 0, 0, 0))
case("body_one_short_at_end_stream", S().headers(1, cl=10).data(1, 9, end_stream=True), events=[(OPENED, 0, 0), (RESET_SENT, -1, 0)],
     replies=RST(1, -1), counters=(1, 0, 0, 0))
PE = params(max_streams=4, max_request_entity_size=100)
case("entity_at_the_limit", S().headers(1).data(1, 100), events=[(OPENED, 0, 0), (BODY, 0, 100)], counters=(1, 0, 1, 0), P=PE,
     streams={1: (RECV_BODY, BODY_OPEN, W0, W0 - 100, 0)})
case("entity_one_over_the_limit", S().headers(1).data(1, 60).data(1, 41), events=[(OPENED, 0, 0), (BODY, 0, 60), (RESET_SENT, -7, 0)],
     replies=RST(1, -7), counters=(1, 0, 0, 0), P=PE)
BIG = S().headers(1).data(1, 16384).data(1, 16384).data(1, 16384).data(1, 16200)   # the window is down to 183
case("padding_alone_owes_the_window_update", [BIG, S().data(1, 0, pad=100)], events=[(WUS, 0, 0)], replies=WU(1, 100),
     counters=(1, 0, 1, 0), streams={1: (RECV_BODY, BODY_OPEN, W0, 183, 0)})
case("padding_one_short_of_the_window", [BIG, S().data(1, 0, pad=91)], events=[(0, 0, 0)], counters=(1, 0, 1, 0),
     streams={1: (RECV_BODY, BODY_OPEN, W0, 92, 91)})
case("padding_accumulates", [BIG, S().data(1, 0, pad=60).data(1, 0, pad=50)], events=[(0, 0, 0), (WUS, 0, 0)], replies=WU(1, 110),
     counters=(1, 0, 1, 0), streams={1: (RECV_BODY, BODY_OPEN, W0, 183, 0)})
case("an_overdrawn_window_owes_nothing", [BIG, S().data(1, 184).data(1, 0, pad=100)], events=[(BODY, 0, 184), (0, 0, 0)],
     counters=(1, 0, 1, 0), streams={1: (RECV_BODY, BODY_OPEN, W0, -101, 100)})
case("first_frame_with_the_default_active_window", S().headers(1).data(1, 10), events=[(OPENED, 0, 0), (BODY, 0, 10)],
     counters=(1, 0, 1, 0), streams={1: (RECV_BODY, BODY_OPEN, W0, W0 - 10, 0)})
case("first_frame_extension_below_the_window", S().headers(1).data(1, 10).data(1, 10),
     events=[(OPENED, 0, 0), (BODY, 0, 10), (BODY, 0, 10)], counters=(1, 0, 1, 0),
     P=params(max_streams=4, active_stream_window_size=W0 + 1000), streams={1: (RECV_BODY, BODY_OPEN, W0, W0 - 20, 1000)})
case("first_frame_extension_owes_the_window_update", S().headers(1).data(1, 10).data(1, 10),
     events=[(OPENED, 0, 0), (BODY | WUS, 0, 10), (BODY, 0, 10)], replies=WU(1, 16 * 1048576 - W0), counters=(1, 0, 1, 0),
     P=params(max_streams=4, active_stream_window_size=16 * 1048576), streams={1: (RECV_BODY, BODY_OPEN, W0, 16 * 1048576 - 20, 0)})
case("first_frame_with_end_stream_extends_nothing", S().headers(1).data(1, 10, end_stream=True), events=[(OPENED, 0, 0), (BODY | RC, 0, 10)],
     counters=(1, 0, 1, 0), P=params(max_streams=4, active_stream_window_size=16 * 1048576),
     streams={1: (HANDED, BODY_CLOSE_DELIVERED, W0, W0 - 10, 0)})
case("streamed_bodies_extend_nothing", S().headers(1).data(1, 10), events=[(OPENED, 0, 0), (BODY, 0, 10)], counters=(1, 0, 1, 0),
     P=params(max_streams=4, active_stream_window_size=16 * 1048576, flags=STREAM_BODIES),
     streams={1: (RECV_BODY, BODY_OPEN, W0, W0 - 10, 0)})
BIG_CL = S().headers(1, cl=65352).data(1, 16384).data(1, 16384).data(1, 16384).data(1, 16200)   # the same, the body complete
case("padding_owes_the_window_update_and_the_data_the_reset", [BIG_CL, S().data(1, 1, pad=100)],
     events=[(WUS | RESET_SENT, -1, 0)], replies=WU(1, 100) + RST(1, -1), counters=(1, 0, 0, 0))

# ---- PRIORITY
case("priority_at_the_limit", S().priority(1).priority(3), events=[(PRIORITY_ONLY_OPENED, 0, 0), (PRIORITY_ONLY_OPENED, 0, 0)],
     counters=(0, 0, 0, 2), streams={1: (IDLE, BODY_NONE, W0, W0, 0), 3: (IDLE, BODY_NONE, W0, W0, 0)})
case("priority_above_the_limit", S().priority(1).priority(3).priority(5), status=-11, err=E_TOO_MANY_IDLE, nstr=2,
     events=[(PRIORITY_ONLY_OPENED, 0, 0), (PRIORITY_ONLY_OPENED, 0, 0), (0, -11, 0)], counters=(0, 0, 0, 2),
     streams={1: (IDLE, BODY_NONE, W0, W0, 0), 3: (IDLE, BODY_NONE, W0, W0, 0)})
case("priority_on_live_closed_and_even_ids", S().headers(3).priority(3).priority(1).priority(2),
     events=[(OPENED, 0, 0), (PRIORITY_EV, 0, 0), (IGNORED, 0, 0), (IGNORED, 0, 0)], counters=(3, 0, 1, 0),
     streams={3: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0)})
case("priority_only_stream_gets_headers", S().priority(5).headers(5, True), events=[(PRIORITY_ONLY_OPENED, 0, 0), (OPENED | RC, 0, 0)],
     counters=(5, 0, 1, 0), streams={5: (HANDED, BODY_NONE, W0, W0, 0)})
case("priority_only_stream_gets_data", S().priority(5).data(5, 3), events=[(PRIORITY_ONLY_OPENED, 0, 0), (RESET_SENT, -5, 0)],
     replies=RST(5, -5), counters=(0, 0, 0, 0))
case("priority_only_stream_gets_rst_stream", S().priority(5).rst(5), status=-1, err=E_RST_STREAM_STREAM_ID, nstr=1,
     events=[(PRIORITY_ONLY_OPENED, 0, 0), (0, -1, 0)], counters=(0, 0, 0, 1), streams={5: (IDLE, BODY_NONE, W0, W0, 0)})
case("priority_only_stream_below_a_later_request", S().priority(3).headers(5, True).rst(3),
     events=[(PRIORITY_ONLY_OPENED, 0, 0), (OPENED | RC, 0, 0), (RESET_BY_PEER, 0, 0)], counters=(5, 0, 1, 0),
     streams={5: (HANDED, BODY_NONE, W0, W0, 0)})

# ---- RST_STREAM, and even ids before and after OPEN_PUSH and GOAWAY
case("rst_stream_on_live_and_closed", S().headers(1).headers(3, True).rst(1).rst(1),
     events=[(OPENED, 0, 0), (OPENED | RC, 0, 1), (RESET_BY_PEER, 0, 0), (IGNORED, 0, 0)], counters=(3, 0, 1, 0),
     streams={3: (HANDED, BODY_NONE, W0, W0, 0)})
case("rst_stream_on_an_idle_id", S().headers(1).rst(3), status=-1, err=E_RST_STREAM_STREAM_ID, nstr=1, events=[(OPENED, 0, 0), (0, -1, 0)],
     counters=(1, 0, 1, 0), streams={1: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0)})
case("even_id_before_a_push", S().headers(5, True).rst(2), status=-1, err=E_RST_STREAM_STREAM_ID, nstr=1,
     events=[(OPENED | RC, 0, 0), (0, -1, 0)], counters=(5, 0, 1, 0), streams={5: (HANDED, BODY_NONE, W0, W0, 0)})
case("even_ids_after_a_push", [S().headers(5, True), S().op(4, OP_OPEN_PUSH).rst(2).wu(4, 10).rst(4).rst(6)], status=-1,
     err=E_RST_STREAM_STREAM_ID, nstr=3, op_events=[(0, 0, 0)],
     events=[(IGNORED, 0, 0), (0, 0, 0), (RESET_BY_PEER, 0, 0), (0, -1, 0)], counters=(5, 4, 1, 0),
     streams={5: (HANDED, BODY_NONE, W0, W0, 0)})
case("even_ids_after_goaway", S().goaway().rst(6).wu(8, 1), events=[(0, 0, 0), (IGNORED, 0, 0), (IGNORED, 0, 0)],
     counters=(0, 0x7ffffffe, 0, 0))
case("no_push_after_goaway", [S().goaway(), S().op(2, OP_OPEN_PUSH)], op_events=[(0, EINVAL, 0)], counters=(0, 0x7ffffffe, 0, 0))

# ---- WINDOW_UPDATE on a stream
HI = INT32_MAX - 100
case("window_update_to_int32_max", S().headers(1).wu(1, 100), events=[(OPENED, 0, 0), (0, 0, 0)], counters=(1, 0, 1, 0), iws=HI,
     streams={1: (RECV_BODY, BODY_BEFORE_FIRST, INT32_MAX, W0, 0)})
case("window_update_one_above_int32_max", S().headers(1).wu(1, 101), events=[(OPENED, 0, 0), (RESET_SENT, -3, 0)], replies=RST(1, -3),
     counters=(1, 0, 0, 0), iws=HI)
case("window_update_opens_the_send_window", S().headers(1).wu(1, 1).wu(1, 1), events=[(OPENED, 0, 0), (SEND_WINDOW_OPENED, 0, 0), (0, 0, 0)],
     counters=(1, 0, 1, 0), iws=0, streams={1: (RECV_BODY, BODY_BEFORE_FIRST, 2, W0, 0)})
case("window_update_on_idle_and_closed_ids", S().headers(3, True).wu(1, 5).wu(5, 5), status=-1, err=E_WINDOW_UPDATE_STREAM_ID, nstr=2,
     events=[(OPENED | RC, 0, 0), (IGNORED, 0, 0), (0, -1, 0)], counters=(3, 0, 1, 0), streams={3: (HANDED, BODY_NONE, W0, W0, 0)})
case("zero_increment_on_a_live_stream", S().headers(1).wu(1, 0).ping(), events=[(OPENED, 0, 0), (RESET_SENT, -1, 0), (0, 0, 0)],
     replies=RST(1, -1) + S().ping().frames[0]["ctl_reply"], counters=(1, 0, 0, 0))
case("zero_increment_on_a_closed_and_an_idle_stream", S().headers(3, True).wu(1, 0).wu(9, 0),
     events=[(OPENED | RC, 0, 0), (RESET_SENT, -1, 0), (RESET_SENT, -1, 0)], replies=RST(1, -1) + RST(9, -1), counters=(3, 0, 1, 0),
     streams={3: (HANDED, BODY_NONE, W0, W0, 0)})

# ---- SETTINGS with a window delta
case("settings_delta_to_int32_max", S().headers(1).wu(1, 90).headers(3).settings(10),
     events=[(OPENED, 0, 0), (0, 0, 0), (OPENED, 0, 1), (0, 0, 0)], replies=ACK, counters=(3, 0, 2, 0), iws=HI + 10,
     streams={1: (RECV_BODY, BODY_BEFORE_FIRST, INT32_MAX, W0, 0), 3: (RECV_BODY, BODY_BEFORE_FIRST, HI + 10, W0, 0)})
case("settings_delta_one_above_keeps_the_window", S().headers(1).wu(1, 90).headers(3).settings(11),
     events=[(OPENED, 0, 0), (0, 0, 0), (OPENED, 0, 1), (0, 0, 0)], replies=ACK, counters=(3, 0, 2, 0), iws=HI + 11,
     streams={1: (RECV_BODY, BODY_BEFORE_FIRST, HI + 90, W0, 0), 3: (RECV_BODY, BODY_BEFORE_FIRST, HI + 11, W0, 0)})
case("a_shrinking_settings_leaves_a_negative_window",
     [S().headers(1), S(sends=[(1, 150)]).settings(-200).wu(1, 150).wu(1, 1).headers(3)],
     events=[(0, 0, 0), (0, 0, 0), (SEND_WINDOW_OPENED, 0, 0), (OPENED, 0, 0)], replies=ACK, counters=(3, 0, 2, 0), iws=[200, 0],
     streams={1: (RECV_BODY, BODY_BEFORE_FIRST, 1, W0, 0), 3: (RECV_BODY, BODY_BEFORE_FIRST, 0, W0, 0)})
case("settings_delta_opens_send_windows", S().headers(1).headers(3).priority(5).settings(5),
     events=[(OPENED, 0, 0), (OPENED, 0, 1), (PRIORITY_ONLY_OPENED, 0, 0), (SEND_WINDOW_OPENED, 0, 3)], replies=ACK,
     counters=(3, 0, 2, 1), iws=5,
     streams={1: (RECV_BODY, BODY_BEFORE_FIRST, 5, W0, 0), 3: (RECV_BODY, BODY_BEFORE_FIRST, 5, W0, 0), 5: (IDLE, BODY_NONE, 5, W0, 0)})

# ---- the reply region and the walk's bounds
case("reply_region_exact", S(rep_cap=13 + 17).headers(1, cl=1).ping().data(1, 2),
     events=[(OPENED, 0, 0), (0, 0, 0), (RESET_SENT, -1, 0)], replies=S().ping().frames[0]["ctl_reply"] + RST(1, -1), counters=(1, 0, 0, 0))
case("reply_region_one_byte_short", S(rep_cap=13 + 17 - 1).headers(1, cl=1).ping().data(1, 2), status=SPACE, nstr=2,
     events=[(OPENED, 0, 0), (0, 0, 0)], replies=S().ping().frames[0]["ctl_reply"], counters=(1, 0, 1, 0),
     streams={1: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0)})
case("no_room_for_a_control_reply", S(rep_cap=16).headers(1, True).ping(), status=SPACE, nstr=1, events=[(OPENED | RC, 0, 0)],
     counters=(1, 0, 1, 0), streams={1: (HANDED, BODY_NONE, W0, W0, 0)})
case("frames_behind_the_control_calls_failure", S(nctl=1).headers(1, True).headers(3, True), nstr=1, events=[(OPENED | RC, 0, 0)],
     counters=(1, 0, 1, 0), streams={1: (HANDED, BODY_NONE, W0, W0, 0)})
case("no_frames", S(), counters=(0, 0, 0, 0))

# ---- the ops
case("close_present_and_absent", [S().headers(1).headers(3, True), S().op(3, OP_CLOSE).op(3, OP_CLOSE).op(5, OP_CLOSE)],
     op_events=[(0, 0, 0), (0, ENOENT, 0), (0, ENOENT, 0)], counters=(3, 0, 1, 0), streams={1: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0)})
case("credit_present_and_absent", [S().headers(1).data(1, 1000), S().op(1, OP_CREDIT, 1000).op(3, OP_CREDIT, 5)],
     op_events=[(0, 0, 0), (0, ENOENT, 0)], counters=(1, 0, 1, 0), streams={1: (RECV_BODY, BODY_OPEN, W0, W0 - 1000, 1000)})
case("credit_owes_a_window_update", [BIG, S().op(1, OP_CREDIT, 182).op(1, OP_CREDIT, 1).data(1, 10)],
     op_events=[(0, 0, 0), (WUS, 0, 0)], events=[(BODY, 0, 10)], replies=WU(1, 183), counters=(1, 0, 1, 0),
     streams={1: (RECV_BODY, BODY_OPEN, W0, 183 + 183 - 10, 0)})
case("credit_without_room_for_its_window_update", [BIG, S(rep_cap=12).op(1, OP_CREDIT, 183).data(1, 10)], status=SPACE, nstr=0,
     counters=(1, 0, 1, 0), streams={1: (RECV_BODY, BODY_OPEN, W0, 183, 0)})
case("open_push", [S().settings(-65000), S().op(2, OP_OPEN_PUSH).op(2, OP_OPEN_PUSH).op(3, OP_OPEN_PUSH).op(4, OP_OPEN_PUSH).data(2, 1)],
     op_events=[(0, 0, 0), (0, EINVAL, 0), (0, EINVAL, 0), (0, 0, 0)], events=[(RESET_SENT, -5, 0)], replies=RST(2, -5),
     counters=(0, 4, 0, 0), iws=535, streams={4: (HANDED, BODY_NONE, 535, W0, 0)})
case("open_push_without_room", [S().headers(1), S().op(2, OP_OPEN_PUSH)], op_events=[(0, EFULL, 0)], counters=(1, 0, 1, 0),
     P=params(max_streams=4, max_entries=1), streams={1: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0)})
case("malformed_ops", S().op(0, OP_CLOSE).op(1, 0).op(1, 9).op(1 << 31, OP_CLOSE),
     op_events=[(0, EINVAL, 0), (0, EINVAL, 0), (0, EINVAL, 0), (0, EINVAL, 0)], counters=(0, 0, 0, 0))
case("credit_above_int32_max", [S().headers(1), S().op(1, OP_CREDIT, 1 << 31)], op_events=[(0, EINVAL, 0)], counters=(1, 0, 1, 0),
     streams={1: (RECV_BODY, BODY_BEFORE_FIRST, W0, W0, 0)})


def expected(c):
    return (c["status"], c["err"], c["nstr"], c["events"], c["op_events"], c["replies"], c["counters"], c["streams"])


def observed(w, conn):
    """a walk's result and the connection behind it, in the form of expected()"""
    counters, streams = M.snapshot(conn)
    return (w["status"], w["err"], w["nstr"], [(e[4], e[2], e[1]) for e in w["events"]], [(e[4], e[2], e[1]) for e in w["op_events"]],
            w["replies"], counters, {sid: (s[0], s[1], s[3], s[4], s[5]) for sid, s in streams})


def run_model(c, defects=()):
    conn, w = M.new_conn(), None
    for st, iws in zip(c["steps"], c["iws"]):
        if st.sends:
            ids = [sid for sid, _ in st.sends]
            M.fill_sends(conn, ids)
            M.commit_sent(conn, ids, [n for _, n in st.sends])
        w = M.walk(conn, c["P"], iws, st.frames, st.blocks, st.ops, st.rep_cap, st.nctl, defects)
    return observed(w, conn)
