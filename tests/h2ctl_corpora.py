"""Hand-built HTTP/2 connections for hhuff_h2_control (include/hhuff.h (2k')), each with its expected outcome written
out: every row of the section's rules on both sides of its edge.  No GPU, no numpy.

  CASES  [dict(name, buf, client, rws, peer, rep_cap, in_size, status, err, nctl, records, replies, after)]
         buf      the connection's bytes (whole frames)            client, rws   HHUFF_H2C_CLIENT, recv_window_size
         peer     the state at the start (h2ctl_model.new_peer() changed by the case's keywords)
         rep_cap  bytes of the reply region (None: the bound)      in_size   None, or a hostile in_size for the records
         records  [(a, b, status, err, flags, reply_len)] as written, the failing frame's included
         after    (settings, flags, send_window, recv_window) of the state afterwards
"""
from h2ctl_model import (E_DATA_FRAME, E_DATA_STREAM_ID, E_FLOW_CONTROL, E_GOAWAY_FRAME, E_GOAWAY_STREAM_ID, E_NONE, E_PING_FRAME,
                         E_PRIORITY_FRAME, E_PRIORITY_STREAM_ID, E_RST_STREAM_FRAME, E_RST_STREAM_STREAM_ID, E_SELF_DEPENDENCY,
                         E_SETTINGS_ACK, E_SETTINGS_FRAME, E_SETTINGS_SIZE, E_SETTINGS_STREAM_ID, E_WINDOW_UPDATE_FRAME, EINVAL,
                         FLOW_CONTROL, FRAME_SIZE, P_GOAWAY, P_SETTINGS, PROTOCOL, R_ACK, R_NEEDS_STREAM, R_STREAM_ERROR,
                         R_WINDOW_DELTA, R_WINDOW_UPDATE, SPACE, new_peer)

DATA, HEADERS, PRIORITY, RST_STREAM, SETTINGS, PING, GOAWAY, WINDOW_UPDATE = 0, 1, 2, 3, 4, 6, 7, 8
ACK, PADDED, EH = 0x1, 0x8, 0x4
NS, SE, WD, WU = R_NEEDS_STREAM, R_STREAM_ERROR, R_WINDOW_DELTA, R_WINDOW_UPDATE
DEF = (4096, 1, 0xFFFFFFFF, 65535, 16384)  # H2O_HTTP2_SETTINGS_DEFAULT
I32MAX = 0x7fffffff


def fr(typ, flags, sid, payload=b""):
    return len(payload).to_bytes(3, "big") + bytes([typ, flags]) + sid.to_bytes(4, "big") + payload


def u32(v):
    return v.to_bytes(4, "big")


def S(*pairs, tail=b"", flags=0, sid=0):
    return fr(SETTINGS, flags, sid, b"".join(i.to_bytes(2, "big") + u32(v) for i, v in pairs) + tail)


def W(sid, inc):
    return fr(WINDOW_UPDATE, 0, sid, u32(inc))


def P(data, flags=0, sid=0):
    return fr(PING, flags, sid, data)


# the replies, byte for byte (lib/http2/frame.c:68-122)
ACK9 = bytes([0, 0, 0, 4, 1, 0, 0, 0, 0])


def PONG(data):
    return bytes([0, 0, 8, 6, 1, 0, 0, 0, 0]) + data


def RST(sid, code):
    return bytes([0, 0, 4, 3, 0]) + u32(sid) + u32(code)


def WUP(inc):
    return bytes([0, 0, 4, 8, 0, 0, 0, 0, 0]) + u32(inc)


CASES = []


def C(name, buf, status, err, nctl, records, replies=b"", settings=DEF, pflags=0, send=65535, recv=65535, client=False, rws=0,
      rep_cap=None, in_size=None, **start):
    peer = new_peer()
    if "start_settings" in start:
        peer["settings"] = list(start.pop("start_settings"))
    peer.update(start)
    if "recv_window" in start and recv == 65535:
        recv = start["recv_window"]
    CASES.append(dict(name=name, buf=buf, client=client, rws=rws, peer=peer, rep_cap=rep_cap, in_size=in_size, status=status,
                      err=err, nctl=nctl, records=records, replies=replies, after=(list(settings), pflags, send, recv)))


def bad(status, err, a=0):
    return (a, 0, status, err, 0, 0)


OPAQUE, OPAQUE2 = b"\x01\x02\x03\x04\xa5\xa6\xa7\xa8", b"\xff\x00\x00\x01\x80\x00\x00\x02"
PING_REC = (0x01020304, 0xa5a6a7a8, 0, E_NONE, 0, 17)
PING2_REC = (0xff000001, 0x80000002, 0, E_NONE, 0, 17)

# --- DATA
C("data_plain", fr(DATA, 0, 1, b"hello"), 0, E_NONE, 1, [(9, 5, 0, E_NONE, NS, 0)])
C("data_empty", fr(DATA, 0, 1), 0, E_NONE, 1, [(9, 0, 0, E_NONE, NS, 0)])
C("data_second_frame_offset", fr(DATA, 1, 3, b"ab") + fr(DATA, 0, 5, b"cde"), 0, E_NONE, 2,
  [(9, 2, 0, E_NONE, NS, 0), (20, 3, 0, E_NONE, NS, 0)])
C("data_stream0", fr(DATA, 0, 0, b"x"), PROTOCOL, E_DATA_STREAM_ID, 0, [bad(PROTOCOL, E_DATA_STREAM_ID)])
C("data_padded_len0", fr(DATA, PADDED, 1), PROTOCOL, E_DATA_FRAME, 0, [bad(PROTOCOL, E_DATA_FRAME)])
C("data_padded", fr(DATA, PADDED, 1, b"\x01abZ"), 0, E_NONE, 1, [(10, 2, 0, E_NONE, NS, 0)])
C("data_pad_is_length_minus_1", fr(DATA, PADDED, 1, b"\x03abc"), 0, E_NONE, 1, [(10, 0, 0, E_NONE, NS, 0)])
C("data_pad_is_length", fr(DATA, PADDED, 1, b"\x04abc"), PROTOCOL, E_DATA_FRAME, 0, [bad(PROTOCOL, E_DATA_FRAME)])
C("data_pad_only_byte", fr(DATA, PADDED, 1, b"\x00"), 0, E_NONE, 1, [(10, 0, 0, E_NONE, NS, 0)])

# --- PRIORITY: lengths 4 / 5 / 6
C("priority_4", fr(PRIORITY, 0, 1, b"\0\0\0\3"), FRAME_SIZE, E_PRIORITY_FRAME, 0, [bad(FRAME_SIZE, E_PRIORITY_FRAME)])
C("priority_5_exclusive_weight_256", fr(PRIORITY, 0, 3, b"\x80\0\0\1\xff"), 0, E_NONE, 1, [(0x80000001, 256, 0, E_NONE, NS, 0)])
C("priority_5_weight_1", fr(PRIORITY, 0, 3, b"\0\0\0\0\0"), 0, E_NONE, 1, [(0, 1, 0, E_NONE, NS, 0)])
C("priority_6", fr(PRIORITY, 0, 1, b"\0\0\0\3\x10\0"), FRAME_SIZE, E_PRIORITY_FRAME, 0, [bad(FRAME_SIZE, E_PRIORITY_FRAME)])
C("priority_stream0_wrong_size", fr(PRIORITY, 0, 0, b"\0\0\0\3"), PROTOCOL, E_PRIORITY_STREAM_ID, 0,
  [bad(PROTOCOL, E_PRIORITY_STREAM_ID)])
C("priority_self", fr(PRIORITY, 0, 5, b"\0\0\0\5\x10"), PROTOCOL, E_SELF_DEPENDENCY, 0, [bad(PROTOCOL, E_SELF_DEPENDENCY)])
C("priority_self_exclusive", fr(PRIORITY, 0, 5, b"\x80\0\0\5\x10"), PROTOCOL, E_SELF_DEPENDENCY, 0,
  [bad(PROTOCOL, E_SELF_DEPENDENCY)])

# --- RST_STREAM: lengths 3 / 4 / 5
C("rst_3", fr(RST_STREAM, 0, 1, b"\0\0\x08"), FRAME_SIZE, E_RST_STREAM_FRAME, 0, [bad(FRAME_SIZE, E_RST_STREAM_FRAME)])
C("rst_4", fr(RST_STREAM, 0, 1, b"\x80\0\0\x08"), 0, E_NONE, 1, [(0x80000008, 0, 0, E_NONE, NS, 0)])
C("rst_5", fr(RST_STREAM, 0, 1, b"\0\0\0\x08\0"), FRAME_SIZE, E_RST_STREAM_FRAME, 0, [bad(FRAME_SIZE, E_RST_STREAM_FRAME)])
C("rst_stream0", fr(RST_STREAM, 0, 0, b"\0\0\0\x08"), PROTOCOL, E_RST_STREAM_STREAM_ID, 0, [bad(PROTOCOL, E_RST_STREAM_STREAM_ID)])
C("rst_stream0_wrong_size", fr(RST_STREAM, 0, 0, b"\0\0\x08"), PROTOCOL, E_RST_STREAM_STREAM_ID, 0,
  [bad(PROTOCOL, E_RST_STREAM_STREAM_ID)])

# --- SETTINGS
C("settings_no_pairs", S(), 0, E_NONE, 1, [(0, 0, 0, E_NONE, 0, 9)], ACK9, pflags=P_SETTINGS)
C("settings_one_pair", S((1, 256)), 0, E_NONE, 1, [(1, 0, 0, E_NONE, 0, 9)], ACK9, (256, 1, 0xFFFFFFFF, 65535, 16384), P_SETTINGS)
C("settings_all_five", S((1, 0), (2, 0), (3, 100), (4, 1 << 20), (5, 32768)), 0, E_NONE, 1,
  [(5, (1 << 20) - 65535, 0, E_NONE, WD, 9)], ACK9, (0, 0, 100, 1 << 20, 32768), P_SETTINGS)
C("settings_stream1", S((1, 256), sid=1), PROTOCOL, E_SETTINGS_STREAM_ID, 0, [bad(PROTOCOL, E_SETTINGS_STREAM_ID)])
C("settings_ack", S(flags=ACK), 0, E_NONE, 1, [(0, 0, 0, E_NONE, R_ACK, 0)])
C("settings_ack_with_payload", S((1, 256), flags=ACK), FRAME_SIZE, E_SETTINGS_ACK, 0, [bad(FRAME_SIZE, E_SETTINGS_ACK)])
C("settings_repeated_identifier", S((1, 100), (1, 200)), 0, E_NONE, 1, [(2, 0, 0, E_NONE, 0, 9)], ACK9,
  (200, 1, 0xFFFFFFFF, 65535, 16384), P_SETTINGS)
C("settings_unknown_identifier", S((0x99, 5), (0, 7), (6, 9), (3, 77)), 0, E_NONE, 1, [(4, 0, 0, E_NONE, 0, 9)], ACK9,
  (4096, 1, 77, 65535, 16384), P_SETTINGS)
C("settings_enable_push_0", S((2, 0)), 0, E_NONE, 1, [(1, 0, 0, E_NONE, 0, 9)], ACK9, (4096, 0, 0xFFFFFFFF, 65535, 16384), P_SETTINGS)
C("settings_enable_push_2_behind_applied_pair", S((1, 0), (2, 2), (3, 5)), PROTOCOL, E_SETTINGS_FRAME, 0,
  [bad(PROTOCOL, E_SETTINGS_FRAME, 1)], b"", (0, 1, 0xFFFFFFFF, 65535, 16384))
C("settings_window_7fffffff", S((4, I32MAX)), 0, E_NONE, 1, [(1, I32MAX - 65535, 0, E_NONE, WD, 9)], ACK9,
  (4096, 1, 0xFFFFFFFF, I32MAX, 16384), P_SETTINGS)
C("settings_window_80000000", S((4, 0x80000000)), FLOW_CONTROL, E_SETTINGS_FRAME, 0, [bad(FLOW_CONTROL, E_SETTINGS_FRAME)])
C("settings_window_unchanged", S((4, 65535)), 0, E_NONE, 1, [(1, 0, 0, E_NONE, 0, 9)], ACK9, pflags=P_SETTINGS)
C("settings_window_0", S((4, 0)), 0, E_NONE, 1, [(1, 0xFFFF0001, 0, E_NONE, WD, 9)], ACK9, (4096, 1, 0xFFFFFFFF, 0, 16384), P_SETTINGS)
C("settings_frame_size_16383", S((5, 16383)), PROTOCOL, E_SETTINGS_FRAME, 0, [bad(PROTOCOL, E_SETTINGS_FRAME)])
C("settings_frame_size_16384", S((5, 16384)), 0, E_NONE, 1, [(1, 0, 0, E_NONE, 0, 9)], ACK9, pflags=P_SETTINGS)
C("settings_frame_size_16777215", S((5, 16777215)), 0, E_NONE, 1, [(1, 0, 0, E_NONE, 0, 9)], ACK9,
  (4096, 1, 0xFFFFFFFF, 65535, 16777215), P_SETTINGS)
C("settings_frame_size_16777216", S((5, 16777216)), PROTOCOL, E_SETTINGS_FRAME, 0, [bad(PROTOCOL, E_SETTINGS_FRAME)])
C("settings_length_7_behind_valid_pair", S((1, 512), tail=b"\0"), FRAME_SIZE, E_SETTINGS_SIZE, 0,
  [bad(FRAME_SIZE, E_SETTINGS_SIZE, 1)], b"", (512, 1, 0xFFFFFFFF, 65535, 16384))
C("settings_length_5", S(tail=b"\0\1\0\0\0"), FRAME_SIZE, E_SETTINGS_SIZE, 0, [bad(FRAME_SIZE, E_SETTINGS_SIZE)])
C("two_settings_with_different_deltas", S((4, 100000)) + S((4, 50000)), 0, E_NONE, 2,
  [(1, 34465, 0, E_NONE, WD, 9), (1, 0xFFFF3CB0, 0, E_NONE, WD, 9)], ACK9 + ACK9, (4096, 1, 0xFFFFFFFF, 50000, 16384), P_SETTINGS)
C("settings_from_a_changed_start", S((5, 20000)), 0, E_NONE, 1, [(1, 0, 0, E_NONE, 0, 9)], ACK9, (0, 0, 7, 1000, 20000), P_SETTINGS,
  start_settings=[0, 0, 7, 1000, 65536])

# --- PING: lengths 7 / 8 / 9
C("ping_7", P(OPAQUE[:7]), FRAME_SIZE, E_PING_FRAME, 0, [bad(FRAME_SIZE, E_PING_FRAME)])
C("ping_8", P(OPAQUE), 0, E_NONE, 1, [PING_REC], PONG(OPAQUE))
C("ping_9", P(OPAQUE + b"\0"), FRAME_SIZE, E_PING_FRAME, 0, [bad(FRAME_SIZE, E_PING_FRAME)])
C("ping_ack", P(OPAQUE2, flags=ACK), 0, E_NONE, 1, [(0xff000001, 0x80000002, 0, E_NONE, R_ACK, 0)])
C("ping_stream1", P(OPAQUE, sid=1), PROTOCOL, E_PING_FRAME, 0, [bad(PROTOCOL, E_PING_FRAME)])
C("ping_stream1_wrong_size", P(OPAQUE[:7], sid=1), PROTOCOL, E_PING_FRAME, 0, [bad(PROTOCOL, E_PING_FRAME)])

# --- GOAWAY: lengths 7 / 8 / 8 + debug data
C("goaway_7", fr(GOAWAY, 0, 0, b"\0\0\0\5\0\0\0"), FRAME_SIZE, E_GOAWAY_FRAME, 0, [bad(FRAME_SIZE, E_GOAWAY_FRAME)])
C("goaway_8_reserved_bit", fr(GOAWAY, 0, 0, b"\x80\0\0\7\0\0\0\2"), 0, E_NONE, 1, [(7, 2, 0, E_NONE, 0, 0)], pflags=P_GOAWAY)
C("goaway_debug_data", fr(GOAWAY, 0, 0, b"\0\0\0\x09\xff\0\0\x0bbye"), 0, E_NONE, 1, [(9, 0xff00000b, 0, E_NONE, 0, 0)], pflags=P_GOAWAY)
C("goaway_stream1", fr(GOAWAY, 0, 1, b"\0\0\0\7\0\0\0\2"), PROTOCOL, E_GOAWAY_STREAM_ID, 0, [bad(PROTOCOL, E_GOAWAY_STREAM_ID)])
C("goaway_stream1_wrong_size", fr(GOAWAY, 0, 1, b"\0\0\0\7\0\0\0"), PROTOCOL, E_GOAWAY_STREAM_ID, 0,
  [bad(PROTOCOL, E_GOAWAY_STREAM_ID)])

# --- WINDOW_UPDATE: lengths 3 / 4 / 5, the zero increment, the send window
C("window_update_3", fr(WINDOW_UPDATE, 0, 0, b"\0\0\1"), FRAME_SIZE, E_WINDOW_UPDATE_FRAME, 0, [bad(FRAME_SIZE, E_WINDOW_UPDATE_FRAME)])
C("window_update_3_on_a_stream", fr(WINDOW_UPDATE, 0, 1, b"\0\0\1"), FRAME_SIZE, E_WINDOW_UPDATE_FRAME, 0,
  [bad(FRAME_SIZE, E_WINDOW_UPDATE_FRAME)])
C("window_update_4", W(0, 1000), 0, E_NONE, 1, [(1000, 0, 0, E_NONE, 0, 0)], send=66535)
C("window_update_5", fr(WINDOW_UPDATE, 0, 0, b"\0\0\0\1\0"), FRAME_SIZE, E_WINDOW_UPDATE_FRAME, 0,
  [bad(FRAME_SIZE, E_WINDOW_UPDATE_FRAME)])
C("window_update_on_a_stream_reserved_bit", W(3, 0x80000010), 0, E_NONE, 1, [(16, 0, 0, E_NONE, NS, 0)])
C("window_update_zero_on_stream0", W(0, 0), PROTOCOL, E_WINDOW_UPDATE_FRAME, 0, [bad(PROTOCOL, E_WINDOW_UPDATE_FRAME)])
C("window_update_80000000_on_stream0", W(0, 0x80000000), PROTOCOL, E_WINDOW_UPDATE_FRAME, 0, [bad(PROTOCOL, E_WINDOW_UPDATE_FRAME)])
C("window_update_zero_on_a_stream_walk_goes_on", W(5, 0) + P(OPAQUE), 0, E_NONE, 2,
  [(0, 0, PROTOCOL, E_WINDOW_UPDATE_FRAME, SE | NS, 13), PING_REC], RST(5, 1) + PONG(OPAQUE))
C("window_update_80000000_on_a_stream", W(0x7fffffff, 0x80000000), 0, E_NONE, 1,
  [(0, 0, PROTOCOL, E_WINDOW_UPDATE_FRAME, SE | NS, 13)], RST(0x7fffffff, 1))
C("send_window_lands_on_int32_max", W(0, I32MAX - 65535), 0, E_NONE, 1, [(I32MAX - 65535, 0, 0, E_NONE, 0, 0)], send=I32MAX)
C("send_window_one_past_int32_max", W(0, I32MAX - 65534), FLOW_CONTROL, E_FLOW_CONTROL, 0, [bad(FLOW_CONTROL, E_FLOW_CONTROL)])
C("send_window_accumulates_then_overflows", W(0, 1000) + W(0, I32MAX - 66535) + W(0, 1), FLOW_CONTROL, E_FLOW_CONTROL, 2,
  [(1000, 0, 0, E_NONE, 0, 0), (I32MAX - 66535, 0, 0, E_NONE, 0, 0), bad(FLOW_CONTROL, E_FLOW_CONTROL)], send=I32MAX)
C("send_window_from_a_negative_start", W(0, I32MAX), 0, E_NONE, 1, [(I32MAX, 0, 0, E_NONE, 0, 0)], send=I32MAX - 70000,
  send_window=-70000)

# --- the server's receive window (connection.c:986-989)
D499 = fr(DATA, PADDED, 1, b"\x0a" + b"d" * 488 + b"\0" * 10)  # 499 bytes of payload, 488 of data
C("recv_window_crosses_half_at_exactly_one_frame", D499 + fr(DATA, 0, 1, b"x"), 0, E_NONE, 2,
  [(10, 488, 0, E_NONE, NS, 0), (517, 1, 0, E_NONE, NS | WU, 13)], WUP(500), rws=1000, recv=1000, recv_window=1000)
C("recv_window_one_above_half", D499, 0, E_NONE, 1, [(10, 488, 0, E_NONE, NS, 0)], rws=1000, recv=501, recv_window=1000)
C("recv_window_client_left_alone", D499 + fr(DATA, 0, 1, b"x"), 0, E_NONE, 2, [(10, 488, 0, E_NONE, NS, 0), (517, 1, 0, E_NONE, NS, 0)],
  client=True, rws=1000, recv=1000, recv_window=1000)
C("recv_window_not_kept", D499 + fr(DATA, 0, 1, b"x"), 0, E_NONE, 2, [(10, 488, 0, E_NONE, NS, 0), (517, 1, 0, E_NONE, NS, 0)],
  rws=0, recv=1000, recv_window=1000)
C("recv_window_new_connection_h2o_size", fr(DATA, 0, 1, b"12345"), 0, E_NONE, 1, [(9, 5, 0, E_NONE, NS | WU, 13)],
  WUP(16777216 - 65530), rws=16777216, recv=16777216)
C("recv_window_refused_data_not_charged", fr(DATA, PADDED, 1, b"\x09abc"), PROTOCOL, E_DATA_FRAME, 0, [bad(PROTOCOL, E_DATA_FRAME)],
  rws=4, recv=1000, recv_window=1000)

# --- other types: zeroed records
C("unknown_types_and_header_frames", fr(0x0a, 0xff, 7, b"altsvc") + fr(0xfa, 0, 0, b"\1") + fr(HEADERS, EH, 1, b"\x82") + P(OPAQUE), 0,
  E_NONE, 4, [(0, 0, 0, E_NONE, 0, 0)] * 3 + [PING_REC], PONG(OPAQUE))
C("empty_connection", b"", 0, E_NONE, 0, [])

# --- the first failure cuts the rest; replies owed on both sides of it
C("failure_in_the_middle", P(OPAQUE) + S((1, 128)) + fr(PRIORITY, 0, 1, b"\0\0\0\3") + P(OPAQUE2) + S((1, 64)), FRAME_SIZE,
  E_PRIORITY_FRAME, 2, [PING_REC, (1, 0, 0, E_NONE, 0, 9), bad(FRAME_SIZE, E_PRIORITY_FRAME)], PONG(OPAQUE) + ACK9,
  (128, 1, 0xFFFFFFFF, 65535, 16384), P_SETTINGS)
C("everything_in_one_step", S((4, 70000), (1, 0)) + W(0, 5) + P(OPAQUE2) + fr(DATA, 0, 1, b"body") + S(flags=ACK) +
  fr(GOAWAY, 0, 0, b"\0\0\0\1\0\0\0\0"), 0, E_NONE, 6,
  [(2, 4465, 0, E_NONE, WD, 9), (5, 0, 0, E_NONE, 0, 0), PING2_REC, (60, 4, 0, E_NONE, NS, 0), (0, 0, 0, E_NONE, R_ACK, 0),
   (1, 0, 0, E_NONE, 0, 0)], ACK9 + PONG(OPAQUE2), (0, 1, 0xFFFFFFFF, 70000, 16384), P_SETTINGS | P_GOAWAY, send=65540)

# --- reply space
C("space_exact", P(OPAQUE) + S((1, 99)), 0, E_NONE, 2, [PING_REC, (1, 0, 0, E_NONE, 0, 9)], PONG(OPAQUE) + ACK9,
  (99, 1, 0xFFFFFFFF, 65535, 16384), P_SETTINGS, rep_cap=26)
C("space_one_short_nothing_applied", P(OPAQUE) + S((1, 99)) + P(OPAQUE2), SPACE, E_NONE, 1, [PING_REC], PONG(OPAQUE), rep_cap=25)
C("space_none_for_the_window_update", fr(DATA, 0, 1, b"abcdef"), SPACE, E_NONE, 0, [], rws=10, recv=10, recv_window=10, rep_cap=12)
C("space_zero_but_nothing_owed", S(flags=ACK) + W(0, 1) + fr(DATA, 0, 1, b"a"), 0, E_NONE, 3,
  [(0, 0, 0, E_NONE, R_ACK, 0), (1, 0, 0, E_NONE, 0, 0), (31, 1, 0, E_NONE, NS, 0)], send=65536, rep_cap=0)

# --- a hostile frame record (its payload leaves in_size)
C("record_past_in_size", S((1, 99)) + P(OPAQUE), EINVAL, E_NONE, 1, [(1, 0, 0, E_NONE, 0, 9)], ACK9, (99, 1, 0xFFFFFFFF, 65535, 16384),
  P_SETTINGS, in_size=31)
