"""Hand-built HTTP/2 connections for the de-framer (include/hhuff.h (2k)), each with its expected outcome written out:
at least one case per rule and per edge of a rule.  No GPU, no numpy.

  CASES  [dict(name, buf, cap, mfs, mbb, flags, status, err, consumed, nframes, blocks[, frames])]
         blocks  [(stream_id, end_stream_id, flags, dependency, weight, promised_stream_id, nframes, data)]
         frames  (some cases) [(type, block or None, frag_off, frag_len)], offsets relative to buf
"""
from frames_model import (ACCEPT_PUSH, B_CONTINUED, B_END_STREAM, B_EXCLUSIVE, B_PRIORITY, B_PROMISE, B_SELF_DEPENDENCY,
                          E_EXPECTED_CONTINUATION, E_HEADERS_FRAME, E_HEADERS_PRIORITY, E_HEADERS_STREAM_ID,
                          E_INVALID_CONTINUATION, E_NONE, E_PROMISE_FRAME, E_PROMISE_STREAM_ID, E_PUSH_PROMISE, FRAMES,
                          FRAME_SIZE, PROTOCOL, REFUSED)

ES, EH, PAD, PRI = 0x1, 0x4, 0x8, 0x20
DATA, HEADERS, SETTINGS, PUSH, PING, WINDOW_UPDATE, CONT = 0, 1, 4, 5, 6, 8, 9


def head(typ, flags, sid, length):
    return length.to_bytes(3, "big") + bytes([typ, flags]) + sid.to_bytes(4, "big")


def fr(typ, flags, sid, payload=b""):
    return head(typ, flags, sid, len(payload)) + payload


def H(flags, sid, payload=b""):
    return fr(HEADERS, flags, sid, payload)


def CO(flags, sid, payload=b""):
    return fr(CONT, flags, sid, payload)


def PP(flags, sid, payload=b""):
    return fr(PUSH, flags, sid, payload)


CASES = []


def C(name, buf, status, err, consumed, nframes, blocks, cap=64, mfs=16384, mbb=0, flags=0, frames=None):
    CASES.append(dict(name=name, buf=buf, cap=cap, mfs=mfs, mbb=mbb, flags=flags, status=status, err=err, consumed=consumed,
                      nframes=nframes, blocks=blocks, frames=frames))


D2 = fr(DATA, 0, 1, b"dd")  # 11 bytes

# --- complete blocks
C("lone", H(EH, 1, b"\x82\x86"), 0, E_NONE, 11, 1, [(1, 1, 0, 0, 16, 0, 1, b"\x82\x86")], frames=[(HEADERS, 0, 9, 2)])
C("lone_end_stream", H(EH | ES, 3, b"\x82"), 0, E_NONE, 10, 1, [(3, 3, B_END_STREAM, 0, 16, 0, 1, b"\x82")])
C("empty_fragment", H(EH, 1), 0, E_NONE, 9, 1, [(1, 1, 0, 0, 16, 0, 1, b"")], frames=[(HEADERS, 0, 9, 0)])
C("cont1", H(0, 1, b"ab") + CO(EH, 1, b"cd"), 0, E_NONE, 22, 2, [(1, 1, B_CONTINUED, 0, 16, 0, 2, b"abcd")],
  frames=[(HEADERS, 0, 9, 2), (CONT, 0, 20, 2)])
C("cont2_zero_length_cont", H(0, 1, b"ab") + CO(0, 1) + CO(EH, 1, b"c"), 0, E_NONE, 30, 3,
  [(1, 1, B_CONTINUED, 0, 16, 0, 3, b"abc")], frames=[(HEADERS, 0, 9, 2), (CONT, 0, 20, 0), (CONT, 0, 29, 1)])
C("cont3_zero_length_opener", H(ES, 5) + CO(0, 5, b"x") + CO(0, 5, b"yz") + CO(EH, 5, b"w"), 0, E_NONE, 40, 4,
  [(5, 5, B_END_STREAM | B_CONTINUED, 0, 16, 0, 4, b"xyzw")])
C("cont_other_stream", H(0, 1, b"a") + CO(EH, 7, b"b"), 0, E_NONE, 20, 2, [(1, 7, B_CONTINUED, 0, 16, 0, 2, b"ab")])
C("two_blocks", H(EH, 1, b"a") + H(EH, 3, b"bc"), 0, E_NONE, 21, 2, [(1, 1, 0, 0, 16, 0, 1, b"a"), (3, 3, 0, 0, 16, 0, 1, b"bc")])

# --- padding
C("pad_0", H(EH | PAD, 1, b"\x00abc"), 0, E_NONE, 13, 1, [(1, 1, 0, 0, 16, 0, 1, b"abc")], frames=[(HEADERS, 0, 10, 3)])
C("pad_mid", H(EH | PAD, 1, b"\x02hi\x00\x00"), 0, E_NONE, 14, 1, [(1, 1, 0, 0, 16, 0, 1, b"hi")])
C("pad_exact", H(EH | PAD, 1, b"\x03\x00\x00\x00"), 0, E_NONE, 13, 1, [(1, 1, 0, 0, 16, 0, 1, b"")])
C("pad_only_byte", H(EH | PAD, 1, b"\x00"), 0, E_NONE, 10, 1, [(1, 1, 0, 0, 16, 0, 1, b"")])
C("pad_over", H(EH | PAD, 1, b"\x04\x00\x00\x00"), PROTOCOL, E_HEADERS_FRAME, 0, 0, [])
C("pad_length_0", H(EH | PAD, 1), PROTOCOL, E_HEADERS_FRAME, 0, 0, [])

# --- priority
C("prio_5", H(EH | PRI, 1, b"\x00\x00\x00\x03\x0f"), 0, E_NONE, 14, 1, [(1, 1, B_PRIORITY, 3, 16, 0, 1, b"")])
C("prio_fragment", H(EH | PRI, 1, b"\x00\x00\x01\x03\x20zz"), 0, E_NONE, 16, 1, [(1, 1, B_PRIORITY, 259, 33, 0, 1, b"zz")],
  frames=[(HEADERS, 0, 14, 2)])
C("prio_4", H(EH | PRI, 1, b"\x00\x00\x00\x03"), PROTOCOL, E_HEADERS_PRIORITY, 0, 0, [])
C("prio_0", H(EH | PRI, 1), PROTOCOL, E_HEADERS_PRIORITY, 0, 0, [])
C("prio_exclusive_weight_1", H(EH | PRI, 7, b"\x80\x00\x00\x05\x00q"), 0, E_NONE, 15, 1,
  [(7, 7, B_PRIORITY | B_EXCLUSIVE, 5, 1, 0, 1, b"q")])
C("prio_weight_256", H(EH | PRI, 1, b"\x00\x00\x00\x00\xff"), 0, E_NONE, 14, 1, [(1, 1, B_PRIORITY, 0, 256, 0, 1, b"")])
C("pad_prio", H(EH | PAD | PRI, 1, b"\x02\x00\x00\x00\x09\x07hey\x00\x00"), 0, E_NONE, 20, 1,
  [(1, 1, B_PRIORITY, 9, 8, 0, 1, b"hey")], frames=[(HEADERS, 0, 15, 3)])
C("pad_swallows_prio", H(EH | PAD | PRI, 1, b"\x03\x00\x00\x00\x01\x10"), PROTOCOL, E_HEADERS_PRIORITY, 0, 0, [])
C("self_dependency", H(EH | PRI, 5, b"\x00\x00\x00\x05\x0f"), 0, E_NONE, 14, 1,
  [(5, 5, B_PRIORITY | B_SELF_DEPENDENCY, 5, 16, 0, 1, b"")])
C("prio_cont", H(PRI, 9, b"\x80\x00\x00\x09\x01a") + CO(EH, 9, b"b"), 0, E_NONE, 25, 2,
  [(9, 9, B_PRIORITY | B_EXCLUSIVE | B_SELF_DEPENDENCY | B_CONTINUED, 9, 2, 0, 2, b"ab")])

# --- stream ids
C("stream_0", H(EH, 0, b"a"), PROTOCOL, E_HEADERS_STREAM_ID, 0, 0, [])
C("stream_even", H(EH, 2, b"a"), PROTOCOL, E_HEADERS_STREAM_ID, 0, 0, [])
C("stream_even_short_prio", H(EH | PRI, 2), PROTOCOL, E_HEADERS_PRIORITY, 0, 0, [])  # the payload is decoded first
C("stream_0_padded_0", H(EH | PAD, 0), PROTOCOL, E_HEADERS_STREAM_ID, 0, 0, [])
C("stream_top_bit", H(EH, 0x80000001, b"a"), 0, E_NONE, 10, 1, [(1, 1, 0, 0, 16, 0, 1, b"a")])
C("stream_top_bit_only", H(EH, 0x80000000, b"a"), PROTOCOL, E_HEADERS_STREAM_ID, 0, 0, [])

# --- frame size
C("max_frame_size", H(EH, 1, bytes(16384)), 0, E_NONE, 16393, 1, [(1, 1, 0, 0, 16, 0, 1, bytes(16384))])
C("max_frame_size_plus_1_header_only", head(HEADERS, EH, 1, 16385), FRAME_SIZE, E_NONE, 0, 0, [])
C("max_frame_size_plus_1_data", D2 + head(DATA, 0, 1, 16385), FRAME_SIZE, E_NONE, 11, 1, [])
C("max_frame_size_plus_1_in_block", H(0, 1, b"a") + head(CONT, EH, 1, 16385), FRAME_SIZE, E_NONE, 0, 0, [])
C("larger_limit", H(EH, 1, bytes(16385)), 0, E_NONE, 16394, 1, [(1, 1, 0, 0, 16, 0, 1, bytes(16385))], mfs=16385)

# --- incomplete input
for k in range(9):
    C("cut_header_%d" % k, D2 + H(EH, 1, b"abc")[:k], 0, E_NONE, 11, 1, [])
C("cut_payload", H(EH, 1, b"abcdef")[:12], 0, E_NONE, 0, 0, [])
C("cut_data_payload", H(EH, 1, b"a") + fr(DATA, 0, 1, b"dddd")[:11], 0, E_NONE, 10, 1, [(1, 1, 0, 0, 16, 0, 1, b"a")])
C("open_block_at_end", fr(SETTINGS, 0, 0) + fr(PING, 0, 0, bytes(8)) + H(0, 1, b"ab") + CO(0, 1, b"c"), 0, E_NONE, 26, 2, [],
  frames=[(SETTINGS, None, 0, 0), (PING, None, 0, 0)])
C("open_block_cut_in_cont", H(EH, 1, b"k") + H(0, 3, b"ab") + CO(EH, 3, b"zz")[:5], 0, E_NONE, 10, 1, [(1, 1, 0, 0, 16, 0, 1, b"k")])
C("open_block_cut_in_cont_payload", H(0, 3, b"ab") + CO(EH, 3, b"zz")[:10], 0, E_NONE, 0, 0, [])

# --- sequencing
C("data_in_block", H(0, 1, b"a") + D2 + CO(EH, 1, b"b"), PROTOCOL, E_EXPECTED_CONTINUATION, 0, 0, [])
C("headers_in_block", D2 + H(0, 1, b"a") + H(EH, 3, b"b"), PROTOCOL, E_EXPECTED_CONTINUATION, 11, 1, [])
C("unknown_in_block", H(0, 1, b"a") + fr(0xfa, 0, 1) + CO(EH, 1, b"b"), PROTOCOL, E_EXPECTED_CONTINUATION, 0, 0, [])
C("stray_continuation", D2 + CO(EH, 1, b"a"), PROTOCOL, E_INVALID_CONTINUATION, 11, 1, [])
C("continuation_after_block", H(EH, 1, b"a") + CO(EH, 1, b"b"), PROTOCOL, E_INVALID_CONTINUATION, 10, 1,
  [(1, 1, 0, 0, 16, 0, 1, b"a")])

# --- PUSH_PROMISE
C("push_refused", PP(EH, 1, b"\x00\x00\x00\x02ab"), PROTOCOL, E_PUSH_PROMISE, 0, 0, [])
C("push_refused_stream_0", PP(EH, 0), PROTOCOL, E_PUSH_PROMISE, 0, 0, [])
C("push", PP(EH, 1, b"\x00\x00\x00\x02ab"), 0, E_NONE, 15, 1, [(1, 1, B_PROMISE, 0, 16, 2, 1, b"ab")], flags=ACCEPT_PUSH,
  frames=[(PUSH, 0, 13, 2)])
for k in range(4):
    C("push_payload_%d" % k, PP(EH, 1, bytes(k)), PROTOCOL, E_PROMISE_FRAME, 0, 0, [], flags=ACCEPT_PUSH)
C("push_payload_4", PP(EH, 1, b"\xff\xff\xff\xff"), 0, E_NONE, 13, 1, [(1, 1, B_PROMISE, 0, 16, 0x7fffffff, 1, b"")], flags=ACCEPT_PUSH)
C("push_stream_0", PP(EH, 0, b"\x00\x00\x00\x02"), PROTOCOL, E_PROMISE_STREAM_ID, 0, 0, [], flags=ACCEPT_PUSH)
C("push_padded", PP(EH | PAD, 3, b"\x02\x80\x00\x00\x04xyz\x00\x00"), 0, E_NONE, 19, 1, [(3, 3, B_PROMISE, 0, 16, 4, 1, b"xyz")],
  flags=ACCEPT_PUSH, frames=[(PUSH, 0, 14, 3)])
C("push_pad_over", PP(EH | PAD, 3, b"\x05\x00\x00\x00\x04"), PROTOCOL, E_PROMISE_FRAME, 0, 0, [], flags=ACCEPT_PUSH)
C("push_pad_length_0", PP(EH | PAD, 3), PROTOCOL, E_PROMISE_FRAME, 0, 0, [], flags=ACCEPT_PUSH)
C("push_pad_swallows_id", PP(EH | PAD, 3, b"\x02\x00\x00\x00\x04\x00"), PROTOCOL, E_PROMISE_FRAME, 0, 0, [], flags=ACCEPT_PUSH)
C("push_end_stream_bit_ignored", PP(EH | ES, 1, b"\x00\x00\x00\x02"), 0, E_NONE, 13, 1, [(1, 1, B_PROMISE, 0, 16, 2, 1, b"")],
  flags=ACCEPT_PUSH)
C("push_cont", PP(0, 1, b"\x00\x00\x00\x02a") + CO(0, 1, b"b") + CO(EH, 1, b"c"), 0, E_NONE, 34, 3,
  [(1, 1, B_PROMISE | B_CONTINUED, 0, 16, 2, 3, b"abc")], flags=ACCEPT_PUSH)
C("push_then_headers", PP(EH, 1, b"\x00\x00\x00\x02p") + H(EH | ES, 1, b"h"), 0, E_NONE, 24, 2,
  [(1, 1, B_PROMISE, 0, 16, 2, 1, b"p"), (1, 1, B_END_STREAM, 0, 16, 0, 1, b"h")], flags=ACCEPT_PUSH)

# --- other types
C("unknown_type", fr(0xfa, 0xff, 0x7fffffff, b"junk"), 0, E_NONE, 13, 1, [], frames=[(0xfa, None, 0, 0)])
C("interleaved", D2 + H(EH, 1, b"aa") + fr(SETTINGS, 1, 0) + fr(PING, 0, 0, bytes(8)) + H(0, 3, b"b") + CO(EH, 3, b"cc") +
  fr(WINDOW_UPDATE, 0, 0, b"\x00\x00\x10\x00"), 0, E_NONE, 82, 7,
  [(1, 1, 0, 0, 16, 0, 1, b"aa"), (3, 3, B_CONTINUED, 0, 16, 0, 2, b"bcc")],
  frames=[(DATA, None, 0, 0), (HEADERS, 0, 20, 2), (SETTINGS, None, 0, 0), (PING, None, 0, 0), (HEADERS, 1, 57, 1),
          (CONT, 1, 67, 2), (WINDOW_UPDATE, None, 0, 0)])
C("padded_data_not_examined", fr(DATA, PAD, 0, b"\xff"), 0, E_NONE, 10, 1, [])

# --- max_block_bytes
C("block_cap_exact", H(0, 1, bytes(10)) + CO(0, 1, bytes(20)) + CO(EH, 1, bytes(10)), 0, E_NONE, 67, 3,
  [(1, 1, B_CONTINUED, 0, 16, 0, 3, bytes(40))], mbb=40)
C("block_cap_plus_1", H(EH, 3, b"k") + H(0, 1, bytes(10)) + CO(0, 1, bytes(20)) + CO(EH, 1, bytes(11)), REFUSED, E_NONE, 10, 1,
  [(3, 3, 0, 0, 16, 0, 1, b"k")], mbb=40)
C("block_cap_opener_alone", H(EH, 1, bytes(50)), 0, E_NONE, 59, 1, [(1, 1, 0, 0, 16, 0, 1, bytes(50))], mbb=40)
C("block_cap_off", H(0, 1, bytes(10)) + CO(EH, 1, bytes(100)), 0, E_NONE, 128, 2, [(1, 1, B_CONTINUED, 0, 16, 0, 2, bytes(110))])
_BIG = H(0, 1) + CO(0, 1, bytes(16384)) * 25
C("block_cap_reqlen_exact", _BIG + CO(EH, 1, bytes(8192)), 0, E_NONE, 9 + 25 * 16393 + 8201, 27,
  [(1, 1, B_CONTINUED, 0, 16, 0, 27, bytes(417792))], mbb=417792)
C("block_cap_reqlen_plus_1", _BIG + CO(EH, 1, bytes(8193)), REFUSED, E_NONE, 0, 0, [], mbb=417792)

# --- frame slots
C("slots_exact", D2 + H(0, 1, b"a") + CO(EH, 1, b"b"), 0, E_NONE, 31, 3, [(1, 1, B_CONTINUED, 0, 16, 0, 2, b"ab")], cap=3)
C("slots_short_single", D2 + H(EH, 1, b"a"), FRAMES, E_NONE, 11, 1, [], cap=1)
C("slots_short_three", D2 + H(0, 1, b"a") + CO(0, 1, b"b") + CO(EH, 1, b"c"), FRAMES, E_NONE, 11, 1, [], cap=3)
C("slots_none", D2, FRAMES, E_NONE, 0, 0, [], cap=0)
C("slots_none_empty", b"", 0, E_NONE, 0, 0, [], cap=0)
C("slots_error_first", D2 + CO(EH, 1, b"a"), PROTOCOL, E_INVALID_CONTINUATION, 11, 1, [], cap=1)
C("slots_incomplete_first", D2 + H(0, 1, b"a"), 0, E_NONE, 11, 1, [], cap=1)

# --- nothing
C("empty", b"", 0, E_NONE, 0, 0, [])


def busy_and_empty():
    """connections for a batch with empty ones between busy ones: (bufs, caps)"""
    one = H(EH, 1, b"abc")
    return [b"", one, b"", b"", D2 + one, b""], [0, 1, 4, 0, 2, 3]
