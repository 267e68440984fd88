"""Hand-built HTTP/3 streams for the de-framer (include/hhuff.h (2l)), each with its literal expectations beside it:
status, error, consumed, the frames listed as (type, avail, aux), the state to present next, the section's and the
encoder run's bytes, and what SETTINGS said as (max_table_capacity, max_blocked, max_field_section_size, h3_datagram).
Names begin with the side (s_: h2o's server receives, c_: its client) or, where the side does not matter, the kind of
stream.  connections() puts the streams together into connections for the batch tests."""
import h3frames_model as M

S, C = 0, M.CLIENT
NONE64 = M.NONE64
PU_REQ, PU_PUSH = M.PRIORITY_UPDATE_REQUEST, M.PRIORITY_UPDATE_PUSH
GP, FU, FR, XL = M.GENERAL_PROTOCOL, M.FRAME_UNEXPECTED, M.FRAME, M.EXCESSIVE_LOAD


def vi(v, width=None):
    """a QUIC varint of `width` bytes (default: the shortest)"""
    if width is None:
        width = 1 if v < 1 << 6 else 2 if v < 1 << 14 else 4 if v < 1 << 30 else 8
    assert v < 1 << (8 * width - 2)
    return ((v | ({1: 0, 2: 1, 4: 2, 8: 3}[width] << (8 * width - 2))).to_bytes(width, "big"))


def fr(typ, payload=b"", tw=None, lw=None, length=None):
    """a frame; length: the length field when it is not the payload's"""
    return vi(typ, tw) + vi(len(payload) if length is None else length, lw) + payload


def st(kind=M.K_REQUEST, phase=0, flags=0, data_left=0, stream_id=0, rsv=0):
    return dict(kind=kind, phase=phase, flags=flags, data_left=data_left, stream_id=stream_id, rsv=rsv)


CASES = []


def case(name, flags, buf, state, out, status=0, err=M.E_NONE, consumed=None, frames=(), section=None, enc=None, settings=None,
         cap=8, mfps=16384):
    """out: (kind, phase, data_left) to present next; consumed: default everything"""
    CASES.append(dict(name=name, flags=flags, buf=buf, st=state, cap=cap, mfps=mfps, status=status, err=err,
                      consumed=len(buf) if consumed is None else consumed, frames=list(frames), out=out, section=section, enc=enc,
                      settings=settings))


REQ_H, REQ_D, REQ_P, REQ_T = (M.K_REQUEST, M.P_HEADERS, 0), (M.K_REQUEST, M.P_DATA, 0), M.P_DATA_PAYLOAD, (M.K_REQUEST, M.P_POST_TRAILERS, 0)
SEC = b"\x00\x00\xd1\xd7\x50\x83abc"  # (the de-framer does not look inside a section)
HDRS = fr(M.HEADERS, SEC)
NOSEC = M.NOSEC

# ---- rule 1: read_frame -------------------------------------------------------------------------------------------
case("s_empty", S, b"", st(), REQ_H)
case("s_type_cut", S, b"\x40", st(), REQ_H, consumed=0)
case("s_type_cut_8", S, b"\xc0\x00\x00\x00\x00\x00\x00", st(), REQ_H, consumed=0)
case("s_length_cut", S, b"\x01\x80\x00\x00", st(), REQ_H, consumed=0)
case("s_payload_cut", S, HDRS[:-1], st(), REQ_H, consumed=0)
case("s_too_large_before_complete", S, fr(0x21, b"", length=16385), st(), REQ_H, GP, M.E_FRAME_TOO_LARGE, 0)
case("s_at_the_limit", S, fr(0x21, b"x" * 16384, lw=4)[:8] + b"y" * 40, st(), REQ_H, consumed=0)
case("s_at_a_small_limit", S, fr(0x21, b"x" * 40), st(), REQ_H, frames=[(0x21, 40, 0)], mfps=40)
case("s_small_limit", S, fr(0x21, b"xy"), st(), REQ_H, GP, M.E_FRAME_TOO_LARGE, 0, mfps=1)
case("s_settings_on_request_cut", S, fr(M.SETTINGS, b"\x01", length=5), st(), REQ_H, consumed=0)
case("s_settings_on_request", S, fr(M.SETTINGS, b"\x01\x02"), st(), REQ_H, FU, consumed=0)
case("s_goaway_on_request_in_data", S, fr(M.GOAWAY, b"\x00"), st(phase=M.P_DATA), REQ_D, FU, consumed=0)
case("s_push_promise", S, fr(M.PUSH_PROMISE, b"\x01"), st(phase=M.P_DATA), REQ_D, FU, consumed=0)
case("s_non_minimal_varints", S, fr(M.HEADERS, SEC, tw=8, lw=4), st(stream_id=8), REQ_D, frames=[(M.HEADERS, len(SEC), 0)],
     section=SEC)
case("s_non_minimal_2_and_4", S, fr(0x21, b"q", tw=2, lw=8) + fr(M.HEADERS, SEC, tw=4, lw=2), st(), REQ_D,
     frames=[(0x21, 1, 0), (M.HEADERS, len(SEC), 0)], section=SEC)
case("s_type_above_2_32", S, fr((1 << 40) + 0x21, b"zz") + HDRS, st(), REQ_D, frames=[((1 << 40) + 0x21, 2, 0), (M.HEADERS, len(SEC), 0)],
     section=SEC)
# ---- rule 2: the server before HEADERS ------------------------------------------------------------------------------
case("s_headers_too_large", S, fr(M.HEADERS, b"", length=16385), st(), REQ_H, M.REJECTED, M.E_FRAME_TOO_LARGE, 0)
case("s_data_before_headers", S, fr(M.DATA, b"abc"), st(), REQ_H, FU, consumed=0)
case("s_unknown_then_cut", S, fr(0x40, b"grease") + HDRS[:3], st(), REQ_H, consumed=9, frames=[(0x40, 6, 0)])
# ---- rule 3: the section and the stop behind it ---------------------------------------------------------------------
case("s_headers", S, HDRS, st(stream_id=4), REQ_D, frames=[(M.HEADERS, len(SEC), 0)], section=SEC)
case("s_empty_headers", S, fr(M.HEADERS), st(), REQ_D, frames=[(M.HEADERS, 0, 0)], section=b"")
case("s_stop_behind_section", S, HDRS + fr(M.DATA, b"body"), st(), REQ_D, consumed=len(HDRS), frames=[(M.HEADERS, len(SEC), 0)],
     section=SEC)
case("s_walk_on", S, HDRS + fr(M.DATA, b"body") + fr(M.HEADERS, b"trailers") + fr(0x21), st(flags=M.S_WALK_ON), REQ_T,
     frames=[(M.HEADERS, len(SEC), 0), (M.DATA, 4, 0), (M.HEADERS, 8, NOSEC), (0x21, 0, 0)], section=SEC)
# ---- rule 4: the server's body ----------------------------------------------------------------------------------------
case("s_trailers", S, fr(M.HEADERS, b"trailers"), st(phase=M.P_DATA), REQ_T, frames=[(M.HEADERS, 8, NOSEC)])
case("s_tunnel_headers", S, fr(M.HEADERS, b"t"), st(phase=M.P_DATA, flags=M.S_TUNNEL), REQ_D, FU, M.E_UNEXPECTED_TYPE, 0)
case("s_data_whole", S, fr(M.DATA, b"0123456789") + fr(M.DATA, b"ab"), st(phase=M.P_DATA), REQ_D, frames=[(M.DATA, 10, 0), (M.DATA, 2, 0)])
case("s_data_partial", S, fr(M.DATA, b"0123", length=10), st(phase=M.P_DATA), (M.K_REQUEST, REQ_P, 6), frames=[(M.DATA, 4, 0)])
case("s_data_header_only", S, fr(M.DATA, b"", length=10), st(phase=M.P_DATA), (M.K_REQUEST, REQ_P, 10), frames=[(M.DATA, 0, 0)])
case("s_data_resume", S, b"456789" + fr(M.DATA) + fr(0x21, b"x"), st(phase=REQ_P, data_left=6), REQ_D,
     frames=[(M.DATA, 6, 0), (M.DATA, 0, 0), (0x21, 1, 0)])
case("s_data_resume_short", S, b"45", st(phase=REQ_P, data_left=6), (M.K_REQUEST, REQ_P, 4), frames=[(M.DATA, 2, 0)])
case("s_data_zero", S, fr(M.DATA), st(phase=M.P_DATA), REQ_D, frames=[(M.DATA, 0, 0)])
case("s_data_above_2_32", S, fr(M.DATA, b"01234", length=1 << 33), st(phase=M.P_DATA), (M.K_REQUEST, REQ_P, (1 << 33) - 5),
     frames=[(M.DATA, 5, 0)])
case("s_data_above_2_32_goes_on", S, b"567", st(phase=REQ_P, data_left=(1 << 33) - 5), (M.K_REQUEST, REQ_P, (1 << 33) - 8),
     frames=[(M.DATA, 3, 0)])
case("s_data_any_size_passes_the_limit", S, fr(M.DATA, b"x" * 40), st(phase=M.P_DATA), REQ_D, frames=[(M.DATA, 40, 0)], mfps=8)
# ---- rule 5: behind the trailers --------------------------------------------------------------------------------------
case("s_post_trailers_headers", S, fr(M.HEADERS, b"t"), st(phase=M.P_POST_TRAILERS), REQ_T, FU, consumed=0)
case("s_post_trailers_data", S, fr(0x21) + fr(M.DATA, b"d"), st(phase=M.P_POST_TRAILERS), REQ_T, FU, consumed=2, frames=[(0x21, 0, 0)])
case("s_post_trailers_too_large", S, fr(0x21, length=20000), st(phase=M.P_POST_TRAILERS), REQ_T, GP, M.E_FRAME_TOO_LARGE, 0)
# ---- rule 6: the client before HEADERS --------------------------------------------------------------------------------
case("c_headers", C, HDRS + fr(M.DATA, b"body"), st(stream_id=12), REQ_D, consumed=len(HDRS), frames=[(M.HEADERS, len(SEC), 0)],
     section=SEC)
case("c_headers_too_large", C, fr(M.HEADERS, b"", length=16385), st(), REQ_H, XL, M.E_RESPONSE_TOO_LARGE, 0)
case("c_unexpected_before_headers", C, fr(M.SETTINGS), st(), REQ_H, XL, M.E_RESPONSE_TOO_LARGE, 0)
case("c_data_before_headers", C, fr(M.DATA, b"abc"), st(), REQ_H, FU, M.E_DATA_BEFORE_HEADERS, 0)
case("c_push_promise_before_headers", C, fr(M.PUSH_PROMISE, b"\x01") + HDRS[:2], st(), REQ_H, consumed=3, frames=[(M.PUSH_PROMISE, 1, 0)])
# ---- rule 7: the client's body ----------------------------------------------------------------------------------------
case("c_walk_on", C, HDRS + fr(M.DATA, b"body") + fr(M.HEADERS, b"trailers") + fr(M.PUSH_PROMISE, b"\x02") + fr(M.DATA, b"more", length=6),
     st(flags=M.S_WALK_ON), (M.K_REQUEST, REQ_P, 2),
     frames=[(M.HEADERS, len(SEC), 0), (M.DATA, 4, 0), (M.HEADERS, 8, NOSEC), (M.PUSH_PROMISE, 1, 0), (M.DATA, 4, 0)], section=SEC)
case("c_tunnel_headers", C, fr(M.HEADERS, b"t"), st(phase=M.P_DATA, flags=M.S_TUNNEL), REQ_D, FU, consumed=0)
case("c_too_large_in_data", C, fr(0x21, length=16385), st(phase=M.P_DATA), REQ_D, GP, M.E_FRAME_TOO_LARGE, 0)
case("c_unexpected_in_data", C, fr(M.CANCEL_PUSH, b"\x00"), st(phase=M.P_DATA), REQ_D, FU, consumed=0)
case("c_data_zero", C, fr(M.DATA), st(phase=M.P_DATA), REQ_D, frames=[(M.DATA, 0, 0)])
case("c_post_trailers_state", C, HDRS, st(phase=M.P_POST_TRAILERS), REQ_T, M.EINVAL, consumed=0)
# ---- rules 8-11: unidirectional streams -------------------------------------------------------------------------------
UNI = (M.K_UNI, 0, 0)
SET = fr(M.SETTINGS, vi(1) + vi(4096) + vi(7) + vi(100) + vi(6) + vi(65536))
case("uni_empty", S, b"", st(M.K_UNI), UNI)
case("uni_type_cut", S, b"\x80\x00\x00", st(M.K_UNI), UNI, consumed=0)
case("uni_control", S, b"\x00" + SET + fr(M.CANCEL_PUSH, b"\x07"), st(M.K_UNI), (M.K_CONTROL, M.P_OPEN, 0),
     frames=[(M.SETTINGS, len(SET) - 2, 0), (M.CANCEL_PUSH, 1, 0)], settings=(4096, 100, 65536, 0))
case("uni_control_alone", C, b"\x00", st(M.K_UNI), (M.K_CONTROL, M.P_SETTINGS, 0))
case("uni_encoder", S, vi(2, 2) + b"\x3f\xe1\x1f\xc0", st(M.K_UNI), (M.K_QPACK_ENCODER, 0, 0), enc=b"\x3f\xe1\x1f\xc0")
case("uni_decoder", C, b"\x03\x80\x81", st(M.K_UNI), (M.K_QPACK_DECODER, 0, 0), consumed=1)
case("uni_push_stream", C, b"\x01\x04\x00", st(M.K_UNI), (M.K_DISCARD, 0, 0))
case("uni_grease", S, vi(0x21 + 0x1f * 7, 4) + b"whatever", st(M.K_UNI), (M.K_DISCARD, 0, 0))
case("encoder_stream", S, b"\x20\xc0", st(M.K_QPACK_ENCODER), (M.K_QPACK_ENCODER, 0, 0), enc=b"\x20\xc0")
case("encoder_stream_empty", S, b"", st(M.K_QPACK_ENCODER), (M.K_QPACK_ENCODER, 0, 0))
case("decoder_stream", S, b"\x84\x85", st(M.K_QPACK_DECODER), (M.K_QPACK_DECODER, 0, 0), consumed=0)
case("discard_stream", S, b"anything", st(M.K_DISCARD), (M.K_DISCARD, 0, 0))
# ---- rule 12: the control stream's order -----------------------------------------------------------------------------
CTL_S, CTL_O = (M.K_CONTROL, M.P_SETTINGS, 0), (M.K_CONTROL, M.P_OPEN, 0)
case("ctl_first_frame_not_settings", S, fr(M.GOAWAY, b"\x00"), st(M.K_CONTROL), CTL_S, FU, consumed=0)
case("ctl_unknown_before_settings", C, fr(0x21), st(M.K_CONTROL), CTL_S, FU, consumed=0)
case("ctl_second_settings", S, fr(0x21) + SET, st(M.K_CONTROL, M.P_OPEN), CTL_O, FU, consumed=2, frames=[(0x21, 0, 0)])
case("ctl_data", S, fr(M.DATA), st(M.K_CONTROL, M.P_OPEN), CTL_O, FU, consumed=0)
case("ctl_headers", C, fr(M.HEADERS, b"h"), st(M.K_CONTROL, M.P_OPEN), CTL_O, FU, consumed=0)
case("ctl_max_push_id_at_the_server", S, fr(M.MAX_PUSH_ID, b"\x09"), st(M.K_CONTROL, M.P_OPEN), CTL_O, frames=[(M.MAX_PUSH_ID, 1, 0)])
case("ctl_max_push_id_at_the_client", C, fr(M.MAX_PUSH_ID, b"\x09"), st(M.K_CONTROL, M.P_OPEN), CTL_O, FU, consumed=0)
case("ctl_settings_cut", S, SET[:-1], st(M.K_CONTROL), CTL_S, consumed=0)
case("ctl_settings_too_large", S, fr(M.SETTINGS, length=17000), st(M.K_CONTROL), CTL_S, GP, M.E_FRAME_TOO_LARGE, 0)
# ---- rule 13: the control stream's payloads --------------------------------------------------------------------------
case("ctl_settings_empty", C, fr(M.SETTINGS), st(M.K_CONTROL), CTL_O, frames=[(M.SETTINGS, 0, 0)], settings=(0, 0, NONE64, 0))
case("ctl_settings_repeated_id", S, fr(M.SETTINGS, vi(1) + vi(100) + vi(1) + vi(200) + vi(0x21) + vi(5)), st(M.K_CONTROL), CTL_O,
     frames=[(M.SETTINGS, 8, 0)], settings=(200, 0, NONE64, 0))
case("ctl_settings_saturated", S, fr(M.SETTINGS, vi(1) + vi(1 << 40) + vi(7, 2) + vi((1 << 62) - 1) + vi(6) + vi((1 << 62) - 1)),
     st(M.K_CONTROL), CTL_O, frames=[(M.SETTINGS, 28, 0)], settings=(0xFFFFFFFF, 0xFFFFFFFF, (1 << 62) - 1, 0))
case("ctl_settings_value_cut", S, fr(M.SETTINGS, vi(1) + b"\x40"), st(M.K_CONTROL), CTL_S, FR, M.E_MALFORMED_SETTINGS, 0)
case("ctl_settings_id_cut", C, fr(M.SETTINGS, vi(7) + vi(1) + b"\xc0\x00"), st(M.K_CONTROL), CTL_S, FR, M.E_MALFORMED_SETTINGS, 0)
case("ctl_settings_datagram_2", S, fr(M.SETTINGS, vi(0x33) + vi(2)), st(M.K_CONTROL, flags=M.S_PEER_DATAGRAMS), CTL_S, FR,
     M.E_MALFORMED_SETTINGS, 0)
case("ctl_settings_datagram_without_transport", S, fr(M.SETTINGS, vi(0x276) + vi(1)), st(M.K_CONTROL), CTL_S, FR, M.E_MALFORMED_SETTINGS, 0)
case("ctl_settings_datagram", S, fr(M.SETTINGS, vi(0x33) + vi(1) + vi(0x276) + vi(0)), st(M.K_CONTROL, flags=M.S_PEER_DATAGRAMS), CTL_O,
     frames=[(M.SETTINGS, 5, 0)], settings=(0, 0, NONE64, 1))
case("ctl_settings_datagram_draft", C, fr(M.SETTINGS, vi(0x276) + vi(1)), st(M.K_CONTROL, flags=M.S_PEER_DATAGRAMS), CTL_O,
     frames=[(M.SETTINGS, 3, 0)], settings=(0, 0, NONE64, 1))
case("ctl_settings_datagram_0_without_transport", C, fr(M.SETTINGS, vi(0x33) + vi(0)), st(M.K_CONTROL), CTL_O,
     frames=[(M.SETTINGS, 2, 0)], settings=(0, 0, NONE64, 0))
case("ctl_priority_update", S, fr(PU_REQ, vi(4, 2) + b"u=1") + fr(PU_PUSH, vi(3) + b"i"), st(M.K_CONTROL, M.P_OPEN), CTL_O,
     frames=[(PU_REQ, 5, 2), (PU_PUSH, 2, 1)])
case("ctl_priority_update_empty", S, fr(PU_REQ), st(M.K_CONTROL, M.P_OPEN), CTL_O, FR, consumed=0)
# (an id cut short: h2o's 63-bit `element` keeps 2^63 - 1, a server's unidirectional stream, and no err_desc is set)
case("ctl_priority_update_cut", S, fr(PU_REQ, b"\x40"), st(M.K_CONTROL, M.P_OPEN), CTL_O, FR, consumed=0)
case("ctl_priority_update_push_cut", S, fr(PU_PUSH, b"\xc0\x00\x00"), st(M.K_CONTROL, M.P_OPEN), CTL_O, frames=[(PU_PUSH, 3, 1)])
case("ctl_priority_update_of_a_server_stream", S, fr(PU_REQ, vi(5)), st(M.K_CONTROL, M.P_OPEN), CTL_O, FR, consumed=0)
case("ctl_priority_update_of_a_uni_stream", S, fr(PU_REQ, vi(2)), st(M.K_CONTROL, M.P_OPEN), CTL_O, FR, consumed=0)
case("ctl_priority_update_push_of_a_request", S, fr(PU_PUSH, vi(4)), st(M.K_CONTROL, M.P_OPEN), CTL_O, FR, consumed=0)
case("ctl_priority_update_at_the_client", C, fr(PU_REQ, vi(4)), st(M.K_CONTROL, M.P_OPEN), CTL_O, FU, consumed=0)
case("ctl_goaway_at_the_client", C, fr(M.GOAWAY, vi(1 << 20)), st(M.K_CONTROL, M.P_OPEN), CTL_O, frames=[(M.GOAWAY, 4, 4)])
case("ctl_goaway_trailing_byte", C, fr(M.GOAWAY, vi(8) + b"\x00"), st(M.K_CONTROL, M.P_OPEN), CTL_O, FR, M.E_INVALID_GOAWAY, 0)
case("ctl_goaway_empty", C, fr(M.GOAWAY), st(M.K_CONTROL, M.P_OPEN), CTL_O, FR, M.E_INVALID_GOAWAY, 0)
case("ctl_goaway_at_the_server", S, fr(M.GOAWAY, vi(8) + b"\x00"), st(M.K_CONTROL, M.P_OPEN), CTL_O, frames=[(M.GOAWAY, 2, 0)])
# ---- rule 14: frame slots ---------------------------------------------------------------------------------------------
case("s_no_slot_for_headers", S, fr(0x21, b"g") + HDRS, st(), REQ_H, M.FRAMES, consumed=3, frames=[(0x21, 1, 0)], cap=1)
case("s_no_slot_for_body_bytes", S, b"body", st(phase=REQ_P, data_left=9), (M.K_REQUEST, REQ_P, 9), M.FRAMES, consumed=0, cap=0)
case("ctl_no_slot", C, SET, st(M.K_CONTROL), CTL_S, M.FRAMES, consumed=0, cap=0)
case("s_error_wins_over_no_slot", S, fr(M.DATA), st(), REQ_H, FU, consumed=0, cap=0)
case("encoder_needs_no_slot", S, b"\x02abc", st(M.K_UNI), (M.K_QPACK_ENCODER, 0, 0), enc=b"abc", cap=0)
# ---- state records the call does not write ----------------------------------------------------------------------------
for _name, _st in (("kind", st(6)), ("kind_255", st(255)), ("request_phase", st(phase=4)), ("control_phase", st(M.K_CONTROL, 2)),
                   ("phase_on_encoder", st(M.K_QPACK_ENCODER, 1)), ("flag", st(flags=8)), ("reserved", st(rsv=1)),
                   ("data_left_outside_payload", st(phase=M.P_DATA, data_left=1)), ("data_left_on_control", st(M.K_CONTROL, data_left=5)),
                   ("payload_without_data_left", st(phase=REQ_P))):
    case("einval_" + _name, S, HDRS, _st, (_st["kind"], _st["phase"], _st["data_left"]), M.EINVAL, consumed=0)


def connections(flags):
    """the cases of one side as connections: alternately one, three and no streams a connection, plus a connection
    with two encoder streams and two control streams (the first SETTINGS stands)"""
    cs = [c for c in CASES if c["flags"] == flags and c["mfps"] == 16384]
    conns, i, k = [], 0, 0
    while i < len(cs):
        n = (1, 3, 0)[k % 3]
        conns.append([(c["buf"], c["st"], c["cap"]) for c in cs[i:i + n]])
        i, k = i + n, k + 1
    two = [(b"\x02first", st(M.K_UNI, stream_id=2), 0), (b"\x00" + fr(M.SETTINGS, vi(1) + vi(111)), st(M.K_UNI, stream_id=6), 2),
           (HDRS, st(stream_id=0), 2), (b"second", st(M.K_QPACK_ENCODER, stream_id=10), 0),
           (fr(M.SETTINGS, vi(1) + vi(222)), st(M.K_CONTROL, stream_id=14), 2), (fr(M.HEADERS, b"sec2"), st(stream_id=4), 1)]
    return conns + [two]
