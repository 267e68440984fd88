"""Hand-built connections for the DATA framer (include/hhuff.h (2k'')) with literal expectations: every number below was
written out by hand from lib/http2/stream.c, none computed by the model.  A case is one connection:
  m, window, room    the peer's max_frame_size, conn->_write.window, the region's size (capacity - size)
  sends              [(body_off, body_len, stream_id, window, flags, max_frames)]
  frames             the DATA frames expected, in order: [(stream_id, length, flags)]; their payloads are the records'
                     bytes of BODY, in order
  sent               per record served: (sent, nframes, out_off relative to the region, flags, window afterwards)
  out_len, after     the bytes written, conn->_write.window afterwards
  status             0, or EINVAL: the records from len(sent) on are not served"""
M = 16384
F, T = 1, 2                               # HHUFF_H2S_FINAL, _TRAILERS
ES, DONE, SW, ROOM, CW, MAXF = 1, 2, 4, 8, 16, 32   # HHUFF_H2T_*
EINVAL = -314
BIG = 100000
BODY = bytes((i * 131 + (i >> 8) + 7) & 0xFF for i in range(72000))


def case(name, sends, frames, sent, out_len, after, m=M, window=BIG, room=BIG, status=0):
    return dict(name=name, m=m, window=window, room=room, sends=sends, frames=frames, sent=sent, out_len=out_len, after=after,
                status=status)


CASES = [
    # the room: h2o wants a header and more (ret < 9 -> 0; ret - 9 <= 0 -> nothing to send)
    case("room_8", [(0, 1, 1, 100, F, 0)], [], [(0, 0, 0, ROOM, 100)], 0, BIG, room=8),
    case("room_9", [(0, 1, 1, 100, F, 0)], [], [(0, 0, 0, ROOM, 100)], 0, BIG, room=9),
    case("room_10", [(0, 1, 1, 100, F, 0)], [(1, 1, 1)], [(1, 1, 0, DONE | ES, 99)], 10, BIG - 1, room=10),
    case("room_10_two_bytes", [(5, 2, 1, 100, 0, 0)], [(1, 1, 0)], [(1, 1, 0, ROOM, 99)], 10, BIG - 1, room=10),
    case("room_0", [(0, 1, 1, 100, F, 0)], [], [(0, 0, 0, ROOM, 100)], 0, BIG, room=0),
    case("room_cuts_second_frame", [(0, 2 * M, 7, BIG, F, 0)], [(7, M, 0), (7, 5, 0)], [(M + 5, 2, 0, ROOM, BIG - M - 5)],
         2 * 9 + M + 5, BIG - M - 5, room=9 + M + 9 + 5),
    case("room_ends_behind_a_full_frame_and_a_header", [(0, 2 * M, 7, BIG, F, 0)], [(7, M, 0)], [(M, 1, 0, ROOM, BIG - M)],
         9 + M, BIG - M, room=9 + M + 9),
    case("room_9_and_conn_window_0", [(0, 1, 1, 100, F, 0)], [], [(0, 0, 0, ROOM, 100)], 0, 0, window=0, room=9),
    # the stream's window
    case("stream_window_minus_1", [(0, 3, 1, -1, F, 0)], [], [(0, 0, 0, SW, -1)], 0, BIG),
    case("stream_window_0", [(0, 3, 1, 0, F, 0)], [], [(0, 0, 0, SW, 0)], 0, BIG),
    case("stream_window_1", [(0, 3, 1, 1, F, 0)], [(1, 1, 0)], [(1, 1, 0, SW, 0)], 10, BIG - 1),
    case("stream_window_0_wins_over_room_and_conn_window", [(0, 3, 1, 0, F, 0)], [], [(0, 0, 0, SW, 0)], 0, -5, window=-5, room=3),
    # the connection's window
    case("conn_window_minus_1", [(0, 3, 1, 50, F, 0)], [], [(0, 0, 0, CW, 50)], 0, -1, window=-1),
    case("conn_window_0", [(0, 3, 1, 50, F, 0)], [], [(0, 0, 0, CW, 50)], 0, 0, window=0),
    case("conn_window_1", [(0, 3, 1, 50, F, 0)], [(1, 1, 0)], [(1, 1, 0, CW, 49)], 10, 0, window=1),
    case("conn_window_mid_frame", [(0, M, 1, 65535, 0, 0), (M, M, 3, 65535, F, 0)], [(1, M, 0), (3, 3616, 0)],
         [(M, 1, 0, DONE, 65535 - M), (3616, 1, M + 9, CW, 65535 - 3616)], M + 9 + 3616 + 9, 0, window=20000),
    # the length of the body against m
    case("empty_in_progress", [(0, 0, 1, 50, 0, 0)], [], [(0, 0, 0, DONE, 50)], 0, BIG),
    case("empty_final", [(0, 0, 1, 50, F, 0)], [(1, 0, 1)], [(0, 1, 0, DONE | ES, 50)], 9, BIG),
    case("empty_final_with_trailers", [(0, 0, 1, 50, F | T, 0)], [], [(0, 0, 0, DONE, 50)], 0, BIG),
    case("empty_final_stream_window_0", [(0, 0, 1, 0, F, 0)], [], [(0, 0, 0, SW, 0)], 0, BIG),
    case("empty_final_room_9", [(0, 0, 1, 50, F, 0)], [], [(0, 0, 0, ROOM, 50)], 0, BIG, room=9),
    case("empty_final_room_10", [(0, 0, 1, 50, F, 0)], [(1, 0, 1)], [(0, 1, 0, DONE | ES, 50)], 9, BIG, room=10),
    case("empty_final_conn_window_0", [(0, 0, 1, 50, F, 0)], [], [(0, 0, 0, CW, 50)], 0, 0, window=0),
    case("one_byte", [(9, 1, 1, BIG, F, 0)], [(1, 1, 1)], [(1, 1, 0, DONE | ES, BIG - 1)], 10, BIG - 1),
    case("m_minus_1", [(1, M - 1, 1, BIG, F, 0)], [(1, M - 1, 1)], [(M - 1, 1, 0, DONE | ES, BIG - M + 1)], M + 8, BIG - M + 1),
    case("m", [(2, M, 1, BIG, F, 0)], [(1, M, 1)], [(M, 1, 0, DONE | ES, BIG - M)], M + 9, BIG - M),
    case("m_plus_1", [(3, M + 1, 1, BIG, F, 0)], [(1, M, 0), (1, 1, 1)], [(M + 1, 2, 0, DONE | ES, BIG - M - 1)], M + 19, BIG - M - 1),
    case("two_m", [(4, 2 * M, 1, BIG, F, 0)], [(1, M, 0), (1, M, 1)], [(2 * M, 2, 0, DONE | ES, BIG - 2 * M)], 2 * M + 18, BIG - 2 * M),
    case("two_m_in_progress", [(4, 2 * M, 1, BIG, 0, 0)], [(1, M, 0), (1, M, 0)], [(2 * M, 2, 0, DONE, BIG - 2 * M)], 2 * M + 18,
         BIG - 2 * M),
    case("two_m_with_trailers", [(4, 2 * M, 1, BIG, F | T, 0)], [(1, M, 0), (1, M, 0)], [(2 * M, 2, 0, DONE, BIG - 2 * M)], 2 * M + 18,
         BIG - 2 * M),
    # the peer's MAX_FRAME_SIZE
    case("m_32768", [(0, 32769, 5, BIG, F, 0)], [(5, 32768, 0), (5, 1, 1)], [(32769, 2, 0, DONE | ES, BIG - 32769)], 32769 + 18,
         BIG - 32769, m=32768),
    case("m_largest_length_over_16_bits", [(100, 70000, 0x7FFFFFFF, BIG, F, 0)], [(0x7FFFFFFF, 70000, 1)],
         [(70000, 1, 0, DONE | ES, 30000)], 70009, 30000, m=16777215),
    # max_frames: at most k calls of send_pending_data
    case("max_frames_1", [(0, 2 * M + 1, 1, BIG, F, 1)], [(1, M, 0)], [(M, 1, 0, MAXF, BIG - M)], M + 9, BIG - M),
    case("max_frames_2", [(0, 2 * M + 1, 1, BIG, F, 2)], [(1, M, 0), (1, M, 0)], [(2 * M, 2, 0, MAXF, BIG - 2 * M)], 2 * M + 18,
         BIG - 2 * M),
    case("max_frames_3", [(0, 2 * M + 1, 1, BIG, F, 3)], [(1, M, 0), (1, M, 0), (1, 1, 1)],
         [(2 * M + 1, 3, 0, DONE | ES, BIG - 2 * M - 1)], 2 * M + 28, BIG - 2 * M - 1),
    case("max_frames_1_takes_the_short_frame", [(0, 7, 1, BIG, F, 1)], [(1, 7, 1)], [(7, 1, 0, DONE | ES, BIG - 7)], 16, BIG - 7),
    case("interleaved_visits", [(0, 20000, 1, BIG, F, 1), (20000, 5, 3, BIG, F, 1), (M, 20000 - M, 1, BIG - M, F, 1)],
         [(1, M, 0), (3, 5, 1), (1, 20000 - M, 1)],
         [(M, 1, 0, MAXF, BIG - M), (5, 1, M + 9, DONE | ES, BIG - 5), (20000 - M, 1, M + 9 + 14, DONE | ES, BIG - 20000)],
         20005 + 27, BIG - 20005),
    # records without a frame between records with frames; the room carries over
    case("blocked_stream_between", [(0, 1, 1, 10, F, 0), (1, 4, 3, 0, F, 0), (5, 2, 5, 10, 0, 0), (0, 0, 7, 10, 0, 0), (7, 1, 9, 10, F, 0)],
         [(1, 1, 1), (5, 2, 0), (9, 1, 1)],
         [(1, 1, 0, DONE | ES, 9), (0, 0, 10, SW, 0), (2, 1, 10, DONE, 8), (0, 0, 21, DONE, 10), (1, 1, 21, DONE | ES, 9)], 31, BIG - 4),
    case("room_runs_out_over_records", [(0, 3, 1, 10, F, 0), (3, 3, 3, 10, F, 0), (6, 3, 5, 10, F, 0)], [(1, 3, 1), (3, 2, 0)],
         [(3, 1, 0, DONE | ES, 7), (2, 1, 12, ROOM, 8), (0, 0, 23, ROOM, 10)], 23, BIG - 5, room=23),
    case("no_records", [], [], [], 0, BIG),
    # what stops a connection with EINVAL: the earlier records stay
    case("stream_id_0", [(0, 1, 1, 10, 0, 0), (1, 1, 0, 10, 0, 0), (2, 1, 3, 10, 0, 0)], [(1, 1, 0)], [(1, 1, 0, DONE, 9)], 10, BIG - 1,
         status=EINVAL),
    case("stream_id_2_31", [(1, 1, 0x80000000, 10, 0, 0)], [], [], 0, BIG, status=EINVAL),
    case("unknown_flag", [(1, 1, 1, 10, 4, 0)], [], [], 0, BIG, status=EINVAL),
    case("body_range_one_past", [(0, 2, 1, 10, 0, 0), (71999, 2, 3, 10, 0, 0)], [(1, 2, 0)], [(2, 1, 0, DONE, 8)], 11, BIG - 2,
         status=EINVAL),
    case("body_range_wraps", [(0xFFFFFFFF, 2, 1, 10, 0, 0)], [], [], 0, BIG, status=EINVAL),
    case("body_range_to_the_end", [(71998, 2, 1, 10, F, 0)], [(1, 2, 1)], [(2, 1, 0, DONE | ES, 8)], 11, BIG - 2),
    case("peer_frame_size_16383", [(0, 1, 1, 10, 0, 0)], [], [], 0, BIG, m=16383, status=EINVAL),
    case("peer_frame_size_2_24", [(0, 1, 1, 10, 0, 0)], [], [], 0, BIG, m=16777216, status=EINVAL),
]
