"""A plain model of HTTP/2 control-frame handling (include/hhuff.h (2k')), written from h2o's own lines --
lib/http2/frame.c:37-66 (h2o_http2_update_peer_settings), 68-122 (the reply layouts), 152-177, 226-310 (the payload
decoders), include/h2o/http2_common.h:234-241 (h2o_http2_window_update), lib/http2/connection.c:976-989, 1097-1108,
1151-1261 and lib/common/http2client.c:662-871 (the handlers) -- not from h2o_amd/csrc/hhuff_h2ctl.h.

  decode_*_payload(length, flags, sid, pay, defects)   one h2o decoder each: (ret, err, out-parameters ...)
  update_peer_settings(settings, pay, defects)         (ret, err, pairs), `settings` (a list of five) changed in place
  walk(frames, peer, client, recv_window_size, rep_cap, defects) -> dict
      frames   [(type, flags, stream_id, payload bytes, payload_off)]
      peer     new_peer(), changed in place
      records  [(a, b, status, err, flags, reply_len)]; nctl, status, err, replies (bytes)
  batch(conns, caps, ...)   what hhuff_h2_control writes for these connections (numpy), via frames_model.batch

defects  names of DEFECTS: each makes the model wrong in one way; the corpus has to tell every one of them apart"""
DATA, HEADERS, PRIORITY, RST_STREAM, SETTINGS, PUSH_PROMISE, PING, GOAWAY, WINDOW_UPDATE, CONTINUATION = range(10)
F_ACK, F_PADDED = 0x1, 0x8
PROTOCOL, FLOW_CONTROL, FRAME_SIZE = -1, -3, -6
SPACE, EINVAL = -312, -313  # HHUFF_H2C_SPACE, HHUFF_H2C_EINVAL
CLIENT = 1
P_SETTINGS, P_GOAWAY = 1, 2
R_ACK, R_NEEDS_STREAM, R_STREAM_ERROR, R_WINDOW_DELTA, R_WINDOW_UPDATE = 1, 2, 4, 8, 16
(E_NONE, E_DATA_STREAM_ID, E_DATA_FRAME, E_PRIORITY_STREAM_ID, E_PRIORITY_FRAME, E_SELF_DEPENDENCY, E_RST_STREAM_STREAM_ID,
 E_RST_STREAM_FRAME, E_SETTINGS_STREAM_ID, E_SETTINGS_ACK, E_SETTINGS_FRAME, E_SETTINGS_SIZE, E_PING_FRAME, E_GOAWAY_STREAM_ID,
 E_GOAWAY_FRAME, E_WINDOW_UPDATE_FRAME, E_FLOW_CONTROL) = range(17)
ALL_STATUS = (0, PROTOCOL, FLOW_CONTROL, FRAME_SIZE, SPACE, EINVAL)
ALL_ERR = tuple(range(17))
ALL_FLAGS = (R_ACK, R_NEEDS_STREAM, R_STREAM_ERROR, R_WINDOW_DELTA, R_WINDOW_UPDATE)
INT32_MAX = 0x7fffffff
# h2o's err_desc texts, by HHUFF_H2C_ERR_* (None: h2o sets none)
ERR_TEXT = (None, "invalid stream id in DATA frame", "invalid DATA frame", "invalid stream id in PRIORITY frame",
            "invalid PRIORITY frame", "stream cannot depend on itself", "invalid stream id in RST_STREAM frame",
            "invalid RST_STREAM frame", "invalid stream id in SETTINGS frame", "invalid SETTINGS frame (+ACK)",
            "invalid SETTINGS frame", None, "invalid PING frame", "invalid stream id in GOAWAY frame", "invalid GOAWAY frame",
            "invalid WINDOW_UPDATE frame", "flow control window overflow")

DEFECTS = (
    "size_before_stream_id",   # a fixed-size frame's length tested before its stream id
    "reserved_bit_kept",       # the reserved bit of an increment / a last stream id / a dependency not masked
    "overflow_off_by_one",     # a send window landing exactly on INT32_MAX refused
    "settings_rollback",       # a SETTINGS error rolls the frame's earlier pairs back
    "ack_answered",            # SETTINGS and PING with ACK answered as well
    "window_update_lt",        # the connection WINDOW_UPDATE sent at < half, not <=
    "replies_behind_failure",  # the frames behind the failure still answered
    "client_as_server",        # the client's receive window consumed like the server's
    "pad_eq_ok",               # DATA with pad == length accepted
    "weight_raw",              # weight = the byte, not the byte + 1
    "goaway_8_refused",        # a GOAWAY of exactly 8 bytes refused
    "unknown_setting_error",   # an unknown SETTINGS identifier refused
    "first_setting_wins",      # the first of a repeated identifier kept
    "settings_partial_pair_ok",  # trailing bytes of a SETTINGS frame ignored
    "zero_increment_stream_fatal",  # a zero increment on a stream ends the connection
    "delta_unsigned",          # the initial window's change not taken as int32
    "padding_not_consumed",    # the receive window charged the data without the padding
    "unknown_type_error",      # frame types from 10 on refused
    "space_half_applied",      # a frame whose reply does not fit still changes the state
)


def new_peer():
    """HHUFF_H2_PEER_INIT"""
    return dict(settings=[4096, 1, 0xFFFFFFFF, 65535, 16384], flags=0, send_window=65535, recv_window=65535)


def be32(b, at=0):
    return int.from_bytes(b[at:at + 4], "big")


def decode_data_payload(length, flags, sid, pay, defects=()):
    """frame.c:152-177: (ret, err, data offset in the payload, data length)"""
    if sid == 0:
        return PROTOCOL, E_DATA_STREAM_ID, 0, 0
    if flags & F_PADDED:
        if length < 1:
            return PROTOCOL, E_DATA_FRAME, 0, 0
        pad = pay[0]
        if length < 1 + pad and not ("pad_eq_ok" in defects and length == pad):
            return PROTOCOL, E_DATA_FRAME, 0, 0
        return 0, E_NONE, 1, max(0, length - (1 + pad))
    return 0, E_NONE, 0, length


def _fixed(length, want, sid, sid_bad, e_sid, e_size, defects):
    """the two opening tests of a fixed-size frame, in h2o's order (the defect swaps them)"""
    tests = [(sid_bad(sid), PROTOCOL, e_sid), (not want(length), FRAME_SIZE, e_size)]
    if "size_before_stream_id" in defects:
        tests.reverse()
    for bad, ret, err in tests:
        if bad:
            return ret, err
    return 0, E_NONE


def decode_priority_payload(length, flags, sid, pay, defects=()):
    """frame.c:226-239: (ret, err, exclusive, dependency, weight)"""
    ret, err = _fixed(length, lambda n: n == 5, sid, lambda s: s == 0, E_PRIORITY_STREAM_ID, E_PRIORITY_FRAME, defects)
    if ret:
        return ret, err, 0, 0, 0
    u4 = be32(pay)
    dep = u4 if "reserved_bit_kept" in defects else u4 & INT32_MAX
    return 0, E_NONE, u4 >> 31, dep, pay[4] + (0 if "weight_raw" in defects else 1)


def decode_rst_stream_payload(length, flags, sid, pay, defects=()):
    """frame.c:241-255: (ret, err, error_code)"""
    ret, err = _fixed(length, lambda n: n == 4, sid, lambda s: s == 0, E_RST_STREAM_STREAM_ID, E_RST_STREAM_FRAME, defects)
    return (ret, err, 0) if ret else (0, E_NONE, be32(pay))


def decode_ping_payload(length, flags, sid, pay, defects=()):
    """frame.c:257-270: (ret, err, the 8 bytes)"""
    ret, err = _fixed(length, lambda n: n == 8, sid, lambda s: s != 0, E_PING_FRAME, E_PING_FRAME, defects)
    return (ret, err, b"") if ret else (0, E_NONE, bytes(pay[:8]))


def decode_goaway_payload(length, flags, sid, pay, defects=()):
    """frame.c:272-291: (ret, err, last_stream_id, error_code, debug data length)"""
    ok = (lambda n: n > 8) if "goaway_8_refused" in defects else (lambda n: n >= 8)
    ret, err = _fixed(length, ok, sid, lambda s: s != 0, E_GOAWAY_STREAM_ID, E_GOAWAY_FRAME, defects)
    if ret:
        return ret, err, 0, 0, 0
    last = be32(pay)
    return 0, E_NONE, last if "reserved_bit_kept" in defects else last & INT32_MAX, be32(pay, 4), length - 8


def decode_window_update_payload(length, flags, sid, pay, defects=()):
    """frame.c:293-310: (ret, err, increment, err_is_stream_level)"""
    if length != 4:
        return FRAME_SIZE, E_WINDOW_UPDATE_FRAME, 0, 0
    inc = be32(pay)
    if "reserved_bit_kept" not in defects:
        inc &= INT32_MAX
    if inc == 0:
        return PROTOCOL, E_WINDOW_UPDATE_FRAME, 0, int(sid != 0)
    return 0, E_NONE, inc, 0


def update_peer_settings(settings, pay, defects=()):
    """frame.c:37-66 on settings = [header_table_size, enable_push, max_concurrent_streams, initial_window_size,
    max_frame_size]: (ret, err, pairs read without error)"""
    limits = {1: (0, 0xFFFFFFFF, 0), 2: (0, 1, PROTOCOL), 3: (0, 0xFFFFFFFF, 0), 4: (0, INT32_MAX, FLOW_CONTROL),
              5: (16384, 16777215, PROTOCOL)}
    before, seen, pairs, n = list(settings), set(), 0, len(pay)
    at = 0
    while n - at >= 6:
        ident, value = int.from_bytes(pay[at:at + 2], "big"), be32(pay, at + 2)
        if ident in limits:
            lo, hi, code = limits[ident]
            if not lo <= value <= hi:
                if "settings_rollback" in defects:
                    settings[:] = before
                return code, E_SETTINGS_FRAME, pairs
            if not ("first_setting_wins" in defects and ident in seen):
                settings[ident - 1] = value
            seen.add(ident)
        elif "unknown_setting_error" in defects:
            return PROTOCOL, E_SETTINGS_FRAME, pairs
        at += 6
        pairs += 1
    if n - at != 0 and "settings_partial_pair_ok" not in defects:
        if "settings_rollback" in defects:
            settings[:] = before
        return FRAME_SIZE, E_SETTINGS_SIZE, pairs
    return 0, E_NONE, pairs


def frame_header(length, typ, flags, sid):
    """h2o_http2_encode_frame_header, frame.c:68-79"""
    return length.to_bytes(3, "big") + bytes([typ, flags]) + (sid & 0xFFFFFFFF).to_bytes(4, "big")


def handle(typ, flags, sid, pay, payload_off, peer, client=False, recv_window_size=0, defects=()):
    """one frame's handler on `peer` (changed in place): (ret, record (a, b, status, err, flags), reply bytes)"""
    length = len(pay)
    if typ == DATA:  # connection.c:976-989
        ret, err, off, n = decode_data_payload(length, flags, sid, pay, defects)
        if ret:
            return ret, (0, 0, ret, err, 0), b""
        rf, reply = R_NEEDS_STREAM, b""
        if recv_window_size and (not client or "client_as_server" in defects):
            peer["recv_window"] -= n if "padding_not_consumed" in defects else length
            half = recv_window_size // 2
            if peer["recv_window"] < half or (peer["recv_window"] == half and "window_update_lt" not in defects):
                inc = (recv_window_size - peer["recv_window"]) & 0xFFFFFFFF
                reply = frame_header(4, WINDOW_UPDATE, 0, 0) + inc.to_bytes(4, "big")  # frame.c:118-122
                peer["recv_window"] = recv_window_size
                rf |= R_WINDOW_UPDATE
        return 0, (payload_off + off, n, 0, E_NONE, rf), reply
    if typ == PRIORITY:  # connection.c:1097-1108, http2client.c:662-676
        ret, err, excl, dep, weight = decode_priority_payload(length, flags, sid, pay, defects)
        if ret == 0 and dep == sid:
            ret, err = PROTOCOL, E_SELF_DEPENDENCY
        if ret:
            return ret, (0, 0, ret, err, 0), b""
        return 0, ((excl << 31 | dep) & 0xFFFFFFFF, weight, 0, E_NONE, R_NEEDS_STREAM), b""
    if typ == RST_STREAM:
        ret, err, code = decode_rst_stream_payload(length, flags, sid, pay, defects)
        return ret, (code, 0, ret, err, 0 if ret else R_NEEDS_STREAM), b""
    if typ == SETTINGS:  # connection.c:1151-1187
        if sid != 0:
            return PROTOCOL, (0, 0, PROTOCOL, E_SETTINGS_STREAM_ID, 0), b""
        if flags & F_ACK:
            if length != 0:
                return FRAME_SIZE, (0, 0, FRAME_SIZE, E_SETTINGS_ACK, 0), b""
            return 0, (0, 0, 0, E_NONE, R_ACK), frame_header(0, SETTINGS, F_ACK, 0) if "ack_answered" in defects else b""
        prev = peer["settings"][3]
        ret, err, pairs = update_peer_settings(peer["settings"], pay, defects)
        if ret:
            return ret, (pairs, 0, ret, err, 0), b""
        delta = peer["settings"][3] - prev  # both below 2^31: the int32 difference
        if "delta_unsigned" in defects:
            delta = abs(delta)
        peer["flags"] |= P_SETTINGS
        return 0, (pairs, delta & 0xFFFFFFFF, 0, E_NONE, R_WINDOW_DELTA if delta else 0), frame_header(0, SETTINGS, F_ACK, 0)
    if typ == PING:  # connection.c:1247-1261, frame.c:94-99
        ret, err, data = decode_ping_payload(length, flags, sid, pay, defects)
        if ret:
            return ret, (0, 0, ret, err, 0), b""
        answer = not flags & F_ACK or "ack_answered" in defects
        return 0, (be32(data), be32(data, 4), 0, E_NONE, R_ACK if flags & F_ACK else 0), \
            frame_header(8, PING, F_ACK, 0) + data if answer else b""
    if typ == GOAWAY:  # connection.c:1233-1245
        ret, err, last, code, _ = decode_goaway_payload(length, flags, sid, pay, defects)
        if ret:
            return ret, (0, 0, ret, err, 0), b""
        peer["flags"] |= P_GOAWAY
        return 0, (last, code, 0, E_NONE, 0), b""
    if typ == WINDOW_UPDATE:  # connection.c:1189-1231
        ret, err, inc, stream_level = decode_window_update_payload(length, flags, sid, pay, defects)
        if ret:
            if stream_level and "zero_increment_stream_fatal" not in defects:  # stream_send_error(conn, stream_id, ret)
                return 0, (0, 0, ret, err, R_STREAM_ERROR | R_NEEDS_STREAM), frame_header(4, RST_STREAM, 0, sid) + (-ret).to_bytes(4, "big")
            return ret, (0, 0, ret, err, 0), b""
        if sid == 0:
            v = peer["send_window"] + inc  # http2_common.h:234-241
            if v > INT32_MAX or ("overflow_off_by_one" in defects and v == INT32_MAX):
                return FLOW_CONTROL, (0, 0, FLOW_CONTROL, E_FLOW_CONTROL, 0), b""
            peer["send_window"] = v
            return 0, (inc & 0xFFFFFFFF, 0, 0, E_NONE, 0), b""
        return 0, (inc & 0xFFFFFFFF, 0, 0, E_NONE, R_NEEDS_STREAM), b""
    if typ >= 10 and "unknown_type_error" in defects:
        return PROTOCOL, (0, 0, PROTOCOL, E_NONE, 0), b""
    return 0, (0, 0, 0, E_NONE, 0), b""  # header frames are the de-framer's; expect_default ignores types >= 10


def copy_peer(p):
    return dict(settings=list(p["settings"]), flags=p["flags"], send_window=p["send_window"], recv_window=p["recv_window"])


def walk(frames, peer, client=False, recv_window_size=0, rep_cap=1 << 30, in_size=None, defects=()):
    """one connection: frames [(type, flags, stream_id, payload, payload_off)] in wire order against `peer` (changed in
    place).  in_size: a frame with payload_off + len(payload) above it is a hostile record (EINVAL)."""
    out = dict(records=[], nctl=0, status=0, err=E_NONE, replies=b"")
    for k, (typ, flags, sid, pay, off) in enumerate(frames):
        if in_size is not None and off + len(pay) > in_size:
            out["status"] = EINVAL
            return out
        trial = copy_peer(peer)
        ret, rec, reply = handle(typ, flags, sid, pay, off, trial, client, recv_window_size, defects)
        if ret:
            peer.update(trial)
            out["records"].append(rec + (0,))
            out["status"], out["err"] = ret, rec[3]
            if "replies_behind_failure" in defects:
                rest = walk(frames[k + 1:], copy_peer(peer), client, recv_window_size, rep_cap - len(out["replies"]), in_size,
                            tuple(d for d in defects if d != "replies_behind_failure"))
                out["replies"] += rest["replies"]
            return out
        if len(reply) > rep_cap - len(out["replies"]):
            if "space_half_applied" in defects:
                peer.update(trial)
            out["status"] = SPACE
            return out
        peer.update(trial)
        out["replies"] += reply
        out["records"].append(rec + (len(reply),))
        out["nctl"] += 1
    return out


def split_frames(buf, base=0):
    """a connection's listed frames by the length fields alone: [(type, flags, stream_id, payload, payload_off)]"""
    out, pos = [], 0
    while len(buf) - pos >= 9:
        n = int.from_bytes(buf[pos:pos + 3], "big")
        if len(buf) - pos < 9 + n:
            break
        out.append((buf[pos + 3], buf[pos + 4], be32(buf, pos + 5) & INT32_MAX, bytes(buf[pos + 9:pos + 9 + n]), base + pos + 9))
        pos += 9 + n
    return out


def peers_array(peers):
    import numpy as np

    from h2o_amd import codec

    a = np.zeros(len(peers), codec.H2_PEER_DTYPE)
    for i, p in enumerate(peers):
        a[i] = tuple(p["settings"]) + (p["flags"], p["send_window"], p["recv_window"])
    return a


def peers_list(arr):
    return [dict(settings=[int(r[k]) for k in ("header_table_size", "enable_push", "max_concurrent_streams",
                                                "initial_window_size", "max_frame_size")],
                 flags=int(r["flags"]), send_window=int(r["send_window"]), recv_window=int(r["recv_window"])) for r in arr]


def batch(conns, caps, peers=None, client=False, recv_window_size=0, rep_caps=None):
    """What hhuff_h2_deframe and then hhuff_h2_control write for the connections `conns` (bytes each) with caps[c] frame
    slots, from the states `peers` (default: new connections): the de-framer's dict (frames_model.batch) plus ctl,
    ctl_used (bool per slot), nctl, ctl_status, ctl_err, rep_off, rep_len, rep (the regions back to back, rep_caps[c]
    bytes each; default the bound) and peers_out (H2_PEER_DTYPE)."""
    import numpy as np

    import frames_model
    from h2o_amd import codec

    r = frames_model.batch(conns, caps)
    nconn = len(conns)
    peers = [new_peer() for _ in conns] if peers is None else [copy_peer(p) for p in peers]
    rep_caps = [17 * int(c) for c in caps] if rep_caps is None else rep_caps
    rep_off = np.zeros(nconn + 1, np.uint32)
    rep_off[1:] = np.cumsum(rep_caps, dtype=np.uint64)
    rep = np.zeros(int(rep_off[-1]), np.uint8)
    rep_used = np.zeros(int(rep_off[-1]), bool)
    ctl = np.zeros(r["frm_cap"], codec.H2_CTL_DTYPE)
    used = np.zeros(r["frm_cap"], bool)
    nctl, cerr, rep_len = (np.zeros(nconn, np.uint32) for _ in range(3))
    cstatus = np.zeros(nconn, np.int32)
    data = r["data"]
    for c in range(nconn):
        f0 = int(r["frm_first"][c])
        fl = []
        for f in r["frames"][f0:f0 + int(r["nframes"][c])]:
            off, n = int(f["payload_off"]), int(f["length"])
            fl.append((int(f["type"]), int(f["flags"]), int(f["stream_id"]), bytes(data[off:off + n]), off))
        w = walk(fl, peers[c], client, recv_window_size, int(rep_caps[c]))
        for i, rec in enumerate(w["records"]):
            ctl[f0 + i] = rec
            used[f0 + i] = True
        nctl[c], cstatus[c], cerr[c], rep_len[c] = w["nctl"], w["status"], w["err"], len(w["replies"])
        o = int(rep_off[c])
        rep[o:o + len(w["replies"])] = np.frombuffer(w["replies"], np.uint8)
        rep_used[o:o + len(w["replies"])] = True
    r.update(ctl=ctl, ctl_used=used, nctl=nctl, ctl_status=cstatus, ctl_err=cerr, rep_off=rep_off, rep_len=rep_len, rep=rep,
             rep_used=rep_used, peers_out=peers_array(peers), peers_out_list=peers)
    return r
