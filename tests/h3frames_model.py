"""A plain-Python model of the HTTP/3 de-framer (include/hhuff.h (2l)), written from h2o's lines and independent of
h2o_amd/csrc/hhuff_h3frames.h: one function per h2o function -- quicint (ptls_decode_quicint), read_frame
(lib/http3/common.c:1057-1145), the server's request handlers (lib/http3/server.c:1367-1453, 1499-1536), the client's
(lib/common/http3client.c:438-540), the unidirectional streams (common.c:365-439), handle_settings_frame
(common.c:1422-1473), decode_priority_update_frame and decode_goaway_frame (lib/http3/frame.c:40-98) -- driven per
stream by walk(), which loops as h2o's handle_buffered_input loops over a stream's handler.  batch() places sections
and encoder bytes of many streams and connections as the call documents it.

DEFECTS: switchable deviations from h2o, at least one per numbered rule of (2l); the corpus (h3frames_corpora.py) must
tell each of them from the model proper."""
import numpy as np

DATA, HEADERS, CANCEL_PUSH, SETTINGS, PUSH_PROMISE, GOAWAY, MAX_PUSH_ID = 0, 1, 3, 4, 5, 7, 13
PRIORITY_UPDATE_REQUEST, PRIORITY_UPDATE_PUSH = 0xF0700, 0xF0701
INCOMPLETE = -1
GENERAL_PROTOCOL, FRAME_UNEXPECTED, FRAME, EXCESSIVE_LOAD, MISSING_SETTINGS = 0x30101, 0x30105, 0x30106, 0x30107, 0x3010a
REJECTED, FRAMES, EINVAL = -320, -321, -322
ALL_STATUS = (0, GENERAL_PROTOCOL, FRAME_UNEXPECTED, FRAME, EXCESSIVE_LOAD, REJECTED, FRAMES, EINVAL)
(E_NONE, E_FRAME_TOO_LARGE, E_UNEXPECTED_TYPE, E_DATA_BEFORE_HEADERS, E_RESPONSE_TOO_LARGE, E_MALFORMED_SETTINGS,
 E_INVALID_PRIORITY, E_INVALID_GOAWAY) = ALL_ERR = tuple(range(8))
K_REQUEST, K_UNI, K_CONTROL, K_QPACK_ENCODER, K_QPACK_DECODER, K_DISCARD = ALL_KINDS = tuple(range(6))
P_HEADERS, P_DATA, P_DATA_PAYLOAD, P_POST_TRAILERS = range(4)
P_SETTINGS, P_OPEN = 0, 1
S_WALK_ON, S_TUNNEL, S_PEER_DATAGRAMS = ALL_STATE_FLAGS = (1, 2, 4)
CLIENT = 1
NOSEC = 0xFFFFFFFF
NONE64 = (1 << 64) - 1

DEFECTS = ("too_large_after_complete", "table_before_complete", "minimal_varints_only",  # rule 1
           "rejected_for_any_type",          # rule 2: every too-large frame in _HEADERS resets the stream
           "no_stop_behind_section",         # rule 3: walks on without HHUFF_H3S_WALK_ON
           "trailers_as_section",            # rule 4
           "tunnel_ignored",                 # rule 4 / 7
           "post_trailers_takes_data",       # rule 5
           "client_error_as_is",             # rule 6: the EXCESSIVE_LOAD mapping dropped
           "client_post_trailers",           # rule 7: the client gets the server's post-trailers phase
           "uni_waits_behind_type",          # rule 8: the new kind starts with the next call
           "push_stream_is_control",         # rule 8: type 1 taken for 0
           "encoder_bytes_kept",             # rule 9
           "decoder_bytes_consumed",         # rule 10
           "discard_keeps",                  # rule 11
           "settings_order",                 # rule 12: MISSING_SETTINGS before the has_received_settings test
           "setting_first_value",            # rule 13
           "datagram_without_transport_ok",  # rule 13
           "goaway_trailing_bytes_ok",       # rule 13
           "priority_kind_unchecked",        # rule 13
           "frame_slots_unlimited")          # rule 14


def quicint(b, pos, end, defects=()):
    """ptls_decode_quicint: -> (value, new pos), value None when cut short"""
    if pos == end:
        return None, pos
    first = b[pos]
    n = 1 << (first >> 6)
    if end - pos < n:
        return None, pos
    v = first & 0x3F
    for i in range(1, n):
        v = (v << 8) | b[pos + i]
    if "minimal_varints_only" in defects and n > 1 and v < (1 << {2: 6, 4: 14, 8: 30}[n]):
        return None, pos
    return v, pos + n


# the table of common.c:1124-1132: type -> (req client, req server, ctl client, ctl server), the column naming the
# SENDER: a frame is accepted from a client when we are the server
TABLE = {DATA: (1, 1, 0, 0), HEADERS: (1, 1, 0, 0), CANCEL_PUSH: (0, 0, 1, 1), SETTINGS: (0, 0, 1, 1),
         PUSH_PROMISE: (0, 1, 0, 0), GOAWAY: (0, 0, 1, 1), MAX_PUSH_ID: (0, 0, 1, 0), PRIORITY_UPDATE_REQUEST: (0, 0, 1, 0),
         PRIORITY_UPDATE_PUSH: (0, 0, 1, 0)}


def table_ok(typ, is_client, control):
    if typ not in TABLE:
        return True
    req_clnt, req_srvr, ctl_clnt, ctl_srvr = TABLE[typ]
    clnt, srvr = (ctl_clnt, ctl_srvr) if control else (req_clnt, req_srvr)
    return bool((clnt and not is_client) or (srvr and is_client))


def read_frame(b, pos, end, mfps, is_client, control, defects=()):
    """h2o_http3_read_frame: -> (ret, err, type, length, header size, new pos)"""
    typ, p = quicint(b, pos, end, defects)
    if typ is None:
        return INCOMPLETE, E_NONE, None, 0, 0, pos
    length, p = quicint(b, p, end, defects)
    if length is None:
        return INCOMPLETE, E_NONE, typ, 0, 0, pos
    hdr = p - pos
    if "table_before_complete" in defects and not table_ok(typ, is_client, control):
        return FRAME_UNEXPECTED, E_NONE, typ, length, hdr, pos
    if typ != DATA:
        if "too_large_after_complete" in defects:
            if end - p < length:
                return INCOMPLETE, E_NONE, typ, length, hdr, pos
            if length > mfps:
                return GENERAL_PROTOCOL, E_FRAME_TOO_LARGE, typ, length, hdr, pos
        else:
            if length > mfps:
                return GENERAL_PROTOCOL, E_FRAME_TOO_LARGE, typ, length, hdr, pos
            if end - p < length:
                return INCOMPLETE, E_NONE, typ, length, hdr, pos
        p += length
    if not table_ok(typ, is_client, control):
        return FRAME_UNEXPECTED, E_NONE, typ, length, hdr, pos
    return 0, E_NONE, typ, length, hdr, p


def handle_settings_frame(payload, peer_datagrams, defects=()):
    """h2o_http3_handle_settings_frame: -> (ret, dict)"""
    s = dict(max_field_section_size=NONE64, max_table_capacity=0, max_blocked=0, h3_datagram=0)
    seen = set()
    pos, end = 0, len(payload)
    while pos != end:
        ident, pos = quicint(payload, pos, end)
        if ident is None:
            return FRAME, None
        value, pos = quicint(payload, pos, end)
        if value is None:
            return FRAME, None
        if "setting_first_value" in defects and ident in seen:
            continue
        seen.add(ident)
        if ident == 6:
            s["max_field_section_size"] = value
        elif ident == 1:
            s["max_table_capacity"] = value
        elif ident == 7:
            s["max_blocked"] = value
        elif ident in (0x33, 0x276):
            if value == 0:
                pass
            elif value == 1:
                if not peer_datagrams and "datagram_without_transport_ok" not in defects:
                    return FRAME, None
                s["h3_datagram"] = 1
            else:
                return FRAME, None
    return 0, s


def decode_priority_update_frame(payload, is_push, defects=()):
    """-> (ret, err, id bytes).  frame->element is a 63-bit field: `(frame->element = quicly_decodev(..)) == UINT64_MAX`
    (frame.c:49) compares the truncated value, is never true, and a cut id goes on as 2^63 - 1 with *src behind the one
    byte ptls_decode_quicint took; E_INVALID_PRIORITY is never returned."""
    if len(payload) == 0:
        return FRAME, E_NONE, 0
    element, pos = quicint(payload, 0, len(payload))
    if element is None:
        element, pos = (1 << 63) - 1, 1
    client_initiated, uni = (element & 1) == 0, (element & 2) != 0
    if "priority_kind_unchecked" not in defects:
        if is_push:
            if not (not client_initiated and uni):
                return FRAME, E_NONE, 0
        elif not (client_initiated and not uni):
            return FRAME, E_NONE, 0
    return 0, E_NONE, pos


def decode_goaway_frame(payload, defects=()):
    ident, pos = quicint(payload, 0, len(payload))
    if ident is None or (pos != len(payload) and "goaway_trailing_bytes_ok" not in defects):
        return FRAME, E_INVALID_GOAWAY, 0
    return 0, E_NONE, pos


def state_valid(st, is_client):
    kind, phase, flags, data_left = st["kind"], st["phase"], st["flags"], st["data_left"]
    if flags & ~7 or st.get("rsv", 0):
        return False
    if kind == K_REQUEST:
        if phase not in ((P_HEADERS, P_DATA, P_DATA_PAYLOAD) if is_client else (P_HEADERS, P_DATA, P_DATA_PAYLOAD, P_POST_TRAILERS)):
            return False
    elif kind == K_CONTROL:
        if phase not in (P_SETTINGS, P_OPEN):
            return False
    elif kind not in ALL_KINDS or phase != 0:
        return False
    return (data_left != 0) == (kind == K_REQUEST and phase == P_DATA_PAYLOAD)


def walk(buf, st, cap, mfps=16384, flags=0, defects=()):
    """one stream: -> dict(status, err, consumed, frames, section, enc, settings, out) -- frames: dicts with offsets
    relative to buf; section / enc: (offset, length) or None; out: the state to present next time"""
    b, end = bytes(buf), len(buf)
    is_client = bool(flags & CLIENT)
    r = dict(status=0, err=E_NONE, consumed=0, frames=[], section=None, enc=None, settings=None, out=dict(st))
    if not state_valid(st, is_client):
        r["status"] = EINVAL
        return r
    kind, phase, data_left, pos = st["kind"], st["phase"], st["data_left"], 0
    tunnel, walk_on = bool(st["flags"] & S_TUNNEL) and "tunnel_ignored" not in defects, bool(st["flags"] & S_WALK_ON)

    def stop(ret, err):
        r["status"], r["err"] = (0, E_NONE) if ret == INCOMPLETE else (ret, err)

    def slot():
        if len(r["frames"]) >= cap and "frame_slots_unlimited" not in defects:
            stop(FRAMES, E_NONE)
            return False
        return True

    def listed(typ, at, hdr, length, avail, aux=0):
        r["frames"].append(dict(type=typ, hdr_off=at, payload_off=at + hdr, length=length, avail=avail, aux=aux))

    while True:
        if kind == K_UNI:  # unknown_type_handle_input
            typ, p = quicint(b, pos, end)
            if typ is None:
                break
            pos = p
            if typ == 1 and "push_stream_is_control" in defects:
                typ = 0
            kind = {0: K_CONTROL, 2: K_QPACK_ENCODER, 3: K_QPACK_DECODER}.get(typ, K_DISCARD)
            phase = P_SETTINGS if kind == K_CONTROL else 0
            if "uni_waits_behind_type" in defects:
                break
            continue
        if kind == K_QPACK_ENCODER:
            if "encoder_bytes_kept" not in defects:
                if end > pos:
                    r["enc"] = (pos, end - pos)
                pos = end
            break
        if kind == K_QPACK_DECODER:
            if "decoder_bytes_consumed" in defects:
                pos = end
            break
        if kind == K_DISCARD:
            if "discard_keeps" not in defects:
                pos = end
            break
        if pos == end:
            break
        if kind == K_CONTROL:  # control_stream_handle_input
            ret, err, typ, length, hdr, p = read_frame(b, pos, end, mfps, is_client, True, defects)
            if ret != 0:
                stop(ret, err)
                break
            received = phase == P_OPEN
            if "settings_order" in defects and not received and typ != SETTINGS:
                stop(MISSING_SETTINGS, E_NONE)
                break
            if received == (typ == SETTINGS) or typ == DATA:
                stop(FRAME_UNEXPECTED, E_NONE)
                break
            payload, aux, got = b[pos + hdr:p], 0, None
            if not received:
                ret, got = handle_settings_frame(payload, bool(st["flags"] & S_PEER_DATAGRAMS), defects)
                err = E_MALFORMED_SETTINGS if ret else E_NONE
            elif not is_client and typ in (PRIORITY_UPDATE_REQUEST, PRIORITY_UPDATE_PUSH):
                ret, err, aux = decode_priority_update_frame(payload, typ == PRIORITY_UPDATE_PUSH, defects)
            elif is_client and typ == GOAWAY:
                ret, err, aux = decode_goaway_frame(payload, defects)
            if ret != 0:
                stop(ret, err)
                break
            if not slot():
                break
            listed(typ, pos, hdr, length, length, aux)
            pos = p
            if got is not None:
                r["settings"], phase = got, P_OPEN
            continue
        # request streams
        if phase == P_DATA_PAYLOAD:  # handle_input_expect_data_payload / handle_input_data_payload
            if not slot():
                break
            take = min(data_left, end - pos)
            listed(DATA, pos, 0, data_left, take)
            pos, data_left = pos + take, data_left - take
            if data_left == 0:
                phase = P_DATA
            continue
        ret, err, typ, length, hdr, p = read_frame(b, pos, end, mfps, is_client, False, defects)
        if phase == P_HEADERS:  # handle_input_expect_headers of either side
            if ret != 0:
                if ret == INCOMPLETE:
                    pass
                elif is_client:
                    if "client_error_as_is" not in defects:
                        ret, err = EXCESSIVE_LOAD, E_RESPONSE_TOO_LARGE
                elif err == E_FRAME_TOO_LARGE and (typ == HEADERS or "rejected_for_any_type" in defects):
                    ret = REJECTED
                stop(ret, err)
                break
            if typ == DATA:
                stop(FRAME_UNEXPECTED, E_DATA_BEFORE_HEADERS if is_client else E_NONE)
                break
            if not slot():
                break
            listed(typ, pos, hdr, length, length, 0)
            pos = p
            if typ == HEADERS:
                r["section"], phase = (pos - length, length), P_DATA
                if not walk_on and "no_stop_behind_section" not in defects:
                    break
            continue
        if ret != 0:  # handle_input_expect_data / _post_trailers / the client's handle_input_expect_data_frame
            stop(ret, err)
            break
        if phase == P_POST_TRAILERS:
            if typ == HEADERS or (typ == DATA and "post_trailers_takes_data" not in defects):
                stop(FRAME_UNEXPECTED, E_NONE)
                break
        elif typ == HEADERS and tunnel:
            stop(FRAME_UNEXPECTED, E_NONE if is_client else E_UNEXPECTED_TYPE)
            break
        if not slot():
            break
        if typ == DATA:
            take = min(length, end - p)
            listed(DATA, pos, hdr, length, take)
            pos, data_left = p + take, length - take
            if data_left:
                phase = P_DATA_PAYLOAD
            continue
        if typ == HEADERS and "trailers_as_section" in defects and r["section"] is None:
            listed(typ, pos, hdr, length, length, 0)
            r["section"] = (p - length, length)
        else:
            listed(typ, pos, hdr, length, length, NOSEC if typ == HEADERS else 0)
        if typ == HEADERS and (not is_client or "client_post_trailers" in defects):
            phase = P_POST_TRAILERS
        pos = p
    r["consumed"] = pos
    r["out"] = dict(st, kind=kind, phase=phase, data_left=data_left)
    return r


def sat32(v):
    return min(v, 0xFFFFFFFF)


STREAM_DT = np.dtype([("stream_id", "<u8"), ("data_left", "<u8"), ("kind", "u1"), ("phase", "u1"), ("flags", "u1"),
                      ("rsv", "u1", (13,))])
FRAME_DT = np.dtype([("type", "<u8"), ("hdr_off", "<u4"), ("payload_off", "<u4"), ("length", "<u8"), ("avail", "<u4"),
                     ("aux", "<u4")])
SETTINGS_DT = np.dtype([("max_field_section_size", "<u8"), ("h3_datagram", "<u4"), ("rsv", "<u4")])
PEER_DT = np.dtype([("max_table_capacity", "<u4"), ("max_blocked", "<u4")])


def pack_states(states):
    a = np.zeros(len(states), STREAM_DT)
    for i, st in enumerate(states):
        for k in ("stream_id", "data_left", "kind", "phase", "flags"):
            a[k][i] = st[k]
        a["rsv"][i, 0] = st.get("rsv", 0)
    return a


def batch(conns, mfps=16384, flags=0, arena_fixed=0, arena_per_byte=0):
    """conns: [[(bytes, state, frame cap)] per connection].  -> the call's inputs (data, str_off, conn_str, frm_first,
    frm_cap, st_in) and every output array as (2l) documents it; frame_used marks the frame slots written, and `walks`
    keeps the per-stream results."""
    streams = [s for c in conns for s in c]
    nstr, nconn = len(streams), len(conns)
    conn_str = np.concatenate([[0], np.cumsum([len(c) for c in conns])]).astype(np.uint32)
    lens = np.array([len(s[0]) for s in streams], np.int64)
    str_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    data = np.frombuffer(b"".join(bytes(s[0]) for s in streams), np.uint8).copy()
    frm_first = np.concatenate([[0], np.cumsum([s[2] for s in streams])]).astype(np.uint32)
    frm_cap = int(frm_first[-1])
    walks = [walk(s[0], s[1], s[2], mfps, flags) for s in streams]
    e = dict(data=data, str_off=str_off, conn_str=conn_str, frm_first=frm_first, frm_cap=frm_cap,
             st_in=pack_states([s[1] for s in streams]), walks=walks)
    e["st_out"] = pack_states([w["out"] for w in walks])
    e["nframes"] = np.array([len(w["frames"]) for w in walks], np.uint32)
    e["consumed"] = np.array([w["consumed"] for w in walks], np.uint32)
    e["sstatus"] = np.array([w["status"] for w in walks], np.int32)
    e["serr"] = np.array([w["err"] for w in walks], np.uint32)
    enc_total = sum(w["enc"][1] for w in walks if w["enc"])
    sec_total = sum(w["section"][1] for w in walks if w["section"])
    out = np.zeros(enc_total + sec_total, np.uint8)
    frames = np.zeros(frm_cap, FRAME_DT)
    used = np.zeros(frm_cap, bool)
    sec_off, sec_stream_id, sec_stream = [], [], []
    enc_at, sec_at = 0, enc_total
    enc_off, enc_len, conn_first = np.zeros(nconn, np.uint32), np.zeros(nconn, np.uint32), np.zeros(nconn + 1, np.uint32)
    peers, settings, got = np.zeros(nconn, PEER_DT), np.zeros(nconn, SETTINGS_DT), np.zeros(nconn, np.uint32)
    for c in range(nconn):
        conn_first[c], enc_off[c] = len(sec_off), enc_at
        for s in range(int(conn_str[c]), int(conn_str[c + 1])):
            w, base = walks[s], int(str_off[s])
            if w["enc"]:
                o, n = w["enc"]
                out[enc_at:enc_at + n] = data[base + o:base + o + n]
                enc_at += n
            for i, f in enumerate(w["frames"]):
                g = int(frm_first[s]) + i
                used[g] = True
                aux = len(sec_off) if f["type"] == HEADERS and f["aux"] != NOSEC else f["aux"]
                frames[g] = (f["type"], base + f["hdr_off"], base + f["payload_off"], f["length"], f["avail"], aux)
            if w["section"]:
                o, n = w["section"]
                out[sec_at:sec_at + n] = data[base + o:base + o + n]
                sec_off.append(sec_at), sec_stream_id.append(streams[s][1]["stream_id"]), sec_stream.append(s)
                sec_at += n
            if w["settings"] and not got[c]:
                g = w["settings"]
                got[c] = 1
                peers[c] = (sat32(g["max_table_capacity"]), sat32(g["max_blocked"]))
                settings[c] = (g["max_field_section_size"], g["h3_datagram"], 0)
        enc_len[c] = enc_at - int(enc_off[c])
    nsec = len(sec_off)
    conn_first[nconn] = nsec
    e.update(out=out, frames=frames, frame_used=used, enc_off=enc_off, enc_len=enc_len, conn_first=conn_first,
             sec_off=np.array(sec_off + [enc_total + sec_total] * (nstr + 1 - nsec), np.uint32),
             sec_stream_id=np.array(sec_stream_id, np.uint64), sec_stream=np.array(sec_stream, np.uint32),
             totals=np.array([nsec, sec_total, enc_total], np.uint32), peers=peers, settings=settings, got_settings=got)
    off = e["sec_off"].astype(np.uint64) - np.uint64(enc_total)
    idx = np.minimum(np.arange(nstr + 1), nsec).astype(np.uint64)
    e["arena_off"] = np.uint64(arena_fixed) * idx + np.uint64(arena_per_byte) * off
    return e
