"""A plain model of the HTTP/2 de-framer's per-connection walk (include/hhuff.h (2k), rules 1-9), written from h2o's
own lines -- lib/http2/frame.c:130-224 (h2o_http2_decode_frame, h2o_http2_decode_headers_payload),
lib/http2/connection.c:757-803, 1023-1095, 1288-1325 (expect_continuation_of_headers, handle_headers_frame,
expect_default) -- and RFC 9113 6.6 for the PUSH_PROMISE route, not from h2o_amd/csrc/hhuff_frames.h.

  walk(buf, cap, max_frame_size=16384, max_block_bytes=0, flags=0, defects=()) -> dict
      frames    [dict(payload_off, length, stream_id, type, flags, frag_off, frag_len, block)]: offsets relative to
                buf, block = the block's number within the connection or None
      blocks    [dict(stream_id, end_stream_id, flags, dependency, weight, promised_stream_id, first_frame, nframes,
                data)]: first_frame within the connection, data = the block's bytes
      consumed, status, err
  batch(conns, caps, ...) -> the arrays hhuff_h2_deframe writes for these connections (numpy)

defects  names of DEFECTS: each makes the model wrong in one way; the corpus has to tell every one of them apart"""
HEADERS, PUSH_PROMISE, CONTINUATION = 1, 5, 9
END_STREAM, END_HEADERS, PADDED, PRIORITY = 0x1, 0x4, 0x8, 0x20
PROTOCOL, FRAME_SIZE = -1, -6
REFUSED, FRAMES = -310, -311  # HHUFF_H2F_REFUSED, HHUFF_H2F_FRAMES
ACCEPT_PUSH = 1
# HHUFF_H2F_ERR_*
(E_NONE, E_HEADERS_STREAM_ID, E_HEADERS_FRAME, E_HEADERS_PRIORITY, E_EXPECTED_CONTINUATION, E_INVALID_CONTINUATION,
 E_PUSH_PROMISE, E_PROMISE_STREAM_ID, E_PROMISE_FRAME) = range(9)
# HHUFF_H2B_*
B_END_STREAM, B_PRIORITY, B_EXCLUSIVE, B_CONTINUED, B_PROMISE, B_SELF_DEPENDENCY = 1, 2, 4, 8, 16, 32
ALL_STATUS = (0, PROTOCOL, FRAME_SIZE, REFUSED, FRAMES)
ALL_ERR = tuple(range(9))
ALL_BLOCK_FLAGS = (B_END_STREAM, B_PRIORITY, B_EXCLUSIVE, B_CONTINUED, B_PROMISE, B_SELF_DEPENDENCY)

DEFECTS = (
    "size_after_complete",    # the frame size limit tested after completeness
    "size_ge",                # length == max_frame_size refused
    "cont_stream_checked",    # a CONTINUATION on another stream refused
    "pad_eq_refused",         # a pad length equal to the bytes behind the pad byte refused
    "pad_zero_len_ok",        # PADDED with length 0 taken as an empty fragment
    "prio_4_ok",              # a priority field of 4 bytes accepted
    "prio_before_pad",        # the priority field read before the padding is cut off
    "weight_raw",             # weight = the byte, not the byte + 1
    "even_ok",                # an even stream id accepted
    "topbit_kept",            # the reserved bit of the stream id kept
    "self_dep_error",         # dependency == stream id refused
    "open_block_consumed",    # an open block's frames consumed and listed
    "push_always",            # PUSH_PROMISE accepted without the flag
    "promise_3_ok",           # a promised id of 3 bytes accepted
    "unknown_type_error",     # frame types from 10 on refused
    "block_cap_ge",           # a block of exactly max_block_bytes refused
    "cap_counts_headers",     # the frame headers counted into the block's size
    "frames_block_started",   # a block whose frames do not all fit keeps those that do
    "end_stream_from_last",   # END_STREAM read off the last frame
    "end_id_from_opener",     # end_stream_id = the opener's
    "stray_cont_skipped",     # a stray CONTINUATION stepped over
    "other_in_block_skipped",  # another frame inside an open block stepped over
    "exclusive_in_dependency",  # the exclusive bit left in the dependency
)


def decode_frame(buf, pos, max_frame_size, defects=()):
    """h2o_http2_decode_frame: (size, length, type, flags, stream_id); size 0 = incomplete, -6 = too long"""
    if len(buf) - pos < 9:  # frame.c:133
        return 0, 0, 0, 0, 0
    length = int.from_bytes(buf[pos:pos + 3], "big")
    typ, flags = buf[pos + 3], buf[pos + 4]
    sid = int.from_bytes(buf[pos + 5:pos + 9], "big")
    if "topbit_kept" not in defects:
        sid &= 0x7fffffff
    too_long = length >= max_frame_size if "size_ge" in defects else length > max_frame_size
    if too_long and "size_after_complete" not in defects:  # :141
        return FRAME_SIZE, length, typ, flags, sid
    if len(buf) - pos < 9 + length:  # :144
        return 0, length, typ, flags, sid
    if too_long:
        return FRAME_SIZE, length, typ, flags, sid
    return 9 + length, length, typ, flags, sid


def _padding(pay, flags, defects, err):
    """frame.c:198-210: (at, end) of what is left, or the error"""
    at, end = 0, len(pay)
    if flags & PADDED:
        if end == 0:
            if "pad_zero_len_ok" in defects:
                return at, end, E_NONE
            return 0, 0, err
        padlen = pay[0]
        at = 1
        if end - at < padlen or ("pad_eq_refused" in defects and end - at == padlen):
            return 0, 0, err
        end -= padlen
    return at, end, E_NONE


def headers_payload(pay, flags, sid, defects=(), parity=True):
    """h2o_http2_decode_headers_payload, then handle_headers_frame's parity test (connection.c:1032):
    (ret, err, frag_off, frag_len, exclusive, dependency, weight); parity=False: the first function alone"""
    bad = lambda e: (PROTOCOL, e, 0, 0, 0, 0, 16)  # noqa: E731
    if sid == 0:  # frame.c:193
        return bad(E_HEADERS_STREAM_ID)
    excl, dep, weight = 0, 0, 16  # h2o_http2_default_priority
    if "prio_before_pad" in defects and flags & PRIORITY and flags & PADDED and len(pay) >= 6:
        at, end = 1, len(pay)
        u4 = int.from_bytes(pay[1:5], "big")
        excl, dep, weight = u4 >> 31, u4 & 0x7fffffff, pay[5] + 1
        return 0, E_NONE, 6, max(0, end - 6 - pay[0]), excl, dep, weight
    at, end, e = _padding(pay, flags, defects, E_HEADERS_FRAME)
    if e:
        return bad(e)
    if flags & PRIORITY:
        need = 4 if "prio_4_ok" in defects else 5
        if end - at < need:  # :213
            return bad(E_HEADERS_PRIORITY)
        u4 = int.from_bytes(pay[at:at + 4], "big")
        excl, dep = u4 >> 31, u4 if "exclusive_in_dependency" in defects else u4 & 0x7fffffff
        w = pay[at + 4] if at + 4 < end else 0
        weight = w if "weight_raw" in defects else w + 1
        at = min(at + 5, end)
    if parity and sid & 1 == 0 and "even_ok" not in defects:
        return bad(E_HEADERS_STREAM_ID)
    return 0, E_NONE, at, end - at, excl, dep, weight


def promise_payload(pay, flags, sid, defects=()):
    """RFC 9113 6.6: (ret, err, frag_off, frag_len, promised)"""
    if sid == 0:
        return PROTOCOL, E_PROMISE_STREAM_ID, 0, 0, 0
    at, end, e = _padding(pay, flags, defects, E_PROMISE_FRAME)
    if e:
        return PROTOCOL, e, 0, 0, 0
    need = 3 if "promise_3_ok" in defects else 4
    if end - at < need:
        return PROTOCOL, E_PROMISE_FRAME, 0, 0, 0
    promised = int.from_bytes(pay[at:at + 4], "big") & 0x7fffffff
    at = min(at + 4, end)
    return 0, E_NONE, at, end - at, promised


def walk(buf, cap, max_frame_size=16384, max_block_bytes=0, flags=0, defects=()):
    buf = bytes(buf)
    frames, blocks = [], []
    out = dict(frames=frames, blocks=blocks, consumed=0, status=0, err=E_NONE)

    def stop(status, err=E_NONE):
        out["status"], out["err"] = status, err
        return out

    pos = 0
    while True:
        size, length, typ, fl, sid = decode_frame(buf, pos, max_frame_size, defects)
        if size <= 0:
            return stop(size)
        pay = pos + 9
        rec = dict(payload_off=pay, length=length, stream_id=sid, type=typ, flags=fl, frag_off=0, frag_len=0, block=None)
        skipped = typ not in (HEADERS, PUSH_PROMISE, CONTINUATION) or (typ == CONTINUATION and "stray_cont_skipped" in defects)
        if skipped:
            if typ >= 10 and "unknown_type_error" in defects:
                return stop(PROTOCOL)
            if len(frames) == cap:
                return stop(FRAMES)
            frames.append(rec)
            pos += size
            out["consumed"] = pos
            continue
        if typ == CONTINUATION:  # connection.c:1294-1298
            return stop(PROTOCOL, E_INVALID_CONTINUATION)
        payload = buf[pay:pay + length]
        promised, excl, dep, weight = 0, 0, 0, 16
        if typ == PUSH_PROMISE:
            if not flags & ACCEPT_PUSH and "push_always" not in defects:  # :1288-1292
                return stop(PROTOCOL, E_PUSH_PROMISE)
            ret, err, foff, flen, promised = promise_payload(payload, fl, sid, defects)
        else:
            ret, err, foff, flen, excl, dep, weight = headers_payload(payload, fl, sid, defects)
        if ret:
            return stop(ret, err)
        rec.update(frag_off=pay + foff, frag_len=flen, block=len(blocks))
        unit, data, q, last = [rec], [buf[pay + foff:pay + foff + flen]], pos + size, (fl, sid)
        total = flen + (9 if "cap_counts_headers" in defects else 0)
        if not fl & END_HEADERS:
            while True:  # expect_continuation_of_headers
                size2, len2, typ2, fl2, sid2 = decode_frame(buf, q, max_frame_size, defects)
                verdict = None
                if size2 <= 0:
                    verdict = (size2, E_NONE)
                elif typ2 != CONTINUATION:  # :766-769
                    if "other_in_block_skipped" in defects:
                        q += size2
                        continue
                    verdict = (PROTOCOL, E_EXPECTED_CONTINUATION)
                elif "cont_stream_checked" in defects and sid2 != sid:
                    verdict = (PROTOCOL, E_EXPECTED_CONTINUATION)
                elif max_block_bytes and (total + len2 >= max_block_bytes if "block_cap_ge" in defects
                                          else total + len2 > max_block_bytes):  # :777
                    verdict = (REFUSED, E_NONE)
                if verdict is not None:
                    if "open_block_consumed" in defects:
                        frames.extend(unit[:max(0, cap - len(frames))])
                        out["consumed"] = q
                    return stop(*verdict)
                total += len2 + (9 if "cap_counts_headers" in defects else 0)
                unit.append(dict(payload_off=q + 9, length=len2, stream_id=sid2, type=typ2, flags=fl2, frag_off=q + 9,
                                 frag_len=len2, block=len(blocks)))
                data.append(buf[q + 9:q + 9 + len2])
                q += size2
                last = (fl2, sid2)
                if fl2 & END_HEADERS:
                    break
        if len(unit) > cap - len(frames):
            if "frames_block_started" in defects:
                frames.extend(unit[:cap - len(frames)])
            return stop(FRAMES)
        bflags = B_PROMISE if typ == PUSH_PROMISE else 0
        es = last[0] if "end_stream_from_last" in defects else fl
        if typ == HEADERS and es & END_STREAM:
            bflags |= B_END_STREAM
        if len(unit) > 1:
            bflags |= B_CONTINUED
        if typ == HEADERS and fl & PRIORITY:
            bflags |= B_PRIORITY | (B_EXCLUSIVE if excl else 0)
            if dep == sid:
                if "self_dep_error" in defects:
                    return stop(PROTOCOL)
                bflags |= B_SELF_DEPENDENCY
        blocks.append(dict(stream_id=sid, end_stream_id=sid if "end_id_from_opener" in defects else last[1], flags=bflags,
                           dependency=dep, weight=weight, promised_stream_id=promised, first_frame=len(frames),
                           nframes=len(unit), data=b"".join(data)))
        frames.extend(unit)
        pos = q
        out["consumed"] = pos


def batch(conns, caps, max_frame_size=16384, max_block_bytes=0, flags=0, arena_fixed=None, arena_per_byte=0):
    """What hhuff_h2_deframe writes for the connections `conns` (bytes each) with caps[c] frame slots: a dict of numpy
    arrays named as the call's arguments, plus data, in_off, frm_first (the inputs) and frame_used (bool per slot)."""
    import numpy as np

    from h2o_amd import codec

    nconn = len(conns)
    in_off = np.zeros(nconn + 1, np.uint32)
    in_off[1:] = np.cumsum([len(c) for c in conns], dtype=np.uint64)
    frm_first = np.zeros(nconn + 1, np.uint32)
    frm_first[1:] = np.cumsum(caps, dtype=np.uint64)
    frm_cap = int(frm_first[-1])
    frames = np.zeros(frm_cap, codec.H2_FRAME_DTYPE)
    used = np.zeros(frm_cap, bool)
    blocks = np.zeros(frm_cap, codec.H2_BLOCK_DTYPE)
    u32 = lambda: np.zeros(nconn, np.uint32)  # noqa: E731
    nframes, consumed, cerr, cstatus = u32(), u32(), u32(), np.zeros(nconn, np.int32)
    conn_first = np.zeros(nconn + 1, np.uint32)
    blk, blk_off = [], [0]
    nb = 0
    for c, buf in enumerate(conns):
        w = walk(buf, int(caps[c]), max_frame_size, max_block_bytes, flags)
        nframes[c], consumed[c], cstatus[c], cerr[c] = len(w["frames"]), w["consumed"], w["status"], w["err"]
        conn_first[c] = nb
        f0, base = int(frm_first[c]), int(in_off[c])
        for i, f in enumerate(w["frames"]):
            hdr = f["block"] is not None
            frames[f0 + i] = (f["payload_off"] + base, f["length"], f["stream_id"], f["type"], f["flags"], 0,
                              f["frag_off"] + base if hdr else 0, f["frag_len"], nb + f["block"] if hdr else 0xFFFFFFFF, 0)
            used[f0 + i] = True
        for b in w["blocks"]:
            blocks[nb] = (b["stream_id"], b["end_stream_id"], b["flags"], b["dependency"], b["weight"],
                          b["promised_stream_id"], b["first_frame"] + f0, b["nframes"])
            blk.append(b["data"])
            blk_off.append(blk_off[-1] + len(b["data"]))
            nb += 1
    conn_first[nconn] = nb
    full_off = np.full(frm_cap + 1, blk_off[-1], np.uint32)
    full_off[:nb + 1] = blk_off
    r = dict(data=np.frombuffer(b"".join(bytes(c) for c in conns), np.uint8).copy(), in_off=in_off, frm_first=frm_first,
             frm_cap=frm_cap, frames=frames, frame_used=used, nframes=nframes, consumed=consumed, cstatus=cstatus, cerr=cerr,
             blk=np.frombuffer(b"".join(blk), np.uint8).copy(), blk_off=full_off, conn_first=conn_first, blocks=blocks,
             totals=np.array([nb, blk_off[-1]], np.uint32))
    if arena_fixed is not None:
        k = np.minimum(np.arange(frm_cap + 1, dtype=np.uint64), np.uint64(nb))
        r["arena_off"] = k * np.uint64(arena_fixed) + full_off.astype(np.uint64) * np.uint64(arena_per_byte)
    return r
