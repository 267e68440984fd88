"""A plain-Python model of hhuff_qpack_flatten_sessions (include/hhuff.h (2g')): QPACK encoder sessions with a
dynamic table per connection.  Written from the contract: the 1-based table that never evicts, lookup newest to
oldest, the per-field decision, the section prefix, the inflight list and the decoder stream.  It is the
byte-level expectation for the GPU; the decoders (restatement, reference, GPU) pin it by round trip.
"""
import numpy as np

from h2o_amd import codec as C
from h2o_amd import tables
from h2o_amd.hpack_synth import encode_int
from h2o_amd.qpack_synth import qstring

QSTATIC = tables.QPACK_STATIC_TABLE
NONE64 = 0xFFFFFFFFFFFFFFFF
STATUS_INDEX = {103: 24, 200: 25, 304: 26, 404: 27, 503: 28, 100: 63, 204: 64, 206: 65, 302: 66, 400: 67, 403: 68,
                421: 69, 425: 70, 500: 71}
DECODER_STREAM = 0x30202
DECOMPRESSION_FAILED = 0x30200
SKIPPED = -301
INT64_MAX = (1 << 63) - 1


def static_lookup(name, value):
    """h2o_qpack_lookup_static for a token: the entry with the name and value, else the first with the name"""
    first = None
    for i, (n, v) in enumerate(QSTATIC):
        if n == name:
            if v == value:
                return i, True
            if first is None:
                first = i
    return first, False


def varint(v):
    if v <= 63:
        return bytes([v])
    if v <= 16383:
        return (0x4000 | v).to_bytes(2, "big")
    if v <= 1073741823:
        return (0x80000000 | v).to_bytes(4, "big")
    return (0xC000000000000000 | v).to_bytes(8, "big")


def decode_int(b, p, prefix):
    """-> (value, next p); value None: incomplete; value -1: overflow"""
    mx = (1 << prefix) - 1
    if p >= len(b):
        return None, p
    v = b[p] & mx
    p += 1
    if v != mx:
        return v, p
    for shift in range(0, 56, 7):
        if p == len(b):
            return None, p
        v += (b[p] & 127) << shift
        p += 1
        if not b[p - 1] & 128:
            return v, p
    if p == len(b):
        return None, p
    if b[p] & 128:
        return -1, p
    v += (b[p] & 127) << 56
    return (-1 if v > INT64_MAX else v), p + 1


class Conn:
    def __init__(self, cap):
        self.cap = cap
        self.ent = []          # (name, value); entry k has the 1-based index k + 1
        self.used = 0
        self.lkr = 0           # largest_known_received
        self.num_blocked = 0
        self.inflight = []     # [stream_id, largest_ref, blocking]
        self.failed = False

    def snapshot(self):
        return len(self.ent), self.used

    def restore(self, s):
        del self.ent[s[0]:]
        self.used = s[1]

    def lookup(self, name, value, acked_only):
        """-> (index or -1, exact): newest to oldest, the first exact match, else the newest name match"""
        found = -1
        for i in range(self.lkr if acked_only else len(self.ent), 0, -1):
            n, v = self.ent[i - 1]
            if n != name:
                continue
            if v == value:
                return i, True
            if found < 0:
                found = i
        return found, False

    def handle_input(self, b):
        """the decoder stream -> (status, consumed)"""
        p = 0
        while p < len(b):
            kind = b[p] >> 6
            v, q = decode_int(b, p, 7 if kind >= 2 else 6)
            if v is None:
                return 0, p
            if v < 0:
                return DECOMPRESSION_FAILED, p
            p = q
            if kind == 0:  # Insert Count Increment
                if v == 0 or self.lkr + v >= len(self.ent) + 1:
                    return DECODER_STREAM, p
                self.lkr += v
            elif kind == 1:  # Stream Cancellation
                for e in [e for e in self.inflight if e[0] == v]:
                    self.num_blocked -= e[2]
                self.inflight = [e for e in self.inflight if e[0] != v]
            else:  # Section Acknowledgment
                k = next((k for k, e in enumerate(self.inflight) if e[0] == v), None)
                if k is None:
                    return DECODER_STREAM, p
                e = self.inflight.pop(k)
                self.lkr = max(self.lkr, e[1])
                self.num_blocked -= e[2]
        return 0, p


class _Section:
    """one response against one connection; mode: 2 with an encoder buffer, 1 without, 0 no encoder at all"""

    def __init__(self, conn, mode):
        self.c, self.mode = conn, mode
        self.base = len(conn.ent)
        self.largest = 0
        self.body = bytearray()
        self.enc = bytearray()

    def dyn_indexed(self, i):
        self.largest = max(self.largest, i)
        if i <= self.base:
            self.body += encode_int(self.base - i, 6, 0x80)
        else:
            self.body += encode_int(i - self.base - 1, 4, 0x10)

    def field(self, sidx, sexact, ltr, name, value, dc):
        c = self.c
        if sidx is not None and sexact:
            self.body += encode_int(sidx, 6, 0xC0)
            return
        dyn, dexact = c.lookup(name, value, self.mode == 1) if self.mode else (-1, False)
        if dyn > 0 and dexact:
            self.dyn_indexed(dyn)
            return
        if ltr and self.mode == 2 and ((sidx is None and dyn < 0) or len(value) >= 8) and \
                len(name) + len(value) + 32 <= c.cap - c.used:
            if sidx is not None:
                self.enc += encode_int(sidx, 6, 0xC0)
            elif dyn > 0:
                self.enc += encode_int(len(c.ent) - dyn, 6, 0x80)  # relative (RFC 9204 4.3.2), not h2o's absolute
            else:
                self.enc += qstring(name, 5, 0x40)
            self.enc += qstring(value, 7)
            c.ent.append((name, value))
            c.used += len(name) + len(value) + 32
            self.dyn_indexed(len(c.ent))
            return
        vs = qstring(value, 7, 0, force_raw=dc)
        if sidx is not None:
            self.body += encode_int(sidx, 4, 0x50 | (0x20 if dc else 0)) + vs
        elif dyn > 0:
            self.largest = max(self.largest, dyn)
            if dyn <= self.base:
                self.body += encode_int(self.base - dyn, 4, 0x40 | (0x20 if dc else 0)) + vs
            else:
                self.body += encode_int(dyn - self.base - 1, 3, 0x08 if dc else 0) + vs
        else:
            self.body += qstring(name, 3, 0x20 | (0x10 if dc else 0)) + vs


class Model:
    def __init__(self, nconn, header_table_size=4096, max_blocked=100, max_inflight=64):
        self.H, self.max_blocked, self.max_inflight = header_table_size, max_blocked, max_inflight
        self.conns = [Conn(header_table_size) for _ in range(nconn)]

    def _walk(self, q, c, R, mode):
        data = q["_bytes"]
        s = _Section(c, mode)
        fl = int(R["flags"])
        request = bool(fl & C.QRES_REQUEST)
        if not request:
            st = int(R["status"])
            if st in STATUS_INDEX:
                s.field(STATUS_INDEX[st], True, 0, b":status", b"", False)
            else:
                s.field(24, False, 0, b":status", b"%d" % (st & 0xFFFF), False)
            if fl & C.RES_SERVER and q["server_len"]:
                s.field(92, False, 1, b"server", data[q["server_off"]:q["server_off"] + q["server_len"]], False)
            cl = int(R["content_length"])
            if cl == 0:
                s.field(4, True, 0, b"content-length", b"0", False)
            elif cl != NONE64:
                s.field(4, False, 0, b"content-length", b"%d" % cl, False)
        for h in q["hdr"][int(R["hdr_first"]):int(R["hdr_first"]) + int(R["nhdr"])]:
            name = data[h["name_off"]:int(h["name_off"]) + int(h["name_len"])]
            value = data[h["value_off"]:int(h["value_off"]) + int(h["value_len"])]
            f = int(h["flags"])
            sidx, sexact = static_lookup(name, value) if f & C.HDR_TOKEN else (None, False)
            ltr = bool(f & C.HDR_TOKEN) and bool(f & C.HDR_LIKELY_TO_REPEAT)
            s.field(sidx, sexact, ltr, name, value, bool(f & C.HDR_DONT_COMPRESS))
        if fl & C.QRES_DATAGRAM:
            s.field(None, False, 0, b"datagram-flow-id", data[R["dfid_off"]:int(R["dfid_off"]) + int(R["dfid_len"])], False)
        return s

    def _bad(self, q, R):
        n = q["data"].size if q.get("in_size") is None else q["in_size"]
        h0, nh = int(R["hdr_first"]), int(R["nhdr"])
        if h0 + nh > q["hdr"].size:
            return True
        fl = int(R["flags"])
        if not fl & C.QRES_REQUEST and fl & C.RES_SERVER and q["server_len"] and q["server_off"] + q["server_len"] > n:
            return True
        if fl & C.QRES_DATAGRAM and int(R["dfid_off"]) + int(R["dfid_len"]) > n:
            return True
        h = q["hdr"][h0:h0 + nh]
        return bool(((h["name_off"].astype(np.int64) + h["name_len"] > n) |
                     (h["value_off"].astype(np.int64) + h["value_len"] > n)).any())

    def step(self, q, dec=None, flags=0):
        """One hhuff_qpack_flatten_sessions call.  q: data, hdr, res, conn_first, stream_id, server_off,
        server_len, out_off and optionally enc_out_off; dec: the decoder-stream bytes per connection or None.
        -> dict frames (bytes per response), out_len, header_len, rstatus, rflags, enc (bytes per connection),
        dec_status, dec_consumed, inflight (per response: the section joined the inflight list), blocking"""
        q = dict(q)
        q["_bytes"] = q["data"].tobytes()
        nconn, nres = len(self.conns), q["res"].size
        if not flags & C.QENC_CONTINUE:
            self.conns = [Conn(self.H) for _ in range(nconn)]
        r = dict(frames=[b""] * nres, out_len=np.zeros(nres, np.uint32), header_len=np.zeros(nres, np.uint32),
                 rstatus=np.zeros(nres, np.int32), rflags=np.zeros(nres, np.uint8), enc=[b""] * nconn,
                 dec_status=np.zeros(nconn, np.int32), dec_consumed=np.zeros(nconn, np.uint32),
                 inflight=np.zeros(nres, bool), blocking=np.zeros(nres, bool))
        eo = q.get("enc_out_off")
        for ci, c in enumerate(self.conns):
            r0, r1 = int(q["conn_first"][ci]), int(q["conn_first"][ci + 1])
            room = self.H + 4 if eo is None else int(eo[ci + 1]) - int(eo[ci])
            if c.failed:
                r["dec_status"][ci] = SKIPPED
            elif dec is not None:
                r["dec_status"][ci], r["dec_consumed"][ci] = c.handle_input(dec[ci])
                c.failed = r["dec_status"][ci] != 0
            if c.failed:
                r["rstatus"][r0:r1] = C.RES_SKIPPED
                continue
            enc = bytearray()
            fresh = not flags & C.QENC_CONTINUE
            setcap = encode_int(self.H, 5, 0x20) if fresh and flags & C.QENC_SET_CAPACITY else b""
            if len(setcap) > room:  # not even the capacity instruction fits: nothing of this step is written
                r["rstatus"][r0:r1] = C.RES_SPACE
                continue
            enc += setcap
            for k in range(r0, r1):
                R = q["res"][k]
                region = int(q["out_off"][k + 1]) - int(q["out_off"][k])
                if self._bad(q, R) or region < 0:
                    r["rstatus"][k] = C.RES_EINVAL
                    continue
                buf = not int(R["flags"]) & C.QRES_NO_ENCODER_STREAM and c.num_blocked < self.max_blocked
                snap = c.snapshot()
                s = self._walk(q, c, R, 2 if buf else 1)
                if s.largest and len(c.inflight) >= self.max_inflight:  # no slot: as with no encoder at all
                    c.restore(snap)
                    s = self._walk(q, c, R, 0)
                    r["rflags"][k] |= 1
                largest, base, blocking = s.largest, s.base, False
                if largest == 0:
                    prefix = b"\0\0"
                else:
                    if largest < c.lkr:
                        largest = c.lkr
                    blocking = largest > c.lkr
                    prefix = encode_int(largest + 1, 8)
                    prefix += encode_int(base - largest, 7) if largest <= base else encode_int(largest - base - 1, 7, 0x80)
                body = prefix + bytes(s.body)
                frame = b"\x01" + varint(len(body)) + body
                if len(frame) > region or len(enc) + len(s.enc) > room:
                    c.restore(snap)
                    r["rstatus"][k] = C.RES_SPACE
                    r["rflags"][k] = 0
                    continue
                if s.largest:
                    c.inflight.append([int(q["stream_id"][k]), largest, int(blocking)])
                    c.num_blocked += int(blocking)
                    r["inflight"][k], r["blocking"][k] = True, blocking
                enc += s.enc
                r["frames"][k], r["out_len"][k], r["header_len"][k] = frame, len(frame), len(body)
            r["enc"][ci] = bytes(enc)
        r["enc_out_len"] = np.array([len(e) for e in r["enc"]], np.uint32)
        return r
