"""A plain-Python model of hhuff_qpack_flatten_sessions with HHUFF_QENC_EVICT (include/hhuff.h (2g'), "Under the
flag"): the table that evicts entries no section still needs.  Written from the contract's six points -- absolute
indices with `evicted`, pins, the insert rule, the wrapped Required Insert Count, refusals decided before the
section touches the table -- on top of the model of the table that only grows (qpenc_dyn_model.py), whose static
lookup, integer and string coding, decoder stream and per-field order it shares.  It is the byte-level expectation
for the GPU; the decoders (restatement, reference, GPU) pin it by round trip.
"""
import numpy as np

import qpenc_dyn_model as M
from h2o_amd import codec as C
from qpenc_dyn_model import NONE64, SKIPPED, STATUS_INDEX, encode_int, qstring, static_lookup, varint  # noqa: F401

MAX_COUNT = (1 << 31) - 1


class Conn(M.Conn):
    """ent holds the live entries only: ent[k] has the absolute 1-based index evicted + k + 1"""

    def __init__(self, cap):
        super().__init__(cap)
        self.evicted = 0
        # inflight: [stream_id, largest_ref, blocking, smallest_ref]

    @property
    def count(self):
        return self.evicted + len(self.ent)

    def lookup(self, name, value, acked_only):
        found = -1
        for i in range(min(self.lkr, self.count) if acked_only else self.count, self.evicted, -1):
            n, v = self.ent[i - self.evicted - 1]
            if n != name:
                continue
            if v == value:
                return i, True
            if found < 0:
                found = i
        return found, False

    def handle_input(self, b):
        """M.Conn.handle_input reads the total insert count as len(ent): lend it that view for the call"""
        live, self.ent = self.ent, [None] * self.evicted + self.ent
        try:
            return super().handle_input(b)
        finally:
            self.ent = live

    def make_room(self, need, pin):
        """point 3: True when `need` fits after evicting the shortest unpinned prefix (then evicted), else nothing
        changes.  pin = the smallest pinned index, None when nothing is pinned"""
        if need > self.cap or self.count >= MAX_COUNT:
            return False
        k, used = 0, self.used
        while used + need > self.cap:
            if k == len(self.ent) or (pin is not None and self.evicted + k + 1 >= pin):
                return False
            used -= len(self.ent[k][0]) + len(self.ent[k][1]) + 32
            k += 1
        del self.ent[:k]
        self.evicted += k
        self.used = used
        return True


class _Section(M._Section):
    def __init__(self, conn, mode):
        self.c, self.mode = conn, mode
        self.base = conn.count
        self.largest, self.smallest = 0, None
        self.body, self.enc = bytearray(), bytearray()

    def ref(self, i):
        self.largest = max(self.largest, i)
        self.smallest = i if self.smallest is None else min(self.smallest, i)

    def dyn_indexed(self, i):
        self.ref(i)
        super().dyn_indexed(i)

    def field(self, sidx, sexact, ltr, name, value, dc):
        c = self.c
        if sidx is not None and sexact:
            self.body += encode_int(sidx, 6, 0xC0)
            return
        dyn, dexact = c.lookup(name, value, self.mode == 1) if self.mode else (-1, False)
        if dyn > 0 and dexact:
            self.dyn_indexed(dyn)
            return
        if ltr and self.mode == 2 and ((sidx is None and dyn < 0) or len(value) >= 8):
            pins = [e[3] for e in c.inflight] + ([self.smallest] if self.smallest is not None else [])
            if sidx is None and dyn > 0:
                pins.append(dyn)  # the entry the instruction names
            if c.make_room(len(name) + len(value) + 32, min(pins) if pins else None):
                if sidx is not None:
                    self.enc += encode_int(sidx, 6, 0xC0)
                elif dyn > 0:
                    self.enc += encode_int(c.count - dyn, 6, 0x80)
                else:
                    self.enc += qstring(name, 5, 0x40)
                self.enc += qstring(value, 7)
                c.ent.append((name, value))
                c.used += len(name) + len(value) + 32
                self.dyn_indexed(c.count)
                return
        vs = qstring(value, 7, 0, force_raw=dc)
        if sidx is not None:
            self.body += encode_int(sidx, 4, 0x50 | (0x20 if dc else 0)) + vs
        elif dyn > 0:
            self.ref(dyn)
            if dyn <= self.base:
                self.body += encode_int(self.base - dyn, 4, 0x40 | (0x20 if dc else 0)) + vs
            else:
                self.body += encode_int(dyn - self.base - 1, 3, 0x08 if dc else 0) + vs
        else:
            self.body += qstring(name, 3, 0x20 | (0x10 if dc else 0)) + vs


def response_bound(q, R):
    """hhuff_qpack_session_response_bound of response R: its headers' bytes, server_len when it sends the server
    name, dfid_len when it has a datagram flow id"""
    fl = int(R["flags"])
    h = q["hdr"][int(R["hdr_first"]):int(R["hdr_first"]) + int(R["nhdr"])]
    nv = int(h["name_len"].astype(np.int64).sum() + h["value_len"].astype(np.int64).sum())
    server = q["server_len"] if not fl & C.QRES_REQUEST and fl & C.RES_SERVER else 0
    return int(C.qpack_session_response_bound(nv, int(R["nhdr"]), server, int(R["dfid_len"]) if fl & C.QRES_DATAGRAM else 0))


def insert_bound(q, R):
    """point 5: 20 + name_len + value_len over the section's token headers that are likely to repeat and over the
    server name when the section sends it"""
    fl = int(R["flags"])
    h = q["hdr"][int(R["hdr_first"]):int(R["hdr_first"]) + int(R["nhdr"])]
    ltr = (h["flags"] & (C.HDR_TOKEN | C.HDR_LIKELY_TO_REPEAT)) == (C.HDR_TOKEN | C.HDR_LIKELY_TO_REPEAT)
    b = int((20 + h["name_len"].astype(np.int64) + h["value_len"])[ltr].sum())
    if not fl & C.QRES_REQUEST and fl & C.RES_SERVER and q["server_len"]:
        b += 20 + 6 + q["server_len"]
    return b


class Model(M.Model):
    """M.Model with HHUFF_QENC_EVICT on every step"""

    def __init__(self, nconn, header_table_size=4096, max_blocked=100, max_inflight=64):
        super().__init__(nconn, header_table_size, max_blocked, max_inflight)
        self.conns = [Conn(header_table_size) for _ in range(nconn)]
        self.started = False

    def _walk(self, q, c, R, mode):
        """the fields in M.Model._walk's order against an evicting section"""
        real, M._Section = M._Section, _Section
        try:
            return super()._walk(q, c, R, mode)
        finally:
            M._Section = real

    def counts(self):
        return np.array([c.count for c in self.conns])

    def step(self, q, dec=None, flags=C.QENC_EVICT):
        """One hhuff_qpack_flatten_sessions call with HHUFF_QENC_EVICT; M.Model.step's arguments and result.  A
        continued call without the flag is the mode mismatch: HHUFF_RES_EINVAL everywhere, no state change"""
        q = dict(q)
        q["_bytes"] = q["data"].tobytes()
        nconn, nres = len(self.conns), q["res"].size
        r = dict(frames=[b""] * nres, out_len=np.zeros(nres, np.uint32), header_len=np.zeros(nres, np.uint32),
                 rstatus=np.zeros(nres, np.int32), rflags=np.zeros(nres, np.uint8), enc=[b""] * nconn,
                 dec_status=np.zeros(nconn, np.int32), dec_consumed=np.zeros(nconn, np.uint32),
                 inflight=np.zeros(nres, bool), blocking=np.zeros(nres, bool),
                 enc_out_len=np.zeros(nconn, np.uint32))
        fresh = not flags & C.QENC_CONTINUE
        if not fresh and not flags & C.QENC_EVICT:
            r["rstatus"][:int(q["conn_first"][nconn])] = C.RES_EINVAL
            r["dec_status"][:] = C.RES_EINVAL
            return r
        assert flags & C.QENC_EVICT, "a fresh step without the flag is qpenc_dyn_model's"
        if fresh:
            self.conns = [Conn(self.H) for _ in range(nconn)]
        eo = q.get("enc_out_off")
        full = 2 * (self.H // 32)
        for ci, c in enumerate(self.conns):
            r0, r1 = int(q["conn_first"][ci]), int(q["conn_first"][ci + 1])
            room = self.H + 4 if eo is None else max(0, int(eo[ci + 1]) - int(eo[ci]))
            if c.failed:
                r["dec_status"][ci] = SKIPPED
            elif dec is not None:
                r["dec_status"][ci], r["dec_consumed"][ci] = c.handle_input(dec[ci])
                c.failed = r["dec_status"][ci] != 0
            if c.failed:
                r["rstatus"][r0:r1] = C.RES_SKIPPED
                continue
            enc = bytearray()
            setcap = encode_int(self.H, 5, 0x20) if fresh and flags & C.QENC_SET_CAPACITY else b""
            if len(setcap) > room:
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
                mode = 0 if len(c.inflight) >= self.max_inflight else 2 if buf else 1
                bound = response_bound(q, R)
                if region < bound or bound >= 1 << 32 or (mode == 2 and room - len(enc) < insert_bound(q, R)):
                    r["rstatus"][k] = C.RES_SPACE
                    continue
                r["rflags"][k] = 1 if mode == 0 else 0
                s = self._walk(q, c, R, mode)
                largest, base, blocking = s.largest, s.base, False
                if largest == 0:
                    prefix = b"\0\0"
                else:
                    if largest < c.lkr:
                        largest = c.lkr
                    blocking = largest > c.lkr
                    prefix = encode_int(largest % full + 1, 8)
                    prefix += encode_int(base - largest, 7) if largest <= base else encode_int(largest - base - 1, 7, 0x80)
                    c.inflight.append([int(q["stream_id"][k]), largest, int(blocking), s.smallest])
                    c.num_blocked += int(blocking)
                    r["inflight"][k], r["blocking"][k] = True, blocking
                body = prefix + bytes(s.body)
                frame = b"\x01" + varint(len(body)) + body
                assert len(frame) <= region and len(enc) + len(s.enc) <= room, "the bounds of point 5 hold"
                enc += s.enc
                r["frames"][k], r["out_len"][k], r["header_len"][k] = frame, len(frame), len(body)
            r["enc"][ci] = bytes(enc)
        r["enc_out_len"] = np.array([len(e) for e in r["enc"]], np.uint32)
        return r
