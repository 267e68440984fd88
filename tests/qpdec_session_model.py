"""A plain-Python model of the QPACK decoder sessions (include/hhuff.h (2e'''), hhuff_qpack_parse_requests_sessions /
_parse_responses_sessions): what h2o keeps around its QPACK decoder, restated from the contract -- a stream that comes
up blocked is parked with its Required Insert Count while a slot is free (lib/http3/server.c:1551-1555), a reset stream
is released with a Stream Cancellation (:562-571) or silently (:919-922), parked streams whose count the table has
reached are woken oldest first (:1950-1966); the decoder stream carries the Section Acknowledgments (qpack.c:643-650),
the Stream Cancellations (:500-504) and, on request, the Insert Count Increment (:487-498, with the Known Received
Count of RFC 9204 4.4).  The QPACK decoding itself is the oracle's (oracle.QpackSession, restatement or reference), one
session per slot with a blocked-streams limit that never bites: the limit is this model's to apply.
"""
import numpy as np

from oracle import oracle as O

DF, SKIPPED, BLOCKED, EINVAL = 0x30200, -301, -302, -303
SYNC = SILENT = WAKE_PENDING = 1
CONN_RESET = 1
NO_LIMIT = 1 << 40


def prefix_int(first, v, bits):
    """h2o_hpack_encode_int's form: v behind `first` with a prefix of `bits` bits"""
    mask = (1 << bits) - 1
    if v < mask:
        return bytes([first | v])
    out, v = bytearray([first | mask]), v - mask
    while v >= 128:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    out.append(v)
    return bytes(out)


def out_bound(nsec, ncancel):
    return 10 * (nsec + ncancel) + 10


def reset_record(responses):
    """the record of a section nothing was read of: a refused connection's"""
    if responses:
        r = np.zeros(1, O.QRES_DTYPE)
        r["datagram_flow_id"] = -1
        return r[0]
    r = np.zeros(1, O.QREQ_DTYPE)
    r["content_length"] = 0xFFFFFFFFFFFFFFFF
    for k in ("method", "scheme", "authority", "path", "protocol", "expect", "datagram_flow_id"):
        r[k] = -1
    return r[0]


class Session:
    def __init__(self):
        self.parked = []  # [stream_id, ref], oldest first
        self.known_received = 0

    def find(self, sid):
        return next((i for i, e in enumerate(self.parked) if e[0] == sid), None)


class Model:
    def __init__(self, codec, nslots, header_table_size=4096, max_blocked=100, responses=False):
        self.codec, self.nslots, self.H, self.max_blocked, self.responses = codec, nslots, header_table_size, max_blocked, responses
        self.fresh(range(nslots))

    def fresh(self, which):
        if not hasattr(self, "sess"):
            self.dec, self.sess, self.total, self.failed = ([None] * self.nslots, [None] * self.nslots, [0] * self.nslots,
                                                           [False] * self.nslots)
        for s in which:
            self.dec[s], self.sess[s], self.total[s], self.failed[s] = None, Session(), 0, False

    def _decode(self, s, st, c, stream_id):
        """connection c's encoder stream and sections through slot s's decoder -> the oracle's dict, rebased"""
        if self.dec[s] is None:
            self.dec[s] = O.QpackSession(self.codec, 1, self.H, NO_LIMIT)
        k0, k1 = int(st["conn_first"][c]), int(st["conn_first"][c + 1])
        data = st["data"].tobytes()
        so = st["sec_off"].astype(np.int64)
        secs = data[int(so[k0]):int(so[k1])]
        e0 = int(st["enc_off"][c])
        enc = data[e0:e0 + int(st["enc_len"][c])]
        local = np.frombuffer(secs + enc + b"\0", np.uint8)
        sec_off = (so[k0:k1 + 1] - so[k0]).astype(np.uint32)
        return self.dec[s].step(local, [len(secs)], [len(enc)], sec_off, [0, k1 - k0], O.default_arena_off(sec_off, self.H),
                                stream_id=np.asarray(stream_id[k0:k1], np.uint64) if k1 > k0 else np.zeros(1, np.uint64),
                                responses=self.responses)

    def step(self, st, stream_id, slot=None, cflags=None, cont=True, cancels=None, dec_room=None, wake_room=None,
             sync=False, cancel_first=None):
        """One call.  st: data, enc_off, enc_len, sec_off, conn_first of the call's connections; slot / cflags: the
        slot map (None: connection c in slot c); cancels: per connection [(stream id, flags)]; dec_room / wake_room:
        per connection the sizes of its dec_out / wake_id regions (None: the bound / max_blocked); cancel_first: the
        array as given, when it is to be malformed.  -> dict sstatus, rec, req_insert_count, enc_status,
        enc_consumed, insert_count, dec (bytes per connection), dec_out_len, wake (ids per connection), nwake, parked,
        dflags"""
        cf = np.asarray(st["conn_first"], np.int64)
        nconn, nsec = cf.size - 1, int(cf[-1])
        if not cont:
            self.fresh(range(self.nslots))
        cancels = [[]] * nconn if cancels is None else cancels
        r = dict(sstatus=np.zeros(nsec, np.int32), rec=np.zeros(nsec, O.QRES_DTYPE if self.responses else O.QREQ_DTYPE),
                 req_insert_count=np.zeros(nsec, np.uint64), enc_status=np.zeros(nconn, np.int32),
                 enc_consumed=np.zeros(nconn, np.uint32), insert_count=np.zeros(nconn, np.uint64), dec=[b""] * nconn,
                 wake=[[] for _ in range(nconn)], parked=np.zeros(nconn, np.uint32), dflags=np.zeros(nconn, np.uint8))
        owner = {}
        for c in range(nconn):
            s = c if slot is None else int(slot[c])
            if s < self.nslots:
                owner.setdefault(s, c)
        for c in range(nconn):
            k0, k1 = int(cf[c]), int(cf[c + 1])
            s = c if slot is None else int(slot[c])
            f = 0 if cflags is None else int(cflags[c])
            room = out_bound(k1 - k0, len(cancels[c])) if dec_room is None else int(dec_room[c])
            refused = s >= self.nslots or owner[s] != c or f & ~CONN_RESET or room < out_bound(k1 - k0, len(cancels[c]))
            if cancel_first is not None and int(cancel_first[c + 1]) < int(cancel_first[c]):
                refused = True
            if refused:  # before anything touches its table or session
                r["enc_status"][c] = EINVAL
                r["sstatus"][k0:k1] = EINVAL
                r["rec"][k0:k1] = reset_record(self.responses)
                continue
            if f & CONN_RESET:
                self.fresh([s])
            d = self._decode(s, st, c, stream_id)
            key = "res" if self.responses else "req"
            r["enc_status"][c], r["enc_consumed"][c], r["insert_count"][c] = d["enc_status"][0], d["enc_consumed"][0], d["insert_count"][0]
            r["sstatus"][k0:k1], r["rec"][k0:k1] = d["sstatus"][:k1 - k0], d[key][:k1 - k0]
            r["req_insert_count"][k0:k1] = d["req_insert_count"][:k1 - k0]
            if int(d["insert_count"][0]):
                self.total[s] = int(d["insert_count"][0])
            self.failed[s] = self.failed[s] or int(d["enc_status"][0]) != 0
            se = self.sess[s]
            if self.failed[s]:  # emits nothing, wakes nothing
                r["parked"][c] = len(se.parked)
                continue
            out = bytearray()

            def put(b):  # an instruction, whole or not at all
                if len(out) + len(b) <= room:
                    out.extend(b)
            for k in range(k0, k1):  # 1. the sections
                stt, sid = int(r["sstatus"][k]), int(stream_id[k])
                if stt in (SKIPPED, EINVAL):
                    continue
                i = se.find(sid)
                if stt == BLOCKED:
                    if i is None:
                        if len(se.parked) >= self.max_blocked:
                            r["sstatus"][k] = DF
                        else:
                            se.parked.append([sid, int(r["req_insert_count"][k])])
                    continue
                if i is not None:
                    del se.parked[i]
                n = int(r["rec"]["ack_len"][k])
                if n:
                    put(bytes(r["rec"]["ack"][k][:n]))
                    se.known_received = max(se.known_received, int(r["req_insert_count"][k]))
            for sid, fl in cancels[c]:  # 2. the cancellations
                i = se.find(int(sid))
                if i is not None:
                    del se.parked[i]
                if not fl & SILENT:
                    put(prefix_int(0x40, int(sid), 6))
            wroom = self.max_blocked if wake_room is None else int(wake_room[c])  # 3. wake
            keep = []
            for e in se.parked:
                if e[1] <= self.total[s]:
                    if len(r["wake"][c]) < wroom:
                        r["wake"][c].append(e[0])
                        continue
                    r["dflags"][c] |= WAKE_PENDING
                keep.append(e)
            se.parked = keep
            if sync and self.total[s] > se.known_received:  # 4. Insert Count Increment
                put(prefix_int(0x00, self.total[s] - se.known_received, 6))
                se.known_received = self.total[s]
            r["dec"][c], r["parked"][c] = bytes(out), len(se.parked)
        r["dec_out_len"] = np.array([len(x) for x in r["dec"]], np.uint32)
        r["nwake"] = np.array([len(x) for x in r["wake"]], np.uint32)
        return r
