"""A plain-Python model of hhuff_qpack_flatten_sessions_peers (include/hhuff.h (2g'')): QPACK encoder sessions whose
table capacity, Required Insert Count modulus and blocked-stream limit come from each connection's own peer record.
Built on the three models of the uniform call without editing them: per connection one Model(1, cap_c, mb_c,
max_inflight) of the session's kind (qpenc_dyn_model: the table that only grows, qpenc_evict_model:
HHUFF_QENC_EVICT, qpenc_dup_model: with HHUFF_QENC_DUP), cap_c = min(max_table_capacity, H), mb_c = min(max_blocked
of the peer, max_blocked of the call) -- point 4 of the contract, the equivalence, taken as the definition.  A
splitter hands each model its own slice of a batch and a merger puts the results back.  Two things the uniform
models cannot say are added here: the MaxEntries modulus when the peer advertised more than H (point 2), and the
stability refusal (point 5)."""
import numpy as np

import qpenc_dup_model as D
import qpenc_dyn_model as M0
import qpenc_evict_model as E
from h2o_amd import codec as C

EV, DUP, CONT = C.QENC_EVICT, C.QENC_DUP, C.QENC_CONTINUE
PER_RESPONSE = ("out_len", "header_len", "rstatus", "rflags", "inflight", "blocking")
PER_CONN = ("dec_status", "dec_consumed", "enc_out_len")


def subset(q, conns):
    """the batch q with the connections `conns` alone, in that order: their responses, stream ids and regions (the
    regions' sizes kept, their starts packed); data and hdr are shared, so hdr_first still holds"""
    cf = q["conn_first"].astype(np.int64)
    idx = np.concatenate([np.arange(cf[c], cf[c + 1]) for c in conns] + [np.zeros(0, np.int64)]).astype(np.int64)
    oo = np.asarray(q["out_off"]).astype(np.int64)
    s = dict(q, res=q["res"][idx], stream_id=q["stream_id"][idx],
             conn_first=np.concatenate([[0], np.cumsum([cf[c + 1] - cf[c] for c in conns])]).astype(np.uint32),
             out_off=np.concatenate([[0], np.cumsum(oo[idx + 1] - oo[idx])]).astype(np.int64).view(np.uint64))
    if q.get("enc_out_off") is not None:
        eo = np.asarray(q["enc_out_off"]).astype(np.int64)
        cc = np.asarray(conns, np.int64)
        s["enc_out_off"] = np.concatenate([[0], np.cumsum(eo[cc + 1] - eo[cc])]).astype(np.int64).view(np.uint64)
    s["_responses"] = idx
    return s


def merge(q, parts):
    """parts = [(conns, result of the step on subset(q, conns))] covering every connection once -> the result of
    the whole step, in q's order"""
    cf = q["conn_first"].astype(np.int64)
    nconn, nres = cf.size - 1, q["res"].size
    r = dict(frames=[b""] * nres, enc=[b""] * nconn)
    for conns, p in parts:
        idx = np.concatenate([np.arange(cf[c], cf[c + 1]) for c in conns] + [np.zeros(0, np.int64)]).astype(np.int64)
        for k in PER_RESPONSE:
            if k in p:
                r.setdefault(k, np.zeros(nres, np.asarray(p[k]).dtype))[idx] = np.asarray(p[k])[:idx.size]
        for k in PER_CONN:
            r.setdefault(k, np.zeros(nconn, np.asarray(p[k]).dtype))[list(conns)] = np.asarray(p[k])[:len(conns)]
        for j, k in enumerate(idx):
            r["frames"][k] = p["frames"][j]
        for j, c in enumerate(conns):
            r["enc"][c] = p["enc"][j]
    return r


def reencode_ric(frame, ric):
    """the HEADERS frame with its Required Insert Count written as `ric`"""
    n = 1 << (frame[1] >> 6)
    sec = frame[1 + n:]
    _, p = M0.decode_int(sec, 0, 8)
    body = M0.encode_int(ric, 8) + sec[p:]
    return b"\x01" + M0.varint(len(body)) + body


class Model:
    """peers: a QPACK_PEER array, one record per connection; H, max_blocked, max_inflight: the call's"""

    def __init__(self, peers, header_table_size=4096, max_blocked=100, max_inflight=64):
        self.H, self.max_blocked, self.max_inflight = header_table_size, max_blocked, max_inflight
        self.peers = np.array(peers, C.QPACK_PEER)
        self.sub = [None] * self.peers.size
        self.adv = [0] * self.peers.size  # the capacity the connection's peer advertised when it started

    def cap(self, c, peers=None):
        p = self.peers if peers is None else peers
        return min(int(p["max_table_capacity"][c]), self.H)

    def blocked(self, c, peers=None):
        p = self.peers if peers is None else peers
        return min(int(p["max_blocked"][c]), self.max_blocked)

    def _new(self, c, flags, peers):
        kind = D.Model if flags & DUP else E.Model if flags & EV else M0.Model
        self.sub[c] = kind(1, self.cap(c, peers), self.blocked(c, peers), self.max_inflight)
        self.adv[c] = int(peers["max_table_capacity"][c])

    def conn(self, c):
        return self.sub[c].conns[0]

    def counts(self):
        """the insert count of every connection"""
        return np.array([0 if m is None else getattr(m.conns[0], "count", len(m.conns[0].ent)) for m in self.sub])

    def used(self):
        return np.array([0 if m is None else m.conns[0].used for m in self.sub])

    def step(self, q, dec=None, flags=0, peers=None, reset=None):
        """One hhuff_qpack_flatten_sessions_peers call on every connection; the uniform models' arguments and
        result.  peers: this step's records when they differ from the model's own (a fresh connection takes them, a
        continuing one must fit them); reset: per connection, HHUFF_CONN_RESET"""
        peers = self.peers if peers is None else np.array(peers, C.QPACK_PEER)
        n = self.peers.size
        parts = []
        for c in range(n):
            fresh = not flags & CONT or (reset is not None and reset[c])
            s = subset(q, [c])
            if fresh:
                self._new(c, flags, peers)
            elif self.conn(c).used > self.cap(c, peers):
                # point 5: the table holds more than this record allows -- refused like the mode mismatch
                k = s["res"].size
                parts.append(([c], dict(frames=[b""] * k, enc=[b""], out_len=np.zeros(k, np.uint32),
                                        header_len=np.zeros(k, np.uint32), rstatus=np.full(k, C.RES_EINVAL, np.int32),
                                        rflags=np.zeros(k, np.uint8), inflight=np.zeros(k, bool), blocking=np.zeros(k, bool),
                                        dec_status=np.array([C.RES_EINVAL], np.int32), dec_consumed=np.zeros(1, np.uint32),
                                        enc_out_len=np.zeros(1, np.uint32))))
                continue
            m = self.sub[c]
            r = m.step(s, None if dec is None else [dec[c]], flags=(flags & ~CONT) | (0 if fresh else CONT))
            if flags & EV and self.adv[c] > self.H:
                # point 2: MaxEntries of what the decoder advertised, not of the capacity in use.  The sections that
                # joined the inflight list in this step are its last records, in order.
                conn = m.conns[0]
                joined = [k for k in range(s["res"].size) if r["inflight"][k]]
                full = 2 * (self.adv[c] // 32)
                for k, e in zip(joined, conn.inflight[len(conn.inflight) - len(joined):]):
                    f = reencode_ric(r["frames"][k], e[1] % full + 1)
                    r["frames"][k], r["out_len"][k], r["header_len"][k] = f, len(f), len(f) - 1 - (1 << (f[1] >> 6))
            parts.append(([c], r))
        return merge(q, parts)
