"""A plain-Python model of hhuff_qpack_flatten_sessions with HHUFF_QENC_EVICT | HHUFF_QENC_DUP (include/hhuff.h
(2g'), "Under the flag", point 7): the evicting table whose draining entries are duplicated instead of pinned.
Written from the contract -- the draining test, the rule at "an exact dynamic match", the room test whose pins
leave the matched entry out, the Duplicate instruction -- on top of the model of the evicting table
(qpenc_evict_model.py), which does everything else.  It is the byte-level expectation for the GPU; the decoders
(restatement, reference, GPU) pin it by round trip.
"""
import qpenc_dyn_model as M0
import qpenc_evict_model as E
from h2o_amd import codec as C
from qpenc_evict_model import encode_int

EVICT, DUP, CONTINUE = C.QENC_EVICT, C.QENC_DUP, C.QENC_CONTINUE


def older(c, i):
    """the bytes of the live entries below i, with the 32 per entry"""
    return sum(len(n) + len(v) + 32 for n, v in c.ent[:i - c.evicted - 1])


def draining(c, i):
    """point 7-1: the inserts the table can still take before entry i has to go are under a quarter of it"""
    return (c.cap - c.used) + older(c, i) < c.cap // 4


class _Section(E._Section):
    def field(self, sidx, sexact, ltr, name, value, dc):
        c = self.c
        if not (sidx is not None and sexact) and self.mode == 2 and ltr:
            i, exact = c.lookup(name, value, False)
            if i > 0 and exact and draining(c, i):
                # the room test of point 3; the matched entry is no pin: the prefix that goes may hold it
                pins = [e[3] for e in c.inflight] + ([self.smallest] if self.smallest is not None else [])
                count = c.count
                if c.make_room(len(name) + len(value) + 32, min(pins) if pins else None):
                    self.enc += encode_int(count - i, 5, 0x00)  # Duplicate, relative to the newest entry
                    c.ent.append((name, value))
                    c.used += len(name) + len(value) + 32
                    self.dyn_indexed(c.count)
                    return
        super().field(sidx, sexact, ltr, name, value, dc)


class Model(E.Model):
    """E.Model whose sessions duplicate when their first step has HHUFF_QENC_DUP"""

    def __init__(self, nconn, header_table_size=4096, max_blocked=100, max_inflight=64):
        super().__init__(nconn, header_table_size, max_blocked, max_inflight)
        self.dup = False

    def _walk(self, q, c, R, mode):
        if not self.dup:
            return super()._walk(q, c, R, mode)
        real, M0._Section = M0._Section, _Section
        try:
            return M0.Model._walk(self, q, c, R, mode)
        finally:
            M0._Section = real

    def step(self, q, dec=None, flags=EVICT | DUP):
        """One hhuff_qpack_flatten_sessions call; E.Model.step's arguments and result.  HHUFF_QENC_DUP without
        HHUFF_QENC_EVICT is the caller's error (the call returns HHUFF_RES_EINVAL before anything runs): not
        modelled.  A continued call whose DUP or EVICT bit differs from the session's is the mode mismatch:
        HHUFF_RES_EINVAL everywhere, no state change"""
        assert flags & EVICT or not flags & DUP, "HHUFF_QENC_DUP needs HHUFF_QENC_EVICT"
        if flags & CONTINUE:
            if bool(flags & DUP) != self.dup:
                return super().step(q, dec, flags=CONTINUE)  # E.Model's refusal
        else:
            self.dup = bool(flags & DUP)
        return super().step(q, dec, flags=flags & ~DUP)
