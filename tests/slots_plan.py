"""Sparse steps over connection slots (include/hhuff.h (2h)) for the tests: a dense multi-step session of one of
the four stateful families is cut into per-connection chunks -- chunk k of connection c is what c does in dense
step k -- and a plan lists, per sparse step, some connections in some order.  A listed connection runs its next
chunk in its own slot.  A connection's results depend only on its own history, so chunk k's results in the sparse
run must equal chunk k's in the dense run whichever step it ran in and whoever ran beside it.

A family (Blocks, QpackDecode, HpackEncode, QpackSessions) knows the call layout of its generator's step dicts:
    chunk(step, c)      connection c's part of a dense step, position-free
    pack(chunks, like)  one call's step dict listing these chunks as connections 0 .. n-1 (`like`: a dense step,
                        for what every step shares: table sizes, the server name)
    records(step, r)    the results r (a dict of numpy arrays named as h2o_amd.codec returns them) as one
                        (connection record, [item record, ...]) per listed connection: decoded names and values as
                        bytes, flags, statuses, records, frame and stream bytes -- no arena or field-slot offsets,
                        which move with a block's place in the call
Plan(family, dense, slot_of, order) builds every sparse step; Plan.unmap(t, records) keys step t's records by
(connection, chunk).  numpy only: the GPU side is tests/test_conn_slots_gpu.py.
"""
import numpy as np

from h2o_amd import hpenc_synth as HE


def _off(lens, dtype=np.uint32):
    out = np.zeros(len(lens) + 1, np.uint64)
    out[1:] = np.cumsum(np.asarray(lens, np.uint64)) if len(lens) else []
    return out.astype(dtype)


def _fields(r, slot, nf):
    """the fields of one block / section: (name, value, fflags) from the arena"""
    a = r["arena"]
    out = []
    for f in range(slot, slot + nf):
        no, nl, vo, vl = (int(r[k][f]) & 0xFFFFFFFF for k in ("name_off", "name_len", "value_off", "value_len"))
        out.append((a[no:no + nl].tobytes(), a[vo:vo + vl].tobytes(), int(r["fflags"][f])))
    return tuple(out)


class Blocks:
    """HPACK header blocks: hpack_synth.make_connections / make_response_connections batches, cut by hpack_session"""
    name = "blocks"

    @staticmethod
    def chunk(step, c):
        cf, off = step["conn_first"], step["blk_off"]
        bs = range(int(cf[c]), int(cf[c + 1]))
        ch = dict(blocks=[step["data"][int(off[b]):int(off[b + 1])].tobytes() for b in bs])
        if "trailers" in step:
            ch["trailers"] = [int(step["trailers"][b]) for b in bs]
        return ch

    @staticmethod
    def pack(chunks, like):
        blocks = [b for ch in chunks for b in ch["blocks"]]
        out = dict(data=np.frombuffer(b"".join(blocks), np.uint8).copy(), blk_off=_off([len(b) for b in blocks]),
                   conn_first=_off([len(ch["blocks"]) for ch in chunks]), table_size=like["table_size"])
        if "trailers" in like:
            out["trailers"] = np.asarray([t for ch in chunks for t in ch["trailers"]], np.uint8)
        return out

    @staticmethod
    def records(step, r):
        cf, off = step["conn_first"], step["blk_off"]
        out = []
        for c in range(cf.size - 1):
            items = []
            for b in range(int(cf[c]), int(cf[c + 1])):
                rec = tuple(r[k][b].tobytes() for k in ("req", "res") if k in r)
                items.append((int(r["bstatus"][b]), int(r["nfields"][b]), _fields(r, int(off[b]), int(r["nfields"][b])), rec))
            out.append(((), items))
        return out


def hpack_session(batch, steps, seed=0, max_blocks=3):
    """a make_connections / make_response_connections batch as `steps` dense steps: every connection's blocks in
    order, 0 .. max_blocks of them a step (blocks left over are dropped)"""
    rng = np.random.default_rng(seed)
    nconn = batch["conn_first"].size - 1
    whole = [Blocks.chunk(batch, c) for c in range(nconn)]
    done = [0] * nconn
    out = []
    for _ in range(steps):
        chunks = []
        for c in range(nconn):
            n = min(int(rng.integers(0, max_blocks + 1)), len(whole[c]["blocks"]) - done[c])
            chunks.append({k: v[done[c]:done[c] + n] for k, v in whole[c].items()})
            done[c] += n
        out.append(Blocks.pack(chunks, batch))
    return out


class QpackDecode:
    """QPACK decoder steps: qpack_synth.make_session"""
    name = "qpack"

    @staticmethod
    def chunk(step, c):
        cf, off = step["conn_first"], step["sec_off"]
        e = int(step["enc_off"][c])
        ch = dict(sections=[step["data"][int(off[k]):int(off[k + 1])].tobytes() for k in range(int(cf[c]), int(cf[c + 1]))],
                  enc=step["data"][e:e + int(step["enc_len"][c])].tobytes())
        if "stream_id" in step:
            ch["stream_id"] = [int(x) for x in step["stream_id"][int(cf[c]):int(cf[c + 1])]]
        return ch

    @staticmethod
    def pack(chunks, like):
        secs = [s for ch in chunks for s in ch["sections"]]
        sec_off = _off([len(s) for s in secs])
        enc_len = np.asarray([len(ch["enc"]) for ch in chunks], np.uint32)
        enc_off = (_off(enc_len, np.uint64)[:-1] + np.uint64(sec_off[-1])).astype(np.uint32)
        out = dict(data=np.frombuffer(b"".join(secs) + b"".join(ch["enc"] for ch in chunks), np.uint8).copy(),
                   sec_off=sec_off, conn_first=_off([len(ch["sections"]) for ch in chunks]), enc_off=enc_off,
                   enc_len=enc_len, header_table_size=like["header_table_size"])
        if "stream_id" in like:
            out["stream_id"] = np.asarray([x for ch in chunks for x in ch["stream_id"]], np.uint64)
        return out

    @staticmethod
    def records(step, r):
        cf, off = step["conn_first"], step["sec_off"]
        out = []
        for c in range(cf.size - 1):
            items = []
            for k in range(int(cf[c]), int(cf[c + 1])):
                rec = tuple(r[n][k].tobytes() for n in ("req", "res") if n in r)
                items.append((int(r["sstatus"][k]), int(r["nfields"][k]), int(r["req_insert_count"][k]),
                              _fields(r, int(off[k]), int(r["nfields"][k])), rec))
            out.append(((int(r["enc_status"][c]), int(r["enc_consumed"][c]), int(r["insert_count"][c])), items))
        return out


class _Encode:
    """what the two encoder families share: response records over shared header records and strings"""
    res_extra = ()  # per-response arrays beside `res`

    @classmethod
    def chunk(cls, step, c):
        a, b = int(step["conn_first"][c]), int(step["conn_first"][c + 1])
        ch = dict(data=step["data"], hdr=step["hdr"], res=step["res"][a:b])
        for k in cls.res_extra:
            ch[k] = step[k][a:b]
        return ch

    @classmethod
    def pack(cls, chunks, like):
        # chunks of one dense step share its strings and header records as they are; chunks of several steps get
        # theirs put one behind the other, offsets and header ranges shifted
        blobs = []
        for ch in chunks:
            if not any(ch["data"] is d and ch["hdr"] is h for d, h in blobs):
                blobs.append((ch["data"], ch["hdr"]))
        if not blobs:
            blobs = [(like["data"], like["hdr"])]
        dbase = _off([d.size for d, _ in blobs], np.uint64)
        hbase = _off([h.size for _, h in blobs], np.uint64)
        hdrs = []
        for i, (d, h) in enumerate(blobs):
            h = h.copy()
            h["name_off"] += np.uint32(dbase[i])
            h["value_off"] += np.uint32(dbase[i])
            hdrs.append(h)
        res = []
        for ch in chunks:
            i = next(i for i, (d, h) in enumerate(blobs) if ch["data"] is d and ch["hdr"] is h)
            r = ch["res"].copy()
            r["hdr_first"] += np.uint32(hbase[i])
            if "dfid_off" in r.dtype.names:
                r["dfid_off"] += np.uint32(dbase[i])
            res.append(r)
        single = len(blobs) == 1
        out = dict(data=blobs[0][0] if single else np.concatenate([d for d, _ in blobs]),
                   hdr=blobs[0][1] if single else np.concatenate(hdrs),
                   res=np.concatenate(res) if res else like["res"][:0],
                   conn_first=_off([ch["res"].size for ch in chunks]),
                   server_off=int(like["server_off"]), server_len=int(like["server_len"]))
        for k in cls.res_extra:
            out[k] = np.concatenate([ch[k] for ch in chunks]) if chunks else like[k][:0]
        out["out_off"] = cls.out_offsets(out["hdr"], out["res"], out["server_len"])
        return out


class HpackEncode(_Encode):
    """HPACK encoder: hpenc_synth.make_session / make_push_session / make_request_session (every step has its own
    strings, all with the server name first)"""
    name = "hpenc"
    out_offsets = staticmethod(HE.out_offsets)

    @staticmethod
    def records(step, r):
        cf, oo = step["conn_first"], step["out_off"]
        out = []
        for c in range(cf.size - 1):
            items = []
            for k in range(int(cf[c]), int(cf[c + 1])):
                n = int(r["out_len"][k])
                items.append((int(r["rstatus"][k]), n, int(r["headers_size"][k]), r["out"][int(oo[k]):int(oo[k]) + n].tobytes()))
            out.append(((), items))
        return out


class QpackSessions(_Encode):
    """QPACK encoder sessions: hpenc_synth.to_qpack_sessions (the steps share strings and header records); a step
    may carry dec_off / dec_len (the decoder streams, in data) and gets enc_out_off from session_enc_offsets"""
    name = "qpenc"
    res_extra = ("stream_id",)
    out_offsets = staticmethod(HE.qpack_session_out_offsets)

    @classmethod
    def chunk(cls, step, c):
        ch = super().chunk(step, c)
        if "dec_off" in step:
            o = int(step["dec_off"][c])
            ch["dec"] = step["data"][o:o + int(step["dec_len"][c])].tobytes()
        return ch

    @classmethod
    def pack(cls, chunks, like):
        out = super().pack(chunks, like)
        out["enc_out_off"] = session_enc_offsets(out)
        if any("dec" in ch for ch in chunks):  # the decoder streams go behind the strings
            dec = [ch.get("dec", b"") for ch in chunks]
            out["dec_len"] = np.asarray([len(d) for d in dec], np.uint32)
            out["dec_off"] = (_off(out["dec_len"], np.uint64)[:-1] + np.uint64(out["data"].size)).astype(np.uint32)
            out["data"] = np.concatenate([out["data"], np.frombuffer(b"".join(dec), np.uint8)])
        return out

    @staticmethod
    def records(step, r):
        cf, oo, eo = step["conn_first"], step["out_off"], step["enc_out_off"]
        out = []
        for c in range(cf.size - 1):
            items = []
            for k in range(int(cf[c]), int(cf[c + 1])):
                n = int(r["out_len"][k])
                items.append((int(r["rstatus"][k]), int(r["rflags"][k]), n, int(r["header_len"][k]),
                              r["out"][int(oo[k]):int(oo[k]) + n].tobytes()))
            n = int(r["enc_out_len"][c])
            out.append(((int(r["dec_status"][c]), int(r["dec_consumed"][c]), r["enc_out"][int(eo[c]):int(eo[c]) + n].tobytes()),
                        items))
        return out


def session_enc_offsets(step):
    """[nconn + 1] u64 encoder-stream regions, 16-byte aligned: room for Set Dynamic Table Capacity and for an
    insert of every header and of the server name of every response of the connection (above
    hhuff_qpack_session_enc_bound, which counts only the likely-to-repeat headers)"""
    hdr, res, cf = step["hdr"], step["res"], step["conn_first"]
    nv = hdr["name_len"].astype(np.int64) + hdr["value_len"] + 20
    csum = np.concatenate([[0], np.cumsum(nv)])
    first = res["hdr_first"].astype(np.int64)
    per = csum[first + res["nhdr"]] - csum[first] + 26 + int(step["server_len"])
    rsum = np.concatenate([[0], np.cumsum(per)])
    b = 4 + rsum[cf[1:].astype(np.int64)] - rsum[cf[:-1].astype(np.int64)]
    return _off((b + 15) // 16 * 16, np.uint64)


class Plan:
    """dense: list of dense step dicts of `family`; slot_of[c]: connection c's slot (injective); order: per sparse
    step the connections it lists, in call order.  steps[t] = (the call's step dict, slot u32[n], [(c, chunk)])"""

    def __init__(self, family, dense, slot_of, order):
        slot_of = np.asarray(slot_of, np.uint32)
        assert np.unique(slot_of).size == slot_of.size, "the slot map must be injective"
        self.family = family
        nconn = dense[0]["conn_first"].size - 1
        cursor = [0] * nconn
        self.steps = []
        for conns in order:
            conns = [int(c) for c in conns]
            assert len(set(conns)) == len(conns) and all(cursor[c] < len(dense) for c in conns)
            keys = [(c, cursor[c]) for c in conns]
            for c in conns:
                cursor[c] += 1
            chunks = [family.chunk(dense[k], c) for c, k in keys]
            self.steps.append((family.pack(chunks, dense[0]), slot_of[conns] if conns else slot_of[:0], keys))

    def unmap(self, t, records):
        """records = family.records of step t's results -> {(connection, chunk): (connection record, items)}"""
        keys = self.steps[t][2]
        assert len(records) == len(keys)
        return dict(zip(keys, records))


def dense_records(family, dense, results):
    """the dense run's records under the same keys: {(connection, step): ...}"""
    out = {}
    for k, (step, r) in enumerate(zip(dense, results)):
        for c, rec in enumerate(family.records(step, r)):
            out[(c, k)] = rec
    return out
