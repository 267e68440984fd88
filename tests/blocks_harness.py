"""Hand-built HPACK header blocks and QPACK sessions, exact-size guarded calls and a checker -- plain helpers, no
GPU.  hpack_synth / qpack_synth model browser traffic; the builders here emit one representation each, so a case
can aim at an edge of the integer decoder, the dynamic table, the arena contract or the literal pre-pass.

  builders     integer / string / indexed / literal / size_update (RFC 7541) and the QPACK encoder-stream
               instructions, section prefix and field lines (RFC 9204)
  batches      a corpus is a list of named cases, a case a list of connections; batch() packs them (repeated in
               varying orders up to a connection count, one-block connections with an empty block in between) into
               the arrays of include/hhuff.h, one set per call
  expected()   the oracle's results in each call's own layout (the restatement or the compiled reference)
  run()        every call on exact-size arrays between guards, twice (bounds_harness.RUNS); between two calls the
               previous call's input, arena and per-slot outputs are overwritten and the scratch is moved
  check_call() guards, statuses, fields, bytes, records; nothing outside a block's own arena slice written

An implementation is an object with call(a) and poison(): GpuBlocks (libhhuff through h2o_amd.codec.lib()) or
OracleBlocks (the oracle itself, or one of its faulty variants: the harness has to catch those)."""
import ctypes

import numpy as np

from bounds_harness import EXTRA, GUARD, RUNS, entries, guarded, huffman, text_for_huffman_len, to_device
from h2o_amd import hpack_synth as HS

POISON = 0x5A
ARENA, SKIPPED, COMPRESSION, PROTOCOL, INVALID_CHAR = -300, -301, -9, -1, -254
SPACER_SLICE = 48  # arena bytes of a spacer connection's empty block: written by nobody
SLOT_ARRAYS = (("name_off", np.uint32), ("name_len", np.uint32), ("value_off", np.uint32), ("value_len", np.uint32),
               ("fflags", np.uint8))
RECORD_WORDS = {"req": 12, "res": 4, "qreq": 18, "qres": 10}  # hhuff_request_t / _response_t / _qpack_request_t /
# _qpack_response_head_t as u32 words
DTYPES = {"arena": np.uint8, "bstatus": np.int32, "sstatus": np.int32, "enc_status": np.int32,
          "req_insert_count": np.uint64, "insert_count": np.uint64}  # every other output array is u32


# ------------------------------------------------------------------------------------------------
# builders (RFC 7541 6.x)
# ------------------------------------------------------------------------------------------------
def integer(value, prefix_bits, first=0, nbytes=None):
    """prefix integer; nbytes forces the total byte count: the prefix is full and the rest is padded with 0x80
    continuation octets (a non-minimal encoding of the same value)"""
    if nbytes is None:
        return HS.encode_int(value, prefix_bits, first)
    mx = (1 << prefix_bits) - 1
    assert value >= mx and nbytes >= 2
    rest, out = value - mx, [first | mx]
    for k in range(nbytes - 1):
        out.append((rest & 127) | (0x80 if k < nbytes - 2 else 0))
        rest >>= 7
    assert rest == 0, "value does not fit %d bytes" % nbytes
    return bytes(out)


def raw_string(payload, h=False, nbytes=None):
    """a string literal with the H bit as given, whatever the payload is"""
    return integer(len(payload), 7, 0x80 if h else 0, nbytes) + payload


def string(s, huff=None, nbytes=None):
    """huff None: as h2o's encoder chooses; True / False: forced"""
    if huff is None:
        return HS.encode_string(s)
    return raw_string(huffman(s) if huff else s, huff, nbytes)


def indexed(i, nbytes=None):
    return integer(i, 7, 0x80, nbytes)


def literal(name, value, how="inc"):
    """name: a table index or an encoded string; value: an encoded string (b"" cuts the field after its name);
    how: "inc" (incremental indexing), "without", "never" """
    first, bits = {"inc": (0x40, 6), "without": (0x00, 4), "never": (0x10, 4)}[how]
    if isinstance(name, int):
        return integer(name, bits, first) + value
    return bytes([first]) + name + value


def size_update(n, nbytes=None):
    return integer(n, 5, 0x20, nbytes)


def huff_of_len(rng, L, need_pad=False):
    """a valid Huffman string of exactly L bytes (need_pad: its last byte ends in at least one padding bit)"""
    if need_pad and L == 1:
        return huffman(b"e")  # five bits and three of padding
    for _ in range(200):
        h = huffman(text_for_huffman_len(rng, L))
        assert len(h) == L
        if not need_pad or L == 0:
            return h
        # padding present <=> clearing the last bit makes the oracle reject it
        from oracle import oracle as O

        if O.oracle().decode(h[:-1] + bytes([h[-1] & 0xFE]))[0] is None:
            return h
    raise AssertionError("no padded Huffman string of %d bytes" % L)


def huff_variants(rng, L):
    """-> [(tag, payload)]: a valid Huffman string of L bytes and, the defect in its last byte(s): eight bits of
    padding, a zero bit in the padding, EOS"""
    from oracle import oracle as O

    dec = lambda p: O.oracle().decode(p)[0]  # noqa: E731
    ok = huff_of_len(rng, L, need_pad=True)
    out = [("ok", ok)]
    assert dec(ok) is not None
    if L >= 1:
        out.append(("pad8", huff_of_len(rng, L - 1) + b"\xff"))
        out.append(("pad0", ok[:-1] + bytes([ok[-1] & 0xFE])))
    if L >= 5:
        out.append(("eos", huff_of_len(rng, L - 4) + b"\xff\xff\xff\xff"))
    for tag, p in out[1:]:
        assert len(p) == L and dec(p) is None, (tag, L)
    return out


# ------------------------------------------------------------------------------------------------
# cases and batches
# ------------------------------------------------------------------------------------------------
def case(name, *conns, arena=None, ent=64, room=0, trailers=()):
    """one call: every connection is a list of blocks.  trailers: the (conn, call, block) that are trailers blocks in
    response mode (hhuff_hpack_parse_responses' trailers array; no case with any: the call passes NULL).  arena: {(conn, call, block): bytes} overrides of the
    default slice (floor(8 L / 5) + L * ent + 64 + room for a block of L bytes: a field takes at least one byte and
    an indexed one copies at most ent bytes; room: for the few fields that copy more)"""
    return dict(name=name, conns=[[list(c)] for c in conns], arena=arena or {}, ent=ent, room=room, trailers=set(trailers))


def ccase(name, *conns, arena=None, ent=64, room=0, trailers=()):
    """several calls: every connection is a list (one entry per call) of lists of blocks"""
    return dict(name=name, conns=[[list(b) for b in c] for c in conns], arena=arena or {}, ent=ent, room=room,
                trailers=set(trailers))


def default_slice(L, ent, room=0):
    return (8 * L) // 5 + L * ent + 64 + room


def batch(cases, table_size, nconn=None, seed=0, spacers=True, arena_base=0, tail=0):
    """The arrays of every call of a batch.  The cases' connections in order (nconn None) or repeated in a new order
    each round until there are nconn connections; with spacers, every second connection is a one-block connection
    whose block is empty: it owns an arena slice (SPACER_SLICE bytes) that nothing may write.  arena_base =
    arena_off[0]; tail = input bytes behind the last block (in_size - blk_off[nblk]).
    -> dict(table_size, nconn, calls=[dict(data, in_size, blk_off, conn_first, arena_off, labels, nblk[, trailers])])"""
    rng = np.random.default_rng(seed)
    ncalls = max(len(c) for k in cases for c in k["conns"])
    conns = []  # (label, per-call block lists, per-call slice lists, per-call trailers flags)
    any_trailers = any(k.get("trailers") for k in cases)
    rounds = 0
    while True:
        order = np.arange(len(cases)) if rounds == 0 else rng.permutation(len(cases))
        for ci in order:
            k = cases[ci]
            for j, c in enumerate(k["conns"]):
                per_call = [list(c[i]) if i < len(c) else [] for i in range(ncalls)]
                slices = [[k["arena"].get((j, i, b), default_slice(len(blk), k["ent"], k["room"]))
                           for b, blk in enumerate(bl)] for i, bl in enumerate(per_call)]
                tr = [[int((j, i, b) in k.get("trailers", ())) for b in range(len(bl))] for i, bl in enumerate(per_call)]
                conns.append((k["name"], per_call, slices, tr))
                if spacers:
                    conns.append(("spacer", [[b""]] * ncalls, [[SPACER_SLICE]] * ncalls, [[0]] * ncalls))
        rounds += 1
        if nconn is None or len(conns) >= nconn:
            break
    if nconn is not None:
        conns = conns[:nconn]
    calls = []
    for i in range(ncalls):
        blocks, labels, sizes, conn_first, trailers = [], [], [], [0], []
        for label, per_call, slices, tr in conns:
            blocks += per_call[i]
            sizes += slices[i]
            trailers += tr[i]
            labels += ["%s[call %d block %d]" % (label, i, b) for b in range(len(per_call[i]))]
            conn_first.append(len(blocks))
        blk_off = np.zeros(len(blocks) + 1, np.uint64)
        blk_off[1:] = np.cumsum([len(b) for b in blocks])
        arena_off = np.full(len(blocks) + 1, arena_base, np.uint64)
        arena_off[1:] += np.cumsum(np.asarray(sizes, np.uint64))
        data = np.frombuffer(b"".join(blocks) + bytes(tail), np.uint8).copy()
        assert int(arena_off[-1]) < 2 ** 32 and data.size < 2 ** 31
        calls.append(dict(data=data, in_size=int(data.size), blk_off=blk_off.astype(np.uint32),
                          conn_first=np.asarray(conn_first, np.uint32), arena_off=arena_off, labels=labels,
                          nblk=len(blocks)))
        if any_trailers:
            calls[-1]["trailers"] = np.asarray(trailers, np.uint8)
    return dict(table_size=table_size, nconn=len(conns), calls=calls)


# ------------------------------------------------------------------------------------------------
# the oracle's results in every call's own layout
# ------------------------------------------------------------------------------------------------
def _empty_result(cl, mode):
    nslot, nblk = cl["in_size"], cl["nblk"]
    r = dict(arena=np.zeros(int(cl["arena_off"][-1]), np.uint8), nfields=np.zeros(nblk, np.uint32),
             bstatus=np.zeros(nblk, np.int32), used=np.zeros(nblk, np.int64))
    for k, dt in SLOT_ARRAYS:
        r[k] = np.zeros(nslot, dt)
    if mode in RECORD_WORDS:
        r[mode] = np.zeros((nblk, RECORD_WORDS[mode]), np.uint32)
    return r


def combined_run(codec, calls, table_size, modes, extra=0):
    """The calls' blocks decoded connection by connection in one oracle run per mode (the oracle keeps no tables
    between runs; the blocks of a plain-mode call take no part in a request / response run's rules, as in the
    continuation they stand for), every block with an arena slice of its own call's size (+ extra), and the results put back into
    each call's layout: offsets relative to the call's arena_off, slots at the call's blk_off.  "used" = bytes of
    each block's slice its fields take."""
    ncalls, nconn = len(calls), len(calls[0]["conn_first"]) - 1
    blocks, where, conn_first, trailers, plain = [], [], [0], [], []
    for c in range(nconn):
        for i, cl in enumerate(calls):
            cf, bo = cl["conn_first"], cl["blk_off"]
            for b in range(int(cf[c]), int(cf[c + 1])):
                blocks.append(cl["data"][int(bo[b]):int(bo[b + 1])].tobytes())
                where.append((i, b))
                trailers.append(int(cl["trailers"][b]) if cl.get("trailers") is not None else 0)
                plain.append(int(modes[i] in (None, "plain")))
        conn_first.append(len(blocks))
    pk = HS.pack_connections([blocks[conn_first[c]:conn_first[c + 1]] for c in range(nconn)])
    sizes = np.asarray([int(calls[i]["arena_off"][b + 1]) - int(calls[i]["arena_off"][b]) + extra for i, b in where],
                       np.uint64)
    cao = np.zeros(len(blocks) + 1, np.uint64)
    cao[1:] = np.cumsum(sizes)
    assert int(cao[-1]) < 2 ** 32
    runs = {}
    for m in set(modes):
        runs[m] = codec.hpack_decode_blocks(pk["data"], pk["blk_off"], pk["conn_first"], table_size, arena_off=cao,
                                            nthreads=8, requests=m == "req", responses=m == "res",
                                            trailers=np.asarray(trailers, np.uint8) if m == "res" and any(trailers)
                                            else None,
                                            plain=np.asarray(plain, np.uint8) if m in ("req", "res") and any(plain)
                                            else None)
    out = [_empty_result(cl, modes[i]) for i, cl in enumerate(calls)]
    for g, (i, b) in enumerate(where):
        r, o, cl = runs[modes[i]], out[i], calls[i]
        nf = int(r["nfields"][g])
        o["nfields"][b], o["bstatus"][b] = nf, r["bstatus"][g]
        s, d = int(pk["blk_off"][g]), int(cl["blk_off"][b])
        shift = int(cl["arena_off"][b]) - int(cao[g])
        for k, _ in SLOT_ARRAYS:
            v = r[k][s:s + nf]
            o[k][d:d + nf] = v + np.uint32(shift & 0xFFFFFFFF) if k.endswith("_off") else v
        if nf:
            end = max(int((r["name_off"][s:s + nf].astype(np.int64) + r["name_len"][s:s + nf]).max()),
                      int((r["value_off"][s:s + nf].astype(np.int64) + r["value_len"][s:s + nf]).max()))
            used = end - int(cao[g])
            o["used"][b] = used
            if not extra:
                o["arena"][int(cl["arena_off"][b]):int(cl["arena_off"][b]) + used] = r["arena"][int(cao[g]):end]
            else:
                o.setdefault("wide", {})[b] = r["arena"][int(cao[g]):end].copy()
        if modes[i] in RECORD_WORDS:
            o[modes[i]][b] = np.ascontiguousarray(r[modes[i]][g:g + 1]).view(np.uint32).reshape(-1)
    return out


def expected(codec, bt, modes):
    return combined_run(codec, bt["calls"], bt["table_size"], modes)


# ------------------------------------------------------------------------------------------------
# the guarded call
# ------------------------------------------------------------------------------------------------
def _poisoned(vals, dtype, lo, hi):
    a = np.empty(len(vals) + EXTRA, dtype)
    a[:len(vals)] = vals
    a[len(vals):] = [lo if j % 2 == 0 else hi for j in range(EXTRA)]
    return a


def call_args(cl, table_size, nconn, mode, cont, fill, sentinel):
    """One call's arrays: the input between guards of `fill`; blk_off, conn_first and arena_off followed by EXTRA
    in-range poisoned entries; every output array of exactly its contractual size between guards of `sentinel`:
    the arena arena_off[nblk] bytes, the per-slot arrays in_size entries, nfields / bstatus / req / res nblk"""
    whole, inner = guarded(np, cl["in_size"], fill)
    inner[:] = cl["data"]
    nblk, n = cl["nblk"], cl["in_size"]
    out = {"arena": guarded(np, int(cl["arena_off"][-1]), sentinel)[0], "nfields": guarded(np, 4 * nblk, sentinel)[0],
           "bstatus": guarded(np, 4 * nblk, sentinel)[0]}
    for k, dt in SLOT_ARRAYS:
        out[k] = guarded(np, n * np.dtype(dt).itemsize, sentinel)[0]
    if mode in RECORD_WORDS:
        out[mode] = guarded(np, 4 * RECORD_WORDS[mode] * nblk, sentinel)[0]
    return dict(in_whole=whole, data=inner, in_size=n, nblk=nblk, nconn=nconn, table_size=table_size, mode=mode,
                cont=cont, labels=cl["labels"], sentinel=sentinel,
                blk_off=_poisoned(cl["blk_off"], np.uint32, 0, n),
                conn_first=_poisoned(cl["conn_first"], np.uint32, 0, nblk),
                arena_off=_poisoned(cl["arena_off"], np.uint64, int(cl["arena_off"][0]), int(cl["arena_off"][-1])),
                trailers=_poisoned(cl["trailers"], np.uint8, 0, 1) if cl.get("trailers") is not None else None,
                out=out, scratch_guards=None)


def out_view(a, name):
    dt = dict(SLOT_ARRAYS).get(name, DTYPES.get(name, np.uint32))
    return entries(a["out"][name], dt)


def run(impl_factory, bt, modes, check=None, poison=True):
    """Every call of the batch through impl_factory(sentinel), twice (RUNS).  After a call's results are copied out
    (and checked: check(a, call index, sentinel)), its input, arena and per-slot outputs are overwritten in place with
    POISON and impl.poison() does the same on its side and moves the scratch; only then comes the next call.
    -> the calls' argument dicts of the last run (outputs copied)"""
    done = []
    for fill, sentinel in RUNS:
        impl = impl_factory(sentinel)
        done = []
        for i, cl in enumerate(bt["calls"]):
            a = call_args(cl, bt["table_size"], bt["nconn"], modes[i], i > 0, fill, sentinel)
            impl.call(a)
            kept = dict(a, out={k: v.copy() for k, v in a["out"].items()})
            if check is not None:
                check(kept, i, sentinel)
            done.append(kept)
            if poison:
                a["in_whole"][:] = POISON
                for k in ("arena",) + tuple(k for k, _ in SLOT_ARRAYS):
                    a["out"][k][:] = POISON
                impl.poison()
    return done


# ------------------------------------------------------------------------------------------------
# the check
# ------------------------------------------------------------------------------------------------
def _ranges(starts, lens):
    """the concatenation of arange(s, s + l)"""
    starts, lens = np.asarray(starts, np.int64), np.asarray(lens, np.int64)
    total = int(lens.sum())
    return np.repeat(starts, lens) + (np.arange(total) - np.repeat(np.cumsum(lens) - lens, lens))


def check_call(a, exp, label="", records=True):
    """a: a call's arguments with its outputs filled in; exp: the oracle's result for the call (expected()).
      - every guard intact (the scratch's too, where the implementation reports them)
      - nfields and bstatus equal, block by block
      - the first nfields[b] slots of every block: offsets, lengths, fflags and the bytes equal
      - request / response records equal word for word
      - per-slot entries outside [blk_off[0], blk_off[nblk]) and arena bytes outside the slices of non-empty blocks
        (before arena_off[0], the slices of empty blocks) still hold the sentinel
    Slots past nfields[b] and the bytes of a block's slice its fields do not cover are unspecified."""
    sentinel, nblk, labels = a["sentinel"], a["nblk"], a["labels"]

    def fail(msg, b=None):
        raise AssertionError("%s%s: %s" % (label, "" if b is None else " " + labels[b], msg))

    for name, whole in a["out"].items():
        for side, g in (("front", whole[:GUARD]), ("rear", whole[whole.size - GUARD:])):
            hit = np.nonzero(g != sentinel)[0]
            if hit.size:
                fail("%s: %s guard byte %d written (%#x)" % (name, side, hit[0], g[hit[0]]))
    if a["scratch_guards"] is not None and (a["scratch_guards"] != sentinel).any():
        fail("a scratch guard byte was written")
    bo = a["blk_off"][:nblk + 1].astype(np.int64)
    ao = a["arena_off"][:nblk + 1].astype(np.int64)
    for name in a.get("exact", ("nfields", "bstatus")):  # per block / section, or (QPACK) per connection
        got, want = out_view(a, name), exp[name]
        bad = np.nonzero(got != want)[0]
        if bad.size:
            per_block = name in ("nfields", "bstatus", "sstatus", "req_insert_count")
            fail("%s%s = %d, oracle %d (%d differ)" % (name, "" if per_block else " of connection %d" % bad[0],
                                                      got[bad[0]], want[bad[0]], bad.size),
                 int(bad[0]) if per_block else None)
    nf = exp["nfields"].astype(np.int64)
    slots = _ranges(bo[:-1], nf)
    blk_of = np.repeat(np.arange(nblk), nf)
    for name, _ in SLOT_ARRAYS:
        got, want = out_view(a, name)[slots], exp[name][slots]
        bad = np.nonzero(got != want)[0]
        if bad.size:
            b = int(blk_of[bad[0]])
            fail("%s of field %d = %#x, oracle %#x (%d slots differ)"
                 % (name, slots[bad[0]] - bo[b], got[bad[0]], want[bad[0]], bad.size), b)
        rest = np.ones(a["in_size"], bool)
        rest[int(bo[0]):int(bo[-1])] = False
        if (out_view(a, name)[rest] != (sentinel if name == "fflags" else 0x01010101 * sentinel)).any():
            fail("%s written outside the blocks' slots" % name)
    arena = out_view(a, "arena")
    for offk, lenk in (("name_off", "name_len"), ("value_off", "value_len")):
        st, ln = exp[offk][slots].astype(np.int64), exp[lenk][slots].astype(np.int64)
        out_of = np.nonzero((st < ao[blk_of]) | (st + ln > ao[blk_of + 1]))[0]
        if out_of.size:
            fail("the oracle's %s leaves the block's slice" % offk, int(blk_of[out_of[0]]))
        pos = _ranges(st, ln)
        bad = np.nonzero(arena[pos] != exp["arena"][pos])[0]
        if bad.size:
            f = int(np.searchsorted(np.cumsum(ln), bad[0], side="right"))
            b = int(blk_of[f])
            fail("%s bytes of field %d differ at arena byte %d: %#x, oracle %#x (%d bytes)"
                 % (offk[:-4], slots[f] - bo[b], pos[bad[0]], arena[pos[bad[0]]], exp["arena"][pos[bad[0]]], bad.size), b)
    owned = np.zeros(arena.size + 1, np.int32)
    full = np.nonzero(bo[1:] > bo[:-1])[0]
    np.add.at(owned, ao[full], 1)
    np.add.at(owned, ao[full + 1], -1)
    stray = np.nonzero((np.cumsum(owned)[:arena.size] == 0) & (arena != sentinel))[0]
    if stray.size:
        b = int(np.searchsorted(ao, stray[0], side="right")) - 1
        fail("arena byte %d, which belongs to no non-empty block, was written: %#x (%d bytes)"
             % (stray[0], arena[stray[0]], stray.size), b if 0 <= b < nblk else None)
    if records and a["mode"] in RECORD_WORDS:
        w = RECORD_WORDS[a["mode"]]
        got = entries(a["out"][a["mode"]], np.uint32).reshape(nblk, w)
        bad = np.nonzero((got != exp[a["mode"]]).any(axis=1))[0]
        if bad.size:
            b = int(bad[0])
            fail("%s record %s, oracle %s" % (a["mode"], got[b].tolist(), exp[a["mode"]][b].tolist()), b)


# ------------------------------------------------------------------------------------------------
# implementations
# ------------------------------------------------------------------------------------------------
class OracleBlocks:
    """The oracle as an implementation of the call sequence: call i decodes the blocks of calls 0..i (the oracle has no
    HHUFF_BLK_CONTINUE) and writes call i's part into the caller's arrays.  Faulty variants, which the harness has
    to catch:
      "arena+1"   one byte written just past a block's arena slice
      "slot+1"    the slot past in_size written
      "stale"     earlier calls' blocks are read from the caller's input buffers at the time of the later call (a
                  table entry that still points at the previous call's input), not from a copy
      "huff_len"  a Huffman literal's arena room checked against its decoded length, not floor(8 len / 5)"""

    def __init__(self, codec, fault=None):
        self.codec, self.fault, self.history = codec, fault, []

    def poison(self):
        pass

    def call(self, a):
        nblk, nconn = a["nblk"], a["nconn"]
        data = a["data"] if self.fault == "stale" else a["data"].copy()
        self.history.append(dict(data=data, blk_off=a["blk_off"][:nblk + 1].copy(), in_size=a["in_size"], nblk=nblk,
                                 conn_first=a["conn_first"][:nconn + 1].copy(),
                                 arena_off=a["arena_off"][:nblk + 1].copy(), mode=a["mode"],
                                 trailers=None if a.get("trailers") is None else a["trailers"][:nblk].copy()))
        modes = [h["mode"] for h in self.history]
        if self.fault == "huff_len":
            r = self._by_decoded_length(a)
        else:
            r = combined_run(self.codec, self.history, a["table_size"], modes)[-1]
        ao = a["arena_off"][:nblk + 1].astype(np.int64)
        bo = a["blk_off"][:nblk + 1].astype(np.int64)
        arena = out_view(a, "arena")
        for b in range(nblk):
            u = int(r["used"][b])
            arena[ao[b]:ao[b] + u] = r["arena"][ao[b]:ao[b] + u]
            nf = int(r["nfields"][b])
            for k, _ in SLOT_ARRAYS:
                out_view(a, k)[bo[b]:bo[b] + nf] = r[k][bo[b]:bo[b] + nf]
        out_view(a, "nfields")[:] = r["nfields"]
        out_view(a, "bstatus")[:] = r["bstatus"]
        if a["mode"] in RECORD_WORDS:
            entries(a["out"][a["mode"]], np.uint32)[:] = r[a["mode"]].reshape(-1)
        if self.fault == "arena+1":
            b = next(b for b in range(nblk) if bo[b + 1] > bo[b] and (b + 1 == nblk or bo[b + 2] == bo[b + 1]))
            a["out"]["arena"][GUARD + ao[b + 1]] ^= 0xFF
        if self.fault == "slot+1":
            a["out"]["name_off"][GUARD + 4 * a["in_size"]] ^= 0xFF

    def _by_decoded_length(self, a):
        """every string's room checked against the bytes it takes: decode with slices wide enough for any need, then
        cut each block at the first field that ends past the block's real slice"""
        modes = [h["mode"] for h in self.history]
        wide = combined_run(self.codec, self.history, a["table_size"], modes, extra=1 << 17)
        # connections that met HHUFF_BLK_ARENA in an earlier call stay failed
        dead = getattr(self, "dead", set())
        r, cl = wide[-1], self.history[-1]
        ao, bo = cl["arena_off"].astype(np.int64), cl["blk_off"].astype(np.int64)
        for c in range(a["nconn"]):
            for b in range(int(cl["conn_first"][c]), int(cl["conn_first"][c + 1])):
                if c in dead:
                    r["nfields"][b], r["bstatus"][b], r["used"][b] = 0, SKIPPED, 0
                    continue
                nf, s = int(r["nfields"][b]), int(bo[b])
                ends = np.maximum(r["name_off"][s:s + nf].astype(np.int64) + r["name_len"][s:s + nf],
                                  r["value_off"][s:s + nf].astype(np.int64) + r["value_len"][s:s + nf])
                over = np.nonzero(ends > ao[b + 1])[0]
                if over.size:
                    nf = int(over[0])
                    r["nfields"][b], r["bstatus"][b] = nf, ARENA
                    r["used"][b] = int(ends[nf - 1] - ao[b]) if nf else 0
                    dead.add(c)
                elif r["bstatus"][b] not in (0, INVALID_CHAR):
                    dead.add(c)
                u = int(r["used"][b])
                r["arena"][ao[b]:ao[b] + u] = r.get("wide", {}).get(b, np.zeros(0, np.uint8))[:u]
        self.dead = dead
        return r


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _inner(pair):
    """the address of a guarded device buffer's inner part (an empty tensor's data_ptr() is NULL)"""
    return ctypes.c_void_p(pair[0].data_ptr() + GUARD)


class GpuBlocks:
    """hhuff_hpack_decode_blocks / _parse_requests / _parse_responses through h2o_amd.codec.lib() on guarded device
    arrays; the scratch has exactly hhuff_hpack_scratch_size bytes between guards and moves to a new buffer in
    poison(), the old one overwritten and kept allocated."""

    def __init__(self, torch, sentinel):
        from h2o_amd import codec

        self.torch, self.lib, self.sentinel = torch, codec.lib(), sentinel
        self.scratch = None
        self.keep, self.last = [], None

    def call(self, a):
        torch, L = self.torch, self.lib
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).cuda()  # noqa: E731
        inp = to_device(torch, a["in_whole"])
        in_whole = inp[0]
        blk_off, conn_first, arena_off = dev(a["blk_off"]), dev(a["conn_first"]), dev(a["arena_off"])
        out = {k: to_device(torch, v) for k, v in a["out"].items()}
        ss = int(L.hhuff_hpack_scratch_size(a["nconn"], a["table_size"]))
        if self.scratch is None:
            self.scratch = guarded(torch, ss, self.sentinel)
        o = lambda k: _inner(out[k])  # noqa: E731
        args = [_inner(inp), a["in_size"], _vp(blk_off), _vp(conn_first), a["nconn"], a["table_size"], o("arena"),
                _vp(arena_off), o("name_off"), o("name_len"), o("value_off"), o("value_len"), o("fflags"), o("nfields"),
                o("bstatus")]
        tail = [_inner(self.scratch), ss, 1 if a["cont"] else 0, None]
        if a["mode"] == "res":
            trailers = None if a.get("trailers") is None else dev(a["trailers"])
            rc = L.hhuff_hpack_parse_responses(*args[:6], None if trailers is None else _vp(trailers), *args[6:],
                                               o("res"), *tail)
        elif a["mode"] == "req":
            rc = L.hhuff_hpack_parse_requests(*args, o("req"), *tail)
        else:
            rc = L.hhuff_hpack_decode_blocks(*args, *tail)
        assert rc == 0, "the call returned %d: %s" % (rc, L.hhuff_last_error_string())
        torch.cuda.synchronize()
        for k, (whole, _) in out.items():
            a["out"][k][:] = whole.cpu().numpy()
        w = self.scratch[0].cpu().numpy()
        a["scratch_guards"] = np.concatenate([w[:GUARD], w[w.size - GUARD:]])
        self.last = [in_whole] + [out[k][0] for k in ("arena",) + tuple(k for k, _ in SLOT_ARRAYS)]
        self.keep.append((blk_off, conn_first, arena_off, out, trailers if a["mode"] == "res" else None))

    def poison(self):
        for t in self.last:  # overwritten in place: they stay allocated, a stale offset would read the pattern
            t.fill_(POISON)
        self.keep.append(self.last)
        old = self.scratch
        self.scratch = guarded(self.torch, old[1].numel(), self.sentinel)
        self.scratch[1].copy_(old[1])
        old[0].fill_(POISON)
        self.keep.append(old)
        self.torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# summaries: what the reference reports too (it keeps one soft-error code per field, name first)
# ------------------------------------------------------------------------------------------------
def soft_code(bits):
    bits = np.asarray(bits)
    return np.where(bits & 1, 1, np.where(bits & 2, 2, 0)).astype(np.uint8)


def result_of(a):
    """a call's outputs as the arrays expected() returns"""
    r = {k: out_view(a, k) for k in ("arena", "nfields", "bstatus") + tuple(k for k, _ in SLOT_ARRAYS)}
    if a["mode"] in RECORD_WORDS:
        r[a["mode"]] = entries(a["out"][a["mode"]], np.uint32).reshape(a["nblk"], RECORD_WORDS[a["mode"]])
    return r


def summary(results, bt, modes):
    """-> {key: array}: per call the statuses, the decoded fields' bytes and lengths in block order, one soft-error code
    and the header-list flag per field, and the request / response records"""
    out = {}
    for i, (e, cl) in enumerate(zip(results, bt["calls"])):
        nblk = cl["nblk"]
        nf = np.asarray(e["nfields"][:nblk]).astype(np.int64)
        slots = _ranges(cl["blk_off"][:nblk].astype(np.int64), nf)
        out["%d_nfields" % i] = nf.astype(np.uint32)
        out["%d_bstatus" % i] = np.asarray(e["bstatus"][:nblk]).astype(np.int32)
        for which in ("name", "value"):
            st, ln = e[which + "_off"][slots].astype(np.int64), e[which + "_len"][slots].astype(np.int64)
            out["%d_%s" % (i, which)] = np.asarray(e["arena"])[_ranges(st, ln)]
            out["%d_%s_len" % (i, which)] = ln.astype(np.uint32)
        fl = np.asarray(e["fflags"])[slots]
        out["%d_soft" % i] = soft_code(fl & 3)
        out["%d_header" % i] = (fl & 4).astype(np.uint8)
        if modes[i] in RECORD_WORDS:
            out["%d_%s" % (i, modes[i])] = np.ascontiguousarray(e[modes[i]][:nblk]).view(np.uint32).reshape(
                nblk, RECORD_WORDS[modes[i]])
    return out


def assert_same_summary(got, want, label=""):
    assert set(got) == set(want), label
    for k in sorted(want, key=lambda k: (int(k.split("_")[0]), not k.endswith(("nfields", "bstatus")), k)):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.shape != w.shape or (g != w).any():
            bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0] if g.shape == w.shape else []
            raise AssertionError("%s: %s differs (shapes %s / %s, first at %s)"
                                 % (label, k, g.shape, w.shape, bad[0] if len(bad) else "-"))


# ------------------------------------------------------------------------------------------------
# QPACK (RFC 9204): builders, sessions, the guarded step
# ------------------------------------------------------------------------------------------------
def qstr(payload, prefix_bits, first=0, h=False, nbytes=None):
    """a QPACK string literal: the H bit just above the length prefix, whatever the payload is"""
    return integer(len(payload), prefix_bits, first | ((1 << prefix_bits) if h else 0), nbytes) + payload


def q_set_capacity(n, nbytes=None):
    return integer(n, 5, 0x20, nbytes)


def q_insert_ref(index, value, static=False):
    """Insert With Name Reference; value: an encoded 7-bit-prefix string"""
    return integer(index, 6, 0x80 | (0x40 if static else 0)) + value


def q_insert(name, value, h=False):
    """Insert With Literal Name; name: the payload (h: it is Huffman coded), value: an encoded string"""
    return qstr(name, 5, 0x40, h) + value


def q_duplicate(index):
    return integer(index, 5, 0x00)


def q_prefix(ric, base, max_entries):
    """the section prefix: Required Insert Count (RFC 9204 4.5.1.1) and Base"""
    out = b"\x00" if ric == 0 else integer(ric % (2 * max_entries) + 1, 8)
    return out + (integer(base - ric, 7, 0) if base >= ric else integer(ric - base - 1, 7, 0x80))


def q_indexed(index, static=False):
    return integer(index, 6, 0x80 | (0x40 if static else 0))


def q_indexed_post(index):
    return integer(index, 4, 0x10)


def q_literal_ref(index, value, static=False, never=False):
    return integer(index, 4, 0x40 | (0x20 if never else 0) | (0x10 if static else 0)) + value


def q_literal_post(index, value, never=False):
    return integer(index, 3, 0x08 if never else 0) + value


def q_literal(name, value, h=False, never=False):
    """Literal Field Line With Literal Name; name: the payload, value: an encoded string"""
    return qstr(name, 3, 0x20 | (0x10 if never else 0), h) + value


def qcase(name, *conns, arena=None, ent=80, room=0, blocked=0):
    """every connection: a list over steps of (encoder-stream buffer, [sections]); blocked = its num_blocked"""
    return dict(name=name, conns=[[(e, list(s)) for e, s in c] for c in conns], arena=arena or {}, ent=ent, room=room,
                blocked=blocked)


def qbatch(cases, header_table_size, max_blocked, nconn=None, seed=0, spacers=True, arena_base=0):
    """a session: per step the arrays of hhuff_qpack_decode (sections packed back to back first, then the encoder
    buffers).  A spacer connection sends nothing on its encoder stream and one empty section per step, which fails
    and writes nothing."""
    rng = np.random.default_rng(seed)
    nsteps = max(len(c) for k in cases for c in k["conns"])
    conns, rounds = [], 0
    while True:
        order = np.arange(len(cases)) if rounds == 0 else rng.permutation(len(cases))
        for ci in order:
            k = cases[ci]
            for j, c in enumerate(k["conns"]):
                steps = [c[i] if i < len(c) else (b"", []) for i in range(nsteps)]
                slices = [[k["arena"].get((j, i, s), default_slice(len(sec), k["ent"], k["room"]))
                           for s, sec in enumerate(st[1])] for i, st in enumerate(steps)]
                conns.append((k["name"], steps, slices, k["blocked"]))
                if spacers:
                    conns.append(("spacer", [(b"", [b""])] * nsteps, [[SPACER_SLICE]] * nsteps, 0))
        rounds += 1
        if nconn is None or len(conns) >= nconn:
            break
    if nconn is not None:
        conns = conns[:nconn]
    out = []
    for i in range(nsteps):
        secs, labels, sizes, conn_first, enc = [], [], [], [0], []
        for label, steps, slices, _ in conns:
            secs += steps[i][1]
            sizes += slices[i]
            labels += ["%s[step %d section %d]" % (label, i, s) for s in range(len(steps[i][1]))]
            conn_first.append(len(secs))
            enc.append(steps[i][0])
        sec_off = np.zeros(len(secs) + 1, np.uint64)
        sec_off[1:] = np.cumsum([len(s) for s in secs])
        enc_len = np.asarray([len(e) for e in enc], np.uint64)
        enc_off = int(sec_off[-1]) + np.cumsum(enc_len) - enc_len
        arena_off = np.full(len(secs) + 1, arena_base, np.uint64)
        arena_off[1:] += np.cumsum(np.asarray(sizes, np.uint64))
        data = np.frombuffer(b"".join(secs) + b"".join(enc), np.uint8).copy()
        out.append(dict(data=data, in_size=int(data.size), blk_off=sec_off.astype(np.uint32), nblk=len(secs),
                        conn_first=np.asarray(conn_first, np.uint32), enc_off=enc_off.astype(np.uint32),
                        enc_len=enc_len.astype(np.uint32), arena_off=arena_off, labels=labels,
                        conn_labels=[c[0] for c in conns],
                        stream_id=(np.arange(len(secs), dtype=np.uint64) * 4 + 1000 * i) << np.uint64(7 * (i % 3))))
    return dict(table_size=header_table_size, max_blocked=max_blocked, nconn=len(conns), calls=out,
                num_blocked=np.asarray([c[3] for c in conns], np.uint32))


Q_SECTION = ("nfields", "sstatus", "req_insert_count")
Q_CONN = ("enc_status", "enc_consumed", "insert_count")


def _qwords(r, mode, nsec):
    """the oracle's records of a step as u32 words"""
    rec = r["req" if mode == "qreq" else "res"][:nsec]
    return np.ascontiguousarray(rec).view(np.uint8).reshape(nsec, 4 * RECORD_WORDS[mode]).view(np.uint32)


def qexpected(codec, bt, mode="plain"):
    """the oracle's session over the steps -> per step the arrays of expected(), QPACK's per-section and
    per-connection arrays and, in mode "qreq" (hhuff_qpack_parse_requests) / "qres" (hhuff_qpack_parse_responses),
    the request / response records"""
    from oracle import oracle as O

    s = O.QpackSession(codec, bt["nconn"], bt["table_size"], bt["max_blocked"])
    out = []
    try:
        for cl in bt["calls"]:
            r = s.step(cl["data"], cl["enc_off"], cl["enc_len"], cl["blk_off"], cl["conn_first"], cl["arena_off"],
                       bt["num_blocked"], stream_id=cl["stream_id"] if mode != "plain" else None,
                       responses=mode == "qres")
            e = {k: r[k][:cl["nblk"]] for k in Q_SECTION}
            e.update({k: r[k][:bt["nconn"]] for k in Q_CONN})
            e["arena"] = r["arena"][:int(cl["arena_off"][-1])]
            for k, _ in SLOT_ARRAYS:
                e[k] = r[k][:cl["in_size"]]
            if mode != "plain":
                e[mode] = _qwords(r, mode, cl["nblk"])
            out.append(e)
    finally:
        s.close()
    return out


def qcall_args(cl, bt, mode, cont, fill, sentinel):
    """one step's arrays, as call_args(): the per-section arrays have nsec entries, the per-connection ones nconn"""
    whole, inner = guarded(np, cl["in_size"], fill)
    inner[:] = cl["data"]
    nsec, n, nconn = cl["nblk"], cl["in_size"], bt["nconn"]
    size = {"arena": int(cl["arena_off"][-1]), "nfields": 4 * nsec, "sstatus": 4 * nsec, "req_insert_count": 8 * nsec,
            "enc_status": 4 * nconn, "enc_consumed": 4 * nconn, "insert_count": 8 * nconn}
    for k, dt in SLOT_ARRAYS:
        size[k] = n * np.dtype(dt).itemsize
    if mode != "plain":
        size[mode] = 4 * RECORD_WORDS[mode] * nsec
    return dict(in_whole=whole, data=inner, in_size=n, nblk=nsec, nconn=nconn, table_size=bt["table_size"],
                max_blocked=bt["max_blocked"], mode=mode, cont=cont, labels=cl["labels"], sentinel=sentinel,
                exact=Q_SECTION + Q_CONN, blk_off=_poisoned(cl["blk_off"], np.uint32, 0, n),
                conn_first=_poisoned(cl["conn_first"], np.uint32, 0, nsec),
                enc_off=_poisoned(cl["enc_off"], np.uint32, 0, n), enc_len=_poisoned(cl["enc_len"], np.uint32, 0, 0),
                num_blocked=_poisoned(bt["num_blocked"], np.uint32, 0, 0),
                stream_id=_poisoned(cl["stream_id"], np.uint64, 0, 0),
                arena_off=_poisoned(cl["arena_off"], np.uint64, int(cl["arena_off"][0]), int(cl["arena_off"][-1])),
                out={k: guarded(np, v, sentinel)[0] for k, v in size.items()}, scratch_guards=None)


def qrun(impl_factory, bt, mode="plain", check=None, poison=True):
    """run() for a QPACK session"""
    done = []
    for fill, sentinel in RUNS:
        impl = impl_factory(sentinel)
        done = []
        for i, cl in enumerate(bt["calls"]):
            a = qcall_args(cl, bt, mode, i > 0, fill, sentinel)
            impl.call(a)
            kept = dict(a, out={k: v.copy() for k, v in a["out"].items()})
            if check is not None:
                check(kept, i, sentinel)
            done.append(kept)
            if poison:
                a["in_whole"][:] = POISON
                for k in ("arena",) + tuple(k for k, _ in SLOT_ARRAYS):
                    a["out"][k][:] = POISON
                impl.poison()
        impl.close()
    return done


class OracleQpack:
    """the oracle's session as an implementation of the steps"""

    def __init__(self, codec, bt):
        from oracle import oracle as O

        self.s = O.QpackSession(codec, bt["nconn"], bt["table_size"], bt["max_blocked"])

    def poison(self):
        pass

    def close(self):
        self.s.close()

    def call(self, a):
        nsec, nconn = a["nblk"], a["nconn"]
        r = self.s.step(a["data"].copy(), a["enc_off"][:nconn], a["enc_len"][:nconn], a["blk_off"][:nsec + 1],
                        a["conn_first"][:nconn + 1], a["arena_off"][:nsec + 1], a["num_blocked"][:nconn],
                        stream_id=a["stream_id"][:nsec] if a["mode"] != "plain" else None,
                        responses=a["mode"] == "qres")
        bo = a["blk_off"][:nsec + 1].astype(np.int64)
        slots = _ranges(bo[:-1], r["nfields"][:nsec].astype(np.int64))
        for k, _ in SLOT_ARRAYS:
            out_view(a, k)[slots] = r[k][slots]
        arena = out_view(a, "arena")
        for offk, lenk in (("name_off", "name_len"), ("value_off", "value_len")):
            pos = _ranges(r[offk][slots].astype(np.int64), r[lenk][slots].astype(np.int64))
            arena[pos] = r["arena"][pos]
        for k in Q_SECTION:
            out_view(a, k)[:] = r[k][:nsec]
        for k in Q_CONN:
            out_view(a, k)[:] = r[k][:nconn]
        if a["mode"] != "plain":
            entries(a["out"][a["mode"]], np.uint32)[:] = _qwords(r, a["mode"], nsec).reshape(-1)


class GpuQpack:
    """hhuff_qpack_decode / hhuff_qpack_parse_requests / _parse_responses on guarded device arrays, the scratch of exactly
    hhuff_qpack_scratch_size bytes between guards, moved in poison()"""

    def __init__(self, torch, sentinel):
        from h2o_amd import codec

        self.torch, self.lib, self.sentinel = torch, codec.lib(), sentinel
        self.scratch, self.keep, self.last = None, [], None

    def close(self):
        pass

    def call(self, a):
        torch, L = self.torch, self.lib
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).cuda()  # noqa: E731
        inp = to_device(torch, a["in_whole"])
        ins = {k: dev(a[k]) for k in ("enc_off", "enc_len", "blk_off", "conn_first", "num_blocked", "arena_off",
                                      "stream_id")}
        out = {k: to_device(torch, v) for k, v in a["out"].items()}
        ss = int(L.hhuff_qpack_scratch_size(a["nconn"], a["table_size"]))
        if self.scratch is None:
            self.scratch = guarded(torch, ss, self.sentinel)
        o = lambda k: _inner(out[k])  # noqa: E731
        i = lambda k: _vp(ins[k])  # noqa: E731
        args = [_inner(inp), a["in_size"], i("enc_off"), i("enc_len"), i("blk_off"), i("conn_first"), a["nconn"],
                a["nblk"], a["table_size"], a["max_blocked"], i("num_blocked"), o("arena"), i("arena_off"),
                o("name_off"), o("name_len"), o("value_off"), o("value_len"), o("fflags"), o("nfields"), o("sstatus"),
                o("req_insert_count"), o("enc_status"), o("enc_consumed"), o("insert_count")]
        tail = [_inner(self.scratch), ss, 1 if a["cont"] else 0, None]
        if a["mode"] == "qreq":
            rc = L.hhuff_qpack_parse_requests(*args, i("stream_id"), o("qreq"), *tail)
        elif a["mode"] == "qres":
            rc = L.hhuff_qpack_parse_responses(*args, i("stream_id"), o("qres"), *tail)
        else:
            rc = L.hhuff_qpack_decode(*args, *tail)
        assert rc == 0, "the call returned %d: %s" % (rc, L.hhuff_last_error_string())
        torch.cuda.synchronize()
        for k, (whole, _) in out.items():
            a["out"][k][:] = whole.cpu().numpy()
        w = self.scratch[0].cpu().numpy()
        a["scratch_guards"] = np.concatenate([w[:GUARD], w[w.size - GUARD:]])
        self.last = [inp[0]] + [out[k][0] for k in ("arena",) + tuple(k for k, _ in SLOT_ARRAYS)]
        self.keep.append((ins, out))

    poison = GpuBlocks.poison


def qsummary(results, bt, mode="plain"):
    """summary() for a session, plus QPACK's per-section and per-connection arrays"""
    out = summary([dict(e, bstatus=e["sstatus"]) for e in results], bt, [mode] * len(results))
    for i, e in enumerate(results):
        for k in ("req_insert_count",) + Q_CONN:
            out["%d_%s" % (i, k)] = np.asarray(e[k])
    return out


def qresult_of(a):
    r = {k: out_view(a, k) for k in ("arena",) + Q_SECTION + Q_CONN + tuple(k for k, _ in SLOT_ARRAYS)}
    if a["mode"] != "plain":
        r[a["mode"]] = entries(a["out"][a["mode"]], np.uint32).reshape(a["nblk"], RECORD_WORDS[a["mode"]])
    return r
