"""Hand-placed strings, exact-size guarded calls and a footprint checker for the header encoders
(hhuff_hpack_flatten_responses and the stateless hhuff_qpack_flatten_responses, include/hhuff.h (2f) / (2g)) --
plain helpers, no GPU.  What bounds_harness.py does for the batch codec and blocks_harness.py for the header-block
decoders, on the encode side:

  builders     make_batch() on top of hpenc_synth.build_batch / to_qpack (connections as lists of records);
               relay() re-lays the input: every string where the case wants it (an offset modulo 4 or 16, ending on
               a 16-byte line, last in the buffer), everything else packed without filler, the last string ending at
               in_size - 1, and every byte that belongs to no string holding the run's fill
  symbols      strings_with(bits, length): a string of `length` bytes whose Huffman code is exactly `bits` bits, built
               from the code-length classes of h2o_amd/tables.py (5, 6, 7, 8 and >= 19 bits)
  payloads     pad_to_payload(): one filler value grows until the model's headers_size / header_len is the target
  regions      exact_fit() / short_by_one(): out_off re-laid so that every region is exactly what the model says the
               record needs, back to back from an odd offset; or one region a byte too small
  groups       a group is a list of cases (enc_corpora.py) merged into one batch per call: build_group()
  the call     guarded_call(): `in` between guards of the run's fill; out, out_len, headers_size / header_len and
               rstatus of exactly the documented size between guards of the run's sentinel; run() does every call of
               a group twice (bounds_harness.RUNS) and overwrites the previous call's input before the next
  check()      statuses, lengths and bytes against the model; every byte of `out` outside
               [out_off[r], out_off[r] + out_len[r]) -- the tail of a region, the whole region of a refused record,
               the guards -- still holds the sentinel

The model is the pinned restatement: oracle/hpack_encode.c through hpenc_push_model.PushModel (which adds the
PUSH_PROMISE records and the HHUFF_RES_SPACE verdict against the caller's regions) and oracle/qpack_encode.c.
An implementation is an object with call(a) and poison(fill): ModelEnc (the model itself, the compiled reference,
or a faulty variant the harness has to catch) or GpuEnc (libhhuff through h2o_amd.codec)."""
import numpy as np

from bounds_harness import GUARD, RUNS, entries, guarded, huffman, ranges_mask, to_device
from h2o_amd import codec as C
from h2o_amd import hpack_synth as HS_SYNTH
from h2o_amd import hpenc_synth as HE
from h2o_amd import tables as T
from hpenc_push_model import deframe

NBITS = np.asarray(T.ENC_NBITS, np.int64)
HS = {"h": "headers_size", "q": "header_len"}  # the payload-size output of each encoder
NO_LENGTH = 0xFFFFFFFFFFFFFFFF


# ------------------------------------------------------------------------------------------------
# symbol classes (h2o_amd/tables.py) and strings of an exact code length
# ------------------------------------------------------------------------------------------------
def symbol_classes(name=False):
    """code bits -> the bytes with a code of that length, among the bytes valid in a header value (or name)"""
    cls = {}
    for b in sorted(T.NAME_VALID if name else T.VALUE_VALID):
        cls.setdefault(int(NBITS[b]), []).append(b)
    return cls


def code_bits(s):
    return int(NBITS[np.frombuffer(s, np.uint8)].sum()) if s else 0


def strings_with(bits, length, name=False, seed=0, min_long=0):
    """`length` bytes whose Huffman code has exactly `bits` bits: 5-, 6-, 7- and 8-bit symbols, and as many symbols
    of 19 bits and more as the number needs (at least min_long; names have none).  Which symbol of a class, and the
    order, come from `seed`."""
    cls = symbol_classes(name)
    longs = sorted(b for b in cls if b >= 19)
    rng = np.random.default_rng([int(x) for x in np.atleast_1d(seed)] + [bits, length])
    if length == 0:
        assert bits == 0
        return b""
    extra = bits - 5 * length
    assert extra >= 0, "%d bits are fewer than %d symbols of 5" % (bits, length)
    k = min_long
    while True:
        assert k <= length and (k == 0 or longs), "no %d-byte string of %d bits" % (length, bits)
        lo, hi = ((longs[0] - 5) * k, (longs[-1] - 5) * k) if k else (0, 0)
        take = min(hi, extra)  # the bits over 5 that the long symbols carry
        if take >= lo and extra - take <= 3 * (length - k):
            break
        k += 1
    lens, rest = [longs[0] if k else 0] * k, take - lo
    for i in range(k):
        up = min(rest, longs[-1] - longs[0])
        lens[i] += up
        rest -= up
    small, rest = [5] * (length - k), extra - take
    for i in range(length - k):
        up = min(rest, 3)
        small[i] += up
        rest -= up
    assert rest == 0
    lens = np.array(lens + small)
    rng.shuffle(lens)
    s = bytes(int(rng.choice(cls[int(b)])) for b in lens)
    assert len(s) == length and code_bits(s) == bits
    return s


def text(length, seed=0, name=False):
    """`length` bytes of 5- to 8-bit symbols (about 6.2 bits each: Huffman wins from 4 bytes on)"""
    rng = np.random.default_rng([int(x) for x in np.atleast_1d(seed)] + [length, 7])
    cls = symbol_classes(name)
    pool = np.array(cls[5] * 3 + cls[6] * 3 + cls[7] + cls[8][:2], np.uint8)
    return bytes(rng.choice(pool, length))


def huffman_len(s):
    return (code_bits(s) + 7) // 8


# ------------------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------------------
def make_batch(conns, proto, server=HE.SERVER):
    """conns = [[record, ...] per connection], records as hpenc_synth.build_batch takes them; for proto "q" a record
    may carry dfid=bytes (HHUFF_QRES_DATAGRAM) and qrequest=True (HHUFF_QRES_REQUEST), and trailers are not allowed"""
    b = HE.build_batch(conns, server=server)
    if proto == "h":
        return b
    recs = [r for rs in conns for r in rs]
    assert not any(r.get("flags", 0) & C.RES_TRAILERS for r in recs)
    q = HE.to_qpack(b, dfid_frac=0.0, odd_status_frac=0.0)
    data, extra = q["data"], []
    for k, r in enumerate(recs):
        if r.get("qrequest"):
            q["res"]["flags"][k] = C.QRES_REQUEST
        if "dfid" in r:
            q["res"]["flags"][k] |= C.QRES_DATAGRAM
            q["res"]["dfid_off"][k] = data.size + sum(len(e) for e in extra)
            q["res"]["dfid_len"][k] = len(r["dfid"])
            extra.append(r["dfid"])
    if extra:
        q["data"] = np.concatenate([data, np.frombuffer(b"".join(extra), np.uint8)])
    q["out_off"] = HE.qpack_out_offsets(q["hdr"], q["res"], q["server_len"])
    q["conn_first"] = b["conn_first"]
    return q


def _string_refs(b):
    """every (array, row, offset field, length field) of the batch that names a string of `in`"""
    refs = []
    for i in range(b["hdr"].size):
        refs += [(b["hdr"], i, "name_off", "name_len"), (b["hdr"], i, "value_off", "value_len")]
    if "dfid_off" in b["res"].dtype.names:
        for i in np.flatnonzero(b["res"]["flags"] & C.QRES_DATAGRAM):
            refs.append((b["res"], int(i), "dfid_off", "dfid_len"))
    return refs


def relay(b, place=None, tail=0):
    """The batch with its input laid out again.  Every distinct string stands once, in the order of the original
    buffer, packed with no filler -- except where `place` (string bytes -> rule) says otherwise:
      ("mod", m, k)   the string starts at an offset that is k modulo m
      ("end", m)      the string ends where offset + length is a multiple of m
      ("last",)       the string comes last (its last byte is in[in_size - 1] when tail == 0)
    -> a new batch; b["owned"] marks the bytes that belong to a string (with_fill() sets the others) and
    b["str_off"] maps a string's bytes to its offset."""
    place = place or {}
    raw = b["data"].tobytes()
    out = dict(b, hdr=b["hdr"].copy(), res=b["res"].copy())
    refs = _string_refs(out)
    keys = {(int(b["server_off"]), int(b["server_len"]))}
    keys |= {(int(a[i][o]), int(a[i][n])) for a, i, o, n in refs}
    last = [k for k in keys if place.get(raw[k[0]:k[0] + k[1]], ("",))[0] == "last"]
    assert len(last) <= 1, "two strings want to be last"
    order = sorted(k for k in keys if k not in last) + last
    new, pos, chunks = {}, 0, []
    for off, n in order:
        s = raw[off:off + n]
        rule = place.get(s)
        if rule is not None and rule[0] == "mod":
            pos += (rule[2] - pos) % rule[1]
        elif rule is not None and rule[0] == "end":
            pos += (-(pos + n)) % rule[1]
        new[(off, n)] = pos
        chunks.append((pos, s))
        pos += n
    in_size = pos + tail
    data, owned = np.zeros(in_size, np.uint8), np.zeros(in_size, bool)
    for p, s in chunks:
        assert not owned[p:p + len(s)].any()
        data[p:p + len(s)] = np.frombuffer(s, np.uint8)
        owned[p:p + len(s)] = True
    for a, i, o, n in refs:
        a[i][o] = new[(int(a[i][o]), int(a[i][n]))]
    out["server_off"] = new[(int(b["server_off"]), int(b["server_len"]))]
    out["data"], out["owned"] = data, owned
    out["str_off"] = {raw[off:off + n]: p for (off, n), p in new.items()}
    return out


def with_fill(b, fill):
    """the batch's input with `fill` in every byte that belongs to no string"""
    data = b["data"].copy()
    data[~b["owned"]] = fill
    return data


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
class Model:
    """One session of the restatement (codec None) or of the compiled reference (codec = oracle.ref(): no promises):
    step(batch) -> dict out, out_len, headers_size / header_len, rstatus"""

    def __init__(self, proto, nconn, codec=None):
        from oracle import oracle as O

        self.proto, self.codec = proto, codec
        if proto == "h" and codec is None:
            from hpenc_push_model import PushModel

            self.sess = PushModel(nconn)
        elif proto == "h":
            self.sess = O.HpeSession(codec, nconn)

    def step(self, b):
        from oracle import oracle as O

        if self.proto == "q":
            return O.qpe_step(self.codec or O.oracle(), b["data"], b["hdr"], b["res"], b["out_off"], b["server_off"],
                              b["server_len"])
        if self.codec is None:
            return self.sess.step(b)
        return self.sess.step(b["data"], b["hdr"], b["res"], b["conn_first"], b["out_off"], b["server_off"], b["server_len"])


def model_run(proto, calls, codec=None):
    m = Model(proto, calls[0]["conn_first"].size - 1, codec)
    return [m.step(b) for b in calls]


def pad_to_payload(records, target, proto="h", r=-1, h=0, kind="raw", server=HE.SERVER):
    """One connection's records with the value of header `h` of record `r` lengthened until the model's
    headers_size (header_len for proto "q") of that record is `target`.  kind "raw": bytes whose code is longer
    than themselves (the value goes as it is); "huff": 5-bit symbols (Huffman, 5/8 of a byte each: every size is
    reachable).  The filler keeps what the value held as its head.  -> the records (copies)"""
    sym = b"~" if kind == "raw" else b"aeiost012c"
    rec0 = records[r]
    name, head, fl = rec0["headers"][h]
    k = r % len(records)

    def build(n):
        hs = list(rec0["headers"])
        hs[h] = (name, head + (sym * (n // len(sym) + 1))[:n], fl)
        return records[:k] + [dict(rec0, headers=hs)] + records[k + 1:]

    def size(n):
        res = model_run(proto, [make_batch([build(n)], proto, server)])[0]
        assert res["rstatus"][k] == 0
        return int(res[HS[proto]][k])

    lo, hi = 0, max(64, 2 * target)  # the size is monotone in n and grows by at most one per byte
    assert size(lo) <= target <= size(hi), "target %d outside [%d, %d]" % (target, size(lo), size(hi))
    while lo < hi:
        mid = (lo + hi) // 2
        if size(mid) < target:
            lo = mid + 1
        else:
            hi = mid
    assert size(lo) == target, "no filler length gives %d" % target
    return build(lo)


# ------------------------------------------------------------------------------------------------
# regions
# ------------------------------------------------------------------------------------------------
def _with_sizes(b, sizes, first):
    out = dict(b)
    out["out_off"] = (first + np.concatenate([[0], np.cumsum(sizes)])).astype(np.uint64)
    return out


def exact_fit(b, res, first=1):
    """out_off re-laid: every region exactly the model's out_len[r] (nothing for a refused record), back to back,
    the first at `first`"""
    n = b["res"].size
    return _with_sizes(b, res["out_len"][:n].astype(np.int64), first)


def short_by_one(b, res, r, first=None):
    """region r one byte smaller than the model's out_len[r]; the other regions as they are (first None) or exactly
    fitting as exact_fit() lays them"""
    n = b["res"].size
    assert res["rstatus"][r] == 0 and res["out_len"][r] > 0
    if first is None:
        sizes = np.diff(b["out_off"].astype(np.int64))
        first = int(b["out_off"][0])
    else:
        sizes = res["out_len"][:n].astype(np.int64).copy()
    sizes[r] = int(res["out_len"][r]) - 1
    return _with_sizes(b, sizes, first)


# ------------------------------------------------------------------------------------------------
# groups of cases
# ------------------------------------------------------------------------------------------------
class Case:
    """name; what it must hit (text) and the predicate that says so, hit(ctx) over the model's result; calls = one
    list of connections per call (every call lists the same connections; stateless QPACK has one call); place =
    relay() rules; shorts = [(call, record)]: that record's region is one byte short; patch(batch, call, rows) edits
    the merged batch (rows = the case's first record and header row); ref = the reference harness accepts it (or the
    reason why not); roundtrip = the blocks decode to the input fields (or the reason why not)"""

    def __init__(self, name, must, calls, hit, place=None, shorts=(), patch=None, ref=True, roundtrip=True):
        self.name, self.must, self.calls, self.hit = name, must, calls, hit
        self.place, self.shorts, self.patch, self.ref, self.roundtrip = place or {}, tuple(shorts), patch, ref, roundtrip
        assert all(len(c) == len(calls[0]) for c in calls), name


class Ctx:
    """what a case's predicate sees: the merged batches, the model's final results, the results before any region
    was shortened (want), and where the case's records are"""

    def __init__(self, group, i):
        self.g, self.i, self.proto = group, i, group["proto"]

    def rows(self, call=0):
        lo, n, _ = self.g["rows"][call][self.i]
        return lo, lo + n

    def batch(self, call=0):
        return self.g["calls"][call]

    def get(self, key, call=0, want=False):
        lo, hi = self.rows(call)
        key = HS[self.proto] if key == "hs" else key
        return [int(x) for x in (self.g["want"] if want else self.g["exp"])[call][key][lo:hi]]

    def frames(self, k, call=0, want=True):
        res = (self.g["want_fit"] if want else self.g["exp"])[call]
        b = (self.g["want_calls"] if want else self.g["calls"])[call]
        r = self.rows(call)[0] + k
        o = int(b["out_off"][r])
        return res["out"][o:o + int(res["out_len"][r])].tobytes()

    def block(self, k, call=0):
        """record k's header block: HPACK the frames' payloads joined (a promise's 4 id bytes included); QPACK the
        field section behind the frame header"""
        f = self.frames(k, call)
        if self.proto == "h":
            return b"".join(x[3] for x in deframe(f))
        n = 1 << (f[1] >> 6)
        return f[1 + n:]

    def fields(self, k, call=0, skip=0):
        blk = self.block(k, call)[skip:]
        return walk(blk) if self.proto == "h" else walk_q(blk)

    def off(self, s, call=0):
        return self.batch(call)["str_off"][s]


def build_group(cases, proto, server=HE.SERVER, keep=None):
    """The cases' connections side by side, one batch per call (a case with fewer calls has empty connections in
    the later ones), laid out by relay() with every case's rules, patched, and with the shortened regions applied.
    -> dict proto, cases, calls (batches), rows[call][case] = (first record, records, first header row), exp (the
    model's result per call), want (its result before the regions were shortened) and labels (one per record)"""
    cases = [c for c in cases if keep is None or keep(c)]
    ncalls = max(len(c.calls) for c in cases)
    place = {}
    for c in cases:
        for s, rule in c.place.items():
            assert place.setdefault(s, rule) == rule, "%s: another case places %r differently" % (c.name, s[:16])
    calls, rows, labels = [], [], []
    for k in range(ncalls):
        conns, rw, lab, nres, nhdr = [], [], [], 0, 0
        for c in cases:
            cc = c.calls[k] if k < len(c.calls) else [[] for _ in c.calls[0]]
            n = sum(len(rs) for rs in cc)
            rw.append((nres, n, nhdr))
            lab += ["%s[%d]" % (c.name, j) for j in range(n)]
            nres += n
            nhdr += sum(len(r.get("headers", [])) for rs in cc for r in rs)
            conns += cc
        b = relay(make_batch(conns, proto, server), place)
        for c, r in zip(cases, rw):
            if c.patch is not None:
                c.patch(b, k, r)
        calls.append(b)
        rows.append(rw)
        labels.append(lab)
    want = model_run(proto, calls)
    final = []
    for k, b in enumerate(calls):
        for c, r in zip(cases, rows[k]):
            for call, j in c.shorts:
                if call == k:
                    b = short_by_one(b, want[k], r[0] + j)
        final.append(b)
    g = dict(proto=proto, cases=cases, calls=final, rows=rows, labels=labels, want=want, want_fit=want, want_calls=calls,
             server=server)
    g["exp"] = model_run(proto, final)
    return g


def refit(g, first):
    """the group with every call's regions exactly fitting (exact_fit at `first`); a shortened region is one byte
    short of what the record needed before"""
    calls = []
    for k, b in enumerate(g["calls"]):
        sizes = g["exp"][k]["out_len"][:b["res"].size].astype(np.int64).copy()
        for c, r in zip(g["cases"], g["rows"][k]):
            for call, j in c.shorts:
                if call == k:
                    sizes[r[0] + j] = int(g["want"][k]["out_len"][r[0] + j]) - 1
        calls.append(_with_sizes(b, sizes, first))
    out = dict(g, calls=calls)
    out["exp"] = model_run(g["proto"], calls)
    return out


# ------------------------------------------------------------------------------------------------
# reading an encoded block back (predicates, planted faults)
# ------------------------------------------------------------------------------------------------
def _int(b, p, bits):
    v, q = b[p] & ((1 << bits) - 1), p + 1
    if v == (1 << bits) - 1:
        shift = 0
        while True:
            x = b[q]
            q += 1
            v += (x & 127) << shift
            shift += 7
            if not x & 128:
                break
    return v, q


def _str(b, p, bits=7):
    n, q = _int(b, p, bits)
    return dict(huff=(b[p] >> bits) & 1, len=n, int=(p, q), pay=(q, q + n)), q + n


def walk(block):
    """the representations of an HPACK block (RFC 7541 6): -> [dict kind ("indexed", "inc", "without", "never",
    "update"), index / size, idx_int (the index's bytes), name / value (dict huff, len, int, pay: byte ranges),
    start, end]"""
    out, p = [], 0
    while p < len(block):
        x, f = block[p], dict(start=p)
        if x & 0x80:
            f["kind"] = "indexed"
            f["index"], q = _int(block, p, 7)
            f["idx_int"] = (p, q)
        elif x & 0x40 or not x & 0x20:
            f["kind"] = "inc" if x & 0x40 else "never" if x & 0x10 else "without"
            f["index"], q = _int(block, p, 6 if x & 0x40 else 4)
            f["idx_int"] = (p, q)
            if f["index"] == 0:
                f["name"], q = _str(block, q)
            f["value"], q = _str(block, q)
        else:
            f["kind"] = "update"
            f["size"], q = _int(block, p, 5)
        f["end"] = p = q
        out.append(f)
    return out


def walk_q(section):
    """the field lines of a QPACK field section behind its two prefix bytes (RFC 9204 4.5; the stateless encoder
    uses the static table only): -> [dict kind ("indexed", "nameref", "literal"), index, name / value, start, end]"""
    assert section[:2] == b"\x00\x00"
    out, p = [], 2
    while p < len(section):
        x, f = section[p], dict(start=p)
        if x & 0x80:
            assert x & 0x40, "a dynamic reference"
            f["kind"] = "indexed"
            f["index"], q = _int(section, p, 6)
        elif x & 0x40:
            assert x & 0x10, "a dynamic reference"
            f["kind"], f["never"] = "nameref", (x >> 5) & 1
            f["index"], q = _int(section, p, 4)
            f["value"], q = _str(section, q)
        else:
            assert x & 0x20, "a post-base line"
            f["kind"], f["never"] = "literal", (x >> 4) & 1
            f["name"], q = _str(section, p, 3)
            f["value"], q = _str(section, q)
        f["end"] = p = q
        out.append(f)
    return out


# ------------------------------------------------------------------------------------------------
# the guarded call
# ------------------------------------------------------------------------------------------------
def guarded_call(b, proto, fill, sentinel, cont=False, labels=None):
    """One call's arrays: `in` (in_size bytes, `fill` where no string is) between guards of `fill`; out
    (out_off[nres] bytes), out_len, headers_size / header_len and rstatus (nres entries each) between guards of
    `sentinel`, filled with it"""
    n = int(b["res"].size)
    whole, inner = guarded(np, b["data"].size, fill)
    inner[:] = with_fill(b, fill)
    out = {"out": guarded(np, int(b["out_off"][-1]), sentinel)[0]}
    for k in ("out_len", HS[proto], "rstatus"):
        out[k] = guarded(np, 4 * n, sentinel)[0]
    return dict(batch=b, proto=proto, in_whole=whole, data=inner, in_size=int(b["data"].size), nres=n,
                nconn=b["conn_first"].size - 1, cont=cont, sentinel=sentinel, out=out, scratch_guards=None,
                labels=labels or ["record %d" % r for r in range(n)])


def run(impl_factory, g, check_fn=None):
    """Every call of the group through impl_factory(sentinel), under both (fill, sentinel) pairs of
    bounds_harness.RUNS.  After a call is checked (check_fn(a, call index), default check() against the group's
    model results) its input is overwritten with the run's other fill, on the implementation's side too
    (impl.poison), and the next call gets a new `in`.  -> the last run's call arguments"""
    done = []
    for k, (fill, sentinel) in enumerate(RUNS):
        impl = impl_factory(sentinel)
        other = RUNS[1 - k][0]
        done = []
        for i, b in enumerate(g["calls"]):
            a = guarded_call(b, g["proto"], fill, sentinel, cont=i > 0, labels=g["labels"][i])
            impl.call(a)
            if check_fn is None:
                check(a, g["exp"][i], "call %d, fill %#x" % (i, fill))
            else:
                check_fn(a, i)
            done.append(a)
            a["in_whole"][:] = other
            impl.poison(other)
    return done


def check(a, exp, label=""):
    """a: a call's arguments with its outputs filled in; exp: the model's result for the call.  Asserts, in this
    order, each with its own message:
      - the guards of out_len, headers_size / header_len and rstatus (and of the scratch, where reported) intact
      - rstatus, then out_len, then headers_size / header_len equal, record by record
      - the bytes [out_off[r], out_off[r] + out_len[r]) of every accepted record equal
      - every other byte of `out` -- the tail of a region, the whole region of a refused record, the space before
        the first region, both guards -- still the sentinel"""
    n, sentinel, labels, proto = a["nres"], a["sentinel"], a["labels"], a["proto"]

    def fail(msg, r=None):
        raise AssertionError("%s%s: %s" % (label, "" if r is None else " " + labels[r], msg))

    for name, whole in a["out"].items():
        if name == "out":
            continue
        for side, g in (("front", whole[:GUARD]), ("rear", whole[whole.size - GUARD:])):
            hit = np.nonzero(g != sentinel)[0]
            if hit.size:
                fail("%s: %s guard byte %d written (%#x)" % (name, side, hit[0], g[hit[0]]))
    if a["scratch_guards"] is not None and (a["scratch_guards"] != sentinel).any():
        fail("a scratch guard byte was written")
    for name, dt in (("rstatus", np.int32), ("out_len", np.uint32), (HS[proto], np.uint32)):
        got, want = entries(a["out"][name], dt), np.asarray(exp[name][:n]).astype(dt)
        bad = np.nonzero(got != want)[0]
        if bad.size:
            fail("%s = %d, model %d (%d records differ)" % (name, got[bad[0]], want[bad[0]], bad.size), int(bad[0]))
    whole = a["out"]["out"]
    out = whole[GUARD:whole.size - GUARD]
    off = a["batch"]["out_off"].astype(np.int64)
    ln = np.asarray(exp["out_len"][:n]).astype(np.int64)
    assert out.size == int(off[-1])
    for r in np.nonzero(ln)[0]:
        got, want = out[off[r]:off[r] + ln[r]], exp["out"][off[r]:off[r] + ln[r]]
        bad = np.nonzero(got != want)[0]
        if bad.size:
            fail("bytes differ from byte %d of %d on: %s, model %s (%d bytes)"
                 % (bad[0], ln[r], got[bad[0]:bad[0] + 8].tobytes().hex(), want[bad[0]:bad[0] + 8].tobytes().hex(),
                    bad.size), int(r))
    stray = whole != sentinel
    stray[GUARD:GUARD + out.size] &= ~ranges_mask(off[:n], off[:n] + ln, out.size)
    hit = np.nonzero(stray)[0]
    if hit.size:
        p = int(hit[0]) - GUARD
        r = int(np.searchsorted(off, p, side="right")) - 1
        if 0 <= p < out.size and r < n and exp["rstatus"][r] != 0:
            fail("byte %d of a refused record's region written: %#x (%d stray bytes)"
                 % (p - off[r], whole[hit[0]], hit.size), r)
        if 0 <= p < out.size and r < n:
            fail("byte %d past out_len written: %#x (%d stray bytes)" % (p - off[r] - ln[r], whole[hit[0]], hit.size), r)
        fail("out byte %d (buffer of %d) written outside every region: %#x (%d stray bytes)"
             % (p, out.size, whole[hit[0]], hit.size))


# ------------------------------------------------------------------------------------------------
# implementations
# ------------------------------------------------------------------------------------------------
FAULTS = ("past", "refused", "name_index", "huff_tie", "cont-1")


class ModelEnc:
    """The model as an implementation: a session over the calls, writing into the caller's guarded arrays only what
    the contract lets a call write.  codec: None (the restatement) or oracle.ref().  Faulty variants, which the
    harness has to catch:
      "past"        one byte written just past a record's out_len
      "refused"     a byte written into the region of a refused record
      "name_index"  a literal's name index one too high
      "huff_tie"    a string whose Huffman form is exactly as long as the string sent as Huffman (h2o sends it raw)
      "cont-1"      the last CONTINUATION frame header written with 8 bytes"""

    def __init__(self, proto, nconn, fault=None, codec=None):
        assert fault is None or fault in FAULTS
        self.proto, self.fault, self.model = proto, fault, Model(proto, nconn, codec)
        self.planted = 0

    def poison(self, fill):
        pass

    def call(self, a):
        b, n, proto = a["batch"], a["nres"], a["proto"]
        r = self.model.step(dict(b, data=a["data"]))
        off = b["out_off"].astype(np.int64)
        out = entries(a["out"]["out"], np.uint8)
        ln = r["out_len"][:n].astype(np.int64).copy()
        frames = [r["out"][off[k]:off[k] + ln[k]].tobytes() for k in range(n)]
        if self.fault in ("name_index", "huff_tie", "cont-1"):
            for k in range(n):
                f = getattr(self, "_" + self.fault.replace("-", "_"))(frames[k], a, k)
                if f is not None:
                    frames[k], ln[k] = f, len(f)
                    self.planted += 1
                    break
        for k in range(n):
            out[off[k]:off[k] + ln[k]] = np.frombuffer(frames[k], np.uint8)
        entries(a["out"]["out_len"], np.uint32)[:] = ln
        entries(a["out"][HS[proto]], np.uint32)[:] = r[HS[proto]][:n]
        entries(a["out"]["rstatus"], np.int32)[:] = r["rstatus"][:n]
        if self.fault == "past":
            k = int(np.nonzero(ln)[0][0])
            a["out"]["out"][GUARD + off[k] + ln[k]] ^= 0xFF
            self.planted += 1
        if self.fault == "refused":
            for k in np.nonzero((r["rstatus"][:n] != 0) & (np.diff(off) > 0))[0][:1]:
                a["out"]["out"][GUARD + off[k]] ^= 0xFF
                self.planted += 1

    def _name_index(self, f, a, k):
        if not f or a["proto"] != "h":
            return None
        fr = deframe(f)
        if len(fr) != 1 or fr[0][0] != 1:
            return None
        blk = bytearray(fr[0][3])
        for x in walk(bytes(blk)):
            if x["kind"] == "inc" and 0 < x["index"] < 62:  # one byte, and the next index fits it too
                blk[x["start"]] += 1
                return f[:9] + bytes(blk)
        return None

    def _huff_tie(self, f, a, k):
        b = a["batch"]
        R = b["res"][k]
        raw = a["data"].tobytes()
        for h in b["hdr"][int(R["hdr_first"]):int(R["hdr_first"]) + int(R["nhdr"])]:
            s = raw[int(h["value_off"]):int(h["value_off"]) + int(h["value_len"])]
            if len(s) > 127 and huffman_len(s) == len(s):  # the cases built for the rule's boundary
                lit = HS_SYNTH.encode_int(len(s), 7, 0) + s
                if f.count(lit) == 1 and len(deframe(f) if a["proto"] == "h" else [0]) == 1:
                    return f.replace(lit, HS_SYNTH.encode_int(len(s), 7, 0x80) + huffman(s))
        return None

    def _cont_1(self, f, a, k):
        if not f or a["proto"] != "h":
            return None
        fr = deframe(f)
        if len(fr) < 2:
            return None
        p = len(f) - len(fr[-1][3]) - 1  # the last byte of the last frame header
        return f[:p] + f[p + 1:]


class GpuEnc:
    """hhuff_hpack_flatten_responses (proto "h"; slots = a permutation: through hhuff_hpack_flatten_responses_slots,
    connection c in scratch slot slots[c] of len(slots) + 3) or hhuff_qpack_flatten_responses (proto "q") through
    h2o_amd.codec on guarded device arrays.  The HPACK scratch has exactly hhuff_hpack_enc_scratch_size bytes between
    guards and moves to a new buffer in poison(), which also overwrites the device copy of the call's input; the old
    buffers stay allocated, so a stale pointer reads the pattern."""

    def __init__(self, torch, proto, sentinel, slots=None):
        self.torch, self.proto, self.sentinel, self.slots = torch, proto, sentinel, slots
        self.scratch, self.keep, self.last_in = None, [], None

    def call(self, a):
        torch, b, proto, n = self.torch, a["batch"], a["proto"], a["nres"]
        dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).view(dt)).cuda()  # noqa: E731
        inp = to_device(torch, a["in_whole"])
        out = {k: to_device(torch, v) for k, v in a["out"].items()}
        hdr = dev(b["hdr"] if b["hdr"].size else np.zeros(20, np.uint8), np.uint8)
        hdr = hdr if b["hdr"].size else hdr[:0]
        res, out_off = dev(b["res"], np.uint8), dev(b["out_off"], np.int64)
        i32 = lambda k: out[k][1].view(torch.int32)  # noqa: E731
        kw = dict(in_size=a["in_size"], out=out["out"][1], out_len=i32("out_len"), rstatus=i32("rstatus"))
        if proto == "q":
            C.qpack_flatten_responses(inp[1], hdr, res, n, out_off, b["server_off"], b["server_len"],
                                      header_len=i32("header_len"), **kw)
        else:
            nconn, cs = a["nconn"], None
            if self.slots is not None:
                assert len(self.slots) == nconn
                cs = C.ConnSlots(dev(np.asarray(self.slots, np.uint32), np.int32), None, nconn + 3)
            if self.scratch is None:
                ss = int(C.lib().hhuff_hpack_enc_scratch_size(nconn if cs is None else cs.nslots))
                self.scratch = guarded(torch, ss, self.sentinel)
            C.hpack_flatten_responses(inp[1], hdr, res, dev(b["conn_first"], np.int32), n, out_off, b["server_off"],
                                      b["server_len"], headers_size=i32("headers_size"), scratch=self.scratch[1],
                                      cont=a["cont"], slots=cs, **kw)
        torch.cuda.synchronize()
        for k, (whole, _) in out.items():
            a["out"][k][:] = whole.cpu().numpy()
        if self.scratch is not None:
            w = self.scratch[0].cpu().numpy()
            a["scratch_guards"] = np.concatenate([w[:GUARD], w[w.size - GUARD:]])
        self.last_in = inp[0]
        self.keep.append((inp, out, hdr, res, out_off))

    def poison(self, fill):
        self.last_in.fill_(fill)
        if self.scratch is not None:
            old = self.scratch
            self.scratch = guarded(self.torch, old[1].numel(), self.sentinel)
            self.scratch[1].copy_(old[1])
            old[0].fill_(fill)
            self.keep.append(old)
        self.torch.cuda.synchronize()
