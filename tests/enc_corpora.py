"""The header encoders' edge corpus: hand-built cases for hhuff_hpack_flatten_responses ("h") and the stateless
hhuff_qpack_flatten_responses ("q"), grouped so that a group is one batch per call (enc_harness.build_group).

Every case names what it must hit and carries the predicate that says so over the model's result (Case.hit):
tests/test_enc_harness.py evaluates it on the CPU, so a case that drifts off its edge fails there instead of passing
silently.  GROUPS maps a group's name to (proto, builder); group(name) builds it once."""
import functools

import numpy as np

from enc_harness import NBITS, Case, build_group, code_bits, huffman_len, make_batch, model_run, pad_to_payload, \
    strings_with, text, walk
from h2o_amd import codec as C
from h2o_amd import hpenc_synth as HE
from h2o_amd import tables as T
from hpenc_push_model import deframe

TOK, DC = C.HDR_TOKEN, C.HDR_DONT_COMPRESS
SPACE, SKIPPED, EINVAL = C.RES_SPACE, C.RES_SKIPPED, C.RES_EINVAL
M0 = 16384


def rec(headers=(), status=200, **kw):
    return dict(status=status, headers=list(headers), **kw)


def one(*records):
    """one call, one connection"""
    return [[list(records)]]


def ok(ctx, call=0):
    return all(s == 0 for s in ctx.get("rstatus", call))


def own(ctx, k, call=0):
    """record k's representations without the response's own :status (HPACK) -- the case's headers' lines"""
    f = ctx.fields(k, call)
    if ctx.proto == "h":
        return [x for x in f if not (x["kind"] == "indexed" and x["index"] < 15)]
    return f[1:]  # :status comes first


def value_of(x, s):
    """does line x carry string s as its value, in the form h2o's rule picks?"""
    v = x["value"]
    huff = huffman_len(s) < len(s)
    return v["huff"] == huff and v["len"] == (huffman_len(s) if huff else len(s))


# ------------------------------------------------------------------------------------------------
# strings (both encoders)
# ------------------------------------------------------------------------------------------------
LENS = (0, 1, 3, 4, 5, 15, 16, 17, 126, 127, 128, 254, 255, 256, 257, 258, 511, 512, 513)


def _distinct(length, count, tag):
    out, seed = [], 0
    while len(out) < count:
        s = text(length, seed=[tag, seed])
        if s not in out:
            out.append(s)
        seed += 1
    return out


def _len_case(L):
    if L == 0:
        return Case("len0", "an empty value", one(rec([(b"l0-0", b"", 0), (b"l0-1", b"", 0)])),
                    lambda ctx: ok(ctx) and [x["value"]["len"] for x in own(ctx, 0)] == [0, 0])
    vals = _distinct(L, 5, L)
    place = {v: ("mod", 4, k) for k, v in enumerate(vals[:4])}
    place[vals[4]] = ("end", 16)

    def hit(ctx):
        offs = [ctx.off(v) for v in vals]
        return (ok(ctx) and [o % 4 for o in offs[:4]] == [0, 1, 2, 3] and (offs[4] + L) % 16 == 0 and
                all(value_of(x, v) for x, v in zip(own(ctx, 0), vals)))

    return Case("len%d" % L, "values of %d bytes at offsets 0-3 modulo 4 and ending on a 16-byte line" % L,
                one(rec([(b"l%d-%d" % (L, k), v, 0) for k, v in enumerate(vals)])), hit, place=place)


def _value_case(name, must, s, want_huff, extra=None):
    def hit(ctx):
        x = own(ctx, 0)[0]
        return ok(ctx) and x["value"]["huff"] == want_huff and value_of(x, s) and (extra is None or extra(s, x))

    return Case(name, must, one(rec([(name.encode(), s, 0)])), hit)


def string_cases(proto):
    cs = [_len_case(L) for L in LENS]
    for L in (256, 257):
        cs.append(_value_case("tie-huff-%d" % L, "code bits 8 len - 8: Huffman, one byte shorter",
                              strings_with(8 * L - 8, L, seed=1), 1))
        cs.append(_value_case("tie-raw-%d" % L, "code bits 8 len - 7: as long as the string, sent raw",
                              strings_with(8 * L - 7, L, seed=2), 0))
    for n in (126, 127, 128, 255):
        cs.append(_value_case("huff-payload-%d" % n, "a Huffman payload of %d bytes (the prefix integer's steps)" % n,
                              strings_with(8 * n - 2, n + n // 3, seed=3), 1, lambda s, x, n=n: x["value"]["len"] == n))
    cs.append(Case("empty-name", "an empty name", one(rec([(b"", b"empty-name-value", 0)])),
                   lambda ctx: ok(ctx) and own(ctx, 0)[0]["name"]["len"] == 0,
                   roundtrip="h2o's decoders refuse an empty header name"))
    for name, L, bits, rule in (("stream-32", 400, 2400, lambda b: b % 32 == 0),
                                ("stream-8", 640, 3848, lambda b: b % 8 == 0 and b % 32 != 0),
                                ("stream-1mod8", 1000, 6001, lambda b: b % 8 == 1)):
        cs.append(_value_case(name, "a %d-byte string whose code has %d bits" % (L, bits), strings_with(bits, L, seed=4), 1,
                              lambda s, x, rule=rule: len(s) > 256 and rule(code_bits(s))))
    rw = strings_with(1600, 256, seed=5) + text(100, seed=5)
    cs.append(_value_case("round-word", "the first 256-byte round of a long string ends on a 32-bit word", rw, 1,
                          lambda s, x: code_bits(s[:256]) % 32 == 0))
    for L in (256, 512):
        cs.append(_value_case("long-only-%d" % L, "%d bytes of symbols of 19 bits and more: raw" % L,
                              strings_with(20 * L, L, seed=6, min_long=L), 0,
                              lambda s, x: int(NBITS[list(s)].min()) >= 19))
    lw = strings_with(20 * 256, 256, seed=7, min_long=256) + strings_with(5 * 1100, 1100, seed=7)
    cs.append(_value_case("long-wins", "256 long-code symbols, then enough 5-bit ones that Huffman wins", lw, 1,
                          lambda s, x: int(NBITS[list(s)].max()) >= 19))
    for L in (257, 300):
        nm = text(L, seed=8, name=True)

        def hit(ctx, L=L):
            a, b = own(ctx, 0)
            if ctx.proto == "q":
                return ok(ctx) and a["kind"] == b["kind"] == "literal" and a["name"]["len"] == b["name"]["len"] > 150
            return ok(ctx) and a["kind"] == b["kind"] == "inc" and a["index"] == 0 and a["name"]["huff"] and b["index"] == 62

        cs.append(Case("long-name-%d" % L, "a non-token name of %d bytes twice: a dynamic name reference (HPACK), a "
                       "literal name (QPACK)" % L, one(rec([(nm, b"first-%d" % L, 0), (nm, b"other-%d" % L, 0)])), hit))
    if proto == "q":
        for L in (6, 7, 8):
            nm = (b"&*" * 4)[:L] if L != 8 else b"*&" * 4  # 8-bit symbols: the Huffman form is no shorter, so raw

            def hit(ctx, L=L):
                n = own(ctx, 0)[0]["name"]
                return ok(ctx) and n["huff"] == 0 and n["len"] == L and n["int"][1] - n["int"][0] == (1 if L < 7 else 2)

            cs.append(Case("qname-%d" % L, "a literal name of %d bytes against the 3-bit length prefix" % L,
                           one(rec([(nm, b"qname-value-%d" % L, 0)])), hit))
    return cs


# ------------------------------------------------------------------------------------------------
# the HPACK encoder's table
# ------------------------------------------------------------------------------------------------
def kinds(ctx, k, call=0):
    return [(x["kind"], x.get("index", x.get("size"))) for x in ctx.fields(k, call)]


def table_cases():
    cs = []
    a = rec([(b"c%02d" % i, b"v", 0) for i in range(33)])
    b = rec([(b"c01", b"v", 0), (b"c00", b"v", 0), (b"c02", b"v", 0)])
    cs.append(Case("cap32", "33 small fields: the oldest of 32 entries is index 62 + 31, the first field was evicted "
                   "and goes as a literal, whose entry makes the third field the oldest",
                   [[[a]], [[b]]],
                   lambda ctx: (ok(ctx, 1) and
                                kinds(ctx, 0, 1) == [("indexed", 8), ("indexed", 93), ("inc", 0), ("indexed", 93)])))
    n1, n2 = b"x-na", b"x-nb"

    def hit(ctx):
        f = ctx.fields(0)
        return (ok(ctx) and [(x["kind"], x["index"]) for x in f[3:]] == [("inc", 63), ("inc", 62)] and
                f[3]["idx_int"] == (f[3]["start"], f[3]["start"] + 2) and f[4]["idx_int"][1] - f[4]["idx_int"][0] == 1)

    cs.append(Case("name-index", "a name match at table position 1 (index 63: two bytes under the 6-bit prefix) and 0",
                   one(rec([(n1, b"a", 0), (n2, b"b", 0), (n1, b"z", 0), (n1, b"y", 0)])), hit))

    def hit(ctx):
        f = ctx.fields(0)
        return (ok(ctx) and [(x["kind"], x["index"]) for x in f[2:]] == [("never", 62), ("never", 33)] and
                all(x["idx_int"][1] - x["idx_int"][0] == 2 for x in f[2:]))

    cs.append(Case("name-index-dc", "dont_compress: the 4-bit prefix takes two bytes for a table name and for a token of "
                   "static index 33", one(rec([(b"x-nc", b"q", 0), (b"x-nc", b"short", DC), (b"date", b"today", TOK | DC)])),
                   hit))
    n, v, v1 = b"x-big-fill", text(4054, seed=11), text(4055, seed=12)
    cs.append(Case("fill-4096", "an entry of exactly 4096 bytes is stored and indexed by the next record and the next "
                   "call; one byte more empties the table and is not stored",
                   [[[rec([(n, v, 0)]), rec([(n, v, 0)])]],
                    [[rec([(n, v, 0)]), rec([(n, v1, 0)]), rec([(n, v1, 0), (n, v, 0)]), rec([(n, v, 0)])]]],
                   lambda ctx: (ok(ctx) and ok(ctx, 1) and ctx.block(1) == b"\x88\xbe" and ctx.block(0, 1) == b"\x88\xbe" and
                                kinds(ctx, 1, 1) == [("indexed", 8), ("inc", 62)] and
                                kinds(ctx, 2, 1) == [("indexed", 8), ("inc", 0), ("inc", 0)] and
                                ctx.block(3, 1) == b"\x88\xbe")))
    n, v = b"x-cap", b"0123456789"  # an entry of 47 bytes
    sizes = (0, 32, 33, 46, 47)

    def hit(ctx):
        for c, S in enumerate(sizes):
            k1 = kinds(ctx, 2 * c + 1)
            if k1[0] != ("update", S) or k1[2:] != ([("indexed", 62)] if S >= 47 else [("inc", 0)]):
                return False
            if kinds(ctx, c, 1) != [("indexed", 8), ("indexed", 62) if S >= 47 else ("inc", 0)]:
                return False
        return ok(ctx) and ok(ctx, 1)

    cs.append(Case("cap-sizes", "header_table_size 0, 32, 33, entry - 1 and entry on a populated table, then the same "
                   "size again in the next call",
                   [[[rec([(n, v, 0)]), rec([(n, v, 0)], header_table_size=S)] for S in sizes],
                    [[rec([(n, v, 0)], header_table_size=S)] for S in sizes]], hit))
    caps = (4096, 1024, 100, 4096, 65536)
    rs = [rec([(b"x-s%d" % i, text(30, seed=20 + i), 0)], header_table_size=S) for i, S in enumerate(caps)]

    def hit(ctx):
        first = [kinds(ctx, 0)[0], kinds(ctx, 1)[0], kinds(ctx, 0, 1)[0], kinds(ctx, 1, 1)[0], kinds(ctx, 0, 2)[0]]
        return first == [("indexed", 8), ("update", 1024), ("update", 100), ("indexed", 8), ("indexed", 8)]

    cs.append(Case("cap-steps", "the capacity lowered twice, then raised: no update, the capacity stays",
                   [[rs[0:2]], [rs[2:4]], [rs[4:5]]], hit))
    c19, c20, s19, s20, d20, e19, d19 = (text(L, seed=30 + i) for i, L in enumerate((19, 20, 19, 20, 20, 19, 19)))

    def hit(ctx):
        f = ctx.fields(0)[1:]
        return (ok(ctx) and [(x["kind"], x["index"]) for x in f] ==
                [("never", 32), ("inc", 32), ("never", 55), ("inc", 55), ("inc", 0), ("never", 34), ("inc", 0)] and
                [x["value"]["huff"] for x in f] == [0, 1, 0, 1, 1, 0, 0])

    cs.append(Case("never-20", "values of 19 and 20 bytes under dont_compress and under the cookie / set-cookie tokens",
                   one(rec([(b"cookie", c19, TOK), (b"cookie", c20, TOK), (b"set-cookie", s19, TOK),
                            (b"set-cookie", s20, TOK), (b"x-dc", d20, DC), (b"etag", e19, TOK | DC), (b"x-dc2", d19, DC)])),
                   hit))
    e = b"etag"
    ca = rec([(e, b"tv-aaa", TOK), (e, b"tv-aaa", 0), (e, b"tv-aab", TOK), (e, b"tv-aab", 0)])
    cb = rec([(e, b"tv-aaa", 0), (e, b"tv-aaa", TOK), (e, b"tv-aab", 0)])
    cs.append(Case("token-vs-not", "the same name bytes with and without HHUFF_HDR_TOKEN in both orders, and another "
                   "value of equal length", [[[ca], [cb]]],
                   lambda ctx: (ok(ctx) and
                                kinds(ctx, 0)[1:] == [("inc", 34), ("indexed", 62), ("inc", 34), ("indexed", 62)] and
                                kinds(ctx, 1)[1:] == [("inc", 0), ("inc", 34), ("inc", 62)])))
    sv = rec(flags=C.RES_SERVER)
    cs.append(Case("server-indexed", "the server name is a table entry from the second response on",
                   [[[sv, sv]], [[sv]]],
                   lambda ctx: (kinds(ctx, 0) == [("indexed", 8), ("inc", 54)] and ctx.block(1) == b"\x88\xbe" and
                                ctx.block(0, 1) == b"\x88\xbe")))
    lv = text(300, seed=40)
    r3 = rec([(b"x-3c", lv, 0), (b"x-3d", b"three-calls", 0)])
    cs.append(Case("three-calls", "entries added in the first call and used in the second and third: they cross both "
                   "rings while the earlier inputs are overwritten", [[[r3]], [[r3]], [[r3]]],
                   lambda ctx: (ok(ctx, 2) and ctx.block(0, 1) == b"\x88\xbf\xbe" and ctx.block(0, 2) == b"\x88\xbf\xbe")))
    cs.append(collision_case())
    return cs


def _mix32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def string_hash(words, length):
    """hhuff_enc.h's string hash restated: words = u32 [n, k] (the strings' little-endian 4-byte words, zero past
    the end) -> hash_final(sum of word_term(w_k, k), length)"""
    k = np.arange(words.shape[1], dtype=np.uint32)
    s = _mix32(words ^ (k * np.uint32(0x9E3779B9))).sum(axis=1, dtype=np.uint32)
    return _mix32(s ^ np.uint32((length * 0x85EBCA6B) & 0xFFFFFFFF))


@functools.lru_cache(maxsize=None)
def hash_collision(n=400000, seed=80):
    """two different 8-byte values with the same string hash: a birthday search (about n^2 / 2^33 pairs among n)"""
    rng = np.random.default_rng(seed)
    raw = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz012345", np.uint8)[rng.integers(0, 32, (n, 8))]
    raw = np.unique(raw, axis=0)
    h = string_hash(np.ascontiguousarray(raw).view("<u4"), 8)
    order = np.argsort(h, kind="stable")
    same = np.nonzero(h[order][1:] == h[order][:-1])[0]
    assert same.size, "no collision among %d strings" % n
    return raw[order[same[0]]].tobytes(), raw[order[same[0] + 1]].tobytes()


def collision_case():
    """Optional case: two values of equal length and equal hhuff_enc.h string hash under one name.  The hash is a
    prefilter only, so the second value must go as a literal with the first one's name, and the first value is
    still found afterwards.  The assertion on the GPU is equality with the model, whatever the hashes are: if the
    Python restatement above goes stale the two values merely stop colliding in the kernel, which weakens this case
    but can never fail it.  The predicate checks the restatement's own verdict."""
    a, b = hash_collision()

    def hit(ctx):
        w = np.frombuffer(a + b, "<u4").reshape(2, 2)
        h = string_hash(w, 8)
        return (ok(ctx) and a != b and len(a) == len(b) == 8 and h[0] == h[1] and
                kinds(ctx, 0)[1:] == [("inc", 0), ("inc", 62), ("indexed", 63), ("indexed", 62)])

    return Case("hash-collision", "two equal-length values with the same string hash under one name",
                one(rec([(b"x-hc", a, 0), (b"x-hc", b, 0), (b"x-hc", a, 0), (b"x-hc", b, 0)])), hit)


def server_cases(proto):
    sv = rec(flags=C.RES_SERVER)
    if proto == "q":
        return [Case("server-257", "a server name of 257 bytes", one(sv, sv),
                     lambda ctx: ok(ctx) and all(ctx.fields(k)[1]["value"]["len"] > 127 for k in (0, 1)))]
    return [Case("server-257", "a server name of 257 bytes, indexed from the second response on", [[[sv, sv]], [[sv]]],
                 lambda ctx: (ctx.fields(0)[1]["value"]["len"] > 127 and ctx.block(1) == b"\x88\xbe" and
                              ctx.block(0, 1) == b"\x88\xbe"))]


SERVER_257 = text(257, seed=99)


# ------------------------------------------------------------------------------------------------
# HPACK frames
# ------------------------------------------------------------------------------------------------
_OWN = [(b":method", b"GET", TOK), (b":scheme", b"https", TOK), (b":authority", b"frames.example", TOK),
        (b":path", b"/", TOK)]


def _kind_record(kind, head, M, more=()):
    hs = [(b"x-f", head, 0)] + list(more)
    if kind == "response":
        return rec(hs, max_frame_size=M), 0
    if kind == "trailers":
        return rec(hs, flags=C.RES_TRAILERS, max_frame_size=M), 0
    if kind == "request":
        return rec(_OWN + hs, status=4, flags=C.RES_REQUEST | C.RES_END_STREAM, max_frame_size=M), 4
    return rec(_OWN + hs, status=4, flags=C.RES_PUSH_PROMISE, stream_id=2, parent_stream_id=1, max_frame_size=M), 4


def _frame_case(kind, M, P, huff=False, name=None):
    name = name or "%s-%d-%d" % (kind, M, P)
    r, h = _kind_record(kind, name.encode() + b":", M)
    padded = pad_to_payload([r], P, "h", 0, h, "huff" if huff else "raw")

    def hit(ctx):
        fr = deframe(ctx.frames(0))
        return (ok(ctx) and ctx.get("hs") == [P] and len(fr) == -(-P // M) and
                [len(f[3]) for f in fr] == [M] * ((P - 1) // M) + [P - (P - 1) // M * M])

    return Case(name, "a %s of payload %d at max_frame_size %d%s" % (kind, P, M, ", a Huffman filler" if huff else ""),
                one(*padded), hit, ref=kind != "promise" or "the reference harness has no push promises")


def payloads(M):
    return (M - 1, M, M + 1, 2 * M - 1, 2 * M, 2 * M + 1, 3 * M + 1)


def frame_cases_response():
    cs = [_frame_case("response", M, P, huff=(M, P) in ((M0, 2 * M0 + 1), (16385, 16385), (20000, 40000)))
          for M in (M0, 16385, 20000) for P in payloads(M)]
    for last in (8191, 8192, 8193):  # M + 1 above is the last chunk of one byte
        cs.append(_frame_case("response", M0, M0 + last, name="last-chunk-%d" % last))
    return cs


def frame_cases_other():
    cs = [_frame_case(kind, M0, P, huff=P == 2 * M0) for kind in ("trailers", "request", "promise") for P in payloads(M0)]
    long_value = text(600, seed=50)

    def two(name, P):
        r, _ = _kind_record("response", name.encode() + b":", M0, [(b"x-h", long_value, 0)])
        return pad_to_payload([r], P, "h", 0, 0, "raw")

    def hit(ctx):
        x = ctx.fields(0)[-1]["value"]
        return ok(ctx) and x["huff"] and x["len"] >= 257 and x["pay"][0] < M0 < x["pay"][1] - 1

    cs.append(Case("boundary-in-long-huffman", "a frame boundary inside a long-path Huffman payload",
                   one(*two("boundary-in-long-huffman", M0 + 200)), hit))
    probe = two("boundary-in-integer", M0 + 300)
    res = model_run("h", [make_batch([probe], "h")])[0]
    blk = b"".join(f[3] for f in deframe(res["out"][:int(res["out_len"][0])].tobytes()))
    start = walk(blk)[-1]["value"]["int"][0]

    def hit(ctx):
        x = ctx.fields(0)[-1]["value"]
        return ok(ctx) and x["int"] == (M0 - 1, M0 + 2)

    cs.append(Case("boundary-in-integer", "a frame boundary inside a three-byte prefix integer",
                   one(*two("boundary-in-integer", M0 + 300 + (M0 - 1) - start)), hit))
    r, _ = _kind_record("response", b"boundary-at-content-length:", M0)
    r["content_length"] = 12345
    cs.append(Case("boundary-at-content-length", "a frame boundary at the first byte of the content-length field",
                   one(*pad_to_payload([r], M0 + 8, "h", 0, 0, "raw")),
                   lambda ctx: ok(ctx) and ctx.block(0)[M0:M0 + 3] == b"\x0f\x0d\x05"))
    return cs


# ------------------------------------------------------------------------------------------------
# regions and the end of the input
# ------------------------------------------------------------------------------------------------
LAST = b"the-last-string-of-the-input"


def _patch_past(b, call, rows):
    if call != 0:
        return
    h = b["hdr"][rows[2]]
    h["value_off"] = b["data"].size + 1 - int(h["value_len"])


def region_cases(proto):
    sts = lambda *s: (lambda ctx: ctx.get("rstatus") == list(s))  # noqa: E731
    cs = [Case("short-one-frame", "a one-frame record in a region one byte short",
               one(rec([(b"x-r1", text(40, seed=60), 0)])), sts(SPACE), shorts=[(0, 0)])]
    mid = [rec([(b"x-m%d" % i, text(24, seed=61 + i), 0)]) for i in range(4)]
    if proto == "h":
        three = pad_to_payload([rec([(b"x-f", b"short-three:", 0)])], 2 * M0 + 1, "h", 0, 0, "raw")
        cs.append(Case("short-three-frames", "a three-frame record in a region one byte short: the 9 bytes of each "
                       "CONTINUATION count", one(*three),
                       lambda ctx: (ctx.get("rstatus") == [SPACE] and len(deframe(ctx.frames(0))) == 3 and
                                    ctx.get("out_len", want=True) == [2 * M0 + 1 + 27]), shorts=[(0, 0)]))
        cs.append(Case("short-mid", "a short region in the middle of a connection: the later records are SKIPPED, in the "
                       "next call too", [[mid[:3]], [mid[3:]]],
                       lambda ctx: ctx.get("rstatus") == [0, SPACE, SKIPPED] and ctx.get("rstatus", 1) == [SKIPPED],
                       shorts=[(0, 1)]))
    else:
        cs.append(Case("short-mid", "a short region between two records: the stateless encoder goes on", one(*mid[:3]),
                       sts(0, SPACE, 0), shorts=[(0, 1)]))
        for n in (63, 64, 16383, 16384):
            for short in (False, True):
                name = "q%s-%d" % ("short" if short else "fit", n)
                r = pad_to_payload([rec([(b"x-q", name.encode() + b":", 0)])], n, "q", 0, 0, "raw")
                cs.append(Case(name, "a field section of %d bytes (the frame length varint's steps)%s"
                               % (n, ", region one byte short" if short else ""), one(*r),
                               lambda ctx, n=n, short=short, v=1 if n < 64 else 2 if n < 16384 else 4: (
                                   ctx.get("hs", want=True) == [n] and ctx.get("out_len", want=True) == [1 + v + n] and
                                   ctx.get("rstatus") == [SPACE if short else 0]),
                               shorts=[(0, 0)] if short else ()))
    cs.append(Case("in-size-end", "a string whose last byte is in[in_size - 1]", one(rec([(b"x-end", LAST, 0)])),
                   lambda ctx: ok(ctx) and ctx.off(LAST) + len(LAST) == ctx.batch()["data"].size, place={LAST: ("last",)}))
    after = rec([(b"x-after", b"1", 0)])
    cs.append(Case("past-in-size", "a string that ends at in_size + 1: HHUFF_RES_EINVAL",
                   one(rec([(b"x-past", b"past-the-end", 0)]), after), sts(EINVAL, SKIPPED if proto == "h" else 0),
                   patch=_patch_past))
    return cs


# ------------------------------------------------------------------------------------------------
# QPACK static lookups
# ------------------------------------------------------------------------------------------------
def static_cases():
    static = {}
    for i, (n, v) in enumerate(T.QPACK_STATIC_TABLE):
        static.setdefault((n, v), i)
    statuses = sorted(int(v) for (n, v) in static if n == b":status")
    assert len(statuses) == 14

    def hit(ctx):
        for k, st in enumerate(statuses):
            f = ctx.fields(k)[0]
            if (f["kind"], f["index"]) != ("indexed", static[(b":status", b"%d" % st)]):
                return False
        return ok(ctx) and all(ctx.fields(len(statuses) + k)[0]["kind"] == "nameref" for k in (0, 1))

    cs = [Case("status-static", "every :status with a static entry, and 201 and 599 without one",
               one(*[rec(status=s) for s in statuses + [201, 599]]), hit)]
    cs.append(Case("content-length-0", "content-length 0 is a static entry", one(rec(content_length=0)),
                   lambda ctx: ok(ctx) and (ctx.fields(0)[1]["kind"], ctx.fields(0)[1]["index"]) == ("indexed", 4)))
    cs.append(Case("token-static", "a token whose name and value match a static entry, and one whose name alone does",
                   one(rec([(b"content-type", b"text/css", TOK), (b"content-type", b"text/x-edge", TOK),
                            (b"content-type", b"text/css", 0)])),
                   lambda ctx: ok(ctx) and [x["kind"] for x in own(ctx, 0)] == ["indexed", "nameref", "literal"]))
    cs.append(Case("request-static", "a request (HHUFF_QRES_REQUEST): :method GET, :scheme https and :path / are static "
                   "entries, :authority a name reference",
                   one(rec(_OWN + [(b"x-rq", b"request-static", 0)], status=4, qrequest=True)),
                   lambda ctx: (ok(ctx) and [(x["kind"], x.get("index")) for x in ctx.fields(0)] ==
                                [("indexed", 17), ("indexed", 23), ("nameref", 0), ("indexed", 1), ("literal", None)])))
    d257 = text(257, seed=70)
    cs.append(Case("datagram", "HHUFF_QRES_DATAGRAM with a value of 0 bytes and of 257",
                   one(rec(dfid=b""), rec(dfid=d257)),
                   lambda ctx: (ok(ctx) and ctx.fields(0)[-1]["value"]["len"] == 0 and value_of(ctx.fields(1)[-1], d257) and
                                ctx.fields(1)[-1]["kind"] == "literal")))
    return cs


# ------------------------------------------------------------------------------------------------
GROUPS = {
    "h-strings": ("h", lambda: string_cases("h"), HE.SERVER),
    "q-strings": ("q", lambda: string_cases("q"), HE.SERVER),
    "h-table": ("h", table_cases, HE.SERVER),
    "h-server": ("h", lambda: server_cases("h"), SERVER_257),
    "q-server": ("q", lambda: server_cases("q"), SERVER_257),
    "h-frames-response": ("h", frame_cases_response, HE.SERVER),
    "h-frames-other": ("h", frame_cases_other, HE.SERVER),
    "h-regions": ("h", lambda: region_cases("h"), HE.SERVER),
    "q-regions": ("q", lambda: region_cases("q"), HE.SERVER),
    "q-static": ("q", static_cases, HE.SERVER),
}
HPACK_GROUPS = [g for g, v in GROUPS.items() if v[0] == "h"]


@functools.lru_cache(maxsize=None)
def cases(name):
    from oracle import oracle as O

    O.build()  # the cases are sized on the model, at collection time too: what conftest's oracle_codec does
    return tuple(GROUPS[name][1]())


@functools.lru_cache(maxsize=None)
def group(name, ref_only=False):
    """the built group (enc_harness.build_group); ref_only: without the cases the reference harness does not accept"""
    proto, _, server = GROUPS[name]
    return build_group(cases(name), proto, server, keep=(lambda c: c.ref is True) if ref_only else None)


def input_bytes():
    """the corpus' input, all calls of all groups"""
    return sum(int(b["data"].size) for name in GROUPS for b in group(name)["calls"])
