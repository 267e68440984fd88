"""The hand-built HPACK corpora of the header-block edge tests (built with blocks_harness' builders; QPACK's are in
qpack_corpora.py).  A corpus is dict(name, table_size, cases, modes, ...): `modes` lists the modes of its calls
("plain", "req", "res"); `alone` corpora run each case as a batch of its own, without spacers, so that the case's
first block starts at input byte 0 and its literals are the first of the literal list."""
import functools

import numpy as np

from blocks_harness import (case, ccase, huff_of_len, huff_variants, indexed, integer, literal, raw_string, size_update,
                            string)

GET, HTTPS = indexed(2), indexed(7)  # :method GET, :scheme https
A = lambda n, c=b"a": c * n  # noqa: E731


def stages_from_source():
    """IN_STAGE and OUT_STAGE of the staged kernel that decodes header literals: DEC_S's template arguments in
    csrc/hhuff_kernels.hip"""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "h2o_amd", "csrc",
                            "hhuff_kernels.hip")).read()
    m = re.search(r"#define DEC_S decode_staged_kernel<\w+, (\d+), (\d+),", src)
    return int(m.group(1)), int(m.group(2))


IN_STAGE, OUT_STAGE = stages_from_source()


def tile_plan(block, payloads):
    """What decode_staged_kernel plans for a tile of 64 literals (hhuff_kernels.hip, the plan lambda, as the literal
    pre-pass calls it: offsets and lengths in pairs, raw literals with length 0): the input span from the first
    Huffman payload's start down to a multiple of 16 to the last one's end up to one, and the output stage extent,
    the sum of floor(8 len / 5) + 3 over the tile.  The tile is staged in LDS when span <= IN_STAGE and ospan <=
    OUT_STAGE, else every lane decodes from global memory.  payloads: [(offset in block, length, Huffman?)], checked
    against the block's bytes (a one-byte length in front of every payload).  -> (span, ospan, staged)"""
    assert len(payloads) == 64
    for off, ln, h in payloads:
        assert ln < 127 and block[off - 1] == (0x80 if h else 0) | ln, (off, ln, h)
    huff = [(o, ln) for o, ln, h in payloads if h and ln]
    lo, hi = min(o for o, _ in huff), max(o + ln for o, ln in huff)
    span = (hi + 15) // 16 * 16 - lo // 16 * 16
    ospan = sum((8 * (ln if h else 0)) // 5 + 3 for _, ln, h in payloads)
    return span, ospan, span <= IN_STAGE and ospan <= OUT_STAGE


def stage_tiles(rng, line, lead, pad):
    """The 64-literal tiles of the stage cases.  line(payload, huffman) -> a field line whose last bytes are a
    one-byte length and the payload; lead = bytes in front of the first line; pad = a one-byte field line (16 of
    them in front move `lo` into the next 16-byte unit).  -> [(name, bytes after the lead, payloads, staged?)]
      input stage: a Huffman literal at each end of the span and seven short ones inside, raw literals (no part of
        the span or the output extent) in between: the Huffman bytes stay far below OUT_STAGE, so IN_STAGE decides
      output stage: 64 Huffman literals of 43 to 45 bytes, their span below IN_STAGE: OUT_STAGE decides"""
    def build(lens, huffs, pre=b""):
        out, pays = bytearray(pre), []
        for ln, h in zip(lens, huffs):
            p = huff_of_len(rng, ln) if h else bytes(rng.integers(97, 123, ln, dtype=np.uint8))
            ln_ = line(p, h)
            pays.append((lead + len(out) + len(ln_) - ln, ln, h))
            out += ln_
        return bytes(out), pays

    gap = len(line(b"", False))  # bytes of a line in front of its payload
    tiles = []
    for tag, pre, hi, staged in (("IN_STAGE - 16", 0, IN_STAGE - 16, True), ("IN_STAGE", 0, IN_STAGE, True),
                                 ("IN_STAGE + 1", 0, IN_STAGE + 1, False), ("IN_STAGE + 16", 0, IN_STAGE + 16, False),
                                 ("IN_STAGE from the next 16-byte unit", 16, IN_STAGE + 16, True),
                                 ("IN_STAGE + 16 from the next 16-byte unit", 16, IN_STAGE + 32, False)):
        huffs = [k in (0, 63) or k % 8 == 0 for k in range(64)]
        lens = [30 if k in (0, 63) else 10 if huffs[k] else 0 for k in range(64)]
        lo = lead + pre + gap
        rest = hi - lo - 63 * gap - sum(lens)  # the raw payloads' bytes
        raws = [k for k in range(64) if not huffs[k]]
        for j, k in enumerate(raws):
            lens[k] = rest // len(raws) + (1 if j < rest % len(raws) else 0)
        blk, pays = build(lens, huffs, pad * pre)
        assert pays[63][0] + 30 == hi and pays[0][0] == lo
        tiles.append(("tile input span, %s" % tag, blk, pays, staged))
    base = [43] * 32 + [44] * 32  # sum of floor(8 len / 5) + 3 = 32 * 71 + 32 * 73 = 4608
    assert sum(8 * ln // 5 + 3 for ln in base) == OUT_STAGE
    for tag, lens, staged in (("OUT_STAGE - 2", [43] * 33 + [44] * 31, True), ("OUT_STAGE", base, True),
                              ("OUT_STAGE + 4", [43] * 31 + [44] * 32 + [45], False)):
        blk, pays = build(lens, [True] * 64)
        tiles.append(("tile output extent, %s" % tag, blk, pays, staged))
    return tiles


def mini(k):
    """a minimum-size entry: a one-byte name, an empty value (33 bytes of the table)"""
    return literal(string(bytes([97 + k % 26]), False), string(b"", False))


def fill(n):
    return b"".join(mini(k) for k in range(n))


# ------------------------------------------------------------------------------------------------
def integers():
    v = string(b"v", False)
    cs = [
        case("index 0", [b"\x80"]),
        case("index 61", [indexed(61), indexed(1)]),
        case("index 62, empty table", [indexed(62)]),
        case("index 62+num-1", [fill(3), indexed(64) + indexed(62)]),
        case("index 62+num", [fill(3), indexed(65)]),
        case("7f 00 empty", [b"\x7f\x00" + v]),
        case("7f 00 filled", [fill(3), b"\x7f\x00" + v, indexed(62)]),
        case("0f 00", [b"\x0f\x00" + v]),
        case("1f 00", [b"\x1f\x00" + v]),
        case("3f 00", [b"\x3f\x00" + GET, b"\x3f\x00"]),
        case("ff 00 empty", [b"\xff\x00"]),
        case("ff 00 filled", [fill(70), b"\xff\x00" + indexed(62 + 69) + indexed(62 + 70)]),
        case("2^63", [indexed(2 ** 63, 10)]),
        case("2^63-1+127 as a string length", [literal(1, integer(2 ** 63 - 1, 7, 0, 10) + b"xx", "never")]),
        case("string length 2^63", [literal(1, integer(2 ** 63, 7, 0x80, 10) + b"xx", "never")]),
        case("ninth octet continues", [indexed(127, 11)], [literal(1, integer(127, 7, 0, 11) + b"x", "never")],
             [size_update(31, 11)], [literal(127, v, "inc")[:1] + b"\x80" * 9 + b"\x00" + v]),
        case("ninth octet continues, the index exists", [fill(70), indexed(127, 11)], [fill(70), indexed(127, 10) + GET],
             [fill(70), literal(127, v, "never")[:1] + b"\x80" * 9 + b"\x00" + v],
             [literal(string(b"n", False), integer(127, 7, 0, 11) + A(127), "never")],
             [fill(3), size_update(31, 11) + indexed(62)]),
        case("block ends after a name", [literal(string(b"name", False), b"")], [literal(string(b"name", True), b"")],
             [GET + literal(1, b"", "never")]),
        case("trailing size update", [GET + size_update(100)], [size_update(0)], [GET, size_update(64) + size_update(0)]),
        case("literal ends at the block end", [literal(1, raw_string(b"12345"), "never")]),
        case("literal ends a byte past the block", [literal(1, raw_string(b"12345")[:-1], "never")],
             [literal(1, raw_string(huff_of_len(np.random.default_rng(1), 9), True)[:-1], "never")],
             [GET + literal(raw_string(b"name")[:-1], b"", "inc")]),
    ]
    # non-minimal integers: 127 as 2 .. 10 bytes, for an index (table filled so that it exists), a name index, a
    # string length and a size update
    for nb in range(2, 11):
        cs.append(case("non-minimal %d bytes" % nb,
                       [fill(70), indexed(127, nb) + literal(string(b"n", False), integer(127, 7, 0, nb) + A(127), "never")
                        + size_update(31, nb) + integer(15, 4, 0x10, nb) + v + integer(63, 6, 0x40, nb) + v]))
    # an integer cut by the block end after each of its bytes
    for rep, enc in (("index", indexed(300000)), ("name index", integer(300000, 4, 0x10)),
                     ("size update", size_update(300000)), ("length", literal(1, integer(300000, 7), "never")),
                     ("ten-byte index", indexed(2 ** 62, 10))):
        cs.append(case("%s cut" % rep, *[[GET + enc[:k]] for k in range(1, len(enc) + 1)]))
    rng = np.random.default_rng(2)
    for L in (126, 127, 128, 16510):
        cs.append(case("string length %d" % L, [literal(1, raw_string(A(L)), "never") + GET,
                                                 literal(raw_string(huff_of_len(rng, L), True), v, "inc") + indexed(62)],
                       ent=0, room=4 * L + 64))
    return dict(name="integers", table_size=4096, cases=cs, modes=["plain"])


# ------------------------------------------------------------------------------------------------
TABLE_SIZES = (0, 31, 32, 33, 100, 4096, 4097, 65536)


def table(ts):
    E = ts // 32 + 1  # the ring's entries
    live = ts // 33   # minimum-size entries that fit
    n = lambda k: string(b"n" * k, False)  # noqa: E731
    cs = []
    if ts >= 32:
        body = ts - 32
        ent = literal(n(min(body, 1)), string(A(body - min(body, 1)), False))
        cs.append(case("entry of exactly cap", [GET + ent + indexed(62), indexed(62) + indexed(63)], ent=0,
                       room=3 * ts + 64))
        big = literal(n(1), string(A(body), False))
        cs.append(case("entry of cap+1", [mini(0) + indexed(62) + big, GET + indexed(62)], ent=0, room=2 * ts + 64))
    else:
        cs.append(case("nothing fits", [mini(0) + GET, indexed(62)]))
    cs.append(case("three ring lengths of minimum entries",
                   [fill(3 * E) + indexed(62), indexed(62) + indexed(62 + max(live, 1) - 1), indexed(62 + live)], ent=2))
    if ts >= 32:
        # an empty name and an empty value cost 32 bytes: table_size / 32 live entries, all the ring holds but one
        empty = literal(string(b"", False), string(b"", False))
        cs.append(case("three ring lengths of 32-byte entries",
                       [mini(0) + empty * (3 * E) + indexed(62), indexed(62) + indexed(62 + ts // 32 - 1),
                        indexed(62 + ts // 32), indexed(62) + mini(1) + indexed(62) + indexed(62 + (ts - 33) // 32),
                        indexed(62 + (ts - 33) // 32 + 1)], ent=2))
    cs.append(case("size update to 0 and back", [mini(0) + size_update(0) + size_update(ts) + mini(1) + indexed(62),
                                                 indexed(62), indexed(63)]))
    cs.append(case("size update to the maximum", [mini(0) + size_update(ts) + indexed(62), indexed(62)]))
    cs.append(case("size update to the maximum plus one", [mini(0) + size_update(ts + 1) + indexed(62)]))
    cs.append(case("two size updates in a row", [fill(3) + size_update(ts // 2) + size_update(ts) + indexed(62),
                                                 size_update(33) + size_update(34) + indexed(62), indexed(63)]))
    cs.append(case("size update between two fields", [mini(0) + mini(1) + GET, GET + size_update(40) + indexed(62)]))
    cs.append(case("an entry with soft bits",
                   [literal(string(b"a b", False), string(b"\x01v", False)) + indexed(62),
                    indexed(62) + literal(62, string(b"ok", False), "never"),
                    literal(string(b"a\x7fb", True), string(b" v", True)) + indexed(62) + indexed(63)]))
    if ts >= 100:
        # size + the new entry == the capacity: nothing is evicted
        exact = literal(n(1), string(A(ts - 66), False))
        cs.append(case("an insert fills the table exactly", [mini(0) + exact + indexed(63), indexed(63) + indexed(62),
                                                             mini(1) + indexed(63) + indexed(64)], ent=0, room=3 * ts))
        # the entry the insert's name refers to is evicted by that insert: 42 bytes live, the new entry takes all
        old = literal(n(10), string(b"", False))
        new = literal(62, string(A(ts - 42, b"v"), False))
        cs.append(case("insert evicts its own name reference", [old, new + indexed(62), indexed(62)], ent=0, room=3 * ts))
        cs.append(case("insert evicts its own name reference, two left", [old + mini(0), literal(63, string(
            A(ts - 42 - 33 + 1, b"w"), True)) + indexed(62), indexed(62) + indexed(63)], ent=0, room=3 * ts + 256))
    return dict(name="table_%d" % ts, table_size=ts, cases=cs, modes=["plain"])


# ------------------------------------------------------------------------------------------------
def _arena_block(items, probe, short):
    """items: [(bytes, [(need, taken), ...] per string)].  -> (block, slice): the slice that holds every string of the
    block exactly (short = 0) or that is `short` bytes too small for string `probe` = (item, string)"""
    cur, need_all = 0, 0
    for i, (_, strs) in enumerate(items):
        for j, (need, taken) in enumerate(strs):
            if short and (i, j) == probe:
                return b"".join(b for b, _ in items), cur + need - short
            need_all = max(need_all, cur + need)
            cur += taken
    return b"".join(b for b, _ in items), need_all


def arena():
    rng = np.random.default_rng(3)
    h = huff_of_len(rng, 20)
    from oracle import oracle as O

    hd = len(O.oracle().decode(h)[0])
    assert hd < 32
    bad = huff_variants(rng, 20)[2][1]
    filler = (GET, [(7, 7), (3, 3)])
    setup = literal(string(b"dname-xyz", False), string(b"dvalue-12345", False))
    kinds = {  # the field and its strings; the probed string
        "static name": ((literal(1, string(b"x", False), "never"), [(10, 10), (1, 1)]), 0),
        "static value": ((GET, [(7, 7), (3, 3)]), 1),
        "dynamic name": ((literal(62, string(b"x", False), "never"), [(9, 9), (1, 1)]), 0),
        "dynamic value": ((indexed(62), [(9, 9), (12, 12)]), 1),
        "raw literal": ((literal(string(b"rawname", False), string(b"rawvalue!", False), "without"), [(7, 7), (9, 9)]), 1),
        "raw name": ((literal(string(b"rawname", False), string(b"rawvalue!", False), "without"), [(7, 7), (9, 9)]), 0),
        "Huffman literal": ((literal(1, raw_string(h, True), "never"), [(10, 10), (32, hd)]), 1),
        "Huffman name": ((literal(raw_string(h, True), string(b"v", False), "never"), [(32, hd), (1, 1)]), 0),
    }
    cs = []
    for kind, (item, j) in kinds.items():
        for where, items, i in (("first", [item, filler, filler], 0), ("middle", [filler, item, filler], 1),
                                ("last", [filler, filler, item], 2)):
            for short in (0, 1):
                blk, sl = _arena_block(items, (i, j), short)
                cs.append(case("%s %s, %s" % (kind, where, "one byte short" if short else "exact fit"),
                               [setup, blk, GET], arena={(0, 0, 1): sl}))
    item = kinds["Huffman literal"][0]
    # room for the decoded bytes, not for floor(8 len / 5)
    for extra in (0, 31 - hd):
        cs.append(case("Huffman literal fits decoded (+%d)" % extra, [GET + item[0], GET],
                       arena={(0, 0, 0): 10 + 10 + hd + extra}))
    cs.append(case("Huffman name fits decoded", [kinds["Huffman name"][0][0]], arena={(0, 0, 0): hd + 1}))
    for sl in (0, 2, 5):
        cs.append(case("upper-case raw name, slice of %d" % sl, [literal(string(b"Upper", False), string(b"v", False))],
                       arena={(0, 0, 0): sl}))
        cs.append(case("upper-case raw name behind a field, slice of %d" % (10 + sl),
                       [GET + literal(string(b"uppeR", False), string(b"v", False))], arena={(0, 0, 0): 10 + sl}))
    cs.append(case("bad Huffman value, slice too small", [literal(1, raw_string(bad, True), "never")],
                   arena={(0, 0, 0): 10 + 31}))
    cs.append(case("bad Huffman value, slice fits", [literal(1, raw_string(bad, True), "never")],
                   arena={(0, 0, 0): 10 + 32}))
    cs.append(case("bad Huffman name, slice too small", [literal(raw_string(bad, True), string(b"v", False), "never")],
                   arena={(0, 0, 0): 31}))
    cs.append(case("zero-byte slice", [GET], [size_update(0)], [literal(string(b"", False), string(b"", False))],
                   [literal(string(b"a", False), string(b"", False))],
                   arena={(0, 0, 0): 0, (1, 0, 0): 0, (2, 0, 0): 0, (3, 0, 0): 0}))
    return dict(name="arena", table_size=4096, cases=cs, modes=["plain"])


# ------------------------------------------------------------------------------------------------
def slots():
    rng = np.random.default_rng(4)
    lit = b"".join(literal(string(bytes(rng.integers(97, 123, 12, dtype=np.uint8))), string(
        bytes(rng.integers(97, 123, 40, dtype=np.uint8)))) for _ in range(12))
    full = {L: GET * L for L in (1, 64, 65, 4096)}
    cs = [case("nfields == L", [full[1]], [full[64]], [lit], [full[65]], [full[4096]], [lit], ent=16),
          case("nfields == L, blocks of one connection", [full[64], full[65], lit, full[1], full[1], full[4096], lit],
               ent=16)]
    return dict(name="slots", table_size=4096, cases=cs, modes=["plain"])


# ------------------------------------------------------------------------------------------------
HUFF_LENS = (0, 1, 511, 512, 513, 4095, 4096, 4097, 65535, 65536, 65537)
RAW_LENS = (0, 1, 511, 512, 513, 1536, 65536)


def _as_name_and_value(tag, payload, h, cs):
    """the payload as a name and as a value, each with and without incremental indexing, read back where indexed"""
    s = raw_string(payload, h)
    L = len(payload)
    sl = (8 * (L + 16)) // 5 + 64
    for how in ("inc", "never"):
        back = [indexed(62)] if how == "inc" else []
        ar = {(0, 0, 0): sl, (0, 0, 1): sl, (1, 0, 0): sl, (1, 0, 1): sl}
        cs.append(case("%s, %s" % (tag, how), [literal(s, string(b"v", False), how)] + back,
                       [literal(1, s, how)] + back, arena=ar))


def long_literals():
    rng = np.random.default_rng(5)
    cs = []
    for L in HUFF_LENS:
        for tag, p in huff_variants(rng, L):
            _as_name_and_value("Huffman %d %s" % (L, tag), p, True, cs)
    low = lambda L: bytes(rng.integers(97, 123, L, dtype=np.uint8))  # noqa: E731
    for L in RAW_LENS:
        _as_name_and_value("raw %d" % L, low(L), False, cs)
        if L > 512:
            for at in sorted(set(o for o in (0, 15, 16, 1023, 1024, L - 1) if o < L)):
                p = bytearray(low(L))
                p[at] = 0x01
                _as_name_and_value("raw %d, invalid character at %d" % (L, at), bytes(p), False, cs)
    L = 1536
    names = {"soft before upper-case": {100: b" ", 900: b"Q"}, "upper-case before soft": {100: b"Q", 900: b" "},
             "upper-case only": {1535: b"Z"}, "upper-case first": {0: b"A"},
             "soft and upper-case in one lane's bytes": {1029: b"\x7f", 1030: b"Q"},
             "upper-case and soft in one lane's bytes": {1029: b"Q", 1030: b"\x7f"},
             "leading ':'": {0: b":", 5: b"Q", 700: b" "}, "':' not leading": {1: b":", 5: b"Q"}}
    for tag, edits in names.items():
        p = bytearray(low(L))
        for at, c in edits.items():
            p[at:at + 1] = c
        sl = (8 * L) // 5 + 64
        cs.append(case("long raw name, %s" % tag, [literal(raw_string(bytes(p)), string(b"v", False), "inc"), indexed(62)],
                       arena={(0, 0, 0): sl, (0, 0, 1): sl}))
    for tag, at, c in (("a space first", 0, b" "), ("a tab first", 0, b"\t"), ("a space last", L - 1, b" "),
                       ("a tab last", L - 1, b"\t"), ("a space inside", 700, b" ")):
        p = bytearray(low(L))
        p[at:at + 1] = c
        sl = (8 * L) // 5 + 64
        cs.append(case("long raw value, %s" % tag, [literal(1, raw_string(bytes(p)), "inc"), indexed(62)],
                       arena={(0, 0, 0): sl, (0, 0, 1): sl}))
    return dict(name="long", table_size=65536, cases=cs, modes=["plain"], shapes=(None,))


def stage():
    """tiles of 64 consecutive literals on either side of the staged kernel's input and output stages (stage_tiles);
    every case alone, its block at input byte 0, so that its literals are the literal list's first tile"""
    rng = np.random.default_rng(6)
    cs = []
    for name, blk, pays, staged in stage_tiles(rng, lambda p, h: literal(1, raw_string(p, h), "never"), 0, GET):
        k = case(name, [blk, GET])
        k["plan"] = tile_plan(blk, pays) + (staged,)
        cs.append(k)
    return dict(name="stage", table_size=4096, cases=cs, modes=["plain"], alone=True)


# ------------------------------------------------------------------------------------------------
def prepass():
    rng = np.random.default_rng(7)
    hv = raw_string(huff_of_len(rng, 30), True)
    cs = [
        case("value header at byte 31", [GET * 30 + literal(1, hv, "never") + literal(1, hv, "inc") + indexed(62)]),
        case("value header at byte 32", [GET * 31 + literal(1, hv, "never") + literal(1, hv, "inc") + indexed(62)]),
        case("name header at byte 31, value header at 32",
             [GET * 30 + literal(string(b"", False), hv, "inc") + indexed(62)]),
        case("name header at byte 32", [GET * 31 + literal(hv, hv, "inc") + indexed(62)]),
    ]
    # the padding field (0x10, a one-byte name, a raw value) ends at byte 32766: 0x40 there, the name header behind it
    blk = next(b for b in (b"\x10" + string(b"p", False) + raw_string(A(n)) for n in range(32740, 32766)) if len(b) == 32766)
    cs.append(case("name header at byte 32767",
                   [blk + literal(raw_string(huff_of_len(rng, 5), True), hv, "inc") + indexed(62)], ent=2))
    cs.append(case("an index past the table, then literals",
                   [indexed(70) + literal(hv, hv, "inc") + literal(1, raw_string(A(600)), "never"), GET]))
    return dict(name="prepass", table_size=4096, cases=cs, modes=["plain"], alone=True)


def big():
    """about 8.5 MiB: 140 one-block connections, each a Huffman field, a never-indexed raw value of about 60 KB and
    another Huffman field; literal-bearing fields lie before, across and after input byte 8 MiB"""
    rng = np.random.default_rng(8)
    conns, ar = [], {}
    for c in range(140):
        hv = raw_string(huff_of_len(rng, 20 + c % 7), True)
        padlen = 62000 + 37 * c + (5 if c == 139 else 0)
        blk = (literal(hv, hv, "inc") + literal(1, raw_string(bytes(rng.integers(97, 123, padlen, dtype=np.uint8))), "never")
               + literal(1, hv, "inc") + indexed(62) + indexed(63))
        conns.append([blk])
        ar[(c, 0, 0)] = (8 * len(blk)) // 5 + 256
    total = sum(len(c[0]) for c in conns)
    assert total > (8 << 20) + 300000 and total % 32 != 0
    return dict(name="big", table_size=4096, cases=[case("8.5 MiB", *conns, arena=ar)], modes=["plain"], shapes=(None,),
                spacers=False)


# ------------------------------------------------------------------------------------------------
def _untouched(k):
    return [[GET] if i % 2 else [] for i in range(k)]


def continuation(ncalls):
    rng = np.random.default_rng(9)
    h = lambda s: string(s, True)  # noqa: E731
    r = lambda s: string(s, False)  # noqa: E731
    mid = ncalls - 2
    read = [indexed(62), literal(62, r(b"again"), "never") + indexed(62)]
    cs = []
    for tag, ins in (("static name, raw value", literal(1, r(b"raw-value-0123456789"))),
                     ("static name, Huffman value", literal(1, h(b"huffman-value-0123456789"))),
                     ("raw name, Huffman value", literal(r(b"raw-name"), h(b"huffman value"))),
                     ("Huffman name, raw value", literal(h(b"huffman-name"), r(b"raw value"))),
                     ("dynamic name", literal(r(b"first-name"), r(b"one")) + literal(62, h(b"second value"))),
                     ("long raw value", literal(1, raw_string(bytes(rng.integers(97, 123, 700, dtype=np.uint8))))),
                     ("long Huffman value", literal(1, raw_string(huff_of_len(rng, 700), True)))):
        cs.append(ccase("%s kept over %d calls" % (tag, mid), [[ins]] + _untouched(mid) + [read], ent=1200))
    cs.append(ccase("no block in a middle call", [[mini(0) + mini(1)]] + [[]] * mid + [[indexed(62) + indexed(63)]]))
    cs.append(ccase("lowered capacity decides a later eviction",
                    [[size_update(100) + mini(0) + mini(1)], [GET], [mini(2) + mini(3)]] + [[]] * (ncalls - 4)
                    + [[indexed(62) + indexed(63) + indexed(64), indexed(65)]]))
    cs.append(ccase("fails in the second call", [[mini(0)], [indexed(62), indexed(99), GET]]
                    + [[GET, indexed(62)]] * (ncalls - 2)))
    cs.append(ccase("arena error in the second call", [[mini(0)], [GET]] + [[GET, indexed(62)]] * (ncalls - 2),
                    arena={(0, 1, 0): 9}))
    old = literal(r(b"n" * 10), r(b""))
    cs.append(ccase("insert evicts a name reference of an earlier call",
                    [[size_update(100) + old], [], [literal(62, r(b"v" * 58)) + indexed(62)]] + [[]] * (ncalls - 4)
                    + [[indexed(62), indexed(63)]], ent=100))
    # entries move inside the rings when newer ones arrive: every live entry is read back in the last call
    def ent(i, k):
        value = b"value %d/%d " % (i, k) + bytes([65 + k]) * (k % 7)
        return literal(r(b"name-%d-%02d" % (i, k)), (h if k % 2 else r)(value))

    cs.append(ccase("every entry read back after inserts in every call",
                    [[b"".join(ent(i, k) for k in range(9 + i))] for i in range(ncalls - 1)]
                    + [[b"".join(indexed(62 + j) for j in range(sum(9 + i for i in range(ncalls - 1)))), indexed(62)]]))
    cs.append(ccase("ring refilled in every call", *[[[fill(40 + 3 * i) + indexed(62 + i)] for i in range(ncalls)]]))
    return dict(name="continuation_%d" % ncalls, table_size=4096, cases=cs, modes=["plain"] * ncalls, shapes=(None, 65))


def continuation_empty_call():
    """a middle call with no input at all (in_size 0): no connection has a block there"""
    cs = [ccase("entries over an empty call", [[mini(0) + literal(1, string(b"huffman-value-0123456789", True))], [GET],
                                               [], [indexed(62) + indexed(63)], [indexed(62)]]),
          ccase("failed over an empty call", [[indexed(62)], [GET], [], [GET], [GET]])]
    return dict(name="continuation_empty_call", table_size=4096, cases=cs, modes=["plain"] * 5, spacers=False,
                shapes=(None, 5))


def continuation_request_mode():
    """plain mode in the first call, request mode from the second on, over the same scratch: the names inserted by the
    first call carry no name class yet"""
    r = lambda s: string(s, False)  # noqa: E731
    first = GET + HTTPS + literal(4, r(b"/x")) + literal(38, r(b"h.example")) + literal(28, r(b"42"))
    later = GET + HTTPS + indexed(64) + indexed(63) + indexed(62) + literal(63, r(b"other.example"), "never")
    bad_cl = GET + HTTPS + indexed(64) + literal(62, r(b"4x2"), "never")
    names = literal(string(b":path", True), r(b"/lit")) + literal(r(b"host"), string(b"lit.example", True)) + \
        literal(r(b"content-length"), r(b"7"))
    cs = [ccase("names inserted in plain mode, referenced by requests", [[first], [later], [later, bad_cl], [later]]),
          ccase("literal names inserted in plain mode", [[GET + HTTPS + names],
                                                         [GET + HTTPS + indexed(64) + indexed(63) + indexed(62)],
                                                         [GET + HTTPS + literal(64, r(b"/p"), "never")
                                                          + literal(62, r(b"x"), "never")],
                                                         [GET + HTTPS + indexed(64) + indexed(64)]])]
    return dict(name="continuation_request_mode", table_size=4096, cases=cs, modes=["plain", "req", "req", "req"],
                shapes=(None, 65))


def requests_and_responses():
    """blocks that decode as valid requests / responses, for the request and response modes"""
    r = lambda s: string(s, False)  # noqa: E731
    req = GET + HTTPS + literal(4, r(b"/index")) + literal(1, string(b"www.example.com", True)) + \
        literal(string(b"x-custom", True), r(b"v")) + literal(28, r(b"12"), "never")
    req2 = indexed(3) + indexed(6) + indexed(65) + indexed(64) + indexed(63) + \
        literal(r(b"expect"), r(b"100-continue"), "never")
    res = indexed(8) + literal(31, r(b"text/html")) + literal(string(b"x-served-by", True), r(b"a")) + indexed(62)
    res2 = literal(8, r(b"204"), "never") + indexed(63) + indexed(62)
    cs = [case("requests", [req, req2, req2]), case("responses", [res, res2, res2]),
          case("many fields", [GET + HTTPS + indexed(4) + indexed(19) * 120], [indexed(8) + indexed(19) * 120],
               [GET * 1001], [indexed(8) + indexed(19) * 1001], ent=16),
          case("soft errors", [GET + HTTPS + indexed(4) + literal(r(b"x-a"), r(b"\x01v")) + indexed(62), GET + HTTPS
                               + indexed(4) + literal(r(b"x b"), r(b"v"), "never")],
               [indexed(8) + literal(r(b"x-a"), r(b"v\t")) + indexed(62), indexed(8) + literal(r(b""), r(b"v"))]),
          case("upper-case name", [GET + HTTPS + indexed(4) + literal(r(b"Upper"), r(b"v")), GET],
               [indexed(8) + literal(r(b"Upper"), r(b"v")), indexed(8)])]
    return cs


# the corpora's names, and those that also run in request and response mode -- lists, so that a test module can be
# collected without building a corpus (the builders ask the oracle whether a Huffman string decodes)
NAMES = ["integers"] + ["table_%d" % ts for ts in TABLE_SIZES] + [
    "arena", "slots", "long", "stage", "prepass", "continuation_4", "continuation_5", "continuation_empty_call",
    "continuation_request_mode", "big"]
ALL_MODES = ("integers", "table_4096", "table_100", "arena")


def all_corpora():
    out = [integers()] + [table(ts) for ts in TABLE_SIZES] + [arena(), slots(), long_literals(), stage(), prepass(),
                                                              continuation(4), continuation(5), continuation_empty_call(),
                                                              continuation_request_mode(), big()]
    extra = requests_and_responses()
    for c in out:
        if c["name"] in ALL_MODES:
            c["cases"] = c["cases"] + extra
            c["all_modes"] = True
    return out


@functools.lru_cache(maxsize=None)
def corpora():
    out = {c["name"]: c for c in all_corpora()}
    assert list(out) == NAMES
    return out


SMALL_SHAPES = (1, 63, 64, 65, 255, 256, 257)


def roomy(corpus):
    """the corpus with every arena slice at its default size.  h2o has no arena: the compiled reference copies what h2o
    decoded into the slice and knows nothing of HHUFF_BLK_ARENA's rules (a Huffman literal needs floor(8 len / 5)
    bytes, verdict order), so it is compared where no slice is tight; the tight cases' expected statuses follow from
    include/hhuff.h and are asserted case by case (test_blocks_harness.py)."""
    return dict(corpus, cases=[dict(k, arena={}) for k in corpus["cases"]])


MODES = ("plain", "req", "res")
LARGEST = ("4095", "4096", "4097", "65535", "65536", "65537")  # literal lengths the reference fixture leaves out


def corpus_modes(c):
    return MODES if c.get("all_modes") else (None,)


def in_fixture(corpus, k):
    """the fixture (tests/golden/block_edges.npz) leaves out the largest-literal cases of the long-literal corpora,
    whose decoded text would make it several MB"""
    return not (corpus["name"] in ("long", "q_literals") and any(n in k["name"].split(",")[0].split() for n in LARGEST))


def reference_pairs(c):
    """-> [(label, batch, modes)]: the batches whose reference results the fixture holds -- the cases once, in order
    (`alone` corpora: every case), arena slices roomy"""
    c = roomy(c)
    small = dict(c, cases=[k for k in c["cases"] if in_fixture(c, k)])
    out = []
    for mode in corpus_modes(c):
        for label, bt, modes in batches(small, mode)[:None if c.get("alone") else 1]:
            out.append(("%s %s" % (label, mode or "plain"), bt, modes))
    return out


def fixture_key(name, label, key):
    return "%s|%s|%s" % (name, label, key)


def reference_results(codec):
    """the HPACK arrays of tests/golden/block_edges.npz (oracle/gen_golden.py): `codec` is the compiled reference"""
    import blocks_harness as BH

    out = {}
    for name, c in corpora().items():
        if name == "big":
            continue
        for label, bt, modes in reference_pairs(c):
            for k, v in BH.summary(BH.expected(codec, bt, modes), bt, modes).items():
                out[fixture_key(name, label, k)] = v
    return out


def batches(corpus, mode=None):
    """-> [(label, batch, modes)]: the corpus's batches.  `alone`: one batch per case, no spacers; else one batch per
    shape (None = the cases once, in order; a number = that many connections, cases repeated in varying orders)."""
    from blocks_harness import batch

    modes = corpus["modes"] if mode is None else [mode] * len(corpus["modes"])
    ts, out = corpus["table_size"], []
    if corpus.get("alone"):
        for k in corpus["cases"]:
            out.append((k["name"], batch([k], ts, spacers=False), modes))
        return out
    for n in corpus.get("shapes", (None,) + SMALL_SHAPES):
        bt = batch(corpus["cases"], ts, nconn=n, seed=n or 0, spacers=corpus.get("spacers", True),
                   arena_base=0 if n in (None, 64) else 16 * ((n or 0) % 7) + 3, tail=0 if n in (None, 256) else (n % 5))
        out.append(("%s nconn=%s" % (corpus["name"], n or "all"), bt, modes))
    return out
