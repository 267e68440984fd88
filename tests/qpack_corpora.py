"""The hand-built QPACK sessions of the header-block edge tests (blocks_harness' builders).  A corpus is dict(name,
table_size, max_blocked, cases, ...); a case's connections are lists over the steps of (encoder-stream buffer,
[sections]).  The buffer of a step holds what the decoder left unconsumed in the step before, then the new bytes.
The cases stay inside hhuff_qpack_decode's contract: a step's sections are decoded against the table as the step's
whole encoder stream leaves it, so an evicting instruction comes in a later step than the sections that use the
entry."""
import functools

import numpy as np

from blocks_corpora import _arena_block, stage_tiles, tile_plan
from blocks_harness import (huff_of_len, huff_variants, integer, q_duplicate, q_indexed, q_indexed_post, q_insert,
                            q_insert_ref, q_literal, q_literal_post, q_literal_ref, q_prefix, q_set_capacity, qbatch,
                            qcase, qstr)

HTS = 4096
ME = HTS // 32  # h2o's max_entries
V = lambda s, h=False: qstr(s, 7, 0, h)  # noqa: E731: a value string
NONE = (b"", [])


def mini(k):
    """a minimum-size entry: a one-byte name, an empty value"""
    return q_insert(bytes([97 + k % 26]), V(b""))


def sec(ric, base, *lines, me=ME):
    return q_prefix(ric, base, me) + b"".join(lines)


def steps_and_poisoning():
    a, b, c = q_insert(b"x-a", V(b"one")), q_insert(b"x-b", V(b"two")), q_insert_ref(0, V(b"three"))
    cs = [qcase("sections only, encoder stream only",
                [(a + b, []), (b"", [sec(2, 2, q_indexed(0), q_indexed(1)), sec(1, 1, q_indexed(0))]), (c, []),
                 (b"", [sec(3, 3, q_indexed(0), q_indexed(2)), sec(3, 1, q_indexed_post(1), q_indexed_post(0))]),
                 (mini(0), [sec(4, 4, q_indexed(0), q_indexed(3)), sec(0, 0, q_indexed(17, True))])]),
          qcase("every entry read back after inserts in every step",
                [(b"".join(q_insert(b"name-%d-%02d" % (i, k), V(b"value %d/%d" % (i, k) + bytes([65 + k]) * (k % 7)))
                           for k in range(9 + i)), [sec(n, n, *[q_indexed(j) for j in range(n)])])
                 for i, n in ((i, sum(9 + j for j in range(i + 1))) for i in range(5))]),
          qcase("nothing at all in a step", [(a, [sec(1, 1, q_indexed(0))]), NONE, NONE, (b, []),
                                             (b"", [sec(2, 2, q_indexed(0), q_indexed(1))])])]
    # an instruction cut at each of its bytes: nothing of it is consumed, the whole instruction comes again
    hv = huff_of_len(np.random.default_rng(21), 11)
    for tag, ins in (("literal-name insert", q_insert(b"cut-name", V(b"cut-value"))),
                     ("Huffman literal-name insert", q_insert(huff_of_len(np.random.default_rng(22), 6), V(hv, True), True)),
                     ("static-name insert", q_insert_ref(70, V(hv, True), True)),
                     ("set capacity", q_set_capacity(4000)), ("duplicate", q_duplicate(0))):
        conns = []
        for k in range(0, len(ins)):
            use = sec(2, 2, q_indexed(0)) if tag != "set capacity" else sec(1, 1, q_indexed(0))
            conns.append([(a + ins[:k], [sec(1, 1, q_indexed(0))]), (ins, [use]), (ins[:k], []), (ins[:k] + ins[k:], []),
                          (b"", [use])])
        cs.append(qcase("%s cut" % tag, *conns))
    return dict(name="q_steps", table_size=HTS, max_blocked=2, cases=cs)


def table(hts=HTS):
    me = max(1, hts // 32)
    live = hts // 33
    n32 = hts // 32  # entries of an empty name and value that fit
    S = lambda *a: sec(*a, me=me)  # noqa: E731
    big = q_insert(b"n", V(b"v" * (hts - 33)))  # an entry of exactly the capacity
    cs = [
        qcase("capacity to 0 and back", [(mini(0) + q_set_capacity(0) + q_set_capacity(hts) + mini(1), []),
                                         (b"", [S(2, 2, q_indexed(0)), S(2, 2, q_indexed(1))])]),
        qcase("capacity exactly the maximum", [(q_set_capacity(hts) + mini(0), [S(1, 1, q_indexed(0))])]),
        qcase("capacity one past the maximum", [(mini(0), [S(1, 1, q_indexed(0))]), (q_set_capacity(hts + 1) + mini(1), [
            S(1, 1, q_indexed(0))]), (mini(2), [S(1, 1, q_indexed(0))])]),
        qcase("entry of exactly the capacity", [(mini(0) + big, [S(2, 2, q_indexed(0))]),
                                                (b"", [S(2, 2, q_indexed(0)), S(2, 2, q_indexed(1))]),
                                                (mini(1), [S(3, 3, q_indexed(0)), S(3, 3, q_indexed(1))])],
              ent=0, room=3 * hts),
        qcase("entry one past the capacity", [(mini(0) + q_insert(b"n", V(b"v" * (hts - 32))), [S(1, 1, q_indexed(0))]),
                                              (mini(1), [S(1, 1, q_indexed(0))])]),
        qcase("three table lengths of minimum entries",
              [(b"".join(mini(k) for k in range(live)), [S(live, live, q_indexed(0), q_indexed(live - 1))]),
               (b"".join(mini(k) for k in range(live)), [S(2 * live, 2 * live, q_indexed(0), q_indexed(live - 1)),
                                                          S(2 * live, 2 * live, q_indexed(live))]),
               (b"".join(mini(k) for k in range(live)), [S(3 * live, 3 * live, q_indexed(0), q_indexed(live - 1)),
                                                          S(3 * live, 2 * live, q_indexed_post(live - 1), q_indexed_post(live))])]),
        qcase("three table lengths of 32-byte entries (an empty name, an empty value)",
              [(mini(0) + q_insert(b"", V(b"")) * n32, [S(n32 + 1, n32 + 1, q_indexed(0), q_indexed(n32 - 1)),
                                                        S(n32 + 1, n32 + 1, q_indexed(n32))]),
               (q_insert(b"", V(b"")) * n32, [S(2 * n32 + 1, 2 * n32 + 1, q_indexed(0), q_indexed(n32 - 1))]),
               (q_insert(b"", V(b"")) * n32 + mini(1), [S(3 * n32 + 2, 3 * n32 + 2, q_indexed(0), q_indexed(n32 - 1)),
                                                        S(3 * n32 + 2, 3 * n32 + 2, q_indexed(n32))])]),
        qcase("duplicate of the oldest entry, which the duplication evicts",
              [(b"".join(mini(k) for k in range(live)) + q_set_capacity(33 * live), []),
               (q_duplicate(live - 1), [S(live + 1, live + 1, q_indexed(0), q_indexed(live - 1))]),
               (b"", [S(live + 1, live + 1, q_indexed(live))])]),
        qcase("an insert fills the table exactly",
              [(mini(0) + q_insert(b"n", V(b"v" * (hts - 66))), [S(2, 2, q_indexed(0), q_indexed(1))]),
               (b"", [S(2, 2, q_indexed(1), q_indexed(0))]), (mini(1), [S(3, 3, q_indexed(0), q_indexed(1))]),
               (b"", [S(3, 3, q_indexed(2))])], ent=0, room=3 * hts),
        qcase("insert evicts its own name reference",
              [(q_insert(b"n" * 10, V(b"")), [S(1, 1, q_indexed(0))]),
               (q_insert_ref(0, V(b"v" * (hts - 42))), [S(2, 2, q_indexed(0))]), (b"", [S(2, 2, q_indexed(1))])],
              ent=0, room=3 * hts),
    ]
    return dict(name="q_table_%d" % hts, table_size=hts, max_blocked=2, cases=cs,
                shapes=(None, 1, 63, 64, 65, 255, 256, 257) if hts == HTS else (None, 5))


def index_edges():
    three = mini(0) + mini(1) + mini(2)
    wrap = b"".join(mini(k) for k in range(2 * ME - 2))
    cs = [
        qcase("relative index 0 and base-1", [(three, [sec(3, 3, q_indexed(0), q_indexed(2)), sec(3, 3, q_indexed(3))])]),
        qcase("relative name index 0, base-1, base", [(three, [sec(3, 3, q_literal_ref(0, V(b"v")), q_literal_ref(2, V(b"w"), never=True)),
                                                             sec(3, 3, q_literal_ref(3, V(b"v")))])]),
        qcase("post-base index 0, the last, one past it",
              [(three, [sec(3, 0, q_indexed_post(0), q_indexed_post(2)), sec(3, 0, q_indexed_post(3)),
                        sec(3, 1, q_literal_post(0, V(b"v")), q_literal_post(1, V(b"w"), True)), sec(3, 1, q_literal_post(2, V(b"v")))])]),
        qcase("static index 98 and 99", [(b"", [sec(0, 0, q_indexed(98, True), q_indexed(0, True)), sec(0, 0, q_indexed(99, True)),
                                                sec(0, 0, q_literal_ref(98, V(b"v"), True)), sec(0, 0, q_literal_ref(99, V(b"v"), True))]),
                                         (q_insert_ref(98, V(b"v"), True), [sec(1, 1, q_indexed(0))]),
                                         (q_insert_ref(99, V(b"v"), True), [sec(1, 1, q_indexed(0))]), (b"", [sec(1, 1, q_indexed(0))])]),
        qcase("Required Insert Count at the wrap of 2 max_entries",
              [(three, [sec(3, 3, q_indexed(0))]),
               (wrap, [sec(2 * ME - 1, 2 * ME - 1, q_indexed(0)), sec(2 * ME, 2 * ME, q_indexed(0)),
                       sec(2 * ME + 1, 2 * ME + 1, q_indexed(0))]),
               (three, [sec(2 * ME + 1, 2 * ME + 1, q_indexed(0)), sec(2 * ME + 4, 2 * ME + 4, q_indexed(0)),
                        b"\x00\x00" + q_indexed(0), integer(2 * ME + 1, 8) + b"\x00" + q_indexed(0),
                        integer(2 * ME, 8) + b"\x00" + q_indexed(0)])], blocked=0),
        qcase("a section cut in its prefix", [(three, [sec(3, 3, q_indexed(0))[:k] for k in range(0, 3)]
                                               + [integer(300, 8)[:1] + b"", integer(3 + 1, 8) + integer(200, 7)[:1]])]),
    ]
    for nb, tag in ((1, "max_blocked-1"), (2, "max_blocked"), (0, "none blocked")):
        cs.append(qcase("blocked with num_blocked at %s" % tag,
                        [(mini(0), [sec(2, 2, q_indexed(0)), sec(1, 1, q_indexed(0)), sec(3, 3, q_indexed(0)),
                                    sec(4, 4, q_indexed(0))]),
                         (mini(1), [sec(2, 2, q_indexed(0)), sec(3, 3, q_indexed(0))])], blocked=nb))
    return dict(name="q_index", table_size=HTS, max_blocked=2, cases=cs)


def literals():
    rng = np.random.default_rng(23)
    low = lambda L: bytes(rng.integers(97, 123, L, dtype=np.uint8))  # noqa: E731
    cs = []

    def both(tag, payload, h):
        """as a section's literal name (3-bit prefix) and value (7-bit), and -- where it fits the table -- as an
        inserted literal name (5-bit) and value, referenced in the next step"""
        sl = (8 * (len(payload) + 16)) // 5 + 64
        steps = [(b"", [sec(0, 0, q_literal(payload, V(b"v"), h)), sec(0, 0, q_literal_ref(0, qstr(payload, 7, 0, h), True)),
                        sec(0, 0, q_indexed(17, True), q_literal(payload, qstr(payload, 7, 0, h), h, True))])]
        ar = {(0, 0, 0): sl, (0, 0, 1): sl, (0, 0, 2): 2 * sl, (0, 2, 0): 2 * sl, (0, 2, 1): sl}
        if len(payload) <= 1600:
            steps += [(q_insert(payload, V(b"v"), h) + q_insert_ref(0, qstr(payload, 7, 0, h), True), []),
                      (b"", [sec(2, 2, q_indexed(0), q_indexed(1)), sec(2, 0, q_literal_post(0, V(b"w")))])]
        cs.append(qcase(tag, steps, arena=ar))

    for L in (0, 1, 511, 512, 513, 1536, 4095, 4096, 4097, 65535, 65536, 65537):
        for tag, p in huff_variants(rng, L):
            both("Huffman %d %s" % (L, tag), p, True)
        both("raw %d" % L, low(L), False)
        if L > 512:
            for at in sorted(set(o for o in (0, 15, 16, 1023, 1024, L - 1) if o < L)):
                p = bytearray(low(L))
                p[at] = 0x01
                both("raw %d, invalid character at %d" % (L, at), bytes(p), False)
    L = 1536
    for tag, edits in {"soft before upper-case": {100: b" ", 900: b"Q"}, "upper-case before soft": {100: b"Q", 900: b" "},
                       "upper-case only": {1535: b"Z"}, "leading ':'": {0: b":", 5: b"Q"},
                       "a pseudo-header token, then upper-case": {0: b":path"}}.items():
        p = bytearray(low(L))
        for at, c in edits.items():
            p[at:at + len(c)] = c
        both("long raw name, %s" % tag, bytes(p), False)
    for tag, at, c in (("a space first", 0, b" "), ("a tab first", 0, b"\t"), ("a space last", L - 1, b" "),
                       ("a tab last", L - 1, b"\t"), ("a space inside", 700, b" ")):
        p = bytearray(low(L))
        p[at:at + 1] = c
        cs.append(qcase("long raw value, %s" % tag, [(q_insert(b"n", qstr(bytes(p), 7)), [sec(0, 0, q_literal(b"n", qstr(bytes(p), 7)))]),
                                                       (b"", [sec(1, 1, q_indexed(0))])], ent=0, room=8 * L))
    # the pre-pass verdict is a failure: the section / the encoder stream must fail as the reference does
    bad = huff_variants(rng, 20)[2][1]
    for tag, name, h in (("bad Huffman name", bad, True), ("upper-case raw name", b"X-Upper", False),
                         ("pseudo-header token name", b":path", False), ("raw name with a leading ':'", b":Bogus", False)):
        cs.append(qcase(tag, [(mini(0), [sec(0, 0, q_indexed(17, True), q_literal(name, V(b"v"), h), q_indexed(17, True))]),
                              (q_insert(name, V(b"v"), h) + mini(1), [sec(1, 1, q_indexed(0))]),
                              (mini(2), [sec(1, 1, q_indexed(0))])]))
    cs.append(qcase("bad Huffman value", [(mini(0), [sec(0, 0, q_literal(b"n", V(bad, True))), sec(1, 1, q_literal_ref(0, V(bad, True)))]),
                                          (q_insert_ref(0, V(bad, True)), [sec(1, 1, q_indexed(0))])]))
    return dict(name="q_literals", table_size=HTS, max_blocked=2, cases=cs, shapes=(None,))


def arena():
    rng = np.random.default_rng(24)
    h = huff_of_len(rng, 20)
    from oracle import oracle as O

    hd = len(O.oracle().decode(h)[0])
    bad = huff_variants(rng, 20)[2][1]
    setup = q_insert(b"dname-xyz", V(b"dvalue-12345"))
    filler = (q_indexed(17, True), [(7, 7), (3, 3)])  # :method GET
    kinds = {
        "static name": ((q_literal_ref(0, V(b"x"), True), [(10, 10), (1, 1)]), 0),
        "static value": ((q_indexed(17, True), [(7, 7), (3, 3)]), 1),
        "dynamic name": ((q_literal_ref(0, V(b"x")), [(9, 9), (1, 1)]), 0),
        "dynamic value": ((q_indexed(0), [(9, 9), (12, 12)]), 1),
        "post-base value": ((q_indexed_post(0), [(9, 9), (12, 12)]), 1),
        "raw literal": ((q_literal(b"rawname", V(b"rawvalue!")), [(7, 7), (9, 9)]), 1),
        "raw name": ((q_literal(b"rawname", V(b"rawvalue!")), [(7, 7), (9, 9)]), 0),
        "Huffman literal": ((q_literal_ref(0, V(h, True), True), [(10, 10), (32, hd)]), 1),
        "Huffman name": ((q_literal(h, V(b"v"), True), [(32, hd), (1, 1)]), 0),
    }
    cs = []
    for kind, (item, j) in kinds.items():
        for where, items, i in (("first", [item, filler, filler], 0), ("middle", [filler, item, filler], 1),
                                ("last", [filler, filler, item], 2)):
            for short in (0, 1):
                blk, sl = _arena_block(items, (i, j), short)
                pre = q_prefix(1, 0 if kind == "post-base value" else 1, ME)
                cs.append(qcase("%s %s, %s" % (kind, where, "one byte short" if short else "exact fit"),
                                [(setup, [pre + blk, sec(0, 0, q_indexed(17, True))])], arena={(0, 0, 0): sl}))
    item = kinds["Huffman literal"][0][0]
    cs.append(qcase("Huffman literal fits decoded", [(b"", [sec(0, 0, q_indexed(17, True), item)])], arena={(0, 0, 0): 20 + hd}))
    cs.append(qcase("upper-case raw name, slice too small", [(b"", [sec(0, 0, q_literal(b"Upper", V(b"v")))])], arena={(0, 0, 0): 2}))
    cs.append(qcase("bad Huffman value, slice too small", [(b"", [sec(0, 0, q_literal_ref(0, V(bad, True), True))])],
                    arena={(0, 0, 0): 10 + 31}))
    cs.append(qcase("zero-byte slice", [(b"", [sec(0, 0, q_indexed(17, True)), sec(0, 0), sec(0, 0, q_literal(b"", V(b"")))])],
                    arena={(0, 0, 0): 0, (0, 0, 1): 0, (0, 0, 2): 0}))
    return dict(name="q_arena", table_size=HTS, max_blocked=2, cases=cs)


def positions():
    """literal headers at input bytes 31 and 32, and a name header at byte 32767 with its value in the next chunk of
    the literal bitmap: each case alone, its first section at input byte 0"""
    rng = np.random.default_rng(25)
    hv = qstr(huff_of_len(rng, 30), 7, 0, True)
    g = q_indexed(17, True)
    cs = [qcase("value header at byte 31", [(b"", [sec(0, 0, g * 28, q_literal_ref(0, hv, True), g)])]),
          qcase("value header at byte 32", [(b"", [sec(0, 0, g * 29, q_literal_ref(0, hv, True), g)])]),
          qcase("name header at byte 31", [(b"", [sec(0, 0, g * 29, q_literal(huff_of_len(rng, 5), hv, True), g)])]),
          qcase("name header at byte 32", [(b"", [sec(0, 0, g * 30, q_literal(b"", hv), g)])])]
    pad = next(p for p in (q_literal(b"p", qstr(b"a" * n, 7)) for n in range(32700, 32766)) if len(p) == 32765)
    cs.append(qcase("name header at byte 32767", [(b"", [sec(0, 0, pad, q_literal(huff_of_len(rng, 6), hv, True), g)])], ent=2))
    # tiles of 64 literals on either side of the staged kernel's input and output stages (blocks_corpora.stage_tiles)
    pre = sec(0, 0)
    for name, body, pays, staged in stage_tiles(rng, lambda p, h: q_literal_ref(0, qstr(p, 7, 0, h), True), len(pre), g):
        k = qcase(name, [(b"", [pre + body, sec(0, 0, g)])])
        k["plan"] = tile_plan(pre + body, pays) + (staged,)
        cs.append(k)
    # a reference past the table, then well-formed literals: marked by the pre-pass, decoded, unused
    lits = q_literal(huff_of_len(rng, 9), hv, True) + q_literal_ref(0, qstr(b"a" * 600, 7), True) + q_literal(b"raw-name", hv)
    cs.append(qcase("a reference past the table, then literals",
                    [(mini(0), [sec(1, 1, q_indexed(1), lits), sec(1, 1, q_indexed(0), lits), sec(0, 0, q_indexed(99, True), lits),
                                sec(1, 0, q_indexed_post(1), lits), sec(1, 1, q_literal_ref(1, hv), lits),
                                sec(1, 0, q_literal_post(1, hv), lits), sec(0, 0, q_literal_ref(99, hv, True), lits)])]))
    return dict(name="q_positions", table_size=HTS, max_blocked=2, cases=cs, alone=True)


def requests():
    """sections that decode as valid requests (and a few that break a rule), for hhuff_qpack_parse_requests"""
    r = [q_indexed(17, True), q_indexed(23, True), q_indexed(1, True), q_literal_ref(0, V(b"www.example.com"), True)]
    cs = [qcase("requests", [(q_insert(b"x-custom", V(b"v")) + q_insert_ref(0, V(b"h.example"), True),
                              [sec(0, 0, *r), sec(2, 2, *r[:3], q_indexed(0), q_indexed(1)), sec(3, 3, *r)]),
                             (mini(0), [sec(3, 3, *r, q_indexed(0)), sec(0, 0, *r, q_literal(b"x b", V(b"\x01"))),
                                        sec(0, 0, *r, q_literal(b"x-ok", V(b"v\t"))),
                                        sec(0, 0, *r, q_literal(b"Upper", V(b"v"))), sec(0, 0, r[0] * 2)])])]
    return cs


NAMES = ["q_steps", "q_table_4096", "q_table_65536", "q_index", "q_literals", "q_arena", "q_positions"]
ALL_MODES = ("q_steps", "q_index")  # also through hhuff_qpack_parse_requests


def all_corpora():
    out = [steps_and_poisoning(), table(HTS), table(65536), index_edges(), literals(), arena(), positions()]
    for c in out:
        if c["name"] in ALL_MODES:
            c["cases"] = c["cases"] + requests()
            c["all_modes"] = True
    return out


@functools.lru_cache(maxsize=None)
def corpora():
    out = {c["name"]: c for c in all_corpora()}
    assert list(out) == NAMES
    return out


def batches(corpus):
    """-> [(label, session)]: as blocks_corpora.batches()"""
    hts, mb = corpus["table_size"], corpus["max_blocked"]
    if corpus.get("alone"):
        return [(k["name"], qbatch([k], hts, mb, spacers=False)) for k in corpus["cases"]]
    return [("%s nconn=%s" % (corpus["name"], n or "all"),
             qbatch(corpus["cases"], hts, mb, nconn=n, seed=n or 0, arena_base=0 if n in (None, 64) else 16 * ((n or 0) % 7) + 5))
            for n in corpus.get("shapes", (None, 1, 63, 64, 65, 255, 256, 257))]


def roomy(corpus):
    """as blocks_corpora.roomy()"""
    return dict(corpus, cases=[dict(k, arena={}) for k in corpus["cases"]])


def qmodes(c):
    return ("plain", "qreq") if c.get("all_modes") else ("plain",)


def reference_pairs(c):
    """as blocks_corpora.reference_pairs(): -> [(label, session, mode)]"""
    from blocks_corpora import in_fixture

    c = roomy(c)
    small = dict(c, cases=[k for k in c["cases"] if in_fixture(c, k)])
    return [("%s %s" % (label, mode), bt, mode) for mode in qmodes(c)
            for label, bt in batches(small)[:None if c.get("alone") else 1]]


def reference_results(codec):
    """the QPACK arrays of tests/golden/block_edges.npz (oracle/gen_golden.py)"""
    import blocks_harness as BH
    from blocks_corpora import fixture_key

    out = {}
    for name, c in corpora().items():
        for label, bt, mode in reference_pairs(c):
            for k, v in BH.qsummary(BH.qexpected(codec, bt, mode), bt, mode).items():
                out[fixture_key(name, label, k)] = v
    return out
