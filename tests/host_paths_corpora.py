"""Hand-built batches for the host-array batch paths (hhuff_{de,en}code_batch_host, _host_pipelined, _host_packed
and the host mode of _batch_multi), each with the predicate that names its edge, evaluated over
tests/host_paths_model.py (tests/test_host_paths_host.py holds every predicate; tests/test_host_paths.py runs the
cases on the GPU).

All cases are tiny: at most 300 strings of 0..100 B unless the edge is a length, chunk_bytes from 1 to a few KB.
Moving a cut to another multiple of 32 strings changes no result (the kernels see absolute offsets, and a chunk is
a sub-range of the batch): the cut model serves the coverage predicates only, and what a wrong address does is
told by the emulators' defects.

Not reachable here:
  - the clamp of the cut target to 2^32 - 1 needs a batch of 4 GiB;
  - kSplitBig (65,536 Huffman bytes) in a chunk: tests/test_batch_bounds.py has it on the device path, and a
    chunk is that path on a sub-range;
  - a failing hipMemcpy / launch in the middle of a call (what leaves staging slots busy): no test provokes one."""
import numpy as np

import bounds_harness as H
import host_paths_model as M

HUGE = 1 << 40
FULL5 = H.huffman(b"01aceist")  # 8 five-bit symbols: 5 Huffman bytes that decode to the whole 8-byte slot
assert len(FULL5) == 5
UPPER = H.huffman(b"Host-Name")  # as a name: soft error 1 (upper case); as a value: none
EOS = b"\xff\xff\xff\xff"


class Case:
    """one batch: strings (Huffman strings for decode, plain for encode), name flags, placement, chunk_bytes and
    holds(case, plan, exp) -> bool, the predicate of the edge `why` names (exp: the oracle's whole-batch result)"""

    def __init__(self, label, op, strings, why, holds, flags=None, in_off0=0, tail=0, chunk_bytes=1, defer=None,
                 group="", boundary=None):
        self.label, self.op, self.strings, self.why, self.holds = "%s %s" % (op, label), op, list(strings), why, holds
        self.n = len(self.strings)
        rng = np.random.default_rng(self.n)
        self.flags = (rng.random(self.n) < 0.5) if flags is None else np.asarray(flags, bool)
        self.in_off0, self.tail, self.chunk_bytes, self.defer = in_off0, tail, chunk_bytes, defer
        self.group, self.boundary = group, boundary

    def arrays(self, fill, sentinel, exact=True, with_status=True, with_off=True):
        """place_input()'s dict for one run, with the names, the sentinel and out_size: the slots' exact end, or
        (exact=False) include/hhuff.h's slot_of(in_size)"""
        end = self.in_off0 + sum(map(len, self.strings))
        a = H.place_input(self.strings, "contiguous", self.in_off0, fill, in_size=end + self.tail, op=self.op)
        a["names"] = H.name_bits(self.flags, fill) if self.op == "decode" else None
        a["sentinel"], a["with_status"], a["with_off"] = sentinel, with_status, with_off
        a["out_size"] = M.slot_of(self.op, end if exact else a["in_size"])
        return a

    def off(self):
        L = np.array([len(s) for s in self.strings], np.int64)
        return self.in_off0 + np.concatenate([[0], np.cumsum(L)])

    def plan(self, defer_min=None):
        d = self.defer if defer_min is None else defer_min
        return M.plan(self.op, self.off(), self.n, self.chunk_bytes, M.DEFER_NEVER if d is None else d)


def expected(oracle, case, arrays):
    """the oracle's whole-batch result at arrays' out_size, and the bytes of `out` a pipelined call may change:
    the slot range [slot_of(in_off[0]), slot_of(in_off[n]))"""
    _, exp = H.oracle_run(oracle, case.op, arrays, arrays["sentinel"], names=arrays["names"])
    exp["out"] = exp["out"][:arrays["out_size"]]
    if not arrays["with_status"]:
        del exp["status"]
    mask = np.zeros(arrays["out_size"], bool)
    mask[M.slot_of(case.op, case.in_off0):M.slot_of(case.op, int(case.off()[-1]))] = True
    return exp, mask, H.out_starts(case.op, arrays)


# ------------------------------------------------------------------------------------------------
# strings
# ------------------------------------------------------------------------------------------------
def huff(rng, L):
    """a Huffman string of exactly L bytes (header text)"""
    h = H.huffman(H.text_for_huffman_len(rng, int(L)))
    assert len(h) == L
    return h


def strings_of(op, rng, lens):
    return [huff(rng, L) if op == "decode" else H.text(rng, L) for L in lens]


def bad_strings(op, rng):
    """four strings that fail: decode -- bad padding, an EOS inside, over-long padding, a code cut short;
    encode -- long codes only, arbitrary bytes (twice each)"""
    if op == "decode":
        h = huff(rng, 20)
        # (zero bits where the padding should be; an EOS at a byte boundary; 8 bits and more of padding; 0xfe: seven
        # ones and a zero, the start of a 10-bit code)
        return [h + b"\x00", FULL5 + EOS + h, h + b"\xff", FULL5 * 3 + b"\xfe"]
    return [bytes(rng.choice(H.LONG_CODES, 24)), bytes(rng.integers(128, 256, 31, dtype=np.uint8)),
            bytes(rng.choice(H.LONG_CODES, 9)), bytes(rng.integers(128, 256, 40, dtype=np.uint8))]


def _failed(exp, idx):
    return all(exp["out_len"][i] == H.FAIL for i in idx)


def _kept(exp, idx):
    return all(exp["out_len"][i] != H.FAIL and exp["out_len"][i] > 0 for i in idx)


# ------------------------------------------------------------------------------------------------
# the pipelined corpus
# ------------------------------------------------------------------------------------------------
COUNT_NS = (1, 31, 32, 33, 63, 64, 65, 97, 193, 225)  # chunk_bytes 1: 1, 1, 1, 2, 2, 2, 3, 4, 7, 8 chunks


def chunk_counts(op):
    """1, 2, kDepth, kDepth + 1, 2 kDepth + 1 and 8 chunks of exactly 32 strings (chunk_bytes 1; last chunks of
    1, 31 and 32 strings), and every n with chunk_bytes huge (one chunk, and one more of the n % 32 last strings).
    The last string of every chunk decodes to its whole slot (FULL5), so the last byte of each D2H range is a kept
    byte"""
    rng = np.random.default_rng(11)
    base = strings_of(op, rng, rng.integers(0, 101, max(COUNT_NS)))
    if op == "decode":
        for i in range(31, len(base), 32):
            base[i] = FULL5
    out = []
    for n in COUNT_NS:
        s = base[:n]
        if op == "decode":
            s[-1] = FULL5
        want = (n + 31) // 32
        out.append(Case("n=%d chunk_bytes=1" % n, op, s, "%d chunks of 32 strings, the last of %d" % (want, n - 32 * (want - 1)),
                        lambda c, p, e, want=want: len(p) == want and all(x.m == 32 for x in p[:-1]) and
                        [x.slot for x in p] == [k % M.K_DEPTH for k in range(want)], group="counts"))
        # (the cut is rounded down to a multiple of 32 at the batch's end too -- the search ends one entry behind
        # in_off[n] --: a tail of n % 32 strings follows unless that is 0 or 31)
        out.append(Case("n=%d chunk_bytes huge" % n, op, s, "one chunk of floor(n / 32) 32 strings, and the tail's",
                        lambda c, p, e: [x.i1 for x in p] == ([c.n] if c.n <= 32 or c.n % 32 in (0, 31) else
                                                              [c.n // 32 * 32, c.n]),
                        chunk_bytes=HUGE, group="counts"))
    assert {(n + 31) // 32 for n in COUNT_NS} >= {1, 2, M.K_DEPTH, M.K_DEPTH + 1, 2 * M.K_DEPTH + 1}
    for n in (97, 225):
        off = np.concatenate([[0], np.cumsum([len(x) for x in base[:n]])])
        for k in (32, 64):
            for d in (-1, 0, 1):
                # minus one: the target lies inside string k - 1, the cut is k; exact and plus one: string k starts
                # at the target and k + 1 is the first past it, rounded down to k again
                out.append(Case("n=%d chunk_bytes=span%d%+d" % (n, k, d), op, base[:n],
                                "chunk_bytes = the span of %d strings %+d: the first cut at %d" % (k, d, k),
                                lambda c, p, e, k=k, d=d: p[0].i1 == k and p[0].e0 - p[0].s0 + d == c.chunk_bytes and
                                len(c.strings[k - 1]) > 0 and len(c.strings[k]) > 0,
                                chunk_bytes=int(off[k]) + d, group="counts"))
    return out


def empties(op):
    rng = np.random.default_rng(12)
    out = []
    lens = rng.integers(1, 101, 70)
    lens[29:35] = 0
    lens[63:66] = 0
    out.append(Case("empty on the cuts", op, strings_of(op, rng, lens), "strings 29..34 and 63..65 are empty",
                    lambda c, p, e: [x.i0 for x in p] == [0, 32, 64] and p[1].s0 == p[0].e0 == int(c.off()[29]),
                    group="empties"))
    for name, r in (("base below", 37), ("on its base", 0)):
        lens = rng.integers(2, 101, 96)
        lens[32:64] = 0
        lens[0] += (r - int(lens[:32].sum())) % 80  # in_off[32] % 80 == r
        out.append(Case("32 empty strings as a chunk, " + name, op, strings_of(op, rng, lens),
                        "chunk 1 holds no byte: nbytes = s0 %% 80 = %d%s"
                        % (r, ", a zero-byte H2D and sel_bytes 0" if r == 0 else ""),
                        lambda c, p, e, r=r: p[1].i0 == 32 and p[1].m == 32 and p[1].s0 == p[1].e0 and p[1].nbytes == r and
                        p[1].sel == (r or p[1].e0), group="empties"))
    for off0 in (0, 7, 80):
        out.append(Case("only empty strings in_off0=%d" % off0, op, [b""] * 70, "70 empty strings",
                        lambda c, p, e: len(p) == 2 and all(x.s0 == x.e0 for x in p), in_off0=off0, tail=16,
                        group="empties"))
    return out


OFFSETS = (1, 7, 15, 16, 79, 80, 81, 159)


def offsets(op):
    """in_off[0] at the residues of 16 and 80 around zero; poison before the first string and, 37 bytes of it,
    behind the last; n = 97 (four chunks) and n = 33 (two, and a batch the multi call leaves shards empty with)"""
    rng = np.random.default_rng(13)
    base = strings_of(op, rng, rng.integers(0, 101, 97))
    out = []
    for off0 in OFFSETS:
        for n in (97, 33):
            out.append(Case("in_off0=%d n=%d" % (off0, n), op, base[:n], "in_off[0] = %d, 37 poisoned bytes behind" % off0,
                            lambda c, p, e, off0=off0: p[0].s0 == off0 and p[0].base == off0 // 80 * 80 and c.tail == 37,
                            in_off0=off0, tail=37, group="offsets"))
    return out


def lengths(op):
    rng = np.random.default_rng(14)
    out = []
    s = strings_of(op, rng, rng.integers(0, 60, 70))
    s[0] = strings_of(op, rng, [3000])[0]
    out.append(Case("a string longer than chunk_bytes", op, s, "string 0 (3000 B) exceeds chunk_bytes 1024: the a + 32 arm",
                    lambda c, p, e: p[0].i1 == 32 and len(c.strings[0]) > c.chunk_bytes, chunk_bytes=1024, group="lengths"))
    for L in (M.SPLIT_MIN - 1, M.SPLIT_MIN, M.SPLIT_MIN + 1):
        lens = rng.integers(0, 30, 128)
        lens[40] = L
        s = strings_of(op, rng, lens)
        # chunk_bytes 1: string 40 in a chunk of 32 strings, whose mean its own length lifts to 128 and more
        out.append(Case("a %d-B string, chunk mean >= 128" % L, op, s, "string 40 in a 32-string chunk of mean >= 128",
                        lambda c, p, e: p[1].i0 == 32 and p[1].m == 32 and p[1].mean >= M.SPLIT_MEAN and
                        (c.op == "encode" or p[1].split), in_off0=3, group="lengths"))
        # chunk_bytes = the span of 96 strings: strings 0..95 as one chunk of mean < 128
        out.append(Case("a %d-B string, chunk mean < 128" % L, op, s, "string 40 in a 96-string chunk of mean < 128",
                        lambda c, p, e: p[0].i1 == 96 and p[0].mean < M.SPLIT_MEAN and not p[0].split, in_off0=3,
                        chunk_bytes=sum(len(x) for x in s[:96]), group="lengths"))
    few = [M.SPLIT_MIN_FEW - 1, M.SPLIT_MIN_FEW, M.SPLIT_MIN_FEW + 1, M.SPLIT_BIG_FEW - 1, M.SPLIT_BIG_FEW,
           M.SPLIT_BIG_FEW + 1]
    lens = list(rng.integers(0, 40, 32)) + [9] + few[:3] + [0, 21] + few[3:]
    out.append(Case("split thresholds in a tail chunk of 9", op, strings_of(op, rng, lens),
                    "511/512/513 and 4095/4096/4097 B in a last chunk of 9 strings: the few-strings thresholds",
                    lambda c, p, e: len(p) == 2 and p[1].m == 9 and p[1].smin == M.SPLIT_MIN_FEW and
                    p[1].big_min == M.SPLIT_BIG_FEW and (c.op == "encode" or p[1].split), in_off0=5, group="lengths"))
    lens = [13, 0] + few[:3] + list(rng.integers(0, 40, 8)) + few[3:]
    out.append(Case("a batch of 16", op, strings_of(op, rng, lens), "one chunk of 16 strings with the same lengths",
                    lambda c, p, e: len(p) == 1 and p[0].m == 16 and p[0].smin == M.SPLIT_MIN_FEW and
                    (c.op == "encode" or p[0].split), in_off0=1, group="lengths"))
    return out


# lengths a family's chunk draws from: its mean (over the chunk's bytes from its base, up to 79 more) stays inside
BANDS = {"decode": {"short": (8, 30), "mixed": (70, 90), "stream": (180, 220)},
         "encode": {"sorted_small": (20, 40), "sorted": (50, 50), "lanes": (70, 100), "lanes_long": (180, 220)}}


def _family_strings(op, rng, fams, per=32):
    s = []
    for f in fams:
        lo, hi = BANDS[op][f]
        s += strings_of(op, rng, rng.integers(lo, hi + 1, per))
    return s


def families(op):
    """one call whose consecutive 32-string chunks pick every kernel family, so that three different ones are in
    flight on the three streams, in two orders; then with edges deferred from 64 strings a chunk"""
    rng = np.random.default_rng(15)
    names = list(BANDS[op])
    out = []
    for order in (names + names[:2], names[::-1] + names[::-1][:2]):
        out.append(Case("families " + ">".join(order), op, _family_strings(op, rng, order),
                        "32-string chunks of the families " + ", ".join(order),
                        lambda c, p, e, order=order: [x.family for x in p] == order and not any(x.deferred for x in p) and
                        all(len({x.family for x in p[k:k + 3]}) == 3 for k in range(len(p) - 2)), group="families"))
    # deferred edges: blocks of 64 strings of a family, chunk_bytes between the span of 64 strings of one family and
    # of the next, so that some chunks have 64 strings and more (deferred) and the rest 32 (not)
    first, second, longest = names[0], names[-2], names[-1]
    for cb, fams in ((64 * BANDS[op][first][1] + 80, (first, second, longest, first)),
                     (64 * BANDS[op][second][1] + 80, (second, longest, first, second))):
        s = _family_strings(op, rng, fams, 64)
        out.append(Case("families deferred chunk_bytes=%d %s" % (cb, ">".join(fams)), op, s,
                        "edge_defer_min 64: chunks of 64 strings and more defer their edges, 32-string chunks do not",
                        lambda c, p, e, longest=longest: {x.deferred for x in p} == {True, False} and
                        any(x.m == 32 and not x.deferred for x in p) and
                        any(x.m >= 64 and x.deferred and x.family != longest for x in p) and
                        len({x.family for x in p}) >= 3, chunk_bytes=cb, defer=64, group="families"))
    return out


def seams(op):
    """failing strings as the last string of a chunk and the first of the next; name flags that differ at strings
    31 / 32 / 33 and in the last partial word"""
    rng = np.random.default_rng(16)
    lens = rng.integers(1, 101, 100)
    lens[[30, 33, 62, 65]] = 40
    s = strings_of(op, rng, lens)
    bad = bad_strings(op, rng)
    at = (31, 32, 63, 64)
    for i, b in zip(at, bad):
        s[i] = b
    out = [Case("failing strings at the seams", op, s, "strings 31, 32, 63 and 64 fail, their neighbours do not",
                lambda c, p, e: [x.i0 for x in p] == [0, 32, 64, 96] and _failed(e, at) and _kept(e, (30, 33, 62, 65)),
                in_off0=9, group="seams")]
    if op == "decode":
        s = strings_of(op, rng, lens)
        flags = rng.random(100) < 0.5
        for i, f in ((30, 0), (31, 1), (32, 0), (33, 1), (63, 1), (64, 0), (96, 1), (97, 0), (98, 1), (99, 0)):
            s[i], flags[i] = UPPER, bool(f)
        # "Host-Name" is a soft error as a name only: status says which bit the kernel read
        out.append(Case("name flags at the word seams", op, s, "is_name differs at 31/32/33, 63/64 and in the 4-bit last word",
                        lambda c, p, e: all(e["status"][i] == int(c.flags[i]) for i in (30, 31, 32, 33, 63, 64, 96, 97, 98, 99))
                        and c.n % 32 == 4, flags=flags, in_off0=2, group="seams"))
    return out


def pipelined_corpus(op):
    return chunk_counts(op) + empties(op) + offsets(op) + lengths(op) + families(op) + seams(op)


# ------------------------------------------------------------------------------------------------
# the packed staging boundary
# ------------------------------------------------------------------------------------------------
def _kept_len(op, text):
    """bytes string `text` keeps in the packed output: decode (of its Huffman string) the text; encode its Huffman
    string if that is shorter, else nothing"""
    if op == "decode":
        return len(text)
    h = len(H.huffman(text))
    return h if h < len(text) else 0


def _runs(c, e):
    exp, _ = M.packed_from_slots(c.op, c.off(), c.n, e)
    return M.packed_runs(c.op, c.off(), c.n, exp["out_off"], exp["out_len"])


def packed_boundary(op, B):
    """158 short strings (tiles of 64, 64 and 30) placed so that, against the staging boundary B of host_packed, a
    tile's run straddles B, ends exactly at B, starts exactly at B, an all-failed tile's empty run sits at B, and
    every run lies behind B.  B = 4096 for the emulator; the GPU tests use the real 64 MiB"""
    assert B % 8 == 0
    rng = np.random.default_rng(17)
    texts = [H.text(rng, L) for L in rng.integers(4, 31, 158)]
    to_in = (lambda t: H.huffman(t)) if op == "decode" else (lambda t: t)
    unslot = lambda pos: -((-5 * pos) // 8) if op == "decode" else pos  # noqa: E731  the least x, slot_of(x) >= pos

    def make(name, texts, off0, why, holds, bad_tile=None):
        s = [to_in(t) for t in texts]
        if bad_tile is not None:
            bad = bad_strings(op, rng)
            for i in range(64 * bad_tile, 64 * bad_tile + 64):
                s[i] = bad[i % 4]
        return Case("packed %s B=%d" % (name, B), op, s, why, holds, in_off0=off0, group="packed_boundary", boundary=B)

    K0 = sum(_kept_len(op, t) for t in texts[:64])
    span0 = sum(len(to_in(t)) for t in texts[:64])
    out = [make("straddles", texts, unslot(B - K0 // 2), "tile 0's run straddles B",
                lambda c, p, e: _runs(c, e)[0][0] < B < _runs(c, e)[0][1])]
    t2 = list(texts)
    while M.slot_of(op, unslot(B - K0)) != B - K0:  # decode: not every position is a slot start
        t2[0] += b"e"
        K0 = sum(_kept_len(op, t) for t in t2[:64])
    out.append(make("ends at", t2, unslot(B - K0), "tile 0's run ends exactly at B",
                    lambda c, p, e: _runs(c, e)[0][1] == B and _runs(c, e)[1][0] > B))
    start = unslot(B) - span0
    out.append(make("starts at", texts, start, "tile 1's run starts exactly at B",
                    lambda c, p, e: _runs(c, e)[1][0] == B < _runs(c, e)[1][1] and _runs(c, e)[0][1] < B))
    out.append(make("empty at", texts, start, "tile 1 fails whole: its empty run sits at B, tile 2's lies behind",
                    lambda c, p, e: _runs(c, e)[1] == (B, B) and _failed(e, range(64, 128)) and
                    _runs(c, e)[2][0] > B and _runs(c, e)[2][1] > _runs(c, e)[2][0], bad_tile=1))
    out.append(make("all behind", texts, unslot(B) + 3, "every run lies behind B: the first staged chunk holds none",
                    lambda c, p, e: _runs(c, e)[0][0] >= B))
    return out


def corpus():
    """every case of both directions"""
    return [c for op in ("decode", "encode") for c in pipelined_corpus(op)]


def packed_corpus(B):
    return [c for op in ("decode", "encode") for c in packed_boundary(op, B)]
