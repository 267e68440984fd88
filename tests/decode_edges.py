"""Huffman strings built for the places where each device decoder of h2o_hpack_decode_huffman has logic of its own:
the stream kernel's window, bulk limit, rounds and output flush; the split decoders' segment boundaries, leads
and merges; the per-string service's rounds.  Plain helpers, no GPU; tests/test_decode_edges_host.py checks the
corpora themselves (reference against oracle, coverage, sensitivity), tests/test_decode_edges.py runs them.

Every generator returns Case objects: a label, the Huffman bytes, the name flag the case is about, and `facts`
-- the geometry the label claims, as numbers ("end": 576, "sym_at": 545 ...).  A test judges coverage from the
facts, recomputed from huff_ref's symbol offsets, never from the label's text.

The constants below restate the kernels' geometry; test_decode_edges_host.py::test_constants_match_the_sources
reads the same values out of hhuff_kernels.hip / hhuff_launch.h, so a retuned kernel fails there first and its
edges move with it."""
import numpy as np

import bounds_harness as H
import huff_ref as R
from test_decode_tail import _codes, special_strings, tail_cases  # the staged decoders' tail corpus

# ---- stream kernel: decode_stream_kernel<8, 20, 144, 16> (hhuff_kernels.hip:1214-1513, HHUFF_DECT_* :2945-2950)
STREAM_NW = 20                          # :2946 window dwords a lane
STREAM_LIMW = 32 * (STREAM_NW - 2) - 30  # :1240 kLimW = 546: bulk steps start while pm < kLimW (pm: the bit before the code)
STREAM_FINAL = 32 * (STREAM_NW - 2)      # :1241 kFinal = 576: a string whose end bit is <= this ends in the window
STREAM_NEXT = 4 * (STREAM_NW - 3)        # :1321 the window that is prefetched starts 68 bytes on
STREAM_SEG = 16                         # :2950 flush granularity
STREAM_OUT = 144                        # :2947 a lane's output buffer
STREAM_TAIL = 26                        # :1337 lim = min(end - 26, kLimW)
STREAM_CLAIM_BYTES = 23040              # :3095 stream_claim: 64..256 strings a claim
LUT_BITS = 13                           # hhuff_tables.h:8 codes up to 13 bits (and pairs up to 13) are one LUT step
# ---- split decoders: seg_walk / split_decode_wave / split_decode_block (:820-1126), launch_decode (:3397-3411)
SPLIT_MIN, SPLIT_MIN_FEW = 4096, 512    # :803-804 Huffman bytes from which a string is listed (few: n <= 16)
SPLIT_BIG, SPLIT_BIG_FEW = 65536, 4096  # :3397 from which a block takes it
SPLIT_FEW_N = 16                        # :3404
SPLIT_MEAN = 128                        # :3405 the list exists in batches of this mean, or of <= 16 strings
SPLIT_LEAD = 256                        # :805
SPLIT_BLOCK_WAVES = 16                  # :3395 split_decode_kernel<16, true>
ONE_STRING_WAVES = 4                    # :3902 one_string_kernel's split_decode_block<4>
# ---- per-string service (hhuff_launch.h:18,27; wave_decode :3651-3656)
SVC_ROUND = 64                          # candidate bits a round and column (kWin = 64 NC)
SVC_MAX = 768                           # kSvcMax: the longest mailbox string
ONE_MAX = 32768                         # kOneMax: the longest one_string_kernel string


def split_seg(nbytes, waves=1, block=False):
    """(seg, lead) in bits of split_decode_wave (:989-993) / split_decode_block<waves> (:1061-1062)"""
    tb, n = 8 * nbytes, 64 * waves
    seg = (tb + n * 32 - 1) // (n * 32) * 32
    if block:
        seg = max(seg, 128)
    return seg, 64 if seg <= 64 else 128 if seg <= 256 else SPLIT_LEAD


def stream_claim(in_size, n):
    """:3097-3101.  With n strings and in_size = mean * n: mean <= 90 -> 256, 91..120 -> 192, 121..180 -> 128,
    181 and up -> 64 strings a claim"""
    c = STREAM_CLAIM_BYTES // max(in_size // n, 1)
    return 256 if c >= 256 else 192 if c >= 192 else 128 if c >= 128 else 64


class Case:
    __slots__ = ("label", "data", "is_name", "facts")

    def __init__(self, label, bits, is_name=False, **facts):
        self.label, self.is_name, self.facts = label, is_name, facts
        self.data = to_bytes(bits) if isinstance(bits, str) else bytes(bits)

    def __repr__(self):
        return "<%s: %d B %r>" % (self.label, len(self.data), self.facts)


# ------------------------------------------------------------------------------------------------
# building blocks
# ------------------------------------------------------------------------------------------------
CODES = _codes()
NBITS = [len(c) for c in CODES]
EOS_BITS = "1" * 30
# symbols that are valid in names and in values and are no SP / HT / ':' -- text that sets no soft bit
CLEAN = {5: b"012aceiost", 6: b"%-.3456789", 7: b"jkqvwxyz", 8: b"&*"}
LONG = {14: 94, 19: 195, 23: 135, 28: 220, 30: 10}  # a symbol of each long length (30 bits: only control bytes)
SP, HT = 0x20, 0x09
VALUE_BAD_LUT, VALUE_BAD_LONG = 0x00, 0x01  # value-invalid bytes: a 13-bit code (LUT step), a 23-bit one (long path)
NAME_BAD_LUT, NAME_BAD_LONG = ord("A"), 0x80  # name-invalid, value-valid: 6 bits, 20 bits


def _combos():
    best = {0: ()}
    for n in range(1, 48):
        for L in (5, 6, 7, 8):
            if n - L in best and n not in best:
                best[n] = best[n - L] + (L,)
    return best


_COMBO = _combos()  # bits -> code lengths 5..8 that add up to them (1..4 and 9 have none)
_CLEAN_SYMS = np.frombuffer(b"".join(CLEAN[L] for L in (5, 6, 7, 8)), np.uint8)
_CLEAN_LEN = np.array(NBITS, np.int64)


class Unfillable(ValueError):
    pass


def to_bytes(bits):
    assert len(bits) % 8 == 0, len(bits)
    return int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""


def close(bits):
    """pad with ones to whole bytes (0..7 bits)"""
    return bits + "1" * ((-len(bits)) % 8)


def fill(rng, nbits):
    """exactly nbits of clean text"""
    if nbits not in _COMBO and nbits < 48:
        raise Unfillable(nbits)
    head = ""
    if nbits >= 48:  # random clean symbols up to 40..47 bits before the end, the rest by the table
        syms = _CLEAN_SYMS[rng.integers(0, _CLEAN_SYMS.size, nbits // 5 + 1)]
        cum = np.cumsum(_CLEAN_LEN[syms])
        m = int(np.searchsorted(cum, nbits - 40, side="right"))
        head = "".join(map(CODES.__getitem__, syms[:m].tolist()))
        nbits -= int(cum[m - 1]) if m else 0
    return head + "".join(CODES[CLEAN[L][int(rng.integers(len(CLEAN[L])))]] for L in _COMBO[nbits])


def fill5(n):
    """n 5-bit symbols"""
    return "".join(CODES[CLEAN[5][k % 10]] for k in range(n))


def compose(rng, items, total=None):
    """items: [(bit, bits)] in order -> one bit string with every item at its bit, clean text between them and
    up to `total` bits (None: the last item ends the string)"""
    out = ""
    for at, bits in items:
        out += fill(rng, at - len(out)) + bits
    if total is not None:
        out += fill(rng, total - len(out))
    return out


def fillable(n):
    return n >= 48 or n in _COMBO


# ------------------------------------------------------------------------------------------------
# models of the kernels' step structure (geometry only: which symbols a round or a lane takes)
# ------------------------------------------------------------------------------------------------
def lut_step(lens, i):
    """symbols the LUT step at symbol i takes: 0 (a long code: the long path's), 1 or 2 (a pair within 13 bits)"""
    if i >= len(lens) or lens[i] > LUT_BITS:
        return 0
    return 2 if i + 1 < len(lens) and lens[i] + lens[i + 1] <= LUT_BITS else 1


def stream_rounds(w, align):
    """The rounds of decode_stream_kernel on a whole, valid string (walk w) that starts at a byte s with s % 4 ==
    align: -> [(first symbol, symbols made, window bit of the round's first code, end bit in the window)].
    A round's window starts at the dword of the string's current byte; bulk steps (two LUT steps, or one long
    code on every second step) run while pm < min(end - 26, kLimW); a round whose end bit is <= kFinal finishes."""
    assert not w.eos and w.stop + 7 >= w.nbits
    lens = [b - a for a, b in zip(w.starts, w.starts[1:] + [w.stop])]
    idx = {s: k for k, s in enumerate(w.starts)}
    idx[w.stop] = len(lens)
    rounds, P = [], 0
    while True:
        w0 = 8 * (((align + (P >> 3)) & ~3) - align)  # the window's first bit, in string bits
        end = w.nbits - w0
        i0 = i = idx[P]
        if end <= STREAM_FINAL:
            rounds.append((i0, len(lens) - i0, P - w0, end))
            return rounds
        lim = min(end - STREAM_TAIL, STREAM_LIMW)
        longchk = False
        while P - w0 - 1 < lim:
            if i < len(lens) and lens[i] > LUT_BITS:
                if longchk:
                    P += lens[i]
                    i += 1
            else:
                for _ in range(2):
                    k = lut_step(lens, i)
                    P += sum(lens[i:i + k])
                    i += k
            longchk = not longchk
        rounds.append((i0, i - i0, w.starts[i0] - w0 if i0 < len(lens) else P - w0, end))


def split_lanes(w, seg):
    """symbols per lane of a split decoder: lane k counts the symbols that start in [k seg, (k + 1) seg)"""
    n = (w.nbits + seg - 1) // seg
    cnt = [0] * n
    for s in w.starts:
        cnt[s // seg] += 1
    return cnt


def svc_rounds(w, win):
    """rounds of the service's wave decoders on a valid string: a round follows the LUT-step chain from W until a
    step starts at or past W + win -> [(W, symbols)]"""
    lens = [b - a for a, b in zip(w.starts, w.starts[1:] + [w.stop])]
    rounds, i, W = [], 0, 0
    while True:
        i0 = i
        while i < len(lens) and w.starts[i] < W + win:
            i += max(lut_step(lens, i), 1)
        rounds.append((W, i - i0))
        if i >= len(lens):
            if w.stop >= W + win:  # the chain left the window at the end of the data: a round of padding only
                rounds.append((w.stop, 0))
            return rounds
        W = w.starts[i]


# ------------------------------------------------------------------------------------------------
# (a) the stream corpus
# ------------------------------------------------------------------------------------------------
# A string's end bit in a window is 8 (s % 4 + len) - 544 k: a multiple of 8.  Of the edges 545, 546, 547,
# 575, 576, 577, 578 only 576 can be a string's end; the others are reached by the end of the last whole code,
# with 7..1 bits of padding behind it up to the next byte.  STREAM_ENDS are the ends of whole strings around
# both thresholds (min(end - 26, 546) changes at 572, fin at 576), STREAM_CODE_ENDS the last code's.
STREAM_ENDS = (544, 552, 568, 576, 584)
STREAM_CODE_ENDS = (545, 546, 547, 575, 576, 577, 578)
STREAM_TAILS = ("long30 last", "5 long14 5", "eos", "pad7 zero@6", "cut 13 of 14")


def stream_window_edge(seed=11):
    """every alignment x window 0..2 x (string end at STREAM_ENDS x tail) + (last code's end at STREAM_CODE_ENDS);
    facts: align, window, end (the string's end bit in that window), code_end"""
    rng = np.random.default_rng(seed)
    tails = dict(tail_cases(CODES))
    out = []
    for align in range(4):
        for k in range(3):
            base = 8 * STREAM_NEXT * k - 8 * align  # string bit of window bit 0 (window k at +68 k bytes)
            for end in STREAM_ENDS:
                for t in STREAM_TAILS:
                    bits = fill(rng, base + end - len(tails[t])) + tails[t]
                    out.append(Case("edge a%d w%d end%d %s" % (align, k, end, t), bits, align=align, window=k, end=end,
                                    tail=t))
            for ce in STREAM_CODE_ENDS:
                bits = close(fill(rng, base + ce))
                out.append(Case("edge a%d w%d text pad%d code_end%d" % (align, k, len(bits) - base - ce, ce), bits,
                                align=align, window=k, end=len(bits) - base, code_end=ce, tail="text pad"))
    return out


def stream_long_codes(seed=12):
    """a 14..30-bit code whose first bit is window bit 540..548 (pm 539..547 around kLimW), or that ends at kFinal
    exactly; once with text behind it, once with the string ending inside it (the lane parks); windows 0 and 1.
    facts: align, window, sym_at (window bit of the code's first bit), sym_len, cut (True: the string ends in it)"""
    rng = np.random.default_rng(seed)
    out = []
    for align in range(4):
        for k in (0, 1):
            base = 8 * STREAM_NEXT * k - 8 * align
            for L, sym in LONG.items():
                for at in sorted(set(range(540, 549)) | {STREAM_FINAL - L}):
                    head = fill(rng, base + at)
                    follow = close(head + CODES[sym] + fill(rng, 120))
                    out.append(Case("long%d a%d w%d at%d text" % (L, align, k, at), follow, align=align, window=k,
                                    sym_at=at, sym_len=L, cut=False))
                    cut_end = (len(head) + 8 + 7) // 8 * 8  # >= 8 bits of the code: no padding
                    if cut_end < len(head) + L:
                        out.append(Case("long%d a%d w%d at%d cut" % (L, align, k, at),
                                        (head + CODES[sym])[:cut_end], align=align, window=k, sym_at=at, sym_len=L,
                                        cut=True))
                    if at == STREAM_FINAL - L:  # the string's last code ends at kFinal
                        out.append(Case("long%d a%d w%d ends at final" % (L, align, k), head + CODES[sym],
                                        align=align, window=k, sym_at=at, sym_len=L, cut=False, end=STREAM_FINAL))
    return out


def stream_eos(seed=13):
    """30 one-bits from window bit 516 (ends at kLimW), 545 and 546, text behind; facts: align, window, eos_at"""
    rng = np.random.default_rng(seed)
    out = []
    for align in range(4):
        for k in (0, 1):
            base = 8 * STREAM_NEXT * k - 8 * align
            for at in (516, 545, 546):
                bits = close(fill(rng, base + at) + EOS_BITS + fill(rng, 90))
                out.append(Case("eos a%d w%d at%d" % (align, k, at), bits, align=align, window=k, eos_at=at))
    return out


def _search(rng, make, want, align, lo, hi, tries=1):
    """the first string make(nbits) for nbits in [lo, hi) whose rounds (stream_rounds at `align`) satisfy want();
    make() draws random text, so a range may be tried again"""
    for _ in range(tries):
        for nbits in range(lo, hi):
            try:
                bits = make(nbits)
            except Unfillable:
                continue
            w = R.walk(bits)
            rounds = stream_rounds(w, align)
            if want(w, rounds):
                return bits, rounds
    raise AssertionError("no string in [%d, %d) bits" % (lo, hi))


def stream_soft(seed=14, lengths=(2, 3)):
    """values and names of two and of three rounds whose one soft-bit cause sits at a chosen round.
    facts: align, rounds, what ("sp first", "sp last", "bad"), round (the round that makes the byte), made (bytes the
    last round makes), first_round_made.

    A first round that makes no byte does not exist: the string's first code starts at window bit 8 (s % 4) <= 24
    and has at most 30 bits, so it ends by bit 54; the bulk loop runs to min(end - 26, 546) and the tail takes the
    rest, so the first code is always decoded in round 1 unless the string ends inside it -- then the string
    fails and no byte counts.  Every string built here is checked for it (first_round_made > 0)."""
    rng = np.random.default_rng(seed)
    out = []
    sp = CODES[SP]
    for align in range(4):
        for nr in lengths:
            lo, hi = 8 * (STREAM_NEXT * (nr - 1) + 8), 8 * (STREAM_NEXT * nr - 4)

            def add(label, is_name, bits, rounds, **facts):
                assert len(rounds) == nr and rounds[0][1] > 0
                out.append(Case("soft a%d r%d %s" % (align, nr, label), bits, is_name, align=align, rounds=nr,
                                made=rounds[-1][1], first_round_made=rounds[0][1], **facts))

            is_nr = lambda w, r: len(r) == nr  # noqa: E731
            # the only SP / HT is the first byte
            for ws, nm in ((SP, "sp"), (HT, "ht")):
                bits, r = _search(rng, lambda n: close(CODES[ws] + fill(rng, n)), is_nr, align, lo, hi)
                add(nm + " first", False, bits, r, what="sp first", round=1)
            # ... is the last byte: the last round makes several bytes, or exactly one (the SP).  (A last round that
            # makes none does not exist: a round that goes on has end >= 584, its bulk steps start below bit 546
            # and take at most 30 bits, so at least 8 bits -- more than padding -- are left for the next round.)
            # Exactly one: the round before must stop within 13 bits of the end, so its last bulk step starts at
            # pm = 545 and takes 26..30 bits -- here a 28-bit code at window bit 546, then the SP and 4 bits of padding.
            bits, r = _search(rng, lambda n: close(fill(rng, n) + sp), lambda w, r: len(r) == nr and r[-1][1] >= 2,
                              align, lo, hi)
            add("sp last made2", False, bits, r, what="sp last", round=nr)
            at = 8 * STREAM_NEXT * (nr - 2) - 8 * align + STREAM_LIMW
            bits, r = _search(rng, lambda n: close(fill(rng, n) + CODES[LONG[28]] + sp),
                              lambda w, r: len(r) == nr and r[-1][1] == 1, align, at - 16, at + 1, tries=400)
            add("sp last made1", False, bits, r, what="sp last", round=nr)
            # the only invalid byte is made in round 1, 2 .. the last
            for is_name, syms in ((False, (VALUE_BAD_LUT, VALUE_BAD_LONG)), (True, (NAME_BAD_LUT, NAME_BAD_LONG))):
                for sym in syms:
                    for rd in range(1, nr + 1):
                        at = 8 * STREAM_NEXT * (rd - 1) + (200 if rd < nr else 40)

                        def want(w, r, rd=rd, sym=sym):
                            k = w.syms.index(bytes([sym]))
                            return len(r) == nr and r[rd - 1][0] <= k < r[rd - 1][0] + r[rd - 1][1]
                        bits, r = _search(rng, lambda n: close(compose(rng, [(at, CODES[sym])], n)), want, align,
                                          max(lo, at + 60), hi + 600)
                        add("%s bad %#x round%d" % ("name" if is_name else "value", sym, rd), is_name, bits, r,
                            what="bad", round=rd)
            # a ':'-prefixed name with a name-invalid byte in round 2: no soft bit
            colon = CODES[ord(":")]
            bits, r = _search(rng, lambda n: close(colon + compose(rng, [(8 * STREAM_NEXT + 100, CODES[NAME_BAD_LUT])],
                                                                  n)), is_nr, align, lo, hi)
            add("colon name bad round2", True, bits, r, what="colon", round=2)
    return out


# (107..113: around what one round makes of 5-bit text -- 112 bytes at s % 4 == 0, 108 at the other alignments)
FLUSH_LENS = (0, 1, 15, 16, 17, 31, 32, 33, 107, 108, 109, 111, 112, 113)
FLUSH_DST = (0, 1, 5, 15)
# contiguous layout: dst = floor(8 s / 5) takes the residues {0, 1, 3, 4, 6, 8, 9, 11, 12, 14} mod 16 only (s mod 10
# = 0..9), never 5 or 15: 4, 6 and 14 stand in for them.  s mod 10 for dst mod 16 = 0, 1, 4, 6, 14:
FLUSH_S_MOD10 = {0: 0, 1: 1, 4: 3, 6: 4, 14: 9}


def stream_flush():
    """5-bit text of every FLUSH_LENS output length (x 4 copies, one for each destination alignment), strings whose
    first round leaves 0, 1 and 15 bytes to carry, and the two sides of the implicit slots' whole last chunk.
    facts: out_len; dst16 (explicit layout: the destination's residue to give it); s_mod (contiguous layout:
    (m, r), the input offset to give it, s % m == r); carry; whole"""
    out = []
    for n in FLUSH_LENS:
        for j, d in enumerate(FLUSH_DST):
            s10 = FLUSH_S_MOD10[(0, 1, 4 if n % 2 else 6, 14)[j]]
            out.append(Case("flush len%d dst%d" % (n, d), close(fill5(n)), out_len=n, dst16=d, s_mod=(10, s10)))
    # the carry: round 1 of 5-bit text at s % 4 == 0 makes `made` bytes; (dst + made) % 16 bytes stay in the buffer
    bits = close(fill5(200))
    made = stream_rounds(R.walk(bits), 0)[0][1]
    for carry in (0, 1, 15):
        out.append(Case("flush carry%d" % carry, bits, out_len=200, dst16=(carry - made) % 16, carry=carry,
                        s_mod=(4, 0), made1=made))
    # `whole` (:1491): under implicit slots the last 16-B chunk is stored whole iff its end, ceil16(dst + out_len),
    # is <= the slot's end floor(8 (s + len) / 5); s % 80 fixes both residues.  Equality, and the nearest miss: a
    # slot's end is never 15 mod 16 (floor(8 m / 5) mod 16 is one of 0, 1, 3, 4, 6, 8, 9, 11, 12, 14), so no chunk
    # misses its slot by one byte; by two it does.
    for want, label in ((0, "fits"), (2, "short by 2")):
        for s in range(80):
            hit = None
            for n in range(1, 60):  # n 6-bit symbols: 6 n bits, out_len n
                ln = (6 * n + 7) // 8
                dst, slot_end = (8 * s) // 5, (8 * (s + ln)) // 5
                if (dst + n) % 16 and (dst + n + 15) // 16 * 16 - slot_end == want and (dst + n) // 16 > dst // 16:
                    hit = n
                    break
            if hit:
                bits = close("".join(CODES[CLEAN[6][k % 10]] for k in range(hit)))
                out.append(Case("flush whole %s" % label, bits, out_len=hit, whole=want == 0, s_mod=(80, s),
                                dst16=((8 * s) // 5) % 16))
                break
        else:
            raise AssertionError(label)
    return out


def clean_string(rng, nbytes):
    """a valid string of exactly nbytes (fillers between arranged cases)"""
    return to_bytes(finish(rng, "", 8 * nbytes))


def finish(rng, bits, total):
    """`bits`, clean text and 0..7 bits of padding: `total` bits in all"""
    rem = total - len(bits)
    pad = next(p for p in (3, 2, 1, 0, 4, 5, 6, 7) if rem - p >= 0 and fillable(rem - p))
    return bits + fill(rng, rem - pad) + "1" * pad


def arrange(cases, seed=0, in_off0=0):
    """Put the cases in one contiguous batch so that each starts at the input offset its facts ask for ("s_mod":
    (m, r), or "align": s % 4), with clean filler strings (Case "filler") of 1..m-1 bytes in between.
    -> [Case] in batch order.  (Holds for the first string at in_off0; the other in_off0 of a test shift every
    string alike.)"""
    rng = np.random.default_rng(seed)
    out, pos = [], in_off0
    for c in cases:
        m, r = c.facts.get("s_mod") or ((4, c.facts["align"]) if "align" in c.facts else (1, 0))
        gap = (r - pos) % m
        if gap:
            out.append(Case("filler", clean_string(rng, gap), filler=True))
            pos += gap
        out.append(c)
        pos += len(c.data)
    return out


def dilute(cases, mean, seed=0):
    """the cases with short clean strings (0..20 B, Case "filler") spread among them until the batch's mean length
    is at most `mean` bytes: a batch of long strings can then take the routes of a shorter mean"""
    rng = np.random.default_rng(seed)
    total, n = sum(len(c.data) for c in cases), len(cases)
    extra = []
    while total > mean * (n + len(extra)):
        extra.append(Case("filler", clean_string(rng, int(rng.integers(0, 21))), filler=True))
        total += len(extra[-1].data)
    out, k = [], 0
    for j, c in enumerate(cases):
        out.append(c)
        while k < len(extra) and k * len(cases) < (j + 1) * len(extra):
            out.append(extra[k])
            k += 1
    return out + extra[k:]


def offsets(batch, in_off0=0):
    """the input offset of every string of a contiguous batch"""
    return in_off0 + np.concatenate([[0], np.cumsum([len(c.data) for c in batch])[:-1]]).astype(np.int64)


def stream_corpus():
    """-> {class: [Case]}"""
    return {"window_edge": stream_window_edge(), "long_codes": stream_long_codes(), "eos": stream_eos(),
            "soft": stream_soft(), "flush": stream_flush()}


# ------------------------------------------------------------------------------------------------
# (b) the split corpus
# ------------------------------------------------------------------------------------------------
# Huffman bytes by form (launch_decode's lists): n <= 16: 512 B and up one wave, 4096 B and up a block; n = 17 at
# a mean >= 128: 4096 B and up one wave
SPLIT_WAVE_FEW = (512, 513, 1024, 1025, 2048, 2049, 4095)  # seg 64, 96, 128, 160, 256, 288, 512: every lead
SPLIT_BLOCK_FEW = (4096, 4097, 8200)                       # 16 waves, seg 128, inactive lanes
SPLIT_WAVE_MANY = (4096, 5000)                             # seg 512, 640
SPLIT_ONE_STRING = (769, 1024, 4096, 32768)  # one_string_kernel (HHUFF_NO_SERVICE=1): 4 waves, 256 segments
# a code that sets no soft bit in a value, by how many bits it must at least have (to straddle a boundary)
_STRADDLE = ((5, ord("a")), (6, ord("-")), (7, ord("j")), (8, ord("&")), (14, 94), (19, 195), (23, 135), (28, 220))


def split_boundaries(nbytes, waves=1, block=False):
    """(seg, the lanes k whose segment start k seg is tested): 1, 2, 63, the last active lane; in a block also 64
    and 128, the first lanes of the next waves"""
    seg, _ = split_seg(nbytes, waves, block)
    last = (8 * nbytes - 1) // seg
    ks = [1, 2, 63, last] + ([64, 128] if block else [])
    return seg, sorted({k for k in ks if 1 <= k <= last})


def split_cases(nbytes, waves=1, block=False, seed=21):
    """Every boundary case for one string length and decoder shape.  A code placement is made at several
    boundaries of one string (the lanes are independent; two strings hold them all, so that neighbouring
    boundaries have room); an EOS or an only-invalid byte gets a string per boundary.
    facts: nbytes, seg, lead, kind, rel (the item's offset from the boundary), at ([the item's string bit]),
    bounds ([k])"""
    rng = np.random.default_rng(seed + nbytes)
    seg, lead = split_seg(nbytes, waves, block)
    _, ks = split_boundaries(nbytes, waves, block)
    tb = 8 * nbytes
    out = []

    def add(kind, rel, item, is_name=False, single=False):
        groups = [[k] for k in ks] if single else [ks[0::2], ks[1::2]]
        for grp in groups:
            # (an item needs 17 bits behind it: text of >= 10 bits and the padding)
            items = [(k * seg + rel, item) for k in grp if k * seg + rel + len(item) + 17 <= tb]
            if not items:
                continue
            bits = finish(rng, compose(rng, items), tb)
            out.append(Case("split %dB seg%d %s rel%+d k=%s" % (nbytes, seg, kind, rel, [(a - rel) // seg for a, _ in items]),
                            bits, is_name, nbytes=nbytes, seg=seg, lead=lead, kind=kind, rel=rel,
                            at=[a for a, _ in items], bounds=[(a - rel) // seg for a, _ in items]))

    for L in (5, 8, 14, 30):
        for rel in (-1, 0, 1):
            add("code%d" % L, rel, CODES[LONG[L] if L > LUT_BITS else CLEAN[L][0]])
    add("code30", -29, CODES[LONG[30]])
    for rel in (-5, -3):
        add("pair5+5", rel, CODES[ord("a")] + CODES[ord("e")])
    for rel in (-30, -1, 0):
        add("eos", rel, EOS_BITS, single=True)
    for rel in (-1, 0):
        add("only bad", rel, CODES[VALUE_BAD_LUT], single=True)
        add("only bad name", rel, CODES[NAME_BAD_LUT], is_name=True, single=True)

    def whole(label, bits, is_name=False, **facts):
        assert len(bits) == tb, (label, len(bits), tb)
        out.append(Case("split %dB seg%d %s" % (nbytes, seg, label), bits, is_name, nbytes=nbytes, seg=seg, lead=lead,
                        **facts))

    # the only SP / HT is the first symbol; the last symbol
    sp = CODES[SP]
    whole("sp first", sp + fill(rng, tb - 9) + "111", kind="sp first")
    whole("sp last", fill(rng, tb - 9) + sp + "111", kind="sp last")
    # The last lane's segment has `tailbits` bits, a multiple of 8 (seg is one of 32).  It holds only the SP and
    # the padding, or only 1..7 bits of padding, when a code that starts before the lane covers the rest of it:
    # possible for tailbits - 6 - pad <= 27, or tailbits - pad <= 27 (a 28-bit code; the 30-bit ones are control
    # bytes, which would set the soft bit themselves).
    ks_last = (tb - 1) // seg * seg
    tailbits = tb - ks_last

    def straddle(x):  # a code of more than x bits that starts x bits before the end of what it covers
        return next((CODES[s] for L, s in _STRADDLE if L > x), None)

    for pad in (0, 1, 7):
        x = tailbits - 6 - pad
        if 1 <= x <= 27 and fillable(ks_last + x - len(straddle(x))):
            whole("sp alone in the last lane pad%d" % pad, fill(rng, ks_last + x - len(straddle(x))) + straddle(x) + sp +
                  "1" * pad, kind="sp alone", pad=pad, tailbits=tailbits)
    for pad in range(1, 8):
        x = tailbits - pad
        if 1 <= x <= 27 and fillable(ks_last + x - len(straddle(x))):
            whole("last lane pad%d only" % pad, fill(rng, ks_last + x - len(straddle(x))) + straddle(x) + "1" * pad,
                  kind="pad only", pad=pad, tailbits=tailbits)
    # the string's end cuts a code: 14 bits of a 30-bit code are left, and 9 of a 10-bit one
    for L, sym, keep in ((30, LONG[30], 14), (10, ord("!"), 9)):
        whole("end cuts code%d" % L, fill(rng, tb - keep) + CODES[sym][:keep], kind="cut", cut_at=tb - keep)
    # strings that resynchronise late or never: the lanes' first walks disagree and the re-walk loop runs
    for label, unit in (("0e", CODES[ord("0")] + CODES[ord("e")]), ("a", CODES[ord("a")]),
                        ("30-bit", CODES[10] + CODES[13] + CODES[22]), ("5-bit", fill5(10))):
        bits = (unit * (tb // len(unit) + 1))[:tb]
        whole("periodic " + label, finish(rng, bits[:R.walk(bits).stop], tb), kind="periodic", unit=label)
    # one flipped bit in the first, a middle and the last segment
    good = finish(rng, fill(rng, tb - 16), tb)
    for where, bit in (("first", seg // 2), ("middle", ks_last // seg // 2 * seg + seg // 3), ("last", ks_last + 1)):
        whole("flip %s" % where, good[:bit] + ("1" if good[bit] == "0" else "0") + good[bit + 1:], kind="flip",
              where=where, bit=bit)
    return out


def split_corpus():
    """-> {(form, Huffman bytes): [Case]}; form "wave_few" / "block_few" (batches of <= 16 strings), "wave_many" (17
    strings at a mean >= 128)"""
    out = {}
    for L in SPLIT_WAVE_FEW:
        out["wave_few", L] = split_cases(L)
    for L in SPLIT_BLOCK_FEW:
        out["block_few", L] = split_cases(L, SPLIT_BLOCK_WAVES, True)
    for L in SPLIT_WAVE_MANY:
        out["wave_many", L] = split_cases(L, seed=22)
    return out


_ONE_STRING_KINDS = ("code30", "pair5+5", "eos", "only bad", "sp first", "sp last", "sp alone", "pad only", "cut",
                     "periodic", "flip")


def one_string_cases():
    """the block form in one_string_kernel (4 waves, 256 segments of >= 128 bits): -> {Huffman bytes: [Case]}, the
    kinds of _ONE_STRING_KINDS (a child process decodes one string a call)"""
    return {L: [c for c in split_cases(L, ONE_STRING_WAVES, True, seed=23) if c.facts["kind"] in _ONE_STRING_KINDS]
            for L in SPLIT_ONE_STRING}


# ------------------------------------------------------------------------------------------------
# (c) the per-string corpus
# ------------------------------------------------------------------------------------------------
SVC_WINS = (SVC_ROUND, 2 * SVC_ROUND, 4 * SVC_ROUND)  # a round's bits: one column (the default and HHUFF_SVC_NC=1), two, four


def _svc_try(rng, make, ok):
    for _ in range(200):
        bits = make()
        if ok(svc_rounds(R.walk(bits), ok.win)):
            return bits
    raise AssertionError("no such string")


def per_string_cases(oracle, seed=31):
    """facts: kind; total / pad (bits of codes, of padding); win (the round length the case is about), at (round bit),
    round; nbytes"""
    rng = np.random.default_rng(seed)
    out = [Case("tail %d" % k, s, bool(k & 1), kind="tail") for k, s in enumerate(special_strings(oracle, CODES, 31))]
    for total in (64, 128, 192, 384):
        out.append(Case("svc total%d pad0" % total, fill(rng, total), kind="exact", total=total, pad=0))
        for pad in range(1, 8):
            out.append(Case("svc total%d pad%d" % (total - pad, pad), fill(rng, total - pad) + "1" * pad, kind="padded",
                            total=total - pad, pad=pad))
    long30 = CODES[LONG[30]]
    for win in SVC_WINS:
        # A 30-bit code at round bit 34 (ends with the first 64 candidates), 35, 63 (the last candidate), 64 (the
        # next column's first, or the next round's), and the same against the round's end.  Round 1 starts at bit
        # 0; round 2 where the chain left the window, here at bit win + 3 (checked with svc_rounds()).
        for at in sorted({34, 35, 63, 64, win - 30, win - 29, win - 1, win}):
            out.append(Case("svc win%d long30 at%d" % (win, at), close(fill(rng, at) + long30 + fill(rng, 40)),
                            kind="long30", win=win, at=at, round=1))

            def ok(rounds, win=win):
                return len(rounds) > 1 and rounds[1][0] == win + 3
            ok.win = win
            bits = _svc_try(rng, lambda: close(fill(rng, win - 3) + CODES[ord("-")] + fill(rng, at) + long30 +
                                               fill(rng, 40)), ok)
            out.append(Case("svc win%d long30 at%d round2" % (win, at), bits, kind="long30", win=win, at=at, round=2,
                            start2=win + 3))
        for k in (1, 2):  # an EOS whose last bit is string bit k win - 1: the last candidate bit of round 1's window, or
            # of a second window that starts at bit win
            out.append(Case("svc win%d eos ends at %d" % (win, k * win), close(fill(rng, k * win - 30) + EOS_BITS),
                            kind="eos", win=win, eos_end=k * win))
            out.append(Case("svc win%d eos ends at %d text" % (win, k * win),
                            close(fill(rng, k * win - 30) + EOS_BITS + fill(rng, 30)), kind="eos", win=win,
                            eos_end=k * win))
        for pad in (1, 7):  # the last round holds only padding: the last step ends at or past the window's end

            def ok(rounds, win=win):
                return rounds[-1][1] == 0 and len(rounds) >= 2
            ok.win = win
            n = next(n for n in range(win, win + 8) if (n + pad) % 8 == 0)
            out.append(Case("svc win%d last round pad%d" % (win, pad), _svc_try(rng, lambda: fill(rng, n) + "1" * pad, ok),
                            kind="pad round", win=win, pad=pad))
    for L in (SVC_MAX - 1, SVC_MAX, SVC_MAX + 1):
        out.append(Case("svc %d B" % L, H.huffman_of_len(oracle, rng, L), kind="limit", nbytes=L))
        out.append(Case("svc %d B name" % L, H.huffman_of_len(oracle, rng, L), True, kind="limit", nbytes=L))
    # the stream corpus' soft-bit cases, shortened to 20..100 B
    sp = CODES[SP]
    for nb in (20, 47, 100):
        n = 8 * nb - 9
        out.append(Case("svc soft sp first %dB" % nb, sp + fill(rng, n) + "111", kind="soft", what="sp first"))
        out.append(Case("svc soft ht first %dB" % nb, finish(rng, CODES[HT], 8 * nb), kind="soft", what="sp first"))
        out.append(Case("svc soft sp last %dB" % nb, fill(rng, n) + sp + "111", kind="soft", what="sp last"))
        for is_name, syms in ((False, (VALUE_BAD_LUT, VALUE_BAD_LONG)), (True, (NAME_BAD_LUT, NAME_BAD_LONG))):
            for sym in syms:
                for at in (0, 4 * nb + 12, 8 * nb - 8 - NBITS[sym]):
                    out.append(Case("svc soft %s bad %#x at%d %dB" % ("name" if is_name else "value", sym, at, nb),
                                    finish(rng, compose(rng, [(at, CODES[sym])]), 8 * nb), is_name, kind="soft",
                                    what="bad"))
        out.append(Case("svc soft colon name %dB" % nb,
                        finish(rng, CODES[ord(":")] + compose(rng, [(60, CODES[NAME_BAD_LUT])]), 8 * nb), True,
                        kind="soft", what="colon"))
    return out


# ------------------------------------------------------------------------------------------------
# the reference's results, kept: a corpus is walked once however many tests use it
# ------------------------------------------------------------------------------------------------
_WALKS = {}
_CORPORA = {}


def walk_of(data):
    w = _WALKS.get(data)
    if w is None:
        w = _WALKS[data] = R.walk(data)
    return w


def ref(data, is_name):
    """huff_ref.decode(data, is_name) from the kept walk"""
    return R.verdict(data, walk_of(data), is_name)


def corpus(name, oracle=None):
    """"stream" / "split" / "one_string" / "per_string" (needs the oracle: the tail corpus' strings), built once"""
    if name not in _CORPORA:
        _CORPORA[name] = {"stream": stream_corpus, "split": split_corpus, "one_string": one_string_cases,
                          "per_string": lambda: per_string_cases(oracle)}[name]()
    return _CORPORA[name]


