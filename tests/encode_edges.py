"""Strings and call plans for the per-string symbols h2o_hpack_encode_huffman / h2o_hpack_decode_huffman, built for
the places where their device side has logic of its own: wave_encode's 64-byte rounds and early verdict,
block_encode<4>'s wave parts, encode_long_kernel's 16-KB rounds, the 768 / 769 and 32768 / 32769 hand-overs, and the
resident service's mailboxes (12-byte tagged chunks in, 12-byte tagged chunks out, the hot mailbox read ahead).
Plain helpers, no GPU: tests/test_encode_edges_host.py checks the corpus, the plans and the model themselves,
tests/test_per_string_service.py runs them through tests/per_string_check.c.

  corpus()        -> [Case]: label, op (1 encode, 0 decode), the call's input, `facts` -- the geometry the label claims
                     as numbers; a test judges coverage from the facts, recomputed from huff_ref, never from the text
  plan(T)         -> [[Req] per thread]: T threads x PLAN_ROUNDS calls whose answers tell the threads apart
  Mailbox model   -> model_run(): the host's post, the wave's poll with the hot mailbox's chunks read ahead, the tagged
                     result chunks, with four switchable defects; each must disagree with the plan's expectations

The constants restate hhuff_launch.h / hhuff_kernels.hip; test_encode_edges_host.py reads them out of the sources."""
import functools
import struct

import numpy as np

import huff_ref as R
from h2o_amd import tables

NB = list(tables.ENC_NBITS)
SVC_SLOTS = 64      # kSvcSlots
SVC_CHUNK = 12      # payload bytes of a 16-byte chunk
SVC_IN_CHUNKS = 64  # SvcSlot::chunk
SVC_OUT_CHUNKS = 104  # SvcSlot::outc
SVC_MAX = SVC_CHUNK * SVC_IN_CHUNKS  # kSvcMax = 768
SVC_WAVES = 16      # service_waves()'s default
SVC_IDLE_TICKS = 200000  # kSvcIdle: 2 ms of the 100 MHz counter
ONE_MAX = 32768     # kOneMax
ROUND = 64          # bytes a wave_encode round
BLOCK_WAVES = 4     # one_string_kernel: block_encode<4>
LONG_CHUNK = 16384  # encode_long_kernel: kLongChunk
SIZE_MAX = 2 ** 64 - 1

BY_LEN = {L: bytes(b for b in range(256) if NB[b] == L) for L in sorted(set(NB))}
S5, S6, S7, S8 = BY_LEN[5], BY_LEN[6], BY_LEN[7], BY_LEN[8]
TEXT = S5 + S6 + S7  # 68 symbols that always compress
LONG30 = bytes(BY_LEN[30])  # 0x0a, 0x0d, 0x16
LENGTHS = ([0, 1, 2] + [n for a in (12, 24, 64, 128, 192, 1024, 1280) for n in (a - 1, a, a + 1)] +
           [766, 767, 768, 769, 32767, 32768, 32769])
VERDICT_LENGTHS = (64, 65, 768, 769, 32769)


def service_waves(env):
    """service_waves() (hhuff_kernels.hip): HHUFF_SVC_WAVES when it is a divisor of 64 from 2 on, else 16"""
    try:
        w = int(env) if env else SVC_WAVES
    except ValueError:
        w = 0
    return w if 2 <= w <= SVC_SLOTS and SVC_SLOTS % w == 0 else SVC_WAVES


def route(op, n):
    """which device code a per-string call of n input bytes runs on the default path"""
    if n <= SVC_MAX:
        return "service"
    if n <= ONE_MAX:
        return "one_string"
    return "long"


def bits_of(data):
    return sum(NB[b] for b in data)


def round_bits(data):
    """code bits of every 64-byte round of wave_encode"""
    return [bits_of(data[i:i + ROUND]) for i in range(0, len(data), ROUND)]


def part_starts(n_or_data, waves=BLOCK_WAVES):
    """block_encode<waves>: the byte at which each wave's part starts (per = 64-byte multiples), and with data the
    bit at which its codes start"""
    data = n_or_data if isinstance(n_or_data, (bytes, bytearray)) else None
    n = len(data) if data is not None else n_or_data
    per = (n + ROUND * waves - 1) // (ROUND * waves) * ROUND
    at = [min(w * per, n) for w in range(waves)]
    return at if data is None else [(a, bits_of(data[:a])) for a in at]


def pack(text):
    """the Huffman bytes of `text` whatever their length (no len - 1 rule): a decode call's input"""
    bits = R.code_bits(text)
    bits += "1" * (-len(bits) % 8)
    return bytes(int(bits[p:p + 8], 2) for p in range(0, len(bits), 8))


def pick(rng, syms, n):
    return bytes(np.frombuffer(syms, np.uint8)[rng.integers(0, len(syms), n)]) if n else b""


class Case:
    __slots__ = ("label", "op", "data", "is_name", "facts")

    def __init__(self, label, op, data, is_name=False, **facts):
        self.label, self.op, self.data, self.is_name, self.facts = label, op, bytes(data), is_name, facts

    def __repr__(self):
        return "<%s: %s %d B %r>" % (self.label, "encode" if self.op else "decode", len(self.data), self.facts)


# ------------------------------------------------------------------------------------------------
# the corpus
# ------------------------------------------------------------------------------------------------
def length_cases(rng):
    out = [Case("len %d" % n, 1, pick(rng, TEXT, n), kind="length", len=n) for n in LENGTHS]
    for at in (LONG_CHUNK - 1, LONG_CHUNK, LONG_CHUNK + 1):  # a 30-bit code on either side of the first 16-KB round
        d = bytearray(pick(rng, S5 + S6, 40000))
        d[at] = LONG30[at % 3]
        out.append(Case("len 40000, 30-bit code at byte %d" % at, 1, d, kind="long_round", len=40000, at=at))
    return out


def exact_text(rng, nsyms, bits):
    """nsyms symbols of 5..8 bits whose codes take exactly `bits`"""
    assert 5 * nsyms <= bits <= 8 * nsyms, (nsyms, bits)
    lens = np.full(nsyms, 5)
    for _ in range(bits - 5 * nsyms):
        i = int(rng.integers(nsyms))
        while lens[i] == 8:
            i = (i + 1) % nsyms
        lens[i] += 1
    return bytes(BY_LEN[int(L)][int(rng.integers(len(BY_LEN[int(L)])))] for L in lens)


def verdict_cases(rng):
    """8 len - 8 bits (len - 1 bytes: encodes) and 8 len - 7 bits (SIZE_MAX) from 5-, 6-, 7- and 8-bit symbols: 8-bit
    ones but for a 5- and two 6-bit symbols (-7) somewhere and the symbol at `spot`, 7 bits in the string that
    encodes and 8 in the one that does not -- in the first round, in the last, in the byte after a round boundary"""
    out = []
    for n in VERDICT_LENGTHS:
        spots = [("first", 5), ("last", n - 1)]
        if n > ROUND and n - 1 != ROUND:
            spots.append(("after", ROUND))
        if (n - 1) % ROUND == 0:
            spots[1] = ("last+after", n - 1)  # the last round is the one byte after a boundary
        for name, at in spots:
            d = bytearray(pick(rng, S8, n))
            others = [i for i in rng.permutation(n)[:4].tolist() if i != at][:3]
            for i, syms in zip(others, (S5, S6, S6)):
                d[i] = syms[int(rng.integers(len(syms)))]
            for over in (0, 1):
                d[at] = (S8 if over else S7)[int(rng.integers(6))]
                out.append(Case("verdict len %d, %s byte %d, %d bits" % (n, name, at, bits_of(d)), 1, d, kind="verdict",
                                len=n, spot=name, at=at, bits=bits_of(d), over=over))
    # the early break: a round that alone exceeds the limit, compressible text behind it
    for n, head, sym_len, rnd in ((200, 64, 30, 0), (300, 128, 28, 1), (768, 256, 28, 3), (1024, 320, 28, None),
                                  (33000, LONG_CHUNK, 28, 0)):
        d = pick(rng, BY_LEN[sym_len], head) + pick(rng, S5, n - head)
        out.append(Case("early break len %d: %d %d-bit symbols first" % (n, head, sym_len), 1, d, kind="early", len=n,
                        round=rnd))
    return out


def code_cases(rng):
    out = []
    for b in range(256):  # every code of the table between 5-bit symbols
        out.append(Case("symbol %#04x (%d bits)" % (b, NB[b]), 1, pick(rng, S5, 8) + bytes([b]) + pick(rng, S5, 8),
                        kind="code", sym=b, nbits=NB[b]))
    for b in LONG30:
        for k in range(32):  # 5 k mod 32 takes every value: the code's first bit at every offset of an output word
            for n in (k + 13, 800, 40000 if b == LONG30[0] and k % 4 == 0 else 0):
                if n:
                    d = pick(rng, S5, k) + bytes([b]) + pick(rng, S5, n - k - 1)
                    out.append(Case("30-bit %#04x at word offset %d, len %d" % (b, 5 * k % 32, n), 1, d, kind="long30",
                                    sym=b, at=k, word_off=5 * k % 32, len=n))
        for k in range(8):  # as the last symbol: 5 (16 + k) + 30 bits leave every pad width
            d = pick(rng, S5, 16 + k) + bytes([b])
            out.append(Case("30-bit %#04x last, pad %d" % (b, -bits_of(d) % 8), 1, d, kind="long30_last", sym=b,
                            pad=-bits_of(d) % 8))
    return out


def meeting_cases(rng):
    """block_encode<4>: k 5-bit symbols and 6-bit ones in wave 0's part put wave 1's first code at bit -k mod 32 of an
    output word; the other parts are text"""
    out = []
    for n in (1024, 1280):
        per = part_starts(n)[1]
        for k in range(1, 32):
            d = pick(rng, S5, k) + pick(rng, S6, per - k) + pick(rng, TEXT, n - per)
            out.append(Case("len %d: wave 1 starts at bit %d of its word" % (n, -k % 32), 1, d, kind="meeting", len=n,
                            word_off=-k % 32))
    return out


def residue_cases(rng):
    out = []
    for r in list(range(2, 38)) + [599, 600, 601]:
        n = max(r + 1, (8 * r + 6) // 7)
        for pad in (0, 3):
            if 5 * n <= 8 * r - pad:
                out.append(Case("encode to %d bytes, pad %d" % (r, pad), 1, exact_text(rng, n, 8 * r - pad), kind="out_len",
                                out_len=r, pad=pad))
    # decode: the largest mailbox answer and its neighbours, and answers of whole chunks
    for nbytes in (768, 767, 766):
        text = pick(rng, S5, 8 * nbytes // 5)
        out.append(Case("decode %d bytes of 5-bit codes" % nbytes, 0, pack(text), kind="dec_out", in_len=nbytes,
                        out_len=len(text)))
    for n in (11, 12, 13, 24, 600, 1224):
        text = pick(rng, S5 if n > 1000 else TEXT, n)
        out.append(Case("decode to %d bytes" % n, 0, pack(text), kind="dec_out", in_len=len(pack(text)), out_len=n))
    return out


@functools.lru_cache(None)
def corpus():
    rng = np.random.default_rng(0x5EC0DE)
    return tuple(length_cases(rng) + verdict_cases(rng) + code_cases(rng) + meeting_cases(rng) + residue_cases(rng))


# ------------------------------------------------------------------------------------------------
# calls with their expectations
# ------------------------------------------------------------------------------------------------
class Req:
    """one call and what it must give: ret (None: SIZE_MAX), out (the bytes behind dst), soft (the soft_errors word
    after the call: OR semantics, untouched by a call that fails)"""
    __slots__ = ("label", "op", "is_name", "soft_in", "data", "ret", "out", "soft", "st")

    def __init__(self, label, op, data, is_name=False, soft_in=0):
        self.label, self.op, self.data, self.is_name, self.soft_in = label, op, bytes(data), bool(is_name), soft_in
        self.ret = self.out = self.soft = self.st = None  # st: the soft bits the call itself adds

    def answer(self):
        return (self.ret, self.out, self.soft)


def ref_answer(op, data, is_name, soft_in=0):
    """huff_ref's answer to a call: (ret, out, soft)"""
    if op:
        enc = R.encode(data)
        return (None, b"", soft_in) if enc is None else (len(enc), enc, soft_in)
    dec, st = R.decode(data, is_name)
    return (None, b"", soft_in) if dec is None else (len(dec), dec, soft_in | st)


def oracle_answer(oracle, op, data, is_name, soft_in=0):
    """the oracle restatement's answer to the same call"""
    if op:
        enc = oracle.encode(data)
        return (None, b"", soft_in) if enc is None else (len(enc), enc, soft_in)
    dec, soft = oracle.decode(data, is_name, soft_in)
    return (None, b"", soft_in) if dec is None else (len(dec), dec, soft)


def expect(req, oracle=None):
    answer = functools.partial(oracle_answer, oracle) if oracle else ref_answer
    req.ret, req.out, req.soft = answer(req.op, req.data, req.is_name, req.soft_in)
    req.st = answer(req.op, req.data, req.is_name, 0)[2] if req.soft_in else req.soft
    return req


def corpus_reqs(cases, oracle=None, back=True):
    """every case as a call; behind every encode that succeeds, the decode of its result (back)"""
    out = []
    for c in cases:
        q = expect(Req(c.label, c.op, c.data, c.is_name), oracle)
        out.append(q)
        if back and c.op and q.ret is not None:
            out.append(expect(Req(c.label + " / decoded back", 0, q.out), oracle))
    return out


# ------------------------------------------------------------------------------------------------
# plans: T threads, PLAN_ROUNDS calls each, thread t on mailbox t mod 64
# ------------------------------------------------------------------------------------------------
PLAN_ROUNDS = 40
PLAN_MAX_THREADS = 72


def plan_len(t, r):
    """input bytes of thread t's call in round r.  Blocks of five rounds: long, short (768 then 1 for the thread
    whose j is 0), longer (more chunks than the hot read ahead), the same length again, shorter; j differs between
    the threads of a round, so no two requests posted together have one length"""
    b, k = divmod(r, 5)
    j = (t + 7 * b) % PLAN_MAX_THREADS
    return (SVC_MAX - 7 * j, 1 + 3 * j, 100 + 9 * j, 100 + 9 * j, 13 + 3 * j)[k]


def plan_op(t, r):
    """encode and decode alternate on every thread (two threads of one mailbox, t and t + 64, move together)"""
    return (t + r) & 1


def plan_fails(t, r):
    """the one request of a round that is built to fail (and the 1-byte encode of the short round fails by itself)"""
    b, k = divmod(r, 5)
    return k == 4 and (t + 7 * b) % PLAN_MAX_THREADS == 1 + (b & 1)  # (an encode and a decode in turn)


def chunks_differ(a, b):
    """every 12-byte chunk that both strings have bytes in differs within the bytes both have"""
    n = min(len(a), len(b))
    return all(a[i:min(i + SVC_CHUNK, n)] != b[i:min(i + SVC_CHUNK, n)] for i in range(0, n, SVC_CHUNK))


def _huff_input(rng, n, fail):
    """n Huffman bytes: text whose codes end 0..7 bits before the end (fail: EOS at the end instead)"""
    if fail:
        return _huff_input(rng, n - 4, False) + b"\xff\xff\xff\xff"
    syms, bits = bytearray(), 0
    pool = np.frombuffer(TEXT, np.uint8)
    for b in pool[rng.integers(0, len(pool), 8 * n // 5 + 2)].tolist():
        if bits + NB[b] > 8 * n - 13:
            break
        if n >= 24 and bits < 8 * n - 64 and rng.integers(50) == 0:
            b = int(rng.integers(256))  # now and then any symbol of the table
            if bits + NB[b] > 8 * n - 13:
                break
        syms.append(b)
        bits += NB[b]
    rem = 8 * n - bits  # 0..20: a last symbol or two and 0..7 ones
    while rem >= 8:
        L = int(rng.integers(5, 9)) if rem >= 13 or rem == 8 else 5
        syms.append(BY_LEN[L][int(rng.integers(len(BY_LEN[L])))])
        rem -= L
    out = pack(syms)
    assert len(out) == n, (n, len(out))
    return out


def _plain_input(rng, n, fail):
    if fail:
        return pick(rng, S8, n)
    d = bytearray(pick(rng, TEXT, n))
    if n >= 24:
        for i in rng.integers(0, n, n // 50).tolist():
            d[i] = int(rng.integers(256))
    return bytes(d)


@functools.lru_cache(None)
def _full_plan():
    """the plan of PLAN_MAX_THREADS threads; plan(T) is its first T threads.  A request is drawn again until it
    differs from every other request of its mailbox in every input chunk and every output chunk both have, and from
    every request of its round in the answer"""
    rng = np.random.default_rng(0x9A17B0)
    threads = [[] for _ in range(PLAN_MAX_THREADS)]
    boxes = [[] for _ in range(SVC_SLOTS)]
    for r in range(PLAN_ROUNDS):
        answers = set()
        for t in range(PLAN_MAX_THREADS):
            n, op, fail = plan_len(t, r), plan_op(t, r), plan_fails(t, r)
            for _ in range(200):
                data = (_plain_input if op else _huff_input)(rng, n, fail)
                q = expect(Req("plan t%d r%d %s %d B" % (t, r, "enc" if op else "dec", n), op, data,
                               is_name=bool(rng.integers(2)), soft_in=int(rng.choice((0, 0, 1, 2, 3, 0x10)))))
                if (q.ret is None) != (fail or (op and n < 3)):
                    continue
                if q.ret is not None and q.out in answers:
                    continue
                if all(chunks_differ(data, p.data) and chunks_differ(q.out, p.out) for p in boxes[t % SVC_SLOTS]):
                    break
            else:
                raise AssertionError("no request for thread %d round %d" % (t, r))
            answers.add(q.out)
            threads[t].append(q)
            boxes[t % SVC_SLOTS].append(q)
    return threads


def plan(nthreads):
    assert 1 <= nthreads <= PLAN_MAX_THREADS
    return _full_plan()[:nthreads]


def mailbox_of(t):
    return t % SVC_SLOTS


# ------------------------------------------------------------------------------------------------
# a plain model of the mailbox exchange (svc_call in hhuff_capi_string.hip, service_kernel in hhuff_kernels.hip)
# ------------------------------------------------------------------------------------------------
DEFECTS = ("trust_hot",      # the chunks read ahead for the hot mailbox are used without testing their tags
           "keep_ck_slot",   # ck_slot is not cleared after the first mailbox served in a poll
           "wrong_mailbox",  # the answer is stored to the wave's next mailbox, g + G (s + 1)
           "stale_out")      # the host takes an output chunk that carries the previous request's number
_ZERO = (0, bytes(SVC_CHUNK))


class _Box:
    def __init__(self):
        self.seq = 0
        self.hdr = (0, 0, 0, 0)
        self.chunk = [_ZERO] * SVC_IN_CHUNKS
        self.done = (0, 0, 0)
        self.outc = [_ZERO] * SVC_OUT_CHUNKS
        self.late = {}  # output chunks the device has stored but the host has not seen land yet


def model_run(threads, waves=SVC_WAVES, defect=None, limit=None):
    """the plan's calls through the model: rounds in lock step, threads t >= 64 after the first owners of their
    mailboxes.  In rounds 0, 3, .. the wave's read-ahead of its hot mailbox lands before the host's post, in rounds
    1, 4, .. between the first and the second half of the post's chunks, else after the post; the device's output
    chunks land after the host's first look at them.  -> [(thread, mailbox, round, label, what)] for every call whose
    answer is not the expected one"""
    assert defect is None or defect in DEFECTS
    G, M = waves, SVC_SLOTS // waves
    boxes = [_Box() for _ in range(SVC_SLOTS)]
    wave = [{"handled": [0] * M, "hot": 0, "hot_ck": 1} for _ in range(G)]
    known = {(q.op, q.data, q.is_name): (q.ret, q.out, q.st) for th in threads for q in th}
    bad = []

    def code(op, data, is_name):
        key = (op, data, bool(is_name))
        if key not in known:
            ret, out, soft = ref_answer(op, data, bool(is_name))
            known[key] = (ret, out, soft)
        return known[key]

    def post(m, q, lo, hi, header):
        bx = boxes[m]
        for i in range(lo, min(hi, (len(q.data) + SVC_CHUNK - 1) // SVC_CHUNK)):
            bx.chunk[i] = (bx.seq, q.data[SVC_CHUNK * i:SVC_CHUNK * i + SVC_CHUNK].ljust(SVC_CHUNK, b"\0"))
        if header:
            bx.hdr = (bx.seq, q.op, len(q.data), int(q.is_name))

    def ahead(g):
        w = wave[g]
        src = boxes[g + G * w["hot"]].chunk
        return [src[i] if i < w["hot_ck"] else _ZERO for i in range(SVC_IN_CHUNKS)]

    def poll(g, ck):
        w = wave[g]
        pend = [s for s in range(M) if boxes[g + G * s].hdr[0] - w["handled"][s] > 0]
        ck_slot = w["hot"]
        for s in pend:
            m = g + G * s
            tag, op, n, is_name = boxes[m].hdr
            need = (n + SVC_CHUNK - 1) // SVC_CHUNK
            stale = any(ck[i][0] != tag for i in range(need))
            if s != ck_slot or (stale and defect != "trust_hot"):
                ck = list(boxes[m].chunk)
            if defect != "keep_ck_slot":
                ck_slot = -1
            data = b"".join(c[1] for c in ck[:need])[:n]
            ret, out, st = code(op, data, is_name)
            to = boxes[g + G * ((s + 1) % M)] if defect == "wrong_mailbox" else boxes[m]
            for i in range(0, len(out), SVC_CHUNK):
                to.late[i // SVC_CHUNK] = (tag, out[i:i + SVC_CHUNK].ljust(SVC_CHUNK, b"\0"))
            to.done = (tag, 0xFFFFFFFF if ret is None else ret, 0x80 if ret is None else st)
            w["handled"][s], w["hot"], w["hot_ck"] = tag, s, min(n // SVC_CHUNK + 2, SVC_IN_CHUNKS)

    def collect(m, t, r, q):
        bx = boxes[m]
        n = bx.seq
        if bx.done[0] != n:
            return bad.append((t, m, r, q.label, "no answer (done carries %d, the request is %d)" % (bx.done[0], n)))
        ret = None if bx.done[1] == 0xFFFFFFFF else bx.done[1]
        out = bytearray()
        for i in range((ret + SVC_CHUNK - 1) // SVC_CHUNK if ret else 0):
            tag, data = bx.outc[i]
            if not (tag == n or (defect == "stale_out" and tag == n - 1)):
                if i in bx.late:
                    bx.outc[i] = bx.late.pop(i)
                tag, data = bx.outc[i]
                if tag != n:
                    return bad.append((t, m, r, q.label, "output chunk %d never arrives" % i))
            out += data
        soft = q.soft_in | (bx.done[2] & 3) if ret is not None else q.soft_in
        got = (ret, bytes(out[:ret or 0]), soft)
        if got != q.answer():
            what = "returns %r, expected %r" % (got[0], q.ret) if got[0] != q.ret else \
                "soft_errors %#x, expected %#x" % (soft, q.soft) if got[1] == q.out else \
                "byte %d differs" % next(i for i in range(len(q.out)) if got[1][i] != q.out[i])
            bad.append((t, m, r, q.label, what))

    def land(m):
        bx = boxes[m]
        for i, c in bx.late.items():
            bx.outc[i] = c
        bx.late = {}

    rounds = len(threads[0])
    for r in range(rounds):
        for lo in range(0, len(threads), SVC_SLOTS):  # the second owners of a mailbox call after the first
            calls = [(t, threads[t][r]) for t in range(lo, min(lo + SVC_SLOTS, len(threads)))]
            for t, q in calls:
                boxes[t % SVC_SLOTS].seq += 1
            when = r % 3
            cks = [ahead(g) for g in range(G)] if when == 0 else None
            for t, q in calls:
                post(t % SVC_SLOTS, q, 0, 2 if when == 1 else SVC_IN_CHUNKS, when != 1)
            if when == 1:
                cks = [ahead(g) for g in range(G)]
                for t, q in calls:
                    post(t % SVC_SLOTS, q, 2, SVC_IN_CHUNKS, True)
            if when == 2:
                cks = [ahead(g) for g in range(G)]
            for g in range(G):
                poll(g, cks[g])
            for t, q in calls:
                collect(t % SVC_SLOTS, t, r, q)
                if limit and len(bad) >= limit:
                    return bad
            for m in range(SVC_SLOTS):
                land(m)
    return bad


# ------------------------------------------------------------------------------------------------
# the files tests/per_string_check.c reads
# ------------------------------------------------------------------------------------------------
def write_cases(path, reqs):
    """'PSC1', u32 count; per call u32 op, is_name, soft_in, in_len, out_len, soft, label_len, pad and u64 ret
    (SIZE_MAX: the call fails), then the label, the input and the expected bytes"""
    with open(path, "wb") as f:
        f.write(b"PSC1" + struct.pack("<I", len(reqs)))
        for q in reqs:
            assert q.soft is not None, "expect() first"
            label = q.label.encode()
            f.write(struct.pack("<8IQ", q.op, int(q.is_name), q.soft_in, len(q.data), len(q.out), q.soft, len(label), 0,
                                SIZE_MAX if q.ret is None else q.ret))
            f.write(label + q.data + q.out)


KIND_CALLS, KIND_BATCH = 0, 1
FLAG_LOOP = 1  # go round the list until every thread without this flag is done


def write_plan(path, threads, lockstep=True):
    """'PSP1', u32 threads, u32 lockstep; per thread u32 kind, device, flags, count, then count x {u32 case, u32
    microseconds to sleep before the call}.  threads: [{"kind", "device", "flags", "calls": [(case, sleep_us)]}]"""
    with open(path, "wb") as f:
        f.write(b"PSP1" + struct.pack("<2I", len(threads), int(lockstep)))
        for th in threads:
            calls = th["calls"]
            f.write(struct.pack("<4I", th.get("kind", KIND_CALLS), th.get("device", 0), th.get("flags", 0), len(calls)))
            for case, sleep_us in calls:
                f.write(struct.pack("<2I", case, sleep_us))


def write_batch(path, strings, names, oracle):
    """a decode batch in the contiguous layout with the oracle's answers: 'PSB1', u32 n, u64 in_size, u64 out_size,
    in_off[n + 1], name words, exp_len[n], exp_status[n] padded to 4, the input, the expected output slots"""
    n = len(strings)
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(s) for s in strings])
    words = np.zeros((n + 31) // 32, np.uint32)
    size = int(off[n])
    out = np.zeros(8 * size // 5 + 16, np.uint8)
    exp_len, exp_st = np.zeros(n, np.uint32), np.zeros((n + 3) // 4 * 4, np.uint8)
    for i, s in enumerate(strings):
        if names[i]:
            words[i // 32] |= np.uint32(1 << (i % 32))
        ret, dec, soft = oracle_answer(oracle, 0, s, bool(names[i]))
        exp_len[i] = 0xFFFFFFFF if ret is None else ret
        exp_st[i] = 0x80 if ret is None else soft
        at = 8 * int(off[i]) // 5
        out[at:at + len(dec)] = np.frombuffer(dec, np.uint8)
    with open(path, "wb") as f:
        f.write(b"PSB1" + struct.pack("<IQQ", n, size, out.size))
        for a in (off, words, exp_len, exp_st, np.frombuffer(b"".join(strings), np.uint8), out):
            f.write(a.tobytes())
