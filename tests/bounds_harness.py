"""Exact-size buffers, poisoned inputs and write footprints for the batch API (include/hhuff.h) -- plain helpers,
no GPU.  A batch call gets `out`, `out_len` and `status` of exactly the documented size, each between two guard
zones filled with a sentinel; every input byte that belongs to no string holds a fill pattern.  check() compares a
result with the oracle's and asserts that nothing outside the call's footprint -- the bytes include/hhuff.h lets
it write -- changed.  Arena carves such buffers out of one host array (a pinned tensor's: the guards are pinned too).

Every case runs twice (RUNS): input fill 0x00 with output sentinel 0xA5, then 0xFF with 0x5A.  0xFF behind a
Huffman string reads as padding / EOS and 0x00 as further symbols, so a kernel that looks a byte too far
disagrees with the oracle in one of the two runs; and a kept byte that was never written cannot equal the oracle's
byte under both sentinels (0xA5 != 0x5A)."""
import ctypes

import numpy as np

FAIL = 0xFFFFFFFF
GUARD = 256
RUNS = ((0x00, 0xA5), (0xFF, 0x5A))  # (input fill, output sentinel)
EXTRA = 128  # poisoned entries behind every per-string input array


# ------------------------------------------------------------------------------------------------
# buffers
# ------------------------------------------------------------------------------------------------
def guarded(xp, nbytes, fill, guard=GUARD):
    """A buffer of guard + nbytes + guard bytes filled with `fill`: -> (whole, inner), inner = the nbytes in the
    middle, starting at a multiple of 16 (the batch API wants `in` and `out` 16-byte aligned).  xp is numpy or
    torch (device memory)."""
    assert guard % 16 == 0 and nbytes >= 0
    total = 2 * guard + nbytes
    if xp is np:
        raw = np.full(total + 16, fill, np.uint8)
        start = (-(raw.ctypes.data + guard)) % 16
        whole = raw[start:start + total]
        assert (whole.ctypes.data + guard) % 16 == 0
    else:
        whole = xp.full((total,), fill, dtype=xp.uint8, device="cuda")
        assert (whole.data_ptr() + guard) % 16 == 0
    return whole, whole[guard:guard + nbytes]


class Arena:
    """Guarded buffers carved out of one host array, for pinned memory: `buf` is the numpy view of a uint8 tensor
    made with pin_memory=True, so a buffer's guards are pinned too (and one allocation serves a whole test).
    guarded(nbytes, fill, offset) -> (whole, inner) as guarded(); inner starts `offset` bytes past a multiple of 16."""

    def __init__(self, buf):
        assert buf.dtype == np.uint8 and buf.ndim == 1 and buf.flags["C_CONTIGUOUS"]
        self.buf, self.pos = buf, 0

    def reset(self):
        self.pos = 0

    def guarded(self, nbytes, fill, offset=0, guard=GUARD):
        assert guard % 16 == 0 and nbytes >= 0 and 0 <= offset < 16
        start = self.pos + (offset - (self.buf.ctypes.data + self.pos + guard)) % 16
        total = 2 * guard + nbytes
        assert start + total <= self.buf.size, "arena of %d bytes exhausted" % self.buf.size
        whole = self.buf[start:start + total]
        whole[:] = fill
        self.pos = start + total
        assert (whole.ctypes.data + guard) % 16 == offset
        return whole, whole[guard:guard + nbytes]

    def copy(self, whole_np, offset=0, guard=GUARD):
        """a guarded numpy buffer copied into the arena with its guards"""
        whole, inner = self.guarded(whole_np.size - 2 * guard, 0, offset, guard)
        whole[:] = whole_np
        return whole, inner


def to_device(torch, whole_np, guard=GUARD):
    """a guarded numpy buffer copied to the device with its guards: -> (whole, inner) tensors"""
    whole = torch.from_numpy(np.ascontiguousarray(whole_np)).cuda()
    assert (whole.data_ptr() + guard) % 16 == 0
    return whole, whole[guard:whole.numel() - guard]


def entries(whole_np, dtype, guard=GUARD):
    """the inner part of a guarded numpy buffer as an array of dtype"""
    return whole_np[guard:whole_np.size - guard].view(dtype)


def name_bits(flags, fill, extra_words=8):
    """is_name_bits of the bools `flags`: the unused high bits of the last word and extra_words more words hold the
    run's fill pattern"""
    n = len(flags)
    words = np.full((n + 31) // 32 + extra_words, 0x01010101 * fill, np.uint32)
    bits = np.full(((n + 31) // 32) * 32, bool(fill & 1))
    bits[:n] = np.asarray(flags, bool)
    packed = np.packbits(bits, bitorder="little")
    words[:(n + 31) // 32] = packed.view(np.uint32)
    return words


def _poisoned(vals, poison):
    """vals followed by EXTRA in-range poison entries (poison(j) for the j-th)"""
    a = np.empty(len(vals) + EXTRA, np.uint32)
    a[:len(vals)] = vals
    a[len(vals):] = [poison(j) for j in range(EXTRA)]
    return a


REGION = {"encode": lambda L: L, "decode": lambda L: (8 * L) // 5, "flatten": lambda L: L + 11}


def place_input(strings, layout, in_off0=0, fill=0, in_size=None, op="encode", seed=0, guard=GUARD, permute=True):
    """The input arrays of one batch call in one of three layouts:
      "contiguous"  in_off[n + 1], the first string at in_off0 (0, 1, 7, 13 ...), implicit output slots
      "pairs"       in_off[n] + in_len[n]: the strings in a permuted order (permute=False: in index order, which
                    flatten's implicit slots in_off[i] + 11 i need) with 0..9 filler bytes between them (the
                    first at in_off0), implicit output slots
      "explicit"    the contiguous input with out_off[n]: destinations (regions of REGION[op] bytes) at every
                    alignment, in reversed order with gaps of 0..7 bytes (gap 0 occurs whenever n > 1: neighbours
                    share a dword and a 16-B chunk)
    Every byte that belongs to no string is `fill`: before the first string, the filler, from the last string to
    in_size (default: the end of the last string) and both guards.  The per-string arrays carry EXTRA poisoned
    entries past their end -- offsets 0 or in_size, lengths that stay inside the buffer -- so a kernel that reads
    one shows as a mismatch, never as a bad address.
    -> dict(whole, data, in_size, in_off, in_len, out_off, out_size, lens, n); whole is the guarded buffer, data its
    in_size inner bytes; in_off / in_len / out_off include the poison (the call sees n of them)."""
    rng = np.random.default_rng(seed)
    n = len(strings)
    lens = np.array([len(s) for s in strings], np.int64)
    if layout == "pairs":
        order = rng.permutation(n) if permute else np.arange(n)
        gaps = rng.integers(0, 10, n)
        starts = np.zeros(n, np.int64)
        pos = in_off0
        for k, i in enumerate(order):
            starts[i] = pos
            pos += int(lens[i]) + (int(gaps[k]) if k + 1 < n else 0)
        end = pos
    else:
        starts = in_off0 + np.concatenate([[0], np.cumsum(lens)[:-1]]) if n else np.zeros(0, np.int64)
        end = in_off0 + int(lens.sum())
    in_size = end if in_size is None else in_size
    assert in_size >= end and in_size < 2 ** 31
    whole, data = guarded(np, in_size, fill, guard)
    for s, st in zip(strings, starts):
        data[st:st + len(s)] = np.frombuffer(s, np.uint8)
    in_len = out_off = None
    if layout == "pairs":
        # a poisoned pair: (0, in_size) -- the whole buffer as one string -- or (in_size, 0)
        in_off = _poisoned(starts, lambda j: 0 if j % 2 == 0 else in_size)
        in_len = _poisoned(lens, lambda j: in_size if j % 2 == 0 else 0)
    else:
        in_off = _poisoned(np.append(starts, end), lambda j: 0 if j % 2 == 0 else in_size)
    out_size = None
    if layout == "explicit":
        reg = REGION[op](lens)
        gaps = rng.integers(0, 8, n)
        gaps[1::3] = 0  # (gaps[0] is not used: string 0 comes last)
        dst = np.zeros(n, np.int64)
        pos = int(rng.integers(0, 16))
        for i in reversed(range(n)):
            dst[i] = pos
            pos += int(reg[i]) + (int(gaps[i]) if i else 0)
        out_size = pos  # the exact end of the last region
        out_off = _poisoned(dst, lambda j: 0)
    return dict(whole=whole, data=data, in_size=in_size, in_off=in_off, in_len=in_len, out_off=out_off,
                out_size=out_size, lens=lens, n=n, layout=layout, end=end)


def implicit_out_size(op, inp):
    """include/hhuff.h's exact size of `out` for the implicit layouts"""
    if op == "decode":
        return (8 * inp["in_size"]) // 5
    if op == "encode":
        return inp["in_size"]
    return inp["end"] + 11 * inp["n"]  # contiguous: in_off[n] + 11 n


def out_starts(op, inp):
    """where string i's output begins"""
    n = inp["n"]
    if inp["out_off"] is not None:
        return inp["out_off"][:n].astype(np.int64)
    s = inp["in_off"][:n].astype(np.int64)
    return (8 * s) // 5 if op == "decode" else s + 11 * np.arange(n) if op == "flatten" else s


def footprint(op, layout, in_off, lens, n, out_off, size):
    """bool[size]: the bytes of `out` the call may write
      encode   [start_i, start_i + len_i)            start_i = out_off[i], or in_off[i]
      decode   explicit [out_off[i], out_off[i] + floor(8 len_i / 5));  implicit [floor(8 s_i / 5),
               floor(8 (s_i + len_i) / 5)) -- the slot, up to where the next input byte's slot would begin
      flatten  [start_i, start_i + len_i + 11)       start_i = out_off[i], or in_off[i] + 11 i"""
    s = np.asarray(in_off[:n], np.int64)
    L = np.asarray(lens[:n], np.int64)
    if layout == "explicit":
        lo = np.asarray(out_off[:n], np.int64)
        hi = lo + REGION[op](L)
    elif op == "decode":
        lo, hi = (8 * s) // 5, (8 * (s + L)) // 5
    elif op == "flatten":
        lo = s + 11 * np.arange(n)
        hi = lo + L + 11
    else:
        lo, hi = s, s + L
    return ranges_mask(lo, hi, size)


def ranges_mask(lo, hi, size):
    """bool[size], true in every [lo_i, hi_i)"""
    assert len(lo) == 0 or (np.min(lo) >= 0 and np.max(hi) <= size), "a region leaves the buffer"
    d = np.zeros(size + 1, np.int32)
    np.add.at(d, lo, 1)
    np.add.at(d, hi, -1)
    return np.cumsum(d, dtype=np.int32)[:size] > 0


# ------------------------------------------------------------------------------------------------
# the check
# ------------------------------------------------------------------------------------------------
def check(result, oracle_result, mask, sentinel, starts=None, label="", guard=GUARD):
    """result: name -> the whole guarded buffer (numpy u8, guards included) of every array the call wrote;
    oracle_result: name -> the oracle's array (its dtype says how to read the buffer).  Asserts that
      - every array but "out" (out_len, status, out_off ...) equals the oracle's, entry by entry;
      - the kept bytes of "out" -- [starts[i], starts[i] + out_len[i]) of the strings that did not fail -- equal
        the oracle's (starts: default the oracle's "out_off");
      - every byte of "out" outside `mask`, both guards included, still holds `sentinel`;
      - the guards of the other arrays are intact."""
    def fail(msg):
        raise AssertionError("%s: %s" % (label, msg))

    for name, exp in oracle_result.items():
        if name == "out":
            continue
        whole = result[name]
        got = whole[guard:whole.size - guard].view(exp.dtype)
        if got.size != exp.size:
            fail("%s has %d entries, the oracle %d" % (name, got.size, exp.size))
        bad = np.nonzero(got != exp)[0]
        if bad.size:
            fail("%s[%d] = %#x, oracle %#x (%d differ)" % (name, bad[0], got[bad[0]], exp[bad[0]], bad.size))
        for side, g in (("front", whole[:guard]), ("rear", whole[whole.size - guard:])):
            hit = np.nonzero(g != sentinel)[0]
            if hit.size:
                fail("%s: %s guard byte %d written (%#x)" % (name, side, hit[0], g[hit[0]]))
    whole = result["out"]
    out = whole[guard:whole.size - guard]
    exp = oracle_result["out"]
    if out.size != exp.size or mask.size != out.size:
        fail("out has %d bytes, the oracle %d, the mask %d" % (out.size, exp.size, mask.size))
    olen = oracle_result["out_len"].astype(np.int64)
    ok = olen != FAIL
    st = np.asarray(oracle_result["out_off"][:olen.size] if starts is None else starts, np.int64)
    kept = ranges_mask(st[ok], st[ok] + olen[ok], out.size)
    if (kept & ~mask).any():
        fail("an output lies outside the footprint (byte %d)" % np.nonzero(kept & ~mask)[0][0])
    bad = np.nonzero(kept & (out != exp))[0]
    if bad.size:
        i = int(np.searchsorted(np.sort(st[ok]), bad[0], side="right")) - 1
        fail("out[%d] = %#x, oracle %#x (%d kept bytes differ; region %d in output order)"
             % (bad[0], out[bad[0]], exp[bad[0]], bad.size, i))
    stray = whole != sentinel
    stray[guard:guard + out.size] &= ~mask
    hit = np.nonzero(stray)[0]
    if hit.size:
        fail("out byte %d (buffer of %d) written outside the footprint: %#x (%d bytes)"
             % (hit[0] - guard, out.size, whole[hit[0]], hit.size))


# ------------------------------------------------------------------------------------------------
# the oracle as an implementation: its batch drivers write into the caller's (guarded) arrays
# ------------------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def oracle_into(codec, op, inp, out, out_len, status=None, names=None, prefix_bits=7, first=None, raw=None):
    """run the oracle's batch driver of `op` on place_input()'s arrays, writing into out / out_len / status (numpy
    views, e.g. the inner parts of guarded buffers)"""
    f = getattr(codec.lib, "%s_%s_batch" % (codec.prefix, op))
    V = ctypes.c_void_p
    n = inp["n"]
    # the driver takes no in_size: it addresses data through the offsets alone
    head = [_p(inp["data"]), _p(inp["in_off"]), _p(inp["in_len"]), ctypes.c_uint32(n)]
    if op == "decode":
        f.argtypes = [V] * 3 + [ctypes.c_uint32] + [V] * 5 + [ctypes.c_int]
        rc = f(*head, _p(names), _p(out), _p(inp["out_off"]), _p(out_len), _p(status), 1)
    elif op == "encode":
        f.argtypes = [V] * 3 + [ctypes.c_uint32] + [V] * 4 + [ctypes.c_int]
        rc = f(*head, _p(out), _p(inp["out_off"]), _p(out_len), _p(status), 1)
    else:
        f.argtypes = [V] * 3 + [ctypes.c_uint32, V, ctypes.c_uint] + [V] * 4 + [ctypes.c_int]
        rc = f(*head, _p(first), prefix_bits, _p(raw), _p(out), _p(inp["out_off"]), _p(out_len), 1)
    assert rc == 0


def oracle_run(codec, op, inp, sentinel, names=None, prefix_bits=7, first=None, raw=None):
    """the oracle on guarded, sentinel-filled exact-size arrays: -> (result for check(), oracle_result)"""
    n = inp["n"]
    size = inp["out_size"] if inp["out_off"] is not None else implicit_out_size(op, inp)
    res = {"out": guarded(np, size, sentinel)[0], "out_len": guarded(np, 4 * n, sentinel)[0]}
    if op != "flatten":
        res["status"] = guarded(np, n, sentinel)[0]
    oracle_into(codec, op, inp, entries(res["out"], np.uint8), entries(res["out_len"], np.uint32),
                entries(res["status"], np.uint8) if op != "flatten" else None, names, prefix_bits, first, raw)
    exp = {"out": entries(res["out"], np.uint8).copy(), "out_len": entries(res["out_len"], np.uint32).copy()}
    if op != "flatten":
        exp["status"] = entries(res["status"], np.uint8).copy()
    return res, exp


def mask_of(op, inp):
    size = inp["out_size"] if inp["out_off"] is not None else implicit_out_size(op, inp)
    return footprint(op, inp["layout"], inp["in_off"], inp["lens"], inp["n"], inp["out_off"], size)


# ------------------------------------------------------------------------------------------------
# batches (seeded; built once at their largest count, a case takes the first n strings)
# ------------------------------------------------------------------------------------------------
LONG_CODES = np.frombuffer(b"{}~^|<>\\", np.uint8)


def _alphabet():
    from h2o_amd import synth, tables

    syms, p = synth.header_alphabet()
    return syms, p, np.asarray(tables.ENC_NBITS, np.int64)


def text(rng, L):
    syms, p, _ = _alphabet()
    return bytes(rng.choice(syms, int(L), p=p))


def text_for_huffman_len(rng, L):
    """header text whose Huffman string is exactly L bytes long"""
    if L == 0:
        return b""
    syms, p, nbits = _alphabet()
    t = rng.choice(syms, (8 * L) // 5 + 8, p=p)
    cum = np.cumsum(nbits[t])
    t = list(t[:int(np.searchsorted(cum, 8 * L - 5, side="right"))])
    r = 8 * L - int(nbits[t].sum()) if t else 8 * L
    while r > 12:
        t.append(ord("e"))  # 5 bits
        r -= 5
    if r >= 5:  # a last symbol of min(r, 8) bits leaves at most 4 bits of padding
        t.append({5: ord("e"), 6: ord("d"), 7: ord("j"), 8: ord("X")}[min(r, 8)])
        r -= min(r, 8)
    assert 0 <= r <= 7
    return bytes(np.asarray(t, np.uint8))


def huffman(plain):
    """the RFC 7541 Huffman string of `plain` (any length: h2o's encoder returns only those shorter than the
    plain string), padded with ones"""
    from h2o_amd import tables

    t = np.frombuffer(plain, np.uint8)
    nb = np.asarray(tables.ENC_NBITS, np.int64)[t]
    code = np.asarray(tables.ENC_CODE, np.int64)[t]
    start = np.cumsum(nb) - nb
    total = int(nb.sum())
    bits = np.ones((total + 7) // 8 * 8, np.uint8)
    for j in range(int(nb.max()) if t.size else 0):
        m = nb > j
        bits[start[m] + j] = (code[m] >> (nb[m] - 1 - j)) & 1
    return np.packbits(bits).tobytes()


def huffman_of_len(oracle, rng, L):
    plain = text_for_huffman_len(rng, L)
    h = huffman(plain)
    assert len(h) == L and (L < 8 or h == oracle.encode(plain)), L
    return h


def corrupt(rng, h):
    """bad padding, an EOS inside, truncation, or a zero byte appended"""
    k = int(rng.integers(4))
    h = bytearray(h)
    if k == 0 and h:
        h[-1] &= 0xFE
    elif k == 1:
        cut = int(rng.integers(0, len(h) + 1))
        h[cut:cut] = b"\xff\xff\xff\xff"
    elif k == 2 and len(h) > 1:
        h = h[:int(rng.integers(1, len(h)))]
    else:
        h += b"\x00"
    return bytes(h)


def huffman_batch(oracle, kind, n, seed):
    """n Huffman strings (about 5 % corrupted) and their name flags:
      "short"  Huffman lengths 0..39, several empty
      "mixed"  Zipf 8..512
      "long"   130..900 B, with strings of exactly 4095, 4096 and 4097 Huffman bytes at indices 1, 2 and 40"""
    rng = np.random.default_rng(seed)
    if kind == "short":
        lens = rng.integers(0, 36, n)
        lens[rng.random(n) < 0.06] = 0
        lens[::7] = rng.integers(36, 40, len(lens[::7]))
        lens[0] = 23
    elif kind == "mixed":
        L = np.arange(8, 513)
        lens = rng.choice(L, n, p=(1.0 / L) / (1.0 / L).sum())
    else:
        lens = rng.integers(130, 901, n)
        for i, v in ((1, 4095), (2, 4096), (40, 4097)):
            if i < n:
                lens[i] = v
    out = [huffman_of_len(oracle, rng, int(v)) for v in lens]
    cap = 39 if kind == "short" else 1 << 30
    for i in np.nonzero(rng.random(n) < 0.05)[0]:
        if kind == "long" and i in (1, 2, 40):
            continue
        c = corrupt(rng, out[i])
        if len(c) <= cap:
            out[i] = c
    return out, rng.random(n) < 0.5


def plain_batch(kind, n, seed):
    """n plain strings for encode / flatten: the texts of the Huffman batches' lengths (x 8/6), with arbitrary bytes
    and long-code-only strings among them, so that failures (HHUFF_FAIL_LEN) sit next to successes"""
    rng = np.random.default_rng(seed)
    if kind == "short":
        lens = rng.integers(0, 50, n)
        lens[rng.random(n) < 0.06] = 0
        lens[0] = 31
    elif kind == "mixed":
        L = np.arange(8, 683)
        lens = rng.choice(L, n, p=(1.0 / L) / (1.0 / L).sum())
    else:
        lens = rng.integers(170, 1200, n)
        for i, v in ((1, 5450), (2, 3584), (40, 8200)):
            if i < n:
                lens[i] = v
    out = []
    for i, L in enumerate(lens):
        k = rng.random()
        if i and k < 0.08:
            out.append(bytes(rng.choice(LONG_CODES, int(L))))
        elif i and k < 0.14:
            out.append(bytes(rng.integers(0, 256, int(L), dtype=np.uint8)))
        else:
            out.append(text(rng, L))
    return out
