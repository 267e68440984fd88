"""Token interning on the GPU (include/hhuff.h (2j)) through the C ABI, under the guarded-array pattern of
tests/bounds_harness.py: every output array has exactly its documented size between two sentinel zones, every input
byte that belongs to no string holds a fill pattern, every case runs with two fill / sentinel pairs (BH.RUNS), and
the whole write footprint is asserted -- the expected arrays are built from the sentinel, so a slot the call must
leave alone has to still hold it.  The reference is the model (tests/tokens_model.py), which test_tokens.py holds to
h2o_lookup_token's own answers."""
import numpy as np
import pytest

import bounds_harness as BH
import tokens_model as TM
from conftest import load_golden
from h2o_amd import codec as C
from test_tokens import encoder_sessions, qpack_sessions, strip

pytestmark = pytest.mark.gpu
LDS_BUDGET = 32768  # hhuff_tokens.hip kLdsBudget: larger tables are probed in global memory
MISS = 0xDEADBEEF


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from h2o_amd import build

    build.build(verbose=False)
    return torch


@pytest.fixture(scope="module")
def fx():
    return TM.load_fixture()


class Set:
    """a token set on the device with its model"""

    def __init__(self, torch, names, user):
        self.model = TM.Model(names, user)
        self.host = C.tokens_build(self.model.names, self.model.user)
        self.whole, self.table = BH.to_device(torch, embed(self.host, 0x3C))
        self.size = int(self.host.size)


def embed(a, fill):
    whole, inner = BH.guarded(np, a.size, fill)
    inner[:] = a
    return whole


def words_of(n):
    return (np.arange(n, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32) | np.uint32(1)


def sentinel_array(n, dtype, sentinel):
    return np.full(n * np.dtype(dtype).itemsize, sentinel, np.uint8).view(dtype)


def check_out(whole, want, sentinel, what):
    """the guarded buffer `whole` (host copy): its inner part equals `want` entry by entry, both guards are intact"""
    g = BH.GUARD
    got = whole[g:whole.size - g].view(want.dtype)
    assert got.size == want.size, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s[%d] = %r, want %r (%d differ)" % (what, bad[0], got[bad[0]], want[bad[0]], bad.size)
    assert (whole[:g] == sentinel).all() and (whole[whole.size - g:] == sentinel).all(), what + ": a guard byte was written"


def place(strings, fill, seed=1, starts=None, in_size=None):
    """the strings at rising offsets with 0..3 fill bytes in front of each (or at `starts`), in a buffer that ends
    with the last string's last byte (or has in_size bytes) -> (whole guarded buffer, in_size, off, len)"""
    rng = np.random.default_rng(seed)
    off, pos = [], 0
    for i, s in enumerate(strings):
        pos = pos + int(rng.integers(0, 4)) if starts is None else int(starts[i])
        off.append(pos)
        pos += len(s)
    end = max([o + len(s) for o, s in zip(off, strings)] + [0])
    in_size = end if in_size is None else in_size
    whole, data = BH.guarded(np, in_size, fill)
    for o, s in zip(off, strings):
        data[o:o + len(s)] = np.frombuffer(s, np.uint8)
    return whole, in_size, np.asarray(off, np.uint32), np.asarray([len(s) for s in strings], np.uint32)


def dev_u32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.uint32)).view(np.int32).copy()).cuda()


def gpu_strings(torch, ts, whole_in, in_size, off, length, n, sentinel, with_user=True, table=None, table_size=None):
    """hhuff_intern_strings on exact-size guarded arrays -> (token buffer, user_out buffer) as host copies, guards
    included"""
    _, din = BH.to_device(torch, whole_in)
    tok_w, tok = BH.guarded(torch, 4 * n, sentinel)
    usr_w, usr = BH.guarded(torch, 4 * n, sentinel)
    d_off, d_len = dev_u32(torch, off[:n]), dev_u32(torch, length[:n])
    table = ts.table if table is None else table
    rc = C.lib().hhuff_intern_strings(table.data_ptr(), ts.size if table_size is None else table_size, din.data_ptr(),
                                      in_size, d_off.data_ptr(), d_len.data_ptr(), n, tok.data_ptr(),
                                      usr.data_ptr() if with_user else None, MISS, C._stream(None))
    assert rc == 0
    torch.cuda.synchronize()
    return tok_w.cpu().numpy(), usr_w.cpu().numpy()


def check_strings(torch, ts, strings, what, starts=None, in_size=None, extra=(), counts=None):
    """the strings (and the raw (off, len) pairs of `extra`) against the model, both runs, every count of `counts`"""
    for fill, sentinel in BH.RUNS:
        whole, size, off, length = place(strings, fill, starts=starts, in_size=in_size)
        off = np.concatenate([np.asarray([e[0] for e in extra], np.uint32), off])
        length = np.concatenate([np.asarray([e[1] for e in extra], np.uint32), length])
        data = whole[BH.GUARD:BH.GUARD + size]
        want_t, want_u = ts.model.intern_strings(data, off, length, MISS, in_size=size)
        for n in counts or [off.size]:
            tok, usr = gpu_strings(torch, ts, whole, size, off, length, n, sentinel)
            check_out(tok, want_t[:n], sentinel, "%s: token (n = %d, fill %#x)" % (what, n, fill))
            check_out(usr, want_u[:n], sentinel, "%s: user_out (n = %d, fill %#x)" % (what, n, fill))
    return want_t


def mutations(names, rng, per=3):
    out = []
    for nm in names:
        for _ in range(per):
            k = int(rng.integers(0, 4))
            i = int(rng.integers(0, len(nm)))
            if k == 0:
                out.append(nm[:i] + bytes([(nm[i] + 1 + int(rng.integers(0, 255))) % 256]) + nm[i + 1:])
            elif k == 1 and len(nm) > 1:
                out.append(nm[:i] + nm[i + 1:])
            elif k == 2:
                out.append(nm + bytes([int(rng.integers(0, 256))]))
            else:
                out.append(nm[:max(1, i)])
    return out


# ---------------------------------------------------------------------------------------------------
# 1. the fixture's probes
# ---------------------------------------------------------------------------------------------------
def test_fixture_probes(torch_cuda, fx):
    """the whole probe list with the 85-name table: h2o_lookup_token's recorded answers, the word or miss_user"""
    ts = Set(torch_cuda, fx["names"], words_of(85))
    assert ts.size <= LDS_BUDGET
    want = check_strings(torch_cuda, ts, fx["probes"], "fixture probes")
    np.testing.assert_array_equal(want, fx["answer"])
    # user_out == NULL: the tokens alone, nothing else written
    whole, size, off, length = place(fx["probes"], 0x00)
    tok, usr = gpu_strings(torch_cuda, ts, whole, size, off, length, off.size, 0xA5, with_user=False)
    check_out(tok, fx["answer"], 0xA5, "token without user_out")
    assert (usr == 0xA5).all()


# ---------------------------------------------------------------------------------------------------
# 2. edge strings
# ---------------------------------------------------------------------------------------------------
EDGE_LENGTHS = (0, 1, 3, 4, 5, 31, 32, 33, 255, 256)


def edge_name(L):
    return bytes((7 * i + 3 * L) % 26 + 97 for i in range(L))


def test_edge_strings(torch_cuda, fx):
    """every length at every start offset modulo 4 (modulo 16 for 32 and 33), as a hit and with its last byte changed;
    a name that ends on the last byte of `in`, a range one byte past in_size, ranges that wrap 32 bits; n = 1, 63, 64,
    65 and 257 (one lane, a wave less one, a wave, a wave and one, a workgroup and one)"""
    names = [edge_name(L) for L in EDGE_LENGTHS if 1 <= L <= 255] + fx["names"]
    ts = Set(torch_cuda, names, words_of(len(names)))
    strings, starts, pos = [], [], 16
    for L in EDGE_LENGTHS:
        for r in range(16 if L in (32, 33) else 4):
            for hit in (True, False):
                s = edge_name(L)
                if not hit and L:
                    s = s[:-1] + bytes([s[-1] ^ 0x20])
                pos = (pos + 15) // 16 * 16 + r  # a fresh 16-byte line, start offset r: fill in front and behind
                strings.append(s)
                starts.append(pos)
                pos += L + 1
    rng = np.random.default_rng(5)
    for s in fx["names"] + mutations(fx["names"], rng, 1):  # more than 257 entries in all
        strings.append(s)
        starts.append(pos + int(rng.integers(0, 4)))
        pos = starts[-1] + len(s)
    strings.append(edge_name(33))  # the buffer ends with this name's last byte, at an odd address
    starts.append(pos + (0 if (pos + 33) % 4 else 1))
    in_size = starts[-1] + 33
    assert in_size % 4 != 0
    extra = [(in_size - 33, 33),                      # (first: n = 1 is the name on the last byte)
             (in_size - 32, 33), (in_size - 33, 34),  # one byte past in_size, the bytes inside are a name's
             (in_size, 0), (in_size, 1), (in_size + 5, 3), (0xFFFFFFFF, 1), (0xFFFFFF01, 255), (0xFFFFFFFF, 0xFFFFFFFF),
             (0, 0xFFFFFFFF), (16, 0x80000003)]
    want = check_strings(torch_cuda, ts, strings, "edge strings", starts=starts, in_size=in_size, extra=extra,
                         counts=(1, 63, 64, 65, 257, len(strings) + len(extra)))
    assert want[0] == names.index(edge_name(33)) and (want[1:len(extra)] == -1).all()
    k = len(extra)
    for L in EDGE_LENGTHS:  # the hits are hits and the near misses are misses
        for r in range(16 if L in (32, 33) else 4):
            assert want[k] == (names.index(edge_name(L)) if 1 <= L <= 255 else -1) and want[k + 1] == -1, (L, r)
            k += 2


# ---------------------------------------------------------------------------------------------------
# 3. sets
# ---------------------------------------------------------------------------------------------------
def colliding_sets():
    """the sets of tools/tokens_host.cpp: equal length and last byte; equal first dword"""
    a = [b"%04d-collide-x" % i for i in range(600)]
    b = []
    for i in range(600):
        b += [b"x-co%d" % i, b"x-co" + bytes([97 + i // 40]) * (i % 40 + 1)]
    return a, b


def big_set():
    rng = np.random.default_rng(11)
    out = []
    for i in range(4096):
        s = b"h%d-" % i
        L = i + 6 if i < 250 else 6 + int(rng.integers(0, 30))
        out.append(s + bytes(rng.integers(97, 123, L - len(s), dtype=np.uint8)))
    return out


@pytest.mark.parametrize("which", ["one", "last_byte", "first_dword"])
def test_small_and_colliding_sets(torch_cuda, which):
    names = dict(one=[b"x"], last_byte=colliding_sets()[0], first_dword=colliding_sets()[1])[which]
    ts = Set(torch_cuda, names, words_of(len(names)))
    rng = np.random.default_rng(3)
    probes = names + mutations(names, rng, 2) + [b"", b"X", b"xx", b"y", b"x" * 256]
    want = check_strings(torch_cuda, ts, probes, which)
    assert list(want[:len(names)]) == list(range(len(names)))


def test_4096_names_in_global_memory_and_a_set_that_fits(torch_cuda):
    """a table over the LDS budget is probed where it lies; the same strings against a set that is staged"""
    names = big_set()
    rng = np.random.default_rng(4)
    probes = names + mutations(names[::4], rng, 2)
    big = Set(torch_cuda, names, words_of(4096))
    small = Set(torch_cuda, names[1024:1536], words_of(512))  # (the short ones: 20 KiB of table)
    assert big.size > LDS_BUDGET >= small.size
    want = check_strings(torch_cuda, big, probes, "4096 names")
    assert list(want[:4096]) == list(range(4096))
    want = check_strings(torch_cuda, small, probes, "512 names")
    assert list(want[1024:1536]) == list(range(512)) and (want[:1024] == -1).all() and (want[1536:4096] == -1).all()


# ---------------------------------------------------------------------------------------------------
# 4. slots
# ---------------------------------------------------------------------------------------------------
def gpu_fields(torch, ts, arena, arena_size, name_off, name_len, first, nfields, nslots, sentinel, table=None,
               table_size=None):
    """hhuff_intern_fields on exact-size guarded outputs; arena: the device copy of the guarded arena's inner part"""
    tok_w, tok = BH.guarded(torch, 4 * nslots, sentinel)
    usr_w, usr = BH.guarded(torch, 4 * nslots, sentinel)
    d = [dev_u32(torch, a) for a in (name_off, name_len, first, nfields)]
    table = ts.table if table is None else table
    rc = C.lib().hhuff_intern_fields(table.data_ptr(), ts.size if table_size is None else table_size, arena.data_ptr(),
                                     arena_size, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                     len(nfields), nslots, tok.data_ptr(), usr.data_ptr(), MISS, C._stream(None))
    assert rc == 0
    torch.cuda.synchronize()
    return tok_w.cpu().numpy(), usr_w.cpu().numpy()


def check_fields(torch, ts, whole_arena, arena_size, name_off, name_len, first, nfields, what):
    """both sentinels: the field slots hold the model's answer, every other slot and both guards the sentinel"""
    nslots = int(first[-1])
    arena = whole_arena[BH.GUARD:BH.GUARD + arena_size]
    _, d_arena = BH.to_device(torch, whole_arena)  # (once: a decoder's arena is large)
    for _, sentinel in BH.RUNS:
        want_t, want_u = ts.model.intern_fields(arena, name_off, name_len, first, nfields, sentinel_array(nslots, np.int32, sentinel),
                                                sentinel_array(nslots, np.uint32, sentinel), MISS, arena_size)
        tok, usr = gpu_fields(torch, ts, d_arena, arena_size, name_off, name_len, first, nfields, nslots, sentinel)
        check_out(tok, want_t, sentinel, what + ": token")
        check_out(usr, want_u, sentinel, what + ": user_out")
    return want_t


SLOT_LAYOUT = (  # (slots of the block, nfields)
    (5, 0),      # no field
    (5, 5),      # nfields equal to the range
    (3, 9),      # nfields above the range: clamped
    (1, 1),      # a block of one slot
    (0, 3),      # no slot at all
    (56, 56),    # slots 14 .. 69: over slot 64
    (60, 58),    # 70 .. 129, fields up to 127: ends with a wave's last slot
    (70, 70),    # 130 .. 199: over 192
    (60, 10),    # 200 .. 259
    (64, 64),    # 260 .. 323: over 320
    (1, 2),
)
# more than 64 blocks begin inside one wave's 64 slots: blocks of one slot, and runs of blocks without any
MANY_BLOCKS = ((1, 1),) * 100 + ((0, 5),) * 150 + ((3, 2),) + ((0, 1),) * 70 + ((1, 1),) * 40 + ((2, 1),) * 50 + ((0, 0),) * 65


@pytest.mark.parametrize("layout", [SLOT_LAYOUT, MANY_BLOCKS], ids=["ranges", "many_blocks"])
def test_slots(torch_cuda, fx, layout):
    ts = Set(torch_cuda, fx["names"], words_of(85))
    first = np.concatenate([[0], np.cumsum([s for s, _ in layout])]).astype(np.uint32)
    nfields = np.array([f for _, f in layout], np.uint32)
    nslots = int(first[-1])
    rng = np.random.default_rng(8)
    pool = fx["names"] + mutations(fx["names"], rng, 1)
    for fill, _ in BH.RUNS:
        strings = [pool[int(rng.integers(0, len(pool)))] for _ in range(nslots)]
        whole, size, off, length = place(strings, fill, seed=9)
        listed = np.zeros(nslots, bool)
        listed[ts.model.field_slots(first, nfields)] = True
        off[~listed] = length[~listed] = 0xFFFFFFFF  # the slots no decoder writes
        want = check_fields(torch_cuda, ts, whole, size, off, length, first, nfields, "slots (fill %#x)" % fill)
        assert listed.sum() > nslots // 2 and (want[listed] >= 0).sum() > nslots // 5
    # one block, one slot; and blocks whose first slots lie past a wave's range
    whole, size, off, length = place([b"host"], 0x00)
    check_fields(torch_cuda, ts, whole, size, off, length, np.array([0, 1], np.uint32), np.array([1], np.uint32), "one slot")
    whole, size, off, length = place([b"host"] * 200, 0xFF)
    check_fields(torch_cuda, ts, whole, size, off, length, np.array([0, 0, 0, 200, 200], np.uint32),
                 np.array([4, 0, 130, 7], np.uint32), "empty blocks around one")


# ---------------------------------------------------------------------------------------------------
# 5. behind the decoders
# ---------------------------------------------------------------------------------------------------
REQ_WORD = dict(method=2, scheme=3, authority=4, path=5, protocol=6)  # hhuff_request_t words (content_length: 0-1)


def check_request_records(ts, want, first, nfields, req_words, what):
    """every field a request record names as method, scheme, authority, path or protocol carries that token"""
    ids, seen = ts.model.ids, 0
    req_words = np.ascontiguousarray(req_words, dtype=np.uint32).view(np.int32)
    for b in range(len(nfields)):
        for key, w in REQ_WORD.items():
            f = int(req_words[b][w])
            if f < 0 or f >= min(int(nfields[b]), int(first[b + 1]) - int(first[b])):
                continue
            ok = (ids[b":" + key.encode()], ids[b"host"]) if key == "authority" else (ids[b":" + key.encode()],)
            assert want[int(first[b]) + f] in ok, (what, b, key)
            seen += 1
    assert seen > len(nfields) // 2, what


def test_behind_the_hpack_request_decoder(torch_cuda, fx):
    from test_hpack_blocks import gpu_blocks

    g = load_golden("blocks_256")
    nconn = 300
    nblk = int(g["conn_first"][nconn])
    blk_off, conn_first = g["blk_off"][:nblk + 1].astype(np.uint32), g["conn_first"][:nconn + 1].astype(np.uint32)
    data = g["data"][:int(blk_off[-1])]
    r = gpu_blocks(torch_cuda, data, blk_off, conn_first, int(g["table_size"][0]), requests=True)
    ts = Set(torch_cuda, fx["names"], words_of(85))
    arena = np.ascontiguousarray(r["arena"])
    want = check_fields(torch_cuda, ts, embed(arena, 0x00), arena.size, r["name_off"], r["name_len"], blk_off,
                        r["nfields"][:nblk], "hpack requests")
    slots = ts.model.field_slots(blk_off, r["nfields"][:nblk])
    assert slots.size > 2000 and (want[slots] >= 0).sum() > slots.size // 2
    check_request_records(ts, want, blk_off, r["nfields"][:nblk], np.asarray(r["req"]).view(np.uint32), "hpack")


def test_behind_the_qpack_request_decoder(torch_cuda, fx):
    from test_qpack import golden_steps, gpu_session, req_words

    nconn, hts, mb, nbl, steps = golden_steps(load_golden("qpack"), "qreq")
    st = steps[0]
    r = gpu_session(torch_cuda, nconn, hts, mb, nbl, steps[:1], requests=True)[0]
    ts = Set(torch_cuda, fx["names"], words_of(85))
    sec_off = np.asarray(st["sec_off"], np.uint32)
    ns = sec_off.size - 1
    arena = np.ascontiguousarray(r["arena"])
    want = check_fields(torch_cuda, ts, embed(arena, 0xFF), arena.size, r["name_off"], r["name_len"], sec_off,
                        r["nfields"][:ns], "qpack requests")
    slots = ts.model.field_slots(sec_off, r["nfields"][:ns])
    assert slots.size > 500 and (want[slots] >= 0).sum() > slots.size // 2
    check_request_records(ts, want, sec_off, r["nfields"][:ns], req_words(r["req"], ns), "qpack")


# ---------------------------------------------------------------------------------------------------
# 6. before the encoders
# ---------------------------------------------------------------------------------------------------
def gpu_headers(torch, ts, data, hdr, sentinel, keep_mask=C.HDR_DONT_COMPRESS, table=None, table_size=None):
    """hhuff_intern_headers on an exact-size guarded hdr array -> (hdr records, token buffer) as host copies"""
    n = hdr.size
    _, din = BH.to_device(torch, embed(np.asarray(data, np.uint8), sentinel))
    hdr_w, dh = BH.to_device(torch, embed(hdr.view(np.uint8), sentinel))
    tok_w, tok = BH.guarded(torch, 4 * n, sentinel)
    table = ts.table if table is None else table
    rc = C.lib().hhuff_intern_headers(table.data_ptr(), ts.size if table_size is None else table_size, din.data_ptr(),
                                      len(data), dh.data_ptr(), n, keep_mask, tok.data_ptr(), C._stream(None))
    assert rc == 0
    torch.cuda.synchronize()
    return hdr_w.cpu().numpy(), tok_w.cpu().numpy()


def restore(torch, ts, st):
    """strip the token flags from the step's headers and let the GPU put them back: the hdr array is the original
    byte for byte (so no other byte of a record changed), the tokens are the model's, the guards intact"""
    for _, sentinel in BH.RUNS:
        hdr_w, tok_w = gpu_headers(torch, ts, st["data"], strip(st["hdr"]), sentinel)
        check_out(hdr_w, st["hdr"].view(np.uint8), sentinel, "hdr")
        _, want = ts.model.intern_headers(np.asarray(st["data"], np.uint8), strip(st["hdr"]))
        check_out(tok_w, want, sentinel, "token")
    g = BH.GUARD
    return hdr_w[g:hdr_w.size - g].view(C.HPE_HEADER_DTYPE).copy()


@pytest.mark.parametrize("requests", [False, True])
def test_before_the_hpack_encoder(torch_cuda, oracle_codec, fx, requests):
    """restored flags, then hhuff_hpack_flatten_responses on them: the restatement's bytes"""
    from oracle import oracle as O
    from test_hpenc import KEYS, frames_of, gpu_step, host, oracle_step

    words = TM.encoder_words(fx["flags"]) & ~np.uint32(C.HDR_LIKELY_TO_REPEAT)  # (2f) has no such flag
    ts = Set(torch_cuda, fx["names"], words)
    steps = encoder_sessions(requests)
    s = O.HpeSession(O.oracle(), steps[0]["conn_first"].size - 1)
    scratch = None
    for k, st in enumerate(steps):
        assert (st["hdr"]["flags"] & C.HDR_TOKEN).any() and (st["hdr"]["flags"] & C.HDR_DONT_COMPRESS).any()
        q = oracle_step(s, st)
        r = host(gpu_step(torch_cuda, dict(st, hdr=restore(torch_cuda, ts, st)), scratch=scratch, cont=k > 0))
        scratch = r["scratch"]
        for key in KEYS:
            np.testing.assert_array_equal(r[key], q[key], err_msg=key)
        assert frames_of(r["out"], st["out_off"], r["out_len"]) == frames_of(q["out"], st["out_off"], q["out_len"])


@pytest.mark.parametrize("requests", [False, True])
def test_before_the_qpack_session_encoder(torch_cuda, fx, requests):
    """the same once through hhuff_qpack_flatten_sessions, HHUFF_HDR_LIKELY_TO_REPEAT included, against the model"""
    import qpenc_dyn_model as M
    from test_qpenc_dyn import Gpu, same

    ts = Set(torch_cuda, fx["names"], TM.encoder_words(fx["flags"]))
    st = qpack_sessions(requests)
    nconn = st[0]["conn_first"].size - 1
    m, g = M.Model(nconn), Gpu(torch_cuda, nconn)
    for k, q in enumerate(st):
        assert (q["hdr"]["flags"] & C.HDR_LIKELY_TO_REPEAT).any()
        flags = C.QENC_CONTINUE if k else C.QENC_SET_CAPACITY
        same(g.step(dict(q, hdr=restore(torch_cuda, ts, q)), flags=flags), m.step(q, flags=flags), "step %d: " % k)


def test_headers_keep_mask_and_ranges(torch_cuda, fx):
    """keep_mask picks the bits that stay; a name out of range is a miss; token == NULL"""
    ts = Set(torch_cuda, fx["names"], TM.encoder_words(fx["flags"]))
    data = np.frombuffer(b"hostdatex-none", np.uint8)
    hdr = np.zeros(6, C.HPE_HEADER_DTYPE)
    hdr["name_off"], hdr["name_len"] = [0, 4, 8, 10, 0xFFFFFFF0, 0], [4, 4, 6, 5, 64, 0]
    hdr["value_off"], hdr["value_len"], hdr["flags"] = 0x11111111, 0x22222222, [0xFFFFFFFF, 1, 0xF0, 7, 3, 6]
    for keep in (C.HDR_DONT_COMPRESS, 0, 0xFFFFFFF9):
        want, wtok = ts.model.intern_headers(data, hdr, keep)
        for _, sentinel in BH.RUNS:
            hdr_w, tok_w = gpu_headers(torch_cuda, ts, data, hdr, sentinel, keep_mask=keep)
            check_out(hdr_w, want.view(np.uint8), sentinel, "hdr (keep %#x)" % keep)
            check_out(tok_w, wtok, sentinel, "token (keep %#x)" % keep)
    assert list(wtok) == [ts.model.ids[b"host"], ts.model.ids[b"date"], -1, -1, -1, -1]
    d, dh = dev_u32(torch_cuda, np.frombuffer(bytes(data) + b"\0\0", np.uint32)), dev_u32(torch_cuda, hdr.view(np.uint32))
    assert C.lib().hhuff_intern_headers(ts.table.data_ptr(), ts.size, d.data_ptr(), data.size, dh.data_ptr(), 6, 1, None,
                                        C._stream(None)) == 0
    torch_cuda.cuda.synchronize()
    assert dh.cpu().numpy().tobytes() == ts.model.intern_headers(data, hdr, 1)[0].tobytes()


# ---------------------------------------------------------------------------------------------------
# 7. the table header
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("damage", ["magic", "short"])
def test_table_header_is_checked(torch_cuda, fx, damage):
    """a changed magic, and a table_size 16 below the table's own: every token HHUFF_TOK_EFORMAT (in
    hhuff_intern_fields: every field's), user_out and the headers' flags untouched"""
    ts = Set(torch_cuda, fx["names"], TM.encoder_words(fx["flags"]))
    table, size = ts.table, ts.size
    if damage == "magic":
        host = ts.host.copy()
        host[0] ^= 1
        _, table = BH.to_device(torch_cuda, embed(host, 0x3C))
    else:
        size -= 16
    strings = fx["names"] + [b"nothing", b""]
    for fill, sentinel in BH.RUNS:
        whole, in_size, off, length = place(strings, fill)
        n = off.size
        tok, usr = gpu_strings(torch_cuda, ts, whole, in_size, off, length, n, sentinel, table=table, table_size=size)
        check_out(tok, np.full(n, C.TOK_EFORMAT, np.int32), sentinel, "strings: token")
        assert (usr == sentinel).all()
        first, nfields = np.array([0, 40, 40, n], np.uint32), np.array([3, 9, 100], np.uint32)
        want = sentinel_array(n, np.int32, sentinel)
        want[ts.model.field_slots(first, nfields)] = C.TOK_EFORMAT
        tok, usr = gpu_fields(torch_cuda, ts, BH.to_device(torch_cuda, whole)[1], in_size, off, length, first, nfields, n,
                              sentinel, table=table, table_size=size)
        check_out(tok, want, sentinel, "fields: token")
        assert (usr == sentinel).all()
        hdr = np.zeros(n, C.HPE_HEADER_DTYPE)
        hdr["name_off"], hdr["name_len"], hdr["flags"] = off, length, np.arange(n) % 8
        data = whole[BH.GUARD:BH.GUARD + in_size]
        hdr_w, tok_w = gpu_headers(torch_cuda, ts, data, hdr, sentinel, table=table, table_size=size)
        check_out(hdr_w, hdr.view(np.uint8), sentinel, "headers: hdr")
        check_out(tok_w, np.full(n, C.TOK_EFORMAT, np.int32), sentinel, "headers: token")
