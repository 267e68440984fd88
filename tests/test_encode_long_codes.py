"""Codes longer than 16 bits in strings that compress, through every batch encoder.

The sorted and the staged encoders place a dword that holds such a code in a second walk over the string, and only
for strings that were kept (encode_chunk_v2's DEFER_LONG); the proportional-lane encoder and the framing kernel
place it on the spot.  The strings here are header text with one to three bytes whose codes have 19..30 bits: in the
head dword, in a whole dword and in the tail dword of a string that starts at each alignment mod 4, two of them in
one dword, with loose text (kept), text of 8-bit codes (fails) and text chosen so that the code bits are exactly
8 len - 8 (the longest that is kept) and 8 len - 7 (the shortest that fails).

Every case compares out_len, status and the bytes inside each kept slot with oracle.oracle().encode_batch (slot
tails and the slots of failing strings are unspecified), with the chunks' shared 16-B edges stored in the kernel and
deferred to the fix-up kernel.  The oracle alone first shows that the case set holds kept and failing strings of
each placement."""
import numpy as np
import pytest

from h2o_amd import tables

pytestmark = pytest.mark.gpu

FAIL = 0xFFFFFFFF
NBITS = np.asarray(tables.ENC_NBITS[:256], np.int64)
RARE = [b for b in range(256) if 19 <= NBITS[b] <= 30]
RARE30 = [10, 13, 22]
TEXT = {k: [c for c in range(0x20, 0x7F) if NBITS[c] == k] for k in (5, 6, 7, 8)}
LOOSE = TEXT[5] + TEXT[6] + TEXT[7]
PLACEMENTS = ("head", "whole", "tail", "pair")
VERDICTS = ("loose", "tight", "edge_kept", "edge_fail")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


assert all(NBITS[b] == 30 for b in RARE30) and set(RARE30) <= set(RARE) and all(TEXT[k] for k in TEXT)


def header_strings(rng, lens):
    return [rng.choice(LOOSE + TEXT[8], int(L)).astype(np.uint8) for L in lens]


def rare_string(rng, off, placement, verdict, lo=24, hi=72, nrare=None):
    """One string for byte offset `off`: rare bytes by `placement`, the text around them by `verdict`.
    -> (bytes, placement used): a string that starts on a dword has no head dword, its rare byte goes to a whole one."""
    if placement == "head" and off % 4 == 0:
        placement = "whole"
    while True:
        L = int(rng.integers(lo, hi + 1))
        if placement == "tail" and (off + L) % 4 == 0:
            continue
        k = int(rng.integers(1, 4)) if nrare is None else nrare
        if placement == "pair":
            k = max(k, 2)
        vals = [int(rng.choice(RARE30 if rng.random() < 0.4 else RARE)) for _ in range(k)]
        R = int(NBITS[vals].sum())
        d = R - 8 * k + (8 if verdict == "edge_kept" else 7)  # bits to take off text of 8-bit codes
        if verdict.startswith("edge") and d > 3 * (L - k):
            continue
        if verdict == "loose" and R + 6 * (L - k) > 8 * L - 8:  # text of 5- and 6-bit codes must keep it
            continue
        break
    first_whole = (4 - off % 4) % 4              # string index of the first whole dword's first byte
    n_whole = (L - first_whole) // 4
    tail0 = L - (off + L) % 4
    if placement == "head":
        pos = [int(rng.integers(0, 4 - off % 4))]
    elif placement == "tail":
        pos = [int(rng.integers(tail0, L))]
    else:
        w = first_whole + 4 * int(rng.integers(0, n_whole))
        pos = [w + int(b) for b in rng.choice(4, 2 if placement == "pair" else 1, replace=False)]
    free = [i for i in range(L) if i not in pos]
    pos += [int(i) for i in rng.choice(free, k - len(pos), replace=False)]
    s = np.empty(L, np.uint8)
    text = np.array([i for i in range(L) if i not in pos])
    if verdict == "loose":
        s[text] = rng.choice(TEXT[5] + TEXT[6], text.size)
    else:
        s[text] = rng.choice(TEXT[8], text.size)
        if verdict.startswith("edge"):
            cut = rng.permutation(text)
            s[cut[:d // 3]] = rng.choice(TEXT[5], d // 3)
            if d % 3:
                s[cut[d // 3]] = rng.choice(TEXT[8 - d % 3])
    s[pos] = vals
    bits = int(NBITS[s].sum())
    if verdict.startswith("edge"):
        assert bits == 8 * L - (8 if verdict == "edge_kept" else 7)
    return s, placement


def rare_batch(rng, n, off0, lo, hi, every=1):
    """n strings from offset off0: every `every`-th one a rare_string; the start alignments come from the lengths, and
    each alignment goes through the placements and verdicts in a rotation of its own
    -> strings, tags [(index, alignment, placement, verdict)]"""
    strings, tags, off, count = [], [], off0, [0] * 4
    for i in range(n):
        if i % every == 0:
            c = count[off % 4]
            count[off % 4] += 1
            p, v = PLACEMENTS[c % 4], VERDICTS[(c // 4 + c) % 4]
            s, p = rare_string(rng, off, p, v, lo, hi)
            tags.append((i, off % 4, p, v))
        else:
            s = header_strings(rng, [rng.integers(lo, hi + 1)])[0]
        strings.append(s)
        off += len(s)
    return strings, tags


def layout(strings, off0=0, fill=0xFF):
    lens = np.array([len(s) for s in strings], np.int64)
    in_off = np.empty(len(strings) + 1, np.uint32)
    in_off[0] = off0
    in_off[1:] = off0 + np.cumsum(lens)
    data = np.full(int(in_off[-1]) + 48, fill, np.uint8)
    data[off0:int(in_off[-1])] = np.concatenate(strings)
    return data, in_off


def slot_positions(starts, lens):
    lens = lens.astype(np.int64)
    return np.repeat(starts.astype(np.int64) - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()))


def coverage(tags, r_len, need_align=True):
    """the oracle's verdicts by placement: every placement kept and failing, both edge verdicts as constructed, and
    (need_align) every start alignment with a kept rare byte in each kind of dword it has"""
    kept = {(a, p) for i, a, p, v in tags if r_len[i] != FAIL}
    for i, a, p, v in tags:
        if v in ("loose", "edge_kept"):
            assert r_len[i] != FAIL, (i, p, v)
        else:
            assert r_len[i] == FAIL, (i, p, v)
    for p in PLACEMENTS:
        for v in VERDICTS:
            assert any(t[2] == p and t[3] == v for t in tags), (p, v)
    if need_align:
        want = {(a, p) for a in range(4) for p in PLACEMENTS if not (a == 0 and p == "head")}
        assert want <= kept, want - kept


def check(torch, oracle, strings, off0=0, label="", mean=None, route="contiguous"):
    """the batch through `route` against the oracle: contiguous (hhuff_encode_batch's implicit slots), explicit
    (in_len / out_off: the staged kernels) or packed (hhuff_encode_batch_packed)"""
    from h2o_amd import codec

    data, in_off = layout(strings, off0)
    n = len(strings)
    in_size = int(in_off[-1])
    if mean is not None:
        assert mean[0] <= in_size // n <= mean[1], (label, in_size // n)
    kw, okw, o_starts = {}, {}, in_off[:-1].astype(np.int64)
    if route == "explicit":  # slots of len + 3 bytes, in reverse order
        in_len = np.diff(in_off.astype(np.int64)).astype(np.uint32)
        sizes = in_len.astype(np.int64) + 3
        out_off = (np.cumsum(sizes[::-1]) - sizes[::-1])[::-1].astype(np.uint32)
        okw = dict(in_len=in_len, out_off=np.ascontiguousarray(out_off), out_size=int(sizes.sum()) + 16)
        o_starts = out_off.astype(np.int64)
        in_off = np.ascontiguousarray(in_off[:-1])
    r_out, r_len, r_st = oracle.encode_batch(data, in_off, n, **okw)
    kept = r_len != FAIL
    pos = slot_positions(o_starts[kept], r_len[kept])
    d_data = torch.from_numpy(data).cuda()
    d_off = torch.from_numpy(in_off.view(np.int32)).cuda()
    if route == "explicit":
        kw = dict(in_len=torch.from_numpy(okw["in_len"].view(np.int32)).cuda(),
                  out_off=torch.from_numpy(okw["out_off"].view(np.int32)).cuda())
    for defer in (0xFFFFFFFF, 0):
        prev = codec.set_edge_defer_min(defer)
        try:
            out = torch.full((okw.get("out_size", in_size + 16),), 0xA5, dtype=torch.uint8, device="cuda")
            if route == "packed":
                _, g_off, g_len, g_st = codec.encode_batch_packed(d_data, d_off, n, out=out, in_size=in_size)
                g_off = g_off.cpu().numpy().view(np.uint32).astype(np.int64)
            else:
                _, g_len, g_st = codec.encode_batch(d_data, d_off, n, out=out, in_size=in_size, **kw)
            torch.cuda.synchronize()
        finally:
            codec.set_edge_defer_min(prev)
        g_len = g_len.cpu().numpy().view(np.uint32)[:n]
        g_st = g_st.cpu().numpy()[:n]
        g_out = out.cpu().numpy()
        what = "%s %s off0=%d defer=%#x" % (label, route, off0, defer)
        bad = np.nonzero(g_len != r_len)[0]
        assert bad.size == 0, (what, "out_len", bad[:8], g_len[bad[:8]], r_len[bad[:8]])
        bad = np.nonzero(g_st != r_st)[0]
        assert bad.size == 0, (what, "status", bad[:8], g_st[bad[:8]], r_st[bad[:8]])
        g_pos = pos
        if route == "packed":  # a tile's kept strings back to back from the tile's first slot
            klen = np.where(kept, r_len, 0).astype(np.int64)
            run = np.cumsum(klen) - klen
            exp_off = o_starts[(np.arange(n) // 64) * 64] + run - run[(np.arange(n) // 64) * 64]
            assert np.array_equal(g_off[:n], exp_off), (what, "out_off")
            assert g_off[n] == exp_off[-1] + klen[-1], (what, "out_off[n]")
            g_pos = slot_positions(exp_off[kept], r_len[kept])
        bad = np.nonzero(g_out[g_pos] != r_out[pos])[0]
        if bad.size:
            i = int(np.nonzero(kept)[0][np.searchsorted(np.cumsum(r_len[kept].astype(np.int64)), bad[0], side="right")])
            assert False, (what, "bytes", "kept string", i, len(bad))


# ---- rare bytes in compressible strings, both stages (n = 600: two chunk boundaries) --------------------------------
@pytest.mark.parametrize("lo,hi,mean", [(24, 70, (40, 48)), (30, 72, (49, 52))])
def test_placements_sorted(torch_cuda, oracle_codec, lo, hi, mean):
    """mean <= 48: the small stage's kernel; 49..52: the large stage's"""
    for off0 in (0, 3):
        strings, tags = rare_batch(np.random.default_rng(100 + lo + off0), 600, off0, lo, hi)
        data, in_off = layout(strings, off0)
        coverage(tags, oracle_codec.encode_batch(data, in_off, 600)[1])
        check(torch_cuda, oracle_codec, strings, off0=off0, label="placements", mean=mean)


# ---- who needs the second walk -------------------------------------------------------------------------------------
def test_one_lane_of_a_wave(torch_cuda, oracle_codec):
    """one kept string with a rare byte among 599 of plain text, at each placement"""
    for k, p in enumerate(PLACEMENTS):
        rng = np.random.default_rng(200 + k)
        strings = header_strings(rng, rng.integers(24, 70, 600))
        off = 1 + sum(len(s) for s in strings[:77])
        strings[77], _ = rare_string(rng, off, p, "edge_kept" if k % 2 else "loose", lo=len(strings[77]),
                                     hi=len(strings[77]) + 3)
        r_len = oracle_codec.encode_batch(*layout(strings, 1), 600)[1]
        assert r_len[77] != FAIL
        check(torch_cuda, oracle_codec, strings, off0=1, label="one lane " + p, mean=(40, 48))


def test_whole_length_group(torch_cuda, oracle_codec):
    """the 64 longest strings of a chunk (one wave's length group after the sort) all kept with rare bytes, the other
    192 plain and shorter; the chunk behind it plain"""
    rng = np.random.default_rng(210)
    strings = header_strings(rng, rng.integers(24, 56, 400))
    off = 2
    for i in range(256):
        if i % 4 == 1:
            strings[i], _ = rare_string(rng, off, PLACEMENTS[(i // 4) % 4], ("loose", "edge_kept")[(i // 16) % 2],
                                        lo=68, hi=72)
        off += len(strings[i])
    r_len = oracle_codec.encode_batch(*layout(strings, 2), 400)[1]
    assert (r_len[1:256:4] != FAIL).all()
    check(torch_cuda, oracle_codec, strings, off0=2, label="length group", mean=(40, 48))


def test_only_failing_rare_strings(torch_cuda, oracle_codec):
    """no string needs the second walk: every rare-byte string fails (at the edge and clearly), and the plain
    neighbours' kept bytes are intact"""
    rng = np.random.default_rng(220)
    strings = header_strings(rng, rng.integers(24, 70, 600))
    off, hit = 3, []
    for i in range(600):
        if i in range(100, 107) or i in (0, 255, 256, 300, 511, 599) or i % 50 == 9:
            strings[i], _ = rare_string(rng, off, PLACEMENTS[i % 4], ("tight", "edge_fail")[len(hit) % 2])
            hit.append(i)
        off += len(strings[i])
    r_len = oracle_codec.encode_batch(*layout(strings, 3), 600)[1]
    assert (r_len[hit] == FAIL).all() and (r_len != FAIL).sum() > 500
    check(torch_cuda, oracle_codec, strings, off0=3, label="failing only", mean=(40, 48))


# ---- the other routes ----------------------------------------------------------------------------------------------
def test_chunk_past_its_stage(torch_cuda, oracle_codec):
    """a string of about 13,400 B in the second chunk sends that chunk to the per-thread path; the chunks around it are
    staged (its length keeps the later strings' alignments)"""
    rng = np.random.default_rng(230)
    strings, tags = rare_batch(rng, 1024, 0, 24, 40, every=3)
    strings[300] = header_strings(rng, [13400 + (len(strings[300]) - 13400) % 4])[0]
    tags = [t for t in tags if t[0] != 300]
    data, in_off = layout(strings)
    coverage(tags, oracle_codec.encode_batch(data, in_off, 1024)[1], need_align=False)
    check(torch_cuda, oracle_codec, strings, label="past the stage", mean=(40, 48))


@pytest.mark.parametrize("route", ["explicit", "packed"])
@pytest.mark.parametrize("lo,hi,mean", [(24, 72, (44, 52)), (60, 110, (80, 90))])
def test_staged_kernels(torch_cuda, oracle_codec, route, lo, hi, mean):
    """encode_staged_kernel, 16 waves (mean <= 52) and 8 waves (53..120): slots through in_len / out_off, and the
    packed entry point"""
    strings, tags = rare_batch(np.random.default_rng(240 + lo), 600, 1, lo, hi)
    data, in_off = layout(strings, 1)
    coverage(tags, oracle_codec.encode_batch(data, in_off, 600)[1])
    check(torch_cuda, oracle_codec, strings, off0=1, label="staged", mean=mean, route=route)


def test_proportional_lanes_unchanged(torch_cuda, oracle_codec):
    """a contiguous batch of mean >= 53: encode_pl_kernel, which places long codes on the spot as before"""
    strings, tags = rare_batch(np.random.default_rng(250), 600, 2, 40, 72)
    data, in_off = layout(strings, 2)
    coverage(tags, oracle_codec.encode_batch(data, in_off, 600)[1])
    check(torch_cuda, oracle_codec, strings, off0=2, label="lanes", mean=(53, 60))


def test_flatten_unchanged(torch_cuda, oracle_codec):
    """flatten_batch with prefix 7 (flatten_pl_kernel) on the same kind of batch: every framed literal equal"""
    from h2o_amd import codec

    strings, tags = rare_batch(np.random.default_rng(260), 600, 0, 24, 72)
    data, in_off = layout(strings)
    coverage(tags, oracle_codec.encode_batch(data, in_off, 600)[1])
    r_out, r_len = oracle_codec.flatten_batch(data, in_off, 600, 7)
    pos = slot_positions(in_off[:-1].astype(np.int64) + 11 * np.arange(600), r_len)
    out, g_len = codec.flatten_batch(torch_cuda.from_numpy(data).cuda(), torch_cuda.from_numpy(in_off.view(np.int32)).cuda(),
                                     600, 7, in_size=int(in_off[-1]))
    torch_cuda.cuda.synchronize()
    assert np.array_equal(g_len.cpu().numpy().view(np.uint32)[:600], r_len)
    assert np.array_equal(out.cpu().numpy()[pos], r_out[pos])
