"""The trimmed sorted encoder's moved span commit and the staged decoder's instantiation for the contiguous layout.

Encoder (five::encode_sorted_kernel): a chunk's input span is loaded behind barrier 3 of the chunk before and
committed to the input stage in front of its own barrier 2; the first chunk of a workgroup and a chunk that follows
one past the stage load theirs in place.  The cases walk those paths: chunk edges, several trips a workgroup with a
short last chunk, chunks past the stage alternating with fitting ones in both orders, and buffers that end on the
batch's last byte (the commit's bounded tail load).

Decoder (decode_staged_kernel<16, 3072, 4608, false, true>): contiguous batches without `in_len` take it, the same
strings as (offset, length) pairs take the general instantiation; both must give the oracle's bytes, lengths and
statuses.

Every call runs on `in`, `out`, `out_len` and `status` of exactly the documented size between sentinel guards and is
compared bit for bit with the CPU oracle: out_len, status, every byte inside a kept string's slot, and the guards."""
import numpy as np
import pytest

import bounds_harness as H

pytestmark = pytest.mark.gpu

FAIL = 0xFFFFFFFF
ALPHABET = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789-_./:=;, ", np.uint8)
SENT = 0xA5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def plain_strings(rng, lens, fail_frac=0.02):
    """header-alphabet text of the given lengths, a few strings of arbitrary bytes among them (they do not compress)"""
    lens = np.asarray(lens, np.int64)
    off = np.zeros(lens.size + 1, np.int64)
    off[1:] = np.cumsum(lens)
    data = ALPHABET[rng.integers(0, ALPHABET.size, int(off[-1]))]
    for i in np.nonzero(rng.random(lens.size) < fail_frac)[0]:
        data[off[i]:off[i + 1]] = rng.integers(0, 256, int(lens[i]), dtype=np.uint8)
    return data


def offsets(lens, first=0):
    off = np.zeros(len(lens) + 1, np.uint32)
    off[0] = first
    off[1:] = first + np.cumsum(np.asarray(lens, np.int64))
    return off


def slot_mask(starts, lens, size):
    """bool[size]: the bytes inside [start_i, start_i + len_i)"""
    d = np.zeros(size + 1, np.int32)
    keep = lens > 0
    np.add.at(d, starts[keep], 1)
    np.add.at(d, starts[keep] + lens[keep], -1)
    return np.cumsum(d[:size]) > 0


def dev_u32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def run_encode(torch, oracle, data, off, n, what):
    """encode strings [off[i], off[i + 1]) of `data` (data[:off[0]] is padding): in_size = off[n], `out` of in_size bytes"""
    from h2o_amd import codec

    in_size = int(off[n])
    assert data.size == in_size
    assert codec.lib().hhuff_debug_encode_blocks_per_cu(in_size, n) > 0, what + ": not the sorted encoder's batch"
    win, din = H.guarded(torch, in_size, SENT)
    din.copy_(torch.from_numpy(data))
    wout, dout = H.guarded(torch, in_size, SENT)
    wlen, dlen = H.guarded(torch, 4 * n, SENT)
    wst, dst = H.guarded(torch, n, SENT)
    codec.encode_batch(din, dev_u32(torch, off), n, out=dout, out_len=dlen.view(torch.int32), status=dst, in_size=in_size)
    torch.cuda.synchronize()
    ref_out, ref_len, ref_st = oracle.encode_batch(data, off, n, out_size=in_size, nthreads=8)
    got_len = dlen.cpu().numpy().view(np.uint32)
    bad = np.nonzero(got_len != ref_len)[0]
    assert bad.size == 0, "%s: out_len differs at string %d (%d strings)" % (what, bad[0], bad.size)
    assert (dst.cpu().numpy() == ref_st).all(), what + ": status differs"
    ok = ref_len != FAIL
    m = slot_mask(off[:n].astype(np.int64)[ok], ref_len[ok].astype(np.int64), in_size)
    got = dout.cpu().numpy()
    bad = np.nonzero((got != ref_out[:in_size]) & m)[0]
    assert bad.size == 0, "%s: encoded byte %d differs (%d bytes)" % (what, bad[0], bad.size)
    for name, whole, inner in (("out", wout, dout), ("out_len", wlen, dlen), ("status", wst, dst), ("in", win, din)):
        w = whole.cpu().numpy()
        g = (w.size - inner.numel()) // 2
        assert (w[:g] == SENT).all() and (w[w.size - g:] == SENT).all(), "%s: the guards of `%s` changed" % (what, name)
    return int(ok.sum())


def resident_workgroups(torch, in_size, n):
    from h2o_amd import codec

    per_cu = codec.lib().hhuff_debug_encode_blocks_per_cu(in_size, n)
    assert per_cu > 0
    return per_cu * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("n", [1, 255, 256, 257, 511, 513])
def test_encode_chunk_edges(torch_cuda, oracle_codec, n):
    rng = np.random.default_rng(1000 + n)
    for first in (0, 7):
        lens = rng.integers(16, 65, n)
        lens[rng.random(n) < 0.05] = 0
        lens[0] = 33
        off = offsets(lens, first)
        data = np.concatenate([np.full(first, SENT, np.uint8), plain_strings(rng, lens)])
        kept = run_encode(torch_cuda, oracle_codec, data, off, n, "n=%d first=%d" % (n, first))
        assert kept > 0


def test_encode_several_trips(torch_cuda, oracle_codec):
    """every workgroup takes at least two chunks, and a one-string last chunk is prepared behind a full one"""
    rng = np.random.default_rng(7)
    n = 2 * resident_workgroups(torch_cuda, 24 * 1024, 1024) * 256 + 1
    lens = rng.integers(16, 33, n)
    off = offsets(lens)
    assert resident_workgroups(torch_cuda, int(off[n]), n) * 256 * 2 < n
    kept = run_encode(torch_cuda, oracle_codec, plain_strings(rng, lens, 0.01), off, n, "several trips")
    assert kept > n // 2


def test_encode_chunks_past_the_stage_alternate(torch_cuda, oracle_codec):
    """four trips a workgroup; chunks of 56-B strings (a 14,336-B span, past the 13,312-B stage) among chunks of 8-B
    strings: workgroup 0 meets past, fitting, past, fitting, workgroup 1 the other order, workgroup 2 past, past,
    fitting, fitting, workgroup 3 fitting, fitting, past, past; the last chunk is short"""
    rng = np.random.default_rng(8)
    G = resident_workgroups(torch_cuda, 24 * 1024, 1024)
    nch = 4 * G
    n = nch * 256 - 100
    past = np.zeros(nch, bool)
    for w, trips in ((0, (0, 2)), (1, (1, 3)), (2, (0, 1)), (3, (2, 3)), (G - 1, (0, 3))):
        for k in trips:
            past[w + k * G] = True
    lens = np.where(np.repeat(past, 256)[:n], 56, 8)
    lens[rng.random(n) < 0.01] = 0
    off = offsets(lens)
    assert int(off[n]) // n <= 48, "the batch's mean must keep the small stage"
    assert resident_workgroups(torch_cuda, int(off[n]), n) == G
    kept = run_encode(torch_cuda, oracle_codec, plain_strings(rng, lens, 0.01), off, n, "chunks past the stage")
    assert kept > n // 2


@pytest.mark.parametrize("tail", [1, 5, 15, 16, 17])
def test_encode_exact_buffers(torch_cuda, oracle_codec, tail):
    """the batch ends `tail` bytes into its last 16-B chunk, in its first chunk (n = 200) and in its second (n = 300):
    the commit's last load is the bounded one"""
    rng = np.random.default_rng(50 + tail)
    for n in (200, 300):
        lens = rng.integers(24, 49, n)
        lens[n - 1] += (tail - int(lens.sum())) % 16
        off = offsets(lens)
        assert int(off[n]) % 16 == tail % 16
        run_encode(torch_cuda, oracle_codec, plain_strings(rng, lens), off, n, "n=%d tail=%d" % (n, tail))


# ---- the staged decoder's lean instantiation ----

def gather(buf, starts, lens):
    """the bytes [starts_i, starts_i + lens_i) of buf, back to back"""
    lens = np.asarray(lens, np.int64)
    first = np.cumsum(lens) - lens
    return buf[np.repeat(np.asarray(starts, np.int64) - first, lens) + np.arange(int(lens.sum()))]


def huffman_strings(oracle, rng, plain_lens, lo=0, hi=1 << 30, corrupt_frac=0.03):
    """the Huffman codings of header text of the given plain lengths whose coded length lies in [lo, hi], some of
    them overwritten with arbitrary bytes (failures and soft errors); plain length 0 gives an empty string
    -> (bytes back to back, lengths)"""
    plain_lens = np.asarray(plain_lens, np.int64)
    off = offsets(plain_lens)
    text = plain_strings(rng, plain_lens, 0.0)
    out, olen, _ = oracle.encode_batch(text, off, plain_lens.size, nthreads=8)
    olen = np.where(plain_lens == 0, 0, olen).astype(np.int64)
    keep = (olen != FAIL) & (((olen >= lo) & (olen <= hi)) | (plain_lens == 0))
    lens = olen[keep]
    data = gather(out, off[:-1][keep], lens)
    hoff = offsets(lens)
    for i in np.nonzero((rng.random(lens.size) < corrupt_frac) & (lens > 0))[0]:
        data[hoff[i]:hoff[i + 1]] = rng.integers(0, 256, int(lens[i]), dtype=np.uint8)
    return data, lens


def run_decode(torch, oracle, data, off, n, names, what, pairs=False):
    """decode Huffman strings [off[i], off[i + 1]) on exact buffers, as a contiguous batch (the lean instantiation) or
    as (offset, length) pairs; -> (out_len, status, the kept strings' bytes back to back), checked against the oracle"""
    from h2o_amd import codec

    in_size = int(off[n])
    assert data.size == in_size and in_size // n <= 40, what + ": not the short staged decoder's batch"
    lens = (off[1:n + 1] - off[:n]).astype(np.uint32)
    win, din = H.guarded(torch, in_size, SENT)
    din.copy_(torch.from_numpy(data))
    out_size = (8 * in_size) // 5
    wout, dout = H.guarded(torch, out_size, SENT)
    wlen, dlen = H.guarded(torch, 4 * n, SENT)
    wst, dst = H.guarded(torch, n, SENT)
    kw = dict(in_len=dev_u32(torch, lens), in_off=dev_u32(torch, off[:n])) if pairs else dict(in_off=dev_u32(torch, off))
    codec.decode_batch(din, kw.pop("in_off"), n, is_name_bits=None if names is None else dev_u32(torch, names), out=dout,
                       out_len=dlen.view(torch.int32), status=dst, in_size=in_size, **kw)
    torch.cuda.synchronize()
    ref_out, ref_len, ref_st = oracle.decode_batch(data, off, n, is_name_bits=names, out_size=max(out_size, 1), nthreads=8)
    got_len, got_st, got = dlen.cpu().numpy().view(np.uint32), dst.cpu().numpy(), dout.cpu().numpy()
    bad = np.nonzero(got_len != ref_len)[0]
    assert bad.size == 0, "%s: out_len differs at string %d (%d strings)" % (what, bad[0], bad.size)
    bad = np.nonzero(got_st != ref_st)[0]
    assert bad.size == 0, "%s: status differs at string %d (%d strings)" % (what, bad[0], bad.size)
    ok = ref_len != FAIL
    starts = (8 * off[:n].astype(np.int64)) // 5
    m = slot_mask(starts[ok], ref_len[ok].astype(np.int64), out_size)
    bad = np.nonzero((got != ref_out[:out_size]) & m)[0]
    assert bad.size == 0, "%s: decoded byte %d differs (%d bytes)" % (what, bad[0], bad.size)
    for name, whole, inner in (("out", wout, dout), ("out_len", wlen, dlen), ("status", wst, dst), ("in", win, din)):
        w = whole.cpu().numpy()
        g = (w.size - inner.numel()) // 2
        assert (w[:g] == SENT).all() and (w[w.size - g:] == SENT).all(), "%s: the guards of `%s` changed" % (what, name)
    return got_len, got_st, got[m]


def name_words(rng, n):
    return rng.integers(0, 1 << 32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32)


@pytest.fixture(scope="module")
def short_huffman(oracle_codec):
    """300 Huffman strings of up to 39 bytes, several empty, some corrupted"""
    rng = np.random.default_rng(21)
    plain = rng.integers(1, 52, 340)
    plain[rng.random(plain.size) < 0.06] = 0
    data, lens = huffman_strings(oracle_codec, rng, plain, 0, 39, 0.08)
    assert lens.size >= 300
    return data, lens


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_decode_tile_edges_and_instantiation_parity(torch_cuda, oracle_codec, short_huffman, n):
    """the first n strings as a contiguous batch (lean) and as pairs (general), with and without name flags: both
    equal the oracle, hence each other; compared directly as well"""
    from h2o_amd import codec

    data, lens = short_huffman
    off = offsets(lens[:n])
    d = data[:int(off[n])]
    if d.size == 0:
        pytest.fail("the first string must not be empty")
    for names in (None, name_words(np.random.default_rng(n), n)):
        tag = "n=%d names=%s" % (n, names is not None)
        lean = run_decode(torch_cuda, oracle_codec, d, off, n, names, tag + " contiguous")
        gen = run_decode(torch_cuda, oracle_codec, d, off, n, names, tag + " pairs", pairs=True)
        prev = codec.set_edge_defer_min(0)  # the general instantiation again, with deferred edges
        try:
            dfr = run_decode(torch_cuda, oracle_codec, d, off, n, names, tag + " deferred edges")
        finally:
            codec.set_edge_defer_min(prev)
        for other in (gen, dfr):
            assert all((a == b).all() for a, b in zip(lean, other)), tag + ": the instantiations differ"


def test_decode_two_trips_a_wave(torch_cuda, oracle_codec):
    """n = 2 x 256 workgroups x 16 waves x 64 strings + 1 on 18..30-B Huffman strings: every wave of a full grid
    decodes two tiles, and one wave a third of one string"""
    rng = np.random.default_rng(22)
    n = 2 * 256 * 16 * 64 + 1
    data, lens = huffman_strings(oracle_codec, rng, rng.integers(24, 41, n + n // 4), 18, 30, 0.01)
    assert lens.size >= n
    off = offsets(lens[:n])
    run_decode(torch_cuda, oracle_codec, data[:int(off[n])], off, n, name_words(rng, n), "two trips a wave")


@pytest.mark.parametrize("with_names", [False, True])
def test_decode_input_edges(torch_cuda, oracle_codec, with_names):
    """five tiles of about 20-B strings with tile 2 past the 3,072-B input stage (64 strings of about 58 B), tile 1
    and tile 3 with an empty string at their first and last lanes, tile 4 short"""
    rng = np.random.default_rng(23)
    plain = rng.integers(20, 33, 5 * 64 - 10)
    plain[128:192] = rng.integers(76, 84, 64)
    plain[[64, 127, 192, 255]] = 0
    data, lens = huffman_strings(oracle_codec, rng, plain, 0, 1 << 30, 0.04)
    n = lens.size
    assert n == plain.size and (lens[[64, 127, 192, 255]] == 0).all()
    off = offsets(lens)
    assert int(off[192] - off[128]) > 3072 and int(off[128] - off[64]) + 15 <= 3072
    names = name_words(rng, n) if with_names else None
    lean = run_decode(torch_cuda, oracle_codec, data, off, n, names, "input edges")
    gen = run_decode(torch_cuda, oracle_codec, data, off, n, names, "input edges, pairs", pairs=True)
    assert all((a == b).all() for a, b in zip(lean, gen)), "the instantiations differ"
