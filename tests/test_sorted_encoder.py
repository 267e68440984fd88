"""The length-sorted encoder's two stage sizes (five::encode_sorted_kernel: 13,312 B at five workgroups a CU for batches
with a mean string of at most 48 B; encode_sorted_kernel: 16,384 B at four for means 49..52) against the oracle: chunk
edges, a chunk at and past the stage, the host's choice between the two, the packed string records, the 257-entry code
table, residency.

Every case compares out_len, status and the bytes inside each kept slot with oracle.oracle().encode_batch (slot tails
and the slots of failing strings are unspecified), with the chunks' shared 16-B edges stored in the kernel and
deferred to the fix-up kernel."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAIL = 0xFFFFFFFF
STAGE = 13312  # the small stage; a chunk is 256 strings


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def header_strings(rng, lens):
    """compressible strings (printable ASCII) of the given lengths"""
    return [rng.integers(0x20, 0x7F, int(L)).astype(np.uint8) for L in lens]


def place(strings, off0=0, fill=0xFF):
    """the contiguous layout: string 0 at byte off0, `fill` before it and in 48 bytes behind the last one"""
    lens = np.array([len(s) for s in strings], np.int64)
    in_off = np.empty(len(strings) + 1, np.uint32)
    in_off[0] = off0
    in_off[1:] = off0 + np.cumsum(lens)
    data = np.full(int(in_off[-1]) + 48, fill, np.uint8)
    if lens.sum():
        data[off0:int(in_off[-1])] = np.concatenate([s for s in strings if len(s)])
    return data, in_off


def mean_of(in_off):
    return int(in_off[-1]) // (len(in_off) - 1)


def check(torch, oracle, strings, off0=0, fill=0xFF, label="", mean=None):
    from h2o_amd import codec

    data, in_off = place(strings, off0, fill)
    n = len(strings)
    in_size = int(in_off[-1])
    if mean is not None:
        assert in_size // n == mean, (label, in_size // n)
    assert in_size // n <= 52, label  # the sorted encoder's batches
    r_out, r_len, r_st = oracle.encode_batch(data, in_off, n)
    kept = r_len != FAIL
    lens = r_len[kept].astype(np.int64)
    starts = in_off[:-1][kept].astype(np.int64)
    pos = np.repeat(starts - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()))
    d_data = torch.from_numpy(data).cuda()
    d_off = torch.from_numpy(in_off.view(np.int32)).cuda()
    for defer in (0xFFFFFFFF, 0):
        prev = codec.set_edge_defer_min(defer)
        try:
            out = torch.full((in_size + 16,), 0xA5, dtype=torch.uint8, device="cuda")
            _, g_len, g_st = codec.encode_batch(d_data, d_off, n, out=out, in_size=in_size)
            torch.cuda.synchronize()
        finally:
            codec.set_edge_defer_min(prev)
        g_len = g_len.cpu().numpy().view(np.uint32)[:n]
        g_st = g_st.cpu().numpy()[:n]
        g_out = out.cpu().numpy()
        what = "%s off0=%d fill=%#x defer=%#x" % (label, off0, fill, defer)
        bad = np.nonzero(g_len != r_len)[0]
        assert bad.size == 0, (what, "out_len", bad[:8], g_len[bad[:8]], r_len[bad[:8]])
        bad = np.nonzero(g_st != r_st)[0]
        assert bad.size == 0, (what, "status", bad[:8], g_st[bad[:8]], r_st[bad[:8]])
        bad = np.nonzero(g_out[pos] != r_out[pos])[0]
        if bad.size:
            i = int(np.searchsorted(starts, pos[bad[0]], side="right") - 1)
            assert False, (what, "bytes", "kept string", i, "byte", int(pos[bad[0]] - starts[i]))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_chunk_edges(torch_cuda, oracle_codec, n):
    rng = np.random.default_rng(n)
    check(torch_cuda, oracle_codec, header_strings(rng, rng.integers(24, 73, n)), label="n=%d" % n)


def at_stage_strings():
    rng = np.random.default_rng(7)
    return header_strings(rng, [52] * 256 + [40] * 256)


@pytest.mark.parametrize("off0", [0, 1])
def test_chunk_at_and_past_the_stage(torch_cuda, oracle_codec, off0):
    """256 x 52 B = 13,312 B: from byte 0 the first chunk's 16-B aligned span fills the small stage exactly; from byte
    1 it is 13,328 B and the chunk goes to the per-thread path (the second chunk, 10,240 B, is staged either way)"""
    assert 256 * 52 == STAGE
    check(torch_cuda, oracle_codec, at_stage_strings(), off0=off0, label="at stage", mean=46)


@pytest.mark.parametrize("off0", [0, 1])
@pytest.mark.parametrize("tail,mean", [(1100, 48), (1600, 49)])
def test_host_selection(torch_cuda, oracle_codec, off0, tail, mean):
    """the same strings and one trailing string: mean 48 takes the small stage, mean 49 the large one"""
    rng = np.random.default_rng(8)
    check(torch_cuda, oracle_codec, at_stage_strings() + header_strings(rng, [tail]), off0=off0,
          label="mean %d" % mean, mean=mean)


def test_empty_strings(torch_cuda, oracle_codec):
    """empty strings inside chunks, at a chunk's end (offset = the span's end), a whole chunk of them (span 0) and
    as the batch's last strings"""
    rng = np.random.default_rng(9)
    lens = rng.integers(24, 73, 700)
    lens[::3] = 0
    lens[250:256] = 0
    lens[256:512] = 0
    lens[-5:] = 0
    for off0 in (0, 5):
        check(torch_cuda, oracle_codec, header_strings(rng, lens), off0=off0, label="empty strings")


def test_incompressible_run(torch_cuda, oracle_codec):
    """strings of bytes 0x80..0xFF (codes of 20 bits and more: they fail, and stop being placed at their limit) between
    compressible neighbours, whose slots they must not touch"""
    rng = np.random.default_rng(10)
    strings = header_strings(rng, rng.integers(24, 73, 600))
    for i in list(range(100, 107)) + [255, 256, 300, 599]:
        strings[i] = rng.integers(0x80, 0x100, len(strings[i])).astype(np.uint8)
    for off0 in (0, 3):
        check(torch_cuda, oracle_codec, strings, off0=off0, label="incompressible run")


@pytest.mark.parametrize("long_len,lo,hi,small", [(13400, 24, 41, True), (17000, 26, 42, False)])
def test_string_longer_than_the_stage(torch_cuda, oracle_codec, long_len, lo, hi, small):
    """one string longer than the stage inside a chunk, which is then encoded a string a thread: 13,400 B in a batch
    of mean <= 48 (the small stage), 17,000 B in one of mean 49..52 (the large stage)"""
    rng = np.random.default_rng(long_len)
    lens = rng.integers(lo, hi, 1024)
    lens[300] = long_len
    strings = header_strings(rng, lens)
    assert (mean_of(place(strings)[1]) <= 48) == small
    check(torch_cuda, oracle_codec, strings, label="long string %d" % long_len)


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_start_and_end_alignments(torch_cuda, oracle_codec, fill):
    """strings at all 16 combinations of start and end alignment mod 4 (the head and tail words' masked lookups go
    to table entry 256), the input's unused bytes 0xFF and 0x00"""
    walk = [0, 0, 1, 0, 2, 0, 3, 1, 1, 2, 1, 3, 2, 2, 3, 3, 0]  # every ordered pair of residues mod 4 once
    rng = np.random.default_rng(11)
    for off0 in (0, 16):
        lens = [(walk[i + 1] - walk[i]) % 4 + 4 * int(rng.integers(6, 18)) for i in range(16)]
        strings = header_strings(rng, lens)
        _, in_off = place(strings, off0)
        assert len({(int(in_off[i]) % 4, int(in_off[i + 1]) % 4) for i in range(16)}) == 16
        check(torch_cuda, oracle_codec, strings, off0=off0, fill=fill, label="alignments")
    # the same inside longer chunks, where the neighbours' bytes lie beside the masks
    lens = rng.integers(24, 73, 520)
    strings = header_strings(rng, lens)
    _, in_off = place(strings, 2)
    assert len({(int(in_off[i]) % 4, int(in_off[i + 1]) % 4) for i in range(520)}) == 16
    check(torch_cuda, oracle_codec, strings, off0=2, fill=fill, label="alignments in chunks")


def test_residency(torch_cuda):
    """the workgroups a CU of the kernel that launch_encode picks: five with the small stage, four with the large"""
    from h2o_amd import codec

    q = codec.lib().hhuff_debug_encode_blocks_per_cu
    q.restype = ctypes.c_int
    q.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    torch_cuda.cuda.set_device(0)
    assert q(47 * 65536, 65536) == 5
    assert q(50 * 65536, 65536) == 4
