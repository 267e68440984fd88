"""The host-array batch paths on the GPU: hhuff_{de,en}code_batch_host, _host_pipelined, _host_packed and the host
mode of hhuff_{de,en}code_batch_multi, through the C ABI (codec.lib()), on the hand-built batches of
tests/host_paths_corpora.py -- chunk cuts, staging-slot reuse, offsets and residues, lengths at the split
thresholds, every kernel family in flight at once, failing strings and name flags at the seams, the packed path's
64 MiB staging boundary.

Every call gets `out`, `out_len` and `status` of exactly the documented size between sentinel guards, the input's
unused bytes hold a fill pattern, and every case runs under both bounds_harness.RUNS pairs; the result must equal
the oracle's (bounds_harness.check).  On the slot-layout paths every byte of `out` inside the batch's slot range
may change and no other; on the packed paths only the tiles' runs may.  Pinned buffers are interior views of one
pin_memory tensor (bounds_harness.Arena), so their guards are pinned too.

Each test loops over its cases and names the failing one in the assertion message."""
import ctypes
import threading

import numpy as np
import pytest

import bounds_harness as H
import host_paths_corpora as C
import host_paths_model as M

pytestmark = pytest.mark.gpu

PIPELINED_KINDS = ["pageable", "pinned_bytes", "zero_copy", "pinned_dma"] + ["pinned_off%d" % k for k in range(1, 16)]
B = M.PACKED_CHUNK


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def corpus():
    return C.corpus()


@pytest.fixture(scope="module")
def arena(torch_cuda):
    t = torch_cuda.empty(8 << 20, dtype=torch_cuda.uint8, pin_memory=True)
    a = H.Arena(t.numpy())
    a.keep = t
    return a


_cache = {}


def expect(oracle, c, r, exact=True, with_status=True):
    """(arrays, exp, mask, starts) of case c under RUNS[r], computed once and shared by every test (read only)"""
    key = (c.label, r, exact, with_status)
    if key not in _cache:
        fill, sentinel = H.RUNS[r]
        a = c.arrays(fill, sentinel, exact=exact, with_status=with_status)
        _cache[key] = (a,) + C.expected(oracle, c, a)
    return _cache[key]


def packed_expect(oracle, c, r):
    key = (c.label, r, "packed")
    if key not in _cache:
        a, slots, _, _ = expect(oracle, c, r)
        _cache[key] = M.packed_from_slots(c.op, a["in_off"], c.n, slots)
    return _cache[key]


# ------------------------------------------------------------------------------------------------
# buffers of every memory kind, and the calls
# ------------------------------------------------------------------------------------------------
def _addr(whole):
    return ctypes.c_void_p(whole.ctypes.data + H.GUARD)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def buffers(kind, arena, a, want):
    """the caller's arrays of one call: -> (in pointer, in_off, names, result buffers name -> whole).
    pageable: numpy; pinned_bytes: `in` and `out` pinned, the metadata pageable; zero_copy / pinned_dma / pinned:
    everything pinned and aligned; pinned_offK: everything pinned, `in` and `out` K bytes off a multiple of 16"""
    size = {"out": a["out_size"], "out_len": 4 * a["n"], "status": a["n"], "out_off": 4 * (a["n"] + 1)}
    s = a["sentinel"]
    if kind == "pageable":
        return _p(a["data"]), a["in_off"], a["names"], {k: H.guarded(np, size[k], s)[0] for k in want}
    arena.reset()
    k = int(kind[10:]) if kind.startswith("pinned_off") else 0
    data = _addr(arena.copy(a["whole"], k)[0])
    res = {"out": arena.guarded(size["out"], s, k)[0]}
    if kind == "pinned_bytes":
        res.update({n: H.guarded(np, size[n], s)[0] for n in want if n != "out"})
        return data, a["in_off"], a["names"], res
    res.update({n: arena.guarded(size[n], s)[0] for n in want if n != "out"})

    def pin(x):
        if x is None:
            return None
        v = arena.guarded(4 * x.size, 0)[1].view(np.uint32)
        v[:] = x
        return v

    return data, pin(a["in_off"]), pin(a["names"]), res


def call_pipelined(c, a, data, off, names, res, chunk_bytes):
    from h2o_amd import codec

    L = codec.lib()
    st = _addr(res["status"]) if "status" in res else None
    if c.op == "decode":
        rc = L.hhuff_decode_batch_host_pipelined(data, a["in_size"], _p(off), c.n, _p(names), _addr(res["out"]),
                                                 a["out_size"], _addr(res["out_len"]), st, 0, chunk_bytes)
    else:
        rc = L.hhuff_encode_batch_host_pipelined(data, a["in_size"], _p(off), c.n, _addr(res["out"]), a["out_size"],
                                                 _addr(res["out_len"]), st, 0, chunk_bytes)
    assert rc == 0, (c.label, L.hhuff_last_error_string())


class edge_defer:
    """hhuff_set_edge_defer_min for a block (None: left alone), restored afterwards"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from h2o_amd import codec

        self.prev = None if self.value is None else codec.set_edge_defer_min(self.value)

    def __exit__(self, *exc):
        from h2o_amd import codec

        if self.value is not None:
            codec.set_edge_defer_min(self.prev)


def run_pipelined(oracle, arena, c, r, kind, exact=True, with_status=True):
    a, exp, mask, starts = expect(oracle, c, r, exact, with_status)
    data, off, names, res = buffers(kind, arena, a, ["out", "out_len"] + (["status"] if with_status else []))
    with edge_defer(c.defer):
        call_pipelined(c, a, data, off, names, res, c.chunk_bytes)
    H.check(res, exp, mask, a["sentinel"], starts=starts,
            label="%s %s fill=%#x out_size=%d%s" % (c.label, kind, H.RUNS[r][0], a["out_size"],
                                                    "" if with_status else " status=NULL"))


# ------------------------------------------------------------------------------------------------
# the pipelined calls
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", PIPELINED_KINDS)
def test_pipelined(torch_cuda, oracle_codec, corpus, arena, kind, monkeypatch):
    """every corpus case, both runs, `out` of exactly slot_of(in_off[n]) bytes -- and, where poisoned bytes follow
    the last string, of include/hhuff.h's floor(8 in_size / 5) | in_size as well -- under one memory kind.
    zero_copy: everything pinned and aligned, one launch on host memory; pinned_dma: the same arrays with
    HHUFF_HOST_COPY=1, the chunked pipeline DMAing in place; pinned_offK: misaligned byte buffers, chunked too"""
    if kind == "pinned_dma":
        monkeypatch.setenv("HHUFF_HOST_COPY", "1")
    ran = 0
    for c in corpus:
        for r in range(len(H.RUNS)):
            run_pipelined(oracle_codec, arena, c, r, kind)
            ran += 1
        if c.tail:
            run_pipelined(oracle_codec, arena, c, 1, kind, exact=False)
            ran += 1
    assert ran == 2 * len(corpus) + sum(1 for c in corpus if c.tail)


@pytest.mark.parametrize("kind", ["pageable", "zero_copy", "pinned_dma"])
def test_pipelined_encode_without_status(torch_cuda, oracle_codec, corpus, arena, kind, monkeypatch):
    if kind == "pinned_dma":
        monkeypatch.setenv("HHUFF_HOST_COPY", "1")
    for c in corpus:
        if c.op == "encode":
            for r in range(len(H.RUNS)):
                run_pipelined(oracle_codec, arena, c, r, kind, with_status=False)


def _by_label(corpus, label):
    (c,) = [c for c in corpus if c.label == label]
    return c


def _in_thread(f):
    """run f on a fresh thread (its own staging slots, stream and scratch) and re-raise what it raised"""
    err = []

    def body():
        try:
            f()
        except BaseException as e:  # noqa: B902
            err.append(e)

    t = threading.Thread(target=body)
    t.start()
    t.join()
    if err:
        raise err[0]


def test_staging_reuse_across_calls(torch_cuda, oracle_codec, corpus, arena):
    """one thread's three staging slots over a sequence of calls: a large call (they grow), a small one (reused as
    they are), then three chunks of 64 KB (every slot regrows), decode and encode alternating, each against the
    oracle under both sentinels.  On a fresh thread, so that the slots start empty whatever ran before"""
    rng = np.random.default_rng(21)
    big = {op: C.Case("regrow", op, C.strings_of(op, rng, [2000] * 96), "three chunks of 32 x 2000 B",
                      lambda c, p, e: [x.m for x in p] == [32, 32, 32], chunk_bytes=60000, in_off0=11)
           for op in ("decode", "encode")}
    for c in big.values():
        assert c.holds(c, c.plan(), None)
    seq = ["a 4097-B string, chunk mean >= 128", "n=1 chunk_bytes=1", None, "n=225 chunk_bytes=1", "in_off0=81 n=33", None]

    def body():
        for r in range(len(H.RUNS)):
            for k, label in enumerate(seq):
                for op in (("decode", "encode"), ("encode", "decode"))[k % 2]:
                    c = big[op] if label is None else _by_label(corpus, "%s %s" % (op, label))
                    run_pipelined(oracle_codec, arena, c, r, "pageable")

    _in_thread(body)


def test_pipelined_from_four_threads(torch_cuda, oracle_codec, corpus):
    """the worker-thread use the library documents: four threads, each three pipelined calls on its own arrays with
    different chunk_bytes, concurrently; every result equals the oracle's"""
    labels = ["decode n=225 chunk_bytes=1", "encode n=193 chunk_bytes=1", "decode failing strings at the seams",
              "encode in_off0=81 n=97"]
    jobs = []
    for t, label in enumerate(labels):
        c = _by_label(corpus, label)
        for k, cb in enumerate((1, 700, C.HUGE)):
            a, exp, mask, starts = expect(oracle_codec, c, (t + k) % 2)
            data, off, names, res = buffers("pageable", None, a, ["out", "out_len", "status"])
            jobs.append((t, c, a, data, off, names, res, cb, exp, mask, starts))
    start = threading.Barrier(len(labels))
    err = []

    def body(t):
        try:
            start.wait()
            for j in jobs:
                if j[0] == t:
                    call_pipelined(j[1], j[2], j[3], j[4], j[5], j[6], j[7])
        except BaseException as e:  # noqa: B902
            err.append(e)

    threads = [threading.Thread(target=body, args=(t,)) for t in range(len(labels))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not err, err
    for t, c, a, _, _, _, res, cb, exp, mask, starts in jobs:
        H.check(res, exp, mask, a["sentinel"], starts=starts, label="thread %d %s chunk_bytes=%d" % (t, c.label, cb))


# ------------------------------------------------------------------------------------------------
# large buffers: the batch's strings moved far into a buffer, checked through a window
# ------------------------------------------------------------------------------------------------
def moved(a, delta, in_size=None):
    """place_input()'s arrays with every offset moved up by delta (a multiple of 80: every slot moves by
    slot_of(delta)), the bytes in front filled: -> (guarded input buffer, its data pointer, in_off, in_size)"""
    assert delta % 80 == 0
    fill = int(a["whole"][0])
    in_size = a["in_size"] + delta if in_size is None else in_size
    whole, data = H.guarded(np, in_size, fill)
    data[delta:delta + a["in_size"]] = a["data"]
    off = (a["in_off"].astype(np.uint64) + delta).astype(np.uint32)
    return whole, data, off, in_size


def window(whole, shift, untouched, sentinel, label):
    """the guarded buffer of `out` bytes [shift, end): where the call leaves the bytes in front alone they must
    all hold the sentinel still, and the last of them serve as the window's guard"""
    if untouched:
        assert (whole[:H.GUARD + shift] == sentinel).all(), label + ": a byte in front of the batch's slots written"
        return whole[shift:]
    return np.concatenate([whole[:H.GUARD], whole[H.GUARD + shift:]])


@pytest.mark.parametrize("where", ["start", "end"])
@pytest.mark.parametrize("in_size", [M.ROUTE_MIN, M.ROUTE_MIN - 16])
@pytest.mark.parametrize("op", ["decode", "encode"])
def test_host_batch_routing(torch_cuda, oracle_codec, corpus, op, in_size, where):
    """hhuff_*_batch_host at in_size = 128 MiB (the chunked pipeline) and 16 bytes less (one piece), 65 strings at
    the start of the buffer and at its end, once each run.  One piece: the whole of `out` comes back (any byte
    may change); pipeline: only the batch's slots"""
    from h2o_amd import codec

    L = codec.lib()
    c = _by_label(corpus, "%s in_off0=7 n=97" % op)
    c = C.Case("routing", op, c.strings[:65], "", None, flags=c.flags[:65], in_off0=7, tail=3)
    r = where == "end"
    a, exp, mask, starts = expect(oracle_codec, c, int(r), exact=False)
    delta = 0 if where == "start" else (in_size - a["in_size"]) // 80 * 80
    whole, data, off, _ = moved(a, delta, in_size)
    shift = M.slot_of(op, delta)
    pipeline = in_size >= M.ROUTE_MIN
    # at the start `out` ends with the batch's slots; at the end it has include/hhuff.h's size for in_size
    out_size = M.slot_of(op, int(off[c.n])) if where == "start" else M.slot_of(op, in_size)
    sentinel = a["sentinel"]
    res = {"out": H.guarded(np, out_size, sentinel)[0], "out_len": H.guarded(np, 4 * c.n, sentinel)[0],
           "status": H.guarded(np, c.n, sentinel)[0]}
    args = [_p(data), in_size, _p(off), None, c.n] + ([_p(a["names"])] if op == "decode" else []) + \
        [_addr(res["out"]), out_size, None, _addr(res["out_len"]), _addr(res["status"]), 0]
    rc = (L.hhuff_decode_batch_host if op == "decode" else L.hhuff_encode_batch_host)(*args)
    assert rc == 0, L.hhuff_last_error_string()
    label = "%s host in_size=%d strings at the %s" % (op, in_size, where)
    res["out"] = window(res["out"], shift, pipeline, sentinel, label)
    size = out_size - shift
    e = dict(exp, out=np.resize(exp["out"], size) if size > exp["out"].size else exp["out"][:size])
    m = np.zeros(size, bool) if pipeline else np.ones(size, bool)
    if pipeline:
        k = min(size, mask.size)
        m[:k] = mask[:k]
    H.check(res, e, m, sentinel, starts=starts, label=label)


# ------------------------------------------------------------------------------------------------
# the packed calls
# ------------------------------------------------------------------------------------------------
def call_packed(c, in_size, data, off, names, res, out_size):
    from h2o_amd import codec

    L = codec.lib()
    ooff = _addr(res["out_off"]) if "out_off" in res else None
    st = _addr(res["status"]) if "status" in res else None
    if c.op == "decode":
        rc = L.hhuff_decode_batch_host_packed(data, in_size, _p(off), c.n, _p(names), _addr(res["out"]), out_size, ooff,
                                              _addr(res["out_len"]), st, 0)
    else:
        rc = L.hhuff_encode_batch_host_packed(data, in_size, _p(off), c.n, _addr(res["out"]), out_size, ooff,
                                              _addr(res["out_len"]), st, 0)
    assert rc == 0, (c.label, L.hhuff_last_error_string())


def packed_starts(c, exp):
    from h2o_amd import codec

    return codec.packed_positions(c.off()[:c.n], exp["out_len"], c.op == "decode")


@pytest.mark.parametrize("kind", ["pageable", "pinned", "pinned_off5"])
def test_packed(torch_cuda, oracle_codec, corpus, arena, kind):
    """the corpus through hhuff_*_batch_host_packed: staged (pageable, and pinned with misaligned byte buffers) and
    zero copy (pinned, aligned), with and without out_off, an encode with and without status.  `out` has exactly
    the slot end's size, and every byte of it in no tile's run keeps the sentinel on either route"""
    for c in corpus:
        for r in range(len(H.RUNS)):
            a, _, _, _ = expect(oracle_codec, c, r)
            exp, mask = packed_expect(oracle_codec, c, r)
            for with_off, with_status in ((True, True), (False, True)) + (((True, False),) if c.op == "encode" else ()):
                want = ["out", "out_len"] + (["out_off"] if with_off else []) + (["status"] if with_status else [])
                data, off, names, res = buffers(kind, arena, a, want)
                call_packed(c, a["in_size"], data, off, names, res, a["out_size"])
                e = {k: v for k, v in exp.items() if k in want}
                H.check(res, e, mask, a["sentinel"], starts=exp["out_off"][:c.n] if with_off else packed_starts(c, exp),
                        label="packed %s %s fill=%#x out_off=%d status=%d" % (c.label, kind, H.RUNS[r][0], with_off, with_status))


@pytest.mark.parametrize("which", range(5), ids=["straddles", "ends_at", "starts_at", "empty_at", "all_behind"])
@pytest.mark.parametrize("op", ["decode", "encode"])
def test_packed_staging_boundary(torch_cuda, oracle_codec, op, which):
    """the staged route's 64 MiB chunk of the device output against the tiles' runs: the cases of
    host_paths_corpora.packed_boundary at the real boundary (pageable arrays; one 64 MiB copy each way).  The batch
    is built near zero and moved up by a multiple of 80 bytes; `out` is checked through a window at its end, and
    every byte in front of it must keep the sentinel"""
    c = C.packed_boundary(op, B)[which]
    delta = c.in_off0 // 80 * 80
    small = C.Case(c.label, op, c.strings, c.why, c.holds, flags=c.flags, in_off0=c.in_off0 - delta)
    shift = M.slot_of(op, delta)
    for r in range(len(H.RUNS)):
        fill, sentinel = H.RUNS[r]
        a, slots, _, _ = expect(oracle_codec, small, r)
        exp, mask = M.packed_from_slots(op, a["in_off"], c.n, slots)
        if r == 0:  # the edge is there: the predicate over the runs at their real positions
            real = dict(exp, out_off=(exp["out_off"].astype(np.int64) + shift))
            runs = M.packed_runs(op, c.off(), c.n, real["out_off"], real["out_len"])
            assert {0: runs[0][0] < B < runs[0][1], 1: runs[0][1] == B, 2: runs[1][0] == B < runs[1][1],
                    3: runs[1] == (B, B) and runs[2][0] > B, 4: runs[0][0] >= B}[which], (c.label, runs)
        whole, data, off, in_size = moved(a, delta)
        out_size = a["out_size"] + shift
        res = {"out": H.guarded(np, out_size, sentinel)[0], "out_off": H.guarded(np, 4 * (c.n + 1), sentinel)[0],
               "out_len": H.guarded(np, 4 * c.n, sentinel)[0], "status": H.guarded(np, c.n, sentinel)[0]}
        call_packed(c, in_size, _p(data), off, a["names"], res, out_size)
        label = "%s fill=%#x" % (c.label, fill)
        res["out"] = window(res["out"], shift, True, sentinel, label)
        e = dict(exp, out_off=(exp["out_off"].astype(np.int64) + shift).astype(np.uint32))
        H.check(res, e, mask, sentinel, starts=exp["out_off"][:c.n], label=label)


# ------------------------------------------------------------------------------------------------
# the host mode of the multi-device calls
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pageable", "pinned"])
@pytest.mark.parametrize("nshards", [1, 2, 3])
def test_multi_host_mode(torch_cuda, oracle_codec, corpus, arena, nshards, kind):
    """hhuff_*_batch_multi(src_device = HHUFF_HOST_MEMORY) with 1, 2 and 3 shards on device 0 over the cases whose
    first string lies off zero: with fewer than 64 strings all shards but the last are empty (a shard starts on
    a multiple of 64 strings), with 97 strings and three shards the last one starts at 64"""
    from h2o_amd import codec

    L = codec.lib()
    cases = [c for c in corpus if c.in_off0 != 0 and (c.n < 64 or c.group == "offsets")]
    assert sum(1 for c in cases if c.n < 64) >= 16 and sum(1 for c in cases if c.n > 64) >= 16
    dev = (ctypes.c_int * nshards)(*([0] * nshards))
    for c in cases:
        for r in range(len(H.RUNS)):
            a, exp, mask, starts = expect(oracle_codec, c, r)
            data, off, names, res = buffers(kind, arena, a, ["out", "out_len", "status"])
            head = [nshards, dev, codec.HOST_MEMORY, data, a["in_size"], _p(off), c.n]
            tail = [_addr(res["out"]), a["out_size"], _addr(res["out_len"]), _addr(res["status"]), None]
            if c.op == "decode":
                rc = L.hhuff_decode_batch_multi(*(head + [_p(names)] + tail))
            else:
                rc = L.hhuff_encode_batch_multi(*(head + tail))
            assert rc == 0, (c.label, L.hhuff_last_error_string())
            H.check(res, exp, mask, a["sentinel"], starts=starts,
                    label="multi %s %d shards %s fill=%#x" % (c.label, nshards, kind, H.RUNS[r][0]))
