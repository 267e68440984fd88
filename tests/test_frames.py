"""The HTTP/2 de-framer on the GPU (include/hhuff.h (2k), h2o_amd/csrc/hhuff_frames.hip) against the model
(frames_model.py): the hand-built corpus, fuzz-corpus files and seeded random connections, every output array
compared; exact-size guarded outputs; the gather at every pair of alignments; a connection cut at every byte and
resumed; and the closed loops encoder -> de-framer -> decoder with nothing but device arrays between the last two, which are
enqueued back to back on one stream before anything synchronises."""
import numpy as np
import pytest

import bounds_harness as BH
import frames_corpora as K
import frames_model as M
from conftest import load_golden
from h2o_amd import codec as C
from h2o_amd import hpenc_synth as HE

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
OUTPUTS = ("frames", "nframes", "consumed", "cstatus", "cerr", "blk", "blk_off", "conn_first", "blocks", "totals", "arena_off")
ARENA = (1024, 16)  # arena_fixed, arena_per_byte of these tests


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from h2o_amd import build

    build.build(verbose=False)
    return torch


def dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).cuda()


def out_bytes(nconn, frm_cap, in_size):
    return dict(frames=32 * frm_cap, nframes=4 * nconn, consumed=4 * nconn, cstatus=4 * nconn, cerr=4 * nconn, blk=in_size,
                blk_off=4 * (frm_cap + 1), conn_first=4 * (nconn + 1), blocks=32 * frm_cap, totals=8, arena_off=8 * (frm_cap + 1))


def deframe(torch, e, mfs=16384, mbb=0, flags=0, sentinel=SENTINEL, guard=False, then=None):
    """hhuff_h2_deframe on the connections of the model's batch e, every output of exactly its documented size and
    filled with the sentinel (guard: between two guard zones, which are checked): -> (numpy arrays, device tensors).
    then(r), if given, runs right behind the call -- before anything synchronises or is copied to the host -- and its
    result is kept as r["then"]."""
    nconn, frm_cap, in_size = e["in_off"].size - 1, e["frm_cap"], int(e["data"].size)
    data = dev(torch, e["data"] if in_size else np.zeros(1, np.uint8))
    kinds = dict(nframes=torch.int32, consumed=torch.int32, cstatus=torch.int32, cerr=torch.int32, blk_off=torch.int32,
                 conn_first=torch.int32, totals=torch.int32, arena_off=torch.int64)
    whole, out = {}, {}
    for k, n in out_bytes(nconn, frm_cap, in_size).items():
        if n == 0:  # (no such array: the wrapper passes a dummy)
            continue
        if guard:
            whole[k], inner = BH.guarded(torch, n, sentinel)
        else:
            inner = torch.full((n,), sentinel, dtype=torch.uint8, device="cuda")
        out[k] = inner.view(kinds[k]) if k in kinds else inner
    r = C.h2_deframe(data, dev(torch, e["in_off"]), dev(torch, e["frm_first"]), frm_cap, mfs, mbb, flags, in_size=in_size,
                     arena_fixed=ARENA[0], arena_per_byte=ARENA[1], out=out)
    if then is not None:
        r["then"] = then(r)
    torch.cuda.synchronize()
    for k, w in whole.items():
        w = w.cpu().numpy()
        n = w.size - 2 * BH.GUARD
        assert (w[:BH.GUARD] == sentinel).all() and (w[BH.GUARD + n:] == sentinel).all(), "guard of " + k
    h = {k: r[k].cpu().numpy() for k in OUTPUTS}
    return h, r


def compare(h, e, sentinel=SENTINEL):
    """every output array against the model's; what the call may not write still holds the sentinel"""
    nconn, frm_cap = e["in_off"].size - 1, e["frm_cap"]
    for k in ("nframes", "consumed", "cerr", "conn_first", "totals", "blk_off"):
        np.testing.assert_array_equal(h[k].view(np.uint32)[:e[k].size], e[k], err_msg=k)
    np.testing.assert_array_equal(h["cstatus"][:nconn], e["cstatus"], err_msg="cstatus")
    np.testing.assert_array_equal(h["arena_off"].view(np.uint64)[:frm_cap + 1], e["arena_off"], err_msg="arena_off")
    nblk, total = int(e["totals"][0]), int(e["totals"][1])
    frames = h["frames"][:32 * frm_cap].view(C.H2_FRAME_DTYPE)
    used = e["frame_used"]
    np.testing.assert_array_equal(frames[used], e["frames"][used], err_msg="frames")
    assert (h["frames"][:32 * frm_cap].reshape(-1, 32)[~used] == sentinel).all(), "a frame slot past nframes[c] was written"
    blocks = h["blocks"][:32 * frm_cap].view(C.H2_BLOCK_DTYPE)
    np.testing.assert_array_equal(blocks[:nblk], e["blocks"][:nblk], err_msg="blocks")
    assert (h["blocks"][32 * nblk:32 * frm_cap] == sentinel).all(), "a block record past nblk was written"
    np.testing.assert_array_equal(h["blk"][:total], e["blk"], err_msg="blk")
    assert (h["blk"][total:e["data"].size] == sentinel).all(), "blk written past the block bytes"


def groups(cases):
    """the corpus cases by the call's parameters: {(mfs, mbb, flags): [case]}"""
    g = {}
    for c in cases:
        g.setdefault((c["mfs"], c["mbb"], c["flags"]), []).append(c)
    return g


@pytest.fixture(scope="module")
def corpus_batches():
    """the model's batches, made once: {(params, order): batch}"""
    out = {}
    for params, cs in groups(K.CASES).items():
        for order in ("in_order", "shuffled"):
            idx = np.arange(len(cs)) if order == "in_order" else np.random.default_rng(5).permutation(len(cs))
            out[params, order] = M.batch([cs[i]["buf"] for i in idx], [cs[i]["cap"] for i in idx], *params, arena_fixed=ARENA[0],
                                         arena_per_byte=ARENA[1])
    return out


@pytest.mark.parametrize("order", ["in_order", "shuffled"])
def test_corpus(torch_cuda, corpus_batches, order):
    for (params, o), e in corpus_batches.items():
        if o == order:
            compare(deframe(torch_cuda, e, *params)[0], e)


def test_corpus_literal_expectations(torch_cuda):
    """the GPU against the corpus's own numbers, without the model in between"""
    for params, cs in groups(K.CASES).items():
        e = M.batch([c["buf"] for c in cs], [c["cap"] for c in cs], *params, arena_fixed=0)
        h, _ = deframe(torch_cuda, e, *params)
        blocks = h["blocks"].view(C.H2_BLOCK_DTYPE)
        first, off = h["conn_first"].view(np.uint32), h["blk_off"].view(np.uint32)
        for i, c in enumerate(cs):
            assert (int(h["cstatus"][i]), int(h["cerr"][i]), int(h["consumed"][i]), int(h["nframes"][i])) == \
                (c["status"], c["err"], c["consumed"], c["nframes"]), c["name"]
            got = [tuple(int(blocks[b][k]) for k in ("stream_id", "end_stream_id", "flags", "dependency", "weight",
                                                       "promised_stream_id", "nframes")) +
                   (h["blk"][int(off[b]):int(off[b + 1])].tobytes(),) for b in range(int(first[i]), int(first[i + 1]))]
            assert got == c["blocks"], c["name"]


def test_empty_connections_between_busy_ones(torch_cuda):
    e = M.batch(*K.busy_and_empty(), arena_fixed=ARENA[0], arena_per_byte=ARENA[1])
    compare(deframe(torch_cuda, e)[0], e)
    e = M.batch([b"", b"", b""], [0, 0, 0], arena_fixed=ARENA[0], arena_per_byte=ARENA[1])  # nothing at all
    compare(deframe(torch_cuda, e)[0], e)


def fuzz_and_random():
    fx = load_golden("frames")
    files = [bytes(fx["files"][int(fx["file_off"][f]):int(fx["file_off"][f + 1])]) for f in range(fx["file_off"].size - 1)]
    caps = []
    for i, b in enumerate(files):  # the frames by their length fields; every fourth connection one slot short
        n, pos = 0, 0
        while len(b) - pos >= 9:
            pos += 9 + int.from_bytes(b[pos:pos + 3], "big")
            n += 1
        caps.append(max(0, n - (i % 4 == 0)))
    rng = np.random.default_rng(17)
    lo = int(fx["ret"].size) - 4000  # the fixture's seeded random frames
    rand = []
    for _ in range(1500):
        ps = [bytes(fx["probes"][int(fx["probe_off"][i]):int(fx["probe_off"][i + 1])])
              for i in rng.integers(lo, fx["ret"].size, int(rng.integers(1, 7)))]
        rand.append(b"".join(p for p in ps if len(p) < 4096))
    return files, caps, rand, [int(rng.integers(0, 8)) for _ in rand]


def test_fuzz_corpus_and_random_connections(torch_cuda):
    files, caps, rand, rcaps = fuzz_and_random()
    for flags in (0, C.H2F_ACCEPT_PUSH):
        e = M.batch(files + rand, caps + rcaps, 16384, 300, flags, arena_fixed=ARENA[0], arena_per_byte=ARENA[1])
        assert len(set(e["cstatus"].tolist())) >= 4 and int(e["totals"][0]) > 500
        compare(deframe(torch_cuda, e, 16384, 300, flags)[0], e)


@pytest.mark.parametrize("sentinel", [s for _, s in BH.RUNS])
def test_exact_size_buffers(torch_cuda, corpus_batches, sentinel):
    """outputs of exactly the documented sizes between guard zones: nothing outside blk[0 .. totals[1]), the frame
    slots in use, blocks[0 .. nblk) and the other arrays is written; blk_off past nblk holds the total"""
    for (params, o), e in corpus_batches.items():
        if o == "shuffled":
            h, _ = deframe(torch_cuda, e, *params, sentinel=sentinel, guard=True)
            compare(h, e, sentinel)
            nblk = int(e["totals"][0])
            assert (h["blk_off"].view(np.uint32)[nblk:] == e["totals"][1]).all()
    files, caps, rand, rcaps = fuzz_and_random()
    e = M.batch(files[:200] + rand[:200], caps[:200] + rcaps[:200], arena_fixed=ARENA[0], arena_per_byte=ARENA[1])
    compare(deframe(torch_cuda, e, sentinel=sentinel, guard=True)[0], e, sentinel)


GATHER_LENGTHS = (0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 255, 256, 257, 16384)


def test_gather_edges(torch_cuda):
    """one HEADERS + CONTINUATION pair a connection: the CONTINUATION's fragment of every length of GATHER_LENGTHS at
    all 16 source alignments x all 16 destination alignments.  A filler frame of 0..15 bytes in front shifts the
    source, the opening fragment of 0..15 bytes the destination (both buffers start 16-byte aligned)."""
    rng = np.random.default_rng(3)
    conns, src_at, dst_at, seen = [], 0, 0, set()
    for L in GATHER_LENGTHS:
        for sa in range(16):
            for da in range(16):
                a = (da - dst_at) % 16  # the opening fragment: the pair's second fragment lands at da
                f = (sa - (src_at + 9 + 9 + a + 9)) % 16  # the filler frame's payload: ... and is read from sa
                x = bytes(rng.integers(0, 256, L, dtype=np.uint8))
                c = K.fr(0xfa, 0, 0, bytes(f)) + K.H(0, 1, bytes(rng.integers(0, 256, a, dtype=np.uint8))) + K.CO(K.EH, 1, x)
                assert (src_at + len(c) - L) % 16 == sa and (dst_at + a) % 16 == da
                seen.add((L, sa, da))
                conns.append(c)
                src_at += len(c)
                dst_at += a + L
    assert len(seen) == len(GATHER_LENGTHS) * 256
    e = M.batch(conns, [3] * len(conns), arena_fixed=ARENA[0], arena_per_byte=ARENA[1])
    assert int(e["totals"][0]) == len(conns) and (e["cstatus"] == 0).all()
    h, r = deframe(torch_cuda, e)
    assert r["blk"].data_ptr() % 16 == 0
    compare(h, e)


def test_resume_at_every_byte(torch_cuda):
    """a three-block connection cut at every byte: the first call sees the first part, the second what the first did
    not consume followed by the rest; blocks and records together are the single call's"""
    buf = (K.D2 + K.H(K.EH, 1, b"abc") + K.H(0, 3, b"de") + K.CO(K.EH, 3, b"fgh") +
           K.H(K.EH | K.ES | K.PRI, 5, b"\x00\x00\x00\x03\x07ij"))
    n = len(buf)
    assert n == 62
    cuts = list(range(n + 1))
    full = M.walk(buf, 16)
    assert len(full["blocks"]) == 3 and full["consumed"] == n

    def call(conns):
        e = M.batch(conns, [16] * len(conns), arena_fixed=ARENA[0], arena_per_byte=ARENA[1])
        h, _ = deframe(torch_cuda, e)
        compare(h, e)
        return h, e

    h1, e1 = call([buf[:t] for t in cuts])
    consumed = h1["consumed"].view(np.uint32)
    h2, e2 = call([buf[int(consumed[t]):] for t in cuts])

    def parts(h, e, t, shift):
        fr = h["frames"].view(C.H2_FRAME_DTYPE)[int(e["frm_first"][t]):int(e["frm_first"][t]) + int(h["nframes"][t])]
        base = int(e["in_off"][t]) - shift
        frames = [(int(f["payload_off"]) - base, int(f["length"]), int(f["stream_id"]), int(f["type"]), int(f["flags"]),
                   int(f["frag_off"]) - base if f["block"] != 0xFFFFFFFF else 0, int(f["frag_len"])) for f in fr]
        first, off = h["conn_first"].view(np.uint32), h["blk_off"].view(np.uint32)
        bl = h["blocks"].view(C.H2_BLOCK_DTYPE)
        blocks = [tuple(int(bl[b][k]) for k in ("stream_id", "end_stream_id", "flags", "dependency", "weight", "nframes")) +
                  (h["blk"][int(off[b]):int(off[b + 1])].tobytes(),) for b in range(int(first[t]), int(first[t + 1]))]
        return frames, blocks

    want = parts(*call([buf]), 0, 0)
    assert len(want[0]) == 5 and len(want[1]) == 3
    for t in cuts:
        f1, b1 = parts(h1, e1, t, 0)
        f2, b2 = parts(h2, e2, t, int(consumed[t]))
        assert (f1 + f2, b1 + b2) == want, t
        assert int(h2["consumed"][t]) == n - int(consumed[t]) and int(h1["cstatus"][t]) == 0


# ---------------------------------------------------------------------------------------------------
# closed loops: hhuff_hpack_flatten_responses -> the wire -> hhuff_h2_deframe -> the block decoders
# ---------------------------------------------------------------------------------------------------
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
PUSH = C.RES_PUSH_PROMISE


def flatten(torch, st):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()  # noqa: E731
    r = C.hpack_flatten_responses(d(st["data"]), d(st["hdr"].view(np.uint8)), d(st["res"].view(np.uint8)),
                                  d(st["conn_first"].view(np.int32)), int(st["res"].size), d(st["out_off"].view(np.int64)),
                                  st["server_off"], st["server_len"], in_size=int(st["data"].size))
    torch.cuda.synchronize()
    assert (r["rstatus"].cpu().numpy() == 0).all()
    return r["out"].cpu().numpy(), r["out_len"].cpu().numpy().view(np.uint32)


def wire(st, out, out_len):
    """what each connection's socket carries: its responses' frames back to back -> [bytes per connection]"""
    conns = []
    for c in range(st["conn_first"].size - 1):
        rs = range(int(st["conn_first"][c]), int(st["conn_first"][c + 1]))
        conns.append(b"".join(out[int(st["out_off"][r]):int(st["out_off"][r]) + int(out_len[r])].tobytes() for r in rs))
    return conns


def frame_count(b):
    n, pos = 0, 0
    while pos < len(b):
        pos += 9 + int.from_bytes(b[pos:pos + 3], "big")
        n += 1
    return n


def decode_after(torch, r, in_size, nconn, frm_cap, kind, trailers=None):
    """enqueue the block decoder `kind` on the de-framer's device tensors r as they are: no size is read back, every
    output is sized from in_size and frm_cap, nothing synchronises: -> its output tensors (downloaded() waits)"""
    i32 = lambda n: torch.empty(max(1, n), dtype=torch.int32, device="cuda")  # noqa: E731
    d = dict(arena=torch.empty(ARENA[0] * frm_cap + ARENA[1] * in_size + 16, dtype=torch.uint8, device="cuda"),
             name_off=i32(in_size), name_len=i32(in_size), value_off=i32(in_size), value_len=i32(in_size),
             fflags=torch.empty(max(1, in_size), dtype=torch.uint8, device="cuda"), nfields=i32(frm_cap), bstatus=i32(frm_cap))
    L = C.lib()
    scratch = torch.empty(max(16, int(L.hhuff_hpack_scratch_size(nconn, 4096))), dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    head = [p(r["blk"]), in_size, p(r["blk_off"]), p(r["conn_first"]), nconn, 4096]
    mid = [p(d["arena"]), p(r["arena_off"]), p(d["name_off"]), p(d["name_len"]), p(d["value_off"]), p(d["value_len"]),
           p(d["fflags"]), p(d["nfields"]), p(d["bstatus"])]
    tail = [p(scratch), scratch.numel(), 0, torch.cuda.current_stream().cuda_stream]
    if kind == "responses":
        d["rec"] = torch.empty((max(1, frm_cap), 4), dtype=torch.int32, device="cuda")
        rc = L.hhuff_hpack_parse_responses(*head, p(trailers), *mid, p(d["rec"]), *tail)
    elif kind == "requests":
        d["rec"] = torch.empty((max(1, frm_cap), 12), dtype=torch.int32, device="cuda")
        rc = L.hhuff_hpack_parse_requests(*head, *mid, p(d["rec"]), *tail)
    else:
        rc = L.hhuff_hpack_decode_blocks(*head, *mid, *tail)
    assert rc == 0
    return d


def downloaded(torch, d):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def field(st, h):
    d = st["data"]
    return (d[int(h["name_off"]):int(h["name_off"]) + int(h["name_len"])].tobytes(),
            d[int(h["value_off"]):int(h["value_off"]) + int(h["value_len"])].tobytes())


def want_fields(st, R):
    """the fields the encoder put into record R's block, in its order (hpack.c:1157-1168)"""
    fs = [field(st, h) for h in st["hdr"][int(R["hdr_first"]):int(R["hdr_first"]) + int(R["nhdr"])]]
    if R["flags"] & (PUSH | C.RES_REQUEST | C.RES_TRAILERS):
        return fs
    head = [(b":status", b"%d" % R["status"])]
    if R["flags"] & C.RES_SERVER and st["server_len"]:
        head.append((b"server", st["data"][st["server_off"]:st["server_off"] + st["server_len"]].tobytes()))
    return head + fs + ([(b"content-length", b"%d" % R["content_length"])] if R["content_length"] != NONE else [])


def check_fields(st, h, d, blocks_of_records):
    """record r's fields came back in block blocks_of_records[r]"""
    off = h["blk_off"].view(np.uint32)
    for r, b in enumerate(blocks_of_records):
        assert int(d["bstatus"][b]) == 0, (r, int(d["bstatus"][b]))
        s0, got = int(off[b]), []
        for k in range(int(d["nfields"][b])):
            no, nl, vo, vl = (int(d[x].view(np.uint32)[s0 + k]) for x in ("name_off", "name_len", "value_off", "value_len"))
            got.append((d["arena"][no:no + nl].tobytes(), d["arena"][vo:vo + vl].tobytes()))
        assert got == want_fields(st, st["res"][r]), r


def loop(torch, st, flags=0, decode=None):
    """flatten, lay the bytes on the wire, de-frame against the model: -> (model batch, host outputs, device tensors).
    decode(r, in_size, nconn, frm_cap) enqueues the block decoder right behind the de-framer, on its stream, before
    anything synchronises or reads a result back (the de-framer's pool workspace is released on that stream too);
    its output tensors are r["then"]."""
    conns = wire(st, *flatten(torch, st))
    e = M.batch(conns, [frame_count(b) for b in conns], 16384, C.H2O_MAX_REQLEN, flags, arena_fixed=ARENA[0],
                arena_per_byte=ARENA[1])
    then = None if decode is None else (lambda r: decode(r, int(e["data"].size), len(conns), e["frm_cap"]))
    h, r = deframe(torch, e, 16384, C.H2O_MAX_REQLEN, flags, then=then)
    compare(h, e)
    return e, h, r


def response_session():
    """responses and trailers mixed; every eighth response's header list needs CONTINUATION frames (within
    H2O_MAX_HEADERS = 100 fields, past which the response rules end a block with -254)"""
    rng = np.random.default_rng(12)
    TOK = C.HDR_TOKEN
    pool = [(b"date", b"Tue, 20 Oct 2026 10:00:00 GMT", TOK), (b"content-type", b"text/html; charset=utf-8", TOK),
            (b"cache-control", b"max-age=3600", TOK), (b"vary", b"accept-encoding", TOK), (b"etag", b'"5f2a-1b"', TOK),
            (b"x-request-id", b"7f3c9a12-00aa", 0), (b"x-frame-options", b"DENY", 0)]
    conns, k = [], 0
    for c in range(96):
        rs, sid = [], 1
        for _ in range(int(rng.integers(0, 5))):
            hs = [pool[i] for i in rng.choice(len(pool), int(rng.integers(1, len(pool))), replace=False)]
            if k % 8 == 3:  # 80 fields of 500 to 700 bytes, 40 to 56 KB: two or three CONTINUATIONs
                hs += [(b"x-trace-%d" % i, bytes(rng.integers(97, 123, int(rng.integers(500, 700)), dtype=np.uint8)), 0)
                       for i in range(80)]
            with_trailers = k % 3 == 1
            rs.append(dict(status=int(rng.choice([200, 204, 404, 503])), headers=hs, stream_id=sid,
                           content_length=int(rng.integers(0, 1 << 20)) if k % 2 else None,
                           flags=C.RES_SERVER | (0 if with_trailers or k % 5 == 0 else C.RES_END_STREAM)))
            if with_trailers:
                rs.append(dict(flags=C.RES_TRAILERS, stream_id=sid, headers=[(b"x-checksum", b"%08x" % int(rng.integers(0, 1 << 32)), 0)]))
            sid += 2
            k += 1
        conns.append(rs)
    return HE.build_batch(conns)


def test_closed_loop_responses(torch_cuda):
    torch = torch_cuda
    st = response_session()
    is_trailers = (st["res"]["flags"] & C.RES_TRAILERS) != 0
    assert is_trailers.any() and not is_trailers.all()

    def decode(r, in_size, nconn, frm_cap):
        # the second block on a stream is its trailers: a block whose stream id is its predecessor's, within a
        # connection (device ops on the de-framer's records, enqueued behind it)
        rec = r["blocks"].view(torch.int32).view(-1, 8)
        first = torch.zeros(frm_cap + 1, dtype=torch.bool, device="cuda")
        first[r["conn_first"][:-1].long()] = True
        trailers = torch.zeros(frm_cap, dtype=torch.uint8, device="cuda")
        trailers[1:] = ((rec[1:, 0] == rec[:-1, 0]) & ~first[1:frm_cap]).to(torch.uint8)
        return dict(decode_after(torch, r, in_size, nconn, frm_cap, "responses", trailers), trailers=trailers)

    e, h, r = loop(torch, st, decode=decode)
    nres, nconn = st["res"].size, st["conn_first"].size - 1
    assert int(h["totals"][0]) == nres and (h["cstatus"][:nconn] == 0).all()
    blocks = h["blocks"].view(C.H2_BLOCK_DTYPE)[:nres]
    assert (blocks["flags"] & C.H2B_CONTINUED).sum() >= 8 and (blocks["nframes"] >= 3).any()
    d = downloaded(torch, r["then"])
    np.testing.assert_array_equal(d["trailers"][:nres] != 0, is_trailers)
    check_fields(st, h, d, range(nres))
    np.testing.assert_array_equal(blocks["stream_id"], st["res"]["stream_id"])
    np.testing.assert_array_equal(blocks["end_stream_id"], st["res"]["stream_id"])
    np.testing.assert_array_equal((blocks["flags"] & C.H2B_END_STREAM) != 0,
                                  ((st["res"]["flags"] & C.RES_END_STREAM) != 0) | is_trailers)
    np.testing.assert_array_equal(d["rec"][:nres, 0], np.where(is_trailers, 0, st["res"]["status"]))


def push_session():
    """promises and the parents' responses in wire order.  The generator's responses on the pushed (even) streams are
    left out: rule 5 refuses HEADERS on an even stream, as h2o's server does."""
    st = HE.make_push_session(150, seed=8, small_table_frac=0.2, big_frac=0.02, frame_frac=0.0, dont_compress_frac=0.0)[0]
    keep = ((st["res"]["flags"] & PUSH) != 0) | (st["res"]["stream_id"] % 2 == 1)
    before = np.concatenate([[0], np.cumsum(keep)])
    res = st["res"][keep]
    return dict(st, res=res, conn_first=before[st["conn_first"]].astype(np.uint32),
                out_off=HE.out_offsets(st["hdr"], res, st["server_len"]))


def test_closed_loop_promises(torch_cuda):
    torch = torch_cuda
    st = push_session()
    is_push = (st["res"]["flags"] & PUSH) != 0
    assert is_push.any() and not is_push.all()
    e, h, r = loop(torch, st, C.H2F_ACCEPT_PUSH, decode=lambda r, *a: decode_after(torch, r, *a, "blocks"))
    nres, nconn = st["res"].size, st["conn_first"].size - 1
    assert int(h["totals"][0]) == nres and (h["cstatus"][:nconn] == 0).all()
    d = downloaded(torch, r["then"])
    check_fields(st, h, d, range(nres))
    blocks = h["blocks"].view(C.H2_BLOCK_DTYPE)[:nres]
    assert (blocks["flags"] & C.H2B_CONTINUED).any()
    np.testing.assert_array_equal((blocks["flags"] & C.H2B_PROMISE) != 0, is_push)
    np.testing.assert_array_equal(blocks["promised_stream_id"], np.where(is_push, st["res"]["stream_id"], 0))
    np.testing.assert_array_equal(blocks["stream_id"], np.where(is_push, st["res"]["parent_stream_id"], st["res"]["stream_id"]))
    # without the flag the same connections stop at their first promise, as h2o does
    e0, h0, _ = loop(torch, st)
    for c in range(nconn):
        rs = np.arange(int(st["conn_first"][c]), int(st["conn_first"][c + 1]))
        p = rs[is_push[rs]]
        before = (p[0] - rs[0]) if p.size else rs.size
        assert int(h0["conn_first"].view(np.uint32)[c + 1]) - int(h0["conn_first"].view(np.uint32)[c]) == before
        assert (int(h0["cstatus"][c]), int(h0["cerr"][c])) == ((-1, C.H2F_ERR_PUSH_PROMISE) if p.size else (0, 0))


def test_closed_loop_requests(torch_cuda):
    torch = torch_cuda
    st = HE.make_request_session(300, seed=31, big_frac=0.02, frame_frac=0.0, small_table_frac=0.2, dont_compress_frac=0.0)[0]
    e, h, r = loop(torch, st, decode=lambda r, *a: decode_after(torch, r, *a, "requests"))
    nres, nconn = st["res"].size, st["conn_first"].size - 1
    assert int(h["totals"][0]) == nres
    d = downloaded(torch, r["then"])
    check_fields(st, h, d, range(nres))
    blocks = h["blocks"].view(C.H2_BLOCK_DTYPE)[:nres]
    assert (blocks["flags"] & C.H2B_CONTINUED).any()
    np.testing.assert_array_equal(blocks["stream_id"], st["res"]["stream_id"])
    np.testing.assert_array_equal((blocks["flags"] & C.H2B_END_STREAM) != 0, (st["res"]["flags"] & C.RES_END_STREAM) != 0)
    assert (d["rec"][:nres, 2] == 0).all()  # hhuff_request_t.method: the block's first field
