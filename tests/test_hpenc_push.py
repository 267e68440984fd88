"""HTTP/2 server push, encode side: h2o_hpack_flatten_push_promise (lib/http2/hpack.c:1098-1135) as
HHUFF_RES_PUSH_PROMISE records of hhuff_hpack_flatten_responses (include/hhuff.h (2f)), mixed with the
connection's responses on one encoder table.
The expectation is tests/hpenc_push_model.py: the pinned restatement's request bytes, re-framed as a promise.
CPU: hand-written known answers, the model's own consistency, the bound, what make_push_session covers, that
the older generators are unchanged, and a round trip through the restatement's decoder.
GPU: the known answers byte for byte, sessions against the model, payloads around max_frame_size, refusals
with exact regions over a sentinel-filled output, old records with a non-zero parent_stream_id, and round
trips through the device decoders."""
import hashlib

import numpy as np
import pytest

from conftest import load_golden
from h2o_amd import codec as C
from h2o_amd import hpenc_synth as HE
from hpenc_push_model import CONTINUATION, END_HEADERS, PUSH_PROMISE, PushModel, block_of, deframe

TOK = C.HDR_TOKEN
PUSH = C.RES_PUSH_PROMISE
KEYS = ("out_len", "headers_size", "rstatus")
M_, SC, AU, PA = b":method", b":scheme", b":authority", b":path"
NONE = 0xFFFFFFFFFFFFFFFF


def promise(promised, parent, path=b"/", headers=((b"accept-encoding", b"gzip, deflate", TOK),), scheme=b"https",
            authority=b"a.example", **k):
    own = [(M_, b"GET", TOK), (SC, scheme, TOK), (AU, authority, TOK), (PA, path, TOK)]
    return dict(status=4, headers=own + list(headers), flags=PUSH | k.pop("fl", 0), stream_id=promised,
                parent_stream_id=parent, **k)


def region(r, b, k):
    o = int(b["out_off"][k])
    return np.asarray(r["out"])[o:o + int(r["out_len"][k])].tobytes()


def frames_of(out, out_off, out_len):
    return b"".join(np.asarray(out)[int(o):int(o) + int(L)].tobytes() for o, L in zip(out_off, out_len))


# ---- known answers, written by hand ----
KAT_FIRST = bytes.fromhex("000011050400000001" "00000002" "828741871ae5f23a6ba0bf8490")
KAT_SECOND = bytes.fromhex("000009050400000001" "00000004" "8287c08490")  # :authority: dynamic index 64
KAT_RESPONSE = dict(status=200, flags=C.RES_SERVER, stream_id=1, headers=[(b"content-type", b"text/html", TOK)])


def kat_batch():
    c0 = [promise(2, 1), KAT_RESPONSE, promise(4, 1)]
    c1 = [promise(2, 1, header_table_size=256)]
    return HE.build_batch([c0, c1])


def check_kats(r, b, oracle_mod):
    assert list(r["rstatus"][:4]) == [0, 0, 0, 0]
    assert region(r, b, 0) == KAT_FIRST
    assert region(r, b, 2) == KAT_SECOND
    assert list(r["headers_size"][:4]) == [17, int(r["out_len"][1]) - 9, 9, int(r["out_len"][3]) - 9]
    # the response between them carries no dynamic reference: the bytes of the same batch without the promises
    alone = HE.build_batch([[KAT_RESPONSE]])
    q = oracle_mod.HpeSession(oracle_mod.oracle(), 1).step(alone["data"], alone["hdr"], alone["res"], alone["conn_first"],
                                                           alone["out_off"], alone["server_off"], alone["server_len"])
    assert region(r, b, 1) == region(q, alone, 0)
    third = region(r, b, 3)
    assert third[:9] == bytes([0, 0, len(third) - 9, 5, 4, 0, 0, 0, 1])
    assert third[9:16] == bytes.fromhex("00000002" "3fe101")  # the id, then the size update to 256
    assert third[16:18] == bytes.fromhex("8287")


def test_kats_model(oracle_codec):
    from oracle import oracle as O

    b = kat_batch()
    check_kats(PushModel(2).step(b), b, O)


# ---- the model against itself and the restatement ----
def run_model(steps, nconn):
    m = PushModel(nconn)
    return [m.step(st) for st in steps]


def test_model_push_only_is_request_payload(oracle_codec):
    from oracle import oracle as O

    steps = HE.make_push_session(60, steps=2, seed=4, push_only=True, small_table_frac=0.3, big_frac=0.02, frame_frac=0.2,
                                 notoken_frac=0.1, dont_compress_frac=0.1)
    s = O.HpeSession(O.oracle(), 60)
    nbig = 0
    for st, r in zip(steps, run_model(steps, 60)):
        assert (st["res"]["flags"] == PUSH).all() and (r["rstatus"] == 0).all()
        rq = st["res"].copy()
        rq["flags"] = C.RES_REQUEST
        q = s.step(st["data"], st["hdr"], rq, st["conn_first"], st["out_off"], st["server_off"], st["server_len"])
        for k, R in enumerate(st["res"]):
            fs, qs = deframe(region(r, st, k)), deframe(region(q, st, k))
            payload = b"".join(f[3] for f in fs)
            assert payload[:4] == int(R["stream_id"]).to_bytes(4, "big")
            assert payload[4:] == b"".join(f[3] for f in qs)
            assert len(payload) == r["headers_size"][k] and sum(len(f[3]) for f in fs) == r["headers_size"][k]
            assert r["out_len"][k] == len(payload) + 9 * len(fs)
            assert [f[0] for f in fs] == [PUSH_PROMISE] + [CONTINUATION] * (len(fs) - 1)
            assert [f[1] for f in fs] == [0] * (len(fs) - 1) + [END_HEADERS]  # never END_STREAM
            assert all(f[2] == R["parent_stream_id"] for f in fs)
            assert all(len(f[3]) == R["max_frame_size"] for f in fs[:-1]) and 0 < len(fs[-1][3]) <= R["max_frame_size"]
            nbig += len(fs) > 1
    assert nbig > 0


def test_bound_holds(oracle_codec):
    """hhuff_hpack_response_bound(.., 0, M) covers a promise's worst representation: every header a new-name
    literal sent raw, the size update, the id"""
    names = [bytes([0x7f - i]) * (1 + i) for i in range(30)]  # raw (Huffman longer than the input)
    conn = [dict(status=0, headers=[(n, n * 3, C.HDR_DONT_COMPRESS) for n in names], flags=PUSH | C.RES_SERVER,
                 content_length=2 ** 64 - 2, stream_id=0xFFFFFFFE, parent_stream_id=0x7FFFFFFF, header_table_size=0)]
    b = HE.build_batch([conn], server=b"\x7f" * 300)
    nv = int(b["hdr"]["name_len"].sum() + b["hdr"]["value_len"].sum())
    bound = int(C.hpack_response_bound(nv, 30, 0, 16384))
    b["out_off"] = np.array([0, bound], np.uint64)
    r = PushModel(1).step(b)
    assert r["rstatus"][0] == 0 and 0 < r["out_len"][0] <= bound
    assert region(r, b, 0)[9:13] == b"\xff\xff\xff\xfe" and region(r, b, 0)[5:9] == b"\x7f\xff\xff\xff"


def field(st, h):
    d = st["data"]
    return (d[h["name_off"]:h["name_off"] + h["name_len"]].tobytes(), d[h["value_off"]:h["value_off"] + h["value_len"]].tobytes())


def test_push_session_coverage(oracle_codec):
    steps = HE.make_push_session(150, steps=3)
    seen = set()
    for st, r in zip(steps, run_model(steps, 150)):
        assert (r["rstatus"] == 0).all()
        conn = np.repeat(np.arange(150), np.diff(st["conn_first"].astype(np.int64)))
        last_even = {}
        for k, R in enumerate(st["res"]):
            if not R["flags"] & PUSH:
                assert R["parent_stream_id"] == 0
                seen.add("pushed response" if R["stream_id"] % 2 == 0 else "parent response")
                continue
            c = int(conn[k])
            assert R["stream_id"] % 2 == 0 and R["parent_stream_id"] % 2 == 1 and R["status"] == 4
            assert R["stream_id"] > last_even.get(c, 0)
            last_even[c] = int(R["stream_id"])
            fs = [field(st, h) for h in st["hdr"][R["hdr_first"]:R["hdr_first"] + R["nhdr"]]]
            assert [f[0] for f in fs[:4]] == [M_, SC, AU, PA] and fs[0][1] == b"GET"
            assert {f[0] for f in fs[4:]} <= {b"accept", b"accept-charset", b"accept-encoding", b"accept-language", b"user-agent"}
            block, pid = block_of(region(r, st, k))
            assert pid == R["stream_id"]
            if block[0] & 0xE0 == 0x20:
                seen.add("size update")
            if len(block) + 4 > R["max_frame_size"]:
                seen.add("over max_frame_size")
            if len(block) == R["nhdr"] and all(x & 0x80 for x in block):
                seen.add("all indexed or one-byte")
            seen.add("scheme http(s)" if fs[1][1] in (b"http", b"https") else "scheme other")
            seen.add("path " + {b"/": "/", b"/index.html": "/index.html"}.get(fs[3][1], "other"))
            for n, v in fs[4:]:
                if n == b"accept-encoding":
                    seen.add("gzip, deflate" if v == b"gzip, deflate" else "other accept-encoding")
    assert seen >= {"size update", "over max_frame_size", "all indexed or one-byte", "scheme other", "scheme http(s)",
                    "path /", "path /index.html", "path other", "gzip, deflate", "other accept-encoding",
                    "pushed response", "parent response"}, seen


def digest(steps):
    h = hashlib.sha256()
    for st in steps:
        for k in sorted(st):
            v = st[k]
            h.update(k.encode())
            h.update(np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else b"%d" % int(v))
    return h.hexdigest()


def test_older_generators_unchanged():
    """digests taken from the commit before make_push_session existed"""
    assert digest(HE.make_session(64, seed=3)) == "4819a31b472276ead6b3fb3c058dbba932b9a2029c7be92434da7113d8c310ac"
    assert digest(HE.make_request_session(64, seed=3)) == "778e9b34409ce416d5c32e21335e5492b97defc4eb6fa181e5cfd0297d4db745"


def blocks_in_wire_order(st, r):
    """-> (data, blk_off): every record's header block (frame headers and a promise's id stripped), in record order
    = wire order"""
    blocks = []
    for k, R in enumerate(st["res"]):
        block, pid = block_of(region(r, st, k))
        assert (pid is not None) == bool(R["flags"] & PUSH) and (pid is None or pid == R["stream_id"])
        blocks.append(block)
    blk_off = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.uint32)
    return np.frombuffer(b"".join(blocks), np.uint8).copy(), blk_off


def want_fields(st, R):
    fs = [field(st, h) for h in st["hdr"][R["hdr_first"]:R["hdr_first"] + R["nhdr"]]]
    if R["flags"] & (PUSH | C.RES_REQUEST | C.RES_TRAILERS):
        return fs
    d = st["data"]
    head = [(b":status", b"%d" % R["status"])]
    if R["flags"] & C.RES_SERVER and st["server_len"]:
        head.append((b"server", d[st["server_off"]:st["server_off"] + st["server_len"]].tobytes()))
    return head + fs + ([(b"content-length", b"%d" % R["content_length"])] if R["content_length"] != NONE else [])


def check_roundtrip(st, blk_off, d):
    assert (np.asarray(d["bstatus"])[:blk_off.size - 1] == 0).all()
    A = np.asarray(d["arena"])
    for b, R in enumerate(st["res"]):
        s0 = int(blk_off[b])
        got = []
        for k in range(int(d["nfields"][b])):
            no, nl, vo, vl = (int(d[x][s0 + k]) for x in ("name_off", "name_len", "value_off", "value_len"))
            got.append((A[no:no + nl].tobytes(), A[vo:vo + vl].tobytes()))
        assert got == want_fields(st, R), b


def mixed_session(nconn, seed):
    """no header-level dont_compress: see tests/test_hpenc.py check_request_roundtrip for why no round trip
    holds across it"""
    return HE.make_push_session(nconn, seed=seed, small_table_frac=0.2, big_frac=0.01, frame_frac=0.2, dont_compress_frac=0.0)[0]


def push_only_session(nconn, seed):
    return HE.make_push_session(nconn, seed=seed, push_only=True, small_table_frac=0.2, big_frac=0.01, frame_frac=0.2,
                                dont_compress_frac=0.0)[0]


def check_own_slots(st, d):
    req = np.asarray(d["req"]).reshape(-1).view(np.int32).reshape(-1, 12)[:st["res"].size]
    for col, name in ((2, "method"), (3, "scheme"), (4, "authority"), (5, "path")):
        assert (req[:, col] == col - 2).all(), name  # field 0 .. 3 of the block: the own fields in order


def test_roundtrip_restatement(oracle_codec):
    from oracle import oracle as O

    st = mixed_session(120, 6)
    r = PushModel(120).step(st)
    assert (r["rstatus"] == 0).all() and (st["res"]["flags"] & PUSH).any() and not (st["res"]["flags"] & PUSH).all()
    data, blk_off = blocks_in_wire_order(st, r)
    check_roundtrip(st, blk_off, O.oracle().hpack_decode_blocks(data, blk_off, st["conn_first"]))
    st = push_only_session(120, 7)
    r = PushModel(120).step(st)
    data, blk_off = blocks_in_wire_order(st, r)
    d = O.oracle().hpack_decode_blocks(data, blk_off, st["conn_first"], requests=True)
    check_roundtrip(st, blk_off, d)
    check_own_slots(st, d)


# ---------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from h2o_amd import build

    build.build(verbose=False)
    return torch


def gpu_step(torch, st, scratch=None, cont=False, fill=None):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()  # noqa: E731
    data = dev(st["data"] if st["data"].size else np.zeros(1, np.uint8))
    hdr = dev(st["hdr"].view(np.uint8) if st["hdr"].size else np.zeros(20, np.uint8))
    out = None if fill is None else torch.full((max(1, int(st["out_off"][-1])),), fill, dtype=torch.uint8, device="cuda")
    r = C.hpack_flatten_responses(data, hdr if st["hdr"].size else hdr[:0], dev(st["res"].view(np.uint8)),
                                  dev(st["conn_first"].view(np.int32)), int(st["res"].size), dev(st["out_off"].view(np.int64)),
                                  st["server_off"], st["server_len"], in_size=int(st["data"].size), out=out, scratch=scratch,
                                  cont=cont)
    torch.cuda.synchronize()
    h = {k: (v.cpu().numpy() if k != "scratch" else v) for k, v in r.items()}
    return dict(out=h["out"], out_len=h["out_len"].view(np.uint32), headers_size=h["headers_size"].view(np.uint32),
                rstatus=h["rstatus"], scratch=h["scratch"])


def check_against(r, q, st):
    for key in KEYS:
        np.testing.assert_array_equal(r[key], q[key], err_msg=key)
    assert frames_of(r["out"], st["out_off"], r["out_len"]) == frames_of(q["out"], st["out_off"], q["out_len"])


@pytest.mark.gpu
def test_gpu_kats(torch_cuda, oracle_codec):
    """the test that shows the feature: a library without the flag takes `status` 4 for a response status and
    refuses every promise (HHUFF_RES_EINVAL)"""
    from oracle import oracle as O

    b = kat_batch()
    check_kats(gpu_step(torch_cuda, b), b, O)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [41, 42])
def test_gpu_vs_model(torch_cuda, oracle_codec, seed):
    steps = HE.make_push_session(150, steps=3, seed=seed, small_table_frac=0.25, big_frac=0.01, notoken_frac=0.1,
                                 dont_compress_frac=0.1, frame_frac=0.2)
    m = PushModel(150)
    scratch = None
    for k, st in enumerate(steps):
        q = m.step(st)
        r = gpu_step(torch_cuda, st, scratch=scratch, cont=k > 0)
        scratch = r["scratch"]
        check_against(r, q, st)


def edge_batch(M):
    """one promise per connection whose payload P, id included, is M-1, M, M+1, M+4, 2M, 2M+1: a raw value of
    0x00 bytes (13-bit codes: Huffman never shortens it) of the length that gives P"""
    targets = [M - 1, M, M + 1, M + 4, 2 * M, 2 * M + 1]
    conns = []
    for P in targets:
        L = P - 64
        for _ in range(4):
            c = [promise(2, 1, path=b"/p", headers=[(b"x-pad", b"\0" * L, 0)], max_frame_size=M)]
            got = int(PushModel(1).step(HE.build_batch([c]))["headers_size"][0])
            if got == P:
                break
            L += P - got
        conns.append(c)
    return HE.build_batch(conns), targets


@pytest.mark.gpu
@pytest.mark.parametrize("M", [16384, 16385])
def test_gpu_frame_edges(torch_cuda, oracle_codec, M):
    b, targets = edge_batch(M)
    q = PushModel(len(targets)).step(b)
    assert list(q["headers_size"]) == targets and (q["rstatus"] == 0).all()
    assert [len(deframe(region(q, b, k))) for k in range(6)] == [1, 1, 2, 2, 2, 3]
    check_against(gpu_step(torch_cuda, b), q, b)


@pytest.mark.gpu
def test_gpu_refusals(torch_cuda, oracle_codec):
    """refused promises write nothing, fail their connection, and nothing is written past out_len anywhere"""
    resp = dict(status=200, flags=C.RES_SERVER, headers=[(b"content-type", b"text/html", TOK)])
    conns = [[promise(2, 1, fl=C.RES_TRAILERS), promise(4, 1)],
             [promise(2, 1, fl=C.RES_REQUEST), resp],
             [dict(promise(2, 1), status=6), promise(4, 1)],
             [promise(2, 1, path=b"/one-byte-short"), resp],
             [promise(2, 1, path=b"/exact"), resp]]
    b = HE.build_batch(conns)
    sizes = np.diff(b["out_off"].astype(np.int64))
    fit = PushModel(5).step(b)
    assert list(fit["rstatus"][6:10]) == [0, 0, 0, 0]
    sizes[6] = int(fit["out_len"][6]) - 1
    sizes[8] = int(fit["out_len"][8])
    b["out_off"] = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    q = PushModel(5).step(b, fill=0xA5)
    E, K, S = C.RES_EINVAL, C.RES_SKIPPED, C.RES_SPACE
    assert list(q["rstatus"]) == [E, K, E, K, E, K, S, K, 0, 0]
    r = gpu_step(torch_cuda, b, fill=0xA5)
    for key in KEYS:
        np.testing.assert_array_equal(r[key], q[key], err_msg=key)
    np.testing.assert_array_equal(r["out"], q["out"])  # frames, and the sentinel everywhere else


def golden_steps(g, name):
    nconn, nsteps = (int(x) for x in g[name + "_meta"])
    steps = []
    for k in range(nsteps):
        p = "%s_%d_" % (name, k)
        st = {key[len(p):]: v for key, v in g.items() if key.startswith(p)}
        st["hdr"] = st["hdr"].view(C.HPE_HEADER_DTYPE)
        st["res"] = st["res"].view(C.HPE_RESPONSE_DTYPE)
        st["server_off"], st["server_len"] = (int(x) for x in st["server"])
        steps.append(st)
    return nconn, steps


@pytest.mark.gpu
def test_gpu_old_records_ignore_parent(torch_cuda):
    """records without the flag give the fixture's bytes whatever parent_stream_id holds"""
    nconn, steps = golden_steps(load_golden("hpenc"), "h4096")
    scratch = None
    for k, st in enumerate(steps):
        st["res"] = st["res"].copy()
        st["res"]["parent_stream_id"] = 0xDEADBEEF
        r = gpu_step(torch_cuda, st, scratch=scratch, cont=k > 0)
        scratch = r["scratch"]
        n = st["res"].size
        for key in KEYS:
            np.testing.assert_array_equal(r[key][:n].astype(st[key].dtype), st[key], err_msg=key)
        assert frames_of(r["out"], st["out_off"], st["out_len"]) == st["frames"].tobytes()


def gpu_decode(torch, st, data, blk_off, requests):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()  # noqa: E731
    L = np.diff(blk_off.astype(np.int64))
    ao = np.concatenate([[0], np.cumsum(16 * L + 1024)]).astype(np.int64)  # 8/5 of a block is its longest decode
    d = C.hpack_decode_blocks(dev(data), dev(blk_off.view(np.int32)), dev(st["conn_first"].view(np.int32)), arena_off=dev(ao),
                              requests=requests)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in d.items() if k != "scratch"}
    for k in ("name_off", "name_len", "value_off", "value_len", "nfields"):
        h[k] = h[k].view(np.uint32)  # u32 bits in int32 tensors
    return h


@pytest.mark.gpu
def test_gpu_roundtrip(torch_cuda):
    """GPU flatten -> deframe in wire order -> GPU decode: every field of every block comes back; a push-only
    session passes h2o_hpack_parse_request's rules with the own fields in their slots"""
    st = mixed_session(300, 8)
    r = gpu_step(torch_cuda, st)
    assert (r["rstatus"] == 0).all() and (st["res"]["flags"] & PUSH).any() and not (st["res"]["flags"] & PUSH).all()
    data, blk_off = blocks_in_wire_order(st, r)
    check_roundtrip(st, blk_off, gpu_decode(torch_cuda, st, data, blk_off, requests=False))
    st = push_only_session(300, 9)
    r = gpu_step(torch_cuda, st)
    assert (r["rstatus"] == 0).all()
    data, blk_off = blocks_in_wire_order(st, r)
    d = gpu_decode(torch_cuda, st, data, blk_off, requests=True)
    check_roundtrip(st, blk_off, d)
    check_own_slots(st, d)
