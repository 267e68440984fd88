"""The HTTP/3 de-framer on the GPU (include/hhuff.h (2l), h2o_amd/csrc/hhuff_h3frames.hip) against the model
(h3frames_model.py): the hand-built corpus in order and shuffled, every output array compared; the corpus's literal
expectations directly; empty connections and streams across the walk workgroup's boundary and a batch that makes the
second-level scan sum runs; varints of every width; every corpus stream cut at every byte and resumed; exact-size
guarded outputs with st_out on st_in; the gather at every pair of alignments; hostile bytes, states and offsets; and
closed loops with nothing but device arrays between the de-framer and what is enqueued behind it: the response encoder
and decoder, the encoder and decoder sessions over three steps, and SETTINGS into the peers call."""
import numpy as np
import pytest

import bounds_harness as BH
import h3frames_corpora as K
import h3frames_model as M
from h2o_amd import codec as C
from h2o_amd import hpenc_synth as HE

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
ARENA = (1024, 16)  # arena_fixed, arena_per_byte of these tests
U32 = ("nframes", "consumed", "serr", "enc_off", "enc_len", "sec_off", "conn_first", "totals", "got_settings")
OUTPUTS = U32 + ("st_out", "frames", "sstatus", "out", "sec_stream_id", "sec_stream", "peers", "settings", "arena_off")


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
    if a.dtype.names:
        a = a.view(np.uint8)
    return torch.from_numpy(a.copy()).cuda()


def out_bytes(nstr, nconn, frm_cap, in_size):
    return dict(st_out=32 * nstr, frames=32 * frm_cap, nframes=4 * nstr, consumed=4 * nstr, sstatus=4 * nstr, serr=4 * nstr, out=in_size,
                enc_off=4 * nconn, enc_len=4 * nconn, sec_off=4 * (nstr + 1), conn_first=4 * (nconn + 1), sec_stream_id=8 * nstr,
                sec_stream=4 * nstr, totals=12, peers=8 * nconn, settings=16 * nconn, got_settings=4 * nconn, arena_off=8 * (nstr + 1))


def deframe(torch, e, mfps=16384, flags=0, sentinel=SENTINEL, guard=False, then=None, alias=False, fill=0):
    """hhuff_h3_deframe on the model's batch e, every output of exactly its documented size and filled with the sentinel
    (guard: between two guard zones, which are checked; the input then lies between zones of `fill` too): -> (numpy
    arrays, device tensors).  alias: st_out is st_in.  then(r), if given, runs right behind the call -- before anything
    synchronises or is copied to the host -- and its result is kept as r["then"]."""
    nstr, nconn, frm_cap, in_size = e["str_off"].size - 1, e["conn_str"].size - 1, e["frm_cap"], int(e["data"].size)
    if guard:
        whole_in = np.full(in_size + 2 * BH.GUARD, fill, np.uint8)
        whole_in[BH.GUARD:BH.GUARD + in_size] = e["data"]
        data = dev(torch, whole_in)[BH.GUARD:BH.GUARD + max(1, in_size)]
    else:
        data = dev(torch, e["data"] if in_size else np.zeros(1, np.uint8))
    kinds = {k: torch.int32 for k in U32 + ("sstatus", "sec_stream")}
    kinds.update(sec_stream_id=torch.int64, arena_off=torch.int64)
    whole, out = {}, {}
    st_in = dev(torch, e["st_in"])
    for k, n in out_bytes(nstr, nconn, frm_cap, in_size).items():
        if n == 0:  # (no such array: the wrapper passes a dummy)
            continue
        if k == "st_out" and alias:
            out[k] = st_in
            continue
        if guard:
            whole[k], inner = BH.guarded(torch, n, sentinel)
        else:
            inner = torch.full((n,), sentinel, dtype=torch.uint8, device="cuda")
        out[k] = inner.view(kinds[k]) if k in kinds else inner
    r = C.h3_deframe(data, dev(torch, e["str_off"]), dev(torch, e["conn_str"]), dev(torch, e["frm_first"]), frm_cap, st_in, mfps,
                     flags, in_size=in_size, arena_fixed=ARENA[0], arena_per_byte=ARENA[1], out=out)
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
    nstr, nconn, frm_cap = e["str_off"].size - 1, e["conn_str"].size - 1, e["frm_cap"]
    for k in U32:
        np.testing.assert_array_equal(h[k].view(np.uint32)[:e[k].size], e[k], err_msg=k)
    np.testing.assert_array_equal(h["sstatus"][:nstr], e["sstatus"], err_msg="sstatus")
    np.testing.assert_array_equal(h["arena_off"].view(np.uint64)[:nstr + 1], e["arena_off"], err_msg="arena_off")
    np.testing.assert_array_equal(h["st_out"][:32 * nstr].view(C.H3_STREAM_DTYPE), e["st_out"], err_msg="st_out")
    frames, used = h["frames"][:32 * frm_cap].view(C.H3_FRAME_DTYPE), e["frame_used"]
    np.testing.assert_array_equal(frames[used], e["frames"][used], err_msg="frames")
    assert (h["frames"][:32 * frm_cap].reshape(-1, 32)[~used] == sentinel).all(), "a frame slot past nframes[s] was written"
    nsec, total = int(e["totals"][0]), int(e["totals"][1]) + int(e["totals"][2])
    np.testing.assert_array_equal(h["sec_stream_id"].view(np.uint64)[:nsec], e["sec_stream_id"], err_msg="sec_stream_id")
    np.testing.assert_array_equal(h["sec_stream"].view(np.uint32)[:nsec], e["sec_stream"], err_msg="sec_stream")
    assert (h["sec_stream_id"].view(np.uint8)[8 * nsec:8 * nstr] == sentinel).all() and \
        (h["sec_stream"].view(np.uint8)[4 * nsec:4 * nstr] == sentinel).all(), "a section record past nsec was written"
    np.testing.assert_array_equal(h["out"][:total], e["out"], err_msg="out")
    assert (h["out"][total:e["data"].size] == sentinel).all(), "out written past the gathered bytes"
    got = e["got_settings"] != 0
    peers, settings = h["peers"][:8 * nconn].view(C.QPACK_PEER), h["settings"][:16 * nconn].view(C.H3_SETTINGS_DTYPE)
    np.testing.assert_array_equal(peers[got], e["peers"][got], err_msg="peers")
    np.testing.assert_array_equal(settings[got], e["settings"][got], err_msg="settings")
    assert (h["peers"][:8 * nconn].reshape(-1, 8)[~got] == sentinel).all() and \
        (h["settings"][:16 * nconn].reshape(-1, 16)[~got] == sentinel).all(), "settings written for a connection that sent none"


def groups(cases):
    """the corpus cases by the call's parameters: {(mfps, flags): [case]}"""
    g = {}
    for c in cases:
        g.setdefault((c["mfps"], c["flags"]), []).append(c)
    return g


def as_conns(cs, order=None):
    """cases as connections of 1, 3, 0, 2 ... streams, in `order`"""
    idx = list(range(len(cs))) if order is None else list(order)
    conns, i, k = [], 0, 0
    while i < len(idx):
        n = (1, 3, 0, 2)[k % 4]
        conns.append([(cs[j]["buf"], cs[j]["st"], cs[j]["cap"]) for j in idx[i:i + n]])
        i, k = i + n, k + 1
    return conns


def batch(conns, mfps=16384, flags=0):
    return M.batch(conns, mfps, flags, arena_fixed=ARENA[0], arena_per_byte=ARENA[1])


@pytest.fixture(scope="module")
def corpus_batches():
    """the model's batches, made once: {(params, order): batch}"""
    out = {}
    for params, cs in groups(K.CASES).items():
        out[params, "in_order"] = batch(as_conns(cs), *params)
        out[params, "shuffled"] = batch(as_conns(cs, np.random.default_rng(5).permutation(len(cs))), *params)
    for flags in (0, M.CLIENT):  # with the connection of two encoder and two control streams
        out[(16384, flags), "connections"] = batch(K.connections(flags), 16384, flags)
    return out


@pytest.mark.parametrize("order", ["in_order", "shuffled", "connections"])
def test_corpus(torch_cuda, corpus_batches, order):
    for (params, o), e in corpus_batches.items():
        if o == order:
            compare(deframe(torch_cuda, e, *params)[0], e)


def test_corpus_literal_expectations(torch_cuda):
    """the GPU against the corpus's own numbers, without the model in between: one connection a stream"""
    for (mfps, flags), cs in groups(K.CASES).items():
        nstr = len(cs)
        lens = [len(c["buf"]) for c in cs]
        e = dict(data=np.frombuffer(b"".join(c["buf"] for c in cs), np.uint8), str_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32),
                 conn_str=np.arange(nstr + 1, dtype=np.uint32), st_in=M.pack_states([c["st"] for c in cs]),
                 frm_first=np.concatenate([[0], np.cumsum([c["cap"] for c in cs])]).astype(np.uint32))
        e["frm_cap"] = int(e["frm_first"][-1])
        h, _ = deframe(torch_cuda, e, mfps, flags)
        frames, st_out = h["frames"].view(C.H3_FRAME_DTYPE), h["st_out"].view(C.H3_STREAM_DTYPE)
        sec_off, first = h["sec_off"].view(np.uint32), h["conn_first"].view(np.uint32)
        for i, c in enumerate(cs):
            assert (int(h["sstatus"][i]), int(h["serr"][i]), int(h["consumed"][i]), int(h["nframes"][i])) == \
                (c["status"], c["err"], c["consumed"], len(c["frames"])), c["name"]
            assert (int(st_out["kind"][i]), int(st_out["phase"][i]), int(st_out["data_left"][i])) == c["out"], c["name"]
            k = int(first[i])
            fs = frames[int(e["frm_first"][i]):int(e["frm_first"][i]) + len(c["frames"])]
            want = [(t, a, k if t == M.HEADERS and x == 0 else x) for t, a, x in c["frames"]]
            assert [(int(f["type"]), int(f["avail"]), int(f["aux"])) for f in fs] == want, c["name"]
            assert int(first[i + 1]) - k == (0 if c["section"] is None else 1), c["name"]
            if c["section"] is not None:
                assert h["out"][int(sec_off[k]):int(sec_off[k + 1])].tobytes() == c["section"], c["name"]
                assert int(h["sec_stream"][k]) == i and int(h["sec_stream_id"][k]) == c["st"]["stream_id"]
            enc = h["out"][int(h["enc_off"].view(np.uint32)[i]):][:int(h["enc_len"].view(np.uint32)[i])].tobytes()
            assert enc == (c["enc"] or b""), c["name"]
            assert int(h["got_settings"][i]) == (0 if c["settings"] is None else 1), c["name"]
            if c["settings"] is not None:
                p, s = h["peers"].view(C.QPACK_PEER)[i], h["settings"].view(C.H3_SETTINGS_DTYPE)[i]
                assert (int(p["max_table_capacity"]), int(p["max_blocked"]), int(s["max_field_section_size"]), int(s["h3_datagram"])) == \
                    c["settings"], c["name"]


HDRS, SET = K.HDRS, K.SET


def busy(i):
    """a busy stream of one of five kinds"""
    return [(HDRS, K.st(stream_id=4 * i), 2), (b"\x02enc%d" % i, K.st(M.K_UNI, stream_id=4 * i + 2), 0),
            (b"\x00" + K.fr(M.SETTINGS, K.vi(1) + K.vi(i)), K.st(M.K_UNI, stream_id=4 * i + 2), 1),
            (K.fr(M.DATA, b"body"), K.st(phase=M.P_DATA, stream_id=4 * i), 1), (b"", K.st(stream_id=4 * i), 0)][i % 5]


@pytest.mark.parametrize("nstr", [255, 256, 257, 513])
def test_gaps_across_the_walk_workgroups_boundary(torch_cuda, nstr):
    """connections with no streams and streams with no bytes between busy ones, the stream count at the walk
    workgroup's boundary: the last streams are busy, so their places depend on every sum before them"""
    rng = np.random.default_rng(nstr)
    streams = [busy(i) if rng.random() < 0.4 or i >= nstr - 3 else (b"", K.st(stream_id=4 * i), 0) for i in range(nstr)]
    conns, i = [], 0
    while i < nstr:
        n = int(rng.choice([0, 0, 1, 2, 5, 40]))
        conns.append(streams[i:i + n])
        i += n
    conns += [[], []]
    e = batch(conns)
    assert e["totals"][0] > 10 and e["totals"][2] > 20 and e["got_settings"].sum() > 5 and (np.diff(e["conn_str"]) == 0).sum() > 5
    compare(deframe(torch_cuda, e)[0], e)


def test_second_level_scan_sums_runs(torch_cuda):
    """262,145 streams are 1,025 walk workgroups: a lane of the one-workgroup scan sums a run of two entries.  All
    streams are empty but a few at the ends of the range and at a workgroup's and a run's boundary."""
    torch = torch_cuda
    nstr = 262145
    at = {0: 0, 255: 1, 256: 0, 511: 1, 512: 0, 131072: 1, 262143: 0, 262144: 0, 262142: 2}
    lens, kinds, cap = np.zeros(nstr, np.int64), np.zeros(nstr, np.uint8), np.zeros(nstr, np.int64)
    for s, k in at.items():
        b = busy(k)
        lens[s], kinds[s], cap[s] = len(b[0]), b[1]["kind"], b[2]
    str_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    data = np.zeros(int(str_off[-1]), np.uint8)
    for s, k in at.items():
        data[int(str_off[s]):int(str_off[s + 1])] = np.frombuffer(busy(k)[0], np.uint8)
    st = np.zeros(nstr, C.H3_STREAM_DTYPE)
    st["kind"], st["stream_id"] = kinds, 4 * np.arange(nstr)
    conn_str = np.array([0, 0, 300, 300, 131073, 262144, nstr], np.uint32)
    frm_first = np.concatenate([[0], np.cumsum(cap)]).astype(np.uint32)
    r = C.h3_deframe(dev(torch, data), dev(torch, str_off), dev(torch, conn_str), dev(torch, frm_first), int(frm_first[-1]),
                     dev(torch, st), arena_fixed=0)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in r.items()}
    secs = sorted(s for s, k in at.items() if k == 0)  # the section streams, in stream order
    sec_len, enc = len(K.SEC), [len(busy(1)[0]) - 1 if at.get(s) == 1 else 0 for s in (255, 511, 131072)]
    assert h["totals"].tolist() == [len(secs), len(secs) * sec_len, sum(enc)]
    assert h["sec_stream"][:len(secs)].tolist() == secs and h["sec_stream_id"][:len(secs)].tolist() == [4 * s for s in secs]
    off = h["sec_off"].view(np.uint32)
    assert off[:len(secs)].tolist() == [sum(enc) + sec_len * k for k in range(len(secs))] and (off[len(secs):] == h["totals"][1] + h["totals"][2]).all()
    assert h["conn_first"].tolist() == [0, 0, 2, 2, 3, 4, 5] and h["enc_off"].view(np.uint32).tolist() == [0, 0, enc[0], enc[0], sum(enc), sum(enc)]
    assert h["enc_len"].tolist() == [0, enc[0], 0, enc[1] + enc[2], 0, 0] and h["got_settings"].tolist() == [0, 0, 0, 0, 1, 0]
    assert int(h["peers"].view(C.QPACK_PEER)["max_table_capacity"][4]) == 2
    assert int(h["nframes"].sum()) == len(secs) + 1 and int(h["consumed"].view(np.uint32).sum()) == data.size and not h["sstatus"].any()
    for k, s in enumerate(secs):
        assert h["out"][int(off[k]):int(off[k + 1])].tobytes() == K.SEC
    st_out = h["st_out"].view(C.H3_STREAM_DTYPE)
    idle = np.ones(nstr, bool)
    idle[list(at)] = False
    assert (h["st_out"].reshape(-1, 32)[idle] == st.view(np.uint8).reshape(-1, 32)[idle]).all() and (st_out["phase"][secs] == M.P_DATA).all()


def test_varints_of_every_width(torch_cuda):
    """all four widths for type and length, non-minimal encodings included, a type above 2^32, and a DATA length above
    2^32 carried over three steps in data_left"""
    torch = torch_cuda
    streams = []
    for tw in (1, 2, 4, 8):
        for lw in (1, 2, 4, 8):
            typ = {1: 0x21, 2: 0x21 + 31 * 9, 4: 0xF0700 + 5, 8: (1 << 40) + 7}[tw]
            streams.append((K.fr(typ, b"p" * 3, tw, lw) + K.fr(0x21, b"q", tw, lw) + K.fr(M.HEADERS, K.SEC, tw, lw), K.st(), 3))
    e = batch([streams[:5], streams[5:]])
    h, _ = deframe(torch, e)
    compare(h, e)
    assert int(e["totals"][0]) == 16 and (e["nframes"] == 3).all() and int(e["frames"]["type"].max()) > 1 << 32
    step = [(K.fr(M.DATA, b"0123", length=(1 << 33) + 5), K.st(phase=M.P_DATA), 1)]
    left = (1 << 33) + 5
    for n, chunk in enumerate([None, b"x" * 7, b"y" * 9]):
        if chunk is not None:
            step = [(chunk, st, 1)]
        e = batch([step])
        h, _ = deframe(torch, e)
        compare(h, e)
        st = {k: (int(h["st_out"].view(C.H3_STREAM_DTYPE)[k][0]) if k != "rsv" else 0) for k in ("stream_id", "data_left", "kind", "phase", "flags", "rsv")}
        left -= 4 if chunk is None else len(chunk)
        assert (st["phase"], st["data_left"]) == (M.P_DATA_PAYLOAD, left) and int(h["frames"].view(C.H3_FRAME_DTYPE)["length"][0]) > 1 << 32


def merged(frames, base):
    """frame records as (type, start, payload start, length, avail, is a section), offsets moved by base; the body bytes
    that continue a DATA frame joined to the record before them"""
    out = []
    for f in frames:
        t, h, p, L, a, x = (int(f[k]) for k in ("type", "hdr_off", "payload_off", "length", "avail", "aux"))
        if t == M.DATA and h == p and out and out[-1][0] == M.DATA and out[-1][2] + out[-1][4] == base + p and out[-1][3] - out[-1][4] == L:
            out[-1] = out[-1][:4] + (out[-1][4] + a, False)
        else:
            out.append((t, base + h, base + p, L, a, t == M.HEADERS and x != M.NOSEC))
    return [f for f in out if not (f[0] == M.DATA and f[1] == f[2] and f[4] == 0)]


def test_resume_at_every_byte(torch_cuda):
    """every corpus stream cut at every position and fed in two steps -- st_out -> st_in, the unconsumed tail in front of
    the rest --: frames, section, encoder bytes and final state equal the one-step result.  (Streams that end out of
    frame slots or with a refused state are left out: every step has the slots anew.  Where the one-step walk stopped
    behind its section, a cut behind that point gives the first step the whole result and the second goes on; those cuts
    compare the first step alone.)"""
    torch = torch_cuda
    for (mfps, flags), cs in groups(K.CASES).items():
        cs = [c for c in cs if c["status"] not in (M.FRAMES, M.EINVAL) and len(c["buf"])]
        pairs = [(c, t) for c in cs for t in range(len(c["buf"]))]
        one = batch([[(c["buf"], c["st"], 16)] for c in cs], mfps, flags)
        h1, _ = deframe(torch, one, mfps, flags)
        compare(h1, one)
        first = batch([[(c["buf"][:t], c["st"], 16)] for c, t in pairs], mfps, flags)
        ha, _ = deframe(torch, first, mfps, flags)
        compare(ha, first)
        sa = ha["st_out"].view(C.H3_STREAM_DTYPE)
        mid = [dict(stream_id=int(s["stream_id"]), data_left=int(s["data_left"]), kind=int(s["kind"]), phase=int(s["phase"]),
                    flags=int(s["flags"]), rsv=0) for s in sa]
        used = ha["consumed"].view(np.uint32)
        second = batch([[(c["buf"][int(used[i]):], mid[i], 16)] for i, (c, t) in enumerate(pairs)], mfps, flags)
        hb, _ = deframe(torch, second, mfps, flags)
        compare(hb, second)
        index = {c["name"]: i for i, c in enumerate(cs)}
        fa, fb, f1 = (x["frames"].view(C.H3_FRAME_DTYPE) for x in (ha, hb, h1))
        for i, (c, t) in enumerate(pairs):
            j = index[c["name"]]
            w1, wa, wb = one["walks"][j], first["walks"][i], second["walks"][i]
            stopped = c["section"] is not None and not c["st"]["flags"] & M.S_WALK_ON
            want = merged(f1[int(one["frm_first"][j]):][:len(w1["frames"])], -int(one["str_off"][j]))
            got = merged(fa[int(first["frm_first"][i]):][:len(wa["frames"])], -int(first["str_off"][i]))
            if stopped and wa["section"] is not None:  # the first step is the whole one-step result
                assert got == want and int(used[i]) == c["consumed"] and int(ha["sstatus"][i]) == c["status"], (c["name"], t)
                continue
            rest = merged(fb[int(second["frm_first"][i]):][:len(wb["frames"])], int(used[i]) - int(second["str_off"][i]))
            if got and rest and rest[0][0] == M.DATA and rest[0][1] == rest[0][2] and got[-1][0] == M.DATA:
                got[-1] = got[-1][:4] + (got[-1][4] + rest[0][4], False)
                rest = rest[1:]
            assert got + rest == want, (c["name"], t)
            assert int(used[i]) + int(hb["consumed"].view(np.uint32)[i]) == c["consumed"], (c["name"], t)
            assert (int(hb["sstatus"][i]), int(hb["serr"][i])) == (c["status"], c["err"]), (c["name"], t)
            sb = hb["st_out"].view(C.H3_STREAM_DTYPE)[i]
            assert (int(sb["kind"]), int(sb["phase"]), int(sb["data_left"])) == c["out"], (c["name"], t)
            sec = [x["out"][int(x["sec_off"].view(np.uint32)[k]):int(x["sec_off"].view(np.uint32)[k + 1])].tobytes()
                   for x, e in ((ha, first), (hb, second)) for k in range(int(e["conn_first"][i]), int(e["conn_first"][i + 1]))]
            assert sec == ([] if c["section"] is None else [c["section"]]), (c["name"], t)
            enc = b"".join(x["out"][int(x["enc_off"].view(np.uint32)[i]):][:int(x["enc_len"].view(np.uint32)[i])].tobytes() for x in (ha, hb))
            assert enc == (c["enc"] or b""), (c["name"], t)
            assert int(ha["got_settings"][i]) + int(hb["got_settings"][i]) == (0 if c["settings"] is None else 1), (c["name"], t)


@pytest.mark.parametrize("fill,sentinel", BH.RUNS)
def test_exact_size_buffers(torch_cuda, corpus_batches, fill, sentinel):
    """every array at exactly its documented size between sentinel zones, the input between zones of the fill byte: the
    guards stay, the write footprint is what compare() allows, and st_out may be st_in"""
    for (params, o), e in corpus_batches.items():
        h, r = deframe(torch_cuda, e, *params, sentinel=sentinel, guard=True, fill=fill)
        compare(h, e, sentinel)
        nsec = int(e["totals"][0])
        assert (h["sec_off"].view(np.uint32)[nsec:] == int(e["totals"][1]) + int(e["totals"][2])).all()
        h2, _ = deframe(torch_cuda, e, *params, sentinel=sentinel, guard=True, alias=True, fill=fill)
        compare(h2, e, sentinel)


LENS = (0, 1, 15, 16, 17, 33)


def gather_streams(encoder):
    """sections (or encoder runs) of every length of LENS at every source and destination offset modulo 16: a filler
    section (run) sets the destination's offset, a discarded stream the source's"""
    rng = np.random.default_rng(21)
    streams, src, dst, seen = [], 0, 0, set()
    head = 0 if encoder else 2  # a HEADERS frame's two header bytes
    unit = (lambda b: (b, K.st(M.K_QPACK_ENCODER), 0)) if encoder else (lambda b: (K.fr(M.HEADERS, b), K.st(), 1))
    for L in LENS:
        for so in range(16):
            for do in range(16):
                pad = (do - dst) % 16
                if pad:
                    streams.append(unit(bytes(rng.integers(0, 256, pad, dtype=np.uint8))))
                    src, dst = src + head + pad, dst + pad
                fill = (so - head - src) % 16
                streams.append((bytes(rng.integers(0, 256, fill, dtype=np.uint8)), K.st(M.K_DISCARD), 0))
                src += fill
                seen.add((L, (src + head) % 16, dst % 16))
                streams.append(unit(bytes(rng.integers(0, 256, L, dtype=np.uint8))))
                src, dst = src + head + L, dst + L
    assert len(seen) == len(LENS) * 256
    return streams


@pytest.mark.parametrize("encoder", [False, True])
def test_gather_edges(torch_cuda, encoder):
    """the last stream's section (run) ends at in + in_size"""
    streams = gather_streams(encoder)
    conns = [streams[i:i + 7] for i in range(0, len(streams), 7)]
    e = batch(conns)
    assert int(e["totals"][2 if encoder else 1]) > 20000 and int(e["totals"][1 if encoder else 2]) == 0
    for fill, sentinel in BH.RUNS:
        h, r = deframe(torch_cuda, e, sentinel=sentinel, guard=True, fill=fill)
        assert r["out"].data_ptr() % 16 == 0
        compare(h, e, sentinel)


def hostile_streams(seed, n):
    """seeded random bytes and mutated corpus streams under states of every kind and phase"""
    rng = np.random.default_rng(seed)
    states = [K.st(k, p) for k, ps in ((M.K_REQUEST, (0, 1, 3)), (M.K_UNI, (0,)), (M.K_CONTROL, (0, 1)), (M.K_QPACK_ENCODER, (0,)),
                                       (M.K_QPACK_DECODER, (0,)), (M.K_DISCARD, (0,))) for p in ps] + [K.st(phase=2, data_left=9), K.st(7)]
    small = [c for c in K.CASES if len(c["buf"]) < 200]
    streams = []
    for i in range(n):
        st = dict(states[int(rng.integers(len(states)))], flags=int(rng.integers(0, 8)), stream_id=int(rng.integers(0, 1 << 62)))
        if rng.random() < 0.5:
            b = bytearray(small[int(rng.integers(len(small)))]["buf"])
            for _ in range(int(rng.integers(0, 3))):
                if b:
                    b[int(rng.integers(len(b)))] ^= int(rng.integers(1, 256))
        else:
            b = bytearray(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes())
            if len(b) > 2 and rng.random() < 0.7:  # a plausible header in front
                b[0], b[1] = int(rng.choice([0, 1, 3, 4, 5, 7, 13, 0x21])), int(rng.integers(0, len(b)))
        streams.append((bytes(b), st, int(rng.integers(0, 6))))
    return streams


@pytest.mark.parametrize("flags", [0, M.CLIENT])
def test_hostile_input(torch_cuda, flags):
    streams = hostile_streams(100 + flags, 1500)
    conns = [streams[i:i + 5] for i in range(0, len(streams), 5)]
    for mfps in (16384, 12):
        e = batch(conns, mfps, flags)
        assert len(set(e["sstatus"].tolist())) >= 6
        compare(deframe(torch_cuda, e, mfps, flags, guard=True)[0], e)


def test_offsets_that_are_no_running_sums(torch_cuda):
    """str_off, conn_str and frm_first with entries that fall back, overlap and point past the arrays: the ranges are
    clamped as (2l) says, the guards stay, every status is one the call reports, and nothing past the slots is written"""
    streams = hostile_streams(7, 600)
    e = batch([streams[i:i + 4] for i in range(0, 600, 4)])
    rng = np.random.default_rng(8)
    for name, top in (("str_off", e["data"].size), ("conn_str", 600), ("frm_first", e["frm_cap"])):
        a = e[name].astype(np.int64)
        hit = rng.random(a.size) < 0.15
        a[hit] = rng.choice([0, top // 2, top, top + 1, 0xFFFFFFFF, 1 << 31], int(hit.sum()))
        a[-1] = e[name][-1]
        e[name] = a.astype(np.uint32)
    h, _ = deframe(torch_cuda, e, guard=True)
    assert set(h["sstatus"].tolist()) <= set(M.ALL_STATUS)
    nsec = int(h["totals"][0])
    assert nsec <= 600 and (h["nframes"].view(np.uint32) <= 5).all() and (h["consumed"].view(np.uint32) <= e["data"].size).all()
    assert (h["sec_stream"][:nsec] < 600).all()


def test_closed_loop_responses(torch_cuda):
    """hhuff_qpack_flatten_responses' frames, one response a request stream -> the client's de-framer ->
    hhuff_qpack_parse_responses on its outputs as they are, enqueued behind it before anything synchronises: every
    field back"""
    import test_qpenc_dyn as QD

    torch = torch_cuda
    q = HE.to_qpack(HE.make_session(300, seed=61, big_frac=0.01, dont_compress_frac=0.1)[0], seed=61, dfid_frac=0.2, odd_status_frac=0.0)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()  # noqa: E731
    n = int(q["res"].size)
    f = C.qpack_flatten_responses(d(q["data"]), d(q["hdr"].view(np.uint8)), d(q["res"].view(np.uint8)), n, d(q["out_off"].view(np.int64)),
                                  q["server_off"], q["server_len"], in_size=int(q["data"].size))
    torch.cuda.synchronize()
    assert (f["rstatus"].cpu().numpy()[:n] == 0).all()
    out, out_len = f["out"].cpu().numpy(), f["out_len"].cpu().numpy().view(np.uint32)
    frames = [out[int(o):int(o) + int(L)].tobytes() for o, L in zip(q["out_off"], out_len[:n])]
    rng = np.random.default_rng(3)
    conns, i = [], 0
    while i < n:  # a connection's responses on its request streams, a DATA frame behind some
        k = int(rng.integers(0, 5))
        conns.append([(frames[j] + (K.fr(M.DATA, b"body") if j % 3 == 0 else b""), K.st(stream_id=4 * j), 1) for j in range(i, min(n, i + k))])
        if len(conns) % 9 == 0:  # a stream whose HEADERS frame has not arrived whole: no section
            conns[-1].insert(len(conns[-1]) // 2, (frames[i][:3], K.st(stream_id=4 * n), 1))
        i += k
    conns[-1].append((b"", K.st(stream_id=4 * n + 4), 1))
    e = batch(conns, 1 << 20, M.CLIENT)
    nconn, in_size, nstr = len(conns), int(e["data"].size), int(e["str_off"].size) - 1
    assert nstr > n + 5  # the decoder is given nstr, an upper bound of the section count it is not told

    def decode(r):
        """the decoder's outputs sized from in_size and the stream count alone: no size is read back"""
        i32 = lambda k: torch.empty(max(1, k), dtype=torch.int32, device="cuda")  # noqa: E731
        i64 = lambda k: torch.empty(max(1, k), dtype=torch.int64, device="cuda")  # noqa: E731
        u8 = lambda k: torch.empty(max(1, k), dtype=torch.uint8, device="cuda")  # noqa: E731
        dd = dict(arena=u8(ARENA[0] * nstr + ARENA[1] * in_size + 16), name_off=i32(in_size), name_len=i32(in_size), value_off=i32(in_size),
                  value_len=i32(in_size), fflags=u8(in_size), nfields=i32(nstr), sstatus=i32(nstr), req_insert_count=i64(nstr),
                  enc_status=i32(nconn), enc_consumed=i32(nconn), insert_count=i64(nconn), res=u8(nstr * C.QRES_BYTES))
        L = C.lib()
        scratch = u8(max(16, int(L.hhuff_qpack_scratch_size(nconn, 4096))))
        p = lambda t: t.data_ptr()  # noqa: E731
        rc = L.hhuff_qpack_parse_responses(p(r["out"]), in_size, p(r["enc_off"]), p(r["enc_len"]), p(r["sec_off"]), p(r["conn_first"]), nconn,
                                           nstr, 4096, 100, None, p(dd["arena"]), p(r["arena_off"]), p(dd["name_off"]), p(dd["name_len"]),
                                           p(dd["value_off"]), p(dd["value_len"]), p(dd["fflags"]), p(dd["nfields"]), p(dd["sstatus"]),
                                           p(dd["req_insert_count"]), p(dd["enc_status"]), p(dd["enc_consumed"]), p(dd["insert_count"]),
                                           p(r["sec_stream_id"]), p(dd["res"]), p(scratch), scratch.numel(), 0,
                                           torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        return dd
    h, r = deframe(torch, e, 1 << 20, M.CLIENT, then=decode)
    compare(h, e)
    assert h["totals"].tolist()[::2] == [n, 0] and not h["sstatus"].any()
    dd = {k: v.cpu().numpy() for k, v in r["then"].items()}
    assert (dd["sstatus"][:n] == 0).all()
    off, a = h["sec_off"].view(np.uint32), dd["arena"]
    for k in range(n):
        s0 = int(off[k])
        got = [(a[int(dd["name_off"][x]):int(dd["name_off"][x]) + int(dd["name_len"][x])].tobytes(),
                a[int(dd["value_off"][x]):int(dd["value_off"][x]) + int(dd["value_len"][x])].tobytes())
               for x in range(s0, s0 + int(dd["nfields"][k]))]
        assert got == QD.fields_of(q, k), k


def test_closed_loop_settings_to_the_peers_call(torch_cuda):
    """SETTINGS frames on 65 connections' control streams -> the de-framer's peers array, as it is and enqueued behind it,
    -> hhuff_qpack_flatten_sessions_peers: every output equals the call with the same records made on the host"""
    import test_qpenc_peers as QP

    torch = torch_cuda
    peers = QP.mixed_population()
    conns = [[(b"\x00" + K.fr(M.SETTINGS, K.vi(7) + K.vi(int(p["max_blocked"])) + K.vi(1) + K.vi(int(p["max_table_capacity"]))),
               K.st(M.K_UNI, stream_id=2), 1), (HDRS, K.st(stream_id=0), 1)] for p in peers]
    e = batch(conns)
    q = QP.turnover(65, 1, 97)[0]
    host = QP.PGpu(torch, 65, 4096, 100, peers=peers).step(q, None, QP.SETCAP | QP.EV)
    g, real = QP.Gpu(torch, 65, 4096, 100), C.qpack_flatten_sessions

    def encode(r):
        C.qpack_flatten_sessions = lambda *a, **k: real(*a, evict=True, peers=r["peers"], **k)
        try:
            return g.step(q, None, QP.SETCAP | QP.EV)
        finally:
            C.qpack_flatten_sessions = real
    h, r = deframe(torch, e, then=encode)
    compare(h, e)
    assert h["got_settings"].all()
    np.testing.assert_array_equal(h["peers"].view(C.QPACK_PEER), peers)
    QP.same(r["then"], host, "peers from the de-framer against peers from the host: ")


def test_closed_loop_sessions(torch_cuda, oracle_codec):
    """hhuff_qpack_flatten_sessions' encoder streams (behind a 0x02 type byte in the first step, on the open encoder stream
    afterwards) and its request frames, a DATA frame behind every other one -> the server's de-framer ->
    hhuff_qpack_parse_requests_sessions on the de-framer's device tensors as they are (the Python wrapper reads one offset
    back to size its outputs; nothing is copied or rebuilt between the two calls) -> its decoder stream, device to
    device, into the encoder sessions' next step.  Three steps: the inserts of step 1 arrive with step 2's, so sections
    park and are presented again as HEADERS frames on their streams.  Every field of every section comes back."""
    import test_qpdec_sessions as QT
    import test_qpenc_dyn as QD

    torch, nconn, real = torch_cuda, 60, C.qpack_decode
    g = QT.Gpu(torch, nconn, 100, responses=False)
    state = dict(scratch=None, due={}, fields=0, parked=0)

    def encode(s, q, dec):
        flags = C.QENC_CONTINUE if s else C.QENC_SET_CAPACITY
        r, state["scratch"] = QT.encoder_step(torch, q, state["scratch"], dec and dec["t"], flags)
        if dec:  # the decoder stream of the step before is consumed whole
            np.testing.assert_array_equal(r["dec_consumed"], dec["len"])
        for c in range(nconn):
            for k in range(int(q["conn_first"][c]), int(q["conn_first"][c + 1])):
                state["due"][(c, int(q["stream_id"][k]))] = QD.fields_of(q, k)
        return r

    def decode(s, st, sid):
        cf, data = st["conn_first"], st["data"]
        nsec = int(cf[-1])
        conns = []
        for c in range(nconn):
            enc = data[int(st["enc_off"][c]):int(st["enc_off"][c]) + int(st["enc_len"][c])].tobytes()
            streams = [(b"\x02" + enc, K.st(M.K_UNI, stream_id=2), 0) if s == 0 else (enc, K.st(M.K_QPACK_ENCODER, stream_id=2), 0)]
            for k in range(int(cf[c]), int(cf[c + 1])):
                sec = data[int(st["sec_off"][k]):int(st["sec_off"][k + 1])].tobytes()
                streams.append((K.fr(M.HEADERS, sec) + (K.fr(M.DATA, b"body") if k % 2 else b""), K.st(stream_id=int(sid[k])), 1))
            conns.append(streams)
        e = batch(conns, 1 << 20)
        in_size = int(e["data"].size)

        def then(r):
            def on_the_deframers_tensors(_data, _enc_off, _enc_len, _sec_off, _conn_first, n, *a, **k):
                k.update(in_size=in_size, stream_id=r["sec_stream_id"])
                return real(r["out"], r["enc_off"], r["enc_len"], r["sec_off"], r["conn_first"], n, *a, **k)
            C.qpack_decode = on_the_deframers_tensors
            try:
                return g.step(st, sid, cont=s > 0)
            finally:
                C.qpack_decode = real
        h, r = deframe(torch, e, 1 << 20, then=then)
        compare(h, e)
        d = r["then"]
        assert int(h["totals"][0]) == nsec and not h["sstatus"].any() and d["guards_intact"]
        np.testing.assert_array_equal(h["sec_stream_id"].view(np.uint64)[:nsec], np.asarray(sid, np.uint64)[:nsec])
        np.testing.assert_array_equal(h["enc_len"].view(np.uint32)[:nconn], st["enc_len"])
        off, raw = h["sec_off"].view(np.uint32), d["raw"]
        a = raw["arena"]
        for c in range(nconn):
            for k in range(int(cf[c]), int(cf[c + 1])):
                if d["sstatus"][k] == QT.BLOCKED:
                    state["parked"] += 1
                    continue
                s0 = int(off[k])
                got = [(a[int(raw["name_off"][f]):int(raw["name_off"][f]) + int(raw["name_len"][f])].tobytes(),
                        a[int(raw["value_off"][f]):int(raw["value_off"][f]) + int(raw["value_len"][f])].tobytes())
                       for f in range(s0, s0 + int(raw["nfields"].view(np.uint32)[k]))]
                assert got == state["due"].pop((c, int(sid[k]))), (s, c, k)
                state["fields"] += len(got)
        t = d["t"]
        return dict(t=(t["dec_out"], t["dec_out_off"], t["dec_out_len"]), host=d["dec"], len=d["dec_out_len"]), d

    QT.closed_loop(nconn, True, encode, decode, lambda dec: None)
    assert not state["due"] and state["fields"] > 6 * nconn and state["parked"] >= nconn
