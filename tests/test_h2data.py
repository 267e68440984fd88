"""HTTP/2 DATA frames on the send side on the GPU (include/hhuff.h (2k''), h2o_amd/csrc/hhuff_h2data.hip) against the
frame-by-frame model (h2data_model.py): every output -- the frames' bytes, sent, out_len, peers_out, cstatus -- is
compared, and what the call may not write still holds its sentinel.  The hand-built corpus and the cases of
golden/h2data.npz (h2o's own frames) in order and shuffled;
every alignment of source and destination; headers at every residue of a line; workgroup edges; exact-size guarded
buffers; hostile records, peers, send_first and out_off; steps with the peers in place and hhuff_h2_control between;
max_frames visits; one large record over the whole device; and the closed loops framer -> de-framer -> control and
SETTINGS -> control -> framer."""
import numpy as np
import pytest

import bounds_harness as BH
import h2data_corpora as K
import h2data_model as M
from conftest import load_golden
from h2o_amd import codec as C

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


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
    return torch.from_numpy(a.copy()).cuda()


def body_of(n, seed=1):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def frame_data(torch, e, sentinel=SENTINEL, guard=False, in_place=False):
    """hhuff_h2_frame_data on the model's batch e, every output of exactly its documented size and filled with the
    sentinel (guard: between two guard zones, which are checked): -> numpy arrays"""
    nconn, nsend, out_size = e["send_first"].size - 1, e["nsend"], e["out_size"]
    body = dev(torch, e["body"] if e["body"].size else np.zeros(1, np.uint8))
    sizes = dict(sent=24 * nsend, out_len=4 * nconn, cstatus=4 * nconn, out=out_size, peers=40 * nconn)
    whole, out = {}, {}
    for k, n in sizes.items():
        if n == 0:  # (no such array: the wrapper passes a dummy)
            continue
        if guard:
            whole[k], inner = BH.guarded(torch, n, sentinel)
        else:
            inner = torch.full((n,), sentinel, dtype=torch.uint8, device="cuda")
        out[k] = inner.view(torch.int32) if k in ("out_len", "cstatus") else inner
    peers_in = dev(torch, e["peers_in"].view(np.uint8))
    if in_place:
        out["peers"] = peers_in
        whole.pop("peers", None)
    sends = dev(torch, e["sends"].view(np.uint8) if e["sends"].size else np.zeros(24, np.uint8))
    r = C.h2_frame_data(body, sends, dev(torch, e["send_first"]), peers_in, dev(torch, e["out_off"]), body_size=int(e["body"].size),
                        nsend=nsend, out_size=out_size, out=out)
    torch.cuda.synchronize()
    for k, w in whole.items():
        w = w.cpu().numpy()
        n = w.size - 2 * BH.GUARD
        assert (w[:BH.GUARD] == sentinel).all() and (w[BH.GUARD + n:] == sentinel).all(), "guard of " + k
    h = {k: r[k].cpu().numpy() for k in sizes}
    if not in_place:
        np.testing.assert_array_equal(peers_in.cpu().numpy(), e["peers_in"].view(np.uint8), err_msg="peers_in written")
    return h


def compare(h, e, sentinel=SENTINEL):
    """every output array against the model's; what the call may not write still holds the sentinel"""
    nconn, nsend, out_size = e["send_first"].size - 1, e["nsend"], e["out_size"]
    np.testing.assert_array_equal(h["cstatus"][:nconn], e["cstatus"], err_msg="cstatus")
    np.testing.assert_array_equal(h["out_len"][:nconn].view(np.uint32), e["out_len"], err_msg="out_len")
    np.testing.assert_array_equal(h["peers"][:40 * nconn].view(C.H2_PEER_DTYPE), e["peers_out"], err_msg="peers_out")
    sent, used = h["sent"][:24 * nsend].view(C.H2_SENT_DTYPE), e["sent_used"][:nsend]
    np.testing.assert_array_equal(sent[used], e["sent"][:nsend][used], err_msg="sent")
    assert (h["sent"][:24 * nsend].reshape(-1, 24)[~used] == sentinel).all(), "a record that was not served was written"
    out = h["out"][:out_size]
    bad = np.flatnonzero(out != e["out"])
    assert bad.size == 0, "out differs at %s (%d bytes): got %s, want %s; written behind out_len: %s" % (
        bad[:8], bad.size, out[bad[:8]], e["out"][bad[:8]], bool((~e["out_used"][bad]).any()))


def run(torch, e, **kw):
    compare(frame_data(torch, e, **kw), e)
    return e


# ---------------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------------
def corpus_batch(order):
    cases = [K.CASES[i] for i in order]
    return M.batch(K.BODY, [c["sends"] for c in cases], [(c["m"], c["window"]) for c in cases], rooms=[c["room"] for c in cases])


@pytest.mark.parametrize("order", ("listed", "reversed", "shuffled"))
def test_corpus_connections(torch_cuda, order):
    idx = list(range(len(K.CASES)))
    idx = {"listed": idx, "reversed": idx[::-1], "shuffled": list(np.random.default_rng(5).permutation(len(idx)))}[order]
    e = run(torch_cuda, corpus_batch(idx), guard=True)
    # the literal expectations, not only the model's
    for c, i in enumerate(idx):
        k = K.CASES[i]
        assert int(e["cstatus"][c]) == k["status"] and int(e["out_len"][c]) == k["out_len"]
        assert int(e["peers_out"]["send_window"][c]) == k["after"]


@pytest.fixture(scope="module")
def fixture_batches():
    """golden/h2data.npz's cases (h2o's own frames), one connection each, in the file's order and shuffled: the
    model's batches, made once"""
    fx = load_golden("h2data")
    n = fx["cases"].shape[0]
    body = body_of(int(fx["cases"][:, 4].max()) + 64, 15)
    out = {}
    for order in ("listed", "shuffled"):
        idx = np.arange(n) if order == "listed" else np.random.default_rng(6).permutation(n)
        rows = [[int(v) for v in fx["cases"][i]] for i in idx]
        conns = [[M.send_rec((13 * int(i)) % 64, L, 1, Ws, flags, maxf)] for i, (m, R, Wc, Ws, L, flags, maxf) in zip(idx, rows)]
        out[order] = (fx, idx, M.batch(body, conns, [(r[0], r[2]) for r in rows], rooms=[r[1] for r in rows]))
    return out


@pytest.mark.parametrize("order", ("listed", "shuffled"))
def test_fixture_connections(torch_cuda, fixture_batches, order):
    fx, idx, e = fixture_batches[order]
    h = frame_data(torch_cuda, e)
    compare(h, e)
    # h2o's own answers, not only the model's: the frame count, every header, both windows
    sent = h["sent"].view(C.H2_SENT_DTYPE)
    np.testing.assert_array_equal(sent["nframes"], fx["nframes"][idx])
    np.testing.assert_array_equal(h["peers"].view(C.H2_PEER_DTYPE)["send_window"], fx["after"][idx, 0])
    np.testing.assert_array_equal(sent["window"], fx["after"][idx, 1])
    for c, i in enumerate(idx):
        want = fx["headers"][9 * int(fx["frame_off"][i]):9 * int(fx["frame_off"][i + 1])].reshape(-1, 9)
        pos = int(e["out_off"][c])
        for w in want:
            assert bytes(h["out"][pos:pos + 9]) == bytes(w), (c, i)
            pos += 9 + int.from_bytes(bytes(w[:3]), "big")
        assert pos == int(e["out_off"][c]) + int(h["out_len"].view(np.uint32)[c])


# ---------------------------------------------------------------------------------------------------
# alignments
# ---------------------------------------------------------------------------------------------------
def test_every_alignment_of_source_and_region(torch_cuda):
    """all 256 pairs of body_off mod 16 x region start mod 16, payloads of 1..40 bytes cut by the stream's window"""
    body = body_of(16 * 300 + 64)
    conns, rooms, at = [], [], 0
    for i in range(256):
        a, b = i % 16, i // 16
        n = 1 + (i * 7) % 40
        conns.append([M.send_rec(16 * i + a, 50, 2 * i + 1, n, M.FINAL)])
        nxt = i + 1
        want = (nxt // 16) % 16 if nxt < 256 else 0  # the next region's start modulo 16
        room = n + 9
        room += (want - (at + room)) % 16
        rooms.append(room)
        assert at % 16 == b
        at += room
    e = run(torch_cuda, M.batch(body, conns, [(16384, 1 << 20)] * 256, rooms=rooms), guard=True)
    assert e["sent"]["sent"].tolist() == [1 + (i * 7) % 40 for i in range(256)] and (e["sent"]["flags"] == M.STREAM_WINDOW).all()


@pytest.mark.parametrize("m", (16384, 16385))
def test_headers_at_every_residue_of_a_line(torch_cuda, m):
    """17 full frames: (m + 9) mod 16 is 9 or 10, so consecutive headers start at many residues of a 16-byte line --
    at all 16 for m = 16384 -- and at m = 16385 the source's shift against the destination changes from frame to frame"""
    body = body_of(17 * m + 3, 2)
    e = M.batch(body, [[M.send_rec(3, 17 * m, 5, 1 << 30, M.FINAL)]], [(m, 1 << 30)], rooms=[17 * (m + 9) + 10])
    if m == 16384:
        assert {(k * (m + 9)) % 16 for k in range(17)} == set(range(16))
    run(torch_cuda, e, guard=True)
    assert list(e["sent"][0].tolist()[:2]) == [17 * m, 17] and e["frames"][0] == [(m, 0)] * 16 + [(m, 1)]


# ---------------------------------------------------------------------------------------------------
# workgroup edges
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nconn", (1, 255, 256, 257, 513))
def test_workgroup_edges(torch_cuda, nconn):
    """connections with 0, 1 and 300 records around the walk's workgroups of 256; records without a frame (a stream
    window of 0, an empty body in progress) between records with frames"""
    body = body_of(5000, 3)
    conns = []
    for c in range(nconn):
        if c % 3 == 0 and nconn > 1:
            conns.append([])
        elif c in (1, 256, nconn - 1) or nconn == 1:
            conns.append([M.send_rec((7 * i) % 4000, (i * 5) % 23 if i % 4 else 0, 2 * i + 1, 0 if i % 5 == 2 else 100, M.FINAL if i % 2 else 0)
                          for i in range(300)])
        else:
            conns.append([M.send_rec(c, 1 + c % 30, 1, 100, M.FINAL)])
    e = run(torch_cuda, M.batch(body, conns, [(16384, 1 << 20)] * nconn), guard=True)
    c = 1 if nconn > 1 else 0  # a connection of 300 records
    k = e["sent"]["nframes"][int(e["send_first"][c]):int(e["send_first"][c + 1])]
    assert k.size == 300 and 0 in k[1:-1].tolist() and k.sum() > 100


# ---------------------------------------------------------------------------------------------------
# guarded buffers
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", (0, 1, 9))
def test_regions_of_exactly_the_bytes_owed(torch_cuda, short):
    """every region is exactly its frames' bytes, or one or nine bytes less: the last frame shrinks or vanishes as the
    model says, no guard and no neighbour's byte is touched, and the bytes behind out_len keep the sentinel"""
    body = body_of(40000, 4)
    conns = [[M.send_rec(1, 20, 1, 100, 0), M.send_rec(30, 5, 3, 100, M.FINAL)],
             [M.send_rec(100, 16384 + 7, 1, 1 << 20, M.FINAL)],
             [M.send_rec(7, 3, 1, 100, M.FINAL)],
             [M.send_rec(50, 33, 7, 100, M.FINAL), M.send_rec(90, 12, 9, 100, M.FINAL)]]
    owed = [29 + 14, 16384 + 9 + 7 + 9, 12, 42 + 21]
    e = M.batch(body, conns, [(16384, 1 << 20)] * 4, rooms=[n - short for n in owed])
    run(torch_cuda, e, guard=True)
    last = [int(e["sent"]["sent"][i]) for i in (1, 2, 3, 5)]
    assert last == {0: [5, 16391, 3, 12], 1: [4, 16390, 2, 11], 9: [0, 16384, 0, 3]}[short]
    assert e["out_used"].sum() == sum(owed) - {0: 0, 1: 4, 9: 14 + 7 + 12 + 9 + 9}[short]


# ---------------------------------------------------------------------------------------------------
# hostile input
# ---------------------------------------------------------------------------------------------------
def test_hostile_records(torch_cuda):
    """body ranges that leave the body or wrap, stream ids 0 and above 2^31 - 1, unknown flags: HHUFF_H2D_EINVAL, the
    earlier records written, nothing for the record and those behind it"""
    body = body_of(1000, 6)
    ok = M.send_rec(10, 20, 1, 100, M.FINAL)
    bad = [M.send_rec(990, 11, 1), M.send_rec(1001, 0, 1), M.send_rec(0xFFFFFFFF, 2, 1), M.send_rec(5, 0xFFFFFFFF, 1),
           M.send_rec(0, 1, 0), M.send_rec(0, 1, 0x80000000), M.send_rec(0, 1, 0xFFFFFFFF), M.send_rec(0, 1, 1, 100, 4),
           M.send_rec(0, 1, 1, 100, 0x80000001)]
    conns = [[ok, b, ok] for b in bad] + [[b] for b in bad] + [[ok, M.send_rec(1000, 0, 3, 100, M.FINAL), M.send_rec(990, 10, 5, 100)]]
    e = run(torch_cuda, M.batch(body, conns, [(16384, 65535)] * len(conns), rooms=[100] * len(conns)), guard=True)
    assert e["cstatus"].tolist() == [M.EINVAL] * (2 * len(bad)) + [0]
    assert e["out_len"].tolist() == [29] * len(bad) + [0] * len(bad) + [29 + 9 + 19]
    assert e["sent_used"].sum() == len(bad) + 3


def test_hostile_peers(torch_cuda):
    body = body_of(40000, 7)
    rec = [M.send_rec(0, 20000, 1, 1 << 20, M.FINAL)]
    frame_sizes = (0, 1, 16383, 16384, 16777215, 16777216, 0xFFFFFFFF)
    windows = (65535, -(1 << 62), (1 << 62), 0, 1, -1, 65535)
    e = run(torch_cuda, M.batch(body, [rec] * 7, list(zip(frame_sizes, windows)), rooms=[30000] * 7), guard=True)
    assert e["cstatus"].tolist() == [M.EINVAL] * 3 + [0, 0] + [M.EINVAL] * 2
    assert e["out_len"].tolist() == [0, 0, 0, 0, 10, 0, 0]
    assert e["peers_out"]["send_window"].tolist() == [65535, -(1 << 62), (1 << 62), 0, 0, -1, 65535]


def test_hostile_send_first(torch_cuda):
    """a send_first that is no running sum is clamped to nsend as (2k') clamps frm_first; no record outside
    sends[0 .. nsend) is read, none outside sent[0 .. nsend) written"""
    body = body_of(100, 8)
    recs = [M.send_rec(i, 10, 2 * i + 1, 100, M.FINAL) for i in range(4)]
    for send_first in ([2, 4, 0, 2, 2], [0, 0xFFFFFFFF, 0xFFFFFFFF, 2, 0], [4, 4, 9, 3, 4], [0xFFFFFFFF, 0, 0, 0, 0]):
        e = M.batch(body, [recs], [(16384, 65535)] * 4, rooms=[50] * 4, send_first=send_first, nsend=4)
        run(torch_cuda, e, guard=True)
    assert e["out_len"].tolist() == [0, 0, 0, 0]
    e = M.batch(body, [recs], [(16384, 65535)] * 4, rooms=[50] * 4, send_first=[2, 4, 0, 2, 2], nsend=4)
    assert e["out_len"].tolist() == [38, 0, 38, 0] and e["sent_used"].all()


def test_hostile_out_off(torch_cuda):
    """an out_off that is no running sum is clamped to out_size as (2k') clamps rep_off: nothing outside `out`"""
    body = body_of(100, 9)
    conns = [[M.send_rec(0, 21, 1, 100, M.FINAL)], [M.send_rec(30, 5, 3, 100, M.FINAL)], [M.send_rec(40, 31, 5, 100, M.FINAL)]]
    peers = [(16384, 65535)] * 3
    e = run(torch_cuda, M.batch(body, conns, peers, out_off=[0, 60, 40, 0xFFFFFFFF], out_size=100), guard=True)
    assert e["out_len"].tolist() == [30, 0, 40] and e["sent"]["flags"].tolist() == [3, M.ROOM, 3]
    assert e["sent"]["out_off"].tolist() == [0, 60, 40]
    e = run(torch_cuda, M.batch(body, conns, peers, out_off=[0xFFFFFFFF, 200, 100, 70], out_size=100), guard=True)
    assert e["out_len"].tolist() == [0, 0, 0] and e["sent"]["out_off"].tolist() == [100, 100, 100]
    e = run(torch_cuda, M.batch(body, conns, peers, out_off=[90, 120, 5, 5], out_size=100), guard=True)
    assert e["out_len"].tolist() == [10, 0, 0] and e["sent"]["sent"].tolist() == [1, 0, 0]


# ---------------------------------------------------------------------------------------------------
# steps
# ---------------------------------------------------------------------------------------------------
def control_bytes(torch, peers, conns_bytes):
    """the control frames of each connection through hhuff_h2_deframe and hhuff_h2_control, the peers in place"""
    data = np.frombuffer(b"".join(conns_bytes), np.uint8)
    in_off = np.cumsum([0] + [len(b) for b in conns_bytes]).astype(np.uint32)
    caps = [len(M.split_frames(b)) for b in conns_bytes]
    frm_first = np.cumsum([0] + caps).astype(np.uint32)
    frm_cap = int(frm_first[-1])
    d_data, d_first = dev(torch, data), dev(torch, frm_first)
    d = C.h2_deframe(d_data, dev(torch, in_off), d_first, frm_cap, max_frame_size=16777215)
    rep_off = (17 * frm_first).astype(np.uint32)
    r = C.h2_control(d_data, d["frames"], d["nframes"], d_first, frm_cap, peers, dev(torch, rep_off), recv_window_size=0,
                     rep_size=int(rep_off[-1]), out={"peers": peers})
    torch.cuda.synchronize()
    assert (r["cstatus"].cpu().numpy() == 0).all() and (d["cstatus"].cpu().numpy() == 0).all()
    return d, r


def frame(typ, flags, stream_id, payload):
    return len(payload).to_bytes(3, "big") + bytes([typ, flags]) + stream_id.to_bytes(4, "big") + payload


def test_three_steps_with_the_peers_in_place(torch_cuda):
    """the windows run dry; hhuff_h2_control applies a WINDOW_UPDATE on stream 0; the next step continues from sent"""
    torch = torch_cuda
    body = body_of(200000, 10)
    lens = [100000, 70000]
    peers = [(16384, 65535), (16384, 65535)]
    conns = [[M.send_rec(0, lens[0], 1, 1 << 20, M.FINAL)], [M.send_rec(100000, lens[1], 3, 1 << 20, M.FINAL)]]
    e1 = M.batch(body, conns, peers)
    h1 = frame_data(torch, e1)
    compare(h1, e1)
    assert e1["sent"]["sent"].tolist() == [65535, 65535] and (e1["sent"]["flags"] == M.CONN_WINDOW).all()
    assert e1["peers_out"]["send_window"].tolist() == [0, 0]
    d_peers = dev(torch, h1["peers"])
    control_bytes(torch, d_peers, [frame(8, 0, 0, (50000).to_bytes(4, "big")), frame(8, 0, 0, (1000).to_bytes(4, "big"))])
    after = d_peers.cpu().numpy().view(C.H2_PEER_DTYPE)
    assert after["send_window"].tolist() == [50000, 1000]
    # the next step continues from sent, in place
    conns2 = [[M.send_rec(int(s[0] + t["sent"]), int(s[1] - t["sent"]), s[2], int(t["window"]), M.FINAL)]
              for (s,), t in zip(conns, e1["sent"])]
    e2 = M.batch(body, conns2, [(16384, 50000), (16384, 1000)])
    e2["peers_in"] = after.copy()
    h2 = frame_data(torch, e2, in_place=True)
    compare(h2, e2)
    assert e2["sent"]["sent"].tolist() == [34465, 1000] and e2["sent"]["flags"].tolist() == [M.DONE | M.END_STREAM, M.CONN_WINDOW]
    assert e2["peers_out"]["send_window"].tolist() == [15535, 0]


def test_max_frames_visits_interleave_three_streams(torch_cuda):
    """one frame a visit, round robin over three streams as h2o's scheduler does among equals: the model makes one call
    of h2o_http2_stream_send_pending_data per record"""
    body = body_of(120000, 11)
    left = {1: [0, 50000], 3: [50000, 20000], 5: [70000, 40000]}
    win = {1: 1 << 20, 3: 17000, 5: 1 << 20}
    recs, conn = [], M.new_conn(16384, 100000, 1 << 30)
    for _ in range(4):
        for sid in (1, 3, 5):
            off, n = left[sid]
            recs.append(M.send_rec(off, n, sid, win[sid], M.FINAL, 1))
            got, k, fl, w = M.visit(conn, body[off:off + n], sid, win[sid], M.FINAL, 1)
            assert k <= 1
            left[sid], win[sid] = [off + got, n - got], w
    e = run(torch_cuda, M.batch(body, [recs], [(16384, 100000)]), guard=True)
    assert bytes(e["out"][:int(e["out_len"][0])]) == bytes(conn["buf"])
    order = [(f[3], f[0]) for f in M.split_frames(bytes(conn["buf"]))]
    assert order[:7] == [(1, 16384), (3, 16384), (5, 16384), (1, 16384), (3, 616), (5, 16384), (1, 16384)]
    assert set(e["sent"]["flags"].tolist()) >= {M.MAX_FRAMES, M.STREAM_WINDOW, M.CONN_WINDOW}


@pytest.mark.parametrize("m", (16384, 16777215))
def test_one_large_record_is_right_to_the_byte(torch_cuda, m):
    """8 MiB in one record: its lines are dealt over the whole grid by position"""
    n = 8 << 20
    body = body_of(n + 5, 12)
    e = M.batch(body, [[M.send_rec(5, n, 0x7FFFFFFF, 1 << 30, M.FINAL)]], [(m, 1 << 30)])
    run(torch_cuda, e)
    assert int(e["sent"]["nframes"][0]) == -(-n // m) and int(e["out_len"][0]) == n + 9 * -(-n // m)


# ---------------------------------------------------------------------------------------------------
# closed loops
# ---------------------------------------------------------------------------------------------------
def test_loop_to_the_receiving_side(torch_cuda):
    """the framer's output through hhuff_h2_deframe and hhuff_h2_control as the receiving peer: the DATA records' a / b
    reassemble every stream's body, no frame exceeds m, END_STREAM sits where expected, and the sender's window drops
    by what the receiver's recv_window drops"""
    torch = torch_cuda
    body = body_of(150000, 13)
    m = 20000
    streams = {1: (0, 50000, M.FINAL), 3: (50000, 45000, M.FINAL | M.TRAILERS), 5: (95000, 0, M.FINAL), 7: (95000, 30001, M.FINAL)}
    conns = [[M.send_rec(o, n, sid, 1 << 20, fl) for sid, (o, n, fl) in streams.items()], [M.send_rec(130000, 17, 9, 1 << 20, M.FINAL)]]
    e = M.batch(body, conns, [(m, 1 << 20)] * 2)
    h = frame_data(torch, e)
    compare(h, e)
    out = dev(torch, h["out"])
    nfr = [sum(int(k) for k in e["sent"]["nframes"][a:b]) for a, b in zip(e["send_first"][:-1], e["send_first"][1:])]
    frm_first = np.cumsum([0] + nfr).astype(np.uint32)
    # (each region's unused end is no frame: the receiver is given the bytes written)
    used = np.concatenate([h["out"][int(o):int(o) + int(n)] for o, n in zip(e["out_off"][:-1], e["out_len"])])
    in_off = np.cumsum([0] + [int(n) for n in e["out_len"]]).astype(np.uint32)
    data = dev(torch, used)
    d_first = dev(torch, frm_first)
    d = C.h2_deframe(data, dev(torch, in_off), d_first, int(frm_first[-1]), max_frame_size=m)
    rws = 1 << 24
    peers = C.h2_new_peers(2)
    peers["recv_window"] = rws
    r = C.h2_control(data, d["frames"], d["nframes"], d_first, int(frm_first[-1]), dev(torch, peers.view(np.uint8)),
                     dev(torch, (17 * frm_first).astype(np.uint32)), recv_window_size=rws, rep_size=17 * int(frm_first[-1]))
    torch.cuda.synchronize()
    assert d["cstatus"].cpu().tolist() == [0, 0] and r["cstatus"].cpu().tolist() == [0, 0]
    assert d["nframes"].cpu().tolist() == nfr and r["nctl"].cpu().tolist() == nfr
    frames = d["frames"].cpu().numpy().view(C.H2_FRAME_DTYPE)
    ctl = r["ctl"].cpu().numpy().view(C.H2_CTL_DTYPE)
    got, ended = {}, {}
    for f, t in zip(frames, ctl):
        assert f["type"] == 0 and f["length"] <= m and t["status"] == 0
        got[int(f["stream_id"])] = got.get(int(f["stream_id"]), b"") + used[int(t["a"]):int(t["a"]) + int(t["b"])].tobytes()
        assert not ended.get(int(f["stream_id"])), "a frame behind END_STREAM"
        ended[int(f["stream_id"])] = bool(f["flags"] & 1)
    want = {sid: body[o:o + n] for sid, (o, n, fl) in streams.items()}
    want[9] = body[130000:130017]
    assert got == want
    assert ended == {1: True, 3: False, 5: True, 7: True, 9: True}
    drop_recv = rws - r["peers"].cpu().numpy().view(C.H2_PEER_DTYPE)["recv_window"]
    drop_send = (1 << 20) - h["peers"].view(C.H2_PEER_DTYPE)["send_window"]
    assert drop_recv.tolist() == drop_send.tolist() == [125001, 17]


def test_loop_on_the_sending_side(torch_cuda):
    """a SETTINGS with MAX_FRAME_SIZE = 32768 and a new INITIAL_WINDOW_SIZE through hhuff_h2_control: the framer cuts at
    32768, and the records' windows move by the record's WINDOW_DELTA"""
    torch = torch_cuda
    body = body_of(100000, 14)
    d_peers = C.h2_new_peers(1, "cuda")
    settings = frame(4, 0, 0, (5).to_bytes(2, "big") + (32768).to_bytes(4, "big") + (4).to_bytes(2, "big") + (40000).to_bytes(4, "big"))
    d, r = control_bytes(torch, d_peers, [settings + frame(8, 0, 0, (1 << 20).to_bytes(4, "big"))])
    ctl = r["ctl"].cpu().numpy().view(C.H2_CTL_DTYPE)
    assert ctl["flags"][0] & C.H2R_WINDOW_DELTA
    delta = int(ctl["b"][0]) - (1 << 32)  # the int32 change, carried in a u32
    assert delta == 40000 - 65535
    peers = d_peers.cpu().numpy().view(C.H2_PEER_DTYPE).copy()
    assert peers["max_frame_size"].tolist() == [32768] and peers["send_window"].tolist() == [65535 + (1 << 20)]
    windows = [65535 + delta, 10 + delta]  # two streams opened before the SETTINGS: their windows move by the delta
    assert windows == [40000, -25525]
    conns = [[M.send_rec(0, 70000, 1, windows[0], M.FINAL), M.send_rec(70000, 100, 3, windows[1], M.FINAL)]]
    e = M.batch(body, conns, [(32768, 65535 + (1 << 20))])
    e["peers_in"] = peers.copy()
    e["peers_out"] = peers.copy()
    e["peers_out"]["send_window"] -= 40000
    compare(frame_data(torch, e), e)
    assert e["frames"][0] == [(32768, 0), (7232, 0)] and e["sent"]["flags"].tolist() == [M.STREAM_WINDOW, M.STREAM_WINDOW]
