"""HTTP/2 control frames on the GPU (include/hhuff.h (2k'), h2o_amd/csrc/hhuff_h2ctl.hip) against the model
(h2ctl_model.py): connections go through hhuff_h2_deframe and then hhuff_h2_control, and every output -- records,
peers, statuses, nctl, reply bytes -- is compared, what the call may not write still holding its sentinel.  The
hand-built corpus and fuzz-corpus connections on both sides; workgroup edges; exact-size guarded buffers and reply
regions; hostile frame records; a connection's frames cut over two and three calls; and the closed loops SETTINGS ->
de-framer -> control -> hhuff_hpack_responses_set_peers -> encoder, and replies -> de-framer -> control."""
import numpy as np
import pytest

import bounds_harness as BH
import h2ctl_corpora as K
import h2ctl_model as M
from conftest import load_golden
from h2o_amd import codec as C
from h2o_amd import hpenc_synth as HE

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
RWS = 1000  # the receive window of the mixed batches: small, so that a few DATA frames cross its half


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


def control(torch, e, client=False, rws=0, sentinel=SENTINEL, guard=False, tamper=None, in_place=False):
    """hhuff_h2_deframe and then hhuff_h2_control on the connections of the model's batch e (its peers_in, rep_off),
    every output of exactly its documented size and filled with the sentinel (guard: between two guard zones, which
    are checked): -> numpy arrays.  tamper(d, torch), if given, changes the de-framer's device outputs in between."""
    nconn, frm_cap, in_size = e["in_off"].size - 1, e["frm_cap"], int(e["data"].size)
    data = dev(torch, e["data"] if in_size else np.zeros(1, np.uint8))
    frm_first = dev(torch, e["frm_first"])
    d = C.h2_deframe(data, dev(torch, e["in_off"]), frm_first, frm_cap, in_size=in_size)
    if tamper is not None:
        tamper(d, torch)
    rep_size = int(e["rep_off"][-1])
    sizes = dict(ctl=16 * frm_cap, nctl=4 * nconn, cstatus=4 * nconn, cerr=4 * nconn, rep_len=4 * nconn, rep=rep_size, peers=40 * nconn)
    whole, out = {}, {}
    for k, n in sizes.items():
        if n == 0:  # (no such array: the wrapper passes a dummy)
            continue
        if guard:
            whole[k], inner = BH.guarded(torch, n, sentinel)
        else:
            inner = torch.full((n,), sentinel, dtype=torch.uint8, device="cuda")
        out[k] = inner.view(torch.int32) if k in ("nctl", "cstatus", "cerr", "rep_len") else inner
    peers_in = dev(torch, e["peers_in"].view(np.uint8))
    if in_place:
        out["peers"] = peers_in
        whole.pop("peers", None)
    r = C.h2_control(data, d["frames"], d["nframes"], frm_first, frm_cap, peers_in, dev(torch, e["rep_off"]),
                     C.H2C_CLIENT if client else 0, rws, in_size=in_size, rep_size=rep_size, out=out)
    torch.cuda.synchronize()
    for k, w in whole.items():
        w = w.cpu().numpy()
        n = w.size - 2 * BH.GUARD
        assert (w[:BH.GUARD] == sentinel).all() and (w[BH.GUARD + n:] == sentinel).all(), "guard of " + k
    h = {k: r[k].cpu().numpy() for k in sizes}
    h["nframes"] = d["nframes"].cpu().numpy().view(np.uint32)
    if not in_place:
        np.testing.assert_array_equal(peers_in.cpu().numpy(), e["peers_in"].view(np.uint8), err_msg="peers_in written")
    return h


def compare(h, e, sentinel=SENTINEL, skip=()):
    """every output array against the model's; what the call may not write still holds the sentinel.  skip: connections
    left out (their slots and regions too)"""
    nconn, frm_cap = e["in_off"].size - 1, e["frm_cap"]
    keep = np.ones(nconn, bool)
    keep[list(skip)] = False
    np.testing.assert_array_equal(h["nframes"][:nconn], e["nframes"], err_msg="the de-framer's nframes")
    for k, m in (("nctl", "nctl"), ("cerr", "ctl_err"), ("rep_len", "rep_len")):
        np.testing.assert_array_equal(h[k].view(np.uint32)[:nconn][keep], e[m][keep], err_msg=k)
    np.testing.assert_array_equal(h["cstatus"][:nconn][keep], e["ctl_status"][keep], err_msg="cstatus")
    slot_keep, rep_keep = np.ones(frm_cap, bool), np.ones(int(e["rep_off"][-1]), bool)
    for c in skip:
        slot_keep[int(e["frm_first"][c]):int(e["frm_first"][c + 1])] = False
        rep_keep[int(e["rep_off"][c]):int(e["rep_off"][c + 1])] = False
    ctl = h["ctl"][:16 * frm_cap].view(C.H2_CTL_DTYPE)
    used = e["ctl_used"]
    np.testing.assert_array_equal(ctl[used & slot_keep], e["ctl"][used & slot_keep], err_msg="ctl")
    assert (h["ctl"][:16 * frm_cap].reshape(-1, 16)[~used & slot_keep] == sentinel).all(), "a record behind the last one was written"
    rep, ru = h["rep"][:rep_keep.size], e["rep_used"]
    np.testing.assert_array_equal(rep[ru & rep_keep], e["rep"][ru & rep_keep], err_msg="rep")
    assert (rep[~ru & rep_keep] == sentinel).all(), "reply region written behind rep_len"
    peers = h["peers"][:40 * nconn].view(C.H2_PEER_DTYPE)
    np.testing.assert_array_equal(peers[keep], e["peers_out"][keep], err_msg="peers_out")


def batch(conns, caps=None, peers=None, client=False, rws=0, rep_caps=None):
    """the model's batch, with the start states kept as peers_in; caps default to the connections' whole frames"""
    if caps is None:
        caps = [count_frames(b) for b in conns]
    peers = [M.new_peer() for _ in conns] if peers is None else peers
    e = M.batch(conns, caps, peers, client, rws, rep_caps)
    e["peers_in"] = M.peers_array(peers)
    return e


def count_frames(b):
    n, pos = 0, 0
    while len(b) - pos >= 9:
        pos += 9 + int.from_bytes(b[pos:pos + 3], "big")
        n += 1
    return n


# ---------------------------------------------------------------------------------------------------
# corpus and fuzz
# ---------------------------------------------------------------------------------------------------
def corpus_cases():
    return [c for c in K.CASES if c["in_size"] is None]  # (hostile records: test_hostile_records)


def corpus_batch(cases, client, rws):
    caps = [count_frames(c["buf"]) for c in cases]
    rep_caps = [17 * n if c["rep_cap"] is None else c["rep_cap"] for c, n in zip(cases, caps)]
    return batch([c["buf"] for c in cases], caps, [c["peer"] for c in cases], client, rws, rep_caps)


@pytest.fixture(scope="module")
def corpus_batches():
    """the model's batches, made once: {(client, rws, order): batch}; a batch has the cases of one recv_window_size"""
    out = {}
    cs = corpus_cases()
    for rws in sorted({c["rws"] for c in cs}):
        mine = [c for c in cs if c["rws"] == rws]
        for order in ("in_order", "shuffled"):
            idx = np.arange(len(mine)) if order == "in_order" else np.random.default_rng(5).permutation(len(mine))
            for client in (False, True):
                out[client, rws, order] = corpus_batch([mine[i] for i in idx], client, rws)
    return out


@pytest.mark.parametrize("order", ["in_order", "shuffled"])
@pytest.mark.parametrize("side", ["server", "client"])
def test_corpus(torch_cuda, corpus_batches, side, order):
    for (client, rws, o), e in corpus_batches.items():
        if o == order and client == (side == "client"):
            compare(control(torch_cuda, e, client, rws), e)


def test_corpus_literal_expectations(torch_cuda):
    """the GPU against the corpus's own numbers, without the model in between"""
    cs = corpus_cases()
    for client, rws in sorted({(c["client"], c["rws"]) for c in cs}):
        mine = [c for c in cs if (c["client"], c["rws"]) == (client, rws)]
        e = corpus_batch(mine, client, rws)
        h = control(torch_cuda, e, client, rws)
        ctl, peers = h["ctl"].view(C.H2_CTL_DTYPE), h["peers"].view(C.H2_PEER_DTYPE)
        for i, c in enumerate(mine):
            assert (int(h["cstatus"][i]), int(h["cerr"][i]), int(h["nctl"][i])) == (c["status"], c["err"], c["nctl"]), c["name"]
            f0, r0 = int(e["frm_first"][i]), int(e["rep_off"][i])
            got = [tuple(int(v) for v in ctl[f0 + k]) for k in range(len(c["records"]))]
            for k, g in enumerate(got):  # a DATA record's offset is in `in`: the corpus counts from the connection's start
                if int(e["frames"]["type"][f0 + k]) == K.DATA and g[2] == 0:
                    got[k] = (g[0] - int(e["in_off"][i]),) + g[1:]
            assert got == c["records"], c["name"]
            assert h["rep"][r0:r0 + int(h["rep_len"][i])].tobytes() == c["replies"], c["name"]
            p = peers[i]
            assert ([int(v) for v in tuple(p)[:5]], int(p["flags"]), int(p["send_window"]), int(p["recv_window"])) == c["after"], c["name"]


def fuzz_connections():
    """the corpus files inside golden/frames.npz, and connections put together from the seeded random control frames of
    golden/h2ctl.npz"""
    fx = load_golden("frames")
    files = [bytes(fx["files"][int(fx["file_off"][f]):int(fx["file_off"][f + 1])]) for f in range(fx["file_off"].size - 1)]
    gx = load_golden("h2ctl")
    n = gx["pret"].size
    rng = np.random.default_rng(23)
    ok = np.flatnonzero(gx["pret"][n - 4000:] >= 0) + n - 4000
    rand = []
    for k in range(1200):  # mostly frames h2o accepts, so that walks get past their first frames
        pick = rng.choice(ok, int(rng.integers(1, 9))) if k % 3 else rng.integers(n - 4000, n, int(rng.integers(1, 6)))
        rand.append(b"".join(bytes(gx["probes"][int(gx["probe_off"][i]):int(gx["probe_off"][i + 1])]) for i in pick))
    return files + rand


@pytest.fixture(scope="module")
def fuzz_batches():
    conns = fuzz_connections()
    peers = []
    for i in range(len(conns)):
        p = M.new_peer()
        p["recv_window"] = RWS if i % 2 else RWS // 2 + 4  # every other one a few DATA bytes above the half
        if i % 5 == 0:
            p["send_window"] = 0x7fffffff - 100 * (i % 7)
        peers.append(p)
    return {client: batch(conns, None, peers, client, RWS) for client in (False, True)}


@pytest.mark.parametrize("side", ["server", "client"])
def test_fuzz_corpus_and_random_connections(torch_cuda, fuzz_batches, side):
    e = fuzz_batches[side == "client"]
    assert len(set(e["ctl_status"].tolist())) >= 4 and len(set(e["ctl_err"].tolist())) >= 10 and int(e["rep_len"].sum()) > 5000
    assert int((e["nctl"] > 3).sum()) > 200
    compare(control(torch_cuda, e, side == "client", RWS), e)


# ---------------------------------------------------------------------------------------------------
# workgroup edges
# ---------------------------------------------------------------------------------------------------
def long_connection(n=300):
    parts = []
    for k in range(n):
        parts.append([K.P(k.to_bytes(8, "big")), K.S((4, 65535 + k)), K.W(0, 1 + k), K.fr(K.DATA, 0, 1, b"d" * (k % 50)),
                      K.W(2 * k + 1, 0)][k % 5])
    return b"".join(parts)


@pytest.mark.parametrize("nconn", [1, 255, 256, 257, 513])
def test_workgroup_edges(torch_cuda, nconn):
    """connections without frames between busy ones, one connection of 300 frames, one whose frames end below its slots"""
    pool = [c["buf"] for c in K.CASES if c["peer"] == M.new_peer() and c["in_size"] is None]
    conns = [b"" if i % 3 == 1 else pool[(7 * i) % len(pool)] for i in range(nconn)]
    conns[nconn // 2] = long_connection()
    roomy = nconn - 1
    if nconn > 1:
        conns[roomy] = K.P(K.OPAQUE) + K.S((1, 77))
    caps = [count_frames(b) for b in conns]
    caps[roomy] += 3
    peers = [M.new_peer() for _ in conns]
    for p in peers:
        p["recv_window"] = RWS
    e = batch(conns, caps, peers, False, RWS)
    assert int(e["nctl"][nconn // 2]) == 300 and int(e["nframes"][roomy]) == caps[roomy] - 3
    if nconn > 2:
        assert int(e["nframes"][1]) == 0 and int((e["nctl"] > 0).sum()) > nconn // 5
    h = control(torch_cuda, e, False, RWS)
    compare(h, e)
    assert (h["ctl"][16 * (e["frm_cap"] - 3):16 * e["frm_cap"]] == SENTINEL).all()  # the last connection's unused slots


# ---------------------------------------------------------------------------------------------------
# guarded buffers, reply regions of exactly the bytes owed and one byte short, payloads ending at in + in_size
# ---------------------------------------------------------------------------------------------------
def owing_connections():
    return [c for c in corpus_cases() if c["rws"] == 0 and not c["client"] and c["rep_cap"] is None]


@pytest.mark.parametrize("sentinel", [s for _, s in BH.RUNS])
def test_exact_size_buffers(torch_cuda, corpus_batches, fuzz_batches, sentinel):
    for (client, rws, o), e in corpus_batches.items():
        if o == "shuffled":
            compare(control(torch_cuda, e, client, rws, sentinel=sentinel, guard=True), e, sentinel)
    compare(control(torch_cuda, fuzz_batches[False], False, RWS, sentinel=sentinel, guard=True), fuzz_batches[False], sentinel)


def test_reply_regions_of_exactly_the_bytes_owed_and_one_short(torch_cuda):
    cs = owing_connections()
    roomy = corpus_batch(cs, False, 0)
    owed = roomy["rep_len"].astype(np.int64)
    assert int((owed > 0).sum()) > 15
    conns, caps, peers = [c["buf"] for c in cs], [count_frames(c["buf"]) for c in cs], [c["peer"] for c in cs]
    exact = batch(conns, caps, peers, False, 0, owed.tolist())
    for k in ("nctl", "ctl_status", "ctl_err", "rep_len"):
        np.testing.assert_array_equal(exact[k], roomy[k])
    compare(control(torch_cuda, exact, guard=True), exact)
    short = batch(conns, caps, peers, False, 0, np.maximum(owed - 1, 0).tolist())
    owing = owed > 0
    assert (short["ctl_status"][owing] == C.H2C_SPACE).all() and (short["nctl"][owing] < roomy["nframes"][owing]).all()
    h = control(torch_cuda, short, guard=True)
    compare(h, short)
    # the state is the one before the frame that found no room: that of a call that ends in front of it
    before = batch([M_prefix(b, int(n)) for b, n in zip(conns, short["nctl"])], caps, peers, False, 0)
    np.testing.assert_array_equal(h["peers"].view(C.H2_PEER_DTYPE)[owing], before["peers_out"][owing])


def M_prefix(buf, nframes):
    """the first nframes whole frames of a connection"""
    pos = 0
    for _ in range(nframes):
        pos += 9 + int.from_bytes(buf[pos:pos + 3], "big")
    return buf[:pos]


@pytest.mark.parametrize("residue", [0, 1, 2, 3])
@pytest.mark.parametrize("last", ["ping", "settings", "window_update", "goaway", "priority", "data"])
def test_payload_ends_at_the_end_of_the_input(torch_cuda, residue, last):
    """the last connection's last payload ends at in + in_size, at every address residue (the input tensor has exactly
    in_size bytes)"""
    tail = dict(ping=K.P(K.OPAQUE2), settings=K.S((1, 1), (5, 16384)), window_update=K.W(0, 0x7fffffff - 65535),
                goaway=K.fr(K.GOAWAY, 0, 0, b"\0\0\0\3\0\0\0\1x"), priority=K.fr(K.PRIORITY, 0, 1, b"\0\0\0\7\x0f"),
                data=K.fr(K.DATA, K.PADDED, 1, b"\2abc\0\0"))[last]
    conns = [K.P(K.OPAQUE), K.fr(0xfa, 0, 0, b"\0" * residue) + tail]
    size = sum(len(b) for b in conns) + 9
    conns[0] += K.fr(0x0b, 0, 0, b"\0" * ((residue - size) % 4))  # the total's residue, whatever the tail's length
    e = batch(conns)
    assert int(e["data"].size) % 4 == residue and (e["ctl_status"] == 0).all()
    compare(control(torch_cuda, e, guard=True), e)


# ---------------------------------------------------------------------------------------------------
# hostile frame records and counts
# ---------------------------------------------------------------------------------------------------
def test_hostile_records(torch_cuda):
    """frames[] overwritten with payloads past in_size and nframes[] above the slots: HHUFF_H2C_EINVAL or clamping, the
    guards intact, the other connections as the model has them"""
    rich = K.S((1, 100)) + K.P(K.OPAQUE) + K.W(0, 7) + K.P(K.OPAQUE2) + K.S((1, 200))
    conns = [K.P(K.OPAQUE), rich, rich, K.S((3, 9)) + K.P(K.OPAQUE2), rich, rich, K.P(K.OPAQUE2)]
    e = batch(conns)
    in_size = int(e["data"].size)
    first = e["frm_first"]
    edits = {1: (2, in_size - 3, 4), 2: (0, 0xFFFFFFF0, 0x20), 4: (4, 5, 0xFFFFFFFF), 5: (1, in_size + 1, 0)}  # c: (frame, off, len)

    def tamper(d, torch):
        rec = d["frames"].view(torch.int32).view(-1, 8)
        for c, (k, off, n) in edits.items():
            rec[int(first[c]) + k, 0] = int(np.uint32(off).view(np.int32))
            rec[int(first[c]) + k, 1] = int(np.uint32(n).view(np.int32))
        d["nframes"][3] = int(first[4] - first[3]) + 1000  # above the slots: clamped to them
        d["nframes"][6] = -1

    h = control(torch_cuda, e, guard=True, tamper=tamper)
    h["nframes"] = e["nframes"]
    compare(h, e, skip=list(edits))
    peers, ctl = h["peers"].view(C.H2_PEER_DTYPE), h["ctl"].view(C.H2_CTL_DTYPE)
    for c, (k, _, _) in edits.items():
        want = batch([M_prefix(conns[c], k)])
        assert (int(h["cstatus"][c]), int(h["cerr"][c]), int(h["nctl"][c])) == (C.H2C_EINVAL, 0, k), c
        assert peers[c] == want["peers_out"][0] and int(h["rep_len"][c]) == int(want["rep_len"][0]), c
        f0, r0 = int(first[c]), int(e["rep_off"][c])
        np.testing.assert_array_equal(ctl[f0:f0 + k], want["ctl"][:k])
        assert (h["ctl"][16 * (f0 + k):16 * int(first[c + 1])] == SENTINEL).all(), c
        assert h["rep"][r0:r0 + int(want["rep_len"][0])].tobytes() == want["rep"][:int(want["rep_len"][0])].tobytes()
        assert (h["rep"][r0 + int(want["rep_len"][0]):int(e["rep_off"][c + 1])] == SENTINEL).all(), c


def test_hostile_slot_table(torch_cuda):
    """frm_first and rep_off that are no running sums, entries past frm_cap and rep_size: clamped, nothing outside the
    arrays touched"""
    torch = torch_cuda
    conns = [K.P(K.OPAQUE), K.S((1, 5)), K.P(K.OPAQUE2)]
    e = batch(conns)
    in_size, frm_cap = int(e["data"].size), e["frm_cap"]
    data = dev(torch, e["data"])
    d = C.h2_deframe(data, dev(torch, e["in_off"]), dev(torch, e["frm_first"]), frm_cap, in_size=in_size)
    out, whole = {}, {}
    for k, n in dict(ctl=16 * frm_cap, nctl=12, cstatus=12, cerr=12, rep_len=12, rep=20, peers=120).items():
        whole[k], inner = BH.guarded(torch, n, SENTINEL)
        out[k] = inner.view(torch.int32) if k in ("nctl", "cstatus", "cerr", "rep_len") else inner
    bad_first = dev(torch, np.array([0, 0xFFFFFFFF, 1, 7], np.uint32))
    bad_rep = dev(torch, np.array([0, 17, 0xFFFFFFF0, 5000], np.uint32))
    nfr = torch.full((3,), 1000, dtype=torch.int32, device="cuda")
    r = C.h2_control(data, d["frames"], nfr, bad_first, frm_cap, dev(torch, M.peers_array([M.new_peer()] * 3).view(np.uint8)),
                     bad_rep, 0, 0, in_size=in_size, rep_size=20, out=out)
    torch.cuda.synchronize()
    for k, w in whole.items():
        w = w.cpu().numpy()
        n = w.size - 2 * BH.GUARD
        assert (w[:BH.GUARD] == SENTINEL).all() and (w[BH.GUARD + n:] == SENTINEL).all(), "guard of " + k
    # connection 0: slots [0, 3) hold all three frames, its region is rep[0 .. 17): the PONG, then no room for the ACK;
    # connection 1: no slots; connection 2: slots [1, 3), its region clamped to nothing: no room for the ACK
    assert r["nctl"].cpu().tolist() == [1, 0, 0] and r["cstatus"].cpu().tolist() == [C.H2C_SPACE, 0, C.H2C_SPACE]
    assert r["rep_len"].cpu().tolist() == [17, 0, 0]
    assert r["rep"].cpu().numpy()[:17].tobytes() == K.PONG(K.OPAQUE) and (r["rep"].cpu().numpy()[17:] == SENTINEL).all()
    assert (r["ctl"].cpu().numpy()[16:] == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------
# state across steps
# ---------------------------------------------------------------------------------------------------
STEP_FRAMES = [K.S((4, 70000), (1, 0)), K.W(0, 5), K.P(K.OPAQUE), K.fr(K.DATA, 0, 1, b"b" * 300), K.S((4, 1000), (5, 32768)),
               K.fr(K.DATA, K.PADDED, 3, b"\x05" + b"c" * 250), K.W(9, 0), K.fr(K.GOAWAY, 0, 0, b"\0\0\0\1\0\0\0\0"), K.P(K.OPAQUE2),
               K.W(0, 0x7fffffff)]  # the last one overflows the send window


@pytest.mark.parametrize("in_place", [False, True], ids=["peers_out", "peers_in_place"])
def test_state_across_steps(torch_cuda, in_place):
    """the connection's frames over two and over three calls, cut at every frame boundary, peers_out fed back as
    peers_in: the state at the end and the replies laid end to end are those of the one call"""
    n = len(STEP_FRAMES)
    cuts = [(i, j) for i in range(n + 1) for j in range(i, n + 1)]  # i == j or j == n: two calls
    start = M.new_peer()
    start["recv_window"] = RWS
    whole = batch([b"".join(STEP_FRAMES)], None, [start], False, RWS)
    assert int(whole["ctl_status"][0]) == -3 and int(whole["nctl"][0]) == n - 1 and int(whole["rep_len"][0]) > 60
    peers = [start] * len(cuts)
    replies = [b""] * len(cuts)
    for step in range(3):
        parts = [b"".join(STEP_FRAMES[(0, i, j)[step]:(i, j, n)[step]]) for i, j in cuts]
        e = batch(parts, None, peers, False, RWS)
        h = control(torch_cuda, e, False, RWS, in_place=in_place)
        compare(h, e)
        peers = M.peers_list(h["peers"].view(C.H2_PEER_DTYPE))
        for k in range(len(cuts)):
            r0 = int(e["rep_off"][k])
            replies[k] += h["rep"][r0:r0 + int(h["rep_len"][k])].tobytes()
    want_rep = whole["rep"][:int(whole["rep_len"][0])].tobytes()
    for k in range(len(cuts)):
        assert replies[k] == want_rep, cuts[k]
        assert M.peers_array([peers[k]])[0] == whole["peers_out"][0], cuts[k]


# ---------------------------------------------------------------------------------------------------
# closed loops
# ---------------------------------------------------------------------------------------------------
def test_closed_loop_settings_reach_the_encoder(torch_cuda):
    """SETTINGS and request HEADERS -> de-framer -> control -> hhuff_hpack_responses_set_peers ->
    hhuff_hpack_flatten_responses, nothing but device arrays in between: byte for byte the call with the two fields
    filled on the host"""
    torch = torch_cuda
    sizes = [(t, f) for t in (0, 256, 4096, 65536) for f in (16384, 32768)]
    nconn = 3 * len(sizes)
    conns, rs = [], []
    for c in range(nconn):
        t, f = sizes[c % len(sizes)]
        nreq = c % 3  # connections without responses among them
        conns.append(K.S((1, t), (5, f)) + b"".join(K.fr(K.HEADERS, 5, 2 * k + 1, b"\x82\x86\x84") for k in range(nreq)))
        rs.append([dict(status=200, stream_id=2 * k + 1, flags=C.RES_SERVER | C.RES_END_STREAM, content_length=1000 + k,
                        headers=[(b"content-type", b"text/html", C.HDR_TOKEN), (b"x-request-%d" % k, b"v" * (40 + c), 0)],
                        header_table_size=t, max_frame_size=f) for k in range(nreq)])
    st = HE.build_batch(rs)
    nres = int(st["res"].size)
    d8 = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()  # noqa: E731

    def flatten(res_t):
        r = C.hpack_flatten_responses(d8(st["data"]), d8(st["hdr"].view(np.uint8)), res_t, d8(st["conn_first"].view(np.int32)), nres,
                                      d8(st["out_off"].view(np.int64)), st["server_off"], st["server_len"],
                                      in_size=int(st["data"].size))
        return r

    host = flatten(d8(st["res"].view(np.uint8)))
    blank = st["res"].copy()
    blank["header_table_size"], blank["max_frame_size"] = 0xDEADBEEF, 0xDEADBEEF
    res_t = d8(blank.view(np.uint8))
    e = batch(conns)
    data = dev(torch, e["data"])
    frm_first = dev(torch, e["frm_first"])
    d = C.h2_deframe(data, dev(torch, e["in_off"]), frm_first, e["frm_cap"], in_size=int(e["data"].size))
    ctl = C.h2_control(data, d["frames"], d["nframes"], frm_first, e["frm_cap"], C.h2_new_peers(nconn, "cuda"),
                       dev(torch, e["rep_off"]), rep_size=int(e["rep_off"][-1]))
    C.hpack_responses_set_peers(ctl["peers"], res_t, d["conn_first"], nres)
    dev_run = flatten(res_t)
    torch.cuda.synchronize()
    # the de-framer's blocks are the requests: its conn_first is the responses' conn_first
    np.testing.assert_array_equal(d["conn_first"].cpu().numpy().view(np.uint32), st["conn_first"])
    got = res_t.cpu().numpy().view(C.HPE_RESPONSE_DTYPE)
    np.testing.assert_array_equal(got, st["res"])  # the two fields set, no other byte of a record changed
    for k in ("out_len", "headers_size", "rstatus"):
        np.testing.assert_array_equal(dev_run[k].cpu().numpy()[:nres], host[k].cpu().numpy()[:nres], err_msg=k)
    assert (host["rstatus"].cpu().numpy()[:nres] == 0).all()
    a, b, lens = dev_run["out"].cpu().numpy(), host["out"].cpu().numpy(), host["out_len"].cpu().numpy()
    updates = 0
    for r in range(nres):
        o = int(st["out_off"][r])
        assert a[o:o + int(lens[r])].tobytes() == b[o:o + int(lens[r])].tobytes(), r
    for c in range(nconn):
        r = int(st["conn_first"][c])
        if r == int(st["conn_first"][c + 1]):
            continue
        # the connection's first block opens with a Dynamic Table Size Update carrying the peer's size where that is
        # below the encoder's 4096; h2o never grows its table (header_table_adjust_size, lib/http2/hpack.c:843), so
        # 4096 and 65536 bring none
        t, o = sizes[c % len(sizes)][0], int(st["out_off"][r]) + 9
        if t < 4096:
            want = {0: b"\x20", 256: b"\x3f\xe1\x01"}[t] + b"\x88"  # the update, then :status 200
            assert a[o:o + len(want)].tobytes() == want, c
            updates += 1
        else:
            assert a[o] & 0xE0 != 0x20, c
    assert updates >= 6
    np.testing.assert_array_equal(ctl["peers"].cpu().numpy().view(C.H2_PEER_DTYPE), e["peers_out"])


def test_closed_loop_replies_are_what_the_peer_expects(torch_cuda):
    """a batch's reply bytes go back in as the peer would receive them: every SETTINGS reply parses as an ACK, every
    PING reply carries ACK and the original opaque bytes, and the second pass owes nothing"""
    rng = np.random.default_rng(41)
    conns, want = [], []
    for c in range(200):
        parts, acks = [], []
        for _ in range(int(rng.integers(0, 7))):
            if rng.random() < 0.5:
                opaque = bytes(rng.integers(0, 256, 8, dtype=np.uint8))
                parts.append(K.P(opaque))
                acks.append((M.PING, opaque))
            else:
                parts.append(K.S((3, int(rng.integers(0, 1000)))))
                acks.append((M.SETTINGS, b""))
            if rng.random() < 0.3:
                parts.append(K.W(0, 10))
        conns.append(b"".join(parts))
        want.append(acks)
    e = batch(conns)
    h = control(torch_cuda, e)
    compare(h, e)
    back = [h["rep"][int(e["rep_off"][c]):int(e["rep_off"][c]) + int(h["rep_len"][c])].tobytes() for c in range(len(conns))]
    assert sum(len(b) for b in back) > 5000
    e2 = batch(back)
    h2 = control(torch_cuda, e2, client=True)
    compare(h2, e2)
    assert (h2["cstatus"][:len(conns)] == 0).all() and (h2["rep_len"][:len(conns)] == 0).all()
    ctl = h2["ctl"].view(C.H2_CTL_DTYPE)
    for c, acks in enumerate(want):
        f0 = int(e2["frm_first"][c])
        assert int(h2["nctl"][c]) == len(acks), c
        for k, (typ, opaque) in enumerate(acks):
            rec = ctl[f0 + k]
            assert int(rec["flags"]) == C.H2R_ACK and int(rec["status"]) == 0 and int(e2["frames"]["type"][f0 + k]) == typ, (c, k)
            if typ == M.PING:
                assert int(rec["a"]).to_bytes(4, "big") + int(rec["b"]).to_bytes(4, "big") == opaque, (c, k)
