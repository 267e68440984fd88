"""The HTTP/2 stream table on the GPU (include/hhuff.h (2k'''), h2o_amd/csrc/hhuff_h2streams.hip) against the model
(h2streams_model.py): the hand-built corpus, every case a connection of a batch and its second step through connection
slots; every output -- events, op events, statuses, nstr, the merged reply bytes -- is compared, what the call may not
write still holding its sentinel, and the tables behind it are read through hhuff_h2_streams_fill_sends.  Workgroup
edges; refused and reset slots; the two bridge calls around hhuff_h2_frame_data; and real bytes through hhuff_h2_deframe,
hhuff_h2_control and hhuff_hpack_parse_requests into the stream table."""
import numpy as np
import pytest

import h2streams_corpora as K
import h2streams_model as M
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
    if a.itemsize > 8 or a.dtype.names:
        a = a.view(np.uint8)
    return torch.from_numpy(a.copy()).cuda()


def peers_of(iws):
    p = C.h2_new_peers(len(iws))
    p["initial_window_size"] = iws
    return p.view(np.uint8)


def streams_call(torch, P, scratch, conns, iws, cont=False, slots=None, slack=0):
    """hhuff_h2_streams on the model's layout of conns (h2streams_model.build), every output filled with the sentinel:
    -> (the layout, numpy outputs)"""
    a = M.build(conns, slack)
    nconn, frm_cap = a["nconn"], a["frm_cap"]
    nops = a["ops"].shape[0]
    full = lambda n: torch.full((max(1, n),), SENTINEL, dtype=torch.uint8, device="cuda")  # noqa: E731
    out = dict(sev=full(16 * frm_cap), op_sev=full(16 * nops), rep=full(a["rep_size"]))
    for k in ("nstr", "sstatus", "serr", "rep_len"):
        out[k] = full(4 * nconn).view(torch.int32)
    t = lambda k: dev(torch, a[k])  # noqa: E731
    r = C.h2_streams(P, scratch, torch.zeros(8, dtype=torch.uint8, device="cuda"), t("frames"), t("nframes"), t("frm_first"), frm_cap,
                     t("ctl"), t("nctl"), t("ctl_rep"), t("ctl_rep_off"), t("blocks"), t("conn_first"), t("bstatus"), t("req"),
                     t("arena"), t("blk_off"), t("value_off"), t("value_len"), dev(torch, peers_of(iws)), t("rep_off"),
                     ops=dev(torch, a["ops"].astype(np.uint32).reshape(-1).view(np.uint8)) if nops else None, op_first=t("op_first") if nops else None,
                     flags=C.H2ST_CONTINUE if cont else 0, slots=slots, in_size=a["in_size"], ctl_rep_size=a["ctl_rep_size"],
                     arena_size=a["arena_size"], rep_size=a["rep_size"], out=out)
    torch.cuda.synchronize()
    return a, {k: v.cpu().numpy() for k, v in r.items()}


def compare(a, h, walks, refused=()):
    """the outputs against the model's walks (one per connection; None: not compared), sentinels elsewhere"""
    sev = h["sev"][:16 * a["frm_cap"]].reshape(-1, 16)
    op_sev = h["op_sev"][:16 * a["ops"].shape[0]].reshape(-1, 16)
    rep = h["rep"]
    for c, w in enumerate(walks):
        if w is None:
            continue
        f0, f1 = int(a["frm_first"][c]), int(a["frm_first"][c + 1])
        o0, o1 = int(a["op_first"][c]), int(a["op_first"][c + 1])
        r0, r1 = int(a["rep_off"][c]), int(a["rep_off"][c + 1])
        if c in refused:
            assert (h["nstr"][c], h["sstatus"][c], h["serr"][c], h["rep_len"][c]) == (0, M.ESLOT, 0, 0), c
            assert (sev[f0:f1] == SENTINEL).all() and (op_sev[o0:o1] == SENTINEL).all() and (rep[r0:r1] == SENTINEL).all(), c
            continue
        assert (h["nstr"][c], h["sstatus"][c], h["serr"][c], h["rep_len"][c]) == (w["nstr"], w["status"], w["err"], len(w["replies"])), c
        b0 = int(a["conn_first"][c])
        got = sev[f0:f0 + len(w["events"])].copy().view(M.SEV_DTYPE).reshape(-1)
        want = [(e[0], e[1] + (b0 if e[4] & M.OPENED else 0), e[2], e[3], e[4]) for e in w["events"]]
        assert [tuple(int(v) for v in g) for g in got] == want, c
        assert (sev[f0 + len(w["events"]):f1] == SENTINEL).all(), "an event behind the last one was written (%d)" % c
        got = op_sev[o0:o0 + len(w["op_events"])].copy().view(M.SEV_DTYPE).reshape(-1)
        assert [tuple(int(v) for v in g) for g in got] == [tuple(e) for e in w["op_events"]], c
        assert (op_sev[o0 + len(w["op_events"]):o1] == SENTINEL).all(), c
        assert bytes(rep[r0:r0 + len(w["replies"])]) == w["replies"], c
        assert (rep[r0 + len(w["replies"]):r1] == SENTINEL).all(), "reply region written behind rep_len (%d)" % c


def windows(torch, P, scratch, ids, slots=None):
    """hhuff_h2_streams_fill_sends for ids [[stream ids] per connection] -> [[(window, miss)]]"""
    send_first = np.concatenate([[0], np.cumsum([len(x) for x in ids])]).astype(np.uint32)
    sends = np.zeros(max(1, int(send_first[-1])), C.H2_SEND_DTYPE)
    flat = [s for x in ids for s in x]
    sends["stream_id"][:len(flat)] = flat
    sends["window"] = 12345
    d = dev(torch, sends)
    miss = C.h2_streams_fill_sends(P["max_entries"], scratch, d, dev(torch, send_first), slots=slots, nsend=len(flat))
    torch.cuda.synchronize()
    s, m = d.cpu().numpy().view(C.H2_SEND_DTYPE), miss.cpu().numpy()
    return [[(int(s["window"][k]), int(m[k])) for k in range(int(send_first[c]), int(send_first[c + 1]))] for c in range(len(ids))], d


def by_params():
    groups = {}
    for c in K.CASES:
        groups.setdefault(tuple(sorted(c["P"].items())), []).append(c)
    return list(groups.values())


@pytest.mark.parametrize("cases", by_params(), ids=lambda cs: cs[0]["name"])
def test_corpus_in_batches_and_its_second_steps_through_slots(torch_cuda, cases):
    """every case of one parameter set as a connection of one call; then the second steps of those that have one, listed
    in reverse order through connection slots with HHUFF_H2ST_CONTINUE, the send side's bookings in front"""
    torch = torch_cuda
    P, n = cases[0]["P"], len(cases)
    scratch = torch.full((C.h2_streams_scratch_size(n, P["max_entries"]),), SENTINEL, dtype=torch.uint8, device="cuda")
    conns = [M.new_conn() for _ in cases]
    step = lambda c, k: dict(frames=c["steps"][k].frames, blocks=c["steps"][k].blocks, ops=c["steps"][k].ops,  # noqa: E731
                             nctl=c["steps"][k].nctl, rep_cap=c["steps"][k].rep_cap)
    walks = [M.walk(conns[i], P, c["iws"][0], c["steps"][0].frames, c["steps"][0].blocks, c["steps"][0].ops, c["steps"][0].rep_cap,
                    c["steps"][0].nctl) for i, c in enumerate(cases)]
    a, h = streams_call(torch, P, scratch, [step(c, 0) for c in cases], [c["iws"][0] for c in cases], slack=1)
    compare(a, h, walks)
    for i, c in enumerate(cases):
        if len(c["steps"]) == 1:
            assert K.observed(walks[i], conns[i]) == K.expected(c), c["name"]
    second = [i for i, c in enumerate(cases) if len(c["steps"]) == 2][::-1]
    if second:
        slots = C.ConnSlots(dev(torch, np.array(second, np.uint32)), None, n)
        booked = [cases[i]["steps"][1].sends for i in second]
        if any(booked):
            _, d = windows(torch, P, scratch, [[s for s, _ in b] for b in booked], slots)
            sent = np.zeros(max(1, sum(len(b) for b in booked)), C.H2_SENT_DTYPE)
            sent["sent"][:sum(len(b) for b in booked)] = [v for b in booked for _, v in b]
            first = np.concatenate([[0], np.cumsum([len(b) for b in booked])]).astype(np.uint32)
            C.h2_streams_commit_sent(P["max_entries"], scratch, d, dev(torch, sent), dev(torch, first), slots=slots,
                                     nsend=int(first[-1]))
        walks2 = []
        for i in second:
            st = cases[i]["steps"][1]
            if st.sends:
                M.fill_sends(conns[i], [s for s, _ in st.sends])
                M.commit_sent(conns[i], [s for s, _ in st.sends], [v for _, v in st.sends])
            walks2.append(M.walk(conns[i], P, cases[i]["iws"][1], st.frames, st.blocks, st.ops, st.rep_cap, st.nctl))
        a, h = streams_call(torch, P, scratch, [step(cases[i], 1) for i in second], [cases[i]["iws"][1] for i in second], cont=True,
                            slots=slots)
        compare(a, h, walks2)
        for k, i in enumerate(second):
            assert K.observed(walks2[k], conns[i]) == K.expected(cases[i]), cases[i]["name"]
    # the tables behind it: every stream the model has, with its send window, and one it has not
    ids = [sorted(cn["streams"]) + [0x7ffffff1] for cn in conns]
    got, _ = windows(torch, P, scratch, ids)
    for i, cn in enumerate(conns):
        want = [(max(-M.INT32_MAX, min(M.INT32_MAX, cn["streams"][s]["output_window"])), 0) for s in sorted(cn["streams"])] + [(0, 1)]
        assert got[i] == want, cases[i]["name"]


@pytest.mark.parametrize("nconn", [1, 63, 64, 65, 129])
def test_workgroup_edges(torch_cuda, nconn):
    """one lane a connection, 64 a workgroup: batches that end on, one before and one behind a workgroup's last lane"""
    torch = torch_cuda
    P = K.CASES[0]["P"]
    pool = [c for c in K.CASES if c["P"] == P and len(c["steps"]) == 1 and c["iws"][0] == 65535]
    cases = [pool[(7 * i) % len(pool)] for i in range(nconn)]
    scratch = torch.zeros(C.h2_streams_scratch_size(nconn, P["max_entries"]), dtype=torch.uint8, device="cuda")
    conns = [M.new_conn() for _ in cases]
    walks = [M.walk(conns[i], P, 65535, c["steps"][0].frames, c["steps"][0].blocks, c["steps"][0].ops, c["steps"][0].rep_cap,
                    c["steps"][0].nctl) for i, c in enumerate(cases)]
    a, h = streams_call(torch, P, scratch, [dict(frames=c["steps"][0].frames, blocks=c["steps"][0].blocks, ops=c["steps"][0].ops,
                                                 nctl=c["steps"][0].nctl, rep_cap=c["steps"][0].rep_cap) for c in cases], [65535] * nconn)
    compare(a, h, walks)


def test_slots_refused_reset_and_untouched(torch_cuda):
    """(2h): a repeated slot and a slot out of range are refused and write nothing; HHUFF_CONN_RESET starts a connection
    empty under HHUFF_H2ST_CONTINUE; the slab of a slot nobody names is not touched"""
    torch = torch_cuda
    P = M.params(max_streams=4, max_streams_for_priority=2, max_entries=8)
    slab = C.h2_streams_scratch_size(1, 8)
    scratch = torch.full((4 * slab,), SENTINEL, dtype=torch.uint8, device="cuda")
    one = lambda s: dict(frames=s.frames, blocks=s.blocks, ops=s.ops)  # noqa: E731
    first = [one(K.S().headers(1)), one(K.S().headers(1).headers(3)), one(K.S().headers(5))]
    slots = C.ConnSlots(dev(torch, np.array([2, 0, 1], np.uint32)), None, 4)
    conns = [M.new_conn() for _ in first]
    walks = [M.walk(conns[i], P, 65535, f["frames"], f["blocks"]) for i, f in enumerate(first)]
    a, h = streams_call(torch, P, scratch, first, [65535] * 3, slots=slots)
    compare(a, h, walks)
    assert (scratch[3 * slab:].cpu().numpy() == SENTINEL).all(), "the slab of a slot nobody names was written"
    # the same slots again: data for each stream 1; connection 1 repeats slot 2, connection 3 names slot 9, connection 2 resets
    nxt = [one(K.S().data(1, 3)), one(K.S().data(1, 3)), one(K.S().data(1, 3)), one(K.S().data(1, 3))]
    slots = C.ConnSlots(dev(torch, np.array([2, 2, 0, 9], np.uint32)), dev(torch, np.array([0, 0, C.CONN_RESET, 0], np.uint8)), 4)
    fresh = M.new_conn()
    walks = [M.walk(conns[0], P, 65535, nxt[0]["frames"], []), {}, M.walk(fresh, P, 65535, nxt[2]["frames"], []), {}]
    assert walks[0]["events"][0][4] == M.BODY and walks[2]["status"] == -1 and walks[2]["err"] == M.E_DATA_FRAME
    a, h = streams_call(torch, P, scratch, nxt, [65535] * 4, cont=True, slots=slots)
    compare(a, h, walks, refused=(1, 3))
    got, _ = windows(torch, P, scratch, [[1], [5], [1], []])
    assert got == [[(0, 1)], [(65535, 0)], [(65535, 0)], []]  # slot 0 was reset, slot 1 was not listed, slot 2 went on


def test_fill_sends_and_commit_sent_around_frame_data(torch_cuda):
    """the two bridge calls around hhuff_h2_frame_data: the windows travel from the table to the send records, a repeated
    and a missing stream get window 0 and are stopped by the framer, and what was sent leaves the table's windows"""
    torch = torch_cuda
    P = M.params(max_streams=4, max_streams_for_priority=2, max_entries=8)
    scratch = torch.zeros(C.h2_streams_scratch_size(2, 8), dtype=torch.uint8, device="cuda")
    st = [K.S().headers(1, True).headers(3, True), K.S().headers(1, True)]
    streams_call(torch, P, scratch, [dict(frames=s.frames, blocks=s.blocks) for s in st], [100, 30])
    body = np.arange(200, dtype=np.uint8)
    sends = np.zeros(5, C.H2_SEND_DTYPE)
    sends["stream_id"] = [1, 3, 1, 7, 1]
    sends["body_off"], sends["body_len"], sends["flags"] = [0, 60, 120, 130, 140], [60, 60, 10, 10, 50], C.H2S_FINAL
    send_first = dev(torch, np.array([0, 4, 5], np.uint32))
    d = dev(torch, sends)
    miss = C.h2_streams_fill_sends(8, scratch, d, send_first)
    peers = dev(torch, C.h2_new_peers(2).view(np.uint8))
    out_off = dev(torch, np.array([0, 400, 800], np.uint32))
    r = C.h2_frame_data(dev(torch, body), d, send_first, peers, out_off, out_size=800)
    C.h2_streams_commit_sent(8, scratch, d, r["sent"], send_first)
    C.h2_streams_commit_sent(8, scratch, d, r["sent"], send_first)  # a second commit behind one fill books nothing again
    torch.cuda.synchronize()
    assert miss.cpu().numpy().tolist() == [0, 0, 2, 1, 0]
    assert d.cpu().numpy().view(C.H2_SEND_DTYPE)["window"].tolist() == [100, 100, 0, 0, 30]
    sent = r["sent"].cpu().numpy().view(C.H2_SENT_DTYPE)
    assert sent["sent"].tolist() == [60, 60, 0, 0, 30]
    sw = C.H2T_STREAM_WINDOW
    assert [int(f) & sw for f in sent["flags"]] == [0, 0, sw, sw, sw]
    got, _ = windows(torch, P, scratch, [[3, 1], [1]])
    assert got == [[(40, 0), (40, 0)], [(0, 0)]]


def h2frame(typ, flags, sid, payload):
    return M.frame_bytes(typ, flags, sid, payload)


def lit(name, value):  # literal header field without indexing, new name (RFC 7541 6.2.2)
    return b"\x00" + bytes([len(name)]) + name + bytes([len(value)]) + value


def test_real_bytes_through_the_four_calls(torch_cuda):
    """socket bytes -> hhuff_h2_deframe -> hhuff_h2_control -> hhuff_hpack_parse_requests -> hhuff_h2_streams: the stream
    table's outputs against the model fed with what the three calls left, and the request's verdicts as literals"""
    torch = torch_cuda
    get, post = b"\x82\x86\x84", b"\x83\x86\x84"  # :method GET / POST, :scheme http, :path /
    c0 = (h2frame(1, 4, 1, post + lit(b"content-length", b"5")) + h2frame(0, 1, 1, b"hello") + h2frame(1, 5, 3, get) +
          h2frame(6, 0, 0, b"12345678") + h2frame(8, 0, 3, M.be32(10)) + h2frame(1, 1, 5, get[:1]) + h2frame(9, 4, 5, get[1:]) +
          h2frame(1, 5, 7, get + lit(b"x\x01", b"v")) + h2frame(3, 0, 9, M.be32(8)))
    c1 = (h2frame(4, 0, 0, b"\x00\x04" + M.be32(100)) + h2frame(1, 5, 1, b"\x82\x84") + h2frame(1, 4, 3, get) +
          h2frame(0, 0, 3, b"xy") + h2frame(1, 5, 3, lit(b"t", b"1")) + h2frame(0, 0, 3, b"z") + h2frame(8, 0, 5, M.be32(0)))
    conns = [c0, c1, b""]
    data = np.frombuffer(b"".join(conns), np.uint8)
    in_off = np.concatenate([[0], np.cumsum([len(b) for b in conns])]).astype(np.uint32)
    frm_first = np.array([0, 12, 20, 22], np.uint32)
    frm_cap, nconn = 22, 3
    t_data, t_first = dev(torch, data), dev(torch, frm_first)
    d = C.h2_deframe(t_data, dev(torch, in_off), t_first, frm_cap, arena_fixed=1024, arena_per_byte=16)
    ctl_rep_off = dev(torch, np.array([0, 12 * 17, 20 * 17, 22 * 17], np.uint32))
    k = C.h2_control(t_data, d["frames"], d["nframes"], t_first, frm_cap, C.h2_new_peers(nconn, "cuda"), ctl_rep_off, 0, 65535,
                     rep_size=22 * 17)
    q = C.hpack_decode_blocks(d["blk"], d["blk_off"], d["conn_first"], arena_off=d["arena_off"], requests=True)
    P = M.params(max_streams=4, max_streams_for_priority=2, max_entries=8)
    scratch = torch.zeros(C.h2_streams_scratch_size(nconn, 8), dtype=torch.uint8, device="cuda")
    rep_off = np.array([0, 12 * 43, 20 * 43, 22 * 43], np.uint32)
    out = dict(sev=torch.full((16 * frm_cap,), SENTINEL, dtype=torch.uint8, device="cuda"),
               rep=torch.full((22 * 43,), SENTINEL, dtype=torch.uint8, device="cuda"))
    r = C.h2_streams(P, scratch, t_data, d["frames"], d["nframes"], t_first, frm_cap, k["ctl"], k["nctl"], k["rep"], ctl_rep_off,
                     d["blocks"], d["conn_first"], q["bstatus"], q["req"], q["arena"], d["blk_off"], q["value_off"], q["value_len"],
                     k["peers"], dev(torch, rep_off), rep_size=22 * 43, out=out)
    torch.cuda.synchronize()
    # the model's input: what the three calls left
    n = lambda t: t.cpu().numpy()  # noqa: E731
    frames, ctl = n(d["frames"]).view(C.H2_FRAME_DTYPE), n(k["ctl"]).view(C.H2_CTL_DTYPE)
    blocks, req = n(d["blocks"]).view(C.H2_BLOCK_DTYPE), n(q["req"]).reshape(-1).view(M.REQ_DTYPE)
    bstatus, conn_first, blk_off = n(q["bstatus"]), n(d["conn_first"]).view(np.uint32), n(d["blk_off"]).view(np.uint32)
    arena, voff, vlen = n(q["arena"]), n(q["value_off"]).view(np.uint32), n(q["value_len"]).view(np.uint32)
    ctl_rep, peers = n(k["rep"]), n(k["peers"]).view(C.H2_PEER_DTYPE)
    assert n(d["nframes"]).tolist() == [9, 7, 0] and n(k["nctl"]).tolist() == [9, 7, 0] and conn_first.tolist() == [0, 4, 7, 7]
    sev, rep = n(r["sev"]).view(M.SEV_DTYPE), n(r["rep"])
    for c in range(nconn):
        f0, b0 = int(frm_first[c]), int(conn_first[c])

        def value(b, field):
            if field < 0:
                return None
            s = int(blk_off[b]) + field
            return bytes(arena[int(voff[s]):int(voff[s]) + int(vlen[s])])

        mb = [dict(stream_id=int(blocks["stream_id"][b]), flags=int(blocks["flags"][b]), first_frame=int(blocks["first_frame"][b]) - f0,
                   nframes=int(blocks["nframes"][b]), bstatus=int(bstatus[b]), exists_map=int(req["exists_map"][b]),
                   content_length=int(req["content_length"][b]), method=value(b, int(req["method"][b])),
                   path=value(b, int(req["path"][b])), host=int(req["authority"][b]) >= 0 and not int(req["exists_map"][b]) & 8)
              for b in range(b0, int(conn_first[c + 1]))]
        mf, pos = [], int(n(ctl_rep_off).view(np.uint32)[c])
        for i in range(f0, f0 + int(n(d["nframes"])[c])):
            rl = int(ctl["reply_len"][i])
            blk = int(frames["block"][i])
            mf.append(dict(type=int(frames["type"][i]), flags=int(frames["flags"][i]), stream_id=int(frames["stream_id"][i]),
                           length=int(frames["length"][i]), ctl=(int(ctl["a"][i]), int(ctl["b"][i]), int(ctl["flags"][i])),
                           ctl_reply=bytes(ctl_rep[pos:pos + rl]), block=None if blk == 0xFFFFFFFF else blk - b0))
            pos += rl
        w = M.walk(M.new_conn(), P, int(peers["initial_window_size"][c]), mf, mb)
        assert (n(r["nstr"])[c], n(r["sstatus"])[c], n(r["serr"])[c], n(r["rep_len"])[c]) == (w["nstr"], w["status"], w["err"],
                                                                                              len(w["replies"])), c
        got = [tuple(int(v) for v in e) for e in sev[f0:f0 + len(w["events"])]]
        assert got == [(e[0], e[1] + (b0 if e[4] & M.OPENED else 0), e[2], e[3], e[4]) for e in w["events"]], c
        assert (n(r["sev"]).reshape(-1, 16)[f0 + len(w["events"]):int(frm_first[c + 1])] == SENTINEL).all(), c
        assert bytes(rep[int(rep_off[c]):int(rep_off[c]) + len(w["replies"])]) == w["replies"], c
    # the verdicts, as literals
    RC = M.REQUEST_COMPLETE
    assert [int(f) for f in sev["flags"][:9]] == [M.OPENED, M.BODY | RC, M.OPENED | RC, 0, 0, 0, M.OPENED | RC,
                                                  M.OPENED | M.INVALID_HEADER, 0]
    assert (int(r["sstatus"][0]), int(r["serr"][0]), int(r["nstr"][0])) == (-1, M.E_RST_STREAM_STREAM_ID, 8)
    pong = M.frame_bytes(6, 1, 0, b"12345678")
    assert bytes(rep[:int(r["rep_len"][0])]) == pong
    assert [int(f) for f in sev["flags"][12:19]] == [0, M.RESET_SENT, M.OPENED, M.BODY, M.TRAILERS | RC, M.RESET_SENT, M.RESET_SENT]
    want = K.ACK + M.rst_stream_bytes(1, -1) + M.rst_stream_bytes(3, -5) + M.rst_stream_bytes(5, -1)
    assert bytes(rep[int(rep_off[1]):int(rep_off[1]) + int(r["rep_len"][1])]) == want and int(r["sstatus"][1]) == 0
    got, _ = windows(torch, P, scratch, [[1, 3, 5, 7], [1, 3], []])
    assert got == [[(65535, 0), (65545, 0), (65535, 0), (65535, 0)], [(0, 1), (0, 1)], []]
