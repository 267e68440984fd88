"""Connection images (include/hhuff.h (2i)) on the GPU.  The image is pinned by behaviour, not by bytes: the
expectation is the uninterrupted session through the existing entry points (pinned to the restatement, the reference
and the models by their own suites), and a connection moved at a step boundary must produce, from then on, exactly
the records of the connection that never moved.

Shapes are the slots tests' (tests/test_conn_slots_gpu.py, whose helpers run the family calls here): 70 connections
(a wave and a partial second), a source scratch of 131 slots, a destination of 67 allocated separately and filled
with 0xC3, 4 steps, the cut after step 1; again with 1 and 64 connections.  Every buffer a call writes is the inner
part of a sentinel-filled guarded buffer."""
import ctypes

import numpy as np
import pytest

import bounds_harness as BH
import slots_plan as SP
import test_conn_slots_gpu as T
from h2o_amd import codec as C
from h2o_amd import hpack_synth as HS

pytestmark = pytest.mark.gpu

NA, NB, CUT, SENT, FILL = T.NSLOTS, 67, 2, 0x5A, T.SCR_FILL
SKIPPED, QPK_BLOCKED = -301, -302  # HHUFF_BLK_SKIPPED, HHUFF_QPK_BLOCKED


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def family(kind):
    fam = T.KINDS[kind]
    if fam is SP.Blocks:
        return C.conn_family(C.FAM_HPACK_DEC, T.TABLE)
    if fam is SP.QpackDecode:
        return C.conn_family(C.FAM_QPACK_DEC, T.TABLE)
    if fam is SP.HpackEncode:
        return C.conn_family(C.FAM_HPACK_ENC)
    return C.conn_family(C.FAM_QPACK_ENC, T.TABLE, T.MAX_INFLIGHT)


def u32(torch, a):
    return torch.from_numpy(np.asarray(a, np.uint32).view(np.int32).copy()).cuda()


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


class Images:
    """the images of one export: img = the inner part of a guarded buffer, region k = [off[k], off[k + 1])"""

    def __init__(self, torch, whole, img, off, lens, status):
        self.torch, self.whole, self.img, self.off, self.len, self.status = torch, whole, img, off, lens, status

    def bytes(self, k):
        o = int(self.off[k])
        return self.img[o:o + int(self.len[k])].cpu().numpy().tobytes()

    def guards_ok(self):
        w = self.whole.cpu().numpy()
        return bool((w[:BH.GUARD] == SENT).all() and (w[w.size - BH.GUARD:] == SENT).all())

    def to(self, device):
        whole = self.whole.to(device)  # a peer copy
        return Images(self.torch, whole, whole[BH.GUARD:whole.numel() - BH.GUARD], self.off, self.len, self.status)


def export(torch, fam, scr, nslots, slot, room=None):
    """hhuff_conn_export through the C ABI: the size query, then the images into regions of exactly their length
    (room(lens) -> other region sizes, multiples of 16) inside a guarded buffer"""
    L = C.lib()
    n = len(slot)
    ds = u32(torch, slot)
    ln = torch.full((max(1, n),), -1, dtype=torch.int32, device="cuda")
    st = torch.full((max(1, n),), -1, dtype=torch.int32, device="cuda")
    head = [ctypes.byref(fam), scr.data_ptr(), scr.numel(), nslots, ds.data_ptr(), n]
    assert L.hhuff_conn_export(*head, None, None, ln.data_ptr(), st.data_ptr(), _stream(torch)) == 0, L.hhuff_last_error_string()
    torch.cuda.synchronize()
    need = ln.cpu().numpy().view(np.uint32)[:n].copy()
    st0 = st.cpu().numpy()[:n].copy()
    sizes = need.astype(np.int64) if room is None else np.asarray(room(need), np.int64)
    assert (sizes % 16 == 0).all()
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    whole, img = BH.guarded(torch, int(off[-1]), SENT)
    doff = torch.from_numpy(off.view(np.int64).copy()).cuda()
    ln.fill_(-1)
    st.fill_(-1)
    assert L.hhuff_conn_export(*head, img.data_ptr(), doff.data_ptr(), ln.data_ptr(), st.data_ptr(), _stream(torch)) == 0
    torch.cuda.synchronize()
    im = Images(torch, whole, img, off, ln.cpu().numpy().view(np.uint32)[:n].copy(), st.cpu().numpy()[:n].copy())
    assert im.guards_ok()
    # img == NULL gave the same lengths, and refused the same items
    assert (need == im.len).all() and ((st0 != 0) == (im.status == C.IMG_EINVAL)).all()
    return im


def imp(torch, fam, scr, nslots, slot, im, lens=None):
    """hhuff_conn_import of the images -> status[n]"""
    L = C.lib()
    n = len(slot)
    st = torch.full((max(1, n),), -1, dtype=torch.int32, device="cuda")
    doff = torch.from_numpy(im.off.view(np.int64).copy()).cuda()
    ds, dl = u32(torch, slot), u32(torch, im.len if lens is None else lens)  # (named: they live until the call has run)
    rc = L.hhuff_conn_import(ctypes.byref(fam), scr.data_ptr(), scr.numel(), nslots, ds.data_ptr(), n, im.img.data_ptr(),
                             doff.data_ptr(), dl.data_ptr(), st.data_ptr(), _stream(torch))
    assert rc == 0, L.hhuff_last_error_string()
    torch.cuda.synchronize()
    return st.cpu().numpy()[:n].copy()


def scratch_of(torch, fam, nslots):
    return BH.guarded(torch, nslots * C.conn_slab_size(fam), FILL)


def hop(torch, fam, scr, nconn, seed, fill=FILL):
    """every connection of a dense scratch (connection c in slab c) into permuted slots of a 131-slot scratch and from
    there into a new dense one; the two it leaves behind are overwritten -> (whole, inner) of the new one"""
    every, via = np.arange(nconn), np.random.default_rng(seed).permutation(NA)[:nconn]
    whole_b, b = scratch_of(torch, fam, NA)
    assert (imp(torch, fam, b, NA, via, export(torch, fam, scr, nconn, every)) == 0).all()
    whole_c, c = BH.guarded(torch, nconn * C.conn_slab_size(fam), fill)
    assert (imp(torch, fam, c, nconn, every, export(torch, fam, b, NA, via)) == 0).all()
    assert T.guards_ok(whole_b)
    w = whole_c.cpu().numpy()
    assert (w[:BH.GUARD] == fill).all() and (w[w.size - BH.GUARD:] == fill).all()
    scr.fill_(0x11)
    b.fill_(0x11)
    return whole_c, c


def step_of(kind, dense, conns, k):
    fam = T.KINDS[kind]
    return fam.pack([fam.chunk(dense[k], int(c)) for c in conns], dense[0])


def run_listed(torch, kind, dense, want, conns, k, scr, slots, nslots, cont=True):
    """chunk k of the listed connections in their slots: every record is the dense run's"""
    if len(conns) == 0:
        return 0
    step = step_of(kind, dense, conns, k)
    r = T.call(torch, kind, step, scr, T.CONT if cont else 0, T.Slots(slots, None, nslots))
    recs = T.KINDS[kind].records(step, r)
    for c, rec in zip(conns, recs):
        assert rec == want[(int(c), k)], (kind, k, int(c))
    return sum(len(rec[1]) for rec in recs)


def moved_set(nconn):
    return np.array(sorted(set(range(1, nconn, 2)) | {0, nconn - 1}))


def move_and_continue(torch, kind, nconn, dense, want, dev_b=None, before_b=None):
    """steps 0-1 in scratch A, half of the connections exported and imported into scratch B (on dev_b) in permuted
    slots, steps 2-3 with the moved ones in B and the rest in A; then steps 2-3 of the moved ones in A as well: the
    source was not modified.  -> the items compared after the move"""
    fam = family(kind)
    rng = np.random.default_rng(5 + nconn)
    slot_of = rng.permutation(NA)[:nconn].astype(np.uint32)
    everyone = np.arange(nconn)
    whole_a, a = scratch_of(torch, fam, NA)
    for k in range(CUT):
        run_listed(torch, kind, dense, want, everyone, k, a, slot_of, NA, cont=k > 0)
    moved = moved_set(nconn)
    rest = np.setdiff1d(everyone, moved)
    slot_b = rng.permutation(NB)[:moved.size].astype(np.uint32)
    before = a.cpu().numpy().copy()
    im = export(torch, fam, a, NA, slot_of[moved])
    assert (im.status == 0).all() and (a.cpu().numpy() == before).all(), "export wrote scratch"
    for j, c in enumerate(moved):  # compact: header, state, 32 bytes an entry or record, the strings
        assert im.len[j] % 16 == 0 and 96 <= im.len[j] <= C.conn_image_bound(fam)
    ctx = torch.cuda.device(dev_b) if dev_b is not None else torch.cuda.device(torch.cuda.current_device())
    with ctx:
        whole_b, b = scratch_of(torch, fam, NB)
        imb = im.to("cuda:%d" % dev_b) if dev_b is not None else im
        assert (imp(torch, fam, b, NB, slot_b, imb) == 0).all()
        idle = np.setdiff1d(np.arange(NB), slot_b)
        assert (b.cpu().numpy().reshape(NB, -1)[idle] == FILL).all() and T.guards_ok(whole_b)
        if before_b:
            before_b(b, slot_b, moved)
        items = 0
        for k in range(CUT, T.STEPS):
            items += run_listed(torch, kind, dense, want, moved, k, b, slot_b, NB)
        assert T.guards_ok(whole_b)
    for k in range(CUT, T.STEPS):
        run_listed(torch, kind, dense, want, rest, k, a, slot_of[rest], NA)
        run_listed(torch, kind, dense, want, moved, k, a, slot_of[moved], NA)
    assert T.guards_ok(whole_a)
    return items


# 1. move and continue
@pytest.mark.parametrize("nconn", [70, 1, 64])
@pytest.mark.parametrize("kind", list(T.KINDS))
def test_move_and_continue(torch, kind, nconn):
    want = T.dense_run(torch, kind, nconn)  # (first: it gives the sessions their decoder streams)
    dense = T.dense_session(kind, nconn)
    checks = []

    def mode_mismatch(b, slot_b, moved):
        # 2. a session moved under HHUFF_QENC_EVICT and called without the flag is refused, as at its source, and
        # the refusal leaves its slab as it is
        step = step_of(kind, dense, moved[:3], CUT)
        before = b.cpu().numpy().copy()
        r = T.call(torch, "qpenc", step, b, T.CONT, T.Slots(slot_b[:3], None, NB))
        assert (r["rstatus"] == T.EINVAL).all() and (r["dec_status"] == T.EINVAL).all()
        assert (b.cpu().numpy() == before).all()
        checks.append(1)
    items = move_and_continue(torch, kind, nconn, dense, want, before_b=mode_mismatch if kind == "qpenc_evict" else None)
    assert nconn == 1 or items > nconn // 2  # the comparison saw real blocks / sections / responses after the move
    assert checks or kind != "qpenc_evict"


# 5. two devices
@pytest.mark.parametrize("kind", ["requests", "qpenc_evict"])
def test_move_to_another_device(torch, kind):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    want = T.dense_run(torch, kind, 70)
    assert move_and_continue(torch, kind, 70, T.dense_session(kind, 70), want, dev_b=1) > 35


# 2. states that matter at the cut: HPACK decoders
def hpack_session_at(kind, nconn, table, extras=None):
    """the slots tests' session of a Blocks kind at another table size, with hand-built connections behind the
    generated ones (extras: per connection a list of STEPS chunks)"""
    make = HS.make_response_connections if kind == "responses" else HS.make_connections
    kw = {} if kind == "responses" else dict(request_frac=0.2)
    # (at least a block a connection: the generator's mutations want one)
    st = SP.hpack_session(make(nconn, (1, 3 * T.STEPS), seed=16, table_size=table, **kw), T.STEPS, 16)
    if extras:
        st = [SP.Blocks.pack([SP.Blocks.chunk(s, c) for c in range(nconn)] + [e[k] for e in extras], s)
              for k, s in enumerate(st)]
    return st


@pytest.mark.parametrize("table", [256, 0])
@pytest.mark.parametrize("kind", ["blocks", "requests", "responses"])
def test_hpack_decoders_at_small_tables(torch, monkeypatch, kind, table):
    monkeypatch.setattr(T, "TABLE", table)
    nconn = 70
    dense = hpack_session_at(kind, nconn, table)
    want, _, scr = T.run_dense(torch, kind, dense[:CUT])
    if table == 256:  # some moved connection's table has evicted and its entry ring does not start at slot 0:
        # `start` steps down one slot an insert from 0, so start + num > E says more inserts than live entries
        E = table // 32 + 1
        st = T.slabs(scr, kind)[:, :8].copy().view(np.uint32)
        assert any(st[c, 0] != 0 and st[c, 0] + st[c, 1] > E for c in moved_set(nconn))
    want = T.run_dense(torch, kind, dense)[0]
    assert move_and_continue(torch, kind, nconn, dense, want) > (35 if table else 0)


def lit(name, value):
    return bytes([0x40, len(name)]) + name + bytes([len(value)]) + value  # literal with incremental indexing


def test_hpack_failed_and_resized_connections(torch):
    """two hand-built connections behind 69 generated ones, both among the moved.  69: fails in step 0 (the indexed field 62 on an empty
    table), so its later blocks are HHUFF_BLK_SKIPPED, after the move as in the dense run.  70: inserts two entries,
    takes a dynamic table size update to 64 before the cut; after it an insert that must evict under that capacity
    and an indexed reference to it, then a reference past the one entry the table can hold."""
    kind, nconn = "blocks", 69
    failing = [dict(blocks=[bytes([0xBE])]), dict(blocks=[]), dict(blocks=[lit(b"a", b"b")]), dict(blocks=[lit(b"c", b"d")])]
    resized = [dict(blocks=[lit(b"aaaa", b"bbbb") + lit(b"eeee", b"ffff")]), dict(blocks=[bytes([0x3F, 0x21, 0xBE])]),
               dict(blocks=[lit(b"cccc", b"dddd") + bytes([0xBE])]), dict(blocks=[bytes([0xBE]), bytes([0xBF])])]
    dense = hpack_session_at(kind, nconn, T.TABLE, [failing, resized])
    want = T.run_dense(torch, kind, dense)[0]
    assert want[(69, 0)][1][0][0] == -9  # COMPRESSION
    assert [it[0] for it in want[(69, 2)][1] + want[(69, 3)][1]] == [SKIPPED, SKIPPED]
    assert want[(70, 1)][1][0][:3] == (0, 1, ((b"eeee", b"ffff", 0),))  # the update kept the newest entry (40 <= 64)
    assert want[(70, 2)][1][0][:3] == (0, 2, ((b"cccc", b"dddd", 0), (b"cccc", b"dddd", 0)))
    assert [it[0] for it in want[(70, 3)][1]] == [0, -9]  # one entry left: index 63 is past the table
    assert {69, 70} <= set(moved_set(nconn + 2).tolist())
    move_and_continue(torch, kind, nconn + 2, dense, want)


# 2. QPACK decoder
def test_qpack_decoder_partial_stream_and_blocked_section(torch):
    """a hand-built connection behind the generated ones: its encoder stream ends inside an instruction in steps 0
    and 1 (enc_consumed < enc_len: the caller feeds the rest again), its section of step 1 needs three inserts and
    blocks; after the move the third insert arrives and the section, submitted again, decodes"""
    from test_qpdec_sessions import ins, sec

    kind, nconn = "qpack", 70
    base = T.dense_session(kind, nconn, seed=9)
    extra = [dict(sections=[], enc=ins(1) + ins(2)[:3], stream_id=[]),
             dict(sections=[sec(3)], enc=ins(2) + ins(3)[:4], stream_id=[40000]),
             dict(sections=[sec(3)], enc=ins(3), stream_id=[40000]),
             dict(sections=[sec(1), sec(3)], enc=b"", stream_id=[40004, 40008])]
    dense = [SP.QpackDecode.pack([SP.QpackDecode.chunk(s, c) for c in range(nconn)] + [extra[k]], s) for k, s in enumerate(base)]
    want = T.run_dense(torch, kind, dense)[0]
    for k in (0, 1):
        (est, consumed, _), items = want[(nconn, k)]
        assert est == 0 and 0 < consumed < len(extra[k]["enc"])
    assert want[(nconn, 1)][1][0][0] == QPK_BLOCKED
    assert want[(nconn, 2)][0][:2] == (0, len(ins(3))) and want[(nconn, 2)][1][0][:2] == (0, 5)
    assert [it[0] for it in want[(nconn, 3)][1]] == [0, 0]
    assert nconn in moved_set(nconn + 1)
    move_and_continue(torch, kind, nconn + 1, dense, want)


# 2. QPACK encoder sessions whose tables turn over
@pytest.mark.parametrize("H", [128, 256])
def test_evicting_sessions_move_at_every_step(torch, oracle_codec, H):
    """the turnover sessions of tests/test_qpenc_evict.py against the evicting model in a closed loop with the
    restatement's decoder; between any two steps every session goes from its dense scratch into permuted slots of a
    131-slot scratch and from there into a new dense one -- with evicted prefixes, wrapped entry rings, inflight
    sections whose acknowledgments arrive after the move, and entries the peer has not acknowledged"""
    import qpenc_evict_model as M
    from oracle import oracle as O
    from test_qpenc_dyn import closed_loop, cpu_decoder, same
    from test_qpenc_evict import EGpu, EV, turnover

    nconn = 70
    fam = C.conn_family(C.FAM_QPACK_ENC, H, 64)
    st = turnover(nconn, 6, 95)
    m, g = M.Model(nconn, H), EGpu(torch, nconn, H)
    seen = dict(evicted=0, wrapped=0, blocking=0, unacked=0)

    def encode(s, q, dec):
        flags = EV | (C.QENC_CONTINUE if s else C.QENC_SET_CAPACITY)
        if s:
            for c in m.conns:
                seen["evicted"] += c.evicted > 0
                seen["wrapped"] += c.evicted > 0 and c.count > H // 32
                seen["blocking"] += any(e[2] for e in c.inflight)
                seen["unacked"] += c.lkr < c.count
            g.scratch = hop(torch, fam, g.scratch, nconn, 30 + s)[1]
        w = m.step(q, dec, flags=flags)
        w["count"] = m.counts()
        same(g.step(q, dec, flags=flags), w, "step %d: " % s)
        return w
    closed_loop(st, encode, cpu_decoder(O.oracle(), nconn, H, 100, False), False)
    assert all(v > 0 for v in seen.values()), seen


# 2. decoder sessions: the table slab and the session slab move together
def test_decoder_sessions_move_with_parked_streams(torch, oracle_codec):
    """the withheld-encoder-stream sessions of tests/test_qpdec_sessions.py: after step 1 the odd connections have
    parked streams; both slabs of every connection go from the dense scratch and state into permuted slots of
    131-slot ones, and the streams wake, cancel and acknowledge there as in the model"""
    import qpdec_session_model as DM
    import test_qpdec_sessions as QT

    nconn, mb = 70, 2
    tfam, sfam = C.conn_family(C.FAM_QPACK_DEC, QT.H), C.conn_family(C.FAM_QPACK_DSESSION, max_blocked=mb)
    g = QT.Gpu(torch, nconn, mb)
    rng = np.random.default_rng(4)
    via = rng.permutation(NA)[:nconn]
    seen = dict(parked_at_cut=0, woken_after=0)

    def replay(k, st, sid, kw, want):
        if k == CUT:
            seen["parked_at_cut"] = int(sum(len(s.parked) for s in model_before["sess"]))
            g2 = QT.Gpu(torch, NA, mb)
            whole_t, t = scratch_of(torch, tfam, NA)
            whole_s, s = BH.guarded(torch, C.conn_slab_size(sfam) * NA, 0xA5, QT.GUARD)
            every = np.arange(nconn)
            assert (imp(torch, tfam, t, NA, via, export(torch, tfam, g.scratch, nconn, every)) == 0).all()
            assert (imp(torch, sfam, s, NA, via, export(torch, sfam, g._state(), nconn, every)) == 0).all()
            g2.scratch, g2.state_whole = t, whole_s
            g.scratch.fill_(0x11)
            g.state_whole.fill_(0x11)
            state["g"] = g2
        gg = state["g"]
        got = gg.step(st, sid, **(dict(kw, slot=via) if gg is not g else kw))
        QT.same(got, want, "step %d: " % k)
        if k >= CUT:
            seen["woken_after"] += int(want["nwake"].sum())
        model_before["sess"] = [type("S", (), dict(parked=list(x.parked)))() for x in model.sess]

    state, model_before = dict(g=g), dict(sess=[])
    model = DM.Model(oracle_codec, nconn, QT.H, mb)
    QT.withheld_sessions(nconn, 11, False, model, replay)
    assert seen["parked_at_cut"] > nconn // 4 and seen["woken_after"] > nconn // 8, seen


def test_closed_loop_with_both_halves_moved(torch, oracle_codec):
    """hhuff_qpack_flatten_sessions -> the session decoder -> its decoder stream into the encoder's next step, as
    tests/test_qpdec_sessions.py runs it against the two models; here every connection's encoder session, decoder
    table and decoder session move between any two steps.  The encoder streams of step 1 are withheld, so streams
    are parked and sections inflight and blocking at a cut; in the end every num_blocked is back at 0."""
    import qpdec_session_model as DM
    import qpenc_dyn_model as EM
    import test_qpdec_sessions as QT
    import test_qpenc_dyn as QD

    nconn = 70
    efam = C.conn_family(C.FAM_QPACK_ENC, QT.H, 64)
    tfam, sfam = C.conn_family(C.FAM_QPACK_DEC, QT.H), C.conn_family(C.FAM_QPACK_DSESSION, max_blocked=100)
    enc_m = EM.Model(nconn, QT.H, 100)
    dec_m = DM.Model(oracle_codec, nconn, QT.H, 100, responses=True)
    g = QT.Gpu(torch, nconn, 100, responses=True)
    state = dict(scratch=None, blocked_at_cut=0, parked_at_cut=0)

    def encode(s, q, dec):
        flags = C.QENC_CONTINUE if s else C.QENC_SET_CAPACITY
        if s:
            state["blocked_at_cut"] += sum(c.num_blocked for c in enc_m.conns)
            im = export(torch, efam, state["scratch"], nconn, np.arange(nconn))
            for c, conn in enumerate(enc_m.conns):  # the image's state record: ninflight, num_blocked
                b = im.bytes(c)
                assert int(np.frombuffer(b[36:40], np.uint32)[0]) == len(conn.inflight)
                assert int(np.frombuffer(b[76:80], np.uint32)[0]) == conn.num_blocked
            state["scratch"] = hop(torch, efam, state["scratch"], nconn, 50 + s)[1]
        r, state["scratch"] = QT.encoder_step(torch, q, state["scratch"], dec and dec["t"], flags)
        QD.same(r, enc_m.step(q, dec and dec["host"], flags=flags), "encoder step %d: " % s)
        return r

    def decode(s, st, sid):
        if s:
            state["parked_at_cut"] += sum(len(x.parked) for x in dec_m.sess)
            g.scratch = hop(torch, tfam, g.scratch, nconn, 60 + s)[1]
            g.state_whole = hop(torch, sfam, g._state(), nconn, 70 + s, fill=0xA5)[0]
        d = g.step(st, sid, cont=s > 0)
        QT.same(d, dec_m.step(st, sid, cont=s > 0), "decoder step %d: " % s)
        t = d["t"]
        return dict(t=(t["dec_out"], t["dec_out_off"], t["dec_out_len"]), host=d["dec"], len=d["dec_out_len"]), d

    def finish(dec):
        for c, conn in enumerate(enc_m.conns):
            assert conn.handle_input(dec["host"][c]) == (0, len(dec["host"][c]))
            assert conn.num_blocked == 0 and not conn.inflight, c
    QT.closed_loop(nconn, False, encode, decode, finish)
    assert state["blocked_at_cut"] > 0 and state["parked_at_cut"] >= nconn, state


# 3. canonical and position-free
@pytest.mark.parametrize("kind", T.MAIN)
def test_images_are_canonical(torch, kind):
    nconn = 70
    T.dense_run(torch, kind, nconn)
    dense = T.dense_session(kind, nconn)
    fam = family(kind)
    every = np.arange(nconn)
    # the dense session, two steps, connection c in slot c
    whole_a, a = scratch_of(torch, fam, nconn)
    for k in range(CUT):
        T.call(torch, kind, dense[k], a, T.CONT if k else 0, None)
    first = export(torch, fam, a, nconn, every)
    images = [first.bytes(c) for c in every]
    # export -> import into another slot of another scratch -> export: the same bytes
    rng = np.random.default_rng(6)
    via = rng.permutation(NB)[:NB]
    some = every[:NB]
    whole_b, b = scratch_of(torch, fam, NB)
    sub = export(torch, fam, a, nconn, some)
    assert (imp(torch, fam, b, NB, via, sub) == 0).all() and T.guards_ok(whole_b)
    again = export(torch, fam, b, NB, via)
    assert [again.bytes(j) for j in range(NB)] == [images[c] for c in some]
    # the same session through another slot map, another partition into calls and a scratch elsewhere
    slot_of = rng.permutation(NA)[:nconn]
    evens, odds = every[::2], every[1::2]
    plan = SP.Plan(T.KINDS[kind], dense, slot_of, [evens, odds, odds[::-1], evens[::-1]])
    whole_c, c = scratch_of(torch, fam, NA)
    for t, (step, slot, keys) in enumerate(plan.steps):
        flags = np.asarray([C.CONN_RESET if k == 0 else 0 for _, k in keys], np.uint8)
        T.call(torch, kind, step, c, T.CONT if t else 0, T.Slots(slot, flags if t else None, NA))
    other = export(torch, fam, c, NA, slot_of)
    bad = [int(x) for x in every if other.bytes(x) != images[x]]
    assert not bad, (kind, bad[:8])
    assert len(set(images)) > nconn // 4  # (and the images do tell connections apart)


def test_small_images(torch, monkeypatch):
    """a fresh connection is 96 bytes; after one block that inserts `x-a: b` at table size 65536 the image is the
    fixed part, one record and four string bytes: 144 with the pad"""
    monkeypatch.setattr(T, "TABLE", 65536)
    fam = family("blocks")
    like = dict(table_size=65536)
    whole, scr = scratch_of(torch, fam, 2)
    step = SP.Blocks.pack([dict(blocks=[]), dict(blocks=[lit(b"x-a", b"b")])], like)
    r = T.call(torch, "blocks", step, scr, 0, None)
    assert list(r["bstatus"]) == [0] and int(r["nfields"][0]) == 1
    im = export(torch, fam, scr, 2, [0, 1])
    assert list(im.len) == [96, 144] and im.len[1] <= 96 + 32 * 1 + 4 + 15
    assert C.conn_image_bound(fam) >= 96 + 32 * (65536 // 32) + 65536 + 15


# 4. footprints and refusals
def exported_after_two_steps(torch, kind, nconn=70):
    T.dense_run(torch, kind, nconn)
    dense = T.dense_session(kind, nconn)
    fam = family(kind)
    whole, a = scratch_of(torch, fam, nconn)
    for k in range(CUT):
        T.call(torch, kind, dense[k], a, T.CONT if k else 0, None)
    return fam, a


@pytest.mark.parametrize("kind", ["requests", "qpenc_evict"])
def test_export_footprints(torch, kind):
    nconn = 70
    fam, a = exported_after_two_steps(torch, kind)
    every = np.arange(nconn)
    exact = export(torch, fam, a, nconn, every)
    assert (exact.status == 0).all()
    # regions with 32 bytes to spare: nothing past img_len is written, the bytes between the strings and img_len are 0
    wide = export(torch, fam, a, nconn, every, room=lambda need: need.astype(np.int64) + 32)
    raw = wide.img.cpu().numpy()
    padded = 0
    for c in every:
        o, n = int(wide.off[c]), int(wide.len[c])
        assert raw[o:o + n].tobytes() == exact.bytes(c)
        assert (raw[o + n:int(wide.off[c + 1])] == SENT).all()
        nent, nlist, strs = (int(x) for x in raw[o + 32:o + 44].view(np.uint32))
        end = 96 + 32 * nent + 16 * nlist + strs
        assert n == (end + 15) // 16 * 16 and not raw[o + end:o + n].any()
        padded += n != end
    assert padded > nconn // 4
    # regions 16 bytes short: HHUFF_IMG_SPACE, the length needed, the region still the sentinel; every third only
    short = export(torch, fam, a, nconn, every, room=lambda need: need.astype(np.int64) - 16 * (np.arange(need.size) % 3 == 0))
    raw = short.img.cpu().numpy()
    for c in every:
        o, e = int(short.off[c]), int(short.off[c + 1])
        assert short.len[c] == exact.len[c]
        if c % 3 == 0:
            assert short.status[c] == C.IMG_SPACE and (raw[o:e] == SENT).all()
        else:
            assert short.status[c] == 0 and raw[o:e].tobytes() == exact.bytes(c)
    # several items may name one slot; a slot >= nslots is refused alone
    odd = export(torch, fam, a, nconn, [3, 3, nconn, 0xFFFFFFFF, 5])
    assert list(odd.status) == [0, 0, C.IMG_EINVAL, C.IMG_EINVAL, 0] and list(odd.len[2:4]) == [0, 0]
    assert odd.bytes(0) == odd.bytes(1) == exact.bytes(3) and odd.bytes(4) == exact.bytes(5)


@pytest.mark.parametrize("kind", ["requests", "qpenc_evict"])
def test_import_refusals(torch, kind):
    nconn = 70
    fam, a = exported_after_two_steps(torch, kind)
    slab = C.conn_slab_size(fam)
    every = export(torch, fam, a, nconn, np.arange(nconn))
    counts = [tuple(int(x) for x in np.frombuffer(every.bytes(c)[32:40], np.uint32)) for c in range(nconn)]
    # a connection with entries and (sessions) inflight records to edit
    src = next(c for c in range(nconn) if counts[c][0] >= 2 and (kind != "qpenc_evict" or counts[c][1] >= 1))
    im = export(torch, fam, a, nconn, [src] * 16)
    good = im.bytes(0)
    nent, nlist = counts[src]

    # slots: out of range, and a slot an earlier item names
    whole_b, b = scratch_of(torch, fam, NB)
    st = imp(torch, fam, b, NB, [7, NB, 7, 0xFFFFFFFF, 9, 7][:6], Images(torch, im.whole, im.img, im.off[:7], im.len[:6], None))
    assert list(st) == [0, C.IMG_EINVAL, C.IMG_EINVAL, C.IMG_EINVAL, 0, C.IMG_EINVAL]
    slabs = b.cpu().numpy().reshape(NB, slab)
    assert (slabs[np.setdiff1d(np.arange(NB), [7, 9])] == FILL).all() and T.guards_ok(whole_b)
    assert export(torch, fam, b, NB, [7, 9]).bytes(0) == good  # the winner is imported

    # edited images: each a valid image with one named field changed
    raw = im.img.cpu().numpy().copy()
    E = {"requests": T.TABLE // 32 + 1, "qpenc_evict": T.TABLE // 32}[kind]

    def word(k, off):
        return raw[int(im.off[k]) + off:int(im.off[k]) + off + 4].view(np.uint32)
    lens = im.len.copy()
    edits = [("magic", C.IMG_EFORMAT), ("version", C.IMG_EFORMAT), ("length", C.IMG_EFORMAT), ("reserved", C.IMG_EFORMAT),
             ("img_len", C.IMG_EFORMAT), ("family", C.IMG_EPARAM), ("table_size", C.IMG_EPARAM), ("nent", C.IMG_EFORMAT),
             ("entry length", C.IMG_EFORMAT), ("used", C.IMG_EFORMAT), ("state reserved", C.IMG_EFORMAT), ("pad", C.IMG_EFORMAT)]
    word(0, 0)[0] ^= 1
    raw[int(im.off[1]) + 4] = 2
    word(2, 20)[0] += 16
    word(3, 28)[0] = 1
    lens[4] -= 16
    raw[int(im.off[5]) + 6] = C.FAM_QPACK_DEC if kind == "requests" else C.FAM_HPACK_DEC
    word(6, 8)[0] = T.TABLE // 2
    word(7, 32)[0] = E + 1
    word(8, 96 + 32)[0] += 1 << 20
    word(9, 48)[0] += 1
    word(10, 88)[0] = 1
    if kind == "qpenc_evict":
        edits += [("ninflight", C.IMG_EFORMAT), ("evicted", C.IMG_EFORMAT), ("lkr", C.IMG_EFORMAT), ("largest", C.IMG_EFORMAT)]
        word(12, 36)[0] = T.MAX_INFLIGHT + 1
        word(13, 80)[0] = int(word(13, 64)[0]) + 1       # evicted > count
        word(14, 72)[0] = int(word(14, 64)[0]) + 1       # lkr > count
        word(15, 96 + 32 * nent + 8)[0] = int(word(15, 64)[0]) + 1  # an inflight section's largest reference
    strs = int(np.frombuffer(good[40:44], np.uint32)[0])
    if strs % 16:
        raw[int(im.off[11]) + int(im.len[11]) - 1] = 1
    else:
        edits[11] = ("none", 0)
    n = len(edits)
    whole_m, inner = BH.guarded(torch, raw.size, SENT)
    inner.copy_(torch.from_numpy(raw).cuda())
    whole_b, b = scratch_of(torch, fam, NB)
    st = imp(torch, fam, b, NB, np.arange(n) + 20, Images(torch, whole_m, inner, im.off[:n + 1], lens[:n], None))
    assert [(name, int(s)) for (name, _), s in zip(edits, st)] == [(name, want) for name, want in edits]
    slabs = b.cpu().numpy().reshape(NB, slab)
    ok = [20 + k for k, (_, want) in enumerate(edits) if want == 0]
    assert (slabs[np.setdiff1d(np.arange(NB), ok)] == FILL).all() and T.guards_ok(whole_b)

    # the same images into a scratch of another family, and of the same family at another table size
    for other in (C.conn_family(C.FAM_HPACK_ENC), C.conn_family(fam.family, T.TABLE * 2, fam.max_inflight)):
        whole_o, o = scratch_of(torch, other, 3)
        st = imp(torch, other, o, 3, [0, 1, 2], Images(torch, im.whole, im.img, im.off[:4], im.len[:3], None))
        assert (st == C.IMG_EPARAM).all() and (whole_o.cpu().numpy() == FILL).all()
