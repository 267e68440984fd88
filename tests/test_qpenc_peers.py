"""QPACK encoder sessions with per-connection peer settings (include/hhuff.h (2g''),
hhuff_qpack_flatten_sessions_peers): one call steps connections whose peers advertised different table capacities and
blocked-stream limits, in one scratch of equal slabs.
CPU: the export and the host-only refusals; the peers model (tests/qpenc_peers_model.py: one uniform model per
connection, the MaxEntries and stability overrides) round-tripped through the decoders, every connection decoded at
the capacity its peer advertised -- the restatement always, the real qpack.c where oracle/_ref is built; the table
operations at capacities under the slab's on the host under sanitizers (tools/qtable_host.cpp).
GPU: a mixed population against the uniform entry point run over each settings group alone and against the model;
a peer that advertised more than the slab holds (the Required Insert Count wraps at the advertised MaxEntries); the
stability refusal; a slot reused by another peer; the pass-through with peers NULL; encoder-stream regions of exactly
cap_c + 4 bytes."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import qpenc_evict_model as E
import qpenc_peers_model as PM
from h2o_amd import codec as C
from h2o_amd import hpenc_synth as HE
from test_qpenc_dyn import (LTR, Gpu, acks_of, batch, closed_loop, cpu_decoder, decoded_fields, edge_scripts, fields_of,
                            gpu_decoder, per_conn, resp, run_script, same, section_lines, section_of)
from test_qpenc_evict import evict_scripts, script_steps, turnover, with_enc_regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EV, DUP, CONT, SETCAP = C.QENC_EVICT, C.QENC_DUP, C.QENC_CONTINUE, C.QENC_SET_CAPACITY
CAPACITIES, BLOCKED = (0, 31, 32, 64, 220, 1024, 4096), (0, 1, 2, 100)


def mixed_population():
    """the 65 peers of the equivalence test: one 64-lane workgroup of the walk plus one lane"""
    return HE.qpack_peer_population(65, CAPACITIES, BLOCKED, seed=7)


def peer(cap, blocked=100):
    return np.array([(cap, blocked)], C.QPACK_PEER)


def peers_of(*records):
    return np.array(list(records), C.QPACK_PEER)


def clamp_steps(nconn=3, steps=14):
    """per connection and step one response with ten likely-to-repeat headers never seen before: 47 bytes an entry,
    so a table of 1024 bytes holds two steps' worth and turns over once the acknowledgments come back; after 13 steps
    the insert count passes 128 = 2 * (2048 / 32)"""
    return [with_enc_regions(batch([[resp([(b"link", b"</%02d/%02d/%02d>" % (c, s, j), LTR) for j in range(10)],
                                          stream_id=4 * s)] for c in range(nconn)]))
            for s in range(steps)]


def groups_by_capacity(peers):
    """[(advertised capacity, connections)]: the decoders' view, one decoder per distinct capacity"""
    caps = peers["max_table_capacity"]
    return [(int(cap), [int(c) for c in np.flatnonzero(caps == cap)]) for cap in np.unique(caps)]


def peers_loop(steps, encode, decoders):
    """test_qpenc_dyn.closed_loop with one decoder per group of connections: decoders = [(connections, decode)].
    Every step: the encoder streams are consumed whole, every section decodes to its response's fields, a section is
    acknowledged exactly when the encoder made it inflight; the acknowledgments are the next step's decoder stream"""
    dec, log = None, []
    for s, q in enumerate(steps):
        r = encode(s, q, dec)
        n, nconn = q["res"].size, q["conn_first"].size - 1
        assert (r["rstatus"][:n] == 0).all() and (r["dec_status"][:nconn] == 0).all()
        if dec is not None:
            np.testing.assert_array_equal(r["dec_consumed"][:nconn], [len(x) for x in dec])
        acks = [b""] * n
        for conns, decode in decoders:
            sq = PM.subset(q, conns)
            idx = sq["_responses"]
            d = decode(sq, [r["frames"][k] for k in idx], [r["enc"][c] for c in conns])
            assert (d["enc_status"][:len(conns)] == 0).all(), (s, conns)
            np.testing.assert_array_equal(d["enc_consumed"][:len(conns)], r["enc_out_len"][conns])
            assert (d["sstatus"][:idx.size] == 0).all(), (s, conns, np.flatnonzero(d["sstatus"][:idx.size])[:8])
            for j in range(idx.size):
                assert decoded_fields(d, d["sec_off"], j) == fields_of(sq, j), (s, conns, j)
            a = acks_of(d, sq, False)
            np.testing.assert_array_equal([len(x) > 0 for x in a], r["inflight"][idx])
            for j, k in enumerate(idx):
                acks[k] = a[j]
        dec = per_conn(q, acks)
        log.append((q, r))
    return log


def cpu_decoders(codec, peers):
    return [(conns, cpu_decoder(codec, len(conns), cap, 100, False)) for cap, conns in groups_by_capacity(peers)]


def model_encoder(m, mode):
    def encode(s, q, dec):
        return m.step(q, dec, flags=mode | (CONT if s else SETCAP))
    return encode


def rics(log, nconn):
    """per connection: the Required Insert Counts as written, in order, of the sections that have one"""
    out = [[] for _ in range(nconn)]
    for q, r in log:
        cf = q["conn_first"]
        for c in range(nconn):
            for k in range(int(cf[c]), int(cf[c + 1])):
                ric = section_lines(section_of(r["frames"][k]))[0]
                if ric:
                    out[c].append(ric)
    return out


# ---------------------------------------------------------------------------------------------------
# CPU 1: the export and the host-only refusals (nothing here touches a GPU)
# ---------------------------------------------------------------------------------------------------
def test_export_and_host_only_refusals():
    from h2o_amd import build

    build.build(verbose=False)
    L = C.lib()
    assert "hhuff_qpack_flatten_sessions_peers" in C.EXPORTED
    nul = [None] * 12

    def call(peers, nconn=1, H=4096, flags=0, slots=None):
        """every array NULL: only the host's checks can answer"""
        return L.hhuff_qpack_flatten_sessions_peers(peers, slots, None, 0, None, 0, None, None, nconn, 0, None, None, None,
                                                    H, 100, 64, 0, 0, *nul, 0, flags, None)
    buf = (ctypes.c_uint32 * 4)()
    aligned = ctypes.addressof(buf)
    for odd in (1, 2, 3):  # a peers pointer that is not 4-byte aligned: HHUFF_EINVAL, whatever else the call says
        assert call(aligned + odd) == -1 and call(aligned + odd, nconn=0) == -1
    assert b"peers" in L.hhuff_last_error_string()
    # what the _slots call refuses, with peers given or not
    for p in (None, aligned):
        assert call(p, H=65537) == C.RES_EINVAL and call(p, flags=16) == C.RES_EINVAL and call(p, flags=DUP) == C.RES_EINVAL
        assert call(p) == -1  # NULL arrays
        assert call(p, nconn=0) == 0
        st = C._ConnSlotsStruct(None, None, 0)  # nslots 0
        assert call(p, slots=ctypes.byref(st)) == -1


def test_header_declares_the_record():
    text = open(os.path.join(ROOT, "include", "hhuff.h")).read()
    assert "hhuff_qpack_flatten_sessions_peers(const hhuff_qpack_peer_t *peers" in text
    assert C.QPACK_PEER.itemsize == 8 and C.QPACK_PEER.names == ("max_table_capacity", "max_blocked")


def test_population_helper():
    p = mixed_population()
    assert p.dtype == C.QPACK_PEER and p.size == 65
    assert set(p["max_table_capacity"]) == set(CAPACITIES) and set(p["max_blocked"]) == set(BLOCKED)
    key = p["max_table_capacity"].astype(np.int64) * 1000 + p["max_blocked"]
    assert (key[1:] != key[:-1]).sum() >= 56  # the lanes of a wave differ from their neighbours
    assert (HE.qpack_peer_population(65, CAPACITIES, BLOCKED, seed=7) == p).all()


# ---------------------------------------------------------------------------------------------------
# CPU 2: the model against the decoders, every connection decoded at the capacity its peer advertised
# ---------------------------------------------------------------------------------------------------
def loop_case(name):
    """-> steps, peers, H, mode"""
    if name == "clamp":
        return clamp_steps(), peers_of((2048, 100), (2048, 100), (2048, 100)), 1024, EV
    return turnover(65, 6, 97), mixed_population(), 4096, {"mixed": 0, "mixed_evict": EV, "mixed_dup": EV | DUP}[name]


def check_case(name, m, log):
    if name == "clamp":
        assert (m.counts() > 128).all() and (m.used() <= 1024).all()
        assert any(b < a for seq in rics(log, 3) for a, b in zip(seq, seq[1:])), "no Required Insert Count wrapped"
        assert max(max(seq) for seq in rics(log, 3)) > 64  # past the modulus of a 1024-byte table
    else:
        caps = np.minimum(m.peers["max_table_capacity"], m.H)
        assert (m.used() <= caps).all() and (m.counts()[caps < 32] == 0).all()
        assert (m.counts()[(caps >= 220) & (m.peers["max_blocked"] > 0)] > 0).all()  # (no buffer at a limit of 0)


CASES = ["mixed", "mixed_evict", "mixed_dup", "clamp"]


@pytest.mark.parametrize("name", CASES)
def test_model_round_trip_restatement(oracle_codec, name):
    from oracle import oracle as O

    st, peers, H, mode = loop_case(name)
    m = PM.Model(peers, H, 100)
    check_case(name, m, peers_loop(st, model_encoder(m, mode), cpu_decoders(O.oracle(), peers)))


@pytest.mark.parametrize("name", CASES[:2] + ["clamp"])
def test_model_round_trip_reference(oracle_codec, name):
    from oracle import oracle as O

    if not O.ref_available():
        pytest.skip("oracle/_ref not built")
    st, peers, H, mode = loop_case(name)
    m = PM.Model(peers, H, 100)
    peers_loop(st, model_encoder(m, mode), cpu_decoders(O.ref(), peers))


def test_model_is_the_uniform_model_per_group(oracle_codec):
    """point 4 on the CPU: the splitter and the merger change nothing -- a group of connections with one setting,
    stepped by the uniform evicting model at that setting, gives the slice of the peers model's result"""
    st, peers = turnover(65, 3, 98), mixed_population()
    m = PM.Model(peers, 4096, 100)
    conns = [int(c) for c in np.flatnonzero((peers["max_table_capacity"] == 220) & (peers["max_blocked"] == 2))]
    assert len(conns) >= 2
    u = E.Model(len(conns), 220, 2)
    for s, q in enumerate(st):
        flags = EV | (CONT if s else SETCAP)
        w, sq = m.step(q, None, flags), PM.subset(q, conns)
        g = u.step(sq, None, flags)
        assert [w["frames"][k] for k in sq["_responses"]] == g["frames"] and [w["enc"][c] for c in conns] == g["enc"]
        np.testing.assert_array_equal(w["rstatus"][sq["_responses"]], g["rstatus"])


def test_model_stability_refusal_and_maxentries(oracle_codec):
    q = with_enc_regions(batch([[resp([(b"link", b"</path/%02d>" % j, LTR) for j in range(10)])]]))
    m = PM.Model(peer(1024), 1024)
    r0 = m.step(q, None, EV | SETCAP)
    assert r0["enc"][0][:3] == E.encode_int(1024, 5, 0x20) and m.conn(0).used > 64
    before = (m.conn(0).used, m.conn(0).count, list(m.conn(0).inflight))
    r1 = m.step(q, None, EV | CONT, peers=peer(64))
    assert r1["rstatus"][0] == C.RES_EINVAL and r1["dec_status"][0] == C.RES_EINVAL and r1["frames"] == [b""]
    assert (m.conn(0).used, m.conn(0).count, list(m.conn(0).inflight)) == before
    assert m.step(q, None, EV | CONT)["rstatus"][0] == 0
    # under 32 bytes advertised nothing is inserted: no modulus is ever needed
    z = PM.Model(peer(31), 1024)
    assert z.step(q, None, EV | SETCAP)["enc"][0] == E.encode_int(31, 5, 0x20) and z.counts()[0] == 0


# ---------------------------------------------------------------------------------------------------
# CPU 3: the table operations at capacities under the slab's, on the host under sanitizers
# ---------------------------------------------------------------------------------------------------
def test_qtable_host_clean_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "qtable_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "h2o_amd", "csrc"),
                    os.path.join(ROOT, "tools", "qtable_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, "1500"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok: 2 x 1500 sequences"), r.stdout


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


class PGpu(Gpu):
    """Gpu whose steps pass evict= and dup= from the step's flags and, where given, the peer records (peers: a
    QPACK_PEER array, per object or per step), connection slots (slot: the slot of every connection, nslots) with
    per-step reset flags, and the pass-through switch"""

    def __init__(self, torch, nconn, H=4096, max_blocked=100, max_inflight=64, move=False, peers=None, slot=None,
                 nslots=None, peers_call=False):
        super().__init__(torch, nconn, H, max_blocked, max_inflight, move)
        self.peers, self.slot, self.nslots, self.peers_call = peers, slot, nslots, peers_call

    def step(self, q, dec=None, flags=0, guard=64, peers=None, reset=None):
        torch = self.t
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()  # noqa: E731
        kw = dict(evict=bool(flags & EV), dup=bool(flags & DUP), peers_call=self.peers_call)
        p = self.peers if peers is None else peers
        if p is not None:
            kw["peers"] = dev(np.array(p, C.QPACK_PEER).view(np.uint8))
        if self.slot is not None:
            fl = None if reset is None else dev(np.asarray(reset, np.uint8))
            kw["slots"] = C.ConnSlots(dev(np.asarray(self.slot, np.uint32).view(np.int32)), fl, self.nslots)
        real = C.qpack_flatten_sessions
        C.qpack_flatten_sessions = lambda *a, **k: real(*a, **kw, **k)
        try:
            return super().step(q, dec, flags, guard)
        finally:
            C.qpack_flatten_sessions = real


def settings_groups(peers, H, max_blocked):
    """{(cap_c, blocked limit): connections}: the groups the uniform entry point can step alone"""
    g = {}
    for c, p in enumerate(peers):
        g.setdefault((min(int(p["max_table_capacity"]), H), min(int(p["max_blocked"]), max_blocked)), []).append(c)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("mode,slots", [(0, False), (EV, False), (EV | DUP, False), (EV, True)])
def test_gpu_mixed_population_equivalence(torch_cuda, oracle_codec, mode, slots):
    """65 connections, H = 4096, 6 steps with the acknowledgments fed back: every output equals the uniform entry
    point's run over each settings group alone (header_table_size = the group's capacity, max_blocked = its limit)
    and the model's.  slots: the connections sit in a permutation of 70 slots and the scratch is reallocated between
    the steps"""
    from oracle import oracle as O

    st, peers = turnover(65, 6, 97), mixed_population()
    m = PM.Model(peers, 4096, 100)
    kw = dict(slot=np.random.default_rng(3).permutation(70)[:65], nslots=70, move=True) if slots else {}
    g = PGpu(torch_cuda, 65, 4096, 100, peers=peers, **kw)
    groups = settings_groups(peers, 4096, 100)
    assert len(groups) >= 20
    uniform = {k: PGpu(torch_cuda, len(conns), k[0], k[1]) for k, conns in groups.items()}

    def encode(s, q, dec):
        flags = mode | (CONT if s else SETCAP)
        w = m.step(q, dec, flags)
        r = g.step(q, dec, flags)
        same(r, w, "step %d against the model: " % s)
        parts = []
        for k, conns in groups.items():
            u = uniform[k].step(PM.subset(q, conns), None if dec is None else [dec[c] for c in conns], flags)
            assert u["guards_intact"]
            parts.append((conns, u))
        u = PM.merge(q, parts)
        u["guards_intact"] = True
        same(r, u, "step %d against the uniform call per group: " % s)
        return w
    log = peers_loop(st, encode, cpu_decoders(O.oracle(), peers))
    check_case("mixed", m, log)
    assert any(r["blocking"].any() for _, r in log) and any(len(e) > 3 for _, r in log[1:] for e in r["enc"])


@pytest.mark.gpu
def test_gpu_clamp_and_wrap(torch_cuda):
    """3 connections whose peers advertised 2048 bytes in slabs of H = 1024, evicting: the table holds 1024 bytes,
    the Required Insert Count wraps at 2 * (2048 / 32) = 128 -- where the GPU decoder at header_table_size 2048
    expects it -- and not at the 64 of a uniform call at 1024"""
    st, peers = clamp_steps(), peers_of((2048, 100), (2048, 100), (2048, 100))
    m = PM.Model(peers, 1024, 100)
    g, u = PGpu(torch_cuda, 3, 1024, 100, peers=peers), PGpu(torch_cuda, 3, 1024, 100)
    uniform_frames = []

    def encode(s, q, dec):
        flags = EV | (CONT if s else SETCAP)
        w, r = m.step(q, dec, flags), g.step(q, dec, flags)
        same(r, w, "step %d: " % s)
        uniform_frames.append(u.step(q, dec, flags)["frames"])
        r["inflight"], r["count"] = w["inflight"], m.counts()
        return r
    log = closed_loop(st, encode, gpu_decoder(torch_cuda, 3, 2048, 100, False), False)
    log = [(q, r) for q, r, _ in log]
    check_case("clamp", m, log)
    ric = lambda f: section_lines(section_of(f))[0]  # noqa: E731
    differ = [(s, k) for s, (_, r) in enumerate(log) for k in range(3) if ric(r["frames"][k]) != ric(uniform_frames[s][k])]
    assert differ, "no Required Insert Count differs from the uniform call's at 1024"
    s, k = differ[0]
    # both counts fit the prefix's first byte: behind it the delta base and the field lines are the same
    assert section_of(log[s][1]["frames"][k])[1:] == section_of(uniform_frames[s][k])[1:]


def fill_steps(nconn, steps, nh=12):
    """per connection and step one response with nh likely-to-repeat headers never seen before, 47 bytes an entry"""
    return [with_enc_regions(batch([[resp([(b"link", b"</%02d/%02d/%02d>" % (c, s, j), LTR) for j in range(nh)],
                                          stream_id=4 * s)] for c in range(nconn)])) for s in range(steps)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, EV])
def test_gpu_stability_refusal(torch_cuda, mode):
    """a connection that filled its 1024-byte table continues with a record saying 64: refused for the step like the
    mode mismatch, its slab untouched (an export before and after is the same image), its neighbours unaffected; the
    next step, with the right record, goes on as the model says"""
    torch = torch_cuda
    st = fill_steps(3, 3, nh=22)  # 21 entries fill the 1024 bytes, the 22nd finds no room
    ack0 = E.encode_int(0, 7, 0x80)
    right = peers_of((1024, 100), (1024, 100), (1024, 100))
    wrong = peers_of((1024, 100), (64, 100), (1024, 100))
    m, g = PM.Model(right, 1024, 100), PGpu(torch, 3, 1024, 100, peers=right)
    same(g.step(st[0], None, mode | SETCAP), m.step(st[0], None, mode | SETCAP))
    assert m.conn(1).used == 21 * 47
    fam = C.conn_family(C.FAM_QPACK_ENC, 1024, 64)
    one = torch.tensor([1], dtype=torch.int32, device="cuda")

    def image():
        img, _, img_len, status = C.conn_export(fam, g.scratch, 3, one)
        torch.cuda.synchronize()
        assert int(status[0]) == 0
        return img.cpu().numpy()[:int(img_len[0])].tobytes()
    before = image()
    acks = [ack0, ack0, ack0]  # of step 0's sections; the refused connection does not read its own
    r, w = g.step(st[1], acks, mode | CONT, peers=wrong), m.step(st[1], acks, mode | CONT, peers=wrong)
    same(r, w, "the refused step: ")
    assert r["rstatus"][1] == C.RES_EINVAL and r["dec_status"][1] == C.RES_EINVAL and r["out_len"][1] == 0
    assert list(r["rstatus"][[0, 2]]) == [0, 0] and r["enc_out_len"][1] == 0
    assert list(r["dec_consumed"]) == [1, 0, 1]
    o, e = st[1]["out_off"].astype(np.int64), st[1]["enc_out_off"].astype(np.int64)
    assert (r["out_raw"][o[1]:o[2]] == 0xA5).all() and (r["enc_raw"][e[1]:e[2]] == 0xA5).all()
    assert image() == before
    acks = [b"", ack0, b""]
    same(g.step(st[2], acks, mode | CONT), m.step(st[2], acks, mode | CONT), "the step after: ")
    assert image() != before and m.conn(1).lkr == 21 and (m.counts()[1] > 21) == bool(mode & EV)


@pytest.mark.gpu
def test_gpu_slot_reused_by_another_peer(torch_cuda, oracle_codec):
    """HHUFF_CONN_RESET in the slot a 4096-byte peer left, with a 64-byte peer's record and HHUFF_QENC_SET_CAPACITY:
    the encoder stream opens with capacity 64, the table never holds more than 64 bytes, and a decoder at 64 reads
    every field; the neighbour in the next slot goes on"""
    from oracle import oracle as O

    st = fill_steps(2, 4)
    big, small = peers_of((4096, 100), (4096, 100)), peers_of((64, 100), (4096, 100))
    m = PM.Model(big, 4096, 100)
    g = PGpu(torch_cuda, 2, 4096, 100, peers=big, slot=[2, 1], nslots=4)
    same(g.step(st[0], None, SETCAP), m.step(st[0], None, SETCAP))
    assert m.conn(0).used > 64
    dec64, w = cpu_decoder(O.oracle(), 1, 64, 100, False), None
    for s in (1, 2, 3):
        reset = [1, 0] if s == 1 else None
        flags = CONT | SETCAP
        w = m.step(st[s], None, flags, peers=small, reset=reset)
        r = g.step(st[s], None, flags, peers=small, reset=reset)
        same(r, w, "step %d: " % s)
        assert m.conn(0).used <= 64 and (r["rstatus"] == 0).all()
        if s == 1:
            assert r["enc"][0][:2] == E.encode_int(64, 5, 0x20) == b"\x3f\x21" and len(r["enc"][0]) > 2
            assert r["enc"][1][:1] != b"\x3f"  # the neighbour continues: no capacity instruction
        sq = PM.subset(st[s], [0])
        d = dec64(sq, [r["frames"][k] for k in sq["_responses"]], [r["enc"][0]])
        assert d["enc_status"][0] == 0 and d["enc_consumed"][0] == len(r["enc"][0]) and (d["sstatus"][:1] == 0).all()
        assert decoded_fields(d, d["sec_off"], 0) == fields_of(sq, 0)
    assert m.counts()[0] == 1 and m.counts()[1] > 20


PASS_THROUGH = [("dyn", "max_blocked_1"), ("dyn", "set_capacity"), ("evict", "exact_fit"), ("evict", "mode_mix")]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,name", PASS_THROUGH)
def test_gpu_peers_null_is_the_slots_call(torch_cuda, kind, name):
    """peers == NULL through hhuff_qpack_flatten_sessions_peers: the bytes, statuses and sessions of the entry point
    without it, on existing edge scripts"""
    sc = (edge_scripts if kind == "dyn" else evict_scripts)()[name]
    n = len(sc["steps"][0][0])
    args = (torch_cuda, n, sc.get("H", 4096), sc.get("max_blocked", 100), sc.get("max_inflight", 64))
    a, b = PGpu(*args, peers_call=True), PGpu(*args)
    if kind == "dyn":
        got = [run_script(sc, lambda k, q, dec, flags, g=g: g.step(q, dec, flags)) for g in (a, b)]
    else:
        got = [[r for _, r in script_steps(sc, g.step)] for g in (a, b)]
    for k, (x, y) in enumerate(zip(*got)):
        same(x, y, "%s step %d: " % (name, k))
        np.testing.assert_array_equal(x["out_raw"], y["out_raw"])
        np.testing.assert_array_equal(x["enc_raw"], y["enc_raw"])
    # the scratch contents: a slab's unused ring slots and string bytes are whatever the allocation held, so the
    # sessions are compared as their images
    fam = C.conn_family(C.FAM_QPACK_ENC, sc.get("H", 4096), sc.get("max_inflight", 64))
    slot = torch_cuda.arange(n, dtype=torch_cuda.int32, device="cuda")
    imgs = []
    for g in (a, b):
        img, off, ln, status = C.conn_export(fam, g.scratch, n, slot)
        torch_cuda.cuda.synchronize()
        assert (status.cpu().numpy() == 0).all()
        imgs.append((img.cpu().numpy()[:int(off[-1])].tobytes(), ln.cpu().numpy().tolist()))
    assert imgs[0] == imgs[1]


@pytest.mark.gpu
def test_gpu_exact_fit_encoder_regions(torch_cuda):
    """without HHUFF_QENC_EVICT an encoder-stream region of exactly cap_c + 4 bytes per connection is accepted, also
    for connections that fill their tables, and nothing is written outside any region.  An insert's instruction is at
    least 26 bytes shorter than what the table accounts for the entry (32 against a name reference or a name length
    and a value length of at most 3 bytes each), so a step's stream stays under cap_c + 3 as well: the model says
    so and the GPU agrees.  The region that does refuse is the one a byte short of the stream itself: the section
    whose insert no longer fits gets HHUFF_RES_SPACE, writes nothing and leaves the table as it was"""
    caps = (0, 31, 64, 220, 1024)
    peers = peers_of(*[(cap, 100) for cap in caps])
    # per connection two sections that together offer more entries than any of the tables holds
    q = batch([[resp([(b"link", b"</%02d/%02d>" % (c, j), LTR) for j in range(12)], stream_id=0),
                resp([(b"link", b"<//%02d/%02d>" % (c, j), LTR) for j in range(12)], stream_id=4)] for c in range(5)])
    streams = None
    for less in (0, 1):
        q["enc_out_off"] = np.concatenate([[0], np.cumsum([cap + 4 - less for cap in caps])]).astype(np.uint64)
        m, g = PM.Model(peers, 4096, 100), PGpu(torch_cuda, 5, 4096, 100, peers=peers)
        w, r = m.step(q, None, SETCAP), g.step(q, None, SETCAP)
        same(r, w, "cap_c + %d: " % (4 - less))
        assert (r["rstatus"] == 0).all() and r["guards_intact"]
        assert [m.conn(c).cap - m.conn(c).used < 44 for c in range(5)] == [True] * 5  # every table is full
        streams = w["enc"]
    # a byte short of the stream itself, for the connections that insert
    rooms = [len(e) - (1 if cap >= 64 else 0) for e, cap in zip(streams, caps)]
    q["enc_out_off"] = np.concatenate([[0], np.cumsum(rooms)]).astype(np.uint64)
    m, g = PM.Model(peers, 4096, 100), PGpu(torch_cuda, 5, 4096, 100, peers=peers)
    w, r = m.step(q, None, SETCAP), g.step(q, None, SETCAP)
    same(r, w, "a byte short: ")
    assert r["guards_intact"]
    for c, cap in enumerate(caps):
        st = list(r["rstatus"][2 * c:2 * c + 2])
        assert C.RES_SPACE in st if cap >= 64 else st == [0, 0]
        assert len(r["enc"][c]) <= rooms[c]
