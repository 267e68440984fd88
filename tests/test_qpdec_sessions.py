"""QPACK decoder sessions (include/hhuff.h (2e'''), hhuff_qpack_parse_requests_sessions / _parse_responses_sessions):
the parked streams of a connection and its decoder stream kept on the device.
CPU: the exports and the host-side refusals; edge scripts whose expected values are written out here and which the
plain-Python model (tests/qpdec_session_model.py) must reproduce; the model's statuses against the existing oracle
given the num_blocked a caller of hhuff_qpack_parse_requests would have kept; the model in a closed loop with the
encoder model (tests/qpenc_dyn_model.py); the list operations on the host under sanitizers (tools/qpark_host.cpp).
GPU: the calls through the C ABI against the model byte for byte -- the edge scripts, 65 and 300 connections with
withheld encoder streams and moved state, the existing call where nothing blocks, connection slots, a closed loop
with hhuff_qpack_flatten_sessions whose decoder stream never leaves the device, and guards around every buffer the
session writes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import qpdec_session_model as DM
import qpenc_dyn_model as EM
from h2o_amd import codec as C
from h2o_amd import qpack_synth as QS
from h2o_amd.hpack_synth import encode_int
from h2o_amd.qpack_synth import qstring

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 4096
ME = H // 32
DF, BLOCKED, EINVAL = DM.DF, DM.BLOCKED, DM.EINVAL
ID62 = (1 << 62) - 1


# ---------------------------------------------------------------------------------------------------
# hand-built steps
# ---------------------------------------------------------------------------------------------------
def ins(i):
    """encoder-stream instruction: insert entry i (1-based) with a literal name"""
    return qstring(b"x-k%d" % i, 5, 0x40) + qstring(b"value-%d" % i, 7)


def sec(ric, responses=False):
    """a section that needs `ric` inserts (0: none) and references the newest of them"""
    head = b"\0\0" if ric == 0 else encode_int(ric % (2 * ME) + 1, 8) + b"\0"
    if responses:
        body = encode_int(25, 6, 0xC0)  # :status 200
    else:  # :method GET, :scheme https, :path /, :authority
        body = encode_int(17, 6, 0xC0) + encode_int(23, 6, 0xC0) + encode_int(1, 6, 0xC0) + encode_int(0, 4, 0x50) + \
            qstring(b"a.example", 7)
    return head + body + (encode_int(0, 6, 0x80) if ric else b"")


def pack(conns):
    """conns = [(encoder bytes, [(stream id, section bytes), ...]), ...] -> (step dict, stream ids)"""
    secs = [s for _, ss in conns for _, s in ss]
    sid = np.array([i for _, ss in conns for i, _ in ss], np.uint64)
    sec_off = np.concatenate([[0], np.cumsum([len(s) for s in secs])]).astype(np.uint32)
    conn_first = np.concatenate([[0], np.cumsum([len(ss) for _, ss in conns])]).astype(np.uint32)
    enc_len = np.array([len(e) for e, _ in conns], np.uint32)
    enc_off = (int(sec_off[-1]) + np.concatenate([[0], np.cumsum(enc_len)[:-1]])).astype(np.uint32)
    data = np.frombuffer(b"".join(secs) + b"".join(e for e, _ in conns) + b"\0", np.uint8).copy()
    return dict(data=data, sec_off=sec_off, conn_first=conn_first, enc_off=enc_off, enc_len=enc_len), sid


def step(enc=b"", secs=(), cancels=(), expect=None, **kw):
    """one step of a one-connection script: secs = [(stream id, ric)], cancels = [(stream id, flags)]"""
    return dict(enc=enc, secs=list(secs), cancels=list(cancels), kw=kw, expect=expect or {})


def edge_scripts(enc_int=None):
    """name -> dict(max_blocked=, steps=[...]); every step's expected outputs are written out.  enc_int(v, bits,
    first): the prefix integers of the ids script (the model's own when None)"""
    ei = enc_int or (lambda v, bits, first: DM.prefix_int(first, v, bits))
    ids = [62, 63, 64, 126, 127, 128, ID62]
    S = DM.SILENT
    return {
        "three_blocked_then_wake": dict(max_blocked=2, steps=[
            step(secs=[(4, 1), (8, 1), (12, 1)], expect=dict(sstatus=[BLOCKED, BLOCKED, DF], parked=2, dec=b"", wake=[])),
            step(secs=[(4, 1)], expect=dict(sstatus=[BLOCKED], parked=2, dec=b"", wake=[])),  # a resubmission: one slot
            step(secs=[(16, 1)], expect=dict(sstatus=[DF], parked=2)),  # and the list is still full
            step(enc=ins(1), expect=dict(parked=0, wake=[4, 8], dec=b"", dflags=0, enc_status=0, insert_count=1)),
            step(secs=[(4, 1), (8, 1)], expect=dict(sstatus=[0, 0], parked=0, dec=b"\x84\x88", wake=[]))]),
        "speculative_resubmission": dict(max_blocked=2, steps=[
            step(secs=[(4, 1), (8, 2)], expect=dict(sstatus=[BLOCKED, BLOCKED], parked=2)),
            # with the insert: stream 4 decodes and leaves, stream 8 still waits and keeps its slot; nothing to wake
            step(enc=ins(1), secs=[(4, 1), (8, 2)], expect=dict(sstatus=[0, BLOCKED], parked=1, dec=b"\x84", wake=[])),
            step(enc=ins(2), expect=dict(parked=0, wake=[8]))]),
        "cancel": dict(max_blocked=2, steps=[
            step(secs=[(4, 1)], expect=dict(sstatus=[BLOCKED], parked=1)),
            step(cancels=[(4, 0)], expect=dict(parked=0, dec=b"\x44")),          # parked: slot freed, 0x40 | id
            step(cancels=[(16, 0)], expect=dict(parked=0, dec=b"\x50")),         # not parked: sent all the same
            step(secs=[(8, 1), (12, 1)], expect=dict(sstatus=[BLOCKED, BLOCKED], parked=2)),
            step(cancels=[(8, S)], expect=dict(parked=1, dec=b"")),              # silent: slot freed, nothing sent
            step(secs=[(20, 1)], cancels=[(12, 0), (20, S), (99, S)], expect=dict(sstatus=[BLOCKED], parked=0, dec=b"\x4c"))]),
        "prefix_integer_edges": dict(max_blocked=2, steps=[
            step(enc=ins(1), secs=[(i, 1) for i in ids], cancels=[(i, 0) for i in ids],
                 expect=dict(sstatus=[0] * len(ids), parked=0,
                             dec=b"".join(ei(i, 7, 0x80) for i in ids) + b"".join(ei(i, 6, 0x40) for i in ids)))]),
        "wake_region_of_one": dict(max_blocked=2, steps=[
            step(secs=[(4, 1), (8, 1)], expect=dict(sstatus=[BLOCKED, BLOCKED], parked=2)),
            step(enc=ins(1), wake_room=[1], expect=dict(wake=[4], parked=1, dflags=DM.WAKE_PENDING)),
            step(wake_room=[1], expect=dict(wake=[8], parked=0, dflags=0))]),
        "max_blocked_0": dict(max_blocked=0, steps=[
            step(secs=[(4, 1)], expect=dict(sstatus=[DF], parked=0, wake=[], dec=b"")),
            step(secs=[(8, 1), (12, 0)], expect=dict(sstatus=[DF, 0], parked=0)),
            step(enc=ins(1), secs=[(16, 1)], expect=dict(sstatus=[0], parked=0, wake=[], dec=b"\x90"))]),
        "sync": dict(max_blocked=2, steps=[
            step(enc=ins(1) + ins(2), sync=True, expect=dict(dec=b"\x02")),                    # n = the inserts
            step(enc=ins(3) + ins(4), secs=[(4, 3)], sync=True, expect=dict(sstatus=[0], dec=b"\x84\x01")),  # n = 4 - 3
            step(sync=True, expect=dict(dec=b"")),                                               # total == known
            step(enc=ins(5), expect=dict(dec=b"")),                                              # no SYNC: nothing
            step(sync=True, expect=dict(dec=b"\x01"))]),
        "refused_region_one_byte_short": dict(max_blocked=2, steps=[
            step(enc=ins(1), secs=[(4, 2)], expect=dict(sstatus=[BLOCKED], parked=1, insert_count=1)),
            step(enc=ins(2), secs=[(8, 2)], cancels=[(4, 0)], dec_room=[10 * 2 + 10 - 1],
                 expect=dict(sstatus=[EINVAL], enc_status=EINVAL, enc_consumed=0, insert_count=0, parked=0, dec=b"", wake=[],
                             dflags=0)),
            # as if the refused step had not happened: the insert arrives now, stream 4 is still parked and wakes
            step(enc=ins(2), secs=[(8, 2)], expect=dict(sstatus=[0], enc_status=0, enc_consumed=len(ins(2)), insert_count=2,
                                                        parked=0, dec=b"\x88", wake=[4]))]),
    }


def run_script(sc, call, responses=False):
    """call(st, stream_id, cancels=, **kw) -> a result in the model's shape, step after step; -> the results"""
    out = []
    for k, s in enumerate(sc["steps"]):
        st, sid = pack([(s["enc"], [(i, sec(r, responses)) for i, r in s["secs"]])])
        out.append(call(st, sid, cont=k > 0, cancels=[s["cancels"]], **s["kw"]))
    return out


def check_expect(sc, results, what=""):
    for k, (s, r) in enumerate(zip(sc["steps"], results)):
        for key, want in s["expect"].items():
            got = r[key]
            if key in ("dec", "wake"):
                got = got[0] if key == "dec" else [int(x) for x in got[0]]
            elif key == "sstatus":
                got = [int(x) for x in got]
            else:
                got = int(got[0])
            assert got == want, "%s step %d %s: got %r want %r" % (what, k, key, got, want)


def model_call(codec, sc, responses=False):
    m = DM.Model(codec, 1, H, sc["max_blocked"], responses)
    return lambda st, sid, **kw: m.step(st, sid, **kw)


# ---------------------------------------------------------------------------------------------------
# CPU 1: exports and host-only checks (fails before the sessions exist)
# ---------------------------------------------------------------------------------------------------
def test_exports_and_host_only_checks():
    import ctypes

    from h2o_amd import build

    build.build(verbose=False)
    L = C.lib()
    for name in ("hhuff_qpack_parse_requests_sessions", "hhuff_qpack_parse_responses_sessions",
                 "hhuff_qpack_dsession_state_size", "hhuff_qpack_dsession_out_bound"):
        assert hasattr(L, name) and name in C.EXPORTED, name
    size = L.hhuff_qpack_dsession_state_size
    for m in (0, 1, 100, 4095):
        assert size(0, m) == 0
        assert size(3, m) == 3 * size(1, m) and size(1, m) % 16 == 0 and size(1, m) >= 16 * m
        assert size(1, m + 1) - size(1, m) == 16
    assert C.qpack_dsession_state_size(2, 100) == size(2, 100)
    assert L.hhuff_qpack_dsession_out_bound(3, 2) == 60 == C.qpack_dsession_out_bound(3, 2)
    assert L.hhuff_qpack_dsession_out_bound(0, 0) == 10
    p = 1 << 20  # a 16-byte aligned dummy address: never dereferenced on these paths
    ss = int(L.hhuff_qpack_scratch_size(1, H))
    for call in (L.hhuff_qpack_parse_requests_sessions, L.hhuff_qpack_parse_responses_sessions):
        def run(ds, nconn, max_blocked, call=call):
            return call(ds, None, p, 16, p, p, p, p, nconn, 0, H, max_blocked, *([p] * 15), p, ss, 0, None)
        full = C._QpackDsessionsStruct(p, 1 << 20, None, None, None, p, p, p, p, p, p, p, p, 0)
        ok = ctypes.byref(full)
        assert run(ok, 1, 4097) == -1 and b"4096" in L.hhuff_last_error_string()
        assert run(ok, 0, 100) == 0 and run(None, 0, 100) == 0  # nothing to do, nothing enqueued
        assert run(None, 1, 100) == -1
        for field in ("state", "dec_out", "dec_out_off", "dec_out_len", "wake_id", "wake_first", "nwake", "parked", "dflags"):
            bad = C._QpackDsessionsStruct(p, 1 << 20, None, None, None, p, p, p, p, p, p, p, p, 0)
            setattr(bad, field, None)
            assert run(ctypes.byref(bad), 1, 100) == -1, field
            assert b"NULL" in L.hhuff_last_error_string()
        small = C._QpackDsessionsStruct(p, size(1, 100) - 1, None, None, None, p, p, p, p, p, p, p, p, 0)
        assert run(ctypes.byref(small), 1, 100) == -1 and b"state" in L.hhuff_last_error_string()
        flag = C._QpackDsessionsStruct(p, 1 << 20, None, None, None, p, p, p, p, p, p, p, p, 2)
        assert run(ctypes.byref(flag), 1, 100) == -1
        nocid = C._QpackDsessionsStruct(p, 1 << 20, p, None, None, p, p, p, p, p, p, p, p, 0)
        assert run(ctypes.byref(nocid), 1, 100) == -1


# ---------------------------------------------------------------------------------------------------
# CPU 2: the edge scripts on the model
# ---------------------------------------------------------------------------------------------------
def codecs(oracle_codec):
    from oracle import oracle as O

    return [("restatement", oracle_codec)] + ([("reference", O.ref())] if O.ref_available() else [])


@pytest.mark.parametrize("responses", [False, True])
@pytest.mark.parametrize("name", sorted(edge_scripts()))
def test_edge_scripts_on_the_model(oracle_codec, name, responses):
    for what, codec in codecs(oracle_codec):
        sc = edge_scripts(lambda v, bits, first: codec.encode_int(v, bits, first))[name]
        check_expect(sc, run_script(sc, model_call(codec, sc, responses), responses), "%s %s" % (what, name))


def test_prefix_integers_are_the_oracles(oracle_codec):
    for what, codec in codecs(oracle_codec):
        for v in (0, 1, 62, 63, 64, 126, 127, 128, 16383, 16384, ID62):
            assert DM.prefix_int(0x40, v, 6) == codec.encode_int(v, 6, 0x40), (what, v)
            assert DM.prefix_int(0x00, v, 6) == codec.encode_int(v, 6, 0x00), (what, v)
            assert DM.prefix_int(0x80, v, 7) == codec.encode_int(v, 7, 0x80), (what, v)
            assert len(DM.prefix_int(0x40, v, 6)) <= 10  # hhuff_qpack_dsession_out_bound's 10 bytes an instruction


# ---------------------------------------------------------------------------------------------------
# sessions with withheld encoder streams
# ---------------------------------------------------------------------------------------------------
def withheld_sessions(nconn, seed, responses, model, replay=None):
    """3 steps of a synthetic session; the encoder stream of step 1 reaches odd connections only with step 2's.  The
    sections step 1 parked are resubmitted in step 2 ahead of the connection's new ones when c % 4 == 1 (with the
    inserts: speculative), and in a step 3 after they were woken when c % 4 == 3.  Every step runs on `model` (its
    results say what was parked and woken) and then, with the same inputs, on replay(k, st, sid, kw, want).
    -> per step (st, sid, kw, want)"""
    raw = QS.make_session(nconn, steps=3, seed=seed, header_table_size=H, adversarial_frac=0.05, blocked_frac=0.0,
                          responses=responses)
    per = []  # per step, per connection: (encoder bytes, [section bytes])
    for st in raw:
        d, so, cf = st["data"].tobytes(), st["sec_off"], st["conn_first"]
        per.append([(d[int(st["enc_off"][c]):int(st["enc_off"][c]) + int(st["enc_len"][c])],
                     [d[int(so[k]):int(so[k + 1])] for k in range(int(cf[c]), int(cf[c + 1]))]) for c in range(nconn)])
    nid = [0] * nconn
    body = [dict() for _ in range(nconn)]  # stream id -> its section
    parked = [[] for _ in range(nconn)]    # the streams the model holds parked, oldest first
    woken = [[] for _ in range(nconn)]     # the streams the last step woke: submitted again in this one
    log = []
    for k in range(4):
        conns = []
        for c in range(nconn):
            enc, secs = per[k][c] if k < 3 else (b"", [])
            if c & 1 and k == 1:
                enc = b""
            if c & 1 and k == 2:
                enc = per[1][c][0] + enc
            new = [(4 * (nid[c] + j), s) for j, s in enumerate(secs)]
            nid[c] += len(secs)
            body[c].update(new)
            again = woken[c] + (parked[c] if (k == 2 and c % 4 == 1) or k == 3 else [])
            conns.append((enc, [(i, body[c][i]) for i in again] + new))
        st, sid = pack(conns)
        cancels = [[(4 * 1000 + c, 0)] if c % 7 == 0 else [(i, c % 2) for i in parked[c][:1]] if c % 5 == 0 and k == 2 else []
                   for c in range(nconn)]
        kw = dict(cont=k > 0, cancels=cancels, sync=k == 2)
        want = model.step(st, sid, **kw)
        if replay:
            replay(k, st, sid, kw, want)
        for c in range(nconn):
            parked[c] = [int(e[0]) for e in model.sess[c].parked]
            woken[c] = [int(x) for x in want["wake"][c]]
        log.append((st, sid, kw, want))
    return log


# ---------------------------------------------------------------------------------------------------
# CPU 3: the model against the existing oracle
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("responses", [False, True])
def test_model_statuses_are_the_oracles_with_the_callers_count(oracle_codec, responses):
    """a caller of hhuff_qpack_parse_requests keeps num_blocked itself: given the model's parked count at the
    step's start, less the parked streams the step resubmits, the existing oracle gives the model's statuses; and
    the model's acknowledgment bytes are the oracle's ack fields joined in section order"""
    from oracle import oracle as O

    for what, codec in codecs(oracle_codec):
        nconn, mb = 40, 2
        model = DM.Model(codec, nconn, H, mb, responses)
        sess = O.QpackSession(codec, nconn, H, mb)
        before = [dict() for _ in range(nconn)]
        seen = dict(df=0, blocked=0, ack=0)

        def replay(k, st, sid, kw, want):
            cf = st["conn_first"]
            nb = np.zeros(nconn, np.uint32)
            for c in range(nconn):
                mine = set(int(x) for x in sid[int(cf[c]):int(cf[c + 1])])
                nb[c] = len([i for i in before[c] if i not in mine])
            d = sess.step(st["data"], st["enc_off"], st["enc_len"], st["sec_off"], cf, O.default_arena_off(st["sec_off"], H),
                          num_blocked=nb, stream_id=sid, responses=responses)
            n = int(cf[-1])
            np.testing.assert_array_equal(d["sstatus"][:n], want["sstatus"], err_msg="%s step %d" % (what, k))
            rec = d["res" if responses else "req"]
            for c in range(nconn):
                acks = b"".join(bytes(rec["ack"][j][:int(rec["ack_len"][j])]) for j in range(int(cf[c]), int(cf[c + 1])))
                tail = b"".join(DM.prefix_int(0x40, i, 6) for i, f in kw["cancels"][c] if not f & DM.SILENT)
                if int(want["enc_status"][c]) == 0:
                    assert want["dec"][c][:len(acks)] == acks and want["dec"][c][len(acks):len(acks) + len(tail)] == tail
                seen["ack"] += len(acks) > 0
            seen["df"] += int((want["sstatus"] == DF).sum())
            seen["blocked"] += int((want["sstatus"] == BLOCKED).sum())
            for c in range(nconn):
                before[c] = {int(e[0]) for e in model.sess[c].parked}
        withheld_sessions(nconn, 7 + responses, responses, model, replay)
        assert seen["blocked"] > 5 and seen["ack"] > 5, seen


# ---------------------------------------------------------------------------------------------------
# CPU 4: the model in a closed loop with the encoder model
# ---------------------------------------------------------------------------------------------------
def loop_step(q, frames, encs, again):
    """the decoder's step for the encoder's step q: again = per connection the parked (stream id, section) ahead"""
    import test_qpenc_dyn as QD

    cf = q["conn_first"]
    return pack([(encs[c], again[c] + [(int(q["stream_id"][k]), QD.section_of(frames[k]))
                                       for k in range(int(cf[c]), int(cf[c + 1]))]) for c in range(cf.size - 1)])


def closed_loop(nconn, requests, encode, decode, finish):
    """3 encoder steps; the encoder streams of step 1 reach the decoder with step 2's, and the sections that parked
    are resubmitted then, ahead of the new ones.  encode(s, q, dec) -> frames, enc (bytes), rstatus, dec_status,
    dec_consumed; dec = whatever decode(s, st, sid) returned last (its decoder streams).  finish(dec): the last
    decoder streams."""
    import test_qpenc_dyn as QD

    steps = QD.loop_sessions(nconn, 3, requests)
    dec, held, again = None, None, [[] for _ in range(nconn)]
    for s, q in enumerate(steps):
        r = encode(s, q, dec)
        n = q["res"].size
        assert (np.asarray(r["rstatus"])[:n] == 0).all() and (np.asarray(r["dec_status"])[:nconn] == 0).all()
        encs = list(r["enc"])
        if s == 1:
            held, encs = encs, [b""] * nconn
        elif s == 2:
            encs = [held[c] + encs[c] for c in range(nconn)]
        st, sid = loop_step(q, r["frames"], encs, again)
        dec, d = decode(s, st, sid)
        cf = st["conn_first"]
        again = [[] for _ in range(nconn)]
        for c in range(nconn):
            rows = [(int(sid[k]), st["data"][int(st["sec_off"][k]):int(st["sec_off"][k + 1])].tobytes())
                    for k in range(int(cf[c]), int(cf[c + 1]))]
            stt = d["sstatus"][int(cf[c]):int(cf[c + 1])]
            assert all(x in (0, BLOCKED) for x in stt), (s, c, stt)
            again[c] = [rows[j] for j in range(len(rows)) if stt[j] == BLOCKED]
            if s != 1:
                assert not again[c], (s, c)
        if s == 1:
            assert sum(len(a) for a in again) >= nconn  # the withheld inserts parked a stream a connection
        assert (d["enc_status"] == 0).all()
        np.testing.assert_array_equal(d["enc_consumed"], st["enc_len"])
    finish(dec)


@pytest.mark.parametrize("requests", [False, True])
def test_model_closed_loop_with_the_encoder_model(oracle_codec, requests):
    nconn = 20
    enc = EM.Model(nconn, H, 100)
    dec = DM.Model(oracle_codec, nconn, H, 100, responses=not requests)

    def encode(s, q, streams):
        r = enc.step(q, streams, flags=C.QENC_CONTINUE if s else C.QENC_SET_CAPACITY)
        if streams is not None:  # every decoder stream is consumed whole
            np.testing.assert_array_equal(r["dec_consumed"], [len(x) for x in streams])
        return r

    def decode(s, st, sid):
        d = dec.step(st, sid, cont=s > 0)
        return d["dec"], d

    def finish(streams):
        for c, conn in enumerate(enc.conns):
            assert conn.handle_input(streams[c]) == (0, len(streams[c]))
            assert conn.num_blocked == 0 and not conn.inflight, c  # everything is acknowledged
    closed_loop(nconn, requests, encode, decode, finish)


# ---------------------------------------------------------------------------------------------------
# CPU 5: the list operations on the host under sanitizers
# ---------------------------------------------------------------------------------------------------
def test_qpark_host_clean_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "qpark_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "h2o_amd", "csrc"),
                    os.path.join(ROOT, "tools", "qpark_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, "2000"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok:"), r.stdout


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


GUARD = 256


class Gpu:
    """the session calls step after step, table scratch and session state carried; dec_out, wake_id and state are
    the inner parts of guarded buffers of exactly the stated sizes (tests/bounds_harness.py's guards)"""

    def __init__(self, torch, nslots, max_blocked, responses=False, move=False):
        self.t, self.nslots, self.mb, self.responses, self.move = torch, nslots, max_blocked, responses, move
        self.scratch = self.state_whole = None

    def _state(self):
        from bounds_harness import guarded

        size = C.qpack_dsession_state_size(self.nslots, self.mb)
        if self.state_whole is None:
            self.state_whole, _ = guarded(self.t, size, 0xA5, GUARD)
        elif self.move:  # a new allocation: offsets, not addresses; the old one stays, overwritten
            moved = self.state_whole.clone()
            self.state_whole.fill_(0x5A)
            self.old, self.state_whole = self.state_whole, moved
            ms = self.scratch.clone()
            self.scratch.fill_(0x5A)
            self.old_scratch, self.scratch = self.scratch, ms
        return self.state_whole[GUARD:GUARD + size]

    def state_bytes(self):
        size = C.qpack_dsession_state_size(self.nslots, self.mb)
        return self.state_whole[GUARD:GUARD + size].cpu().numpy().reshape(self.nslots, -1)

    def step(self, st, sid, slot=None, cflags=None, cont=True, cancels=None, dec_room=None, wake_room=None, sync=False,
             cancel_first=None, plain=False):
        from bounds_harness import guarded
        from oracle import oracle as O

        torch = self.t
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()  # noqa: E731
        u32 = lambda a: dev(np.asarray(a, np.uint32).view(np.int32))  # noqa: E731
        cf = np.asarray(st["conn_first"], np.int64)
        nconn, nsec = cf.size - 1, int(cf[-1])
        cancels = [[]] * nconn if cancels is None else cancels
        ncan = np.array([len(x) for x in cancels], np.int64)
        if cancel_first is None:
            cancel_first = np.concatenate([[0], np.cumsum(ncan)])
        cid = np.array([i for x in cancels for i, _ in x] + [0], np.uint64)
        cfl = np.array([f for x in cancels for _, f in x] + [0], np.uint8)
        room = DM.out_bound(np.diff(cf), ncan) if dec_room is None else np.asarray(dec_room, np.int64)
        doff = np.concatenate([[0], np.cumsum(room)]).astype(np.uint64)
        wroom = np.full(nconn, self.mb, np.int64) if wake_room is None else np.asarray(wake_room, np.int64)
        wfirst = np.concatenate([[0], np.cumsum(wroom)]).astype(np.uint32)
        dec_whole, dec_out = guarded(torch, int(doff[-1]), 0xA5, GUARD)
        wake_whole, wake_b = guarded(torch, 8 * int(wfirst[-1]), 0xA5, GUARD)
        ds = None if plain else C.QpackDsessions(
            state=self._state(), cancel_first=u32(cancel_first), cancel_id=dev(cid.view(np.int64)), cancel_flags=dev(cfl),
            dec_out_off=dev(doff.view(np.int64)), dec_out=dec_out, wake_first=u32(wfirst), wake_id=wake_b.view(torch.int64),
            sync=sync)
        slots = None if slot is None else C.ConnSlots(u32(slot), None if cflags is None else dev(np.asarray(cflags, np.uint8)),
                                                      self.nslots)
        arena_off = O.default_arena_off(st["sec_off"], H)
        r = C.qpack_decode(dev(st["data"]), u32(st["enc_off"]), u32(st["enc_len"]), u32(st["sec_off"]), u32(cf), nsec, H,
                           self.mb, arena_off=dev(arena_off.view(np.int64)), in_size=int(st["data"].size) - 1,
                           scratch=self.scratch, cont=cont, arena=torch.zeros(max(1, int(arena_off[-1])), dtype=torch.uint8,
                                                                              device="cuda"),
                           stream_id=dev(np.asarray(sid if nsec else [0], np.uint64).view(np.int64)),
                           responses=self.responses, slots=slots, sessions=ds)
        torch.cuda.synchronize()
        self.scratch = r["scratch"]
        h = {k: r[k].cpu().numpy() for k in ("sstatus", "req_insert_count", "enc_status", "enc_consumed", "insert_count",
                                              "nfields", "name_off", "name_len", "value_off", "value_len", "fflags", "arena")}
        g = dict(sstatus=h["sstatus"][:nsec], req_insert_count=h["req_insert_count"].view(np.uint64)[:nsec],
                 enc_status=h["enc_status"][:nconn], enc_consumed=h["enc_consumed"].view(np.uint32)[:nconn],
                 insert_count=h["insert_count"].view(np.uint64)[:nconn], raw=h)
        rec = r["res" if self.responses else "req"].cpu().numpy().reshape(-1)
        g["rec"] = rec.view(O.QRES_DTYPE if self.responses else O.QREQ_DTYPE)[:nsec]
        if plain:
            return g
        dw, ww = dec_whole.cpu().numpy(), wake_whole.cpu().numpy()
        sw = self.state_whole.cpu().numpy()
        g["guards_intact"] = bool((dw[:GUARD] == 0xA5).all() and (dw[dw.size - GUARD:] == 0xA5).all() and
                                  (ww[:GUARD] == 0xA5).all() and (ww[ww.size - GUARD:] == 0xA5).all() and
                                  (sw[:GUARD] == 0xA5).all() and (sw[sw.size - GUARD:] == 0xA5).all())
        for k in ("dec_out_len", "nwake", "parked"):
            g[k] = r[k].cpu().numpy().view(np.uint32)[:nconn]
        g["dflags"] = r["dflags"].cpu().numpy()[:nconn]
        inner, wid = dw[GUARD:dw.size - GUARD], ww[GUARD:ww.size - GUARD].view(np.uint64)
        g["dec"] = [inner[int(doff[c]):int(doff[c]) + int(g["dec_out_len"][c])].tobytes() for c in range(nconn)]
        g["wake"] = [[int(x) for x in wid[int(wfirst[c]):int(wfirst[c]) + int(g["nwake"][c])]] for c in range(nconn)]
        # the bytes of a region behind the step's own are not written
        g["regions_clean"] = all((inner[int(doff[c]) + int(g["dec_out_len"][c]):int(doff[c + 1])] == 0xA5).all()
                                 for c in range(nconn))
        g["t"] = r  # the device tensors (the closed loop passes dec_out on without a host copy)
        return g


def same(g, w, what=""):
    """the GPU's step g against the model's w: every output"""
    for k in ("sstatus", "req_insert_count", "enc_status", "enc_consumed", "insert_count", "dec_out_len", "nwake", "parked",
              "dflags"):
        np.testing.assert_array_equal(np.asarray(g[k]).astype(np.int64), np.asarray(w[k]).astype(np.int64), err_msg=what + k)
    assert g["rec"].tobytes() == w["rec"].tobytes(), what + "records"
    bad = [c for c in range(len(w["dec"])) if g["dec"][c] != w["dec"][c]]
    assert not bad, "%s%d decoder streams differ; first %d: got %s want %s" % (what, len(bad), bad[0], g["dec"][bad[0]].hex(),
                                                                               w["dec"][bad[0]].hex())
    assert g["wake"] == [[int(x) for x in v] for v in w["wake"]], what + "wake_id"
    assert g["guards_intact"] and g["regions_clean"], what + "guards"


@pytest.mark.gpu
@pytest.mark.parametrize("responses", [False, True])
@pytest.mark.parametrize("name", sorted(edge_scripts()))
def test_gpu_edge_scripts(torch_cuda, oracle_codec, name, responses):
    sc = edge_scripts()[name]
    want = run_script(sc, model_call(oracle_codec, sc, responses), responses)
    g = Gpu(torch_cuda, 1, sc["max_blocked"], responses)
    got = run_script(sc, g.step, responses)
    check_expect(sc, got, name)
    for k, (a, b) in enumerate(zip(got, want)):
        same(a, b, "%s step %d: " % (name, k))


@pytest.mark.gpu
@pytest.mark.parametrize("nconn,responses", [(65, False), (65, True), (300, False), (300, True)])
def test_gpu_withheld_encoder_streams(torch_cuda, oracle_codec, nconn, responses):
    """one past a wave and one past a 256-lane block; about half the sections park and wake; the state and the
    table scratch move to fresh allocations between the steps (guards, too: exact sizes)"""
    g = Gpu(torch_cuda, nconn, 2, responses, move=True)
    seen = dict(parked=0, woken=0, df=0, pending=0)

    def replay(k, st, sid, kw, want):
        same(g.step(st, sid, **kw), want, "step %d: " % k)
        seen["parked"] += int(want["parked"].sum())
        seen["woken"] += int(want["nwake"].sum())
        seen["df"] += int((want["sstatus"] == DF).sum())
    withheld_sessions(nconn, 11 + responses, responses, DM.Model(oracle_codec, nconn, H, 2, responses), replay)
    assert seen["parked"] > nconn // 4 and seen["woken"] > nconn // 8 and seen["df"] > 0, seen


@pytest.mark.gpu
@pytest.mark.parametrize("responses", [False, True])
def test_gpu_equals_the_existing_call_when_nothing_parks(torch_cuda, responses):
    """no cancellations and every encoder stream in time: every array the session call shares with
    hhuff_qpack_parse_requests / _parse_responses is identical, and dec_out is the ack fields joined"""
    raw = QS.make_session(65, steps=2, seed=21 + responses, header_table_size=H, adversarial_frac=0.05, blocked_frac=0.0,
                          responses=responses)
    a, b = Gpu(torch_cuda, 65, 100, responses), Gpu(torch_cuda, 65, 100, responses)
    for x in (a, b):  # zeroed, so the bytes no table uses compare too
        x.scratch = torch_cuda.zeros(int(C.lib().hhuff_qpack_scratch_size(65, H)), dtype=torch_cuda.uint8, device="cuda")
    for k, st in enumerate(raw):
        st = dict(st, data=np.concatenate([st["data"], np.zeros(1, np.uint8)]))
        n = int(st["conn_first"][-1])
        sid = 4 * np.arange(n, dtype=np.uint64) + 8 * n * k
        x, y = a.step(st, sid, cont=k > 0), b.step(st, sid, cont=k > 0, plain=True)
        for key in ("sstatus", "req_insert_count", "enc_status", "enc_consumed", "insert_count"):
            np.testing.assert_array_equal(x[key], y[key], err_msg=key)
        assert x["rec"].tobytes() == y["rec"].tobytes()
        for key in ("nfields", "arena"):
            np.testing.assert_array_equal(x["raw"][key][:n] if key == "nfields" else x["raw"][key],
                                          y["raw"][key][:n] if key == "nfields" else y["raw"][key], err_msg=key)
        for j in range(n):
            s0, nf = int(st["sec_off"][j]), int(x["raw"]["nfields"].view(np.uint32)[j])
            for key in ("name_off", "name_len", "value_off", "value_len", "fflags"):
                np.testing.assert_array_equal(x["raw"][key][s0:s0 + nf], y["raw"][key][s0:s0 + nf], err_msg=key)
        assert torch_cuda.equal(a.scratch, b.scratch)
        cf = st["conn_first"]
        for c in range(65):
            acks = b"".join(bytes(y["rec"]["ack"][j][:int(y["rec"]["ack_len"][j])]) for j in range(int(cf[c]), int(cf[c + 1])))
            assert x["dec"][c] == acks, c
        assert x["guards_intact"] and not x["nwake"].any()


@pytest.mark.gpu
def test_gpu_slots(torch_cuda, oracle_codec):
    """a sparse step lists 3 of 8 slots in shuffled order, one with HHUFF_CONN_RESET: the reset connection has an
    empty list and a Known Received Count of 0, the slots the step does not list keep their bytes; a connection
    naming an owned slot is refused and the slab unchanged"""
    m, g = DM.Model(oracle_codec, 8, H, 2), Gpu(torch_cuda, 8, 2)
    # step 0, all 8: an insert, an acknowledged section (Known Received Count 1) and a stream parked at 2
    st, sid = pack([(ins(1), [(4, sec(1)), (8, sec(2))])] * 8)
    kw = dict(slot=np.arange(8), cont=False)
    same(g.step(st, sid, **kw), m.step(st, sid, **kw), "dense: ")
    before = g.state_bytes().copy()
    assert (before[:, :4].view(np.uint32) == 1).all() and (before[:, 8:16].view(np.uint64) == 1).all()
    # step 1, slots 5, 1, 6: slot 1 reset (its section needs inserts the new table lacks: it parks at 2 again), slot 5
    # gets the second insert and wakes stream 8, slot 6 gets nothing
    st, sid = pack([(ins(2), []), (ins(1), [(12, sec(2))]), (b"", [])])
    kw = dict(slot=np.array([5, 1, 6]), cflags=np.array([0, 1, 0], np.uint8), cont=True)
    got, want = g.step(st, sid, **kw), m.step(st, sid, **kw)
    same(got, want, "sparse: ")
    assert got["wake"] == [[8], [], []] and list(got["parked"]) == [0, 1, 1]
    after = g.state_bytes()
    for s in (0, 2, 3, 4, 6, 7):
        assert after[s].tobytes() == before[s].tobytes(), s
    assert after[1, :4].view(np.uint32)[0] == 1 and after[1, 8:16].view(np.uint64)[0] == 0  # fresh: stream 12 at 2
    assert after[1, 16:32].view(np.uint64).tolist() == [12, 2]
    # step 2: a reset alone leaves an empty session
    st, sid = pack([(b"", [])])
    kw = dict(slot=np.array([1]), cflags=np.array([1], np.uint8), cont=True)
    same(g.step(st, sid, **kw), m.step(st, sid, **kw), "reset: ")
    assert not g.state_bytes()[1, :16].any()
    # step 3: two connections name slot 3; the second is refused, and the first does nothing: the slab stays
    before = g.state_bytes().copy()
    st, sid = pack([(b"", []), (ins(2), [(16, sec(0))])])
    kw = dict(slot=np.array([3, 3]), cont=True, cancels=[[], [(8, 0)]])
    got, want = g.step(st, sid, **kw), m.step(st, sid, **kw)
    same(got, want, "owned: ")
    assert int(got["enc_status"][1]) == EINVAL and list(got["sstatus"]) == [EINVAL] and got["dec"][1] == b""
    assert g.state_bytes().tobytes() == before.tobytes()
    # and a cancel_first that decreases over a connection refuses that connection alone
    st, sid = pack([(b"", []), (b"", [])])
    kw = dict(slot=np.array([0, 2]), cont=True, cancels=[[(8, 0)], []], cancel_first=np.array([1, 0, 1]), dec_room=[20, 20])
    got, want = g.step(st, sid, **kw), m.step(st, sid, **dict(kw, cancels=[[], [(8, 0)]]))
    same(got, want, "cancel_first: ")
    assert int(got["enc_status"][0]) == EINVAL and int(got["enc_status"][1]) == 0 and got["dec"][1] == b"\x48"


def encoder_step(torch, q, scratch, dec, flags):
    """hhuff_qpack_flatten_sessions on step q; dec = (dec_out, dec_out_off, dec_out_len) device tensors of the decoder's
    last step or None: the bytes are appended to `data` on the device and the regions passed as dec_off / dec_len"""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()  # noqa: E731
    u32 = lambda a: dev(np.asarray(a, np.uint32).view(np.int32))  # noqa: E731
    n, nconn = q["res"].size, q["conn_first"].size - 1
    data = dev(q["data"])
    dec_off = dec_len = None
    if dec is not None:
        dec_out, off, ln = dec
        dec_off = (off[:nconn] + data.numel()).to(torch.int32)
        dec_len = ln[:nconn].clone()
        data = torch.cat([data, dec_out])
    in_size = data.numel()
    data = torch.cat([data, torch.zeros(4, dtype=torch.uint8, device="cuda")])
    r = C.qpack_flatten_sessions(data, dev(q["hdr"].view(np.uint8)), dev(q["res"].view(np.uint8)), u32(q["conn_first"]), n,
                                 dev(q["stream_id"].view(np.int64)), dev(np.asarray(q["out_off"], np.uint64).view(np.int64)),
                                 dec_off, dec_len, H, 100, 64, q["server_off"], q["server_len"], in_size=in_size,
                                 scratch=scratch, cont=bool(flags & C.QENC_CONTINUE),
                                 set_capacity=bool(flags & C.QENC_SET_CAPACITY))
    torch.cuda.synchronize()
    h = {k: r[k].cpu().numpy() for k in ("out_len", "header_len", "rstatus", "rflags", "enc_out_len", "dec_status",
                                          "dec_consumed")}
    for k in ("out_len", "header_len", "enc_out_len", "dec_consumed"):
        h[k] = h[k].view(np.uint32)
    h = {k: v[:(nconn if k in ("enc_out_len", "dec_status", "dec_consumed") else n)] for k, v in h.items()}
    o, e, eoff = r["out"].cpu().numpy(), r["enc_out"].cpu().numpy(), r["enc_out_off"].cpu().numpy()
    h["frames"] = [o[int(a):int(a) + int(L)].tobytes() for a, L in zip(q["out_off"], h["out_len"])]
    h["enc"] = [e[int(a):int(a) + int(L)].tobytes() for a, L in zip(eoff, h["enc_out_len"])]
    h["guards_intact"] = True
    return h, r["scratch"]


@pytest.mark.gpu
@pytest.mark.parametrize("requests", [False, True])
def test_gpu_closed_loop_on_the_device(torch_cuda, oracle_codec, requests):
    """hhuff_qpack_flatten_sessions -> the session decoder -> dec_out, device to device, into the encoder's next
    step: consumed whole, every field back, the encoder still the encoder model's bytes"""
    import test_qpenc_dyn as QD

    nconn = 200
    enc_m = EM.Model(nconn, H, 100)
    dec_m = DM.Model(oracle_codec, nconn, H, 100, responses=not requests)
    g = Gpu(torch_cuda, nconn, 100, responses=not requests)
    state = dict(scratch=None, fields=0, due={})

    def encode(s, q, dec):
        flags = C.QENC_CONTINUE if s else C.QENC_SET_CAPACITY
        r, state["scratch"] = encoder_step(torch_cuda, q, state["scratch"], dec and dec["t"], flags)
        w = enc_m.step(q, dec and dec["host"], flags=flags)
        QD.same(r, w, "encoder step %d: " % s)
        if dec:
            np.testing.assert_array_equal(r["dec_consumed"], dec["len"])
        for c in range(nconn):  # what every section has to come back as, sooner or later
            for k in range(int(q["conn_first"][c]), int(q["conn_first"][c + 1])):
                state["due"][(c, int(q["stream_id"][k]))] = QD.fields_of(q, k)
        return r

    def decode(s, st, sid):
        d = g.step(st, sid, cont=s > 0)
        same(d, dec_m.step(st, sid, cont=s > 0), "decoder step %d: " % s)
        cf, h = st["conn_first"], d["raw"]
        a = h["arena"]
        for c in range(nconn):
            for k in range(int(cf[c]), int(cf[c + 1])):
                if d["sstatus"][k] == BLOCKED:
                    continue
                s0 = int(st["sec_off"][k])
                got = [(a[int(h["name_off"][f]):int(h["name_off"][f]) + int(h["name_len"][f])].tobytes(),
                        a[int(h["value_off"][f]):int(h["value_off"][f]) + int(h["value_len"][f])].tobytes())
                       for f in range(s0, s0 + int(h["nfields"].view(np.uint32)[k]))]
                assert got == state["due"].pop((c, int(sid[k]))), (s, c, k)
                state["fields"] += len(got)
        t = d["t"]
        return dict(t=(t["dec_out"], t["dec_out_off"], t["dec_out_len"]), host=d["dec"], len=d["dec_out_len"]), d

    def finish(dec):
        for c, conn in enumerate(enc_m.conns):
            assert conn.handle_input(dec["host"][c]) == (0, len(dec["host"][c]))
            assert conn.num_blocked == 0 and not conn.inflight, c
    closed_loop(nconn, requests, encode, decode, finish)
    assert not state["due"] and state["fields"] > 6 * nconn  # every section of every step came back
