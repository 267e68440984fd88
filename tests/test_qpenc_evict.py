"""QPACK encoder sessions that evict (include/hhuff.h (2g'), HHUFF_QENC_EVICT): a connection's table turns over
instead of freezing once it is full.
CPU: the plain-Python model of the contract (tests/qpenc_evict_model.py) against the decoders -- the restatement
always, the real qpack.c where oracle/_ref is built -- in closed loops at table sizes 128 and 256 whose insert
counts pass the full range of the wrapped Required Insert Count, and on hand scripts for every rule (pins, exact
fit, refusals before the table is touched, the mode of a session).
GPU: hhuff_qpack_flatten_sessions with the flag through codec.qpack_flatten_sessions, byte for byte against the
model; a closed loop with the GPU decoder; and the unchanged bytes of a call without the flag."""
import numpy as np
import pytest

import qpenc_dyn_model as M0
import qpenc_evict_model as M
from h2o_amd import codec as C
from h2o_amd import hpenc_synth as HE
from test_qpenc_dyn import (LTR, Gpu, T, batch, closed_loop, cpu_decoder, decoded_fields, fields_of, gpu_decoder, resp,
                            run_script, same, section_lines, section_of)

EV = C.QENC_EVICT


def model_encoder(m):
    def encode(s, q, dec):
        r = m.step(q, dec, flags=EV | (C.QENC_CONTINUE if s else C.QENC_SET_CAPACITY))
        r["count"] = m.counts()
        return r
    return encode


def with_enc_regions(q):
    """q with an encoder-stream region of hhuff_qpack_session_enc_bound per connection, 16-byte aligned"""
    h, res, cf = q["hdr"], q["res"], q["conn_first"].astype(np.int64)
    ltr = (h["flags"] & LTR) == LTR
    nv = np.concatenate([[0], np.cumsum(np.where(ltr, h["name_len"].astype(np.int64) + h["value_len"], 0))])
    nl = np.concatenate([[0], np.cumsum(ltr.astype(np.int64))])
    first, nh = res["hdr_first"].astype(np.int64), res["nhdr"].astype(np.int64)
    rv = np.concatenate([[0], np.cumsum(nv[first + nh] - nv[first])])
    rn = np.concatenate([[0], np.cumsum(nl[first + nh] - nl[first])])
    b = C.qpack_session_enc_bound(rv[cf[1:]] - rv[cf[:-1]], rn[cf[1:]] - rn[cf[:-1]], q["server_len"], cf[1:] - cf[:-1])
    return dict(q, enc_out_off=np.concatenate([[0], np.cumsum((b + 15) // 16 * 16)]).astype(np.uint64))


def turnover(nconn, steps, seed, requests=False):
    """per connection and step one to three responses whose likely-to-repeat values partly stay (the connection's
    cache-control, content-type / :authority, user-agent) and partly change with every step or response (date,
    link, vary / referer), in a random order: a table of 128 or 256 bytes holds two to four of them, so it turns
    over as the acknowledgments come back; the server name goes out now and then only (an entry that every
    section refers to first stays the oldest for good: there is no Duplicate instruction).  Plain tokens and digits only: every decoder takes them"""
    rng = np.random.default_rng(seed)
    sid = np.zeros(nconn, np.int64)
    out = []
    for s in range(steps):
        conns = []
        for c in range(nconn):
            rs = []
            for k in range(int(rng.integers(1, 4))):
                if requests:
                    own = [(b":method", b"GET", T), (b":scheme", b"https", T), (b":authority", b"host-%d.example.com" % c, T),
                           (b":path", b"/p/%d/%d/%d" % (c, s, k), T)]
                    pool = [(b"user-agent", b"agent/%d.0 (conn %d)" % (c % 7, c), LTR),
                            (b"referer", b"https://host-%d.example.com/%d" % (c, s), LTR),
                            (b"accept-language", b"en-GB;q=0.%d, en" % ((s + k) % 9 + 1), LTR), (b"x-trace", b"%d-%d" % (c, s), 0)]
                else:
                    own = []
                    pool = [(b"cache-control", b"max-age=%d" % (1000 + c), LTR), (b"content-type", b"text/x-conn-%d" % c, LTR),
                            (b"date", HE._date(86400 * c + 3 * s + k), LTR), (b"link", b"</p/%d/%d>; rel=preload" % (c, s), LTR),
                            (b"vary", b"accept-%d, origin" % ((s + k) % 5), LTR), (b"etag", b'"%d-%d"' % (c, s), T),
                            (b"x-trace", b"%d-%d" % (c, s), 0)]
                hs = own + [pool[j] for j in rng.permutation(len(pool))[:int(rng.integers(2, len(pool) + 1))]]
                rs.append(dict(status=4 if requests else 200, headers=hs, stream_id=int(sid[c]),
                               flags=C.RES_SERVER if not requests and rng.random() < 0.15 else 0))
                sid[c] += 4
            conns.append(rs)
        out.append(with_enc_regions(batch(conns, requests=requests)))
    return out


def rics(log, nconn):
    """per connection: the Required Insert Counts as written, in order, of the sections that have one"""
    out = [[] for _ in range(nconn)]
    for q, r, _ in log:
        cf = q["conn_first"]
        for c in range(nconn):
            for k in range(int(cf[c]), int(cf[c + 1])):
                ric = section_lines(section_of(r["frames"][k]))[0]
                if ric:
                    out[c].append(ric)
    return out


def check_turnover(log, m, nconn, H):
    counts = m.counts()
    assert (counts > H // 32).sum() >= nconn // 2, np.sort(counts)
    assert (counts >= 2 * (H // 32)).any()
    assert sum(c.evicted > 0 for c in m.conns) >= nconn // 2
    wrapped = [c for c, seq in enumerate(rics(log, nconn)) if any(b < a for a, b in zip(seq, seq[1:]))]
    assert wrapped, "no Required Insert Count wrapped"
    assert all(ric <= 2 * (H // 32) for seq in rics(log, nconn) for ric in seq)


# ---------------------------------------------------------------------------------------------------
# CPU 1: the model against the decoders, tables that turn over
# ---------------------------------------------------------------------------------------------------
LOOPS = [(128, 120, 7, 91, False), (256, 120, 6, 92, False), (256, 60, 6, 93, True)]


@pytest.mark.parametrize("H,nconn,steps,seed,requests", LOOPS)
def test_model_round_trip_restatement(oracle_codec, H, nconn, steps, seed, requests):
    from oracle import oracle as O

    st = turnover(nconn, steps, seed, requests)
    m = M.Model(nconn, H, 100)
    log = closed_loop(st, model_encoder(m), cpu_decoder(O.oracle(), nconn, H, 100, requests), requests)
    check_turnover(log, m, nconn, H)


@pytest.mark.parametrize("H,nconn,steps,seed,requests", LOOPS[:2])
def test_model_round_trip_reference(oracle_codec, H, nconn, steps, seed, requests):
    from oracle import oracle as O

    if not O.ref_available():
        pytest.skip("oracle/_ref not built")
    st = turnover(nconn, steps, seed, requests)
    m = M.Model(nconn, H, 100)
    closed_loop(st, model_encoder(m), cpu_decoder(O.ref(), nconn, H, 100, requests), requests)


def test_field_section_bytes_shrink(oracle_codec):
    """what the feature buys: over the same 6 steps at table size 256 the sections of the evicting sessions are
    shorter in total than those of the sessions whose table freezes"""
    from oracle import oracle as O
    from test_qpenc_dyn import model_encoder as frozen_encoder

    st = turnover(300, 6, 94)
    a = closed_loop(st, model_encoder(M.Model(300, 256, 100)), cpu_decoder(O.oracle(), 300, 256, 100, False), False)
    b = closed_loop(st, frozen_encoder(M0.Model(300, 256, 100)), cpu_decoder(O.oracle(), 300, 256, 100, False), False)
    evict, frozen = (sum(int(r["header_len"].sum()) for _, r, _ in log) for log in (a, b))
    print("field-section bytes, 6 steps x 300 connections, table 256: evicting %d, frozen %d" % (evict, frozen))
    assert evict < frozen


# ---------------------------------------------------------------------------------------------------
# CPU 2: hand scripts, one rule each; the GPU replays them byte for byte
# ---------------------------------------------------------------------------------------------------
def val(ch, n):
    return ch.encode() * n


A28, B28, C28, D28 = (val(ch, 28) for ch in "abcd")  # "vary" + 28 + 32 = 64: two fill a table of 128
P24, Q24, R24 = (val(ch, 24) for ch in "pqr")         # "priority" + 24 + 32 = 64, no static name
ack = lambda sid: M.encode_int(sid, 7, 0x80)  # noqa: E731
cancel = lambda sid: M.encode_int(sid, 6, 0x40)  # noqa: E731
CONT = C.QENC_CONTINUE


def one_under_response_bound(k, q):
    """step 0: response 0's region is one byte under its bound, response 1's exactly its bound"""
    if k == 0:
        b = [M.response_bound(q, R) for R in q["res"]]
        q["out_off"] = np.concatenate([[0], np.cumsum([b[0] - 1] + b[1:])]).astype(np.uint64)
    return q


def one_under_insert_bound(k, q):
    """step 0: the encoder-stream region is one byte under the first response's insert bound"""
    q["enc_out_off"] = np.array([0, 20 + 4 + 28 - 1 if k == 0 else 256], np.uint64)
    return q


def evict_scripts():
    """name -> dict(H=, max_inflight=, steps=[(conns, decoder streams or None)], flags=[per step] (default: the flag
    on every step), tweak=f(step, q) -> q, twin=the script of the session in which the refused response never was)"""
    s = {}
    two = [resp([(b"vary", A28, LTR), (b"vary", B28, LTR)], stream_id=0)]
    s["pinned_by_inflight"] = dict(H=128, steps=[
        ([two + [resp([(b"vary", C28, LTR)], stream_id=4)]], None),
        ([[resp([(b"vary", C28, LTR)], stream_id=8)]], [ack(0)])])
    s["pinned_by_same_section"] = dict(H=128, steps=[
        ([two, two], None),
        ([[resp([(b"vary", A28, LTR), (b"vary", C28, LTR)], stream_id=4)],     # refers to 1: the oldest stays
          [resp([(b"vary", B28, LTR), (b"vary", C28, LTR)], stream_id=4)]],    # refers to 2: 1 goes
         [ack(0), ack(0)])])
    s["nameref_source_oldest"] = dict(H=128, steps=[
        ([[resp([(b"priority", P24, LTR), (b"vary", A28, LTR)], stream_id=0)]], None),
        ([[resp([(b"priority", Q24, LTR)], stream_id=4)]], [ack(0)])])
    four = [resp([(b"vary", v, LTR) for v in (A28, B28, C28, D28)], stream_id=0)]
    s["exact_fit"] = dict(H=256, steps=[
        ([four, four], None),
        ([[resp([(b"vary", val("e", 92), LTR)], stream_id=4)],   # need 128: entries 1 and 2 go
          [resp([(b"vary", val("e", 93), LTR)], stream_id=4)]],  # need 129: entry 3 too
         [ack(0), ack(0)])])
    s["larger_than_capacity"] = dict(H=128, steps=[
        ([[resp([(b"vary", A28, LTR)], stream_id=0)]], None),
        ([[resp([(b"vary", val("x", 93), LTR)], stream_id=4)]], [ack(0)])])
    s["cancel_releases_pin"] = dict(H=128, steps=[
        ([two], None), ([[resp([(b"vary", C28, LTR)], stream_id=4)]], [cancel(0)])])
    s["acks_withheld"] = dict(H=128, steps=[
        ([[resp([(b"vary", val(ch, 28), LTR), (b"x-n", b"%d" % k, 0)], stream_id=4 * k)]], None)
        for k, ch in enumerate("abcdef")])
    for H in (0, 31):
        s["table_%d" % H] = dict(H=H, steps=[([[resp([(b"vary", A28, LTR), (b"priority", b"u=1", LTR)],
                                                     flags=C.RES_SERVER, stream_id=4 * k)]], None) for k in range(2)])
    first = resp([(b"vary", A28, LTR)], stream_id=0)
    second = resp([(b"vary", b"12345678", LTR), (b"x-a", b"b", 0)], stream_id=4)
    later = [([[resp([(b"vary", A28, LTR), (b"vary", b"12345678", LTR)], stream_id=8)]], None)]
    s["space_response"] = dict(H=128, steps=[([[first, second]], None)] + later, tweak=one_under_response_bound,
                               twin=dict(H=128, steps=[([[second]], None)] + later), refused=0)
    s["space_enc"] = dict(H=128, steps=[([[first, second]], None)] + later, tweak=one_under_insert_bound,
                          twin=dict(H=128, steps=[([[second]], None)] + later, tweak=one_under_insert_bound), refused=0)
    s["inflight_full"] = dict(H=128, max_inflight=1, steps=[
        ([[resp([(b"vary", A28, LTR)], stream_id=0), resp([(b"x-a", b"b", 0)], stream_id=4)]], None)])
    s["mode_mix"] = dict(H=128, flags=[EV, CONT, CONT | EV], steps=[
        ([two], None), ([[resp([(b"vary", C28, LTR)], stream_id=4)]], [ack(0)]),
        ([[resp([(b"vary", C28, LTR)], stream_id=4)]], [ack(0)])])
    return s


def script_steps(sc, encode):
    """-> [(q, result)] per step; encode(q, dec, flags) -> model-shaped result"""
    out = []

    def step(k, q, dec, flags):
        q = with_enc_regions(q)
        q = sc["tweak"](k, q) if "tweak" in sc else q
        out.append((q, encode(q, dec, sc["flags"][k] if "flags" in sc else flags | EV)))
        return out[-1][1]
    run_script(sc, step)
    return out


def model_script(sc):
    n = len(sc["steps"][0][0])
    m = M.Model(n, sc.get("H", 4096), sc.get("max_blocked", 100), sc.get("max_inflight", 64))
    return m, script_steps(sc, m.step)


def decode_script(sc, log, codec):
    """every step's encoder streams are consumed whole and every section decodes to its response's fields"""
    n = len(sc["steps"][0][0])
    dec = cpu_decoder(codec, n, sc.get("H", 4096), 100, False)
    for k, (q, r) in enumerate(log):
        assert (r["rstatus"] == 0).all(), k
        d = dec(q, r["frames"], r["enc"])
        assert (d["enc_status"][:n] == 0).all() and (d["sstatus"][:q["res"].size] == 0).all(), k
        np.testing.assert_array_equal(d["enc_consumed"][:n], r["enc_out_len"][:n])
        for j in range(q["res"].size):
            assert decoded_fields(d, d["sec_off"], j) == fields_of(q, j), (k, j)


# (mode_mix's accepted steps are pinned_by_inflight's; a script with a refused response is decoded as its twin)
@pytest.mark.parametrize("name", sorted(set(evict_scripts()) - {"mode_mix"}))
def test_scripts_decode(oracle_codec, name):
    from oracle import oracle as O

    sc = evict_scripts()[name]
    sc = sc.get("twin", sc)
    for codec in [O.oracle()] + ([O.ref()] if O.ref_available() else []):
        decode_script(sc, model_script(sc)[1], codec)


def kinds(frame):
    return section_lines(section_of(frame))[1]


def insert_of(name_ref, value):
    return name_ref + M.qstring(value)


VARY = bytes([0xC0 | 59])  # Insert With Name Reference, static 59 (vary)


def test_script_pinned_by_inflight(oracle_codec):
    m, ((_, r0), (_, r1)) = model_script(evict_scripts()["pinned_by_inflight"])
    assert r0["enc"][0] == insert_of(VARY, A28) + insert_of(VARY, B28)
    assert kinds(r0["frames"][1]) == ["static", "sname"] and not r0["inflight"][1]  # entry 1 is pinned: no insert
    assert r1["enc"][0] == insert_of(VARY, C28) and kinds(r1["frames"][0]) == ["static", "post"]
    c = m.conns[0]
    assert (c.evicted, c.count, c.used) == (1, 3, 128)


def test_script_pinned_by_same_section(oracle_codec):
    m, (_, (_, r1)) = model_script(evict_scripts()["pinned_by_same_section"])
    assert r1["enc"][0] == b"" and kinds(r1["frames"][0]) == ["static", "pre", "sname"]
    assert r1["enc"][1] == insert_of(VARY, C28) and kinds(r1["frames"][1]) == ["static", "pre", "post"]
    assert [(c.evicted, c.count) for c in m.conns] == [(0, 2), (1, 3)]


def test_script_nameref_source_is_the_oldest(oracle_codec):
    m, (_, (_, r1)) = model_script(evict_scripts()["nameref_source_oldest"])
    assert r1["enc"][0] == b"" and kinds(r1["frames"][0]) == ["static", "pre-name"]
    assert (m.conns[0].evicted, m.conns[0].count) == (0, 2)


def test_script_exact_fit_and_one_byte_more(oracle_codec):
    m, _ = model_script(evict_scripts()["exact_fit"])
    assert [(c.evicted, c.count, c.used) for c in m.conns] == [(2, 5, 256), (3, 5, 64 + 129)]


def test_script_larger_than_capacity(oracle_codec):
    m, (_, (_, r1)) = model_script(evict_scripts()["larger_than_capacity"])
    assert r1["enc"][0] == b"" and kinds(r1["frames"][0]) == ["static", "sname"]
    assert (m.conns[0].evicted, m.conns[0].count, m.conns[0].used) == (0, 1, 64)


def test_script_cancel_releases_pin(oracle_codec):
    m, (_, (_, r1)) = model_script(evict_scripts()["cancel_releases_pin"])
    c = m.conns[0]
    assert r1["enc"][0] == insert_of(VARY, C28) and (c.evicted, c.count, c.lkr) == (1, 3, 0) and r1["blocking"][0]


def test_script_acks_withheld(oracle_codec):
    m, log = model_script(evict_scripts()["acks_withheld"])
    assert [len(r["enc"][0]) > 0 for _, r in log] == [True, True, False, False, False, False]
    assert all((r["rstatus"] == 0).all() for _, r in log)
    assert (m.conns[0].evicted, m.conns[0].count) == (0, 2) and len(m.conns[0].inflight) == 2


@pytest.mark.parametrize("H", [0, 31])
def test_script_tables_too_small_never_insert(oracle_codec, H):
    m, log = model_script(evict_scripts()["table_%d" % H])
    assert all(r["enc"][0] == b"" and not r["inflight"].any() and (r["rstatus"] == 0).all() for _, r in log)
    assert m.conns[0].count == 0


@pytest.mark.parametrize("name", ["space_response", "space_enc"])
def test_script_refusal_leaves_no_trace(oracle_codec, name):
    sc = evict_scripts()[name]
    m, log = model_script(sc)
    t, twin = model_script(sc["twin"])
    assert list(log[0][1]["rstatus"]) == [C.RES_SPACE, 0] and log[0][1]["frames"][0] == b""
    assert log[0][1]["frames"][1] == twin[0][1]["frames"][0] and log[0][1]["enc"] == twin[0][1]["enc"]
    assert log[0][1]["enc"][0] != b""
    assert log[1][1]["frames"] == twin[1][1]["frames"] and log[1][1]["enc"] == twin[1][1]["enc"]
    assert (log[1][1]["rstatus"] == 0).all()
    assert (m.conns[0].evicted, m.conns[0].count, m.conns[0].inflight) == (t.conns[0].evicted, t.conns[0].count, t.conns[0].inflight)


def test_script_region_of_exactly_the_bound_is_accepted(oracle_codec):
    q = batch([[resp([(b"vary", A28, LTR), (b"x-a", b"b", 0)], flags=C.RES_SERVER, content_length=5, dfid=b"77")]])
    b = M.response_bound(q, q["res"][0])
    for region, want in ((b, 0), (b - 1, C.RES_SPACE)):
        q["out_off"] = np.array([0, region], np.uint64)
        assert M.Model(1, 128).step(q)["rstatus"][0] == want
    q["out_off"] = np.array([0, b], np.uint64)
    ib = M.insert_bound(q, q["res"][0])
    assert ib == 20 + 4 + 28 + 20 + 6 + q["server_len"]
    for room, want in ((ib, 0), (ib - 1, C.RES_SPACE)):
        q["enc_out_off"] = np.array([0, room], np.uint64)
        assert M.Model(1, 128).step(q)["rstatus"][0] == want


def test_script_inflight_list_full(oracle_codec):
    m, ((_, r0),) = model_script(evict_scripts()["inflight_full"])
    assert list(r0["rflags"]) == [0, 1] and list(r0["rstatus"]) == [0, 0]
    assert section_of(r0["frames"][1])[:2] == b"\0\0" and len(m.conns[0].inflight) == 1


def test_script_mode_mix_is_refused(oracle_codec):
    m, log = model_script(evict_scripts()["mode_mix"])
    r1, r2 = log[1][1], log[2][1]
    assert (r1["rstatus"] == C.RES_EINVAL).all() and r1["dec_status"][0] == C.RES_EINVAL and r1["dec_consumed"][0] == 0
    assert r1["frames"] == [b""] and r1["enc"] == [b""]
    assert r2["enc"][0] == insert_of(VARY, C28) and (r2["rstatus"] == 0).all() and r2["dec_consumed"][0] == 1


def test_bound_helpers_match_the_header():
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hhuff.h")).read()
    assert re.search(r"#define HHUFF_QENC_EVICT 4u", text) and C.QENC_EVICT == 4
    assert "hhuff_qpack_session_enc_bound" in text
    assert C.qpack_session_enc_bound(100, 3, 10, 2) == 4 + 100 + 60 + 2 * 36
    assert C.qpack_session_enc_bound(100, 3, 0, 2) == 4 + 100 + 60


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


class EGpu(Gpu):
    """Gpu whose steps pass evict= from the step's flags"""

    def step(self, q, dec=None, flags=0, guard=64):
        real = C.qpack_flatten_sessions
        C.qpack_flatten_sessions = lambda *a, **kw: real(*a, evict=bool(flags & EV), **kw)
        try:
            return super().step(q, dec, flags, guard)
        finally:
            C.qpack_flatten_sessions = real


def gpu_of(torch, sc, n):
    return EGpu(torch, n, sc.get("H", 4096), sc.get("max_blocked", 100), sc.get("max_inflight", 64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(evict_scripts()))
def test_gpu_scripts(torch_cuda, name):
    sc = evict_scripts()[name]
    want = model_script(sc)[1]
    g = gpu_of(torch_cuda, sc, len(sc["steps"][0][0]))
    got = script_steps(sc, g.step)
    for k, ((_, a), (_, b)) in enumerate(zip(got, want)):
        same(a, b, "%s step %d: " % (name, k))


def gpu_against_model(torch, st, nconn, H, move=False, decoder=None):
    from oracle import oracle as O

    m, g = M.Model(nconn, H), EGpu(torch, nconn, H, move=move)
    enc_m = model_encoder(m)

    def encode(s, q, dec):
        w = enc_m(s, q, dec)
        same(g.step(q, dec, flags=EV | (C.QENC_CONTINUE if s else C.QENC_SET_CAPACITY)), w, "step %d: " % s)
        return w
    log = closed_loop(st, encode, decoder or cpu_decoder(O.oracle(), nconn, H, 100, False), False)
    return m, log


@pytest.mark.gpu
@pytest.mark.parametrize("move", [False, True])
def test_gpu_300_connections_6_steps(torch_cuda, oracle_codec, move):
    """bytes against the model at table size 256, the restatement's acknowledgments fed back; move: the scratch is
    copied to a new allocation between the steps (it holds offsets, not addresses)"""
    st = turnover(300, 6, 94)
    m, log = gpu_against_model(torch_cuda, st, 300, 256, move=move)
    check_turnover(log, m, 300, 256)


@pytest.mark.gpu
def test_gpu_65_connections(torch_cuda, oracle_codec):
    """one past a 64-lane block"""
    st = turnover(65, 6, 95)
    m, log = gpu_against_model(torch_cuda, st, 65, 128)
    assert (m.counts() > 4).any()


@pytest.mark.gpu
def test_gpu_closed_loop_with_the_gpu_decoder(torch_cuda):
    """GPU encoder -> GPU decoder -> its acknowledgments back into the GPU encoder at table size 128"""
    st = turnover(120, 7, 91)
    g, m = EGpu(torch_cuda, 120, 128), M.Model(120, 128)

    def encode(s, q, dec):
        flags = EV | (C.QENC_CONTINUE if s else C.QENC_SET_CAPACITY)
        r, w = g.step(q, dec, flags=flags), m.step(q, dec, flags=flags)
        assert r["guards_intact"]
        r["inflight"], r["count"] = w["inflight"], m.counts()
        return r
    log = closed_loop(st, encode, gpu_decoder(torch_cuda, 120, 128, 100, False), False)
    check_turnover(log, m, 120, 128)


@pytest.mark.gpu
def test_gpu_without_the_flag_the_old_bytes(torch_cuda, oracle_codec):
    """a session that fills a 256-byte table, flattened without the flag: the bytes of the table that freezes"""
    from oracle import oracle as O
    from test_qpenc_dyn import model_encoder as frozen_encoder

    st = turnover(100, 4, 96)
    m, g = M0.Model(100, 256), EGpu(torch_cuda, 100, 256)
    enc_m = frozen_encoder(m)

    def encode(s, q, dec):
        w = enc_m(s, q, dec)
        same(g.step(q, dec, flags=C.QENC_CONTINUE if s else C.QENC_SET_CAPACITY), w, "step %d: " % s)
        return w
    closed_loop(st, encode, cpu_decoder(O.oracle(), 100, 256, 100, False), False)
    assert sum(c.cap - c.used < 64 for c in m.conns) >= 50  # the tables are full


@pytest.mark.gpu
def test_gpu_flag_on_a_session_started_without_it(torch_cuda):
    q = batch([[resp([(b"vary", A28, LTR)], stream_id=0)]])
    g = EGpu(torch_cuda, 1, 128)
    assert g.step(q)["rstatus"][0] == 0
    before = g.scratch.cpu().numpy().copy()
    r = g.step(q, flags=CONT | EV)
    assert r["rstatus"][0] == C.RES_EINVAL and r["dec_status"][0] == C.RES_EINVAL and r["out_len"][0] == 0
    assert (r["out_raw"] == 0xA5).all() and (r["enc_raw"] == 0xA5).all() and r["guards_intact"]
    np.testing.assert_array_equal(g.scratch.cpu().numpy(), before)
    w = M0.Model(1, 128)
    w.step(q)
    same(g.step(q, flags=CONT), w.step(q, flags=CONT))


def test_unknown_flag_is_refused():
    from h2o_amd import build

    build.build(verbose=False)
    L = C.lib()
    nul = [None] * 12
    assert L.hhuff_qpack_flatten_sessions(None, 0, None, 0, None, None, 1, 0, None, None, None, 4096, 100, 64, 0, 0,
                                          *nul, 0, 8, None) == C.RES_EINVAL
