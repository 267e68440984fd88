"""QPACK encoder sessions that duplicate draining entries (include/hhuff.h (2g'), HHUFF_QENC_EVICT | HHUFF_QENC_DUP,
point 7 of "Under the flag"): an entry every section refers to -- the server name -- no longer ends up the oldest
and pinned for good; it is re-inserted by a Duplicate instruction and the table goes on turning over behind it.
CPU: the plain-Python model of the contract (tests/qpenc_dup_model.py) against the decoders -- the restatement
always, the real qpack.c where oracle/_ref is built -- in closed loops whose every response sends the server name,
at table sizes 128 and 256; what the rule buys against HHUFF_QENC_EVICT alone; hand scripts, one rule each.
GPU: hhuff_qpack_flatten_sessions with both flags through codec.qpack_flatten_sessions, byte for byte against the
model; a closed loop with the GPU decoder; the refusal of a call whose mode is not the session's."""
import numpy as np
import pytest

import qpenc_dup_model as M
import qpenc_dyn_model as M0
import qpenc_evict_model as ME
from h2o_amd import codec as C
from h2o_amd import hpenc_synth as HE
from test_qpenc_dyn import LTR, NOENC, Gpu, T, batch, closed_loop, cpu_decoder, gpu_decoder, resp, run_script, same
from test_qpenc_evict import (A28, B28, C28, P24, VARY, ack, check_turnover, decode_script, insert_of, kinds, turnover, val,
                              with_enc_regions)

EV, DUP, CONT = C.QENC_EVICT, C.QENC_DUP, C.QENC_CONTINUE
SRV = C.RES_SERVER


def model_encoder(m, mode=EV | DUP):
    def encode(s, q, dec):
        r = m.step(q, dec, flags=mode | (CONT if s else C.QENC_SET_CAPACITY))
        r["count"] = m.counts()
        return r
    return encode


def hot_server(nconn, steps, seed):
    """test_qpenc_evict.turnover()'s responses -- per connection and step one to three, likely-to-repeat values that
    partly stay and partly change -- with the server name on every one of them, as an HTTP/3 server sends it: the
    entry every section refers to"""
    rng = np.random.default_rng(seed)
    sid = np.zeros(nconn, np.int64)
    out = []
    for s in range(steps):
        conns = []
        for c in range(nconn):
            rs = []
            for k in range(int(rng.integers(1, 4))):
                pool = [(b"cache-control", b"max-age=%d" % (1000 + c), LTR), (b"content-type", b"text/x-conn-%d" % c, LTR),
                        (b"date", HE._date(86400 * c + 3 * s + k), LTR), (b"link", b"</p/%d/%d>; rel=preload" % (c, s), LTR),
                        (b"vary", b"accept-%d, origin" % ((s + k) % 5), LTR), (b"etag", b'"%d-%d"' % (c, s), T),
                        (b"x-trace", b"%d-%d" % (c, s), 0)]
                hs = [pool[j] for j in rng.permutation(len(pool))[:int(rng.integers(2, len(pool) + 1))]]
                rs.append(dict(status=200, headers=hs, stream_id=int(sid[c]), flags=SRV))
                sid[c] += 4
            conns.append(rs)
        out.append(with_enc_regions(batch(conns)))
    return out


def evicted(m):
    return np.array([c.evicted for c in m.conns])


def duplicates(log):
    """the Duplicate instructions (000 pattern) of every encoder stream of a closed loop"""
    n = 0
    for _, r, _ in log:
        for e in r["enc"]:
            p = 0
            while p < len(e):
                b = e[p]
                if b & 0x80:    # Insert With Name Reference, then the value
                    _, p = M0.decode_int(e, p, 6)
                elif b & 0x40:  # Insert With Literal Name
                    v, p = M0.decode_int(e, p, 5)
                    p += v
                else:           # Set Dynamic Table Capacity (001) or Duplicate (000)
                    n += 0 if b & 0x20 else 1
                    p = M0.decode_int(e, p, 5)[1]
                    continue
                v, p = M0.decode_int(e, p, 7)
                p += v
            assert p == len(e)
    return n


# ---------------------------------------------------------------------------------------------------
# CPU 1: the model against the decoders, every response with the server name
# ---------------------------------------------------------------------------------------------------
LOOPS = [(128, 120, 7, 191), (256, 100, 8, 192)]


@pytest.mark.parametrize("H,nconn,steps,seed", LOOPS)
def test_model_round_trip_restatement(oracle_codec, H, nconn, steps, seed):
    from oracle import oracle as O

    st = hot_server(nconn, steps, seed)
    m = M.Model(nconn, H, 100)
    log = closed_loop(st, model_encoder(m), cpu_decoder(O.oracle(), nconn, H, 100, False), False)
    check_turnover(log, m, nconn, H)
    assert duplicates(log) >= nconn


@pytest.mark.parametrize("H,nconn,steps,seed", LOOPS)
def test_model_round_trip_reference(oracle_codec, H, nconn, steps, seed):
    from oracle import oracle as O

    if not O.ref_available():
        pytest.skip("oracle/_ref not built")
    st = hot_server(nconn, steps, seed)
    m = M.Model(nconn, H, 100)
    closed_loop(st, model_encoder(m), cpu_decoder(O.ref(), nconn, H, 100, False), False)


def test_model_round_trip_requests(oracle_codec):
    """the client side: test_qpenc_evict.turnover()'s requests, whose user-agent every one of a connection's
    sections may refer to"""
    from oracle import oracle as O

    st = turnover(60, 6, 93, True)
    m = M.Model(60, 256, 100)
    log = closed_loop(st, model_encoder(m), cpu_decoder(O.oracle(), 60, 256, 100, True), True)
    assert duplicates(log) > 0 and (evicted(m) > 0).sum() >= 30


@pytest.mark.parametrize("H", [128, 256])
def test_what_duplicating_buys(oracle_codec, H):
    """the same 8 steps x 100 connections under HHUFF_QENC_EVICT alone and with HHUFF_QENC_DUP: with the server
    name on every response the evicting table alone freezes behind it; the duplicating one turns over and its field
    sections are shorter in total"""
    from oracle import oracle as O

    st = hot_server(100, 8, 193)
    ma, mb = M.Model(100, H, 100), M.Model(100, H, 100)
    a = closed_loop(st, model_encoder(ma), cpu_decoder(O.oracle(), 100, H, 100, False), False)
    b = closed_loop(st, model_encoder(mb, EV), cpu_decoder(O.oracle(), 100, H, 100, False), False)
    dup, alone = (sum(int(r["header_len"].sum()) for _, r, _ in log) for log in (a, b))
    dup_enc, alone_enc = (sum(int(r["enc_out_len"].sum()) for _, r, _ in log) for log in (a, b))
    print("8 steps x 100 connections, table %d, server name on every response: evicted entries %d with DUP, %d with "
          "EVICT alone; field-section bytes %d against %d; encoder-stream bytes %d against %d; %d Duplicate instructions"
          % (H, evicted(ma).sum(), evicted(mb).sum(), dup, alone, dup_enc, alone_enc, duplicates(a)))
    assert (evicted(ma) > 0).sum() >= 50
    assert evicted(mb).sum() < evicted(ma).sum()
    assert dup < alone
    assert duplicates(b) == 0


# ---------------------------------------------------------------------------------------------------
# CPU 2: hand scripts, one rule each; the GPU replays them byte for byte
# ---------------------------------------------------------------------------------------------------
def dup_scripts():
    """name -> dict(H=, steps=[(conns, decoder streams or None)], flags=[per step] (default: both flags on every
    step))"""
    s = {}
    two = [resp([(b"vary", A28, LTR), (b"vary", B28, LTR)], stream_id=0)]

    def after_two(headers, dec=(ack(0),), **kw):
        return dict(H=128, steps=[([two], None), ([[resp(headers, stream_id=4, **kw)]], list(dec) if dec else None)])
    s["oldest_evicts_itself"] = after_two([(b"vary", A28, LTR)])
    s["second_oldest_not_draining"] = after_two([(b"vary", B28, LTR)])
    s["pinned_by_inflight"] = after_two([(b"vary", A28, LTR)], dec=None)
    s["twice_in_a_section"] = after_two([(b"vary", A28, LTR), (b"vary", A28, LTR)])
    s["pinned_by_same_section"] = dict(H=128, steps=[
        ([[resp([(b"priority", P24, LTR), (b"vary", A28, LTR)], stream_id=0)]], None),
        ([[resp([(b"priority", b"u=1", LTR), (b"priority", P24, LTR)], stream_id=4)]], [ack(0)])])
    s["not_ltr"] = after_two([(b"vary", A28, T)])
    s["no_encoder_stream"] = after_two([(b"vary", A28, LTR)], flags=NOENC)
    s["server"] = dict(H=128, steps=[([[resp([(b"vary", A28, LTR)], stream_id=0, flags=SRV)]], None),
                                     ([[resp([], stream_id=4, flags=SRV)]], [ack(0)])])
    for name, third in (("edge_at_D", C28), ("edge_under_D", val("c", 29))):  # headroom of the oldest: 64 = H / 4, 63
        s[name] = dict(H=256, steps=[
            ([[resp([(b"vary", A28, LTR), (b"vary", B28, LTR), (b"vary", third, LTR)], stream_id=0)]], None),
            ([[resp([(b"vary", A28, LTR)], stream_id=4)]], [ack(0)])])
    v64 = [b"%028d" % k for k in range(64)]
    s["two_byte_index"] = dict(H=4096, steps=[
        ([[resp([(b"vary", v, LTR) for v in v64], stream_id=0)]], None),
        ([[resp([(b"vary", v64[0], LTR), (b"vary", v64[15], LTR), (b"vary", v64[16], LTR)], stream_id=4)]], [ack(0)])])
    mix = [([two], None), ([[resp([(b"vary", A28, LTR)], stream_id=4)]], [ack(0)]),
           ([[resp([(b"vary", A28, LTR)], stream_id=4)]], [ack(0)])]
    s["dup_mode_mix"] = dict(H=128, flags=[EV | DUP, CONT | EV, CONT | EV | DUP], steps=mix)
    s["dup_mode_mix_on_evict"] = dict(H=128, flags=[EV, CONT | EV | DUP, CONT | EV], steps=mix)
    return s


def script_steps(sc, encode):
    """-> [(q, result)] per step; encode(q, dec, flags) -> model-shaped result"""
    out = []

    def step(k, q, dec, flags):
        q = with_enc_regions(q)
        out.append((q, encode(q, dec, sc["flags"][k] if "flags" in sc else flags | EV | DUP)))
        return out[-1][1]
    run_script(sc, step)
    return out


def model_script(sc):
    m = M.Model(len(sc["steps"][0][0]), sc.get("H", 4096))
    return m, script_steps(sc, m.step)


def state(m):
    c = m.conns[0]
    return c.evicted, c.count, c.used


@pytest.mark.parametrize("name", sorted(set(dup_scripts()) - {"dup_mode_mix", "dup_mode_mix_on_evict"}))
def test_scripts_decode(oracle_codec, name):
    from oracle import oracle as O

    sc = dup_scripts()[name]
    for codec in [O.oracle()] + ([O.ref()] if O.ref_available() else []):
        decode_script(sc, model_script(sc)[1], codec)


def test_script_oldest_evicts_itself(oracle_codec):
    m, ((_, r0), (_, r1)) = model_script(dup_scripts()["oldest_evicts_itself"])
    assert r0["enc"][0] == insert_of(VARY, A28) + insert_of(VARY, B28)
    assert r1["enc"][0] == b"\x01" and kinds(r1["frames"][0]) == ["static", "post"]
    assert state(m) == (1, 3, 128) and m.conns[0].ent == [(b"vary", B28), (b"vary", A28)]
    assert r1["blocking"][0] and r1["inflight"][0]


def test_script_second_oldest_is_not_draining(oracle_codec):
    m, (_, (_, r1)) = model_script(dup_scripts()["second_oldest_not_draining"])
    assert r1["enc"][0] == b"" and kinds(r1["frames"][0]) == ["static", "pre"] and state(m) == (0, 2, 128)


def test_script_pinned_by_inflight(oracle_codec):
    m, (_, (_, r1)) = model_script(dup_scripts()["pinned_by_inflight"])
    assert r1["enc"][0] == b"" and kinds(r1["frames"][0]) == ["static", "pre"] and state(m) == (0, 2, 128)


def test_script_twice_in_a_section(oracle_codec):
    """the second A finds the duplicate, the newest entry, which is not draining"""
    m, (_, (_, r1)) = model_script(dup_scripts()["twice_in_a_section"])
    assert r1["enc"][0] == b"\x01" and kinds(r1["frames"][0]) == ["static", "post", "post"] and state(m) == (1, 3, 128)


def test_script_pinned_by_same_section(oracle_codec):
    """the name reference to entry 1 pins it before the exact match on it asks for room"""
    m, (_, (_, r1)) = model_script(dup_scripts()["pinned_by_same_section"])
    assert r1["enc"][0] == b"" and kinds(r1["frames"][0]) == ["static", "pre-name", "pre"] and state(m) == (0, 2, 128)


@pytest.mark.parametrize("name", ["not_ltr", "no_encoder_stream"])
def test_script_rule_is_not_tried(oracle_codec, name):
    m, (_, (_, r1)) = model_script(dup_scripts()[name])
    assert r1["enc"][0] == b"" and kinds(r1["frames"][0]) == ["static", "pre"] and state(m) == (0, 2, 128)


def test_script_server(oracle_codec):
    """the server's slot carries the instruction: entry 1 (server, 6 + 13 + 32 = 51 bytes) goes and comes back"""
    m, ((_, r0), (_, r1)) = model_script(dup_scripts()["server"])
    assert [n for n, _ in m.conns[0].ent] == [b"vary", b"server"]
    assert r1["enc"][0] == b"\x01" and kinds(r1["frames"][0]) == ["static", "post"] and state(m) == (1, 3, 115)


def test_script_edge_of_the_quarter(oracle_codec):
    m, (_, (_, r1)) = model_script(dup_scripts()["edge_at_D"])
    assert r1["enc"][0] == b"" and kinds(r1["frames"][0]) == ["static", "pre"] and state(m) == (0, 3, 192)
    m, (_, (_, r1)) = model_script(dup_scripts()["edge_under_D"])
    assert r1["enc"][0] == b"\x02" and kinds(r1["frames"][0]) == ["static", "post"] and state(m) == (1, 4, 193)


def test_script_two_byte_index(oracle_codec):
    """relative indices 63, 49 and 49: past the 5-bit prefix"""
    m, (_, (_, r1)) = model_script(dup_scripts()["two_byte_index"])
    assert r1["enc"][0] == bytes.fromhex("1f201f121f12") and kinds(r1["frames"][0]) == ["static", "post", "post", "post"]
    assert state(m) == (3, 67, 4096)


def test_script_dup_needs_evict():
    from h2o_amd import build

    build.build(verbose=False)
    L = C.lib()
    nul = [None] * 12
    for flags, want in ((DUP, C.RES_EINVAL), (DUP | CONT, C.RES_EINVAL), (DUP | C.QENC_SET_CAPACITY, C.RES_EINVAL),
                        (DUP | EV, 0), (16, C.RES_EINVAL)):
        assert L.hhuff_qpack_flatten_sessions(None, 0, None, 0, None, None, 0, 0, None, None, None, 4096, 100, 64, 0, 0,
                                              *nul, 0, flags, None) == want, flags
    with pytest.raises(AssertionError):
        M.Model(1, 128).step(batch([[resp([])]]), flags=DUP)


@pytest.mark.parametrize("name,third", [("dup_mode_mix", b"\x01"), ("dup_mode_mix_on_evict", b"")])
def test_script_dup_mode_mix_is_refused(oracle_codec, name, third):
    m, log = model_script(dup_scripts()[name])
    r1, r2 = log[1][1], log[2][1]
    assert (r1["rstatus"] == C.RES_EINVAL).all() and r1["dec_status"][0] == C.RES_EINVAL and r1["dec_consumed"][0] == 0
    assert r1["frames"] == [b""] and r1["enc"] == [b""]
    assert r2["enc"][0] == third and (r2["rstatus"] == 0).all() and r2["dec_consumed"][0] == 1


def test_flag_value_matches_the_header():
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hhuff.h")).read()
    assert re.search(r"#define HHUFF_QENC_DUP 8u", text) and C.QENC_DUP == 8 and M.DUP == 8


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


class DGpu(Gpu):
    """Gpu whose steps pass evict= and dup= from the step's flags"""

    def step(self, q, dec=None, flags=0, guard=64):
        real = C.qpack_flatten_sessions
        C.qpack_flatten_sessions = lambda *a, **kw: real(*a, evict=bool(flags & EV), dup=bool(flags & DUP), **kw)
        try:
            return super().step(q, dec, flags, guard)
        finally:
            C.qpack_flatten_sessions = real


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(dup_scripts()))
def test_gpu_scripts(torch_cuda, name):
    sc = dup_scripts()[name]
    want = model_script(sc)[1]
    g = DGpu(torch_cuda, len(sc["steps"][0][0]), sc.get("H", 4096))
    got = script_steps(sc, g.step)
    for k, ((_, a), (_, b)) in enumerate(zip(got, want)):
        same(a, b, "%s step %d: " % (name, k))


def gpu_against_model(torch, st, nconn, H, move=False, requests=False):
    from oracle import oracle as O

    m, g = M.Model(nconn, H), DGpu(torch, nconn, H, move=move)
    enc_m = model_encoder(m)

    def encode(s, q, dec):
        w = enc_m(s, q, dec)
        same(g.step(q, dec, flags=EV | DUP | (CONT if s else C.QENC_SET_CAPACITY)), w, "step %d: " % s)
        return w
    log = closed_loop(st, encode, cpu_decoder(O.oracle(), nconn, H, 100, requests), requests)
    return m, log


@pytest.mark.gpu
@pytest.mark.parametrize("move", [False, True])
def test_gpu_300_connections_6_steps(torch_cuda, oracle_codec, move):
    """bytes against the model at table size 256 with the hot server name, the restatement's acknowledgments fed
    back; move: the scratch is copied to a new allocation between the steps (it holds offsets, not addresses)"""
    st = hot_server(300, 6, 194)
    m, log = gpu_against_model(torch_cuda, st, 300, 256, move=move)
    assert (evicted(m) > 0).sum() >= 150 and duplicates(log) >= 300


@pytest.mark.gpu
def test_gpu_65_connections(torch_cuda, oracle_codec):
    """one past a 64-lane block"""
    st = hot_server(65, 6, 195)
    m, log = gpu_against_model(torch_cuda, st, 65, 128)
    assert (evicted(m) > 0).sum() >= 32 and duplicates(log) >= 65


@pytest.mark.gpu
def test_gpu_requests(torch_cuda, oracle_codec):
    """the client side against the model: test_model_round_trip_requests' sessions"""
    m, log = gpu_against_model(torch_cuda, turnover(60, 6, 93, True), 60, 256, requests=True)
    assert duplicates(log) > 0


@pytest.mark.gpu
def test_gpu_closed_loop_with_the_gpu_decoder(torch_cuda):
    """GPU encoder -> GPU decoder -> its acknowledgments back into the GPU encoder at table size 128"""
    st = hot_server(120, 7, 191)
    g, m = DGpu(torch_cuda, 120, 128), M.Model(120, 128)

    def encode(s, q, dec):
        flags = EV | DUP | (CONT if s else C.QENC_SET_CAPACITY)
        r, w = g.step(q, dec, flags=flags), m.step(q, dec, flags=flags)
        assert r["guards_intact"]
        r["inflight"], r["count"] = w["inflight"], m.counts()
        return r
    log = closed_loop(st, encode, gpu_decoder(torch_cuda, 120, 128, 100, False), False)
    check_turnover(log, m, 120, 128)
    assert duplicates(log) >= 120


@pytest.mark.gpu
def test_gpu_dup_on_a_session_started_with_evict_alone(torch_cuda):
    q = with_enc_regions(batch([[resp([(b"vary", A28, LTR)], stream_id=0)]]))
    g = DGpu(torch_cuda, 1, 128)
    assert g.step(q, flags=EV)["rstatus"][0] == 0
    before = g.scratch.cpu().numpy().copy()
    r = g.step(q, flags=CONT | EV | DUP)
    assert r["rstatus"][0] == C.RES_EINVAL and r["dec_status"][0] == C.RES_EINVAL and r["out_len"][0] == 0
    assert r["enc_out_len"][0] == 0 and r["dec_consumed"][0] == 0
    assert (r["out_raw"] == 0xA5).all() and (r["enc_raw"] == 0xA5).all() and r["guards_intact"]
    np.testing.assert_array_equal(g.scratch.cpu().numpy(), before)
    w = ME.Model(1, 128)
    w.step(q)
    same(g.step(q, flags=CONT | EV), w.step(q, flags=CONT | EV))
