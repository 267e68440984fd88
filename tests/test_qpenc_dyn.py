"""QPACK encoder sessions (include/hhuff.h (2g'), hhuff_qpack_flatten_sessions): a dynamic table per connection,
the encoder stream it produces and the decoder stream it reads (h2o_qpack_flatten_response / _request with an
encoder-stream buffer, lib/http3/qpack.c:1148-1213 and :1244-1310; h2o_qpack_encoder_handle_input, :902-1005).
CPU: the plain-Python model of the contract (tests/qpenc_dyn_model.py) against the decoders -- the restatement
always, the real qpack.c where oracle/_ref is built -- in a closed loop (sections and encoder streams decoded,
acknowledgments fed back), against the pinned bytes of the static path (tests/golden/qpenc.npz), on the
reference's own unit test, on the decision's and the decoder stream's edges, and the library's exports.
GPU: hhuff_qpack_flatten_sessions through the C ABI, byte for byte against the model; a closed loop with the GPU
decoder (hhuff_qpack_parse_responses / _requests); the unchanged static path; malformed input."""
import os

import numpy as np
import pytest

import qpenc_dyn_model as M
from conftest import load_golden
from h2o_amd import codec as C
from h2o_amd import hpenc_synth as HE

T, LTR, DC = C.HDR_TOKEN, C.HDR_TOKEN | C.HDR_LIKELY_TO_REPEAT, C.HDR_DONT_COMPRESS
NOENC = C.QRES_NO_ENCODER_STREAM


# ---------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------
def batch(conns, server=HE.SERVER, requests=False):
    """conns = [[response, ...] per connection]; response = dict(status=, headers=[(name, value, flags)],
    content_length=None, flags=, stream_id=, dfid=None) -> one step's dict for the model and the GPU"""
    b = HE.build_batch([[dict(r, flags=(C.RES_REQUEST if requests else r.get("flags", 0) & C.RES_SERVER)) for r in rs]
                        for rs in conns], server)
    q = HE.to_qpack_requests(b, dfid_frac=0.0) if requests else HE.to_qpack(b, dfid_frac=0.0, odd_status_frac=0.0)
    rs = [r for c in conns for r in c]
    extra = b""
    for k, r in enumerate(rs):
        q["res"]["flags"][k] |= r.get("flags", 0) & NOENC
        q["res"]["status"][k] = r.get("status", 200)
        if r.get("dfid") is not None:
            q["res"]["flags"][k] |= C.QRES_DATAGRAM
            q["res"]["dfid_off"][k], q["res"]["dfid_len"][k] = q["data"].size + len(extra), len(r["dfid"])
            extra += r["dfid"]
    q["data"] = np.concatenate([q["data"], np.frombuffer(extra, np.uint8)])
    q["conn_first"] = b["conn_first"]
    q["stream_id"] = np.array([r.get("stream_id", 4 * k) for k, r in enumerate(rs)], np.uint64)
    q["out_off"] = HE.qpack_session_out_offsets(q["hdr"], q["res"], q["server_len"])
    return q


def fields_of(q, k):
    """response k as the list of fields its section carries"""
    data, R = q["data"].tobytes(), q["res"][k]
    fl = []
    if not R["flags"] & C.QRES_REQUEST:
        fl.append((b":status", b"%d" % (int(R["status"]) & 0xFFFF)))
        if R["flags"] & C.RES_SERVER and q["server_len"]:
            fl.append((b"server", data[q["server_off"]:q["server_off"] + q["server_len"]]))
        if R["content_length"] != M.NONE64:
            fl.append((b"content-length", b"%d" % int(R["content_length"])))
    for h in q["hdr"][int(R["hdr_first"]):int(R["hdr_first"]) + int(R["nhdr"])]:
        fl.append((data[h["name_off"]:int(h["name_off"]) + int(h["name_len"])],
                   data[h["value_off"]:int(h["value_off"]) + int(h["value_len"])]))
    if R["flags"] & C.QRES_DATAGRAM:
        fl.append((b"datagram-flow-id", data[R["dfid_off"]:int(R["dfid_off"]) + int(R["dfid_len"])]))
    return fl


def section_of(frame):
    assert frame[0] == 1
    n = 1 << (frame[1] >> 6)
    v = int.from_bytes(frame[1:1 + n], "big") & ((1 << (8 * n - 2)) - 1)
    assert len(frame) == 1 + n + v
    return frame[1 + n:]


def decoder_input(q, frames, encs):
    """a decoder step: the sections packed back to back, then the encoder streams"""
    secs = [section_of(f) for f in frames]
    sec_off = np.concatenate([[0], np.cumsum([len(s) for s in secs])]).astype(np.uint32)
    enc_len = np.array([len(e) for e in encs], np.uint32)
    enc_off = (int(sec_off[-1]) + np.concatenate([[0], np.cumsum(enc_len)[:-1]])).astype(np.uint32)
    data = np.frombuffer(b"".join(secs) + b"".join(encs) + b"\0", np.uint8)
    arena_off = np.concatenate([[0], np.cumsum([8 * len(s) + 4096 + sum(len(n) + len(v) for n, v in fields_of(q, k))
                                                for k, s in enumerate(secs)])]).astype(np.uint64)
    return dict(data=data, enc_off=enc_off, enc_len=enc_len, sec_off=sec_off, arena_off=arena_off)


def decoded_fields(d, sec_off, k):
    a = d["arena"]
    return [(a[int(d["name_off"][f]):int(d["name_off"][f]) + int(d["name_len"][f])].tobytes(),
             a[int(d["value_off"][f]):int(d["value_off"][f]) + int(d["value_len"][f])].tobytes())
            for f in range(int(sec_off[k]), int(sec_off[k]) + int(d["nfields"][k]))]


def acks_of(d, q, requests):
    rec = d["req" if requests else "res"]
    return [bytes(rec["ack"][k][:int(rec["ack_len"][k])]) for k in range(q["res"].size)]


def per_conn(q, parts):
    cf = q["conn_first"]
    return [b"".join(parts[int(cf[c]):int(cf[c + 1])]) for c in range(cf.size - 1)]


def cpu_decoder(codec, nconn, H, max_blocked, requests):
    from oracle import oracle as O

    sess = O.QpackSession(codec, nconn, H, max_blocked)

    def step(q, frames, encs):
        di = decoder_input(q, frames, encs)
        d = sess.step(di["data"], di["enc_off"], di["enc_len"], di["sec_off"], q["conn_first"], di["arena_off"],
                      stream_id=q["stream_id"], responses=not requests)
        d["sec_off"] = di["sec_off"]
        return d
    return step


def closed_loop(steps, encode, decode, requests):
    """encode(s, q, dec) -> model-shaped result; decode(q, frames, encs) -> decoder dict.  Every step: the encoder
    streams are consumed whole, every section decodes to its response, a section is acknowledged exactly when the
    encoder made it inflight; the acknowledgments are the next step's decoder stream.  -> per step (q, r, d)"""
    dec, count, log = None, None, []
    for s, q in enumerate(steps):
        r = encode(s, q, dec)
        n, nconn = q["res"].size, q["conn_first"].size - 1
        assert (r["rstatus"][:n] == 0).all() and (r["dec_status"][:nconn] == 0).all()
        if dec is not None:
            np.testing.assert_array_equal(r["dec_consumed"][:nconn], [len(x) for x in dec])
        d = decode(q, r["frames"], r["enc"])
        assert (d["enc_status"][:nconn] == 0).all()
        np.testing.assert_array_equal(d["enc_consumed"][:nconn], r["enc_out_len"][:nconn])
        assert (d["sstatus"][:n] == 0).all(), np.flatnonzero(d["sstatus"][:n])[:8]
        for k in range(n):
            assert decoded_fields(d, d["sec_off"], k) == fields_of(q, k), (s, k)
        if "count" in r:  # the new Insert Count, 0 when the step inserted nothing
            prev = np.zeros(nconn, np.int64) if count is None else count
            count = np.asarray(r["count"], np.int64)
            np.testing.assert_array_equal(d["insert_count"][:nconn].astype(np.int64), np.where(count != prev, count, 0))
        acks = acks_of(d, q, requests)
        np.testing.assert_array_equal([len(a) > 0 for a in acks], r["inflight"][:n])
        dec = per_conn(q, acks)
        log.append((q, r, d))
    return log


def model_encoder(m, first_flags=C.QENC_SET_CAPACITY):
    def encode(s, q, dec):
        r = m.step(q, dec, flags=C.QENC_CONTINUE if s else first_flags)
        r["count"] = np.array([len(c.ent) for c in m.conns])
        return r
    return encode


def sessions(nconn, steps, seed, requests=False):
    if requests:
        b = HE.make_request_session(nconn, seed=seed, req_per_conn=(steps, 2 * steps), big_frac=0.0, frame_frac=0.0)[0]
    else:
        b = HE.make_session(nconn, seed=seed, resp_per_conn=(steps, 2 * steps), big_frac=0.0, trailers_frac=0.0,
                            dont_compress_frac=0.05)[0]
    return HE.to_qpack_sessions(b, steps, seed=seed, requests=requests, dfid_frac=0.1, odd_status_frac=0.0)


# ---------------------------------------------------------------------------------------------------
# CPU 1: the model against the decoders
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("requests,steps,seed", [(False, 4, 61), (False, 3, 62), (True, 3, 63)])
def test_model_round_trip_restatement(oracle_codec, requests, steps, seed):
    from oracle import oracle as O

    st = sessions(200, steps, seed, requests)
    m = M.Model(200, 4096, 100)
    log = closed_loop(st, model_encoder(m), cpu_decoder(O.oracle(), 200, 4096, 100, requests), requests)
    assert sum(int(r["inflight"].sum()) for _, r, _ in log) > 200  # the dynamic table is in use
    assert any(len(e) > 3 for _, r, _ in log[1:] for e in r["enc"])


@pytest.mark.parametrize("requests,steps,seed", [(False, 4, 61), (True, 3, 63)])
def test_model_round_trip_reference(oracle_codec, requests, steps, seed):
    from oracle import oracle as O

    if not O.ref_available():
        pytest.skip("oracle/_ref not built (needs /root/reference)")
    st = sessions(200, steps, seed, requests)
    closed_loop(st, model_encoder(M.Model(200, 4096, 100)), cpu_decoder(O.ref(), 200, 4096, 100, requests), requests)


# ---------------------------------------------------------------------------------------------------
# CPU 2: the pinned bytes of the static path
# ---------------------------------------------------------------------------------------------------
def golden_static(name):
    g = load_golden("qpenc")
    p = name + "_"
    q = {k[len(p):]: v for k, v in g.items() if k.startswith(p)}
    q["hdr"] = q["hdr"].view(C.HPE_HEADER_DTYPE)
    q["res"] = q["res"].view(C.QPE_RESPONSE_DTYPE).copy()
    q["server_off"], q["server_len"] = (int(x) for x in q["server"])
    n = q["res"].size
    q["res"]["flags"] |= NOENC
    q["conn_first"] = np.arange(n + 1, dtype=np.uint32)  # every response on a connection of its own
    q["stream_id"] = np.zeros(n, np.uint64)
    return q


@pytest.mark.parametrize("name", ["q1", "qedge", "qrq"])
def test_model_static_path_is_the_pinned_bytes(oracle_codec, name):
    from oracle import oracle as O

    q = golden_static(name)
    n = q["res"].size
    w = O.qpe_step(O.oracle(), q["data"], q["hdr"], q["res"], q["out_off"], q["server_off"], q["server_len"])
    r = M.Model(n).step(q)
    np.testing.assert_array_equal(r["rstatus"], w["rstatus"][:n])
    np.testing.assert_array_equal(r["out_len"], w["out_len"][:n])
    np.testing.assert_array_equal(r["header_len"], w["header_len"][:n])
    for k in range(n):
        assert r["frames"][k] == w["out"][int(q["out_off"][k]):int(q["out_off"][k]) + int(w["out_len"][k])].tobytes(), k
    assert all(e == b"" for e in r["enc"]) and not r["inflight"].any()
    wf = q["frames"].tobytes()  # and the reference's own bytes, as the fixture holds them
    assert b"".join(r["frames"]) == wf


# ---------------------------------------------------------------------------------------------------
# CPU 3: the reference's unit test with an encoder stream (t/00unit/lib/http3/qpack.c:59-112)
# ---------------------------------------------------------------------------------------------------
def unit_request():
    own = [(b":method", b"GET", T), (b":scheme", b"https", T), (b":authority", b"example.com", LTR), (b":path", b"/foobar", T)]
    return batch([[dict(status=4, stream_id=123, headers=own + [(b"dnt", b"1", 0), (b"x-hoge", b"A", 0)])]], requests=True)


def check_unit(codec):
    q = unit_request()
    m = M.Model(1, 4096, 100)
    r = m.step(q)
    assert len(r["enc"][0]) > 0 and r["inflight"][0]
    d = cpu_decoder(codec, 1, 4096, 100, True)(q, r["frames"], r["enc"])
    assert d["enc_status"][0] == 0 and d["enc_consumed"][0] == len(r["enc"][0])
    assert d["sstatus"][0] == 0 and decoded_fields(d, d["sec_off"], 0) == fields_of(q, 0)
    rq = d["req"][0]
    assert rq["method"] >= 0 and rq["authority"] >= 0 and rq["path"] >= 0 and rq["nheaders"] == 2
    ack = acks_of(d, q, True)[0]
    assert ack == M.encode_int(123, 7, 0x80)
    r2 = m.step(batch([[]]), [ack], flags=C.QENC_CONTINUE)
    assert r2["dec_status"][0] == 0 and r2["dec_consumed"][0] == len(ack)
    assert m.conns[0].inflight == [] and m.conns[0].lkr == 1 and m.conns[0].num_blocked == 0


def test_unit_request_with_encoder_stream(oracle_codec):
    from oracle import oracle as O

    check_unit(O.oracle())
    if O.ref_available():
        check_unit(O.ref())


# ---------------------------------------------------------------------------------------------------
# CPU 4 and 5: edges of the decision and of the decoder stream, as scripts the GPU replays byte for byte
# ---------------------------------------------------------------------------------------------------
V8, V7 = b"12345678", b"1234567"
LONG = (b"</assets/app.%d.js>; rel=preload; as=script, " * 12) % tuple(range(12))  # over kLongStr (256)


def resp(headers, **kw):
    return dict(dict(status=200, headers=headers), **kw)


def edge_scripts():
    """name -> dict(H=, max_blocked=, max_inflight=, steps=[(conns, decoder streams or None)], flags of step 0)"""
    ack = lambda sid: M.encode_int(sid, 7, 0x80)  # noqa: E731
    fill = b"x" * (64 - 32 - len(b"vary"))
    s = {}
    s["value_7_against_8"] = dict(steps=[([[resp([(b"date", V7, LTR)]), resp([(b"date", V8, LTR)])]], None)])
    s["exact_fill"] = dict(H=64, steps=[([[resp([(b"vary", fill, LTR), (b"vary", b"12345678", LTR)])],
                                          [resp([(b"vary", fill + b"y", LTR)])]], None)])
    s["table_0"] = dict(H=0, steps=[([[resp([(b"date", V8, LTR)], flags=C.RES_SERVER)]], None)])
    s["table_64"] = dict(H=64, steps=[([[resp([(b"date", V8, LTR), (b"vary", V8, LTR)])]], None)])
    two = [[resp([(b"date", V8, LTR)], stream_id=0), resp([(b"date", V8, LTR)], stream_id=4)]]
    s["max_blocked_0"] = dict(max_blocked=0, steps=[(two, None), (two, None)])
    s["max_blocked_1"] = dict(max_blocked=1, steps=[(two, None), (two, [ack(0)]), (two, [ack(4) + ack(0)])])
    s["priority_twice"] = dict(steps=[([[resp([(b"priority", b"u=3, i=?0", LTR), (b"priority", b"u=1, i=?1", LTR)])]], None)])
    s["non_token_name"] = dict(steps=[([[resp([(b"priority", V8, LTR), (b"priority", b"u=0", 0)])]], None)])
    s["dont_compress"] = dict(steps=[([[resp([(b"priority", V8, LTR), (b"priority", b"aaaaaaaaaaaaaaaa", T | DC),
                                              (b"date", b"aaaaaaaaaaaa", LTR | DC), (b"x-a", b"aaaaaaaaaaaa", DC),
                                              (b"date", b"bbbbbbbbbbbb", T | DC)]),
                                        resp([(b"priority", b"cccccccccccc", T | DC), (b"date", b"aaaaaaaaaaaa", T)])]], None)])
    s["set_capacity"] = dict(first=C.QENC_SET_CAPACITY, steps=[([[resp([(b"date", V8, LTR)])]], None)])
    s["long_value_inserted"] = dict(steps=[([[resp([(b"link", LONG, LTR)]), resp([(b"link", LONG, LTR)])]], None)])
    s["max_inflight_1"] = dict(max_inflight=1, steps=[(two, None), (two, [ack(0)])])
    s["own_fields"] = dict(steps=[([[resp([(b"date", V8, LTR)], status=999, content_length=12345, flags=C.RES_SERVER,
                                          dfid=b"77"),
                                     resp([], status=999, content_length=0, flags=C.RES_SERVER, dfid=b"77", stream_id=8)]],
                                   None)])
    one = [[resp([(b"date", V8, LTR)], stream_id=0)]]
    later = [[resp([(b"date", V8, LTR)], stream_id=4), resp([], stream_id=8)]]
    for name, stream, status, consumed in [
            ("increment_0", b"\x00", M.DECODER_STREAM, 1), ("increment_past", b"\x02", M.DECODER_STREAM, 1),
            ("ack_unknown", ack(44), M.DECODER_STREAM, 1), ("cancel_unknown", b"\x40" + bytes([0x40 | 7]), 0, 2),
            ("cut_mid_integer", ack(0) + b"\xff\x80", 0, 1), ("increment_1", b"\x01", 0, 1),
            ("cancel_inflight", b"\x40", 0, 1),
            ("integer_overflow", b"\x3f" + b"\xff" * 9, M.DECOMPRESSION_FAILED, 0)]:
        s["dec_" + name] = dict(steps=[(one, None), (later, [stream]), (later, [b""])], dec=(status, consumed))
    return s


def run_script(sc, encode_step):
    """-> the results of every step; encode_step(s, q, dec, flags, sc) -> model-shaped result"""
    out = []
    for k, (conns, dec) in enumerate(sc["steps"]):
        out.append(encode_step(k, batch(conns), dec, C.QENC_CONTINUE if k else sc.get("first", 0)))
    return out


def model_script(sc):
    n = len(sc["steps"][0][0])
    m = M.Model(n, sc.get("H", 4096), sc.get("max_blocked", 100), sc.get("max_inflight", 64))
    return m, run_script(sc, lambda k, q, dec, flags: m.step(q, dec, flags))


def body(frame):
    """a frame's field lines: the section without its two-byte prefix (Required Insert Count below 254 here)"""
    return section_of(frame)[2:]


def test_edge_value_length_8_under_a_static_name(oracle_codec):
    m, (r,) = model_script(edge_scripts()["value_7_against_8"])
    assert r["enc"][0] == bytes([0xC0 | 6]) + M.qstring(V8)  # only the 8-byte value is inserted
    assert body(r["frames"][0])[1:] == bytes([0x50 | 6]) + M.qstring(V7)
    assert body(r["frames"][1])[1:] == bytes([0x10])


def test_edge_exact_fill_and_one_byte_over(oracle_codec):
    m, (r,) = model_script(edge_scripts()["exact_fill"])
    assert m.conns[0].used == 64 and len(m.conns[0].ent) == 1 and m.conns[1].used == 0
    assert r["enc"][1] == b"" and not r["inflight"][1]


def test_edge_table_sizes_0_and_64(oracle_codec):
    m, (r,) = model_script(edge_scripts()["table_0"])
    assert r["enc"][0] == b"" and section_of(r["frames"][0])[:2] == b"\0\0"
    m, (r,) = model_script(edge_scripts()["table_64"])
    assert len(m.conns[0].ent) == 1 and m.conns[0].ent[0][0] == b"date"


def test_edge_max_blocked_0_never_inserts(oracle_codec):
    m, rs = model_script(edge_scripts()["max_blocked_0"])
    assert all(r["enc"][0] == b"" and not r["inflight"].any() for r in rs) and m.conns[0].ent == []


def test_edge_max_blocked_1_second_section_has_no_buffer(oracle_codec):
    m, rs = model_script(edge_scripts()["max_blocked_1"])
    assert list(rs[0]["blocking"]) == [True, False] and list(rs[0]["inflight"]) == [True, False]
    assert body(rs[0]["frames"][1])[1:] == bytes([0x50 | 6]) + M.qstring(V8)  # entry 1 is not acknowledged yet
    assert list(rs[1]["inflight"]) == [True, True] and not rs[1]["blocking"].any()  # acknowledged: pre-base references
    assert body(rs[1]["frames"][0])[1:] == bytes([0x80])


def test_edge_dynamic_name_reference_insert_decodes(oracle_codec):
    """priority twice with two values of 8 bytes or more: the second insert names the first entry -- the case the
    reference's own encoder gets wrong (absolute index, qpack.c:1177) and its decoder rejects"""
    from oracle import oracle as O

    sc = edge_scripts()["priority_twice"]
    m, (r,) = model_script(sc)
    first = M.qstring(b"priority", 5, 0x40) + M.qstring(b"u=3, i=?0")
    assert r["enc"][0] == first + bytes([0x80 | 0]) + M.qstring(b"u=1, i=?1")
    q = batch(sc["steps"][0][0])
    for codec in [O.oracle()] + ([O.ref()] if O.ref_available() else []):
        d = cpu_decoder(codec, 1, 4096, 100, False)(q, r["frames"], r["enc"])
        assert d["enc_status"][0] == 0 and d["sstatus"][0] == 0 and d["insert_count"][0] == 2
        assert decoded_fields(d, d["sec_off"], 0) == fields_of(q, 0)


def test_edge_non_token_header_takes_the_dynamic_name_reference(oracle_codec):
    m, (r,) = model_script(edge_scripts()["non_token_name"])
    assert body(r["frames"][0])[2:] == bytes([0x00]) + M.qstring(b"u=0")  # post-base name reference 0


def test_edge_dont_compress_bits(oracle_codec):
    m, (r,) = model_script(edge_scripts()["dont_compress"])
    raw = lambda v: M.qstring(v, force_raw=True)  # noqa: E731
    b0 = body(r["frames"][0])[1:]
    want = bytes([0x10]) + bytes([0x08 | 0]) + raw(b"aaaaaaaaaaaaaaaa") + bytes([0x11])  # the insert ignores the flag
    want += M.qstring(b"x-a", 3, 0x30) + raw(b"aaaaaaaaaaaa") + bytes([0x70 | 6]) + raw(b"bbbbbbbbbbbb")
    assert b0 == want
    assert body(r["frames"][1])[1:] == bytes([0x60 | 1]) + raw(b"cccccccccccc") + bytes([0x80 | 0])


def test_edge_set_capacity_is_accepted(oracle_codec):
    from oracle import oracle as O

    sc = edge_scripts()["set_capacity"]
    m, (r,) = model_script(sc)
    assert r["enc"][0][:3] == M.encode_int(4096, 5, 0x20)
    q = batch(sc["steps"][0][0])
    for codec in [O.oracle()] + ([O.ref()] if O.ref_available() else []):
        d = cpu_decoder(codec, 1, 4096, 100, False)(q, r["frames"], r["enc"])
        assert d["enc_status"][0] == 0 and d["enc_consumed"][0] == len(r["enc"][0]) and d["sstatus"][0] == 0


def test_edge_inflight_list_full_falls_back(oracle_codec):
    m, rs = model_script(edge_scripts()["max_inflight_1"])
    assert list(rs[0]["rflags"]) == [0, 1] and list(rs[0]["rstatus"]) == [0, 0]
    assert section_of(rs[0]["frames"][1])[:2] == b"\0\0" and len(m.conns[0].inflight) == 1


def test_edge_own_fields_use_the_table(oracle_codec):
    """server is inserted (likely to repeat) and referenced by the next response; :status, content-length and
    datagram-flow-id never are"""
    m, (r,) = model_script(edge_scripts()["own_fields"])
    assert [n for n, _ in m.conns[0].ent] == [b"server", b"date"]
    assert bytes([0x80 | 1]) in body(r["frames"][1])[:12]


@pytest.mark.parametrize("name", ["increment_0", "increment_past", "ack_unknown", "cancel_unknown", "cut_mid_integer",
                                  "increment_1", "cancel_inflight", "integer_overflow"])
def test_decoder_stream_on_the_model(oracle_codec, name):
    sc = edge_scripts()["dec_" + name]
    m, rs = model_script(sc)
    status, consumed = sc["dec"]
    assert rs[1]["dec_status"][0] == status and rs[1]["dec_consumed"][0] == consumed
    if status:  # this step's and every later response of the connection are skipped
        assert (rs[1]["rstatus"] == C.RES_SKIPPED).all() and (rs[2]["rstatus"] == C.RES_SKIPPED).all()
        assert rs[2]["dec_status"][0] == M.SKIPPED and all(f == b"" for f in rs[1]["frames"] + rs[2]["frames"])
    else:
        assert (rs[1]["rstatus"] == 0).all() and (rs[2]["rstatus"] == 0).all()
    if name == "cut_mid_integer":
        assert m.conns[0].lkr == 1
    if name == "cancel_inflight":
        assert m.conns[0].lkr == 0 and [e[0] for e in m.conns[0].inflight] == [4, 4]


def test_size_property_second_response_is_shorter(oracle_codec):
    """a likely-to-repeat token header with a value of 8 bytes or more, sent twice on a connection: the second
    section is strictly shorter than the static-only section of the same response"""
    hs = [(b"cache-control", b"public, max-age=86400", LTR), (b"content-type", b"image/webp", LTR)]
    conns = [[resp(hs, stream_id=0), resp(hs, stream_id=4)]]
    r = M.Model(1).step(batch(conns))
    static = M.Model(1).step(batch([[dict(x, flags=NOENC) for x in conns[0]]]))
    assert static["header_len"][0] == static["header_len"][1]
    assert r["header_len"][1] < static["header_len"][1]


# ---------------------------------------------------------------------------------------------------
# CPU 6: exports (the library is cross-compiled where there is no GPU; nothing here touches one)
# ---------------------------------------------------------------------------------------------------
def test_exports_and_host_only_checks():
    from h2o_amd import build

    build.build(verbose=False)
    L = C.lib()  # (loads torch's HIP runtime first: one runtime per process)
    size, call = L.hhuff_qpack_enc_scratch_size, L.hhuff_qpack_flatten_sessions
    assert size(0, 4096, 64) == 0
    assert size(3, 4096, 64) == 3 * size(1, 4096, 64) and size(1, 4096, 64) >= 2 * 4096 + 16 * 64
    assert size(1, 4096, 65) - size(1, 4096, 64) == 16 and size(1, 4096, 64) % 16 == 0
    nul = [None] * 12
    assert call(None, 0, None, 0, None, None, 1, 0, None, None, None, 65537, 100, 64, 0, 0, *nul, 0, 0, None) == C.RES_EINVAL
    assert call(None, 0, None, 0, None, None, 0, 0, None, None, None, 4096, 100, 64, 0, 0, *nul, 0, 0, None) == 0
    assert call(None, 0, None, 0, None, None, 1, 0, None, None, None, 4096, 100, 64, 0, 0, *nul, 0, 0, None) == -1  # NULL arrays
    assert os.path.exists(C.LIB_PATH)


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


class Gpu:
    """hhuff_qpack_flatten_sessions step after step, the sessions carried in scratch"""

    def __init__(self, torch, nconn, H=4096, max_blocked=100, max_inflight=64, move=False, enc_room=None):
        self.t, self.nconn, self.H, self.mb, self.mi, self.move = torch, nconn, H, max_blocked, max_inflight, move
        self.scratch, self.enc_room = None, enc_room

    def step(self, q, dec=None, flags=0, guard=64):
        torch = self.t
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()  # noqa: E731
        u32 = lambda a: dev(np.asarray(a, np.uint32).view(np.int32))  # noqa: E731
        data, in_size = q["data"], q.get("in_size")
        dec_off = dec_len = None
        if dec is not None:
            lens = np.array([len(x) for x in dec], np.uint32)
            offs = q.get("dec_off", data.size + np.concatenate([[0], np.cumsum(lens)[:-1]]))
            data = np.concatenate([data, np.frombuffer(b"".join(dec), np.uint8)])
            dec_off, dec_len = u32(offs), u32(q.get("dec_len", lens))
        in_size = int(data.size) if in_size is None else in_size
        data = np.concatenate([data, np.zeros(4, np.uint8)])
        n, nconn = q["res"].size, self.nconn
        room = (self.H + 4 + 15) // 16 * 16 if self.enc_room is None else self.enc_room
        eoff = q.get("enc_out_off", np.arange(nconn + 1, dtype=np.uint64) * room)
        # sentinels around out and enc_out: the call works on the inner part of a larger buffer
        out_size, enc_size = max(1, int(np.max(q["out_off"]))), max(1, int(np.max(eoff)))
        out = torch.full((guard + out_size + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        enc = torch.full((guard + enc_size + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        hdr = dev(q["hdr"].view(np.uint8)) if q["hdr"].size else torch.zeros(0, dtype=torch.uint8, device="cuda")
        if self.move and self.scratch is not None:
            moved = torch.empty_like(self.scratch)
            moved.copy_(self.scratch)
            self.scratch.fill_(0x5A)  # stays allocated: a stale address would read this
            self.old, self.scratch = self.scratch, moved
        if "scratch_size" in q:
            self.scratch = torch.empty(max(16, q["scratch_size"]), dtype=torch.uint8, device="cuda")
        r = C.qpack_flatten_sessions(
            dev(data), hdr, dev(q["res"].view(np.uint8)) if n else torch.zeros(32, dtype=torch.uint8, device="cuda"),
            u32(q["conn_first"]), n, dev(q["stream_id"].view(np.int64)) if n else torch.zeros(1, dtype=torch.int64, device="cuda"),
            dev(np.asarray(q["out_off"], np.uint64).view(np.int64)), dec_off, dec_len, self.H, self.mb, self.mi,
            q["server_off"], q["server_len"], enc_out_off=dev(np.asarray(eoff, np.uint64).view(np.int64)), in_size=in_size,
            out=out[guard:guard + out_size], enc_out=enc[guard:guard + enc_size], scratch=self.scratch,
            cont=bool(flags & C.QENC_CONTINUE), set_capacity=bool(flags & C.QENC_SET_CAPACITY))
        torch.cuda.synchronize()
        self.scratch = r["scratch"]
        h = {k: r[k].cpu().numpy() for k in ("out_len", "header_len", "rstatus", "rflags", "enc_out_len", "dec_status",
                                              "dec_consumed")}
        for k in ("out_len", "header_len", "enc_out_len", "dec_consumed"):
            h[k] = h[k].view(np.uint32)
        h = {k: v[:(nconn if k in ("enc_out_len", "dec_status", "dec_consumed") else n)] for k, v in h.items()}
        o, e = out.cpu().numpy(), enc.cpu().numpy()
        h["guards_intact"] = bool((o[:guard] == 0xA5).all() and (o[guard + out_size:] == 0xA5).all() and
                                  (e[:guard] == 0xA5).all() and (e[guard + enc_size:] == 0xA5).all())
        h["out_raw"], h["enc_raw"] = o[guard:guard + out_size], e[guard:guard + enc_size]
        h["frames"] = [o[guard + int(a):guard + int(a) + int(L)].tobytes() for a, L in zip(q["out_off"], h["out_len"])]
        h["enc"] = [e[guard + int(a):guard + int(a) + int(L)].tobytes() for a, L in zip(eoff, h["enc_out_len"])]
        return h


def same(g, w, what=""):
    """the GPU's step g against the model's w: every output"""
    for k in ("rstatus", "rflags", "out_len", "header_len", "enc_out_len", "dec_status", "dec_consumed"):
        np.testing.assert_array_equal(np.asarray(g[k]).astype(np.int64), np.asarray(w[k]).astype(np.int64), err_msg=what + k)
    bad = [k for k in range(len(w["frames"])) if g["frames"][k] != w["frames"][k]]
    assert not bad, "%s%d frames differ; first %d: got %s want %s" % (what, len(bad), bad[0], g["frames"][bad[0]][:64].hex(),
                                                                      w["frames"][bad[0]][:64].hex())
    bad = [c for c in range(len(w["enc"])) if g["enc"][c] != w["enc"][c]]
    assert not bad, "%s%d encoder streams differ; first %d: got %s want %s" % (what, len(bad), bad[0], g["enc"][bad[0]][:64].hex(),
                                                                               w["enc"][bad[0]][:64].hex())
    assert g["guards_intact"]


@pytest.mark.gpu
def test_gpu_one_response(torch_cuda):
    q = batch([[resp([(b"date", V8, LTR), (b"x-a", b"b", 0)], flags=C.RES_SERVER, content_length=7)]])
    same(Gpu(torch_cuda, 1).step(q), M.Model(1).step(q))


@pytest.mark.gpu
def test_gpu_65_connections(torch_cuda):
    """one past a 64-lane block; a header range no response lists"""
    st = sessions(65, 2, 71)
    q = dict(st[0])
    q["hdr"] = np.concatenate([q["hdr"], q["hdr"][:3]])  # three headers behind every range
    m, g = M.Model(65), Gpu(torch_cuda, 65)
    same(g.step(q, flags=C.QENC_SET_CAPACITY), m.step(q, flags=C.QENC_SET_CAPACITY))
    q1 = dict(st[1], hdr=q["hdr"])
    same(g.step(q1, flags=C.QENC_CONTINUE), m.step(q1, flags=C.QENC_CONTINUE))


@pytest.mark.gpu
@pytest.mark.parametrize("requests,move", [(False, False), (False, True), (True, False)])
def test_gpu_300_connections_3_steps(torch_cuda, oracle_codec, requests, move):
    """bytes against the model with HHUFF_QENC_CONTINUE, the acknowledgments of the decoder restatement fed
    back; move: the scratch is copied to a new allocation between the steps"""
    from oracle import oracle as O

    st = sessions(300, 3, 72 + requests, requests)
    m, g = M.Model(300), Gpu(torch_cuda, 300, move=move)
    enc_m = model_encoder(m)

    def encode(s, q, dec):
        w = enc_m(s, q, dec)
        same(g.step(q, dec, flags=C.QENC_CONTINUE if s else C.QENC_SET_CAPACITY), w, "step %d: " % s)
        return w
    closed_loop(st, encode, cpu_decoder(O.oracle(), 300, 4096, 100, requests), requests)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(edge_scripts()))
def test_gpu_edges(torch_cuda, name):
    sc = edge_scripts()[name]
    m, want = model_script(sc)
    g = Gpu(torch_cuda, len(sc["steps"][0][0]), sc.get("H", 4096), sc.get("max_blocked", 100), sc.get("max_inflight", 64))
    got = run_script(sc, lambda k, q, dec, flags: g.step(q, dec, flags))
    for k, (a, b) in enumerate(zip(got, want)):
        same(a, b, "%s step %d: " % (name, k))


def gpu_decoder(torch, nconn, H, max_blocked, requests):
    state = dict(scratch=None)

    def step(q, frames, encs):
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()  # noqa: E731
        u32 = lambda a: dev(np.asarray(a, np.uint32).view(np.int32))  # noqa: E731
        di = decoder_input(q, frames, encs)
        n = q["res"].size
        r = C.qpack_decode(dev(di["data"]), u32(di["enc_off"]), u32(di["enc_len"]), u32(di["sec_off"]), u32(q["conn_first"]),
                           n, H, max_blocked, arena_off=dev(di["arena_off"].view(np.int64)), in_size=int(di["data"].size) - 1,
                           scratch=state["scratch"], cont=state["scratch"] is not None,
                           stream_id=dev(q["stream_id"].view(np.int64)), responses=not requests)
        torch.cuda.synchronize()
        state["scratch"] = r.pop("scratch")
        from oracle import oracle as O

        d = {k: v.cpu().numpy() for k, v in r.items()}
        for k in ("name_off", "name_len", "value_off", "value_len", "nfields", "enc_consumed"):
            d[k] = d[k].view(np.uint32)
        d["insert_count"] = d["insert_count"].view(np.uint64)
        if requests:
            d["req"] = d["req"].reshape(-1).view(O.QREQ_DTYPE)
        else:
            d["res"] = d["res"].reshape(-1).view(O.QRES_DTYPE)
        d["sec_off"] = di["sec_off"]
        return d
    return step


def gpu_encoder(g):
    def encode(s, q, dec):
        return g.step(q, dec, flags=C.QENC_CONTINUE if s else C.QENC_SET_CAPACITY)
    return encode


def section_lines(sec):
    """-> (Required Insert Count as written, the field lines' kinds): "static", "pre" / "post" (indexed), "sname",
    "pre-name" / "post-name" (name references), "literal" """
    def string(p, prefix):
        n, p = M.decode_int(sec, p, prefix)
        return p + n
    ric, p = M.decode_int(sec, 0, 8)
    _, p = M.decode_int(sec, p, 7)
    kinds = []
    while p < len(sec):
        b = sec[p]
        if b & 0x80:
            kinds.append("static" if b & 0x40 else "pre")
            p = M.decode_int(sec, p, 6)[1]
        elif b & 0x40:
            kinds.append("sname" if b & 0x10 else "pre-name")
            p = string(M.decode_int(sec, p, 4)[1], 7)
        elif b & 0x20:
            kinds.append("literal")
            p = string(string(p, 3), 7)
        elif b & 0x10:
            kinds.append("post")
            p = M.decode_int(sec, p, 4)[1]
        else:
            kinds.append("post-name")
            p = string(M.decode_int(sec, p, 3)[1], 7)
    assert p == len(sec)
    return ric, kinds


def loop_sessions(nconn, steps, requests):
    """per connection and step: a response with the connection's own repeating headers and a new date (an insert:
    post-base), then one with the repeating headers alone (from step 2 on: pre-base references only)"""
    out = []
    for s in range(steps):
        conns = []
        for c in range(nconn):
            if requests:
                own = [(b":method", b"GET", T), (b":scheme", b"https", T), (b":authority", b"host-%d.example.com" % c, LTR),
                       (b":path", b"/p/%d/%d" % (c, s), T)]
                rep = own + [(b"user-agent", b"agent/%d.0 (conn %d)" % (c % 7, c), LTR), (b"x-trace", b"%d-%d" % (c, s), 0)]
                new = rep + [(b"referer", b"https://host-%d.example.com/from/%d" % (c, s), LTR)]
                rs = [dict(status=4, headers=new, stream_id=8 * s), dict(status=4, headers=rep, stream_id=8 * s + 4)]
            else:
                rep = [(b"cache-control", b"max-age=%d, private" % (1000 + c), LTR), (b"content-type", b"text/x-conn-%d" % c, LTR),
                       (b"etag", b'"%d-%d"' % (c, s), T)]
                new = rep + [(b"date", HE._date(86400 * c + s), LTR)]
                rs = [resp(new, flags=C.RES_SERVER, content_length=100 + c, stream_id=8 * s),
                      resp(rep, flags=C.RES_SERVER, status=404, stream_id=8 * s + 4, dfid=b"%d" % c if c % 9 == 0 else None)]
            conns.append(rs)
        out.append(batch(conns, requests=requests))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("requests", [False, True])
def test_gpu_closed_loop(torch_cuda, requests):
    """GPU encoder -> GPU decoder -> the acknowledgments back into the GPU encoder, 3 steps x 200 connections:
    every field comes back; from step 2 on every connection has a section with a pre-base dynamic reference
    whose Required Insert Count the decoder had reached before the step"""
    st = loop_sessions(200, 3, requests)
    g = Gpu(torch_cuda, 200)
    m = M.Model(200)  # says which sections became inflight: the loop's check of the acknowledgments
    enc_g = gpu_encoder(g)

    def encode(s, q, dec):
        r = enc_g(s, q, dec)
        w = m.step(q, dec, flags=C.QENC_CONTINUE if s else C.QENC_SET_CAPACITY)
        r["inflight"] = w["inflight"]
        return r
    log = closed_loop(st, encode, gpu_decoder(torch_cuda, 200, 4096, 100, requests), requests)
    reached = np.zeros(200, np.int64)
    for s, (q, r, d) in enumerate(log):
        cf = q["conn_first"]
        for c in range(200 if s >= 1 else 0):
            lines = [section_lines(section_of(r["frames"][k])) for k in range(int(cf[c]), int(cf[c + 1]))]
            assert any(0 < ric - 1 <= reached[c] and ("pre" in kinds or "pre-name" in kinds) for ric, kinds in lines), (s, c)
        ic = d["insert_count"][:200].astype(np.int64)
        reached = np.where(ic > 0, ic, reached)


@pytest.mark.gpu
def test_gpu_withheld_encoder_stream_blocks(torch_cuda):
    """the decoder does not get a step's encoder stream: exactly the sections the encoder marked blocking are
    HHUFF_QPK_BLOCKED"""
    st = sessions(200, 2, 83)
    g, m = Gpu(torch_cuda, 200), M.Model(200)
    dec = gpu_decoder(torch_cuda, 200, 4096, 100, False)
    r0, w0 = g.step(st[0]), m.step(st[0])
    d0 = dec(st[0], r0["frames"], r0["enc"])
    assert (d0["sstatus"][:st[0]["res"].size] == 0).all()
    acks = per_conn(st[0], acks_of(d0, st[0], False))
    r1, w1 = g.step(st[1], acks, flags=C.QENC_CONTINUE), m.step(st[1], acks, flags=C.QENC_CONTINUE)
    same(r1, w1)
    assert w1["blocking"].any() and not w1["blocking"].all()
    d1 = dec(st[1], r1["frames"], [b""] * 200)
    n = st[1]["res"].size
    np.testing.assert_array_equal(d1["sstatus"][:n] == C.QPK_BLOCKED, w1["blocking"])
    assert (d1["sstatus"][:n][~w1["blocking"]] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["q1", "qedge", "qrq"])
def test_gpu_static_path_unchanged(torch_cuda, name):
    """HHUFF_QRES_NO_ENCODER_STREAM everywhere: the frames of hhuff_qpack_flatten_responses"""
    q = golden_static(name)
    n = q["res"].size
    g = Gpu(torch_cuda, n).step(q)
    dev = lambda a: torch_cuda.from_numpy(np.ascontiguousarray(a).copy()).cuda()  # noqa: E731
    res = q["res"].copy()
    res["flags"] &= ~np.uint32(NOENC)
    s = C.qpack_flatten_responses(dev(np.concatenate([q["data"], np.zeros(4, np.uint8)])), dev(q["hdr"].view(np.uint8)),
                                  dev(res.view(np.uint8)), n, dev(q["out_off"].view(np.int64)), q["server_off"],
                                  q["server_len"], in_size=int(q["data"].size))
    torch_cuda.cuda.synchronize()
    out, out_len = s["out"].cpu().numpy(), s["out_len"].cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(g["rstatus"], s["rstatus"].cpu().numpy()[:n])
    np.testing.assert_array_equal(g["out_len"], out_len[:n])
    np.testing.assert_array_equal(g["header_len"], s["header_len"].cpu().numpy().view(np.uint32)[:n])
    for k in range(n):
        assert g["frames"][k] == out[int(q["out_off"][k]):int(q["out_off"][k]) + int(out_len[k])].tobytes(), k
    assert (g["enc_out_len"] == 0).all() and g["guards_intact"]
    assert b"".join(g["frames"]) == q["frames"].tobytes()


def malformed_base():
    return batch([[resp([(b"date", V8, LTR)], flags=C.RES_SERVER), resp([(b"vary", V8, LTR)], stream_id=4)],
                  [resp([(b"x-a", b"1", 0)], stream_id=8)]])


@pytest.mark.gpu
def test_gpu_malformed_strings_past_in_size(torch_cuda):
    q = malformed_base()
    q["in_size"] = int(q["hdr"]["value_off"][0]) + 3  # every string from the first header's value on is cut
    g = Gpu(torch_cuda, 2).step(q)
    assert list(g["rstatus"]) == [C.RES_EINVAL] * 3 and (g["out_len"] == 0).all() and (g["enc_out_len"] == 0).all()
    assert (g["out_raw"] == 0xA5).all() and (g["enc_raw"] == 0xA5).all() and g["guards_intact"]


@pytest.mark.gpu
def test_gpu_malformed_decoder_stream_range(torch_cuda):
    q = malformed_base()
    q["dec_off"], q["dec_len"] = np.array([0, 0xFFFFFFF0], np.uint32), np.array([0, 0x20], np.uint32)
    g = Gpu(torch_cuda, 2).step(q, [b"", b""])
    assert list(g["rstatus"]) == [0, 0, C.RES_SKIPPED] and list(g["dec_status"]) == [0, C.RES_EINVAL]
    assert g["out_len"][2] == 0 and g["enc_out_len"][1] == 0 and g["guards_intact"]
    o2 = int(q["out_off"][2])
    assert (g["out_raw"][o2:] == 0xA5).all()


@pytest.mark.gpu
def test_gpu_malformed_out_off(torch_cuda):
    q = malformed_base()
    q["out_off"] = q["out_off"].copy()
    q["out_off"][2] = q["out_off"][1] - 1  # response 1's region ends before it starts; response 2's is larger
    g, w = Gpu(torch_cuda, 2).step(q), M.Model(2).step(q)
    assert list(g["rstatus"]) == [0, C.RES_EINVAL, 0] and g["out_len"][1] == 0
    same(g, w)


@pytest.mark.gpu
def test_gpu_scratch_too_small_and_small_regions(torch_cuda):
    q = malformed_base()
    q["scratch_size"] = C.qpack_enc_scratch_size(2) - 16
    with pytest.raises(C.HhuffError):
        Gpu(torch_cuda, 2).step(q)
    q = malformed_base()  # an encoder-stream region of 8 bytes: the inserts do not fit; the frames' regions too small
    g, w = Gpu(torch_cuda, 2, enc_room=16), M.Model(2)
    q["enc_out_off"] = np.array([0, 8, 16], np.uint64)
    same(g.step(q), w.step(q))
    q2 = malformed_base()
    q2["out_off"] = np.concatenate([[0], np.cumsum([5, 200, 3])]).astype(np.uint64)
    g2, w2 = Gpu(torch_cuda, 2).step(q2), M.Model(2).step(q2)
    assert list(g2["rstatus"]) == [C.RES_SPACE, 0, C.RES_SPACE]
    same(g2, w2)
