"""Connection slots (include/hhuff.h (2h)), the part that needs no GPU: the test helper that cuts dense sessions
into sparse steps (tests/slots_plan.py) round-trips; the restatement's sessions confirm what the GPU tests lean on
-- a connection's results depend on its own history, not on its place in the call; the header compiles as C99 and
C++17; the library exports the eight _slots symbols.  The GPU side is tests/test_conn_slots_gpu.py."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import slots_plan as SP
from h2o_amd import codec as C
from h2o_amd import hpack_synth as HS
from h2o_amd import hpenc_synth as HE
from h2o_amd import qpack_synth as QS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCONN, STEPS = 23, 3


def dense_session(name, nconn=NCONN, steps=STEPS, seed=5):
    if name == "blocks":
        return SP.Blocks, SP.hpack_session(HS.make_connections(nconn, (0, 3 * steps), seed=seed, request_frac=0.2), steps, seed)
    if name == "responses":
        return SP.Blocks, SP.hpack_session(HS.make_response_connections(nconn, (0, 3 * steps), seed=seed), steps, seed)
    if name == "qpack":
        return SP.QpackDecode, QS.make_session(nconn, steps, seed=seed, max_sections=(0, 3))
    if name == "hpenc":
        return SP.HpackEncode, HE.make_session(nconn, steps, resp_per_conn=(0, 3), seed=seed)
    if name == "push":
        return SP.HpackEncode, HE.make_push_session(nconn, steps, seed=seed)
    assert name == "qpenc"
    st = HE.to_qpack_sessions(HE.make_session(nconn, 1, resp_per_conn=(0, 3 * steps), seed=seed)[0], steps, seed=seed)
    for s in st:
        s["enc_out_off"] = SP.session_enc_offsets(s)
    return SP.QpackSessions, st


FAMILIES = ["blocks", "responses", "qpack", "hpenc", "push", "qpenc"]


def same_step(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("name", FAMILIES)
def test_identity_plan_rebuilds_the_dense_arrays(name):
    fam, dense = dense_session(name)
    plan = SP.Plan(fam, dense, np.arange(NCONN), [np.arange(NCONN)] * STEPS)
    for k, (step, slot, keys) in enumerate(plan.steps):
        same_step(step, dense[k])
        assert slot.tolist() == list(range(NCONN)) and keys == [(c, k) for c in range(NCONN)]


def synthetic_results(fam, step):
    """results a family's records() can read, made from the step's own bytes: every item's status is a checksum of
    its content, so a record that lands under the wrong key is seen"""
    crc = lambda b: zlib.crc32(b) & 0x7FFFFFFF  # noqa: E731
    nconn = step["conn_first"].size - 1
    n = int(step["conn_first"][-1])
    if fam is SP.Blocks:
        o = step["blk_off"]
        st = [crc(step["data"][int(o[b]):int(o[b + 1])].tobytes()) for b in range(n)]
        return dict(bstatus=np.asarray(st, np.int32), nfields=np.zeros(n, np.uint32), arena=np.zeros(1, np.uint8))
    if fam is SP.QpackDecode:
        o = step["sec_off"]
        st = [crc(step["data"][int(o[k]):int(o[k + 1])].tobytes()) for k in range(n)]
        enc = [crc(step["data"][int(e):int(e) + int(L)].tobytes()) for e, L in zip(step["enc_off"], step["enc_len"])]
        return dict(sstatus=np.asarray(st, np.int32), nfields=np.zeros(n, np.uint32), req_insert_count=np.zeros(n, np.uint64),
                    arena=np.zeros(1, np.uint8), enc_status=np.asarray(enc, np.int32), enc_consumed=step["enc_len"],
                    insert_count=np.zeros(nconn, np.uint64))
    st = np.asarray([crc(step["res"][k:k + 1].tobytes()[:16]) for k in range(n)], np.int32)  # (not hdr_first: it moves)
    r = dict(rstatus=st, out_len=np.zeros(n, np.uint32), out=np.zeros(1, np.uint8), headers_size=np.zeros(n, np.uint32))
    if fam is SP.QpackSessions:
        r.update(rflags=np.zeros(n, np.uint8), header_len=np.zeros(n, np.uint32), enc_out=np.zeros(1, np.uint8),
                 enc_out_len=np.zeros(nconn, np.uint32), dec_status=np.arange(nconn).astype(np.int32) * 0,
                 dec_consumed=np.zeros(nconn, np.uint32))
    return r


def random_order(rng, nconn, steps, frac=0.6):
    return [rng.permutation(nconn)[:max(1, int(frac * nconn))] for _ in range(steps)]


@pytest.mark.parametrize("name", FAMILIES)
def test_unmapping_a_permuted_plan_restores_dense_order(name):
    fam, dense = dense_session(name)
    want = SP.dense_records(fam, dense, [synthetic_results(fam, s) for s in dense])
    rng = np.random.default_rng(11)
    plan = SP.Plan(fam, dense, rng.permutation(131)[:NCONN], random_order(rng, NCONN, STEPS))
    seen = 0
    for t, (step, slot, keys) in enumerate(plan.steps):
        assert slot.size == len(keys) == step["conn_first"].size - 1
        got = plan.unmap(t, fam.records(step, synthetic_results(fam, step)))
        for key, rec in got.items():
            assert rec == want[key], key
            seen += len(rec[1])
    assert seen > NCONN // 2  # the comparison saw real items


def test_restatement_qpack_session_permuted(oracle_codec):
    from oracle import oracle as O

    fam, dense = dense_session("qpack")
    perm = np.random.default_rng(3).permutation(NCONN)
    plan = SP.Plan(fam, dense, np.arange(NCONN), [perm] * STEPS)

    def run(steps):
        s = O.QpackSession(oracle_codec, NCONN)
        out = [s.step(d["data"], d["enc_off"], d["enc_len"], d["sec_off"], d["conn_first"],
                      QS.arena_offsets(d["sec_off"], 4096)) for d in steps]
        s.close()
        return out

    want = SP.dense_records(fam, dense, run(dense))
    got = run([st for st, _, _ in plan.steps])
    for t, (step, _, _) in enumerate(plan.steps):
        for key, rec in plan.unmap(t, fam.records(step, got[t])).items():
            assert rec == want[key], key
    assert any(items and items[0][1] for _, items in want.values())  # sections with fields were compared


def test_restatement_hpack_encoder_session_permuted(oracle_codec):
    from oracle import oracle as O

    fam, dense = dense_session("hpenc")
    perm = np.random.default_rng(4).permutation(NCONN)
    plan = SP.Plan(fam, dense, np.arange(NCONN), [perm] * STEPS)

    def run(steps):
        s = O.HpeSession(oracle_codec, NCONN)
        out = [s.step(d["data"], d["hdr"], d["res"], d["conn_first"], d["out_off"], d["server_off"], d["server_len"])
               for d in steps]
        s.close()
        return out

    want = SP.dense_records(fam, dense, run(dense))
    got = run([st for st, _, _ in plan.steps])
    for t, (step, _, _) in enumerate(plan.steps):
        for key, rec in plan.unmap(t, fam.records(step, got[t])).items():
            assert rec == want[key], key
    assert any(items and items[0][1] for _, items in want.values())  # frames with bytes were compared


@pytest.mark.parametrize("cc, std", [("gcc", "-std=c99"), ("g++", "-std=c++17")])
def test_header_compiles(tmp_path, cc, std):
    src = tmp_path / ("t.c" if cc == "gcc" else "t.cpp")
    src.write_text('#include "hhuff.h"\n'
                   "int use(const hhuff_conn_slots_t *s) { return (int)s->nslots + (int)HHUFF_CONN_RESET + HHUFF_BLK_EINVAL"
                   " + HHUFF_QPK_EINVAL; }\n")
    subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                    str(src)], check=True)


def test_library_exports_the_slots_symbols():
    L = C.lib()
    for name in ("hhuff_hpack_decode_blocks_slots", "hhuff_hpack_parse_requests_slots", "hhuff_hpack_parse_responses_slots",
                 "hhuff_qpack_decode_slots", "hhuff_qpack_parse_requests_slots", "hhuff_qpack_parse_responses_slots",
                 "hhuff_hpack_flatten_responses_slots", "hhuff_qpack_flatten_sessions_slots"):
        assert hasattr(L, name), name
        assert name in C.EXPORTED
