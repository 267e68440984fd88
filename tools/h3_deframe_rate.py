"""What the HTTP/3 de-framer costs in front of the request decoder (include/hhuff.h (2l)): 65,536 connections, each
with a control stream (its type byte and a SETTINGS frame), a QPACK encoder stream (its type byte and the step's
encoder instructions) and one or two request streams (a HEADERS frame each, every third with a DATA frame of 100
bytes behind it, which the walk stops in front of).  The sections and encoder bytes are a qpack_synth decoder session
of --unique connections, repeated to the connection count (the de-framer reads every byte either way; generating
65,536 different sessions would only lengthen the run).  Two configurations: "headers" as above, and "walk_on", where
every request stream has HHUFF_H3S_WALK_ON and eight more small frames behind the DATA frame, so that a lane's chain
is ten frames instead of one.  Three device times per configuration:
  deframe   hhuff_h3_deframe
  parse     hhuff_qpack_parse_requests on its output, the step it precedes
  memcpy    hipMemcpyAsync device to device of the same number of section and encoder bytes: the gather's floor
HIP events around each call, the median of 30 calls after 5 warm-ups.  Every timed call works on the next of several
separate copies of the buffers it touches, each rotation sized from the bytes its own calls touch so that one turn is
twice the 256 MB Infinity Cache (tools/deframe_rate.py explains why); the decoder's sets are counted at 3 B a gathered
byte.  The only memory a call shares with its predecessor is the de-framer's pooled workspace (65 bytes a stream).

    python tools/h3_deframe_rate.py [--connections 65536] [--unique 4096] [--out profiles/h3_deframe_rate.jsonl]

One JSON line per configuration: the three times, deframe / parse, deframe / memcpy, and for "walk_on" the time a
frame of a lane's chain adds.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEPS, WARMUP = 30, 5
CACHE = 256 << 20
ARENA_FIXED, ARENA_PER_BYTE = 4096 + 1024, 16  # a section's slice: a table's worth of entries and 16 B a section byte
K_REQUEST, K_UNI, S_WALK_ON = 0, 1, 1


def vi(v):
    w = 1 if v < 1 << 6 else 2 if v < 1 << 14 else 4 if v < 1 << 30 else 8
    return (v | ({1: 0, 2: 1, 4: 2, 8: 3}[w] << (8 * w - 2))).to_bytes(w, "big")


def wire(sess, nconn, walk_on, seed):
    """-> data, str_off, conn_str, frm_first, states, frames, the gathered bytes the call must produce"""
    rng = np.random.default_rng(seed)
    raw, uniq = sess["data"].tobytes(), sess["conn_first"].size - 1
    settings = b"\x00\x04" + vi(6) + vi(1) + vi(4096) + vi(7) + vi(100)
    extra = b"".join(vi(0x21 + 0x1f * k) + vi(3) + b"abc" for k in range(8))
    streams, conn_str, caps, kinds, flags, ids = [], [0], [], [], [], []
    enc_bytes, sec_bytes = [], []
    for c in range(nconn):
        u = c % uniq
        enc = raw[int(sess["enc_off"][u]):int(sess["enc_off"][u]) + int(sess["enc_len"][u])]
        streams += [settings, b"\x02" + enc]
        caps += [1, 0]
        kinds += [K_UNI, K_UNI]
        flags += [0, 0]
        ids += [3, 7]
        enc_bytes.append(enc)
        for k in range(int(sess["conn_first"][u]), int(sess["conn_first"][u + 1])):
            sec = raw[int(sess["sec_off"][k]):int(sess["sec_off"][k + 1])]
            body = b"\x00" + vi(100) + bytes(rng.integers(0, 256, 100, dtype=np.uint8)) if walk_on or k % 3 == 0 else b""
            streams.append(b"\x01" + vi(len(sec)) + sec + body + (extra if walk_on else b""))
            caps.append(10 if walk_on else 1)
            kinds.append(K_REQUEST)
            flags.append(S_WALK_ON if walk_on else 0)
            ids.append(4 * (k - int(sess["conn_first"][u])))
            sec_bytes.append(sec)
        conn_str.append(len(streams))
    nstr = len(streams)
    str_off = np.zeros(nstr + 1, np.uint64)
    str_off[1:] = np.cumsum([len(s) for s in streams])
    frm_first = np.zeros(nstr + 1, np.uint64)
    frm_first[1:] = np.cumsum(caps)
    st = np.zeros((nstr, 32), np.uint8)
    st[:, :8] = np.asarray(ids, np.uint64).view(np.uint8).reshape(-1, 8)
    st[:, 16], st[:, 18] = kinds, flags
    return (np.frombuffer(b"".join(streams), np.uint8).copy(), str_off.astype(np.uint32), np.asarray(conn_str, np.uint32),
            frm_first.astype(np.uint32), st.reshape(-1), int(frm_first[-1]), b"".join(enc_bytes) + b"".join(sec_bytes), len(sec_bytes))


def main():
    from deframe_rate import hip_runtime, timed

    ap = argparse.ArgumentParser()
    ap.add_argument("--connections", type=int, default=65536)
    ap.add_argument("--unique", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from h2o_amd import codec
    from h2o_amd import qpack_synth as QS

    L = codec.lib()
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    nconn = a.connections
    sess = QS.make_session(min(a.unique, nconn), steps=1, seed=5, adversarial_frac=0.0, max_sections=(1, 2), blocked_frac=0.0)[0]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()  # noqa: E731
    i32 = lambda n: torch.empty(max(1, n), dtype=torch.int32, device="cuda")  # noqa: E731
    i64 = lambda n: torch.empty(max(1, n), dtype=torch.int64, device="cuda")  # noqa: E731
    u8 = lambda n: torch.empty(max(1, n), dtype=torch.uint8, device="cuda")  # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    base = None
    for name, walk_on in (("headers", False), ("walk_on", True)):
        data, str_off, conn_str, frm_first, st, frm_cap, gathered, nsec = wire(sess, nconn, walk_on, seed=6)
        nstr, in_size, moved = str_off.size - 1, int(data.size), len(gathered)
        scratch_size = int(L.hhuff_qpack_scratch_size(nconn, 4096))
        arena_size = ARENA_FIXED * nstr + ARENA_PER_BYTE * in_size
        touched_copy = 2 * moved
        touched_deframe = in_size + moved + 32 * frm_cap + 32 * 2 * nstr + 36 * nstr + 44 * nconn
        touched_decoder = 3 * moved
        rot = max(2, -(-2 * CACHE // min(touched_copy, touched_deframe)))
        rot_dec = max(2, -(-2 * CACHE // touched_decoder))
        sets, decs = [], []
        for _ in range(rot):
            s = dict(data=dev(data), str_off=dev(str_off.view(np.int32)), conn_str=dev(conn_str.view(np.int32)),
                     frm_first=dev(frm_first.view(np.int32)), st=dev(st))
            s["out"] = dict(st_out=u8(32 * nstr), frames=u8(32 * frm_cap), nframes=i32(nstr), consumed=i32(nstr), sstatus=i32(nstr),
                            serr=i32(nstr), out=u8(in_size), enc_off=i32(nconn), enc_len=i32(nconn), sec_off=i32(nstr + 1),
                            conn_first=i32(nconn + 1), sec_stream_id=i64(nstr), sec_stream=i32(nstr), totals=i32(3), peers=u8(8 * nconn),
                            settings=u8(16 * nconn), got_settings=i32(nconn), arena_off=i64(nstr + 1))
            s["copy"] = u8(moved)
            sets.append(s)
        for _ in range(rot_dec):
            decs.append(dict(arena=u8(arena_size), f=[i32(in_size) for _ in range(4)], fflags=u8(in_size), nfields=i32(nstr),
                             sstatus=i32(nstr), ric=i64(nstr), enc_status=i32(nconn), enc_consumed=i32(nconn), ic=i64(nconn),
                             req=u8(nstr * codec.QREQ_BYTES), scratch=u8(max(16, scratch_size))))

        def deframe(i):
            s = sets[i % rot]
            codec.h3_deframe(s["data"], s["str_off"], s["conn_str"], s["frm_first"], frm_cap, s["st"], 16384, 0, in_size=in_size,
                             arena_fixed=ARENA_FIXED, arena_per_byte=ARENA_PER_BYTE, out=s["out"])

        def parse(i):
            o, k = sets[i % rot]["out"], decs[i % rot_dec]
            p = lambda t: t.data_ptr()  # noqa: E731
            rc = L.hhuff_qpack_parse_requests(p(o["out"]), in_size, p(o["enc_off"]), p(o["enc_len"]), p(o["sec_off"]), p(o["conn_first"]),
                                              nconn, nsec, 4096, 100, None, p(k["arena"]), p(o["arena_off"]), p(k["f"][0]), p(k["f"][1]),
                                              p(k["f"][2]), p(k["f"][3]), p(k["fflags"]), p(k["nfields"]), p(k["sstatus"]), p(k["ric"]),
                                              p(k["enc_status"]), p(k["enc_consumed"]), p(k["ic"]), p(o["sec_stream_id"]), p(k["req"]),
                                              p(k["scratch"]), k["scratch"].numel(), 0, stream)
            assert rc == 0

        def memcpy(i):
            s = sets[i % rot]
            assert hip.hipMemcpyAsync(s["copy"].data_ptr(), s["out"]["out"].data_ptr(), moved, 3, stream) == 0  # D2D

        t_def = timed(torch, deframe)
        for i in range(rot):  # every set de-framed: the decoder's input
            deframe(i)
        torch.cuda.synchronize()
        o = sets[0]["out"]
        assert o["totals"].tolist() == [nsec, moved - int(o["totals"][2]), int(o["totals"][2])] and bool((o["sstatus"] == 0).all())
        assert bool(o["got_settings"].all()) and torch.equal(o["out"][:moved], dev(np.frombuffer(gathered, np.uint8)))
        nframes = int(o["nframes"].sum())
        t_par = timed(torch, parse)
        torch.cuda.synchronize()
        sst = decs[0]["sstatus"][:nsec]
        ok = int((sst == 0).sum())
        t_cpy = timed(torch, memcpy)
        line = {"call": "hhuff_h3_deframe", "config": name, "connections": nconn, "streams": nstr, "sections": nsec, "frames": nframes,
                "wire_bytes": in_size, "gathered_bytes": moved, "rotated_sets": rot, "decoder_sets": rot_dec,
                "touched_bytes": {"deframe": touched_deframe, "parse_at_least": touched_decoder, "memcpy": touched_copy},
                "sections_decoded_ok": ok, "deframe_ms": round(t_def, 4), "parse_requests_ms": round(t_par, 4),
                "memcpy_d2d_ms": round(t_cpy, 4), "deframe_over_parse": round(t_def / t_par, 4),
                "deframe_over_memcpy": round(t_def / t_cpy, 2), "wire_bytes_per_s": round(in_size / (t_def * 1e-3), 1)}
        if base is None:
            base = (t_def, nframes, nstr)
        else:  # both walks follow the longer chains: what one more frame of a lane's chain adds to the call
            line["us_per_chain_frame"] = round(1e3 * (t_def - base[0]) / 9.0, 3)
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del sets, decs


if __name__ == "__main__":
    main()
