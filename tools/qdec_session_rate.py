"""What the decoder sessions cost (include/hhuff.h (2e''')): device time of one hhuff_qpack_parse_requests_sessions
step against hhuff_qpack_parse_requests on the same batch -- the QPACK decoder's bench shape (65,536 synthetic
HTTP/3 connections, tools/bench_configs.py qpack_line) and a sparse step of 1,024 of 65,536 connection slots
(hhuff_qpack_parse_requests_slots on the other side).  The session call runs the same passes with the blocked-limit
pass replaced by the session pass and the refusal test inside the encoder-stream pass; every buffer of both calls is
allocated once, outside the timed region.  HIP events around each call, the median of 30 calls after 5 warm-ups; every
call starts its connections fresh.

    python tools/qdec_session_rate.py [--out profiles/qdec_session_rate.jsonl]

One JSON line per shape: plain_ms, sessions_ms, their ratio, and what the step decoded, parked and acknowledged.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NSLOTS = 65536
MAX_BLOCKED = 100


def line(torch, codec, BC, active, sparse):
    from h2o_amd import qpack_synth as QS

    st = QS.make_session(active, steps=1, seed=9, adversarial_frac=0.01)[0]
    L = np.diff(st["sec_off"].astype(np.uint64))  # the arena slices of bench_configs.qpack_line
    ao_np = np.concatenate([[0], np.cumsum((L * 8) // 5 + L * np.uint64(64) + np.uint64(512))]).astype(np.uint64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()  # noqa: E731
    u32 = lambda a: dev(np.asarray(a, np.uint32).view(np.int32))  # noqa: E731
    d, eo, el, so, cf = dev(st["data"]), u32(st["enc_off"]), u32(st["enc_len"]), u32(st["sec_off"]), u32(st["conn_first"])
    ao = dev(ao_np.view(np.int64))
    nsec = int(st["conn_first"][-1])
    nstate = NSLOTS if sparse else active
    slots = None
    if sparse:
        slot = np.random.default_rng(1).permutation(NSLOTS)[:active]
        slots = codec.ConnSlots(u32(slot), None, NSLOTS)
    scratch = torch.empty(int(codec.lib().hhuff_qpack_scratch_size(nstate, 4096)), dtype=torch.uint8, device="cuda")
    arena = torch.empty(int(ao_np[-1]), dtype=torch.uint8, device="cuda")
    sid = dev(np.arange(nsec, dtype=np.int64) * 4)
    room = codec.qpack_dsession_out_bound(np.diff(st["conn_first"].astype(np.int64)))
    doff = dev(np.concatenate([[0], np.cumsum(room)]).astype(np.int64))
    ds = dict(state=torch.empty(codec.qpack_dsession_state_size(nstate, MAX_BLOCKED), dtype=torch.uint8, device="cuda"),
              dec_out_off=doff, dec_out=torch.empty(int(room.sum()), dtype=torch.uint8, device="cuda"),
              wake_first=u32(np.arange(active + 1, dtype=np.int64) * 4),
              wake_id=torch.empty(4 * active, dtype=torch.int64, device="cuda"))
    kw = dict(arena_off=ao, in_size=int(st["data"].size), scratch=scratch, arena=arena, stream_id=sid, slots=slots)
    res = {}

    def plain():
        res["p"] = codec.qpack_decode(d, eo, el, so, cf, nsec, 4096, MAX_BLOCKED, **kw)

    def sessions():
        res["s"] = codec.qpack_decode(d, eo, el, so, cf, nsec, 4096, MAX_BLOCKED, sessions=codec.QpackDsessions(**ds), **kw)

    tp, ts = BC.timed(torch, plain, steps=30, warmup=5), BC.timed(torch, sessions, steps=30, warmup=5)
    p, s = res["p"], res["s"]
    assert torch.equal(p["sstatus"][:nsec], s["sstatus"][:nsec]) and torch.equal(p["req"][:nsec], s["req"][:nsec])
    return {"call": "hhuff_qpack_parse_requests_sessions", "against": "hhuff_qpack_parse_requests" + ("_slots" if sparse else ""),
            "slots": nstate, "active": active, "sections": nsec, "ok_sections": int((s["sstatus"][:nsec] == 0).sum().item()),
            "parked": int(s["parked"][:active].to(torch.int64).sum().item()),
            "decoder_stream_bytes": int(s["dec_out_len"][:active].to(torch.int64).sum().item()),
            "plain_ms": round(tp, 4), "sessions_ms": round(ts, 4), "ratio": round(ts / tp, 4),
            "sessions_sections_per_s": round(nsec / (ts * 1e-3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    args = ap.parse_args()
    import torch

    import bench_configs as BC
    from h2o_amd import codec

    torch.cuda.set_device(0)
    for active, sparse in ((65536, False), (1024, True)):
        out = json.dumps(line(torch, codec, BC, active, sparse))
        print(out, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(out + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
