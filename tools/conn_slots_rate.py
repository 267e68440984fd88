"""What sparse steps buy (include/hhuff.h (2h)): a scratch of 65,536 connection slots of which 1,024 / 8,192 / 65,536
have work this step, through hhuff_hpack_parse_requests_slots and hhuff_qpack_flatten_sessions_slots (the call
lists the active connections only), against the way without slots: the dense call over all 65,536 connections
with empty ranges for the idle ones.  Both do the same work for the same connections in the same slabs; every call
starts its connections fresh.  HIP events around each call, the median of 30 calls after 5 warm-ups.

    python tools/conn_slots_rate.py [--out profiles/conn_slots_rate.jsonl]

One JSON line per family and active count: sparse_ms, dense_ms and what was encoded or decoded.
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


def spread(conn_first, slot):
    """conn_first of the listed connections -> conn_first over all slots, the idle ones empty (slot ascending)"""
    n = np.diff(conn_first.astype(np.int64))
    per = np.zeros(NSLOTS, np.int64)
    per[slot] = n
    return np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)


def requests_line(torch, codec, BC, active, slot):
    from h2o_amd import hpack_synth as HS

    b = HS.make_connections(active, seed=5, adversarial_frac=0.01)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()  # noqa: E731
    d, bo = dev(b["data"]), dev(b["blk_off"].view(np.int32))
    L = np.diff(b["blk_off"].astype(np.int64))
    ao = dev(np.concatenate([[0], np.cumsum(16 * L + 1024)]).astype(np.int64))  # as bench_configs.blocks_line
    scratch = torch.empty(int(codec.lib().hhuff_hpack_scratch_size(NSLOTS, 4096)), dtype=torch.uint8, device="cuda")
    cf_sparse = dev(b["conn_first"].view(np.int32))
    cf_dense = dev(spread(b["conn_first"], slot).view(np.int32))
    slots = codec.ConnSlots(dev(slot.astype(np.uint32).view(np.int32)), None, NSLOTS)
    kw = dict(arena_off=ao, in_size=int(b["data"].size), requests=True, scratch=scratch)
    res = {}

    def sparse():
        res["s"] = codec.hpack_decode_blocks(d, bo, cf_sparse, 4096, slots=slots, **kw)

    def dense():
        res["d"] = codec.hpack_decode_blocks(d, bo, cf_dense, 4096, **kw)

    ts, td = BC.timed(torch, sparse, steps=30, warmup=5), BC.timed(torch, dense, steps=30, warmup=5)
    nblk = len(b["blk_off"]) - 1
    assert torch.equal(res["s"]["bstatus"][:nblk], res["d"]["bstatus"][:nblk])
    return {"call": "hhuff_hpack_parse_requests_slots", "slots": NSLOTS, "active": active, "blocks": nblk,
            "ok_blocks": int((res["s"]["bstatus"][:nblk] == 0).sum().item()), "sparse_ms": round(ts, 4), "dense_ms": round(td, 4)}


def sessions_line(torch, codec, BC, active, slot):
    from h2o_amd import hpenc_synth as HE

    base = HE.to_qpack_sessions(HE.make_session(min(active, 4096), seed=13)[0], 2, seed=13)[0]
    q = BC._qpack_tiled(base, max(1, active // 4096), HE.qpack_session_out_offsets)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()  # noqa: E731
    d, hd, rs = dev(q["data"]), dev(q["hdr"].view(np.uint8)), dev(q["res"].view(np.uint8))
    sid, oo = dev(q["stream_id"].view(np.int64)), dev(q["out_off"].view(np.int64))
    nres, room = int(q["res"].size), 4112
    out = torch.empty(int(q["out_off"][-1]), dtype=torch.uint8, device="cuda")
    enc_out = torch.empty(active * room, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(codec.qpack_enc_scratch_size(NSLOTS, 4096, 64), dtype=torch.uint8, device="cuda")
    eo_sparse = torch.arange(active + 1, dtype=torch.int64, device="cuda") * room
    per = np.zeros(NSLOTS, np.int64)
    per[slot] = room
    eo_dense = dev(np.concatenate([[0], np.cumsum(per)]).astype(np.int64))
    cf_sparse = dev(q["conn_first"].view(np.int32))
    cf_dense = dev(spread(q["conn_first"], slot).view(np.int32))
    slots = codec.ConnSlots(dev(slot.astype(np.uint32).view(np.int32)), None, NSLOTS)
    kw = dict(max_blocked=1 << 20, server_off=q["server_off"], server_len=q["server_len"], in_size=int(q["data"].size),
              out=out, enc_out=enc_out, scratch=scratch, set_capacity=True)
    res = {}

    def sparse():
        res["s"] = codec.qpack_flatten_sessions(d, hd, rs, cf_sparse, nres, sid, oo, enc_out_off=eo_sparse, slots=slots, **kw)

    def dense():
        res["d"] = codec.qpack_flatten_sessions(d, hd, rs, cf_dense, nres, sid, oo, enc_out_off=eo_dense, **kw)

    ts, td = BC.timed(torch, sparse, steps=30, warmup=5), BC.timed(torch, dense, steps=30, warmup=5)
    assert torch.equal(res["s"]["out_len"][:nres], res["d"]["out_len"][:nres])
    return {"call": "hhuff_qpack_flatten_sessions_slots", "slots": NSLOTS, "active": active, "responses": nres,
            "ok_responses": int((res["s"]["rstatus"][:nres] == 0).sum().item()), "sparse_ms": round(ts, 4),
            "dense_ms": round(td, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    args = ap.parse_args()
    import torch

    import bench_configs as BC
    from h2o_amd import codec

    torch.cuda.set_device(0)
    rng = np.random.default_rng(1)
    for active in (1024, 8192, 65536):
        slot = np.sort(rng.permutation(NSLOTS)[:active])  # ascending: the dense call needs the connections in slot order
        for fn in (requests_line, sessions_line):
            line = json.dumps(fn(torch, codec, BC, active, slot))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
