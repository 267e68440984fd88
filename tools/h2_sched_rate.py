"""What hhuff_h2_schedule costs (include/hhuff.h (2o)): a step of ops plus run for many new connections, in two
shapes, beside hhuff_h2_frame_data on the very records it ordered
  flat4     four streams under the root (weights 16, 32, 64, 256), opened and activated by the step, each with a
            candidate of 1 KiB: the common flat tree
  chain16   a Chromium-style chain: 16 exclusive opens, each under the stream in front, all activated, 16 candidates
Every stream is visited once (the region has room for all).  HIP events around each call, the median of 30 calls after 5
warm-ups (deframe_rate.py's `timed`); every timed call works on the next of --sets separate copies of its buffers and
slabs, and starts its connections fresh: a fresh connection reads no slab and writes only the entries in use, so the
slabs' traffic is small and may stay in the last-level cache between calls.

    python tools/h2_sched_rate.py [--connections 65536] [--out profiles/h2_sched_rate.jsonl]

One JSON line per shape.  --dry builds the batch and prints the sizes without a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

BODY = 1024


def shape(name):
    """-> [(stream_id, op, parent_id, weight, exclusive)], the stream ids"""
    if name == "flat4":
        ids, ops = [1, 3, 5, 7], []
        for i, w in zip(ids, (16, 32, 64, 256)):
            ops += [(i, 1, 0, w, 0), (i, 4, 0, 0, 0)]
        return ops, ids
    ids, ops = [2 * k + 1 for k in range(16)], []
    for k, i in enumerate(ids):
        ops += [(i, 1, ids[k - 1] if k else 0, 16 + k, 1), (i, 4, 0, 0, 0)]
    return ops, ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--connections", type=int, default=65536)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--max-nodes", type=int, default=117)
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    nconn = a.connections
    for name in ("flat4", "chain16"):
        ops1, ids = shape(name)
        ns, region = len(ids), len(ids) * (BODY + 9) + 16
        info = {"call": "hhuff_h2_schedule", "config": name, "connections": nconn, "streams": ns, "ops": nconn * len(ops1),
                "records": nconn * ns, "max_nodes": a.max_nodes, "scratch_bytes": nconn * ((32 + 24 * a.max_nodes + 15) & ~15),
                "framed_bytes": nconn * ns * (BODY + 9)}
        if a.dry:
            print(json.dumps(info), flush=True)
            continue
        import torch

        import deframe_rate as DR
        from h2o_amd import codec as C

        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
        first = lambda n: torch.from_numpy((np.arange(nconn + 1, dtype=np.uint64) * n).astype(np.uint32).view(np.int32)).cuda()  # noqa: E731
        ops = np.zeros(len(ops1), C.H2_SCHED_OP_DTYPE)
        for k, f in enumerate(("stream_id", "op", "parent_id", "weight", "exclusive")):
            ops[f] = [o[k] for o in ops1]
        sends = np.zeros(ns, C.H2_SEND_DTYPE)
        sends["stream_id"], sends["body_len"], sends["window"], sends["flags"] = ids[::-1], BODY, 65535, C.H2S_FINAL
        peers = C.h2_new_peers(nconn)
        peers["send_window"] = 1 << 24
        assert C.h2_sched_scratch_size(nconn, a.max_nodes) == info["scratch_bytes"]
        body = torch.zeros(BODY, dtype=torch.uint8, device="cuda")
        sets = []
        for _ in range(a.sets):
            t = dict(ops=dev(np.tile(ops, nconn)), op_first=first(len(ops1)), sends=dev(np.tile(sends, nconn)), send_first=first(ns),
                     peers=dev(peers), out_off=first(region), scratch=torch.empty(info["scratch_bytes"], dtype=torch.uint8, device="cuda"))
            u8, i32 = torch.uint8, torch.int32
            t["out"] = dict(ordered=torch.empty(24 * nconn * ns, dtype=u8, device="cuda"), active=torch.empty(nconn, dtype=u8, device="cuda"),
                            op_status=torch.empty(nconn * len(ops1), dtype=i32, device="cuda"),
                            **{k: torch.empty(nconn * ns, dtype=i32, device="cuda") for k in ("order", "pos")},
                            **{k: torch.empty(nconn, dtype=i32, device="cuda") for k in ("nvisit", "cstatus")})
            t["fout"] = dict(sent=torch.empty(24 * nconn * ns, dtype=u8, device="cuda"), out=torch.empty(nconn * region, dtype=u8, device="cuda"),
                             peers=torch.empty(40 * nconn, dtype=u8, device="cuda"),
                             **{k: torch.empty(nconn, dtype=i32, device="cuda") for k in ("out_len", "cstatus")})
            sets.append(t)

        def sched(i):
            t = sets[i % a.sets]
            C.h2_schedule(a.max_nodes, t["scratch"], t["sends"], t["send_first"], t["peers"], t["out_off"], ops=t["ops"], op_first=t["op_first"],
                          out_size=nconn * region, out=t["out"])

        def frame(i):
            t = sets[i % a.sets]
            C.h2_frame_data(body, t["out"]["ordered"], t["send_first"], t["peers"], t["out_off"], out_size=nconn * region, out=t["fout"])

        t_sched = DR.timed(torch, sched)
        torch.cuda.synchronize()
        o = sets[0]["out"]
        assert bool((o["nvisit"] == ns).all()) and not bool(o["cstatus"].any()) and not bool(o["op_status"].any()) and not bool(o["active"].any())
        t_frame = DR.timed(torch, frame)
        torch.cuda.synchronize()
        assert int(sets[0]["fout"]["out_len"].sum().item()) == info["framed_bytes"]
        info.update({"schedule_ms": round(t_sched, 4), "frame_data_ms": round(t_frame, 4), "schedule_over_frame_data": round(t_sched / t_frame, 3),
                     "visits_per_s": round(nconn * ns / (t_sched * 1e-3), 1), "connections_per_s": round(nconn / (t_sched * 1e-3), 1)})
        print(json.dumps(info), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(info) + "\n")
        del sets


if __name__ == "__main__":
    main()
