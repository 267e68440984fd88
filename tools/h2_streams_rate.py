"""What hhuff_h2_streams costs (include/hhuff.h (2k''')): a step of many connections in two shapes, laid out as the three
calls in front leave it (tests/h2streams_model.build)
  requests  per connection a SETTINGS, three GETs with END_STREAM and a WINDOW_UPDATE on the first of them
  upload    per connection one POST and 16 DATA frames of 1 KiB, every eighth padded, the last with END_STREAM
Two device times per shape: the call on new connections (every table cleared first), and the same step again on the
tables it left (HHUFF_H2ST_CONTINUE: the streams are there, so HEADERS fail as h2o fails them and DATA meets closed
streams -- the table is probed, nothing is inserted).  HIP events around each call, the median of 30 calls after 5
warm-ups (deframe_rate.py's `timed`); every timed call works on the next of --sets separate copies of its buffers and
slabs.

    python tools/h2_streams_rate.py [--connections 65536] [--out profiles/h2_streams_rate.jsonl]

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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import h2streams_corpora as K  # noqa: E402
import h2streams_model as M  # noqa: E402


def shape(name):
    s = K.S()
    if name == "requests":
        s.settings(1000).headers(1, True).headers(3, True).headers(5, True).wu(1, 100)
    else:
        s.headers(1)
        for k in range(16):
            s.data(1, 1024, pad=8 if k % 8 == 7 else 0, end_stream=k == 15)
    return dict(frames=s.frames, blocks=s.blocks, ops=s.ops)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--connections", type=int, default=65536)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    nconn = a.connections
    P = M.params(max_streams=100, max_streams_for_priority=16, active_stream_window_size=16 * 1048576, max_entries=None)
    P["max_entries"] = 117
    for name in ("requests", "upload"):
        one = shape(name)
        lay = M.build([one] * nconn)
        w = M.walk(M.new_conn(), P, 66535, one["frames"], one["blocks"])
        slab = 32 + 256 * 48
        info = {"call": "hhuff_h2_streams", "config": name, "connections": nconn, "frames": lay["frm_cap"], "max_entries": P["max_entries"],
                "scratch_bytes": nconn * slab, "reply_bytes": nconn * len(w["replies"])}
        if a.dry:
            print(json.dumps(info), flush=True)
            continue
        import torch

        import deframe_rate as DR
        from h2o_amd import codec as C

        def dev(x):
            x = np.ascontiguousarray(x)
            x = x.view(np.int32) if x.dtype == np.uint32 else (x.view(np.uint8) if x.dtype.names else x)
            return torch.from_numpy(x.copy()).cuda()

        assert C.h2_streams_scratch_size(nconn, P["max_entries"]) == nconn * slab
        peers = C.h2_new_peers(nconn)
        peers["initial_window_size"] = 66535
        sets = []
        for _ in range(a.sets):
            t = {k: dev(lay[k]) for k in ("frames", "nframes", "frm_first", "ctl", "nctl", "ctl_rep", "ctl_rep_off", "blocks", "conn_first",
                                          "bstatus", "req", "arena", "blk_off", "value_off", "value_len", "rep_off")}
            t["peers"], t["data"] = dev(peers.view(np.uint8)), torch.zeros(8, dtype=torch.uint8, device="cuda")
            t["scratch"] = torch.empty(nconn * slab, dtype=torch.uint8, device="cuda")
            u8, i32 = torch.uint8, torch.int32
            t["out"] = dict(sev=torch.empty(16 * lay["frm_cap"], dtype=u8, device="cuda"), rep=torch.empty(lay["rep_size"], dtype=u8, device="cuda"),
                            **{k: torch.empty(nconn, dtype=i32, device="cuda") for k in ("nstr", "sstatus", "serr", "rep_len")})
            sets.append(t)

        def call(flags):
            def f(i):
                t = sets[i % a.sets]
                C.h2_streams(P, t["scratch"], t["data"], t["frames"], t["nframes"], t["frm_first"], lay["frm_cap"], t["ctl"], t["nctl"],
                             t["ctl_rep"], t["ctl_rep_off"], t["blocks"], t["conn_first"], t["bstatus"], t["req"], t["arena"], t["blk_off"],
                             t["value_off"], t["value_len"], t["peers"], t["rep_off"], flags=flags, in_size=lay["in_size"],
                             ctl_rep_size=lay["ctl_rep_size"], arena_size=lay["arena_size"], rep_size=lay["rep_size"], out=t["out"])
            return f

        t_new = DR.timed(torch, call(0))
        torch.cuda.synchronize()
        o = sets[0]["out"]
        assert bool((o["sstatus"] == w["status"]).all()) and bool((o["nstr"] == w["nstr"]).all())
        assert int(o["rep_len"].sum().item()) == nconn * len(w["replies"])
        t_cont = DR.timed(torch, call(C.H2ST_CONTINUE))
        torch.cuda.synchronize()
        info.update({"new_ms": round(t_new, 4), "continue_ms": round(t_cont, 4), "frames_per_s": round(lay["frm_cap"] / (t_new * 1e-3), 1),
                     "connections_per_s": round(nconn / (t_new * 1e-3), 1)})
        print(json.dumps(info), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(info) + "\n")
        del sets


if __name__ == "__main__":
    main()
