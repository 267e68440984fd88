#!/usr/bin/env python3
"""Promises per second of hhuff_hpack_flatten_responses on a pushing server's batch: 4,096 synthetic connections
(h2o_amd/hpenc_synth.make_push_session: promises, their parents' responses and the pushed responses in wire
order) tiled 16 times, timed the way tools/bench_configs.hpenc_line times the response batch (an event pair a
call, the median of 10 after 2 warm-up calls).  Prints one JSON line.  Informational: no gate reads it.

    python tools/push_promise_rate.py [--connections 65536] [--push-only]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--connections", type=int, default=65536)
    ap.add_argument("--push-only", action="store_true", help="leave the responses out: promises alone")
    args = ap.parse_args()

    import torch

    import bench_configs as BC
    from h2o_amd import codec
    from h2o_amd import hpenc_synth as HE

    assert torch.cuda.is_available(), "needs a GPU"
    base = HE.make_push_session(4096, seed=13, push_only=args.push_only)[0]
    b = HE.tile(base, max(1, args.connections // 4096))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()  # noqa: E731
    d, hd, rs = dev(b["data"]), dev(b["hdr"].view(np.uint8)), dev(b["res"].view(np.uint8))
    cf, oo = dev(b["conn_first"].view(np.int32)), dev(b["out_off"].view(np.int64))
    nres, nc = int(b["res"].size), int(b["conn_first"].size - 1)
    out = torch.empty(int(b["out_off"][-1]), dtype=torch.uint8, device="cuda")
    scratch = torch.empty(int(codec.lib().hhuff_hpack_enc_scratch_size(nc)), dtype=torch.uint8, device="cuda")
    res = {}

    def run():
        res["r"] = codec.hpack_flatten_responses(d, hd, rs, cf, nres, oo, b["server_off"], b["server_len"],
                                                 in_size=int(b["data"].size), out=out, scratch=scratch)

    t = BC.timed(torch, run, steps=10, warmup=2)
    r = res["r"]
    push = (b["res"]["flags"] & codec.RES_PUSH_PROMISE) != 0
    npush = int(push.sum())
    ok = (r["rstatus"][:nres] == 0).cpu().numpy()
    print(json.dumps({"config": "push", "connections": nc, "records": nres, "promises": npush,
                      "ok_records": int(ok.sum()), "ok_promises": int(ok[push].sum()), "fields": int(b["hdr"].size),
                      "frame_bytes": int(r["out_len"][:nres].to(torch.int64).sum().item()), "flatten_ms": round(t, 4),
                      "records_per_s": round(nres / (t * 1e-3), 1), "promises_per_s": round(npush / (t * 1e-3), 1)}))


if __name__ == "__main__":
    main()
