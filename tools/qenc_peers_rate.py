"""What per-connection peer settings cost (include/hhuff.h (2g'')): one fresh step of 65,536 QPACK encoder sessions
through hhuff_qpack_flatten_sessions_peers with a mixed peer population -- table capacities from {0, 31, 32, 64, 220,
1024, 4096}, blocked-stream limits from {0, 1, 2, 100}, drawn independently per connection
(hpenc_synth.qpack_peer_population) -- against the uniform hhuff_qpack_flatten_sessions call on the same batch, the
same header_table_size (4096) and the same scratch.  conn_slots_rate.py's batch, warm-up and clock: HIP events around
each call, the median of 30 calls after 5 warm-ups.  The uniform call is timed three times, before, between and after
the two mixed measurements; the spread of its three medians is the run-to-run noise the mixed step is held against.
The mixed population does less work than the uniform call (a connection whose peer allows no table inserts nothing),
so a third call isolates the record's own cost: the peers entry point with the record {4096, 2^32 - 1} for every
connection, which does exactly the uniform call's work and writes its bytes.

    python tools/qenc_peers_rate.py [--out profiles/qenc_peers_rate.jsonl]

One JSON line: uniform_ms (the three medians), uniform_spread_ms, mixed_ms (the two), same_settings_ms (the two)
and what each call encoded.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NCONN = 65536
CAPACITIES = (0, 31, 32, 64, 220, 1024, 4096)
BLOCKED = (0, 1, 2, 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the line to this file as well")
    ap.add_argument("--evict", action="store_true", help="HHUFF_QENC_EVICT sessions")
    args = ap.parse_args()
    import torch

    import bench_configs as BC
    from h2o_amd import codec
    from h2o_amd import hpenc_synth as HE

    torch.cuda.set_device(0)
    base = HE.to_qpack_sessions(HE.make_session(4096, seed=13)[0], 2, seed=13)[0]
    q = BC._qpack_tiled(base, NCONN // 4096, HE.qpack_session_out_offsets)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()  # noqa: E731
    d, hd, rs = dev(q["data"]), dev(q["hdr"].view(np.uint8)), dev(q["res"].view(np.uint8))
    sid, oo, cf = dev(q["stream_id"].view(np.int64)), dev(q["out_off"].view(np.int64)), dev(q["conn_first"].view(np.int32))
    nres = int(q["res"].size)
    # an encoder-stream region that holds a step's inserts with or without eviction (hhuff_qpack_session_enc_bound)
    h = q["hdr"]
    both = codec.HDR_TOKEN | codec.HDR_LIKELY_TO_REPEAT
    ltr = (h["flags"] & both) == both
    nv = np.concatenate([[0], np.cumsum(np.where(ltr, h["name_len"].astype(np.int64) + h["value_len"], 0))])
    nl = np.concatenate([[0], np.cumsum(ltr.astype(np.int64))])
    first, nh = q["res"]["hdr_first"].astype(np.int64), q["res"]["nhdr"].astype(np.int64)
    rv = np.concatenate([[0], np.cumsum(nv[first + nh] - nv[first])])
    rn = np.concatenate([[0], np.cumsum(nl[first + nh] - nl[first])])
    c64 = q["conn_first"].astype(np.int64)
    b = codec.qpack_session_enc_bound(rv[c64[1:]] - rv[c64[:-1]], rn[c64[1:]] - rn[c64[:-1]], q["server_len"],
                                      c64[1:] - c64[:-1])
    eo = dev(np.concatenate([[0], np.cumsum((np.maximum(b, 4100) + 15) // 16 * 16)]).astype(np.int64))
    out = torch.empty(int(q["out_off"][-1]), dtype=torch.uint8, device="cuda")
    enc_out = torch.empty(int(eo[-1].item()), dtype=torch.uint8, device="cuda")
    scratch = torch.empty(codec.qpack_enc_scratch_size(NCONN, 4096, 64), dtype=torch.uint8, device="cuda")
    peers = dev(HE.qpack_peer_population(NCONN, CAPACITIES, BLOCKED, seed=29).view(np.uint8))
    same = np.zeros(NCONN, codec.QPACK_PEER)
    same["max_table_capacity"], same["max_blocked"] = 4096, 0xFFFFFFFF
    same = dev(same.view(np.uint8))
    kw = dict(max_blocked=1 << 20, server_off=q["server_off"], server_len=q["server_len"], in_size=int(q["data"].size),
              out=out, enc_out=enc_out, enc_out_off=eo, scratch=scratch, set_capacity=True, evict=args.evict)
    res = {}

    def uniform():
        res["u"] = codec.qpack_flatten_sessions(d, hd, rs, cf, nres, sid, oo, **kw)

    def mixed():
        res["m"] = codec.qpack_flatten_sessions(d, hd, rs, cf, nres, sid, oo, peers=peers, **kw)

    def same_settings():
        res["s"] = codec.qpack_flatten_sessions(d, hd, rs, cf, nres, sid, oo, peers=same, **kw)

    t = [BC.timed(torch, fn, steps=30, warmup=5)
         for fn in (uniform, mixed, same_settings, uniform, mixed, same_settings, uniform)]
    tu, tm, ts = t[0::3], t[1::3], t[2::3]
    for k in ("out_len", "header_len", "rstatus"):
        assert torch.equal(res["s"][k][:nres], res["u"][k][:nres]), k
    assert torch.equal(res["s"]["enc_out_len"][:NCONN], res["u"]["enc_out_len"][:NCONN])
    stat = lambda r: dict(ok_responses=int((r["rstatus"][:nres] == 0).sum().item()),  # noqa: E731
                          field_bytes=int(r["header_len"][:nres].to(torch.int64).sum().item()),
                          encoder_stream_bytes=int(r["enc_out_len"][:NCONN].to(torch.int64).sum().item()))
    line = json.dumps({"call": "hhuff_qpack_flatten_sessions_peers", "connections": NCONN, "responses": nres,
                       "header_table_size": 4096, "evict": bool(args.evict), "capacities": CAPACITIES, "blocked": BLOCKED,
                       "uniform_ms": [round(x, 4) for x in tu], "uniform_spread_ms": round(max(tu) - min(tu), 4),
                       "mixed_ms": [round(x, 4) for x in tm], "same_settings_ms": [round(x, 4) for x in ts],
                       "uniform": stat(res["u"]), "mixed": stat(res["m"])})
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
