"""What token interning costs behind a decoder (include/hhuff.h (2j)): one batch of the shape bench.py --full uses for
its header-block key (tools/bench_configs.py blocks_line: 65,536 browser-like HTTP/2 connections), through
hhuff_hpack_parse_requests and then hhuff_intern_fields over its output with h2o's 85-name token set
(tests/golden/tokens.npz); and hhuff_intern_strings on the same names packed densely, which takes the slot mapping
(one lane per slot, most slots no field) out of the picture.  HIP events around each call, the median of 30 calls
after 5 warm-ups.

    python tools/intern_rate.py [--connections 65536] [--out profiles/intern_rate.jsonl]

One JSON line: fields per second, the intern pass as a share of the decode step, and the bytes the pass must move
(name bytes + 8 B of offset and length + 4 B of token per field) against the HBM peak.
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

HBM_PEAK = 8.0e12  # bytes / s, MI355X data sheet


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--connections", type=int, default=65536)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import bench_configs as BC
    import tokens_model as TM
    from h2o_amd import codec
    from h2o_amd import hpack_synth as HS

    fx = TM.load_fixture()
    ts = codec.TokenSet(fx["names"], TM.encoder_words(fx["flags"]))
    b = HS.make_connections(a.connections, seed=5, adversarial_frac=0.01)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()  # noqa: E731
    d, bo, cf = dev(b["data"]), dev(b["blk_off"].view(np.int32)), dev(b["conn_first"].view(np.int32))
    L = np.diff(b["blk_off"].astype(np.int64))
    ao = dev(np.concatenate([[0], np.cumsum(16 * L + 1024)]).astype(np.int64))  # as bench_configs.blocks_line
    nblk, nslots = len(b["blk_off"]) - 1, int(b["blk_off"][-1])
    res = {}

    def decode():
        res["q"] = codec.hpack_decode_blocks(d, bo, cf, 4096, arena_off=ao, in_size=int(b["data"].size), requests=True,
                                             scratch=res.get("scratch"))
        res["scratch"] = res["q"]["scratch"]

    t_dec = BC.timed(torch, decode, steps=30, warmup=5)
    q = res["q"]
    token = torch.full((nslots,), codec.TOK_NONE, dtype=torch.int32, device="cuda")
    user = torch.zeros(nslots, dtype=torch.int32, device="cuda")

    def fields():
        ts.intern_fields(q["arena"], q["name_off"], q["name_len"], bo, q["nfields"][:nblk], nslots, token=token, user_out=user)

    t_fld = BC.timed(torch, fields, steps=30, warmup=5)

    def fields_tokens_only():
        ts.intern_fields(q["arena"], q["name_off"], q["name_len"], bo, q["nfields"][:nblk], nslots, token=token,
                         want_user=False)

    t_fld1 = BC.timed(torch, fields_tokens_only, steps=30, warmup=5)

    # the same names packed densely: the field slots' offsets and lengths, one after the other
    nf_b = torch.minimum(q["nfields"][:nblk].to(torch.int64) & 0xFFFFFFFF, (bo[1:] - bo[:-1]).to(torch.int64))
    start = torch.cumsum(nf_b, 0) - nf_b
    nf = int(nf_b.sum().item())
    blk = torch.repeat_interleave(torch.arange(nblk, device="cuda"), nf_b)
    slot = bo[:-1].to(torch.int64)[blk] + (torch.arange(nf, device="cuda") - start[blk])
    off, length = q["name_off"][slot].contiguous(), q["name_len"][slot].contiguous()
    tok_d = torch.empty(nf, dtype=torch.int32, device="cuda")
    usr_d = torch.empty(nf, dtype=torch.int32, device="cuda")

    def strings():
        ts.intern_strings(q["arena"], off, length, nf, token=tok_d, user_out=usr_d)

    t_str = BC.timed(torch, strings, steps=30, warmup=5)
    torch.cuda.synchronize()
    assert torch.equal(token[slot], tok_d) and torch.equal(user[slot], usr_d)
    hits = int((tok_d >= 0).sum().item())
    name_bytes = int((length.to(torch.int64) & 0xFFFFFFFF).sum().item())
    moved = name_bytes + 12 * nf
    line = {"call": "hhuff_intern_fields", "connections": a.connections, "blocks": nblk, "slots": nslots, "fields": nf,
            "token_fields": hits, "name_bytes": name_bytes, "table_bytes": ts.size,
            "parse_requests_ms": round(t_dec, 4), "intern_fields_ms": round(t_fld, 4),
            "intern_fields_tokens_only_ms": round(t_fld1, 4), "intern_strings_dense_ms": round(t_str, 4),
            "fields_per_s": round(nf / (t_fld * 1e-3), 1), "dense_fields_per_s": round(nf / (t_str * 1e-3), 1),
            "share_of_decode_step": round(t_fld / t_dec, 4), "slot_mapping_ms": round(t_fld - t_str, 4),
            "bytes_moved": moved,
            "hbm_fraction": round(moved / (t_fld * 1e-3) / HBM_PEAK, 5),
            "dense_hbm_fraction": round(moved / (t_str * 1e-3) / HBM_PEAK, 5)}
    print(json.dumps(line))
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
