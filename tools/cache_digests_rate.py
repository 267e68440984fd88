"""What cache digests cost on the device (include/hhuff.h (2m)).
  load     65,536 requests with one `cache-digest` value of about 1 KB each (pbits 7, about 900 keys; 256 distinct
           digests, every request its own copy), and the same batch with 1,024 of the requests carrying one: against a
           device-to-device copy of the bytes the call reads and writes (values + images)
  lookup   8 queries a request (URLs of about 60 bytes in four segments) on the loaded images: against
           hhuff_hpack_parse_requests on a batch of as many browser-like connections (tools/bench_configs.py blocks_line)
HIP events around each call, the median of 20 calls after 3 warm-ups; the images (about 480 MB) do not fit the
last-level cache, so every call starts from HBM.

    python tools/cache_digests_rate.py [--requests 65536] [--out profiles/cache_digests_rate.jsonl]
"""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def digest_pool(n, nbytes=1024, pbits=7, seed=3):
    import cdigest_model as M

    rng, pool = random.Random(seed), []
    for _ in range(n):
        keys, k, bits = [], -1, 10
        while bits + 2 * pbits + 8 < 8 * nbytes:
            gap = rng.randrange(0, 3 << pbits)
            k, bits = k + 1 + gap, bits + (gap >> pbits) + 1 + pbits
            keys.append(k)
        pool.append((M.gcs(24, pbits, keys), len(keys)))
    return pool


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=65536)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import bench_configs as BC
    from h2o_amd import codec as C
    from h2o_amd import hpack_synth as HS

    assert torch.cuda.is_available(), "the rate tool needs an MI355X"
    n = a.requests
    dev = lambda x: torch.from_numpy(np.array(x)).cuda()  # noqa: E731
    pool = digest_pool(256)
    vals = [pool[r % len(pool)][0] + b"; complete" for r in range(n)]
    nkeys = np.array([pool[r % len(pool)][1] for r in range(n)], np.int64)
    off = np.concatenate([[0], np.cumsum([len(v) for v in vals])]).astype(np.int64)
    urls = [b"/assets/app-%08x/bundle-%05d.min.js" % (r * 2654435761 % 2 ** 32, r) for r in range(8 * n)]
    head = b"https" + b"://" + b"static.example.com"
    uoff = int(off[-1]) + len(head) + np.concatenate([[0], np.cumsum([len(u) for u in urls])]).astype(np.int64)
    data = dev(np.frombuffer(b"".join(vals) + head + b"".join(urls) + b"\0" * 8, np.uint8))
    val_off, val_len = dev(off[:-1].astype(np.int32)), dev(np.diff(off).astype(np.int32))
    room = (16 + 16 + 8 * nkeys + 15) & ~15  # (regions start 16-byte aligned)
    dig_off = dev(np.concatenate([[0], np.cumsum(room)]).astype(np.int64))
    dig = torch.empty(int(room.sum()), dtype=torch.uint8, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    lines = []
    for name, present in (("dense", n), ("sparse", min(1024, n))):
        has = np.zeros(n, np.int64)
        has[np.linspace(0, n - 1, present).astype(np.int64)] = 1
        # the values of the requests that carry one, in request order
        sel = np.flatnonzero(has)
        vo, vl, first = val_off[dev(sel)], val_len[dev(sel)], dev(np.concatenate([[0], np.cumsum(has)]).astype(np.int32))
        t = BC.timed(torch, lambda: C.cache_digests_load(data, vo, vl, first, dig_off, dig=dig, status=status), steps=20, warmup=3)
        assert int((status != 0).sum().item()) == 0
        moved = int(np.diff(off)[sel].sum() + room[sel].sum() + 16 * (n - present))
        src = torch.empty(max(moved // 2, 1), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        t_copy = BC.timed(torch, lambda: dst.copy_(src), steps=20, warmup=3)
        lines.append({"call": "hhuff_cache_digests_load", "batch": name, "requests": n, "with_digest": present,
                      "value_bytes": int(np.diff(off)[sel].sum()), "keys": int(nkeys[sel].sum()), "bytes_moved": moved,
                      "load_ms": round(t, 4), "copy_of_moved_bytes_ms": round(t_copy, 4), "times_the_copy": round(t / t_copy, 2),
                      "keys_per_s": round(nkeys[sel].sum() / (t * 1e-3), 1), "value_bytes_per_s": round(np.diff(off)[sel].sum() / (t * 1e-3), 1)})
        del src, dst
    # lookup on the dense images (loaded again: the sparse run emptied most)
    C.cache_digests_load(data, val_off, val_len, dev(np.arange(n + 1, dtype=np.int32)), dig_off, dig=dig, status=status)
    q = np.zeros(8 * n, C.CD_QUERY_DTYPE)
    q["req"] = np.arange(8 * n) // 8
    for k, (o, ln) in enumerate(((int(off[-1]), 5), (int(off[-1]) + 5, 3), (int(off[-1]) + 8, len(head) - 8))):
        q["off"][:, k], q["len"][:, k] = o, ln
    q["off"][:, 3], q["len"][:, 3] = uoff[:-1], np.diff(uoff)
    qd = dev(q.view(np.uint8))
    state = torch.empty(8 * n, dtype=torch.int32, device="cuda")
    t_look = BC.timed(torch, lambda: C.cache_digests_lookup(dig, dig_off, data, qd, state=state), steps=20, warmup=3)
    counts = torch.bincount(state + 400, minlength=403).cpu().numpy()
    assert counts[:400].sum() == 0, "a lookup failed"
    b = HS.make_connections(n, seed=5, adversarial_frac=0.01)
    d, bo, cf = dev(b["data"]), dev(b["blk_off"].view(np.int32)), dev(b["conn_first"].view(np.int32))
    ao = dev(np.concatenate([[0], np.cumsum(16 * np.diff(b["blk_off"].astype(np.int64)) + 1024)]).astype(np.int64))
    res = {}

    def decode():
        res["q"] = C.hpack_decode_blocks(d, bo, cf, 4096, arena_off=ao, in_size=int(b["data"].size), requests=True,
                                         scratch=res.get("scratch"))
        res["scratch"] = res["q"]["scratch"]

    t_dec = BC.timed(torch, decode, steps=20, warmup=3)
    lines.append({"call": "hhuff_cache_digests_lookup", "requests": n, "queries": 8 * n, "message_bytes": int(len(head) * 8 * n + uoff[-1] - uoff[0]),
                  "keys_a_frame": int(nkeys.mean()), "lookup_ms": round(t_look, 4), "queries_per_s": round(8 * n / (t_look * 1e-3), 1),
                  "states_unknown_notcached_fresh": counts[400:403].tolist(), "parse_requests_ms": round(t_dec, 4),
                  "share_of_decode_step": round(t_look / t_dec, 3)})
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
