"""What a CASPER step costs on the device (include/hhuff.h (2n)): 65,536 connections, max_keys 256, capacity_bits 13,
remainder_bits 6, three scripts, a connection each:
  full     INIT, one cookie of about 100 keys consumed, 8 marks of paths of about 40 bytes, the cookie out
  marks    the 8 marks alone, on the slabs `full` left (every key is present from the second call on: no insert)
  cookie   the cookie out alone
against a device-to-device copy of the bytes the call reads and writes (ops, results, strings, slab headers and keys
in and out, cookie bytes), and `full` against hhuff_cache_digests_load on a batch of digests of the same keys.
HIP events around each call: the median of 20 calls after 3 warm-ups, repeated 5 times; the line holds the median of
the five and their smallest and largest.  The slabs (135 MB) do not fit the last-level cache.

    python tools/casper_rate.py [--connections 65536] [--out profiles/casper_rate.jsonl]
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
REPEATS, MAX_KEYS, CAP, REM, NMARK = 5, 256, 13, 6, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--connections", type=int, default=65536)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import bench_configs as BC
    import casper_model as M
    import cdigest_model as CD
    from h2o_amd import codec as C

    assert torch.cuda.is_available(), "the rate tool needs an MI355X"
    n = a.connections
    dev = lambda x: torch.from_numpy(np.array(x)).cuda()  # noqa: E731
    rng = random.Random(5)
    pool = [sorted(rng.sample(range(1 << CAP), 100)) for _ in range(256)]
    cookies = [M.NAME + M.encode(k, REM) for k in pool]
    digests = [CD.gcs(CAP - REM, REM, k) for k in pool]
    paths = [b"/assets/app-%08x/bundle-%05d.min.js" % (i * 2654435761 % 2 ** 32, i % 99991) for i in range(NMARK * n)]
    strings = [cookies[c % 256] for c in range(n)] + paths
    off = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int64)
    data = dev(np.frombuffer(b"".join(strings) + b"\0" * 8, np.uint8))
    scratch = torch.zeros(C.casper_scratch_bytes(n, MAX_KEYS), dtype=torch.uint8, device="cuda")
    room = 512
    out = torch.empty(n * room, dtype=torch.uint8, device="cuda")
    out_off = dev((np.arange(n + 1, dtype=np.int64) * room).astype(np.int32))

    def script(kinds):
        ops = np.zeros((n, len(kinds)), C.CSP_OP_DTYPE)
        marks = 0
        for j, kind in enumerate(kinds):
            ops["kind"][:, j] = kind
            if kind == M.INIT:
                ops["a"][:, j], ops["b"][:, j] = CAP, REM
            elif kind == M.CONSUME:
                ops["a"][:, j], ops["b"][:, j] = off[:n], np.diff(off)[:n]
            elif kind == M.MARK:
                s = n + NMARK * np.arange(n) + marks
                ops["a"][:, j], ops["b"][:, j] = off[s], np.diff(off)[s]
                marks += 1
        return dev(ops.reshape(-1).view(np.uint8)), dev((np.arange(n + 1, dtype=np.int64) * len(kinds)).astype(np.int32))

    def measure(fn):
        t = sorted(BC.timed(torch, fn, steps=20, warmup=3) for _ in range(REPEATS))
        return t[REPEATS // 2], t[0], t[-1]

    lines, t_full = [], None
    for name, kinds in (("full", [M.INIT, M.CONSUME] + [M.MARK] * NMARK + [M.COOKIE]), ("marks", [M.MARK] * NMARK), ("cookie", [M.COOKIE])):
        ops, first = script(kinds)
        res = torch.empty(ops.numel(), dtype=torch.uint8, device="cuda")
        step = lambda: C.casper_step(scratch, n, MAX_KEYS, ops, first, data, out, out_off, res=res)  # noqa: E731
        t = measure(step)
        r = res.cpu().numpy().view(C.CSP_RESULT_DTYPE).reshape(n, len(kinds))
        assert (r["status"] == 0).all(), "an op failed"
        nkeys, cookie_bytes = r["nkeys"][:, -1].astype(np.int64), int(r["value"][:, -1].sum()) if kinds[-1] == M.COOKIE else 0
        in_bytes = (int(np.diff(off)[:n].sum()) if M.CONSUME in kinds else 0) + (int(np.diff(off)[n:].sum()) if M.MARK in kinds else 0)
        slab = int((16 + 8 * nkeys).sum())
        moved = 32 * ops.numel() // 16 + in_bytes + cookie_bytes + slab * (2 if name == "full" else 1)
        src = torch.empty(max(moved // 2, 1), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        t_copy = measure(lambda: dst.copy_(src))
        del src, dst
        lines.append({"call": "hhuff_casper_step", "script": name, "connections": n, "ops": len(kinds) * n, "max_keys": MAX_KEYS,
                      "keys_a_connection": round(float(nkeys.mean()), 1), "cookie_bytes": cookie_bytes, "bytes_moved": moved,
                      "step_ms": round(t[0], 4), "step_ms_min_max": [round(t[1], 4), round(t[2], 4)], "runs": REPEATS, "calls_a_run": 20,
                      "copy_of_moved_bytes_ms": round(t_copy[0], 4), "times_the_copy": round(t[0] / t_copy[0], 2),
                      "connections_per_s": round(n / (t[0] * 1e-3), 1)})
        t_full = t_full or t[0]
    # the yardstick of (2m): the same keys as `cache-digest` values, one a request
    doff = np.concatenate([[0], np.cumsum([len(digests[c % 256]) for c in range(n)])]).astype(np.int64)
    dd = dev(np.frombuffer(b"".join(digests[c % 256] for c in range(n)) + b"\0" * 8, np.uint8))
    dig_off = dev(np.arange(n + 1, dtype=np.int64) * 848)
    dig = torch.empty(n * 848, dtype=torch.uint8, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    vo, vl, first = dev(doff[:-1].astype(np.int32)), dev(np.diff(doff).astype(np.int32)), dev(np.arange(n + 1, dtype=np.int32))
    t = measure(lambda: C.cache_digests_load(dd, vo, vl, first, dig_off, dig=dig, status=status))
    assert int((status != 0).sum().item()) == 0
    lines.append({"call": "hhuff_cache_digests_load", "requests": n, "keys_a_request": 100, "value_bytes": int(doff[-1]),
                  "load_ms": round(t[0], 4), "load_ms_min_max": [round(t[1], 4), round(t[2], 4)], "runs": REPEATS, "calls_a_run": 20,
                  "full_step_over_load": round(t_full / t[0], 2)})
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
