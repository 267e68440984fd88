"""What moving HTTP/2 connections' stream tables costs (include/hhuff.h (2k'''), hhuff_h2_streams_export /
_import): export plus import of 1,024 and of all 65,536 connections of a 65,536-slot scratch with h2o's default
table (max_entries 117: 256 slots, 12,320 bytes a slab) and about 30 live streams each, against a plain
device-to-device copy of the same slabs -- which moves the bytes but can neither re-size the table nor leave the
scratch's stride, and serves only as the byte-moving floor.  Also the import into a scratch of max_entries 256, the
"scratch that grows" case.

The connections are 1,024 distinct tables of 20 to 40 streams (odd and even ids, mixed states and marks) tiled over
the slots through their own images.  HIP events around each call, the median of 20 calls after 3 warm-ups
(tools/bench_configs.py timed).

    python tools/h2_streams_image_rate.py [--out profiles/h2_streams_image_rate.jsonl]

One JSON line per count: size_ms (the img == NULL query), export_ms, import_ms, import_grow_ms, copy_ms, the images'
mean bytes per connection and their ratio to the slab.
"""
import argparse
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NSLOTS, BASE, ENTRIES, GROWN = 65536, 1024, 117, 256
ENTRY = np.dtype([("stream_id", "<u4"), ("state", "u1"), ("body", "u1"), ("flags", "u1"), ("rsv", "u1"), ("bytes_unnotified", "<u4"),
                  ("mark", "<u4"), ("output_window", "<i8"), ("input_window", "<i8"), ("received", "<u8"), ("content_length", "<u8")])


def i32(torch, a):
    return torch.from_numpy(np.asarray(a, np.uint32).view(np.int32).copy()).cuda()


def image(rng):
    """one connection's image: 20 to 40 streams out of the 200 ids behind a random first one"""
    count = int(rng.integers(20, 41))
    e = np.zeros(count, ENTRY)
    e["stream_id"] = np.sort(rng.choice(200, count, replace=False)) + 1 + 2 * int(rng.integers(0, 1 << 20))
    e["state"], e["body"], e["mark"] = rng.integers(0, 4, count), rng.integers(0, 4, count), rng.integers(0, 2, count)
    e["output_window"], e["input_window"], e["content_length"] = rng.integers(0, 1 << 20, count), 65535, 2**64 - 1
    total = 64 + 48 * count
    return (struct.pack("<IHH6I", 0x49434848, 1, 5, 0, 0, 0, total, 0, 0) +
            struct.pack("<8I", int(e["stream_id"][-1]), 0, count, 0, count, 0, 0, 0) + e.tobytes())


def lines(torch, C, BC):
    rng = np.random.default_rng(7)
    base = [image(rng) for _ in range(BASE)]
    off = np.concatenate([[0], np.cumsum([len(b) for b in base])]).astype(np.int64)
    d_img = torch.from_numpy(np.frombuffer(b"".join(base), np.uint8).copy()).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), i32(torch, [len(b) for b in base])
    slab = C.h2_streams_scratch_size(1, ENTRIES)
    src = torch.zeros(NSLOTS * slab, dtype=torch.uint8, device="cuda")
    for t in range(NSLOTS // BASE):
        assert not C.h2_streams_import(ENTRIES, src, NSLOTS, i32(torch, t * BASE + np.arange(BASE)), d_img, d_off, d_len).any()
    dst = torch.zeros(NSLOTS * slab, dtype=torch.uint8, device="cuda")
    grown = torch.zeros(C.h2_streams_scratch_size(NSLOTS, GROWN), dtype=torch.uint8, device="cuda")
    L, s = C.lib(), torch.cuda.current_stream().cuda_stream
    out = []
    for n in (1024, NSLOTS):
        a, b = rng.permutation(NSLOTS)[:n], rng.permutation(NSLOTS)[:n]
        sa, sb = i32(torch, a), i32(torch, b)
        img, ioff, ln, st = C.h2_streams_export(ENTRIES, src, NSLOTS, sa)
        assert not st.any() and not C.h2_streams_import(ENTRIES, dst, NSLOTS, sb, img, ioff, ln).any()
        assert not C.h2_streams_import(GROWN, grown, NSLOTS, sb, img, ioff, ln).any()
        status, ln2 = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))

        def size():
            L.hhuff_h2_streams_export(ENTRIES, src.data_ptr(), src.numel(), NSLOTS, sa.data_ptr(), n, None, None, ln2.data_ptr(),
                                      status.data_ptr(), s)

        def export():
            L.hhuff_h2_streams_export(ENTRIES, src.data_ptr(), src.numel(), NSLOTS, sa.data_ptr(), n, img.data_ptr(), ioff.data_ptr(),
                                      ln2.data_ptr(), status.data_ptr(), s)

        def imp():
            L.hhuff_h2_streams_import(ENTRIES, dst.data_ptr(), dst.numel(), NSLOTS, sb.data_ptr(), n, img.data_ptr(), ioff.data_ptr(),
                                      ln.data_ptr(), status.data_ptr(), s)

        def imp_grow():
            L.hhuff_h2_streams_import(GROWN, grown.data_ptr(), grown.numel(), NSLOTS, sb.data_ptr(), n, img.data_ptr(), ioff.data_ptr(),
                                      ln.data_ptr(), status.data_ptr(), s)
        ia, ib = torch.from_numpy(a.astype(np.int64)).cuda(), torch.from_numpy(b.astype(np.int64)).cuda()
        s2, d2 = src.view(NSLOTS, slab), dst.view(NSLOTS, slab)

        def copy():
            if n == NSLOTS:
                dst.copy_(src)
            else:
                d2[ib] = s2[ia]
        t = {k: BC.timed(torch, fn, steps=20, warmup=3)
             for k, fn in (("size", size), ("export", export), ("import", imp), ("import_grow", imp_grow), ("copy", copy))}
        assert not status.any()
        total = int(ln.to(torch.int64).sum().item())
        out.append({"max_entries": ENTRIES, "slots": NSLOTS, "moved": n, "slab_bytes": slab, "image_bytes_per_conn": round(total / n, 1),
                    "image_to_slab": round(total / n / slab, 4), "size_ms": round(t["size"], 4), "export_ms": round(t["export"], 4),
                    "import_ms": round(t["import"], 4), "import_grow_ms": round(t["import_grow"], 4), "grown_max_entries": GROWN,
                    "copy_ms": round(t["copy"], 4)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    args = ap.parse_args()
    import torch

    import bench_configs as BC
    from h2o_amd import codec

    torch.cuda.set_device(0)
    for rec in lines(torch, codec, BC):
        text = json.dumps(rec)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
