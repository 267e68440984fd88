"""What hhuff_h2_frame_data costs (include/hhuff.h (2k'')): 256 MiB of body bytes framed in three shapes
  small     65,536 connections x one record of 4 KiB (one frame each)
  frames    4,096 connections x four records of 16 KiB (one full frame each)
  one       one connection x one record of 256 MiB, windows to match (16,384 full frames)
and, on the same bytes and buffers, two yardsticks:
  memcpy    a device-to-device hipMemcpyAsync of the payload: the bytes moved once, no headers
  gather    frm_gather_kernel (h2o_amd/csrc/hhuff_gather.h, through tools/h2_data_gather.hip) given one job per frame:
            the de-framers' copy, which the framer's copy follows, placing the payloads where the frames have them
HIP events around each call, the median of 30 calls after 5 warm-ups (deframe_rate.py's `timed`).  Every timed call
works on the next of several separate sets of the buffers it touches, sized so that a turn is at least twice the
256 MB Infinity Cache: no call finds lines an earlier call left in a cache.

    python tools/h2_data_rate.py [--bytes 268435456] [--out profiles/h2_data_rate.jsonl] [--tag NAME]

One JSON line per shape.  --dry builds the records and prints the sizes without a GPU.

    rocprofv3 --kernel-trace -d DIR -o walk --output-format csv -- python tools/h2_data_rate.py --walk
    python tools/h2_data_rate.py --walk-csv DIR/.../walk_kernel_trace.csv [--out ...]

--walk makes ten calls on the `one` shape and ten on the same record cut to one frame by max_frames = 1, each behind
a 512 MB fill, so that both find their records in HBM and not in a cache the other's smaller copy left warm; --walk-csv
reads h2d_walk_kernel's durations out of the kernel trace of such a run: the walk is a closed form per record, so the
two must agree whatever the frame count.
"""
import argparse
import csv
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import deframe_rate as DR  # noqa: E402

M = 16384
GATHER_LIB = os.path.join(ROOT, "build", "libh2_data_gather.so")


def shape(name, total, max_frames=0):
    """-> dict(nconn, sends (H2_SEND_DTYPE), send_first, peers (H2_PEER_DTYPE), out_off, jobs (uint32 [nframes, 4]: one
    gather job per frame), out_size)"""
    from h2o_amd import codec as C

    per, nrec = {"small": (4096, 1), "frames": (M, 4), "one": (total, 1)}[name]
    nconn = max(1, total // (per * nrec))
    n = nconn * nrec
    sends = np.zeros(n, C.H2_SEND_DTYPE)
    sends["body_off"] = np.arange(n, dtype=np.uint64) * per
    sends["body_len"], sends["stream_id"], sends["flags"], sends["max_frames"] = per, 1 + 2 * (np.arange(n) % nrec), C.H2S_FINAL, max_frames
    sends["window"] = min(0x7FFFFFFF, max(1 << 20, per))
    peers = C.h2_new_peers(nconn)
    peers["send_window"] = min(0x7FFFFFFF, max(1 << 20, per * nrec))
    nfr = -(-per // M)
    room = nrec * (per + 9 * nfr) + 10
    out_off = (np.arange(nconn + 1, dtype=np.uint64) * room).astype(np.uint32)
    send_first = (np.arange(nconn + 1, dtype=np.uint64) * nrec).astype(np.uint32)
    # frame k of record r of connection c
    rec_out = (np.arange(n, dtype=np.uint64) // nrec) * room + (np.arange(n, dtype=np.uint64) % nrec) * (per + 9 * nfr)
    k = np.tile(np.arange(nfr, dtype=np.uint64), n)
    jobs = np.zeros((n * nfr, 4), np.uint32)
    jobs[:, 0] = np.repeat(sends["body_off"].astype(np.uint64), nfr) + k * M
    jobs[:, 1] = np.repeat(rec_out, nfr) + k * (M + 9) + 9
    jobs[:, 2] = np.minimum(M, per - k * M)
    return dict(nconn=nconn, nsend=n, sends=sends, send_first=send_first, peers=peers, out_off=out_off, jobs=jobs,
                out_size=int(nconn * room), frames=n * nfr, payload=n * per)


def gather_lib():
    src = os.path.join(ROOT, "tools", "h2_data_gather.hip")
    dep = os.path.join(ROOT, "h2o_amd", "csrc", "hhuff_gather.h")
    if not os.path.exists(GATHER_LIB) or os.path.getmtime(GATHER_LIB) < max(os.path.getmtime(src), os.path.getmtime(dep)):
        os.makedirs(os.path.dirname(GATHER_LIB), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "--offload-arch=" + os.environ.get("HHUFF_ARCH", "gfx950"),
                        "-std=c++17", "-fPIC", "-shared", "-Wno-unused-function", "-I" + os.path.join(ROOT, "h2o_amd", "csrc"), src, "-o",
                        GATHER_LIB], check=True)
    L = ctypes.CDLL(GATHER_LIB)
    L.h2_data_gather.restype = ctypes.c_int
    L.h2_data_gather.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32, ctypes.c_void_p]
    return L


def device_sets(torch, codec, s, total, rot):
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()  # noqa: E731
    i32 = lambda n: torch.empty(max(1, n), dtype=torch.int32, device="cuda")  # noqa: E731
    sets = []
    for r in range(rot):
        g = torch.Generator(device="cuda").manual_seed(r)
        body = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda", generator=g)
        sets.append(dict(body=body, sends=dev(s["sends"].view(np.uint8)), send_first=dev(s["send_first"].view(np.int32)),
                         peers=dev(s["peers"].view(np.uint8)), out_off=dev(s["out_off"].view(np.int32)), jobs=dev(s["jobs"].view(np.int32)),
                         out=dict(sent=torch.empty(24 * s["nsend"], dtype=torch.uint8, device="cuda"), out_len=i32(s["nconn"]),
                                  cstatus=i32(s["nconn"]), out=torch.zeros(s["out_size"], dtype=torch.uint8, device="cuda"),
                                  peers=torch.empty(40 * s["nconn"], dtype=torch.uint8, device="cuda"))))
    return sets


def call(codec, s, d, total):
    codec.h2_frame_data(d["body"], d["sends"], d["send_first"], d["peers"], d["out_off"], body_size=total, nsend=s["nsend"],
                        out_size=s["out_size"], out=d["out"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="frame_data")
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--walk", action="store_true")
    ap.add_argument("--walk-csv", default=None)
    a = ap.parse_args()
    total = a.bytes

    def emit(info):
        print(json.dumps(info), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(info) + "\n")

    if a.walk_csv:
        rows = [r for r in csv.DictReader(open(a.walk_csv)) if "h2d_walk_kernel" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
        assert len(us) == 2 * 2 * 13, len(us)  # two walks a call; 3 warm-ups and 10 calls for each of the two records
        calls = [us[i] + us[i + 1] for i in range(0, len(us), 2)]  # the counting and the placing walk of a call
        full, one = calls[3:13], calls[16:26]
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        emit({"call": "hhuff_h2_frame_data", "tag": a.tag, "config": "walk_alone", "bytes": total, "frames_full": -(-total // M),
              "walk_us_all_frames": {"median": round(med(full), 2), "min": round(min(full), 2), "max": round(max(full), 2)},
              "walk_us_max_frames_1": {"median": round(med(one), 2), "min": round(min(one), 2), "max": round(max(one), 2)}})
        return
    if not a.dry:
        import torch

        from h2o_amd import codec

        hip = DR.hip_runtime()
        hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        stream = torch.cuda.current_stream().cuda_stream
    if a.walk:
        flush = torch.empty(2 * DR.CACHE, dtype=torch.uint8, device="cuda")
        for mf in (0, 1):
            s = shape("one", total, mf)
            d = device_sets(torch, codec, s, total, 1)[0]
            for _ in range(13):
                flush.zero_()  # both records' walks start from cold caches (the full record's copy leaves them cold anyway)
                call(codec, s, d, total)
                torch.cuda.synchronize()
            assert int(d["out"]["sent"][:8].view(torch.int32)[1].item()) == (1 if mf else s["frames"])
        return
    G = None if a.dry else gather_lib()
    for name in ("small", "frames", "one"):
        s = shape(name, total)
        touched = s["payload"] + s["out_size"]
        rot = max(2, -(-2 * DR.CACHE // touched))
        info = {"call": "hhuff_h2_frame_data", "tag": a.tag, "config": name, "connections": s["nconn"], "records": s["nsend"],
                "frames": s["frames"], "payload_bytes": s["payload"], "out_bytes": s["payload"] + 9 * s["frames"], "rotated_sets": rot}
        if a.dry:
            emit(info)
            continue
        sets = device_sets(torch, codec, s, total, rot)

        def framer(i):
            call(codec, s, sets[i % rot], total)

        def memcpy(i):
            d = sets[i % rot]
            assert hip.hipMemcpyAsync(d["out"]["out"].data_ptr(), d["body"].data_ptr(), s["payload"], 3, stream) == 0

        def gather(i):
            d = sets[i % rot]
            assert G.h2_data_gather(d["body"].data_ptr(), d["out"]["out"].data_ptr(), d["jobs"].data_ptr(), s["frames"], stream) == 0

        t_mem = DR.timed(torch, memcpy)
        t_gat = DR.timed(torch, gather)
        t_frm = DR.timed(torch, framer)  # last: its bytes stay for the checks
        torch.cuda.synchronize()
        d = sets[0]
        assert bool((d["out"]["cstatus"] == 0).all()) and int(d["out"]["out_len"].to(torch.int64).sum().item()) == info["out_bytes"]
        j = s["jobs"]
        for f in (0, len(j) // 2, len(j) - 1):  # the gather wrote the payloads where the framer has them: a header in front
            src, dst, n = int(j[f, 0]), int(j[f, 1]), int(j[f, 2])
            assert torch.equal(d["out"]["out"][dst:dst + n], d["body"][src:src + n])
            assert d["out"]["out"][dst - 9:dst - 6].tolist() == list(n.to_bytes(3, "big"))
        gbs = lambda ms: round((s["payload"] + info["out_bytes"]) / (ms * 1e-3) / 1e9, 1)  # noqa: E731  (read + written)
        info.update({"frame_data_ms": round(t_frm, 4), "memcpy_ms": round(t_mem, 4), "gather_ms": round(t_gat, 4),
                     "frame_data_over_memcpy": round(t_frm / t_mem, 4), "frame_data_over_gather": round(t_frm / t_gat, 4),
                     "frame_data_GBps": gbs(t_frm), "memcpy_GBps": gbs(t_mem), "gather_GBps": gbs(t_gat)})
        emit(info)
        del sets


if __name__ == "__main__":
    main()
