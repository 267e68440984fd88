"""What hhuff_h2_bodies costs (include/hhuff.h (2k'''')): 256 MiB of DATA payload, lying in the receive buffer behind
9-byte frame headers, gathered into per-stream runs in three shapes
  one          one connection x one stream in 16 KiB frames (16,384 frames, one run)
  interleaved  1,024 connections x 4 streams x four 16 KiB frames, the streams' frames interleaved (4 runs a connection)
  small        65,536 connections x one 4 KiB frame
and a fourth, `interleaved_4096`: the interleaved shape with 4,096 connections, which is 1 GiB of payload
and, on the same bytes and buffers, two yardsticks:
  memcpy    a device-to-device hipMemcpyAsync of as many bytes as the payload: the bytes moved once, no frames
  gather    frm_gather_kernel (h2o_amd/csrc/hhuff_gather.h, through tools/h2_data_gather.hip) given one job per frame with
            the places the call computes: the copy alone, one job a slot, no plan
HIP events around each call, the median of 30 calls after 5 warm-ups (deframe_rate.py's `timed`).  Every timed call
works on the next of several separate sets of the buffers it touches, sized so that a turn is at least twice the
256 MB Infinity Cache: no call finds lines an earlier call left in a cache.

    python tools/h2_bodies_rate.py [--bytes 268435456] [--out profiles/h2_bodies_rate.jsonl] [--tag NAME]

One JSON line per shape.  --dry builds the records and prints the sizes without a GPU.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import deframe_rate as DR  # noqa: E402
import h2_data_rate as HD  # noqa: E402

M = 16384


def shape(name, total):
    """-> dict(nconn, frm_cap, sev (H2_SEV_DTYPE), ctl (H2_CTL_DTYPE), frm_first, nstr, out_off, jobs (uint32 [frames, 4]: one
    gather job per frame, at the place the call gives it), in_size, payload)"""
    from h2o_amd import codec as C

    per, nstreams, each = {"one": (M, 1, total // M), "interleaved": (M, 4, 4), "interleaved_4096": (M, 4, 4), "small": (4096, 1, 1)}[name]
    slots = nstreams * each  # a connection's frames: frame k of stream s is slot nstreams * k + s
    nconn = 4096 if name == "interleaved_4096" else max(1, total // (per * slots))
    n = nconn * slots
    i = np.arange(n, dtype=np.uint64)
    s, k = (i % slots) % nstreams, (i % slots) // nstreams
    sev, ctl = np.zeros(n, C.H2_SEV_DTYPE), np.zeros(n, C.H2_CTL_DTYPE)
    sev["stream_id"], sev["a"], sev["flags"] = 1 + 2 * s, per, C.H2SE_BODY
    ctl["a"] = i * (per + 9) + 9
    room = slots * per
    jobs = np.zeros((n, 4), np.uint32)
    jobs[:, 0], jobs[:, 1], jobs[:, 2] = ctl["a"], (i // slots) * room + (s * each + k) * per, per
    edges = lambda step: (np.arange(nconn + 1, dtype=np.uint64) * step).astype(np.uint32)  # noqa: E731
    return dict(nconn=nconn, frm_cap=n, sev=sev, ctl=ctl, frm_first=edges(slots), nstr=np.full(nconn, slots, np.uint32),
                out_off=edges(room), jobs=jobs, in_size=n * (per + 9), payload=n * per, runs=nconn * nstreams)


def device_sets(torch, s, rot):
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()  # noqa: E731
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device="cuda")  # noqa: E731
    sets = []
    for r in range(rot):
        g = torch.Generator(device="cuda").manual_seed(r)
        data = torch.randint(0, 256, (s["in_size"],), dtype=torch.uint8, device="cuda", generator=g)
        sets.append(dict(data=data, sev=dev(s["sev"]), ctl=dev(s["ctl"]), frm_first=dev(s["frm_first"]).view(torch.int32),
                         nstr=dev(s["nstr"]).view(torch.int32), out_off=dev(s["out_off"]).view(torch.int32), jobs=dev(s["jobs"]),
                         out=dict(out=torch.zeros(s["payload"], dtype=torch.uint8, device="cuda"), nrun=i32(s["nconn"]),
                                  runs=torch.empty(32 * s["frm_cap"], dtype=torch.uint8, device="cuda"), out_len=i32(s["nconn"]),
                                  bstatus=i32(s["nconn"]))))
    return sets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="bodies")
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    total = a.bytes

    def emit(info):
        print(json.dumps(info), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(info) + "\n")

    if not a.dry:
        import torch

        from h2o_amd import codec

        hip = DR.hip_runtime()
        hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        stream = torch.cuda.current_stream().cuda_stream
        G = HD.gather_lib()
    for name in ("one", "interleaved", "small", "interleaved_4096"):
        s = shape(name, total)
        rot = max(2, -(-2 * DR.CACHE // (s["in_size"] + s["payload"])))
        info = {"call": "hhuff_h2_bodies", "tag": a.tag, "config": name, "connections": s["nconn"], "frames": s["frm_cap"],
                "runs": s["runs"], "payload_bytes": s["payload"], "in_bytes": s["in_size"], "rotated_sets": rot}
        if a.dry:
            emit(info)
            continue
        sets = device_sets(torch, s, rot)

        def bodies(i):
            d = sets[i % rot]
            codec.h2_bodies(d["data"], d["ctl"], d["sev"], d["frm_first"], s["frm_cap"], d["nstr"], d["out_off"], in_size=s["in_size"],
                            out_size=s["payload"], out=d["out"])

        def memcpy(i):
            d = sets[i % rot]
            assert hip.hipMemcpyAsync(d["out"]["out"].data_ptr(), d["data"].data_ptr(), s["payload"], 3, stream) == 0

        def gather(i):
            d = sets[i % rot]
            assert G.h2_data_gather(d["data"].data_ptr(), d["out"]["out"].data_ptr(), d["jobs"].data_ptr(), s["frm_cap"], stream) == 0

        t_mem = DR.timed(torch, memcpy)
        t_gat = DR.timed(torch, gather)
        for d in sets:
            d["out"]["out"].zero_()
        t_bod = DR.timed(torch, bodies)  # last, on cleared regions: its bytes stay for the checks
        torch.cuda.synchronize()
        d = sets[0]
        assert bool((d["out"]["bstatus"] == 0).all()) and int(d["out"]["out_len"].to(torch.int64).sum().item()) == s["payload"]
        assert int(d["out"]["nrun"].to(torch.int64).sum().item()) == s["runs"]
        j = s["jobs"]
        for f in (0, 1, len(j) // 2, len(j) - 1):  # the call put the payloads where the gather's jobs have them
            src, dst, n = int(j[f, 0]), int(j[f, 1]), int(j[f, 2])
            assert torch.equal(d["out"]["out"][dst:dst + n], d["data"][src:src + n]), f
        gbs = lambda ms: round(2 * s["payload"] / (ms * 1e-3) / 1e9, 1)  # noqa: E731  (read + written)
        info.update({"bodies_ms": round(t_bod, 4), "memcpy_ms": round(t_mem, 4), "gather_ms": round(t_gat, 4),
                     "bodies_over_memcpy": round(t_bod / t_mem, 4), "bodies_over_gather": round(t_bod / t_gat, 4),
                     "bodies_GBps": gbs(t_bod), "memcpy_GBps": gbs(t_mem), "gather_GBps": gbs(t_gat)})
        emit(info)
        del sets


if __name__ == "__main__":
    main()
