"""What hhuff_h3_bodies and hhuff_h3_frame_data cost (include/hhuff.h (2l'), (2l'')): 256 MiB of DATA payload in three
shapes -- the siblings' (tools/h2_bodies_rate.py, h2_data_rate.py)
  wide   4,096 streams x four 16 KiB frames
  small  65,536 streams x one 4 KiB frame
  one    one stream x 16,384 frames of 16 KiB: the shape the lane-per-slot plan exists for
On the receive side the payloads lie in the buffer behind their frame headers (3 or 5 bytes) and are gathered into
per-stream runs; on the send side the same payloads, contiguous, get their headers.  Beside them, on the same bytes and
buffers, two yardsticks:
  memcpy    a device-to-device hipMemcpyAsync of as many bytes as the payload
  gather    frm_gather_kernel (h2o_amd/csrc/hhuff_gather.h, through tools/h2_data_gather.hip) given one job per frame with the
            places the receive call computes: the copy alone, no plan
HIP events around each call, the median of 30 calls after 5 warm-ups (deframe_rate.py's `timed`).  Every timed call works
on the next of several separate sets of the buffers it touches, sized so that a turn is at least twice the 256 MB Infinity
Cache: no call finds lines an earlier call left in a cache.

    python tools/h3_bodies_rate.py [--bytes 268435456] [--out profiles/h3_bodies_rate.jsonl] [--tag NAME]

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


def shape(name, total):
    """-> dict(nstr, frm_cap, frames (H3_FRAME_DTYPE), nframes, frm_first, sends (H3_SEND_DTYPE), jobs (uint32 [frames, 4]:
    one gather job per frame, at the place the receive call gives it), in_size, payload, framed)"""
    from h2o_amd import codec as C

    per, each = {"wide": (16384, 4), "small": (4096, 1), "one": (16384, total // 16384)}[name]
    n = total // per
    nstr, hdr = n // each, 3 if per < 16384 else 5
    i = np.arange(n, dtype=np.uint64)
    frames, sends = np.zeros(n, C.H3_FRAME_DTYPE), np.zeros(n, C.H3_SEND_DTYPE)
    frames["hdr_off"], frames["payload_off"], frames["length"], frames["avail"] = i * (per + hdr), i * (per + hdr) + hdr, per, per
    sends["body_off"], sends["body_len"] = i * per, per
    jobs = np.zeros((n, 4), np.uint32)
    jobs[:, 0], jobs[:, 1], jobs[:, 2] = frames["payload_off"], i * per, per
    return dict(nstr=nstr, frm_cap=n, frames=frames, nframes=np.full(nstr, each, np.uint32), sends=sends, jobs=jobs,
                frm_first=(np.arange(nstr + 1, dtype=np.uint64) * each).astype(np.uint32), in_size=n * (per + hdr), payload=n * per,
                framed=n * (per + hdr))


def device_sets(torch, s, rot):
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()  # noqa: E731
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8, device="cuda")  # noqa: E731
    sets = []
    for r in range(rot):
        g = torch.Generator(device="cuda").manual_seed(r)
        data = torch.randint(0, 256, (s["in_size"],), dtype=torch.uint8, device="cuda", generator=g)
        sets.append(dict(data=data, frames=dev(s["frames"]), nframes=dev(s["nframes"]).view(torch.int32),
                         frm_first=dev(s["frm_first"]).view(torch.int32), sends=dev(s["sends"]), jobs=dev(s["jobs"]),
                         recv=dict(out=u8(s["payload"]), runs=u8(32 * s["nstr"]), totals=torch.zeros(2, dtype=torch.int32, device="cuda")),
                         send=dict(out=u8(s["framed"]), frm_off=torch.zeros(s["frm_cap"] + 1, dtype=torch.int32, device="cuda"),
                                   sstatus=torch.zeros(s["frm_cap"], dtype=torch.int32, device="cuda"))))
    return sets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="h3_bodies")
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()

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
    for name in ("wide", "small", "one"):
        s = shape(name, a.bytes)
        rot = max(2, -(-2 * DR.CACHE // (s["in_size"] + s["payload"])))
        info = {"call": "hhuff_h3_bodies / hhuff_h3_frame_data", "tag": a.tag, "config": name, "streams": s["nstr"], "frames": s["frm_cap"],
                "payload_bytes": s["payload"], "in_bytes": s["in_size"], "rotated_sets": rot}
        if a.dry:
            emit(info)
            continue
        sets = device_sets(torch, s, rot)

        def bodies(i):
            d = sets[i % rot]
            codec.h3_bodies(d["data"], d["frames"], d["nframes"], d["frm_first"], s["frm_cap"], in_size=s["in_size"], out_size=s["payload"],
                            out=d["recv"])

        def frame_data(i):  # the body: what the receive side gathered
            d = sets[i % rot]
            codec.h3_frame_data(d["recv"]["out"], d["sends"], body_size=s["payload"], nsend=s["frm_cap"], out_size=s["framed"], out=d["send"])

        def memcpy(i):
            d = sets[i % rot]
            assert hip.hipMemcpyAsync(d["recv"]["out"].data_ptr(), d["data"].data_ptr(), s["payload"], 3, stream) == 0

        def gather(i):
            d = sets[i % rot]
            assert G.h2_data_gather(d["data"].data_ptr(), d["recv"]["out"].data_ptr(), d["jobs"].data_ptr(), s["frm_cap"], stream) == 0

        t_mem = DR.timed(torch, memcpy)
        t_gat = DR.timed(torch, gather)
        for d in sets:
            d["recv"]["out"].zero_()
        t_bod = DR.timed(torch, bodies)  # on cleared buffers: its bytes stay for the checks and are the send side's body
        t_snd = DR.timed(torch, frame_data)
        torch.cuda.synchronize()
        d = sets[0]
        runs = d["recv"]["runs"].cpu().numpy().view(codec.H3_BODY_RUN_DTYPE)
        assert (runs["status"] == 0).all() and int(runs["len"].astype(np.uint64).sum()) == s["payload"]
        assert d["recv"]["totals"].tolist() == [s["payload"], s["frm_cap"]] and bool((d["send"]["sstatus"] == 0).all())
        per, hdr = int(s["sends"]["body_len"][0]), int(s["frames"]["payload_off"][0])
        head = torch.tensor(list(b"\x00" + ((per | (1 << 14 if hdr == 3 else 2 << 30)).to_bytes(hdr - 1, "big"))), dtype=torch.uint8).cuda()
        for f in (0, 1, s["frm_cap"] // 2, s["frm_cap"] - 1):  # the payloads where the gather's jobs have them; the frames framed
            src, dst = int(s["jobs"][f, 0]), int(s["jobs"][f, 1])
            assert torch.equal(d["recv"]["out"][dst:dst + per], d["data"][src:src + per]), f
            at = int(d["send"]["frm_off"][f])
            assert at == f * (per + hdr) and torch.equal(d["send"]["out"][at:at + hdr], head), f
            assert torch.equal(d["send"]["out"][at + hdr:at + hdr + per], d["recv"]["out"][dst:dst + per]), f
        gbs = lambda ms: round(2 * s["payload"] / (ms * 1e-3) / 1e9, 1)  # noqa: E731  (read + written)
        info.update({"bodies_ms": round(t_bod, 4), "frame_data_ms": round(t_snd, 4), "memcpy_ms": round(t_mem, 4),
                     "gather_ms": round(t_gat, 4), "bodies_over_memcpy": round(t_bod / t_mem, 4),
                     "frame_data_over_memcpy": round(t_snd / t_mem, 4), "bodies_over_gather": round(t_bod / t_gat, 4),
                     "bodies_GBps": gbs(t_bod), "frame_data_GBps": gbs(t_snd), "memcpy_GBps": gbs(t_mem), "gather_GBps": gbs(t_gat)})
        emit(info)
        del sets


if __name__ == "__main__":
    main()
