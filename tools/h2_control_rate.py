"""What hhuff_h2_control costs beside the calls it stands between (include/hhuff.h (2k')): tools/deframe_rate.py's
request batch of 65,536 connections, one header block a connection, in two shapes
  control   in front of the HEADERS frame one SETTINGS (two pairs), one WINDOW_UPDATE on stream 0 and one PING, behind
            it one to four DATA frames of 64 to 512 bytes
  upload    behind the HEADERS frame 64 DATA frames of 32 bytes, every eighth padded
Three device times per shape, on the same batch:
  control   hhuff_h2_control (server, recv_window_size = h2o's 16 MB, new connections)
  deframe   hhuff_h2_deframe, the yardstick: it reads every wire byte, the control call a few bytes a frame
  parse     hhuff_hpack_parse_requests on the de-framer's output
HIP events around each call, the median of 30 calls after 5 warm-ups (deframe_rate.py's `timed`).  Every timed call
works on the next of several separate copies of the buffers it touches; the rotation is sized from the bytes the
control call touches (a frame record's first half and a result record per frame, a sector per payload it reads, the
per-connection arrays and the replies), so that a turn is twice the 256 MB Infinity Cache, within --max-sets: no call
finds lines an earlier call left in a cache.

    python tools/h2_control_rate.py [--connections 65536] [--out profiles/h2_control_rate.jsonl] [--tag NAME]

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

import deframe_rate as DR  # noqa: E402

RWS = 16777216  # H2O_HTTP2_SETTINGS_HOST_CONNECTION_WINDOW_SIZE


def fr(typ, flags, sid, payload):
    return len(payload).to_bytes(3, "big") + bytes([typ, flags]) + sid.to_bytes(4, "big") + payload


def shape(blocks, name, seed):
    """-> (wire bytes, in_off, frames per connection, payloads the control call reads per connection)"""
    rng = np.random.default_rng(seed)
    out, nfr = [], []
    upload = b"".join(fr(0, 0x8 if k % 8 == 7 else 0, 1, (b"\x04" if k % 8 == 7 else b"d") + b"d" * 31) for k in range(64))
    for i, b in enumerate(blocks):
        head = fr(1, 0x4, 1, b)
        if name == "control":
            pre = fr(4, 0, 0, b"\x00\x01" + int(rng.choice([0, 256, 4096, 65536])).to_bytes(4, "big") + b"\x00\x04" +
                     int(rng.integers(65535, 1 << 20)).to_bytes(4, "big")) + \
                fr(8, 0, 0, int(rng.integers(1, 1 << 20)).to_bytes(4, "big")) + fr(6, 0, 0, i.to_bytes(8, "big"))
            k = int(rng.integers(1, 5))
            data = b"".join(fr(0, 0, 1, b"d" * int(rng.integers(64, 513))) for _ in range(k))
            out.append(pre + head + data)
            nfr.append(4 + k)
        else:
            out.append(head + upload)
            nfr.append(65)
    off = np.zeros(len(out) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in out])
    reads = 3 if name == "control" else 8
    return np.frombuffer(b"".join(out), np.uint8).copy(), off.astype(np.uint32), np.array(nfr, np.uint32), reads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--connections", type=int, default=65536)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="single_kernel")
    ap.add_argument("--max-sets", type=int, default=12)
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()

    from h2o_amd import hpack_synth as HS

    nconn = a.connections
    b = HS.make_connections(nconn, blocks_per_conn=(1, 1), seed=5, adversarial_frac=0.0)
    raw = b["data"].tobytes()
    blocks = [raw[int(b["blk_off"][i]):int(b["blk_off"][i + 1])] for i in range(nconn)]
    block_bytes = int(b["data"].size)
    if not a.dry:
        import torch

        from h2o_amd import codec

        L = codec.lib()
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()  # noqa: E731
        i32 = lambda n: torch.empty(max(1, n), dtype=torch.int32, device="cuda")  # noqa: E731
        u8 = lambda n: torch.empty(max(1, n), dtype=torch.uint8, device="cuda")  # noqa: E731
        stream = torch.cuda.current_stream().cuda_stream
    for name in ("control", "upload"):
        wire, in_off, nfr, reads = shape(blocks, name, seed=8)
        frm_first = np.zeros(nconn + 1, np.uint32)
        frm_first[1:] = np.cumsum(nfr, dtype=np.uint64)
        frm_cap, in_size = int(frm_first[-1]), int(wire.size)
        rep_off = (17 * frm_first.astype(np.uint64)).astype(np.uint32)  # hhuff_h2_control_reply_bound of the slots
        rep_size = int(rep_off[-1])
        touched_control = 32 * frm_cap + 32 * reads * nconn + (40 + 40 + 16 + 8 + 4) * nconn + 40 * nconn
        touched_deframe = in_size + block_bytes + 84 * frm_cap + 24 * nconn
        touched_decoder = 3 * block_bytes
        rot = min(a.max_sets, max(2, -(-2 * DR.CACHE // touched_control)))
        rot_dec = min(a.max_sets, max(2, -(-2 * DR.CACHE // touched_decoder)))
        arena_size = DR.ARENA_FIXED * (nconn + 1) + DR.ARENA_PER_BYTE * block_bytes
        info = {"call": "hhuff_h2_control", "tag": a.tag, "config": name, "connections": nconn, "frames": frm_cap, "wire_bytes": in_size,
                "block_bytes": block_bytes, "rotated_sets": rot, "decoder_sets": rot_dec,
                "touched_bytes": {"control": touched_control, "deframe": touched_deframe, "parse_at_least": touched_decoder}}
        if a.dry:
            print(json.dumps(info), flush=True)
            continue
        scratch_size = int(L.hhuff_hpack_scratch_size(nconn, 4096))
        sets, decs = [], []
        for _ in range(rot):
            s = dict(data=dev(wire), in_off=dev(in_off.view(np.int32)), frm_first=dev(frm_first.view(np.int32)),
                     rep_off=dev(rep_off.view(np.int32)), peers=codec.h2_new_peers(nconn, "cuda"))
            s["out"] = dict(frames=u8(32 * frm_cap), nframes=i32(nconn), consumed=i32(nconn), cstatus=i32(nconn), cerr=i32(nconn),
                            blk=u8(in_size), blk_off=i32(frm_cap + 1), conn_first=i32(nconn + 1), blocks=u8(32 * frm_cap),
                            totals=i32(2), arena_off=torch.empty(frm_cap + 1, dtype=torch.int64, device="cuda"))
            s["ctl"] = dict(ctl=u8(16 * frm_cap), nctl=i32(nconn), cstatus=i32(nconn), cerr=i32(nconn), rep_len=i32(nconn),
                            rep=u8(rep_size), peers=u8(40 * nconn))
            sets.append(s)
        for _ in range(rot_dec):
            decs.append(dict(dec=[u8(arena_size)] + [i32(block_bytes) for _ in range(4)] + [u8(block_bytes), i32(frm_cap), i32(frm_cap)],
                             req=i32(12 * frm_cap), scratch=u8(max(16, scratch_size))))

        def deframe(i):
            s = sets[i % rot]
            codec.h2_deframe(s["data"], s["in_off"], s["frm_first"], frm_cap, 16384, codec.H2O_MAX_REQLEN, 0, in_size=in_size,
                             arena_fixed=DR.ARENA_FIXED, arena_per_byte=DR.ARENA_PER_BYTE, out=s["out"])

        def control(i):
            s = sets[i % rot]
            codec.h2_control(s["data"], s["out"]["frames"], s["out"]["nframes"], s["frm_first"], frm_cap, s["peers"], s["rep_off"], 0,
                             RWS, in_size=in_size, rep_size=rep_size, out=s["ctl"])

        def parse(i):
            o, k = sets[i % rot]["out"], decs[i % rot_dec]
            d = k["dec"]
            p = lambda t: t.data_ptr()  # noqa: E731
            rc = L.hhuff_hpack_parse_requests(p(o["blk"]), block_bytes, p(o["blk_off"]), p(o["conn_first"]), nconn, 4096, p(d[0]),
                                              p(o["arena_off"]), p(d[1]), p(d[2]), p(d[3]), p(d[4]), p(d[5]), p(d[6]), p(d[7]),
                                              p(k["req"]), p(k["scratch"]), k["scratch"].numel(), 0, stream)
            assert rc == 0

        t_def = DR.timed(torch, deframe)
        for i in range(rot):  # every set de-framed: the input of the other two
            deframe(i)
        torch.cuda.synchronize()
        s0 = sets[0]
        assert s0["out"]["totals"].tolist() == [nconn, block_bytes] and bool((s0["out"]["cstatus"] == 0).all())
        assert bool((s0["out"]["nframes"] == s0["frm_first"][1:] - s0["frm_first"][:-1]).all())
        t_ctl = DR.timed(torch, control)
        torch.cuda.synchronize()
        c0 = s0["ctl"]
        assert bool((c0["cstatus"] == 0).all()) and bool((c0["nctl"] == s0["out"]["nframes"]).all())
        owed = int(c0["rep_len"].sum().item())
        # what the batch owes: the control shape a SETTINGS ACK and a PING ACK a connection, and the first DATA frame of a
        # new connection (65535 bytes of window against h2o's 16 MB) a WINDOW_UPDATE on both shapes
        assert owed == nconn * (13 + (26 if name == "control" else 0)), owed
        digest = int(c0["ctl"].view(torch.int32).to(torch.int64).sum().item()) & 0xFFFFFFFF
        t_par = DR.timed(torch, parse)
        torch.cuda.synchronize()
        assert bool((decs[0]["dec"][7][:nconn] == 0).all()), "a block failed h2o_hpack_parse_request"
        info.update({"control_ms": round(t_ctl, 4), "deframe_ms": round(t_def, 4), "parse_requests_ms": round(t_par, 4),
                     "control_over_deframe": round(t_ctl / t_def, 4), "control_over_parse": round(t_ctl / t_par, 4),
                     "frames_per_s": round(frm_cap / (t_ctl * 1e-3), 1), "reply_bytes": owed, "ctl_digest": digest})
        print(json.dumps(info), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(info) + "\n")
        del sets, decs


if __name__ == "__main__":
    main()
