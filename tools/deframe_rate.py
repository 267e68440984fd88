"""What the HTTP/2 de-framer costs in front of the request decoder (include/hhuff.h (2k)): an hpack_synth request batch
of 65,536 connections, one header block a connection, framed as a HEADERS frame each ("headers") or with a quarter of
the blocks split into HEADERS + CONTINUATION at a random byte ("split").  Three device times per configuration:
  deframe   hhuff_h2_deframe
  parse     hhuff_hpack_parse_requests on its output, the step it precedes
  memcpy    hipMemcpyAsync device to device of the same number of block bytes: the gather's floor
HIP events around each call, the median of 30 calls after 5 warm-ups.  Every timed call works on the next of several
separate copies of the buffers it touches, and each of the two rotations is sized from the bytes ITS calls touch so
that a turn of the rotation is twice the 256 MB Infinity Cache: the de-framer and the copy (the wire bytes, blk, the
records and offsets: tens of MB a call) go round `rotated_sets` light sets, the decoder's arena, field arrays and
scratch (hundreds of MB allocated, written sparsely: counted at 3 B a block byte) round `decoder_sets`.  So no call finds lines an earlier call left in a cache; the
only memory a call shares with its predecessor is the de-framer's pooled workspace (16 bytes a frame slot, about 1 MB).

    python tools/deframe_rate.py [--connections 65536] [--out profiles/deframe_rate.jsonl]

One JSON line per configuration: the three times, deframe / parse and deframe / memcpy.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS, WARMUP = 30, 5
CACHE = 256 << 20
ARENA_FIXED, ARENA_PER_BYTE = 1024, 16  # the arena slices of tools/bench_configs.py blocks_line


def frame(blocks, split_frac, seed):
    """-> (wire bytes, in_off, frames per connection): block i as HEADERS on stream 1, END_STREAM | END_HEADERS"""
    rng = np.random.default_rng(seed)
    head = lambda n, t, f: n.to_bytes(3, "big") + bytes([t, f]) + b"\x00\x00\x00\x01"  # noqa: E731
    out, nfr = [], []
    for b in blocks:
        if len(b) > 1 and rng.random() < split_frac:
            k = int(rng.integers(1, len(b)))
            out.append(head(k, 1, 0x1) + b[:k] + head(len(b) - k, 9, 0x4) + b[k:])
            nfr.append(2)
        else:
            out.append(head(len(b), 1, 0x5) + b)
            nfr.append(1)
    off = np.zeros(len(out) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in out])
    return np.frombuffer(b"".join(out), np.uint8).copy(), off.astype(np.uint32), np.array(nfr, np.uint32)


def hip_runtime():
    """the HIP runtime this process has loaded already (by its path, so dlopen hands back the same library)"""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no libamdhip64 in this process")


def timed(torch, fn):
    for i in range(WARMUP):
        fn(i)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(WARMUP + i)
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--connections", type=int, default=65536)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from h2o_amd import codec
    from h2o_amd import hpack_synth as HS

    L = codec.lib()
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    nconn = a.connections
    b = HS.make_connections(nconn, blocks_per_conn=(1, 1), seed=5, adversarial_frac=0.0)
    raw = b["data"].tobytes()
    blocks = [raw[int(b["blk_off"][i]):int(b["blk_off"][i + 1])] for i in range(nconn)]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()  # noqa: E731
    i32 = lambda n: torch.empty(max(1, n), dtype=torch.int32, device="cuda")  # noqa: E731
    u8 = lambda n: torch.empty(max(1, n), dtype=torch.uint8, device="cuda")  # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    for name, split in (("headers", 0.0), ("split", 0.25)):
        wire, in_off, nfr = frame(blocks, split, seed=6)
        frm_first = np.zeros(nconn + 1, np.uint32)
        frm_first[1:] = np.cumsum(nfr, dtype=np.uint64)
        frm_cap, in_size, block_bytes = int(frm_first[-1]), int(wire.size), int(b["data"].size)
        scratch_size = int(L.hhuff_hpack_scratch_size(nconn, 4096))
        arena_size = ARENA_FIXED * frm_cap + ARENA_PER_BYTE * in_size
        # bytes a call touches: the copy the fewest (source and destination), the de-framer the wire, blk and its records
        touched_copy = 2 * block_bytes
        touched_deframe = in_size + block_bytes + 84 * frm_cap + 24 * nconn
        # the decoder's arrays span 17 B a block byte, the arena and the scratch, but a call writes them sparsely: count
        # only what it surely touches (blk, the decoded bytes and the field records, about 3 B a block byte)
        touched_decoder = 3 * block_bytes
        rot = max(2, -(-2 * CACHE // min(touched_copy, touched_deframe)))
        rot_dec = max(2, -(-2 * CACHE // touched_decoder))
        sets, decs = [], []
        for _ in range(rot):
            s = dict(data=dev(wire), in_off=dev(in_off.view(np.int32)), frm_first=dev(frm_first.view(np.int32)))
            s["out"] = dict(frames=u8(32 * frm_cap), nframes=i32(nconn), consumed=i32(nconn), cstatus=i32(nconn), cerr=i32(nconn),
                            blk=u8(in_size), blk_off=i32(frm_cap + 1), conn_first=i32(nconn + 1), blocks=u8(32 * frm_cap),
                            totals=i32(2), arena_off=torch.empty(frm_cap + 1, dtype=torch.int64, device="cuda"))
            s["copy"] = u8(block_bytes)
            sets.append(s)
        for _ in range(rot_dec):
            decs.append(dict(dec=[u8(arena_size)] + [i32(in_size) for _ in range(4)] + [u8(in_size), i32(frm_cap), i32(frm_cap)],
                             req=i32(12 * frm_cap), scratch=u8(max(16, scratch_size))))

        def deframe(i):
            s = sets[i % rot]
            codec.h2_deframe(s["data"], s["in_off"], s["frm_first"], frm_cap, 16384, codec.H2O_MAX_REQLEN, 0, in_size=in_size,
                             arena_fixed=ARENA_FIXED, arena_per_byte=ARENA_PER_BYTE, out=s["out"])

        def parse(i):
            o, k = sets[i % rot]["out"], decs[i % rot_dec]
            d = k["dec"]
            p = lambda t: t.data_ptr()  # noqa: E731
            rc = L.hhuff_hpack_parse_requests(p(o["blk"]), in_size, p(o["blk_off"]), p(o["conn_first"]), nconn, 4096, p(d[0]),
                                              p(o["arena_off"]), p(d[1]), p(d[2]), p(d[3]), p(d[4]), p(d[5]), p(d[6]), p(d[7]),
                                              p(k["req"]), p(k["scratch"]), k["scratch"].numel(), 0, stream)
            assert rc == 0

        def memcpy(i):
            s = sets[i % rot]
            assert hip.hipMemcpyAsync(s["copy"].data_ptr(), s["out"]["blk"].data_ptr(), block_bytes, 3, stream) == 0  # D2D

        t_def = timed(torch, deframe)
        for i in range(rot):  # every set de-framed: the decoder's input
            deframe(i)
        torch.cuda.synchronize()
        s0 = sets[0]
        assert s0["out"]["totals"].tolist() == [nconn, block_bytes] and bool((s0["out"]["cstatus"] == 0).all())
        assert torch.equal(s0["out"]["blk"][:block_bytes], dev(b["data"]))
        t_par = timed(torch, parse)
        torch.cuda.synchronize()
        assert bool((decs[0]["dec"][7][:nconn] == 0).all()), "a block failed h2o_hpack_parse_request"
        t_cpy = timed(torch, memcpy)
        line = {"call": "hhuff_h2_deframe", "config": name, "connections": nconn, "frames": frm_cap, "wire_bytes": in_size,
                "block_bytes": block_bytes, "rotated_sets": rot, "decoder_sets": rot_dec,
                "touched_bytes": {"deframe": touched_deframe, "parse_at_least": touched_decoder, "memcpy": touched_copy}, "deframe_ms": round(t_def, 4), "parse_requests_ms": round(t_par, 4),
                "memcpy_d2d_ms": round(t_cpy, 4), "deframe_over_parse": round(t_def / t_par, 4),
                "deframe_over_memcpy": round(t_def / t_cpy, 2), "wire_bytes_per_s": round(in_size / (t_def * 1e-3), 1)}
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del sets, decs


if __name__ == "__main__":
    main()
