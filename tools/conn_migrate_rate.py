"""What moving connections costs (include/hhuff.h (2i)): hhuff_conn_export plus hhuff_conn_import of 1,024 and of all
65,536 connections of a 65,536-slot scratch, per family at table size 4096, against a plain device-to-device copy
of the same slabs -- which is no migration (the slabs hold scratch-relative offsets and a fixed stride) and serves
only as the byte-moving floor.

The connections are the slots tests' sessions (tests/test_conn_slots_gpu.py: 4,096 connections, two steps, the
decoder sessions 256 with withheld encoder streams) tiled over the 65,536 slots through their own images.  HIP
events around each call, the median of 20 calls after 3 warm-ups.

    python tools/conn_migrate_rate.py [--out profiles/conn_migrate_rate.jsonl]

One JSON line per family and count: size_ms (the img == NULL query), export_ms, import_ms, copy_ms, the images' mean
bytes per connection and their ratio to the slab.
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

NSLOTS, BASE, TABLE = 65536, 4096, 4096


def i32(torch, a):
    return torch.from_numpy(np.asarray(a, np.uint32).view(np.int32).copy()).cuda()


def base_scratch(torch, C, kind):
    """-> (family, scratch of `n` connections after two steps of the slots tests' traffic, n)"""
    import test_conn_slots_gpu as T

    if kind == "dsession":
        import qpdec_session_model as DM
        import test_qpdec_sessions as QT
        from oracle import oracle as O

        n = 256
        g = QT.Gpu(torch, n, 100)

        def replay(k, st, sid, kw, want):
            if k < 2:
                g.step(st, sid, **kw)
        QT.withheld_sessions(n, 11, False, DM.Model(O.oracle(), n, QT.H, 100), replay)
        return C.conn_family(C.FAM_QPACK_DSESSION, max_blocked=100), g._state().clone(), n
    fam = {"requests": C.conn_family(C.FAM_HPACK_DEC, TABLE), "qpack_req": C.conn_family(C.FAM_QPACK_DEC, TABLE),
           "hpenc": C.conn_family(C.FAM_HPACK_ENC), "qpenc_evict": C.conn_family(C.FAM_QPACK_ENC, TABLE, T.MAX_INFLIGHT)}[kind]
    if kind == "requests":  # (at least a block a connection: the generator's mutations want one)
        import slots_plan as SP
        from h2o_amd import hpack_synth as HS

        dense = SP.hpack_session(HS.make_connections(BASE, (1, 3 * T.STEPS), seed=16, request_frac=0.2), T.STEPS, 16)
    else:
        dense = T.dense_session(kind, BASE)
    scr = torch.zeros(BASE * C.conn_slab_size(fam), dtype=torch.uint8, device="cuda")
    res = []
    for k in range(2):
        if kind == "qpenc_evict" and k:
            dense[k] = T.with_acks(dense[k], dense[k - 1], res[k - 1])
        res.append(T.call(torch, kind, dense[k], scr, T.CONT if k else 0, None))
    return fam, scr, BASE


def line(torch, C, BC, kind):
    fam, base, nbase = base_scratch(torch, C, kind)
    slab = C.conn_slab_size(fam)
    # tile the base connections over all slots through their images
    src = torch.zeros(NSLOTS * slab, dtype=torch.uint8, device="cuda")
    img, off, ln, st = C.conn_export(fam, base, nbase, i32(torch, np.arange(nbase)))
    assert not st.any()
    for t in range(NSLOTS // nbase):
        assert not C.conn_import(fam, src, NSLOTS, i32(torch, t * nbase + np.arange(nbase)), img, off, ln).any()
    del base, img
    dst = torch.zeros(NSLOTS * slab, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(2)
    out = []
    for n in (1024, NSLOTS):
        a, b = rng.permutation(NSLOTS)[:n], rng.permutation(NSLOTS)[:n]
        sa, sb = i32(torch, a), i32(torch, b)
        img, off, ln, st = C.conn_export(fam, src, NSLOTS, sa)
        assert not st.any() and not C.conn_import(fam, dst, NSLOTS, sb, img, off, ln).any()
        L = C.lib()
        import ctypes

        status = torch.empty(n, dtype=torch.int32, device="cuda")
        ln2 = torch.empty(n, dtype=torch.int32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        f = ctypes.byref(fam)

        def size():
            L.hhuff_conn_export(f, src.data_ptr(), src.numel(), NSLOTS, sa.data_ptr(), n, None, None, ln2.data_ptr(), status.data_ptr(), s)

        def export():
            L.hhuff_conn_export(f, src.data_ptr(), src.numel(), NSLOTS, sa.data_ptr(), n, img.data_ptr(), off.data_ptr(),
                                ln2.data_ptr(), status.data_ptr(), s)

        def imp():
            L.hhuff_conn_import(f, dst.data_ptr(), dst.numel(), NSLOTS, sb.data_ptr(), n, img.data_ptr(), off.data_ptr(),
                                ln.data_ptr(), status.data_ptr(), s)
        ia, ib = torch.from_numpy(a.astype(np.int64)).cuda(), torch.from_numpy(b.astype(np.int64)).cuda()
        s2, d2 = src.view(NSLOTS, slab), dst.view(NSLOTS, slab)

        def copy():
            if n == NSLOTS:
                dst.copy_(src)
            else:
                d2[ib] = s2[ia]
        t = {k: BC.timed(torch, fn, steps=20, warmup=3) for k, fn in (("size", size), ("export", export), ("import", imp), ("copy", copy))}
        total = int((ln.to(torch.int64) & 0xFFFFFFFF).sum().item())
        out.append({"family": kind, "slots": NSLOTS, "moved": n, "slab_bytes": slab, "image_bytes_per_conn": round(total / n, 1),
                    "image_to_slab": round(total / n / slab, 4), "size_ms": round(t["size"], 4), "export_ms": round(t["export"], 4),
                    "import_ms": round(t["import"], 4), "copy_ms": round(t["copy"], 4)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    args = ap.parse_args()
    import torch

    import bench_configs as BC
    from h2o_amd import codec

    torch.cuda.set_device(0)
    for kind in ("requests", "qpack_req", "hpenc", "qpenc_evict", "dsession"):
        for rec in line(torch, codec, BC, kind):
            text = json.dumps(rec)
            print(text, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(text + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
