"""HTTP/2 stream table images on the GPU (include/hhuff.h (2k'''), hhuff_h2_streams_export / _import,
h2o_amd/csrc/hhuff_h2simage.hip).  The image is canonical, so it is pinned by bytes -- images built here in numpy are
imported and must come back from export unchanged, at every table size around the two instantiations -- and by
behaviour: the corpus connections of tests/test_h2streams.py are moved between their steps into a scratch of another
max_entries and must go on exactly as the model's connection that never moved.  Every comparison is exact."""
import functools
import struct

import numpy as np
import pytest

import bounds_harness as BH
import h2streams_model as M
import test_conn_image_gpu as CI
import test_h2streams as TS
from h2o_amd import codec as C

pytestmark = pytest.mark.gpu
FILL = 0xC3
ENTRY = np.dtype([("stream_id", "<u4"), ("state", "u1"), ("body", "u1"), ("flags", "u1"), ("rsv", "u1"), ("bytes_unnotified", "<u4"),
                  ("mark", "<u4"), ("output_window", "<i8"), ("input_window", "<i8"), ("received", "<u8"), ("content_length", "<u8")])


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    return torch


def cap_of(m):
    return max(4, 1 << (2 * m - 1).bit_length())


@functools.lru_cache(maxsize=None)
def homes(cap):  # the table's hash (hhuff_h2streams.h home) of the ids 0 .. 2^23 - 1
    ids = np.arange(1 << 23, dtype=np.uint64)
    return (((ids * 0x9E3779B1) & 0xFFFFFFFF) >> 7) & (cap - 1)


def image(m, count, seed):
    """a valid image of `count` streams for a table of m: a third of the ids with the table's last slot as their home, a
    third sharing home 1, the rest anywhere; mixed states, marks and windows"""
    rng = np.random.default_rng(seed)
    h = homes(cap_of(m))
    chosen = set()
    for home in (cap_of(m) - 1, 1):
        chosen |= set(rng.choice(np.nonzero(h == home)[0][1:], count // 3, replace=False).tolist())
    while len(chosen) < count:
        chosen.add(int(rng.integers(1, 1 << 31)))
    ids = np.array(sorted(chosen), np.uint32)
    e = np.zeros(count, ENTRY)
    e["stream_id"], e["state"], e["body"], e["flags"] = ids, rng.integers(0, 4, count), rng.integers(0, 4, count), rng.integers(0, 16, count)
    e["mark"], e["bytes_unnotified"] = rng.integers(0, 2, count), rng.integers(0, 1 << 32, count)
    e["output_window"], e["input_window"] = rng.integers(-2**31 + 1, 2**31 - 1, (2, count))
    e["received"], e["content_length"] = rng.integers(0, 1 << 40, count), np.where(rng.integers(0, 2, count), np.uint64(2**64 - 1), np.uint64(77))
    total = 64 + 48 * count
    return (struct.pack("<IHH6I", 0x49434848, 1, 5, 0, 0, 0, total, 0, 0) + struct.pack("<8I", *rng.integers(0, 1 << 31, 4), count, 0, 0, 0) +
            e.tobytes())


def records(im):
    return np.frombuffer(im[64:], ENTRY)


def export(torch, m, scr, nslots, slot, room=None):
    """hhuff_h2_streams_export through the C ABI as CI.export does for the other families: the size query, then the images
    into regions of exactly their length (room(lens): other sizes) inside a guarded buffer"""
    L, n = C.lib(), len(slot)
    ds = CI.u32(torch, slot)
    ln, st = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    head = [m, scr.data_ptr(), scr.numel(), nslots, ds.data_ptr(), n]
    assert L.hhuff_h2_streams_export(*head, None, None, ln.data_ptr(), st.data_ptr(), CI._stream(torch)) == 0
    torch.cuda.synchronize()
    need, st0 = ln.cpu().numpy().view(np.uint32).copy(), st.cpu().numpy().copy()
    off = np.concatenate([[0], np.cumsum(need.astype(np.int64) if room is None else np.asarray(room(need), np.int64))]).astype(np.uint64)
    whole, img = BH.guarded(torch, int(off[-1]), CI.SENT)
    doff = torch.from_numpy(off.view(np.int64).copy()).cuda()
    assert L.hhuff_h2_streams_export(*head, img.data_ptr(), doff.data_ptr(), ln.data_ptr(), st.data_ptr(), CI._stream(torch)) == 0
    torch.cuda.synchronize()
    im = CI.Images(torch, whole, img, off, ln.cpu().numpy().view(np.uint32).copy(), st.cpu().numpy().copy())
    assert im.guards_ok() and (need == im.len).all() and ((st0 != 0) == (im.status == C.IMG_EINVAL)).all()
    return im


def put(torch, images, sizes=None):
    """the images back to back (sizes: other region sizes) -> (device bytes, img_off, img_len)"""
    sizes = [len(b) for b in images] if sizes is None else sizes
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    buf = np.full(max(16, int(off[-1])), 0xEE, np.uint8)
    for b, o, s in zip(images, off, sizes):
        buf[o:o + min(s, len(b))] = np.frombuffer(b, np.uint8)[:s]
    return torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda(), CI.u32(torch, [len(b) for b in images])


def imp(torch, m, scr, nslots, slot, images, sizes=None):
    st = C.h2_streams_import(m, scr, nslots, CI.u32(torch, slot), *put(torch, images, sizes))
    torch.cuda.synchronize()
    return st.cpu().numpy().tolist()


def scratch(torch, m, nslots, fill=FILL):
    return BH.guarded(torch, C.h2_streams_scratch_size(nslots, m), fill)


def slabs(scr, m, nslots):
    return scr.cpu().numpy().reshape(nslots, -1)


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("m", [1, 2, 32, 33, 256, 257, 512, 2048])
def test_canonical_round_trip(torch, m, n):
    images = [image(m, c, 100 * m + k) for k, c in enumerate([m, 0, 1, m, max(1, m // 2)][:n])]
    nslots = n + 2
    slot = np.random.default_rng(m).permutation(nslots)[:n]
    whole, scr = scratch(torch, m, nslots)
    assert imp(torch, m, scr, nslots, slot, images) == [0] * n
    first = slabs(scr, m, nslots).copy()
    out = export(torch, m, scr, nslots, slot)
    assert out.status.tolist() == [0] * n and [out.bytes(k) for k in range(n)] == images
    assert CI.T.guards_ok(whole) and (np.delete(first, slot, 0) == FILL).all(), "a guard or the slab of an unlisted slot was written"
    # equal images give equal slab bytes, whatever the slab held
    _, again = scratch(torch, m, nslots, 0x3C)
    assert imp(torch, m, again, nslots, slot, images) == [0] * n and (slabs(again, m, nslots)[slot] == first[slot]).all()
    # every stream is where hhuff_h2_streams_fill_sends looks for it, with its record's window
    ids = [records(im)["stream_id"].tolist() for im in images]
    got, _ = TS.windows(torch, dict(max_entries=m), scr, ids, C.ConnSlots(CI.u32(torch, slot), None, nslots))
    assert got == [[(int(w), 0) for w in records(im)["output_window"]] for im in images]


@pytest.mark.parametrize("m", [64, 256, 2048])
def test_across_table_sizes(torch, m):
    counts = [0, 30, 64, 65, 117]
    images = [image(117, c, c) for c in counts]
    _, src = scratch(torch, 117, 5)
    assert imp(torch, 117, src, 5, [4, 2, 0, 1, 3], images) == [0] * 5
    out = export(torch, 117, src, 5, [4, 2, 0, 1, 3])
    moved = [out.bytes(k) for k in range(5)]
    assert moved == images
    whole, dst = scratch(torch, m, 6)
    assert imp(torch, m, dst, 6, [5, 0, 3, 1, 2], moved) == [0 if c <= m else C.IMG_EPARAM for c in counts]
    fits = [k for k, c in enumerate(counts) if c <= m]
    back = export(torch, m, dst, 6, [[5, 0, 3, 1, 2][k] for k in fits])
    assert [back.bytes(i) for i in range(len(fits))] == [images[k] for k in fits] and CI.T.guards_ok(whole)
    refused = [[5, 0, 3, 1, 2][k] for k, c in enumerate(counts) if c > m] + [4]
    assert (slabs(dst, m, 6)[refused] == FILL).all(), "a refused item's slab was written"


# the groups of the corpus with second steps, cut between the steps; those that book sends there, between fill and commit too
MOVES = [(g, cut) for g in TS.by_params() for cut in ("step", "fill")
         if any(len(c["steps"]) == 2 and (cut == "step" or c["steps"][1].sends) for c in g)]


@pytest.mark.parametrize("cases, cut", MOVES, ids=lambda v: v if isinstance(v, str) else v[0]["name"])
def test_moved_connections_go_on_as_the_model(torch, cases, cut):
    """step 1 in scratch A; the connections with a second step move into other slots of B, of another max_entries, between
    the steps (cut "fill": between hhuff_h2_streams_fill_sends and _commit_sent); step 2 in B against the model"""
    P, n = cases[0]["P"], len(cases)
    second = [i for i, c in enumerate(cases) if len(c["steps"]) == 2][::-1]
    booked = [cases[i]["steps"][1].sends for i in second]
    PB, nb = dict(P, max_entries=P["max_entries"] + 6), len(second) + 3
    _, a = scratch(torch, P["max_entries"], n, TS.SENTINEL)
    whole, b = scratch(torch, PB["max_entries"], nb)
    conns = [M.new_conn() for _ in cases]
    step = lambda c, k: dict(frames=c["steps"][k].frames, blocks=c["steps"][k].blocks, ops=c["steps"][k].ops,  # noqa: E731
                             nctl=c["steps"][k].nctl, rep_cap=c["steps"][k].rep_cap)
    walks = [M.walk(conns[i], P, c["iws"][0], c["steps"][0].frames, c["steps"][0].blocks, c["steps"][0].ops, c["steps"][0].rep_cap,
                    c["steps"][0].nctl) for i, c in enumerate(cases)]
    arr, h = TS.streams_call(torch, P, a, [step(c, 0) for c in cases], [c["iws"][0] for c in cases], slack=1)
    TS.compare(arr, h, walks)
    to = np.random.default_rng(3).permutation(nb)[:len(second)]
    sa, sb = C.ConnSlots(CI.u32(torch, second), None, n), C.ConnSlots(CI.u32(torch, to), None, nb)

    def move():
        out = export(torch, P["max_entries"], a, n, second)
        assert not out.status.any() and imp(torch, PB["max_entries"], b, nb, to, [out.bytes(k) for k in range(len(second))]) == [0] * len(second)
        a.fill_(0x11)

    ids = [[s for s, _ in bk] for bk in booked]
    if cut == "step":
        move()
    if any(booked):
        _, d = TS.windows(torch, P if cut == "fill" else PB, a if cut == "fill" else b, ids, sa if cut == "fill" else sb)
    if cut == "fill":
        move()
    if any(booked):
        sent = np.zeros(sum(len(bk) for bk in booked), C.H2_SENT_DTYPE)
        sent["sent"] = [v for bk in booked for _, v in bk]
        first = np.concatenate([[0], np.cumsum([len(bk) for bk in booked])]).astype(np.uint32)
        C.h2_streams_commit_sent(PB["max_entries"], b, d, TS.dev(torch, sent), TS.dev(torch, first), slots=sb, nsend=int(first[-1]))
    walks2 = []
    for i in second:
        st = cases[i]["steps"][1]
        if st.sends:
            M.fill_sends(conns[i], [s for s, _ in st.sends])
            M.commit_sent(conns[i], [s for s, _ in st.sends], [v for _, v in st.sends])
        walks2.append(M.walk(conns[i], PB, cases[i]["iws"][1], st.frames, st.blocks, st.ops, st.rep_cap, st.nctl))
    arr, h = TS.streams_call(torch, PB, b, [step(cases[i], 1) for i in second], [cases[i]["iws"][1] for i in second], cont=True, slots=sb)
    TS.compare(arr, h, walks2)
    got, _ = TS.windows(torch, PB, b, [sorted(conns[i]["streams"]) + [0x7ffffff1] for i in second], sb)
    for k, i in enumerate(second):
        cn = conns[i]["streams"]
        assert got[k] == [(max(-M.INT32_MAX, min(M.INT32_MAX, cn[s]["output_window"])), 0) for s in sorted(cn)] + [(0, 1)], cases[i]["name"]
    assert CI.T.guards_ok(whole)


def damaged(name):
    """-> (image, region size or None): a valid image of five streams for a table of 8 with one field damaged"""
    im = bytearray(image(8, 5, 9))
    e = np.frombuffer(im, ENTRY, offset=64)  # (a writable view of the records)
    word = lambda o, v: im.__setitem__(slice(o, o + 4), struct.pack("<I", v))  # noqa: E731
    if name in ("count+1", "count-1"):
        word(48, 6 if name == "count+1" else 4)
    elif name in ("magic", "version", "family", "parameter", "total", "state_rsv"):
        o = dict(magic=0, version=4, family=6, parameter=12, total=20, state_rsv=56)[name]
        im[o] ^= 1
    elif name == "zero_id":
        e["stream_id"][0] = 0
    elif name == "id_2^31":
        e["stream_id"][4] = 1 << 31
    elif name == "swapped":
        e["stream_id"][[1, 2]] = e["stream_id"][[2, 1]]
    elif name == "duplicate":
        e["stream_id"][3] = e["stream_id"][2]
    elif name != "short_region":
        field, v = dict(state=("state", 4), body=("body", 4), flags=("flags", 16), rsv=("rsv", 1), mark=("mark", 2))[name]
        e[field][2] = v
    return bytes(im), len(im) - 16 if name == "short_region" else None


@pytest.mark.parametrize("name", ["magic", "version", "family", "parameter", "total", "state_rsv", "count+1", "count-1", "zero_id", "id_2^31",
                                  "swapped", "duplicate", "state", "body", "flags", "rsv", "mark", "short_region"])
def test_import_refuses_damaged_images(torch, name):
    bad, region = damaged(name)
    good = image(8, 5, 9)
    _, scr = scratch(torch, 8, 2)
    assert imp(torch, 8, scr, 2, [1, 0], [bad, good], None if region is None else [region, len(good)]) == [C.IMG_EFORMAT, 0]
    s = slabs(scr, 8, 2)
    assert (s[1] == FILL).all() and (s[0] != FILL).any()


def test_space_slots_and_other_families(torch):
    images = [image(8, c, c) for c in (3, 8, 0)]
    whole, scr = scratch(torch, 8, 4)
    # a slot out of range and a slot named twice: refused, the owner's import stands
    assert imp(torch, 8, scr, 4, [2, 4, 2, 0], images + [images[0]]) == [0, C.IMG_EINVAL, C.IMG_EINVAL, 0]
    before = slabs(scr, 8, 4).copy()
    assert (before[[1, 3]] == FILL).all()
    # the region of item 1 one 16-byte line too small: the length needed, nothing written; a slot out of range
    out = export(torch, 8, scr, 4, [2, 0, 7, 2], room=lambda need: [need[0], need[1] - 16, 16, need[3]])
    assert out.status.tolist() == [0, C.IMG_SPACE, C.IMG_EINVAL, 0] and out.len.tolist() == [len(images[0]), len(images[0]), 0, len(images[0])]
    assert out.bytes(0) == images[0] == out.bytes(3)
    o = int(out.off[1])
    assert (out.img[o:int(out.off[3])].cpu().numpy() == CI.SENT).all() and (slabs(scr, 8, 4) == before).all() and CI.T.guards_ok(whole)
    # hhuff_conn_import knows the four older families and the decoder sessions: another family
    fam = C.conn_family(C.FAM_HPACK_ENC)
    other = torch.full((C.conn_slab_size(fam),), FILL, dtype=torch.uint8, device="cuda")
    st = C.conn_import(fam, other, 1, CI.u32(torch, [0]), *put(torch, [images[0]]))
    assert st.cpu().numpy().tolist() == [C.IMG_EPARAM] and (other.cpu().numpy() == FILL).all()
