"""Cache digests on the device (include/hhuff.h (2m)) against the plain model of tests/cdigest_model.py, which is held
against h2o's recorded answers (tests/golden/cache_digests.npz) here as well.  Images and states must be equal byte
for byte; every buffer the calls write lies between guard bytes."""
import random

import numpy as np
import pytest

import cdigest_model as M
from h2o_amd import codec as C
from h2o_amd import hpenc_synth as HE

G = 0xA5  # guard byte
URL = b"https://127.0.0.1.xip.io:8081/cache-digests.cgi/"
NOTFOUND = b"https://127.0.0.1.xip.io:8081/notfound.js"
BASE = [b"AeLA", b"FOO; stale, AcA; validators; complete", b"AcA; reset"]  # h2o's t/00unit/lib/http2/cache_digests.c


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from h2o_amd import build

    build.build(verbose=False)
    return torch


def filled(nbytes, pbits, seed, last_one=True):
    """a digest of exactly nbytes decoded bytes: random keys, then zeros and (last_one) a terminator on the last bit"""
    rng, bits, keys, k = random.Random(seed), 10, [], -1
    while True:
        gap = rng.randrange(0, 5 << pbits)
        cost = (gap >> pbits) + 1 + pbits
        if bits + cost + 1 > 8 * nbytes:
            break
        k, bits = k + 1 + gap, bits + cost
        keys.append(k)
    tok = M.gcs(31, pbits, keys, tail="0" * (8 * nbytes - bits - 1) + ("1" if last_one else "0"))
    assert len(M.bits_of(tok)) == 8 * nbytes and M.decode_digest(tok)[1][:len(keys)] == keys  # (pbits 0: the last bit is a key)
    return tok


def load_cases():
    """-> [values of one request]: the load and wave edges of the issue"""
    two = M.gcs(3, 7, [5, 300])
    cases = [BASE[:1], BASE[:2], BASE, [b"AeLA; ReSeT"], [b"AeLA, AeLA; foo; reset, AcA;validators"], [b"AeLA; a=b"],
             [b"AeLA;complete = x , AcA ; validators;a=,AeLA;complete"], [b",AeLA"], [b""], [b" \t"], [b","], [b"AeLA,,AcA"],
             [b"AeLA; complete", b"AcA; reset; validators"], [b"AeLA,A*LA;complete,AcA"], [b"AeL A"], [b"AeLA" + b"A"],
             [b"Ke+/gA;validators, Ke-_gA"],  # gcs(5, 7, [62, 189]) in both alphabets
             # a key equal to 2^capacity_bits: dropped with its complete, its reset applied
             [b"AeLA; complete", M.gcs(2, 1, [3, 8]) + b"; complete; reset"], [b"AeLA", M.gcs(2, 1, [3, 7]) + b"; complete"],
             [M.gcs(1, 31, [5, 2 ** 31 + 9], tail="1")],  # a remainder cut short
             [M.gcs(31, 31, [0, 2 ** 33 + 5])],  # (a key near 2^62 would take a unary run of 2^31 bits)
             # wave edges: a terminator on bit 63 (10 + 53 zeros), runs across a window and across a round
             [M.gcs(30, 7, [53 << 7 | 0x55, (53 << 7) + 0x156])], [M.gcs(30, 1, [2 * 100 + 1, 2 * 5300, 2 * 5300 + 1])],
             [M.gcs(20, 0, [9000, 9001, 9003])], [filled(300, 31, 1)]]
    cases += [[t] for L in (2, 3, 4) for t in (two[:L], two[:L] + b"-_")]  # tails 2, 3 and 0 (0 or 1 key survive)
    cases += [[filled(n, pb, n + pb, last)] for n, pb, last in ((512, 7, True), (512, 7, False), (513, 7, True), (1536, 7, True),
                                                              (1536, 0, True), (600, 1, True))]
    return cases


def on_device(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def pack(strings):
    off = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.uint32)
    return np.frombuffer(b"".join(strings) + b"\0", np.uint8).copy(), off


def gpu_load(torch, reqs, rooms, cut=0):
    """one load; region r = rooms[r] bytes from a 16-byte aligned start, guard bytes everywhere else; in_size ends `cut`
    bytes before the last value's end -> [(status, image)]"""
    data, off = pack([v for r in reqs for v in r])
    first = np.concatenate([[0], np.cumsum([len(r) for r in reqs])]).astype(np.uint32)
    out = []
    if len(reqs) == 1:  # an exact region: dig_off[1] need not be aligned
        dig_off = np.array([64, 64 + rooms[0]], np.int64)
    else:
        dig_off = 64 + np.concatenate([[0], np.cumsum([(x + 15) & ~15 for x in rooms])]).astype(np.int64)
    dig = torch.full((int(dig_off[-1]) + 64,), G, dtype=torch.uint8, device="cuda")
    _, status = C.cache_digests_load(on_device(torch, data), on_device(torch, off[:-1].view(np.int32)),
                                     on_device(torch, np.diff(off).astype(np.int32)), on_device(torch, first.view(np.int32)),
                                     on_device(torch, dig_off), dig=dig, in_size=int(off[-1]) - cut)
    torch.cuda.synchronize()
    h, status = dig.cpu().numpy(), status.cpu().numpy()
    assert (h[:64] == G).all() and (h[int(dig_off[-1]):] == G).all()
    for r in range(len(reqs)):
        region = h[int(dig_off[r]):int(dig_off[r + 1])]
        n = int(region[12:16].view(np.uint32)[0]) if region.size >= 16 else 0
        out.append((int(status[r]), region[:n].tobytes()))
    return out


def test_model_matches_h2o():
    assert M.check_fixture() >= 20
    d = M.Digests()
    d.load_header(BASE[0])
    assert d.frames == [(7, 0, [11])] and M.key_hash(URL + b"hello.js") >> 57 == 11 and M.key_hash(NOTFOUND) >> 57 == 47
    assert (d.lookup(0, URL + b"hello.js"), d.lookup(0, NOTFOUND)) == (M.FRESH, M.UNKNOWN)
    d.load_header(BASE[1])
    assert (d.lookup(0, URL + b"hello.js"), d.lookup(0, NOTFOUND)) == (M.FRESH, M.NOT_CACHED)
    d.load_header(BASE[2])
    assert d.frames == [(7, 0, [])] and d.present and not d.complete


@pytest.mark.gpu
def test_gpu_load_edges(torch_cuda):
    cases = load_cases() + [[b"AeLA", b"AeLA"]]  # the last value passes in_size: HHUFF_CD_EINVAL, a header-only image
    want = [M.load(vs, 1 << 30) for vs in cases[:-1]] + [(M.EINVAL, M.Digests().image())]
    assert sum(len(img) > 16 for _, img in want) >= 25  # the cases hold frames
    got = gpu_load(torch_cuda, cases, [M.peak(vs) for vs in cases], cut=1)  # (a reset does not hand back what was appended)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, cases[k][0][:40], g[0], w[0], len(g[1]), len(w[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("short", [0, 8, 24, 1 << 20])
def test_gpu_load_regions(torch_cuda, short):
    """exact fit; 8 bytes short of the second frame; under 16 bytes"""
    values = [b"AeLA, " + M.gcs(3, 7, [5, 300, 900])]
    need = len(M.load(values, 1 << 30)[1])
    room = max(need - short, 8)
    status, img = gpu_load(torch_cuda, [values], [room])[0]
    assert (status, img) == M.load(values, room) and status == (M.SPACE if short else 0)
    assert len(img) == (need if not short else 16 if room >= 16 else 0)


@pytest.mark.gpu
def test_gpu_load_fields(torch_cuda):
    """blocks as the decoders lay them out: the token in slots first, last and twice, on a block of more than 64 slots"""
    torch = torch_cuda
    nf = [3, 0, 70, 2, 1]
    first = np.array([0, 4, 4, 80, 82, 90], np.uint32)  # (gaps behind blocks 0 and 4)
    hits = {0: b"AeLA", 2: b"x", 4: b"AcA; reset", 67: b"AeLA; complete", 68: b"junk", 73: M.gcs(3, 7, [5, 300]), 80: b"AeLA", 81: b"AcA",
            83: b"AeLA"}  # slot 83 lies behind block 4's field
    vals = [hits.get(s, b"AeLA; complete") for s in range(90)]
    token = np.array([9 if s in hits and s not in (2, 68) else 4 for s in range(90)], np.int32)
    data, off = pack(vals)
    want = [M.load([vals[s] for s in range(first[b], first[b] + nf[b]) if token[s] == 9], 1 << 20) for b in range(5)]
    dig_off = np.arange(6, dtype=np.int64) * 256
    dig = torch.full((5 * 256 + 64,), G, dtype=torch.uint8, device="cuda")
    _, status = C.cache_digests_load_fields(on_device(torch, data), on_device(torch, off[:-1].view(np.int32)),
                                            on_device(torch, np.diff(off).astype(np.int32)), on_device(torch, first.view(np.int32)),
                                            on_device(torch, np.array(nf, np.int32)), 90, on_device(torch, token), 9,
                                            on_device(torch, dig_off), dig=dig)
    torch.cuda.synchronize()
    h = dig.cpu().numpy()
    for b, (st, img) in enumerate(want):
        assert int(status[b]) == st == 0 and h[256 * b:256 * b + len(img)].tobytes() == img, b
    assert (h[5 * 256:] == G).all() and [len(w[1]) for w in want] == [40, 16, 88, 56, 16]


# ---- lookup ----
def lookup_cases():
    """-> images, their models, [(req, flags, segments, want or None = the model's)]; six segments: the first is an
    alignment shim in front of the message"""
    imgs, models, qs = [], [], []
    u = [URL + b"%d.js" % i for i in range(4)]
    key = lambda m, cap: M.key_hash(m) >> (64 - cap) if cap else M.key_hash(m)  # noqa: E731

    def image(frames, complete=False, present=True):
        d = M.Digests()
        d.present, d.complete, d.frames = present, complete, frames
        imgs.append(d.image())
        models.append(d)
        return len(imgs) - 1

    k = key(u[0], 20)
    for keys in ([], [k], [k - 1], [k + 1], [k, k + 5], [k - 5, k], [k - 5, k + 5], [k - 5, k, k + 5], [k - 9, k - 5, k], [k, k + 5, k + 9],
                 [k - 9, k - 5, k - 1], [k + 1, k + 5, k + 9], [k - 5, k - 1, k + 1]):
        for complete in (False, True):
            qs.append((image([(20, 0, keys)], complete), 0, [u[0]], None))
    e = u[1] + b'"etag"'
    r = image([(20, 0, [k - 1]), (13, 1, [key(e, 13)]), (20, 0, [k])], True)  # a hit only in the second frame of its kind
    qs += [(r, 0, [u[0]], M.FRESH), (r, 1, [u[1], b'"etag"'], M.FRESH), (r, 0, [u[1], b'"etag"'], M.NOT_CACHED), (r, 1, [u[0]], M.NOT_CACHED)]
    r = image([(0, 0, [M.key_hash(u[2])])])  # capacity_bits 0: the unshifted hash
    qs += [(r, 0, [u[2]], M.FRESH), (r, 0, [u[3]], M.UNKNOWN), (image([], present=False), 0, [u[0]], M.UNKNOWN)]
    for n in (0, 55, 56, 63, 64, 119, 120):  # message lengths around SHA-256's padding
        m = bytes(range(7, 7 + n))
        qs.append((image([(62, 0, [key(m, 62)])]), 0, [m], M.FRESH))
    m = bytes(range(40, 101))
    r = image([(33, 1, [key(m, 33)])])
    for a in range(4):  # five segments at every alignment; empty ones
        qs += [(r, 1, [b"x" * a, m[:5], m[5:8 + a], m[8 + a:29], m[29:30], m[30:]], M.FRESH), (r, 1, [b"", m[:9 + a], b"", m[9 + a:], b""], M.FRESH)]
    bad = bytearray(imgs[2])
    assert len(bad) == 40
    damaged = [bytes(bad[:0] + b"X" + bad[1:]), bytes(bad[:4] + b"\2" + bad[5:]), bytes(bad[:12] + b"\x40" + bad[13:]),
               bytes(bad[:20] + b"\5" + bad[21:]), bytes(bad[:16] + b"\x3f" + bad[17:]), bytes(bad[:12] + b"\x20" + bad[13:])]
    for img in damaged:  # magic, version, bytes over the region, nkeys past bytes, capacity_bits, bytes short of the frames
        imgs.append(img)
        models.append(None)
        qs.append((len(imgs) - 1, 0, [u[0]], M.EFORMAT))
    qs += [(len(imgs), 0, [u[0]], M.EINVAL), (0, 2, [u[0]], M.EINVAL)]  # req out of range; unknown flags
    return imgs, models, qs


@pytest.mark.gpu
def test_gpu_lookup(torch_cuda):
    torch = torch_cuda
    imgs, models, qs = lookup_cases()
    text, rec, want, msgs = bytearray(b"://"), np.zeros(len(qs) + 1, C.CD_QUERY_DTYPE), [], []
    for i, (req, flags, segs, w) in enumerate(qs):
        if len(segs) > 5:
            text += segs[0]
            segs = segs[1:]
        rec["req"][i], rec["flags"][i] = req, flags
        for j, s in enumerate(segs if len(segs) > 1 else [b""] * 2 + segs):
            rec["off"][i, j], rec["len"][i, j] = len(text), len(s)
            text += s
        msgs.append(b"".join(segs))
        want.append(models[req].lookup(flags & 1, msgs[-1]) if w is None else w)
    rec["off"][-1, 3], rec["len"][-1, 3] = len(text) - 2, 3  # a segment past in_size
    want.append(M.EINVAL)
    dig_off = 64 + np.concatenate([[0], np.cumsum([(len(b) + 15) & ~15 for b in imgs])]).astype(np.int64)
    dig = np.full(int(dig_off[-1]) + 64, G, np.uint8)
    for b, o in zip(imgs, dig_off):
        dig[o:o + len(b)] = np.frombuffer(b, np.uint8)
    state = torch.full((len(want) + 8,), 77, dtype=torch.int32, device="cuda")
    hashes = torch.full((len(want) + 8,), 77, dtype=torch.int64, device="cuda")
    C.cache_digests_lookup(on_device(torch, dig), on_device(torch, dig_off), on_device(torch, np.frombuffer(bytes(text) + b"\0" * 8, np.uint8)),
                           on_device(torch, rec.view(np.uint8)), state=state, hash_out=hashes, in_size=len(text))
    torch.cuda.synchronize()
    assert state.cpu().tolist() == want + [77] * 8
    h = hashes.cpu().numpy().view(np.uint64)
    for i, m in enumerate(msgs):
        if want[i] != M.EINVAL:
            assert int(h[i]) == M.key_hash(m), i  # (hashlib)
    assert set(want) >= {M.UNKNOWN, M.NOT_CACHED, M.FRESH, M.EFORMAT, M.EINVAL} and (h[len(want):] == 77).all()


@pytest.mark.gpu
def test_gpu_closed_loop(torch_cuda):
    """load -> lookup -> hhuff_hpack_flatten_responses: a PUSH_PROMISE for exactly the candidates that are not FRESH"""
    torch = torch_cuda
    paths = [b"/a.css", b"/b.js", b"/c.png"]
    value = M.gcs(12, 7, sorted(M.key_hash(b"https://a.example" + p) >> 45 for p in paths[:1])) + b"; complete"
    tok = C.HDR_TOKEN
    b = HE.build_batch([[dict(status=4, flags=C.RES_PUSH_PROMISE, stream_id=2 + 2 * i, parent_stream_id=1,
                              headers=[(b":method", b"GET", tok), (b":scheme", b"https", tok), (b":authority", b"a.example", tok),
                                       (b":path", p, tok)]) for i, p in enumerate(paths)]])
    data, off = pack([value, b"https", b"://", b"a.example"] + paths)
    q = np.zeros(3, C.CD_QUERY_DTYPE)
    for i in range(3):
        q["off"][i, :4], q["len"][i, :4] = off[[1, 2, 3, 4 + i]], np.diff(off)[[1, 2, 3, 4 + i]]
    d = on_device(torch, data)
    dig_off = on_device(torch, np.array([0, 256], np.int64))
    dig, status = C.cache_digests_load(d, on_device(torch, off[:1].view(np.int32)), on_device(torch, np.diff(off)[:1].astype(np.int32)),
                                       on_device(torch, np.array([0, 1], np.int32)), dig_off)
    state, _ = C.cache_digests_lookup(dig, dig_off, d, on_device(torch, q.view(np.uint8)))
    keep = state[:3] != C.CD_FRESH  # the decision stays on the device
    res = on_device(torch, b["res"].view(np.uint8).reshape(3, -1))[keep].contiguous().view(-1)
    nres = int(keep.sum().item())
    r = C.hpack_flatten_responses(on_device(torch, b["data"]), on_device(torch, b["hdr"].view(np.uint8)), res,
                                  on_device(torch, np.array([0, nres], np.int32)), nres, on_device(torch, b["out_off"][:nres + 1].view(np.int64)))
    torch.cuda.synchronize()
    assert status.cpu().tolist()[:1] == [0] and state.cpu().tolist()[:3] == [M.FRESH, M.NOT_CACHED, M.NOT_CACHED] and nres == 2
    out, out_off = r["out"].cpu().numpy(), b["out_off"]
    assert r["rstatus"].cpu().tolist()[:2] == [0, 0]
    for k, promised in enumerate((4, 6)):  # type 5 on the parent stream, then the promised id
        f = out[int(out_off[k]):int(out_off[k]) + int(r["out_len"][k])].tobytes()
        assert f[3] == 5 and f[5:9] == b"\0\0\0\1" and f[9:13] == promised.to_bytes(4, "big")
