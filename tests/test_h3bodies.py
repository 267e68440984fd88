"""HTTP/3 bodies on the GPU (include/hhuff.h (2l'), (2l''), h2o_amd/csrc/hhuff_h3bodies.hip): hhuff_h3_bodies on the frame
records hhuff_h3_deframe lists for hand-built streams, against `gather` below -- h2o's loop over the same records in
plain Python --, and hhuff_h3_frame_data against b"\\x00" + varint + body.  `out` lies between guard bytes and is
compared whole.  tests/test_h3bodies_host.py runs the shared arithmetic on the CPU."""
import numpy as np
import pytest

from h2o_amd import codec as C
from h3frames_corpora import fr, vi
from test_h3frames import dev, torch_cuda  # noqa: F401  (the module fixture: an MI355X and the library built)

pytestmark = pytest.mark.gpu
CANARY, GUARD, NONE = 0xA5, 64, 2 ** 64 - 1
EINVAL, SPACE = C.H3BD_EINVAL, C.H3BD_SPACE
pat = lambda n, k=0: bytes((i * 131 + (i >> 8) + 7 + k) & 255 for i in range(n))  # noqa: E731
D = lambda n, k=0: fr(0, pat(n, k))  # noqa: E731  (a DATA frame)


def deframe(torch, streams, st=None):
    """request streams (in phase _DATA unless st says otherwise) of one connection, a slot for every two bytes ->
    h3_deframe's tensors, the call's arrays and sizes"""
    nstr, data = len(streams), b"".join(streams) or b"\0"
    if st is None:
        st = np.zeros(nstr, C.H3_STREAM_DTYPE)
        st["phase"] = C.H3P_DATA
    edges = lambda v: np.cumsum([0] + list(v)).astype(np.uint32)  # noqa: E731
    first = edges(len(s) // 2 + 1 for s in streams)
    t = dict(data=dev(torch, np.frombuffer(data, np.uint8)), frm_first=dev(torch, first), frm_cap=int(first[-1]), in_size=len(data))
    r = C.h3_deframe(t["data"], dev(torch, edges(len(s) for s in streams)), dev(torch, np.array([0, nstr], np.uint32)), t["frm_first"],
                     t["frm_cap"], dev(torch, st), in_size=len(data))
    return dict(t, raw=data, first=first.tolist(), **r)


def guarded(torch, size, mis):
    """-> `out`, exactly `size` bytes at address mis mod 16 between guard bytes, and written(end): out[0 .. end) after the
    call, once no byte in front of `out` or behind out[end] is found written"""
    whole, lo = torch.full((GUARD + mis + size + GUARD,), CANARY, dtype=torch.uint8, device="cuda"), GUARD + mis

    def written(end):
        img = whole.cpu().numpy().tobytes()
        assert whole.data_ptr() % 16 == 0 and set(img[:lo]) <= {CANARY} and set(img[lo + end:]) <= {CANARY}, "a byte outside was written"
        return img[lo:lo + end]
    return whole[lo:], written


def gather(d, frames, cl, rcv, out_size):
    """-> [(out_off, len, nframes, flags, received, status, 0)], [body bytes, None with a status], the end of the last place"""
    nfr, at, runs, bodies = d["nframes"].cpu().numpy().view(np.uint32).tolist(), 0, [], []
    for s, f0 in enumerate(d["first"][:-1]):
        body, cut, bad, total, ndata, kept = b"", False, False, 0, 0, 0
        for typ, hdr, po, length, avail, _ in frames[f0:f0 + min(nfr[s], d["first"][s + 1] - f0)].tolist():
            if typ != 0:
                continue
            wrong = avail > length or po + avail > d["in_size"]
            bad, ndata, total = bad or wrong, ndata + 1, total + (0 if wrong else avail)
            cut = cut or (hdr != po and cl[s] != NONE and cl[s] - (rcv[s] + len(body)) < length)
            if not cut:
                body, kept = body + (b"" if wrong else d["raw"][po:po + avail]), kept + 1
        status = EINVAL if bad or rcv[s] > cl[s] else SPACE if at + total > out_size else 0
        runs.append((min(at, out_size), 0, ndata, 0, rcv[s], status, 0) if status else
                    (at, len(body), kept, C.H3BR_OVERFLOW if cut else 0, rcv[s] + len(body), 0, 0))
        bodies.append(None if status else body)
        at += total
    return runs, bodies, at


def bodies(torch, d, cl=None, rcv=None, short=0, mis=0, mutate=None):
    """hhuff_h3_bodies behind deframe, `out` of exactly the bytes needed less `short`, at address mis mod 16 between guards;
    mutate = (field, stream, slot, value) spoils a frame record first.  Everything compared with gather -> runs, bodies"""
    nstr = len(d["first"]) - 1
    frames = d["frames"].cpu().numpy().view(C.H3_FRAME_DTYPE).copy()
    if mutate:
        frames[mutate[0]][d["first"][mutate[1]] + mutate[2]] = mutate[3]
    u64 = lambda v: None if v is None else dev(torch, np.array(v, np.uint64))  # noqa: E731  (None: the call's NULL)
    t_cl, t_rcv, cl, rcv = u64(cl), u64(rcv), cl or [NONE] * nstr, rcv or [0] * nstr
    free = gather(d, frames, [NONE] * nstr, [0] * nstr, 2 ** 32)  # no cut, no SPACE: every place and every DATA slot
    total, ndata, out_size = free[2], sum(w[2] for w in free[0]), max(free[2] - short, 0)
    want, want_body, _ = gather(d, frames, cl, rcv, out_size)
    out, written = guarded(torch, out_size, mis)
    r = C.h3_bodies(d["data"], dev(torch, frames), d["nframes"], d["frm_first"], d["frm_cap"], t_cl, t_rcv, in_size=d["in_size"],
                    out_size=out_size, out=dict(out=out, runs=torch.full((32 * nstr,), CANARY, dtype=torch.uint8, device="cuda")))
    torch.cuda.synchronize()
    img = written(min(total, out_size))
    runs = [tuple(x) for x in r["runs"].cpu().numpy().view(C.H3_BODY_RUN_DTYPE).tolist()]
    assert runs == want and r["totals"].tolist() == [total, ndata]
    for s, w in enumerate(want):
        assert want_body[s] is None or img[w[0]:w[0] + w[1]] == want_body[s], "the bytes of stream %d" % s
    return runs, want_body


three = D(10) + D(20, 1) + D(30, 2)
CASES = {
    "lengths": dict(streams=[b"".join(D(n, n) for n in (0, 1, 15, 16, 17, 33)), D(3) + fr(0x21, b"unknown") + D(4) + fr(1, b"trailers"),
                             D(2) * 24, D(3, 1) * 300, b"", fr(0x21, b"no data")]),  # (eight frames a line; 300 slots a stream)
    "residues": dict(streams=[(D(5) + D(40, 1)) * 4]),  # 49 bytes a pair: both payloads at every source address mod 4
    "share_boundary": dict(streams=[D(7), D(65536 + 5), D(9)]),
    "many_slots": dict(streams=[D(1, s) * 4 for s in range(66000)]),  # 264,000 DATA slots: both scan levels, 4,096 segments a share
    "content_length": dict(streams=[three] * 7, cl=[60, 59, 29, 9, NONE, 5, 2 ** 63], rcv=[0, 0, 0, 0, 7, 6, 2 ** 63 - 60]),
    "hostile_offset": dict(streams=[three] * 3, mutate=("payload_off", 1, 1, 2 ** 32 - 3)),
    "hostile_avail": dict(streams=[three] * 3, mutate=("avail", 1, 1, 21)),
}


@pytest.mark.parametrize("name,short,mis", [(n, 0, 0) for n in CASES] + [("lengths", s, m) for s in (0, 1) for m in (1, 6, 15)] +
                         [("residues", 0, m) for m in range(1, 16)])  # ... and at every place mod 16
def test_receive(torch_cuda, name, short, mis):
    case = dict(CASES[name])
    runs, _ = bodies(torch_cuda, deframe(torch_cuda, case.pop("streams")), short=short, mis=mis, **case)
    status = [r[5] for r in runs]
    if name == "content_length":
        assert [(r[1], r[2], r[3]) for r in runs[:5]] == [(60, 3, 0), (30, 2, 1), (10, 1, 1), (0, 0, 1), (60, 3, 0)]
        assert status == [0] * 5 + [EINVAL, 0] and runs[6][4] == 2 ** 63
    elif name.startswith("hostile"):
        assert status == [0, EINVAL, 0] and runs[2][:2] == (100, 60)
    else:  # one byte short: the last place with bytes, and the empty ones behind it, pass out_size
        assert status == ([0, 0, 0, SPACE, SPACE, SPACE] if short else [0] * len(runs))


def frame_data(torch, body, sends, short=0, mis=0):
    """hhuff_h3_frame_data with `out` as in `bodies`, compared whole -> the frames written"""
    want = [b"" if off + n > len(body) or n == 0 else b"\x00" + vi(n) + body[off:off + n] for off, n in sends]
    off = np.cumsum([0] + [len(w) for w in want]).tolist()
    out, written = guarded(torch, off[-1] - short, mis)
    r = C.h3_frame_data(dev(torch, np.frombuffer(body, np.uint8)), dev(torch, np.array(sends, np.uint32).reshape(-1).view(np.uint8)),
                        out_size=off[-1] - short, out=dict(out=out))
    torch.cuda.synchronize()
    status = [EINVAL if o + n > len(body) else SPACE if off[k + 1] > off[-1] - short else 0 for k, (o, n) in enumerate(sends)]
    assert r["sstatus"].tolist() == status and r["frm_off"].tolist() == off
    end = min([off[k] for k, s in enumerate(status) if s == SPACE] + [off[-1]])
    img = written(end)
    assert img == b"".join(want)[:end], "the frames differ"
    return img


@pytest.mark.parametrize("short,mis", [(0, 0), (1, 0), (0, 5), (1, 15)])
def test_send(torch_cuda, short, mis):
    lens = (0, 1, 63, 64, 16383, 16384, 65537)
    sends = [(100 * k + r, n) for r in range(4) for k, n in enumerate(lens)] + [(200000 - 10, 11), (2 ** 32 - 1, 1), (200001, 0)]
    tiny = [(k % 4096, 1) for k in range(256 * 1024 + 300)]  # both scan levels, 4,096 segments a share of the copy
    frame_data(torch_cuda, pat(200000), tiny + sends + [(5, 5)], short, mis)


@pytest.mark.parametrize("cut", (1, 13, 14, 15, 100, 16500))
def test_closed_loop(torch_cuda, cut):
    """h3_frame_data's frames behind a HEADERS frame, de-framed in two steps cut at a byte (from 14 on the second step begins
    with a continued frame's hdr_off == payload_off record): the two steps' bodies with `received` chained are the body"""
    torch, body = torch_cuda, pat(40000, 9)
    wire = fr(1, b"\x00\x00\xd1\xd7") + frame_data(torch, body, [(0, 1), (1, 16384), (16385, 0), (16385, 63), (16448, 40000 - 16448)])
    st = np.zeros(1, C.H3_STREAM_DTYPE)
    st["flags"] = C.H3S_WALK_ON
    d1 = deframe(torch, [wire[:cut]], st=st)
    r1, b1 = bodies(torch, d1, cl=[40000])
    d2 = deframe(torch, [wire[int(d1["consumed"][0]):]], st=d1["st_out"].cpu().numpy().view(C.H3_STREAM_DTYPE))
    r2, b2 = bodies(torch, d2, cl=[40000], rcv=[r1[0][4]])
    f2 = d2["frames"].cpu().numpy().view(C.H3_FRAME_DTYPE)[0]
    assert (f2["hdr_off"] == f2["payload_off"]) == (cut >= 14) and (cut != 100 or (f2["length"], r1[0][1]) == (16384 - 86, 1 + 86))
    assert int(d2["sstatus"][0]) == 0 and r2[0][3] == 0 and r2[0][4] == 40000 and b1[0] + b2[0] == body
