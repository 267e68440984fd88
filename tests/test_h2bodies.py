"""HTTP/2 request bodies on the receive side (include/hhuff.h (2k''''), h2o_amd/csrc/hhuff_h2bodies.hip) on the GPU,
bit for bit against `reference` below: a dict from stream id to a bytearray per connection, in insertion order.  The
inputs are arrays built by hand (the call reads in, ctl[].a, sev[], frm_first, nstr and out_off only); `out` and the
run records start as a canary and are compared whole.  tests/test_h2bodies_host.py runs the same cases through the
plan's own code on the CPU."""
import numpy as np
import pytest

from h2o_amd import codec as C

pytestmark = pytest.mark.gpu
CANARY = 0xA5
BODY, RC, TRAILERS, OPENED = C.H2SE_BODY, C.H2SE_REQUEST_COMPLETE, C.H2SE_TRAILERS, C.H2SE_OPENED
RESET_BY_PEER, RESET_SENT = C.H2SE_RESET_BY_PEER, C.H2SE_RESET_SENT
_i = np.arange(1 << 21, dtype=np.uint32)
DATA = ((_i * 131 + (_i >> 8) + 7) & 255).astype(np.uint8)  # the receive buffer of every hand-built case


def B(sid, a, src, more=0):
    """a BODY slot: (stream id, event flags, sev.a, ctl.a)"""
    return (sid, BODY | more, a, src)


def layout(name, conns, rooms=None, **over):
    """conns: per connection its slots -> the call's arrays as lists; a region has 5 bytes more than its runs need"""
    flat = [s for c in conns for s in c]
    rooms = rooms or [sum(s[2] for s in c if s[1] & BODY) + 5 for c in conns]
    L = dict(name=name, sev=flat, frm_cap=len(flat), frm_first=np.cumsum([0] + [len(c) for c in conns]).tolist(),
             nstr=[len(c) for c in conns], out_off=np.cumsum([0] + rooms).tolist(), out_size=sum(rooms),
             in_size=max([4096] + [s[3] + s[2] for s in flat if s[2]]))
    L.update(over)
    return L


def ranges(L, c):
    """connection c's first slot, slots walked, region start and room, clamped as the header says"""
    f0 = min(L["frm_first"][c], L["frm_cap"])
    f1 = min(max(L["frm_first"][c + 1], f0), L["frm_cap"])
    o0 = min(L["out_off"][c], L["out_size"])
    return f0, min(L["nstr"][c], f1 - f0), o0, min(max(L["out_off"][c + 1], o0), L["out_size"]) - o0


def reference(L):
    """-> out (the whole image), runs {slot: record}, res [(nrun, out_len, bstatus)], plan {slot: (run, offset in the run)}"""
    out, runs, res, plan = bytearray([CANARY]) * L["out_size"], {}, [], {}
    for c in range(len(L["nstr"])):
        f0, n, o0, room = ranges(L, c)
        body, rec, mine, status = {}, {}, {}, 0
        for i in range(f0, f0 + n):
            sid, fl, a, src = L["sev"][i]
            if fl & BODY:
                if sid == 0 or (a and src + a > L["in_size"]):
                    status = C.H2BD_EINVAL
                    break
                if sid not in body:
                    body[sid], rec[sid] = bytearray(), [sid, 0, 0, 0, i, 0, 0, 0]
                mine[i] = (list(rec).index(sid) if rec[sid][4] != i else len(rec) - 1, len(body[sid]))
                body[sid] += DATA[src:src + a].tobytes()
                rec[sid][3] += 1
            if sid in rec:
                rec[sid][5] |= (C.H2BR_COMPLETE if fl & RC else 0) | (C.H2BR_RESET if fl & (RESET_BY_PEER | RESET_SENT) and i != rec[sid][4] else 0)
        if status == 0 and sum(len(b) for b in body.values()) > room:
            status = C.H2BD_SPACE
        if status:
            res.append((0, 0, status))
            continue
        at = o0
        for k, (sid, b) in enumerate(body.items()):
            rec[sid][1:3] = at, len(b)
            out[at:at + len(b)] = b
            runs[f0 + k] = tuple(rec[sid])
            at += len(b)
        plan.update(mine)
        res.append((len(body), at - o0, 0))
    return dict(out=bytes(out), runs=runs, res=res, plan=plan)


def cases():
    lens = (1, 3, 15, 16, 17, 31, 33, 40)
    inter = [B(1, 5, 100), B(3, 7, 9), (5, OPENED, 0, 0), (9, OPENED | RC, 0, 0), B(1, 3, 300, C.H2SE_WINDOW_UPDATE_SENT),
             B(3, 0, 0xFFFFFFF0, RC), B(5, 0, 0, RC), B(9, 2, 50), B(1, 4, 20), (1, RESET_BY_PEER, 0, 0), (7, RC, 0, 0), (0, 0, 0, 0),
             B(11, 6, 70), (11, TRAILERS | RC, 0, 0), B(13, 1, 1, RESET_SENT), B(15, 1, 2), B(15, 1, 3, RESET_SENT)]
    yield layout("interleaving", [inter])
    # a job of every length from a source at every offset mod 16, back to back in one run; region d begins at d mod 16
    one = [B(1, n, 64 * (8 * s + k) + s) for s in range(16) for k, n in enumerate(lens)]
    off = [2561 * d for d in range(17)] + [2561 * 16 + 16384 + 7]
    yield layout("alignment", [one] * 16 + [[B(1, 16384, 8195)]], out_off=off, out_size=off[-1])
    yield layout("one_mib_frame", [[B(1, 1 << 20, 5)]])
    for n in (257, 513):  # the copy's window of 256 jobs
        yield layout("one_byte_frames_%d" % n, [[B(1 + 2 * (i % 3), 1, 7 * i) for i in range(n)]])
    for n in (255, 256, 257):  # the walk's workgroup of 256 connections
        yield layout("connections_%d" % n, [[B(1 + 2 * c, 1 + c % 7, 3 * c)] for c in range(n)])
    yield layout("streams_300", [[B(1 + 2 * i, 1 + i % 3, 5 * i) for i in range(300)]])
    # 16 slots have a table of 32 entries, home (id >> 1) % 32: four streams at home 31, whose probes wrap, four at 0
    ids = [2 * (31 + 32 * j) + 1 for j in range(4)] + [2 * 32 * j + 1 for j in range(1, 5)]
    yield layout("colliding_ids", [[B(s, 2 + k, 10 * k + s % 7) for k in range(2) for s in ids]])
    mid = [B(3 + 2 * i, 1, i) if i % 2 else (3 + 2 * i, OPENED, 0, 0) for i in range(998)]
    yield layout("first_and_last_of_1000", [[B(1, 3, 0)] + mid + [B(1, 2, 7, RC)]])
    # untrusted input, each beside a good connection
    good, two = [B(1, 9, 11), B(3, 4, 40), B(1, 2, 77, RC)], [B(5, 3, 0), B(7, 4, 10)]
    yield layout("payload_leaves_in", [good, [B(5, 3, 0), B(5, 4, 4093)]], in_size=4096, bstatus=[0, C.H2BD_EINVAL])
    yield layout("stream_id_0", [[B(5, 3, 0), B(0, 2, 10)], good], bstatus=[C.H2BD_EINVAL, 0])
    yield layout("region_one_short", [good, two], rooms=[20, 6], bstatus=[0, C.H2BD_SPACE])
    yield layout("region_exact", [good, two, good], rooms=[15, 7, 15])
    yield layout("out_off_beyond_out_size", [good, two, two, []], out_off=[0, 20, 2 ** 32 - 1, 2 ** 32 - 1, 5], out_size=27,
                 bstatus=[0, 0, C.H2BD_SPACE, 0])
    yield layout("nstr_above_the_slots", [two, good], nstr=[100, 2 ** 32 - 1])
    yield layout("frm_first_no_running_sum", [two + good + good], frm_first=[4, 2, 6, 99], nstr=[3, 4, 5], out_off=[0, 10, 40, 60],
                 out_size=60)


CASES = list(cases())


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from h2o_amd import build

    build.build(verbose=False)
    return torch


def call(torch, L, data, ctl, sev):
    """hhuff_h2_bodies with every output a canary -> out, the run records [frm_cap, 8], [(nrun, out_len, bstatus)]"""
    u32 = lambda v: torch.from_numpy(np.array(v, np.uint32).view(np.int32)).cuda()  # noqa: E731
    full = lambda n: torch.full((max(1, n),), CANARY, dtype=torch.uint8, device="cuda")  # noqa: E731
    n = len(L["nstr"])
    out = dict(out=full(L["out_size"]), runs=full(32 * L["frm_cap"]), nrun=full(4 * n).view(torch.int32),
               out_len=full(4 * n).view(torch.int32), bstatus=full(4 * n).view(torch.int32))
    r = C.h2_bodies(data, ctl, sev, u32(L["frm_first"]), L["frm_cap"], u32(L["nstr"]), u32(L["out_off"]), in_size=L["in_size"],
                    out_size=L["out_size"], out=out)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in r.items()}
    res = list(zip(h["nrun"].tolist(), h["out_len"].tolist(), h["bstatus"].tolist()))
    return h["out"][:L["out_size"]].tobytes(), h["runs"][:32 * L["frm_cap"]].view("<u4").reshape(-1, 8), res


@pytest.mark.parametrize("L", CASES, ids=[L["name"] for L in CASES])
def test_hand_built_cases(torch_cuda, L):
    torch = torch_cuda
    sev, ctl = np.zeros(L["frm_cap"], C.H2_SEV_DTYPE), np.zeros(L["frm_cap"], C.H2_CTL_DTYPE)
    for i, (sid, fl, a, src) in enumerate(L["sev"]):
        sev[i], ctl[i]["a"] = (sid, a, 0, 0, fl), src
    dev = lambda a: torch.from_numpy(a.view(np.uint8)).cuda()  # noqa: E731
    out, runs, res = call(torch, L, dev(DATA[:L["in_size"]]), dev(ctl), dev(sev))
    want = reference(L)
    assert res == want["res"]
    assert out == want["out"], "the image differs (runs, the regions' tails or the gaps between regions)"
    for i in range(L["frm_cap"]):
        assert runs[i].tolist() == list(want["runs"].get(i, [CANARY * 0x01010101] * 8)), i
    assert [s for _, _, s in res] == L.get("bstatus", [0] * len(res))


def test_argument_refusals_come_before_any_device_call():
    """HHUFF_EINVAL for a NULL array, a size >= 2^32 or non-zero flags, with nconn == 0 too; nconn == 0 is HHUFF_OK"""
    p = 1 << 20  # a dummy address: never dereferenced on these paths
    names = ("in", "in_size", "ctl", "sev", "frm_first", "frm_cap", "nstr", "nconn", "flags", "out", "out_size", "out_off", "runs",
             "nrun", "out_len", "bstatus", "stream")
    default = dict.fromkeys(names, p)
    default.update(in_size=64, frm_cap=4, nconn=2, flags=0, out_size=64, stream=None)
    f = lambda **k: C.lib().hhuff_h2_bodies(*[k.get(a, default[a]) for a in names])  # noqa: E731
    for a in ("in", "ctl", "sev", "frm_first", "nstr", "out", "out_off", "runs", "nrun", "out_len", "bstatus"):
        assert f(**{a: None}) == -1 and f(**{a: None, "nconn": 0}) == -1, a
    assert f(in_size=1 << 32) == -1 and f(out_size=1 << 32, nconn=0) == -1 and f(flags=1) == -1 and f(flags=1 << 31, nconn=0) == -1
    assert f(nconn=0) == 0 and f(nconn=0, in_size=(1 << 32) - 1, out_size=(1 << 32) - 1) == 0


def test_real_bytes_through_the_five_calls(torch_cuda):
    """two POSTs on one connection, their DATA frames interleaved and padded, trailers on one: socket bytes through
    hhuff_h2_deframe, hhuff_h2_control, hhuff_hpack_parse_requests and hhuff_h2_streams, then the runs are the bodies"""
    import h2streams_model as M
    from test_h2streams import dev, h2frame, lit

    torch = torch_cuda
    post, pad = b"\x83\x86\x84", lambda n, b: bytes([n]) + b + bytes(n)  # noqa: E731
    wire = (h2frame(1, 4, 1, post) + h2frame(1, 4, 3, post) + h2frame(0, 8, 1, pad(3, b"hello ")) + h2frame(0, 0, 3, b"abc") +
            h2frame(0, 0, 1, b"world") + h2frame(0, 9, 3, pad(0, b"defg")) + h2frame(6, 0, 0, b"12345678") + h2frame(0, 8, 1, pad(200, b"!")) +
            h2frame(1, 5, 1, lit(b"t", b"1")))
    frm_cap, size = 9, len(wire)
    t_data, t_first = dev(torch, np.frombuffer(wire, np.uint8)), dev(torch, np.array([0, frm_cap], np.uint32))
    d = C.h2_deframe(t_data, dev(torch, np.array([0, size], np.uint32)), t_first, frm_cap, arena_fixed=1024, arena_per_byte=16)
    ctl_rep_off = dev(torch, np.array([0, frm_cap * 17], np.uint32))
    k = C.h2_control(t_data, d["frames"], d["nframes"], t_first, frm_cap, C.h2_new_peers(1, "cuda"), ctl_rep_off, 0, 65535,
                     rep_size=frm_cap * 17)
    q = C.hpack_decode_blocks(d["blk"], d["blk_off"], d["conn_first"], arena_off=d["arena_off"], requests=True)
    P = M.params(max_streams=4, max_streams_for_priority=2, max_entries=8)
    scratch = torch.zeros(C.h2_streams_scratch_size(1, 8), dtype=torch.uint8, device="cuda")
    r = C.h2_streams(P, scratch, t_data, d["frames"], d["nframes"], t_first, frm_cap, k["ctl"], k["nctl"], k["rep"], ctl_rep_off,
                     d["blocks"], d["conn_first"], q["bstatus"], q["req"], q["arena"], d["blk_off"], q["value_off"], q["value_len"],
                     k["peers"], dev(torch, np.array([0, frm_cap * 43], np.uint32)), rep_size=frm_cap * 43)
    L = dict(frm_first=[0, frm_cap], frm_cap=frm_cap, nstr=[0], out_off=[0, C.h2_bodies_bound(size)], out_size=size, in_size=size)
    L["nstr"] = r["nstr"].cpu().numpy().view(np.uint32).tolist()
    out, runs, res = call(torch, L, t_data, k["ctl"], r["sev"])
    assert L["nstr"] == [9] and int(r["sstatus"][0]) == 0 and res == [(2, 19, 0)]
    assert out == b"hello world!abcdefg" + bytes([CANARY]) * (size - 19)
    assert runs[:2].tolist() == [[1, 0, 12, 3, 2, C.H2BR_COMPLETE, 0, 0], [3, 12, 7, 2, 3, C.H2BR_COMPLETE, 0, 0]]
    assert (runs[2:] == CANARY * 0x01010101).all()
