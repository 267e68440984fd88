"""CASPER on the device (include/hhuff.h (2n)) against the plain model of tests/casper_model.py, which is held against
h2o's recorded answers (tests/golden/casper.npz) here.  Results, cookie bytes and slabs must be equal byte for byte;
scratch, out and res lie between guard bytes."""
import hashlib
import struct

import numpy as np
import pytest

import casper_model as M
from conftest import load_golden
from h2o_amd import codec as C

G = 0xA5  # guard byte
I, CS, CF, L, K, CK = M.INIT, M.CONSUME, M.CONSUME_FIELDS, M.LOOKUP, M.MARK, M.COOKIE
PAD = 64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from h2o_amd import build

    build.build(verbose=False)
    return torch


def fixture_scripts():
    """-> [[(kind, x)]] with x = (cap, rem), a string or None; h2o's (ret, entries, cookie) per op"""
    g = load_golden("casper")
    text = g["strings"].tobytes()
    s = [text[g["str_off"][i]:g["str_off"][i + 1]] for i in range(g["str_off"].size - 1)]
    ops = [(k, (a, b) if k == I else None if k == CK else s[a]) for k, a, b in g["op"].tolist()]
    want = [(int(g["ret"][o]), int(g["entries"][o]), g["cookies"][g["cookie_off"][o]:g["cookie_off"][o + 1]].tobytes()) for o in range(len(ops))]
    cf = g["case_first"]
    return [ops[cf[c]:cf[c + 1]] for c in range(cf.size - 1)], [want[cf[c]:cf[c + 1]] for c in range(cf.size - 1)], int(g["nrandom"])


def pkey(path, cap=30):
    return int.from_bytes(hashlib.sha1(path).digest()[:4], "little") & ((1 << cap) - 1)


def slab_of(conn, max_keys, magic=b"HHCS", nkeys=None):
    return struct.pack("<4sHBBII", magic, 1, conn.cap, conn.rem, len(conn.keys) if nkeys is None else nkeys, max_keys) + struct.pack(
        "<%dQ" % len(conn.keys), *conn.keys)


def conn_of(img, max_keys):
    """the Casper a slab holds, or None where it is not one"""
    w = struct.unpack_from("<4sHBBII", img)
    if not (w[0] == b"HHCS" and w[1] == 1 and 1 <= w[2] <= 30 and w[3] <= 31 and w[4] <= max_keys and w[5] == max_keys):
        return None
    conn = M.Casper(w[2], w[3], max_keys)
    conn.keys = list(struct.unpack_from("<%dQ" % w[4], img, 16))
    return conn


def pack(scripts, align):
    """-> data, [[(kind, a, b)]]: every string behind `align` bytes from a multiple of 4"""
    data, out = bytearray(), []
    for sc in scripts:
        ops = []
        for kind, x in sc:
            if isinstance(x, bytes):
                data += b"#" * (-len(data) % 4 + align)
                ops.append((kind, len(data), len(x)))
                data += x
            else:
                ops.append((kind,) + (x or (0, 0)))
        out.append(ops)
    return bytes(data), out


def check(torch, scripts, max_keys, rooms=None, slabs=None, slot=None, nslots=None, align=0, fields=None, data=None, model=True):
    """one hhuff_casper_step: connection c runs scripts[c] from slab slabs[c] (bytes; default: junk that is no slab) with a
    region of rooms[c] bytes; held against the model op by op -> [(Casper or None, region bytes, res)] of the device"""
    n = len(scripts)
    if data is None:
        data, scripts = pack(scripts, align)
    slot = list(range(n)) if slot is None else slot
    nslots = nslots or max(slot) + 1
    rooms = rooms or [4096] * n
    sb = C.casper_scratch_bytes(1, max_keys)
    scratch = np.full(PAD + nslots * sb + PAD, G, np.uint8)
    for c in range(n):
        img = (slabs[c] if slabs else bytes([c + 1]) * 24)[:max(0, nslots - slot[c]) * sb]  # (none for a slot outside)
        scratch[PAD + slot[c] * sb:PAD + slot[c] * sb + len(img)] = np.frombuffer(img, np.uint8)
    before = scratch.copy()
    ops = np.zeros(sum(len(s) for s in scripts), C.CSP_OP_DTYPE)
    ops["kind"], ops["a"], ops["b"] = np.array([o for s in scripts for o in s], np.uint32).reshape(-1, 3).T
    first = np.concatenate([[0], np.cumsum([len(s) for s in scripts])]).astype(np.int32)
    out_off = (PAD + np.concatenate([[0], np.cumsum(rooms)])).astype(np.int32)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    d_scr, d_out = dev(scratch), torch.full((int(out_off[-1]) + PAD,), G, dtype=torch.uint8, device="cuda")
    d_res = torch.full((PAD + 16 * len(ops) + PAD,), G, dtype=torch.uint8, device="cuda")
    fd = None if fields is None else tuple(dev(np.array(f, np.int32)) for f in fields[:3]) + (len(fields[2]),)
    C.casper_step(d_scr[PAD:], nslots, max_keys, dev(ops.view(np.uint8)), dev(first), dev(np.frombuffer(data + b"\0" * 8, np.uint8)), d_out,
                  dev(out_off), slot=dev(np.array(slot, np.int32)), fields=fd, cookie_token=9, res=d_res[PAD:], in_size=len(data))
    torch.cuda.synchronize()
    scr, out, res = d_scr.cpu().numpy(), d_out.cpu().numpy(), d_res.cpu().numpy()
    assert (scr[:PAD] == G).all() and (scr[-PAD:] == G).all() and (out[:PAD] == G).all() and (out[-PAD:] == G).all()
    assert (res[:PAD] == G).all() and (res[-PAD:] == G).all()
    res, got = res[PAD:-PAD].view(C.CSP_RESULT_DTYPE), []
    for c in range(n):
        r = [tuple(int(x) for x in res[o]) for o in range(first[c], first[c + 1])]
        used = sum(x[1] for x, op in zip(r, scripts[c]) if op[0] == CK and x[0] == 0)
        region = out[out_off[c]:out_off[c + 1]]
        assert (region[used:] == G).all(), c
        img = scr[PAD + slot[c] * sb:PAD + (slot[c] + 1) * sb]
        conn = conn_of(img.tobytes(), max_keys) if img.size else None
        got.append((conn, region[:used].tobytes(), r))
        if model:
            start = conn_of(slabs[c], max_keys) if slabs else None
            want = M.step(start, scripts[c], data, rooms[c], max_keys, fields, 9, int(out_off[c]))
            assert r == want[2], (c, r, want[2])
            assert got[-1][1] == want[1], (c, got[-1][1], want[1])
            if want[0] is None:
                assert (img == before[PAD + slot[c] * sb:PAD + (slot[c] + 1) * sb]).all(), c
            else:
                assert conn and (conn.cap, conn.rem, conn.keys) == (want[0].cap, want[0].rem, want[0].keys), c
    return got


def test_model_matches_h2o():
    scripts, want, nrandom = fixture_scripts()
    assert nrandom >= 36 and pkey(b"/index.html", 13) == int.from_bytes(b"\x14\xfe\x45\x59", "little") & 0x1fff
    for sc, ws in zip(scripts, want):
        conn = None
        for (kind, x), (ret, entries, cookie) in zip(sc, ws):
            data = x if isinstance(x, bytes) else b""
            conn, _, res = M.step(conn, [(kind,) + ((0, len(data)) if kind not in (I, CK) else x or (0, 0))], data, 1 << 20, None)
            assert res[0][0] == 0 and res[0][2] == entries and conn.cookie() == cookie and (kind not in (L, K) or res[0][1] == ret)


@pytest.mark.gpu
@pytest.mark.parametrize("align", [0, 1, 2, 3])
def test_gpu_hash(torch_cuda, align):
    """SHA-1's padding and block edges at every byte alignment; 65 paths in one connection: a second hashing round"""
    edges = [bytes(range(40, 40 + n)) for n in (0, 1, 55, 56, 63, 64, 119, 120)]
    many = [b"/a/%d" % i for i in range(65)]
    got = check(torch_cuda, [[(I, (30, 6))] + [(k, p) for p in edges for k in (K, L)], [(I, (30, 6))] + [(K, p) for p in many] + [(L, many[64])]],
                128, align=align)
    assert got[0][0].keys == sorted(pkey(p) for p in edges) and got[1][2][-1][1] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_gpu_mark(torch_cuda, n):
    """a mark at the front, at the end, in the middle and of a present key, on sets of n keys; the bound max_keys"""
    pa, pb, pc, pd, pe = sorted([b"/p%d" % i for i in range(5)], key=pkey)
    ka, kb, kd = pkey(pa), pkey(pb), pkey(pd)
    conn = M.Casper(30, 6, 66)
    conn.keys = sorted(([kb] + [ka + 1 + i * ((kd - ka - 2) // 70) for i in range(1, n)])[:n])
    got = check(torch_cuda, [[(K, pa), (K, pe), (K, pc), (K, pb), (L, pb), (L, b"/none"), (CK, None)]], 66, slabs=[slab_of(conn, 66)])
    assert [r[1] for r in got[0][2][:5]] == [0, 0, 0, int(n > 0), 1] and got[0][2][3][2] == (4 if n == 0 else min(n + 3, 66))
    if n == 65:  # the 66th key fits, the 67th does not; a present key is still found
        assert [r[0] for r in got[0][2][:4]] == [0, M.SPACE, M.SPACE, 0]


@pytest.mark.gpu
def test_gpu_init_in_the_middle_and_refusals(torch_cuda):
    p = b"/index.html"
    got = check(torch_cuda, [[(I, (13, 6)), (K, p), (L, p), (I, (5, 0)), (L, p), (K, p), (CK, None)],
                             [(I, (0, 6)), (I, (31, 6)), (I, (13, 32)), (L, p), (I, (13, 6)), (7, p), (0, p), (CF, (0, 1)), (K, p)]], 16)
    assert [r[1] for r in got[0][2]][:6] == [0, 0, 1, 0, 0, 0] and got[0][0].keys == [pkey(p, 5)]
    assert [r[0] for r in got[1][2]] == [M.EINVAL] * 3 + [M.EFORMAT, 0] + [M.EINVAL] * 3 + [0]
    data, ops = pack([[(I, (13, 6)), (K, p), (L, p)]], 0)  # a string that passes in_size; a slot at or above nslots
    got = check(torch_cuda, [ops[0][:2] + [(L, ops[0][2][1], len(p) + 1)], ops[0]], 16, slot=[0, 5], nslots=2, data=data, model=False)
    assert [r[0] for r in got[0][2]] == [0, 0, M.EINVAL] and [r[0] for r in got[1][2]] == [M.EINVAL] * 3 and got[1][0] is None


def cookie_of(keys, rem, tail=""):
    return M.NAME + M.encode(keys, rem, tail)


@pytest.mark.gpu
def test_gpu_consume(torch_cuda):
    """names, tails, key counts, the limit L, a long unary run, remainder_bits 0 / 6 / 31, unions; connections of one call"""
    two, a, b = cookie_of([5, 300, 900], 6), list(range(10, 700, 10)), list(range(5, 700, 15))
    sc = [[(I, (13, 6)), (CS, M.NAME), (CS, b"h2o_caspex=" + two[11:]), (CS, two + b"; x=y"), (CS, two[:13] + b" " + two[14:]), (CK, None)]]
    sc += [[(I, (13, 6)), (CS, two[:11 + n]), (CK, None)] for n in (2, 3, 4, 5, 6)]
    for rem in (0, 6, 31):
        sc += [[(I, (13, rem)), (CS, cookie_of([(7 * i * i + 3 * i) << max(rem - 4, 0) for i in range(n)], rem, "1" if n % 2 else "")),
                (CK, None)] for n in (0, 1, 63, 64, 65)]
    sc += [[(I, (cap, 0)), (CS, cookie_of(range(0, 2 * n, 2), 0)), (CK, None)] for cap, n in ((5, 128), (5, 129), (8, 256), (8, 257))]
    sc += [[(I, (13, 2)), (CS, cookie_of([3, 3 + (5000 << 2), 9 + (5000 << 2)], 2)), (CK, None)]]  # across a 4,096-bit decode round
    sc += [[(I, (13, 6)), (CS, cookie_of(x, 6)), (CS, cookie_of(y, 6)), (CK, None)] for x, y in (
        ([], a), (a, []), (a, a), (a, [1, 2, 3]), (a, [900, 901]), (a, b), (list(range(60)), list(range(100, 110))))]
    got = check(torch_cuda, sc, 320)
    assert [len(g[0].keys) for g in got[21:25]] == [128, 0, 256, 0] and got[0][2][-1][2] == 0 and len(got[-1][0].keys) == 70
    # a cookie that fits L but not max_keys; a union that reaches max_keys exactly, and one key more
    got = check(torch_cuda, [[(I, (13, 6)), (CS, cookie_of(range(101), 6)), (CS, cookie_of(range(0, 120, 2), 6)),
                              (CS, cookie_of(range(1, 81, 2), 6)), (CS, cookie_of([0, 500], 6)), (CK, None)]], 100)
    assert [r[:3] for r in got[0][2][1:5]] == [(M.SPACE, 101, 0), (0, 60, 60), (0, 40, 100), (M.SPACE, 2, 100)]


@pytest.mark.gpu
def test_gpu_consume_fields(torch_cuda):
    """slots of which 0, 1 and 3 carry the token, as hhuff_intern_fields leaves them; slots that pass nfslots"""
    vals = [cookie_of([i, 40 + i], 6) for i in range(6)]
    data, off = b"".join(vals), np.concatenate([[0], np.cumsum([len(v) for v in vals])])
    fields = (off[:-1].tolist(), [len(v) for v in vals], [9, 4, 9, 9, 4, 4])
    got = check(torch_cuda, [[(I, 13, 6), (CF, a, b), (CK, 0, 0)] for a, b in ((4, 2), (1, 2), (0, 4), (3, 4))], 32, fields=fields, data=data)
    assert [g[2][1][:3] for g in got] == [(0, 0, 0), (0, 2, 2), (0, 6, 6), (M.EINVAL, 0, 0)]


def cookie_sets():
    """-> [(rem, keys)]: 1, 63, 64, 65 keys; a one-and-remainder across a 3,072-bit tile edge; a run that skips a tile;
    remainder_bits 0 and 31"""
    sets = [(6, [77 * i + (i * i) % 64 for i in range(n)]) for n in (1, 2, 3, 63, 64, 65)]
    sets += [(6, [3070 << 6 | 5, (3070 << 6) + 80]), (6, [9, (2 * 3072 + 100) << 6, (2 * 3072 + 101) << 6]), (0, [0, 1, 5, 3000, 3072, 6200]),
             (31, [5, 1 << 31, 3 << 31, (3 << 31) + 1])]
    return sets


@pytest.mark.gpu
def test_gpu_cookie(torch_cuda):
    """an empty set; exact regions; a byte short: nothing written and the next COOKIE starts where this one would have"""
    sets = cookie_sets()
    lens = [len(M.encode(k, r)) for r, k in sets]
    assert {(3 * n // 4) % 3 for n in lens} == {0, 1, 2} and max(lens) > 1024
    conns = [M.Casper(13, r, 128) for r, _ in sets]
    for c, (_, k) in zip(conns, sets):
        c.keys = k
    n = [len(c.cookie()) for c in conns]
    slabs = [slab_of(c, 128) for c in conns]
    got = check(torch_cuda, [[(CK, None), (CK, None)]] * len(sets) * 3 + [[(I, (13, 6)), (CK, None), (CK, None)]], 128,
                rooms=[2 * x for x in n] + [2 * x - 1 for x in n] + [x - 1 for x in n] + [0], slabs=slabs * 3 + [slabs[0]])
    k = len(sets)
    assert all(g[2][1][0] == 0 and g[1] == 2 * c.cookie() for g, c in zip(got[:k], conns))
    assert all([r[0] for r in g[2]] == [0, M.SPACE] and g[2][1][3] - g[2][0][3] == x for g, x in zip(got[k:2 * k], n))
    assert all([r[0] for r in g[2]] == [M.SPACE] * 2 and g[2][1][3] == g[2][0][3] and g[1] == b"" for g in got[2 * k:3 * k])
    assert [r[:2] for r in got[-1][2][1:]] == [(0, 0)] * 2


@pytest.mark.gpu
def test_gpu_closed_loop(torch_cuda):
    """the fixture's scripts as one batch through a permutation of slots; a second step on the slabs it left; every
    cookie fed back into a fresh slot gives the same set and the same cookie"""
    scripts, want, _ = fixture_scripts()
    n = len(scripts)
    perm = [(37 * c + 11) % n for c in range(n)]
    got = check(torch_cuda, scripts, 320, slot=perm, rooms=[1 << 18] * n)
    for g, sc, ws in zip(got, scripts, want):
        cookies = [w[2] for (kind, _), w in zip(sc, ws) if kind == CK]
        assert g[1] == b"".join(cookies) and [r[2] for r in g[2]] == [w[1] for w in ws]  # h2o's own bytes and entry counts
    slabs = [slab_of(g[0], 320) for g in got]
    back = [(g[0].cookie() or M.NAME).split(b";")[0] for g in got]
    again = check(torch_cuda, [[(K, b"/index.html"), (CK, None)] for _ in got] + [[(I, (g[0].cap, g[0].rem)), (CS, v), (CK, None)] for g, v in zip(got, back)],
                  320, slabs=slabs + [b"\0" * 16] * n, slot=perm + list(range(n, 2 * n)), rooms=[1 << 18] * (2 * n))
    assert all(again[n + c][0].keys == got[c][0].keys and again[n + c][1] == got[c][0].cookie() for c in range(n))


@pytest.mark.gpu
@pytest.mark.parametrize("damage", ["magic", "nkeys", "capacity_bits", "remainder_bits", "max_keys", "version"])
def test_gpu_hostile_slab(torch_cuda, damage):
    conn = M.Casper(13, 6, 16)
    conn.keys = [3, 9]
    img = bytearray(slab_of(conn, 16, magic=b"HHCD" if damage == "magic" else b"HHCS", nkeys=17 if damage == "nkeys" else None))
    at = {"capacity_bits": (6, 31), "remainder_bits": (7, 32), "max_keys": (12, 17), "version": (4, 2)}.get(damage)
    if at:
        img[at[0]] = at[1]
    got = check(torch_cuda, [[(L, b"/x"), (K, b"/x"), (CS, cookie_of([1], 6)), (CK, None)], [(CK, None), (I, (13, 6)), (K, b"/x")]], 16,
                slabs=[bytes(img)] * 2, model=False)
    assert got[0][2] == [(M.EFORMAT, 0, 0, 0)] * 4 and got[0][0] is None and got[0][1] == b""
    assert [r[:3] for r in got[1][2]] == [(M.EFORMAT, 0, 0), (0, 0, 0), (0, 0, 1)]
