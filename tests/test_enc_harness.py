"""The header encoders' edge corpus on the CPU (tests/enc_harness.py, tests/enc_corpora.py): every case hits the
edge it names; the restatement passes the guarded call on every group, with bound-sized and with exactly fitting
regions; the compiled reference, where oracle/_ref is built, gives the same bytes for the cases its harness accepts;
every accepted block decodes to the fields that went in; and the harness catches each planted fault by the assertion
made for it."""
import numpy as np
import pytest

import enc_corpora as EC
import enc_harness as EH
from h2o_amd import codec as C
from hpenc_push_model import block_of

GROUP_NAMES = list(EC.GROUPS)
CASE_IDS = [(g, c.name) for g in GROUP_NAMES for c in EC.cases(g)]
VARIANTS = {"bound": None, "fit1": 1, "fit13": 13}

# what the compiled reference is not asked: its harness (oracle/ref_hpenc.c) has no h2o_hpack_flatten_push_promise
REF_EXCLUDED = {"promise-16384-%d" % P: "the reference harness has no push promises" for P in EC.payloads(EC.M0)}
# blocks that are not decoded again
ROUNDTRIP_EXCLUDED = {"empty-name": "h2o's decoders refuse an empty header name"}


def variant(name, v, ref_only=False):
    g = EC.group(name, ref_only)
    return g if VARIANTS[v] is None else EH.refit(g, VARIANTS[v])


def nconn(g):
    return g["calls"][0]["conn_first"].size - 1


# ---- the building blocks ----
@pytest.mark.parametrize("bits,length,kw", [(40, 8, {}), (8 * 256 - 8, 256, {}), (8 * 257 - 7, 257, {}), (1600, 256, {}),
                                            (6001, 1000, {}), (20 * 512, 512, dict(min_long=512)), (19, 1, {}),
                                            (5 * 300, 300, dict(name=True)), (8 * 300, 300, dict(name=True))])
def test_strings_with(bits, length, kw):
    s = EH.strings_with(bits, length, **kw)
    assert len(s) == length and EH.code_bits(s) == bits
    assert len(EH.huffman(s)) == EH.huffman_len(s)
    valid = EH.T.NAME_VALID if kw.get("name") else EH.T.VALUE_VALID
    assert set(s) <= valid
    if kw.get("min_long"):
        assert min(EH.NBITS[list(s)]) >= 19
    assert s != EH.strings_with(bits, length, seed=1, **kw) or length < 2


def test_relay_places_strings():
    a, b, c, last = b"a" * 5, b"b" * 7, b"c" * 3, b"zz"
    conns = [[dict(headers=[(b"n1", a, 0), (b"n2", b, 0), (b"n3", c, 0), (b"n4", last, 0), (b"n1", a, 0)])]]
    place = {a: ("mod", 16, 9), b: ("end", 16), last: ("last",)}
    for proto in ("h", "q"):
        r = EH.relay(EH.make_batch(conns, proto), place)
        data, off = r["data"].tobytes(), r["str_off"]
        assert off[a] % 16 == 9 and (off[b] + len(b)) % 16 == 0 and off[last] + len(last) == len(data)
        for h in r["hdr"]:
            n = data[h["name_off"]:h["name_off"] + h["name_len"]]
            assert n in (b"n1", b"n2", b"n3", b"n4")
            assert data[h["value_off"]:h["value_off"] + h["value_len"]] == {b"n1": a, b"n2": b, b"n3": c, b"n4": last}[n]
        assert off[b"n3"] == off[c] - 2 and off[b"n4"] == off[c] + 3  # no rule: packed, no filler
        assert data[r["server_off"]:r["server_off"] + r["server_len"]] == EH.HE.SERVER
        gaps = int((~r["owned"]).sum())
        assert gaps > 0 and (EH.with_fill(r, 0xEE)[~r["owned"]] == 0xEE).all()
        assert EH.with_fill(r, 0xEE)[r["owned"]].tobytes() == r["data"][r["owned"]].tobytes()
        want = EH.model_run(proto, [EH.make_batch(conns, proto)])[0]
        got = EH.model_run(proto, [dict(r, data=EH.with_fill(r, 0xEE))])[0]
        assert got["out"].tobytes() == want["out"].tobytes()  # the same records, wherever the strings lie


def test_pad_to_payload():
    for proto, target in (("h", 300), ("h", 16385), ("q", 64), ("q", 16384)):
        for kind in ("raw", "huff"):
            conn = [EC.rec([(b"x-a", b"1", 0)]), EC.rec([(b"x-p", b"head:", 0), (b"x-b", b"2", 0)])]
            recs = EH.pad_to_payload(conn, target, proto, 1, 0, kind)
            r = EH.model_run(proto, [EH.make_batch([recs], proto)])[0]
            assert r[EH.HS[proto]][1] == target and recs[1]["headers"][0][1].startswith(b"head:")


def test_exact_fit_and_short_by_one():
    conns = [[EC.rec([(b"x-a", b"first", 0)]), EC.rec([(b"x-b", EH.text(50), 0)]), EC.rec([(b"x-c", b"third", 0)])]]
    for proto, after in (("h", C.RES_SKIPPED), ("q", 0)):
        b = EH.make_batch(conns, proto)
        res = EH.model_run(proto, [b])[0]
        fit = EH.exact_fit(b, res, first=13)
        assert fit["out_off"][0] == 13 and list(np.diff(fit["out_off"].astype(np.int64))) == list(res["out_len"][:3])
        r = EH.model_run(proto, [fit])[0]
        assert list(r["rstatus"][:3]) == [0, 0, 0] and list(r["out_len"][:3]) == list(res["out_len"][:3])
        for first in (None, 1):
            short = EH.short_by_one(b, res, 1, first)
            assert short["out_off"][2] - short["out_off"][1] == res["out_len"][1] - 1
            r = EH.model_run(proto, [short])[0]
            assert list(r["rstatus"][:3]) == [0, C.RES_SPACE, after] and r["out_len"][1] == 0


def test_corpus_size():
    assert EC.input_bytes() < 2 * 1000 * 1000
    assert max(int(b["data"].size) for g in GROUP_NAMES for b in EC.group(g)["calls"]) < 1 << 20


# ---- the corpus ----
@pytest.mark.parametrize("name,case", CASE_IDS, ids=["%s/%s" % x for x in CASE_IDS])
def test_case_hits(oracle_codec, name, case):
    """the case's "must hit" predicate over the model's result, in the merged batch the GPU sees"""
    g = EC.group(name)
    i = [c.name for c in g["cases"]].index(case)
    assert g["cases"][i].hit(EH.Ctx(g, i)), "%s no longer hits: %s" % (case, g["cases"][i].must)


def test_case_names_unique():
    for g in GROUP_NAMES:
        names = [c.name for c in EC.cases(g)]
        assert len(set(names)) == len(names)


@pytest.mark.parametrize("v", list(VARIANTS))
@pytest.mark.parametrize("name", GROUP_NAMES)
def test_restatement_guarded(oracle_codec, name, v):
    """the model under the guarded call: what the GPU test asks of the kernels holds for the restatement itself"""
    g = variant(name, v)
    EH.run(lambda sentinel: EH.ModelEnc(g["proto"], nconn(g)), g)
    if VARIANTS[v] is not None:
        for k, b in enumerate(g["calls"]):
            n = b["res"].size
            sizes = np.diff(b["out_off"].astype(np.int64))
            okay = g["exp"][k]["rstatus"][:n] == 0
            assert b["out_off"][0] == VARIANTS[v] and (sizes[okay] == g["exp"][k]["out_len"][:n][okay]).all()
            base = EC.group(name)["exp"][k]
            np.testing.assert_array_equal(g["exp"][k]["rstatus"][:n], base["rstatus"][:n])
            np.testing.assert_array_equal(g["exp"][k]["out_len"][:n], base["out_len"][:n])


@pytest.mark.parametrize("v", ["bound", "fit13"])
@pytest.mark.parametrize("name", GROUP_NAMES)
def test_reference(oracle_codec, name, v):
    """the compiled reference (h2o's own flatten functions through oracle/ref_hpenc.c / ref_shim.c) as the
    implementation, byte for byte against the restatement, for every case but REF_EXCLUDED"""
    from oracle import oracle as O

    excluded = {c.name: c.ref for g in GROUP_NAMES for c in EC.cases(g) if c.ref is not True}
    assert excluded == REF_EXCLUDED
    if not O.ref_available():
        pytest.skip("oracle/_ref not built (needs the reference tree)")
    g = variant(name, v, ref_only=True)
    EH.run(lambda sentinel: EH.ModelEnc(g["proto"], nconn(g), codec=O.ref()), g)


def _fields_in(b, r, proto):
    data, R = b["data"].tobytes(), b["res"][r]
    s = lambda o, n: data[int(o):int(o) + int(n)]  # noqa: E731
    hs = [(s(h["name_off"], h["name_len"]), s(h["value_off"], h["value_len"]))
          for h in b["hdr"][int(R["hdr_first"]):int(R["hdr_first"]) + int(R["nhdr"])]]
    fl = int(R["flags"])
    server = [(b"server", s(b["server_off"], b["server_len"]))] if fl & C.RES_SERVER and b["server_len"] else []
    cl = [(b"content-length", b"%d" % int(R["content_length"]))] if R["content_length"] != EH.NO_LENGTH else []
    if proto == "h":
        if fl & (C.RES_TRAILERS | C.RES_REQUEST | C.RES_PUSH_PROMISE):
            return hs
        return [(b":status", b"%d" % int(R["status"]))] + server + hs + cl
    dfid = [(b"datagram-flow-id", s(R["dfid_off"], R["dfid_len"]))] if fl & C.QRES_DATAGRAM else []
    if fl & C.QRES_REQUEST:
        return hs + dfid
    return [(b":status", b"%d" % (int(R["status"]) & 0xFFFF))] + server + cl + hs + dfid


def _decoded(d, first, count):
    a = d["arena"]
    return [(a[d["name_off"][f]:d["name_off"][f] + d["name_len"][f]].tobytes(),
             a[d["value_off"][f]:d["value_off"][f] + d["value_len"][f]].tobytes()) for f in range(first, first + count)]


@pytest.mark.parametrize("name", GROUP_NAMES)
def test_round_trip(oracle_codec, name):
    """every accepted block, decoded by the decoder restatement (oracle/hpack_block.c with the connection's table
    over all calls in wire order; oracle/qpack_decode.c), gives the fields that went in -- but ROUNDTRIP_EXCLUDED"""
    from oracle import oracle as O

    excluded = {c.name: c.roundtrip for g in GROUP_NAMES for c in EC.cases(g) if c.roundtrip is not True}
    assert excluded == ROUNDTRIP_EXCLUDED
    g = EC.group(name)
    proto = g["proto"]
    skip = set()  # (call, record) of the excluded cases
    for k, rows in enumerate(g["rows"]):
        for c, (lo, n, _) in zip(g["cases"], rows):
            if c.roundtrip is not True:
                skip |= {(k, r) for r in range(lo, lo + n)}
    blocks, want, per_conn = [], [], []
    for c in range(nconn(g)):
        mine = 0
        for k, b in enumerate(g["calls"]):
            for r in range(int(b["conn_first"][c]), int(b["conn_first"][c + 1])):
                if (k, r) in skip or g["exp"][k]["rstatus"][r] != 0:
                    continue
                o = int(b["out_off"][r])
                f = g["exp"][k]["out"][o:o + int(g["exp"][k]["out_len"][r])].tobytes()
                if proto == "h":
                    blocks.append(block_of(f)[0])
                else:
                    assert f[0] == 1
                    blocks.append(f[1 + (1 << (f[1] >> 6)):])
                want.append(_fields_in(b, r, proto))
                mine += 1
        per_conn.append(mine)
    assert blocks
    off = np.concatenate([[0], np.cumsum([len(x) for x in blocks])]).astype(np.uint32)
    data = np.frombuffer(b"".join(blocks), np.uint8)
    if proto == "h":
        d = O.oracle().hpack_decode_blocks(data, off, np.concatenate([[0], np.cumsum(per_conn)]).astype(np.uint32))
        status = d["bstatus"]
    else:
        arena_off = np.concatenate([[0], np.cumsum([4 * len(x) + 256 for x in blocks])]).astype(np.uint64)
        d = O.QpackSession(O.oracle(), 1).step(data, np.zeros(1, np.uint32), np.zeros(1, np.uint32), off,
                                               np.array([0, len(blocks)], np.uint32), arena_off)
        status = d["sstatus"]
    assert (status[:len(blocks)] == 0).all(), status[:len(blocks)]
    for k, fl in enumerate(want):
        assert _decoded(d, int(off[k]), int(d["nfields"][k])) == fl, "block %d" % k


# ---- the harness catches what it is for ----
def planted(name, fault, match):
    g = EC.group(name)
    impls = []

    def factory(sentinel):
        impls.append(EH.ModelEnc(g["proto"], nconn(g), fault))
        return impls[-1]

    with pytest.raises(AssertionError, match=match):
        EH.run(factory, g)
    assert impls[0].planted > 0, "the fault was never planted"


@pytest.mark.parametrize("name", ["h-regions", "q-regions"])
def test_catches_byte_past_out_len(oracle_codec, name):
    planted(name, "past", "past out_len written")


@pytest.mark.parametrize("name", ["h-regions", "q-regions"])
def test_catches_byte_in_refused_region(oracle_codec, name):
    planted(name, "refused", "short-one-frame.*refused record's region written")


def test_catches_name_index(oracle_codec):
    planted("h-table", "name_index", "bytes differ")


@pytest.mark.parametrize("name", ["h-strings", "q-strings"])
def test_catches_huffman_at_the_tie(oracle_codec, name):
    planted(name, "huff_tie", r"tie-raw-256\[0\]: bytes differ")


def test_catches_short_continuation_header(oracle_codec):
    planted("h-frames-other", "cont-1", "out_len = ")
