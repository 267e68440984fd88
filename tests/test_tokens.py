"""Token interning (include/hhuff.h (2j)) without a GPU: the fixture of h2o's own list and h2o_lookup_token's answers
(tests/golden/tokens.npz, tools/gen_token_fixture.py), the host-side builder through the C ABI, the model
(tests/tokens_model.py), and the conditions the GPU tests (tests/test_tokens_gpu.py) stand on."""
import ctypes
import os
import re

import numpy as np
import pytest

import tokens_model as TM
from conftest import ROOT
from h2o_amd import codec as C
from h2o_amd import hpenc_synth as HE


@pytest.fixture(scope="module")
def fx():
    return TM.load_fixture()


def test_fixture_is_consistent(fx):
    names, probes, answer = fx["names"], fx["probes"], fx["answer"]
    assert len(names) == 85 and names == sorted(names) and len(set(names)) == 85
    assert sum(len(n) for n in names) == 1075 and max(len(n) for n in names) == 32
    assert fx["flags"].shape == (85, len(TM.FLAGS))
    assert probes[:85] == names and list(answer[:85]) == list(range(85))  # every name's answer is its own index
    assert 3000 < len(probes) == answer.size and answer.min() == -1 and answer.max() == 84
    assert set(n.upper() for n in names) <= set(probes) and all(n[:k] in set(probes) for n in names for k in range(1, len(n)))


def test_model_gives_h2o_lookup_token(fx):
    m = TM.Model(fx["names"])
    got = np.array([m.lookup(p) for p in fx["probes"]], np.int32)
    np.testing.assert_array_equal(got, fx["answer"])


def test_request_name_classes_are_tokens(fx):
    """the names hhuff_request.h classifies by byte comparison (req_name_class) are tokens of the list"""
    src = open(os.path.join(ROOT, "h2o_amd", "csrc", "hhuff_request.h")).read()
    body = src[src.index("uint32_t req_name_class("):src.index("req_strtosize")]
    lits = re.findall(r'bytes_eq\(s, "([^"]+)", (\d+)\)', body)
    classes = set(re.findall(r"\bkN[A-Z]\w*", body)) - {"kNRegular", "kNPseudoOther"}
    assert len(classes) == 13 and len(lits) == 16  # with kNPseudoOther (':' + no token's name): fourteen classes
    for lit, n in lits:
        assert len(lit) == int(n) and lit.encode() in fx["names"], lit


def _build(names, off, n, user, table, size):
    return C.lib().hhuff_tokens_build(names.ctypes.data, None if off is None else off.ctypes.data, n,
                                      None if user is None else user.ctypes.data, None if table is None else table.ctypes.data, size)


def test_table_size():
    f = C.tokens_table_size
    assert f(0, 0) == 0 and f(4097, 4097) == 0 and f(3, 2) == 0 and f(3, 3 * 255 + 1) == 0
    for nt, nb in ((1, 1), (1, 255), (85, 1075), (4096, 4096), (4096, 4096 * 255)):
        assert f(nt, nb) >= 32 + 8 * nt + nb and f(nt, nb) % 16 == 0
    assert f(85, 1075) <= 4096  # h2o's set: "about 4 KiB"


def test_build_is_deterministic_and_sized(fx):
    words = np.arange(85, dtype=np.uint32) * 3 + 1
    a, b = C.tokens_build(fx["names"], words), C.tokens_build(fx["names"], words)
    assert a.size == C.tokens_table_size(85, 1075) and a.tobytes() == b.tobytes()
    hdr = a[:16].view(np.uint32)
    assert a[:4].tobytes() == b"HHTK" and hdr[1] == 1 and hdr[2] == 85 and hdr[3] == a.size
    # a larger buffer: the same bytes, nothing behind them written
    blob = np.frombuffer(b"".join(fx["names"]), np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(n) for n in fx["names"]])]).astype(np.uint32)
    big = np.full(a.size + 64, 0xEE, np.uint8)
    assert _build(blob, off, 85, words, big, big.size) == 0
    assert big[:a.size].tobytes() == a.tobytes() and (big[a.size:] == 0xEE).all()
    # the words are the caller's: other words, the same table but for them
    c = C.tokens_build(fx["names"], None)
    assert c.size == a.size and c.tobytes() != a.tobytes()
    # a shifted name_off (names that do not begin at byte 0) is the same list
    blob2 = np.concatenate([np.zeros(5, np.uint8), blob])
    t2 = np.zeros(a.size, np.uint8)
    assert _build(blob2, off + 5, 85, words, t2, t2.size) == 0 and t2.tobytes() == a.tobytes()


def test_build_refusals():
    names = [b"alpha", b"beta", b"gamma"]
    blob = np.frombuffer(b"".join(names), np.uint8).copy()
    off = np.array([0, 5, 9, 14], np.uint32)
    size = C.tokens_table_size(3, 14)
    table = np.full(size + 64, 0xCD, np.uint8)

    def refused(rc):
        assert rc == -1 and (table == 0xCD).all()

    refused(_build(blob, off, 3, None, table, size - 1))  # a table_size below hhuff_tokens_table_size
    refused(_build(blob, off, 0, None, table, size))
    refused(_build(blob, np.array([0, 5, 5, 14], np.uint32), 3, None, table, size))  # an empty name
    refused(_build(blob, np.array([0, 5, 4, 14], np.uint32), 3, None, table, size))  # a decreasing name_off
    two = np.frombuffer(b"alphabetaalpha", np.uint8).copy()
    refused(_build(two, np.array([0, 5, 9, 14], np.uint32), 3, None, table, size + 64))  # two equal names
    long_ = np.full(256, ord("x"), np.uint8)
    refused(_build(long_, np.array([0, 256], np.uint32), 1, None, table, size + 64))  # a name over 255 bytes
    refused(_build(blob, None, 3, None, table, size))
    assert _build(blob, off, 3, None, None, size) == -1
    many = [b"n%d" % i for i in range(4097)]
    with pytest.raises(C.HhuffError):
        C.tokens_build(many)
    with pytest.raises(C.HhuffError):
        C.tokens_build([b"a", b"a"])
    assert _build(blob, off, 3, None, table, size) == 0 and (table[size:] == 0xCD).all()
    assert C.tokens_build([b"\x00", b"\x00\x00", bytes(range(256))[1:]]).size % 16 == 0  # any byte values, 255 bytes
    assert C.tokens_build(many[:4096]).size == C.tokens_table_size(4096, sum(len(n) for n in many[:4096]))


def test_device_calls_check_their_arguments_without_a_gpu(fx):
    """HHUFF_EINVAL before anything is enqueued: a NULL required array, a table under the header's size, a
    misaligned table; a count of 0 returns 0"""
    L = C.lib()
    p, st = 1 << 20, None  # a 16-byte aligned dummy address: never dereferenced on these paths
    strings = lambda **k: L.hhuff_intern_strings(*[k.get(a, d) for a, d in (  # noqa: E731
        ("table", p), ("size", 3088), ("data", p), ("in_size", 64), ("off", p), ("len", p), ("n", 4), ("token", p),
        ("user", None), ("miss", 0), ("stream", st))])
    fields = lambda **k: L.hhuff_intern_fields(*[k.get(a, d) for a, d in (  # noqa: E731
        ("table", p), ("size", 3088), ("arena", p), ("arena_size", 64), ("name_off", p), ("name_len", p), ("first", p),
        ("nfields", p), ("nblk", 2), ("nslots", 9), ("token", p), ("user", None), ("miss", 0), ("stream", st))])
    headers = lambda **k: L.hhuff_intern_headers(*[k.get(a, d) for a, d in (  # noqa: E731
        ("table", p), ("size", 3088), ("data", p), ("in_size", 64), ("hdr", p), ("nhdr", 3), ("keep", 1), ("token", None),
        ("stream", st))])
    for call, arrays in ((strings, ("data", "off", "len", "token")),
                         (fields, ("arena", "name_off", "name_len", "first", "nfields", "token")), (headers, ("data", "hdr"))):
        for a in arrays + ("table",):
            assert call(**{a: None}) == -1, a
        assert call(size=31) == -1 and call(table=p + 8) == -1
    assert strings(n=0, data=None, off=None, len=None, token=None) == 0
    assert fields(nblk=0, arena=None, first=None) == 0 and fields(nslots=0, arena=None, token=None) == 0
    assert headers(nhdr=0, hdr=None) == 0


def test_header_compiles_and_constants_match(tmp_path):
    import shutil
    import subprocess

    text = open(os.path.join(ROOT, "include", "hhuff.h")).read()
    defs = dict(re.findall(r"#define\s+(HHUFF_TOK_\w+)\s+\((-\d+)\)", text))
    assert {k: int(v) for k, v in defs.items()} == dict(HHUFF_TOK_NONE=C.TOK_NONE, HHUFF_TOK_EFORMAT=C.TOK_EFORMAT)
    assert (TM.TOK_NONE, TM.TOK_EFORMAT) == (C.TOK_NONE, C.TOK_EFORMAT)
    assert (TM.HDR_DONT_COMPRESS, TM.HDR_TOKEN, TM.HDR_LIKELY_TO_REPEAT) == (C.HDR_DONT_COMPRESS, C.HDR_TOKEN,
                                                                            C.HDR_LIKELY_TO_REPEAT)
    for name in ("hhuff_tokens_table_size", "hhuff_tokens_build", "hhuff_intern_strings", "hhuff_intern_fields",
                 "hhuff_intern_headers"):
        assert name in C.EXPORTED and hasattr(C.lib(), name)
    if not shutil.which("gcc"):
        pytest.skip("no host compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "hhuff.h"\n'
                   "int use(void *t, const uint8_t *in, const uint32_t *u, int32_t *tok, uint32_t *w, hhuff_hpack_header_t *h) {\n"
                   "    int rc = hhuff_tokens_build(in, u, 1, u, t, hhuff_tokens_table_size(1, 1));\n"
                   "    rc += hhuff_intern_strings(t, 96, in, 1, u, u, 1, tok, w, 0, 0);\n"
                   "    rc += hhuff_intern_fields(t, 96, in, 1, u, u, u, u, 1, 1, tok, w, 0, 0);\n"
                   "    rc += hhuff_intern_headers(t, 96, in, 1, h, 1, HHUFF_HDR_DONT_COMPRESS, tok, 0);\n"
                   "    return rc + HHUFF_TOK_NONE + HHUFF_TOK_EFORMAT;\n"
                   "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only",
                    "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


# ---------------------------------------------------------------------------------------------------
# the encoder sessions of the GPU tests (shared with tests/test_tokens_gpu.py)
# ---------------------------------------------------------------------------------------------------
def encoder_sessions(requests):
    """an hpenc_synth session in which every header that can be a token is one (notoken_frac=0): its first two steps"""
    if requests:
        return HE.make_request_session(64, steps=2, seed=81, notoken_frac=0.0, dont_compress_frac=0.1)
    return HE.make_session(64, steps=2, seed=80, notoken_frac=0.0, dont_compress_frac=0.1)


def qpack_sessions(requests):
    """the same once through to_qpack_sessions (which adds HHUFF_HDR_LIKELY_TO_REPEAT): two steps"""
    if requests:
        b = HE.make_request_session(64, seed=83, req_per_conn=(2, 4), big_frac=0.0, frame_frac=0.0, notoken_frac=0.0)[0]
    else:
        b = HE.make_session(64, seed=82, resp_per_conn=(2, 4), big_frac=0.0, trailers_frac=0.0, dont_compress_frac=0.05,
                            notoken_frac=0.0)[0]
    return HE.to_qpack_sessions(b, 2, seed=82, requests=requests, dfid_frac=0.1, odd_status_frac=0.0)


def strip(hdr):
    """the headers as a caller without tokens has them: only HHUFF_HDR_DONT_COMPRESS"""
    h = hdr.copy()
    h["flags"] &= ~np.uint32(C.HDR_TOKEN | C.HDR_LIKELY_TO_REPEAT)
    return h


def name_of(data, h):
    return bytes(data[int(h["name_off"]):int(h["name_off"]) + int(h["name_len"])])


@pytest.mark.parametrize("requests", [False, True])
def test_generated_sessions_flag_exactly_the_fixtures_tokens(fx, requests):
    """HHUFF_HDR_TOKEN exactly when the name is one of h2o's tokens, HHUFF_HDR_LIKELY_TO_REPEAT (QPACK sessions) exactly
    as the token's flag says: the hand-kept sets of hpenc_synth agree with the list, so hhuff_intern_headers can
    restore what strip() took (the model does here, the GPU in test_tokens_gpu.py)"""
    m = TM.Model(fx["names"], TM.encoder_words(fx["flags"]))
    ltr = fx["flags"][:, TM.FLAGS.index("likely_to_repeat")]
    seen = set()
    for steps, with_ltr in ((encoder_sessions(requests), False), (qpack_sessions(requests), True)):
        assert len(steps) == 2
        for st in steps:
            data = np.asarray(st["data"], np.uint8)
            for h in st["hdr"]:
                tok = m.lookup(name_of(data, h))
                assert bool(h["flags"] & C.HDR_TOKEN) == (tok >= 0), name_of(data, h)
                if with_ltr:
                    assert bool(h["flags"] & C.HDR_LIKELY_TO_REPEAT) == bool(tok >= 0 and ltr[tok]), name_of(data, h)
                seen.add(tok)
            want = m.user if with_ltr else m.user & ~np.uint32(C.HDR_LIKELY_TO_REPEAT)
            got, _ = TM.Model(fx["names"], want).intern_headers(data, strip(st["hdr"]))
            assert got.tobytes() == st["hdr"].tobytes()
    assert -1 in seen and len(seen) > 8


def test_model_slot_rule():
    m = TM.Model([b"a", b"bb"], [7, 9])
    arena = np.frombuffer(b"abbxa", np.uint8)
    first, nfields = np.array([0, 2, 2, 5]), np.array([5, 3, 2])  # clamped to 2; an empty range; two of three slots
    tok, user = m.intern_fields(arena, [0, 1, 3, 4, 0], [1, 2, 1, 1, 1], first, nfields, np.full(5, 77), np.full(5, 88), miss_user=5)
    assert list(tok) == [0, 1, -1, 0, 77] and list(user) == [7, 9, 5, 7, 88]
    assert m.find(arena, 4, 1, in_size=4) == -1 and m.find(arena, 0, 0) == -1 and m.lookup(b"A") == -1
    assert ctypes.sizeof(ctypes.c_uint32) * 5 == C.HPE_HEADER_DTYPE.itemsize
