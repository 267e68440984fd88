"""The HTTP/3 de-framer (include/hhuff.h (2l)) without a GPU: the model (h3frames_model.py) against h2o's own answers
(golden/h3frames.npz, written by tools/gen_h3frames_fixture.py from the real reference) and against the literal
expectations of the hand-built corpus (h3frames_corpora.py); the corpus's coverage and its power to tell the model's
defects apart; the call's argument checks; the header's constants; and tools/h3frames_host.cpp -- the rules of
h2o_amd/csrc/hhuff_h3frames.h, the code the kernels run -- as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import h3frames_corpora as K
import h3frames_model as M
from conftest import ROOT, load_golden
from h2o_amd import codec as C

KEYS = ("status", "err", "consumed", "frames", "out", "section", "enc", "settings")


@pytest.fixture(scope="module")
def fx():
    return load_golden("h3frames")


def outcome(c, w):
    """a walk's result in the corpus's terms"""
    b, g = c["buf"], w["settings"]
    cut = lambda r: None if r is None else b[r[0]:r[0] + r[1]]  # noqa: E731
    return dict(status=w["status"], err=w["err"], consumed=w["consumed"],
                frames=[(f["type"], f["avail"], f["aux"]) for f in w["frames"]],
                out=(w["out"]["kind"], w["out"]["phase"], w["out"]["data_left"]), section=cut(w["section"]), enc=cut(w["enc"]),
                settings=None if g is None else (M.sat32(g["max_table_capacity"]), M.sat32(g["max_blocked"]),
                                                 g["max_field_section_size"], g["h3_datagram"]))


def run_case(c, defects=()):
    return M.walk(c["buf"], c["st"], c["cap"], c["mfps"], c["flags"], defects)


def probe(fx, i):
    return bytes(fx["probes"][int(fx["probe_off"][i]):int(fx["probe_off"][i + 1])])


DESC = {M.E_NONE: 0, M.E_FRAME_TOO_LARGE: 1, M.E_MALFORMED_SETTINGS: 2, M.E_INVALID_PRIORITY: 3, M.E_INVALID_GOAWAY: 4}


def check_probe(fx, i):
    """the model's function against h2o's on probe i"""
    p, mode, ret, desc = probe(fx, i), int(fx["mode"][i]), int(fx["ret"][i]), int(fx["desc"][i])
    a, v = [int(x) for x in fx["arg"][i]], [int(x) for x in fx["val"][i]]
    if mode == 0:
        r, err, typ, length, hdr, pos = M.read_frame(p, 0, len(p), a[2], bool(a[0]), bool(a[1]))
        assert (r, DESC[err]) == (ret, desc), i
        assert (M.NONE64 if typ is None else typ) == v[0], i  # (the type is there whenever its varint was whole)
        if ret != M.INCOMPLETE:
            assert (length, hdr) == (v[1], v[2]), i
        assert pos == v[3], i
        if ret == 0:
            assert pos == (hdr if typ == M.DATA else hdr + length), i
    elif mode == 1:
        r, s = M.handle_settings_frame(p, bool(a[0]))
        assert (r, 2 if r else 0) == (ret, desc), i
        if r == 0:  # (the fixture's encoder_table_capacity of 2^32 - 1 makes h2o's clamp the saturation)
            assert (s["max_field_section_size"], M.sat32(s["max_table_capacity"]), s["max_blocked"], s["h3_datagram"]) == tuple(v), i
    elif mode == 2:
        r, err, idlen = M.decode_priority_update_frame(p, bool(a[0]))
        assert (r, DESC[err]) == (ret, desc), i
        if r == 0:
            element = M.quicint(p, 0, len(p))[0]
            assert idlen == v[1] and ((1 << 63) - 1 if element is None else element) == v[0], i
    else:
        r, err, idlen = M.decode_goaway_frame(p)
        assert (r, DESC[err]) == (ret, desc), i
        if r == 0:
            assert M.quicint(p, 0, len(p)) == (v[0], len(p)) and idlen == len(p), i


def test_fixture_shape(fx):
    n = fx["ret"].size
    assert n > 5000 and fx["probe_off"].size == n + 1 and fx["val"].shape == (n, 4) and fx["arg"].shape == (n, 4)
    assert set(np.unique(fx["mode"]).tolist()) == {0, 1, 2, 3}
    rf = fx["mode"] == 0
    assert set(np.unique(fx["ret"][rf]).tolist()) == {0, M.INCOMPLETE, M.GENERAL_PROTOCOL, M.FRAME_UNEXPECTED}
    assert set(np.unique(fx["ret"][~rf]).tolist()) == {0, M.FRAME}
    assert set(np.unique(fx["desc"]).tolist()) == {0, 1, 2, 4}  # (3, "invalid PRIORITY frame": h2o never says it)
    cut = (fx["mode"] == 2) & (fx["ret"] == 0) & (fx["val"][:, 0] == (1 << 63) - 1)
    assert int(cut.sum()) > 0 and (fx["arg"][cut, 0] == 1).all() and (fx["val"][cut, 1] == 1).all()  # a push id cut short passes
    assert int(((fx["mode"] == 2) & (fx["ret"] == M.FRAME) & (fx["desc"] == 0)).sum()) > 0  # an element id of the wrong kind
    assert int((rf & (fx["val"][:, 2] == 16)).sum()) > 0  # two 8-byte varints


def test_model_gives_h2os_answers_probe_by_probe(fx):
    for i in range(fx["ret"].size):
        check_probe(fx, i)


@pytest.mark.parametrize("c", K.CASES, ids=[c["name"] for c in K.CASES])
def test_model_gives_the_corpus_expectations(c):
    w = run_case(c)
    got = outcome(c, w)
    assert got == {k: c[k] for k in KEYS}
    at = 0
    for f in w["frames"]:  # the records agree among themselves
        assert f["hdr_off"] >= at and f["payload_off"] + f["avail"] <= len(c["buf"]) and f["avail"] <= f["length"]
        at = f["payload_off"] + f["avail"]
    assert at <= w["consumed"] <= len(c["buf"])


def test_corpus_covers_every_status_error_kind_phase_and_flag():
    names = [c["name"] for c in K.CASES]
    assert len(set(names)) == len(names)
    assert {c["status"] for c in K.CASES} == set(M.ALL_STATUS)
    # every HHUFF_H3F_ERR_* but _INVALID_PRIORITY: h2o's test for it compares a 63-bit field with UINT64_MAX
    # (lib/http3/frame.c:49) and never fires, as golden/h3frames.npz confirms, so no input can produce it
    assert {c["err"] for c in K.CASES} == set(M.ALL_ERR) - {M.E_INVALID_PRIORITY}
    assert {c["st"]["kind"] for c in K.CASES} >= set(M.ALL_KINDS) and {c["out"][0] for c in K.CASES} >= set(M.ALL_KINDS)
    flags = 0
    for c in K.CASES:
        flags |= c["st"]["flags"] if c["status"] != M.EINVAL else 0
    assert flags == sum(M.ALL_STATE_FLAGS)
    moves = {(c["st"]["kind"], c["st"]["phase"], c["out"][0], c["out"][1]) for c in K.CASES if c["status"] != M.EINVAL}
    R, U, CT = M.K_REQUEST, M.K_UNI, M.K_CONTROL
    want = {(R, M.P_HEADERS, R, M.P_HEADERS), (R, M.P_HEADERS, R, M.P_DATA), (R, M.P_HEADERS, R, M.P_POST_TRAILERS),
            (R, M.P_HEADERS, R, M.P_DATA_PAYLOAD), (R, M.P_DATA, R, M.P_DATA), (R, M.P_DATA, R, M.P_DATA_PAYLOAD),
            (R, M.P_DATA, R, M.P_POST_TRAILERS), (R, M.P_DATA_PAYLOAD, R, M.P_DATA), (R, M.P_DATA_PAYLOAD, R, M.P_DATA_PAYLOAD),
            (R, M.P_POST_TRAILERS, R, M.P_POST_TRAILERS), (U, 0, U, 0), (U, 0, CT, M.P_SETTINGS), (U, 0, CT, M.P_OPEN),
            (U, 0, M.K_QPACK_ENCODER, 0), (U, 0, M.K_QPACK_DECODER, 0), (U, 0, M.K_DISCARD, 0), (CT, M.P_SETTINGS, CT, M.P_SETTINGS),
            (CT, M.P_SETTINGS, CT, M.P_OPEN), (CT, M.P_OPEN, CT, M.P_OPEN)}
    assert moves >= want, want - moves
    assert {c["flags"] for c in K.CASES} == {0, M.CLIENT}
    aux = {f[2] for c in K.CASES for f in c["frames"]}
    assert M.NOSEC in aux and {1, 2, 4} <= aux
    assert any(c["settings"] and c["settings"][3] for c in K.CASES) and any(c["settings"] and c["settings"][0] == 0xFFFFFFFF for c in K.CASES)
    assert (M.ALL_STATUS, M.CLIENT) == ((0, C.H3_GENERAL_PROTOCOL, C.H3_FRAME_UNEXPECTED, C.H3_FRAME, C.H3_EXCESSIVE_LOAD, C.H3F_REJECTED,
                                         C.H3F_FRAMES, C.H3F_EINVAL), C.H3F_CLIENT)


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_corpus_tells_each_defect(defect):
    """every defect of the model is told from h2o by some case: none is left that the corpus cannot tell"""
    assert any(outcome(c, run_case(c, (defect,))) != {k: c[k] for k in KEYS} for c in K.CASES), defect


def test_batch_model_places_sections_encoder_bytes_and_settings():
    for flags in (0, M.CLIENT):
        conns = K.connections(flags)
        assert any(len(c) == 0 for c in conns) and any(len(c) == 3 for c in conns)
        e = M.batch(conns, flags=flags, arena_fixed=1024, arena_per_byte=16)
        nsec, sec_bytes, enc_bytes = (int(x) for x in e["totals"])
        assert nsec == sum(1 for w in e["walks"] if w["section"]) and e["out"].size == sec_bytes + enc_bytes
        assert int(e["conn_first"][-1]) == nsec and (np.diff(e["conn_first"].astype(np.int64)) >= 0).all()
        assert int(e["enc_len"].sum()) == enc_bytes and (e["sec_off"][nsec:] == sec_bytes + enc_bytes).all()
        assert int(e["arena_off"][-1]) == 1024 * nsec + 16 * sec_bytes
    e = M.batch(K.connections(0))
    c = e["conn_str"].size - 2  # the connection with two encoder and two control streams
    assert bytes(e["out"][int(e["enc_off"][c]):int(e["enc_off"][c]) + int(e["enc_len"][c])]) == b"firstsecond"
    assert int(e["got_settings"][c]) == 1 and int(e["peers"]["max_table_capacity"][c]) == 111
    k = int(e["conn_first"][c])
    assert int(e["conn_first"][c + 1]) == k + 2 and e["sec_stream_id"][k:k + 2].tolist() == [0, 4]
    assert bytes(e["out"][int(e["sec_off"][k + 1]):int(e["sec_off"][k + 2])]) == b"sec2"


def test_call_checks_its_arguments_without_a_gpu():
    """HHUFF_EINVAL before any device call: a NULL array (arena_off may be NULL), in_size > 2^32 - 3, an unknown flag
    bit; nstr == 0 or nconn == 0 returns 0"""
    L = C.lib()
    p = 1 << 20  # a dummy address: never dereferenced on these paths
    names = ("data", "in_size", "str_off", "nstr", "conn_str", "nconn", "frm_first", "frm_cap", "mfps", "flags", "st_in", "st_out",
             "frames", "nframes", "consumed", "sstatus", "serr", "out", "enc_off", "enc_len", "sec_off", "conn_first", "sec_stream_id",
             "sec_stream", "totals", "peers", "settings", "got_settings", "arena_off", "arena_fixed", "arena_per_byte", "stream")
    arrays = [n for n in names if n not in ("in_size", "nstr", "nconn", "frm_cap", "mfps", "flags", "arena_off", "arena_fixed",
                                            "arena_per_byte", "stream")]
    default = dict({n: p for n in arrays}, in_size=64, nstr=3, nconn=2, frm_cap=4, mfps=16384, flags=0, arena_off=None, arena_fixed=0,
                   arena_per_byte=0, stream=None)
    call = lambda **k: L.hhuff_h3_deframe(*[k.get(a, default[a]) for a in names])  # noqa: E731
    assert len(arrays) == 22
    for a in arrays:
        assert call(**{a: None}) == -1, a
        assert call(**{a: None, "nstr": 0}) == -1 and call(**{a: None, "nconn": 0}) == -1, a
    assert call(in_size=(1 << 32) - 2) == -1 and call(in_size=1 << 40) == -1
    assert call(in_size=(1 << 32) - 3, nstr=0) == 0 and call(nconn=0) == 0 and call(nstr=0, nconn=0) == 0
    assert call(flags=2) == -1 and call(flags=3) == -1 and call(flags=1 << 31) == -1
    assert call(flags=C.H3F_CLIENT, nstr=0) == 0 and call(mfps=0, nconn=0) == 0 and call(mfps=(1 << 64) - 1, nstr=0) == 0


def test_header_compiles_and_constants_match(tmp_path):
    text = open(os.path.join(ROOT, "include", "hhuff.h")).read()
    defs = {k: int(v.rstrip("u")) for k, v in re.findall(r"#define\s+(HHUFF_H3[FKPS]_\w+)\s+\(?(-?\d+u?)\)?", text)}
    py = dict(HHUFF_H3F_CLIENT=C.H3F_CLIENT, HHUFF_H3F_REJECTED=C.H3F_REJECTED, HHUFF_H3F_FRAMES=C.H3F_FRAMES,
              HHUFF_H3F_EINVAL=C.H3F_EINVAL, HHUFF_H3F_ERR_NONE=C.H3F_ERR_NONE, HHUFF_H3F_ERR_FRAME_TOO_LARGE=C.H3F_ERR_FRAME_TOO_LARGE,
              HHUFF_H3F_ERR_UNEXPECTED_TYPE=C.H3F_ERR_UNEXPECTED_TYPE, HHUFF_H3F_ERR_DATA_BEFORE_HEADERS=C.H3F_ERR_DATA_BEFORE_HEADERS,
              HHUFF_H3F_ERR_RESPONSE_TOO_LARGE=C.H3F_ERR_RESPONSE_TOO_LARGE, HHUFF_H3F_ERR_MALFORMED_SETTINGS=C.H3F_ERR_MALFORMED_SETTINGS,
              HHUFF_H3F_ERR_INVALID_PRIORITY=C.H3F_ERR_INVALID_PRIORITY, HHUFF_H3F_ERR_INVALID_GOAWAY=C.H3F_ERR_INVALID_GOAWAY,
              HHUFF_H3K_REQUEST=C.H3K_REQUEST, HHUFF_H3K_UNI=C.H3K_UNI, HHUFF_H3K_CONTROL=C.H3K_CONTROL,
              HHUFF_H3K_QPACK_ENCODER=C.H3K_QPACK_ENCODER, HHUFF_H3K_QPACK_DECODER=C.H3K_QPACK_DECODER, HHUFF_H3K_DISCARD=C.H3K_DISCARD,
              HHUFF_H3P_HEADERS=C.H3P_HEADERS, HHUFF_H3P_DATA=C.H3P_DATA, HHUFF_H3P_DATA_PAYLOAD=C.H3P_DATA_PAYLOAD,
              HHUFF_H3P_POST_TRAILERS=C.H3P_POST_TRAILERS, HHUFF_H3P_SETTINGS=C.H3P_SETTINGS, HHUFF_H3P_OPEN=C.H3P_OPEN,
              HHUFF_H3S_WALK_ON=C.H3S_WALK_ON, HHUFF_H3S_TUNNEL=C.H3S_TUNNEL, HHUFF_H3S_PEER_DATAGRAMS=C.H3S_PEER_DATAGRAMS)
    assert defs == py
    assert (M.REJECTED, M.FRAMES, M.EINVAL, M.CLIENT) == (C.H3F_REJECTED, C.H3F_FRAMES, C.H3F_EINVAL, C.H3F_CLIENT)
    assert M.ALL_ERR == tuple(sorted(v for k, v in py.items() if k.startswith("HHUFF_H3F_ERR_")))
    assert M.ALL_KINDS == tuple(sorted(v for k, v in py.items() if k.startswith("HHUFF_H3K_")))
    assert M.ALL_STATE_FLAGS == tuple(sorted(v for k, v in py.items() if k.startswith("HHUFF_H3S_")))
    assert (M.P_HEADERS, M.P_DATA, M.P_DATA_PAYLOAD, M.P_POST_TRAILERS, M.P_SETTINGS, M.P_OPEN) == \
        (C.H3P_HEADERS, C.H3P_DATA, C.H3P_DATA_PAYLOAD, C.H3P_POST_TRAILERS, C.H3P_SETTINGS, C.H3P_OPEN)
    assert (M.GENERAL_PROTOCOL, M.FRAME_UNEXPECTED, M.FRAME, M.EXCESSIVE_LOAD) == \
        (C.H3_GENERAL_PROTOCOL, C.H3_FRAME_UNEXPECTED, C.H3_FRAME, C.H3_EXCESSIVE_LOAD)
    dts = (("hhuff_h3_stream_t", C.H3_STREAM_DTYPE, M.STREAM_DT, 32), ("hhuff_h3_frame_t", C.H3_FRAME_DTYPE, M.FRAME_DT, 32),
           ("hhuff_h3_settings_t", C.H3_SETTINGS_DTYPE, M.SETTINGS_DT, 16), ("hhuff_qpack_peer_t", C.QPACK_PEER, M.PEER_DT, 8))
    for _, dt, mdt, size in dts:
        assert dt.itemsize == size and dt == mdt
    assert "hhuff_h3_deframe" in C.EXPORTED and hasattr(C.lib(), "hhuff_h3_deframe")
    if not shutil.which("gcc") or not shutil.which("g++"):
        pytest.skip("no host compiler")
    fields = ", ".join("(int)offsetof(%s, %s)" % (t, n) for t, dt, _, _ in dts for n in dt.names)
    sizes = ", ".join("(int)sizeof(%s)" % t for t, _, _, _ in dts)
    body = ('#include <stddef.h>\n#include <stdio.h>\n#include "hhuff.h"\n'
            "int main(void) {\n"
            "    int f[] = {%s, %s};\n"
            "    unsigned i;\n"
            "    for (i = 0; i != sizeof(f) / sizeof(f[0]); ++i) printf(\" %%d\", f[i]);\n"
            "    return 0;\n"
            "}\n" % (sizes, fields))
    want = [s for _, _, _, s in dts] + [dt.fields[n][1] for _, dt, _, _ in dts for n in dt.names]
    for cc, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        src = tmp_path / ("t." + ext)
        src.write_text(body)
        exe = str(tmp_path / ("t_" + ext))
        subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                       check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
        assert got == want, cc


def case_line(c):
    """one line of tools/h3frames_host.cpp's input"""
    s = c["st"]
    return "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %s\n" % (
        c["flags"] & M.CLIENT, c["mfps"], c["cap"], s["kind"], s["phase"], s["flags"], s["rsv"], s["data_left"], c["status"], c["err"],
        c["consumed"], len(c["frames"]), c["out"][0], c["out"][1], c["out"][2], 0 if c["section"] is None else 1,
        len(c["section"] or b""), len(c["enc"] or b""), 0 if c["settings"] is None else 1, c["buf"].hex() or "-")


def test_h3frames_host_clean_under_sanitizers(tmp_path):
    """tools/h3frames_host.cpp over the corpus (its expectations included), every truncation of every corpus stream, each
    carried on over the rest, and 10,000 seeded mutations of bytes, states and parameters"""
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    probe_src = tmp_path / "probe.cpp"
    probe_src.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++", *san, str(probe_src), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes")
    cases = tmp_path / "cases.txt"
    with open(cases, "w") as f:
        for c in K.CASES:
            f.write(case_line(c))
    exe = str(tmp_path / "h3frames_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *san, "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "h2o_amd", "csrc"),
                    os.path.join(ROOT, "tools", "h3frames_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(cases), "10000"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.rstrip().endswith("ok: h3frames_host"), r.stdout
    assert "%d cases" % len(K.CASES) in r.stdout and "10000 mutations" in r.stdout
