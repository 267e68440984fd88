"""HTTP/2 control frames (include/hhuff.h (2k')) without a GPU: the model (h2ctl_model.py) against h2o's own answers
(golden/h2ctl.npz, written by tools/gen_h2ctl_fixture.py from the real reference) and against the literal expectations
of the hand-built corpus (h2ctl_corpora.py); the corpus's coverage and its power to tell the model's defects apart; the
calls' argument checks; the header's constants; and tools/h2ctl_host.cpp -- the rules of h2o_amd/csrc/hhuff_h2ctl.h, the
code the kernel runs -- as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import h2ctl_corpora as K
import h2ctl_model as M
from conftest import ROOT, load_golden
from h2o_amd import codec as C


@pytest.fixture(scope="module")
def fx():
    return load_golden("h2ctl")


def run_case(c, defects=()):
    peer = M.copy_peer(c["peer"])
    frames = M.split_frames(c["buf"])
    cap = 17 * len(frames) if c["rep_cap"] is None else c["rep_cap"]
    w = M.walk(frames, peer, c["client"], c["rws"], cap, c["in_size"], defects)
    return (w["status"], w["err"], w["nctl"], w["records"], w["replies"],
            (peer["settings"], peer["flags"], peer["send_window"], peer["recv_window"]))


def expected(c):
    return (c["status"], c["err"], c["nctl"], c["records"], c["replies"], c["after"])


def probe(fx, i):
    p = bytes(fx["probes"][int(fx["probe_off"][i]):int(fx["probe_off"][i + 1])])
    return p[3], p[4], int.from_bytes(p[5:9], "big") & 0x7fffffff, p[9:]


DECODERS = {M.DATA: M.decode_data_payload, M.PRIORITY: M.decode_priority_payload, M.RST_STREAM: M.decode_rst_stream_payload,
            M.PING: M.decode_ping_payload, M.GOAWAY: M.decode_goaway_payload, M.WINDOW_UPDATE: M.decode_window_update_payload}


def test_fixture_shape(fx):
    n = fx["pret"].size
    assert n > 8000 and fx["probe_off"].size == n + 1 and fx["out"].shape == (n, 3) and fx["settings"].shape == (n, 5)
    types = np.array([probe(fx, i)[0] for i in range(n)])
    assert set(range(13)) - {1, 5, 9} <= set(types.tolist())
    assert set(np.unique(fx["pret"]).tolist()) == {-6, -3, -1, 0, 1}
    assert set(np.unique(fx["desc"]).tolist()) == set(M.ALL_ERR) - {M.E_SELF_DEPENDENCY, M.E_SETTINGS_STREAM_ID, M.E_SETTINGS_ACK,
                                                                   M.E_SETTINGS_SIZE, M.E_FLOW_CONTROL}  # the handlers' texts
    assert int(((fx["pret"] == -6) & (fx["desc"] == 0) & (types == 4)).sum()) > 0  # the SETTINGS size error has no text
    assert int(fx["stream_level"].sum()) > 0 and int(fx["replies"]) == 1
    assert fx["settings2_start"].tolist() == [0, 0, 7, 1000, 65536]


def test_model_gives_h2os_answers_frame_by_frame(fx):
    start2 = fx["settings2_start"].tolist()
    for i in range(fx["pret"].size):
        typ, flags, sid, pay = probe(fx, i)
        pret, desc = int(fx["pret"][i]), int(fx["desc"][i])
        out = [int(v) for v in fx["out"][i]]
        if typ in DECODERS:
            r = DECODERS[typ](len(pay), flags, sid, pay)
            assert r[0] == pret and (M.ERR_TEXT[r[1]] is not None or r[1] == 0) and r[1] == desc, (i, r)
            if pret == 0:
                got = {M.DATA: lambda: [r[2], r[3], 0], M.PRIORITY: lambda: [r[2], r[3], r[4]], M.RST_STREAM: lambda: [r[2], 0, 0],
                       M.PING: lambda: [M.be32(r[2]), M.be32(r[2], 4), 0], M.GOAWAY: lambda: [r[2], r[3], r[4]],
                       M.WINDOW_UPDATE: lambda: [r[2], 0, 0]}[typ]()
                assert got == out, (i, got, out)
            assert int(fx["stream_level"][i]) == (r[3] if typ == M.WINDOW_UPDATE and pret else 0), i
        elif typ == M.SETTINGS:
            for start, key, want in (([4096, 1, 0xFFFFFFFF, 65535, 16384], "settings", pret), (list(start2), "settings2",
                                                                                             int(fx["pret2"][i]))):
                ret, err, _ = M.update_peer_settings(start, pay)
                assert ret == want and start == fx[key][i].tolist(), (i, key)
                assert err == {0: M.E_NONE, -6: M.E_SETTINGS_SIZE}.get(ret, M.E_SETTINGS_FRAME), i
                if key == "settings":  # h2o's text: none for the size error
                    assert desc == (M.E_SETTINGS_FRAME if err == M.E_SETTINGS_FRAME else 0), i
        else:
            assert pret == 1


def test_model_writes_h2os_reply_bytes(fx):
    """h2o_http2_encode_ping_frame, _window_update_frame and h2o_http2__encode_rst_stream_frame against the model's"""
    seen = set()
    for i in range(fx["pret"].size):
        typ, flags, sid, pay = probe(fx, i)
        want = bytes(fx["reply"][int(fx["reply_off"][i]):int(fx["reply_off"][i + 1])])
        if typ == M.PING and len(pay) == 8:
            ret, rec, reply = M.handle(M.PING, 0, 0, pay, 9, M.new_peer())
            assert ret == 0 and reply == want and len(want) == 17, i
            seen.add("ping")
        elif typ == M.WINDOW_UPDATE and len(pay) == 4:
            inc = int(fx["out"][i][0])  # h2o's own increment: the model's connection WINDOW_UPDATE of that size
            if inc:  # a window of `inc` bytes drained by one byte of DATA
                peer = M.new_peer()
                peer["recv_window"] = 1
                _, _, wu = M.handle(M.DATA, 0, 1, b"x", 9, peer, False, inc)
                assert wu == want[:13] and peer["recv_window"] == inc, i
            if sid:
                _, rec, rst = M.handle(M.WINDOW_UPDATE, 0, sid, b"\0\0\0\0", 9, M.new_peer())
                assert rst == want[13:] and rec[2] == -1, i
                seen.add("rst")
            seen.add("wu")
        else:
            assert want == b""
    assert seen == {"ping", "wu", "rst"}


@pytest.mark.parametrize("c", K.CASES, ids=[c["name"] for c in K.CASES])
def test_model_gives_the_corpus_expectations(c):
    assert run_case(c) == expected(c)
    w = run_case(c)
    assert sum(r[5] for r in w[3]) == len(w[4])  # the records' reply lengths add up to the replies


def test_corpus_covers_every_status_error_flag_and_reply():
    names = [c["name"] for c in K.CASES]
    assert len(set(names)) == len(names)
    assert {c["status"] for c in K.CASES} == set(M.ALL_STATUS)
    assert {c["err"] for c in K.CASES} | {r[3] for c in K.CASES for r in c["records"]} == set(M.ALL_ERR)
    seen = 0
    for c in K.CASES:
        for r in c["records"]:
            seen |= r[4]
    assert seen == sum(M.ALL_FLAGS)
    kinds = set()
    for c in K.CASES:
        for typ, fl, sid, pay, _ in M.split_frames(c["replies"]):
            kinds.add((typ, fl, len(pay), sid != 0))
    assert kinds == {(M.SETTINGS, 1, 0, False), (M.PING, 1, 8, False), (M.RST_STREAM, 0, 4, True), (M.WINDOW_UPDATE, 0, 4, False)}
    assert {len(M.split_frames(c["buf"])) for c in K.CASES} >= {0, 1, 2, 3}
    assert any(c["client"] for c in K.CASES) and any(c["rws"] for c in K.CASES)
    assert any(c["peer"] != M.new_peer() for c in K.CASES)
    assert any(c["status"] < 0 and c["nctl"] > 0 and c["replies"] for c in K.CASES)


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_corpus_tells_each_defect(defect):
    assert any(run_case(c, (defect,)) != expected(c) for c in K.CASES), defect


def test_batch_model_places_records_and_replies():
    by = {c["name"]: c for c in K.CASES}
    conns = [by["failure_in_the_middle"]["buf"], b"", by["ping_8"]["buf"]]
    r = M.batch(conns, [6, 0, 2])
    assert r["nframes"].tolist() == [5, 0, 1] and r["nctl"].tolist() == [2, 0, 1] and r["ctl_status"].tolist() == [-6, 0, 0]
    assert r["ctl_used"].tolist() == [True, True, True, False, False, False, True, False]
    assert r["rep_off"].tolist() == [0, 102, 102, 136] and r["rep_len"].tolist() == [26, 0, 17]
    assert bytes(r["rep"][102:119]) == K.PONG(K.OPAQUE) and int(r["ctl"]["a"][6]) == 0x01020304
    assert r["peers_out"]["header_table_size"].tolist() == [128, 4096, 4096]


def test_calls_check_their_arguments_without_a_gpu():
    """HHUFF_EINVAL before any device call: a NULL array, in_size >= 2^32, an unknown flag bit, recv_window_size above
    INT32_MAX; nconn == 0 returns 0"""
    L = C.lib()
    p = 1 << 20  # a dummy address: never dereferenced on these paths
    names = ("data", "in_size", "frames", "nframes", "frm_first", "frm_cap", "nconn", "flags", "rws", "peers_in", "peers_out", "ctl",
             "nctl", "cstatus", "cerr", "rep", "rep_size", "rep_off", "rep_len", "stream")
    default = dict(data=p, in_size=64, frames=p, nframes=p, frm_first=p, frm_cap=4, nconn=2, flags=0, rws=0, peers_in=p, peers_out=p,
                   ctl=p, nctl=p, cstatus=p, cerr=p, rep=p, rep_size=68, rep_off=p, rep_len=p, stream=None)
    call = lambda **k: L.hhuff_h2_control(*[k.get(a, default[a]) for a in names])  # noqa: E731
    for a in ("data", "frames", "nframes", "frm_first", "peers_in", "peers_out", "ctl", "nctl", "cstatus", "cerr", "rep", "rep_off",
              "rep_len"):
        assert call(**{a: None}) == -1, a
        assert call(**{a: None, "nconn": 0}) == -1, a
    assert call(in_size=1 << 32) == -1 and call(in_size=(1 << 32) - 1, nconn=0) == 0
    assert call(flags=2) == -1 and call(flags=3) == -1 and call(flags=1 << 31) == -1
    assert call(rws=1 << 31) == -1 and call(rws=0xFFFFFFFF) == -1 and call(rws=(1 << 31) - 1, nconn=0) == 0
    assert call(flags=C.H2C_CLIENT, nconn=0) == 0 and call(nconn=0) == 0
    sp = L.hhuff_hpack_responses_set_peers
    assert sp(None, p, p, 1, 1, None) == -1 and sp(p, None, p, 1, 1, None) == -1 and sp(p, p, None, 1, 1, None) == -1
    assert sp(None, p, p, 0, 0, None) == -1 and sp(p, p, p, 0, 5, None) == 0 and sp(p, p, p, 5, 0, None) == 0


def test_header_compiles_and_constants_match(tmp_path):
    text = open(os.path.join(ROOT, "include", "hhuff.h")).read()
    defs = {k: int(v.rstrip("u")) for k, v in re.findall(r"#define\s+(HHUFF_H2[CPR]_\w+)\s+\(?(-?\d+u?)\)?", text)}
    py = dict(HHUFF_H2C_CLIENT=C.H2C_CLIENT, HHUFF_H2C_SPACE=C.H2C_SPACE, HHUFF_H2C_EINVAL=C.H2C_EINVAL,
              HHUFF_H2P_SETTINGS=C.H2P_SETTINGS, HHUFF_H2P_GOAWAY=C.H2P_GOAWAY, HHUFF_H2R_ACK=C.H2R_ACK,
              HHUFF_H2R_NEEDS_STREAM=C.H2R_NEEDS_STREAM, HHUFF_H2R_STREAM_ERROR=C.H2R_STREAM_ERROR,
              HHUFF_H2R_WINDOW_DELTA=C.H2R_WINDOW_DELTA, HHUFF_H2R_WINDOW_UPDATE=C.H2R_WINDOW_UPDATE)
    for name in ("NONE", "DATA_STREAM_ID", "DATA_FRAME", "PRIORITY_STREAM_ID", "PRIORITY_FRAME", "SELF_DEPENDENCY",
                 "RST_STREAM_STREAM_ID", "RST_STREAM_FRAME", "SETTINGS_STREAM_ID", "SETTINGS_ACK", "SETTINGS_FRAME", "SETTINGS_SIZE",
                 "PING_FRAME", "GOAWAY_STREAM_ID", "GOAWAY_FRAME", "WINDOW_UPDATE_FRAME", "FLOW_CONTROL"):
        py["HHUFF_H2C_ERR_" + name] = getattr(C, "H2C_ERR_" + name)
        assert getattr(M, "E_" + name) == getattr(C, "H2C_ERR_" + name)
    assert defs == py
    assert (M.SPACE, M.EINVAL, M.CLIENT, M.P_SETTINGS, M.P_GOAWAY) == (C.H2C_SPACE, C.H2C_EINVAL, C.H2C_CLIENT, C.H2P_SETTINGS,
                                                                      C.H2P_GOAWAY)
    assert (M.PROTOCOL, M.FLOW_CONTROL, M.FRAME_SIZE) == (C.ERR_PROTOCOL, C.ERR_FLOW_CONTROL, C.ERR_FRAME_SIZE)
    assert M.ALL_FLAGS == (C.H2R_ACK, C.H2R_NEEDS_STREAM, C.H2R_STREAM_ERROR, C.H2R_WINDOW_DELTA, C.H2R_WINDOW_UPDATE)
    assert M.ALL_ERR == tuple(sorted(v for k, v in py.items() if k.startswith("HHUFF_H2C_ERR_")))
    # the comment beside each HHUFF_H2C_ERR_* quotes h2o's text
    for name, val, text_ in re.findall(r'#define\s+HHUFF_H2C_ERR_(\w+)\s+(\d+)u\s+/\* "([^"]+)" \*/', text):
        assert M.ERR_TEXT[int(val)] == text_, name
    # the shared rules take their codes from the header, and h2o's three from http2_common.h
    rules = open(os.path.join(ROOT, "h2o_amd", "csrc", "hhuff_h2ctl.h")).read()
    assert re.search(r"kProtocol = -1, kFlowControl = -3, kFrameSize = -6;", rules)
    assert set(re.findall(r"HHUFF_H2C_ERR_\w+", rules)) == {k for k in py if k.startswith("HHUFF_H2C_ERR_")}
    assert set(re.findall(r"HHUFF_H2[PR]_\w+", rules)) == {k for k in py if k[:10] in ("HHUFF_H2P_", "HHUFF_H2R_")}
    assert C.H2_PEER_DTYPE.itemsize == 40 and C.H2_CTL_DTYPE.itemsize == 16
    assert tuple(M.peers_array([M.new_peer()])[0]) == C.H2_PEER_INIT
    for name in ("hhuff_h2_control", "hhuff_hpack_responses_set_peers"):
        assert name in C.EXPORTED and hasattr(C.lib(), name)
    assert C.h2_control_reply_bound(7) == 119
    if not shutil.which("gcc"):
        pytest.skip("no host compiler")
    dts = (("hhuff_h2_peer_t", C.H2_PEER_DTYPE), ("hhuff_h2_ctl_t", C.H2_CTL_DTYPE))
    fields = ", ".join("(int)offsetof(%s, %s)" % (t, n) for t, dt in dts for n in dt.names)
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hhuff.h"\n'
                   "int main(void) {\n"
                   "    hhuff_h2_peer_t p = HHUFF_H2_PEER_INIT;\n"
                   "    int f[] = {%s};\n"
                   "    unsigned i;\n"
                   "    printf(\"%%d %%d %%d\", (int)sizeof(hhuff_h2_peer_t), (int)sizeof(hhuff_h2_ctl_t), (int)hhuff_h2_control_reply_bound(7));\n"
                   "    for (i = 0; i != sizeof(f) / sizeof(f[0]); ++i) printf(\" %%d\", f[i]);\n"
                   "    printf(\" %%u %%u %%u %%u %%u %%u %%ld %%ld\", p.header_table_size, p.enable_push, p.max_concurrent_streams,\n"
                   "           p.initial_window_size, p.max_frame_size, p.flags, (long)p.send_window, (long)p.recv_window);\n"
                   "    return 0;\n"
                   "}\n" % fields)
    exe = str(tmp_path / "t")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    want = [40, 16, 119] + [dt.fields[n][1] for _, dt in dts for n in dt.names] + list(C.H2_PEER_INIT)
    assert got == want


def case_line(c):
    peer = lambda p: "%d %d %d %d %d %d %d %d" % (tuple(p[0]) + tuple(p[1:]))  # noqa: E731
    start = (c["peer"]["settings"], c["peer"]["flags"], c["peer"]["send_window"], c["peer"]["recv_window"])
    frames = M.split_frames(c["buf"])
    cap = 17 * len(frames) if c["rep_cap"] is None else c["rep_cap"]
    recs = " ".join("%d %d %d %d %d %d" % r for r in c["records"])
    return "%d %d %d %d %s %d %d %d %s %d %s %s %s\n" % (
        c["client"], c["rws"], cap, -1 if c["in_size"] is None else c["in_size"], peer(start), c["status"], c["err"], c["nctl"],
        peer(c["after"]), len(c["records"]), recs, c["replies"].hex() or "-", c["buf"].hex() or "-")


def test_h2ctl_host_clean_under_sanitizers(tmp_path):
    """tools/h2ctl_host.cpp over the corpus (its expectations included), every truncation of every corpus connection
    and 20,000 seeded mutations of bytes and of frame records"""
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
    exe = str(tmp_path / "h2ctl_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *san, "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "h2o_amd", "csrc"),
                    os.path.join(ROOT, "tools", "h2ctl_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(cases), "20000"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.rstrip().endswith("ok: h2ctl_host"), r.stdout
    assert "%d cases" % len(K.CASES) in r.stdout and "20000 mutations" in r.stdout
    assert int(re.search(r"(\d+) refused as out of range", r.stdout).group(1)) > 100
