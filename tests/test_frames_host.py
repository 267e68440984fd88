"""The HTTP/2 de-framer (include/hhuff.h (2k)) without a GPU: the model (frames_model.py) against h2o's own answers
(golden/frames.npz, written by tools/gen_frames_fixture.py from the real reference) and against the literal
expectations of the hand-built corpus (frames_corpora.py); the corpus's coverage and its power to tell the model's
defects apart; the call's argument checks; the header's constants; and tools/frames_host.cpp -- the rules of
h2o_amd/csrc/hhuff_frames.h, the code the kernels run -- as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import frames_corpora as K
import frames_model as M
from conftest import ROOT, load_golden
from h2o_amd import codec as C


@pytest.fixture(scope="module")
def fx():
    return load_golden("frames")


def outcome(w):
    return (w["status"], w["err"], w["consumed"], len(w["frames"]),
            [(b["stream_id"], b["end_stream_id"], b["flags"], b["dependency"], b["weight"], b["promised_stream_id"], b["nframes"],
              b["data"]) for b in w["blocks"]])


def expected(c):
    return (c["status"], c["err"], c["consumed"], c["nframes"], c["blocks"])


def run_case(c, defects=()):
    return M.walk(c["buf"], c["cap"], c["mfs"], c["mbb"], c["flags"], defects)


def probe(fx, i):
    return bytes(fx["probes"][int(fx["probe_off"][i]):int(fx["probe_off"][i + 1])])


def check_probe(fx, i):
    """the model's decode_frame / headers_payload against h2o's on probe i"""
    p = probe(fx, i)
    size, length, typ, fl, sid = M.decode_frame(p, 0, 16384)
    ret = int(fx["ret"][i])
    assert size == (0 if ret == -255 else ret), (i, size, ret)  # H2O_HTTP2_ERROR_INCOMPLETE: cstatus 0
    if ret >= 0 and typ == M.HEADERS:
        r, err, foff, flen, excl, dep, weight = M.headers_payload(p[9:9 + length], fl, sid, parity=False)
        assert r == int(fx["hret"][i]), i
        if r == 0:
            assert (foff, flen, excl, dep, weight) == tuple(int(fx[k][i]) for k in ("frag_off", "frag_len", "exclusive",
                                                                                      "dependency", "weight")), i
        else:  # h2o's err_desc; the cut-short priority field has none
            assert {M.E_HEADERS_STREAM_ID: 1, M.E_HEADERS_FRAME: 2, M.E_HEADERS_PRIORITY: 0}[err] == int(fx["desc"][i]), i
    else:
        assert int(fx["hret"][i]) == 1


def test_fixture_shape(fx):
    n = fx["ret"].size
    assert n > 5000 and fx["probe_off"].size == n + 1 and fx["file_probe0"].size == fx["file_off"].size
    assert int(fx["file_probe0"][-1]) <= n and int(fx["file_off"][-1]) == fx["files"].size
    assert set(np.unique(fx["ret"][fx["ret"] < 0]).tolist()) == {-255, -6}
    assert set(np.unique(fx["desc"]).tolist()) == {0, 1, 2}
    assert int(((fx["hret"] == -1) & (fx["desc"] == 0)).sum()) > 0  # the priority field cut short


def test_model_gives_h2os_answers_frame_by_frame(fx):
    for i in range(fx["ret"].size):
        check_probe(fx, i)


def test_model_walks_the_corpus_files_as_h2o_decodes_them(fx):
    """every file as one connection: the frames the walk lists are the file's frames in order, every listed HEADERS
    frame's fragment is h2o's, and where the walk stopped on a frame's own rules h2o refused that frame the same way"""
    stops = {}
    for f in range(fx["file_off"].size - 1):
        buf = bytes(fx["files"][int(fx["file_off"][f]):int(fx["file_off"][f + 1])])
        p0 = int(fx["file_probe0"][f])
        w = M.walk(buf, 1 << 20)
        pos, at = 0, []  # the file's frames by the length fields alone
        while pos < len(buf):
            at.append(pos)
            pos += 9 + int.from_bytes(buf[pos:pos + 3], "big") if len(buf) - pos >= 9 else 9
        assert len(at) == int(fx["file_probe0"][f + 1]) - p0
        assert [fr["payload_off"] - 9 for fr in w["frames"]] == at[:len(w["frames"])]
        for k, fr in enumerate(w["frames"]):
            i = p0 + k
            assert int(fx["ret"][i]) == 9 + fr["length"]
            if fr["type"] == M.HEADERS:
                assert int(fx["hret"][i]) == 0
                assert (fr["frag_off"] - fr["payload_off"], fr["frag_len"]) == (int(fx["frag_off"][i]), int(fx["frag_len"][i]))
        n = len(w["frames"])
        assert w["consumed"] == (at[n] if n < len(at) else len(buf))
        stops[(w["status"], w["err"])] = stops.get((w["status"], w["err"]), 0) + 1
        if w["err"] in (M.E_HEADERS_FRAME, M.E_HEADERS_PRIORITY):  # the first frame not consumed is the refused one
            assert int(fx["hret"][p0 + n]) == -1
            assert int(fx["desc"][p0 + n]) == {M.E_HEADERS_FRAME: 2, M.E_HEADERS_PRIORITY: 0}[w["err"]]
        if w["status"] == M.FRAME_SIZE:  # ... or a frame of the block that one opened: the first h2o does not take
            i = p0 + n
            while int(fx["ret"][i]) >= 0:
                i += 1
            assert int(fx["ret"][i]) == -6
    assert len(stops) >= 4, stops  # the files end in several ways


@pytest.mark.parametrize("c", K.CASES, ids=[c["name"] for c in K.CASES])
def test_model_gives_the_corpus_expectations(c):
    w = run_case(c)
    assert outcome(w) == expected(c)
    if c["frames"] is not None:
        assert [(f["type"], f["block"], f["frag_off"], f["frag_len"]) for f in w["frames"]] == c["frames"]
    for b in w["blocks"]:  # the records agree among themselves
        fs = w["frames"][b["first_frame"]:b["first_frame"] + b["nframes"]]
        assert b"".join(c["buf"][f["frag_off"]:f["frag_off"] + f["frag_len"]] for f in fs) == b["data"]


def test_corpus_covers_every_status_error_and_flag():
    names = [c["name"] for c in K.CASES]
    assert len(set(names)) == len(names)
    assert {c["status"] for c in K.CASES} == set(M.ALL_STATUS)
    assert {c["err"] for c in K.CASES} == set(M.ALL_ERR)
    seen = 0
    for c in K.CASES:
        for b in c["blocks"]:
            seen |= b[2]
    assert seen == sum(M.ALL_BLOCK_FLAGS)
    assert (M.ALL_STATUS, M.ACCEPT_PUSH) == ((0, C.ERR_PROTOCOL, C.ERR_FRAME_SIZE, C.H2F_REFUSED, C.H2F_FRAMES), C.H2F_ACCEPT_PUSH)


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_corpus_tells_each_defect(defect):
    assert any(outcome(run_case(c, (defect,))) != expected(c) for c in K.CASES), defect


def test_batch_model_places_empty_connections():
    bufs, caps = K.busy_and_empty()
    r = M.batch(bufs, caps)
    assert r["conn_first"].tolist() == [0, 0, 1, 1, 1, 2, 2] and r["totals"].tolist() == [2, 6]
    assert r["blk_off"].tolist() == [0, 3, 6] + [6] * 8 and r["nframes"].tolist() == [0, 1, 0, 0, 2, 0]
    assert r["frame_used"].tolist() == [True, False, False, False, False, True, True, False, False, False]
    assert r["blocks"]["first_frame"][:2].tolist() == [0, 6] and bytes(r["blk"]) == b"abcabc"


def test_call_checks_its_arguments_without_a_gpu():
    """HHUFF_EINVAL before any device call: a NULL array, in_size >= 2^32, max_frame_size outside 16384 .. 2^24 - 1, an
    unknown flag bit; nconn == 0 returns 0"""
    L = C.lib()
    p = 1 << 20  # a dummy address: never dereferenced on these paths
    names = ("data", "in_size", "in_off", "nconn", "frm_first", "frm_cap", "mfs", "mbb", "flags", "frames", "nframes", "consumed",
             "cstatus", "cerr", "blk", "blk_off", "conn_first", "blocks", "totals", "arena_off", "arena_fixed", "arena_per_byte",
             "stream")
    default = dict(data=p, in_size=64, in_off=p, nconn=2, frm_first=p, frm_cap=4, mfs=16384, mbb=0, flags=0, frames=p, nframes=p,
                   consumed=p, cstatus=p, cerr=p, blk=p, blk_off=p, conn_first=p, blocks=p, totals=p, arena_off=None,
                   arena_fixed=0, arena_per_byte=0, stream=None)
    call = lambda **k: L.hhuff_h2_deframe(*[k.get(a, default[a]) for a in names])  # noqa: E731
    for a in ("data", "in_off", "frm_first", "frames", "nframes", "consumed", "cstatus", "cerr", "blk", "blk_off", "conn_first",
              "blocks", "totals"):
        assert call(**{a: None}) == -1, a
        assert call(**{a: None, "nconn": 0}) == -1, a
    assert call(in_size=1 << 32) == -1 and call(in_size=(1 << 32) - 1, nconn=0) == 0
    for mfs in (0, 16383, 1 << 24, 0xFFFFFFFF):
        assert call(mfs=mfs) == -1, mfs
    for mfs in (16384, (1 << 24) - 1):
        assert call(mfs=mfs, nconn=0) == 0
    assert call(flags=2) == -1 and call(flags=3) == -1 and call(flags=1 << 31) == -1
    assert call(flags=C.H2F_ACCEPT_PUSH, nconn=0) == 0 and call(nconn=0) == 0


def test_header_compiles_and_constants_match(tmp_path):
    text = open(os.path.join(ROOT, "include", "hhuff.h")).read()
    defs = {k: int(v.rstrip("u")) for k, v in re.findall(r"#define\s+(HHUFF_H2[FB]_\w+)\s+\(?(-?\d+u?)\)?", text)}
    py = dict(HHUFF_H2F_ACCEPT_PUSH=C.H2F_ACCEPT_PUSH, HHUFF_H2F_REFUSED=C.H2F_REFUSED, HHUFF_H2F_FRAMES=C.H2F_FRAMES,
              HHUFF_H2F_ERR_NONE=C.H2F_ERR_NONE, HHUFF_H2F_ERR_HEADERS_STREAM_ID=C.H2F_ERR_HEADERS_STREAM_ID,
              HHUFF_H2F_ERR_HEADERS_FRAME=C.H2F_ERR_HEADERS_FRAME, HHUFF_H2F_ERR_HEADERS_PRIORITY=C.H2F_ERR_HEADERS_PRIORITY,
              HHUFF_H2F_ERR_EXPECTED_CONTINUATION=C.H2F_ERR_EXPECTED_CONTINUATION,
              HHUFF_H2F_ERR_INVALID_CONTINUATION=C.H2F_ERR_INVALID_CONTINUATION, HHUFF_H2F_ERR_PUSH_PROMISE=C.H2F_ERR_PUSH_PROMISE,
              HHUFF_H2F_ERR_PROMISE_STREAM_ID=C.H2F_ERR_PROMISE_STREAM_ID, HHUFF_H2F_ERR_PROMISE_FRAME=C.H2F_ERR_PROMISE_FRAME,
              HHUFF_H2B_END_STREAM=C.H2B_END_STREAM, HHUFF_H2B_PRIORITY=C.H2B_PRIORITY, HHUFF_H2B_EXCLUSIVE=C.H2B_EXCLUSIVE,
              HHUFF_H2B_CONTINUED=C.H2B_CONTINUED, HHUFF_H2B_PROMISE=C.H2B_PROMISE,
              HHUFF_H2B_SELF_DEPENDENCY=C.H2B_SELF_DEPENDENCY)
    assert defs == py
    assert (M.REFUSED, M.FRAMES, M.ACCEPT_PUSH) == (C.H2F_REFUSED, C.H2F_FRAMES, C.H2F_ACCEPT_PUSH)
    assert M.ALL_ERR == tuple(sorted(v for k, v in py.items() if k.startswith("HHUFF_H2F_ERR_")))
    assert M.ALL_BLOCK_FLAGS == tuple(sorted(v for k, v in py.items() if k.startswith("HHUFF_H2B_")))
    assert C.H2_FRAME_DTYPE.itemsize == 32 and C.H2_BLOCK_DTYPE.itemsize == 32
    assert "hhuff_h2_deframe" in C.EXPORTED and hasattr(C.lib(), "hhuff_h2_deframe")
    if not shutil.which("gcc"):
        pytest.skip("no host compiler")
    fields_f = ", ".join("(int)offsetof(hhuff_h2_frame_t, %s)" % n for n in C.H2_FRAME_DTYPE.names)
    fields_b = ", ".join("(int)offsetof(hhuff_h2_block_t, %s)" % n for n in C.H2_BLOCK_DTYPE.names)
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hhuff.h"\n'
                   "int main(void) {\n"
                   "    int f[] = {%s}, b[] = {%s};\n"
                   "    unsigned i;\n"
                   "    printf(\"%%d %%d\", (int)sizeof(hhuff_h2_frame_t), (int)sizeof(hhuff_h2_block_t));\n"
                   "    for (i = 0; i != sizeof(f) / sizeof(f[0]); ++i) printf(\" %%d\", f[i]);\n"
                   "    for (i = 0; i != sizeof(b) / sizeof(b[0]); ++i) printf(\" %%d\", b[i]);\n"
                   "    return 0;\n"
                   "}\n" % (fields_f, fields_b))
    exe = str(tmp_path / "t")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    want = [32, 32] + [C.H2_FRAME_DTYPE.fields[n][1] for n in C.H2_FRAME_DTYPE.names] + \
        [C.H2_BLOCK_DTYPE.fields[n][1] for n in C.H2_BLOCK_DTYPE.names]
    assert got == want


def test_frames_host_clean_under_sanitizers(tmp_path):
    """tools/frames_host.cpp over the corpus (its expectations included), every truncation of every corpus connection
    and 10,000 seeded single-byte mutations"""
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    probe_src = tmp_path / "probe.cpp"
    probe_src.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++", *san, str(probe_src), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes")
    cases = tmp_path / "cases.txt"
    with open(cases, "w") as f:
        for c in K.CASES:  # one line a case: the arguments, the expected outcome, the connection in hex
            nbytes = sum(len(b[7]) for b in c["blocks"])
            f.write("%d %d %d %d %d %d %d %d %d %d %s\n" % (c["cap"], c["mfs"], c["mbb"], c["flags"], c["status"], c["err"],
                                                             c["consumed"], c["nframes"], len(c["blocks"]), nbytes,
                                                             c["buf"].hex() or "-"))
    exe = str(tmp_path / "frames_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *san, "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "h2o_amd", "csrc"),
                    os.path.join(ROOT, "tools", "frames_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(cases), "10000"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.rstrip().endswith("ok: frames_host"), r.stdout
    assert "%d cases" % len(K.CASES) in r.stdout and "10000 mutations" in r.stdout
