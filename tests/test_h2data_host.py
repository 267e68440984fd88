"""HTTP/2 DATA frames on the send side (include/hhuff.h (2k'')) without a GPU: the frame-by-frame model
(h2data_model.py) against h2o's own frames (golden/h2data.npz, written by tools/gen_h2data_fixture.py from the real
reference), against the literal expectations of the hand-built corpus (h2data_corpora.py) and against its own closed
form; the corpus's coverage and its power to tell the model's defects apart; the call's argument checks; the
header's constants; and tools/h2data_host.cpp -- the arithmetic of h2o_amd/csrc/hhuff_h2data.h, the code the kernel
runs -- as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer: there the closed form meets a
loop over h2o's calls on the whole domain m in 1..5, R, W_c, W_s, L in -2..40."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import h2data_corpora as K
import h2data_model as M
from conftest import ROOT, load_golden
from h2o_amd import codec as C


def run_case(c, defects=()):
    r = M.connection(K.BODY, c["sends"], c["m"], c["window"], c["room"], 0, defects)
    return r["status"], r["sent"], len(r["buf"]), r["window"], r["buf"]


def expected_bytes(c):
    """the case's frames as bytes: record i has the next sent[i].nframes frames, their payloads are its bytes in order"""
    out, frames = b"", list(c["frames"])
    for s, t in zip(c["sends"], c["sent"]):
        at = s[0]
        for sid, n, fl in [frames.pop(0) for _ in range(t[1])]:
            out += n.to_bytes(3, "big") + bytes([0, fl]) + sid.to_bytes(4, "big") + K.BODY[at:at + n]
            at += n
        assert at == s[0] + t[0]
    assert not frames
    return out


def expected(c):
    return c["status"], c["sent"], c["out_len"], c["after"], expected_bytes(c)


def test_model_gives_h2os_frames_for_every_fixture_case():
    """golden/h2data.npz (tools/gen_h2data_fixture.py: the real static send_data behind
    h2o_http2_stream_send_pending_data, called repeatedly): every frame's header, both windows afterwards, from the
    frame-by-frame model and from the closed form"""
    fx = load_golden("h2data")
    n = fx["cases"].shape[0]
    assert n > 1000 and fx["frame_off"].size == n + 1 and int(fx["frame_off"][-1]) * 9 == fx["headers"].size
    assert {int(m) for m in fx["cases"][:, 0]} >= {16384, 16385, 32768, 16777215} and int(fx["nframes"].max()) >= 3
    empty_final = (fx["cases"][:, 4] == 0) & (fx["cases"][:, 5] == 1)
    assert set(fx["nframes"][empty_final].tolist()) == {0, 1}  # the empty END_STREAM frame and its absence
    for i in range(n):
        m, R, Wc, Ws, L, flags, maxf = (int(v) for v in fx["cases"][i])
        want = bytes(fx["headers"][9 * int(fx["frame_off"][i]):9 * int(fx["frame_off"][i + 1])])
        conn = M.new_conn(m, Wc, R)
        sent, k, why, ws = M.visit(conn, bytes(L), 1, Ws, flags, maxf)
        heads = b"".join(bytes(conn["buf"][p:p + 9]) for p in np.cumsum([0] + [9 + f[0] for f in conn["frames"]])[:-1])
        assert (k, heads, conn["window"], ws) == (int(fx["nframes"][i]), want, int(fx["after"][i][0]), int(fx["after"][i][1])), i
        lens, why2 = closed(m, R, Wc, Ws, L, flags, maxf)
        assert why2 == why and lens == [f[0] for f in conn["frames"]], i


@pytest.mark.parametrize("c", K.CASES, ids=[c["name"] for c in K.CASES])
def test_model_gives_the_corpus_expectations(c):
    assert run_case(c) == expected(c)
    # the expectations among themselves
    assert c["out_len"] == sum(9 + f[1] for f in c["frames"]) and sum(t[1] for t in c["sent"]) == len(c["frames"])
    assert c["after"] == c["window"] - sum(t[0] for t in c["sent"])
    at = 0
    for s, t in zip(c["sends"], c["sent"]):
        assert t[2] == at and t[4] == s[3] - t[0] and sum(1 for v in M.STOPS if t[3] & v) == 1
        at += t[0] + 9 * t[1]


def test_corpus_reaches_every_stop_on_both_sides_of_its_edge():
    names = [c["name"] for c in K.CASES]
    assert len(set(names)) == len(names)
    first = [(c, c["sends"][0], c["sent"][0]) for c in K.CASES if c["sent"]]
    m = K.M
    assert {c["room"] for c, s, t in first if c["room"] < 20} >= {8, 9, 10}
    assert {t[3] & ~1 for c, s, t in first if c["room"] in (8, 9)} == {M.ROOM}
    assert {M.ROOM not in (t[3],) for c, s, t in first if c["room"] == 10 and s[1] <= 1} == {True}
    assert {s[3] for c, s, t in first if t[3] == M.STREAM_WINDOW} >= {-1, 0, 1}
    assert {c["window"] for c, s, t in first if t[3] == M.CONN_WINDOW} >= {-1, 0, 1}
    assert {s[1] for c, s, t in first if c["m"] == m and t[3] & M.DONE} >= {0, 1, m - 1, m, m + 1, 2 * m}
    seen = 0
    for c in K.CASES:
        for t in c["sent"]:
            seen |= t[3]
    assert seen == M.END_STREAM | sum(M.STOPS)
    # the empty FINAL frame and its three ways of not appearing; TRAILERS
    empty = {c["name"]: c["sent"][0] for c in K.CASES if c["sends"] and c["sends"][0][1] == 0 and c["sends"][0][4] & M.FINAL}
    assert {t[3] for t in empty.values() if t[1] == 0} == {M.STREAM_WINDOW, M.ROOM, M.CONN_WINDOW, M.DONE}
    assert sum(t[1] for t in empty.values()) == 2  # (with all the room, and with room for its header and one byte more)
    assert any(s[4] & M.TRAILERS and t[0] for c, s, t in first)
    assert {c["m"] for c in K.CASES} >= {16383, 16384, 32768, 16777215, 16777216}
    assert {c["status"] for c in K.CASES} == {0, M.EINVAL}
    assert any(c["status"] and c["sent"] for c in K.CASES)  # earlier records stay
    assert any(len(c["sends"]) >= 3 and 0 in [t[1] for t in c["sent"][1:-1]] for c in K.CASES)  # no frame between frames
    assert any(f[1] >= 1 << 16 for c in K.CASES for f in c["frames"])


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_corpus_tells_each_defect(defect):
    assert any(run_case(c, (defect,)) != expected(c) for c in K.CASES), defect


def closed(m, R, Wc, Ws, L, flags, maxf):
    K_, tail, empty, why = M.closed_form(m, R, Wc, Ws, L, bool(flags & M.FINAL), bool(flags & M.TRAILERS), maxf)
    lens = [m] * K_ + ([tail] if tail or empty else [])
    return lens, why


def framed(m, R, Wc, Ws, L, flags, maxf):
    conn = M.new_conn(m, Wc, R)
    n, k, why, w = M.visit(conn, bytes(max(L, 0)), 1, Ws, flags, maxf)
    assert w == Ws - n and conn["window"] == Wc - n and conn["room"] == R - n - 9 * k and len(conn["frames"]) == k
    assert [f[1] for f in conn["frames"]] == [0] * (k - 1) + [why & 1] * (k > 0)
    return [f[0] for f in conn["frames"]], why


@pytest.mark.parametrize("m", (1, 2, 3, 4, 5))
def test_closed_form_equals_the_model_at_tiny_sizes(m):
    """The model's closed form against its frame-by-frame functions for R and L in -2..40, FINAL and TRAILERS in all
    combinations and max_frames 0..3 in rotation, with the two windows at every second pair of -2..40 that puts both
    at an edge (-2..2, 38..40), or one at the other or one off it.  A sample: all 43^4 x 5 points of the domain, with
    seven variants each, run in compiled code against the shared header (test_h2data_host_clean_under_sanitizers);
    here they would take minutes."""
    edge = (-2, -1, 0, 1, 2, 38, 39, 40)
    pairs = sorted({(a, b) for a in range(-2, 41) for b in range(-2, 41) if (a in edge and b in edge) or abs(a - b) <= 1})
    variants = ((0, 0), (M.FINAL, 0), (M.TRAILERS, 0), (M.FINAL | M.TRAILERS, 0), (M.FINAL, 1), (M.FINAL, 2), (0, 3))
    n = 0
    for R, L in itertools.product(range(-2, 41, 1), range(-2, 41)):
        for Wc, Ws in pairs[(R + L) % 2::2]:
            flags, maxf = variants[n % 7]
            assert closed(m, R, Wc, Ws, L, flags, maxf) == framed(m, R, Wc, Ws, L, flags, maxf), (m, R, Wc, Ws, L, flags, maxf)
            n += 1
    assert n > 150000


def test_batch_model_places_records_and_regions():
    by = {c["name"]: c for c in K.CASES}
    conns = [by["blocked_stream_between"]["sends"], [], by["m_plus_1"]["sends"]]
    e = M.batch(K.BODY, conns, [(16384, 100000)] * 3, rooms=[40, 0, 16403])
    assert e["send_first"].tolist() == [0, 5, 5, 6] and e["out_off"].tolist() == [0, 40, 40, 16443]
    assert e["out_len"].tolist() == [31, 0, 16403] and e["cstatus"].tolist() == [0, 0, 0]
    assert e["sent"]["out_off"].tolist() == [0, 10, 10, 21, 21, 40] and e["sent_used"].all()
    assert e["out_used"].sum() == 31 + 16403 and not e["out_used"][31:40].any() and (e["out"][31:40] == 0xA5).all()
    assert e["peers_out"]["send_window"].tolist() == [99996, 100000, 100000 - 16385]
    assert bytes(e["out"][40:49]) == bytes([0, 0x40, 0, 0, 0, 0, 0, 0, 1])
    # hostile ranges are clamped as (2k') clamps frm_first
    assert M.clamp_ranges([3, 1, 9, 4], 6) == [(3, 3), (1, 6), (6, 6)]


def test_call_checks_its_arguments_without_a_gpu():
    """HHUFF_EINVAL before any device call: a NULL array, body_size or out_size >= 2^32, non-zero flags; nconn == 0
    returns 0"""
    L = C.lib()
    p = 1 << 20  # a dummy address: never dereferenced on these paths
    names = ("body", "body_size", "sends", "send_first", "nsend", "nconn", "flags", "peers_in", "peers_out", "sent", "out", "out_size",
             "out_off", "out_len", "cstatus", "stream")
    default = dict(body=p, body_size=64, sends=p, send_first=p, nsend=4, nconn=2, flags=0, peers_in=p, peers_out=p, sent=p, out=p,
                   out_size=100, out_off=p, out_len=p, cstatus=p, stream=None)
    call = lambda **k: L.hhuff_h2_frame_data(*[k.get(a, default[a]) for a in names])  # noqa: E731
    for a in ("body", "sends", "send_first", "peers_in", "peers_out", "sent", "out", "out_off", "out_len", "cstatus"):
        assert call(**{a: None}) == -1, a
        assert call(**{a: None, "nconn": 0}) == -1, a
    assert call(body_size=1 << 32) == -1 and call(out_size=1 << 32) == -1 and call(body_size=1 << 40, nconn=0) == -1
    assert call(body_size=(1 << 32) - 1, out_size=(1 << 32) - 1, nconn=0) == 0
    assert call(flags=1) == -1 and call(flags=1 << 31) == -1 and call(flags=1, nconn=0) == -1
    assert call(nconn=0) == 0 and call(nconn=0, nsend=0) == 0


def test_header_compiles_and_constants_match(tmp_path):
    text = open(os.path.join(ROOT, "include", "hhuff.h")).read()
    defs = {k: int(v.rstrip("u")) for k, v in re.findall(r"#define\s+(HHUFF_H2[STD]_\w+)\s+\(?(-?\d+u?)\)?", text)}
    py = dict(HHUFF_H2S_FINAL=C.H2S_FINAL, HHUFF_H2S_TRAILERS=C.H2S_TRAILERS, HHUFF_H2T_END_STREAM=C.H2T_END_STREAM,
              HHUFF_H2T_DONE=C.H2T_DONE, HHUFF_H2T_STREAM_WINDOW=C.H2T_STREAM_WINDOW, HHUFF_H2T_ROOM=C.H2T_ROOM,
              HHUFF_H2T_CONN_WINDOW=C.H2T_CONN_WINDOW, HHUFF_H2T_MAX_FRAMES=C.H2T_MAX_FRAMES, HHUFF_H2D_EINVAL=C.H2D_EINVAL)
    assert defs == py
    assert (M.FINAL, M.TRAILERS, M.EINVAL) == (C.H2S_FINAL, C.H2S_TRAILERS, C.H2D_EINVAL) == (K.F, K.T, K.EINVAL)
    assert (M.END_STREAM, M.DONE, M.STREAM_WINDOW, M.ROOM, M.CONN_WINDOW, M.MAX_FRAMES) == (
        C.H2T_END_STREAM, C.H2T_DONE, C.H2T_STREAM_WINDOW, C.H2T_ROOM, C.H2T_CONN_WINDOW, C.H2T_MAX_FRAMES) == (
        K.ES, K.DONE, K.SW, K.ROOM, K.CW, K.MAXF)
    assert len({C.H2D_EINVAL, C.H2C_EINVAL, C.H2C_SPACE, C.H2F_FRAMES, C.H2F_REFUSED}) == 5
    assert C.H2_SEND_DTYPE.itemsize == 24 and C.H2_SENT_DTYPE.itemsize == 24
    assert "hhuff_h2_frame_data" in C.EXPORTED and hasattr(C.lib(), "hhuff_h2_frame_data")
    # the shared arithmetic takes its codes from the header
    rules = open(os.path.join(ROOT, "h2o_amd", "csrc", "hhuff_h2data.h")).read()
    assert set(re.findall(r"HHUFF_H2[STD]_[A-Z_]+", rules)) == set(py)
    if not shutil.which("gcc") or not shutil.which("g++"):
        pytest.skip("no host compiler")
    dts = (("hhuff_h2_send_t", C.H2_SEND_DTYPE), ("hhuff_h2_sent_t", C.H2_SENT_DTYPE))
    fields = ", ".join("(int)offsetof(%s, %s)" % (t, n) for t, dt in dts for n in dt.names)
    body = ('#include <stddef.h>\n#include <stdio.h>\n#include "hhuff.h"\n'
            "int main(void) {\n"
            "    int f[] = {%s};\n"
            "    unsigned i;\n"
            "    printf(\"%%d %%d\", (int)sizeof(hhuff_h2_send_t), (int)sizeof(hhuff_h2_sent_t));\n"
            "    for (i = 0; i != sizeof(f) / sizeof(f[0]); ++i) printf(\" %%d\", f[i]);\n"
            "    return 0;\n"
            "}\n" % fields)
    want = [24, 24] + [dt.fields[n][1] for _, dt in dts for n in dt.names]
    for cc, std, name in (("gcc", "-std=c99", "t.c"), ("g++", "-std=c++17", "t.cpp")):
        src = tmp_path / name
        src.write_text(body)
        exe = str(tmp_path / (name + ".exe"))
        subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                       check=True)
        assert [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()] == want


def case_line(c):
    sends = " ".join("%d %d %d %d %d %d" % s for s in c["sends"])
    sent = " ".join("%d %d %d %d %d" % t for t in c["sent"])
    frames = " ".join("%d %d %d" % f for f in c["frames"])
    return "%d %d %d %d %d %d %d %s %d %s %d %s\n" % (c["m"], c["window"], c["room"], c["status"], c["out_len"], c["after"],
                                                     len(c["sends"]), sends, len(c["sent"]), sent, len(c["frames"]), frames)


def test_h2data_host_clean_under_sanitizers(tmp_path):
    """tools/h2data_host.cpp: the shared header's closed form against a loop over h2o's calls on the whole small domain,
    the corpus with its expectations, and 20,000 seeded connections of hostile records"""
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
    exe = str(tmp_path / "h2data_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *san, "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "h2o_amd", "csrc"),
                    os.path.join(ROOT, "tools", "h2data_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(cases), "20000"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.rstrip().endswith("ok: h2data_host"), r.stdout
    assert "%d records: closed form = loop" % (5 * 43 ** 4 * 7) in r.stdout
    assert "%d cases" % len(K.CASES) in r.stdout and "20000 mutations" in r.stdout
    assert int(re.search(r"(\d+) refused as out of range", r.stdout).group(1)) > 100
