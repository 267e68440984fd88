"""The HTTP/2 stream table (include/hhuff.h (2k''')) without a GPU: the model (h2streams_model.py) against h2o's own
answers (golden/h2streams.npz, written by tools/gen_h2streams_fixture.py from the real reference) and against the literal
expectations of the hand-built corpus (h2streams_corpora.py); the corpus's coverage and its power to tell the model's
defects apart; the calls' argument checks; the header's constants; and tools/h2streams_host.cpp -- the rules of
h2o_amd/csrc/hhuff_h2streams.h, the code the kernel runs -- as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer, over the corpus with its expectations, the table against a map, and seeded hostile records."""
import os
import re
import shutil
import subprocess

import pytest

import h2streams_corpora as K
import h2streams_model as M
from conftest import ROOT, load_golden
from h2o_amd import codec as C


@pytest.mark.parametrize("c", K.CASES, ids=[c["name"] for c in K.CASES])
def test_model_gives_the_corpus_expectations(c):
    assert K.run_model(c) == K.expected(c)


def h2o_view(c):
    """what tools/gen_h2streams_fixture.py records of a case, from the model: per frame fed (ret, desc), the last step's
    bytes, the counters, and per stream (id, state, body state, windows, bytes_unnotified, received, content-length)"""
    conn, frames, w = M.new_conn(), [], None
    for st, iws in zip(c["steps"], c["iws"]):
        if st.sends:
            M.fill_sends(conn, [s for s, _ in st.sends])
            M.commit_sent(conn, [s for s, _ in st.sends], [n for _, n in st.sends])
        w = M.walk(conn, c["P"], iws, st.frames, st.blocks, st.ops, st.rep_cap, st.nctl)
        for e in w["events"]:
            frames.append((e[2], 99 if e[3] == M.E_HEADER_BLOCK else e[3]) if e[3] != M.E_NONE else (0, 0))
    counters, streams = M.snapshot(conn)
    rows = [(sid, s[0], s[1], s[3], s[4], s[5], s[6], -1 if s[7] == M.NO_LENGTH else s[7]) for sid, s in streams]
    return frames, w["replies"], counters, rows


def test_model_gives_h2os_answers_case_by_case():
    """golden/h2streams.npz (tools/gen_h2streams_fixture.py: the real static handlers of lib/http2/connection.c, frame by
    frame): return values, err_desc, the bytes queued on conn->_write.buf and every live stream's states and windows"""
    fx = load_golden("h2streams")
    by = {c["name"]: c for c in K.CASES}
    names = [str(n) for n in fx["names"]]
    assert len(names) >= 75 and set(names) | {str(n) for n in fx["skipped"]} == set(by) and len(set(names)) == len(names)
    state = {0: M.IDLE, 1: M.RECV_HEADERS, 2: M.RECV_BODY}  # h2o's states from REQ_PENDING on: the request is handed over
    body = {0: M.BODY_NONE, 1: M.BODY_BEFORE_FIRST, 2: M.BODY_OPEN, 3: M.BODY_CLOSE_DELIVERED, 4: M.BODY_CLOSE_DELIVERED}
    seen = set()
    for i, name in enumerate(names):
        frames, replies, counters, rows = h2o_view(by[name])
        f0, f1 = int(fx["frame_first"][i]), int(fx["frame_first"][i + 1])
        got = list(zip(fx["ret"][f0:f1].tolist(), fx["desc"][f0:f1].tolist()))
        assert got == frames, name
        seen |= {d for _, d in got}
        assert bytes(fx["out"][int(fx["out_off"][i]):int(fx["out_off"][i + 1])]) == replies, name
        assert tuple(fx["counters"][i].tolist()) == counters, name
        h = fx["streams"][int(fx["stream_first"][i]):int(fx["stream_first"][i + 1])].tolist()
        assert [(r[0], state.get(r[1], M.HANDED), body[r[2]]) + tuple(r[3:]) for r in h] == rows, name
    assert seen == set(range(11)) | {99}  # every text of the handlers, and the parser's


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_corpus_tells_each_defect(defect):
    assert any(K.run_model(c, (defect,)) != K.expected(c) for c in K.CASES), defect


def test_corpus_covers_every_status_error_flag_and_reply():
    names = [c["name"] for c in K.CASES]
    assert len(set(names)) == len(names)
    assert {c["status"] for c in K.CASES} == {0, -1, -5, -9, -11, -254, M.SPACE, M.EFULL}
    assert {c["err"] for c in K.CASES} == set(M.ALL_ERR)
    flags = 0
    for c in K.CASES:
        for e in c["events"] + c["op_events"]:
            flags |= e[0]
    assert flags == sum(M.ALL_EVENT_FLAGS)
    assert {e[1] for c in K.CASES for e in c["events"] if e[0] & M.RESET_SENT} == {-1, -3, -5, -7}
    assert {e[1] for c in K.CASES for e in c["op_events"]} == {0, M.EINVAL, M.ENOENT, M.EFULL}
    assert {len(c["steps"]) for c in K.CASES} == {1, 2}
    assert any(c["steps"][-1].sends for c in K.CASES) and any(c["steps"][-1].nctl is not None for c in K.CASES)
    assert any(v[2] < 0 for c in K.CASES for v in c["streams"].values()) or any(v[3] < 0 for c in K.CASES for v in c["streams"].values())
    # a frame that owes the most: the control call's reply and two frames of its own
    assert any(len(c["replies"]) == 26 for c in K.CASES)


def test_batch_layout_of_the_model():
    by = {c["name"]: c for c in K.CASES}
    conns = [dict(frames=by[n]["steps"][0].frames, blocks=by[n]["steps"][0].blocks, ops=by[n]["steps"][0].ops)
             for n in ("post", "no_frames", "connect_udp_other_path")]
    a = M.build(conns, slack=1)
    assert a["frm_first"].tolist() == [0, 4, 5, 7] and a["conn_first"].tolist() == [0, 1, 1, 2] and a["frm_cap"] == 7
    assert a["frames"]["block"].tolist() == [0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 1, 0xFFFFFFFF]
    assert a["blocks"]["first_frame"][:2].tolist() == [0, 5] and a["req"]["method"][:2].tolist() == [0, 0]
    assert bytes(a["arena"][:a["arena_size"]]) == b"GET/CONNECT-UDP/x" and a["blk_off"].tolist() == [0, 2, 4, 4, 4, 4, 4, 4]
    assert a["rep_off"].tolist() == [0, 4 * 43, 5 * 43, 7 * 43]


def test_fill_and_commit_model():
    conn = M.new_conn()
    M.walk(conn, M.params(), 100, K.S().headers(1).headers(3).frames, K.S().headers(1).headers(3).blocks)
    assert M.fill_sends(conn, [1, 5, 1, 3]) == [(100, 0), (0, 1), (0, 2), (100, 0)]
    M.commit_sent(conn, [1, 5, 1, 3], [60, 7, 9, 100])
    assert [conn["streams"][s]["output_window"] for s in (1, 3)] == [40, 0]
    M.commit_sent(conn, [1], [5])  # nothing listed any more
    assert conn["streams"][1]["output_window"] == 40


def test_calls_check_their_arguments_without_a_gpu():
    """HHUFF_EINVAL before any device call: a NULL array, a size >= 2^32, an unknown flag bit, max_entries == 0, a scratch
    too small; nconn == 0 returns 0"""
    L = C.lib()
    p = 1 << 20  # a dummy address: never dereferenced on these paths
    names = ("slots", "params", "data", "in_size", "frames", "nframes", "frm_first", "frm_cap", "ctl", "nctl", "ctl_rep", "ctl_rep_size",
             "ctl_rep_off", "blocks", "conn_first", "bstatus", "req", "arena", "arena_size", "blk_off", "value_off", "value_len", "peers",
             "ops", "op_first", "nops", "nconn", "sev", "op_sev", "nstr", "sstatus", "serr", "rep", "rep_size", "rep_off", "rep_len",
             "scratch", "scratch_size", "flags", "stream")
    good = C.h2_streams_params(M.params(max_streams=4, max_streams_for_priority=2, max_entries=8))
    size = C.h2_streams_scratch_size(2, 8)
    assert size == 2 * (32 + 16 * 48) and C.h2_streams_scratch_size(1, 1) == 32 + 4 * 48 and C.h2_streams_scratch_size(1, 0) == 0
    default = dict(slots=None, params=good, data=p, in_size=64, frames=p, nframes=p, frm_first=p, frm_cap=4, ctl=p, nctl=p, ctl_rep=p,
                   ctl_rep_size=8, ctl_rep_off=p, blocks=p, conn_first=p, bstatus=p, req=p, arena=p, arena_size=8, blk_off=p,
                   value_off=p, value_len=p, peers=p, ops=None, op_first=None, nops=0, nconn=0, sev=p, op_sev=None, nstr=p, sstatus=p,
                   serr=p, rep=p, rep_size=172, rep_off=p, rep_len=p, scratch=p, scratch_size=size, flags=0, stream=None)

    def call(**k):
        return L.hhuff_h2_streams(*[k.get(a, default[a]) for a in names])

    assert call() == 0 and call(flags=C.H2ST_CONTINUE) == 0
    for a in ("params", "data", "frames", "nframes", "frm_first", "ctl", "nctl", "ctl_rep", "ctl_rep_off", "blocks", "conn_first", "bstatus",
              "req", "arena", "blk_off", "value_off", "value_len", "peers", "sev", "nstr", "sstatus", "serr", "rep", "rep_off", "rep_len",
              "scratch"):
        assert call(**{a: None}) == -1, a
    assert call(nops=1) == -1 and call(nops=1, ops=p, op_first=p) == -1 and call(nops=1, ops=p, op_first=p, op_sev=p) == 0
    for a in ("in_size", "arena_size", "ctl_rep_size", "rep_size"):
        assert call(**{a: 1 << 32}) == -1 and call(**{a: (1 << 32) - 1}) == 0, a
    assert call(flags=2) == -1 and call(flags=1 << 31) == -1
    assert call(scratch=p + 8) == -1
    assert call(nconn=3) == -1 and call(nconn=2, scratch_size=size - 1) == -1  # (refused before any launch)
    for bad in (dict(max_entries=0), dict(max_entries=(1 << 24) + 1), dict(active_stream_window_size=65534),
                dict(active_stream_window_size=1 << 31), dict(flags=2)):
        assert call(params=C.h2_streams_params(dict(M.params(max_entries=8), **bad))) == -1, bad
    fs, cs = L.hhuff_h2_streams_fill_sends, L.hhuff_h2_streams_commit_sent
    assert fs(None, 8, p, size, p, p, 4, 0, p, None) == 0 and cs(None, 8, p, size, p, p, p, 4, 0, None) == 0
    assert fs(None, 8, p, size, None, p, 4, 0, p, None) == -1 and fs(None, 8, p, size, p, None, 4, 0, p, None) == -1
    assert fs(None, 8, p, size, p, p, 4, 0, None, None) == -1 and fs(None, 0, p, size, p, p, 4, 0, p, None) == -1
    assert fs(None, 8, None, size, p, p, 4, 0, p, None) == -1 and fs(None, 8, p, size, p, p, 4, 3, p, None) == -1
    assert cs(None, 8, p, size, None, p, p, 4, 0, None) == -1 and cs(None, 8, p, size, p, None, p, 4, 0, None) == -1
    assert cs(None, 8, p, size, p, p, None, 4, 0, None) == -1 and cs(None, 0, p, size, p, p, p, 4, 0, None) == -1


def test_header_compiles_and_constants_match(tmp_path):
    text = open(os.path.join(ROOT, "include", "hhuff.h")).read()
    defs = {k: int(v.rstrip("u")) for k, v in re.findall(r"#define\s+(HHUFF_H2(?:ST|SP|SE|O)_\w+)\s+\(?(-?\d+u?)\)?", text)}
    py = dict(HHUFF_H2ST_CONTINUE=C.H2ST_CONTINUE, HHUFF_H2SP_STREAM_BODIES=C.H2SP_STREAM_BODIES, HHUFF_H2O_CLOSE=C.H2O_CLOSE,
              HHUFF_H2O_CREDIT=C.H2O_CREDIT, HHUFF_H2O_OPEN_PUSH=C.H2O_OPEN_PUSH, HHUFF_H2ST_SPACE=C.H2ST_SPACE,
              HHUFF_H2ST_EINVAL=C.H2ST_EINVAL, HHUFF_H2ST_EFULL=C.H2ST_EFULL, HHUFF_H2ST_ENOENT=C.H2ST_ENOENT,
              HHUFF_H2ST_ESLOT=C.H2ST_ESLOT)
    events = ("OPENED", "BODY", "REQUEST_COMPLETE", "TRAILERS", "RESET_BY_PEER", "RESET_SENT", "WINDOW_UPDATE_SENT", "IGNORED",
              "PRIORITY_ONLY_OPENED", "SEND_WINDOW_OPENED", "BAD_CONNECT", "INVALID_HEADER_CHAR", "PRIORITY")
    for i, name in enumerate(events):
        py["HHUFF_H2SE_" + name] = 1 << i
        assert getattr(C, "H2SE_" + name) == 1 << i == M.ALL_EVENT_FLAGS[i]
    errs = ("NONE", "HEADERS_STREAM_ID", "HEADERS_CLOSED", "TUNNEL_TRAILERS", "TRAILERS_END_STREAM", "SELF_DEPENDENCY",
            "CONTINUATION_STREAM_ID", "DATA_FRAME", "TOO_MANY_IDLE", "RST_STREAM_STREAM_ID", "WINDOW_UPDATE_STREAM_ID",
            "TRAILERS_PSEUDO_HEADER", "TRAILERS_HOST", "HEADER_BLOCK")
    for i, name in enumerate(errs):
        py["HHUFF_H2ST_ERR_" + name] = i
        assert getattr(M, "E_" + name) == i == getattr(C, "H2ST_ERR_" + name)
    assert defs == py
    assert (M.SPACE, M.EINVAL, M.EFULL, M.ENOENT, M.ESLOT) == (C.H2ST_SPACE, C.H2ST_EINVAL, C.H2ST_EFULL, C.H2ST_ENOENT, C.H2ST_ESLOT)
    assert (M.OP_CLOSE, M.OP_CREDIT, M.OP_OPEN_PUSH, M.CONTINUE, M.STREAM_BODIES) == (C.H2O_CLOSE, C.H2O_CREDIT, C.H2O_OPEN_PUSH,
                                                                                  C.H2ST_CONTINUE, C.H2SP_STREAM_BODIES)
    # the comment beside each HHUFF_H2ST_ERR_* quotes h2o's text, and each text is in the reference's words
    quoted = dict((int(v), t) for _, v, t in re.findall(r'#define\s+HHUFF_H2ST_ERR_(\w+)\s+(\d+)u\s+/\* "([^"]+)" \*/', text))
    assert quoted == {k: v for k, v in M.ERR_TEXT.items() if v is not None}
    rules = open(os.path.join(ROOT, "h2o_amd", "csrc", "hhuff_h2streams.h")).read()
    assert set(re.findall(r"HHUFF_H2ST_ERR_\w+", rules)) == {k for k in py if k.startswith("HHUFF_H2ST_ERR_")}
    assert set(re.findall(r"HHUFF_H2SE_\w+", rules)) == {k for k in py if k.startswith("HHUFF_H2SE_")}
    assert re.search(r"kProtocol = -1, kFlowControl = -3, kStreamClosed = -5, kRefusedStream = -7, kEnhanceYourCalm = -11;", rules)
    assert C.H2_SEV_DTYPE.itemsize == 16 and C.H2_STREAM_OP_DTYPE.itemsize == 16 and C.H2_SEV_DTYPE == M.SEV_DTYPE
    assert M.FRAME_DTYPE == C.H2_FRAME_DTYPE and M.BLOCK_DTYPE == C.H2_BLOCK_DTYPE and M.CTL_DTYPE == C.H2_CTL_DTYPE
    assert M.REQ_DTYPE.itemsize == 48
    for name in ("hhuff_h2_streams", "hhuff_h2_streams_scratch_size", "hhuff_h2_streams_fill_sends", "hhuff_h2_streams_commit_sent"):
        assert name in C.EXPORTED and hasattr(C.lib(), name)
    assert C.h2_streams_entries(100, 16, 4) == 121 and C.h2_streams_entries(0xFFFFFFFF, 1, 0) == 0xFFFFFFFF
    assert C.h2_streams_reply_bound(3, 2) == 3 * 43 + 26
    if not shutil.which("gcc"):
        pytest.skip("no host compiler")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hhuff.h"\n'
                   "int main(void) {\n"
                   '    printf("%d %d %d %d %d %d %u %u %d", (int)sizeof(hhuff_h2_streams_params_t), (int)sizeof(hhuff_h2_stream_op_t),\n'
                   "           (int)sizeof(hhuff_h2_sev_t), (int)offsetof(hhuff_h2_streams_params_t, max_request_entity_size),\n"
                   "           (int)offsetof(hhuff_h2_streams_params_t, flags), (int)offsetof(hhuff_h2_sev_t, flags),\n"
                   "           hhuff_h2_streams_entries(100, 16, 4), hhuff_h2_streams_entries(0xFFFFFFFFu, 1, 0),\n"
                   "           (int)hhuff_h2_streams_reply_bound(3, 2));\n"
                   "    return 0;\n"
                   "}\n")
    exe = str(tmp_path / "t")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [32, 16, 16, 16, 24, 12, 121, 0xFFFFFFFF, 3 * 43 + 26]


def hexs(b, none=False):
    return "~" if none else (b.hex() or "-")


def case_lines(c):
    P = c["P"]
    out = ["C %d %d %d %d %d %d %d" % (len(c["steps"]), P["max_streams"], P["max_streams_for_priority"], P["active_stream_window_size"],
                                       P["max_entries"], P["max_request_entity_size"], P["flags"])]
    for st, iws in zip(c["steps"], c["iws"]):
        out.append("S %d %d %d %d %d %d %d" % (iws, -1 if st.rep_cap is None else st.rep_cap, -1 if st.nctl is None else st.nctl,
                                               len(st.frames), len(st.blocks), len(st.ops), len(st.sends)))
        for f in st.frames:
            out.append("F %d %d %d %d %d %d %d %d %s" % (f["type"], f["flags"], f["stream_id"], f["length"], f["ctl"][0], f["ctl"][1],
                                                         f["ctl"][2], -1 if f["block"] is None else f["block"], hexs(f["ctl_reply"])))
        for b in st.blocks:
            out.append("B %d %d %d %d %d %d %d %s %s %d" % (
                b["stream_id"], b["flags"], b["first_frame"], b["nframes"], b["bstatus"], b["exists_map"], b["content_length"],
                hexs(b["method"] or b"", b["method"] is None), hexs(b["path"] or b"", b["path"] is None), b["host"]))
        out += ["O %d %d %d" % op for op in st.ops] + ["T %d %d" % t for t in st.sends]
    ev = lambda evs: "%d %s" % (len(evs), " ".join("%d %d %d" % e for e in evs))  # noqa: E731
    out.append("E %d %d %d %s %s %s %d %d %d %d %d %s" % (
        c["status"], c["err"], c["nstr"], ev(c["events"]), ev(c["op_events"]), hexs(c["replies"]), *c["counters"], len(c["streams"]),
        " ".join("%d %d %d %d %d %d" % ((sid,) + v) for sid, v in sorted(c["streams"].items()))))
    return "\n".join(out) + "\n"


def test_h2streams_host_clean_under_sanitizers(tmp_path):
    """tools/h2streams_host.cpp over the corpus (its expectations included), the table against a map and 20,000 seeded
    hostile changes of the records the call takes from the calls in front"""
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
            f.write(case_lines(c))
    exe = str(tmp_path / "h2streams_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *san, "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "h2o_amd", "csrc"),
                    os.path.join(ROOT, "tools", "h2streams_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(cases), "20000"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.rstrip().endswith("ok: h2streams_host"), r.stdout
    assert "%d cases" % len(K.CASES) in r.stdout and "20000 mutations" in r.stdout
    assert int(re.search(r"(\d+) refused as out of range", r.stdout).group(1)) > 100
