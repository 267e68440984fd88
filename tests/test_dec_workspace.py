"""The header-block decoders' workspaces (h2o_amd/csrc/hhuff_decwork.h), carved on the host under sanitizers by
tools/decwork_host.cpp: every piece filled to the bytes its kernel uses and read back at bitmap-word and chunk
edges, and the pieces' room and the total against the table of sizes written out here (S = in_size, each piece
rounded up to 256 bytes: the layout the launchers had when every offset was written by hand)."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SIZES = [0, 1, 2, 31, 32, 33, 32767, 32768, 32769, (1 << 20) + 1]
BIG = [(1 << 32) - 3, (1 << 32) - 1, 1 << 32]


def up256(x):
    return (x + 255) // 256 * 256


def table(kind, S, nconn, ws_bytes):
    """piece -> bytes its kernels use"""
    if kind.startswith("hpack"):
        nwords, n_max = (S + 31) // 32, 2 * S // 3 + 2
        prepass = 0 < S < 1 << 32
    else:
        nwords, n_max = S // 32 + 1, S + 2
        prepass = True
    nchunks = (nwords + 1023) // 1024
    t = {}
    if prepass:
        t.update(lit_bits=4 * nwords, name_bits=4 * nwords, lnames=4 * ((n_max + 31) // 32), word_pre=4 * nwords,
                 chunk=4 * nchunks + 4, list=4 * n_max, len=4 * n_max, pay=4 * n_max, cons=4 * n_max, st=n_max,
                 ws=ws_bytes, out=8 * S // 5 + 64)
        if kind.startswith("qpack"):
            t.update(p3_bits=4 * nwords, pfx=n_max)
    t.update(fsrc_n=8 * S + 8, fsrc_v=8 * S + 8)
    if nconn:
        t["map"] = 4 * nconn
    return t


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("decwork") / "decwork_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "h2o_amd", "csrc"),
                    os.path.join(ROOT, "tools", "decwork_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok", r.stdout[-2000:]
    return [json.loads(x) for x in lines[:-1]]


def test_every_case_ran_clean(cases):
    """the program's own checks (fill and read back, alignment, one zeroed prefix) passed for the whole sweep"""
    seen = {(c["kind"], c["in_size"], c["nconn"]) for c in cases}
    want = {(k, S, n) for S in SIZES for k, n in (("hpack", 0), ("qpack", 0), ("qpack_sessions", 1), ("qpack_sessions", 3))}
    want |= {(k, S, 0) for S in BIG for k in ("hpack_size", "qpack_size")}
    assert seen == want and len(cases) == len(want)


def test_no_piece_is_smaller_than_its_kernels_need(cases):
    for c in cases:
        if "pieces" not in c:
            continue
        t = table(c["kind"], c["in_size"], c["nconn"], c["ws_bytes"])
        assert set(c["pieces"]) == set(t), (c["kind"], c["in_size"])
        for name, (off, room) in c["pieces"].items():
            assert room >= t[name], (c["kind"], c["in_size"], name, room, t[name])
            assert off % 256 == 0


def test_total_is_no_more_than_the_hand_written_layout(cases):
    for c in cases:
        t = table(c["kind"], c["in_size"], c["nconn"], c["ws_bytes"])
        assert c["total"] <= sum(up256(b) for b in t.values()), (c["kind"], c["in_size"])
        if "pieces" in c:
            assert c["total"] == max(off + room for off, room in c["pieces"].values())


def test_hpack_without_a_prepass_holds_the_field_sources_only(cases):
    got = {c["in_size"]: c["total"] for c in cases if c["kind"].startswith("hpack")}
    for S in (0, 1 << 32):
        assert got[S] == 2 * up256(8 * S + 8)
