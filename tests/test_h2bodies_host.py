"""The request-body plan without a GPU: tools/h2bodies_host.cpp -- h2o_amd/csrc/hhuff_h2bodies.h's walk, job list and
line code, the code the kernels run -- as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer,
over the hand-built cases of test_h2bodies.py and over seeded mutations of their records, every array a heap block of
exactly its size.  The plan -- per slot its run and offset, the run records, the statuses -- and the bytes must be the
Python reference's."""
import os
import random
import shutil
import subprocess

import pytest

import test_h2bodies as T
from conftest import ROOT
from h2o_amd import codec as C


def mutated(L, rng):
    """L with one in eight of its slots hostile: a stream id, a flag word, a length or an offset at an edge"""
    edge = (0, 1, 3, 15, 16, 4095, 4096, L["in_size"] - 1, L["in_size"], L["in_size"] + 1, 0x7fffffff, 0xffffffff)
    sev = [list(s) for s in L["sev"]]
    for s in sev:
        if rng.randrange(8) == 0:
            k = rng.randrange(4)
            s[k] = rng.choice((0, 1, 3, 5)) if k == 0 else rng.randrange(64) if k == 1 else rng.choice(edge)
    rooms = [rng.choice((0, 1, r, max(r - 1, 0), r + 16)) for r in (T.ranges(L, c)[3] for c in range(len(L["nstr"])))]
    off = [0]
    for r in rooms:
        off.append(off[-1] + r)
    return dict(L, sev=[tuple(s) for s in sev], out_off=off, out_size=off[-1], frm_first=sorted(L["frm_first"]))


def test_plan_and_bytes_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes")
    rng = random.Random(7)
    small = [L for L in T.CASES if L["frm_cap"] <= 300 and L["in_size"] <= 1 << 16]
    layouts = T.CASES + [mutated(L, rng) for L in small for _ in range(40)]
    want, lines = [], []
    for L in layouts:
        ref = T.reference(L)
        for c in range(len(L["nstr"])):
            f0, n, o0, room = T.ranges(L, c)
            slots = L["sev"][f0:f0 + n]
            lines.append("%d %d %d %d %s\n" % (L["in_size"], o0, room, n, " ".join("%d %d %d %d" % (s[0], s[1], s[2], s[3]) for s in slots)))
            nrun, out_len, status = ref["res"][c]
            if status:
                want.append("%d 0 0 0 |" % status)
                continue
            plan = " ".join("%d %d" % ref["plan"].get(f0 + i, (-1, 0)) for i in range(n))
            recs = [ref["runs"][f0 + k] for k in range(nrun)]
            runs = " ".join("%d %d %d %d %d %d" % (r[0], r[1], r[2], r[3], r[4] - f0, r[5]) for r in recs)
            njobs = sum(1 for s in slots if s[1] & T.BODY and s[2])
            want.append("%d %d %d %d | %s | %s | %s" % (0, nrun, out_len, njobs, plan, runs, ref["out"][o0:o0 + out_len].hex()))
    cases = tmp_path / "cases.txt"
    cases.write_text("".join(lines))
    exe = str(tmp_path / "h2bodies_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *san, "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "h2o_amd", "csrc"),
                    os.path.join(ROOT, "tools", "h2bodies_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "ok: h2bodies_host, %d connections" % len(lines) in r.stderr, r.stderr[-4000:]
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert " ".join(g.split()) == " ".join(w.split()), (i, lines[i][:200])
    statuses = [w.split()[0] for w in want]
    assert statuses.count(str(C.H2BD_EINVAL)) > 50 and statuses.count(str(C.H2BD_SPACE)) > 50 and statuses.count("0") > 500
