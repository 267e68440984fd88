"""The HTTP/2 scheduler without a GPU: tools/h2sched_host.cpp -- the serial form of h2o_amd/csrc/hhuff_h2sched.h, the
very rules the kernel runs -- built with AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program and run
over the fixture's cases with h2o's recorded visits and trees and over hostile op lists; and the argument refusals of
hhuff_h2_schedule, which enqueue nothing."""
import ctypes
import os
import shutil
import subprocess

import pytest

from conftest import ROOT, load_golden


def test_h2sched_host_clean_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes")
    g = load_golden("h2sched")
    lines, starts = [], set(g["case_first"].tolist())
    row = lambda c, r: c + " " + " ".join(str(int(x)) for x in r)  # noqa: E731
    for s in range(len(g["conn"])):
        if s in starts:
            lines.append("N 301")
        for key, first, c in (("ops", "op_first", "o"), ("cands", "cand_first", "c"), ("visits", "visit_first", "v"), ("tree", "tree_first", "t")):
            lines += [row(c, r) for r in g[key][g[first][s]:g[first][s + 1]]]
        lines.append(row("x", list(g["conn"][s]) + [g["active"][s]]))
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "h2sched_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *san, "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "h2o_amd", "csrc"),
                    os.path.join(ROOT, "tools", "h2sched_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(cases), "24"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.rstrip().startswith("ok: h2sched_host, %d cases, %d steps" % (g["case_first"].size - 1, len(g["conn"]))), r.stdout


def test_argument_refusals():
    """HHUFF_EINVAL for a NULL required array, out_size of 2^32, an unknown flag, max_nodes out of range, a small or
    misaligned scratch; HHUFF_OK for an empty batch: before any device call"""
    from h2o_amd import build, codec as C

    build.build(verbose=False)
    L = C.lib()
    err = L.hhuff_last_error_string()
    buf = (ctypes.c_uint8 * 4096)()
    a = (ctypes.addressof(buf) + 15) & ~15
    size = C.h2_sched_scratch_size(1, 8)
    ok = [None, 8, a, a, 1, a, a, 1, 1, a, 64, a, a, a, a, a, a, a, a, a, size, 0, None]
    for k in (2, 3, 5, 6, 9, 11, 12, 13, 14, 15, 16, 17, 18, 19):
        assert L.hhuff_h2_schedule(*[None if i == k else x for i, x in enumerate(ok)]) == -1, k
    for k, bad in ((1, 0), (1, 2049), (10, 1 << 32), (19, a + 8), (20, size - 1), (21, 2)):
        assert L.hhuff_h2_schedule(*[bad if i == k else x for i, x in enumerate(ok)]) == -1, k
    assert L.hhuff_h2_schedule(*[0 if i == 8 else x for i, x in enumerate(ok)]) == 0  # an empty batch
    assert L.hhuff_last_error_string() == err
    assert size == 32 + 24 * 8 and C.h2_sched_scratch_size(2, 2049) == 0 and "hhuff_h2_schedule" in C.EXPORTED
