"""CASPER without a GPU: tools/casper_host.cpp -- the slab check, SHA-1, serial set operations, Golomb decoder and
encoder and base64url writer of h2o_amd/csrc/hhuff_casper.h -- built with AddressSanitizer and
UndefinedBehaviorSanitizer as a stand-alone program and run over the fixture's scripts with h2o's recorded answers, cut
and damaged cookies and slabs; and the argument refusals of hhuff_casper_step, which enqueue nothing."""
import ctypes
import os
import shutil
import subprocess

import pytest

import casper_model as M
from conftest import ROOT, load_golden


def test_casper_host_clean_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes")
    g = load_golden("casper")
    text, lines, starts = g["strings"].tobytes(), [], set(g["case_first"].tolist())
    for o, (kind, a, b) in enumerate(g["op"].tolist()):
        if o in starts:
            lines.append("N")
        arg = "%d %d" % (a, b) if kind == M.INIT else "" if kind == M.COOKIE else "x" + text[g["str_off"][a]:g["str_off"][a + 1]].hex()
        lines.append("%d %s %d %d x%s" % (kind, arg, g["ret"][o], g["entries"][o],
                                          g["cookies"][g["cookie_off"][o]:g["cookie_off"][o + 1]].tobytes().hex()))
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "casper_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *san, "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "h2o_amd", "csrc"),
                    os.path.join(ROOT, "tools", "casper_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(cases), "24"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.rstrip().startswith("ok: casper_host, %d cases, %d ops" % (g["case_first"].size - 1, len(g["op"]))), r.stdout


def test_argument_refusals():
    """HHUFF_EINVAL for a NULL required array, a misaligned scratch or max_keys out of range, HHUFF_OK for an empty
    batch: before any device call"""
    from h2o_amd import build, codec as C

    build.build(verbose=False)
    L = C.lib()
    err = L.hhuff_last_error_string()
    buf = (ctypes.c_uint8 * 256)()
    a = (ctypes.addressof(buf) + 15) & ~15
    ok = [a, 1, 8, None, a, a, 1, a, 64, None, None, None, 0, 0, a, a, a, None]
    for k in (0, 4, 5, 7, 14, 15, 16):
        assert L.hhuff_casper_step(*[None if i == k else x for i, x in enumerate(ok)]) == -1, k
    for k, bad in ((0, a + 8), (2, 0), (2, C.CSP_MAX_KEYS + 1)):
        assert L.hhuff_casper_step(*[bad if i == k else x for i, x in enumerate(ok)]) == -1, k
    assert L.hhuff_casper_step(*[0 if i == 6 else None if x == a else x for i, x in enumerate(ok)]) == 0  # an empty batch
    assert L.hhuff_last_error_string() == err
    assert C.casper_scratch_bytes(3, 5) == 3 * 64 and "hhuff_casper_step" in C.EXPORTED
