"""Cache digests without a GPU: tools/cdigest_host.cpp -- the walk, serial decoder, image writer, SHA-256 and frame walk
of h2o_amd/csrc/hhuff_cdigest.h, the code the kernels run -- built with AddressSanitizer and UndefinedBehaviorSanitizer
as a stand-alone program and run over the fixture's cases with h2o's recorded answers, their truncations and mutations;
the plain model against the same fixture; and the argument refusals of the three calls, which enqueue nothing."""
import ctypes
import os
import shutil
import subprocess

import pytest

import cdigest_model as M
from conftest import ROOT


def test_model_matches_fixture():
    assert M.check_fixture() >= 300


def test_cdigest_host_clean_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes")
    g, vals, urls = M.load_fixture()
    lines = []
    for c in range(g["case_first"].size - 1):
        lines += ["C"] + ["V " + v.hex() for v in vals[g["case_first"][c]:g["case_first"][c + 1]]]
        lines.append("S %d %d %d %d" % tuple(g["summary"][c]))
        if g["summary"][c][0]:
            lines += ["L 0 %s %d" % (u.hex(), g["by_url"][c, k]) for k, u in enumerate(urls)]
            lines += ["L 1 %s %d" % ((u + g["etag"].tobytes()).hex(), g["by_url_etag"][c, k]) for k, u in enumerate(urls)]
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "cdigest_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *san, "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "h2o_amd", "csrc"),
                    os.path.join(ROOT, "tools", "cdigest_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(cases), "40"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.rstrip().startswith("ok: cdigest_host, %d cases" % (g["case_first"].size - 1)), r.stdout


def test_argument_refusals():
    """HHUFF_EINVAL for a NULL required array or a misaligned dig, HHUFF_OK for an empty batch: before any device call"""
    from h2o_amd import build, codec as C

    build.build(verbose=False)
    L = C.lib()
    err = L.hhuff_last_error_string()
    buf = (ctypes.c_uint8 * 256)()
    a = (ctypes.addressof(buf) + 15) & ~15
    calls = ((L.hhuff_cache_digests_load, [a, 64, a, a, a, 1, a, a, a, None], (0, 2, 3, 4, 6, 7, 8), 6, 5),
             (L.hhuff_cache_digests_load_fields, [a, 64, a, a, a, a, 1, 4, a, 0, a, a, a, None], (0, 2, 3, 4, 5, 8, 10, 11, 12), 10, 6),
             (L.hhuff_cache_digests_lookup, [a, a, 1, a, 64, a, 1, a, None, None], (0, 1, 3, 5, 7), 0, 6))
    for fn, ok, required, dig, count in calls:
        for k in required:
            assert fn(*[None if i == k else x for i, x in enumerate(ok)]) == -1, (fn.__name__, k)
        assert fn(*[a + 8 if i == dig else x for i, x in enumerate(ok)]) == -1  # a misaligned dig
        assert fn(*[0 if i == count else None if i in required else x for i, x in enumerate(ok)]) == 0  # an empty batch
    assert L.hhuff_last_error_string() == err
    assert C.cache_digests_bound(1000, 2) == 16 + 32 + 52000
