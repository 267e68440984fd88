"""The HTTP/3 body arithmetic without a GPU: tools/h3bodies_host.cpp -- h2o_amd/csrc/hhuff_h3bodies.h's DATA header, the
content-length bisection and the line writer, the code the kernels run -- as a stand-alone program under AddressSanitizer
and UndefinedBehaviorSanitizer.  The program holds its own expectations (header bytes written out by hand, h2o's loop,
memcpy); it also checks the 8-byte varint, which no GPU test reaches."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_header_bisection_and_lines_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    (tmp_path / "probe.cpp").write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++", *san, str(tmp_path / "probe.cpp"), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes")
    exe = str(tmp_path / "h3bodies_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *san, "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "h2o_amd", "csrc"),
                    os.path.join(ROOT, "tools", "h3bodies_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "ok: h3bodies_host, 2133 streams" in r.stderr, r.stderr[-4000:]

