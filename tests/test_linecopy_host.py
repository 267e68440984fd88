"""The line copy and the range clamp without a GPU: tools/linecopy_host.cpp -- h2o_amd/csrc/hhuff_linecopy.h's load16,
store_part, copy_line, lines_of and clamp_range, the code every copy kernel runs -- as a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer: the copies against memcpy between canary bytes at every source residue
0-3, destination residue 0-15 and length 1-48, the clamp against its definition for all a, b, cap of 0 .. 9,
2^32 - 2 and 2^32 - 1."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_line_copy_and_clamp_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes")
    exe = str(tmp_path / "linecopy_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *san, "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "h2o_amd", "csrc"),
                    os.path.join(ROOT, "tools", "linecopy_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "ok: linecopy_host" in r.stderr, r.stderr[-4000:]
