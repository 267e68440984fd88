"""The untrusted-table check of include/hhuff.h (2j) point 7, on the host: tools/tokens_host.cpp -- the builder and
tok_find of h2o_amd/csrc/hhuff_tokens.h, the code the kernel runs -- built with AddressSanitizer and
UndefinedBehaviorSanitizer as a stand-alone program and run directly over built, damaged and cut-short tables in heap
blocks of exactly their size."""
import os
import shutil
import subprocess

import pytest

import tokens_model as TM
from conftest import ROOT


def test_tokens_host_clean_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes")
    names = tmp_path / "names.txt"
    names.write_bytes(b"".join(n + b"\n" for n in TM.load_fixture()["names"]))
    exe = str(tmp_path / "tokens_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *san, "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "h2o_amd", "csrc"),
                    os.path.join(ROOT, "tools", "tokens_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(names), "2000"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.rstrip().endswith("ok: tokens_host"), r.stdout
    assert "85 names" in r.stdout and "4096 names" in r.stdout
