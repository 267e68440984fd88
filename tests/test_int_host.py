"""The prefix integer of the header decoders (h2o_amd/csrc/hhuff_int.h, the one definition the block decoders, the
literal kernels and the QPACK encoder sessions call) without a GPU: tools/int_host.cpp as a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer against the oracle's decode_int (orc_decode_int, golden-checked
against the reference in test_oracle_golden.py)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

INCOMPLETE, BAD = -255, -9


def encode(v, prefix, high):
    """h2o_hpack_encode_int's octets for v, the bits above the prefix all clear or all set; no limit on v"""
    pmax = (1 << prefix) - 1
    top = (0xFF & ~pmax) if high else 0
    if v < pmax:
        return bytes([top | v])
    out, v = [top | pmax], v - pmax
    while v >= 128:
        out.append(0x80 | (v & 127))
        v >>= 7
    return bytes(out + [v])


def build_cases():
    """(prefix, bytes, expected or None): the expected outcome where it is known by construction"""
    cases = []
    for prefix in (3, 4, 5, 6, 7, 8):
        pmax = (1 << prefix) - 1
        values = [pmax - 1, pmax] + [pmax + d for d in [0, 127, 128] + [x for k in range(2, 9) for x in ((1 << 7 * k) - 1, 1 << 7 * k)]]
        values.append((1 << 63) - 1)
        for high in ((False,) if prefix == 8 else (False, True)):
            full = [(encode(v, prefix, high), (v, None)) for v in values]
            # the two encodings that reach 2^63: the value itself, and every continuation bit set (pmax + 2^63 - 1)
            full.append((encode(1 << 63, prefix, high), (BAD, None)))
            full.append((encode(pmax + (1 << 63) - 1, prefix, high), (BAD, None)))
            assert all(len(e) == 10 for e, _ in full[-2:])
            # a tenth octet with its top bit set, whatever follows
            full.append((encode(pmax, prefix, high)[:1] + bytes([0x80] * 9), (BAD, None)))
            full.append((encode(pmax, prefix, high)[:1] + bytes([0xFF] * 9) + b"\x00", (BAD, None)))
            for enc, (want, _) in full:
                cases.append((prefix, enc, (want, len(enc)) if want >= 0 else (want, None)))
                for cut in range(min(len(enc), 10)):  # cut short at every byte
                    cases.append((prefix, enc[:cut], (INCOMPLETE, None)))
    return cases


def test_int_host_equals_the_oracle_under_sanitizers(tmp_path, oracle_codec):
    for prefix in (3, 4, 5, 6, 7, 8):  # the cases hold what they are meant to
        mine = [c for c in build_cases() if c[0] == prefix]
        assert {c[2][0] for c in mine} >= {(1 << prefix) - 2, (1 << prefix) - 1, (1 << 63) - 1, INCOMPLETE, BAD}
        assert max(len(c[1]) for c in mine) == 11 and any(len(c[1]) == 0 for c in mine)
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    probe_src = tmp_path / "probe.cpp"
    probe_src.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++", *san, str(probe_src), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes")
    cases = build_cases()
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for prefix, enc, _ in cases:
            f.write("%d %s\n" % (prefix, enc.hex() or "-"))
    exe = str(tmp_path / "int_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *san, "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "h2o_amd", "csrc"), os.path.join(ROOT, "tools", "int_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[len(cases)] == "ok: int_host %d" % len(cases), r.stdout[-2000:]
    for (prefix, enc, (want, used)), line in zip(cases, lines):
        got, consumed = (int(x) for x in line.split())
        ref, ref_consumed = oracle_codec.decode_int(enc, prefix)
        assert ref == want and (used is None or ref_consumed == used), (prefix, enc.hex(), ref, ref_consumed, want, used)
        assert got == ref, (prefix, enc.hex(), got, ref)
        if ref >= 0:  # the consumed count on success only
            assert consumed == ref_consumed, (prefix, enc.hex(), consumed, ref_consumed)
