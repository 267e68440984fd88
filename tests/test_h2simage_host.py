"""HTTP/2 stream table images (include/hhuff.h (2k'''), hhuff_h2_streams_export / _import), the part that needs no
GPU: the symbols and their codec names, the image bound, every host-side refusal, and the shared format / validator /
pack / unpack code (hhuff_h2simage.h) on the host under AddressSanitizer and UndefinedBehaviorSanitizer
(tools/h2simage_host.cpp).  The GPU side is tests/test_h2simage.py."""
import os
import shutil
import subprocess

import pytest

from h2o_amd import codec as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20  # a 16-byte aligned dummy address: never dereferenced on the paths below


def test_symbols_and_image_bound():
    L = C.lib()
    for name in ("hhuff_h2_streams_image_bound", "hhuff_h2_streams_export", "hhuff_h2_streams_import"):
        assert hasattr(L, name) and name in C.EXPORTED, name
    assert [C.h2_streams_image_bound(m) for m in (0, 1, 117, 2048, 2049, 1 << 24)] == [0, 112, 64 + 48 * 117, 64 + 48 * 2048, 0, 0]


def test_host_side_refusals():
    L = C.lib()
    slab = C.h2_streams_scratch_size(1, 117)

    def both(m=117, scratch=P, size=3 * slab, nslots=3, slot=P, n=1, img=P, img_off=P, img_len=P, status=P, export_too=True):
        rc = [L.hhuff_h2_streams_import(m, scratch, size, nslots, slot, n, img, img_off, img_len, status, None)]
        if export_too:
            rc.append(L.hhuff_h2_streams_export(m, scratch, size, nslots, slot, n, img, img_off, img_len, status, None))
        return rc

    for kw in (dict(m=0), dict(m=2049), dict(nslots=0), dict(nslots=1 << 31), dict(size=3 * slab - 1), dict(scratch=P + 8),
               dict(img=P + 4), dict(img_off=P + 4), dict(scratch=None), dict(slot=None), dict(img_len=None), dict(status=None),
               dict(img_off=None)):
        assert both(**kw) == [-1, -1], kw
    assert both(img=None, export_too=False) == [-1]  # import needs its images; export's size query does not
    assert both(n=0, slot=None, img=None, img_off=None, img_len=None, status=None) == [0, 0]  # nothing to do


def test_h2simage_host_clean_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "h2simage_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "h2o_amd", "csrc"),
                    os.path.join(ROOT, "tools", "h2simage_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, "120"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok:"), r.stdout
