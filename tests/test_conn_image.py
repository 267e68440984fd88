"""Connection images (include/hhuff.h (2i)), the part that needs no GPU: the symbols and their codec names, the
slab sizes against the families' own size functions, the image bound, every host-side refusal, the header as C99,
C11 and C++17, the constants against h2o_amd.codec, and the shared layout / validator code (hhuff_image.h) on the
host under AddressSanitizer and UndefinedBehaviorSanitizer (tools/image_host.cpp).  The GPU side is
tests/test_conn_image_gpu.py."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from h2o_amd import codec as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hhuff_conn_slab_size", "hhuff_conn_image_bound", "hhuff_conn_export", "hhuff_conn_import")
P = 1 << 20  # a 16-byte aligned dummy address: never dereferenced on the paths below


def test_symbols_are_exported_and_listed():
    L = C.lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in C.EXPORTED


@pytest.mark.parametrize("table", [0, 128, 4096, 65536])
def test_slab_size_is_the_familys_own(table):
    L = C.lib()
    assert C.conn_slab_size(C.conn_family(C.FAM_HPACK_DEC, table)) == L.hhuff_hpack_scratch_size(1, table)
    assert C.conn_slab_size(C.conn_family(C.FAM_QPACK_DEC, table)) == L.hhuff_qpack_scratch_size(1, table)
    assert C.conn_slab_size(C.conn_family(C.FAM_HPACK_ENC)) == L.hhuff_hpack_enc_scratch_size(1)
    for m in (1, 64):
        assert C.conn_slab_size(C.conn_family(C.FAM_QPACK_ENC, table, m)) == L.hhuff_qpack_enc_scratch_size(1, table, m)
    for b in (0, 100, 4096):
        want = L.hhuff_qpack_dsession_state_size(1, b)
        assert want and C.conn_slab_size(C.conn_family(C.FAM_QPACK_DSESSION, max_blocked=b)) == want


BAD = [(C.FAM_QPACK_ENC, 65537, 1, 0), (C.FAM_QPACK_DEC, (1 << 30) + 1, 0, 0), (C.FAM_QPACK_DSESSION, 0, 0, 4097),
       (5, 0, 0, 0), (0xFFFFFFFF, 0, 0, 0),
       # a non-zero unused field
       (C.FAM_HPACK_DEC, 4096, 1, 0), (C.FAM_HPACK_DEC, 4096, 0, 1), (C.FAM_QPACK_DEC, 4096, 1, 0),
       (C.FAM_QPACK_DEC, 4096, 0, 1), (C.FAM_HPACK_ENC, 4096, 0, 0), (C.FAM_HPACK_ENC, 0, 1, 0), (C.FAM_HPACK_ENC, 0, 0, 1),
       (C.FAM_QPACK_ENC, 4096, 64, 1), (C.FAM_QPACK_DSESSION, 4096, 0, 100), (C.FAM_QPACK_DSESSION, 0, 1, 100)]


@pytest.mark.parametrize("fam", BAD)
def test_bad_parameters_have_no_slab(fam):
    f = C.conn_family(*fam)
    assert C.conn_slab_size(f) == 0 and C.conn_image_bound(f) == 0
    L = C.lib()
    assert L.hhuff_conn_export(ctypes.byref(f), P, 1 << 30, 1, P, 1, P, P, P, P, None) == -1
    assert L.hhuff_conn_import(ctypes.byref(f), P, 1 << 30, 1, P, 1, P, P, P, P, None) == -1
    assert L.hhuff_conn_slab_size(None) == 0 and L.hhuff_conn_image_bound(None) == 0


def maxima(fam):
    """(records, string bytes) an image of the family can hold at most: every entry costs its bytes + 32 of the
    table, the lists are as long as their parameters say"""
    kind, table, inflight, blocked = fam
    if kind == C.FAM_HPACK_ENC:
        return 32, 4096
    if kind == C.FAM_QPACK_DSESSION:
        return blocked, 0
    return table // 32 + inflight, table


@pytest.mark.parametrize("fam", [(C.FAM_HPACK_DEC, 0, 0, 0), (C.FAM_HPACK_DEC, 4096, 0, 0), (C.FAM_HPACK_DEC, 65536, 0, 0),
                                 (C.FAM_QPACK_DEC, 0, 0, 0), (C.FAM_QPACK_DEC, 128, 0, 0), (C.FAM_QPACK_DEC, 65536, 0, 0),
                                 (C.FAM_HPACK_ENC, 0, 0, 0), (C.FAM_QPACK_ENC, 128, 1, 0), (C.FAM_QPACK_ENC, 65536, 64, 0),
                                 (C.FAM_QPACK_DSESSION, 0, 0, 0), (C.FAM_QPACK_DSESSION, 0, 0, 4096)])
def test_image_bound(fam):
    b = C.conn_image_bound(C.conn_family(*fam))
    records, strings = maxima(fam)
    assert b % 16 == 0 and b >= 96 + 32 * records + strings + 15
    assert b <= 96 + 32 * (records + 1) + strings + 15 + 32  # and no more than that (one spare ring slot, rounding)


def test_host_side_refusals():
    L = C.lib()
    f = C.conn_family(C.FAM_QPACK_ENC, 4096, 64)
    slab = C.conn_slab_size(f)
    fr = ctypes.byref(f)

    def both(scratch=P, size=3 * slab, nslots=3, slot=P, n=1, img=P, img_off=P, img_len=P, status=P, export_too=True):
        rc = [L.hhuff_conn_import(fr, scratch, size, nslots, slot, n, img, img_off, img_len, status, None)]
        if export_too:
            rc.append(L.hhuff_conn_export(fr, scratch, size, nslots, slot, n, img, img_off, img_len, status, None))
        return rc

    for kw, word in ((dict(nslots=0), b"nslots"), (dict(nslots=1 << 31), b"nslots"), (dict(size=3 * slab - 1), b"scratch"),
                     (dict(scratch=P + 8), b"aligned"), (dict(img=P + 4), b"aligned"), (dict(scratch=None), b"NULL"),
                     (dict(slot=None), b"NULL"), (dict(img_len=None), b"NULL"), (dict(status=None), b"NULL"),
                     (dict(img_off=None), b"NULL")):
        assert both(**kw) == [-1, -1], kw
        assert word in L.hhuff_last_error_string(), (kw, L.hhuff_last_error_string())
    assert both(img=None, export_too=False) == [-1]  # import needs its images; export's size query does not
    # n == 0: nothing to do, whatever the arrays
    assert both(n=0, slot=None, img=None, img_off=None, img_len=None, status=None) == [0, 0]


@pytest.mark.parametrize("cc, std", [("gcc", "-std=c99"), ("gcc", "-std=c11"), ("g++", "-std=c++17")])
def test_header_compiles(tmp_path, cc, std):
    if not shutil.which(cc):
        pytest.skip("no host compiler")
    src = tmp_path / ("t.c" if cc == "gcc" else "t.cpp")
    src.write_text('#include "hhuff.h"\n'
                   "uint64_t use(uint8_t *img, const uint64_t *off, uint32_t *len, int32_t *st, const uint32_t *slot) {\n"
                   "    hhuff_conn_family_t f = {HHUFF_FAM_QPACK_ENC, 4096u, 64u, 0u};\n"
                   "    unsigned fams = HHUFF_FAM_HPACK_DEC + HHUFF_FAM_QPACK_DEC + HHUFF_FAM_HPACK_ENC + HHUFF_FAM_QPACK_DSESSION;\n"
                   "    int codes = HHUFF_IMG_SPACE + HHUFF_IMG_EINVAL + HHUFF_IMG_EFORMAT + HHUFF_IMG_EPARAM;\n"
                   "    int rc = hhuff_conn_export(&f, img, 0, 1, slot, 0, img, off, len, st, 0);\n"
                   "    rc += hhuff_conn_import(&f, img, 0, 1, slot, 0, img, off, len, st, 0);\n"
                   "    return hhuff_conn_slab_size(&f) + hhuff_conn_image_bound(&f) + fams + (uint64_t)(codes + rc);\n"
                   "}\n")
    subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                    str(src)], check=True)


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "hhuff.h")).read()
    defs = {m.group(1): m.group(2) for m in re.finditer(r"#define\s+(HHUFF_(?:FAM|IMG)_\w+)\s+\(?(-?\d+)u?\)?", text)}
    want = dict(HHUFF_FAM_HPACK_DEC=C.FAM_HPACK_DEC, HHUFF_FAM_QPACK_DEC=C.FAM_QPACK_DEC, HHUFF_FAM_HPACK_ENC=C.FAM_HPACK_ENC,
                HHUFF_FAM_QPACK_ENC=C.FAM_QPACK_ENC, HHUFF_FAM_QPACK_DSESSION=C.FAM_QPACK_DSESSION,
                HHUFF_IMG_SPACE=C.IMG_SPACE, HHUFF_IMG_EINVAL=C.IMG_EINVAL, HHUFF_IMG_EFORMAT=C.IMG_EFORMAT,
                HHUFF_IMG_EPARAM=C.IMG_EPARAM)
    assert {k: int(v) for k, v in defs.items()} == want
    assert ctypes.sizeof(C._ConnFamilyStruct) == 16


def test_image_host_clean_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "image_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "h2o_amd", "csrc"),
                    os.path.join(ROOT, "tools", "image_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, "120"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok:"), r.stdout
