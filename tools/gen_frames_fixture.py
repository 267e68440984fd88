#!/usr/bin/env python3
"""Write tests/golden/frames.npz: h2o_http2_decode_frame's and h2o_http2_decode_headers_payload's own answers for a
list of probe frames, from the real reference.

    python tools/gen_frames_fixture.py [REF]        REF: the h2o tree (default $H2O_REF or /root/reference)

lib/http2/frame.c links on its own (-ffunction-sections -Wl,--gc-sections) against the small dump program below,
which is compiled in a temporary directory and removed with it; only the .npz is written.  Data only:
  probes, probe_off   the probes' bytes (u8 blob, u32 offsets [nprobes + 1]): a probe is what is left of a buffer from
                      a frame's first byte on, cut behind the frame where it is complete
  ret                 i32 [nprobes]: h2o_http2_decode_frame(probe, max_frame_size 16384)
  hret                i32 [nprobes]: h2o_http2_decode_headers_payload's return where ret >= 0 and the type is HEADERS,
                      else 1
  desc                u8: its *err_desc -- 0 NULL, 1 "invalid stream id in HEADERS frame", 2 "invalid HEADERS frame",
                      9 anything else
  frag_off, frag_len  u32: payload.headers - frame.payload, payload.headers_len   (hret == 0)
  exclusive, dependency, weight   u32: payload.priority                           (hret == 0)
  files, file_off     a subset of fuzz/http2-corpus, each file behind its 24-byte preface where it has one, back to
                      back (u8 blob, u32 offsets); file_probe0 [nfiles + 1]: the file's frames are the probes
                      file_probe0[f] .. file_probe0[f + 1] - 1, in order, cut by the length fields alone
The probes: every frame of those files; every frame of every connection of tests/frames_corpora.py; and RANDOM seeded
random frames.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "frames.npz")
RANDOM = 4000
FILE_MAX, FILES_TOTAL = 4096, 300 * 1024  # per file and in all (raw bytes): keeps the .npz well under 1 MB
PREFACE = b"PRI * HTTP/2.0\r\n\r\nSM\r\n\r\n"

DUMP_C = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "h2o.h"
#include "h2o/http2_common.h"

/* one hex string per input line -> "ret hret desc frag_off frag_len exclusive dependency weight" */
int main(void)
{
    char *line = NULL;
    size_t cap = 0;
    ssize_t got;
    while ((got = getline(&line, &cap, stdin)) > 0) {
        size_t n = strcspn(line, "\r\n") / 2, k;
        uint8_t *buf = malloc(n + 1);
        h2o_http2_frame_t frame;
        h2o_http2_headers_payload_t payload;
        const char *err_desc = NULL;
        ssize_t ret;
        int hret = 1, desc = 0;
        memset(&payload, 0, sizeof(payload));
        for (k = 0; k != n; ++k) {
            unsigned v;
            sscanf(line + 2 * k, "%2x", &v);
            buf[k] = (uint8_t)v;
        }
        ret = h2o_http2_decode_frame(&frame, buf, n, 16384, &err_desc);
        if (ret >= 0 && frame.type == H2O_HTTP2_FRAME_TYPE_HEADERS) {
            err_desc = NULL;
            hret = h2o_http2_decode_headers_payload(&payload, &frame, &err_desc);
            if (err_desc != NULL)
                desc = strcmp(err_desc, "invalid stream id in HEADERS frame") == 0 ? 1
                       : strcmp(err_desc, "invalid HEADERS frame") == 0            ? 2
                                                                                   : 9;
        }
        if (hret == 0)
            printf("%ld 0 0 %ld %lu %u %u %u\n", (long)ret, (long)(payload.headers - frame.payload),
                   (unsigned long)payload.headers_len, (unsigned)payload.priority.exclusive,
                   (unsigned)payload.priority.dependency, (unsigned)payload.priority.weight);
        else
            printf("%ld %d %d 0 0 0 0 0\n", (long)ret, hret, desc);
        free(buf);
    }
    return 0;
}
"""


def cut_frames(buf):
    """the probes of a buffer: from each frame's first byte, following the length fields, to the frame's end (or the
    buffer's, for the last one)"""
    out, pos = [], 0
    while pos < len(buf):
        if len(buf) - pos < 9:
            out.append(buf[pos:])
            break
        size = 9 + int.from_bytes(buf[pos:pos + 3], "big")
        out.append(buf[pos:pos + size])
        pos += size
    return out


def random_frames(seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(RANDOM):
        typ = int(rng.choice([0, 1, 1, 1, 1, 5, 9, 4, 0xfa]))
        flags = int(rng.integers(0, 256)) if rng.random() < 0.5 else int(rng.choice([0, 4, 5, 0x8, 0xc, 0x20, 0x24, 0x2c, 0x2d]))
        sid = int(rng.choice([0, 1, 2, 3, 0x80000001, int(rng.integers(0, 2 ** 32))]))
        n = int(rng.integers(0, 24))
        payload = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        if n and rng.random() < 0.5:
            payload = bytes([int(rng.integers(0, n + 2))]) + payload[1:]  # a pad length near the payload's size
        length = n if rng.random() < 0.9 else int(rng.choice([n + 1, 16384, 16385, 2 ** 24 - 1]))
        f = length.to_bytes(3, "big") + bytes([typ, flags]) + sid.to_bytes(4, "big") + payload
        if rng.random() < 0.1:
            f = f[:int(rng.integers(0, len(f) + 1))]
        out.append(f)
    return out


def pack(strings):
    off = np.zeros(len(strings) + 1, np.uint32)
    off[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
    return np.frombuffer(b"".join(strings), np.uint8).copy(), off


def main():
    import frames_corpora

    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("H2O_REF", "/root/reference")
    frame_c = os.path.join(ref, "lib", "http2", "frame.c")
    corpus = os.path.join(ref, "fuzz", "http2-corpus")
    if not os.path.exists(frame_c) or not os.path.isdir(corpus):
        sys.exit("no h2o tree at %s (lib/http2/frame.c, fuzz/http2-corpus)" % ref)
    files, total = [], 0
    for name in sorted(os.listdir(corpus)):
        with open(os.path.join(corpus, name), "rb") as f:
            b = f.read()
        if b.startswith(PREFACE):
            b = b[len(PREFACE):]
        if 0 < len(b) <= FILE_MAX and total + len(b) <= FILES_TOTAL:
            files.append(b)
            total += len(b)
    probes, file_probe0 = [], [0]
    for b in files:
        probes += cut_frames(b)
        file_probe0.append(len(probes))
    for c in frames_corpora.CASES:
        probes += cut_frames(c["buf"])
    probes += random_frames()
    inc = [os.path.join(ref, "include")] + [os.path.join(ref, "deps", d) for d in (
        "picotls/include", "quicly/include", "klib", "golombset", "cloexec", "yoml", "libgkc", "libyrmcds", "picohttpparser",
        "hiredis", "brotli/c/include")]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "dump_frames.c"), os.path.join(tmp, "dump_frames")
        with open(src, "w") as f:
            f.write(DUMP_C)
        subprocess.run(["gcc", "-O1", "-w", "-DH2O_USE_LIBUV=0", "-ffunction-sections", "-fdata-sections", src, frame_c] +
                       ["-I" + d for d in inc] + ["-Wl,--gc-sections", "-o", exe], check=True)
        feed = "".join(p.hex() + "\n" for p in probes)
        rows = subprocess.run([exe], input=feed, check=True, capture_output=True, text=True).stdout.split("\n")
    rows = np.array([[int(x) for x in r.split()] for r in rows if r], np.int64)
    assert rows.shape == (len(probes), 8), rows.shape
    pblob, poff = pack(probes)
    fblob, foff = pack(files)
    u32 = lambda k: rows[:, k].astype(np.uint32)  # noqa: E731
    np.savez_compressed(OUT, probes=pblob, probe_off=poff, ret=rows[:, 0].astype(np.int32), hret=rows[:, 1].astype(np.int32),
                        desc=rows[:, 2].astype(np.uint8), frag_off=u32(3), frag_len=u32(4), exclusive=u32(5), dependency=u32(6),
                        weight=u32(7), files=fblob, file_off=foff, file_probe0=np.array(file_probe0, np.uint32))
    print("%s: %d probes (%d from %d corpus files of %d bytes), %d HEADERS payloads decoded, %d refused; %d bytes"
          % (os.path.relpath(OUT, ROOT), len(probes), file_probe0[-1], len(files), total,
             int((rows[:, 1] == 0).sum()), int((rows[:, 1] < 0).sum()), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
