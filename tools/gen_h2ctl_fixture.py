#!/usr/bin/env python3
"""Write tests/golden/h2ctl.npz: the answers of h2o's own payload decoders, h2o_http2_update_peer_settings and reply
encoders for a list of probe frames, from the real reference.

    python tools/gen_h2ctl_fixture.py [REF]        REF: the h2o tree (default $H2O_REF or /root/reference)

lib/http2/frame.c (and, for the reply encoders, lib/common/memory.c) links on its own (-ffunction-sections
-Wl,--gc-sections) against the small dump program below, which is compiled in a temporary directory and removed with
it; only the .npz is written.  Data only:
  probes, probe_off   the probes' bytes (u8 blob, u32 offsets [nprobes + 1]): one whole frame each (9-byte header and
                      payload), of the types 0 .. 12 bar the header frames
  pret                i32 [nprobes]: the return of the type's h2o_http2_decode_*_payload (types 0, 2, 3, 6, 7, 8), of
                      h2o_http2_update_peer_settings on the payload from H2O_HTTP2_SETTINGS_DEFAULT (type 4, whatever
                      its flags), else 1
  desc                u8: *err_desc as its index in tests/h2ctl_model.py ERR_TEXT, 0 NULL, 99 any other text
  out                 u32 [nprobes, 3], pret == 0: DATA payload.data - frame.payload, payload.length, 0; PRIORITY
                      exclusive, dependency, weight; RST_STREAM error_code; PING bytes 0-3 and 4-7 big-endian; GOAWAY
                      last_stream_id, error_code, debug_data.len; WINDOW_UPDATE window_size_increment
  stream_level        u8: WINDOW_UPDATE's *err_is_stream_level where pret != 0, else 0
  settings            u32 [nprobes, 5], type 4: the five settings afterwards, from the defaults
  pret2, settings2    the same from the start SETTINGS2
  replies             1 when the reply encoders linked; then reply, reply_off: per probe the bytes of
                      h2o_http2_encode_ping_frame(is_ack = 1, payload) for a PING of 8 bytes,
                      h2o_http2_encode_window_update_frame(0, out[0]) and h2o_http2__encode_rst_stream_frame(stream_id,
                      1) for a WINDOW_UPDATE of 4 bytes, back to back, else nothing
The probes: every such frame of the corpus files inside tests/golden/frames.npz; every frame of every connection of
tests/h2ctl_corpora.py; and RANDOM seeded random frames.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "h2ctl.npz")
RANDOM = 4000
SETTINGS2 = (0, 0, 7, 1000, 65536)

DUMP_C = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "h2o.h"
#include "h2o/http2_common.h"

static const char *TEXT[] = {NULL, "invalid stream id in DATA frame", "invalid DATA frame", "invalid stream id in PRIORITY frame",
    "invalid PRIORITY frame", "stream cannot depend on itself", "invalid stream id in RST_STREAM frame", "invalid RST_STREAM frame",
    "invalid stream id in SETTINGS frame", "invalid SETTINGS frame (+ACK)", "invalid SETTINGS frame", NULL, "invalid PING frame",
    "invalid stream id in GOAWAY frame", "invalid GOAWAY frame", "invalid WINDOW_UPDATE frame", "flow control window overflow"};

static int desc_of(const char *d)
{
    int i;
    if (d == NULL)
        return 0;
    for (i = 1; i != sizeof(TEXT) / sizeof(TEXT[0]); ++i)
        if (TEXT[i] != NULL && strcmp(TEXT[i], d) == 0)
            return i;
    return 99;
}

#ifdef WITH_REPLIES
int h2o_file_mktemp(const char *fn_template)
{
    return -1;
}
static h2o_buffer_mmap_settings_t mmap_settings = {1u << 30, "/nonexistent/h2ctl.XXXXXX"};
static h2o_buffer_prototype_t prototype = {{4096}, &mmap_settings};
#endif

/* one hex string per input line -> "pret desc out0 out1 out2 stream_level s0..s4 pret2 t0..t4 replyhex" */
int main(int argc, char **argv)
{
    char *line = NULL;
    size_t cap = 0;
    ssize_t got;
    while ((got = getline(&line, &cap, stdin)) > 0) {
        size_t n = strcspn(line, "\r\n") / 2, k;
        uint8_t *buf = malloc(n + 1);
        h2o_http2_frame_t frame;
        const char *err_desc = NULL;
        int pret = 1, pret2 = 1, level = 0;
        unsigned out[3] = {0, 0, 0};
        h2o_http2_settings_t s = H2O_HTTP2_SETTINGS_DEFAULT, t = {SETTINGS2};
        for (k = 0; k != n; ++k) {
            unsigned v;
            sscanf(line + 2 * k, "%2x", &v);
            buf[k] = (uint8_t)v;
        }
        if (h2o_http2_decode_frame(&frame, buf, n, 16777215, &err_desc) != (ssize_t)n) {
            fprintf(stderr, "probe is not one whole frame\n");
            return 1;
        }
        err_desc = NULL;
        switch (frame.type) {
        case H2O_HTTP2_FRAME_TYPE_DATA: {
            h2o_http2_data_payload_t p;
            if ((pret = h2o_http2_decode_data_payload(&p, &frame, &err_desc)) == 0)
                out[0] = (unsigned)(p.data - frame.payload), out[1] = (unsigned)p.length;
        } break;
        case H2O_HTTP2_FRAME_TYPE_PRIORITY: {
            h2o_http2_priority_t p;
            if ((pret = h2o_http2_decode_priority_payload(&p, &frame, &err_desc)) == 0)
                out[0] = p.exclusive, out[1] = p.dependency, out[2] = p.weight;
        } break;
        case H2O_HTTP2_FRAME_TYPE_RST_STREAM: {
            h2o_http2_rst_stream_payload_t p;
            if ((pret = h2o_http2_decode_rst_stream_payload(&p, &frame, &err_desc)) == 0)
                out[0] = p.error_code;
        } break;
        case H2O_HTTP2_FRAME_TYPE_SETTINGS: {
            const char *d2 = NULL;
            pret = h2o_http2_update_peer_settings(&s, frame.payload, frame.length, &err_desc);
            pret2 = h2o_http2_update_peer_settings(&t, frame.payload, frame.length, &d2);
        } break;
        case H2O_HTTP2_FRAME_TYPE_PING: {
            h2o_http2_ping_payload_t p;
            if ((pret = h2o_http2_decode_ping_payload(&p, &frame, &err_desc)) == 0) {
                out[0] = h2o_http2_decode32u(p.data), out[1] = h2o_http2_decode32u(p.data + 4);
            }
        } break;
        case H2O_HTTP2_FRAME_TYPE_GOAWAY: {
            h2o_http2_goaway_payload_t p;
            if ((pret = h2o_http2_decode_goaway_payload(&p, &frame, &err_desc)) == 0)
                out[0] = p.last_stream_id, out[1] = p.error_code, out[2] = (unsigned)p.debug_data.len;
        } break;
        case H2O_HTTP2_FRAME_TYPE_WINDOW_UPDATE: {
            h2o_http2_window_update_payload_t p;
            int lv = 0;
            if ((pret = h2o_http2_decode_window_update_payload(&p, &frame, &err_desc, &lv)) == 0)
                out[0] = p.window_size_increment;
            else
                level = lv;
        } break;
        default:
            break;
        }
        printf("%d %d %u %u %u %d %u %u %u %u %u %d %u %u %u %u %u ", pret, desc_of(err_desc), out[0], out[1], out[2], level,
               s.header_table_size, s.enable_push, s.max_concurrent_streams, s.initial_window_size, s.max_frame_size, pret2,
               t.header_table_size, t.enable_push, t.max_concurrent_streams, t.initial_window_size, t.max_frame_size);
#ifdef WITH_REPLIES
        {
            h2o_buffer_t *b;
            size_t i;
            h2o_buffer_init(&b, &prototype);
            if (frame.type == H2O_HTTP2_FRAME_TYPE_PING && frame.length == 8)
                h2o_http2_encode_ping_frame(&b, 1, frame.payload);
            if (frame.type == H2O_HTTP2_FRAME_TYPE_WINDOW_UPDATE && frame.length == 4) {
                h2o_http2_encode_window_update_frame(&b, 0, (int32_t)out[0]);
                h2o_http2__encode_rst_stream_frame(&b, frame.stream_id, 1);
            }
            for (i = 0; i != b->size; ++i)
                printf("%02x", (uint8_t)b->bytes[i]);
            h2o_buffer_dispose(&b);
        }
#endif
        printf("-\n");
        free(buf);
    }
    return 0;
}
""".replace("SETTINGS2", ", ".join(str(v) for v in SETTINGS2))

HEADER_TYPES = (1, 5, 9)


def whole_frames(buf):
    """the whole frames of a buffer that are no header frames, by the length fields alone"""
    out, pos = [], 0
    while len(buf) - pos >= 9:
        size = 9 + int.from_bytes(buf[pos:pos + 3], "big")
        if len(buf) - pos < size:
            break
        if buf[pos + 3] not in HEADER_TYPES:
            out.append(bytes(buf[pos:pos + size]))
        pos += size
    return out


def random_frames(seed=29):
    rng = np.random.default_rng(seed)
    fixed = {2: 5, 3: 4, 6: 8, 7: 8, 8: 4}
    out = []
    for _ in range(RANDOM):
        typ = int(rng.choice([0, 2, 3, 4, 4, 4, 6, 7, 8, 8, 10, 11, 12]))
        flags = int(rng.integers(0, 256)) if rng.random() < 0.3 else int(rng.choice([0, 0, 1, 8, 9]))
        sid = int(rng.choice([0, 0, 1, 2, 3, 0x80000000, 0x80000001, int(rng.integers(0, 2 ** 32))]))
        if typ == 4:
            pairs = []
            for _ in range(int(rng.integers(0, 5))):
                ident = int(rng.choice([1, 2, 3, 4, 5, 5, 4, 2, 0, 6, 0x99]))
                value = int(rng.choice([0, 1, 2, 100, 16383, 16384, 16385, 65535, 16777215, 16777216, 0x7fffffff, 0x80000000,
                                        0xffffffff, int(rng.integers(0, 2 ** 32))]))
                pairs.append(ident.to_bytes(2, "big") + value.to_bytes(4, "big"))
            payload = b"".join(pairs) + bytes(rng.integers(0, 256, int(rng.choice([0, 0, 0, 1, 5])), dtype=np.uint8))
        else:
            n = fixed.get(typ, int(rng.integers(0, 12)))
            if rng.random() < 0.3:
                n = max(0, n + int(rng.choice([-1, 1, 2])))
            payload = bytes(rng.integers(0, 256, n, dtype=np.uint8))
            if typ in (2, 8, 7) and n >= 4 and rng.random() < 0.5:  # small ids and increments, the reserved bit on and off
                word = int(rng.choice([0, 1, 3, sid & 0x7fffffff, 0x7fffffff])) | (0x80000000 if rng.random() < 0.5 else 0)
                payload = word.to_bytes(4, "big") + payload[4:]
            if typ == 0 and n and rng.random() < 0.7:
                payload = bytes([int(rng.integers(0, n + 2))]) + payload[1:]  # a pad length near the payload's size
        out.append(len(payload).to_bytes(3, "big") + bytes([typ, flags]) + sid.to_bytes(4, "big") + payload)
    return out


def pack(strings):
    off = np.zeros(len(strings) + 1, np.uint32)
    off[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
    return np.frombuffer(b"".join(strings), np.uint8).copy(), off


def main():
    import h2ctl_corpora

    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("H2O_REF", "/root/reference")
    frame_c = os.path.join(ref, "lib", "http2", "frame.c")
    memory_c = os.path.join(ref, "lib", "common", "memory.c")
    if not os.path.exists(frame_c):
        sys.exit("no h2o tree at %s (lib/http2/frame.c)" % ref)
    with np.load(os.path.join(ROOT, "tests", "golden", "frames.npz")) as z:
        files, file_off = z["files"], z["file_off"]
    probes = []
    for f in range(file_off.size - 1):
        probes += whole_frames(bytes(files[int(file_off[f]):int(file_off[f + 1])]))
    n_files = len(probes)
    for c in h2ctl_corpora.CASES:
        probes += whole_frames(c["buf"])
    n_corpus = len(probes) - n_files
    probes += random_frames()
    inc = [os.path.join(ref, "include")] + [os.path.join(ref, "deps", d) for d in (
        "picotls/include", "quicly/include", "klib", "golombset", "cloexec", "yoml", "libgkc", "libyrmcds", "picohttpparser",
        "hiredis", "brotli/c/include")]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "dump_h2ctl.c"), os.path.join(tmp, "dump_h2ctl")
        with open(src, "w") as f:
            f.write(DUMP_C)
        base = ["gcc", "-O1", "-w", "-DH2O_USE_LIBUV=0", "-ffunction-sections", "-fdata-sections"] + ["-I" + d for d in inc]
        tail = ["-Wl,--gc-sections", "-lpthread", "-o", exe]
        replies = subprocess.run(base + ["-DWITH_REPLIES", src, frame_c, memory_c] + tail, capture_output=True).returncode == 0
        if not replies:
            subprocess.run(base + [src, frame_c] + tail, check=True)
        feed = "".join(p.hex() + "\n" for p in probes)
        lines = [r for r in subprocess.run([exe], input=feed, check=True, capture_output=True, text=True).stdout.split("\n") if r]
    assert len(lines) == len(probes), (len(lines), len(probes))
    rows = np.array([[int(x) for x in r.split()[:17]] for r in lines], np.int64)
    reply = [bytes.fromhex(r.split()[17].rstrip("-")) for r in lines]
    pblob, poff = pack(probes)
    rblob, roff = pack(reply)
    np.savez_compressed(OUT, probes=pblob, probe_off=poff, pret=rows[:, 0].astype(np.int32), desc=rows[:, 1].astype(np.uint8),
                        out=rows[:, 2:5].astype(np.uint32), stream_level=rows[:, 5].astype(np.uint8),
                        settings=rows[:, 6:11].astype(np.uint32), pret2=rows[:, 11].astype(np.int32),
                        settings2=rows[:, 12:17].astype(np.uint32), settings2_start=np.array(SETTINGS2, np.uint32),
                        replies=np.array(int(replies), np.uint8), reply=rblob, reply_off=roff)
    print("%s: %d probes (%d from the corpus files, %d from h2ctl_corpora, %d random), %d refused, replies %s; %d bytes"
          % (os.path.relpath(OUT, ROOT), len(probes), n_files, n_corpus, RANDOM, int((rows[:, 0] < 0).sum()),
             "recorded" if replies else "not linked", os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
