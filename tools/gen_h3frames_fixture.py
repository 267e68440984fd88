#!/usr/bin/env python3
"""Write tests/golden/h3frames.npz: the answers of h2o_http3_read_frame, h2o_http3_handle_settings_frame,
h2o_http3_decode_priority_update_frame and h2o_http3_decode_goaway_frame for a list of probes, from the real reference.

    python tools/gen_h3frames_fixture.py [REF]        REF: the h2o tree (default $H2O_REF)

lib/http3/frame.c, lib/http3/common.c and deps/picotls/lib/picotls.c link on their own (-ffunction-sections
-Wl,--gc-sections) against the small dump program below, which brings the few symbols the kept functions still want (a
QPACK context with an encoder_table_capacity of 2^32 - 1, so that h2o's clamp is the saturation (2l) documents;
h2o_qpack_create_encoder, which records its arguments; h2o__fatal) and a quicly connection that is nothing but its public part with
the remote max_datagram_frame_size set.  It is compiled in a temporary directory and removed with it; only the .npz is
written.  Data only:
  probes, probe_off   the probes' bytes (u8 blob, u32 offsets [nprobes + 1])
  mode                u8: 0 read_frame (probe = the stream's bytes from the frame's first byte on), 1 settings,
                      2 priority update, 3 goaway (probe = the payload)
  arg                 u32 [nprobes, 4]: read_frame: is_client, control stream, max_frame_payload_size; settings: the
                      remote max_datagram_frame_size != 0; priority update: is_push
  ret                 i64: the function's return value
  desc                u8: *err_desc -- 0 NULL, 1 h2o_http3_err_frame_too_large, 2 "malformed SETTINGS frame",
                      3 "invalid PRIORITY frame", 4 "Invalid GOAWAY frame", 9 anything else
  val                 u64 [nprobes, 4]: read_frame (ret 0 or a type that was read): type, length, _header_size, the
                      bytes *src moved; settings (ret 0): max_field_section_size (2^64 - 1: untouched), the
                      header_table_size and blocked_streams h2o_qpack_create_encoder got, h3_datagram; priority update
                      (ret 0): element, value.base - payload; goaway (ret 0): stream_or_push_id
The probes: every frame position and every payload of tests/h3frames_corpora.py under both sides and both stream kinds,
and RANDOM seeded random ones.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "h3frames.npz")
RANDOM = 6000

DUMP_C = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "h2o.h"
#include "h2o/http3_common.h"
#include "h2o/http3_internal.h"
#include "h2o/qpack.h"

static uint64_t enc_args[2];
h2o_qpack_encoder_t *h2o_qpack_create_encoder(uint32_t header_table_size, uint64_t max_blocked)
{
    enc_args[0] = header_table_size, enc_args[1] = max_blocked;
    return (void *)enc_args;
}

__attribute__((noreturn)) static void fatal(const char *file, int line, const char *msg, ...)
{
    fprintf(stderr, "fatal: %s:%d: %s\n", file, line, msg);
    abort();
}

__attribute__((noreturn)) void (*h2o__fatal)(const char *, int, const char *, ...) = fatal;

static int desc_of(const char *d)
{
    if (d == NULL)
        return 0;
    if (d == h2o_http3_err_frame_too_large)
        return 1;
    if (strcmp(d, "malformed SETTINGS frame") == 0)
        return 2;
    if (strcmp(d, "invalid PRIORITY frame") == 0)
        return 3;
    if (strcmp(d, "Invalid GOAWAY frame") == 0)
        return 4;
    return 9;
}

/* "mode a0 a1 a2 hex" per input line -> "ret desc v0 v1 v2 v3" */
int main(void)
{
    char *line = NULL;
    size_t cap = 0;
    while (getline(&line, &cap, stdin) > 0) {
        unsigned mode, a0, a1, a2;
        int at = 0;
        sscanf(line, "%u %u %u %u %n", &mode, &a0, &a1, &a2, &at);
        const char *hex = line + at;
        size_t n = *hex == '-' ? 0 : strcspn(hex, "\r\n") / 2, k;
        uint8_t *buf = malloc(n + 1);
        const char *err_desc = NULL;
        long long ret = 0;
        unsigned long long v[4] = {0, 0, 0, 0};
        for (k = 0; k != n; ++k) {
            unsigned x;
            sscanf(hex + 2 * k, "%2x", &x);
            buf[k] = (uint8_t)x;
        }
        if (mode == 0) {
            h2o_http3_read_frame_t frame;
            const uint8_t *src = buf;
            memset(&frame, 0, sizeof(frame));
            frame.type = UINT64_MAX;
            ret = h2o_http3_read_frame(&frame, (int)a0, a1 ? H2O_HTTP3_STREAM_TYPE_CONTROL : H2O_HTTP3_STREAM_TYPE_REQUEST, a2, &src,
                                       buf + n, &err_desc);
            v[0] = frame.type, v[1] = frame.length, v[2] = frame._header_size, v[3] = (unsigned long long)(src - buf);
        } else if (mode == 1) {
            static h2o_http3_conn_t conn;
            static h2o_http3_qpack_context_t qctx;
            static struct _st_quicly_conn_public_t quic;
            memset(&conn, 0, sizeof(conn)), memset(&quic, 0, sizeof(quic));
            qctx.encoder_table_capacity = UINT32_MAX;
            conn.qpack.ctx = &qctx;
            conn.super.quic = (quicly_conn_t *)&quic;
            conn.peer_settings.max_field_section_size = UINT64_MAX;
            quic.remote.transport_params.max_datagram_frame_size = a0 ? 1200 : 0;
            enc_args[0] = enc_args[1] = 0;
            ret = h2o_http3_handle_settings_frame(&conn, buf, n, &err_desc);
            v[0] = conn.peer_settings.max_field_section_size, v[1] = enc_args[0], v[2] = enc_args[1], v[3] = conn.peer_settings.h3_datagram;
        } else if (mode == 2) {
            h2o_http3_priority_update_frame_t frame;
            memset(&frame, 0, sizeof(frame));
            ret = h2o_http3_decode_priority_update_frame(&frame, (int)a0, buf, n, &err_desc);
            if (ret == 0)
                v[0] = frame.element, v[1] = (unsigned long long)((const uint8_t *)frame.value.base - buf);
        } else {
            h2o_http3_goaway_frame_t frame;
            memset(&frame, 0, sizeof(frame));
            ret = h2o_http3_decode_goaway_frame(&frame, buf, n, &err_desc);
            if (ret == 0)
                v[0] = frame.stream_or_push_id;
        }
        printf("%lld %d %llu %llu %llu %llu\n", ret, desc_of(err_desc), v[0], v[1], v[2], v[3]);
        free(buf);
    }
    return 0;
}
"""


def frame_positions(buf):
    """where frames begin in a stream, by the varints alone (DATA payloads stepped over as far as they are there)"""
    import h3frames_model as M

    out, pos = [], 0
    while pos < len(buf):
        out.append(pos)
        typ, p = M.quicint(buf, pos, len(buf))
        if typ is None:
            break
        length, p = M.quicint(buf, p, len(buf))
        if length is None or p + length > len(buf):
            break
        pos = p + length
    return out


def random_probes(seed=17):
    import h3frames_corpora as K

    rng = np.random.default_rng(seed)
    types = [0, 1, 3, 4, 5, 7, 13, 0xF0700, 0xF0701, 0x21, 2, 6, 0x40, (1 << 40) + 1]
    out = []
    for _ in range(RANDOM):
        mode = int(rng.choice([0, 0, 0, 1, 1, 2, 3]))
        n = int(rng.integers(0, 20))
        body = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        if mode == 0:
            w = lambda v: K.vi(v, int(rng.choice([8, 4, 2, 1])) if rng.random() < 0.3 and v < 64 else None)  # noqa: E731
            length = n if rng.random() < 0.8 else int(rng.choice([n + 1, 16384, 16385, 1 << 33]))
            b = w(int(rng.choice(types))) + w(length) + body
            if rng.random() < 0.15:
                b = b[:int(rng.integers(0, len(b) + 1))]
            out.append((0, int(rng.integers(2)), int(rng.integers(2)), int(rng.choice([16384, 16384, 8, 0])), b))
        elif mode == 1:
            ids = [1, 6, 7, 0x33, 0x276, 8, 0x21]
            b = b"".join(K.vi(int(rng.choice(ids))) + K.vi(int(rng.choice([0, 1, 1, 2, 100, 4096, 1 << 33, (1 << 62) - 1])))
                         for _ in range(int(rng.integers(0, 6))))
            if rng.random() < 0.2:
                b = b[:int(rng.integers(0, len(b) + 1))]
            out.append((1, int(rng.integers(2)), 0, 0, b))
        elif mode == 2:
            b = (K.vi(int(rng.integers(0, 64))) if rng.random() < 0.7 else b"") + body
            out.append((2, int(rng.integers(2)), 0, 0, b))
        else:
            b = K.vi(int(rng.choice([0, 4, 63, 64, 1 << 20, 1 << 40]))) if rng.random() < 0.6 else body[:9]
            if rng.random() < 0.2:
                b += b"\x00"
            out.append((3, 0, 0, 0, b))
    return out


def corpus_probes():
    import h3frames_corpora as K
    import h3frames_model as M

    out = []
    for c in K.CASES:
        buf = c["buf"]
        for pos in frame_positions(buf):
            for is_client in (0, 1):
                for control in (0, 1):
                    out.append((0, is_client, control, c["mfps"], buf[pos:]))
            typ, p = M.quicint(buf, pos, len(buf))
            length, p = M.quicint(buf, p, len(buf)) if typ is not None else (None, pos)
            if length is not None and p + length <= len(buf):
                payload = buf[p:p + length]
                out += [(1, 0, 0, 0, payload), (1, 1, 0, 0, payload), (2, 0, 0, 0, payload), (2, 1, 0, 0, payload), (3, 0, 0, 0, payload)]
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("H2O_REF")
    if not ref:
        sys.exit("give the h2o tree as the argument or in $H2O_REF")
    srcs = [os.path.join(ref, "lib", "http3", "frame.c"), os.path.join(ref, "lib", "http3", "common.c"),
            os.path.join(ref, "deps", "picotls", "lib", "picotls.c")]
    if not all(os.path.exists(s) for s in srcs):
        sys.exit("no h2o tree at %s (lib/http3/frame.c, lib/http3/common.c, deps/picotls/lib/picotls.c)" % ref)
    probes = corpus_probes() + random_probes()
    inc = [os.path.join(ref, "include")] + [os.path.join(ref, "deps", d) for d in (
        "picotls/include", "quicly/include", "klib", "golombset", "cloexec", "yoml", "libgkc", "libyrmcds", "picohttpparser",
        "hiredis", "brotli/c/include")]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "dump_h3frames.c"), os.path.join(tmp, "dump_h3frames")
        with open(src, "w") as f:
            f.write(DUMP_C)
        subprocess.run(["gcc", "-O1", "-w", "-D_GNU_SOURCE", "-DH2O_USE_LIBUV=0", "-ffunction-sections", "-fdata-sections", src] + srcs +
                       ["-I" + d for d in inc] + ["-Wl,--gc-sections", "-lpthread", "-o", exe], check=True)
        feed = "".join("%d %d %d %d %s\n" % (m, a0, a1, a2, b.hex() or "-") for m, a0, a1, a2, b in probes)
        rows = subprocess.run([exe], input=feed, check=True, capture_output=True, text=True).stdout.split("\n")
    rows = [[int(x) for x in r.split()] for r in rows if r]
    assert len(rows) == len(probes) and all(len(r) == 6 for r in rows), len(rows)
    off = np.zeros(len(probes) + 1, np.uint32)
    off[1:] = np.cumsum([len(p[4]) for p in probes], dtype=np.uint64)
    np.savez_compressed(OUT, probes=np.frombuffer(b"".join(p[4] for p in probes), np.uint8).copy(), probe_off=off,
                        mode=np.array([p[0] for p in probes], np.uint8), arg=np.array([p[1:4] + (0,) for p in probes], np.uint32),
                        ret=np.array([r[0] for r in rows], np.int64), desc=np.array([r[1] for r in rows], np.uint8),
                        val=np.array([r[2:] for r in rows], np.uint64))
    print("%s: %d probes (%d read_frame, %d settings, %d priority update, %d goaway); %d bytes"
          % (os.path.relpath(OUT, ROOT), len(probes), *[sum(1 for p in probes if p[0] == m) for m in range(4)], os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
