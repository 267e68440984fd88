#!/usr/bin/env python3
"""Write tests/golden/h2data.npz: the DATA frames h2o's own h2o_http2_stream_send_pending_data (the static send_data,
calc_max_payload_size and commit_data_header behind it) queues for a list of cases, from the real reference.

    python tools/gen_h2data_fixture.py [REF]        REF: the h2o tree (default $H2O_REF or /root/reference)

The dump program below includes lib/http2/stream.c, so that it reaches the static functions, and links
lib/http2/frame.c and lib/common/memory.c (-ffunction-sections -Wl,--gc-sections) with stand-ins: a never-called
h2o_socket_do_prepare_for_latency_optimized_write (the socket's latency optimisation is in state DISABLED, its
suggested_write_size SIZE_MAX), a never-called h2o_conn_set_state (the stream stays in state SEND_BODY) and a send
vector whose read_ callback is a memcpy.  It is compiled in a temporary directory and removed with it; only the .npz
is written.  A case is one send record against one connection:
conn->_write.buf gets capacity - size = the room wanted, and h2o_http2_stream_send_pending_data is called until the
body is sent, a call sends nothing, or max_frames calls are made (an empty body: one call).  Data only:
  cases               i64 [n, 7]: m (peer_settings.max_frame_size), the room, conn->_write.window, the stream's
                      output_window, the body's length, flags (1 FINAL, 2 trailers), max_frames
  nframes             u32 [n]: the frames queued
  headers, frame_off  the frames' 9-byte headers back to back (u8 blob), u32 [n + 1]: case i's frames are
                      frame_off[i] .. frame_off[i + 1] - 1
  after               i64 [n, 2]: conn->_write.window and the stream's output_window afterwards
No payload bytes are recorded: the tests make bodies from a seed.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "h2data.npz")
RANDOM = 400

DUMP_C = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "h2o.h"
#include "h2o/http2.h"
#include "h2o/http2_internal.h"
#include STREAM_C

size_t h2o_socket_do_prepare_for_latency_optimized_write(h2o_socket_t *sock, const h2o_socket_latency_optimization_conditions_t *c)
{
    abort(); /* never called: the state is DISABLED */
}
void h2o_conn_set_state(h2o_conn_t *conn, h2o_conn_state_t state)
{
    abort(); /* never called: the stream's state is SEND_BODY, so that h2o_http2_stream_set_state is not reached */
}
int h2o_file_mktemp(const char *fn_template)
{
    return -1;
}
static int read_memcpy(h2o_sendvec_t *vec, void *dst, size_t len)
{
    memcpy(dst, vec->raw, len);
    vec->raw += len;
    vec->len -= len;
    return 1;
}
static const h2o_sendvec_callbacks_t callbacks = {read_memcpy, NULL};
static h2o_buffer_mmap_settings_t mmap_settings = {1u << 30, "/nonexistent/h2data.XXXXXX"};
static h2o_buffer_prototype_t prototype = {{4096}, &mmap_settings};

static h2o_globalconf_t globalconf;
static h2o_context_t ctx;
static h2o_socket_t sock;
static h2o_http2_conn_t conn;
static h2o_http2_stream_t stream;

/* "m room conn_window stream_window length flags max_frames" per input line -> "nframes conn_window stream_window headerhex" */
int main(void)
{
    long long m, room, wc, ws, len, flags, maxf;
    while (scanf("%lld %lld %lld %lld %lld %lld %lld", &m, &room, &wc, &ws, &len, &flags, &maxf) == 7) {
        size_t capacity = (size_t)room + 64, left = (size_t)len, calls = 0, nframes = 0, pos, k;
        h2o_buffer_t *buf = malloc(offsetof(h2o_buffer_t, _buf) + capacity);
        char *body = calloc(1, (size_t)len + 1);
        h2o_sendvec_t vec;
        memset(&conn, 0, sizeof(conn));
        memset(&stream, 0, sizeof(stream));
        ctx.globalconf = &globalconf;
        conn.super.ctx = &ctx;
        sock._latency_optimization.state = H2O_SOCKET_LATENCY_OPTIMIZATION_STATE_DISABLED;
        sock._latency_optimization.suggested_write_size = SIZE_MAX;
        conn.sock = &sock;
        conn.peer_settings = H2O_HTTP2_SETTINGS_DEFAULT;
        conn.peer_settings.max_frame_size = (uint32_t)m;
        conn._write.window._avail = (ssize_t)wc;
        buf->capacity = capacity, buf->size = 64, buf->bytes = buf->_buf, buf->_prototype = &prototype, buf->_fd = -1;
        conn._write.buf = buf;
        stream.stream_id = 1;
        stream.output_window._avail = (ssize_t)ws;
        stream.state = H2O_HTTP2_STREAM_STATE_SEND_BODY;
        stream.send_state = (flags & 1) ? H2O_SEND_STATE_FINAL : H2O_SEND_STATE_IN_PROGRESS;
        stream.req.res.trailers.size = (flags & 2) ? 1 : 0;
        stream._data.entries = &vec, stream._data.capacity = 1;
        vec.callbacks = &callbacks, vec.raw = body, vec.len = left;
        for (;;) {
            size_t before = conn._write.buf->size;
            stream._data.size = vec.len != 0;
            h2o_http2_stream_send_pending_data(&conn, &stream);
            ++calls;
            if (conn._write.buf != buf) {
                fprintf(stderr, "the buffer was reallocated\n");
                return 1;
            }
            if (buf->size != before)
                ++nframes;
            if (vec.len == 0 || (buf->size == before && vec.len == left) || (maxf != 0 && calls >= (size_t)maxf))
                break;
            left = vec.len;
        }
        printf("%zu %lld %lld ", nframes, (long long)conn._write.window._avail, (long long)stream.output_window._avail);
        for (pos = 64; pos < buf->size;) {
            size_t n = ((size_t)(uint8_t)buf->bytes[pos] << 16) | ((size_t)(uint8_t)buf->bytes[pos + 1] << 8) | (uint8_t)buf->bytes[pos + 2];
            for (k = 0; k != 9; ++k)
                printf("%02x", (uint8_t)buf->bytes[pos + k]);
            pos += 9 + n;
        }
        printf("-\n");
        free(buf);
        free(body);
    }
    return 0;
}
"""


def cases(seed=31):
    import h2data_corpora as K

    out = []
    for c in K.CASES:  # the corpus's first records, one connection each
        if c["status"] == 0 and c["sends"]:
            s = c["sends"][0]
            out.append((c["m"], c["room"], c["window"], s[3], s[1], s[4], s[5]))
    m = 16384
    for R in (0, 8, 9, 10, 11, m + 8, m + 9, m + 10, 2 * m + 18, 2 * m + 19, 1 << 18):  # every edge against every other
        for W in (-1, 0, 1, m - 1, m, m + 1, 1 << 18):
            for L in (0, 1, m - 1, m, m + 1, 2 * m):
                out.append((m, R, W, 1 << 18, L, 1, 0))
                out.append((m, R, 1 << 18, W, L, 1, 0))
    rng = np.random.default_rng(seed)
    edge = [-1, 0, 1, 8, 9, 10, m - 1, m, m + 1, 2 * m, 3 * m + 5, 65535, 1 << 18]
    for _ in range(RANDOM):
        mm = int(rng.choice([16384, 16384, 16385, 20000, 32768, 16777215]))
        pick = lambda: int(rng.choice(edge)) if rng.random() < 0.5 else int(rng.integers(0, 5 * m))  # noqa: E731
        out.append((mm, max(0, pick()), pick(), pick(), max(0, pick()), int(rng.integers(0, 4)), int(rng.choice([0, 0, 1, 2, 3]))))
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("H2O_REF", "/root/reference")
    stream_c = os.path.join(ref, "lib", "http2", "stream.c")
    frame_c = os.path.join(ref, "lib", "http2", "frame.c")
    memory_c = os.path.join(ref, "lib", "common", "memory.c")
    if not os.path.exists(stream_c):
        sys.exit("no h2o tree at %s (lib/http2/stream.c)" % ref)
    rows = cases()
    inc = [os.path.join(ref, "include")] + [os.path.join(ref, "deps", d) for d in (
        "picotls/include", "quicly/include", "klib", "golombset", "cloexec", "yoml", "libgkc", "libyrmcds", "picohttpparser",
        "hiredis", "brotli/c/include")]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "dump_h2data.c"), os.path.join(tmp, "dump_h2data")
        with open(src, "w") as f:
            f.write(DUMP_C)
        subprocess.run(["gcc", "-O1", "-w", "-DH2O_USE_LIBUV=0", "-ffunction-sections", "-fdata-sections", '-DSTREAM_C="%s"' % stream_c] +
                       ["-I" + d for d in inc] + [src, frame_c, memory_c, "-Wl,--gc-sections", "-lpthread", "-o", exe], check=True)
        feed = "".join("%d %d %d %d %d %d %d\n" % r for r in rows)
        lines = [r for r in subprocess.run([exe], input=feed, check=True, capture_output=True, text=True).stdout.split("\n") if r]
    assert len(lines) == len(rows), (len(lines), len(rows))
    nframes = np.array([int(r.split()[0]) for r in lines], np.uint32)
    after = np.array([[int(x) for x in r.split()[1:3]] for r in lines], np.int64)
    heads = [bytes.fromhex(r.split()[3].rstrip("-")) for r in lines]
    assert all(len(h) == 9 * int(k) for h, k in zip(heads, nframes))
    frame_off = np.zeros(len(rows) + 1, np.uint32)
    frame_off[1:] = np.cumsum(nframes, dtype=np.uint64)
    np.savez_compressed(OUT, cases=np.array(rows, np.int64), nframes=nframes, headers=np.frombuffer(b"".join(heads), np.uint8).copy(),
                        frame_off=frame_off, after=after)
    print("%s: %d cases, %d frames; %d bytes" % (os.path.relpath(OUT, ROOT), len(rows), int(nframes.sum()), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
