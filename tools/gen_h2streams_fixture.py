#!/usr/bin/env python3
"""Write tests/golden/h2streams.npz: what h2o's own server-side frame handlers (the static functions of
lib/http2/connection.c, reached by including the file) do with the connections of tests/h2streams_corpora.py.

    python tools/gen_h2streams_fixture.py [REF]        REF: the h2o tree (default $H2O_REF or /root/reference)

The dump program includes lib/http2/connection.c and links frame.c, scheduler.c, memory.c and token.c, with stand-ins of
its own for stream.c (h2o_http2_stream_open / _close / _reset over the real hash and counters), for
h2o_hpack_parse_request (scripted per block: return value, exists map, content-length, method, path) and for the request
layer (h2o_process_request, h2o_send_error_*, timers, the socket), which do nothing.  It feeds a case's frames one by one
to conn->_read_expect and records per frame h2o's return value and err_desc, per step the bytes appended to
conn->_write.buf, and behind the last step max_open of both kinds, num_streams.pull.open and .priority.open and every
live stream's id, state, req_body.state, windows, bytes_unnotified, bytes received and content-length.  The ops and the
send side's bookings of a case are done with h2o's own functions (h2o_http2_stream_close, update_stream_input_window,
h2o_http2_stream_open + h2o_http2_stream_prepare_for_request, h2o_http2_window_consume_window).

Cases that h2o's handlers cannot be put through are left out and listed in `skipped`: a reply capacity, a control
failure in front, a full table (all this library's own), ops the call refuses, HHUFF_H2SP_STREAM_BODIES (the request
layer's side of a streamed body), trailers that h2o_hpack_parse_request itself refuses (it is scripted), and control
replies a 16 MB connection window does not produce.

The file holds data only:
  names, skipped      the cases in, and left out
  frame_first         [ncase + 1] into ret / desc
  ret, desc           per frame fed (up to and with the failing one, all steps): h2o's return value (0, or the error) and
                      *err_desc as its index in tests/h2streams_model.py ERR_TEXT (0 NULL, 99 any other text)
  out, out_off        the bytes appended to conn->_write.buf during the LAST step of each case
  counters            [ncase, 4]
  streams, stream_first   [nstream, 8] int64 rows (id, state, req_body.state, output_window, input_window, bytes_unnotified,
                      bytes received, content-length (-1: none)), case c's rows stream_first[c] .. stream_first[c + 1]
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "h2streams.npz")

DUMP_C = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "h2o.h"
#include "h2o/http2.h"
#include "h2o/http2_internal.h"
#include CONNECTION_C

/* ---- stand-ins: stream.c over the real hash and counters */
h2o_http2_stream_t *h2o_http2_stream_open(h2o_http2_conn_t *conn, uint32_t stream_id, h2o_req_t *src_req,
                                          const h2o_http2_priority_t *received_priority)
{
    h2o_http2_stream_t *s = calloc(1, sizeof(*s));
    s->stream_id = stream_id;
    s->state = H2O_HTTP2_STREAM_STATE_IDLE;
    h2o_http2_window_init(&s->output_window, conn->peer_settings.initial_window_size);
    h2o_http2_window_init(&s->input_window.window, H2O_HTTP2_SETTINGS_HOST_STREAM_INITIAL_WINDOW_SIZE);
    s->received_priority = *received_priority;
    h2o_mem_init_pool(&s->req.pool);
    s->req.conn = &conn->super;
    s->req.content_length = SIZE_MAX;
    s->req.version = 0x200;
    h2o_http2_conn_register_stream(conn, s);
    ++conn->num_streams.priority.open;
    s->_num_streams_slot = &conn->num_streams.priority;
    return s;
}
void h2o_http2_stream_close(h2o_http2_conn_t *conn, h2o_http2_stream_t *s)
{
    h2o_http2_conn_unregister_stream(conn, s);
    if (s->req_body.buf != NULL)
        h2o_buffer_dispose(&s->req_body.buf);
    h2o_mem_clear_pool(&s->req.pool);
    free(s);
}
void h2o_http2_stream_reset(h2o_http2_conn_t *conn, h2o_http2_stream_t *s)
{
    if (s->state >= H2O_HTTP2_STREAM_STATE_SEND_HEADERS && s->state != H2O_HTTP2_STREAM_STATE_END_STREAM)
        h2o_http2_stream_set_state(conn, s, H2O_HTTP2_STREAM_STATE_END_STREAM);
    if (s->state == H2O_HTTP2_STREAM_STATE_END_STREAM && h2o_linklist_is_linked(&s->_link))
        return; /* h2o closes it when the write completes */
    h2o_http2_stream_close(conn, s);
}

/* ---- h2o_hpack_parse_request, scripted */
static struct {
    int ret, exists;
    long long cl;
    char method[32], path[32];
    int has_method, has_path;
} script[64];
static int script_n, script_at;
int h2o_hpack_parse_request(h2o_mem_pool_t *pool, h2o_hpack_decode_header_cb decode_cb, void *decode_ctx, h2o_iovec_t *method,
                            const h2o_url_scheme_t **scheme, h2o_iovec_t *authority, h2o_iovec_t *path, h2o_iovec_t *protocol,
                            h2o_headers_t *headers, int *pseudo_header_exists_map, size_t *content_length, h2o_iovec_t *expect,
                            h2o_cache_digests_t **digests, h2o_iovec_t *datagram_flow_id, const uint8_t *src, size_t len,
                            const char **err_desc)
{
    if (script_at >= script_n)
        abort();
    *content_length = script[script_at].cl < 0 ? SIZE_MAX : (size_t)script[script_at].cl;
    if (pseudo_header_exists_map != NULL)
        *pseudo_header_exists_map = script[script_at].exists;
    if (method != NULL && script[script_at].has_method)
        *method = h2o_iovec_init(script[script_at].method, strlen(script[script_at].method));
    if (path != NULL && script[script_at].has_path)
        *path = h2o_iovec_init(script[script_at].path, strlen(script[script_at].path));
    if (script[script_at].ret != 0)
        *err_desc = "scripted";
    return script[script_at++].ret;
}

/* ---- the request layer, the socket, timers, logging: nothing happens */
static h2o_handler_t handler;
h2o_handler_t *h2o_get_first_handler(h2o_req_t *req) { return &handler; }
void h2o_process_request(h2o_req_t *req) {}
void h2o_send_error_generic(h2o_req_t *req, int status, const char *reason, const char *body, int flags) {}
void h2o_send_informational(h2o_req_t *req) {}
ssize_t h2o_add_header(h2o_mem_pool_t *pool, h2o_headers_t *headers, const h2o_token_t *token, const char *orig_name,
                       const char *value, size_t value_len) { return 0; }
void h2o_conn_set_state(h2o_conn_t *conn, h2o_conn_state_t state) {}
void h2o_destroy_connection(h2o_conn_t *conn) { abort(); }
void h2o_cache_destroy(h2o_cache_t *cache) { abort(); }
void h2o_http2_casper_destroy(h2o_http2_casper_t *casper) { abort(); }
void h2o_socket_close(h2o_socket_t *sock) { abort(); }
void h2o_socket_read_stop(h2o_socket_t *sock) { abort(); }
int h2o_socket_ssl_is_early_data(h2o_socket_t *sock) { return 0; }
size_t h2o_socket_do_prepare_for_latency_optimized_write(h2o_socket_t *sock, const h2o_socket_latency_optimization_conditions_t *c) { abort(); }
const char h2o_httpclient_error_is_eos[] = "end of stream";
int h2o_file_mktemp(const char *fn_template) { return -1; }
void h2o_hpack_dispose_header_table(h2o_hpack_header_table_t *t) {}
int h2o_hpack_decode_header(h2o_mem_pool_t *pool, void *ctx, h2o_iovec_t **name, h2o_iovec_t *value, const uint8_t **const src,
                            const uint8_t *src_end, const char **err_desc) { abort(); }
void h2o_timerwheel_link_abs(h2o_timerwheel_t *ctx, h2o_timerwheel_entry_t *entry, uint64_t at) {}
int h2o__lcstris_core(const char *target, const char *test, size_t test_len)
{
    size_t i;
    for (i = 0; i != test_len; ++i)
        if ((target[i] | 0x20) != (test[i] | 0x20))
            return 0;
    return 1;
}
__typeof__(ptls_log) ptls_log;
void ptls_log__recalc_point(int caller_locked, struct st_ptls_log_point_t *point) {}
void ptls_log__recalc_conn(int caller_locked, struct st_ptls_log_conn_state_t *conn, ptls_log_getsni_t getsni) {}
void ptls_log__do_push_element_unsafestr(const char *prefix, size_t prefix_len, const char *s, size_t l) {}
void ptls_log__do_push_element_signed32(const char *prefix, size_t prefix_len, int32_t v) {}
void ptls_log__do_push_element_unsigned64(const char *prefix, size_t prefix_len, uint64_t v) {}
void ptls_log__do_write_start(struct st_ptls_log_point_t *point, int add_time) {}
int ptls_log__do_write_end(struct st_ptls_log_point_t *point, struct st_ptls_log_conn_state_t *conn, ptls_log_getsni_t getsni,
                           int includes_appdata) { return 0; }
const h2o_url_scheme_t H2O_URL_SCHEME_HTTP = {{H2O_STRLIT("http")}, 80, 0};
const h2o_url_scheme_t H2O_URL_SCHEME_HTTPS = {{H2O_STRLIT("https")}, 443, 1};
static h2o_buffer_mmap_settings_t mmap_settings = {1u << 30, "/nonexistent/h2streams.XXXXXX"};
h2o_buffer_prototype_t h2o_socket_buffer_prototype = {{4096}, &mmap_settings};

static h2o_globalconf_t globalconf;
static h2o_context_t ctx;
static h2o_evloop_t loop;
static h2o_socket_t sock;
static h2o_http2_conn_t *conn;

static void new_conn(unsigned max_streams, unsigned max_prio, unsigned active, unsigned long long entity, unsigned iws)
{
    memset(&globalconf, 0, sizeof(globalconf));
    globalconf.http2.max_streams = max_streams;
    globalconf.http2.max_streams_for_priority = max_prio;
    globalconf.http2.active_stream_window_size = active;
    globalconf.http2.max_concurrent_requests_per_connection = 100000;
    globalconf.http2.max_concurrent_streaming_requests_per_connection = 100000;
    globalconf.max_request_entity_size = entity;
    memset(&ctx, 0, sizeof(ctx));
    ctx.globalconf = &globalconf;
    ctx.loop = &loop;
    conn = calloc(1, sizeof(*conn)); /* (the previous one is left alone) */
    conn->super.ctx = &ctx;
    sock._latency_optimization.state = H2O_SOCKET_LATENCY_OPTIMIZATION_STATE_DISABLED;
    sock._latency_optimization.suggested_write_size = SIZE_MAX;
    conn->sock = &sock;
    conn->peer_settings = H2O_HTTP2_SETTINGS_DEFAULT;
    conn->peer_settings.initial_window_size = iws;
    conn->streams = kh_init(h2o_http2_stream_t);
    h2o_http2_scheduler_init(&conn->scheduler);
    conn->state = H2O_HTTP2_CONN_STATE_OPEN;
    conn->_read_expect = expect_default;
    h2o_buffer_init(&conn->_write.buf, &h2o_socket_buffer_prototype);
    h2o_linklist_init_anchor(&conn->_pending_reqs);
    h2o_linklist_init_anchor(&conn->_write.streams_to_proceed);
    h2o_http2_window_init(&conn->_write.window, 65535);
    h2o_http2_window_init(&conn->_input_window, H2O_HTTP2_SETTINGS_HOST_CONNECTION_WINDOW_SIZE);
    conn->dos_mitigation.reset_budget = 100000;
}

static const char *texts[] = {NULL, "invalid stream id in HEADERS frame", "closed stream id in HEADERS frame",
                              "trailer cannot be used in a CONNECT request", "trailing HEADERS frame MUST have END_STREAM flag set",
                              "stream cannot depend on itself", "unexpected stream id in CONTINUATION frame", "invalid DATA frame",
                              "too many streams in idle/closed state", "unexpected stream id in RST_STREAM frame",
                              "invalid stream id in WINDOW_UPDATE frame"};

static int cmp_u32(const void *a, const void *b) { return *(const uint32_t *)a < *(const uint32_t *)b ? -1 : 1; }

int main(void)
{
    char tag;
    static char hex[1 << 18];
    static uint8_t bytes[1 << 17];
    size_t step_base = 0;
    while (scanf(" %c", &tag) == 1) {
        if (tag == 'N') {
            unsigned a, b, c, e;
            unsigned long long d;
            if (scanf("%u %u %u %llu %u", &a, &b, &c, &d, &e) != 5) return 2;
            new_conn(a, b, c, d, e);
            script_n = script_at = 0;
        } else if (tag == 'S') { /* a step begins: its blocks' scripts follow as P lines */
            script_n = script_at = 0;
            step_base = conn->_write.buf->size;
        } else if (tag == 'P') {
            char m[64], p[64];
            if (scanf("%d %d %lld %63s %63s", &script[script_n].ret, &script[script_n].exists, &script[script_n].cl, m, p) != 5) return 2;
            script[script_n].has_method = strcmp(m, "~") != 0, script[script_n].has_path = strcmp(p, "~") != 0;
            strcpy(script[script_n].method, script[script_n].has_method ? m : "");
            strcpy(script[script_n].path, script[script_n].has_path ? p : "");
            ++script_n;
        } else if (tag == 'F') {
            size_t n = 0, i;
            const char *err_desc = NULL;
            ssize_t r;
            int d = 0;
            if (scanf("%262143s", hex) != 1) return 2;
            for (; hex[2 * n] && hex[2 * n + 1]; ++n) {
                unsigned x;
                sscanf(hex + 2 * n, "%2x", &x);
                bytes[n] = (uint8_t)x;
            }
            r = conn->_read_expect(conn, bytes, n, &err_desc);
            if (r >= 0 && (size_t)r != n) return 3;
            if (err_desc != NULL) {
                d = 99;
                for (i = 1; i != sizeof(texts) / sizeof(texts[0]); ++i)
                    if (strcmp(err_desc, texts[i]) == 0)
                        d = (int)i;
            }
            printf("F %d %d\n", r >= 0 ? 0 : (int)r, r >= 0 ? 0 : d);
        } else if (tag == 'O' || tag == 'T') {
            unsigned sid, op, arg;
            h2o_http2_stream_t *s;
            if (scanf("%u %u %u", &sid, &op, &arg) != 3) return 2;
            s = h2o_http2_conn_get_stream(conn, sid);
            if (tag == 'T') {
                h2o_http2_window_consume_window(&s->output_window, arg);
            } else if (op == 1) {
                h2o_http2_stream_close(conn, s);
            } else if (op == 2) {
                update_stream_input_window(conn, s, arg);
            } else {
                s = h2o_http2_stream_open(conn, sid, NULL, &h2o_http2_default_priority);
                h2o_http2_scheduler_open(&s->_scheduler, &conn->scheduler, 16, 0);
                h2o_http2_stream_prepare_for_request(conn, s);
                h2o_http2_stream_set_state(conn, s, H2O_HTTP2_STREAM_STATE_REQ_PENDING);
                h2o_http2_stream_set_state(conn, s, H2O_HTTP2_STREAM_STATE_SEND_HEADERS);
            }
        } else if (tag == 'E') { /* the case ends: the last step's bytes and the state */
            uint32_t ids[1024], n = 0, i;
            size_t k;
            h2o_http2_stream_t *s;
            printf("E ");
            for (k = step_base; k < conn->_write.buf->size; ++k)
                printf("%02x", (uint8_t)conn->_write.buf->bytes[k]);
            printf("- %u %u %zu %zu", conn->pull_stream_ids.max_open, conn->push_stream_ids.max_open, conn->num_streams.pull.open,
                   conn->num_streams.priority.open);
            kh_foreach_value(conn->streams, s, { ids[n++] = s->stream_id; });
            qsort(ids, n, sizeof(ids[0]), cmp_u32);
            printf(" %u", n);
            for (i = 0; i != n; ++i) {
                s = h2o_http2_conn_get_stream(conn, ids[i]);
                printf(" %u %d %d %lld %lld %zu %zu %lld", s->stream_id, (int)s->state, (int)s->req_body.state,
                       (long long)h2o_http2_window_get_avail(&s->output_window),
                       (long long)h2o_http2_window_get_avail(&s->input_window.window), s->input_window.bytes_unnotified,
                       s->req.req_body_bytes_received, s->req.content_length == SIZE_MAX ? -1ll : (long long)s->req.content_length);
            }
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
"""


def wire(f, blk, first, iws_now):
    """one corpus frame as wire bytes (the header block's bytes are arbitrary: the parser is scripted)"""
    import h2streams_model as M

    t, sid = f["type"], f["stream_id"]
    if t == M.HEADERS:
        prio = blk["flags"] & M.B_SELF_DEPENDENCY
        pay = (M.be32(sid) + b"\x0f" if prio else b"") + b"\x82" * (f["length"] - (5 if prio else 0))
        return M.frame_bytes(t, f["flags"] | (0x20 if prio else 0), sid, pay)
    if t == M.CONTINUATION:
        return M.frame_bytes(t, f["flags"], sid, b"\x82" * f["length"])
    if t == M.DATA:
        n = f["ctl"][1]
        pad = f["length"] - n
        return M.frame_bytes(t, f["flags"], sid, (bytes([pad - 1]) if pad else b"") + b"d" * n + b"\0" * max(0, pad - 1))
    if t == M.PRIORITY:
        return M.frame_bytes(t, 0, sid, M.be32(0) + b"\x0f")
    if t == M.RST_STREAM:
        return M.frame_bytes(t, 0, sid, M.be32(8))
    if t == M.WINDOW_UPDATE:
        return M.frame_bytes(t, 0, sid, M.be32(f["ctl"][0]))
    if t == M.SETTINGS:
        return M.frame_bytes(t, 0, 0, b"\x00\x04" + M.be32(iws_now))
    if t == M.GOAWAY:
        return M.frame_bytes(t, 0, 0, M.be32(0) + M.be32(0))
    if t == M.PING:
        return M.frame_bytes(t, 0, 0, b"\0\0\0\1\0\0\0\2")
    raise ValueError(t)


def realizable(c):
    import h2streams_model as M

    if c["P"]["flags"] & M.STREAM_BODIES or c["status"] in (M.SPACE, M.EFULL):
        return False
    for st in c["steps"]:
        if st.rep_cap is not None or st.nctl is not None:
            return False
        if any(f["ctl_reply"] and f["type"] == M.DATA for f in st.frames):
            return False
    if c["err"] in (M.E_TRAILERS_PSEUDO_HEADER, M.E_TRAILERS_HOST):  # the parser's own verdicts: it is scripted here
        return False
    return all(e[1] == 0 for e in c["op_events"])


def feed_of(c):
    import h2streams_model as M

    P = c["P"]
    deltas = lambda st: sum((f["ctl"][1] - (1 << 32) if f["ctl"][1] & 0x80000000 else f["ctl"][1])  # noqa: E731
                            for f in st.frames if f["type"] == M.SETTINGS and f["ctl"][2] & M.R_WINDOW_DELTA)
    out = ["N %d %d %d %d %d" % (P["max_streams"], P["max_streams_for_priority"], P["active_stream_window_size"],
                                  P["max_request_entity_size"], c["iws"][0] - deltas(c["steps"][0]))]
    nfed = 0
    for k, (st, iws) in enumerate(zip(c["steps"], c["iws"])):
        out.append("S")
        for b in st.blocks:
            out.append("P %d %d %d %s %s" % (b["bstatus"], b["exists_map"], -1 if b["content_length"] == M.NO_LENGTH else b["content_length"],
                                             "~" if b["method"] is None else b["method"].decode(), "~" if b["path"] is None else b["path"].decode()))
        out += ["T %d 0 %d" % t for t in st.sends] + ["O %d %d %d" % op for op in st.ops]
        now = iws - deltas(st)
        last = k == len(c["steps"]) - 1
        frames = st.frames[:c["nstr"] + (1 if c["status"] != 0 else 0)] if last else st.frames
        for i, f in enumerate(frames):
            if f["type"] == M.SETTINGS and f["ctl"][2] & M.R_WINDOW_DELTA:
                d = f["ctl"][1]
                now += d - (1 << 32) if d & 0x80000000 else d
            blk = st.blocks[f["block"]] if f["block"] is not None else None
            out.append("F " + wire(f, blk, blk is not None and i == blk["first_frame"], now).hex())
            nfed += 1
    out.append("E")
    return "\n".join(out) + "\n", nfed


def main():
    import h2streams_corpora as K

    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("H2O_REF", "/root/reference")
    src_c = lambda *p: os.path.join(ref, "lib", *p)  # noqa: E731
    if not os.path.exists(src_c("http2", "connection.c")):
        sys.exit("no h2o tree at %s (lib/http2/connection.c)" % ref)
    cases = [c for c in K.CASES if realizable(c)]
    skipped = [c["name"] for c in K.CASES if not realizable(c)]
    feeds = [feed_of(c) for c in cases]
    inc = [os.path.join(ref, "include")] + [os.path.join(ref, "deps", d) for d in (
        "picotls/include", "quicly/include", "klib", "golombset", "cloexec", "yoml", "libgkc", "libyrmcds", "picohttpparser",
        "hiredis", "brotli/c/include")]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "dump_h2streams.c"), os.path.join(tmp, "dump_h2streams")
        with open(src, "w") as f:
            f.write(DUMP_C)
        subprocess.run(["gcc", "-O1", "-w", "-DH2O_USE_LIBUV=0", "-ffunction-sections", "-fdata-sections",
                        '-DCONNECTION_C="%s"' % src_c("http2", "connection.c")] + ["-I" + d for d in inc] +
                       [src, src_c("http2", "frame.c"), src_c("http2", "scheduler.c"), src_c("common", "memory.c"), src_c("common", "token.c"),
                        "-Wl,--gc-sections", "-lpthread", "-o", exe], check=True)
        res = subprocess.run([exe], input="".join(f for f, _ in feeds), capture_output=True, text=True)
        if res.returncode != 0:
            sys.exit("the dump program failed (%d): %s" % (res.returncode, res.stderr[-2000:]))
        lines = [r for r in res.stdout.split("\n") if r]
    ret, desc, first, outs, counters, streams, sfirst = [], [], [0], [], [], [], [0]
    it = iter(lines)
    for (_, nfed), c in zip(feeds, cases):
        for _ in range(nfed):
            w = next(it).split()
            assert w[0] == "F", w
            ret.append(int(w[1]))
            desc.append(int(w[2]))
        w = next(it).split()
        assert w[0] == "E", (c["name"], w)
        outs.append(bytes.fromhex(w[1].rstrip("-")))
        counters.append([int(x) for x in w[2:6]])
        n = int(w[6])
        rows = np.array([int(x) for x in w[7:7 + 8 * n]], np.int64).reshape(n, 8)
        streams.append(rows)
        first.append(len(ret))
        sfirst.append(sfirst[-1] + n)
    out_off = np.concatenate([[0], np.cumsum([len(o) for o in outs])]).astype(np.uint32)
    np.savez_compressed(OUT, names=np.array([c["name"] for c in cases]), skipped=np.array(skipped), frame_first=np.array(first, np.uint32),
                        ret=np.array(ret, np.int32), desc=np.array(desc, np.uint8), out=np.frombuffer(b"".join(outs), np.uint8).copy(),
                        out_off=out_off, counters=np.array(counters, np.int64), streams=np.concatenate(streams + [np.zeros((0, 8), np.int64)]),
                        stream_first=np.array(sfirst, np.uint32))
    print("%s: %d cases (%d left out), %d frames; %d bytes" % (os.path.relpath(OUT, ROOT), len(cases), len(skipped), len(ret),
                                                            os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
