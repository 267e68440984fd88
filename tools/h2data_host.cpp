// The DATA framer's arithmetic (h2o_amd/csrc/hhuff_h2data.h: the code the kernel runs) on the host, as a stand-alone
// program to build with -fsanitize=address,undefined and run directly:
//     h2data_host CASES MUTATIONS
// 1. The closed form of a record (h2d::record) against a loop that makes one call of h2o's
//    h2o_http2_stream_send_pending_data after the other (lib/http2/stream.c:107-184, 410-436), exhaustively for m in
//    1..5 and R, W_c, W_s, L in -2..40 (an L below 0 is an empty body): every frame's length and flags, the stop
//    reason, with FINAL and TRAILERS in all four combinations without max_frames and FINAL with max_frames 1, 2, 3.
// 2. CASES: one line a connection, as tests/test_h2data_host.py writes them from tests/h2data_corpora.py --
//        m window room status out_len after   nsend x (body_off body_len stream_id window flags max_frames)
//        nsent x (sent nframes out_off flags window)   nframes x (stream_id length flags)
//    walked by h2d::walk with the region and the body in heap blocks of exactly their sizes, the frames written from
//    the walk's jobs; the outcome must be the expected one, byte by byte.
// 3. MUTATIONS times a seeded connection of hostile records, peers and rooms: whatever they hold, the jobs stay inside
//    the region and the body (the copies run, under AddressSanitizer), the bytes written are out_len, and the records
//    agree with the frame-by-frame loop.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hhuff_h2data.h"

using namespace hhuff;

static void fail(const char* what, long a, long b, long c) {
    printf("FAIL: %s (%ld, %ld, %ld)\n", what, a, b, c);
    exit(1);
}

struct Frame {
    int64_t length;
    uint32_t flags;
};

// one call of send_pending_data after the other: -> the stop reason | END_STREAM; the frames into v
static uint32_t loop(int64_t m, int64_t R, int64_t Wc, int64_t Ws, int64_t L, bool final, bool trailers, int64_t max_frames,
                     std::vector<Frame>& v) {
    v.clear();
    if (L < 0) L = 0;
    uint32_t es = 0;
    for (int64_t calls = 0;;) {
        if (Ws <= 0) return HHUFF_H2T_STREAM_WINDOW | es;  // h2o_http2_stream_send_pending_data
        int64_t ret = R;                                     // h2o_http2_conn_get_buffer_window
        if (ret < 9) return HHUFF_H2T_ROOM | es;
        ret -= 9;
        if (ret <= 0) return HHUFF_H2T_ROOM | es;
        if (Wc < ret) ret = Wc;
        if (ret <= 0) return HHUFF_H2T_CONN_WINDOW | es;  // calc_max_payload_size
        int64_t max_payload = ret < Ws ? ret : Ws;
        if (m < max_payload) max_payload = m;
        const int64_t fill = max_payload < L ? max_payload : L;  // send_data
        L -= fill;
        if (fill != 0 || final) {
            const bool is_end_stream = final && L == 0 && !trailers;  // commit_data_header
            if (fill != 0 || is_end_stream) {
                v.push_back(Frame{fill, is_end_stream ? 1u : 0u});
                if (is_end_stream) es = HHUFF_H2T_END_STREAM;
                Wc -= fill, Ws -= fill, R -= fill + 9;
            }
        }
        ++calls;
        if (L == 0) return HHUFF_H2T_DONE | es;
        if (max_frames != 0 && calls >= max_frames) return HHUFF_H2T_MAX_FRAMES | es;
    }
}

static void frames_of(const h2d::Frames& F, int64_t m, std::vector<Frame>& v) {
    v.clear();
    for (int64_t i = 0; i < F.full; ++i) v.push_back(Frame{m, 0u});
    if (F.tail > 0 || F.empty) v.push_back(Frame{F.tail, 0u});
    if ((F.flags & HHUFF_H2T_END_STREAM) && !v.empty()) v.back().flags = 1u;
}

static uint64_t exhaustive() {
    std::vector<Frame> a, b;
    uint64_t n = 0;
    const int variants[7][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {1, 1, 0}, {1, 0, 1}, {1, 0, 2}, {1, 0, 3}};
    for (int64_t m = 1; m <= 5; ++m)
        for (int64_t R = -2; R <= 40; ++R)
            for (int64_t Wc = -2; Wc <= 40; ++Wc)
                for (int64_t Ws = -2; Ws <= 40; ++Ws)
                    for (int64_t L = -2; L <= 40; ++L)
                        for (const auto& var : variants) {
                            const uint32_t why = loop(m, R, Wc, Ws, L, var[0], var[1], var[2], a);
                            const h2d::Frames F = h2d::record(m, R, Wc, Ws, L, var[0], var[1], var[2]);
                            frames_of(F, m, b);
                            bool same = why == F.flags && a.size() == b.size();
                            for (size_t i = 0; same && i < a.size(); ++i) same = a[i].length == b[i].length && a[i].flags == b[i].flags;
                            if (!same) {
                                printf("m %ld R %ld Wc %ld Ws %ld L %ld final %d trailers %d max_frames %d: loop %u / %zu frames, closed %u / %zu\n",
                                       (long)m, (long)R, (long)Wc, (long)Ws, (long)L, var[0], var[1], var[2], why, a.size(), F.flags, b.size());
                                exit(1);
                            }
                            ++n;
                        }
    return n;
}

static std::vector<uint8_t> corpus_body() {  // tests/h2data_corpora.py BODY
    std::vector<uint8_t> b(72000);
    for (size_t i = 0; i < b.size(); ++i) b[i] = (uint8_t)(i * 131 + (i >> 8) + 7);
    return b;
}

// The walk's records and, from its jobs, the frames: into a region of exactly `room` bytes on the heap.
struct WriteSink {
    const uint8_t* body;
    uint64_t body_size;
    uint8_t* region;
    uint32_t start, room;
    std::vector<hhuff_h2_sent_t> sent;
    uint64_t written = 0;
    void record(uint32_t i, const hhuff_h2_sent_t& T, const h2d::Job& J) {
        if (i != sent.size()) fail("records out of order", i, (long)sent.size(), 0);
        sent.push_back(T);
        if (T.nframes == 0) {
            if (T.sent != 0) fail("bytes without a frame", i, T.sent, 0);
            return;
        }
        if (J.nframes != T.nframes || J.total != T.sent || J.dst != T.out_off) fail("job and record differ", i, J.total, T.sent);
        if (J.dst != start + written) fail("a job does not follow its predecessor", i, J.dst, (long)(start + written));
        if (J.out_bytes() > room - written) fail("a job leaves the region", i, (long)J.out_bytes(), (long)(room - written));
        if ((uint64_t)J.src + J.total > body_size) fail("a job leaves the body", i, J.src, J.total);
        // the frames as the copy kernel writes them: 256 lanes, each every 256th line of the job, by the kernel's own
        // line code (the region stands at out[start] of an `out` that is 16-byte aligned)
        const uint64_t out_addr = (uint64_t)(uintptr_t)region - start;
        const uint64_t d0 = out_addr + J.dst, d1 = d0 + J.out_bytes(), nlines = ((d1 + 15u) >> 4) - (d0 >> 4);
        for (uint64_t lane = 0; lane < 256 && lane < nlines; ++lane) {
            h2d::At at{0u, 0};
            for (uint64_t li = lane; li < nlines; li += 256) {
                const uint64_t line = (d0 & ~15ull) + 16u * li;
                if (li == lane)
                    at = h2d::locate(J, (int64_t)(line - d0));
                else
                    h2d::advance(J, at, 16u * 256u);
                h2d::write_line((uint64_t)(uintptr_t)body, J, d0, d1, line, at);
            }
        }
        // ... and frame by frame
        std::vector<uint8_t> plain;
        for (uint32_t g = 0; g < J.nframes; ++g) {
            const uint32_t len = g + 1u < J.nframes ? J.m : J.total - g * J.m;
            if (len > J.m) fail("a frame above m", i, len, J.m);
            uint8_t h[9];
            h2d::header(h, len, (g + 1u == J.nframes && J.end_stream) ? 1u : 0u, J.stream_id);
            plain.insert(plain.end(), h, h + 9);
            plain.insert(plain.end(), body + J.src + (uint64_t)g * J.m, body + J.src + (uint64_t)g * J.m + len);
        }
        if (plain.size() != J.out_bytes() || memcmp(plain.data(), region + written, plain.size()) != 0)
            fail("the line code's bytes differ from the frames'", i, J.total, J.m);
        written += J.out_bytes();
    }
};

// A region of `room` bytes whose address is `start` modulo 16, ending exactly at its block's end; the up to 15 bytes
// in front of it hold 0xEE, as the region does.
struct Region {
    uint8_t* block;
    uint8_t* bytes;
    uint32_t pad, room;
    Region(uint32_t start, uint32_t room_) : pad(start & 15u), room(room_) {
        block = (uint8_t*)malloc((size_t)pad + room + (pad + room == 0));
        memset(block, 0xEE, (size_t)pad + room);
        bytes = block + pad;
    }
    void check_front() const {
        for (uint32_t i = 0; i < pad; ++i)
            if (block[i] != 0xEE) fail("a byte in front of the region", i, 0, 0);
    }
    ~Region() { free(block); }
};

static long num(char*& p) {
    char* e;
    const long v = strtol(p, &e, 10);
    if (e == p) fail("a number is missing", 0, 0, 0);
    p = e;
    return v;
}

static size_t run_cases(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) fail("cannot open the cases", 0, 0, 0);
    const std::vector<uint8_t> body = corpus_body();
    std::vector<char> line(1 << 16);
    size_t n = 0;
    while (fgets(line.data(), (int)line.size(), f)) {
        char* p = line.data();
        const int64_t m = num(p), window = num(p);
        const uint32_t room = (uint32_t)num(p);
        const int32_t status = (int32_t)num(p);
        const uint32_t out_len = (uint32_t)num(p);
        const int64_t after = num(p);
        std::vector<hhuff_h2_send_t> sends((size_t)num(p));
        for (auto& s : sends) {
            s.body_off = (uint32_t)num(p), s.body_len = (uint32_t)num(p), s.stream_id = (uint32_t)num(p), s.window = (int32_t)num(p);
            s.flags = (uint32_t)num(p), s.max_frames = (uint32_t)num(p);
        }
        std::vector<hhuff_h2_sent_t> want((size_t)num(p));
        for (auto& t : want) {
            t.sent = (uint32_t)num(p), t.nframes = (uint32_t)num(p), t.out_off = (uint32_t)num(p), t.flags = (uint32_t)num(p);
            t.window = (int32_t)num(p), t.rsv = 0;
        }
        std::vector<uint8_t> bytes;
        const size_t nfr = (size_t)num(p);
        size_t rec = 0, taken = 0, used = 0;  // record rec has the next want[rec].nframes frames; their payloads are its bytes
        for (size_t i = 0; i < nfr; ++i) {
            const uint32_t sid = (uint32_t)num(p), len = (uint32_t)num(p), fl = (uint32_t)num(p);
            while (rec < want.size() && taken == want[rec].nframes) ++rec, taken = 0, used = 0;
            if (rec >= want.size()) fail("the case's frames outnumber its records'", (long)n, (long)i, 0);
            uint8_t h[9];
            h2d::header(h, len, fl, sid);
            bytes.insert(bytes.end(), h, h + 9);
            const uint8_t* src = body.data() + sends[rec].body_off + used;
            bytes.insert(bytes.end(), src, src + len);
            used += len, ++taken;
        }
        const uint32_t start = 1000 + (uint32_t)(n % 16);  // (every alignment of the region over the cases)
        Region reg(start, room);
        uint8_t* region = reg.bytes;
        WriteSink sink{body.data(), body.size(), region, start, room};
        h2d::Result R;
        const hhuff_h2_peer_t P{4096u, 1u, 0xFFFFFFFFu, 65535u, (uint32_t)m, 0u, window, 65535};
        h2d::walk(body.size(), sends.data(), (uint32_t)sends.size(), m, h2d::peer_ok(P), window, start, room, sink, R);
        if (R.status != status) fail("status", (long)n, R.status, status);
        if (R.out_len != out_len || sink.written != out_len) fail("out_len", (long)n, R.out_len, out_len);
        if (R.send_window != after) fail("the connection's window", (long)n, (long)R.send_window, (long)after);
        if (sink.sent.size() != want.size()) fail("records served", (long)n, (long)sink.sent.size(), (long)want.size());
        for (size_t i = 0; i < want.size(); ++i) {
            hhuff_h2_sent_t w = want[i];
            w.out_off += start;
            if (memcmp(&w, &sink.sent[i], sizeof w) != 0) fail("a sent record", (long)n, (long)i, sink.sent[i].flags);
        }
        if (bytes.size() != out_len || (out_len != 0 && memcmp(bytes.data(), region, out_len) != 0)) fail("the frames' bytes", (long)n, (long)bytes.size(), out_len);
        for (uint32_t i = out_len; i < room; ++i)
            if (region[i] != 0xEE) fail("a byte behind out_len", (long)n, i, 0);
        reg.check_front();
        ++n;
    }
    fclose(f);
    return n;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 24);
}
static uint32_t pick(uint32_t n) { return rnd() % n; }

static void mutations(long count, long& refused) {
    const uint32_t body_size = 70000;
    uint8_t* body = (uint8_t*)malloc(body_size);
    for (uint32_t i = 0; i < body_size; ++i) body[i] = (uint8_t)rnd();
    const uint32_t edge[] = {0u, 1u, 8u, 9u, 10u, 16383u, 16384u, 16385u, 32768u, 69999u, 70000u, 70001u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
    const uint32_t nedge = sizeof edge / sizeof edge[0];
    std::vector<Frame> fr;
    for (long it = 0; it < count; ++it) {
        const uint32_t nrec = pick(5);
        std::vector<hhuff_h2_send_t> sends(nrec);
        for (auto& s : sends) {
            s.body_off = pick(4) ? pick(body_size) : edge[pick(nedge)];
            s.body_len = pick(4) ? pick(40000) : edge[pick(nedge)];
            s.stream_id = pick(8) ? 1u + pick(1000) : edge[pick(nedge)];
            s.window = (int32_t)(pick(4) ? pick(70000) : edge[pick(nedge)]);
            s.flags = pick(16) ? pick(4) : rnd();
            s.max_frames = pick(2) ? 0u : pick(4);
        }
        const uint32_t m = pick(8) ? (pick(2) ? 16384u : 16384u + pick(40000)) : edge[pick(nedge)];
        const int64_t window = pick(4) ? (int64_t)pick(100000) : (int64_t)(int32_t)edge[pick(nedge)];
        const uint32_t room = pick(4) ? pick(90000) : edge[pick(10)];
        const uint32_t start = pick(1000);
        Region reg(start, room);
        uint8_t* region = reg.bytes;
        WriteSink sink{body, body_size, region, start, room};
        h2d::Result R;
        const hhuff_h2_peer_t P{4096u, 1u, 0xFFFFFFFFu, 65535u, m, 0u, window, 65535};
        h2d::walk(body_size, sends.data(), nrec, m, h2d::peer_ok(P), window, start, room, sink, R);
        if (R.out_len != sink.written || R.out_len > room) fail("mutation: out_len", it, R.out_len, (long)sink.written);
        // the records served against the loop
        int64_t Wc = window, Rm = room;
        size_t i = 0;
        bool bad = !h2d::peer_ok(P);
        for (; !bad && i < nrec; ++i) {
            const hhuff_h2_send_t& s = sends[i];
            if (!h2d::send_ok(s, body_size)) {
                bad = true;
                break;
            }
            const uint32_t why = loop(m, Rm, Wc, s.window, s.body_len, s.flags & 1u, s.flags & 2u, s.max_frames, fr);
            int64_t bytes = 0;
            for (const Frame& x : fr) bytes += x.length;
            if (i >= sink.sent.size()) fail("mutation: a record not served", it, (long)i, 0);
            const hhuff_h2_sent_t& T = sink.sent[i];
            if (T.flags != why || T.nframes != fr.size() || T.sent != bytes || T.window != (int32_t)(s.window - bytes) ||
                T.out_off != start + (uint32_t)(room - Rm))
                fail("mutation: a record against the loop", it, (long)i, T.flags);
            Wc -= bytes, Rm -= bytes + 9 * (int64_t)fr.size();
        }
        if (sink.sent.size() != i) fail("mutation: records behind the refused one", it, (long)sink.sent.size(), (long)i);
        if ((R.status != 0) != bad || (bad && R.status != HHUFF_H2D_EINVAL)) fail("mutation: status", it, R.status, bad);
        if (R.send_window != Wc) fail("mutation: window", it, (long)R.send_window, (long)Wc);
        refused += bad;
        reg.check_front();
        for (uint32_t b = R.out_len; b < room; ++b)
            if (region[b] != 0xEE) fail("mutation: a byte behind out_len", it, b, 0);
    }
    free(body);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        printf("usage: h2data_host CASES MUTATIONS\n");
        return 2;
    }
    printf("%llu records: closed form = loop\n", (unsigned long long)exhaustive());
    printf("%zu cases\n", run_cases(argv[1]));
    long refused = 0;
    const long count = atol(argv[2]);
    mutations(count, refused);
    printf("%ld mutations, %ld refused as out of range\n", count, refused);
    printf("ok: h2data_host\n");
    return 0;
}
