// The control-frame rules (h2o_amd/csrc/hhuff_h2ctl.h: the code the kernel runs) on the host, as a stand-alone program
// to build with -fsanitize=address,undefined and run directly:
//     h2ctl_host CASES MUTATIONS
// CASES: one line a connection, as tests/test_h2ctl_host.py writes them from tests/h2ctl_corpora.py --
//     client recv_window_size rep_cap in_size(-1: the connection's)   the start state (8 numbers)
//     the expected status err nctl, the state afterwards (8 numbers), nrec and nrec x (a b status err flags reply_len),
//     the expected replies in hex, the connection in hex ("-": none)
// Every connection is de-framed by hhuff_frames.h, as the GPU path does it, into a heap block of exactly its records,
// and walked with its bytes and its reply region in heap blocks of exactly their sizes; the outcome must be the
// expected one.  Then it is cut at every length (under AddressSanitizer the bytes behind the cut are poisoned); then
// MUTATIONS times a seeded choice of connection and either a byte mutation of the connection or a hostile change of one
// frame record, with a random reply capacity and side.  Every walk is checked for the invariants the kernel relies
// on: nothing past the records listed, reply bytes = the records' reply_len summed and inside the region, the
// canary records behind the last one written untouched.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "hhuff_frames.h"
#include "hhuff_h2ctl.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) __asan_poison_memory_region((p), (n))
#define UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
#endif

using namespace hhuff;

static void fail(const char* what, size_t c, long a, long b) {
    printf("FAIL: %s (connection %zu: %ld, %ld)\n", what, c, a, b);
    exit(1);
}

struct Case {
    uint32_t client, rws, rep_cap;
    long in_size;
    hhuff_h2_peer_t start, after;
    int32_t status;
    uint32_t err, nctl;
    std::vector<hhuff_h2_ctl_t> records;
    std::vector<uint8_t> replies, bytes;
};

struct FrameSink {
    std::vector<hhuff_h2_frame_t>& v;
    void frame(uint32_t, const hhuff_h2_frame_t& f, uint32_t) { v.push_back(f); }
    void block(uint32_t, const hhuff_h2_block_t&, uint32_t) {}
};

static std::vector<hhuff_h2_frame_t> deframe(const uint8_t* p, uint32_t len) {
    std::vector<hhuff_h2_frame_t> v;
    FrameSink sink{v};
    frm::Result R;
    frm::walk(p, len, frm::Params{16777215u, 0u, HHUFF_H2F_ACCEPT_PUSH, 1u << 20}, sink, R);
    return v;
}

constexpr uint8_t kCanary = 0xC7;

struct RecSink {
    hhuff_h2_ctl_t* out;
    uint32_t n, next = 0;
    size_t id;
    void record(uint32_t i, const hhuff_h2_ctl_t& r) {
        if (i != next || i >= n) fail("record index", id, i, next);
        out[i] = r, ++next;
    }
};

struct Outcome {
    h2c::Result R;
    hhuff_h2_peer_t S;
    std::vector<hhuff_h2_ctl_t> rec;  // those written
    std::vector<uint8_t> rep;
};

// p[0 .. in_size) are the bytes the records may point into; the records, the results and the replies live in heap
// blocks of exactly their sizes.
static Outcome checked_walk(const uint8_t* p, uint64_t in_size, const std::vector<hhuff_h2_frame_t>& frames, const h2c::Params& P,
                            const hhuff_h2_peer_t& start, uint32_t rep_cap, size_t id) {
    const uint32_t n = (uint32_t)frames.size();
    hhuff_h2_frame_t* fr = (hhuff_h2_frame_t*)malloc(n ? n * sizeof(hhuff_h2_frame_t) : 1);
    if (n) memcpy(fr, frames.data(), n * sizeof(hhuff_h2_frame_t));
    hhuff_h2_ctl_t* ctl = (hhuff_h2_ctl_t*)malloc(n ? n * sizeof(hhuff_h2_ctl_t) : 1);
    memset(ctl, kCanary, n * sizeof(hhuff_h2_ctl_t));
    uint8_t* rep = (uint8_t*)malloc(rep_cap ? rep_cap : 1);
    memset(rep, kCanary, rep_cap);
    Outcome o;
    o.S = start;
    RecSink sink{ctl, n};
    sink.id = id;
    h2c::walk(p, in_size, fr, n, P, o.S, rep, rep_cap, sink, o.R);
    const h2c::Result& R = o.R;
    if (R.nctl > n || R.rep_len > rep_cap) fail("result range", id, R.nctl, R.rep_len);
    const bool h2o_failure = R.status != 0 && R.status != HHUFF_H2C_SPACE && R.status != HHUFF_H2C_EINVAL;
    if (sink.next != R.nctl + (h2o_failure ? 1u : 0u)) fail("records written", id, sink.next, R.nctl);
    if (R.status == 0 && R.nctl != n) fail("no failure, yet frames left", id, R.nctl, n);
    uint32_t sum = 0;
    for (uint32_t i = 0; i < sink.next; ++i) {
        const hhuff_h2_ctl_t& c = ctl[i];
        sum += c.reply_len;
        if (c.reply_len != 0 && c.reply_len != 9 && c.reply_len != 13 && c.reply_len != 17) fail("reply length", id, i, c.reply_len);
        if (i < R.nctl && c.status != 0 && (c.flags & HHUFF_H2R_STREAM_ERROR) == 0) fail("a failing record in front of the stop", id, i, c.status);
        if (i == R.nctl && (c.status != R.status || c.err != R.err || c.reply_len != 0)) fail("the failing record", id, c.status, R.status);
        if (fr[i].type == h2c::kData && c.status == 0 && ((uint64_t)c.a + c.b > in_size || c.a < fr[i].payload_off)) fail("data range", id, c.a, c.b);
        if (fr[i].type == h2c::kPriority && c.status == 0 && (c.b < 1 || c.b > 256)) fail("weight", id, i, c.b);
    }
    if (sum != R.rep_len) fail("reply bytes", id, sum, R.rep_len);
    for (size_t k = (size_t)sink.next * sizeof(hhuff_h2_ctl_t); k < (size_t)n * sizeof(hhuff_h2_ctl_t); ++k)
        if (((const uint8_t*)ctl)[k] != kCanary) fail("a record behind the stop written", id, (long)k, 0);
    for (uint32_t k = R.rep_len; k < rep_cap; ++k)
        if (rep[k] != kCanary) fail("reply region written behind rep_len", id, k, R.rep_len);
    if (o.S.send_window > h2c::kInt32Max && o.S.send_window != start.send_window) fail("send window past INT32_MAX", id, 0, 0);
    o.rec.assign(ctl, ctl + sink.next);
    o.rep.assign(rep, rep + R.rep_len);
    free(fr), free(ctl), free(rep);
    return o;
}

static bool same_peer(const hhuff_h2_peer_t& a, const hhuff_h2_peer_t& b) {
    return a.header_table_size == b.header_table_size && a.enable_push == b.enable_push &&
           a.max_concurrent_streams == b.max_concurrent_streams && a.initial_window_size == b.initial_window_size &&
           a.max_frame_size == b.max_frame_size && a.flags == b.flags && a.send_window == b.send_window && a.recv_window == b.recv_window;
}

static bool read_peer(const char*& s, hhuff_h2_peer_t& p) {
    int at = 0;
    long long send, recv;
    if (sscanf(s, "%u %u %u %u %u %u %lld %lld %n", &p.header_table_size, &p.enable_push, &p.max_concurrent_streams,
               &p.initial_window_size, &p.max_frame_size, &p.flags, &send, &recv, &at) < 8)
        return false;
    p.send_window = send, p.recv_window = recv, s += at;
    return true;
}

static std::vector<uint8_t> read_hex(const char*& s) {
    std::vector<uint8_t> v;
    auto nib = [](char ch) { return (uint8_t)(ch <= '9' ? ch - '0' : ch - 'a' + 10); };
    if (*s == '-') {
        ++s;
    } else {
        for (; s[0] > ' ' && s[1] > ' '; s += 2) v.push_back((uint8_t)(nib(s[0]) << 4 | nib(s[1])));
    }
    while (*s == ' ') ++s;
    return v;
}

int main(int argc, char** argv) {
    if (argc < 3) return printf("usage: h2ctl_host CASES MUTATIONS\n"), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return printf("cannot read %s\n", argv[1]), 2;
    const long mutations = atol(argv[2]);
    std::vector<Case> cases;
    {
        char* line = nullptr;
        size_t cap = 0;
        while (getline(&line, &cap, f) > 0) {
            Case c{};
            const char* s = line;
            int at = 0;
            uint32_t nrec = 0;
            if (sscanf(s, "%u %u %u %ld %n", &c.client, &c.rws, &c.rep_cap, &c.in_size, &at) < 4) return printf("bad line %zu\n", cases.size()), 2;
            s += at;
            if (!read_peer(s, c.start)) return printf("bad start %zu\n", cases.size()), 2;
            if (sscanf(s, "%d %u %u %n", &c.status, &c.err, &c.nctl, &at) < 3) return printf("bad outcome %zu\n", cases.size()), 2;
            s += at;
            if (!read_peer(s, c.after)) return printf("bad end state %zu\n", cases.size()), 2;
            if (sscanf(s, "%u %n", &nrec, &at) < 1) return printf("bad record count %zu\n", cases.size()), 2;
            s += at;
            for (uint32_t i = 0; i < nrec; ++i) {
                unsigned a, b, err, fl, rl;
                int st;
                if (sscanf(s, "%u %u %d %u %u %u %n", &a, &b, &st, &err, &fl, &rl, &at) < 6) return printf("bad record %zu\n", cases.size()), 2;
                s += at;
                c.records.push_back(hhuff_h2_ctl_t{a, b, st, (uint16_t)err, (uint8_t)fl, (uint8_t)rl});
            }
            c.replies = read_hex(s);
            c.bytes = read_hex(s);
            cases.push_back(c);
        }
        free(line);
        fclose(f);
    }
    size_t walks = 0;
    for (size_t i = 0; i < cases.size(); ++i) {
        const Case& c = cases[i];
        const uint32_t len = (uint32_t)c.bytes.size();
        uint8_t* p = (uint8_t*)malloc(len ? len : 1);  // (exactly the connection: a read past it is a heap overflow)
        if (len) memcpy(p, c.bytes.data(), len);
        const h2c::Params P{c.client ? HHUFF_H2C_CLIENT : 0u, c.rws};
        const std::vector<hhuff_h2_frame_t> frames = deframe(p, len);
        const uint64_t in_size = c.in_size < 0 ? len : (uint64_t)c.in_size;
        const Outcome o = checked_walk(p, in_size, frames, P, c.start, c.rep_cap, i);
        if (o.R.status != c.status || o.R.err != c.err || o.R.nctl != c.nctl) fail("status / err / nctl", i, o.R.status, o.R.nctl);
        if (!same_peer(o.S, c.after)) fail("state afterwards", i, (long)o.S.send_window, (long)o.S.recv_window);
        if (o.rep != c.replies) fail("replies", i, (long)o.rep.size(), (long)c.replies.size());
        if (o.rec.size() != c.records.size()) fail("records written", i, (long)o.rec.size(), (long)c.records.size());
        for (size_t k = 0; k < o.rec.size(); ++k)
            if (memcmp(&o.rec[k], &c.records[k], sizeof(hhuff_h2_ctl_t)) != 0) fail("record", i, (long)k, o.rec[k].status);
        ++walks;
        for (uint32_t t = len; t-- > 0;) {  // every truncation: p[t ..) is out of bounds
            POISON(p + t, len - t);
            const std::vector<hhuff_h2_frame_t> cut = deframe(p, t);
            const Outcome q = checked_walk(p, t, cut, P, c.start, c.rep_cap, i);
            if (q.R.nctl > o.R.nctl) fail("a cut connection handles more", i, t, q.R.nctl);
            if (q.rep.size() > o.rep.size() || !std::equal(q.rep.begin(), q.rep.end(), o.rep.begin())) fail("a cut connection answers otherwise", i, t, 0);
            ++walks;
        }
        UNPOISON(p, len ? len : 1);
        free(p);
    }
    printf("%zu cases, %zu walks with truncations\n", cases.size(), walks);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&s]() {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        return s;
    };
    long done = 0, changed = 0, hostile = 0, refused = 0;
    while (done < mutations) {
        const size_t i = (size_t)(rnd() % cases.size());
        const Case& c = cases[i];
        const uint32_t len = (uint32_t)c.bytes.size();
        if (len == 0) continue;
        uint8_t* p = (uint8_t*)malloc(len);
        memcpy(p, c.bytes.data(), len);
        h2c::Params P{(rnd() & 1) ? HHUFF_H2C_CLIENT : 0u, (rnd() & 1) ? c.rws : (uint32_t)(rnd() % 2000)};
        const uint32_t rep_cap = (rnd() & 1) ? c.rep_cap : (uint32_t)(rnd() % 40);
        std::vector<hhuff_h2_frame_t> frames;
        if (rnd() % 3 != 0) {
            p[rnd() % len] ^= (uint8_t)(1u + rnd() % 255u);
            frames = deframe(p, len);
        } else {  // a frame record overwritten: any offset, any length, any type
            frames = deframe(p, len);
            if (!frames.empty()) {
                hhuff_h2_frame_t& fr = frames[rnd() % frames.size()];
                switch (rnd() % 4) {
                    case 0: fr.payload_off = (uint32_t)rnd(); break;
                    case 1: fr.length = (rnd() & 1) ? (uint32_t)rnd() : (uint32_t)(rnd() % (len + 8)); break;
                    case 2: fr.payload_off = len - (uint32_t)(rnd() % 4), fr.length = (uint32_t)(rnd() % 12); break;
                    default: fr.type = (uint8_t)(rnd() % 10), fr.stream_id = (uint32_t)rnd(); break;
                }
                ++hostile;
            }
        }
        const Outcome o = checked_walk(p, len, frames, P, c.start, rep_cap, i);
        changed += o.R.status != c.status || o.R.nctl != c.nctl;
        refused += o.R.status == HHUFF_H2C_EINVAL;
        free(p);
        ++done;
    }
    printf("%ld mutations, %ld with another outcome, %ld hostile records, %ld refused as out of range\n", done, changed, hostile, refused);
    printf("ok: h2ctl_host\n");
    return 0;
}
