// The HTTP/3 de-framer's rules (h2o_amd/csrc/hhuff_h3frames.h: the code the kernels run) on the host, as a
// stand-alone program to build with -fsanitize=address,undefined and run directly:
//     h3frames_host CASES MUTATIONS
// CASES: one line a stream -- the call's flags and max_frame_payload_size, the frame capacity, the state record (kind
// phase flags reserved data_left), then the expected status err consumed nframes, the state to present next (kind
// phase data_left), sections, section bytes, encoder bytes, SETTINGS passed, then the bytes in hex ("-": none) -- as
// tests/test_h3frames_host.py writes them from tests/h3frames_corpora.py.  Every stream is walked in a heap block of
// exactly its size and must give the expected outcome; then cut at every length (under AddressSanitizer the bytes
// behind the cut are poisoned), and the cut stream's outcome carried on over the rest must end where the whole
// stream ended; then MUTATIONS times a seeded choice of stream, byte, value, state and frame capacity.  Every walk is
// checked for the invariants the kernels rely on: offsets inside the stream, frames numbered through without gaps,
// at most one section and never beside an encoder run, nothing past the capacity.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hhuff_h3frames.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) __asan_poison_memory_region((p), (n))
#define UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
#endif

using namespace hhuff;

static void fail(const char* what, size_t c, long long a, long long b) {
    printf("FAIL: %s (stream %zu: %lld, %lld)\n", what, c, a, b);
    exit(1);
}

struct Case {
    h3f::Params P;
    hhuff_h3_stream_t st;
    int32_t status;
    uint32_t err, consumed, nframes, okind, ophase, nsec, sec_bytes, enc_bytes, got;
    uint64_t odata_left;
    std::vector<uint8_t> bytes;
};

struct CheckSink {
    const uint8_t* p;
    uint32_t len, cap;
    bool read_bytes;
    size_t id;
    uint32_t frames = 0, sections = 0, encoders = 0, settings_seen = 0, at = 0, sec_bytes = 0, enc_bytes = 0;
    uint64_t sum = 0;
    void frame(uint32_t i, const hhuff_h3_frame_t& f) {
        if (i != frames || i >= cap) fail("frame index", id, i, frames);
        if (f.hdr_off < at || f.payload_off < f.hdr_off || f.payload_off - f.hdr_off > 16) fail("header range", id, f.hdr_off, f.payload_off);
        if ((uint64_t)f.payload_off + f.avail > len || f.avail > f.length) fail("payload range", id, f.payload_off, f.avail);
        if (f.type != h3f::kData && f.avail != f.length) fail("a frame that is not DATA listed without its payload", id, (long long)f.type, f.avail);
        if (f.type != h3f::kHeaders && f.type != h3f::kGoaway && f.type != h3f::kPriorityUpdateRequest && f.type != h3f::kPriorityUpdatePush && f.aux != 0)
            fail("aux", id, (long long)f.type, f.aux);
        if (read_bytes)
            for (uint32_t k = 0; k < f.avail; ++k) sum += p[f.payload_off + k];
        at = f.payload_off + f.avail;
        ++frames;
    }
    void section(uint32_t off, uint32_t n) {
        if ((uint64_t)off + n > len || off + n != at) fail("section range", id, off, n);
        ++sections, sec_bytes += n;
    }
    void encoder(uint32_t off, uint32_t n) {
        if ((uint64_t)off + n != len || n == 0) fail("encoder range", id, off, n);
        if (read_bytes)
            for (uint32_t k = 0; k < n; ++k) sum += p[off + k];
        ++encoders, enc_bytes += n;
    }
    void settings(const h3f::Settings& S) {
        if (S.h3_datagram > 1) fail("datagram bit", id, S.h3_datagram, 0);
        ++settings_seen;
    }
};

static h3f::Result checked_walk(const uint8_t* p, uint32_t len, const hhuff_h3_stream_t& st, const h3f::Params& P, bool read_bytes,
                                size_t id) {
    CheckSink sink{p, len, P.frame_cap, read_bytes, id};
    h3f::Result R;
    h3f::walk(p, len, st, P, sink, R);
    if (R.nframes != sink.frames || R.nsec != sink.sections || R.sec_bytes != sink.sec_bytes || R.enc_bytes != sink.enc_bytes ||
        R.got_settings != sink.settings_seen)
        fail("counts", id, R.nframes, R.nsec);
    if (R.nsec > 1 || (R.nsec && R.enc_bytes) || sink.encoders > 1 || R.got_settings > 1) fail("more than one copy job", id, R.nsec, R.enc_bytes);
    if (R.consumed > len || R.nframes > P.frame_cap) fail("result range", id, R.consumed, R.nframes);
    if (sink.frames && sink.at > R.consumed) fail("a frame listed past consumed", id, sink.at, R.consumed);
    const hhuff_h3_stream_t next = h3f::next_state(st, R);
    if (R.status != HHUFF_H3F_EINVAL && !h3f::state_valid(next, P.is_client != 0)) fail("the next state is not valid", id, next.kind, next.phase);
    if (R.status == HHUFF_H3F_EINVAL && (R.consumed || R.nframes || memcmp(&next, &st, sizeof(st)) != 0)) fail("EINVAL moved", id, R.consumed, 0);
    h3f::NoSink none;  // the counting walk says the same
    h3f::Result R2;
    h3f::walk(p, len, st, P, none, R2);
    if (memcmp(&R, &R2, sizeof(R)) != 0) fail("the counting walk differs", id, R.status, R2.status);
    return R;
}

int main(int argc, char** argv) {
    if (argc < 3) return printf("usage: h3frames_host CASES MUTATIONS\n"), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return printf("cannot read %s\n", argv[1]), 2;
    const long mutations = atol(argv[2]);
    std::vector<Case> cases;
    {
        char* line = nullptr;
        size_t cap = 0;
        while (getline(&line, &cap, f) > 0) {
            Case c{};
            int at = 0;
            unsigned kind, phase, sflags, rsv;
            unsigned long long mfps, data_left, odata_left;
            if (sscanf(line, "%u %llu %u %u %u %u %u %llu %d %u %u %u %u %u %llu %u %u %u %u %n", &c.P.is_client, &mfps, &c.P.frame_cap, &kind,
                       &phase, &sflags, &rsv, &data_left, &c.status, &c.err, &c.consumed, &c.nframes, &c.okind, &c.ophase, &odata_left,
                       &c.nsec, &c.sec_bytes, &c.enc_bytes, &c.got, &at) < 19)
                return printf("bad line %zu\n", cases.size()), 2;
            c.P.max_frame_payload_size = mfps, c.odata_left = odata_left;
            c.st.data_left = data_left, c.st.kind = (uint8_t)kind, c.st.phase = (uint8_t)phase, c.st.flags = (uint8_t)sflags;
            c.st.rsv[0] = (uint8_t)rsv, c.st.stream_id = 4 * cases.size();
            const char* hex = line + at;
            if (*hex != '-') {
                auto nib = [](char ch) { return (uint8_t)(ch <= '9' ? ch - '0' : ch - 'a' + 10); };
                for (; hex[0] > ' ' && hex[1] > ' '; hex += 2) c.bytes.push_back((uint8_t)(nib(hex[0]) << 4 | nib(hex[1])));
            }
            cases.push_back(c);
        }
        free(line);
        fclose(f);
    }
    size_t walks = 0;
    for (size_t i = 0; i < cases.size(); ++i) {
        const Case& c = cases[i];
        const uint32_t len = (uint32_t)c.bytes.size();
        uint8_t* p = (uint8_t*)malloc(len ? len : 1);  // (exactly the stream: a read past it is a heap overflow)
        if (len) memcpy(p, c.bytes.data(), len);
        const h3f::Result R = checked_walk(len ? p : p + 1, len, c.st, c.P, true, i);
        if (R.status != c.status || R.err != c.err) fail("status / err", i, R.status, R.err);
        if (R.consumed != c.consumed || R.nframes != c.nframes) fail("consumed / nframes", i, R.consumed, R.nframes);
        if (R.kind != c.okind || R.phase != c.ophase || R.data_left != c.odata_left) fail("next state", i, R.kind, R.phase);
        if (R.nsec != c.nsec || R.sec_bytes != c.sec_bytes || R.enc_bytes != c.enc_bytes || R.got_settings != c.got)
            fail("sections / encoder bytes / settings", i, R.nsec, R.enc_bytes);
        ++walks;
        for (uint32_t t = len; t-- > 0;) {  // every truncation: p[t ..) is out of bounds
            POISON(p + t, len - t);
            const h3f::Result T = checked_walk(p, t, c.st, c.P, false, i);
            if (T.consumed > t) fail("consumed past the cut", i, t, T.consumed);
            UNPOISON(p + t, len - t);
            ++walks;
            // carried on with fresh slots the stream ends where the whole stream ended (a frame slot error aside: the
            // second step has slots of its own; and the stop behind a section, which the first step may have made)
            if (T.status != 0 || c.status == HHUFF_H3F_FRAMES || c.status == HHUFF_H3F_EINVAL) continue;
            const hhuff_h3_stream_t mid = h3f::next_state(c.st, T);
            const h3f::Result U = checked_walk(p + T.consumed, len - T.consumed, mid, c.P, false, i);
            ++walks;
            const bool stopped = T.nsec && !(c.st.flags & HHUFF_H3S_WALK_ON);
            if (!stopped && R.status == 0 && !(R.nsec && !(c.st.flags & HHUFF_H3S_WALK_ON)) &&
                (U.status != 0 || T.consumed + U.consumed != R.consumed || U.kind != R.kind || U.phase != R.phase || U.data_left != R.data_left))
                fail("two steps end elsewhere", i, t, T.consumed + U.consumed);
            if (T.nsec + U.nsec > 1 && !stopped) fail("two sections", i, t, 0);
        }
        free(p);
    }
    printf("%zu cases, %zu walks with truncations\n", cases.size(), walks);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&s]() {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        return s;
    };
    long done = 0, changed = 0;
    while (done < mutations) {
        const size_t i = (size_t)(rnd() % cases.size());
        const Case& c = cases[i];
        const uint32_t len = (uint32_t)c.bytes.size();
        if (len == 0) continue;
        uint8_t* p = (uint8_t*)malloc(len);
        memcpy(p, c.bytes.data(), len);
        const uint32_t at = (uint32_t)(rnd() % ((rnd() & 1) && len > 32 ? 32 : len));
        p[at] ^= (uint8_t)(1u + rnd() % 255u);
        h3f::Params P = c.P;
        hhuff_h3_stream_t st = c.st;
        if (rnd() & 1) P.frame_cap = (uint32_t)(rnd() % 5);
        if (rnd() & 1) P.is_client ^= 1u;
        if (rnd() % 4 == 0) P.max_frame_payload_size = rnd() % 64;
        if (rnd() % 4 == 0) st.kind = (uint8_t)(rnd() % 7), st.phase = (uint8_t)(rnd() % 5), st.data_left = rnd() % 3 ? 0 : rnd() % 40;
        if (rnd() % 4 == 0) st.flags = (uint8_t)(rnd() % 9);
        const h3f::Result R = checked_walk(p, len, st, P, true, i);
        changed += R.status != c.status || R.consumed != c.consumed;
        free(p);
        ++done;
    }
    printf("%ld mutations, %ld with another outcome\n", done, changed);
    printf("ok: h3frames_host\n");
    return 0;
}
