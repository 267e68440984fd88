// The de-framer's rules (h2o_amd/csrc/hhuff_frames.h: the code the kernels run) on the host, as a stand-alone program
// to build with -fsanitize=address,undefined and run directly:
//     frames_host CASES MUTATIONS
// CASES: one line a connection -- cap max_frame_size max_block_bytes flags, then the expected status err consumed
// nframes nblocks block_bytes, then the bytes in hex ("-": none) -- as tests/test_frames_host.py writes them from
// tests/frames_corpora.py.  Every connection is walked in a heap block of exactly its size and must give the expected
// outcome; then cut at every length (under AddressSanitizer the bytes behind the cut are poisoned); then MUTATIONS
// times a seeded choice of connection, byte, value and frame capacity.  Every walk is checked for the invariants the
// kernels rely on: offsets inside the connection, fragments inside their payloads, frames and block bytes numbered
// through without gaps, nothing past the capacity.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "hhuff_frames.h"

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
    frm::Params P;
    int32_t status;
    uint32_t err, consumed, nframes, nblocks, nbytes;
    std::vector<uint8_t> bytes;
};

struct CheckSink {
    const uint8_t* p;
    uint32_t len, cap;
    bool read_bytes;
    uint32_t frames = 0, blocks = 0, bytes = 0, block_first = 0, block_at = 0;
    uint64_t sum = 0;
    size_t id;
    void frame(uint32_t i, const hhuff_h2_frame_t& f, uint32_t dst) {
        if (i != frames || i >= cap) fail("frame index", id, i, frames);
        if ((uint64_t)f.payload_off + f.length > len || f.payload_off < 9) fail("payload range", id, f.payload_off, f.length);
        if (f.rsv != 0 || f.rsv2 != 0 || (f.stream_id >> 31)) fail("reserved bits", id, f.rsv, f.rsv2);
        if (f.block == frm::kNoBlock) {
            if (f.frag_off != 0 || f.frag_len != 0) fail("fragment of a frame that has none", id, f.frag_off, f.frag_len);
            if (f.type == frm::kHeaders || f.type == frm::kPushPromise || f.type == frm::kContinuation) fail("header frame without block", id, f.type, 0);
        } else {
            if (f.block != blocks) fail("block number", id, f.block, blocks);
            if (f.frag_off < f.payload_off || (uint64_t)f.frag_off + f.frag_len > (uint64_t)f.payload_off + f.length)
                fail("fragment range", id, f.frag_off, f.frag_len);
            if (dst != bytes) fail("fragment destination", id, dst, bytes);
            if (read_bytes)
                for (uint32_t k = 0; k < f.frag_len; ++k) sum += p[f.frag_off + k];
            bytes += f.frag_len;
        }
        ++frames;
        if (f.block == frm::kNoBlock) block_first = frames;
    }
    void block(uint32_t b, const hhuff_h2_block_t& r, uint32_t off) {
        if (b != blocks) fail("block index", id, b, blocks);
        if (r.first_frame != block_first || r.first_frame + r.nframes != frames || r.nframes == 0) fail("block frames", id, r.first_frame, r.nframes);
        if (off != block_at) fail("block offset", id, off, block_at);
        if (r.weight < 1 || r.weight > 256 || (r.dependency >> 31) || (r.promised_stream_id >> 31)) fail("priority range", id, r.weight, r.dependency);
        if (((r.flags & HHUFF_H2B_CONTINUED) != 0) != (r.nframes > 1)) fail("continued flag", id, r.flags, r.nframes);
        ++blocks, block_first = frames, block_at = bytes;
    }
};

static frm::Result checked_walk(const uint8_t* p, uint32_t len, const frm::Params& P, bool read_bytes, size_t id) {
    CheckSink sink{p, len, P.frame_cap, read_bytes};
    sink.id = id;
    frm::Result R;
    frm::walk(p, len, P, sink, R);
    if (R.nframes != sink.frames || R.nblocks != sink.blocks || R.block_bytes != sink.bytes) fail("counts", id, R.nframes, R.nblocks);
    if (sink.block_first != sink.frames) fail("header frames behind the last block", id, sink.block_first, sink.frames);
    if (R.consumed > len || R.nframes > P.frame_cap || R.block_bytes > R.consumed) fail("result range", id, R.consumed, R.nframes);
    frm::NoSink none;  // the counting walk says the same
    frm::Result R2;
    frm::walk(p, len, P, none, R2);
    if (memcmp(&R, &R2, sizeof(R)) != 0) fail("the counting walk differs", id, R.status, R2.status);
    return R;
}

int main(int argc, char** argv) {
    if (argc < 3) return printf("usage: frames_host CASES MUTATIONS\n"), 2;
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
            if (sscanf(line, "%u %u %u %u %d %u %u %u %u %u %n", &c.P.frame_cap, &c.P.max_frame_size, &c.P.max_block_bytes, &c.P.flags,
                       &c.status, &c.err, &c.consumed, &c.nframes, &c.nblocks, &c.nbytes, &at) < 10)
                return printf("bad line %zu\n", cases.size()), 2;
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
        uint8_t* p = (uint8_t*)malloc(len ? len : 1);  // (exactly the connection: a read past it is a heap overflow)
        if (len) memcpy(p, c.bytes.data(), len);
        const frm::Result R = checked_walk(len ? p : p + 1, len, c.P, true, i);
        if (R.status != c.status || R.err != c.err) fail("status / err", i, R.status, R.err);
        if (R.consumed != c.consumed || R.nframes != c.nframes) fail("consumed / nframes", i, R.consumed, R.nframes);
        if (R.nblocks != c.nblocks || R.block_bytes != c.nbytes) fail("blocks / block bytes", i, R.nblocks, R.block_bytes);
        ++walks;
        for (uint32_t t = len; t-- > 0;) {  // every truncation: p[t ..) is out of bounds
            POISON(p + t, len - t);
            const frm::Result T = checked_walk(p, t, c.P, false, i);
            if (T.consumed > R.consumed || T.nframes > R.nframes) fail("a cut connection gives more", i, t, T.consumed);
            if (T.consumed >= R.consumed && t < R.consumed) fail("consumed past the cut", i, t, T.consumed);
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
    long done = 0, changed = 0;
    while (done < mutations) {
        const size_t i = (size_t)(rnd() % cases.size());
        const Case& c = cases[i];
        const uint32_t len = (uint32_t)c.bytes.size();
        if (len == 0) continue;
        uint8_t* p = (uint8_t*)malloc(len);
        memcpy(p, c.bytes.data(), len);
        // (most of a long connection is payload: aim half of the mutations at the first 64 bytes)
        const uint32_t at = (uint32_t)(rnd() % ((rnd() & 1) && len > 64 ? 64 : len));
        p[at] ^= (uint8_t)(1u + rnd() % 255u);
        frm::Params P = c.P;
        if (rnd() & 1) P.frame_cap = (uint32_t)(rnd() % 5);
        if (rnd() & 1) P.flags ^= HHUFF_H2F_ACCEPT_PUSH;
        const frm::Result R = checked_walk(p, len, P, len <= 65536, i);
        changed += R.status != c.status || R.consumed != c.consumed;
        free(p);
        ++done;
    }
    printf("%ld mutations, %ld with another outcome\n", done, changed);
    printf("ok: frames_host\n");
    return 0;
}
