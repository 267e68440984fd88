// The HTTP/3 body arithmetic (h2o_amd/csrc/hhuff_h3bodies.h: the code the kernels run) on the host, as a stand-alone
// program to build with -fsanitize=address,undefined and run directly: the DATA header at the varint's edges against
// bytes written out by hand, the content-length bisection against h2o's plain loop over every small stream the
// de-framer can list, and write_line against memcpy over seeded segment lists, `out` a heap block of exactly its size.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hhuff_h3bodies.h"

using namespace hhuff;

static void fail(const char* what, long a, long b) {
    fprintf(stderr, "FAIL: %s (%ld, %ld)\n", what, a, b);
    exit(1);
}

static void check_headers() {
    struct { uint64_t len; uint32_t h; uint8_t b[9]; } want[] = {
        {1, 2, {0, 0x01}}, {63, 2, {0, 0x3f}}, {64, 3, {0, 0x40, 0x40}}, {16383, 3, {0, 0x7f, 0xff}}, {16384, 5, {0, 0x80, 0, 0x40, 0}},
        {(1u << 30) - 1, 5, {0, 0xbf, 0xff, 0xff, 0xff}}, {1u << 30, 9, {0, 0xc0, 0, 0, 0, 0x40, 0, 0, 0}},
        {0xFFFFFFFFull, 9, {0, 0xc0, 0, 0, 0, 0xff, 0xff, 0xff, 0xff}}};
    for (auto& w : want) {
        if (h3b::hdr_len(w.len) != w.h || h3b::hdr_of_size(w.len + w.h) != w.h) fail("header length", (long)w.len, w.h);
        for (uint32_t i = 0; i < w.h; ++i)
            if (h3b::hdr_byte(w.len, w.h, i) != w.b[i]) fail("header byte", (long)w.len, i);
    }
    if (h3b::hdr_len(0) != 0 || h3b::hdr_of_size(0) != 0) fail("an empty record has a header", 0, 0);
}

static long check_content_length() {
    long streams = 0;
    for (uint32_t n = 0; n <= 5; ++n)
        for (uint32_t code = 0, end = 1; code < end; ++code) {
            // digit 0: another frame; 1 .. 3: a complete DATA frame of 0 .. 2 bytes; 4: 1 byte of a DATA frame of 2 (last
            // slot only); the first slot may also be 5 / 6: a continued frame of 2 bytes, whole or 1 byte of it (then last)
            std::vector<hhuff_h3_frame_t> F(n);
            bool ok = true;
            end = 1;
            for (uint32_t i = 0, c = code; i < n; ++i, c /= 7, end *= 7) {
                const uint32_t d = c % 7;
                if ((d >= 5 && i != 0) || ((d == 4 || d == 6) && i + 1 != n)) ok = false;
                F[i] = d == 0   ? hhuff_h3_frame_t{0x21, 8, 10, 3, 3, 0}
                       : d <= 3 ? hhuff_h3_frame_t{0, 8, 10, d - 1, d - 1, 0}
                       : d == 4 ? hhuff_h3_frame_t{0, 8, 10, 2, 1, 0}
                                : hhuff_h3_frame_t{0, 10, 10, 2, d == 5 ? 2u : 1u, 0};
            }
            if (!ok) continue;
            ++streams;
            std::vector<uint64_t> P(n + 1, 0);
            for (uint32_t i = 0; i < n; ++i) P[i + 1] = P[i] + h3b::slot_count(F[i], 100).bytes;
            for (uint64_t cl = 0; cl <= 8; ++cl)
                for (uint64_t rcv = 0; rcv <= cl; ++rcv) {
                    if (n && F[0].hdr_off == F[0].payload_off && rcv + F[0].length > cl) continue;  // h2o tested it a step ago
                    uint32_t plain = n;  // server.c:1431, frame by frame
                    uint64_t r = rcv;
                    for (uint32_t i = 0; i < n && plain == n; ++i) {
                        if (F[i].type != 0) continue;
                        if (F[i].hdr_off != F[i].payload_off && cl - r < F[i].length) plain = i;
                        r += F[i].avail;
                    }
                    const uint32_t got = h3b::first_true(n, [&](uint32_t j) { return h3b::over(cl - rcv, P[j], h3b::header_length(F[j])); });
                    if (got != plain) fail("the content-length cut", (long)code, (long)(cl * 16 + rcv));
                }
        }
    return streams;
}

template <bool kHdr>
static void check_lines(uint32_t seed) {
    srand(seed);
    static const uint32_t lens[] = {0, 0, 1, 2, 3, 15, 16, 17, 33, 70, 300};
    const uint32_t src_size = 4096;
    uint8_t* src = (uint8_t*)aligned_alloc(16, src_size);  // whole dwords: the call reads the aligned dwords of a payload
    for (uint32_t i = 0; i < src_size; ++i) src[i] = (uint8_t)(i * 131u + (i >> 8) + 7u);
    const uint32_t nseg = 1 + rand() % 40, a = rand() % 16, cut = rand() % 4 == 0 ? rand() % nseg : nseg;
    std::vector<uint32_t> pre{0}, from;
    std::vector<uint8_t> want;
    for (uint32_t k = 0; k < nseg; ++k) {
        const uint32_t len = lens[rand() % 11], h = kHdr ? h3b::hdr_len(len) : 0u, at = rand() % (src_size - len + 1);
        const bool unread = len != 0 && rand() % 8 == 0;
        from.push_back(len == 0 || unread ? h3b::kBadSrc : at);
        for (uint32_t i = 0; i < h; ++i) want.push_back((uint8_t)h3b::hdr_byte(len, h, i));
        for (uint32_t i = 0; i < len; ++i) want.push_back(unread ? 0 : src[at + i]);
        pre.push_back((uint32_t)want.size());
    }
    const uint32_t limit = pre[cut];
    for (uint32_t& p : pre) p = p < limit ? p : limit;  // as the copy kernel clamps the window
    uint8_t* out = (uint8_t*)malloc(a + limit ? a + limit : 1);  // exactly its size; the lines are cut by its own address
    memset(out, 0xEE, a + limit);
    const uint64_t base = (uint64_t)(uintptr_t)out + a, a2 = base & 15u;
    auto find = [&](uint32_t x) {  // the last segment that begins at or before out[x]
        size_t k = 0;
        for (size_t j = 0; j + 1 < pre.size(); ++j)
            if (pre[j] <= x) k = j;
        return h3b::Seg{pre[k], pre[k + 1], from[k]};
    };
    for (uint64_t l = 0; l < (a2 + limit + 15u) >> 4 && limit; ++l)
        h3b::write_line<kHdr>((uint64_t)(uintptr_t)src, (base & ~15ull) + 16u * l, (int64_t)(16u * l) - (int64_t)a2, limit, find);
    if (limit && memcmp(out + a, want.data(), limit) != 0) fail("the lines differ from memcpy", seed, limit);
    for (uint32_t i = 0; i < a; ++i)
        if (out[i] != 0xEE) fail("a byte in front of out was written", seed, i);
    free(out), free(src);
}

int main() {
    check_headers();
    const long streams = check_content_length();
    for (uint32_t seed = 0; seed < 3000; ++seed) check_lines<false>(seed), check_lines<true>(seed);
    fprintf(stderr, "ok: h3bodies_host, %ld streams\n", streams);
    return 0;
}
