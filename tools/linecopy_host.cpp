// The line copy and the range clamp of h2o_amd/csrc/hhuff_linecopy.h on the host, stand-alone (tests/test_linecopy_host.py
// builds it with -fsanitize=address,undefined; it needs no GPU): the code the copy kernels run.
// 1. load16, store_part and copy_line against memcpy for every source residue 0-3, destination residue 0-15 and
//    length 1-48.  The source is a heap block of exactly the aligned dwords that hold its bytes, so a dword loaded
//    without need is a finding of the sanitizer; the destination lies between canary bytes, and a job's lines are
//    written in both orders.
// 2. lines_of against a count of the lines touched.
// 3. clamp_range against the definition -- the x with a <= x < b and x < cap, counted one by one where they lie
//    below 10 and by 64-bit arithmetic else -- for all a, b, cap of 0 .. 9, 2^32 - 2 and 2^32 - 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hhuff_linecopy.h"

using namespace hhuff;

static void fail(const char* what, long a, long b, long c) {
    fprintf(stderr, "FAIL: %s (%ld, %ld, %ld)\n", what, a, b, c);
    exit(1);
}

static const uint8_t kCanary = 0xEE;

static void check_copies() {
    for (uint32_t r = 0; r < 4; ++r)
        for (uint32_t dr = 0; dr < 16; ++dr)
            for (uint32_t len = 1; len <= 48; ++len) {
                const size_t src_bytes = (r + len + 3u) & ~(size_t)3u;  // the aligned dwords that hold the source
                uint8_t* exact = (uint8_t*)malloc(src_bytes);  // (dword-aligned, and src_bytes to the byte)
                for (size_t i = 0; i < src_bytes; ++i) exact[i] = (uint8_t)(37u * i + 11u * r + len);
                const uint8_t* src = exact + r;
                uint8_t* dblock = (uint8_t*)aligned_alloc(16, 96);
                uint8_t* dst = dblock + 16 + dr;
                const uint64_t d0 = (uint64_t)(uintptr_t)dst, d1 = d0 + len, s0 = (uint64_t)(uintptr_t)src;
                const uint32_t nl = lc::lines_of(d0, len);
                for (int order = 0; order < 2; ++order) {
                    memset(dblock, kCanary, 96);
                    for (uint32_t i = 0; i < nl; ++i) lc::copy_line(s0, d0, d1, order ? nl - 1u - i : i);
                    for (uint32_t i = 0; i < 96; ++i) {
                        const bool in = i >= 16 + dr && i < 16 + dr + len;
                        if (dblock[i] != (in ? src[i - 16 - dr] : kCanary)) fail("copy_line", r, dr, len);
                    }
                }
                // every line of the job through load16 and store_part alone
                memset(dblock, kCanary, 96);
                for (uint32_t li = 0; li < nl; ++li) {
                    const uint64_t line = (d0 & ~15ull) + 16ull * li;
                    const int b0 = (int)((line > d0 ? line : d0) - line), b1 = (int)((line + 16u < d1 ? line + 16u : d1) - line);
                    uint32_t v[4];
                    lc::load16(s0 + (line - d0), b0, b1, v);
                    for (int i = b0; i < b1; ++i)
                        if ((uint8_t)(v[i >> 2] >> (8 * (i & 3))) != src[line + i - d0]) fail("load16", r, dr, len);
                    lc::store_part(reinterpret_cast<uint8_t*>((uintptr_t)line), v, b0, b1);
                }
                uint8_t want[96];
                memset(want, kCanary, 96);
                memcpy(want + 16 + dr, src, len);
                if (memcmp(dblock, want, 96) != 0) fail("load16 and store_part", r, dr, len);
                free(dblock), free(exact);
            }
}

static void check_lines() {
    for (uint64_t addr = 4096; addr < 4096 + 16; ++addr)
        for (uint64_t n = 1; n <= 48; ++n) {
            uint32_t want = 0;
            for (uint64_t i = 0; i < n; ++i)
                if (i == 0 || ((addr + i) & 15u) == 0) ++want;
            if (lc::lines_of(addr, n) != want) fail("lines_of", (long)addr, (long)n, want);
        }
}

static void check_clamp() {
    uint32_t vals[12];
    for (uint32_t i = 0; i < 10; ++i) vals[i] = i;
    vals[10] = 0xFFFFFFFEu, vals[11] = 0xFFFFFFFFu;
    long n = 0;
    for (uint32_t a : vals)
        for (uint32_t b : vals)
            for (uint32_t cap : vals) {
                ++n;
                const lc::Range R = lc::clamp_range(a, b, cap);
                const int64_t first = a < cap ? a : cap, end = b < cap ? b : cap;
                int64_t count = end > first ? end - first : 0;
                if (b <= 9 || cap <= 9) {  // the members lie below 10: one by one
                    int64_t seen = 0;
                    for (uint32_t x = 0; x < 10; ++x)
                        if (a <= x && x < b && x < cap) ++seen;
                    if (seen != count) fail("the test's own two definitions", a, b, cap);
                }
                if (R.first != first || R.count != count) fail("clamp_range", a, b, cap);
                if ((uint64_t)R.first + R.count > cap) fail("clamp_range leaves the buffer", a, b, cap);
            }
    if (n != 12 * 12 * 12) fail("clamp_range cases", n, 0, 0);
}

int main() {
    check_copies();
    check_lines();
    check_clamp();
    fprintf(stderr, "ok: linecopy_host\n");
    return 0;
}
