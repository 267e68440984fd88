// Token tables on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: the builder and the probe of
// h2o_amd/csrc/hhuff_tokens.h -- the code the kernel runs -- over built and damaged tables.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ih2o_amd/csrc
//       tools/tokens_host.cpp -o tokens_host
//   ./tokens_host NAMES [ROUNDS]
//
// NAMES: a text file, one name a line (tests/test_tokens_host.py writes the fixture's 85).  Every table and every
// probe string lives in a heap block of exactly its size, so a read one byte outside is a report.
//   1. sets of 1, 2, the file's and 4096 names, names of 1 and 255 bytes, sets built to collide (equal length and
//      last byte; equal first dword): every name finds its id and word; every name with a byte changed, dropped or
//      appended, upper-cased, and every proper prefix gives what a std::map gives
//   2. every refusal of the builder leaves the table untouched; two builds are byte-equal; the size function
//   3. tables with each header field changed, with random bytes changed (ROUNDS tables a set, default 2000) and cut
//      short: no access outside the block, a result in [-2, ntokens)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "hhuff_tokens.h"

using namespace hhuff::tok;
typedef std::vector<std::string> Names;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 16);
}

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) {                                                       \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);         \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

struct Heap {  // a block of exactly n bytes
    std::unique_ptr<uint8_t[]> p;
    uint64_t n;
    explicit Heap(uint64_t n_) : p(new uint8_t[n_ ? n_ : 1]), n(n_) {}
};

static int32_t find(const Heap& t, uint64_t size, const std::string& s, uint32_t* user) {
    Heap name(s.size());  // exactly the name's bytes
    memcpy(name.p.get(), s.data(), s.size());
    return tok_find(t.p.get(), size, name.p.get(), (uint32_t)s.size(), user);
}

struct Packed {
    std::vector<uint8_t> blob;
    std::vector<uint32_t> off, user;
};
static Packed pack(const Names& names) {
    Packed k;
    k.off.push_back(0);
    for (size_t i = 0; i < names.size(); ++i) {
        k.blob.insert(k.blob.end(), names[i].begin(), names[i].end());
        k.off.push_back((uint32_t)k.blob.size());
        k.user.push_back(0xA0000000u + 7u * (uint32_t)i);
    }
    if (k.blob.empty()) k.blob.push_back(0);
    return k;
}

static Heap build_set(const Names& names) {
    const Packed k = pack(names);
    const uint64_t size = table_bytes((uint32_t)names.size(), k.off.back());
    REQUIRE(size != 0 && size % 16 == 0);
    Heap t(size), t2(size);
    memset(t.p.get(), 0xCD, size), memset(t2.p.get(), 0x11, size);
    REQUIRE(build(k.blob.data(), k.off.data(), (uint32_t)names.size(), k.user.data(), t.p.get(), size) == HHUFF_OK);
    REQUIRE(build(k.blob.data(), k.off.data(), (uint32_t)names.size(), k.user.data(), t2.p.get(), size) == HHUFF_OK);
    REQUIRE(memcmp(t.p.get(), t2.p.get(), size) == 0);  // deterministic, every byte written
    return t;
}

static Names probes_of(const Names& names, size_t cap) {
    Names out;
    const size_t step = names.size() > cap ? names.size() / cap : 1;
    for (size_t i = 0; i < names.size(); i += step) {
        const std::string& nm = names[i];
        for (size_t j = 0; j < nm.size(); j += nm.size() > 40 ? 17 : 1) {
            std::string c = nm, d = nm;
            c[j] = (char)(c[j] + 1 + rnd() % 255);
            d.erase(j, 1);
            out.push_back(c);
            out.push_back(d);
            if (j) out.push_back(nm.substr(0, j));
        }
        out.push_back(nm + (char)rnd());
        std::string u = nm;
        for (char& ch : u)
            if (ch >= 'a' && ch <= 'z') ch = (char)(ch - 32);
        out.push_back(u);
    }
    out.push_back(std::string());
    out.push_back(std::string(256, 'a'));
    return out;
}

static void check_set(const char* what, const Names& names, uint32_t rounds) {
    const Heap t = build_set(names);
    const int32_t nt = (int32_t)names.size();
    std::map<std::string, int32_t> model;
    for (int32_t i = 0; i < nt; ++i) model[names[i]] = i;
    for (int32_t i = 0; i < nt; ++i) {
        uint32_t user = 1;
        REQUIRE(find(t, t.n, names[i], &user) == i);
        REQUIRE(user == 0xA0000000u + 7u * (uint32_t)i);
    }
    const Names probes = probes_of(names, 200);
    for (const std::string& s : probes) {
        uint32_t user = 0x55;
        const auto it = model.find(s);
        const int32_t want = it == model.end() || s.empty() || s.size() > 255 ? HHUFF_TOK_NONE : it->second;
        REQUIRE(find(t, t.n, s, &user) == want);
        REQUIRE(want >= 0 || user == 0x55);
    }
    // ---- damaged tables: only "no access outside, a result in [-2, ntokens)" ----
    auto run = [&](const Heap& d, uint64_t size) {
        uint32_t user, hn;
        memcpy(&hn, d.p.get() + 8, 4);  // a result is below the ntokens the (changed) header states
        const int32_t nt = hn >= 1 && hn <= kMaxTokens ? (int32_t)hn : (int32_t)names.size();
        for (size_t k = 0; k < 6; ++k) {
            const int32_t r = find(d, size, names[rnd() % names.size()], &user);
            REQUIRE(r >= HHUFF_TOK_EFORMAT && r < nt);
        }
        for (size_t k = 0; k < 4; ++k) {
            const int32_t r = find(d, size, probes[rnd() % probes.size()], &user);
            REQUIRE(r >= HHUFF_TOK_EFORMAT && r < nt);
        }
    };
    uint32_t refused = 0;
    for (uint32_t w = 0; w < kHeaderWords; ++w) {  // each header field
        uint32_t orig;
        memcpy(&orig, t.p.get() + 4 * w, 4);
        const uint32_t vals[] = {0u, 1u, orig + 1u, orig - 1u, orig ^ 0x80000000u, orig << 1, 0xFFFFFFFFu, 4096u, 4097u, rnd()};
        for (uint32_t v : vals) {
            if (v == orig) continue;
            Heap d(t.n);
            memcpy(d.p.get(), t.p.get(), t.n);
            memcpy(d.p.get() + 4 * w, &v, 4);
            uint32_t user;
            if (find(d, d.n, names[0], &user) == HHUFF_TOK_EFORMAT) ++refused;
            else REQUIRE(w == 2 || w == 5 || w == 6);  // ntokens within its bucket count, max_probe, seed: only wrong ids
            run(d, d.n);
        }
    }
    REQUIRE(refused >= 5 * 7);  // magic, version, size, nbuckets, the reserved word: every change refused
    for (uint32_t r = 0; r < rounds; ++r) {  // random bytes, mostly where the indices live
        Heap d(t.n);
        memcpy(d.p.get(), t.p.get(), t.n);
        const uint32_t nchg = 1u + rnd() % 8u;
        for (uint32_t c = 0; c < nchg; ++c) {
            const uint64_t span = rnd() % 4u == 0 ? t.n : (rnd() % 2u ? kHeaderBytes : kHeaderBytes + 4ull * buckets_for((uint32_t)nt) + 8ull * nt);
            d.p.get()[rnd() % (span < t.n ? span : t.n)] = (uint8_t)rnd();
        }
        run(d, d.n);
    }
    {  // cut short: a block and a table_size 16 below the recorded size
        Heap d(t.n - 16);
        memcpy(d.p.get(), t.p.get(), t.n - 16);
        uint32_t user;
        REQUIRE(find(d, d.n, names[0], &user) == HHUFF_TOK_EFORMAT);
        REQUIRE(find(t, 16, names[0], &user) == HHUFF_TOK_EFORMAT && find(t, t.n - 1, names[0], &user) == HHUFF_TOK_EFORMAT);
    }
    Header h;
    memcpy(&h, t.p.get(), sizeof(h));
    printf("  %-28s %5d names, table %7llu B, max_probe %u (seed %u)\n", what, nt, (unsigned long long)t.n, h.max_probe, h.seed);
}

static void refusals() {
    const Names names = {"alpha", "beta", "gamma"};
    Packed k = pack(names);
    const uint64_t size = table_bytes(3, k.off.back());
    Heap t(size);
    auto untouched = [&](int rc) {
        REQUIRE(rc == HHUFF_EINVAL);
        for (uint64_t i = 0; i < size; ++i) REQUIRE(t.p.get()[i] == 0xCD);
    };
    memset(t.p.get(), 0xCD, size);
    untouched(build(k.blob.data(), k.off.data(), 3, nullptr, t.p.get(), size - 1));  // table_size below the need
    untouched(build(k.blob.data(), k.off.data(), 0, nullptr, t.p.get(), size));
    untouched(build(nullptr, k.off.data(), 3, nullptr, t.p.get(), size));
    untouched(build(k.blob.data(), nullptr, 3, nullptr, t.p.get(), size));
    REQUIRE(build(k.blob.data(), k.off.data(), 3, nullptr, nullptr, size) == HHUFF_EINVAL);
    {
        std::vector<uint32_t> off = k.off;
        off[2] = off[1];  // an empty name
        untouched(build(k.blob.data(), off.data(), 3, nullptr, t.p.get(), size));
        off = k.off, off[2] = off[1] - 1;  // a decreasing name_off
        untouched(build(k.blob.data(), off.data(), 3, nullptr, t.p.get(), size));
    }
    {
        const Packed d = pack({"alpha", "beta", "alpha"});  // two equal names
        untouched(build(d.blob.data(), d.off.data(), 3, nullptr, t.p.get(), size + 64));
        const Packed l = pack({std::string(256, 'x')});  // a name over 255 bytes
        untouched(build(l.blob.data(), l.off.data(), 1, nullptr, t.p.get(), size));
        Names many(4097);
        for (size_t i = 0; i < many.size(); ++i) many[i] = "n" + std::to_string(i);
        const Packed m = pack(many);
        untouched(build(m.blob.data(), m.off.data(), 4097, nullptr, t.p.get(), size));
    }
    REQUIRE(build(k.blob.data(), k.off.data(), 3, nullptr, t.p.get(), size) == HHUFF_OK);  // user NULL: all 0
    uint32_t user = 9;
    REQUIRE(tok_find(t.p.get(), size, (const uint8_t*)"beta", 4, &user) == 1 && user == 0);
    REQUIRE(table_bytes(0, 0) == 0 && table_bytes(4097, 4097) == 0 && table_bytes(3, 2) == 0 && table_bytes(3, 3 * 255 + 1) == 0);
    REQUIRE(table_bytes(1, 1) != 0 && table_bytes(4096, 4096ull * 255) != 0);
}

int main(int argc, char** argv) {
    if (argc < 2) {
        printf("usage: tokens_host NAMES [ROUNDS]\n");
        return 2;
    }
    Names file;
    {
        std::ifstream f(argv[1]);
        for (std::string line; std::getline(f, line);)
            if (!line.empty()) file.push_back(line);
    }
    REQUIRE(!file.empty());
    const uint32_t rounds = argc > 2 ? (uint32_t)atoi(argv[2]) : 2000u;
    refusals();
    check_set("one name", {"x"}, rounds);
    check_set("two names", {"a", "ab"}, rounds);
    check_set("the file's names", file, rounds);
    {
        Names edge = {"q", std::string(255, 'z')};  // 1 and 255 bytes
        for (int i = 0; i < 30; ++i) {
            std::string s(255, 'z');
            s[(size_t)(rnd() % 255)] = (char)('a' + i % 25), s[254] = (char)('A' + i);
            edge.push_back(s);
        }
        for (int c = 1; c < 256; ++c)
            if (c != 'q') edge.push_back(std::string(1, (char)c));  // every one-byte name
        check_set("1 and 255 bytes", edge, rounds);
    }
    {
        Names a, b;  // equal length and last byte; equal first dword
        for (int i = 0; i < 600; ++i) {
            char buf[32];
            snprintf(buf, sizeof(buf), "%04d-collide-x", i);
            a.push_back(buf);
            snprintf(buf, sizeof(buf), "x-co%d", i);
            b.push_back(buf);
            b.push_back(std::string("x-co") + std::string((size_t)(i % 40) + 1, (char)('a' + i / 40)));
        }
        check_set("equal length and last byte", a, rounds);
        check_set("equal first dword", b, rounds);
    }
    {
        Names big;  // 4096 names, lengths 1..255
        for (int i = 0; i < 4096; ++i) {
            std::string s = "h" + std::to_string(i) + "-";
            const size_t len = i < 250 ? (size_t)i + 6 : 6 + rnd() % 30;
            while (s.size() < len) s.push_back((char)('a' + rnd() % 26));
            big.push_back(s);
        }
        check_set("4096 names", big, rounds / 4);
    }
    printf("ok: tokens_host\n");
    return 0;
}
