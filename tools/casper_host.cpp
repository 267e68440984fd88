// CASPER on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: the slab check, SHA-1, the serial set
// operations, the serial Golomb decoder and encoder and the base64url writer of h2o_amd/csrc/hhuff_casper.h -- the code
// the kernel runs or must equal.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ih2o_amd/csrc
//       tools/casper_host.cpp -o casper_host
//   ./casper_host CASES [ROUNDS]
//
// CASES: a text file (tests/test_casper_host.py writes it from tests/golden/casper.npz), a line an op:
//   N                                       a new case: a slab of zeros
//   kind a b|hex  ret entries x<cookie hex>    the op (INIT: a b; else the string) and h2o's answers after it
// Every slab, string and region lives in a heap block of exactly its size, so a read or write one byte outside is a
// report.
//   1. every op gives h2o's return value and entry count, and a COOKIE op behind it h2o's cookie in a region of exactly
//      its length; one byte less is HHUFF_CSP_SPACE with nothing written
//   2. every truncation of every cookie value and ROUNDS (default 200) byte mutations of each, consumed into a copy of
//      the slab at max_keys and at a small max_keys: status 0 or HHUFF_CSP_SPACE, and the set stays ascending
//   3. byte mutations and truncated key counts of every slab: ops answer a status this library knows, inside the blocks
//   4. SHA-1 known answers at the padding edges
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "hhuff_casper.h"

using namespace hhuff::csp;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 16);
}

#define REQUIRE(c)                                                \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                              \
        }                                                         \
    } while (0)

struct Heap {  // a block of exactly n bytes
    std::unique_ptr<uint8_t[]> p;
    uint64_t n;
    explicit Heap(uint64_t n_) : p(new uint8_t[n_ ? n_ : 1]), n(n_) { memset(p.get(), 0, n); }
    explicit Heap(const std::string& s) : Heap(s.size()) { memcpy(p.get(), s.data(), s.size()); }
};

struct HostSrc {
    const uint8_t* p;
    uint8_t byte(uint64_t i) const { return p[i]; }
    uint32_t chunk(uint64_t pos, uint32_t rem, uint32_t* k) const {  // byte by byte: exactly the message's bytes are read
        const uint32_t n = 1u + rnd() % (rem < 4u ? rem : 4u);
        uint32_t w = 0;
        for (uint32_t i = 0; i < n; ++i) w |= (uint32_t)p[pos + i] << (24u - 8u * i);
        *k = n;
        return w;
    }
};

constexpr uint32_t kMaxKeys = 320;
static const Fields kNoFields{nullptr, nullptr, nullptr, 0, 0};

struct Result {
    int32_t status;
    uint32_t value, nkeys, at;
    std::string out;
};

// one op on the slab (max_keys of it) with the string `text` as `in` and a region of `room` bytes
static Result run(Heap& slab, uint32_t max_keys, uint32_t kind, uint32_t a, uint32_t b, const std::string& text, uint32_t room) {
    const Heap in(text), tmp(8ull * 3u * max_keys);
    Heap out(room);
    memset(out.p.get(), 0xCD, room);
    const HostSrc S{in.p.get()};
    Serial<HostSrc> K{S, text.size(), slab.p.get(), max_keys, reinterpret_cast<uint64_t*>(tmp.p.get()), out.p.get(), 0, room};
    K.load();
    uint32_t r[4];
    K.op(kind, a, b, 0, false, kNoFields, r);
    K.store();
    REQUIRE(K.wpos <= room && (r[0] == 0 || K.wpos == 0));
    for (uint32_t i = K.wpos; i < room; ++i) REQUIRE(out.p.get()[i] == 0xCD);
    return Result{(int32_t)r[0], r[1], r[2], r[3], std::string((const char*)out.p.get(), K.wpos)};
}

static bool ascending(const Heap& slab) {
    uint32_t n;
    memcpy(&n, slab.p.get() + 8, 4);
    const uint64_t* k = reinterpret_cast<const uint64_t*>(slab.p.get() + 16);
    for (uint32_t i = 1; i < n; ++i)
        if (k[i - 1] >= k[i]) return false;
    return true;
}

static bool known(int32_t s) { return s == 0 || s == HHUFF_CSP_SPACE || s == HHUFF_CSP_EINVAL || s == HHUFF_CSP_EFORMAT; }

static std::string unhex(const std::string& h) {
    std::string s;
    for (size_t i = 0; i + 1 < h.size(); i += 2) s.push_back((char)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
    return s;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        printf("usage: casper_host CASES [ROUNDS]\n");
        return 2;
    }
    const uint32_t rounds = argc > 2 ? (uint32_t)atoi(argv[2]) : 200u;
    {  // SHA-1 (FIPS 180-4 examples; h2o's t/00unit/lib/http2/casper.c): the first four bytes, little endian
        auto key = [](const std::string& m) {
            const Heap text(m);
            return path_key(HostSrc{text.p.get()}, 0, (uint32_t)m.size());
        };
        REQUIRE(key("abc") == 0x363e99a9u && key("") == 0xeea339dau && key("/index.html") == 0x5945fe14u);
        REQUIRE(key("abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq") == 0x443e9884u);
        REQUIRE(key(std::string(1000000, 'a')) == 0x3c97aa34u);
    }
    std::ifstream f(argv[1]);
    std::unique_ptr<Heap> slab;
    uint64_t nops = 0, ncases = 0, nruns = 0;
    for (std::string line; std::getline(f, line);) {
        std::istringstream ls(line);
        std::string first, hex, cookie;
        ls >> first;
        if (first == "N") {
            slab.reset(new Heap(slab_bytes(kMaxKeys)));
            ++ncases;
            continue;
        }
        REQUIRE(slab);
        const uint32_t kind = (uint32_t)atoi(first.c_str());
        uint32_t a = 0, b = 0, ret, entries;
        std::string text;
        if (kind == HHUFF_CSP_INIT) ls >> a >> b;
        else if (kind != HHUFF_CSP_COOKIE) ls >> hex, text = unhex(hex.substr(1)), b = (uint32_t)text.size();
        ls >> ret >> entries >> cookie;
        cookie = unhex(cookie.substr(1));
        const Heap before = [&] {
            Heap c(slab->n);
            memcpy(c.p.get(), slab->p.get(), c.n);
            return c;
        }();
        if (kind != HHUFF_CSP_COOKIE) {
            const Result r = run(*slab, kMaxKeys, kind, a, b, text, 0);
            REQUIRE(r.status == 0 && r.nkeys == entries && ascending(*slab));
            REQUIRE(kind == HHUFF_CSP_CONSUME || kind == HHUFF_CSP_INIT || r.value == ret);
        }
        // 1. the cookie, in an exact region and in one a byte short
        const Result c = run(*slab, kMaxKeys, HHUFF_CSP_COOKIE, 0, 0, "", (uint32_t)cookie.size());
        REQUIRE(c.status == 0 && c.value == cookie.size() && c.out == cookie && c.nkeys == entries);
        if (!cookie.empty()) REQUIRE(run(*slab, kMaxKeys, HHUFF_CSP_COOKIE, 0, 0, "", (uint32_t)cookie.size() - 1u).status == HHUFF_CSP_SPACE);
        ++nops;
        // 2. cut and damaged cookie values, into a copy of the slab as it was; also read as a slab of fewer keys
        if (kind == HHUFF_CSP_CONSUME) {
            auto consume = [&](const std::string& v) {
                Heap s(before.n);
                memcpy(s.p.get(), before.p.get(), s.n);
                const Result r = run(s, kMaxKeys, kind, 0, (uint32_t)v.size(), v, 0);
                REQUIRE((r.status == 0 || r.status == HHUFF_CSP_SPACE) && ascending(s) && r.nkeys <= kMaxKeys);
                REQUIRE(r.status == 0 || memcmp(s.p.get(), before.p.get(), s.n) == 0);
                const uint32_t small = 1u + rnd() % 40u;
                Heap t(slab_bytes(small));
                REQUIRE(run(t, small, HHUFF_CSP_INIT, 1u + rnd() % 30u, rnd() % 32u, "", 0).status == 0);
                const Result q = run(t, small, kind, 0, (uint32_t)v.size(), v, 0);
                REQUIRE((q.status == 0 || q.status == HHUFF_CSP_SPACE) && ascending(t) && q.nkeys <= small);
                nruns += 2;
            };
            for (size_t cut = 0; cut < text.size(); ++cut) consume(text.substr(0, cut));
            for (uint32_t r = 0; r < rounds; ++r) {
                std::string v = text;
                for (uint32_t k = 0, nk = 1u + rnd() % 3u; k < nk && !v.empty(); ++k)
                    v[rnd() % v.size()] = rnd() % 2u ? (char)rnd() : "AB-_+/;= 019az"[rnd() % 14u];
                consume(v);
            }
        }
        // 3. damaged slabs: any byte of the header, some of the keys
        for (uint32_t r = 0; r < rounds / 4u; ++r) {
            Heap s(slab->n);
            memcpy(s.p.get(), slab->p.get(), s.n);
            for (uint32_t k = 0, nk = 1u + rnd() % 3u; k < nk; ++k) s.p.get()[rnd() % (rnd() % 2u ? 16u : (uint32_t)s.n)] = (uint8_t)rnd();
            const uint32_t kinds[4] = {HHUFF_CSP_LOOKUP, HHUFF_CSP_MARK, HHUFF_CSP_COOKIE, HHUFF_CSP_CONSUME};
            const std::string v = kind == HHUFF_CSP_INIT || kind == HHUFF_CSP_COOKIE ? std::string("h2o_casper=AeLA") : text;
            const Result q = run(s, kMaxKeys, kinds[rnd() % 4u], 0, (uint32_t)v.size(), v, rnd() % 600u);
            REQUIRE(known(q.status) && q.nkeys <= kMaxKeys);
            ++nruns;
        }
    }
    REQUIRE(ncases != 0);
    printf("ok: casper_host, %llu cases, %llu ops, %llu runs\n", (unsigned long long)ncases, (unsigned long long)nops,
           (unsigned long long)nruns);
    return 0;
}
