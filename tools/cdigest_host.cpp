// Cache digests on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: the walk, the serial decoder, the
// image writer, SHA-256 and the checked frame walk of h2o_amd/csrc/hhuff_cdigest.h -- the code the kernels run.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ih2o_amd/csrc
//       tools/cdigest_host.cpp -o cdigest_host
//   ./cdigest_host CASES [ROUNDS]
//
// CASES: a text file (tests/test_cache_digests_host.py writes it from tests/golden/cache_digests.npz):
//   C                 a new case          V hex        load this header value
//   S p c n0 n1       h2o's digests != NULL, fresh.complete and frame counts        L kind hex state    a lookup's answer
// Every value, image and message lives in a heap block of exactly its size, so a read or write one byte outside is a
// report.
//   1. every case gives h2o's summary and lookup states, in a region of hhuff_cache_digests_bound and, with the same
//      bytes, in one of exactly the image's peak size; one byte less is HHUFF_CD_SPACE and a header-only image
//   2. every truncation of every value, and ROUNDS (default 300) byte mutations of each: loads end with status 0 or
//      HHUFF_CD_SPACE in regions of the bound and of random smaller sizes, and the image is one lookup() accepts
//   3. byte mutations and truncations of every image: lookup() answers a state or HHUFF_CD_EFORMAT
//   4. SHA-256 known answers at the padding edges, segments cut at every place
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "hhuff_cdigest.h"

using namespace hhuff::cd;

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
    explicit Heap(uint64_t n_) : p(new uint8_t[n_ ? n_ : 1]), n(n_) {}
    explicit Heap(const std::string& s) : Heap(s.size()) { memcpy(p.get(), s.data(), s.size()); }
};

struct HostSrc {
    const uint8_t* p;
    uint8_t byte(uint64_t i) const { return p[i]; }
    uint64_t skip_plain(uint64_t cur, uint64_t end) const {
        while (cur < end && !(p[cur] == ' ' || p[cur] == '\t' || p[cur] == ';' || p[cur] == ',' || p[cur] == '=')) ++cur;
        return cur;
    }
    uint32_t chunk(uint64_t pos, uint32_t rem, uint32_t* k) const {  // byte by byte: exactly the message's bytes are read
        const uint32_t n = 1u + rnd() % (rem < 4u ? rem : 4u);
        uint32_t w = 0;
        for (uint32_t i = 0; i < n; ++i) w |= (uint32_t)p[pos + i] << (24u - 8u * i);
        *k = n;
        return w;
    }
};

struct HostImage {
    const uint8_t* p;
    uint32_t word(uint64_t i) const {
        uint32_t w;
        memcpy(&w, p + 4u * i, 4);
        return w;
    }
    uint64_t key(uint64_t i) const {
        uint64_t k;
        memcpy(&k, p + 8u * i, 8);
        return k;
    }
};

typedef std::vector<std::string> Values;

// hhuff_cache_digests_load for one request into a block of exactly `size` bytes -> the status; *peak: the largest image
static int32_t load(const Values& vals, Heap& img, uint64_t* bytes, uint64_t* peak = nullptr) {
    memset(img.p.get(), 0xCD, img.n);
    ImageSink<HostSrc> K{nullptr, img.p.get(), img.n};
    if (peak) *peak = kHeaderBytes;
    for (const std::string& v : vals) {
        if (K.stopped()) break;
        const Heap text(v);
        const HostSrc S{text.p.get()};
        K.S = &S;
        load_value(S, 0, v.size(), K);
        if (peak && K.pos > *peak) *peak = K.pos;  // (a reset inside a value can hide a higher mark: check_case allows for it)
    }
    K.finish();
    *bytes = K.status == 0 ? K.pos : (img.n >= kHeaderBytes ? kHeaderBytes : 0);
    return K.status;
}

static uint64_t hash_of(const std::string& m, uint32_t cut) {
    const Heap text(m);
    const HostSrc S{text.p.get()};
    const uint32_t a = m.size() ? cut % (m.size() + 1) : 0, b = a + (m.size() - a) / 2;
    const uint32_t off[5] = {0, 0, a, 0, b}, len[5] = {a, 0, b - a, 0, (uint32_t)m.size() - b};
    SegWords<HostSrc> W(S, off, len);
    return sha256_first8(W, W.nwords / 16u);
}

static bool is_state(int32_t s) { return s == HHUFF_CD_UNKNOWN || s == HHUFF_CD_NOT_CACHED || s == HHUFF_CD_FRESH; }

struct Case {
    Values vals;
    int summary[4] = {0, 0, 0, 0};
    struct Look {
        uint32_t kind;
        std::string msg;
        int32_t state;
    };
    std::vector<Look> looks;
};

static std::string unhex(const std::string& h) {
    std::string s;
    for (size_t i = 0; i + 1 < h.size(); i += 2) s.push_back((char)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
    return s;
}

static void check_case(const Case& c, uint32_t rounds, uint64_t* nloads) {
    uint64_t total = 0;
    for (const std::string& v : c.vals) total += v.size();
    Heap big(hhuff_cache_digests_bound(total, c.vals.size()));
    uint64_t bytes, peak;
    REQUIRE(load(c.vals, big, &bytes, &peak) == 0 && bytes <= big.n && peak <= big.n);
    const HostImage M{big.p.get()};
    const uint32_t flags = M.word(1) >> 16;
    REQUIRE(M.word(0) == kMagic && (M.word(1) & 0xFFFFu) == kVersion && M.word(3) == bytes);
    REQUIRE((int)(flags & kPresent) == c.summary[0] && (!(flags & kPresent) || (int)((flags >> 1) & 1u) == c.summary[1]));
    uint32_t n[2] = {0, 0};
    for (uint64_t pos = kHeaderBytes, f = 0; f < M.word(2); ++f) {
        ++n[(M.word(pos / 4u) >> 8) & 1u];
        for (uint32_t k = 1; k < M.word(pos / 4u + 1u); ++k) REQUIRE(M.key(pos / 8u + 2u + k - 1u) < M.key(pos / 8u + 2u + k));
        pos += kFrameBytes + 8ull * M.word(pos / 4u + 1u);
    }
    REQUIRE(!(flags & kPresent) || ((int)n[0] == c.summary[2] && (int)n[1] == c.summary[3]));
    for (const Case::Look& L : c.looks) REQUIRE(lookup(M, bytes, L.kind, hash_of(L.msg, rnd())) == L.state);
    {  // a region of exactly the load's bytes; one less
        Heap exact(peak), less(peak - 1u);
        uint64_t b2;
        if (load(c.vals, exact, &b2) == 0) {  // (else a reset inside one value hid a higher mark)
            REQUIRE(b2 == bytes && memcmp(exact.p.get(), big.p.get(), bytes) == 0);
            REQUIRE(peak == kHeaderBytes || load(c.vals, less, &b2) == HHUFF_CD_SPACE);
        }
        REQUIRE(peak != kHeaderBytes || (load(c.vals, less, &b2) == HHUFF_CD_SPACE && b2 == 0));
    }
    // truncations and mutations of the values
    auto run = [&](const Values& vals) {
        Heap img(rnd() % 3u ? big.n : rnd() % (big.n + 1u));
        uint64_t b;
        const int32_t st = load(vals, img, &b);
        REQUIRE(st == 0 || st == HHUFF_CD_SPACE);
        REQUIRE(b <= img.n && (img.n < kHeaderBytes || is_state(lookup(HostImage{img.p.get()}, b, rnd() & 1u, rnd()))));
        ++*nloads;
    };
    for (size_t i = 0; i < c.vals.size(); ++i) {
        Values vals = c.vals;
        for (size_t cut = 0; cut < c.vals[i].size(); ++cut) vals[i] = c.vals[i].substr(0, cut), run(vals);
        for (uint32_t r = 0; r < rounds && !c.vals[i].empty(); ++r) {
            vals[i] = c.vals[i];
            for (uint32_t k = 0, nk = 1u + rnd() % 3u; k < nk; ++k)
                vals[i][rnd() % vals[i].size()] = rnd() % 2u ? (char)rnd() : " \t;,=AeLAcreset-_+/"[rnd() % 19u];
            run(vals);
        }
    }
    // damaged and cut-short images
    for (uint32_t r = 0; r < rounds; ++r) {
        Heap d(rnd() % 4u ? bytes : rnd() % (bytes + 1u));
        memcpy(d.p.get(), big.p.get(), d.n);
        for (uint32_t k = 0, nk = rnd() % 4u; k < nk && d.n; ++k) d.p.get()[rnd() % (rnd() % 2u && d.n > 32 ? 32 : d.n)] = (uint8_t)rnd();
        const int32_t st = lookup(HostImage{d.p.get()}, d.n, rnd() & 1u, (uint64_t)rnd() << 32 | rnd());
        REQUIRE(is_state(st) || st == HHUFF_CD_EFORMAT);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) {
        printf("usage: cdigest_host CASES [ROUNDS]\n");
        return 2;
    }
    const uint32_t rounds = argc > 2 ? (uint32_t)atoi(argv[2]) : 300u;
    // SHA-256 (FIPS 180-4 examples: "abc", the empty message, the 56-byte message)
    REQUIRE(hash_of("abc", 1) == 0xba7816bf8f01cfeaull && hash_of("", 0) == 0xe3b0c44298fc1c14ull);
    const std::string m56 = "abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq";
    for (uint32_t cut = 0; cut <= 56; ++cut) REQUIRE(hash_of(m56, cut) == 0x248d6a61d20638b8ull);
    REQUIRE(hash_of(std::string(1000, 'a'), 333) == 0x41edece42d63e8d9ull);
    std::vector<Case> cases;
    std::ifstream f(argv[1]);
    for (std::string line; std::getline(f, line);) {
        std::istringstream in(line);
        std::string op, hex;
        in >> op;
        if (op == "C") cases.emplace_back();
        REQUIRE(!cases.empty());
        Case& c = cases.back();
        if (op == "V") in >> hex, c.vals.push_back(unhex(hex));
        if (op == "S") in >> c.summary[0] >> c.summary[1] >> c.summary[2] >> c.summary[3];
        if (op == "L") {
            Case::Look L;
            in >> L.kind >> hex >> L.state;
            L.msg = unhex(hex);
            c.looks.push_back(L);
        }
    }
    REQUIRE(!cases.empty());
    uint64_t nloads = 0;
    for (const Case& c : cases) check_case(c, rounds, &nloads);
    printf("ok: cdigest_host, %zu cases, %llu loads\n", cases.size(), (unsigned long long)nloads);
    return 0;
}
