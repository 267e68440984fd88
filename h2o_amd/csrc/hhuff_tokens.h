// Token sets (include/hhuff.h (2j)): the table hhuff_tokens_build writes, its hash, its header check and the probe,
// for the device (hhuff_tokens.hip: one lane per string) and for the host (the builder below, and
// tools/tokens_host.cpp, which runs tok_find over built and damaged tables under AddressSanitizer and
// UndefinedBehaviorSanitizer).  Nothing else knows the layout.
//
// A table is [Header 32 B][nbuckets x u32][ntokens x Rec 8 B, padded to 16 B][names, each zero-padded to a dword]
// and zeros up to its recorded size, hhuff_tokens_table_size(ntokens, name_bytes):
//   Header  magic "HHTK", u16 version, u16 reserved (0), u32 ntokens, u32 size (the whole table, a multiple of 16),
//           u32 nbuckets (buckets_for(ntokens): the power of two >= 2 ntokens, at least 8), u32 max_probe, u32 seed,
//           u32 reserved (0)
//   bucket  0 = empty, else (hash >> 16) << 16 | (id + 1): open addressing, linear probing from hash & (nbuckets - 1).
//           The load is at most 1/2.  max_probe is the longest run any token of the set needs, found at build time
//           for the seed -- of kSeeds tried -- that makes it shortest.
//   Rec     {u32 user, u32 pos << 8 | len}: the caller's word; the name's dword position in the names area and its
//           length in bytes
// A lookup hashes the name's dwords (the last one masked to the name's bytes), reads at most max_probe buckets and
// stops at an empty one; a bucket whose 16 tag bits equal the hash's names the one candidate whose length and then
// whose stored dwords are compared.  No section offset is stored: view() derives them from ntokens and checks
// them against the size, and tok_find checks every index it takes from the table's bytes against the view, so a
// table of arbitrary bytes can give wrong ids but no read outside [table, table + size).
#ifndef HHUFF_TOKENS_H
#define HHUFF_TOKENS_H
#include <stdint.h>
#include <string.h>

#include "hhuff.h"

#if defined(__HIPCC__)
#define HHUFF_TOK_HD __host__ __device__ inline
#else
#define HHUFF_TOK_HD inline
#endif

#include <algorithm>
#include <vector>

namespace hhuff {
namespace tok {
constexpr uint32_t kMagic = 0x4B544848u;  // "HHTK"
constexpr uint32_t kVersion = 1;
constexpr uint32_t kMaxTokens = 4096, kMaxName = 255;
constexpr uint32_t kHeaderBytes = 32, kHeaderWords = 8;
constexpr uint32_t kMinBuckets = 8;
constexpr uint32_t kSeeds = 32;

struct Header {
    uint32_t magic;
    uint16_t version, reserved0;
    uint32_t ntokens, size, nbuckets, max_probe, seed, reserved1;
};
static_assert(sizeof(Header) == kHeaderBytes, "table header");

HHUFF_TOK_HD uint32_t buckets_for(uint32_t ntokens) {
    uint32_t nb = kMinBuckets;
    while (nb < 2u * ntokens) nb <<= 1;
    return nb;
}
HHUFF_TOK_HD uint32_t rec_words(uint32_t ntokens) { return (2u * ntokens + 3u) & ~3u; }  // the records, padded to 16 B

// hhuff_tokens_table_size: every name takes its bytes rounded up to a dword, so name_bytes + 3 ntokens covers the
// names whatever their lengths.  At most 32 + 32 KiB + 32 KiB + 258 x 4096 B.
HHUFF_TOK_HD uint64_t table_bytes(uint32_t ntokens, uint64_t name_bytes) {
    if (ntokens == 0 || ntokens > kMaxTokens || name_bytes < ntokens || name_bytes > (uint64_t)kMaxName * ntokens) return 0;
    const uint64_t names = (name_bytes + 3ull * ntokens + 15u) & ~15ull;
    return kHeaderBytes + 4ull * buckets_for(ntokens) + 4ull * rec_words(ntokens) + names;
}

// ---- the hash: one multiply per dword, a final avalanche; the seed and the length start it ----
HHUFF_TOK_HD uint32_t hash_start(uint32_t seed, uint32_t len) { return (seed + 1u) * 0x85EBCA6Bu ^ len * 0xC2B2AE35u; }
HHUFF_TOK_HD uint32_t hash_step(uint32_t h, uint32_t w) {
    h = (h ^ w) * 0x9E3779B1u;
    return h ^ (h >> 15);
}
HHUFF_TOK_HD uint32_t hash_end(uint32_t h) {
    h = (h ^ (h >> 16)) * 0x85EBCA6Bu;
    return h ^ (h >> 13);
}
// the bytes of a name's last dword that are the name's
HHUFF_TOK_HD uint32_t tail_mask(uint32_t len) { return 0xFFFFFFFFu >> (8u * ((0u - len) & 3u)); }

// A name is anything with a reader(): next() gives the name's little-endian dwords in order; the bytes of the last
// one past the name are whatever the source holds (tok_find masks them).
template <class Name>
HHUFF_TOK_HD uint32_t hash_name(const Name& nm, uint32_t len, uint32_t seed) {
    const uint32_t ndw = (len + 3u) >> 2;
    uint32_t h = hash_start(seed, len);
    auto rd = nm.reader();
    for (uint32_t k = 0; k + 1u < ndw; ++k) h = hash_step(h, rd.next());
    return hash_end(hash_step(h, rd.next() & tail_mask(len)));
}

// a name in memory the reader may touch byte by byte only (the host: exactly the name's bytes are read)
struct BytesName {
    const uint8_t* p;
    uint32_t len;
    struct Reader {
        const uint8_t* p;
        uint32_t left;
        HHUFF_TOK_HD uint32_t next() {
            uint32_t w = 0;
            const uint32_t m = left < 4u ? left : 4u;
            for (uint32_t k = 0; k < m; ++k) w |= (uint32_t)p[k] << (8u * k);
            p += m, left -= m;
            return w;
        }
    };
    HHUFF_TOK_HD Reader reader() const { return Reader{p, len}; }
};

// a table in memory: word(i) = its i-th little-endian dword (the host copy is read with memcpy: any alignment)
struct MemTable {
    const uint8_t* p;
    HHUFF_TOK_HD uint32_t word(uint32_t i) const {
        uint32_t w;
        memcpy(&w, p + 4ull * i, 4);
        return w;
    }
};

// what a checked header says: everything tok_find needs, every section inside the size
struct View {
    uint32_t ntokens, mask, max_probe, seed;
    uint32_t rec_dw, names_dw, names_ndw;  // dword positions of the records and the names; dwords of names
};

// The header check: false = not a table hhuff_tokens_build wrote for this table_size (HHUFF_TOK_EFORMAT).  Reads
// the first 32 bytes only, and only when table_size holds them.
template <class Tab>
HHUFF_TOK_HD bool view(const Tab& T, uint64_t table_size, View& v) {
    if (table_size < kHeaderBytes || (table_size & 15u) != 0) return false;
    const uint32_t w1 = T.word(1), nt = T.word(2), size = T.word(3), nb = T.word(4), mp = T.word(5);
    if (T.word(0) != kMagic || w1 != kVersion /* reserved0 == 0 too */ || T.word(7) != 0) return false;
    if (nt == 0 || nt > kMaxTokens || size != table_size) return false;
    if (nb != buckets_for(nt) || mp == 0 || mp > nb) return false;
    v.ntokens = nt, v.mask = nb - 1u, v.max_probe = mp, v.seed = T.word(6);
    v.rec_dw = kHeaderWords + nb;
    v.names_dw = v.rec_dw + rec_words(nt);
    if (4ull * v.names_dw > size) return false;
    v.names_ndw = size / 4u - v.names_dw;
    return true;
}

// The probe.  -> the token's id and *user = its word, or HHUFF_TOK_NONE with *user untouched.
template <class Tab, class Name>
HHUFF_TOK_HD int32_t tok_find(const Tab& T, const View& v, const Name& nm, uint32_t len, uint32_t* user) {
    if (len == 0 || len > kMaxName) return HHUFF_TOK_NONE;
    const uint32_t ndw = (len + 3u) >> 2, tm = tail_mask(len);
    const uint32_t h = hash_name(nm, len, v.seed);
    for (uint32_t p = 0; p < v.max_probe; ++p) {
        const uint32_t e = T.word(kHeaderWords + ((h + p) & v.mask));
        if (e == 0) return HHUFF_TOK_NONE;
        if (((e ^ h) >> 16) != 0) continue;
        const uint32_t id = (e & 0xFFFFu) - 1u;
        if (id >= v.ntokens) continue;  // (a damaged bucket)
        const uint32_t pl = T.word(v.rec_dw + 2u * id + 1u), pos = pl >> 8;
        if ((pl & 0xFFu) != len || pos > v.names_ndw || ndw > v.names_ndw - pos) continue;
        auto rd = nm.reader();
        uint32_t diff = 0;
        for (uint32_t k = 0; k + 1u < ndw; ++k) diff |= rd.next() ^ T.word(v.names_dw + pos + k);
        diff |= (rd.next() & tm) ^ T.word(v.names_dw + pos + ndw - 1u);
        if (diff == 0) {
            *user = T.word(v.rec_dw + 2u * id);
            return (int32_t)id;
        }
    }
    return HHUFF_TOK_NONE;
}

// header check and probe in one: the host's whole lookup (-> [-2, ntokens))
HHUFF_TOK_HD int32_t tok_find(const void* table, uint64_t table_size, const uint8_t* name, uint32_t len, uint32_t* user) {
    const MemTable T{(const uint8_t*)table};
    View v;
    if (!view(T, table_size, v)) return HHUFF_TOK_EFORMAT;
    return tok_find(T, v, BytesName{name, len}, len, user);
}

// hhuff_tokens_build.  Host memory only; `table` is written only when the whole table is made.
inline int build(const uint8_t* names, const uint32_t* name_off, uint32_t ntokens, const uint32_t* user, void* table,
                 uint64_t table_size) {
    if (!names || !name_off || !table || ntokens == 0 || ntokens > kMaxTokens) return HHUFF_EINVAL;
    for (uint32_t i = 0; i < ntokens; ++i) {
        if (name_off[i + 1] < name_off[i]) return HHUFF_EINVAL;
        const uint32_t len = name_off[i + 1] - name_off[i];
        if (len == 0 || len > kMaxName) return HHUFF_EINVAL;
    }
    const uint64_t need = table_bytes(ntokens, name_off[ntokens] - name_off[0]);
    if (need == 0 || table_size < need) return HHUFF_EINVAL;
    auto nm = [&](uint32_t i) { return names + name_off[i]; };
    auto ln = [&](uint32_t i) { return name_off[i + 1] - name_off[i]; };
    {  // two equal names: sort by length, then bytes, and look at the neighbours
        std::vector<uint32_t> ord(ntokens);
        for (uint32_t i = 0; i < ntokens; ++i) ord[i] = i;
        auto cmp = [&](uint32_t a, uint32_t b) { return ln(a) != ln(b) ? (ln(a) < ln(b) ? -1 : 1) : memcmp(nm(a), nm(b), ln(a)); };
        std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return cmp(a, b) < 0; });
        for (uint32_t i = 0; i + 1 < ntokens; ++i)
            if (cmp(ord[i], ord[i + 1]) == 0) return HHUFF_EINVAL;
    }
    const uint32_t nb = buckets_for(ntokens);
    std::vector<uint32_t> t(need / 4u, 0u);
    const uint32_t rec_dw = kHeaderWords + nb, names_dw = rec_dw + rec_words(ntokens);
    uint32_t pos = 0;
    for (uint32_t i = 0; i < ntokens; ++i) {
        t[rec_dw + 2u * i] = user ? user[i] : 0u;
        t[rec_dw + 2u * i + 1u] = pos << 8 | ln(i);
        for (uint32_t k = 0; k < ln(i); ++k) t[names_dw + pos + (k >> 2)] |= (uint32_t)nm(i)[k] << (8u * (k & 3u));
        pos += (ln(i) + 3u) >> 2;
    }
    std::vector<uint32_t> bk(nb), best;
    uint32_t best_probe = 0, best_seed = 0;
    for (uint32_t seed = 0; seed < kSeeds; ++seed) {
        std::fill(bk.begin(), bk.end(), 0u);
        uint32_t longest = 0;
        for (uint32_t i = 0; i < ntokens; ++i) {
            const uint32_t h = hash_name(BytesName{nm(i), ln(i)}, ln(i), seed);
            uint32_t p = 0;
            while (bk[(h + p) & (nb - 1u)] != 0) ++p;  // (the load is at most 1/2: there is an empty bucket)
            bk[(h + p) & (nb - 1u)] = (h & 0xFFFF0000u) | (i + 1u);
            longest = std::max(longest, p + 1u);
        }
        if (best.empty() || longest < best_probe) best = bk, best_probe = longest, best_seed = seed;
    }
    std::copy(best.begin(), best.end(), t.begin() + kHeaderWords);
    const Header h{kMagic, (uint16_t)kVersion, 0, ntokens, (uint32_t)need, nb, best_probe, best_seed, 0};
    memcpy(t.data(), &h, sizeof(h));
    memcpy(table, t.data(), need);
    return HHUFF_OK;
}
}  // namespace tok
}  // namespace hhuff
#endif
