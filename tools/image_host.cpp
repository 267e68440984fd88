// Connection images (h2o_amd/csrc/hhuff_image.h: the slab layouts, the image format, its validator, img_pack /
// img_unpack) on the host, for AddressSanitizer and UndefinedBehaviorSanitizer.  Every scratch is a heap block of
// exactly nslots slabs and every image a heap block of exactly its length, so a step outside them is reported.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ih2o_amd/csrc
//       tools/image_host.cpp -o build/image_host && build/image_host 300
//
// Per family and round: a random valid slab in a random slot -- entry rings that start anywhere and wrap, bytes in
// either ring, evicted prefixes, full inflight and parked lists, empty tables -- is packed, unpacked into another
// slot of another scratch and packed again: the two images are the same bytes (the canonical form), and so is the
// image of the same connection built with another ring history.  Then mutants of the image -- header fields, counts,
// lengths, random bytes -- go through img_unpack: each is refused with the slab untouched, or unpacked and packed
// again, all inside the blocks.  The run fails unless every family saw a wrapped ring (or a full list), an empty
// table, refusals of both kinds and a mutant that was accepted.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <random>
#include <vector>

#include "hhuff_image.h"

using namespace hhuff;
using namespace hhuff::img;

namespace {
#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            printf("FAIL %s:%d: %s (family %u round %u)\n", __FILE__, __LINE__, #c, g_fam, g_round); \
            exit(1);                                                                      \
        }                                                                                 \
    } while (0)
unsigned g_fam = 0, g_round = 0;
std::mt19937 rng(12345);
uint32_t rnd(uint32_t n) { return n ? (uint32_t)(rng() % n) : 0u; }

struct Block {  // an exact heap block, 16-byte aligned
    uint8_t* p;
    size_t n;
    explicit Block(size_t bytes, int fill = 0xC3) : p((uint8_t*)aligned_alloc(16, bytes ? (bytes + 15) & ~(size_t)15 : 16)), n(bytes) {
        memset(p, fill, bytes ? (bytes + 15) & ~(size_t)15 : 16);
    }
    ~Block() { free(p); }
    Block(const Block&) = delete;
};

struct Ent {
    std::vector<uint8_t> name, value;
    uint32_t a, b, c;
};
struct Conn {  // a connection, layout-free
    std::vector<Ent> ent;  // oldest first
    std::vector<QeInflight> inf;
    std::vector<QpEntry> parked;
    uint32_t failed = 0, lkr = 0, num_blocked = 0, evicted = 0;
    uint64_t cap = 0, counter = 0;
};

Conn random_conn(const Layout& L) {
    Conn c;
    const uint32_t fam = L.family;
    if (fam == HHUFF_FAM_QPACK_DSESSION) {
        const uint32_t n = rnd(4) == 0 ? L.L : rnd(3) == 0 ? 0u : rnd(L.L + 1);
        for (uint32_t i = 0; i < n; ++i) c.parked.push_back(QpEntry{4ull * rng(), rng() % 1000u});
        c.counter = rng();
        return c;
    }
    c.cap = rnd(4) == 0 ? rnd((uint32_t)L.cap_max + 1) : L.cap_max;
    if (fam == HHUFF_FAM_QPACK_ENC) c.cap = L.T;
    uint64_t size = 0;
    const uint32_t want = rnd(5) == 0 ? 0u : rnd(L.E + 1);
    while (c.ent.size() < want) {
        Ent e;
        e.name.resize(rnd(3) == 0 ? 0 : rnd(24));
        e.value.resize(rnd(3) == 0 ? 0 : rnd(90));
        if (size + e.name.size() + e.value.size() + 32 > c.cap) break;
        for (auto& x : e.name) x = (uint8_t)rng();
        for (auto& x : e.value) x = (uint8_t)rng();
        e.a = fam == HHUFF_FAM_HPACK_DEC || fam == HHUFF_FAM_QPACK_DEC ? rnd(4) : (uint32_t)rng();
        e.b = fam == HHUFF_FAM_HPACK_ENC || fam == HHUFF_FAM_QPACK_ENC ? (uint32_t)rng() : 0u;
        e.c = fam == HHUFF_FAM_HPACK_ENC ? rnd(2) : 0u;
        size += e.name.size() + e.value.size() + 32;
        c.ent.push_back(e);
    }
    c.failed = rnd(8) == 0;
    if (fam == HHUFF_FAM_QPACK_DEC) c.counter = c.ent.size() + rnd(1000);
    if (fam == HHUFF_FAM_QPACK_ENC) {
        const bool ev = rnd(2);
        c.failed |= ev ? kQeEvicting | (rnd(2) ? kQeDuplicating : 0u) : 0u;
        c.evicted = ev ? rnd(3 * L.E + 1) : 0u;
        c.counter = c.evicted + c.ent.size();
        c.lkr = rnd((uint32_t)c.counter + 1);
        const uint32_t n = rnd(4) == 0 ? L.L : rnd(3) == 0 ? 0u : rnd(L.L + 1);
        for (uint32_t i = 0; i < n; ++i)
            c.inf.push_back(QeInflight{4ull * rnd(1000), rnd((uint32_t)c.counter + 1), rnd(2) << 31 | rnd(100)});
        c.num_blocked = rnd(n + 1);
    }
    return c;
}

// the connection in slab `slot` with a ring history of its own: ring start, which ring holds the bytes, the bytes'
// order and place
void build_slab(const Layout& L, const Conn& c, uint8_t* scratch, uint64_t slot, bool& wrapped) {
    const uint64_t sbase = slot * L.slab;
    uint8_t* slab = scratch + sbase;
    const uint32_t n = (uint32_t)c.ent.size();
    uint64_t bytes = 0;
    for (const Ent& e : c.ent) bytes += e.name.size() + e.value.size();
    if (L.family == HHUFF_FAM_QPACK_DSESSION) {
        store(slab, QpHead{(uint32_t)c.parked.size(), 0u, c.counter});
        for (size_t i = 0; i < c.parked.size(); ++i) store(slab + L.list_off + 16 * i, c.parked[i]);
        wrapped = wrapped || c.parked.size() == L.L;
        return;
    }
    if (L.family == HHUFF_FAM_QPACK_ENC) {
        uint32_t off = rnd((uint32_t)(L.str_cap - bytes) + 1);  // the live run starts anywhere
        store(slab, QeState{(uint32_t)c.counter, (uint32_t)(bytes + 32ull * n), c.lkr, c.num_blocked, (uint32_t)c.inf.size(), c.failed,
                            (uint32_t)(off + bytes), c.evicted});
        for (uint32_t j = 0; j < n; ++j) {
            const Ent& e = c.ent[j];
            const uint32_t s = qt_slot(c.evicted + j + 1u, L.E);
            wrapped = wrapped || (j && s == 0);
            store(slab + L.ent_off + (uint64_t)s * L.ent_stride,
                  QsEntry{off, (uint32_t)e.name.size(), (uint32_t)e.value.size(), e.a, e.b, 0u, 0u, 0u});
            if (!e.name.empty()) memcpy(slab + L.str_off + off, e.name.data(), e.name.size());
            if (!e.value.empty()) memcpy(slab + L.str_off + off + e.name.size(), e.value.data(), e.value.size());
            off += (uint32_t)(e.name.size() + e.value.size());
        }
        for (size_t i = 0; i < c.inf.size(); ++i) store(slab + L.list_off + 16 * i, c.inf[i]);
        return;
    }
    const uint32_t start = rnd(L.E), ring = rnd(2);
    const bool newest_first = L.family != HHUFF_FAM_QPACK_DEC;
    const uint64_t rbase = L.str_off + ring * L.str_cap;
    uint64_t off = rnd(2) ? 0u : rnd((uint32_t)(L.str_cap - bytes) + 1);
    for (uint32_t k = 0; k < n; ++k) {  // ring position k
        const Ent& e = c.ent[newest_first ? n - 1u - k : k];
        uint32_t s = start + k;
        if (s >= L.E) s -= L.E, wrapped = true;
        const uint64_t no = sbase + rbase + off, vo = no + e.name.size();
        uint8_t* p = slab + L.ent_off + (uint64_t)s * L.ent_stride;
        const uint32_t nl = (uint32_t)e.name.size(), vl = (uint32_t)e.value.size();
        if (L.family == HHUFF_FAM_HPACK_DEC)
            store(p, BlkEntry{kBlkScr | no, kBlkScr | vo, nl, vl, (uint16_t)e.a, (uint16_t)(rnd(2) ? kClsUnknown : rnd(40)), 0u});
        else if (L.family == HHUFF_FAM_QPACK_DEC)
            store(p, QdEntry{kQdScr | no, kQdScr | vo, nl, vl, e.a, 0u});
        else
            store(p, HeEntry{kHeScr | no, kHeScr | vo, nl, vl, e.a, e.b, e.c, 0u});
        if (nl) memcpy(slab + rbase + off, e.name.data(), nl);
        if (vl) memcpy(slab + rbase + off + nl, e.value.data(), vl);
        off += nl + vl;
    }
    const uint64_t size = bytes + 32ull * n;
    if (L.family == HHUFF_FAM_HPACK_DEC)
        store(slab, BlkState{start, n, ring, c.failed, size, c.cap});
    else if (L.family == HHUFF_FAM_QPACK_DEC)
        store(slab, QdState{(int64_t)(c.counter + 1 - n), c.counter, size, c.cap, start, n, ring, c.failed, rnd(2), {0u, 0u, 0u}});
    else
        store(slab, HeState{start, n, ring, c.failed, (uint32_t)size, (uint32_t)c.cap, 0u, 0u});
}

std::unique_ptr<Block> pack(const hhuff_conn_family_t& f, const Layout& L, const uint8_t* scratch, uint64_t slot) {
    uint32_t len = 0, len2 = 0;
    CHECK(img_pack(f, L, scratch, slot, nullptr, 0, &len) == 0);
    CHECK(len % 16 == 0 && len >= kFixed && len <= image_bound(L));
    if (len > 16) {  // a region 16 bytes short: the length needed, nothing written
        Block small(len - 16, 0x5A);
        CHECK(img_pack(f, L, scratch, slot, small.p, len - 16, &len2) == HHUFF_IMG_SPACE && len2 == len);
        for (size_t i = 0; i < small.n; ++i) CHECK(small.p[i] == 0x5A);
    }
    auto out = std::make_unique<Block>(len, 0x5A);
    CHECK(img_pack(f, L, scratch, slot, out->p, len, &len2) == 0 && len2 == len);
    return out;
}

struct Seen {
    bool wrapped = false, empty = false, eformat = false, eparam = false, accepted = false;
};

void round_of(const hhuff_conn_family_t& f, const Layout& L, Seen& seen) {
    const uint32_t nslots = 1 + rnd(3);
    const Conn c = random_conn(L);
    seen.empty = seen.empty || (c.ent.empty() && c.inf.empty() && c.parked.empty());
    Block a(nslots * L.slab), a2(nslots * L.slab);
    const uint64_t sa = rnd(nslots), sa2 = rnd(nslots);
    build_slab(L, c, a.p, sa, seen.wrapped);
    build_slab(L, c, a2.p, sa2, seen.wrapped);  // the same connection after another history
    const auto i1 = pack(f, L, a.p, sa), i1b = pack(f, L, a2.p, sa2);
    CHECK(i1->n == i1b->n && memcmp(i1->p, i1b->p, i1->n) == 0);
    uint64_t strs = 0;
    for (const Ent& e : c.ent) strs += e.name.size() + e.value.size();
    CHECK(i1->n <= 96 + 32 * (c.ent.size() + c.inf.size() + c.parked.size()) + strs + 15);

    const uint32_t nb = 1 + rnd(3);
    Block b(nb * L.slab);
    const uint64_t sb = rnd(nb);
    CHECK(img_unpack(f, L, b.p, sb, i1->p, i1->n) == 0);
    for (uint64_t s = 0; s < nb; ++s)
        if (s != sb)
            for (uint64_t k = 0; k < L.slab; ++k) CHECK(b.p[s * L.slab + k] == 0xC3);
    const auto i2 = pack(f, L, b.p, sb);
    CHECK(i2->n == i1->n && memcmp(i1->p, i2->p, i1->n) == 0);

    // another family, other parameters
    hhuff_conn_family_t g = f;
    g.family = (f.family + 1u) % 5u;
    Layout G;
    if (layout(g, G) || (g = hhuff_conn_family_t{g.family, 0, 0, 0}, layout(g, G))) {
        Block x(G.slab);
        CHECK(img_unpack(g, G, x.p, 0, i1->p, i1->n) == HHUFF_IMG_EPARAM);
        seen.eparam = true;
    }

    for (int m = 0; m < 200; ++m) {
        Block img(i1->n);
        memcpy(img.p, i1->p, i1->n);
        uint64_t len = i1->n;
        const uint32_t kind = rnd(8);
        auto word = [&](size_t off) { return reinterpret_cast<uint32_t*>(img.p + off); };
        const uint32_t bump = rnd(2) ? 1u : rnd(2) ? 0x80000000u : (uint32_t)rng();
        switch (kind) {
            case 0: *word(4 * rnd(8)) += bump; break;                 // a header field
            case 1: *word(32 + 4 * rnd(16)) += bump; break;           // a state field
            case 2: *word(32 + 4 * rnd(3)) += 1 + rnd(3000); break;   // counts, run length
            case 3:                                                   // an entry's lengths
                if (c.ent.empty()) continue;
                *word(kFixed + 32 * rnd((uint32_t)c.ent.size()) + 4 * rnd(2)) += bump;
                break;
            case 4: img.p[rnd((uint32_t)len)] ^= (uint8_t)(1u << rnd(8)); break;  // a random bit
            case 5: len = rnd(2) ? len - 16 : 16 * rnd((uint32_t)(len / 16)); break;  // a shorter region
            case 6:                                                   // a random word of the body
                if (len == kFixed) continue;
                *word(kFixed + 4 * rnd((uint32_t)((len - kFixed) / 4))) = (uint32_t)rng();
                break;
            default: *word(32 + 16 + 4 * rnd(12)) = 0xFFFFFFFFu; break;  // size, capacity, counters at their limit
        }
        Block d(L.slab);
        const int32_t rc = img_unpack(f, L, d.p, 0, img.p, len);
        CHECK(rc == 0 || rc == HHUFF_IMG_EFORMAT || rc == HHUFF_IMG_EPARAM);
        if (rc != 0) {
            for (uint64_t k = 0; k < L.slab; ++k) CHECK(d.p[k] == 0xC3);
            (rc == HHUFF_IMG_EFORMAT ? seen.eformat : seen.eparam) = true;
        } else {
            const auto again = pack(f, L, d.p, 0);  // what was accepted is a slab the family can walk
            CHECK(again->n == len && memcmp(again->p, img.p, len) == 0);
            seen.accepted = true;
        }
    }
}
}  // namespace

int main(int argc, char** argv) {
    const unsigned rounds = argc > 1 ? (unsigned)atoi(argv[1]) : 300u;
    const hhuff_conn_family_t fams[] = {
        {HHUFF_FAM_HPACK_DEC, 4096, 0, 0}, {HHUFF_FAM_HPACK_DEC, 256, 0, 0},  {HHUFF_FAM_HPACK_DEC, 0, 0, 0},
        {HHUFF_FAM_QPACK_DEC, 4096, 0, 0}, {HHUFF_FAM_QPACK_DEC, 100, 0, 0},  {HHUFF_FAM_QPACK_DEC, 0, 0, 0},
        {HHUFF_FAM_HPACK_ENC, 0, 0, 0},    {HHUFF_FAM_QPACK_ENC, 4096, 64, 0}, {HHUFF_FAM_QPACK_ENC, 128, 3, 0},
        {HHUFF_FAM_QPACK_ENC, 31, 1, 0},   {HHUFF_FAM_QPACK_DSESSION, 0, 0, 100}, {HHUFF_FAM_QPACK_DSESSION, 0, 0, 0}};
    unsigned nfam = 0;
    for (const hhuff_conn_family_t& f : fams) {
        g_fam = nfam++;
        Layout L;
        CHECK(layout(f, L));
        Seen seen;
        for (g_round = 0; g_round < rounds; ++g_round) round_of(f, L, seen);
        const bool tiny = L.E + L.L <= 1;  // no ring to wrap, no list to fill
        CHECK(seen.empty && seen.eformat && seen.eparam && seen.accepted && (seen.wrapped || tiny));
    }
    // parameters the families refuse
    const hhuff_conn_family_t bad[] = {{HHUFF_FAM_QPACK_ENC, 65537, 1, 0}, {HHUFF_FAM_QPACK_DEC, (1u << 30) + 1, 0, 0},
                                       {HHUFF_FAM_QPACK_DSESSION, 0, 0, 4097}, {5, 0, 0, 0}, {HHUFF_FAM_HPACK_ENC, 1, 0, 0},
                                       {HHUFF_FAM_HPACK_DEC, 4096, 1, 0}, {HHUFF_FAM_QPACK_DEC, 4096, 0, 1}};
    for (const hhuff_conn_family_t& f : bad) {
        Layout L;
        CHECK(!layout(f, L));
    }
    printf("ok: %u families x %u rounds, images canonical, mutants refused or in bounds\n", nfam, rounds);
    return 0;
}
