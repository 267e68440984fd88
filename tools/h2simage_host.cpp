// HTTP/2 stream table images (h2o_amd/csrc/hhuff_h2simage.h: the image format, its validator, pack / unpack) on the
// host, for AddressSanitizer and UndefinedBehaviorSanitizer.  Every slab is a heap block of exactly its size and every
// image a heap block of exactly its length, so a step outside them is reported.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ih2o_amd/csrc
//       tools/h2simage_host.cpp -o build/h2simage_host && build/h2simage_host 300
//
// Per round: a table of a random max_entries is driven through h2s::insert and h2s::remove with ids drawn from few
// homes, so that chains wrap around the table's end and deletions shift entries, with fill epochs and marks of several
// fills.  It is packed, unpacked into a slab of another max_entries, packed again, unpacked back and packed again: the
// three images are the same bytes, every id is found by h2s::find with the record the source had, two unpacks of one
// image give the same slab bytes, and a table too small answers HHUFF_IMG_EPARAM with its slab untouched.  Then
// truncations and single-byte mutants of the image go through unpack: each is refused with the slab untouched, or
// accepted into a table whose ids h2s::find reaches and that packs again, all inside the blocks.  The run fails unless
// it saw a wrapped chain, an empty and a full table, refusals of both kinds and an accepted mutant.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <random>
#include <vector>

#include "hhuff_h2simage.h"

using namespace hhuff;
using namespace hhuff::h2i;

namespace {
#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) {                                                                \
            printf("FAIL %s:%d: %s (round %u)\n", __FILE__, __LINE__, #c, g_round); \
            exit(1);                                                               \
        }                                                                          \
    } while (0)
unsigned g_round = 0;
std::mt19937 rng(4711);
uint32_t rnd(uint32_t n) { return n ? (uint32_t)(rng() % n) : 0u; }

struct Block {  // an exact heap block, 16-byte aligned
    uint8_t* p;
    size_t n;
    explicit Block(size_t bytes, int fill = 0xC3) : p((uint8_t*)aligned_alloc(16, (bytes + 15) & ~(size_t)15)), n(bytes) { memset(p, fill, n); }
    ~Block() { free(p); }
    Block(const Block&) = delete;
};

uint32_t pick_entries() {
    static const uint32_t edge[] = {1, 2, 3, 32, 33, 117, 256, 257, 2048};
    return rnd(3) == 0 ? 1u + rnd(300) : edge[rnd(sizeof(edge) / sizeof(edge[0]))];
}

// an id whose home in T is one of a few slots around the table's end
uint32_t crowded_id(const h2s::Table& T) {
    for (;;) {
        const uint32_t id = 1u + rnd(0x7ffffffeu);
        if (rnd(4) == 0 || ((h2s::home(T, id) + 2u) & T.mask) < 4u) return id;
    }
}

Entry random_entry(uint32_t id, uint32_t mark) {
    Entry e{};
    e.stream_id = id, e.state = (uint8_t)rnd(4), e.body = (uint8_t)rnd(4), e.flags = (uint8_t)rnd(16), e.rsv = (uint8_t)rnd(256);
    e.bytes_unnotified = rng(), e.mark = mark;
    e.output_window = (int64_t)rng() - (1ll << 31), e.input_window = (int64_t)rng() - (1ll << 31);
    e.received = rng(), e.content_length = rnd(2) ? h2s::kNoLength : rng();
    return e;
}

struct Seen {
    bool wrapped = false, empty = false, full = false, eformat = false, eparam = false, accepted = false;
} seen;

std::vector<uint8_t> packed(uint32_t max_entries, const Block& slab) {
    std::vector<uint32_t> ids(h2s::table_cap(max_entries));
    uint32_t need = 0, len = 0;
    CHECK(pack(max_entries, slab.p, ids.data(), nullptr, 0, &need) == 0);
    Block img(need);
    if (need >= 16) {
        Block small(need - 16);
        CHECK(pack(max_entries, slab.p, ids.data(), small.p, small.n, &len) == HHUFF_IMG_SPACE && len == need);
    }
    CHECK(pack(max_entries, slab.p, ids.data(), img.p, img.n, &len) == 0 && len == need);
    return std::vector<uint8_t>(img.p, img.p + len);
}

// unpack of exactly the image's bytes into a fresh slab of max_entries: the verdict; refused: the slab untouched
int32_t unpacked(uint32_t max_entries, const std::vector<uint8_t>& image, Block& slab) {
    Block in(image.size());
    memcpy(in.p, image.data(), image.size());
    std::vector<uint32_t> work(max_entries);
    const int32_t rc = unpack(max_entries, slab.p, work.data(), in.p, in.n);
    if (rc != 0)
        for (size_t i = 0; i < slab.n; ++i) CHECK(slab.p[i] == 0xC3);
    return rc;
}

// every record of a valid image is in the table, where h2s::find looks for it
void all_found(uint32_t max_entries, Block& slab, const std::vector<uint8_t>& image) {
    const h2s::Table T = h2s::table_at(slab.p, max_entries);
    const State s = load<State>(image.data() + sizeof(Header));
    CHECK(T.head->count == s.count && T.head->fill_epoch == 1u);
    uint32_t live = 0;
    for (uint32_t i = 0; i <= T.mask; ++i) live += T.ent[i].stream_id != 0;
    CHECK(live == s.count);
    for (uint32_t j = 0; j < s.count; ++j) {
        const Entry e = record(image.data(), j);
        const uint32_t at = h2s::find(T, e.stream_id);
        CHECK(at != h2s::kNone && memcmp(&T.ent[at], &e, sizeof(Entry)) == 0);
    }
}

void round_trip() {
    const uint32_t ma = pick_entries(), mb = pick_entries();
    Block a(h2s::slab_size(ma));
    const h2s::Table T = h2s::table_at(a.p, ma);
    h2s::clear(T);
    std::map<uint32_t, Entry> model;
    uint32_t epoch = rnd(3);
    const uint32_t target = rnd(5) == 0 ? 0u : rnd(4) == 0 ? ma : rnd(ma + 1);
    for (uint32_t step = 0; step < 4u * ma + 8u; ++step) {
        const bool grow = model.size() < target || (rnd(3) == 0 && model.size() < ma);
        if (grow) {
            const uint32_t id = crowded_id(T);
            if (model.count(id)) continue;
            const Entry e = random_entry(id, rnd(2) ? epoch : rnd(3));
            h2s::insert(T, e);
            model[id] = e;
            if (h2s::find(T, id) < h2s::home(T, id)) seen.wrapped = true;
        } else if (!model.empty() && (model.size() > target || rnd(2))) {
            auto it = model.begin();
            std::advance(it, rnd((uint32_t)model.size()));
            h2s::remove(T, h2s::find(T, it->first));
            model.erase(it);
        }
        if (rnd(16) == 0) ++epoch;
    }
    *T.head = Head{rnd(~0u), rnd(~0u), rnd(~0u), rnd(~0u), (uint32_t)model.size(), epoch, {0, 0}};
    seen.empty |= model.empty(), seen.full |= model.size() == ma;

    const std::vector<uint8_t> image = packed(ma, a);
    CHECK(image.size() == image_bytes(model.size()));
    uint32_t j = 0;
    for (const auto& kv : model) {  // ascending ids, normalised
        const Entry want = normalised(kv.second, epoch), got = record(image.data(), j++);
        CHECK(memcmp(&want, &got, sizeof(Entry)) == 0);
    }
    Block b(h2s::slab_size(mb)), b2(h2s::slab_size(mb), 0x5A);
    const int32_t rc = unpacked(mb, image, b);
    if (model.size() > mb) {
        CHECK(rc == HHUFF_IMG_EPARAM);
        seen.eparam = true;
    } else {
        CHECK(rc == 0);
        all_found(mb, b, image);
        CHECK(packed(mb, b) == image);
        Block in(image.size());
        memcpy(in.p, image.data(), image.size());
        std::vector<uint32_t> work(mb);
        CHECK(unpack(mb, b2.p, work.data(), in.p, in.n) == 0 && memcmp(b.p, b2.p, b.n) == 0);  // whatever the slab held before
        Block back(h2s::slab_size(ma));
        CHECK(unpacked(ma, packed(mb, b), back) == 0);
        CHECK(packed(ma, back) == image);
    }

    // truncations and single-byte mutants
    for (uint32_t m = 0; m < 40; ++m) {
        std::vector<uint8_t> mut = image;
        if (rnd(4) == 0)
            mut.resize(rnd((uint32_t)mut.size()));
        else
            mut[rnd(8) ? rnd((uint32_t)mut.size()) : rnd(kFixed)] ^= (uint8_t)(1u << rnd(8));
        Block c(h2s::slab_size(ma));
        const int32_t r = unpacked(ma, mut, c);
        CHECK(r == 0 || r == HHUFF_IMG_EFORMAT || r == HHUFF_IMG_EPARAM);
        if (r == HHUFF_IMG_EFORMAT) seen.eformat = true;
        if (r == 0) {
            all_found(ma, c, mut);
            CHECK(packed(ma, c) == mut);
            seen.accepted = true;
        }
    }
    // a slab no call wrote: pack stays inside it
    Block junk(h2s::slab_size(ma), (int)rnd(256));
    for (uint32_t i = 0; i < 64 && i < junk.n; ++i) junk.p[rnd((uint32_t)junk.n)] = (uint8_t)rng();
    Block d(h2s::slab_size(ma));
    (void)unpacked(ma, packed(ma, junk), d);
}
}  // namespace

int main(int argc, char** argv) {
    const unsigned rounds = argc > 1 ? (unsigned)atoi(argv[1]) : 100u;
    for (g_round = 0; g_round < rounds; ++g_round) round_trip();
    CHECK(!entries_ok(0) && !entries_ok(kMaxEntries + 1) && entries_ok(kMaxEntries));
    if (rounds >= 50)
        CHECK(seen.wrapped && seen.empty && seen.full && seen.eformat && seen.eparam && seen.accepted);
    printf("ok: %u rounds\n", rounds);
    return 0;
}
