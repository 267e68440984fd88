// The evicting encoder table's operations (h2o_amd/csrc/hhuff_qtable.h: evict-prefix, ring slot, string
// compaction, lookup bounds, the draining test) on the host, against list bookkeeping, for AddressSanitizer and
// UndefinedBehaviorSanitizer.  The ring and the string area are heap blocks of exactly the sizes the device
// gives them (header_table_size / 32 entries, header_table_size bytes), so a step outside them is reported.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ih2o_amd/csrc
//       tools/qtable_host.cpp -o build/qtable_host && build/qtable_host 4000
//
// Every sequence: a table size of 64 .. 512, then random sections (references to live entries, inserts with and
// without a name-reference pin, duplications of draining entries -- HHUFF_QENC_DUP: the matched entry is no pin,
// so the prefix that goes may hold it, and the new entry's strings come from a copy of the field, as the device
// takes them from its input), acknowledgments and cancellations that release the sections' pins.  After every
// operation the ring is compared with the list: indices, lengths, every string byte, `used`.  The run fails
// unless it saw a duplication that evicted its own source and one whose compaction wrote over the source.
// A second pass replays the same kind of sequences on tables whose capacity is a peer's, clamped below the slab's
// (hhuff_qpack_flatten_sessions_peers): cap < 32 * slots and str_cap > cap, the ring and the string area still
// those of header_table_size -- capacities 0, 31, 32, 33, 64, 100, half the slab and one entry short of it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <deque>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "hhuff_qtable.h"

using namespace hhuff;

namespace {
struct Table {
    uint32_t cap, scap, slots, count = 0, evicted = 0, used = 0, str_used = 0;  // scap: the string area's bytes
    std::unique_ptr<QsEntry[]> ent;
    std::unique_ptr<uint8_t[]> str;
    std::deque<std::string> live;  // the bookkeeping: name + value of entries evicted + 1 .. count
    std::deque<uint32_t> name_len;
    Table(uint32_t H, uint32_t cap_) : cap(cap_), scap(H), slots(qt_slots(H)), ent(new QsEntry[qt_slots(H)]), str(new uint8_t[H]) {}
};

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            exit(1);                                                   \
        }                                                              \
    } while (0)

void compare(const Table& t) {
    CHECK(t.count - t.evicted == t.live.size() && t.live.size() <= t.slots);
    uint32_t used = 0, run = 0;
    for (uint32_t i = t.evicted + 1; i <= t.count; ++i) {
        const QsEntry& e = t.ent[qt_slot(i, t.slots)];
        const std::string& s = t.live[i - t.evicted - 1];
        CHECK(e.nl == t.name_len[i - t.evicted - 1] && e.nl + e.vl == s.size());
        CHECK((uint64_t)e.noff + s.size() <= t.scap && memcmp(t.str.get() + e.noff, s.data(), s.size()) == 0);
        if (i > t.evicted + 1) CHECK(e.noff == run);  // one contiguous run in insert order
        run = e.noff + e.nl + e.vl;
        used += (uint32_t)s.size() + 32u;
    }
    CHECK(used == t.used && t.used <= t.cap);
    if (!t.live.empty()) CHECK(run == t.str_used);
}

uint64_t g_compactions = 0;
bool g_compacted = false;  // the last insert compacted the string area

// the list's draining test: the free bytes and the bytes of the entries older than i, against a quarter
bool draining(const Table& t, uint32_t i) {
    uint64_t headroom = t.cap - t.used;
    for (uint32_t k = 0; k + 1 < i - t.evicted; ++k) headroom += t.live[k].size() + 32u;
    const bool want = headroom < t.cap / 4u;
    CHECK(qt_draining(t.ent.get(), t.slots, t.cap, t.used, t.evicted, i) == want);
    return want;
}

// -> whether the entry went in; pin = the smallest pinned index (~0u: none)
bool insert(Table& t, const std::string& name, const std::string& value, uint32_t pin) {
    const uint64_t need = name.size() + value.size() + 32u;
    // the list's answer
    size_t k = 0;
    uint64_t u = t.used;
    bool want = need <= t.cap;
    while (want && u + need > t.cap) {
        if (k == t.live.size() || t.evicted + k + 1 >= pin) {
            want = false;
            break;
        }
        u -= t.live[k].size() + 32u;
        ++k;
    }
    uint32_t used_after = 0;
    const uint32_t ev = qt_evict_prefix(t.ent.get(), t.slots, t.cap, t.used, t.evicted, t.count, pin, need, used_after);
    CHECK((ev != kQtNoInsert) == want);
    if (!want) return false;
    CHECK(ev == t.evicted + k && used_after == u);
    t.evicted = ev;
    t.used = used_after;
    for (; k; --k) t.live.pop_front(), t.name_len.pop_front();
    const uint32_t len = (uint32_t)(name.size() + value.size());
    const uint32_t tail = t.str_used;
    t.str_used = qt_place(t.str.get(), t.scap, t.ent.get(), t.slots, t.evicted, t.count, t.str_used, len);
    g_compacted = t.str_used != tail;
    g_compactions += g_compacted ? 1u : 0u;
    CHECK((uint64_t)t.str_used + len <= t.scap);
    memcpy(t.str.get() + t.str_used, name.data(), name.size());
    memcpy(t.str.get() + t.str_used + name.size(), value.data(), value.size());
    t.ent[qt_slot(t.count + 1u, t.slots)] =
        QsEntry{t.str_used, (uint32_t)name.size(), (uint32_t)value.size(), 0u, 0u, 0u, 0u, 0u};
    ++t.count;
    t.used += len + 32u;
    t.str_used += len;
    t.live.push_back(name + value);
    t.name_len.push_back((uint32_t)name.size());
    return true;
}
}  // namespace

int main(int argc, char** argv) {
    const int nseq = argc > 1 ? atoi(argv[1]) : 2000;
    std::mt19937 rng(12345);
    auto pick = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };
    uint64_t inserts = 0, refused = 0, evictions = 0;
    uint64_t dups = 0, dup_refused = 0, dup_self = 0, dup_over = 0, not_draining = 0;
    uint64_t clamped_inserts = 0, clamped_evictions = 0, clamped_compactions = 0;
    for (int s = 0; s < 2 * nseq; ++s) {
        if (s == nseq) {  // the first pass, capacity = the slab's, has seen both duplications
            CHECK(dup_self > 0 && dup_over > 0);
            clamped_inserts = inserts, clamped_evictions = evictions, clamped_compactions = g_compactions;
        }
        const uint32_t H = pick(64, 512);
        uint32_t cap = H;
        if (s >= nseq) {  // a peer's capacity under the slab's
            const uint32_t caps[] = {0u, 31u, 32u, 33u, 64u, 100u, H / 2u, H - 32u};
            cap = caps[s % 8];
            if (cap >= 32u * qt_slots(H)) cap = 32u * qt_slots(H) - 1u;
        }
        Table t(H, cap);
        std::vector<uint32_t> inflight;  // the sections' smallest references
        uint32_t lkr = 0;
        for (int op = 0, nop = (int)pick(20, 200); op < nop; ++op) {
            const uint32_t kind = pick(0, 9);
            if (kind < 6) {  // a section: some references, some inserts
                uint32_t smallest = ~0u;
                for (uint32_t f = 0, nf = pick(1, 4); f < nf; ++f) {
                    uint32_t imin = smallest;
                    for (uint32_t x : inflight) imin = x < imin ? x : imin;
                    if (pick(0, 2) == 0 && t.count > t.evicted) {  // a reference to a live entry
                        const uint32_t top = qt_scan_top(t.count, lkr, pick(0, 1) != 0);
                        CHECK(top <= t.count);
                        if (top > t.evicted) {
                            const uint32_t i = pick(t.evicted + 1, top);
                            (void)t.ent[qt_slot(i, t.slots)].noff;
                            smallest = i < smallest ? i : smallest;
                        }
                        continue;
                    }
                    if (pick(0, 3) == 0 && t.count > t.evicted) {  // an exact match: a duplication when it drains
                        const uint32_t i = pick(t.evicted + 1, t.count);
                        if (!draining(t, i)) {
                            ++not_draining;
                            smallest = i < smallest ? i : smallest;
                            continue;
                        }
                        const uint32_t k = i - t.evicted - 1, ev0 = t.evicted;
                        const std::string name = t.live[k].substr(0, t.name_len[k]), value = t.live[k].substr(t.name_len[k]);
                        const uint32_t src_off = t.ent[qt_slot(i, t.slots)].noff;
                        if (insert(t, name, value, imin)) {  // i itself is no pin
                            ++dups;
                            evictions += t.evicted - ev0;
                            if (t.evicted >= i) {
                                ++dup_self;
                                // the compacted run starts at 0: it covers the source's old place when it reaches it
                                if (g_compacted && t.str_used > src_off) ++dup_over;
                            }
                            smallest = t.count < smallest ? t.count : smallest;
                        } else {
                            ++dup_refused;
                            CHECK(t.evicted == ev0);
                            smallest = i < smallest ? i : smallest;
                        }
                        compare(t);
                        continue;
                    }
                    uint32_t pin = imin;
                    if (pick(0, 3) == 0 && t.count > t.evicted) {  // Insert With Name Reference, dynamic
                        const uint32_t d = pick(t.evicted + 1, t.count);
                        pin = d < pin ? d : pin;
                    }
                    const std::string name(pick(1, 24), (char)('a' + op % 26)), value(pick(0, t.cap / 2 + 8), (char)('A' + f));
                    const uint32_t ev0 = t.evicted;
                    if (insert(t, name, value, pin)) {
                        ++inserts;
                        evictions += t.evicted - ev0;
                        smallest = t.count < smallest ? t.count : smallest;
                    } else {
                        ++refused;
                        CHECK(t.evicted == ev0);
                    }
                    compare(t);
                }
                if (smallest != ~0u && inflight.size() < 8) inflight.push_back(smallest);
            } else if (!inflight.empty()) {  // acknowledgment (7, 8: the first; raises lkr) or cancellation (9: any)
                const size_t k = kind == 9 ? pick(0, (uint32_t)inflight.size() - 1) : 0;
                if (kind != 9) lkr = t.count;
                inflight.erase(inflight.begin() + (long)k);
            }
            compare(t);
        }
    }
    CHECK(inserts > clamped_inserts && evictions > clamped_evictions && g_compactions > clamped_compactions);
    printf("ok: 2 x %d sequences (the second half at capacities under the slab's), %llu inserts (%llu entries evicted, %llu compactions), %llu refused; %llu duplications "
           "(%llu evicted their source, %llu of those compacted over it), %llu refused, %llu matches not draining\n",
           nseq, (unsigned long long)inserts, (unsigned long long)evictions, (unsigned long long)g_compactions,
           (unsigned long long)refused, (unsigned long long)dups, (unsigned long long)dup_self,
           (unsigned long long)dup_over, (unsigned long long)dup_refused, (unsigned long long)not_draining);
    return 0;
}
