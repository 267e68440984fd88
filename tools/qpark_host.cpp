// The QPACK decoder sessions' list operations (h2o_amd/csrc/hhuff_qpark.h: find, park, remove, the wake scan, the
// Known Received arithmetic, the prefix integer) on the host, against std::map bookkeeping, for AddressSanitizer and
// UndefinedBehaviorSanitizer.  A session's list is a heap block of exactly max_blocked entries and every integer is
// written into a heap block of exactly its length, so a step outside them is reported.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ih2o_amd/csrc
//       tools/qpark_host.cpp -o build/qpark_host && build/qpark_host 4000
//
// Every sequence: a list of 0 .. 8 entries, then random steps of one connection as the session pass runs them --
// blocked sections of new streams (parked while a slot is free, refused after) and of parked ones (resubmissions:
// nothing moves), decoded sections (a parked stream leaves, an acknowledgment raises the Known Received Count),
// cancellations of parked and of unknown streams, then a wake scan with a region of random size against a table
// that has grown, then the increment.  After every operation the list is compared with the map: the streams, their
// refs and their order (the map keeps each stream's parking sequence number).  The run fails unless it saw a full
// list refuse a stream, a wake region too small for the streams due, and a removal from the middle.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <memory>
#include <random>
#include <utility>
#include <vector>

#include "hhuff_qpark.h"

using namespace hhuff;

namespace {
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            printf("FAIL %s:%d: %s (sequence %u)\n", __FILE__, __LINE__, #c, g_seq); \
            exit(1);                                                   \
        }                                                              \
    } while (0)
unsigned g_seq = 0;

struct Parked {
    uint64_t ref, order;
};

struct Session {
    uint32_t cap, n = 0;
    std::unique_ptr<QpEntry[]> ent;
    std::map<uint64_t, Parked> book;
    uint64_t next_order = 0, known_received = 0, book_known = 0;
    explicit Session(uint32_t c) : cap(c), ent(new QpEntry[c]) {}
};

std::vector<std::pair<uint64_t, Parked>> in_order(const Session& s) {
    std::vector<std::pair<uint64_t, Parked>> v(s.book.begin(), s.book.end());
    std::sort(v.begin(), v.end(), [](const auto& a, const auto& b) { return a.second.order < b.second.order; });
    return v;
}

void compare(const Session& s) {
    const auto v = in_order(s);
    CHECK(v.size() == s.n);
    CHECK(s.n <= s.cap);
    for (uint32_t i = 0; i < s.n; ++i) {
        CHECK(s.ent[i].stream_id == v[i].first);
        CHECK(s.ent[i].ref == v[i].second.ref);
    }
    CHECK(s.known_received == s.book_known);
}

// a prefix integer read back the way h2o_hpack_decode_int reads it
uint64_t read_int(const uint8_t* b, uint32_t len, uint32_t bits, uint32_t& used) {
    const uint64_t mask = (1u << bits) - 1u;
    uint64_t v = b[0] & mask;
    used = 1;
    if (v != mask) return v;
    for (uint32_t shift = 0;; shift += 7) {
        CHECK(used < len);
        const uint8_t x = b[used++];
        v += (uint64_t)(x & 127u) << shift;
        if (!(x & 128u)) return v;
    }
}

void check_int(uint64_t v, uint32_t bits, uint32_t first) {
    uint8_t probe[kQpIntMax + 1];
    const uint32_t len = qp_put_int(probe, first, v, bits);
    CHECK(len >= 1 && len <= kQpIntMax);
    std::unique_ptr<uint8_t[]> exact(new uint8_t[len]);  // exactly its length: a byte more is an ASan report
    CHECK(qp_put_int(exact.get(), first, v, bits) == len);
    uint32_t used = 0;
    CHECK(read_int(exact.get(), len, bits, used) == v);
    CHECK(used == len);
    CHECK((exact[0] & ~((1u << bits) - 1u)) == first);
    if (v < (1ull << 62)) CHECK(len <= 10);  // hhuff_qpack_dsession_out_bound's 10 bytes an instruction
}
}  // namespace

int main(int argc, char** argv) {
    const unsigned nseq = argc > 1 ? (unsigned)atoi(argv[1]) : 4000;
    std::mt19937_64 rng(20240917);
    auto rnd = [&](uint64_t n) { return n ? rng() % n : 0; };
    uint64_t saw_full = 0, saw_pending = 0, saw_middle = 0, saw_resubmit = 0, ops = 0;

    const uint64_t edges[] = {0, 1, 62, 63, 64, 126, 127, 128, 190, 191, 16383, 16384, (1ull << 62) - 1, 1ull << 62, ~0ull};
    for (uint64_t v : edges) {
        check_int(v, 6, 0x40);
        check_int(v, 6, 0x00);
        check_int(v, 7, 0x80);
    }
    for (int k = 0; k < 20000; ++k) check_int(rng() >> rnd(64), rnd(2) ? 6 : 7, rnd(2) ? 0x80 : 0x00);
    CHECK(qp_out_bound(0, 0) == 10 && qp_out_bound(3, 2) == 60);
    CHECK(qp_slab_bytes(0) == 16 && qp_slab_bytes(4096) == 16 + 16 * 4096);

    for (g_seq = 0; g_seq < nseq; ++g_seq) {
        Session s((uint32_t)rnd(9));
        uint64_t total = 0;
        const uint64_t ids = 1 + rnd(12);  // few streams: resubmissions and cancellations of parked ones are common
        for (int step = 0, nsteps = 1 + (int)rnd(8); step < nsteps; ++step) {
            for (int k = 0, nsec = (int)rnd(6); k < nsec; ++k, ++ops) {  // 1. sections
                const uint64_t id = 4 * rnd(ids), ric = total + rnd(4);
                const uint32_t i = qp_find(s.ent.get(), s.n, id);
                CHECK((i != s.n) == (s.book.count(id) != 0));
                if (ric > total) {  // comes up blocked
                    if (i != s.n) {
                        ++saw_resubmit;
                    } else if (qp_park(s.ent.get(), s.n, s.cap, id, ric)) {
                        CHECK(s.book.size() < s.cap);
                        s.book[id] = Parked{ric, s.next_order++};
                    } else {
                        CHECK(s.book.size() == s.cap);
                        ++saw_full;
                    }
                } else {  // decodes: the stream leaves, its acknowledgment counts
                    if (i != s.n) {
                        saw_middle += i + 1 < s.n;
                        qp_remove(s.ent.get(), s.n, i);
                        s.book.erase(id);
                    }
                    if (ric) {
                        s.known_received = qp_acknowledged(s.known_received, ric);
                        s.book_known = std::max(s.book_known, ric);
                    }
                }
                compare(s);
            }
            for (int k = 0, nc = (int)rnd(3); k < nc; ++k, ++ops) {  // 2. cancellations
                const uint64_t id = 4 * rnd(ids + 2);
                const uint32_t i = qp_find(s.ent.get(), s.n, id);
                if (i != s.n) {
                    saw_middle += i + 1 < s.n;
                    qp_remove(s.ent.get(), s.n, i);
                }
                s.book.erase(id);
                compare(s);
            }
            total += rnd(4);  // the step's inserts
            const uint32_t room = (uint32_t)rnd(4);  // 3. wake
            std::unique_ptr<uint64_t[]> out(new uint64_t[room]);
            bool pending = false;
            const uint32_t nw = qp_wake(s.ent.get(), s.n, total, out.get(), room, pending);
            uint32_t due = 0, w = 0;
            for (const auto& e : in_order(s)) {
                if (e.second.ref > total) continue;
                ++due;
                if (w < room) {
                    CHECK(out[w] == e.first);
                    ++w;
                    s.book.erase(e.first);
                }
            }
            CHECK(nw == w && nw == std::min(due, room));
            CHECK(pending == (due > room));
            saw_pending += pending;
            compare(s);
            if (rnd(2)) {  // 4. the increment
                const uint64_t inc = qp_increment(total, s.known_received);
                CHECK(inc == (total > s.book_known ? total - s.book_known : 0));
                if (inc) s.known_received = s.book_known = total;
            }
            ++ops;
        }
    }
    CHECK(saw_full > 0 && saw_pending > 0 && saw_middle > 0 && saw_resubmit > 0);
    printf("ok: %u sequences, %llu operations, %llu refusals of a full list, %llu short wake regions, %llu removals "
           "from the middle, %llu resubmissions\n",
           nseq, (unsigned long long)ops, (unsigned long long)saw_full, (unsigned long long)saw_pending,
           (unsigned long long)saw_middle, (unsigned long long)saw_resubmit);
    return 0;
}
