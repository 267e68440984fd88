// HTTP/2 stream table images (include/hhuff.h (2k'''), hhuff_h2_streams_export / _import): the image format, its
// validator and a serial pack / unpack, for the device (hhuff_h2simage.hip: a wave or a workgroup per listed
// connection) and for the host (tools/h2simage_host.cpp runs pack, check and unpack under AddressSanitizer and
// UndefinedBehaviorSanitizer).
//
// An image is [Header 32 B][State 32 B][count x h2s::Entry 48 B]:
//   Header  the connection images' (hhuff_image.h): magic "HHCI", u16 version = 1, u16 family = 5, the three
//           parameter words 0, u32 total length = 64 + 48 * count, two reserved words 0
//   State   pull_max_open, push_max_open, pull_open, priority_open, count, three reserved words 0
//   Entry   the live entries, ascending stream_id; rsv = 0; mark = 1 when the last hhuff_h2_streams_fill_sends
//           listed the stream (fill_epoch != 0 && mark == fill_epoch), else 0
// The table of a slab is an open-addressed hash table: its probe chains, its deletions, its fill_epoch and its slot
// count are history and parameters, not state, and none of them is in the image.  Export sorts, import hashes
// again -- at the destination's max_entries, which need not be the source's.
//
// Placement on import is by rounds, so that a wave can do it: in round r every entry not yet placed proposes slot
// (home + r) & mask, and of the entries that propose one free slot the one with the lowest record index takes it.
// A taken slot never changes, so the slots between an entry's home and its place were taken before it was placed:
// h2s::find reaches it.  count <= max_entries <= slots / 2, so every entry is placed within `slots` rounds.  The
// result is a function of the image and max_entries alone; unpack below runs the same rounds one entry at a time.
#ifndef HHUFF_H2SIMAGE_H
#define HHUFF_H2SIMAGE_H
#include <stdint.h>
#include <string.h>

#include "hhuff.h"
#include "hhuff_h2streams.h"
#include "hhuff_image.h"

namespace hhuff {
namespace h2i {
using h2s::Entry;
using h2s::Head;
using img::Header;
using img::load;
using img::store;

constexpr uint32_t kFamily = 5;          // the header's family word: none of HHUFF_FAM_*, whose images hhuff_conn_import reads
constexpr uint32_t kMaxEntries = 2048;   // tables of at most 4096 slots: their ids fit 16 KB of LDS
constexpr uint32_t kMaxCap = 2 * kMaxEntries;
constexpr uint32_t kFree = 0xFFFFFFFFu;  // a free slot among the staged ids / the slots' owners

struct State {
    uint32_t pull_max_open, push_max_open, pull_open, priority_open;
    uint32_t count;
    uint32_t rsv[3];
};
static_assert(sizeof(State) == 32 && sizeof(Header) == 32, "image records");
constexpr uint32_t kFixed = sizeof(Header) + sizeof(State);

HHUFF_CTL_HD bool entries_ok(uint32_t max_entries) { return max_entries != 0 && max_entries <= kMaxEntries; }
HHUFF_CTL_HD uint64_t image_bytes(uint64_t count) { return kFixed + sizeof(Entry) * count; }
HHUFF_CTL_HD Header make_header(uint32_t total) {
    return Header{img::kMagic, (uint16_t)img::kVersion, (uint16_t)kFamily, 0u, 0u, 0u, total, 0u, 0u};
}
HHUFF_CTL_HD State state_of(const Head& H, uint32_t count) {
    return State{H.pull_max_open, H.push_max_open, H.pull_open, H.priority_open, count, {0u, 0u, 0u}};
}
HHUFF_CTL_HD Head head_of(const State& s) {
    return Head{s.pull_max_open, s.push_max_open, s.pull_open, s.priority_open, s.count, 1u, {0u, 0u}};
}

// the entry as the image keeps it
HHUFF_CTL_HD Entry normalised(Entry e, uint32_t fill_epoch) {
    e.rsv = 0;
    e.mark = fill_epoch != 0 && e.mark == fill_epoch ? 1u : 0u;
    return e;
}

// ---- the validator: an image is bytes from anywhere ----
// header and state of an image of `len` bytes for a table of max_entries: 0, HHUFF_IMG_EFORMAT, or HHUFF_IMG_EPARAM
// for a well-formed image whose entries the table has no room for
HHUFF_CTL_HD int32_t check_fixed(const Header& h, const State& s, uint64_t len, uint32_t max_entries) {
    if (h.magic != img::kMagic || h.version != img::kVersion || h.family != kFamily) return HHUFF_IMG_EFORMAT;
    if (h.table_size || h.max_inflight || h.max_blocked || h.rsv0 || h.rsv1 || h.total != len) return HHUFF_IMG_EFORMAT;
    if (s.rsv[0] || s.rsv[1] || s.rsv[2] || image_bytes(s.count) != len) return HHUFF_IMG_EFORMAT;
    return s.count > max_entries ? HHUFF_IMG_EPARAM : 0;
}
// a record behind the one of stream prev_id (0: it is the first)
HHUFF_CTL_HD bool check_entry(const Entry& e, uint32_t prev_id) {
    return e.stream_id != 0 && e.stream_id <= 0x7fffffffu && e.stream_id > prev_id && e.state <= 3 && e.body <= 3 && e.flags < 16 &&
           e.rsv == 0 && e.mark <= 1u;
}
HHUFF_CTL_HD Entry record(const uint8_t* in, uint32_t j) { return load<Entry>(in + kFixed + sizeof(Entry) * (uint64_t)j); }

// every check of an image of `len` bytes: 0, HHUFF_IMG_EFORMAT or HHUFF_IMG_EPARAM; *sp = its state
HHUFF_CTL_HD int32_t check(const uint8_t* in, uint64_t len, uint32_t max_entries, State* sp) {
    if (len < kFixed || (len - kFixed) % sizeof(Entry) != 0) return HHUFF_IMG_EFORMAT;
    const State s = load<State>(in + sizeof(Header));
    const int32_t rc = check_fixed(load<Header>(in), s, len, max_entries);
    if (rc) return rc;
    uint32_t prev = 0;
    for (uint32_t j = 0; j < s.count; ++j) {
        const Entry e = record(in, j);
        if (!check_entry(e, prev)) return HHUFF_IMG_EFORMAT;
        prev = e.stream_id;
    }
    *sp = s;
    return 0;
}

// ---- serial pack / unpack (the host's; the kernels do the same with a wave or a workgroup) ----
// the live ids of a slab in ascending order into ids[0 .. slots); -> how many.  Whatever the slab holds, no read
// leaves it and the count is at most max_entries.
HHUFF_CTL_HD uint32_t sorted_ids(const h2s::Table& T, uint32_t* ids) {
    uint32_t n = 0;
    for (uint32_t i = 0; i <= T.mask; ++i) {
        const uint32_t id = T.ent[i].stream_id;
        if (id == 0 || id == kFree) continue;
        uint32_t k = n++;
        for (; k != 0 && ids[k - 1] > id; --k) ids[k] = ids[k - 1];
        ids[k] = id;
    }
    uint32_t count = T.head->count;
    if (count > n) count = n;
    return count > T.max_entries ? T.max_entries : count;
}

// -> 0 with *len = the image's bytes written to out[0 .. room); HHUFF_IMG_SPACE with *len = the bytes needed.
// ids: room for the table's slots.
HHUFF_CTL_HD int32_t pack(uint32_t max_entries, const uint8_t* slab, uint32_t* ids, uint8_t* out, uint64_t room, uint32_t* len) {
    const h2s::Table T = h2s::table_at(const_cast<uint8_t*>(slab), max_entries);
    const uint32_t count = sorted_ids(T, ids);
    const uint64_t total = image_bytes(count);
    *len = (uint32_t)total;
    if (!out) return 0;
    if (total > room) return HHUFF_IMG_SPACE;
    const Head H = *T.head;
    store(out, make_header((uint32_t)total));
    store(out + sizeof(Header), state_of(H, count));
    for (uint32_t j = 0; j < count; ++j) {
        const uint32_t slot = h2s::find(T, ids[j]);
        Entry e{};  // (an id no probe reaches: not a table any call left; import refuses the record)
        if (slot != h2s::kNone) e = normalised(T.ent[slot], H.fill_epoch);
        store(out + kFixed + sizeof(Entry) * (uint64_t)j, e);
    }
    return 0;
}

// -> check's verdict; 0: the slab rebuilt -- every slot written, the free ones zero -- nothing written otherwise.
// work: room for max_entries words (an entry's home while it waits for its place).
HHUFF_CTL_HD int32_t unpack(uint32_t max_entries, uint8_t* slab, uint32_t* work, const uint8_t* in, uint64_t len) {
    State s;
    const int32_t rc = check(in, len, max_entries, &s);
    if (rc) return rc;
    const h2s::Table T = h2s::table_at(slab, max_entries);
    for (uint32_t i = 0; i <= T.mask; ++i) T.ent[i] = Entry{};
    for (uint32_t j = 0; j < s.count; ++j) work[j] = h2s::home(T, record(in, j).stream_id);
    uint32_t left = s.count;
    for (uint32_t r = 0; r <= T.mask && left != 0; ++r) {
        for (uint32_t j = 0; j < s.count; ++j) {  // ascending: of the entries that want one slot the lowest index comes first
            if (work[j] == kFree) continue;
            const uint32_t slot = (work[j] + r) & T.mask;
            if (T.ent[slot].stream_id != 0) continue;
            T.ent[slot] = record(in, j);
            work[j] = kFree;
            --left;
        }
    }
    *T.head = head_of(s);
    return 0;
}
}  // namespace h2i
}  // namespace hhuff
#endif
