// The evicting encoder table of hhuff_qpack_flatten_sessions with HHUFF_QENC_EVICT (include/hhuff.h (2g')):
// the operations on a connection's entry ring and string area, for the device (hhuff_qpenc.hip) and for the
// host (tools/qtable_host.cpp replays random insert / duplicate / ack / cancel sequences against list bookkeeping under
// AddressSanitizer and UndefinedBehaviorSanitizer).  Entries keep absolute 1-based indices; the live ones are
// evicted + 1 .. count, entry i in slot (i - 1) mod slots of a ring of header_table_size / 32 slots; their
// strings lie in insert order as one contiguous run of the string area.
#ifndef HHUFF_QTABLE_H
#define HHUFF_QTABLE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define HHUFF_QT_HD __host__ __device__ inline
#else
#define HHUFF_QT_HD inline
#endif

namespace hhuff {
struct QsEntry {
    uint32_t noff, nl, vl, nh, vh, pad0, pad1, pad2;  // name at str + noff, value behind it
};

constexpr uint32_t kQtNoInsert = 0xFFFFFFFFu;
constexpr uint32_t kQtMaxCount = 0x7FFFFFFFu;  // a connection stops inserting here

HHUFF_QT_HD uint32_t qt_slots(uint32_t cap) { return cap / 32u; }
HHUFF_QT_HD uint32_t qt_slot(uint32_t index, uint32_t slots) { return (index - 1u) % slots; }  // index >= 1, slots >= 1
HHUFF_QT_HD uint32_t qt_next(uint32_t slot, uint32_t slots) { return slot + 1u == slots ? 0u : slot + 1u; }
HHUFF_QT_HD uint32_t qt_prev(uint32_t slot, uint32_t slots) { return (slot == 0u ? slots : slot) - 1u; }

// lookup bounds: the scan runs from here down to evicted + 1 (nothing when this is <= evicted)
HHUFF_QT_HD uint32_t qt_scan_top(uint32_t count, uint32_t lkr, bool acked_only) {
    return acked_only && lkr < count ? lkr : count;
}

// The insert rule's room test: entries evicted + 1, evicted + 2, ... go, in order and only below `pin` (the
// smallest pinned index; anything above count when nothing is pinned), until used + need <= cap.  -> the new
// `evicted` and the bytes left in `used_after`, or kQtNoInsert (then nothing is to be evicted).
HHUFF_QT_HD uint32_t qt_evict_prefix(const QsEntry* ent, uint32_t slots, uint32_t cap, uint32_t used, uint32_t evicted,
                                     uint32_t count, uint32_t pin, uint64_t need, uint32_t& used_after) {
    if (need > cap || count >= kQtMaxCount) return kQtNoInsert;
    uint32_t e = evicted, u = used;
    if ((uint64_t)u + need <= cap) {
        used_after = u;
        return e;
    }
    uint32_t slot = qt_slot(e + 1u, slots);  // used != 0: a live entry, so slots >= 1
    while ((uint64_t)u + need > cap) {
        if (e >= count || e + 1u >= pin) return kQtNoInsert;
        u -= ent[slot].nl + ent[slot].vl + 32u;
        slot = qt_next(slot, slots);
        ++e;
    }
    used_after = u;
    return e;
}

// HHUFF_QENC_DUP's draining test of the live entry i (evicted < i <= count): headroom = the free bytes and the
// bytes of the live entries older than i, what inserts can still take before i has to go; i is draining when
// that is under a quarter of the table.  The strings are one run in insert order, so the older entries' bytes
// are the distance between the two names and 32 an entry: no walk.
HHUFF_QT_HD bool qt_draining(const QsEntry* ent, uint32_t slots, uint32_t cap, uint32_t used, uint32_t evicted, uint32_t i) {
    const uint32_t run = ent[qt_slot(i, slots)].noff - ent[qt_slot(evicted + 1u, slots)].noff;
    return (cap - used) + run + 32u * (i - evicted - 1u) < cap / 4u;
}

// String compaction: the live run [noff of entry evicted + 1, str_used) moves to offset 0 and the live entries'
// noff are rebased.  -> the new str_used
HHUFF_QT_HD uint32_t qt_compact(uint8_t* str, QsEntry* ent, uint32_t slots, uint32_t evicted, uint32_t count, uint32_t str_used) {
    if (evicted >= count) return 0u;
    uint32_t slot = qt_slot(evicted + 1u, slots);
    const uint32_t start = ent[slot].noff;
    if (start == 0u) return str_used;
    for (uint32_t k = start; k < str_used; ++k) str[k - start] = str[k];  // downwards: ascending copy is safe
    for (uint32_t i = evicted; i < count; ++i) {
        ent[slot].noff -= start;
        slot = qt_next(slot, slots);
    }
    return str_used - start;
}

// where an insert's strings (len = name_len + value_len) go in a string area of str_cap bytes: behind the run,
// after compaction when the tail lacks room.  The table's accounting (used + len + 32 <= cap <= str_cap, 32 bytes
// an entry) guarantees that the compacted run leaves the room.
HHUFF_QT_HD uint32_t qt_place(uint8_t* str, uint32_t str_cap, QsEntry* ent, uint32_t slots, uint32_t evicted, uint32_t count,
                              uint32_t str_used, uint32_t len) {
    if ((uint64_t)str_used + len > str_cap) str_used = qt_compact(str, ent, slots, evicted, count, str_used);
    return str_used;
}
}  // namespace hhuff
#endif
