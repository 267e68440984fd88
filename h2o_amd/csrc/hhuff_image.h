// Connection images (include/hhuff.h (2i)): the layout arithmetic of the five slab families, the image format and
// its validator, for the device (hhuff_image.hip: one wave per listed connection) and for the host
// (tools/image_host.cpp packs, unpacks and mutates images under AddressSanitizer and UndefinedBehaviorSanitizer
// with the serial img_pack / img_unpack below, which run the same pieces entry by entry).
//
// An image is [Header 32 B][State 64 B][nent x Rec 32 B][nlist x 16 B][string run, zero-padded to 16 B]:
//   Header  magic "HHCI", u16 version, u16 family, u32 table_size, max_inflight, max_blocked, u32 total length,
//           two reserved words (0)
//   State   one record for every family (fields a family has no use for are 0), see State
//   Rec     the live table entries, oldest first: lengths and what the family keeps beside them; the strings of
//           entry j lie in the run at the sum of the lengths before it, name first
//   list    QPACK_ENC: the inflight records {u64 stream, u32 largest, u32 smallest | blocking << 31 (evicting) or
//           blocking}; QPACK_DSESSION: the parked streams {u64 stream, u64 Required Insert Count}, oldest first
// No scratch offset, ring index or ring start is kept: import places the entries from ring slot 0 (the QPACK
// encoder's at the slots their absolute indices name) and the bytes from the start of ring 0.
//
// The slab structs below restate the families' private records (hhuff_blocks.hip, hhuff_qpack.hip,
// hhuff_hpenc.hip, hhuff_qpenc.hip); each of those files asserts that its own records match them.
#ifndef HHUFF_IMAGE_H
#define HHUFF_IMAGE_H
#include <stdint.h>
#include <string.h>

#include "hhuff.h"
#include "hhuff_qpark.h"
#include "hhuff_qtable.h"

#if defined(__HIPCC__)
#define HHUFF_IMG_HD __host__ __device__ inline
#else
#define HHUFF_IMG_HD inline
#endif

namespace hhuff {
namespace img {
// ---- the slabs ----
struct BlkState {  // HPACK_DEC: [BlkState][E x BlkEntry][ring 0][ring 1], entries newest first from `start`
    uint32_t start, num, ring, failed;
    uint64_t size, cap;
};
struct BlkEntry {
    uint64_t nsrc, vsrc;
    uint32_t nl, vl;
    uint16_t soft, cls;
    uint32_t pad;
};
struct QdState {  // QPACK_DEC: [QdState][E x QdEntry][ring 0][ring 1], entries oldest first from `start`
    int64_t base_offset;
    uint64_t total_inserts, num_bytes, max_size;
    uint32_t start, num, ring, failed;
    uint32_t dirty, pad[3];
};
struct QdEntry {
    uint64_t nsrc, vsrc;
    uint32_t nl, vl, soft, pad;
};
struct HeState {  // HPACK_ENC: [HeState][32 x HeEntry][ring 0][ring 1], entries newest first from `start`
    uint32_t start, num, ring, failed;
    uint32_t size, cap, pad0, pad1;
};
struct HeEntry {
    uint64_t nsrc, vsrc;
    uint32_t nl, vl, nh, vh;
    uint32_t tok, pad;
};
struct QeState {  // QPACK_ENC: [QeState][H / 32 x QsEntry][M x QeInflight][strings]: entry i in slot (i - 1) mod slots
    uint32_t count, used, lkr, num_blocked, ninflight, failed, str_used, evicted;
};
struct QeInflight {
    uint64_t sid;
    uint32_t largest, blocking;
};
static_assert(sizeof(BlkState) == 32 && sizeof(BlkEntry) == 32 && sizeof(QdState) == 64 && sizeof(QdEntry) == 32 &&
                  sizeof(HeState) == 32 && sizeof(HeEntry) == 40 && sizeof(QeState) == 32 && sizeof(QeInflight) == 16,
              "slab records");
constexpr uint64_t kBlkScr = 2ull << 61, kBlkOff = (1ull << 61) - 1;  // kSrcScr | offset (hhuff_blocks.hip)
constexpr uint64_t kQdScr = 2ull << 61, kQdOff = (1ull << 61) - 1;    // kQScr | offset (hhuff_qpack.hip)
constexpr uint64_t kHeScr = 1ull << 62, kHeOff = (1ull << 62) - 1;    // kSrcScr | offset (hhuff_hpenc.hip)
constexpr uint32_t kClsUnknown = 0xFFFFu;  // BlkEntry::cls "not computed yet": what an imported entry carries
constexpr uint32_t kHeEntries = 32, kHeRing = 4096, kHeCap = 4096;
constexpr uint32_t kQeEvicting = 2u, kQeDuplicating = 4u;  // QeState::failed
constexpr uint32_t kMaxTable = 1u << 30;  // image lengths are u32

// ---- the image ----
constexpr uint32_t kMagic = 0x49434848u;  // "HHCI"
constexpr uint32_t kVersion = 1;
struct Header {
    uint32_t magic;
    uint16_t version, family;
    uint32_t table_size, max_inflight, max_blocked;
    uint32_t total;  // bytes of the image, a multiple of 16
    uint32_t rsv0, rsv1;
};
struct State {
    uint32_t nent, nlist;  // table entries; inflight (QPACK_ENC) / parked (QPACK_DSESSION) records
    uint32_t str_bytes;    // the string run
    uint32_t failed;       // the connection's failed flag; QPACK_ENC: with the session's mode bits
    uint64_t size;         // the entries' bytes + 32 each (HPACK size, QPACK num_bytes / used)
    uint64_t cap;          // the table's capacity now (QPACK_ENC: header_table_size)
    uint64_t counter;      // QPACK_DEC total_inserts, QPACK_ENC count, QPACK_DSESSION known_received
    uint32_t lkr, num_blocked, evicted;  // QPACK_ENC
    uint32_t rsv0, rsv1, rsv2;
};
struct Rec {
    uint32_t nl, vl;
    uint32_t a, b, c;  // HPACK_DEC, QPACK_DEC: soft bits; HPACK_ENC: name hash, value hash, token; QPACK_ENC: the hashes
    uint32_t rsv0, rsv1, rsv2;
};
static_assert(sizeof(Header) == 32 && sizeof(State) == 64 && sizeof(Rec) == 32, "image records");
constexpr uint32_t kFixed = sizeof(Header) + sizeof(State);
constexpr uint64_t kMaxImage = 0xFFFFFFF0ull;  // the longest image img_len can state

struct Layout {  // a family's slab
    uint32_t family, T;
    uint32_t E, L;  // entry ring slots; list capacity
    uint32_t ent_stride;
    uint64_t ent_off, list_off, str_off, str_cap, slab;
    uint64_t cap_max;
};

HHUFF_IMG_HD uint64_t up16(uint64_t x) { return (x + 15u) & ~15ull; }

// false: parameters the family's own call refuses (or tables an image length cannot express)
HHUFF_IMG_HD bool layout(const hhuff_conn_family_t& f, Layout& L) {
    L = Layout{};
    L.family = f.family;
    L.T = f.table_size;
    switch (f.family) {
        case HHUFF_FAM_HPACK_DEC:
            if (f.max_inflight || f.max_blocked || f.table_size > kMaxTable) return false;
            L.E = f.table_size / 32u + 1u;
            L.ent_stride = sizeof(BlkEntry);
            L.ent_off = sizeof(BlkState);
            L.str_cap = up16(f.table_size);
            L.str_off = L.ent_off + (uint64_t)L.E * L.ent_stride;
            L.slab = L.str_off + 2u * L.str_cap;
            L.cap_max = f.table_size;
            return true;
        case HHUFF_FAM_QPACK_DEC:
            if (f.max_inflight || f.max_blocked || f.table_size > kMaxTable) return false;
            L.E = f.table_size / 32u + 1u;
            L.ent_stride = sizeof(QdEntry);
            L.ent_off = sizeof(QdState);
            L.str_cap = up16(f.table_size < 16u ? 16u : f.table_size);
            L.str_off = L.ent_off + (uint64_t)L.E * L.ent_stride;
            L.slab = L.str_off + 2u * L.str_cap;
            L.cap_max = f.table_size;
            return true;
        case HHUFF_FAM_HPACK_ENC:
            if (f.table_size || f.max_inflight || f.max_blocked) return false;
            L.E = kHeEntries;
            L.ent_stride = sizeof(HeEntry);
            L.ent_off = sizeof(HeState);
            L.str_cap = kHeRing;
            L.str_off = L.ent_off + (uint64_t)L.E * L.ent_stride;
            L.slab = L.str_off + 2u * L.str_cap;
            L.cap_max = kHeCap;
            return true;
        case HHUFF_FAM_QPACK_ENC:
            if (f.max_blocked || f.table_size > 65536u) return false;
            L.E = qt_slots(f.table_size);
            L.L = f.max_inflight;
            L.ent_stride = sizeof(QsEntry);
            L.ent_off = sizeof(QeState);
            L.list_off = L.ent_off + (uint64_t)L.E * L.ent_stride;
            L.str_off = L.list_off + (uint64_t)L.L * sizeof(QeInflight);
            L.str_cap = up16(f.table_size);
            L.slab = L.str_off + L.str_cap;
            L.cap_max = f.table_size;
            return true;
        case HHUFF_FAM_QPACK_DSESSION:
            if (f.table_size || f.max_inflight || f.max_blocked > kQpMaxBlocked) return false;
            L.L = f.max_blocked;
            L.list_off = sizeof(QpHead);
            L.slab = qp_slab_bytes(f.max_blocked);
            return true;
        default: return false;
    }
}

HHUFF_IMG_HD uint64_t image_bytes(uint64_t nent, uint64_t nlist, uint64_t str_bytes) {
    return kFixed + sizeof(Rec) * nent + 16u * nlist + up16(str_bytes);
}
// hhuff_conn_image_bound: 96 + 32 records + string bytes + 15 at the family's maxima, rounded up to 16
HHUFF_IMG_HD uint64_t image_bound(const Layout& L) { return up16(kFixed + 32u * ((uint64_t)L.E + L.L) + L.str_cap + 15u); }

template <class T>
HHUFF_IMG_HD T load(const uint8_t* p) {
    T v;
    memcpy(&v, p, sizeof(T));
    return v;
}
template <class T>
HHUFF_IMG_HD void store(uint8_t* p, const T& v) {
    memcpy(p, &v, sizeof(T));
}

// The state of a slab as the image keeps it (str_bytes left 0: the entries say), counts clamped to the slab's
// rings so that whatever the slab holds no later read leaves it.  start: where the entry ring begins.
HHUFF_IMG_HD State state_load(const Layout& L, const uint8_t* slab, uint32_t& start) {
    State s{};
    start = 0;
    switch (L.family) {
        case HHUFF_FAM_HPACK_DEC: {
            const BlkState t = load<BlkState>(slab);
            s.nent = t.num, s.failed = t.failed, s.size = t.size, s.cap = t.cap;
            start = t.start;
        } break;
        case HHUFF_FAM_QPACK_DEC: {
            const QdState t = load<QdState>(slab);
            s.nent = t.num, s.failed = t.failed, s.size = t.num_bytes, s.cap = t.max_size, s.counter = t.total_inserts;
            start = t.start;
        } break;
        case HHUFF_FAM_HPACK_ENC: {
            const HeState t = load<HeState>(slab);
            s.nent = t.num, s.failed = t.failed, s.size = t.size, s.cap = t.cap;
            start = t.start;
        } break;
        case HHUFF_FAM_QPACK_ENC: {
            const QeState t = load<QeState>(slab);
            s.nent = t.count >= t.evicted ? t.count - t.evicted : 0u;
            s.nlist = t.ninflight, s.failed = t.failed, s.size = t.used, s.cap = L.T, s.counter = t.count;
            s.lkr = t.lkr, s.num_blocked = t.num_blocked, s.evicted = t.evicted;
        } break;
        default: {
            const QpHead t = load<QpHead>(slab);
            s.nlist = t.parked, s.counter = t.known_received;
        } break;
    }
    if (s.nent > L.E) s.nent = L.E;
    if (s.nlist > L.L) s.nlist = L.L;
    if (L.E) start %= L.E;
    return s;
}

// ring slot of the j-th oldest of the state's nent entries (j < nent <= E)
HHUFF_IMG_HD uint32_t entry_slot(const Layout& L, const State& s, uint32_t start, uint32_t j) {
    if (L.family == HHUFF_FAM_QPACK_ENC) return (uint32_t)(((uint64_t)s.evicted + j) % L.E);
    const uint32_t k = L.family == HHUFF_FAM_QPACK_DEC ? j : s.nent - 1u - j;
    const uint64_t i = (uint64_t)start + k;
    return (uint32_t)(i >= L.E ? i - L.E : i);
}

// a string of an entry: its place in the slab (sbase: the slab's offset in scratch), or length 0 when the
// reference does not lie inside the slab (a slab no call wrote)
HHUFF_IMG_HD uint64_t src_in_slab(const Layout& L, uint64_t src, uint64_t tag, uint64_t mask, uint64_t sbase, uint32_t& len) {
    const uint64_t o = src & mask;
    if ((src & ~mask) != tag || len > L.str_cap || o < sbase || o - sbase > L.slab || len > L.slab - (o - sbase)) {
        len = 0;
        return 0;
    }
    return o - sbase;
}

// entry `slot` of a slab: its image record and where its name and value lie in the slab
HHUFF_IMG_HD Rec entry_load(const Layout& L, const uint8_t* slab, uint64_t sbase, uint32_t slot, uint64_t& noff, uint64_t& voff) {
    Rec r{};
    const uint8_t* p = slab + L.ent_off + (uint64_t)slot * L.ent_stride;
    switch (L.family) {
        case HHUFF_FAM_HPACK_DEC: {
            const BlkEntry e = load<BlkEntry>(p);
            r.nl = e.nl, r.vl = e.vl, r.a = e.soft;
            noff = src_in_slab(L, e.nsrc, kBlkScr, kBlkOff, sbase, r.nl);
            voff = src_in_slab(L, e.vsrc, kBlkScr, kBlkOff, sbase, r.vl);
        } break;
        case HHUFF_FAM_QPACK_DEC: {
            const QdEntry e = load<QdEntry>(p);
            r.nl = e.nl, r.vl = e.vl, r.a = e.soft;
            noff = src_in_slab(L, e.nsrc, kQdScr, kQdOff, sbase, r.nl);
            voff = src_in_slab(L, e.vsrc, kQdScr, kQdOff, sbase, r.vl);
        } break;
        case HHUFF_FAM_HPACK_ENC: {
            const HeEntry e = load<HeEntry>(p);
            r.nl = e.nl, r.vl = e.vl, r.a = e.nh, r.b = e.vh, r.c = e.tok;
            noff = src_in_slab(L, e.nsrc, kHeScr, kHeOff, sbase, r.nl);
            voff = src_in_slab(L, e.vsrc, kHeScr, kHeOff, sbase, r.vl);
        } break;
        default: {  // QPACK_ENC
            const QsEntry e = load<QsEntry>(p);
            r.nl = e.nl, r.vl = e.vl, r.a = e.nh, r.b = e.vh;
            if (e.noff > L.str_cap || r.nl > L.str_cap - e.noff || r.vl > L.str_cap - e.noff - r.nl) r.nl = r.vl = 0;
            noff = L.str_off + (r.nl || r.vl ? e.noff : 0u);
            voff = noff + r.nl;
        } break;
    }
    return r;
}

// import: entry `slot` of the slab from its record, its strings at `run` in ring 0 / the string area
HHUFF_IMG_HD void entry_store(const Layout& L, uint8_t* slab, uint64_t sbase, uint32_t slot, const Rec& r, uint32_t run) {
    uint8_t* p = slab + L.ent_off + (uint64_t)slot * L.ent_stride;
    const uint64_t n = sbase + L.str_off + run, v = n + r.nl;
    switch (L.family) {
        case HHUFF_FAM_HPACK_DEC:
            store(p, BlkEntry{kBlkScr | n, kBlkScr | v, r.nl, r.vl, (uint16_t)r.a, (uint16_t)kClsUnknown, 0u});
            break;
        case HHUFF_FAM_QPACK_DEC: store(p, QdEntry{kQdScr | n, kQdScr | v, r.nl, r.vl, r.a, 0u}); break;
        case HHUFF_FAM_HPACK_ENC: store(p, HeEntry{kHeScr | n, kHeScr | v, r.nl, r.vl, r.a, r.b, r.c, 0u}); break;
        default: store(p, QsEntry{run, r.nl, r.vl, r.a, r.b, 0u, 0u, 0u}); break;
    }
}

// import: the slab's state record, entry ring from slot 0, bytes in ring 0
HHUFF_IMG_HD void state_store(const Layout& L, uint8_t* slab, const State& s) {
    switch (L.family) {
        case HHUFF_FAM_HPACK_DEC: store(slab, BlkState{0u, s.nent, 0u, s.failed, s.size, s.cap}); break;
        case HHUFF_FAM_QPACK_DEC:
            store(slab, QdState{(int64_t)(s.counter + 1u - s.nent), s.counter, s.size, s.cap, 0u, s.nent, 0u, s.failed, 0u, {0u, 0u, 0u}});
            break;
        case HHUFF_FAM_HPACK_ENC: store(slab, HeState{0u, s.nent, 0u, s.failed, (uint32_t)s.size, (uint32_t)s.cap, 0u, 0u}); break;
        case HHUFF_FAM_QPACK_ENC:
            store(slab, QeState{(uint32_t)s.counter, (uint32_t)s.size, s.lkr, s.num_blocked, s.nlist, s.failed, s.str_bytes, s.evicted});
            break;
        default: store(slab, QpHead{s.nlist, 0u, s.counter}); break;
    }
}

HHUFF_IMG_HD Header make_header(const hhuff_conn_family_t& f, uint32_t total) {
    return Header{kMagic, (uint16_t)kVersion, (uint16_t)f.family, f.table_size, f.max_inflight, f.max_blocked, total, 0u, 0u};
}

// ---- the validator: an image is bytes from anywhere ----
// the header of an image of `len` bytes against the call's family: 0, HHUFF_IMG_EFORMAT or HHUFF_IMG_EPARAM
HHUFF_IMG_HD int32_t check_header(const hhuff_conn_family_t& f, const Header& h, uint64_t len) {
    if (h.magic != kMagic || h.version != kVersion || h.total != len || h.rsv0 || h.rsv1) return HHUFF_IMG_EFORMAT;
    if (h.family != f.family || h.table_size != f.table_size || h.max_inflight != f.max_inflight || h.max_blocked != f.max_blocked)
        return HHUFF_IMG_EPARAM;
    return 0;
}

// the state record: every count inside its ring, the byte accounting closed, the image exactly as long as it
// says.  What is left for the caller to check per record: check_rec over the entries with the sum of their
// lengths == str_bytes, check_list over the list records, zero pad bytes.
HHUFF_IMG_HD bool check_state(const Layout& L, const State& s, uint64_t len) {
    if (s.rsv0 || s.rsv1 || s.rsv2) return false;
    if (s.nent > L.E || s.nlist > L.L || s.str_bytes > L.str_cap) return false;
    if (image_bytes(s.nent, s.nlist, s.str_bytes) != len) return false;
    if (s.size != (uint64_t)s.str_bytes + 32ull * s.nent || s.size > s.cap || s.cap > L.cap_max) return false;
    switch (L.family) {
        case HHUFF_FAM_HPACK_DEC:
        case HHUFF_FAM_HPACK_ENC: return s.failed <= 1u && !s.counter && !s.lkr && !s.num_blocked && !s.evicted;
        case HHUFF_FAM_QPACK_DEC: return s.failed <= 1u && s.counter >= s.nent && !s.lkr && !s.num_blocked && !s.evicted;
        case HHUFF_FAM_QPACK_ENC:
            if (s.failed > 7u || ((s.failed & kQeDuplicating) && !(s.failed & kQeEvicting))) return false;
            if (!(s.failed & kQeEvicting) && s.evicted) return false;
            return s.cap == L.T && s.counter <= kQtMaxCount && s.evicted <= s.counter && s.counter - s.evicted == s.nent &&
                   s.lkr <= s.counter && s.num_blocked <= s.nlist;
        default: return !s.failed && !s.lkr && !s.num_blocked && !s.evicted;
    }
}

HHUFF_IMG_HD bool check_rec(const Layout& L, const State& s, const Rec& r) {
    if (r.rsv0 || r.rsv1 || r.rsv2) return false;
    if (r.nl > s.str_bytes || r.vl > s.str_bytes - r.nl) return false;
    switch (L.family) {
        case HHUFF_FAM_HPACK_DEC: return r.a <= 0xFFFFu && !r.b && !r.c;
        case HHUFF_FAM_QPACK_DEC: return !r.b && !r.c;
        case HHUFF_FAM_HPACK_ENC: return r.c <= 1u;
        default: return !r.c;
    }
}

// a list record (16 bytes at p): an inflight section refers to no entry past the table's count
HHUFF_IMG_HD bool check_list(const Layout& L, const State& s, const uint8_t* p) {
    if (L.family != HHUFF_FAM_QPACK_ENC) return true;
    return load<QeInflight>(p).largest <= s.counter;
}

// ---- serial pack / unpack (the host's; the kernels do the same with a wave) ----
// -> 0 with *len = the image's bytes written to out[0 .. room); HHUFF_IMG_SPACE with *len = the bytes needed
HHUFF_IMG_HD int32_t img_pack(const hhuff_conn_family_t& f, const Layout& L, const uint8_t* scratch, uint64_t slot, uint8_t* out,
                              uint64_t room, uint32_t* len) {
    const uint64_t sbase = slot * L.slab;
    const uint8_t* slab = scratch + sbase;
    uint32_t start;
    State s = state_load(L, slab, start);
    uint64_t bytes = 0, no, vo;
    for (uint32_t j = 0; j < s.nent; ++j) {
        const Rec r = entry_load(L, slab, sbase, entry_slot(L, s, start, j), no, vo);
        bytes += (uint64_t)r.nl + r.vl;
    }
    if (bytes > L.str_cap) s.nent = 0, bytes = 0;  // not a table any call left
    s.str_bytes = (uint32_t)bytes;
    const uint64_t total = image_bytes(s.nent, s.nlist, bytes);
    *len = (uint32_t)(total > kMaxImage ? kMaxImage : total);
    if (total > kMaxImage) return HHUFF_IMG_SPACE;  // (an inflight list no u32 length can say: no image)
    if (!out) return 0;
    if (total > room) return HHUFF_IMG_SPACE;
    store(out, make_header(f, (uint32_t)total));
    store(out + sizeof(Header), s);
    uint8_t* recs = out + kFixed;
    uint8_t* list = recs + sizeof(Rec) * (uint64_t)s.nent;
    uint8_t* str = list + 16ull * s.nlist;
    uint64_t run = 0;
    for (uint32_t j = 0; j < s.nent; ++j) {
        const Rec r = entry_load(L, slab, sbase, entry_slot(L, s, start, j), no, vo);
        store(recs + sizeof(Rec) * (uint64_t)j, r);
        memcpy(str + run, slab + no, r.nl);
        memcpy(str + run + r.nl, slab + vo, r.vl);
        run += (uint64_t)r.nl + r.vl;
    }
    memcpy(list, slab + L.list_off, 16ull * s.nlist);
    for (uint64_t k = bytes; k < up16(bytes); ++k) str[k] = 0;
    return 0;
}

// every check of an image of `len` bytes: 0, HHUFF_IMG_EFORMAT or HHUFF_IMG_EPARAM; *sp = its state
HHUFF_IMG_HD int32_t img_check(const hhuff_conn_family_t& f, const Layout& L, const uint8_t* in, uint64_t len, State* sp) {
    if (len < kFixed || (len & 15u)) return HHUFF_IMG_EFORMAT;
    const int32_t rc = check_header(f, load<Header>(in), len);
    if (rc) return rc;
    const State s = load<State>(in + sizeof(Header));
    if (!check_state(L, s, len)) return HHUFF_IMG_EFORMAT;
    const uint8_t* recs = in + kFixed;
    const uint8_t* list = recs + sizeof(Rec) * (uint64_t)s.nent;
    const uint8_t* str = list + 16ull * s.nlist;
    uint64_t bytes = 0;
    for (uint32_t j = 0; j < s.nent; ++j) {
        const Rec r = load<Rec>(recs + sizeof(Rec) * (uint64_t)j);
        if (!check_rec(L, s, r)) return HHUFF_IMG_EFORMAT;
        bytes += (uint64_t)r.nl + r.vl;
    }
    if (bytes != s.str_bytes) return HHUFF_IMG_EFORMAT;
    for (uint32_t k = 0; k < s.nlist; ++k)
        if (!check_list(L, s, list + 16ull * k)) return HHUFF_IMG_EFORMAT;
    for (uint64_t k = bytes; k < up16(bytes); ++k)
        if (str[k]) return HHUFF_IMG_EFORMAT;
    *sp = s;
    return 0;
}

// -> img_check's verdict; 0: the slab of `slot` rebuilt, nothing written otherwise
HHUFF_IMG_HD int32_t img_unpack(const hhuff_conn_family_t& f, const Layout& L, uint8_t* scratch, uint64_t slot, const uint8_t* in,
                                uint64_t len) {
    State s;
    const int32_t rc = img_check(f, L, in, len, &s);
    if (rc) return rc;
    const uint64_t sbase = slot * L.slab;
    uint8_t* slab = scratch + sbase;
    const uint8_t* recs = in + kFixed;
    const uint8_t* list = recs + sizeof(Rec) * (uint64_t)s.nent;
    const uint8_t* str = list + 16ull * s.nlist;
    state_store(L, slab, s);
    uint32_t run = 0;
    for (uint32_t j = 0; j < s.nent; ++j) {
        const Rec r = load<Rec>(recs + sizeof(Rec) * (uint64_t)j);
        entry_store(L, slab, sbase, entry_slot(L, s, 0u, j), r, run);
        run += r.nl + r.vl;
    }
    memcpy(slab + L.str_off, str, s.str_bytes);
    memcpy(slab + L.list_off, list, 16ull * s.nlist);
    return 0;
}
}  // namespace img
}  // namespace hhuff
#endif
