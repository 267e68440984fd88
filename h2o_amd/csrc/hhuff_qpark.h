// QPACK decoder sessions (include/hhuff.h (2i)): the parked-streams list of a connection and the Known Received
// Count, for the device (hhuff_qpack.hip qpack_dsession_kernel) and for the host (tools/qpark_host.cpp replays
// random park / resubmit / cancel / wake sequences against std::map bookkeeping under AddressSanitizer and
// UndefinedBehaviorSanitizer).  A session slab is [QpHead 16 B][max_blocked x QpEntry 16 B]: the entries in
// the order their streams were parked, oldest first, back to back from entry 0.  No addresses are kept.
#ifndef HHUFF_QPARK_H
#define HHUFF_QPARK_H
#include <stdint.h>

#if defined(__HIPCC__)
#define HHUFF_QP_HD __host__ __device__ inline
#else
#define HHUFF_QP_HD inline
#endif

namespace hhuff {
struct QpEntry {  // a parked stream: h2o's stream->qpack_blocked_ref (lib/http3/server.c:245)
    uint64_t stream_id, ref;
};
struct QpHead {
    uint32_t parked, pad;     // conn->num_qpack_blocked (server.c:133)
    uint64_t known_received;  // RFC 9204 4.4: what the peer's encoder knows of this decoder's Insert Count
};
static_assert(sizeof(QpEntry) == 16 && sizeof(QpHead) == 16, "session slab layout");

constexpr uint32_t kQpMaxBlocked = 4096;
constexpr uint32_t kQpIntMax = 11;  // bytes of a prefix integer of a 64-bit value

HHUFF_QP_HD uint64_t qp_slab_bytes(uint32_t max_blocked) { return sizeof(QpHead) + (uint64_t)max_blocked * sizeof(QpEntry); }
// hhuff_qpack_dsession_out_bound
HHUFF_QP_HD uint64_t qp_out_bound(uint64_t nsec, uint64_t ncancel) { return 10u * (nsec + ncancel) + 10u; }

// the entry of stream `id`, or n when it is not parked
HHUFF_QP_HD uint32_t qp_find(const QpEntry* ent, uint32_t n, uint64_t id) {
    uint32_t i = 0;
    while (i < n && ent[i].stream_id != id) ++i;
    return i;
}

// a stream joins the list behind the others (server.c:1551-1555); false: no slot free
HHUFF_QP_HD bool qp_park(QpEntry* ent, uint32_t& n, uint32_t cap, uint64_t id, uint64_t ref) {
    if (n >= cap) return false;
    ent[n].stream_id = id;
    ent[n].ref = ref;
    ++n;
    return true;
}

// entry i (i < n) leaves, the later ones keep their order
HHUFF_QP_HD void qp_remove(QpEntry* ent, uint32_t& n, uint32_t i) {
    for (uint32_t k = i + 1; k < n; ++k) ent[k - 1] = ent[k];
    --n;
}

// qpack_unblock_streams (server.c:1950-1966): every entry whose ref the table's `total` inserts reach leaves, its
// stream id written to out[0 .. room) in list order; entries that are due and find out full stay (pending = true).
// -> the number written
HHUFF_QP_HD uint32_t qp_wake(QpEntry* ent, uint32_t& n, uint64_t total, uint64_t* out, uint32_t room, bool& pending) {
    uint32_t w = 0, keep = 0;
    pending = false;
    for (uint32_t i = 0; i < n; ++i) {
        const QpEntry e = ent[i];
        if (e.ref <= total) {
            if (w < room) {
                out[w++] = e.stream_id;
                continue;
            }
            pending = true;
        }
        ent[keep++] = e;
    }
    n = keep;
    return w;
}

// a Section Acknowledgment of a section with Required Insert Count ric (RFC 9204 4.4.1)
HHUFF_QP_HD uint64_t qp_acknowledged(uint64_t known_received, uint64_t ric) {
    return ric > known_received ? ric : known_received;
}

// the Insert Count Increment that brings the peer to `total`: 0 = none to send
HHUFF_QP_HD uint64_t qp_increment(uint64_t total, uint64_t known_received) {
    return total > known_received ? total - known_received : 0u;
}

// h2o_hpack_encode_int (lib/http2/hpack.c:757-772): v behind `first` with a prefix of `bits` bits -> bytes written
// (at most kQpIntMax)
HHUFF_QP_HD uint32_t qp_put_int(uint8_t* out, uint32_t first, uint64_t v, uint32_t bits) {
    const uint64_t mask = (1u << bits) - 1u;
    if (v < mask) {
        out[0] = (uint8_t)(first | v);
        return 1;
    }
    uint32_t n = 0;
    out[n++] = (uint8_t)(first | mask);
    v -= mask;
    while (v >= 128u) {
        out[n++] = (uint8_t)(0x80u | (v & 0x7Fu));
        v >>= 7;
    }
    out[n++] = (uint8_t)v;
    return n;
}
}  // namespace hhuff
#endif
