// HTTP/2 scheduler (include/hhuff.h (2o)): h2o's lib/http2/scheduler.c over a flat node table, and
// h2o_http2_scheduler_run with emit_writereq_of_openref's rule.  The device kernel (hhuff_h2sched.hip) and the host
// program (tools/h2sched_host.cpp) run this very code; they differ in the steps over the table, which h2o makes as list
// walks and which are handed in as W:
//   W::uni(v)            a value every lane holds, as a scalar
//   W::find              a stream by id, a second one (the parent) and the first free entry, in one pass
//   W::first_child       the head of a node's _all_refs: the child with the lowest place
//   W::weight_sum        close's total over the children (0: none)
//   W::pop               queue_pop: the minimum over the queued children of (anchor257 first, ring distance from the
//                        parent's offset, place in the slot), and whether the slot holds another
//   W::any257            a child on anchor257 (queue_is_empty's second half)
//   W::append_unvisited  the candidates no visit took, behind the visits
// Everything else is serial and the same for every lane of the wave: a node's fields are written by all lanes with the
// same value, so each lane reads what it wrote itself.
//   offset_of      OFFSET_TABLE[weight - 1] of scheduler.c:55-73, computed: round(63 * 65536 / weight), 0 for 257
//   handed_weight  close's proportional hand-down
//   op_check       the refusals that need no tree
//   Sched          queue_set, incr / decr_active_cnt, do_rebind, rebind, convert_to_exclusive, open, close, proceed, run
#ifndef HHUFF_H2SCHED_H
#define HHUFF_H2SCHED_H
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_h2data.h"

#define HHUFF_SCHED_HD HHUFF_DATA_HD

namespace hhuff {
namespace h2q {

constexpr uint32_t kMagic = 0x51324848u;  // "HH2Q"
constexpr uint32_t kMaxNodes = 2048, kRoot = 0xFFFFu, kNone = 0xFFFFFFFFu;
constexpr uint32_t kHeaderBytes = 32, kNodeBytes = 24;
constexpr uint32_t kSlots = 64, kSlot257 = 64, kUnqueued = 255;
constexpr uint32_t kDefaultWeight = 16;  // h2o_http2_default_priority

struct Node {
    uint32_t id, aseq, qseq;
    uint16_t parent, weight, deficit, active_cnt;
    uint8_t slot, qoff, self_active, rsv;
};
struct Header {
    uint32_t magic, max_nodes, seq, nhigh;
    uint64_t root_bits;
    uint32_t root_qoff, count;
};
static_assert(sizeof(Node) == kNodeBytes && sizeof(Header) == kHeaderBytes, "the slab's layout");

HHUFF_SCHED_HD uint64_t slab_bytes(uint64_t max_nodes) { return (kHeaderBytes + kNodeBytes * max_nodes + 15u) & ~(uint64_t)15; }
HHUFF_SCHED_HD Header fresh_header(uint32_t max_nodes) { return Header{kMagic, max_nodes, 0, 0, 0, 0, 0}; }
HHUFF_SCHED_HD bool header_ok(const Header& h, uint32_t max_nodes) {
    return h.magic == kMagic && h.max_nodes == max_nodes && h.nhigh <= max_nodes && h.count <= h.nhigh && h.root_qoff < kSlots;
}
HHUFF_SCHED_HD bool node_ok(const Node& x, uint32_t nhigh) {
    return x.id == 0 || ((x.parent < nhigh || x.parent == kRoot) && x.weight >= 1 && x.weight <= 257 && x.qoff < kSlots &&
                         (x.slot <= kSlot257 || x.slot == kUnqueued) && x.self_active <= 1 && x.id <= 0x7fffffffu);
}

HHUFF_SCHED_HD uint32_t offset_of(uint32_t weight) { return weight > 256 ? 0u : (63u * 65536u + weight / 2u) / weight; }

HHUFF_SCHED_HD uint32_t handed_weight(uint32_t weight, uint32_t total, uint32_t child) {
    const uint32_t factor = (weight * 65536u + total / 2u) / total;
    const uint32_t w = (child * factor / 32768u + 1u) / 2u;
    return w < 1u ? 1u : (w > 256u ? 256u : w);
}

HHUFF_SCHED_HD int32_t op_check(const hhuff_h2_sched_op_t& o) {
    if (o.op < HHUFF_H2Q_OPEN || o.op > HHUFF_H2Q_DEACTIVATE || o.stream_id == 0 || o.stream_id > 0x7fffffffu || o.rsv != 0)
        return HHUFF_H2SC_EINVAL;
    if (o.op <= HHUFF_H2Q_REBIND)
        return o.parent_id > 0x7fffffffu || o.parent_id == o.stream_id || o.exclusive > 1 || o.weight < 1 || o.weight > 257 ? HHUFF_H2SC_EINVAL : 0;
    return o.parent_id != 0 || o.weight != 0 || o.exclusive != 0 ? HHUFF_H2SC_EINVAL : 0;
}

// h2d::send_ok's tests that need no body: a record that fails them is no candidate
HHUFF_SCHED_HD bool candidate_ok(uint32_t stream_id, uint32_t flags) {
    return stream_id != 0 && stream_id <= 0x7fffffffu && (flags & ~(HHUFF_H2S_FINAL | HHUFF_H2S_TRAILERS)) == 0;
}

// h2o_http2_conn_get_buffer_window without the latency optimisation, in the call's terms
HHUFF_SCHED_HD int64_t buffer_window(int64_t R, int64_t Wc) { return R < h2d::kHeaderSize ? 0 : h2d::min2(R - h2d::kHeaderSize, Wc); }

struct Popped {
    uint32_t idx;  // kNone: nothing queued
    uint32_t dist;  // 0: anchor257; else 1 + the ring distance
    bool more;      // the slot holds another node
};

// what a run writes: the visits in front of the connection's range of `ordered`
struct Visits {
    const hhuff_h2_send_t* sends;
    uint32_t lo, hi;  // the candidates
    hhuff_h2_send_t* ordered;
    uint32_t* order;
    uint32_t* pos;
    uint32_t n;
};

template <class W>
struct Sched {
    W& w;
    Node* n;         // max_nodes entries
    uint32_t* cand;  // per node: 1 + the index of its candidate, 0 without one
    Header h;
    uint32_t max_nodes;

    HHUFF_SCHED_HD void queue_set(uint32_t p, uint32_t i) {
        Node& x = n[i];
        uint32_t slot = kSlot257;
        if (x.weight <= 256) {
            uint32_t off = offset_of(x.weight) + x.deficit;
            x.deficit = (uint16_t)(off % 65536u), off /= 65536u;
            slot = ((p == kRoot ? h.root_qoff : n[p].qoff) + off) % kSlots;
            if (p == kRoot) h.root_bits |= 1ull << (63u - off);
        }
        x.slot = (uint8_t)slot, x.qseq = h.seq++;
    }
    // (the walks towards the root stop after max_nodes steps whatever a slab's parents say)
    HHUFF_SCHED_HD void incr_active_cnt(uint32_t i) {
        for (uint32_t s = 0; i != kRoot && s < max_nodes; ++s) {
            if (++n[i].active_cnt != 1) return;
            const uint32_t p = w.uni(n[i].parent);
            queue_set(p, i), i = p;
        }
    }
    HHUFF_SCHED_HD void decr_active_cnt(uint32_t i) {
        for (uint32_t s = 0; i != kRoot && s < max_nodes; ++s) {
            if (--n[i].active_cnt != 0) return;
            n[i].slot = kUnqueued, i = w.uni(n[i].parent);
        }
    }
    // do_rebind without its exclusive half
    HHUFF_SCHED_HD void relink(uint32_t i, uint32_t np) {
        Node& x = n[i];
        x.aseq = h.seq++;
        if (x.active_cnt != 0) {
            x.slot = kUnqueued;
            queue_set(np, i);
            decr_active_cnt(w.uni(x.parent));
            incr_active_cnt(np);
        }
        x.parent = (uint16_t)np;
    }
    // every child of p in front of `added` goes under it (rebind with its own weight: no other branch of rebind applies)
    HHUFF_SCHED_HD void convert_to_exclusive(uint32_t p, uint32_t added) {
        for (uint32_t s = 0; s < max_nodes; ++s) {
            const uint32_t c = w.first_child(n, h.nhigh, p, added);
            if (c == kNone) break;
            relink(c, added);
        }
    }
    HHUFF_SCHED_HD void rebind(uint32_t i, uint32_t np, uint32_t weight, bool exclusive) {
        Node& x = n[i];
        if (x.parent == np && x.weight == weight && !exclusive) return;
        x.weight = (uint16_t)weight;
        if (w.weight_sum(n, h.nhigh, i) != 0) {  // np under i: np becomes i's sibling first (draft-16 5.3.3)
            uint32_t t = np;
            for (uint32_t s = 0; t != kRoot && s < max_nodes; ++s) {
                const uint32_t tp = w.uni(n[t].parent);
                if (tp == i) {
                    relink(np, w.uni(x.parent));
                    break;
                }
                t = tp;
            }
        }
        relink(i, np);
        if (exclusive) convert_to_exclusive(np, i);
    }
    HHUFF_SCHED_HD void open(uint32_t i, uint32_t id, uint32_t p, uint32_t weight, bool exclusive) {
        n[i] = Node{id, h.seq++, 0, (uint16_t)p, (uint16_t)weight, 0, 0, (uint8_t)kUnqueued, 0, 0, 0};
        if (i >= h.nhigh) h.nhigh = i + 1u;
        ++h.count;
        if (exclusive) convert_to_exclusive(p, i);
    }
    HHUFF_SCHED_HD void close(uint32_t i) {
        Node& x = n[i];
        const uint32_t total = w.weight_sum(n, h.nhigh, i), p = w.uni(x.parent);
        if (total != 0) {
            for (uint32_t s = 0; s < max_nodes; ++s) {
                const uint32_t c = w.first_child(n, h.nhigh, i, kNone);
                if (c == kNone) break;
                n[c].weight = (uint16_t)handed_weight(x.weight, total, n[c].weight);
                relink(c, p);
            }
        }
        x.id = 0, --h.count;
        if (x.self_active) x.slot = kUnqueued, decr_active_cnt(p);
        while (h.nhigh != 0 && w.uni(n[h.nhigh - 1u].id) == 0) --h.nhigh;
    }
    HHUFF_SCHED_HD void activate(uint32_t i) {
        if (n[i].self_active) return;
        n[i].self_active = 1, incr_active_cnt(i);
    }
    HHUFF_SCHED_HD void deactivate(uint32_t i) {
        if (!n[i].self_active) return;
        n[i].self_active = 0, decr_active_cnt(i);
    }

    HHUFF_SCHED_HD int32_t apply(const hhuff_h2_sched_op_t& o) {
        const int32_t bad = op_check(o);
        if (bad != 0) return bad;
        uint32_t i, p, free_;
        w.find(n, h.nhigh, o.stream_id, o.parent_id, i, p, free_);
        uint32_t weight = o.weight;
        bool exclusive = o.exclusive != 0;
        if (o.op <= HHUFF_H2Q_REBIND) {
            if (o.parent_id == 0) p = kRoot;
            else if (p == kNone) p = kRoot, weight = kDefaultWeight, exclusive = false;  // set_priority's fallback
        }
        if (o.op == HHUFF_H2Q_OPEN) {
            if (i != kNone) return HHUFF_H2SC_EEXIST;
            if (free_ == kNone && h.nhigh < max_nodes) free_ = h.nhigh;
            if (free_ == kNone) return HHUFF_H2SC_EFULL;
            open(free_, o.stream_id, p, weight, exclusive);
            return 0;
        }
        if (i == kNone) return HHUFF_H2SC_ENOENT;
        if (o.op == HHUFF_H2Q_REBIND) rebind(i, p, weight, exclusive);
        else if (o.op == HHUFF_H2Q_CLOSE) close(i);
        else if (o.op == HHUFF_H2Q_ACTIVATE) activate(i);
        else deactivate(i);
        return 0;
    }

    // queue_pop on p's queue, with the bookkeeping of the root's bits: the shift to the slot found, its bit dropped
    // when the slot empties; nothing queued drops every (stale) bit
    HHUFF_SCHED_HD uint32_t queue_pop(uint32_t p) {
        const uint32_t qoff = p == kRoot ? h.root_qoff : n[p].qoff;
        const Popped P = w.pop(n, h.nhigh, p, qoff);
        if (P.idx == kNone) {
            if (p == kRoot) h.root_bits = 0;
            return kNone;
        }
        if (P.dist != 0) {
            const uint32_t d = P.dist - 1u;
            if (p == kRoot) {
                h.root_qoff = (qoff + d) % kSlots;
                h.root_bits <<= d;
                if (!P.more) h.root_bits &= ~(1ull << 63);
            } else {
                n[p].qoff = (uint8_t)((qoff + d) % kSlots);
            }
        }
        n[P.idx].slot = kUnqueued;
        return P.idx;
    }

    // proceed (scheduler.c:365-399) with emit_writereq_of_openref as the callback: 0 go on, 1 bail out, 2 nothing popped
    HHUFF_SCHED_HD int proceed(Visits& V, int64_t m, int64_t& R, int64_t& Wc) {
        uint32_t node = kRoot;
        for (uint32_t s = 0; s <= max_nodes; ++s) {
            const uint32_t i = queue_pop(node);
            if (i == kNone) return node == kRoot ? 2 : 0;
            Node& x = n[i];
            if (!x.self_active) {  // run the children
                queue_set(node, i), node = i;
                continue;
            }
            bool still = false;
            int bail = 0;
            const uint32_t j = w.uni(cand[i]);
            if (j != 0 && V.lo + V.n < V.hi) {
                const hhuff_h2_send_t S = V.sends[j - 1u];
                const h2d::Frames F = h2d::record(m, R, Wc, S.window, S.body_len, (S.flags & HHUFF_H2S_FINAL) != 0,
                                                  (S.flags & HHUFF_H2S_TRAILERS) != 0, 0);
                const int64_t bytes = F.bytes(m), k = F.count();
                R -= bytes + k * h2d::kHeaderSize, Wc -= bytes;
                still = (F.flags & HHUFF_H2T_DONE) == 0 && (int64_t)S.window - bytes > 0;
                V.ordered[V.lo + V.n] = S, V.order[V.lo + V.n] = j - 1u, V.pos[j - 1u] = V.n, ++V.n;
                cand[i] = 0;
                bail = buffer_window(R, Wc) > 0 ? 0 : 1;
            }
            if (still) {
                queue_set(node, i);
            } else {
                x.self_active = 0;
                if (--x.active_cnt != 0) queue_set(node, i);
                else decr_active_cnt(w.uni(x.parent));
            }
            return bail;
        }
        return 0;
    }

    HHUFF_SCHED_HD uint32_t run(Visits& V, int64_t m, int64_t R, int64_t Wc) {
        for (uint32_t j = V.lo; j < V.hi; ++j) {  // a stream's first candidate is its candidate
            V.pos[j] = kNone;
            const uint32_t id = w.uni(V.sends[j].stream_id), fl = w.uni(V.sends[j].flags);
            if (!candidate_ok(id, fl)) continue;  // (the framer would refuse it: it is never visited)
            uint32_t i, p, free_;
            w.find(n, h.nhigh, id, 0, i, p, free_);
            if (i != kNone && cand[i] == 0) cand[i] = j + 1u;
        }
        if (buffer_window(R, Wc) > 0)
            for (uint32_t s = 0; s <= h.count + 1u; ++s)  // (a proceed that goes on has put one stream to rest)
                if (proceed(V, m, R, Wc) != 0) break;
        const uint32_t nvisit = V.n;
        w.append_unvisited(V);
        return nvisit;
    }

    HHUFF_SCHED_HD bool is_active() { return h.root_bits != 0 || w.any257(n, h.nhigh, kRoot); }
};

}  // namespace h2q
}  // namespace hhuff
#endif
