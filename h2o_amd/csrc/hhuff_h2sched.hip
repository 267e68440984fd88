// HTTP/2 scheduler on the device (include/hhuff.h (2o), hhuff_h2sched.h).
//   h2_schedule_kernel   one wave (a workgroup of 64) per connection.  The connection's node table is loaded from its slab
//     into LDS once, stays there for the whole op list and the run, and goes back once.  Dynamic LDS, sized from
//     max_nodes: 24 bytes a node and one dword a node for its candidate's index.
//     h2o's scheduler is 65 list anchors a parent and pointers everywhere; here a parent owns nothing but a ring offset
//     and every list walk of h2o is a step of the whole wave over the table, lane l on entries l, l + 64, ...:
//       find          three ballots a round of 64 entries: the stream, the parent and the first free entry in one pass
//       first_child   _all_refs.next: every lane keeps its lowest (place, index) key, the wave's minimum by five
//                     ds_swizzle butterflies inside the halves and two v_readlane across them
//       weight_sum    close's total by the same butterfly with an add
//       pop           queue_pop: the key is (0 for anchor257 else 1 + the distance of the node's ring slot from the
//                     parent's offset, the place in the slot, the index); a lane keeps its two lowest keys, so one
//                     ballot behind the minimum says whether the slot holds another node (the root's bits need it)
//     What h2o does between those walks -- queue_set, the counts towards the root, rebind's checks, the visit's
//     arithmetic -- is the serial code of hhuff_h2sched.h, run by all 64 lanes on the same values; every lane stores a
//     node's field itself, so a lane reads its own store; the barriers are behind the load and in front of the store-back.
//     Outputs go straight to global memory: a visit's record by all lanes (one store after coalescing), the candidates
//     no visit took by a ballot's prefix count.  No atomics; the result is a function of the inputs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_h2sched.h"
#include "hhuff_slots.h"

#define HHUFF_API extern "C" __attribute__((visibility("default")))

namespace hhuff {
namespace {
using namespace h2q;
constexpr uint32_t kWave = 64;

template <int X>
__device__ __forceinline__ uint32_t swz(uint32_t v) {  // lane l's value of lane l ^ X, X < 32
    return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (X << 10) | 0x1f);
}
template <int X>
__device__ __forceinline__ uint64_t swz64(uint64_t v) {
    return (uint64_t)swz<X>((uint32_t)(v >> 32)) << 32 | swz<X>((uint32_t)v);
}
__device__ __forceinline__ uint64_t min64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t lane64(uint64_t v, int l) {
    return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32 | (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}
__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
    v = min64(v, swz64<1>(v)), v = min64(v, swz64<2>(v)), v = min64(v, swz64<4>(v)), v = min64(v, swz64<8>(v)), v = min64(v, swz64<16>(v));
    return min64(lane64(v, 0), lane64(v, 32));
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    v += swz<1>(v), v += swz<2>(v), v += swz<4>(v), v += swz<8>(v), v += swz<16>(v);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 32);
}
__device__ __forceinline__ uint32_t below(uint64_t m, uint32_t lane) { return (uint32_t)__popcll(m & ((1ull << lane) - 1u)); }

constexpr uint64_t kNoKey = ~0ull;
constexpr uint32_t kIdxBits = 12, kSeqShift = kIdxBits, kDistShift = kIdxBits + 32;
static_assert(kMaxNodes <= 1u << kIdxBits, "an index fits the key");

struct Wave {  // the steps over the table (hhuff_h2sched.h)
    uint32_t lane;
    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

    __device__ void find(const Node* n, uint32_t nhigh, uint32_t id, uint32_t pid, uint32_t& idx, uint32_t& pidx, uint32_t& free_) const {
        idx = pidx = free_ = kNone;
        for (uint32_t b = 0; b < nhigh; b += kWave) {
            const uint32_t i = b + lane;
            const bool in = i < nhigh;
            const uint32_t v = in ? n[i].id : 0u;
            const uint64_t mi = __ballot(in && v == id), mp = __ballot(in && v == pid && pid != 0), mf = __ballot(in && v == 0);
            if (mi && idx == kNone) idx = b + (uint32_t)__builtin_ctzll(mi);
            if (mp && pidx == kNone) pidx = b + (uint32_t)__builtin_ctzll(mp);
            if (mf && free_ == kNone) free_ = b + (uint32_t)__builtin_ctzll(mf);
        }
    }
    __device__ uint32_t first_child(const Node* n, uint32_t nhigh, uint32_t p, uint32_t skip) const {
        uint64_t best = kNoKey;
        for (uint32_t i = lane; i < nhigh; i += kWave)
            if (n[i].id != 0 && n[i].parent == p && i != skip) best = min64(best, (uint64_t)n[i].aseq << kSeqShift | i);
        const uint64_t k = wave_min(best);
        return k == kNoKey ? kNone : (uint32_t)k & ((1u << kIdxBits) - 1u);
    }
    __device__ uint32_t weight_sum(const Node* n, uint32_t nhigh, uint32_t p) const {
        uint32_t sum = 0;
        for (uint32_t i = lane; i < nhigh; i += kWave)
            if (n[i].id != 0 && n[i].parent == p) sum += n[i].weight;
        return wave_sum(sum);
    }
    __device__ Popped pop(const Node* n, uint32_t nhigh, uint32_t p, uint32_t qoff) const {
        uint64_t best = kNoKey, second = kNoKey;
        for (uint32_t i = lane; i < nhigh; i += kWave) {
            const uint32_t slot = n[i].slot;
            if (n[i].id == 0 || n[i].parent != p || slot == kUnqueued) continue;
            const uint64_t dist = slot == kSlot257 ? 0u : 1u + ((slot - qoff) & (kSlots - 1u));
            const uint64_t key = dist << kDistShift | (uint64_t)n[i].qseq << kSeqShift | i;
            if (key < best) second = best, best = key;
            else second = min64(second, key);
        }
        const uint64_t k = wave_min(best);
        if (k == kNoKey) return Popped{kNone, 0, false};
        const uint64_t d = k >> kDistShift;
        const uint64_t other = best == k ? second : best;
        return Popped{(uint32_t)k & ((1u << kIdxBits) - 1u), (uint32_t)d, __ballot(other != kNoKey && other >> kDistShift == d) != 0};
    }
    __device__ bool any257(const Node* n, uint32_t nhigh, uint32_t p) const {
        bool any = false;
        for (uint32_t i = lane; i < nhigh; i += kWave) any |= n[i].id != 0 && n[i].parent == p && n[i].slot == kSlot257;
        return __ballot(any) != 0;
    }
    __device__ void append_unvisited(Visits& V) const {
        for (uint32_t b = V.lo; b < V.hi; b += kWave) {
            const uint32_t j = b + lane;  // (hi <= nsend < 2^32 and b < hi: j wraps for no lane below hi)
            const bool un = j >= b && j < V.hi && V.pos[j] == kNone;
            const uint64_t m = __ballot(un);
            if (un) {
                const uint32_t k = V.n + below(m, lane);
                hhuff_h2_send_t S = V.sends[j];
                S.window = 0;
                V.ordered[V.lo + k] = S, V.order[V.lo + k] = j, V.pos[j] = k;
            }
            V.n += (uint32_t)__popcll(m);
            if (V.hi - b <= kWave) break;
        }
    }
};

struct SchedArgs {
    uint8_t* scratch;
    uint64_t slab, out_size;
    uint32_t max_nodes, nconn, nops, nsend;
    const hhuff_h2_sched_op_t* ops;
    const uint32_t* op_first;
    const hhuff_h2_send_t* sends;
    const uint32_t* send_first;
    const hhuff_h2_peer_t* peers;
    const uint32_t* out_off;
    int32_t* op_status;
    hhuff_h2_send_t* ordered;
    uint32_t* order;
    uint32_t* pos;
    uint32_t* nvisit;
    int32_t* cstatus;
    uint8_t* active;
    unsigned flags;
    const uint32_t* cmap;
};

template <bool SLOTS>
__global__ __launch_bounds__(kWave) void h2_schedule_kernel(SchedArgs A) {
    // (the table is copied as dwords and used as Nodes: the dword type may alias them)
    typedef uint32_t __attribute__((may_alias)) word_t;
    extern __shared__ word_t lds[];
    const uint32_t c = blockIdx.x, lane = threadIdx.x, mn = A.max_nodes;
    Node* const n = reinterpret_cast<Node*>(lds);
    uint32_t* const cand = reinterpret_cast<uint32_t*>(lds + mn * (kNodeBytes / 4u));
    Wave w{lane};
    // whatever the offset arrays hold, the ops stay inside [0, nops), the records inside [0, nsend)
    lc::Range op{0, 0};
    if (A.nops != 0) op = lc::clamp_range(A.op_first[c], A.op_first[c + 1u], A.nops);
    const lc::Range sr = lc::clamp_range(A.send_first[c], A.send_first[c + 1u], A.nsend);
    const lc::Range rr = lc::clamp_range(A.out_off[c], A.out_off[c + 1u], (uint32_t)A.out_size);
    Visits V{A.sends, sr.first, sr.first + sr.count, A.ordered, A.order, A.pos, 0};
    const ConnSlot cs = conn_slot<SLOTS>(A.cmap, c);
    int32_t status = cs.refused ? HHUFF_H2SC_ESLOT : 0;
    uint8_t* const slab = A.scratch + (cs.refused ? 0u : cs.slot * A.slab);
    word_t* const nodes = reinterpret_cast<word_t*>(slab + kHeaderBytes);
    Header h = fresh_header(mn);
    if (!cs.refused && (A.flags & HHUFF_H2SC_CONTINUE) != 0 && !cs.reset) {
        const uint32_t* hw = reinterpret_cast<const uint32_t*>(slab);
        h = Header{hw[0], hw[1], hw[2], hw[3], (uint64_t)hw[5] << 32 | hw[4], hw[6], hw[7]};
        bool ok = header_ok(h, mn);
        const uint32_t nh = ok ? h.nhigh : 0u;
        for (uint32_t i = lane; i < nh * (kNodeBytes / 4u); i += kWave) lds[i] = nodes[i];
        __syncthreads();
        bool bad = false;
        for (uint32_t i = lane; i < nh; i += kWave) bad |= !node_ok(n[i], nh);
        ok = ok && __ballot(bad) == 0;
        if (!ok) status = HHUFF_H2SC_EFORMAT;
    }
    for (uint32_t i = lane; i < mn; i += kWave) cand[i] = 0;
    __syncthreads();
    if (status != 0) {  // no slab: every op says why, the records pass unvisited
        for (uint32_t o = lane; o < op.count; o += kWave) A.op_status[op.first + o] = status;
        for (uint32_t j = V.lo; j < V.hi; ++j) V.pos[j] = kNone;
        w.append_unvisited(V);
        if (lane == 0) A.nvisit[c] = 0, A.cstatus[c] = status, A.active[c] = 0;
        return;
    }
    Sched<Wave> S{w, n, cand, h, mn};
    for (uint32_t o = 0; o < op.count; ++o) {
        const uint32_t* ow = reinterpret_cast<const uint32_t*>(A.ops + op.first + o);
        const uint32_t w3 = w.uni(ow[3]);
        const hhuff_h2_sched_op_t O{w.uni(ow[0]), w.uni(ow[1]), w.uni(ow[2]), (uint16_t)w3, (uint8_t)(w3 >> 16), (uint8_t)(w3 >> 24)};
        const int32_t st = S.apply(O);
        if (lane == 0) A.op_status[op.first + o] = st;
    }
    const hhuff_h2_peer_t P = A.peers[c];
    // (a peer out of range: the candidates are listed, the entry window is 0 and no visit is made)
    const bool peer = h2d::peer_ok(P);
    if (!peer) status = HHUFF_H2SC_EINVAL;
    const uint32_t nvisit = S.run(V, (int64_t)P.max_frame_size, peer ? (int64_t)rr.count : 0, P.send_window);
    const bool act = S.is_active();
    __syncthreads();
    for (uint32_t i = lane; i < S.h.nhigh * (kNodeBytes / 4u); i += kWave) nodes[i] = lds[i];
    if (lane == 0) {
        uint32_t* hw = reinterpret_cast<uint32_t*>(slab);
        hw[0] = S.h.magic, hw[1] = S.h.max_nodes, hw[2] = S.h.seq, hw[3] = S.h.nhigh, hw[4] = (uint32_t)S.h.root_bits;
        hw[5] = (uint32_t)(S.h.root_bits >> 32), hw[6] = S.h.root_qoff, hw[7] = S.h.count;
        A.nvisit[c] = nvisit, A.cstatus[c] = status, A.active[c] = act ? 1 : 0;
    }
}
}  // namespace
}  // namespace hhuff

HHUFF_API uint64_t hhuff_h2_sched_scratch_size(uint32_t nslots, uint32_t max_nodes) {
    if (max_nodes == 0 || max_nodes > hhuff::h2q::kMaxNodes) return 0;
    return (uint64_t)nslots * hhuff::h2q::slab_bytes(max_nodes);
}

HHUFF_API int hhuff_h2_schedule(const hhuff_conn_slots_t* slots, uint32_t max_nodes, const hhuff_h2_sched_op_t* ops,
                                const uint32_t* op_first, uint32_t nops, const hhuff_h2_send_t* sends, const uint32_t* send_first,
                                uint32_t nsend, uint32_t nconn, const hhuff_h2_peer_t* peers, uint64_t out_size, const uint32_t* out_off,
                                int32_t* op_status, hhuff_h2_send_t* ordered, uint32_t* order, uint32_t* pos, uint32_t* nvisit,
                                int32_t* cstatus, uint8_t* active, void* scratch, uint64_t scratch_size, unsigned flags, void* stream) {
    using namespace hhuff;
    if (!sends || !send_first || !peers || !out_off || !ordered || !order || !pos || !nvisit || !cstatus || !active) return HHUFF_EINVAL;
    if (nops != 0 && (!ops || !op_first || !op_status)) return HHUFF_EINVAL;
    if ((out_size >> 32) || (flags & ~HHUFF_H2SC_CONTINUE) || max_nodes == 0 || max_nodes > h2q::kMaxNodes) return HHUFF_EINVAL;
    const uint64_t slab = h2q::slab_bytes(max_nodes);
    if (conn_slots_check(slots, nconn, scratch_size, slab) != nullptr) return HHUFF_EINVAL;
    if (!scratch || ((uintptr_t)scratch & 15u) != 0 || (!slots && scratch_size / slab < nconn)) return HHUFF_EINVAL;
    if (nconn == 0) return HHUFF_OK;
    SchedArgs A{(uint8_t*)scratch, slab, out_size, max_nodes, nconn, nops, nsend, ops, op_first, sends, send_first, peers, out_off,
                op_status, ordered, order, pos, nvisit, cstatus, active, flags, nullptr};
    uint32_t* cmap = nullptr;
    if (conn_map_make(slots, nconn, (hipStream_t)stream, &cmap) != hipSuccess) return HHUFF_EHIP;
    A.cmap = cmap;
    const uint32_t lds = max_nodes * (h2q::kNodeBytes + 4u);
    if (cmap)
        hipLaunchKernelGGL(h2_schedule_kernel<true>, dim3(nconn), dim3(kWave), lds, (hipStream_t)stream, A);
    else
        hipLaunchKernelGGL(h2_schedule_kernel<false>, dim3(nconn), dim3(kWave), lds, (hipStream_t)stream, A);
    const hipError_t e = hipGetLastError();
    if (cmap) (void)hipFreeAsync(cmap, (hipStream_t)stream);
    return e == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}
