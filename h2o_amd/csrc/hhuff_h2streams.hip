// HTTP/2 stream table (include/hhuff.h (2k'''); the rules live in hhuff_h2streams.h, shared with the host).
//   h2s_walk_kernel    one lane per connection applies its ops and walks its frame records in wire order (h2s::walk)
//                      against its own slab: the connection's counters in registers, one 48-byte entry in and out per
//                      frame, one 16-byte event out, the merged replies into the connection's own region.  A
//                      connection's frames are a dependent chain -- a HEADERS opens what the next DATA needs -- and the
//                      slabs and regions are the connections' own, so there is no scan, no workspace and no atomic.
//                      The lanes of a wave touch unrelated slabs: every access is a lane's own line, which is what one
//                      lane a connection costs; a wave a workgroup spreads the connections over the CUs.
//   h2s_fill_kernel    hhuff_h2_streams_fill_sends and _commit_sent: one lane per connection, its send records in order
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_h2streams.h"
#include "hhuff_slots.h"

#define HHUFF_API extern "C" __attribute__((visibility("default")))

namespace hhuff {
namespace {

constexpr uint32_t kStrThreads = 64;

struct StrArgs {
    const uint8_t* in;
    uint64_t in_size;
    const hhuff_h2_frame_t* frames;
    const uint32_t* nframes;
    const uint32_t* frm_first;
    uint32_t frm_cap, nconn;
    const hhuff_h2_ctl_t* ctl;
    const uint32_t* nctl;
    const uint8_t* ctl_rep;
    uint64_t ctl_rep_size;
    const uint32_t* ctl_rep_off;
    const hhuff_h2_block_t* blocks;
    const uint32_t* conn_first;
    const int32_t* bstatus;
    const hhuff_request_t* req;
    const uint8_t* arena;
    uint64_t arena_size;
    const uint32_t* blk_off;
    const uint32_t* value_off;
    const uint32_t* value_len;
    const hhuff_h2_peer_t* peers;
    const hhuff_h2_stream_op_t* ops;
    const uint32_t* op_first;
    uint32_t nops;
    hhuff_h2_sev_t* sev;
    hhuff_h2_sev_t* op_sev;
    uint32_t* nstr;
    int32_t* sstatus;
    uint32_t* serr;
    uint8_t* rep;
    uint64_t rep_size;
    const uint32_t* rep_off;
    uint32_t* rep_len;
    uint8_t* scratch;
    uint64_t slab;
    h2s::Cfg P;
    unsigned flags;
    const uint32_t* cmap;
};

// [a, b) of an offsets array, inside [0, size)
struct Range {
    uint64_t lo, hi;
    __device__ Range(uint64_t a, uint64_t b, uint64_t size) {
        lo = a < size ? a : size;
        hi = b < lo ? lo : (b < size ? b : size);
    }
};

template <bool SLOTS>
__global__ __launch_bounds__(kStrThreads) void h2s_walk_kernel(StrArgs A) {
    const uint64_t c64 = (uint64_t)blockIdx.x * kStrThreads + threadIdx.x;
    if (c64 >= A.nconn) return;
    const uint32_t c = (uint32_t)c64;
    const ConnSlot cs = conn_slot<SLOTS>(A.cmap, c);
    if (cs.refused) {  // no slab: nothing of it is touched
        A.nstr[c] = 0, A.sstatus[c] = HHUFF_H2ST_ESLOT, A.serr[c] = HHUFF_H2ST_ERR_NONE, A.rep_len[c] = 0;
        return;
    }
    // whatever the offset arrays hold, the slots stay inside [0, frm_cap), the blocks too, the ops inside [0, nops) and
    // the bytes inside their arrays
    const Range fr(A.frm_first[c], A.frm_first[c + 1], A.frm_cap);
    const uint32_t slots = (uint32_t)(fr.hi - fr.lo);
    uint32_t n = A.nframes[c] < slots ? A.nframes[c] : slots;
    n = A.nctl[c] < n ? A.nctl[c] : n;
    const Range bl(A.conn_first[c], A.conn_first[c + 1], A.frm_cap);
    const Range cr(A.ctl_rep_off[c], A.ctl_rep_off[c + 1], A.ctl_rep_size);
    const Range rr(A.rep_off[c], A.rep_off[c + 1], A.rep_size);
    Range op(0, 0, 0);
    if (A.nops != 0) op = Range(A.op_first[c], A.op_first[c + 1], A.nops);
    h2s::Conn C;
    C.in = A.in, C.in_size = A.in_size, C.frames = A.frames, C.ctl = A.ctl, C.f0 = (uint32_t)fr.lo, C.n = n;
    C.ctl_rep = A.ctl_rep + cr.lo, C.ctl_rep_len = (uint32_t)(cr.hi - cr.lo);
    C.blocks = A.blocks, C.bstatus = A.bstatus, C.req = A.req, C.b0 = (uint32_t)bl.lo, C.b1 = (uint32_t)bl.hi;
    C.arena = A.arena, C.arena_size = A.arena_size, C.blk_off = A.blk_off, C.value_off = A.value_off, C.value_len = A.value_len;
    C.initial_window_size = A.peers[c].initial_window_size;
    C.ops = A.ops + op.lo, C.nops = (uint32_t)(op.hi - op.lo);
    C.sev = A.sev, C.op_sev = A.op_sev + op.lo;
    C.rep = A.rep + rr.lo, C.rep_cap = (uint32_t)(rr.hi - rr.lo);
    const h2s::Table T = h2s::table_at(A.scratch + cs.slot * A.slab, A.P.max_entries);
    const bool fresh = (A.flags & HHUFF_H2ST_CONTINUE) == 0 || cs.reset;
    h2s::Result R;
    h2s::walk(C, A.P, T, fresh, R);
    A.nstr[c] = R.nstr, A.sstatus[c] = R.status, A.serr[c] = R.err, A.rep_len[c] = R.rep_len;
}

struct FillArgs {
    uint8_t* scratch;
    uint64_t slab;
    uint32_t max_entries, nconn, nsend;
    hhuff_h2_send_t* sends;
    const hhuff_h2_sent_t* sent;  // NULL: fill; else commit
    const uint32_t* send_first;
    uint8_t* miss;
    const uint32_t* cmap;
};

template <bool SLOTS>
__global__ __launch_bounds__(kStrThreads) void h2s_fill_kernel(FillArgs A) {
    const uint64_t c64 = (uint64_t)blockIdx.x * kStrThreads + threadIdx.x;
    if (c64 >= A.nconn) return;
    const uint32_t c = (uint32_t)c64;
    const Range sr(A.send_first[c], A.send_first[c + 1], A.nsend);
    const uint32_t n = (uint32_t)(sr.hi - sr.lo);
    const ConnSlot cs = conn_slot<SLOTS>(A.cmap, c);
    if (cs.refused) {  // no slab: every record is a miss
        if (A.sent == nullptr)
            for (uint32_t r = 0; r < n; ++r) A.sends[sr.lo + r].window = 0, A.miss[sr.lo + r] = 1;
        return;
    }
    const h2s::Table T = h2s::table_at(A.scratch + cs.slot * A.slab, A.max_entries);
    if (A.sent == nullptr)
        h2s::fill_sends(T, A.sends + sr.lo, n, A.miss + sr.lo);
    else
        h2s::commit_sent(T, A.sends + sr.lo, A.sent + sr.lo, n);
}

// the checks the three calls make of their slabs: 0, or HHUFF_EINVAL
int check_slabs(const hhuff_conn_slots_t* slots, uint32_t max_entries, uint32_t nconn, const void* scratch, uint64_t scratch_size) {
    if (max_entries == 0 || max_entries > h2s::kMaxEntries) return HHUFF_EINVAL;
    const uint64_t slab = h2s::slab_size(max_entries);
    if (conn_slots_check(slots, nconn, scratch_size, slab) != nullptr) return HHUFF_EINVAL;
    if (!scratch || ((uintptr_t)scratch & 15u) != 0) return HHUFF_EINVAL;
    if (!slots && scratch_size / slab < nconn) return HHUFF_EINVAL;
    return HHUFF_OK;
}

int launch_fill(const hhuff_conn_slots_t* slots, FillArgs& A, hipStream_t stream) {
    uint32_t* cmap = nullptr;
    if (conn_map_make(slots, A.nconn, stream, &cmap) != hipSuccess) return HHUFF_EHIP;
    A.cmap = cmap;
    const uint32_t grid = (uint32_t)(((uint64_t)A.nconn + kStrThreads - 1u) / kStrThreads);
    if (cmap)
        hipLaunchKernelGGL(h2s_fill_kernel<true>, dim3(grid), dim3(kStrThreads), 0, stream, A);
    else
        hipLaunchKernelGGL(h2s_fill_kernel<false>, dim3(grid), dim3(kStrThreads), 0, stream, A);
    const hipError_t e = hipGetLastError();
    if (cmap) (void)hipFreeAsync(cmap, stream);
    return e == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}

}  // namespace
}  // namespace hhuff

HHUFF_API uint64_t hhuff_h2_streams_scratch_size(uint32_t nslots, uint32_t max_entries) {
    if (max_entries == 0 || max_entries > hhuff::h2s::kMaxEntries) return 0;
    return (uint64_t)nslots * hhuff::h2s::slab_size(max_entries);
}

HHUFF_API int hhuff_h2_streams(const hhuff_conn_slots_t* slots, const hhuff_h2_streams_params_t* params, const uint8_t* in,
                               uint64_t in_size, const hhuff_h2_frame_t* frames, const uint32_t* nframes, const uint32_t* frm_first,
                               uint32_t frm_cap, const hhuff_h2_ctl_t* ctl, const uint32_t* nctl, const uint8_t* ctl_rep,
                               uint64_t ctl_rep_size, const uint32_t* ctl_rep_off, const hhuff_h2_block_t* blocks,
                               const uint32_t* conn_first, const int32_t* bstatus, const hhuff_request_t* req, const uint8_t* arena,
                               uint64_t arena_size, const uint32_t* blk_off, const uint32_t* value_off, const uint32_t* value_len,
                               const hhuff_h2_peer_t* peers, const hhuff_h2_stream_op_t* ops, const uint32_t* op_first, uint32_t nops,
                               uint32_t nconn, hhuff_h2_sev_t* sev, hhuff_h2_sev_t* op_sev, uint32_t* nstr, int32_t* sstatus,
                               uint32_t* serr, uint8_t* rep, uint64_t rep_size, const uint32_t* rep_off, uint32_t* rep_len,
                               void* scratch, uint64_t scratch_size, unsigned flags, void* stream) {
    using namespace hhuff;
    if (!params || !in || !frames || !nframes || !frm_first || !ctl || !nctl || !ctl_rep || !ctl_rep_off || !blocks || !conn_first ||
        !bstatus || !req || !arena || !blk_off || !value_off || !value_len || !peers || !sev || !nstr || !sstatus || !serr || !rep ||
        !rep_off || !rep_len)
        return HHUFF_EINVAL;
    if (nops != 0 && (!ops || !op_first || !op_sev)) return HHUFF_EINVAL;
    if ((in_size >> 32) || (arena_size >> 32) || (ctl_rep_size >> 32) || (rep_size >> 32)) return HHUFF_EINVAL;
    if ((flags & ~HHUFF_H2ST_CONTINUE) || (params->flags & ~HHUFF_H2SP_STREAM_BODIES) || params->rsv != 0) return HHUFF_EINVAL;
    if (params->active_stream_window_size < h2s::kHostStreamWindow || params->active_stream_window_size > 0x7fffffffu)
        return HHUFF_EINVAL;
    if (const int bad = check_slabs(slots, params->max_entries, nconn, scratch, scratch_size)) return bad;
    if (nconn == 0) return HHUFF_OK;
    StrArgs A{};
    A.in = in, A.in_size = in_size, A.frames = frames, A.nframes = nframes, A.frm_first = frm_first, A.frm_cap = frm_cap, A.nconn = nconn;
    A.ctl = ctl, A.nctl = nctl, A.ctl_rep = ctl_rep, A.ctl_rep_size = ctl_rep_size, A.ctl_rep_off = ctl_rep_off;
    A.blocks = blocks, A.conn_first = conn_first, A.bstatus = bstatus, A.req = req, A.arena = arena, A.arena_size = arena_size;
    A.blk_off = blk_off, A.value_off = value_off, A.value_len = value_len, A.peers = peers;
    A.ops = ops, A.op_first = op_first, A.nops = nops, A.sev = sev, A.op_sev = op_sev;
    A.nstr = nstr, A.sstatus = sstatus, A.serr = serr, A.rep = rep, A.rep_size = rep_size, A.rep_off = rep_off, A.rep_len = rep_len;
    A.scratch = (uint8_t*)scratch, A.slab = h2s::slab_size(params->max_entries);
    A.P = h2s::Cfg{params->max_streams, params->max_streams_for_priority, params->active_stream_window_size - h2s::kHostStreamWindow,
                   params->flags, params->max_entries, params->max_request_entity_size};
    A.flags = flags;
    uint32_t* cmap = nullptr;
    if (conn_map_make(slots, nconn, (hipStream_t)stream, &cmap) != hipSuccess) return HHUFF_EHIP;
    A.cmap = cmap;
    const uint32_t grid = (uint32_t)(((uint64_t)nconn + kStrThreads - 1u) / kStrThreads);
    if (cmap)
        hipLaunchKernelGGL(h2s_walk_kernel<true>, dim3(grid), dim3(kStrThreads), 0, (hipStream_t)stream, A);
    else
        hipLaunchKernelGGL(h2s_walk_kernel<false>, dim3(grid), dim3(kStrThreads), 0, (hipStream_t)stream, A);
    const hipError_t e = hipGetLastError();
    if (cmap) (void)hipFreeAsync(cmap, (hipStream_t)stream);
    return e == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}

HHUFF_API int hhuff_h2_streams_fill_sends(const hhuff_conn_slots_t* slots, uint32_t max_entries, void* scratch, uint64_t scratch_size,
                                          hhuff_h2_send_t* sends, const uint32_t* send_first, uint32_t nsend, uint32_t nconn,
                                          uint8_t* miss, void* stream) {
    using namespace hhuff;
    if (!sends || !send_first || !miss) return HHUFF_EINVAL;
    if (const int bad = check_slabs(slots, max_entries, nconn, scratch, scratch_size)) return bad;
    if (nconn == 0) return HHUFF_OK;
    FillArgs A{(uint8_t*)scratch, h2s::slab_size(max_entries), max_entries, nconn, nsend, sends, nullptr, send_first, miss, nullptr};
    return launch_fill(slots, A, (hipStream_t)stream);
}

HHUFF_API int hhuff_h2_streams_commit_sent(const hhuff_conn_slots_t* slots, uint32_t max_entries, void* scratch, uint64_t scratch_size,
                                           const hhuff_h2_send_t* sends, const hhuff_h2_sent_t* sent, const uint32_t* send_first,
                                           uint32_t nsend, uint32_t nconn, void* stream) {
    using namespace hhuff;
    if (!sends || !sent || !send_first) return HHUFF_EINVAL;
    if (const int bad = check_slabs(slots, max_entries, nconn, scratch, scratch_size)) return bad;
    if (nconn == 0) return HHUFF_OK;
    FillArgs A{(uint8_t*)scratch, h2s::slab_size(max_entries), max_entries, nconn, nsend, const_cast<hhuff_h2_send_t*>(sends), sent,
               send_first, nullptr, nullptr};
    return launch_fill(slots, A, (hipStream_t)stream);
}
