// HTTP/2 de-framer (include/hhuff.h (2k); the rules live in hhuff_frames.h, shared with the host).
//   frm_walk_kernel<false>  one lane per connection follows the dependent chain of 9-byte headers (frm::walk with
//                           a sink that keeps nothing): nframes, consumed, cstatus, cerr, the connection's block
//                           and block-byte counts to the workspace, and their sums over the workgroup's 256
//                           connections
//   frm_scan_kernel         one workgroup: the workgroups' sums -> the sums of the workgroups before each (a lane
//                           sums a run of consecutive entries, the runs' sums are scanned in LDS, the lane walks its
//                           run again; 65,536 connections are 256 entries, one a lane), conn_first[nconn], totals
//   frm_walk_kernel<true>   the same walk with the bases known -- the workgroup's base plus a scan of its 256
//                           counts in LDS --: conn_first, frame and block records and blk_off at their final
//                           places, and per frame slot one gather job (source, destination, length; the workspace
//                           is zeroed first, so a slot without fragment is a job of length 0)
//   frm_finish_kernel       blk_off past nblk, arena_off
//   frm_gather_kernel       the copy, parallel over fragments (hhuff_gather.h, shared with the HTTP/3 de-framer)
// Positions come from the scan alone: no atomics, equal input gives equal bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_frames.h"
#include "hhuff_gather.h"
#include "hhuff_launch.h"

#define HHUFF_API extern "C" __attribute__((visibility("default")))

namespace hhuff {
namespace {

struct FrmArgs {
    const uint8_t* in;
    uint64_t in_size;
    const uint32_t* in_off;
    uint32_t nconn;
    const uint32_t* frm_first;
    uint32_t frm_cap;
    uint32_t max_frame_size, max_block_bytes, flags;
    hhuff_h2_frame_t* frames;
    uint32_t* nframes;
    uint32_t* consumed;
    int32_t* cstatus;
    uint32_t* cerr;
    uint8_t* blk;
    uint32_t* blk_off;
    uint32_t* conn_first;
    hhuff_h2_block_t* blocks;
    uint32_t* totals;
    uint64_t* arena_off;
    uint64_t arena_fixed;
    uint32_t arena_per_byte;
    // workspace
    uint2* count;  // [nconn]: blocks, block bytes
    uint2* part;   // [walk workgroups]: their sums of count, then the sums of the workgroups before
    uint4* job;    // [frm_cap]: source offset in `in`, destination offset in blk, length, 0
};

struct PlaceSink {
    const FrmArgs& A;
    uint32_t start, f0, block0, byte0;
    __device__ void frame(uint32_t i, const hhuff_h2_frame_t& rel, uint32_t dst) {
        hhuff_h2_frame_t f = rel;
        f.payload_off += start;
        if (f.block != frm::kNoBlock) {
            f.frag_off += start, f.block += block0;
            const uint64_t d = (uint64_t)byte0 + dst;
            if (f.frag_len != 0 && d + f.frag_len <= A.in_size) A.job[f0 + i] = make_uint4(f.frag_off, (uint32_t)d, f.frag_len, 0u);
        }
        A.frames[f0 + i] = f;
    }
    __device__ void block(uint32_t b, const hhuff_h2_block_t& rel, uint32_t off) {
        const uint64_t g = (uint64_t)block0 + b;
        if (g >= A.frm_cap) return;  // (only with a frm_first that is no running sum)
        hhuff_h2_block_t r = rel;
        r.first_frame += f0;
        A.blocks[g] = r;
        A.blk_off[g] = byte0 + off;
    }
};

template <bool PLACE>
__global__ __launch_bounds__(kWalkThreads) void frm_walk_kernel(FrmArgs A) {
    const uint64_t c64 = (uint64_t)blockIdx.x * kWalkThreads + threadIdx.x;
    const bool act = c64 < A.nconn;  // (every lane stays for the workgroup's sums)
    const uint32_t c = (uint32_t)c64;
    frm::Result res{};
    if (PLACE) {
        const uint2 mine = act ? A.count[c] : make_uint2(0u, 0u);
        uint2 before, all;
        wg_scan(mine, before, all);
        if (!act) return;
        const uint2 wg = A.part[blockIdx.x];
        const SlotRange R(A.in_off, A.frm_first, c, A.in_size, A.frm_cap);
        const frm::Params P{A.max_frame_size, A.max_block_bytes, A.flags, R.cap};
        A.conn_first[c] = wg.x + before.x;
        PlaceSink sink{A, R.start, R.f0, wg.x + before.x, wg.y + before.y};
        frm::walk(A.in + R.start, R.len, P, sink, res);
    } else {
        if (act) {
            const SlotRange R(A.in_off, A.frm_first, c, A.in_size, A.frm_cap);
            const frm::Params P{A.max_frame_size, A.max_block_bytes, A.flags, R.cap};
            frm::NoSink sink;
            frm::walk(A.in + R.start, R.len, P, sink, res);
            A.nframes[c] = res.nframes, A.consumed[c] = res.consumed, A.cstatus[c] = res.status, A.cerr[c] = res.err;
            A.count[c] = make_uint2(res.nblocks, res.block_bytes);
        }
        uint2 before, all;
        wg_scan(make_uint2(res.nblocks, res.block_bytes), before, all);
        if (threadIdx.x == 0) A.part[blockIdx.x] = all;
    }
}

// part[w] (the sums of walk workgroup w) -> the sums of the workgroups before w, in place; conn_first[nconn], totals.
__global__ __launch_bounds__(kScanThreads) void frm_scan_kernel(FrmArgs A, uint32_t nparts) {
    const uint2 t = scan_parts(A.part, nparts);
    if (threadIdx.x == kScanThreads - 1u) A.conn_first[A.nconn] = t.x, A.totals[0] = t.x, A.totals[1] = t.y;
}

__global__ __launch_bounds__(256) void frm_finish_kernel(FrmArgs A) {
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b > A.frm_cap) return;
    const uint32_t nblk = A.totals[0] < A.frm_cap ? A.totals[0] : A.frm_cap;
    uint32_t off;
    if (b >= nblk)
        A.blk_off[b] = off = A.totals[1];
    else
        off = A.blk_off[b];
    if (A.arena_off) A.arena_off[b] = A.arena_fixed * (b < nblk ? b : nblk) + (uint64_t)A.arena_per_byte * off;
}

hipError_t launch_deframe(FrmArgs& A, hipStream_t stream) {
    const uint32_t wgrid = (uint32_t)(((uint64_t)A.nconn + kWalkThreads - 1u) / kWalkThreads);
    const uint64_t conn_bytes = ((uint64_t)A.nconn * 8u + 15u) & ~15ull;
    const uint64_t job_bytes = (uint64_t)A.frm_cap * 16u;
    uint8_t* ws = nullptr;
    hipError_t e = work_alloc((void**)&ws, job_bytes + conn_bytes + (uint64_t)wgrid * 8u + 16u, stream);
    if (e != hipSuccess) return e;
    A.job = reinterpret_cast<uint4*>(ws);
    A.count = reinterpret_cast<uint2*>(ws + job_bytes);
    A.part = reinterpret_cast<uint2*>(ws + job_bytes + conn_bytes);
    if (job_bytes) e = hipMemsetAsync(A.job, 0, job_bytes, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(frm_walk_kernel<false>, dim3(wgrid), dim3(kWalkThreads), 0, stream, A);
        hipLaunchKernelGGL(frm_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, A, wgrid);
        hipLaunchKernelGGL(frm_walk_kernel<true>, dim3(wgrid), dim3(kWalkThreads), 0, stream, A);
        hipLaunchKernelGGL(frm_finish_kernel, dim3((uint32_t)(((uint64_t)A.frm_cap + 1u + 255u) / 256u)), dim3(256), 0, stream, A);
        if (A.frm_cap)
            hipLaunchKernelGGL(frm_gather_kernel, dim3((uint32_t)(((uint64_t)A.frm_cap + kGatherThreads - 1u) / kGatherThreads)),
                               dim3(kGatherThreads), 0, stream, A.in, A.blk, A.job, A.frm_cap);
        e = hipGetLastError();
    }
    const hipError_t f = hipFreeAsync(ws, stream);
    return e != hipSuccess ? e : f;
}

}  // namespace
}  // namespace hhuff

HHUFF_API int hhuff_h2_deframe(const uint8_t* in, uint64_t in_size, const uint32_t* in_off, uint32_t nconn,
                               const uint32_t* frm_first, uint32_t frm_cap, uint32_t max_frame_size, uint32_t max_block_bytes,
                               unsigned flags, hhuff_h2_frame_t* frames, uint32_t* nframes, uint32_t* consumed, int32_t* cstatus,
                               uint32_t* cerr, uint8_t* blk, uint32_t* blk_off, uint32_t* conn_first, hhuff_h2_block_t* blocks,
                               uint32_t* totals, uint64_t* arena_off, uint64_t arena_fixed, uint32_t arena_per_byte, void* stream) {
    if (!in || !in_off || !frm_first || !frames || !nframes || !consumed || !cstatus || !cerr || !blk || !blk_off || !conn_first ||
        !blocks || !totals)
        return HHUFF_EINVAL;
    if (in_size >> 32) return HHUFF_EINVAL;
    if (max_frame_size < 16384u || max_frame_size > 0xFFFFFFu) return HHUFF_EINVAL;
    if (flags & ~HHUFF_H2F_ACCEPT_PUSH) return HHUFF_EINVAL;
    if (nconn == 0) return HHUFF_OK;
    hhuff::FrmArgs A{};
    A.in = in, A.in_size = in_size, A.in_off = in_off, A.nconn = nconn, A.frm_first = frm_first, A.frm_cap = frm_cap;
    A.max_frame_size = max_frame_size, A.max_block_bytes = max_block_bytes, A.flags = flags;
    A.frames = frames, A.nframes = nframes, A.consumed = consumed, A.cstatus = cstatus, A.cerr = cerr;
    A.blk = blk, A.blk_off = blk_off, A.conn_first = conn_first, A.blocks = blocks, A.totals = totals;
    A.arena_off = arena_off, A.arena_fixed = arena_fixed, A.arena_per_byte = arena_per_byte;
    return hhuff::launch_deframe(A, (hipStream_t)stream) == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}
