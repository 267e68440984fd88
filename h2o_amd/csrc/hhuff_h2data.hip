// HTTP/2 DATA frames on the send side (include/hhuff.h (2k''); the arithmetic lives in hhuff_h2data.h, shared with
// the host).
//   h2d_walk_kernel<false>  one lane per connection serves its send records in order (h2d::walk, a closed form per
//                           record: no loop over frames): the connection's count of records with frames (copy jobs) and
//                           of the 16-byte destination lines they cover, and the sums over the workgroup's 256
//   h2d_scan_kernel         one workgroup: the workgroups' sums -> the sums of the workgroups before each; the totals
//   h2d_walk_kernel<true>   the same walk with the bases known: sent[], out_len, peers_out, cstatus, and per record
//                           with frames one job at its place among all jobs, with the count of lines before it
//   h2d_copy_kernel         the frames' bytes, by window_copy (hhuff_gather.h).  A lane's line: the frame index by one
//                           division when its job changes and by addition afterwards (256 lines are 4 KiB, a frame
//                           16 KiB or more), then h2d::write_line -- a line with header bytes (1 in 1,025 at 16 KiB)
//                           builds them in registers and takes the payload on either side from sources 9 bytes apart.
// Positions come from the scan alone: no atomics, no size read back, equal input gives equal bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_gather.h"
#include "hhuff_h2data.h"
#include "hhuff_launch.h"

#define HHUFF_API extern "C" __attribute__((visibility("default")))

namespace hhuff {
namespace {

struct DataArgs {
    const uint8_t* body;
    uint64_t body_size;
    const hhuff_h2_send_t* sends;
    const uint32_t* send_first;
    uint32_t nsend, nconn;
    const hhuff_h2_peer_t* peers_in;
    hhuff_h2_peer_t* peers_out;
    hhuff_h2_sent_t* sent;
    uint8_t* out;
    uint64_t out_size;
    const uint32_t* out_off;
    uint32_t* out_len;
    int32_t* cstatus;
    // workspace
    uint2* count;   // [nconn]: jobs, lines
    uint2* part;    // [walk workgroups]: their sums of count, then the sums of the workgroups before
    uint2* tot;     // all jobs, all lines
    h2d::Job* job;  // [nsend]
    uint32_t* pre;  // [nsend]: the lines of the jobs before
};

__device__ __forceinline__ uint32_t lines_of(const uint8_t* out, const h2d::Job& J) {
    const uint64_t n = J.out_bytes();
    return n ? lc::lines_of((uint64_t)(uintptr_t)out + J.dst, n) : 0u;
}

struct CountSink {
    const uint8_t* out;
    uint32_t jobs, lines;
    __device__ void record(uint32_t, const hhuff_h2_sent_t& T, const h2d::Job& J) {
        if (T.nframes != 0) ++jobs, lines += lines_of(out, J);
    }
};

struct PlaceSink {
    const DataArgs& A;
    uint32_t s0, jobs, lines;
    __device__ void record(uint32_t i, const hhuff_h2_sent_t& T, const h2d::Job& J) {
        A.sent[s0 + i] = T;
        if (T.nframes == 0) return;
        if (jobs < A.nsend) A.job[jobs] = J, A.pre[jobs] = lines;  // (beyond only with a send_first that is no running sum)
        ++jobs, lines += lines_of(A.out, J);
    }
};

template <bool PLACE>
__global__ __launch_bounds__(kWalkThreads) void h2d_walk_kernel(DataArgs A) {
    const uint64_t c64 = (uint64_t)blockIdx.x * kWalkThreads + threadIdx.x;
    const bool act = c64 < A.nconn;  // (every lane stays for the workgroup's sums)
    const uint32_t c = (uint32_t)c64;
    uint32_t s0 = 0, n = 0, r0 = 0, room = 0;
    hhuff_h2_peer_t P{};
    if (act) {
        const lc::Range recs = lc::clamp_range(A.send_first[c], A.send_first[c + 1], A.nsend);
        // (out_size < 2^32: hhuff_h2_frame_data refuses a larger one, so the cast loses nothing)
        const lc::Range region = lc::clamp_range(A.out_off[c], A.out_off[c + 1], (uint32_t)A.out_size);
        s0 = recs.first, n = recs.count, r0 = region.first, room = region.count;
        P = A.peers_in[c];
    }
    h2d::Result res{};
    if (PLACE) {
        const uint2 mine = act ? A.count[c] : make_uint2(0u, 0u);
        uint2 before, all;
        wg_scan(mine, before, all);
        if (!act) return;
        const uint2 wg = A.part[blockIdx.x];
        PlaceSink sink{A, s0, wg.x + before.x, wg.y + before.y};
        h2d::walk(A.body_size, A.sends + s0, n, P.max_frame_size, h2d::peer_ok(P), P.send_window, r0, room, sink, res);
        P.send_window = res.send_window;
        A.peers_out[c] = P;
        A.out_len[c] = res.out_len, A.cstatus[c] = res.status;
    } else {
        CountSink sink{A.out, 0u, 0u};
        if (act) {
            h2d::walk(A.body_size, A.sends + s0, n, P.max_frame_size, h2d::peer_ok(P), P.send_window, r0, room, sink, res);
            A.count[c] = make_uint2(sink.jobs, sink.lines);
        }
        uint2 before, all;
        wg_scan(make_uint2(sink.jobs, sink.lines), before, all);
        if (threadIdx.x == 0) A.part[blockIdx.x] = all;
    }
}

__global__ __launch_bounds__(kScanThreads) void h2d_scan_kernel(DataArgs A, uint32_t nparts) {
    const uint2 t = scan_parts(A.part, nparts);
    if (threadIdx.x == kScanThreads - 1u) *A.tot = t;
}

// window_copy's line: the lane's place in its job's frames carried from one line of the job to its next
struct FrameLine {
    uint64_t body, out;  // the addresses of body[0] and out[0]
    uint32_t last_k;
    uint64_t last_li;
    h2d::At at;
    __device__ __forceinline__ void admit(h2d::Job&) const {}  // (the walk placed every job inside its region)
    __device__ __forceinline__ void operator()(uint32_t k, const h2d::Job& J, uint64_t li) {
        const uint64_t d0 = out + J.dst, d1 = d0 + J.out_bytes();
        if (d1 == d0 || li >= lc::lines_of(d0, d1 - d0)) return;  // a line of the job's own, whatever pre holds
        const uint64_t line = (d0 & ~15ull) + 16ull * li;
        if (k != last_k)
            at = h2d::locate(J, (int64_t)(line - d0));  // the one division of this lane's span of the job's lines
        else
            h2d::advance(J, at, 16u * (li - last_li));
        last_k = k, last_li = li;
        h2d::write_line(body, J, d0, d1, line, at);
    }
};

__global__ __launch_bounds__(kCopyThreads) void h2d_copy_kernel(const uint8_t* __restrict__ body, uint8_t* __restrict__ out,
                                                                 const h2d::Job* __restrict__ job, const uint32_t* __restrict__ pre,
                                                                 const uint2* __restrict__ tot, uint32_t nsend) {
    FrameLine line{(uint64_t)(uintptr_t)body, (uint64_t)(uintptr_t)out, 0xffffffffu, 0, h2d::At{0u, 0}};
    window_copy(job, [pre](const h2d::Job&, uint32_t k) { return pre[k]; }, tot->x < nsend ? tot->x : nsend, tot->y, line);
}

// the workspace of a call: its size with base = NULL, its pointers with the allocation
uint64_t data_carve(DataArgs& A, uint32_t wgrid, uint8_t* base) {
    Carve cv{base};
    A.job = cv.take<h2d::Job>(A.nsend);
    A.pre = cv.take<uint32_t>(A.nsend);
    A.count = cv.take<uint2>(A.nconn);
    A.part = cv.take<uint2>((uint64_t)wgrid + 1u);
    A.tot = A.part + wgrid;
    return cv.off;
}

hipError_t launch_frame_data(DataArgs& A, hipStream_t stream) {
    const uint32_t wgrid = (uint32_t)(((uint64_t)A.nconn + kWalkThreads - 1u) / kWalkThreads);
    uint8_t* ws = nullptr;
    const hipError_t e = work_alloc((void**)&ws, data_carve(A, wgrid, nullptr), stream);
    if (e != hipSuccess) return e;
    data_carve(A, wgrid, ws);
    hipLaunchKernelGGL(h2d_walk_kernel<false>, dim3(wgrid), dim3(kWalkThreads), 0, stream, A);
    hipLaunchKernelGGL(h2d_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, A, wgrid);
    hipLaunchKernelGGL(h2d_walk_kernel<true>, dim3(wgrid), dim3(kWalkThreads), 0, stream, A);
    if (A.nsend != 0 && A.out_size != 0)  // the lines there can be: those of `out`, and a first or last one shared for every record
        hipLaunchKernelGGL(h2d_copy_kernel, dim3(copy_grid((A.out_size >> 4) + 2u * (uint64_t)A.nsend)), dim3(kCopyThreads), 0, stream,
                           A.body, A.out, A.job, A.pre, A.tot, A.nsend);
    return work_done(hipSuccess, ws, stream);
}

}  // namespace
}  // namespace hhuff

HHUFF_API int hhuff_h2_frame_data(const uint8_t* body, uint64_t body_size, const hhuff_h2_send_t* sends, const uint32_t* send_first,
                                  uint32_t nsend, uint32_t nconn, unsigned flags, const hhuff_h2_peer_t* peers_in,
                                  hhuff_h2_peer_t* peers_out, hhuff_h2_sent_t* sent, uint8_t* out, uint64_t out_size,
                                  const uint32_t* out_off, uint32_t* out_len, int32_t* cstatus, void* stream) {
    if (!body || !sends || !send_first || !peers_in || !peers_out || !sent || !out || !out_off || !out_len || !cstatus) return HHUFF_EINVAL;
    if ((body_size >> 32) || (out_size >> 32)) return HHUFF_EINVAL;
    if (flags != 0) return HHUFF_EINVAL;
    if (nconn == 0) return HHUFF_OK;
    hhuff::DataArgs A{};
    A.body = body, A.body_size = body_size, A.sends = sends, A.send_first = send_first, A.nsend = nsend, A.nconn = nconn;
    A.peers_in = peers_in, A.peers_out = peers_out, A.sent = sent, A.out = out, A.out_size = out_size, A.out_off = out_off;
    A.out_len = out_len, A.cstatus = cstatus;
    return hhuff::launch_frame_data(A, (hipStream_t)stream) == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}
