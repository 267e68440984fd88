// HTTP/2 DATA frames on the send side (include/hhuff.h (2k''); the arithmetic lives in hhuff_h2data.h, shared with
// the host).
//   h2d_walk_kernel<false>  one lane per connection serves its send records in order (h2d::walk, a closed form per
//                           record: no loop over frames): the connection's count of records with frames (copy jobs) and
//                           of the 16-byte destination lines they cover, and the sums over the workgroup's 256
//   h2d_scan_kernel         one workgroup: the workgroups' sums -> the sums of the workgroups before each; the totals
//   h2d_walk_kernel<true>   the same walk with the bases known: sent[], out_len, peers_out, cstatus, and per record
//                           with frames one job at its place among all jobs, with the count of lines before it
//   h2d_copy_kernel         the frames' bytes.  The lines of all jobs are numbered through; a workgroup takes an equal
//                           share of the numbers (a 64 MiB record spreads as 4,096 records of 16 KiB do), finds its
//                           first job by bisection once, and then takes windows of 256 jobs into LDS.  A lane takes
//                           every 256th line of the window: the job by an LDS bisection, the frame index by one
//                           division when the job changes and by addition afterwards (256 lines are 4 KiB, a frame
//                           16 KiB or more).  A line inside one frame's payload is five aligned source dwords,
//                           funnel-shifted, and one 16-byte store, as in frm_gather_kernel; a line with header bytes
//                           (1 in 1,025 at 16 KiB) builds them in registers and takes the payload on either side from
//                           sources 9 bytes apart; a job's first and last line, shared with its neighbours, are dword
//                           and byte stores of its own bytes.
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

constexpr uint32_t kCopyThreads = 256;
constexpr uint32_t kCopyMaxGrid = 2048;  // 8 workgroups a CU

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
    const uint64_t d = (uint64_t)(uintptr_t)out + J.dst, n = J.out_bytes();
    return n ? (uint32_t)(((d + n + 15u) >> 4) - (d >> 4)) : 0u;
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
        // whatever send_first and out_off hold, the records stay inside [0, nsend) and the frames inside out
        const uint32_t a = A.send_first[c], b = A.send_first[c + 1];
        s0 = a < A.nsend ? a : A.nsend;
        n = (b < s0 ? s0 : (b < A.nsend ? b : A.nsend)) - s0;
        const uint64_t o0 = A.out_off[c], o1 = A.out_off[c + 1];
        const uint64_t t0 = o0 < A.out_size ? o0 : A.out_size;
        r0 = (uint32_t)t0, room = (uint32_t)((o1 < t0 ? t0 : (o1 < A.out_size ? o1 : A.out_size)) - t0);
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

__global__ __launch_bounds__(kCopyThreads) void h2d_copy_kernel(const uint8_t* __restrict__ body, uint8_t* __restrict__ out,
                                                                 const h2d::Job* __restrict__ job, const uint32_t* __restrict__ pre,
                                                                 const uint2* __restrict__ tot, uint32_t nsend) {
    __shared__ uint32_t spre[kCopyThreads + 1];  // spre[k] = the lines before job k0 + k
    __shared__ h2d::Job sjob[kCopyThreads];
    const uint32_t tid = threadIdx.x;
    const uint32_t njobs = tot->x < nsend ? tot->x : nsend;
    const uint32_t total = tot->y;
    if (njobs == 0 || total == 0) return;
    // this workgroup's share of the line numbers, in tiles of 256
    const uint64_t tiles = ((uint64_t)total + kCopyThreads - 1u) / kCopyThreads;
    const uint64_t p0 = tiles * blockIdx.x / gridDim.x * kCopyThreads;
    const uint64_t e1 = tiles * (blockIdx.x + 1u) / gridDim.x * kCopyThreads;
    const uint64_t p1 = e1 < total ? e1 : total;
    if (p0 >= p1) return;
    uint32_t k0 = 0;  // the last job with pre[k0] <= p0
    for (uint32_t hi = njobs; hi - k0 > 1u;) {
        const uint32_t mid = k0 + (hi - k0) / 2u;
        if (pre[mid] <= p0)
            k0 = mid;
        else
            hi = mid;
    }
    for (uint64_t p = p0; p < p1;) {
        const uint64_t idx = (uint64_t)k0 + tid;
        spre[tid] = idx < njobs ? pre[idx] : total;
        if (tid == 0) spre[kCopyThreads] = (uint64_t)k0 + kCopyThreads < njobs ? pre[k0 + kCopyThreads] : total;
        h2d::Job Z{};
        if (idx < njobs) Z = job[idx];
        sjob[tid] = Z;
        __syncthreads();
        const uint64_t wend = p1 < spre[kCopyThreads] ? p1 : spre[kCopyThreads];
        uint32_t last_k = 0xffffffffu;
        uint64_t last_q = 0;
        h2d::At at{0u, 0};
        for (uint64_t q = p + tid; q < wend; q += kCopyThreads) {
            uint32_t k = 0;  // the last job of the window with spre[k] <= q
#pragma unroll
            for (uint32_t step = kCopyThreads / 2; step > 0; step >>= 1)
                if (spre[k + step] <= q) k += step;
            const h2d::Job J = sjob[k];
            const uint64_t nbytes = J.out_bytes();
            const uint64_t d0 = (uint64_t)(uintptr_t)out + J.dst, d1 = d0 + nbytes;
            const uint64_t li = q - spre[k];  // the line's number inside the job: a line of the job's own, whatever pre holds
            if (q < spre[k] || nbytes == 0 || li >= ((d1 + 15u) >> 4) - (d0 >> 4)) continue;
            const uint64_t line = (d0 & ~15ull) + 16ull * li;
            if (k != last_k)
                at = h2d::locate(J, (int64_t)(line - d0));  // the one division of this lane's span of the job's lines
            else
                h2d::advance(J, at, 16u * (q - last_q));
            last_k = k, last_q = q;
            h2d::write_line((uint64_t)(uintptr_t)body, J, d0, d1, line, at);
        }
        __syncthreads();
        if (wend <= p) break;  // (only with line counts that wrapped: regions that overlap)
        p = wend, k0 += kCopyThreads;
    }
}

hipError_t launch_frame_data(DataArgs& A, hipStream_t stream) {
    const uint32_t wgrid = (uint32_t)(((uint64_t)A.nconn + kWalkThreads - 1u) / kWalkThreads);
    const uint64_t job_bytes = (uint64_t)A.nsend * sizeof(h2d::Job);
    const uint64_t pre_bytes = ((uint64_t)A.nsend * 4u + 15u) & ~15ull;
    const uint64_t conn_bytes = ((uint64_t)A.nconn * 8u + 15u) & ~15ull;
    uint8_t* ws = nullptr;
    hipError_t e = work_alloc((void**)&ws, job_bytes + pre_bytes + conn_bytes + (uint64_t)wgrid * 8u + 16u, stream);
    if (e != hipSuccess) return e;
    A.job = reinterpret_cast<h2d::Job*>(ws);
    A.pre = reinterpret_cast<uint32_t*>(ws + job_bytes);
    A.count = reinterpret_cast<uint2*>(ws + job_bytes + pre_bytes);
    A.part = reinterpret_cast<uint2*>(ws + job_bytes + pre_bytes + conn_bytes);
    A.tot = A.part + wgrid;
    hipLaunchKernelGGL(h2d_walk_kernel<false>, dim3(wgrid), dim3(kWalkThreads), 0, stream, A);
    hipLaunchKernelGGL(h2d_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, A, wgrid);
    hipLaunchKernelGGL(h2d_walk_kernel<true>, dim3(wgrid), dim3(kWalkThreads), 0, stream, A);
    if (A.nsend != 0 && A.out_size != 0) {
        // the lines there can be: those of `out`, and a first or last one shared for every record
        const uint64_t most = (A.out_size >> 4) + 2u * (uint64_t)A.nsend;
        const uint64_t want = (most + kCopyThreads - 1u) / kCopyThreads;
        const uint32_t grid = (uint32_t)(want < kCopyMaxGrid ? want : kCopyMaxGrid);
        hipLaunchKernelGGL(h2d_copy_kernel, dim3(grid), dim3(kCopyThreads), 0, stream, A.body, A.out, A.job, A.pre, A.tot, A.nsend);
    }
    e = hipGetLastError();
    const hipError_t f = hipFreeAsync(ws, stream);
    return e != hipSuccess ? e : f;
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
