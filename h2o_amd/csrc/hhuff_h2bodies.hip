// HTTP/2 request bodies on the receive side (include/hhuff.h (2k''''); the plan's arithmetic lives in hhuff_h2bodies.h,
// shared with the host).
//   h2b_plan_kernel    one lane per connection walks its events in wire order (h2b::walk): a frame's run is a lookup by
//                      stream id in the connection's own open-addressed table, carved from workspace at two entries a
//                      frame slot -- no scan of the earlier frames, so 4,000 small POSTs on one connection stay linear.
//                      It leaves per BODY slot its run, its offset inside the run, its source and length; per run its
//                      record, placed; per connection the verdict and the counts of copy jobs (BODY slots with bytes)
//                      and of the 16-byte destination lines they cover, and the sums over the workgroup's 256
//   h2b_scan_kernel    one workgroup: the workgroups' sums -> the sums of the workgroups before each; the totals
//   h2b_place_kernel   one lane per connection again, without a lookup: nrun, out_len, bstatus, the run records, and
//                      from the slots' records every job at its place among all jobs with the count of lines before it
//   h2b_copy_kernel    the bytes, by window_copy (hhuff_gather.h): one 1 MiB payload spreads as 256 of 4 KiB do.  Jobs
//                      have no headers inside, so a line is lc::copy_line and needs no frame arithmetic.
// Positions come from the scan alone: no atomics, no size read back, equal input gives equal bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_gather.h"
#include "hhuff_h2bodies.h"
#include "hhuff_launch.h"

#define HHUFF_API extern "C" __attribute__((visibility("default")))

namespace hhuff {
namespace {

struct BodyArgs {
    const uint8_t* in;
    uint64_t in_size;
    const hhuff_h2_ctl_t* ctl;
    const hhuff_h2_sev_t* sev;
    const uint32_t* frm_first;
    const uint32_t* nstr;
    uint32_t frm_cap, nconn;
    uint8_t* out;
    uint64_t out_size;
    const uint32_t* out_off;
    hhuff_h2_body_run_t* runs;
    uint32_t* nrun;
    uint32_t* out_len;
    int32_t* bstatus;
    // workspace
    h2b::Slot* slot;           // [frm_cap]
    hhuff_h2_body_run_t* run;  // [frm_cap]: connection c's runs from its first slot on, as in `runs`
    h2b::Key* tab;             // [2 frm_cap]: connection c's table stands at twice its first slot
    h2b::Job* job;             // [frm_cap]
    h2b::Plan* plan;           // [nconn]
    uint2* part;               // [plan workgroups]: their sums of (jobs, lines), then the sums of the workgroups before
    uint2* tot;                // all jobs, all lines
};

// connection c's slots inside [0, frm_cap) and its region inside out, whatever frm_first, nstr and out_off hold
// (out_size < 2^32: hhuff_h2_bodies refuses a larger one, so the cast loses nothing)
__device__ __forceinline__ h2b::Conn conn_of(const BodyArgs& A, uint32_t c) {
    const lc::Range slots = lc::clamp_range(A.frm_first[c], A.frm_first[c + 1], A.frm_cap);
    const lc::Range region = lc::clamp_range(A.out_off[c], A.out_off[c + 1], (uint32_t)A.out_size);
    const uint32_t f0 = slots.first, cap = slots.count, t0 = region.first, room = region.count;
    const uint32_t n = A.nstr[c] < cap ? A.nstr[c] : cap;
    return h2b::Conn{A.in_size, (uint64_t)(uintptr_t)A.out, A.ctl + f0, A.sev + f0, f0, n, t0, room,
                     A.tab + 2ull * f0, 2u * cap, A.slot + f0, A.run + f0};
}

__global__ __launch_bounds__(kWalkThreads) void h2b_plan_kernel(BodyArgs A) {
    const uint64_t c64 = (uint64_t)blockIdx.x * kWalkThreads + threadIdx.x;
    h2b::CountSink count{(uint64_t)(uintptr_t)A.out, 0u, 0u};
    if (c64 < A.nconn) {  // (every lane stays for the workgroup's sums)
        const uint32_t c = (uint32_t)c64;
        const h2b::Conn C = conn_of(A, c);
        h2b::Plan P = h2b::walk(C);
        h2b::jobs_of(C, P, count);
        P.jobs = count.jobs, P.lines = count.lines;
        A.plan[c] = P;
    }
    uint2 before, all;
    wg_scan(make_uint2(count.jobs, count.lines), before, all);
    if (threadIdx.x == 0) A.part[blockIdx.x] = all;
}

__global__ __launch_bounds__(kScanThreads) void h2b_scan_kernel(BodyArgs A, uint32_t nparts) {
    const uint2 t = scan_parts(A.part, nparts);
    if (threadIdx.x == kScanThreads - 1u) *A.tot = t;
}

struct PlaceSink {
    const BodyArgs& A;
    uint32_t jobs, lines;
    __device__ void job(uint32_t src, uint32_t dst, uint32_t len) {
        if (jobs < A.frm_cap) A.job[jobs] = h2b::Job{src, dst, len, lines};  // (beyond only with slots two connections share)
        ++jobs, lines += lc::lines_of((uint64_t)(uintptr_t)A.out + dst, len);
    }
};

__global__ __launch_bounds__(kWalkThreads) void h2b_place_kernel(BodyArgs A) {
    const uint64_t c64 = (uint64_t)blockIdx.x * kWalkThreads + threadIdx.x;
    const bool act = c64 < A.nconn;
    const uint32_t c = (uint32_t)c64;
    h2b::Plan P{};
    if (act) P = A.plan[c];
    uint2 before, all;
    wg_scan(make_uint2(P.jobs, P.lines), before, all);
    if (!act) return;
    const uint2 wg = A.part[blockIdx.x];
    const h2b::Conn C = conn_of(A, c);
    A.nrun[c] = P.nrun, A.out_len[c] = P.out_len, A.bstatus[c] = P.status;
    for (uint32_t k = 0; k < P.nrun; ++k) A.runs[C.first + k] = C.run[k];
    PlaceSink sink{A, wg.x + before.x, wg.y + before.y};
    h2b::jobs_of(C, P, sink);
}

// window_copy's job check and line: a job is copied only if it lies inside both arrays, whatever the workspace holds.
// (Measured, medians of three runs of tools/h2_bodies_rate.py, ms, before -> on the shared code: one 14.72 -> 14.56,
// interleaved 0.1956 -> 0.1957, interleaved_4096 0.5615 -> 0.5634, all inside the spread of the runs before; small
// (65,536 connections x one 4 KiB frame) 0.1531 -> 0.1540, where the runs before spread over 0.0004 and 0.1537 was the
// bound.  The same shape with this kernel's window loop written out here: 0.1545; with conn_of's clamps written out:
// 0.1544; and a kernel trace of the shape gives every kernel of the call the same mean before and after, within what
// two traces of one build differ by (copy 130.4 and 130.9 us before, 130.6 and 131.4 after; plan 8.18 and 8.21, 8.22 and
// 8.27).  So no body of its own is kept here: it buys nothing.)
struct BodyLine {
    uint64_t in, in_size, out, out_size;  // in, out: the addresses of in[0] and out[0]
    __device__ __forceinline__ void admit(h2b::Job& J) const {
        if ((uint64_t)J.src + J.len > in_size || (uint64_t)J.dst + J.len > out_size) J.len = 0;
    }
    __device__ __forceinline__ void operator()(uint32_t, const h2b::Job& J, uint64_t li) const {
        const uint64_t d0 = out + J.dst;
        if (J.len != 0 && li < lc::lines_of(d0, J.len)) lc::copy_line(in + J.src, d0, d0 + J.len, li);  // a line of the job's own
    }
};

__global__ __launch_bounds__(kCopyThreads) void h2b_copy_kernel(const uint8_t* __restrict__ in, uint64_t in_size, uint8_t* __restrict__ out,
                                                                 uint64_t out_size, const h2b::Job* __restrict__ job,
                                                                 const uint2* __restrict__ tot, uint32_t frm_cap) {
    BodyLine line{(uint64_t)(uintptr_t)in, in_size, (uint64_t)(uintptr_t)out, out_size};
    window_copy(job, [](const h2b::Job& J, uint32_t) { return J.pre; }, tot->x < frm_cap ? tot->x : frm_cap, tot->y, line);
}

// the workspace of a call: its size with base = NULL, its pointers with the allocation
uint64_t body_carve(BodyArgs& A, uint32_t wgrid, uint8_t* base) {
    Carve cv{base};
    const uint64_t cap = A.frm_cap;
    A.slot = cv.take<h2b::Slot>(cap);
    A.run = cv.take<hhuff_h2_body_run_t>(cap);
    A.tab = cv.take<h2b::Key>(2u * cap);
    A.job = cv.take<h2b::Job>(cap);
    A.plan = cv.take<h2b::Plan>(A.nconn);
    A.part = cv.take<uint2>((uint64_t)wgrid + 1u);
    A.tot = A.part + wgrid;
    return cv.off;
}

hipError_t launch_bodies(BodyArgs& A, hipStream_t stream) {
    const uint32_t wgrid = (uint32_t)(((uint64_t)A.nconn + kWalkThreads - 1u) / kWalkThreads);
    uint8_t* ws = nullptr;
    const hipError_t e = work_alloc((void**)&ws, body_carve(A, wgrid, nullptr), stream);
    if (e != hipSuccess) return e;
    body_carve(A, wgrid, ws);
    hipLaunchKernelGGL(h2b_plan_kernel, dim3(wgrid), dim3(kWalkThreads), 0, stream, A);
    hipLaunchKernelGGL(h2b_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, A, wgrid);
    hipLaunchKernelGGL(h2b_place_kernel, dim3(wgrid), dim3(kWalkThreads), 0, stream, A);
    if (A.frm_cap != 0 && A.out_size != 0 && A.in_size != 0)  // the lines there can be: those of `out`, and a first or last one shared for every job
        hipLaunchKernelGGL(h2b_copy_kernel, dim3(copy_grid((A.out_size >> 4) + 2u * (uint64_t)A.frm_cap)), dim3(kCopyThreads), 0, stream,
                           A.in, A.in_size, A.out, A.out_size, A.job, A.tot, A.frm_cap);
    return work_done(hipSuccess, ws, stream);
}

}  // namespace
}  // namespace hhuff

HHUFF_API int hhuff_h2_bodies(const uint8_t* in, uint64_t in_size, const hhuff_h2_ctl_t* ctl, const hhuff_h2_sev_t* sev,
                              const uint32_t* frm_first, uint32_t frm_cap, const uint32_t* nstr, uint32_t nconn, unsigned flags,
                              uint8_t* out, uint64_t out_size, const uint32_t* out_off, hhuff_h2_body_run_t* runs, uint32_t* nrun,
                              uint32_t* out_len, int32_t* bstatus, void* stream) {
    if (!in || !ctl || !sev || !frm_first || !nstr || !out || !out_off || !runs || !nrun || !out_len || !bstatus) return HHUFF_EINVAL;
    if ((in_size >> 32) || (out_size >> 32)) return HHUFF_EINVAL;
    if (flags != 0) return HHUFF_EINVAL;
    if (nconn == 0) return HHUFF_OK;
    hhuff::BodyArgs A{};
    A.in = in, A.in_size = in_size, A.ctl = ctl, A.sev = sev, A.frm_first = frm_first, A.nstr = nstr, A.frm_cap = frm_cap, A.nconn = nconn;
    A.out = out, A.out_size = out_size, A.out_off = out_off, A.runs = runs, A.nrun = nrun, A.out_len = out_len, A.bstatus = bstatus;
    return hhuff::launch_bodies(A, (hipStream_t)stream) == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}
