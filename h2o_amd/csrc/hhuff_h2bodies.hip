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
//   h2b_copy_kernel    the bytes.  The lines of all jobs are numbered through; a workgroup takes an equal share of the
//                      numbers (one 1 MiB payload spreads as 256 of 4 KiB do), finds its first job by bisection once,
//                      and then takes windows of 256 jobs into LDS.  A lane takes every 256th line of the window: the
//                      job by an LDS bisection, then h2b::copy_line -- five aligned source dwords, funnel-shifted, one
//                      16-byte store; a job's first and last line, shared with its neighbours in the run, are dword and
//                      byte stores of its own bytes.  Jobs have no headers inside, so a line needs no frame arithmetic.
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

constexpr uint32_t kCopyThreads = 256;
constexpr uint32_t kCopyMaxGrid = 2048;  // 8 workgroups a CU

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

// whatever frm_first, nstr and out_off hold, the slots stay inside [0, frm_cap) and the region inside out
__device__ __forceinline__ h2b::Conn conn_of(const BodyArgs& A, uint32_t c) {
    const uint32_t a = A.frm_first[c], b = A.frm_first[c + 1];
    const uint32_t f0 = a < A.frm_cap ? a : A.frm_cap;
    const uint32_t cap = (b < f0 ? f0 : (b < A.frm_cap ? b : A.frm_cap)) - f0;
    const uint32_t n = A.nstr[c] < cap ? A.nstr[c] : cap;
    const uint64_t o0 = A.out_off[c], o1 = A.out_off[c + 1];
    const uint64_t t0 = o0 < A.out_size ? o0 : A.out_size;
    const uint32_t room = (uint32_t)((o1 < t0 ? t0 : (o1 < A.out_size ? o1 : A.out_size)) - t0);
    return h2b::Conn{A.in_size, (uint64_t)(uintptr_t)A.out, A.ctl + f0, A.sev + f0, f0, n, (uint32_t)t0, room,
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
        ++jobs, lines += h2b::lines_of((uint64_t)(uintptr_t)A.out + dst, len);
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

__global__ __launch_bounds__(kCopyThreads) void h2b_copy_kernel(const uint8_t* __restrict__ in, uint64_t in_size, uint8_t* __restrict__ out,
                                                                 uint64_t out_size, const h2b::Job* __restrict__ job,
                                                                 const uint2* __restrict__ tot, uint32_t frm_cap) {
    __shared__ uint32_t spre[kCopyThreads + 1];  // spre[k] = the lines before job k0 + k
    __shared__ h2b::Job sjob[kCopyThreads];
    const uint32_t tid = threadIdx.x;
    const uint32_t njobs = tot->x < frm_cap ? tot->x : frm_cap;
    const uint32_t total = tot->y;
    if (njobs == 0 || total == 0) return;
    // this workgroup's share of the line numbers, in tiles of 256
    const uint64_t tiles = ((uint64_t)total + kCopyThreads - 1u) / kCopyThreads;
    const uint64_t p0 = tiles * blockIdx.x / gridDim.x * kCopyThreads;
    const uint64_t e1 = tiles * (blockIdx.x + 1u) / gridDim.x * kCopyThreads;
    const uint64_t p1 = e1 < total ? e1 : total;
    if (p0 >= p1) return;
    uint32_t k0 = 0;  // the last job with pre <= p0
    for (uint32_t hi = njobs; hi - k0 > 1u;) {
        const uint32_t mid = k0 + (hi - k0) / 2u;
        if (job[mid].pre <= p0)
            k0 = mid;
        else
            hi = mid;
    }
    for (uint64_t p = p0; p < p1;) {
        const uint64_t idx = (uint64_t)k0 + tid;
        h2b::Job Z{0u, 0u, 0u, total};
        if (idx < njobs) Z = job[idx];
        // a job is copied only if it lies inside both arrays, whatever the workspace holds
        if ((uint64_t)Z.src + Z.len > in_size || (uint64_t)Z.dst + Z.len > out_size) Z.len = 0;
        sjob[tid] = Z, spre[tid] = Z.pre;
        if (tid == 0) spre[kCopyThreads] = (uint64_t)k0 + kCopyThreads < njobs ? job[k0 + kCopyThreads].pre : total;
        __syncthreads();
        const uint64_t wend = p1 < spre[kCopyThreads] ? p1 : spre[kCopyThreads];
        for (uint64_t q = p + tid; q < wend; q += kCopyThreads) {
            uint32_t k = 0;  // the last job of the window with spre[k] <= q
#pragma unroll
            for (uint32_t step = kCopyThreads / 2; step > 0; step >>= 1)
                if (spre[k + step] <= q) k += step;
            const h2b::Job J = sjob[k];
            const uint64_t li = q - spre[k];  // the line's number inside the job: a line of the job's own, whatever pre holds
            if (q < spre[k] || J.len == 0 || li >= h2b::lines_of((uint64_t)(uintptr_t)out + J.dst, J.len)) continue;
            h2b::copy_line((uint64_t)(uintptr_t)in, (uint64_t)(uintptr_t)out, J, li);
        }
        __syncthreads();
        if (wend <= p) break;  // (only with line counts that wrapped: regions that overlap)
        p = wend, k0 += kCopyThreads;
    }
}

hipError_t launch_bodies(BodyArgs& A, hipStream_t stream) {
    const uint32_t wgrid = (uint32_t)(((uint64_t)A.nconn + kWalkThreads - 1u) / kWalkThreads);
    const uint64_t cap = A.frm_cap;
    const uint64_t slot_bytes = cap * sizeof(h2b::Slot), run_bytes = cap * sizeof(hhuff_h2_body_run_t);
    const uint64_t tab_bytes = 2u * cap * sizeof(h2b::Key), job_bytes = cap * sizeof(h2b::Job);
    const uint64_t plan_bytes = (uint64_t)A.nconn * sizeof(h2b::Plan);
    uint8_t* ws = nullptr;
    hipError_t e = work_alloc((void**)&ws, slot_bytes + run_bytes + tab_bytes + job_bytes + plan_bytes + (uint64_t)wgrid * 8u + 16u, stream);
    if (e != hipSuccess) return e;
    uint8_t* at = ws;  // every piece is a multiple of 16 bytes
    A.slot = reinterpret_cast<h2b::Slot*>(at), at += slot_bytes;
    A.run = reinterpret_cast<hhuff_h2_body_run_t*>(at), at += run_bytes;
    A.tab = reinterpret_cast<h2b::Key*>(at), at += tab_bytes;
    A.job = reinterpret_cast<h2b::Job*>(at), at += job_bytes;
    A.plan = reinterpret_cast<h2b::Plan*>(at), at += plan_bytes;
    A.part = reinterpret_cast<uint2*>(at);
    A.tot = A.part + wgrid;
    hipLaunchKernelGGL(h2b_plan_kernel, dim3(wgrid), dim3(kWalkThreads), 0, stream, A);
    hipLaunchKernelGGL(h2b_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, A, wgrid);
    hipLaunchKernelGGL(h2b_place_kernel, dim3(wgrid), dim3(kWalkThreads), 0, stream, A);
    if (A.frm_cap != 0 && A.out_size != 0 && A.in_size != 0) {
        // the lines there can be: those of `out`, and a first or last one shared for every job
        const uint64_t most = (A.out_size >> 4) + 2u * cap;
        const uint64_t want = (most + kCopyThreads - 1u) / kCopyThreads;
        const uint32_t grid = (uint32_t)(want < kCopyMaxGrid ? want : kCopyMaxGrid);
        hipLaunchKernelGGL(h2b_copy_kernel, dim3(grid), dim3(kCopyThreads), 0, stream, A.in, A.in_size, A.out, A.out_size, A.job, A.tot,
                           A.frm_cap);
    }
    e = hipGetLastError();
    const hipError_t f = hipFreeAsync(ws, stream);
    return e != hipSuccess ? e : f;
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
