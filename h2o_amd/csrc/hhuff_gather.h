// What the device copies share on the device side: the scaffolding of the de-framers' and the body calls' passes, the
// de-framers' gather and the job-window copy.  A line's loads and stores are hhuff_linecopy.h's.
//   SlotRange               a connection's / stream's bytes and frame slots, clamped to the input and to frm_cap
//   lds_scan                an inclusive scan in LDS, one entry a lane (uint2 and uint4 through vadd)
//   wg_scan                 sums over a walk workgroup's 256 lanes (uint2 and uint4 counts)
//   scan_parts              the body of the partial-sums pass: the walk workgroups' sums -> the sums of the workgroups
//                           before each, in place, and the grand total
//   frm_gather_kernel       copy jobs (source offset in `in`, destination offset in `blk`, length, 0), one a slot, jobs
//                           of length 0 skipped; parallel over fragments: a workgroup of 256 lanes takes 256 job slots, cuts
//                           every fragment at the destination's 16-byte lines (by address) into chunks, numbers the
//                           chunks of all its fragments through (an LDS scan of the chunk counts) and deals them
//                           out lane by lane: short fragments share a wave, a 16 KiB fragment's 1,024 chunks go
//                           over all four waves, consecutive lanes at consecutive 16 bytes of source and
//                           destination, each chunk one lc::copy_line.
//   copy_grid, copy_share, window_copy   the copy over a job list that one workgroup cannot hold (described below)
#ifndef HHUFF_GATHER_H
#define HHUFF_GATHER_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff_linecopy.h"

namespace hhuff {
namespace {

constexpr uint32_t kWalkThreads = 256;  // connections / streams a walk workgroup: the unit of the first level of sums
constexpr uint32_t kScanThreads = 1024;
constexpr uint32_t kGatherThreads = 256;

// Item i's bytes inside in[0 .. in_size) and its slots inside [0, frm_cap), whatever off and first hold (lc::clamp_range)
struct SlotRange {
    uint32_t start, len, f0, cap;
    __device__ SlotRange(const uint32_t* off, const uint32_t* first, uint32_t i, uint64_t in_size, uint32_t frm_cap) {
        const lc::Range bytes = lc::clamp_range(off[i], off[i + 1], (uint32_t)in_size);  // (in_size < 2^32: the calls' check)
        const lc::Range slots = lc::clamp_range(first[i], first[i + 1], frm_cap);
        start = bytes.first, len = bytes.count, f0 = slots.first, cap = slots.count;
    }
};

__device__ __forceinline__ uint2 vadd(uint2 a, uint2 b) { return make_uint2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ uint4 vadd(uint4 a, uint4 b) { return make_uint4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// Inclusive scan of s[0 .. N) in LDS by N lanes, one entry a lane (the caller's barrier stands behind its writes of s)
template <uint32_t N, class T>
__device__ __forceinline__ void lds_scan(T* s) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t d = 1; d < N; d <<= 1) {
        T o{};
        if (tid >= d) o = s[tid - d];
        __syncthreads();
        s[tid] = vadd(s[tid], o);
        __syncthreads();
    }
}

// Sums over a workgroup of kWalkThreads lanes: excl = the sum of the lanes before this one, total = all of them.
template <class T>
__device__ __forceinline__ void wg_scan(T v, T& excl, T& total) {
    __shared__ T s[kWalkThreads];
    const uint32_t tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    lds_scan<kWalkThreads>(s);
    excl = tid ? s[tid - 1u] : T{}, total = s[kWalkThreads - 1u];
}

// The partial-sums pass, by one workgroup of kScanThreads lanes: part[w] (the sums of walk workgroup w) -> the sums
// of the workgroups before w, in place.  A lane sums a run of consecutive entries, the runs' sums are scanned in LDS,
// the lane walks its run again.  Returns the sum through the lane's run: the grand total in the last lane.
template <class T>
__device__ __forceinline__ T scan_parts(T* part, uint32_t nparts) {
    __shared__ T run_sum[kScanThreads];
    const uint32_t tid = threadIdx.x;
    const uint32_t run = (nparts + kScanThreads - 1u) / kScanThreads;  // consecutive entries a lane
    const uint64_t p0 = (uint64_t)tid * run;
    const uint64_t p1 = p0 + run < nparts ? p0 + run : nparts;
    T s{};
    for (uint64_t p = p0; p < p1; ++p) s = vadd(s, part[p]);
    run_sum[tid] = s;
    __syncthreads();
    lds_scan<kScanThreads>(run_sum);
    T at = tid ? run_sum[tid - 1u] : T{};
    for (uint64_t p = p0; p < p1; ++p) {
        const T v = part[p];
        part[p] = at;
        at = vadd(at, v);
    }
    return run_sum[tid];
}

__global__ __launch_bounds__(kGatherThreads) void frm_gather_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ blk,
                                                                     const uint4* __restrict__ job, uint32_t njobs) {
    __shared__ uint32_t pre[kGatherThreads + 1];  // pre[k] = chunks of the jobs before k
    __shared__ uint4 sjob[kGatherThreads];
    const uint32_t tid = threadIdx.x;
    const uint64_t j = (uint64_t)blockIdx.x * kGatherThreads + tid;
    const uint4 J = j < njobs ? job[j] : make_uint4(0u, 0u, 0u, 0u);
    sjob[tid] = J;
    if (tid == 0) pre[0] = 0;
    pre[tid + 1u] = J.z ? lc::lines_of((uint64_t)(uintptr_t)blk + J.y, J.z) : 0u;
    __syncthreads();
    for (uint32_t d = 1; d < kGatherThreads; d <<= 1) {  // (on lds_scan this kernel gains an instruction: kept as it was)
        uint32_t o = 0;
        if (tid >= d) o = pre[tid + 1u - d];
        __syncthreads();
        pre[tid + 1u] += o;
        __syncthreads();
    }
    const uint32_t total = pre[kGatherThreads];
    for (uint32_t t = tid; t < total; t += kGatherThreads) {
        uint32_t k = 0;  // the last job with pre[k] <= t: it has a chunk (jobs without one repeat their successor's sum)
#pragma unroll
        for (uint32_t step = kGatherThreads / 2; step > 0; step >>= 1)
            if (pre[k + step] <= t) k += step;
        const uint4 Q = sjob[k];
        const uint64_t d0 = (uint64_t)(uintptr_t)blk + Q.y;  // the fragment's first destination address
        lc::copy_line((uint64_t)(uintptr_t)in + Q.x, d0, d0 + Q.z, t - pre[k]);
    }
}

// The job-window copy of hhuff_h2_frame_data and hhuff_h2_bodies: jobs in destination order, job k (J) with pre(J, k) =
// the 16-byte destination lines of the jobs before it (in the job or in an array beside it), njobs and `total` lines in all.  The lines of all jobs are numbered
// through; a workgroup takes an equal share of the numbers in tiles of 256 (copy_share: one 64 MiB job spreads as
// 4,096 of 16 KiB do), finds its first job by bisection once, and then takes windows of 256 jobs into LDS.  A lane takes
// every 256th line of the window: the job by an LDS bisection, then line(k, J, li) for line li of job k, which is J.
// Both are the caller's, whatever the job array holds: line.admit(J), once as a job enters the window, checks it
// against the caller's buffers (and empties one that leaves them), line(k, J, li) checks li against J and writes.
constexpr uint32_t kCopyThreads = 256;
constexpr uint32_t kCopyMaxGrid = 2048;  // 8 workgroups a CU

// the workgroups of a copy over at most `most` (>= 1) lines
inline uint32_t copy_grid(uint64_t most) {
    const uint64_t want = (most + kCopyThreads - 1u) / kCopyThreads;
    return (uint32_t)(want < kCopyMaxGrid ? want : kCopyMaxGrid);
}

// workgroup `block` of `grid`: its share [p0, p1) of `total` lines, in tiles of kCopyThreads
struct Share {
    uint64_t p0, p1;
};
__host__ __device__ __forceinline__ Share copy_share(uint64_t total, uint32_t block, uint32_t grid) {
    const uint64_t tiles = (total + kCopyThreads - 1u) / kCopyThreads;
    const uint64_t e1 = tiles * (block + 1u) / grid * kCopyThreads;
    return Share{tiles * block / grid * kCopyThreads, e1 < total ? e1 : total};
}

template <class Job, class Pre, class Line>
__device__ __forceinline__ void window_copy(const Job* __restrict__ job, Pre pre, uint32_t njobs, uint32_t total, Line& line) {
    __shared__ uint32_t spre[kCopyThreads + 1];  // spre[k] = the lines before job k0 + k
    __shared__ Job sjob[kCopyThreads];
    const uint32_t tid = threadIdx.x;
    if (njobs == 0 || total == 0) return;
    const Share S = copy_share(total, blockIdx.x, gridDim.x);
    if (S.p0 >= S.p1) return;
    uint32_t k0 = 0;  // the last job with pre <= p0
    for (uint32_t hi = njobs; hi - k0 > 1u;) {
        const uint32_t mid = k0 + (hi - k0) / 2u;
        if (pre(job[mid], mid) <= S.p0)
            k0 = mid;
        else
            hi = mid;
    }
    for (uint64_t p = S.p0; p < S.p1;) {
        const uint64_t idx = (uint64_t)k0 + tid;
        Job Z{};
        if (idx < njobs) Z = job[idx];
        line.admit(Z);
        sjob[tid] = Z, spre[tid] = idx < njobs ? pre(Z, (uint32_t)idx) : total;
        if (tid == 0) spre[kCopyThreads] = (uint64_t)k0 + kCopyThreads < njobs ? pre(job[k0 + kCopyThreads], k0 + kCopyThreads) : total;
        __syncthreads();
        const uint64_t wend = S.p1 < spre[kCopyThreads] ? S.p1 : spre[kCopyThreads];
        for (uint64_t q = p + tid; q < wend; q += kCopyThreads) {
            uint32_t k = 0;  // the last job of the window with spre[k] <= q
#pragma unroll
            for (uint32_t step = kCopyThreads / 2; step > 0; step >>= 1)
                if (spre[k + step] <= q) k += step;
            if (q >= spre[k]) line(k0 + k, sjob[k], q - spre[k]);  // (else pre is no running sum: no job's line)
        }
        __syncthreads();
        if (wend <= p) break;  // (only with line counts that wrapped: regions that overlap)
        p = wend, k0 += kCopyThreads;
    }
}

}  // namespace
}  // namespace hhuff
#endif
