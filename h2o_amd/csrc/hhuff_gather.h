// What the two de-framers (hhuff_frames.hip, hhuff_h3frames.hip) share: the scaffolding of their passes and the gather.
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
//                           destination.  A chunk's bytes come from the five aligned source dwords that hold
//                           them, funnel-shifted; a whole chunk is one 16-byte store, a fragment's first and last
//                           line, which it shares with its neighbours, dword and byte stores of its own bytes.
#ifndef HHUFF_GATHER_H
#define HHUFF_GATHER_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hhuff {
namespace {

constexpr uint32_t kWalkThreads = 256;  // connections / streams a walk workgroup: the unit of the first level of sums
constexpr uint32_t kScanThreads = 1024;
constexpr uint32_t kGatherThreads = 256;

// Whatever off and first hold, item i's bytes stay inside in[0 .. in_size) and its slots inside [0, frm_cap).
struct SlotRange {
    uint32_t start, len, f0, cap;
    __device__ SlotRange(const uint32_t* off, const uint32_t* first, uint32_t i, uint64_t in_size, uint32_t frm_cap) {
        const uint64_t s = off[i], e = off[i + 1];
        start = (uint32_t)(s < in_size ? s : in_size);
        const uint64_t e2 = e < start ? start : (e < in_size ? e : in_size);
        len = (uint32_t)(e2 - start);
        const uint32_t a = first[i], b = first[i + 1];
        f0 = a < frm_cap ? a : frm_cap;
        const uint32_t f1 = b < f0 ? f0 : (b < frm_cap ? b : frm_cap);
        cap = f1 - f0;
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
    uint32_t nch = 0;
    if (J.z != 0) {
        const uint64_t d = (uint64_t)(uintptr_t)blk + J.y;
        nch = (uint32_t)(((d + J.z + 15u) >> 4) - (d >> 4));
    }
    sjob[tid] = J;
    if (tid == 0) pre[0] = 0;
    pre[tid + 1u] = nch;
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
        const uint64_t d0 = (uint64_t)(uintptr_t)blk + Q.y, d1 = d0 + Q.z;  // the fragment's destination addresses
        const uint64_t line = (d0 & ~15ull) + 16ull * (t - pre[k]);
        const uint64_t lo = line > d0 ? line : d0, hi = line + 16u < d1 ? line + 16u : d1;
        const uint32_t b0 = (uint32_t)(lo - line), b1 = (uint32_t)(hi - line);  // the fragment's bytes of the line
        // The line's 16 bytes from the aligned source dwords that hold them: sv = where byte 0 of the line comes
        // from (before the fragment when b0 > 0: no such byte is loaded), dword m = the line's bytes 4 m - r ..
        // 4 m - r + 3, loaded only when one of them is the fragment's.
        const uint64_t sv = (uint64_t)(uintptr_t)in + Q.x + (line - d0);
        const uint32_t r = (uint32_t)(sv & 3u);
        const uint32_t* a = reinterpret_cast<const uint32_t*>((uintptr_t)(sv - r));
        uint32_t w[5], v[4];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            const int first = 4 * m - (int)r;
            w[m] = (first < (int)b1 && first + 4 > (int)b0) ? a[m] : 0u;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = __builtin_amdgcn_alignbit(w[q + 1], w[q], 8u * r);
        uint8_t* d = reinterpret_cast<uint8_t*>((uintptr_t)line);
        if (b1 - b0 == 16u) {
            *reinterpret_cast<uint4*>(d) = make_uint4(v[0], v[1], v[2], v[3]);
        } else {  // a line shared with the neighbours: whole dwords where the fragment has them, else bytes
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                if (b0 <= 4u * q && 4u * q + 4u <= b1) {
                    reinterpret_cast<uint32_t*>(d)[q] = v[q];
                } else {
#pragma unroll
                    for (uint32_t i = 0; i < 4; ++i)
                        if (4u * q + i >= b0 && 4u * q + i < b1) d[4u * q + i] = (uint8_t)(v[q] >> (8u * i));
                }
            }
        }
    }
}

}  // namespace
}  // namespace hhuff
#endif
