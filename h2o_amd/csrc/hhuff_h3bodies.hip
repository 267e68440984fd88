// HTTP/3 bodies: hhuff_h3_bodies on the receive side and hhuff_h3_frame_data on the send side (include/hhuff.h (2l'),
// (2l''); the arithmetic lives in hhuff_h3bodies.h, shared with the host).  Both are a scan and a copy over a list of
// segments in destination order -- a frame slot's payload, or a send record's header and payload:
//   h3b_count_kernel / h3s_count_kernel   one lane per frame slot / send record, never per stream: the slot's stream by
//                      bisection over frm_first, membership by the clamped range, its counts (bytes, DATA slots, bad
//                      slots); the sums of the lanes before it in the workgroup, and the workgroup's sums
//   h3b_scan_kernel    one workgroup: the workgroups' sums -> the sums of the workgroups before each; the totals
//   h3b_runs_kernel    one lane per stream: the run record from differences of the prefix at its first and last slot;
//                      the content-length cut by bisection over its slots (h3b::over is monotone along a stream)
//   h3s_place_kernel   one lane per send record: frm_off and sstatus from the same differences
//   h3b_copy_kernel    the bytes of both calls.  The output is packed, so its 16-byte lines (cut by address) have one
//                      writer each: a workgroup takes an equal share of the lines (copy_share, hhuff_gather.h), bisects the
//                      prefix in global memory for its first and last segment, and pulls windows of up to kWindow segment
//                      prefixes and sources into LDS.  A lane takes every 256th line of the window: the segment of its
//                      first byte by an LDS bisection, then h3b::write_line -- inside one payload the line copy of
//                      hhuff_linecopy.h; with a header or several segments in the line a walk over them, the bytes
//                      assembled in registers, and still one store.  A segment behind the window (only when more than
//                      kWindow segments, empty ones counted, lie in one line's reach) is found in global memory.
// Positions come from the scans alone: no atomics, no size read back, equal input gives equal bytes.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_gather.h"
#include "hhuff_h3bodies.h"
#include "hhuff_launch.h"

#define HHUFF_API extern "C" __attribute__((visibility("default")))

namespace hhuff {
namespace {

using h3b::Cnt;

constexpr uint32_t kWindow = 2048;       // segments a window: 256 lines of eight 2-byte frames each fill the workgroup
static_assert(kWalkThreads == 256, "Prefix::at finds a slot's workgroup by a shift");

// The scans' result: the sums over the segments before i -- at(n): over all of them
struct Prefix {
    const Cnt* pre;   // [n]: the sums of the lanes before, in the workgroup
    const Cnt* part;  // [workgroups]: the sums of the workgroups before
    const Cnt* tot;
    uint32_t n;
    __device__ __forceinline__ Cnt at(uint64_t i) const { return i < n ? h3b::vadd(part[i >> 8], pre[i]) : *tot; }
    __device__ __forceinline__ uint64_t bytes(uint64_t i) const { return i < n ? part[i >> 8].bytes + pre[i].bytes : tot->bytes; }
    // the last k in [lo, hi) with bytes(k) <= x (lo if none): the segment that holds out[x] when it has a byte
    __device__ __forceinline__ uint64_t seg_of(uint64_t x, uint64_t lo, uint64_t hi) const {
        while (hi - lo > 1u) {
            const uint64_t mid = lo + (hi - lo) / 2u;
            if (bytes(mid) <= x)
                lo = mid;
            else
                hi = mid;
        }
        return lo;
    }
};

__device__ __forceinline__ uint32_t sat32(uint64_t v) { return v < 0xFFFFFFFFull ? (uint32_t)v : 0xFFFFFFFFu; }

struct BodyArgs {
    const uint8_t* in;
    uint64_t in_size;
    const hhuff_h3_frame_t* frames;
    const uint32_t* nframes;
    const uint32_t* frm_first;
    uint32_t frm_cap, nstr;
    const uint64_t* content_length;
    const uint64_t* received;
    uint64_t out_size;
    hhuff_h3_body_run_t* runs;
    uint32_t* totals;
    Cnt *pre, *part, *tot;  // workspace
};

// stream s's slots [f0, f0 + n) inside [0, frm_cap), whatever frm_first and nframes hold
struct Slots {
    uint32_t f0, n;
};
__device__ __forceinline__ Slots slots_of(const BodyArgs& A, uint32_t s) {
    const lc::Range R = lc::clamp_range(A.frm_first[s], A.frm_first[s + 1], A.frm_cap);
    return Slots{R.first, A.nframes[s] < R.count ? A.nframes[s] : R.count};
}

__global__ __launch_bounds__(kWalkThreads) void h3b_count_kernel(BodyArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * kWalkThreads + threadIdx.x;
    Cnt c{0, 0, 0};
    if (i < A.frm_cap) {  // (every lane stays for the workgroup's sums)
        uint32_t s = 0;   // the last stream with frm_first[s] <= i: of streams without slots, the one behind them
        for (uint32_t hi = A.nstr; hi - s > 1u;) {
            const uint32_t mid = s + (hi - s) / 2u;
            if (A.frm_first[mid] <= i)
                s = mid;
            else
                hi = mid;
        }
        const Slots R = slots_of(A, s);
        if (i >= R.f0 && i - R.f0 < R.n) c = h3b::slot_count(A.frames[i], A.in_size);
    }
    Cnt before, all;
    wg_scan(c, before, all);
    if (i < A.frm_cap) A.pre[i] = before;
    if (threadIdx.x == 0) A.part[blockIdx.x] = all;
}

__global__ __launch_bounds__(kScanThreads) void h3b_scan_kernel(Cnt* part, uint32_t nparts, Cnt* tot, uint32_t* totals) {
    const Cnt t = scan_parts(part, nparts);
    if (threadIdx.x == kScanThreads - 1u) {
        *tot = t;
        if (totals) totals[0] = sat32(t.bytes), totals[1] = t.data;
    }
}

__global__ __launch_bounds__(kWalkThreads) void h3b_runs_kernel(BodyArgs A) {
    const uint64_t s64 = (uint64_t)blockIdx.x * kWalkThreads + threadIdx.x;
    if (s64 >= A.nstr) return;
    const uint32_t s = (uint32_t)s64;
    const Slots R = slots_of(A, s);
    const Prefix P{A.pre, A.part, A.tot, A.frm_cap};
    const Cnt B0 = P.at(R.f0), B1 = P.at((uint64_t)R.f0 + R.n);
    const uint64_t rcv = A.received ? A.received[s] : 0u, cl = A.content_length ? A.content_length[s] : UINT64_MAX;
    hhuff_h3_body_run_t run{(uint32_t)(B0.bytes < A.out_size ? B0.bytes : A.out_size), 0u, B1.data - B0.data, 0u, rcv, 0, 0u};
    if (rcv > cl || B1.bad != B0.bad) {
        run.status = HHUFF_H3BD_EINVAL;
    } else if (B1.bytes > A.out_size) {
        run.status = HHUFF_H3BD_SPACE;
    } else {
        uint32_t k = R.n;
        if (cl != UINT64_MAX)
            k = h3b::first_true(R.n, [&](uint32_t j) {
                return h3b::over(cl - rcv, P.bytes((uint64_t)R.f0 + j) - B0.bytes, h3b::header_length(A.frames[R.f0 + j]));
            });
        const Cnt Bk = P.at((uint64_t)R.f0 + k);
        run.len = (uint32_t)(Bk.bytes - B0.bytes), run.nframes = Bk.data - B0.data;
        run.flags = k < R.n ? HHUFF_H3BR_OVERFLOW : 0u;
        run.received = rcv + run.len;
    }
    A.runs[s] = run;
}

struct SendArgs {
    uint64_t body_size, out_size;
    const hhuff_h3_send_t* sends;
    uint32_t nsend;
    uint32_t* frm_off;
    int32_t* sstatus;
    Cnt *pre, *part, *tot;  // workspace
};

__global__ __launch_bounds__(kWalkThreads) void h3s_count_kernel(SendArgs A) {
    const uint64_t k = (uint64_t)blockIdx.x * kWalkThreads + threadIdx.x;
    Cnt c{0, 0, 0};
    if (k < A.nsend) {
        const hhuff_h3_send_t S = A.sends[k];
        if ((uint64_t)S.body_off + S.body_len > A.body_size)
            c.bad = 1u;
        else
            c.bytes = (uint64_t)h3b::hdr_len(S.body_len) + S.body_len, c.data = 1u;
    }
    Cnt before, all;
    wg_scan(c, before, all);
    if (k < A.nsend) A.pre[k] = before;
    if (threadIdx.x == 0) A.part[blockIdx.x] = all;
}

__global__ __launch_bounds__(kWalkThreads) void h3s_place_kernel(SendArgs A) {
    const uint64_t k = (uint64_t)blockIdx.x * kWalkThreads + threadIdx.x;
    if (k >= A.nsend) return;
    const Prefix P{A.pre, A.part, A.tot, A.nsend};
    const Cnt B0 = P.at(k), B1 = P.at(k + 1u);
    A.frm_off[k] = sat32(B0.bytes);
    if (k + 1u == A.nsend) A.frm_off[k + 1u] = sat32(B1.bytes);
    A.sstatus[k] = B1.bad != B0.bad ? HHUFF_H3BD_EINVAL : (B1.bytes > A.out_size ? HHUFF_H3BD_SPACE : 0);
}

struct CopyArgs {
    const uint8_t* src;  // the payloads: in / body
    uint64_t src_size;
    uint8_t* out;
    uint64_t out_size;
    const uint8_t* rec;  // segment k's source offset: the u32 at rec + k * stride (payload_off / body_off)
    uint32_t stride;
    Prefix P;
};

// Segment k's source, checked against src whatever the records hold by now: kBadSrc when its payload would leave it
template <bool kHdr>
__device__ __forceinline__ uint32_t source_of(const CopyArgs& A, uint64_t k, uint32_t sz) {
    if (sz == 0) return h3b::kBadSrc;
    const uint32_t src = *reinterpret_cast<const uint32_t*>(A.rec + k * A.stride);
    return (uint64_t)src + (sz - (kHdr ? h3b::hdr_of_size(sz) : 0u)) <= A.src_size ? src : h3b::kBadSrc;
}

template <bool kHdr>
struct Find {
    const CopyArgs& A;
    const uint32_t* spre;  // the window in LDS: segment k0 + j is out[spre[j] .. spre[j + 1]), j < cnt
    const uint32_t* ssrc;
    uint64_t k0;
    uint32_t cnt, limit;
    __device__ __forceinline__ h3b::Seg operator()(uint32_t x) const {
        if (x < spre[cnt]) {
            uint32_t lo = 0;  // the last segment of the window with spre[lo] <= x
            for (uint32_t hi = cnt; hi - lo > 1u;) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                if (spre[mid] <= x)
                    lo = mid;
                else
                    hi = mid;
            }
            return h3b::Seg{spre[lo], spre[lo + 1u], ssrc[lo]};
        }
        const uint64_t k = A.P.seg_of(x, k0 + cnt, A.P.n);  // behind the window
        const uint64_t d0 = A.P.bytes(k), d1 = A.P.bytes(k + 1u);
        const uint32_t s0 = (uint32_t)(d0 < limit ? d0 : limit), s1 = (uint32_t)(d1 < limit ? d1 : limit);
        return h3b::Seg{s0, s1, source_of<kHdr>(A, k, s1 - s0)};
    }
};

template <bool kHdr>
__global__ __launch_bounds__(kCopyThreads) void h3b_copy_kernel(CopyArgs A) {
    __shared__ uint32_t spre[kWindow + 1];
    __shared__ uint32_t ssrc[kWindow];
    const uint32_t tid = threadIdx.x;
    const uint64_t nseg = A.P.n, total = A.P.tot->bytes;
    if (nseg == 0) return;
    // what is written: everything, or the segments in front of the first that passes out_size
    const uint32_t limit = (uint32_t)(total <= A.out_size ? total : A.P.bytes(A.P.seg_of(A.out_size, 0, nseg)));
    if (limit == 0) return;
    const uint64_t base = (uint64_t)(uintptr_t)A.out;
    const uint32_t a = (uint32_t)(base & 15u);
    const uint64_t nlines = ((uint64_t)a + limit + 15u) >> 4;  // line q holds out[16 q - a .. 16 q - a + 16)
    const Share share = copy_share(nlines, blockIdx.x, gridDim.x);
    const uint64_t q0 = share.p0, q1 = share.p1;
    if (q0 >= q1) return;
    const uint64_t x_first = q0 == 0 ? 0u : 16u * q0 - a, x_last = (16u * q1 - a < limit ? 16u * q1 - a : limit) - 1u;
    const uint64_t k_first = A.P.seg_of(x_first, 0, nseg), k_last = A.P.seg_of(x_last, k_first, nseg);
    uint64_t q = q0;
    for (uint64_t k0 = k_first;; k0 += kWindow) {
        const bool last = k_last - k0 < kWindow;
        const uint32_t cnt = last ? (uint32_t)(k_last - k0) + 1u : kWindow;
        for (uint32_t j = tid; j <= cnt; j += kCopyThreads) {
            const uint64_t d = A.P.bytes(k0 + j);
            spre[j] = (uint32_t)(d < limit ? d : limit);
        }
        __syncthreads();
        for (uint32_t j = tid; j < cnt; j += kCopyThreads) ssrc[j] = source_of<kHdr>(A, k0 + j, spre[j + 1u] - spre[j]);
        __syncthreads();
        // the lines whose first byte lies in the window; the last window takes what is left of the share
        const uint64_t qw = ((uint64_t)spre[cnt] + a + 15u) >> 4;
        const uint64_t q_end = last || qw > q1 ? q1 : qw;
        const Find<kHdr> find{A, spre, ssrc, k0, cnt, limit};
        for (uint64_t l = q + tid; l < q_end; l += kCopyThreads)
            h3b::write_line<kHdr>((uint64_t)(uintptr_t)A.src, (base & ~15ull) + 16u * l, (int64_t)(16u * l) - a, limit, find);
        __syncthreads();
        if (last) break;
        if (q_end > q) q = q_end;
    }
}

template <bool kHdr>
void launch_copy(const CopyArgs& C, hipStream_t stream) {
    if (C.P.n == 0 || C.out_size == 0) return;
    hipLaunchKernelGGL(h3b_copy_kernel<kHdr>, dim3(copy_grid((C.out_size >> 4) + 2u)), dim3(kCopyThreads), 0, stream, C);  // the lines there can be
}

// the scans' workspace for n segments (A: BodyArgs or SendArgs): its size with base = NULL, its pointers with the allocation
template <class Args>
uint64_t scan_carve(Args& A, uint64_t n, uint32_t wgrid, uint8_t* base) {
    Carve cv{base};
    A.pre = cv.take<Cnt>(n);
    A.part = cv.take<Cnt>((uint64_t)wgrid + 1u);
    A.tot = A.part + wgrid;
    return cv.off;
}

hipError_t launch_bodies(BodyArgs& A, uint8_t* out, hipStream_t stream) {
    const uint32_t wgrid = (uint32_t)(((uint64_t)A.frm_cap + kWalkThreads - 1u) / kWalkThreads);
    uint8_t* ws = nullptr;
    const hipError_t e = work_alloc((void**)&ws, scan_carve(A, A.frm_cap, wgrid, nullptr), stream);
    if (e != hipSuccess) return e;
    scan_carve(A, A.frm_cap, wgrid, ws);
    if (wgrid != 0) hipLaunchKernelGGL(h3b_count_kernel, dim3(wgrid), dim3(kWalkThreads), 0, stream, A);
    hipLaunchKernelGGL(h3b_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, A.part, wgrid, A.tot, A.totals);
    hipLaunchKernelGGL(h3b_runs_kernel, dim3((uint32_t)(((uint64_t)A.nstr + kWalkThreads - 1u) / kWalkThreads)), dim3(kWalkThreads), 0,
                       stream, A);
    launch_copy<false>(CopyArgs{A.in, A.in_size, out, A.out_size, reinterpret_cast<const uint8_t*>(A.frames) + offsetof(hhuff_h3_frame_t, payload_off),
                                (uint32_t)sizeof(hhuff_h3_frame_t), Prefix{A.pre, A.part, A.tot, A.frm_cap}},
                       stream);
    return work_done(hipSuccess, ws, stream);
}

hipError_t launch_frame_data(SendArgs& A, const uint8_t* body, uint8_t* out, hipStream_t stream) {
    const uint32_t wgrid = (uint32_t)(((uint64_t)A.nsend + kWalkThreads - 1u) / kWalkThreads);
    uint8_t* ws = nullptr;
    const hipError_t e = work_alloc((void**)&ws, scan_carve(A, A.nsend, wgrid, nullptr), stream);
    if (e != hipSuccess) return e;
    scan_carve(A, A.nsend, wgrid, ws);
    hipLaunchKernelGGL(h3s_count_kernel, dim3(wgrid), dim3(kWalkThreads), 0, stream, A);
    hipLaunchKernelGGL(h3b_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, A.part, wgrid, A.tot, (uint32_t*)nullptr);
    hipLaunchKernelGGL(h3s_place_kernel, dim3(wgrid), dim3(kWalkThreads), 0, stream, A);
    launch_copy<true>(CopyArgs{body, A.body_size, out, A.out_size, reinterpret_cast<const uint8_t*>(A.sends) + offsetof(hhuff_h3_send_t, body_off),
                               (uint32_t)sizeof(hhuff_h3_send_t), Prefix{A.pre, A.part, A.tot, A.nsend}},
                      stream);
    return work_done(hipSuccess, ws, stream);
}

}  // namespace
}  // namespace hhuff

HHUFF_API int hhuff_h3_bodies(const uint8_t* in, uint64_t in_size, const hhuff_h3_frame_t* frames, const uint32_t* nframes,
                              const uint32_t* frm_first, uint32_t frm_cap, uint32_t nstr, const uint64_t* content_length,
                              const uint64_t* received, unsigned flags, uint8_t* out, uint64_t out_size, hhuff_h3_body_run_t* runs,
                              uint32_t* totals, void* stream) {
    if (!in || !frames || !nframes || !frm_first || !out || !runs || !totals) return HHUFF_EINVAL;
    if (in_size > 0xFFFFFFFDull || (out_size >> 32) || flags != 0) return HHUFF_EINVAL;
    if (nstr == 0) return HHUFF_OK;
    hhuff::BodyArgs A{};
    A.in = in, A.in_size = in_size, A.frames = frames, A.nframes = nframes, A.frm_first = frm_first, A.frm_cap = frm_cap, A.nstr = nstr;
    A.content_length = content_length, A.received = received, A.out_size = out_size, A.runs = runs, A.totals = totals;
    return hhuff::launch_bodies(A, out, (hipStream_t)stream) == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}

HHUFF_API int hhuff_h3_frame_data(const uint8_t* body, uint64_t body_size, const hhuff_h3_send_t* sends, uint32_t nsend, unsigned flags,
                                  uint8_t* out, uint64_t out_size, uint32_t* frm_off, int32_t* sstatus, void* stream) {
    if (!body || !sends || !out || !frm_off || !sstatus) return HHUFF_EINVAL;
    if ((body_size >> 32) || (out_size >> 32) || flags != 0) return HHUFF_EINVAL;
    if (nsend == 0) return HHUFF_OK;
    hhuff::SendArgs A{};
    A.body_size = body_size, A.out_size = out_size, A.sends = sends, A.nsend = nsend, A.frm_off = frm_off, A.sstatus = sstatus;
    return hhuff::launch_frame_data(A, body, out, (hipStream_t)stream) == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}
