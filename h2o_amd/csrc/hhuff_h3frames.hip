// HTTP/3 de-framer (include/hhuff.h (2l); the rules live in hhuff_h3frames.h, shared with the host).
//   h3f_walk_kernel<false>  one lane per stream follows the dependent chain of varints (h3f::walk with a sink that
//                           keeps nothing): nframes, consumed, sstatus, serr and st_out, the stream's four counts
//                           (sections, section bytes, encoder bytes, SETTINGS frames passed) to the workspace, and
//                           their sums over the workgroup's 256 streams
//   h3f_scan_kernel         one workgroup: the workgroups' sums -> the sums of the workgroups before each (a lane
//                           sums a run of consecutive entries, the runs' sums are scanned in LDS, the lane walks its
//                           run again), the grand total, conn_first[nconn], totals
//   h3f_walk_kernel<true>   the same walk with the bases known -- the workgroup's base plus a scan of its 256
//                           counts in LDS --: frame records, sec_off, sec_stream_id and sec_stream at their final
//                           places, the stream's sums-before to the workspace, the SETTINGS values of a control
//                           stream, and one gather job per stream (a stream has a section or an encoder run, never
//                           both; the jobs are zeroed first, so a stream without either is a job of length 0)
//   h3f_conn_kernel         one lane per connection: conn_first, enc_off, enc_len from the sums at conn_str[c];
//                           got_settings, and peers / settings from the first stream of the connection that passed
//                           SETTINGS (found by bisecting the running count of such streams)
//   h3f_finish_kernel       sec_off past nsec, arena_off
//   frm_gather_kernel       the copy (hhuff_gather.h)
// Positions come from the scan alone: no atomics, equal input gives equal bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_gather.h"
#include "hhuff_h3frames.h"
#include "hhuff_launch.h"

#define HHUFF_API extern "C" __attribute__((visibility("default")))

namespace hhuff {
namespace {

struct H3Args {
    const uint8_t* in;
    uint64_t in_size;
    const uint32_t* str_off;
    uint32_t nstr;
    const uint32_t* conn_str;
    uint32_t nconn;
    const uint32_t* frm_first;
    uint32_t frm_cap;
    uint64_t max_frame_payload_size;
    uint32_t flags;
    const hhuff_h3_stream_t* st_in;
    hhuff_h3_stream_t* st_out;
    hhuff_h3_frame_t* frames;
    uint32_t* nframes;
    uint32_t* consumed;
    int32_t* sstatus;
    uint32_t* serr;
    uint8_t* out;
    uint32_t* enc_off;
    uint32_t* enc_len;
    uint32_t* sec_off;
    uint32_t* conn_first;
    uint64_t* sec_stream_id;
    uint32_t* sec_stream;
    uint32_t* totals;
    hhuff_qpack_peer_t* peers;
    hhuff_h3_settings_t* settings;
    uint32_t* got_settings;
    uint64_t* arena_off;
    uint64_t arena_fixed;
    uint32_t arena_per_byte;
    // workspace
    uint4* job;      // [nstr]: source offset in `in`, destination offset in out, length, 0
    uint4* count;    // [nstr]: sections, section bytes, encoder bytes, SETTINGS passed
    uint4* before;   // [nstr + 1]: the sums of count over the streams before; [nstr] the totals
    uint4* part;     // [walk workgroups + 1]: their sums of count, then the sums of the workgroups before; the totals
    uint4* setting;  // [nstr]: max_table_capacity and max_blocked (saturated), max_field_section_size (lo, hi)
    uint8_t* dgram;  // [nstr]: h3_datagram
};

__device__ __forceinline__ uint32_t sat32(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

struct H3PlaceSink {
    const H3Args& A;
    uint32_t s, start, f0;
    uint64_t stream_id;
    uint32_t sec, sec_at, enc_at;  // the stream's section index; where its section / its encoder bytes go in out
    __device__ void frame(uint32_t i, const hhuff_h3_frame_t& rel) {
        hhuff_h3_frame_t f = rel;
        f.hdr_off += start, f.payload_off += start;
        if (f.type == h3f::kHeaders && f.aux != h3f::kNoSection) f.aux = sec;
        A.frames[f0 + i] = f;
    }
    __device__ void copy(uint32_t off, uint32_t n, uint32_t dst) {
        if (n != 0 && (uint64_t)dst + n <= A.in_size) A.job[s] = make_uint4(start + off, dst, n, 0u);
    }
    __device__ void section(uint32_t off, uint32_t n) {
        if (sec >= A.nstr) return;  // (a stream has at most one section: never taken)
        A.sec_off[sec] = sec_at, A.sec_stream_id[sec] = stream_id, A.sec_stream[sec] = s;
        copy(off, n, sec_at);
    }
    __device__ void encoder(uint32_t off, uint32_t n) { copy(off, n, enc_at); }
    __device__ void settings(const h3f::Settings& S) {
        A.setting[s] = make_uint4(sat32(S.max_table_capacity), sat32(S.max_blocked), (uint32_t)S.max_field_section_size,
                                  (uint32_t)(S.max_field_section_size >> 32));
        A.dgram[s] = (uint8_t)S.h3_datagram;
    }
};

template <bool PLACE>
__global__ __launch_bounds__(kWalkThreads) void h3f_walk_kernel(H3Args A) {
    const uint64_t s64 = (uint64_t)blockIdx.x * kWalkThreads + threadIdx.x;
    const bool act = s64 < A.nstr;  // (every lane stays for the workgroup's sums)
    const uint32_t s = (uint32_t)s64;
    h3f::Result res{};
    if (PLACE) {
        const uint4 mine = act ? A.count[s] : make_uint4(0u, 0u, 0u, 0u);
        uint4 before, all;
        wg_scan(mine, before, all);
        if (!act) return;
        const uint4 at = vadd(A.part[blockIdx.x], before);
        A.before[s] = at;
        const uint32_t enc_total = A.part[gridDim.x].z;  // the sections lie behind all encoder bytes
        const SlotRange R(A.str_off, A.frm_first, s, A.in_size, A.frm_cap);
        const hhuff_h3_stream_t st = A.st_in[s];
        const h3f::Params P{A.max_frame_payload_size, A.flags & HHUFF_H3F_CLIENT, R.cap};
        H3PlaceSink sink{A, s, R.start, R.f0, st.stream_id, at.x, enc_total + at.y, at.z};
        h3f::walk(A.in + R.start, R.len, st, P, sink, res);
        A.st_out[s] = h3f::next_state(st, res);  // (written here, behind the last read of st_in: st_out may be st_in)
    } else {
        if (act) {
            const SlotRange R(A.str_off, A.frm_first, s, A.in_size, A.frm_cap);
            const hhuff_h3_stream_t st = A.st_in[s];
            const h3f::Params P{A.max_frame_payload_size, A.flags & HHUFF_H3F_CLIENT, R.cap};
            h3f::NoSink sink;
            h3f::walk(A.in + R.start, R.len, st, P, sink, res);
            A.nframes[s] = res.nframes, A.consumed[s] = res.consumed, A.sstatus[s] = res.status, A.serr[s] = res.err;
            A.count[s] = make_uint4(res.nsec, res.sec_bytes, res.enc_bytes, res.got_settings);
        }
        uint4 before, all;
        wg_scan(make_uint4(res.nsec, res.sec_bytes, res.enc_bytes, res.got_settings), before, all);
        if (threadIdx.x == 0) A.part[blockIdx.x] = all;
    }
}

// part[w] (the sums of walk workgroup w) -> the sums of the workgroups before w, in place; part[nparts] and
// before[nstr] = the totals; conn_first[nconn], totals.
__global__ __launch_bounds__(kScanThreads) void h3f_scan_kernel(H3Args A, uint32_t nparts) {
    const uint4 t = scan_parts(A.part, nparts);
    if (threadIdx.x == kScanThreads - 1u) {
        A.part[nparts] = t, A.before[A.nstr] = t;
        A.conn_first[A.nconn] = t.x, A.totals[0] = t.x, A.totals[1] = t.y, A.totals[2] = t.z;
    }
}

__global__ __launch_bounds__(256) void h3f_conn_kernel(H3Args A) {
    const uint64_t c64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (c64 >= A.nconn) return;
    const uint32_t c = (uint32_t)c64;
    const uint32_t x = A.conn_str[c], y = A.conn_str[c + 1];
    const uint32_t a = x < A.nstr ? x : A.nstr;  // whatever conn_str holds, streams a .. b - 1 of [0, nstr)
    const uint32_t b = y < a ? a : (y < A.nstr ? y : A.nstr);
    const uint4 lo = A.before[a], hi = A.before[b];
    A.conn_first[c] = lo.x, A.enc_off[c] = lo.z, A.enc_len[c] = hi.z - lo.z;
    const bool got = hi.w != lo.w;
    A.got_settings[c] = got ? 1u : 0u;
    if (!got) return;
    uint32_t l = a, h = b;  // the first stream s of a .. b - 1 with before[s + 1].w > lo.w: before[l].w == lo.w < before[h].w
    while (h - l > 1) {
        const uint32_t mid = l + ((h - l) >> 1);
        if (A.before[mid].w == lo.w)
            l = mid;
        else
            h = mid;
    }
    const uint4 v = A.setting[l];
    hhuff_qpack_peer_t p;
    p.max_table_capacity = v.x, p.max_blocked = v.y;
    A.peers[c] = p;
    hhuff_h3_settings_t t;
    t.max_field_section_size = (uint64_t)v.z | ((uint64_t)v.w << 32), t.h3_datagram = A.dgram[l], t.rsv = 0;
    A.settings[c] = t;
}

__global__ __launch_bounds__(256) void h3f_finish_kernel(H3Args A) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k > A.nstr) return;
    const uint4 t = A.before[A.nstr];  // the totals
    const uint32_t nsec = t.x < A.nstr ? t.x : A.nstr;
    uint32_t off;
    if (k >= nsec)
        A.sec_off[k] = off = t.z + t.y;
    else
        off = A.sec_off[k];
    if (A.arena_off) A.arena_off[k] = A.arena_fixed * (k < nsec ? k : nsec) + (uint64_t)A.arena_per_byte * (uint32_t)(off - t.z);
}

hipError_t launch_h3_deframe(H3Args& A, hipStream_t stream) {
    const uint32_t wgrid = (uint32_t)(((uint64_t)A.nstr + kWalkThreads - 1u) / kWalkThreads);
    const uint64_t n = A.nstr;
    const uint64_t dgram_bytes = (n + 15u) & ~15ull;
    // job, count, setting [nstr], before [nstr + 1], part [wgrid + 1] of 16 bytes each, then dgram
    const uint64_t bytes = 16u * (4u * n + 1u + wgrid + 1u) + dgram_bytes;
    uint8_t* ws = nullptr;
    hipError_t e = work_alloc((void**)&ws, bytes, stream);
    if (e != hipSuccess) return e;
    A.job = reinterpret_cast<uint4*>(ws);
    A.count = A.job + n;
    A.setting = A.count + n;
    A.before = A.setting + n;
    A.part = A.before + n + 1u;
    A.dgram = reinterpret_cast<uint8_t*>(A.part + wgrid + 1u);
    e = hipMemsetAsync(A.job, 0, 16u * n, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(h3f_walk_kernel<false>, dim3(wgrid), dim3(kWalkThreads), 0, stream, A);
        hipLaunchKernelGGL(h3f_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, A, wgrid);
        hipLaunchKernelGGL(h3f_walk_kernel<true>, dim3(wgrid), dim3(kWalkThreads), 0, stream, A);
        hipLaunchKernelGGL(h3f_conn_kernel, dim3((A.nconn + 255u) / 256u), dim3(256), 0, stream, A);
        hipLaunchKernelGGL(h3f_finish_kernel, dim3((uint32_t)((n + 1u + 255u) / 256u)), dim3(256), 0, stream, A);
        hipLaunchKernelGGL(frm_gather_kernel, dim3((uint32_t)((n + kGatherThreads - 1u) / kGatherThreads)), dim3(kGatherThreads), 0,
                           stream, A.in, A.out, A.job, A.nstr);
        e = hipGetLastError();
    }
    const hipError_t f = hipFreeAsync(ws, stream);
    return e != hipSuccess ? e : f;
}

}  // namespace
}  // namespace hhuff

HHUFF_API int hhuff_h3_deframe(const uint8_t* in, uint64_t in_size, const uint32_t* str_off, uint32_t nstr, const uint32_t* conn_str,
                               uint32_t nconn, const uint32_t* frm_first, uint32_t frm_cap, uint64_t max_frame_payload_size,
                               unsigned flags, const hhuff_h3_stream_t* st_in, hhuff_h3_stream_t* st_out, hhuff_h3_frame_t* frames,
                               uint32_t* nframes, uint32_t* consumed, int32_t* sstatus, uint32_t* serr, uint8_t* out,
                               uint32_t* enc_off, uint32_t* enc_len, uint32_t* sec_off, uint32_t* conn_first,
                               uint64_t* sec_stream_id, uint32_t* sec_stream, uint32_t* totals, hhuff_qpack_peer_t* peers,
                               hhuff_h3_settings_t* settings, uint32_t* got_settings, uint64_t* arena_off, uint64_t arena_fixed,
                               uint32_t arena_per_byte, void* stream) {
    if (!in || !str_off || !conn_str || !frm_first || !st_in || !st_out || !frames || !nframes || !consumed || !sstatus || !serr ||
        !out || !enc_off || !enc_len || !sec_off || !conn_first || !sec_stream_id || !sec_stream || !totals || !peers || !settings ||
        !got_settings)
        return HHUFF_EINVAL;
    if (in_size > 0xFFFFFFFDull) return HHUFF_EINVAL;
    if (flags & ~HHUFF_H3F_CLIENT) return HHUFF_EINVAL;
    if (nstr == 0 || nconn == 0) return HHUFF_OK;
    hhuff::H3Args A{};
    A.in = in, A.in_size = in_size, A.str_off = str_off, A.nstr = nstr, A.conn_str = conn_str, A.nconn = nconn;
    A.frm_first = frm_first, A.frm_cap = frm_cap, A.max_frame_payload_size = max_frame_payload_size, A.flags = flags;
    A.st_in = st_in, A.st_out = st_out, A.frames = frames, A.nframes = nframes, A.consumed = consumed, A.sstatus = sstatus;
    A.serr = serr, A.out = out, A.enc_off = enc_off, A.enc_len = enc_len, A.sec_off = sec_off, A.conn_first = conn_first;
    A.sec_stream_id = sec_stream_id, A.sec_stream = sec_stream, A.totals = totals, A.peers = peers, A.settings = settings;
    A.got_settings = got_settings, A.arena_off = arena_off, A.arena_fixed = arena_fixed, A.arena_per_byte = arena_per_byte;
    return hhuff::launch_h3_deframe(A, (hipStream_t)stream) == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}
