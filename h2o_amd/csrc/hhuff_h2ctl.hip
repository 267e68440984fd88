// HTTP/2 control frames (include/hhuff.h (2k'); the rules live in hhuff_h2ctl.h, shared with the host).
//   h2c_walk_kernel       one lane per connection walks its frame records in wire order (h2c::walk): a record's first
//                         16 bytes in, the payload's few bytes read bytewise, one 16-byte result record out, the
//                         replies into the connection's own region.  The order within a connection is the work --
//                         SETTINGS change later deltas, the send window accumulates, the first failure cuts the rest --
//                         and the regions are the caller's, so there is no scan, no workspace and no atomic.
//   set_peers_kernel      hhuff_hpack_responses_set_peers: one lane per response finds its connection by bisection of
//                         conn_first and stores the two settings
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_h2ctl.h"

#define HHUFF_API extern "C" __attribute__((visibility("default")))

namespace hhuff {
namespace {

constexpr uint32_t kCtlThreads = 256;

struct CtlArgs {
    const uint8_t* in;
    uint64_t in_size;
    const hhuff_h2_frame_t* frames;
    const uint32_t* nframes;
    const uint32_t* frm_first;
    uint32_t frm_cap, nconn;
    h2c::Params P;
    const hhuff_h2_peer_t* peers_in;
    hhuff_h2_peer_t* peers_out;
    hhuff_h2_ctl_t* ctl;
    uint32_t* nctl;
    int32_t* cstatus;
    uint32_t* cerr;
    uint8_t* rep;
    uint64_t rep_size;
    const uint32_t* rep_off;
    uint32_t* rep_len;
};

struct StoreSink {
    hhuff_h2_ctl_t* ctl;  // the connection's first record
    __device__ void record(uint32_t i, const hhuff_h2_ctl_t& r) { ctl[i] = r; }
};

__global__ __launch_bounds__(kCtlThreads) void h2c_walk_kernel(CtlArgs A) {
    const uint64_t c64 = (uint64_t)blockIdx.x * kCtlThreads + threadIdx.x;
    if (c64 >= A.nconn) return;
    const uint32_t c = (uint32_t)c64;
    // whatever frm_first, nframes and rep_off hold, the slots stay inside [0, frm_cap) and the replies inside rep
    const uint32_t a = A.frm_first[c], b = A.frm_first[c + 1];
    const uint32_t f0 = a < A.frm_cap ? a : A.frm_cap;
    const uint32_t f1 = b < f0 ? f0 : (b < A.frm_cap ? b : A.frm_cap);
    const uint32_t listed = A.nframes[c];
    const uint32_t n = listed < f1 - f0 ? listed : f1 - f0;
    const uint64_t r0 = A.rep_off[c], r1 = A.rep_off[c + 1];
    const uint64_t s0 = r0 < A.rep_size ? r0 : A.rep_size;
    const uint64_t s1 = r1 < s0 ? s0 : (r1 < A.rep_size ? r1 : A.rep_size);
    hhuff_h2_peer_t S = A.peers_in[c];
    StoreSink sink{A.ctl + f0};
    h2c::Result R;
    h2c::walk(A.in, A.in_size, A.frames + f0, n, A.P, S, A.rep + s0, (uint32_t)(s1 - s0), sink, R);
    A.peers_out[c] = S;
    A.nctl[c] = R.nctl, A.cstatus[c] = R.status, A.cerr[c] = R.err, A.rep_len[c] = R.rep_len;
}

__global__ __launch_bounds__(256) void set_peers_kernel(const hhuff_h2_peer_t* __restrict__ peers, hhuff_hpack_response_t* res,
                                                        const uint32_t* __restrict__ conn_first, uint32_t nconn, uint32_t nres) {
    const uint64_t r64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r64 >= nres) return;
    const uint32_t r = (uint32_t)r64;
    if (conn_first[0] > r || conn_first[nconn] <= r) return;
    uint32_t lo = 0, hi = nconn;  // the last c in [0, nconn) with conn_first[c] <= r (conn_first[lo] <= r throughout)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (conn_first[mid] <= r)
            lo = mid;
        else
            hi = mid;
    }
    res[r].header_table_size = peers[lo].header_table_size;
    res[r].max_frame_size = peers[lo].max_frame_size;
}

}  // namespace
}  // namespace hhuff

HHUFF_API int hhuff_h2_control(const uint8_t* in, uint64_t in_size, const hhuff_h2_frame_t* frames, const uint32_t* nframes,
                               const uint32_t* frm_first, uint32_t frm_cap, uint32_t nconn, unsigned flags, uint32_t recv_window_size,
                               const hhuff_h2_peer_t* peers_in, hhuff_h2_peer_t* peers_out, hhuff_h2_ctl_t* ctl, uint32_t* nctl,
                               int32_t* cstatus, uint32_t* cerr, uint8_t* rep, uint64_t rep_size, const uint32_t* rep_off,
                               uint32_t* rep_len, void* stream) {
    if (!in || !frames || !nframes || !frm_first || !peers_in || !peers_out || !ctl || !nctl || !cstatus || !cerr || !rep || !rep_off ||
        !rep_len)
        return HHUFF_EINVAL;
    if (in_size >> 32) return HHUFF_EINVAL;
    if (flags & ~HHUFF_H2C_CLIENT) return HHUFF_EINVAL;
    if (recv_window_size > 0x7fffffffu) return HHUFF_EINVAL;
    if (nconn == 0) return HHUFF_OK;
    hhuff::CtlArgs A{};
    A.in = in, A.in_size = in_size, A.frames = frames, A.nframes = nframes, A.frm_first = frm_first, A.frm_cap = frm_cap, A.nconn = nconn;
    A.P = hhuff::h2c::Params{flags, recv_window_size};
    A.peers_in = peers_in, A.peers_out = peers_out, A.ctl = ctl, A.nctl = nctl, A.cstatus = cstatus, A.cerr = cerr;
    A.rep = rep, A.rep_size = rep_size, A.rep_off = rep_off, A.rep_len = rep_len;
    const uint32_t grid = (uint32_t)(((uint64_t)nconn + hhuff::kCtlThreads - 1u) / hhuff::kCtlThreads);
    hipLaunchKernelGGL(hhuff::h2c_walk_kernel, dim3(grid), dim3(hhuff::kCtlThreads), 0, (hipStream_t)stream, A);
    return hipGetLastError() == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}

HHUFF_API int hhuff_hpack_responses_set_peers(const hhuff_h2_peer_t* peers, hhuff_hpack_response_t* res, const uint32_t* conn_first,
                                              uint32_t nconn, uint32_t nres, void* stream) {
    if (!peers || !res || !conn_first) return HHUFF_EINVAL;
    if (nconn == 0 || nres == 0) return HHUFF_OK;
    hipLaunchKernelGGL(hhuff::set_peers_kernel, dim3((uint32_t)(((uint64_t)nres + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream,
                       peers, res, conn_first, nconn, nres);
    return hipGetLastError() == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}
