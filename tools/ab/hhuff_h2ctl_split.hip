// A measured-and-rejected variant of hhuff_h2_control, built only into an A/B library in place of
// h2o_amd/csrc/hhuff_h2ctl.hip (HHUFF_AB_LIB): two kernels -- one lane per frame slot for the stateless verdicts into a
// pooled workspace, then one lane per connection for the ordered part (state, replies, the first failure).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_h2ctl.h"
#include "hhuff_launch.h"

#define HHUFF_API extern "C" __attribute__((visibility("default")))

namespace hhuff {
namespace {

constexpr uint32_t kCtlThreads = 256;
enum : uint32_t { kFinal = 0, kSettingsK = 1, kSendWin = 2, kDataWin = 3, kGoawayK = 4, kStreamErr = 5 };

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
    hhuff_h2_ctl_t* ws;
};

__global__ __launch_bounds__(kCtlThreads) void h2c_verdict_kernel(CtlArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * kCtlThreads + threadIdx.x;
    if (i >= A.frm_cap) return;
    const h2c::Frame F{A.frames[i].payload_off, A.frames[i].length, A.frames[i].stream_id, A.frames[i].type, A.frames[i].flags};
    hhuff_h2_ctl_t r{0, 0, 0, 0, 0, 0};
    uint32_t kind = kFinal;
    if ((uint64_t)F.payload_off + F.length > A.in_size) {
        r.status = HHUFF_H2C_EINVAL;
    } else if (F.type == h2c::kSettings && F.stream_id == 0 && (F.flags & h2c::kAck) == 0) {
        kind = kSettingsK;
    } else {
        hhuff_h2_peer_t T = HHUFF_H2_PEER_INIT;
        T.send_window = 0;
        const h2c::Params P0{A.P.flags, 0};
        h2c::Verdict v;
        h2c::Reply rp;
        h2c::step(A.in + F.payload_off, F, P0, T, v, rp);
        r = h2c::record_of(v, rp.len);
        if (v.status == 0 && F.type == h2c::kWindowUpdate && F.stream_id == 0) kind = kSendWin;
        if (v.status == 0 && F.type == h2c::kData) kind = kDataWin, r.err = (uint16_t)(F.length - v.b);
        if (v.status == 0 && F.type == h2c::kGoaway) kind = kGoawayK;
        if ((v.flags & HHUFF_H2R_STREAM_ERROR) != 0) kind = kStreamErr, r.a = F.stream_id;
    }
    r.flags |= (uint8_t)(kind << 5);
    A.ws[i] = r;
}

__global__ __launch_bounds__(kCtlThreads) void h2c_order_kernel(CtlArgs A) {
    const uint64_t c64 = (uint64_t)blockIdx.x * kCtlThreads + threadIdx.x;
    if (c64 >= A.nconn) return;
    const uint32_t c = (uint32_t)c64;
    const uint32_t a = A.frm_first[c], b = A.frm_first[c + 1];
    const uint32_t f0 = a < A.frm_cap ? a : A.frm_cap;
    const uint32_t f1 = b < f0 ? f0 : (b < A.frm_cap ? b : A.frm_cap);
    const uint32_t listed = A.nframes[c];
    const uint32_t n = listed < f1 - f0 ? listed : f1 - f0;
    const uint64_t r0 = A.rep_off[c], r1 = A.rep_off[c + 1];
    const uint64_t s0 = r0 < A.rep_size ? r0 : A.rep_size;
    const uint64_t s1 = r1 < s0 ? s0 : (r1 < A.rep_size ? r1 : A.rep_size);
    const uint32_t rep_cap = (uint32_t)(s1 - s0);
    uint8_t* rep = A.rep + s0;
    hhuff_h2_peer_t S = A.peers_in[c];
    h2c::Result R{0, 0, 0, 0};
    const hhuff_h2_ctl_t* ws = A.ws + f0;
    hhuff_h2_ctl_t next = n ? ws[0] : hhuff_h2_ctl_t{};
    for (uint32_t i = 0; i < n; ++i) {
        hhuff_h2_ctl_t r = next;
        const uint32_t j = i + 1u < n ? i + 1u : i;
        next = ws[j];
        const uint32_t kind = r.flags >> 5;
        r.flags &= 31u;
        if (r.status == HHUFF_H2C_EINVAL) {
            R.status = HHUFF_H2C_EINVAL;
            break;
        }
        hhuff_h2_peer_t T = S;
        h2c::Reply rp{0, 0, 0, 0, 0, 0};
        int32_t fail = 0;
        switch (kind) {
            case kFinal:
                if (r.status != 0) fail = r.status;
                else if (r.reply_len == 17) rp = h2c::Reply{17, h2c::kPing, h2c::kAck, 0, r.a, r.b};
                break;
            case kSettingsK: {
                const hhuff_h2_frame_t& f = A.frames[f0 + i];
                const h2c::Frame F{f.payload_off, f.length, f.stream_id, f.type, f.flags};
                h2c::Verdict v;
                fail = h2c::step(A.in + F.payload_off, F, A.P, T, v, rp);
                r = h2c::record_of(v, 0);
                break;
            }
            case kSendWin:
                if (h2c::window_update(T.send_window, r.a) != 0) fail = h2c::kFlowControl, r = hhuff_h2_ctl_t{0, 0, fail, HHUFF_H2C_ERR_FLOW_CONTROL, 0, 0};
                break;
            case kDataWin: {
                const uint32_t length = r.b + r.err;
                r.err = 0;
                if (A.P.recv_window_size != 0 && (A.P.flags & HHUFF_H2C_CLIENT) == 0) {
                    T.recv_window -= (int64_t)length;
                    if (T.recv_window <= (int64_t)(A.P.recv_window_size / 2u)) {
                        rp = h2c::Reply{13, h2c::kWindowUpdate, 0, 0, (uint32_t)(uint64_t)((int64_t)A.P.recv_window_size - T.recv_window), 0};
                        T.recv_window = A.P.recv_window_size;
                        r.flags |= HHUFF_H2R_WINDOW_UPDATE;
                    }
                }
                break;
            }
            case kGoawayK: T.flags |= HHUFF_H2P_GOAWAY; break;
            default: rp = h2c::Reply{13, h2c::kRstStream, 0, r.a, 1u, 0}, r.a = 0; break;
        }
        if (fail != 0) {
            S = T;
            r.reply_len = 0;
            A.ctl[f0 + i] = r;
            R.status = fail, R.err = r.err;
            break;
        }
        if (rp.len > rep_cap - R.rep_len) {
            R.status = HHUFF_H2C_SPACE;
            break;
        }
        S = T;
        h2c::emit(rep + R.rep_len, rp);
        R.rep_len += rp.len;
        r.reply_len = (uint8_t)rp.len;
        A.ctl[f0 + i] = r;
        ++R.nctl;
    }
    A.peers_out[c] = S;
    A.nctl[c] = R.nctl, A.cstatus[c] = R.status, A.cerr[c] = R.err, A.rep_len[c] = R.rep_len;
}

__global__ __launch_bounds__(256) void set_peers_kernel(const hhuff_h2_peer_t* __restrict__ peers, hhuff_hpack_response_t* res,
                                                        const uint32_t* __restrict__ conn_first, uint32_t nconn, uint32_t nres) {
    const uint64_t r64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r64 >= nres) return;
    const uint32_t r = (uint32_t)r64;
    if (conn_first[0] > r || conn_first[nconn] <= r) return;
    uint32_t lo = 0, hi = nconn;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (conn_first[mid] <= r) lo = mid; else hi = mid;
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
    hipStream_t s = (hipStream_t)stream;
    void* ws = nullptr;
    if (hhuff::work_alloc(&ws, (uint64_t)frm_cap * 16u + 16u, s) != hipSuccess) return HHUFF_EHIP;
    A.ws = (hhuff_h2_ctl_t*)ws;
    if (frm_cap)
        hipLaunchKernelGGL(hhuff::h2c_verdict_kernel, dim3((uint32_t)(((uint64_t)frm_cap + 255u) / 256u)), dim3(256), 0, s, A);
    hipLaunchKernelGGL(hhuff::h2c_order_kernel, dim3((uint32_t)(((uint64_t)nconn + 255u) / 256u)), dim3(256), 0, s, A);
    const hipError_t e = hipGetLastError();
    const hipError_t f = hipFreeAsync(ws, s);
    return e == hipSuccess && f == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}

HHUFF_API int hhuff_hpack_responses_set_peers(const hhuff_h2_peer_t* peers, hhuff_hpack_response_t* res, const uint32_t* conn_first,
                                              uint32_t nconn, uint32_t nres, void* stream) {
    if (!peers || !res || !conn_first) return HHUFF_EINVAL;
    if (nconn == 0 || nres == 0) return HHUFF_OK;
    hipLaunchKernelGGL(hhuff::set_peers_kernel, dim3((uint32_t)(((uint64_t)nres + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream,
                       peers, res, conn_first, nconn, nres);
    return hipGetLastError() == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}
