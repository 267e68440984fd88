// HTTP/2 DATA frames on the send side (include/hhuff.h (2k'')): h2o_http2_stream_send_pending_data, send_data,
// calc_max_payload_size and commit_data_header (lib/http2/stream.c:107-184, 410-436) and
// h2o_http2_conn_get_buffer_window (include/h2o/http2_internal.h:298-319) as a closed form per record.  The device
// kernel (hhuff_h2data.hip) and the host program (tools/h2data_host.cpp) run this very code.
//   stop_of     the three tests in front of a frame, in h2o's order: which of them stops the visit
//   record      one record: every frame of it is m bytes except the last, and once a frame is short whatever cut it is
//               at 0 for the next, so the frames are `full` of m bytes and at most one of `tail` -- no loop over frames.
//               Any m >= 1, all quantities int64: it can be checked exhaustively at tiny sizes.
//   header      the 9 bytes of h2o_http2_encode_frame_header for a DATA frame
//   walk        one connection: the peer and record checks of the call, the records in order, the connection
//               window and the room carried from one to the next
#ifndef HHUFF_H2DATA_H
#define HHUFF_H2DATA_H
#include <stdint.h>

#include "hhuff.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HHUFF_DATA_HD __host__ __device__ __forceinline__
#else
#define HHUFF_DATA_HD inline
#endif

namespace hhuff {
namespace h2d {

constexpr int64_t kHeaderSize = 9;  // H2O_HTTP2_FRAME_HEADER_SIZE
constexpr uint32_t kEndStream = 1;  // H2O_HTTP2_FRAME_FLAG_END_STREAM

HHUFF_DATA_HD int64_t min2(int64_t a, int64_t b) { return a < b ? a : b; }

// send_pending_data's own test, then get_buffer_window's and calc_max_payload_size's: 0 when a frame can be cut
HHUFF_DATA_HD uint32_t stop_of(int64_t R, int64_t Wc, int64_t Ws) {
    if (Ws <= 0) return HHUFF_H2T_STREAM_WINDOW;
    if (R < kHeaderSize || R - kHeaderSize <= 0) return HHUFF_H2T_ROOM;
    if (Wc <= 0) return HHUFF_H2T_CONN_WINDOW;
    return 0;
}

struct Frames {
    int64_t full;    // frames of m bytes
    int64_t tail;    // the bytes of the one frame behind them (0: no such frame, unless `empty`)
    bool empty;      // the frame of 0 bytes with END_STREAM of an empty FINAL body
    uint32_t flags;  // HHUFF_H2T_*
    HHUFF_DATA_HD int64_t count() const { return full + ((tail > 0 || empty) ? 1 : 0); }
    HHUFF_DATA_HD int64_t bytes(int64_t m) const { return full * m + tail; }
};

// One record of L bytes against the room R and the windows Wc, Ws: at most max_frames visits (0: no limit).
HHUFF_DATA_HD Frames record(int64_t m, int64_t R, int64_t Wc, int64_t Ws, int64_t L, bool final, bool trailers, int64_t max_frames) {
    Frames F{0, 0, false, 0};
    const bool end_stream = final && !trailers;
    if (L < 0) L = 0;
    F.flags = stop_of(R, Wc, Ws);
    if (F.flags != 0) return F;
    if (L == 0) {  // commit_data_header: length == 0 is written only for its END_STREAM
        F.empty = end_stream;
        F.flags = HHUFF_H2T_DONE | (end_stream ? HHUFF_H2T_END_STREAM : 0u);
        return F;
    }
    const int64_t cap = min2(Wc, Ws);
    const int64_t room = R - kHeaderSize - m >= 0 ? (R - kHeaderSize - m) / (m + kHeaderSize) + 1 : 0;
    F.full = min2(min2(L / m, cap / m), room);
    if (max_frames != 0 && F.full >= max_frames) {
        F.full = max_frames;
    } else {
        const int64_t rest = min2(min2(L, cap) - F.full * m, R - kHeaderSize - F.full * (m + kHeaderSize));
        if (rest > 0) F.tail = rest;
    }
    const int64_t n = F.bytes(m), k = F.count();
    if (n == L)
        F.flags = HHUFF_H2T_DONE | (end_stream ? HHUFF_H2T_END_STREAM : 0u);
    else if (max_frames != 0 && k >= max_frames)
        F.flags = HHUFF_H2T_MAX_FRAMES;
    else
        F.flags = stop_of(R - n - k * kHeaderSize, Wc - n, Ws - n);  // never 0: whatever cut the last frame is at 0 now
    return F;
}

// h2o_http2_encode_frame_header for type DATA: dst[0 .. 9)
HHUFF_DATA_HD void header(uint8_t* dst, uint32_t length, uint32_t flags, uint32_t stream_id) {
    dst[0] = (uint8_t)(length >> 16), dst[1] = (uint8_t)(length >> 8), dst[2] = (uint8_t)length, dst[3] = 0, dst[4] = (uint8_t)flags;
    dst[5] = (uint8_t)(stream_id >> 24), dst[6] = (uint8_t)(stream_id >> 16), dst[7] = (uint8_t)(stream_id >> 8);
    dst[8] = (uint8_t)stream_id;
}

// What the copy needs of a record with frames: `total` payload bytes from body[src ..) in frames of m (the last one
// shorter, or of 0 bytes when total == 0), the first header at out[dst].
struct Job {
    uint32_t src, dst, total, m;
    uint32_t stream_id, nframes, end_stream, rsv;
    HHUFF_DATA_HD uint64_t out_bytes() const { return (uint64_t)total + (uint64_t)kHeaderSize * nframes; }
};

// The copy, one 16-byte line of the destination (cut by address) at a time.  A line's first byte is byte fo of frame
// f, the 9 header bytes counted (below 0 in a job's first line, which begins in front of the job).
struct At {
    uint32_t f;
    int64_t fo;
};
HHUFF_DATA_HD At locate(const Job& J, int64_t o) {  // o: the line's first byte, counted from the job's first
    const uint32_t fw = J.m + (uint32_t)kHeaderSize;
    const uint32_t f = o < 0 ? 0u : (uint32_t)o / fw;  // (o < 2^32: a job lies inside `out`)
    return At{f, o - (int64_t)f * fw};
}
HHUFF_DATA_HD void advance(const Job& J, At& at, uint64_t bytes) {  // to a later line of the same job, without a division
    const int64_t fw = (int64_t)J.m + kHeaderSize;
    at.fo += (int64_t)bytes;
    while (at.fo >= fw) at.fo -= fw, ++at.f;
}

HHUFF_DATA_HD uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t bits) {  // bits 0, 8, 16, 24
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, bits);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> bits);
#endif
}

// The line's 16 bytes from the aligned source dwords that hold them (frm_gather_kernel's scheme): sv = where byte 0 of
// the line comes from, dword q = the line's bytes 4 q - r .. 4 q - r + 3, loaded only when one of them lies in [lo, hi).
HHUFF_DATA_HD void load16(uint64_t sv, int lo, int hi, uint32_t v[4]) {
    const uint32_t r = (uint32_t)(sv & 3u);
    const uint32_t* a = reinterpret_cast<const uint32_t*>((uintptr_t)(sv - r));
    uint32_t w[5];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = 0; q < 5; ++q) {
        const int first = 4 * q - (int)r;
        w[q] = (first < hi && first + 4 > lo) ? a[q] : 0u;
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = 0; q < 4; ++q) v[q] = funnel(w[q + 1], w[q], 8u * r);
}

HHUFF_DATA_HD void store16(uint8_t* d, const uint32_t v[4]) {  // d: 16-byte aligned
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint4*>(d) = make_uint4(v[0], v[1], v[2], v[3]);
#else
    uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
    d4[0] = v[0], d4[1] = v[1], d4[2] = v[2], d4[3] = v[3];
#endif
}

// byte x (0 .. 8) of a DATA frame's header, as header() writes it
HHUFF_DATA_HD uint32_t header_byte(uint32_t length, uint32_t flags, uint32_t stream_id, int x) {
    const uint32_t h0 = ((length >> 16) & 0xffu) | (length & 0xff00u) | ((length & 0xffu) << 16);  // length, type 0
    const uint32_t h1 = flags | ((stream_id >> 24) << 8) | (((stream_id >> 16) & 0xffu) << 16) | (((stream_id >> 8) & 0xffu) << 24);
    const uint32_t h = x < 4 ? h0 : (x < 8 ? h1 : (stream_id & 0xffu));
    return (h >> (8 * (x & 3))) & 0xffu;
}

// The line at address `line` of the job whose bytes lie at [d0, d1) (addresses; body: the address of body[0]): the
// job's bytes of it, and no other.  A line inside one frame's payload is one 16-byte store.  Else line byte i is byte
// x = fo + i of frame f: its header below 9, its payload below m + 9, then frame f + 1's header and payload, whose
// source lies 9 bytes back (m + 9 > 16 + 9: no third frame in a line).
HHUFF_DATA_HD void write_line(uint64_t body, const Job& J, uint64_t d0, uint64_t d1, uint64_t line, const At& at) {
    const int64_t fw = (int64_t)J.m + kHeaderSize, fo = at.fo;
    const uint32_t f = at.f;
    const uint64_t lo = line > d0 ? line : d0, hi = line + 16u < d1 ? line + 16u : d1;
    const int b0 = (int)(lo - line), b1 = (int)(hi - line);  // the job's bytes of the line
    // where byte 0 of the line would come from, were it payload of frame f
    const uint64_t sv = body + J.src + (uint64_t)f * J.m + (uint64_t)(fo - kHeaderSize);
    uint8_t* d = reinterpret_cast<uint8_t*>((uintptr_t)line);
    uint32_t v[4];
    if (b1 - b0 == 16 && fo >= kHeaderSize && fo + 16 <= fw) {
        load16(sv, 0, 16, v);
        store16(d, v);
        return;
    }
    const int64_t far = 64;  // (anything beyond the line)
    const int h1 = (int)(fw - fo < far ? fw - fo : far);  // where frame f + 1 begins in the line
    const int a0 = (int)(kHeaderSize - fo < far ? kHeaderSize - fo : far);
    const int alo = b0 > a0 ? b0 : a0, ahi = b1 < h1 ? b1 : h1;
    const int blo = b0 > h1 + 9 ? b0 : h1 + 9;
    uint32_t va[4], vb[4];
    load16(sv, alo, ahi, va);
    load16(sv - (uint64_t)kHeaderSize, blo, b1, vb);
    const uint32_t lastf = J.nframes - 1u, short_len = J.total - lastf * J.m;
    const uint32_t len0 = f < lastf ? J.m : short_len, len1 = f + 1u < lastf ? J.m : short_len;
    const uint32_t fl0 = (f == lastf && J.end_stream) ? kEndStream : 0u, fl1 = (f + 1u == lastf && J.end_stream) ? kEndStream : 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = 0; q < 4; ++q) {
        uint32_t word = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 4; ++i) {
            const int p = 4 * q + i;
            const int64_t x = fo + p;
            uint32_t byte;
            if (x < kHeaderSize)
                byte = header_byte(len0, fl0, J.stream_id, x < 0 ? 0 : (int)x);
            else if (p < h1)
                byte = (va[q] >> (8 * i)) & 0xffu;
            else if (p < h1 + 9)
                byte = header_byte(len1, fl1, J.stream_id, p - h1);
            else
                byte = (vb[q] >> (8 * i)) & 0xffu;
            word |= byte << (8 * i);
        }
        v[q] = word;
    }
    if (b1 - b0 == 16) {
        store16(d, v);
        return;
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = 0; q < 4; ++q) {  // whole dwords where the job has them, else bytes: the neighbours' bytes are theirs
        if (b0 <= 4 * q && 4 * q + 4 <= b1) {
            reinterpret_cast<uint32_t*>(d)[q] = v[q];
        } else {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int i = 0; i < 4; ++i)
                if (4 * q + i >= b0 && 4 * q + i < b1) d[4 * q + i] = (uint8_t)(v[q] >> (8 * i));
        }
    }
}

HHUFF_DATA_HD bool peer_ok(const hhuff_h2_peer_t& P) { return P.max_frame_size >= 16384u && P.max_frame_size <= 16777215u; }
HHUFF_DATA_HD bool send_ok(const hhuff_h2_send_t& S, uint64_t body_size) {
    return (uint64_t)S.body_off + S.body_len <= body_size && S.stream_id != 0 && S.stream_id <= 0x7fffffffu &&
           (S.flags & ~(HHUFF_H2S_FINAL | HHUFF_H2S_TRAILERS)) == 0;
}

struct Result {
    uint32_t out_len;
    int32_t status;
    int64_t send_window;
};

// One connection: its n records, its peer record P, its region out[start .. start + room).  sink.record(i, sent, job)
// receives record i's result and, when it has frames (sent.nframes != 0), its copy job.  m: the frame size in use --
// the peer's, checked -- so that the host program can run the walk at tiny sizes too.
template <class Sink>
HHUFF_DATA_HD void walk(uint64_t body_size, const hhuff_h2_send_t* sends, uint32_t n, int64_t m, bool m_ok, int64_t send_window,
                       uint32_t start, uint32_t room, Sink& sink, Result& res) {
    int64_t R = room, Wc = send_window;
    res = Result{0, 0, send_window};
    if (!m_ok) {
        res.status = HHUFF_H2D_EINVAL;
        return;
    }
    for (uint32_t i = 0; i < n; ++i) {
        const hhuff_h2_send_t S = sends[i];
        if (!send_ok(S, body_size)) {
            res.status = HHUFF_H2D_EINVAL;
            break;
        }
        const Frames F = record(m, R, Wc, S.window, S.body_len, (S.flags & HHUFF_H2S_FINAL) != 0, (S.flags & HHUFF_H2S_TRAILERS) != 0,
                                S.max_frames);
        const int64_t bytes = F.bytes(m), k = F.count();
        const uint32_t at = start + (uint32_t)((int64_t)room - R);
        const hhuff_h2_sent_t T{(uint32_t)bytes, (uint32_t)k, at, F.flags, (int32_t)((int64_t)S.window - bytes), 0u};
        const Job J{S.body_off, at, (uint32_t)bytes, (uint32_t)m, S.stream_id, (uint32_t)k, (F.flags & HHUFF_H2T_END_STREAM) ? 1u : 0u, 0u};
        sink.record(i, T, J);
        Wc -= bytes, R -= bytes + k * kHeaderSize;
    }
    res.out_len = (uint32_t)((int64_t)room - R), res.send_window = Wc;
}

}  // namespace h2d
}  // namespace hhuff
#endif
