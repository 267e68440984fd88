// HTTP/3 header encoders on the GPU (encode side): h2o_qpack_flatten_response / _request
// (lib/http3/qpack.c:1352-1399) for many responses, without an encoder-stream buffer (qpe_*: stateless per
// response) and with one (qse_*: an encoder per connection).  Both read the same static table through
// q_lookup_static, describe a field's representation by the same code word (kS*), take its length from
// q_field_len and write it with q_emit_field; a frame starts with q_sink_frame_head.  The HTTP/2 encoder is
// in hhuff_hpenc.hip, what both protocols use (and the long-string kernels' launches) in hhuff_enc.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "hhuff_enc.h"
#include "hhuff_image.h"
#include "hhuff_int.h"
#include "hhuff_qtable.h"
#include "hhuff_slots.h"

namespace hhuff {
namespace {
__device__ const uint8_t q_static_bytes[HHUFF_QSTATIC_NBYTES] = HHUFF_QSTATIC_BYTES_INIT;
__device__ const uint16_t q_static_ent[99 * 4] = HHUFF_QSTATIC_ENT_INIT;
__device__ const uint8_t __attribute__((aligned(16))) q_dfid_name[16] = {'d', 'a', 't', 'a', 'g', 'r', 'a', 'm',
                                                                         '-', 'f', 'l', 'o', 'w', '-', 'i', 'd'};

// A field's code word: the representation (bits 0-2), dont_compress (bit 3), the index (bits 4-20).  The
// stateless encoder uses the first three representations and marks a string past in_size in bit 30.
constexpr uint32_t kSStatic = 0, kSStaticRef = 1, kSLiteral = 2, kSDyn = 3, kSDynPost = 4, kSDynRef = 5, kSDynRefPost = 6;
constexpr uint32_t kSDc = 1u << 3, kSIdxShift = 4;
constexpr uint32_t kSBadStr = 1u << 30;

// flatten_string (qpack.c:1042-1066): its length with prefix p, Huffman when not dont_compress and shorter
__device__ __forceinline__ uint32_t q_str_len(uint32_t len, uint32_t bits, uint32_t p, bool dc) {
    if (!dc && huff_wins(len, bits)) {
        const uint32_t hb = (bits + 7u) >> 3;
        return int_len(hb, p) + hb;
    }
    return int_len(len, p) + len;
}

__device__ __forceinline__ uint32_t code_bits(const uint8_t* p, uint32_t len) {
    uint32_t bits = 0;
    for (uint32_t k = 0; k < len; ++k) bits += g_enc_nbits[p[k]];
    return bits;
}

// h2o_qpack_lookup_static[token] (flatten_header :1219-1224; lib/common/token_table.h): the static entry with
// the name and the value (`exact`), else the first with the name, else -1
__device__ __forceinline__ int32_t q_lookup_static(const uint8_t* n, uint32_t nl, const uint8_t* v, uint32_t vl, bool& exact) {
    int32_t sidx = -1;
    exact = false;
    for (uint32_t k = 0; k < 99 && !exact; ++k) {
        if (q_static_ent[4 * k + 1] != nl || !bytes_eq(q_static_bytes + q_static_ent[4 * k], n, nl)) continue;
        if (sidx < 0) sidx = (int32_t)k;
        if (q_static_ent[4 * k + 3] == vl && bytes_eq(q_static_bytes + q_static_ent[4 * k + 2], v, vl)) {
            sidx = (int32_t)k;
            exact = true;
        }
    }
    return sidx;
}

// do_flatten_header (:1148-1213): the length of a field that does not refer to the dynamic table
__device__ __forceinline__ uint32_t q_field_len(uint32_t code, uint32_t nl, uint32_t vl, uint32_t nbits, uint32_t vbits) {
    const uint32_t kind = code & 7u, idx = (code >> kSIdxShift) & 0x1FFFFu;
    const bool dc = (code & kSDc) != 0;
    if (kind == kSStatic) return int_len(idx, 6);                                     // flatten_static_indexed
    if (kind == kSStaticRef) return int_len(idx, 4) + q_str_len(vl, vbits, 7, dc);    // flatten_static_nameref
    return q_str_len(nl, nbits, 3, false) + q_str_len(vl, vbits, 7, dc);             // flatten_without_nameref
}

// flatten_string on a RegSink: `first` holds the bits above the H bit
__device__ __forceinline__ void q_sink_string(RegSink& sink, const GlobalSource& src, uint32_t first, uint32_t s, uint32_t len,
                                              uint32_t bits, uint32_t p, bool dc, const uint2* enc, const LongWork& L) {
    const bool huff = !dc && huff_wins(len, bits);
    const uint32_t hb = (bits + 7u) >> 3;
    if (huff)
        sink_int(sink, (first & ~((1u << p) - 1u)) | (1u << p), hb, p);
    else
        sink_int(sink, first & ~((2u << p) - 1u), len, p);
    sink_payload(sink, src, s, len, huff, hb, enc, L);
}

// the representation's first part; true when the value string follows it (the literal name is the caller's)
__device__ __forceinline__ bool q_emit_ref(RegSink& sink, uint32_t code) {
    const uint32_t idx = (code >> kSIdxShift) & 0x1FFFFu;
    const bool dc = (code & kSDc) != 0;
    switch (code & 7u) {
        case kSStatic: sink_int(sink, 0xc0u, idx, 6); return false;
        case kSDyn: sink_int(sink, 0x80u, idx, 6); return false;
        case kSDynPost: sink_int(sink, 0x10u, idx, 4); return false;
        case kSStaticRef: sink_int(sink, 0x50u | (dc ? 0x20u : 0u), idx, 4); return true;
        case kSDynRef: sink_int(sink, 0x40u | (dc ? 0x20u : 0u), idx, 4); return true;
        case kSDynRefPost: sink_int(sink, dc ? 0x08u : 0u, idx, 3); return true;
        default: return true;
    }
}

__device__ __forceinline__ void q_emit_field(RegSink& sink, const GlobalSource& nsrc, const GlobalSource& vsrc, uint32_t code,
                                             uint32_t noff, uint32_t nl, uint32_t voff, uint32_t vl, uint32_t nbits,
                                             uint32_t vbits, const uint2* enc, const LongWork& L) {
    const bool dc = (code & kSDc) != 0;
    if ((code & 7u) == kSLiteral)
        q_sink_string(sink, nsrc, 0x20u | (dc ? 0x10u : 0u), noff, nl, nbits, 3, false, enc, L);
    else if (!q_emit_ref(sink, code))
        return;
    q_sink_string(sink, vsrc, 0u, voff, vl, vbits, 7, dc, enc, L);
}

__device__ __forceinline__ uint32_t q_status_index(uint32_t s) {  // INDEXED_STATUS (:1362-1377)
    switch (s) {
        case 103: return 24;
        case 200: return 25;
        case 304: return 26;
        case 404: return 27;
        case 503: return 28;
        case 100: return 63;
        case 204: return 64;
        case 206: return 65;
        case 302: return 66;
        case 400: return 67;
        case 403: return 68;
        case 421: return 69;
        case 425: return 70;
        case 500: return 71;
        default: return 0;
    }
}

__device__ const uint64_t q_pow10[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull,
                                         100000000ull, 1000000000ull, 10000000000ull, 100000000000ull, 1000000000000ull,
                                         10000000000000ull, 100000000000000ull, 1000000000000000ull,
                                         10000000000000000ull, 100000000000000000ull, 1000000000000000000ull,
                                         10000000000000000000ull};
// digit k (most significant first) of the n-digit decimal v
__device__ __forceinline__ uint32_t q_digit(uint64_t v, uint32_t n, uint32_t k) {
    return '0' + (uint32_t)((v / q_pow10[n - 1 - k]) % 10u);
}
// the number of decimal digits of v ("%u" / "%zu")
__device__ __forceinline__ uint32_t q_ndigits(uint64_t v) {
    uint32_t n = 1;
    while (n < 20 && v >= q_pow10[n]) ++n;
    return n;
}
// the decimal digits of v: their count, and their code bits in `bits`
__device__ __forceinline__ uint32_t q_digits(uint64_t v, uint32_t& bits) {
    const uint32_t n = q_ndigits(v);
    bits = 0;
    for (uint32_t k = 0; k < n; ++k) bits += g_enc_nbits[q_digit(v, n, k)];
    return n;
}

// a field whose value is the decimal of v (status / content-length): static name reference `idx`
__device__ __forceinline__ uint32_t q_local_len(uint32_t idx, uint32_t n, uint32_t bits) {
    return int_len(idx, 4) + q_str_len(n, bits, 7, false);
}
// flatten_string (prefix 7) of the decimal of v
__device__ __forceinline__ void q_sink_decimal(RegSink& sink, uint64_t v, const uint2* enc) {
    uint32_t bits;
    const uint32_t n = q_digits(v, bits);
    if (huff_wins(n, bits)) {
        sink_int(sink, 0x80u, (bits + 7u) >> 3, 7);
        uint64_t acc = 0;  // <= 20 digits x 6 bits: flushed a byte at a time
        uint32_t an = 0;
        for (uint32_t k = 0; k < n; ++k) {
            const uint2 e = enc[q_digit(v, n, k)];
            acc = acc << e.y | e.x;
            an += e.y;
            while (an >= 8) {
                an -= 8;
                sink.put1((uint32_t)(acc >> an) & 0xFFu);
            }
        }
        if (an) sink.put1((uint32_t)((acc << (8 - an)) | (0xFFu >> an)) & 0xFFu);  // EOS prefix padding (hpack.c:795-798)
    } else {
        sink_int(sink, 0u, n, 7);
        for (uint32_t k = 0; k < n; ++k) sink.put1(q_digit(v, n, k));
    }
}
__device__ __forceinline__ void q_emit_local(RegSink& sink, uint32_t idx, uint64_t v, const uint2* enc) {
    sink_int(sink, 0x50u, idx, 4);
    q_sink_decimal(sink, v, enc);
}

__device__ __forceinline__ uint32_t q_varint_len(uint64_t v) { return v <= 63 ? 1u : v <= 16383 ? 2u : v <= 1073741823 ? 4u : 8u; }

// a HEADERS frame's head: H2O_HTTP3_FRAME_TYPE_HEADERS, then the section length as a QUIC varint
// (finalize_flatten :1303-1307)
__device__ __forceinline__ void q_sink_frame_head(RegSink& sink, uint32_t section_len) {
    sink.put1(0x01u);
    const uint32_t vl = q_varint_len(section_len);
    const uint32_t tag = vl == 1 ? 0x00u : vl == 2 ? 0x40u : vl == 4 ? 0x80u : 0xC0u;
    for (uint32_t k = 0; k < vl; ++k) {
        const uint32_t b = k + 4 < vl ? 0u : (section_len >> (8 * (vl - 1 - k))) & 0xFFu;
        sink.put1(k == 0 ? (b | tag) : b);
    }
}
}  // namespace

// ---------------------------------------------------------------------------------------------------
// Without an encoder-stream buffer, as h2o's HTTP/3 server calls it (lib/http3/server.c:1680-1683): the
// encoder's dynamic table stays empty (do_flatten_header inserts only with one, :1175-1176), so a field is a
// static reference or a literal and a response depends on nothing but itself -- no sequential walk:
//   qpe_size_kernel (one lane per header): the static lookup for token names, the representation and the
//     code bits of its literals (long ones: long_bits_kernel).  No hashes, and code bits only of strings that
//     can end up Huffman-coded: it is cheaper than the sessions' prep;
//   qpe_layout_kernel (one lane per response): the fields' byte lengths (flatten_string's Huffman verdict
//     from the code bits), status, server, content-length and datagram-flow-id fields, the field positions,
//     the section length and the frame header's varint;
//   qpe_emit_kernel (one lane per field and per response head): the bytes, in place (long payloads:
//     long_payload_kernel).
// ---------------------------------------------------------------------------------------------------
struct QpeArgs : QpeCall {  // the call (the kernels read its members as their own) and its workspace
    uint4* rec;   // [nhdr + 1] {0, code, name code bits, value code bits}; item nhdr: the server name
    uint2* dst;   // [nhdr] the field's output offset (lo, hi); hi = ~0 when its response failed
    uint4* plan;  // [2 nres] {base lo, base hi, section length, frame total} {status size, server size, cl size, dfid size}
    LongWork lw;
};

__global__ __launch_bounds__(256) void qpe_size_kernel(QpeArgs A) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i <= A.nhdr; i += (uint64_t)gridDim.x * 256u) {
        if (i < A.nhdr) A.dst[i] = make_uint2(0u, ~0u);  // a header no response lists writes nothing
        if (i == A.nhdr) {  // the server name: static name reference 92 (:1387-1389)
            const bool bad = (uint64_t)A.server_off + A.server_len > A.in_size;
            uint32_t vb = 0;
            if (!bad && A.server_len > kLongStr)
                push_long_bits(A.lw, (uint32_t)i, 1);
            else if (!bad)
                vb = code_bits(A.in + A.server_off, A.server_len);
            A.rec[i] = make_uint4(0u, kSStaticRef | (92u << kSIdxShift) | (bad ? kSBadStr : 0u), 0u, vb);
            continue;
        }
        const hhuff_hpack_header_t H = A.hdr[i];
        if ((uint64_t)H.name_off + H.name_len > A.in_size || (uint64_t)H.value_off + H.value_len > A.in_size) {
            A.rec[i] = make_uint4(0u, kSBadStr, 0u, 0u);
            continue;
        }
        const uint8_t* n = A.in + H.name_off;
        const uint8_t* v = A.in + H.value_off;
        int32_t sidx = -1;
        bool exact = false;
        if (H.flags & HHUFF_HDR_TOKEN) sidx = q_lookup_static(n, H.name_len, v, H.value_len, exact);
        const bool dc = (H.flags & HHUFF_HDR_DONT_COMPRESS) != 0;
        const uint32_t code =
            (sidx >= 0 ? (exact ? kSStatic : kSStaticRef) | ((uint32_t)sidx << kSIdxShift) : kSLiteral) | (dc ? kSDc : 0u);
        uint32_t nb = 0, vb = 0;
        if (sidx < 0) {  // the name is a literal
            if (H.name_len > kLongStr)
                push_long_bits(A.lw, (uint32_t)i, 0);
            else
                nb = code_bits(n, H.name_len);
        }
        if (!(sidx >= 0 && exact) && !dc) {  // the value may be Huffman-coded
            if (H.value_len > kLongStr)
                push_long_bits(A.lw, (uint32_t)i, 1);
            else
                vb = code_bits(v, H.value_len);
        }
        A.rec[i] = make_uint4(0u, code, nb, vb);
    }
}

__global__ __launch_bounds__(256) void qpe_layout_kernel(QpeArgs A) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < A.nres; r += (uint64_t)gridDim.x * 256u) {
        const hhuff_qpack_response_t R = A.res[r];
        const bool request = (R.flags & HHUFF_QRES_REQUEST) != 0;  // h2o_qpack_flatten_request: its own fields are
        const bool server = !request && (R.flags & HHUFF_RES_SERVER) && A.server_len != 0;  // headers of the list
        const bool dfid = (R.flags & HHUFF_QRES_DATAGRAM) != 0;
        const uint4 sr = A.rec[A.nhdr];
        // a header range past the call's headers or a region that ends before it starts: EINVAL
        const bool malformed = (uint64_t)R.hdr_first + R.nhdr > A.nhdr || A.out_off[r + 1] < A.out_off[r];
        bool bad = malformed || (server && (sr.y & kSBadStr)) || (dfid && (uint64_t)R.dfid_off + R.dfid_len > A.in_size);
        uint32_t bits;
        const uint32_t si = request ? 0u : q_status_index(R.status);
        uint32_t st_len = si ? int_len(si, 6) : 0u;
        if (!si && !request) {
            const uint32_t n = q_digits((uint16_t)R.status, bits);
            st_len = q_local_len(24, n, bits);
        }
        const uint32_t sv_len = server ? q_field_len(sr.y & ~kSBadStr, 0, A.server_len, 0, sr.w) : 0u;
        uint32_t cl_len = 0;
        if (!request && R.content_length != ~0ull) {
            if (R.content_length == 0) {
                cl_len = 1;
            } else {
                const uint32_t n = q_digits(R.content_length, bits);
                cl_len = q_local_len(4, n, bits);
            }
        }
        uint32_t df_len = 0;
        if (dfid && !bad)
            df_len = q_field_len(kSLiteral, 16, R.dfid_len, code_bits(q_dfid_name, 16), code_bits(A.in + R.dfid_off, R.dfid_len));
        const uint32_t h0 = R.hdr_first, h1 = R.hdr_first + R.nhdr;
        uint64_t body = 2u + st_len + sv_len + cl_len;  // after the section prefix 00 00
        for (uint32_t h = h0; h < h1 && !bad; ++h) {
            const uint4 rc = A.rec[h];
            if (rc.y & kSBadStr) {
                bad = true;
                break;
            }
            const hhuff_hpack_header_t H = A.hdr[h];
            body += q_field_len(rc.y, H.name_len, H.value_len, rc.z, rc.w);
        }
        body += df_len;
        const uint64_t base = A.out_off[r];
        int32_t st = bad ? HHUFF_RES_EINVAL : 0;
        const uint64_t total = 1u + q_varint_len(body) + body;
        if (st == 0 && (total > A.out_off[r + 1] - base || body > 0xFFFFFFFFull)) st = HHUFF_RES_SPACE;
        if (st == 0) {
            uint64_t o = base + 1u + q_varint_len(body) + 2u + st_len + sv_len + cl_len;
            for (uint32_t h = h0; h < h1; ++h) {
                A.dst[h] = make_uint2((uint32_t)o, (uint32_t)(o >> 32));
                const uint4 rc = A.rec[h];
                const hhuff_hpack_header_t H = A.hdr[h];
                o += q_field_len(rc.y, H.name_len, H.value_len, rc.z, rc.w);
            }
            A.plan[2 * r] = make_uint4((uint32_t)base, (uint32_t)(base >> 32), (uint32_t)body, (uint32_t)total);
            A.plan[2 * r + 1] = make_uint4(st_len, sv_len, cl_len, df_len);
            A.out_len[r] = (uint32_t)total;
            A.header_len[r] = (uint32_t)body;
        } else {
            for (uint32_t h = h0; h < h1 && !malformed; ++h) A.dst[h] = make_uint2(0u, ~0u);
            A.plan[2 * r] = make_uint4(0u, 0u, 0u, 0u);
            A.out_len[r] = 0;
            A.header_len[r] = 0;
        }
        A.rstatus[r] = st;
    }
}

__global__ __launch_bounds__(256) void qpe_emit_kernel(QpeArgs A) {
    __shared__ uint2 s_enc[256];
    s_enc[threadIdx.x] = make_uint2(g_enc_code[threadIdx.x], g_enc_nbits[threadIdx.x]);
    __syncthreads();
    const GlobalSource src{A.in, A.in_size};
    const uint64_t items = (uint64_t)A.nhdr + A.nres;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < items; i += (uint64_t)gridDim.x * 256u) {
        if (i < A.nhdr) {
            const uint2 o = A.dst[i];
            if (o.y == ~0u) continue;
            const hhuff_hpack_header_t H = A.hdr[i];
            const uint4 rc = A.rec[i];
            __builtin_assume((rc.y & 7u) <= kSLiteral);  // qpe_size_kernel writes no dynamic representation
            RegSink sink;
            sink.init(A.out + ((uint64_t)o.y << 32 | o.x));
            q_emit_field(sink, src, src, rc.y, H.name_off, H.name_len, H.value_off, H.value_len, rc.z, rc.w, s_enc, A.lw);
            sink.finish();
            continue;
        }
        const uint32_t r = (uint32_t)(i - A.nhdr);
        const uint4 p0 = A.plan[2 * r], p1 = A.plan[2 * r + 1];
        if (p0.w == 0) continue;
        const hhuff_qpack_response_t R = A.res[r];
        uint8_t* base = A.out + ((uint64_t)p0.y << 32 | p0.x);
        RegSink sink;
        sink.init(base);
        q_sink_frame_head(sink, p0.z);
        sink.put1(0u);  // Required Insert Count 0
        sink.put1(0u);  // Delta Base 0
        const uint32_t si = q_status_index(R.status);
        if (R.flags & HHUFF_QRES_REQUEST) {
        } else if (si) {
            sink_int(sink, 0xc0u, si, 6);
        } else {
            q_emit_local(sink, 24, (uint16_t)R.status, s_enc);
        }
        if (p1.y) {
            const uint4 sr = A.rec[A.nhdr];
            __builtin_assume((sr.y & 7u) == kSStaticRef);
            q_emit_field(sink, src, src, sr.y & ~kSBadStr, 0u, 0u, A.server_off, A.server_len, 0u, sr.w, s_enc, A.lw);
        }
        if (p1.z) {
            if (R.content_length == 0)
                sink_int(sink, 0xc0u, 4, 6);
            else
                q_emit_local(sink, 4, R.content_length, s_enc);
        }
        sink.finish();
        if (p1.w) {  // datagram-flow-id last (:1396-1398): a literal with its name (no static entry)
            RegSink s2;
            s2.init(base + p0.w - p1.w);
            const GlobalSource nsrc{q_dfid_name, 16};
            q_sink_string(s2, nsrc, 0x20u, 0u, 16u, code_bits(q_dfid_name, 16), 3, false, s_enc, A.lw);
            q_sink_string(s2, src, 0u, R.dfid_off, R.dfid_len, code_bits(A.in + R.dfid_off, R.dfid_len), 7, false, s_enc, A.lw);
            s2.finish();
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Encoder sessions: h2o_qpack_flatten_response / _request WITH an encoder-stream buffer
// (lib/http3/qpack.c:1148-1213, :1244-1310) and h2o_qpack_encoder_handle_input (:902-1005) for many
// connections, each with its encoder dynamic table, its list of unacknowledged sections and its view of
// what the peer has received, kept in scratch between calls (include/hhuff.h (2g')):
//   qse_prep_kernel (one lane per header): bounds, the static lookup, a hash and the code bits of the name
//     and of the value (long ones: long_bits_kernel);
//   qse_walk_kernel (one lane per connection): the decoder stream, then field after field the decision of
//     do_flatten_header against the table in scratch -- hashes first, bytes of the candidates only; it
//     yields each field's representation and place, each insert's instruction and place in the encoder
//     stream, each section's prefix.  It writes no output byte; an insert's strings are copied into the
//     connection's string area so that later calls compare against scratch alone (offsets, no addresses);
//   qse_emit_kernel (one lane per field, per insert, per response head and per connection): the bytes,
//     through RegSink / q_sink_string (long payloads: long_payload_kernel).
// ---------------------------------------------------------------------------------------------------
namespace {
__device__ const uint8_t __attribute__((aligned(16))) q_status_name[16] = {':', 's', 't', 'a', 't', 'u', 's'};
__device__ const uint8_t __attribute__((aligned(16))) q_cl_name[16] = {'c', 'o', 'n', 't', 'e', 'n', 't', '-',
                                                                       'l', 'e', 'n', 'g', 't', 'h'};

// info word of a prepped header: static index (bits 0-6)
constexpr uint32_t kSiStatic = 1u << 7, kSiExact = 1u << 8, kSiDc = 1u << 9, kSiLtr = 1u << 10, kSiBad = 1u << 11;
// encoder-stream instruction of an insert (bits 0-2; the name reference, or the duplicated entry's relative index,
// above)
constexpr uint32_t kInsNone = 0, kInsStatic = 1, kInsDynamic = 2, kInsLiteral = 3, kInsDup = 4;
constexpr uint32_t kInsMask = 7u, kInsShift = 3;

// Without HHUFF_QENC_EVICT: entries 1 .. count in slots 0 .. count - 1, evicted stays 0.  With it: the live
// entries evicted + 1 .. count in a ring (hhuff_qtable.h), bit 1 of `failed` marks the session as evicting, and
// an inflight record's last word is the section's smallest reference with `blocking` in bit 31.  With
// HHUFF_QENC_DUP as well, bit 2 of `failed` marks the session as duplicating.
struct QsState {
    uint32_t count, used;      // the inserts so far; the live entries' bytes with the 32 per entry
    uint32_t lkr;              // largest_known_received
    uint32_t num_blocked, ninflight, failed;
    uint32_t str_used, evicted;
};
struct QsInflight {
    uint64_t sid;
    uint32_t largest, blocking;
};
constexpr uint32_t kQsEvicting = 2u, kQsDuplicating = 4u;  // in QsState::failed
static_assert(sizeof(QsState) == 32 && sizeof(QsEntry) == 32 && sizeof(QsInflight) == 16, "scratch records");
// connection images (hhuff_image.h) restate the state and inflight records and the mode bits
static_assert(offsetof(QsState, lkr) == offsetof(img::QeState, lkr) && offsetof(QsState, ninflight) == offsetof(img::QeState, ninflight) &&
                  offsetof(QsState, failed) == offsetof(img::QeState, failed) && offsetof(QsState, evicted) == offsetof(img::QeState, evicted) &&
                  offsetof(QsInflight, largest) == offsetof(img::QeInflight, largest) && kQsEvicting == img::kQeEvicting &&
                  kQsDuplicating == img::kQeDuplicating,
              "hhuff_image.h: QPACK_ENC slab");

__host__ __device__ inline uint64_t qs_conn_scratch(uint32_t H, uint32_t M) {
    return sizeof(QsState) + (uint64_t)(H / 32u) * sizeof(QsEntry) + (uint64_t)M * sizeof(QsInflight) + ((H + 15ull) & ~15ull);
}
}  // namespace

struct QseArgs {
    QseCall c;
    // workspace
    uint4* rec;      // [nhdr + 1] {name hash, value hash, name code bits, value code bits}; item nhdr: server
    uint32_t* info;  // [nhdr + 1]
    uint4* op;       // [nhdr] {place among the section's fields, response, code, 0}
    uint4* ins;      // [nhdr] {place in enc_out lo, hi, instruction | name reference << 3, 0}
    uint4* plan;     // [4 nres] {base lo, base hi, section length, frame total} {Required Insert Count, delta base |
                     // sign << 31, first field's offset in the frame, datagram-flow-id size} {codes of :status, server,
                     // content-length, datagram-flow-id} {server's insert: place lo, hi, instruction, 0}
    uint4* cplan;    // [nconn] {enc_out region lo, hi, Set Dynamic Table Capacity first, the capacity it sets}
    LongWork lw;
};

namespace {
struct QsConn {
    QsState s;
    QsEntry* ent;
    QsInflight* inf;
    uint8_t* str;
    uint32_t cap;          // the table's capacity: the call's header_table_size, or the peer's clamped to it
    uint32_t scap;         // the string area's bytes: header_table_size whatever the capacity
    uint32_t slots, imin;  // evicting: the ring's size; the smallest reference of any inflight section
};
struct QsField {
    const uint8_t *n, *v;
    uint32_t nl, vl, nh, vh, nb, vb, info;
};
struct QsSection {
    uint32_t base, largest, pos, enc, mode;  // mode 2: with an encoder buffer, 1: without, 0: no encoder at all
    uint32_t smallest;                       // evicting: the smallest index referenced so far
};

// h2o_qpack_encoder_handle_input (qpack.c:963-1005): `consumed` = the bytes of the instructions taken
template <bool EV>
__device__ int32_t qs_handle_input(QsConn& t, const uint8_t* b, uint32_t n, uint32_t& consumed) {
    uint64_t p = 0;
    while (p < n) {
        const uint32_t kind = b[p] >> 6;
        // h2o_hpack_decode_int through decode_int (qpack.c:215-220)
        const int64_t r = hpack_int(b, p, n, kind >= 2 ? 7u : 6u);
        if (r == kIntIncomplete) return 0;  // the rest waits for more input
        if (r < 0) return HHUFF_QPK_DECOMPRESSION_FAILED;
        const uint64_t v = (uint64_t)r;
        consumed = (uint32_t)p;
        if (kind == 0) {  // Insert Count Increment (handle_table_state_synchronize :902-918)
            if (v == 0 || (uint64_t)t.s.lkr + v >= (uint64_t)t.s.count + 1u) return HHUFF_QPK_DECODER_STREAM;
            t.s.lkr += (uint32_t)v;
        } else if (kind == 1) {  // Stream Cancellation (:959-975): every entry of the stream
            uint32_t w = 0;
            for (uint32_t k = 0; k < t.s.ninflight; ++k) {
                const QsInflight e = t.inf[k];
                if (e.sid == v) {
                    t.s.num_blocked -= EV ? e.blocking >> 31 : e.blocking;
                } else {
                    if (w != k) t.inf[w] = e;
                    ++w;
                }
            }
            t.s.ninflight = w;
        } else {  // Section Acknowledgment (handle_header_ack :933-957): the first entry of the stream
            uint32_t k = 0;
            while (k < t.s.ninflight && t.inf[k].sid != v) ++k;
            if (k == t.s.ninflight) return HHUFF_QPK_DECODER_STREAM;
            const QsInflight e = t.inf[k];
            if (t.s.lkr < e.largest) t.s.lkr = e.largest;
            t.s.num_blocked -= EV ? e.blocking >> 31 : e.blocking;
            for (; k + 1 < t.s.ninflight; ++k) t.inf[k] = t.inf[k + 1];  // entry by entry (:928 moves bytes)
            --t.s.ninflight;
        }
    }
    return 0;
}

// lookup_dynamic (qpack.c:1007-1037): newest to oldest, the first exact match, else the newest name match
template <bool EV>
__device__ uint32_t qs_lookup(const QsConn& t, const QsField& F, bool acked_only, bool& exact) {
    uint32_t found = 0;
    exact = false;
    uint32_t i = EV ? qt_scan_top(t.s.count, t.s.lkr, acked_only) : acked_only ? t.s.lkr : t.s.count;
    const uint32_t low = EV ? t.s.evicted : 0u;
    uint32_t slot = EV && i > low ? qt_slot(i, t.slots) : 0u;
    for (; i > low; --i) {
        const QsEntry e = t.ent[EV ? slot : i - 1];
        if (EV) slot = qt_prev(slot, t.slots);
        if (e.nl != F.nl || e.nh != F.nh || !bytes_eq(t.str + e.noff, F.n, F.nl)) continue;
        if (e.vl == F.vl && e.vh == F.vh && bytes_eq(t.str + e.noff + e.nl, F.v, F.vl)) {
            exact = true;
            return i;
        }
        if (found == 0) found = i;
    }
    return found;
}

template <bool EV>
__device__ __forceinline__ uint32_t qs_dyn_indexed(QsSection& S, uint32_t i, uint32_t& len) {  // flatten_dynamic_indexed
    if (i > S.largest) S.largest = i;
    if (EV && i < S.smallest) S.smallest = i;
    if (i <= S.base) {
        len = int_len(S.base - i, 6);
        return kSDyn | (S.base - i) << kSIdxShift;
    }
    len = int_len(i - S.base - 1u, 4);
    return kSDynPost | (i - S.base - 1u) << kSIdxShift;
}

// do_flatten_header (qpack.c:1148-1213): the field's code and length; an insert's instruction and length.
// DUP (HHUFF_QENC_DUP, with EV only): an exact match on a draining entry is duplicated when the room test lets
// it -- the insert below with the matched entry no pin (the prefix that goes may hold it: the strings come from
// the field's bytes, never from the entry) and the Duplicate instruction in place of the insert's.
template <bool EV, bool DUP>
__device__ uint32_t qs_field(QsConn& t, QsSection& S, const QsField& F, uint32_t& len, uint32_t& ins, uint32_t& ins_len) {
    const bool has_s = (F.info & kSiStatic) != 0, dc = (F.info & kSiDc) != 0;
    const uint32_t sidx = F.info & 0x7Fu;
    ins = kInsNone;
    ins_len = 0;
    if (has_s && (F.info & kSiExact)) {
        const uint32_t code = kSStatic | sidx << kSIdxShift;
        len = q_field_len(code, F.nl, F.vl, F.nb, F.vb);
        return code;
    }
    bool dexact = false;
    const uint32_t dyn = S.mode ? qs_lookup<EV>(t, F, S.mode == 1, dexact) : 0u;
    bool dup = false;
    if (dyn && dexact) {
        if (DUP) dup = S.mode == 2 && (F.info & kSiLtr) && qt_draining(t.ent, t.slots, t.cap, t.s.used, t.s.evicted, dyn);
        if (!dup) return qs_dyn_indexed<EV>(S, dyn, len);
    }
    bool fits = dup || ((F.info & kSiLtr) && S.mode == 2 && ((!has_s && !dyn) || F.vl >= 8));
    uint32_t slot = t.s.count;
    if (!EV) {
        fits = fits && (uint64_t)F.nl + F.vl + 32u <= (uint64_t)(t.cap - t.s.used);
    } else if (fits) {  // the oldest entries below every pin make the room, or the field is not inserted
        uint32_t pin = min(t.imin, S.smallest), used = 0;
        if (!dup && !has_s && dyn && dyn < pin) pin = dyn;  // the entry the instruction names
        const uint32_t ev = qt_evict_prefix(t.ent, t.slots, t.cap, t.s.used, t.s.evicted, t.s.count, pin,
                                            (uint64_t)F.nl + F.vl + 32u, used);
        fits = ev != kQtNoInsert;
        if (fits) {
            t.s.evicted = ev;
            t.s.used = used;
            t.s.str_used = qt_place(t.str, t.scap, t.ent, t.slots, ev, t.s.count, t.s.str_used, F.nl + F.vl);
            slot = qt_slot(t.s.count + 1u, t.slots);
        }
    }
    if (fits) {
        if (dup) {  // Duplicate (RFC 9204 4.3.4): relative to the newest entry before this one, no strings
            ins = kInsDup | (t.s.count - dyn) << kInsShift;
            ins_len = int_len(t.s.count - dyn, 5);
        } else if (has_s) {
            ins = kInsStatic | sidx << kInsShift;
            ins_len = int_len(sidx, 6);
        } else if (dyn) {  // relative to the newest entry (RFC 9204 4.3.2), as the decoder reads it (:336-341)
            ins = kInsDynamic | (t.s.count - dyn) << kInsShift;
            ins_len = int_len(t.s.count - dyn, 6);
        } else {
            ins = kInsLiteral;
            ins_len = q_str_len(F.nl, F.nb, 5, false);
        }
        if (!dup) ins_len += q_str_len(F.vl, F.vb, 7, false);
        uint8_t* d = t.str + t.s.str_used;
        for (uint32_t k = 0; k < F.nl; ++k) d[k] = F.n[k];
        for (uint32_t k = 0; k < F.vl; ++k) d[F.nl + k] = F.v[k];
        t.ent[slot] = QsEntry{t.s.str_used, F.nl, F.vl, F.nh, F.vh, 0u, 0u, 0u};
        ++t.s.count;
        t.s.used += F.nl + F.vl + 32u;
        t.s.str_used += F.nl + F.vl;
        return qs_dyn_indexed<EV>(S, t.s.count, len);
    }
    if (dup) return qs_dyn_indexed<EV>(S, dyn, len);  // no room below the pins: the reference, as without the flag
    const uint32_t dcb = dc ? kSDc : 0u;
    if (has_s) {
        const uint32_t code = kSStaticRef | dcb | sidx << kSIdxShift;
        len = q_field_len(code, F.nl, F.vl, F.nb, F.vb);
        return code;
    }
    if (!dyn) {
        len = q_field_len(kSLiteral | dcb, F.nl, F.vl, F.nb, F.vb);
        return kSLiteral | dcb;
    }
    const uint32_t vlen = q_str_len(F.vl, F.vb, 7, dc);  // flatten_dynamic_nameref
    if (dyn > S.largest) S.largest = dyn;
    if (EV && dyn < S.smallest) S.smallest = dyn;
    if (dyn <= S.base) {
        len = int_len(S.base - dyn, 4) + vlen;
        return kSDynRef | dcb | (S.base - dyn) << kSIdxShift;
    }
    len = int_len(dyn - S.base - 1u, 3) + vlen;
    return kSDynRefPost | dcb | (dyn - S.base - 1u) << kSIdxShift;
}

__device__ __forceinline__ uint32_t qs_decimal(uint64_t v, uint8_t* d) {
    const uint32_t n = q_ndigits(v);
    for (uint32_t k = 0; k < n; ++k) d[k] = (uint8_t)q_digit(v, n, k);
    return n;
}

struct QsOwn {       // a response's own fields
    uint32_t code[4];  // :status, server, content-length, datagram-flow-id
    uint32_t sins, sins_at;  // server's insert and its place in the section's instructions
    uint32_t df_len;
    bool bad;
};
struct QsNames {
    uint32_t status, cl, dfid;  // name hashes
};

// One section: prepare_flatten and the fields of h2o_qpack_flatten_response / _request in their order.
// enc0 = the connection's encoder-stream bytes before this section.
template <bool EV, bool DUP>
__device__ void qs_walk_section(const QseArgs& A, QsConn& t, const hhuff_qpack_response_t& R, uint32_t r, uint32_t mode,
                                uint64_t enc0, const QsNames& N, QsSection& S, QsOwn& O) {
    const QseCall& C = A.c;
    S = QsSection{t.s.count, 0u, 0u, 0u, mode, ~0u};
    O = QsOwn{{kOpSkip, kOpSkip, kOpSkip, kOpSkip}, kInsNone, 0u, 0u, false};
    const bool request = (R.flags & HHUFF_QRES_REQUEST) != 0;
    uint32_t len, ins, ins_len;
    uint8_t dg[20];
    if (!request) {
        const uint32_t si = q_status_index(R.status);
        QsField F{q_status_name, dg, 7u, 0u, N.status, 0u, 0u, 0u, 0u};
        if (si) {
            F.info = si | kSiStatic | kSiExact;
        } else {
            F.vl = qs_decimal((uint16_t)R.status, dg);
            hash_bits_lane(dg, F.vl, g_enc_nbits, F.vh, F.vb);
            F.info = 24u | kSiStatic;
        }
        O.code[0] = qs_field<EV, DUP>(t, S, F, len, ins, ins_len);
        S.pos += len;
        if ((R.flags & HHUFF_RES_SERVER) && C.server_len != 0) {
            const uint4 rc = A.rec[C.nhdr];
            const QsField G{e_server, C.in + C.server_off, 6u, C.server_len, rc.x, rc.y, rc.z, rc.w, A.info[C.nhdr]};
            O.code[1] = qs_field<EV, DUP>(t, S, G, len, ins, ins_len);
            S.pos += len;
            O.sins = ins;
            O.sins_at = S.enc;
            S.enc += ins_len;
        }
        if (R.content_length != ~0ull) {
            QsField G{q_cl_name, dg, 14u, 0u, N.cl, 0u, 0u, 0u, 4u | kSiStatic};
            if (R.content_length == 0) {
                G.info |= kSiExact;
            } else {
                G.vl = qs_decimal(R.content_length, dg);
                hash_bits_lane(dg, G.vl, g_enc_nbits, G.vh, G.vb);
            }
            O.code[2] = qs_field<EV, DUP>(t, S, G, len, ins, ins_len);
            S.pos += len;
        }
    }
    const uint32_t h0 = R.hdr_first, h1 = R.hdr_first + R.nhdr;
    for (uint32_t h = h0; h < h1; ++h) {
        const uint32_t info = A.info[h];
        if (info & kSiBad) {  // a string past in_size: the response is refused
            O.bad = true;
            return;
        }
        const hhuff_hpack_header_t H = C.hdr[h];
        const uint4 rc = A.rec[h];
        const QsField F{C.in + H.name_off, C.in + H.value_off, H.name_len, H.value_len, rc.x, rc.y, rc.z, rc.w, info};
        const uint32_t code = qs_field<EV, DUP>(t, S, F, len, ins, ins_len);
        A.op[h] = make_uint4(S.pos, r, code, 0u);
        const uint64_t at = enc0 + S.enc;
        A.ins[h] = make_uint4((uint32_t)at, (uint32_t)(at >> 32), ins, 0u);
        S.pos += len;
        S.enc += ins_len;
    }
    if (R.flags & HHUFF_QRES_DATAGRAM) {  // no static entry, not likely to repeat
        QsField F{q_dfid_name, C.in + R.dfid_off, 16u, R.dfid_len, N.dfid, 0u, 0u, 0u, 0u};
        hash_bits_lane(q_dfid_name, 16u, g_enc_nbits, F.nh, F.nb);
        hash_bits_lane(F.v, F.vl, g_enc_nbits, F.vh, F.vb);
        O.code[3] = qs_field<EV, DUP>(t, S, F, len, ins, ins_len);
        O.df_len = len;
        S.pos += len;
    }
}
}  // namespace

__global__ __launch_bounds__(256) void qse_prep_kernel(QseArgs A) {
    __shared__ uint8_t s_nbits[256];
    s_nbits[threadIdx.x] = g_enc_nbits[threadIdx.x];
    __syncthreads();
    const QseCall& C = A.c;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i <= C.nhdr; i += (uint64_t)gridDim.x * 256u) {
        uint32_t info, nl, vl;
        const uint8_t *n, *v;
        if (i == C.nhdr) {  // the server name: static name reference 92, likely to repeat (:1387-1389)
            const bool bad = (uint64_t)C.server_off + C.server_len > C.in_size;
            n = e_server, nl = 6, v = C.in + C.server_off, vl = bad ? 0u : C.server_len;
            info = 92u | kSiStatic | kSiLtr | (bad ? kSiBad : 0u);
        } else {
            const hhuff_hpack_header_t H = C.hdr[i];
            const bool bad = (uint64_t)H.name_off + H.name_len > C.in_size || (uint64_t)H.value_off + H.value_len > C.in_size;
            nl = bad ? 0u : H.name_len, vl = bad ? 0u : H.value_len;
            n = C.in + H.name_off, v = C.in + H.value_off;
            info = (bad ? kSiBad : 0u) | ((H.flags & HHUFF_HDR_DONT_COMPRESS) ? kSiDc : 0u);
            if (!bad && (H.flags & HHUFF_HDR_TOKEN)) {  // h2o_qpack_lookup_static[token] (flatten_header :1219-1224)
                bool exact;
                const int32_t sidx = q_lookup_static(n, nl, v, vl, exact);
                if (sidx >= 0) info |= (uint32_t)sidx | kSiStatic | (exact ? kSiExact : 0u);
                if (H.flags & HHUFF_HDR_LIKELY_TO_REPEAT) info |= kSiLtr;
            }
            A.op[i] = make_uint4(0u, 0u, kOpSkip, 0u);  // a header no response lists writes nothing
            A.ins[i] = make_uint4(0u, 0u, kInsNone, 0u);
        }
        A.rec[i] = prep_pair(A.lw, (uint32_t)i, n, nl, v, vl, s_nbits);
        A.info[i] = info;
    }
}

namespace {
// hhuff_qpack_session_response_bound (include/hhuff.h) of one response, on the device
__device__ __forceinline__ uint64_t qs_response_bound(uint64_t name_value_bytes, uint32_t nhdr, uint32_t server_len,
                                                      uint32_t dfid_len) {
    return 9u + 2u + 8u + 23u + 26u + (uint64_t)dfid_len + (server_len ? 12ull + server_len : 0ull) + 21ull * nhdr +
           name_value_bytes + 8u;
}
}  // namespace

// the walk: one lane per connection -- its decoder stream, then its responses in order.  EV: the session evicts
// (HHUFF_QENC_EVICT), DUP: it also duplicates draining entries (HHUFF_QENC_DUP, with EV only); <false, false> is
// the table that only grows.  PEERS: the capacity, the Required Insert Count's modulus and the blocked-stream limit
// come from the connection's peer record (include/hhuff.h (2g'')); the ring, the string area and the slab's place
// stay those of the call's header_table_size.
template <bool EV, bool DUP, bool SLOTS, bool PEERS>
__global__ __launch_bounds__(64) void qse_walk_kernel(QseArgs A) {
    static_assert(EV || !DUP, "HHUFF_QENC_DUP is a mode of the evicting table");
    const QseCall& C = A.c;
    const uint64_t c = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (c >= C.nconn) return;
    const uint32_t H = C.header_table_size, M = C.max_inflight;
    // a refused connection (hhuff_slots.h) has no slab: scr is never dereferenced, the call touches nothing of it
    const ConnSlot cs = conn_slot<SLOTS>(C.cmap, c);
    uint8_t* scr = C.scratch + cs.slot * qs_conn_scratch(H, M);
    QsState* ts = reinterpret_cast<QsState*>(scr);
    QsConn t;
    t.s = QsState{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    const bool fresh = !(C.flags & HHUFF_QENC_CONTINUE) || cs.reset;
    if (!fresh && !cs.refused) t.s = *ts;
    // a session is evicting or it is not, duplicating or not: another kind of call touches nothing of it
    constexpr uint32_t kMode = (EV ? kQsEvicting : 0u) | (DUP ? kQsDuplicating : 0u);
    uint32_t cap = H, maxent = 2u * qt_slots(H);
    uint64_t mblk = C.max_blocked;
    if (PEERS) {
        const hhuff_qpack_peer_t P = C.peers[c];
        cap = min(P.max_table_capacity, H);
        maxent = 2u * (P.max_table_capacity / 32u);  // MaxEntries of what the decoder advertised (RFC 9204 4.5.1.1)
        mblk = min((uint64_t)P.max_blocked, mblk);
    }
    // likewise a peer's settings hold for a connection's life, and the record is not stored: a continuing table
    // that holds more than the record allows was filled under another record
    const bool wrong = cs.refused || (!fresh && (t.s.failed & (kQsEvicting | kQsDuplicating)) != kMode) ||
                       (PEERS && !fresh && t.s.used > cap);
    t.s.failed &= 1u;
    t.ent = reinterpret_cast<QsEntry*>(scr + sizeof(QsState));
    t.inf = reinterpret_cast<QsInflight*>(scr + sizeof(QsState) + (uint64_t)(H / 32u) * sizeof(QsEntry));
    t.str = scr + sizeof(QsState) + (uint64_t)(H / 32u) * sizeof(QsEntry) + (uint64_t)M * sizeof(QsInflight);
    t.cap = cap;
    t.scap = H;
    t.slots = qt_slots(H);
    t.imin = ~0u;

    int32_t dst = 0;
    uint32_t consumed = 0;
    if (wrong) {
        dst = HHUFF_RES_EINVAL;
    } else if (t.s.failed) {
        dst = HHUFF_QPK_SKIPPED;
    } else if (C.dec_off != nullptr) {
        const uint32_t off = C.dec_off[c], len = C.dec_len[c];
        dst = (uint64_t)off + len > C.in_size ? HHUFF_RES_EINVAL : qs_handle_input<EV>(t, C.in + off, len, consumed);
        if (dst != 0) t.s.failed = 1u;
    }
    if (EV && !wrong)
        for (uint32_t k = 0; k < t.s.ninflight; ++k) t.imin = min(t.imin, t.inf[k].blocking & 0x7FFFFFFFu);
    C.dec_status[c] = dst;
    C.dec_consumed[c] = consumed;

    const uint64_t ebase = C.enc_out_off[c], eend = C.enc_out_off[c + 1];
    const uint64_t room = eend > ebase ? eend - ebase : 0ull;
    uint64_t enc_len = 0;
    bool setcap = false, nospace = false;
    if (!wrong && !t.s.failed && fresh && (C.flags & HHUFF_QENC_SET_CAPACITY)) {
        const uint32_t n = int_len(cap, 5);
        if (n > room)
            nospace = true;  // not even the capacity instruction fits: nothing of this step is written
        else
            setcap = true, enc_len = n;
    }
    A.cplan[c] = make_uint4((uint32_t)ebase, (uint32_t)(ebase >> 32), setcap ? 1u : 0u, cap);

    QsNames N;
    uint32_t nb;
    hash_bits_lane(q_status_name, 7u, g_enc_nbits, N.status, nb);
    hash_bits_lane(q_cl_name, 14u, g_enc_nbits, N.cl, nb);
    hash_bits_lane(q_dfid_name, 16u, g_enc_nbits, N.dfid, nb);

    const uint32_t r1 = min(C.conn_first[c + 1], C.nres), r0 = min(C.conn_first[c], r1);
    for (uint32_t r = r0; r < r1; ++r) {
        int32_t st = 0;
        uint32_t rf = 0, body = 0;
        uint64_t total = 0;
        if (wrong) {
            st = HHUFF_RES_EINVAL;
        } else if (t.s.failed) {
            st = HHUFF_RES_SKIPPED;
        } else if (nospace) {
            st = HHUFF_RES_SPACE;
        } else {
            const hhuff_qpack_response_t R = C.res[r];
            const uint64_t base = C.out_off[r], limit = C.out_off[r + 1];
            const bool server = !(R.flags & HHUFF_QRES_REQUEST) && (R.flags & HHUFF_RES_SERVER) && C.server_len != 0;
            if ((uint64_t)R.hdr_first + R.nhdr > C.nhdr || limit < base || (server && (A.info[C.nhdr] & kSiBad)) ||
                ((R.flags & HHUFF_QRES_DATAGRAM) && (uint64_t)R.dfid_off + R.dfid_len > C.in_size)) {
                st = HHUFF_RES_EINVAL;
            } else if (EV) {
                // every refusal comes before the section touches the table: eviction cannot be undone
                const uint32_t h0 = R.hdr_first, h1 = R.hdr_first + R.nhdr;
                bool bad = false;
                uint64_t nv = 0, ibound = server ? 26ull + C.server_len : 0ull;
                for (uint32_t h = h0; h < h1 && !bad; ++h) {
                    const uint32_t info = A.info[h];
                    const hhuff_hpack_header_t Hd = C.hdr[h];
                    bad = (info & kSiBad) != 0;
                    nv += (uint64_t)Hd.name_len + Hd.value_len;
                    if (info & kSiLtr) ibound += 20ull + Hd.name_len + Hd.value_len;
                }
                const uint64_t bound = qs_response_bound(nv, R.nhdr, server ? C.server_len : 0u,
                                                         (R.flags & HHUFF_QRES_DATAGRAM) ? R.dfid_len : 0u);
                uint32_t mode = !(R.flags & HHUFF_QRES_NO_ENCODER_STREAM) && (uint64_t)t.s.num_blocked < mblk ? 2u : 1u;
                if (t.s.ninflight >= M) mode = 0u;  // no slot: as with no encoder at all
                if (bad) {
                    st = HHUFF_RES_EINVAL;
                } else if (limit - base < bound || bound > 0xFFFFFFFFull || (mode == 2u && room - enc_len < ibound)) {
                    st = HHUFF_RES_SPACE;
                } else {
                    rf = mode == 0u ? 1u : 0u;
                    QsSection S;
                    QsOwn O;
                    qs_walk_section<EV, DUP>(A, t, R, r, mode, ebase + enc_len, N, S, O);
                    uint32_t ric = 0, delta = 0, plen = 2, largest = S.largest;
                    bool blocking = false;
                    if (largest != 0) {  // finalize_flatten (:1263-1298), the Required Insert Count wrapped (RFC 9204 4.5.1.1)
                        if (largest < t.s.lkr) largest = t.s.lkr;
                        blocking = largest > t.s.lkr;
                        // (a peer that advertised under 32 bytes has no entry to refer to: only a record that
                        // changed in mid-life, the caller's error, meets the guard)
                        ric = (PEERS && maxent == 0u ? 0u : largest % maxent) + 1u;
                        delta = largest <= S.base ? S.base - largest : 0x80000000u | (largest - S.base - 1u);
                        plen = int_len(ric, 8) + int_len(delta & 0x7FFFFFFFu, 7);
                        t.inf[t.s.ninflight] = QsInflight{C.stream_id[r], largest, S.smallest | (blocking ? 0x80000000u : 0u)};
                        ++t.s.ninflight;
                        t.s.num_blocked += blocking ? 1u : 0u;
                        t.imin = min(t.imin, S.smallest);
                    }
                    const uint64_t body64 = (uint64_t)plen + S.pos;
                    total = 1u + q_varint_len(body64) + body64;
                    body = (uint32_t)body64;
                    const uint64_t sat = ebase + enc_len + O.sins_at;
                    A.plan[4 * (uint64_t)r] = make_uint4((uint32_t)base, (uint32_t)(base >> 32), body, (uint32_t)total);
                    A.plan[4 * (uint64_t)r + 1] = make_uint4(ric, delta, 1u + q_varint_len(body64) + plen, O.df_len);
                    A.plan[4 * (uint64_t)r + 2] = make_uint4(O.code[0], O.code[1], O.code[2], O.code[3]);
                    A.plan[4 * (uint64_t)r + 3] = make_uint4((uint32_t)sat, (uint32_t)(sat >> 32), O.sins, 0u);
                    enc_len += S.enc;
                }
            } else {
                const QsState snap = t.s;
                const bool buf = !(R.flags & HHUFF_QRES_NO_ENCODER_STREAM) && (uint64_t)t.s.num_blocked < mblk;
                QsSection S;
                QsOwn O;
                qs_walk_section<EV, DUP>(A, t, R, r, buf ? 2u : 1u, ebase + enc_len, N, S, O);
                if (!O.bad && S.largest != 0 && t.s.ninflight >= M) {  // no slot: as with no encoder at all
                    t.s = snap;
                    qs_walk_section<EV, DUP>(A, t, R, r, 0u, ebase + enc_len, N, S, O);
                    rf = 1u;
                }
                uint32_t ric = 0, delta = 0, plen = 2, largest = S.largest;
                bool blocking = false;
                if (largest != 0) {  // finalize_flatten (:1263-1298)
                    if (largest < t.s.lkr) largest = t.s.lkr;
                    blocking = largest > t.s.lkr;
                    ric = largest + 1u;
                    delta = largest <= S.base ? S.base - largest : 0x80000000u | (largest - S.base - 1u);
                    plen = int_len(ric, 8) + int_len(delta & 0x7FFFFFFFu, 7);
                }
                const uint64_t body64 = (uint64_t)plen + S.pos;
                total = 1u + q_varint_len(body64) + body64;
                if (O.bad)
                    st = HHUFF_RES_EINVAL;
                else if (total > limit - base || body64 > 0xFFFFFFFFull || enc_len + S.enc > room)
                    st = HHUFF_RES_SPACE;
                if (st != 0) {
                    t.s = snap;
                    rf = 0;
                } else {
                    body = (uint32_t)body64;
                    if (S.largest != 0) {
                        t.inf[t.s.ninflight] = QsInflight{C.stream_id[r], largest, blocking ? 1u : 0u};
                        ++t.s.ninflight;
                        t.s.num_blocked += blocking ? 1u : 0u;
                    }
                    const uint64_t sat = ebase + enc_len + O.sins_at;
                    A.plan[4 * (uint64_t)r] = make_uint4((uint32_t)base, (uint32_t)(base >> 32), body, (uint32_t)total);
                    A.plan[4 * (uint64_t)r + 1] = make_uint4(ric, delta, 1u + q_varint_len(body64) + plen, O.df_len);
                    A.plan[4 * (uint64_t)r + 2] = make_uint4(O.code[0], O.code[1], O.code[2], O.code[3]);
                    A.plan[4 * (uint64_t)r + 3] = make_uint4((uint32_t)sat, (uint32_t)(sat >> 32), O.sins, 0u);
                    enc_len += S.enc;
                }
            }
        }
        if (st != 0) {
            total = 0;
            A.plan[4 * (uint64_t)r] = make_uint4(0u, 0u, 0u, 0u);
        }
        C.out_len[r] = (uint32_t)total;
        C.header_len[r] = body;
        C.rstatus[r] = st;
        C.rflags[r] = (uint8_t)rf;
    }
    t.s.failed |= kMode;
    if (!wrong) *ts = t.s;
    C.enc_out_len[c] = (uint32_t)enc_len;
}

namespace {
// an insert's instruction (emit_insert_with_nameref / _without_nameref, qpack.c:1068-1086); Duplicate is one
// prefix integer and no strings
__device__ __forceinline__ void qs_emit_insert(RegSink& sink, const GlobalSource& nsrc, const GlobalSource& vsrc, uint32_t ins,
                                               uint32_t noff, uint32_t nl, uint32_t voff, uint32_t vl, uint32_t nbits,
                                               uint32_t vbits, const uint2* enc, const LongWork& L) {
    switch (ins & kInsMask) {
        case kInsDup: sink_int(sink, 0u, ins >> kInsShift, 5); return;
        case kInsStatic: sink_int(sink, 0xc0u, ins >> kInsShift, 6); break;
        case kInsDynamic: sink_int(sink, 0x80u, ins >> kInsShift, 6); break;
        default: q_sink_string(sink, nsrc, 0x40u, noff, nl, nbits, 5, false, enc, L); break;
    }
    q_sink_string(sink, vsrc, 0u, voff, vl, vbits, 7, false, enc, L);
}
}  // namespace

// emit: items 0 .. nhdr-1 the fields, nhdr .. 2 nhdr-1 their inserts, then the response heads, then the
// connections (Set Dynamic Table Capacity)
__global__ __launch_bounds__(256) void qse_emit_kernel(QseArgs A) {
    __shared__ uint2 s_enc[256];
    s_enc[threadIdx.x] = make_uint2(g_enc_code[threadIdx.x], g_enc_nbits[threadIdx.x]);
    __syncthreads();
    const QseCall& C = A.c;
    const GlobalSource src{C.in, C.in_size};
    const uint64_t nh = C.nhdr, items = 2 * nh + C.nres + C.nconn;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < items; i += (uint64_t)gridDim.x * 256u) {
        if (i < 2 * nh) {
            const bool insert = i >= nh;
            const uint64_t h = insert ? i - nh : i;
            const uint4 o = A.op[h];
            if (o.z & kOpSkip) continue;
            const uint4 p0 = A.plan[4 * (uint64_t)o.y], p1 = A.plan[4 * (uint64_t)o.y + 1];
            if (p0.w == 0) continue;  // the response failed
            const hhuff_hpack_header_t Hd = C.hdr[h];
            const uint4 rc = A.rec[h];
            RegSink sink;
            if (insert) {
                const uint4 I = A.ins[h];
                if ((I.z & kInsMask) == kInsNone) continue;
                sink.init(C.enc_out + ((uint64_t)I.y << 32 | I.x));
                qs_emit_insert(sink, src, src, I.z, Hd.name_off, Hd.name_len, Hd.value_off, Hd.value_len, rc.z, rc.w, s_enc, A.lw);
            } else {
                sink.init(C.out + ((uint64_t)p0.y << 32 | p0.x) + p1.z + o.x);
                q_emit_field(sink, src, src, o.z, Hd.name_off, Hd.name_len, Hd.value_off, Hd.value_len, rc.z, rc.w, s_enc, A.lw);
            }
            sink.finish();
            continue;
        }
        if (i >= 2 * nh + C.nres) {
            const uint4 cp = A.cplan[i - 2 * nh - C.nres];
            if (cp.z) {  // Set Dynamic Table Capacity
                RegSink sink;
                sink.init(C.enc_out + ((uint64_t)cp.y << 32 | cp.x));
                sink_int(sink, 0x20u, cp.w, 5);
                sink.finish();
            }
            continue;
        }
        const uint64_t r = i - 2 * nh;
        const uint4 p0 = A.plan[4 * r], p1 = A.plan[4 * r + 1], p2 = A.plan[4 * r + 2], p3 = A.plan[4 * r + 3];
        if (p0.w == 0) continue;
        const hhuff_qpack_response_t R = C.res[r];
        uint8_t* base = C.out + ((uint64_t)p0.y << 32 | p0.x);
        const uint4 sr = A.rec[C.nhdr];
        RegSink sink;
        sink.init(base);
        q_sink_frame_head(sink, p0.z);
        sink_int(sink, 0u, p1.x, 8);  // Required Insert Count (:1283), delta base with its sign (:1285-1291)
        sink_int(sink, p1.y >> 31 ? 0x80u : 0u, p1.y & 0x7FFFFFFFu, 7);
        if (!(p2.x & kOpSkip) && q_emit_ref(sink, p2.x)) q_sink_decimal(sink, (uint16_t)R.status, s_enc);
        if (!(p2.y & kOpSkip))
            q_emit_field(sink, src, src, p2.y, 0u, 0u, C.server_off, C.server_len, 0u, sr.w, s_enc, A.lw);
        if (!(p2.z & kOpSkip) && q_emit_ref(sink, p2.z)) q_sink_decimal(sink, R.content_length, s_enc);
        sink.finish();
        if (!(p2.w & kOpSkip)) {  // datagram-flow-id last (:1396-1398)
            RegSink s2;
            s2.init(base + p0.w - p1.w);
            const GlobalSource nsrc{q_dfid_name, 16};
            q_emit_field(s2, nsrc, src, p2.w, 0u, 16u, R.dfid_off, R.dfid_len, code_bits(q_dfid_name, 16),
                          code_bits(C.in + R.dfid_off, R.dfid_len), s_enc, A.lw);
            s2.finish();
        }
        if ((p3.z & kInsMask) != kInsNone) {  // the server name's insert or duplication
            RegSink s3;
            s3.init(C.enc_out + ((uint64_t)p3.y << 32 | p3.x));
            qs_emit_insert(s3, src, src, p3.z, 0u, 0u, C.server_off, C.server_len, 0u, sr.w, s_enc, A.lw);
            s3.finish();
        }
    }
}

uint64_t qpenc_conn_scratch(uint32_t header_table_size, uint32_t max_inflight) {
    return qs_conn_scratch(header_table_size, max_inflight);
}

namespace {
// the workspace of a call: its size with base = NULL, its pointers with the allocation
uint64_t qpe_carve(QpeArgs& A, uint64_t long_bits, uint64_t long_jobs, uint8_t* base) {
    Carve cv{base};
    const uint64_t nhdr = A.nhdr, nres = A.nres;
    A.rec = cv.take<uint4>(nhdr + 1);
    A.plan = cv.take<uint4>(2 * nres);
    A.lw = long_ws(cv, long_bits, long_jobs);
    A.dst = cv.take<uint2>(nhdr);
    return cv.off;
}

uint64_t qse_carve(QseArgs& A, uint64_t long_bits, uint64_t long_jobs, uint8_t* base) {
    Carve cv{base};
    const uint64_t nhdr = A.c.nhdr, nres = A.c.nres;
    A.rec = cv.take<uint4>(nhdr + 1);
    A.op = cv.take<uint4>(nhdr);
    A.ins = cv.take<uint4>(nhdr);
    A.plan = cv.take<uint4>(4 * nres);
    A.cplan = cv.take<uint4>(A.c.nconn);
    A.lw = long_ws(cv, long_bits, long_jobs);
    A.info = cv.take<uint32_t>(nhdr + 1);
    return cv.off;
}
}  // namespace

hipError_t launch_qpack_flatten(const QpeCall& call, hipStream_t stream) {
    if (call.nres == 0) return hipSuccess;
    const uint32_t nhdr = call.nhdr, nres = call.nres;
    // long strings: bits of a header's name and value and of the server name; payload jobs of a field's name
    // and value, of a response head's server and datagram-flow-id values
    const uint64_t long_bits = 2ull * nhdr + 2, long_jobs = 2ull * nhdr + 2ull * nres + 2;
    if (long_bits > 0xFFFFFFFFull || long_jobs > 0xFFFFFFFFull) return hipErrorInvalidValue;
    QpeArgs A{call, nullptr, nullptr, nullptr, LongWork{}};
    uint8_t* ws = nullptr;
    hipError_t e = work_alloc((void**)&ws, qpe_carve(A, long_bits, long_jobs, nullptr), stream);
    if (e != hipSuccess) return e;
    qpe_carve(A, long_bits, long_jobs, ws);
    e = hipMemsetAsync(A.lw.bits, 0, 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(A.lw.njobs, 0, 4, stream);
    const uint32_t gs = (uint32_t)std::min<uint64_t>((nhdr + 256ull) / 256u, 16384ull);
    const uint32_t gl = (uint32_t)std::min<uint64_t>((nres + 255ull) / 256u, 16384ull);
    const uint32_t ge = (uint32_t)std::min<uint64_t>(((uint64_t)nhdr + nres + 255u) / 256u, 16384ull);
    HHUFF_LAUNCH(e, qpe_size_kernel, gs, 256, stream, A);
    if (e == hipSuccess) e = launch_long_bits(false, A.in, A.hdr, nhdr, A.server_off, A.server_len, A.rec, A.lw, stream);
    HHUFF_LAUNCH(e, qpe_layout_kernel, gl, 256, stream, A);
    HHUFF_LAUNCH(e, qpe_emit_kernel, ge, 256, stream, A);
    if (e == hipSuccess) e = launch_long_payload(A.in, A.lw, stream);
    const hipError_t f = hipFreeAsync(ws, stream);
    return e != hipSuccess ? e : f;
}

hipError_t launch_qpack_sessions(const QseCall& call, hipStream_t stream) {
    if (call.nconn == 0) return hipSuccess;
    const uint32_t nhdr = call.nhdr, nres = call.nres, nconn = call.nconn;
    // long strings: bits of a header's name and value and of the server name; payload jobs of a field's and of
    // its insert's name and value, of a response head's server value, server insert and datagram-flow-id
    const uint64_t long_bits = 2ull * nhdr + 2, long_jobs = 4ull * nhdr + 3ull * nres + 2;
    if (long_bits > 0xFFFFFFFFull || long_jobs > 0xFFFFFFFFull) return hipErrorInvalidValue;
    QseArgs A{call, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, LongWork{}};
    uint8_t* ws = nullptr;
    hipError_t e = work_alloc((void**)&ws, qse_carve(A, long_bits, long_jobs, nullptr), stream);
    if (e != hipSuccess) return e;
    qse_carve(A, long_bits, long_jobs, ws);
    e = hipMemsetAsync(A.lw.bits, 0, 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(A.lw.njobs, 0, 4, stream);
    if (e == hipSuccess && nres != 0) e = hipMemsetAsync(A.plan, 0, 64ull * nres, stream);  // a response no connection lists writes nothing
    const uint32_t gp = (uint32_t)std::min<uint64_t>((nhdr + 256ull) / 256u, 8192ull);
    const uint32_t ge = (uint32_t)std::min<uint64_t>((2ull * nhdr + nres + nconn + 255u) / 256u, 16384ull);
    HHUFF_LAUNCH(e, qse_prep_kernel, gp, 256, stream, A);
    if (e == hipSuccess) e = launch_long_bits(true, call.in, call.hdr, nhdr, call.server_off, call.server_len, A.rec, A.lw, stream);
    // the kernel's instantiation with or without connection slots (hhuff_slots.h) and peer records
    auto walk = [&](auto slots, auto peers) {
        constexpr bool S = decltype(slots)::value, P = decltype(peers)::value;
        if (call.flags & HHUFF_QENC_DUP) {  // (only with HHUFF_QENC_EVICT: the C entry refuses it alone)
            HHUFF_LAUNCH(e, (qse_walk_kernel<true, true, S, P>), (nconn + 63u) / 64u, 64, stream, A);
        } else if (call.flags & HHUFF_QENC_EVICT) {
            HHUFF_LAUNCH(e, (qse_walk_kernel<true, false, S, P>), (nconn + 63u) / 64u, 64, stream, A);
        } else {
            HHUFF_LAUNCH(e, (qse_walk_kernel<false, false, S, P>), (nconn + 63u) / 64u, 64, stream, A);
        }
    };
    auto walk_slots = [&](auto peers) {
        if (call.cmap)
            walk(std::true_type{}, peers);
        else
            walk(std::false_type{}, peers);
    };
    if (call.peers)
        walk_slots(std::true_type{});
    else
        walk_slots(std::false_type{});
    HHUFF_LAUNCH(e, qse_emit_kernel, ge, 256, stream, A);
    if (e == hipSuccess) e = launch_long_payload(call.in, A.lw, stream);
    const hipError_t f = hipFreeAsync(ws, stream);
    return e != hipSuccess ? e : f;
}
}  // namespace hhuff
