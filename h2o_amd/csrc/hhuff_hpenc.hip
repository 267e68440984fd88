// HTTP/2 header encoder on the GPU (encode side); the HTTP/3 ones are in hhuff_qpenc.hip and
// what both use in hhuff_enc.h.
//
// h2o_hpack_flatten_response (lib/http2/hpack.c:1137-1177), h2o_hpack_flatten_trailers
// (:1179-1196), h2o_hpack_flatten_push_promise (:1098-1135) and, on the client side, h2o_hpack_flatten_request
// (:1044-1096) for many connections, each with its encoder dynamic table (do_encode_header :858-937,
// header_table_add :277-317 with at most 32 entries, header_table_adjust_size :839-856).
// What a field becomes depends on the table, and the table on every earlier field of the connection, so
// the table work is sequential per connection -- but it needs no output bytes: only lengths and equality.
//   1. prep (hpe_prep_kernel, one lane per header): a hash of the name and of the value, the Huffman code
//      bits of each (h2o_hpack_encode_string's verdict and length, hpack.c:816-837), the token facts
//      do_encode_header reads (static name index, dont_compress); strings longer than kLongStr go to
//      long_bits_kernel, one wave per string;
//   2. the walk (hpe_table_kernel, one lane per connection): the table's lengths and hashes sit in LDS, a
//      field compares them with all 32 slots at once (no branch per entry) and checks the bytes of the
//      candidates only; it yields each field's representation, byte length and place in the response.
//      Table entries are references to the bytes (this call's input, or the connection's ring);
//   3. emit (hpe_emit_kernel, one lane per field and one per response head): every field writes its bytes
//      at its place -- prefix integers, raw copies, Huffman codes (encode_core) -- through a register sink;
//      payloads longer than kLongStr are left to long_payload_kernel (one wave per string, OR-placed code
//      bits in LDS), so no lane walks a long string alone;
//   4. frames (hpe_frames_kernel, one workgroup per response longer than max_frame_size): the payload moves
//      apart for the CONTINUATION frame headers, last chunk first (fixup_frame_headers :1012-1042);
//   5. the table pass (hpe_ring_kernel, one wave per connection) copies the live entries' bytes into the
//      connection's other ring, so the next call (HHUFF_ENC_CONTINUE) reads only scratch.
// long_bits_kernel and long_payload_kernel also serve the QPACK encoders, through launch_long_bits and
// launch_long_payload.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hhuff_enc.h"
#include "hhuff_image.h"
#include "hhuff_slots.h"

namespace hhuff {
namespace {
__device__ const uint8_t e_static_bytes[HHUFF_STATIC_NBYTES] = HHUFF_STATIC_BYTES_INIT;
__device__ const uint16_t e_static_ent[61 * 4] = HHUFF_STATIC_ENT_INIT;

constexpr uint32_t kOverhead = 32;     // HEADER_TABLE_ENTRY_SIZE_OFFSET (hpack.c:30)
constexpr uint32_t kTableOffset = 62;  // HEADER_TABLE_OFFSET (hpack.c:29)
constexpr uint32_t kMaxEntries = 32;   // header_table_add(..., 32) (hpack.c:921)
constexpr uint32_t kInitialCap = 4096; // conn->_output_header_table.hpack_capacity (connection.c:1847)
constexpr uint32_t kRing = 4096;       // live entry bytes never exceed the capacity (<= 4096)
constexpr uint32_t kServerIndex = 54;  // H2O_TOKEN_SERVER's http2_static_table_name_index

// info word of a prepped string pair
constexpr uint32_t kInfoStatic = 0x7Fu;  // static name index (tokens only)
constexpr uint32_t kInfoTokDc = 1u << 8;  // token flag dont_compress (cookie, set-cookie)
constexpr uint32_t kInfoTok = 1u << 9;
constexpr uint32_t kInfoHdrDc = 1u << 10;
constexpr uint32_t kInfoBad = 1u << 11;  // a string past in_size
constexpr uint32_t kInfoFastShift = 12;  // bits 12-19: h2o_hpack_flatten_request's one-byte reference, 0 = none
constexpr uint32_t kInfoFastOwn = 1u << 20;  // ... for one of its own fields (:method, :scheme, :path)

// op code of a field
constexpr uint32_t kOpIndexed = 0, kOpIdxName = 1, kOpNever = 2, kOpNewName = 3;
constexpr uint32_t kOpAsIs = 1u << 9;  // the value goes as it is (encode_as_is, hpack.c:806-814)
constexpr uint32_t kOpFast = 1u << 10; // one byte (bits 11-18): flatten_request's static references

// byte sources of a table entry's name / value
constexpr uint64_t kSrcIn = 0;               // input offset (added in this call)
constexpr uint64_t kSrcScr = 1ull << 62;     // scratch offset (a ring: added by an earlier call)
constexpr uint64_t kSrcConst = 2ull << 62;   // e_server
constexpr uint64_t kSrcOff = (1ull << 62) - 1;

struct EncState {
    uint32_t start, num, ring, failed;
    uint32_t size, cap, pad0, pad1;
};
struct EncEntry {
    uint64_t nsrc, vsrc;
    uint32_t nl, vl, nh, vh;
    uint32_t tok, pad;
};
static_assert(sizeof(EncState) == 32 && sizeof(EncEntry) == 40, "scratch records");
constexpr uint64_t kConnScratch = sizeof(EncState) + kMaxEntries * sizeof(EncEntry) + 2 * kRing;
static_assert(kConnScratch % 16 == 0, "scratch alignment");
// connection images (hhuff_image.h) restate the two records, the ring and the scratch source
static_assert(offsetof(EncState, failed) == offsetof(img::HeState, failed) && offsetof(EncState, cap) == offsetof(img::HeState, cap) &&
                  offsetof(EncEntry, vsrc) == offsetof(img::HeEntry, vsrc) && offsetof(EncEntry, vh) == offsetof(img::HeEntry, vh) &&
                  offsetof(EncEntry, tok) == offsetof(img::HeEntry, tok) && kSrcScr == img::kHeScr && kSrcOff == img::kHeOff &&
                  kMaxEntries == img::kHeEntries && kRing == img::kHeRing && kInitialCap == img::kHeCap,
              "hhuff_image.h: HPACK_ENC slab");
}  // namespace

struct HpeArgs : HpeCall {  // the call (the kernels read its members as their own) and its workspace
    uint4* rec;      // [nhdr + 1] {name hash, value hash, name code bits, value code bits}; item nhdr: server
    uint32_t* info;  // [nhdr + 1]
    uint4* op;       // [nhdr] {dst lo, dst hi, code, 0}
    uint4* plan;     // [2 nres] {base lo, base hi, payload, total} {size update or ~0, server code, server pos, cl len}
    uint32_t* big;   // [nres + 1]: count, then the responses longer than their max_frame_size
    LongWork lw;
};

namespace {
__device__ __forceinline__ const uint8_t* hpe_src(const HpeArgs& A, uint64_t s) {
    const uint64_t o = s & kSrcOff;
    switch (s >> 62) {
        case 0: return A.in + o;
        case 1: return A.scratch + o;
        default: return e_server + o;
    }
}

__device__ __forceinline__ uint32_t digits(uint64_t v) {
    uint32_t n = 1;
    while (v >= 10) {
        v /= 10;
        ++n;
    }
    return n;
}

// h2o_hpack_flatten_request's one-byte static references (hpack.c:950-985 for its own fields, :1083-1086 for
// accept-encoding among the headers) as an info word; the walk applies them by the field's place
__device__ __forceinline__ uint32_t request_fast(const uint8_t* n, uint32_t nl, const uint8_t* v, uint32_t vl) {
    uint32_t b = 0, own = kInfoFastOwn;
    if (nl == 7 && lit_eq(n, ":method", 7)) {
        b = vl == 3 && lit_eq(v, "GET", 3) ? 0x82u : vl == 4 && lit_eq(v, "POST", 4) ? 0x83u : 0u;
    } else if (nl == 7 && lit_eq(n, ":scheme", 7)) {
        b = vl == 5 && lit_eq(v, "https", 5) ? 0x87u : vl == 4 && lit_eq(v, "http", 4) ? 0x86u : 0u;
    } else if (nl == 5 && lit_eq(n, ":path", 5)) {
        b = vl == 1 && v[0] == '/' ? 0x84u : vl == 11 && lit_eq(v, "/index.html", 11) ? 0x85u : 0u;
    } else if (nl == 15 && vl == 13 && lit_eq(n, "accept-encoding", 15) && lit_eq(v, "gzip, deflate", 13)) {
        b = 0x90u, own = 0u;
    }
    return b ? (b << kInfoFastShift | own) : 0u;
}

// What a record's kind decides about its frames: the first frame's type and its flags besides END_HEADERS, the
// stream id of every frame header of the block, and the payload bytes ahead of the size update.  HEADERS
// (:1094, :1174, :1194) go out on the record's own stream; a promise (h2o_hpack_flatten_push_promise,
// :1098-1135) is a PUSH_PROMISE without END_STREAM on the parent stream whose payload starts with the
// promised stream id (:1116).  The walk, the emit head and the frames kernel all read it here.
struct FrameRule {
    uint32_t type, flags, sid, lead;
    bool own;  // the header range starts with `status` own fields, no :status / server / content-length
};
__device__ __forceinline__ FrameRule frame_rule(const hhuff_hpack_response_t& R) {
    if (R.flags & HHUFF_RES_PUSH_PROMISE) return FrameRule{5u, 0u, R.parent_stream_id, 4u, true};
    const bool trailers = (R.flags & HHUFF_RES_TRAILERS) != 0;
    const uint32_t es = (trailers || (R.flags & HHUFF_RES_END_STREAM)) ? 1u : 0u;
    return FrameRule{1u, es, R.stream_id, 0u, !trailers && (R.flags & HHUFF_RES_REQUEST)};
}
}  // namespace

// 1. prep: one lane per header (item nhdr: the server name under the server token)
__global__ __launch_bounds__(256) void hpe_prep_kernel(HpeArgs A) {
    __shared__ uint8_t s_nbits[256];
    s_nbits[threadIdx.x] = g_enc_nbits[threadIdx.x];
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i <= A.nhdr; i += (uint64_t)gridDim.x * 256u) {
        uint32_t info;
        const uint8_t *n, *v;
        uint32_t nl, vl;
        bool bad;
        if (i == A.nhdr) {
            bad = (uint64_t)A.server_off + A.server_len > A.in_size;
            n = e_server, nl = 6, v = A.in + A.server_off, vl = bad ? 0u : A.server_len;
            info = kServerIndex | kInfoTok | (bad ? kInfoBad : 0u);
        } else {
            const hhuff_hpack_header_t H = A.hdr[i];
            bad = (uint64_t)H.name_off + H.name_len > A.in_size || (uint64_t)H.value_off + H.value_len > A.in_size;
            nl = bad ? 0u : H.name_len, vl = bad ? 0u : H.value_len;
            n = A.in + H.name_off, v = A.in + H.value_off;
            info = (bad ? kInfoBad : 0u) | ((H.flags & HHUFF_HDR_DONT_COMPRESS) ? kInfoHdrDc : 0u);
            if (H.flags & HHUFF_HDR_TOKEN) {
                // lib/common/token_table.h: a token's http2_static_table_name_index is the first static
                // entry with its name; dont_compress is set for cookie and set-cookie
                uint32_t sidx = 0;
                for (uint32_t k = 0; k < 61 && sidx == 0; ++k)
                    if (e_static_ent[4 * k + 1] == nl && bytes_eq(e_static_bytes + e_static_ent[4 * k], n, nl)) sidx = k + 1;
                const bool dc = (nl == 6 && lit_eq(n, "cookie", 6)) || (nl == 10 && lit_eq(n, "set-cookie", 10));
                info |= kInfoTok | sidx | (dc ? kInfoTokDc : 0u) | request_fast(n, nl, v, vl);
            }
        }
        A.rec[i] = prep_pair(A.lw, (uint32_t)i, n, nl, v, vl, s_nbits);
        A.info[i] = info;
        if (i < A.nhdr) A.op[i] = make_uint4(0u, 0u, kOpSkip, 0u);  // a header no response lists writes nothing
    }
}

// Long strings' hash and code bits, one wave per string (the sums of hash_bits_lane split over the lanes):
// rec[item].x / .z for a name, .y / .w for a value.  HASH = false: the bits only (QPACK).
template <bool HASH>
__global__ __launch_bounds__(256) void long_bits_kernel(const uint8_t* in, const hhuff_hpack_header_t* hdr, uint32_t nhdr,
                                                        uint32_t server_off, uint32_t server_len, uint4* rec, LongWork L) {
    __shared__ uint8_t s_nbits[256];
    s_nbits[threadIdx.x] = g_enc_nbits[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t n = min(L.bits[0], L.cap);
    for (uint32_t j = blockIdx.x * 4u + (threadIdx.x >> 6); j < n; j += gridDim.x * 4u) {
        const uint32_t e = L.bits[1 + j], item = e >> 1, which = e & 1u;
        const uint8_t* p;
        uint32_t len;
        if (item == nhdr) {
            p = in + server_off, len = server_len;
        } else {
            const hhuff_hpack_header_t H = hdr[item];
            p = in + (which ? H.value_off : H.name_off), len = which ? H.value_len : H.name_len;
        }
        uint32_t sum = 0, bits = 0;
        for (uint32_t k = (uint32_t)lane; 4u * k < len; k += 64u) {
            uint32_t b;
            const uint32_t w = string_word(p, len, k, s_nbits, b);
            if (HASH) sum += word_term(w, k);
            bits += b;
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            sum += (uint32_t)__shfl_xor((int)sum, d);
            bits += (uint32_t)__shfl_xor((int)bits, d);
        }
        if (lane == 0) {
            uint32_t* r = reinterpret_cast<uint32_t*>(rec + item);
            if (HASH) r[which] = hash_final(sum, len);
            r[2 + which] = bits;
        }
    }
}

namespace {
// One wave codes src[0 .. len) into dst: ceil(bits / 8) bytes, the last padded with the EOS prefix
// (hpack.c:795-798).  Rounds of 256 input bytes, 4 per lane: a lane's four codes are OR-placed at their
// stream bit in the wave's LDS stage (place_bits), the stage's whole words go out, the partial last word
// moves to the front.  stage: kStageWords + 4 words of LDS, zero on entry, left zero.
constexpr uint32_t kStageWords = 256;  // >= 256 bytes x 30 bits / 32 + 1
__device__ void wave_huff_long(const uint8_t* src, uint32_t len, uint8_t* dst, const uint2* enc, uint32_t* stage, int lane) {
    const uint32_t obase = lds_addr(stage);
    uint32_t cb = 0;       // bits in stage word 0 carried from the last round
    uint64_t flushed = 0;  // bytes of dst written
    for (uint32_t r0 = 0; r0 < len; r0 += 256u) {
        const uint32_t a = r0 + 4u * (uint32_t)lane;
        uint2 e[4];
        uint32_t n = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            e[j] = a + j < len ? enc[src[a + j]] : make_uint2(0u, 0u);
            n += e[j].y;
        }
        const uint32_t off = wave_excl_scan(n, lane);
        const uint32_t tb = cb + off;
        const uint32_t n01 = e[0].y + e[1].y, n23 = e[2].y + e[3].y;
        if (max(max(e[0].y, e[1].y), max(e[2].y, e[3].y)) > 16u) {
            place_bits(obase, tb, (uint64_t)e[0].x << e[1].y | e[1].x, n01);
            place_bits(obase, tb + n01, (uint64_t)e[2].x << e[3].y | e[3].x, n23);
        } else {
            place_bits(obase, tb, ((uint64_t)(e[0].x << e[1].y | e[1].x) << n23) | (e[2].x << e[3].y | e[3].x), n);
        }
        wave_lds_sync();
        const uint32_t total = cb + (uint32_t)__builtin_amdgcn_readlane((int)(off + n), 63);
        const bool last = r0 + 256u >= len;
        const uint32_t whole = total >> 5;
        for (uint32_t w = (uint32_t)lane; w < whole; w += 64u) {  // MSB-first words -> stream bytes
            const uint32_t v = __builtin_bswap32(stage[w]);
            __builtin_memcpy(dst + flushed + 4u * w, &v, 4);
        }
        const uint32_t tail = stage[whole];
        wave_lds_sync();
        for (uint32_t w = (uint32_t)lane; w <= whole; w += 64u) stage[w] = 0u;
        wave_lds_sync();
        flushed += 4ull * whole;
        cb = total & 31u;
        if (last) {
            if (lane == 0 && cb) {
                const uint32_t v = tail | (~0u >> cb);  // EOS-prefix padding of the last byte
                for (uint32_t b = 0; b < (cb + 7u) >> 3; ++b) dst[flushed + b] = (uint8_t)(v >> (24 - 8 * b));
            }
        } else if (lane == 0) {
            stage[0] = tail;
        }
        wave_lds_sync();
    }
}
}  // namespace

// Payloads of long strings (HPACK literals and QPACK flatten_string payloads), one wave per string
__global__ __launch_bounds__(256) void long_payload_kernel(const uint8_t* in, LongWork L) {
    __shared__ uint2 s_enc[256];
    __shared__ uint32_t s_stage[4][kStageWords + 4];
    s_enc[threadIdx.x] = make_uint2(g_enc_code[threadIdx.x], g_enc_nbits[threadIdx.x]);
    for (uint32_t k = threadIdx.x; k < 4 * (kStageWords + 4); k += 256) (&s_stage[0][0])[k] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t n = min(*L.njobs, L.jcap);
    for (uint32_t j = blockIdx.x * 4u + (uint32_t)wv; j < n; j += gridDim.x * 4u) {
        const uint4 job = L.jobs[j];
        uint8_t* dst = reinterpret_cast<uint8_t*>((uint64_t)(job.w & 0x7FFFFFFFu) << 32 | job.z);  // an address in `out`
        if (job.w >> 31)
            wave_huff_long(in + job.x, job.y, dst, s_enc, s_stage[wv], lane);
        else
            wave_copy64(in + job.x, dst, lane == 0 ? job.y : 0u, lane);
    }
}

namespace {
// 2. the walk's table: lengths and hashes in LDS ({nl | token << 31, vl, nh, vh} of slot s at
// s_meta[s * 64 + lane]), byte sources in the connection's scratch entries
struct EncTable {
    EncEntry* ent;
    uint4* meta;  // this lane's column: meta[s * 64]
    uint32_t start, num, size, cap;
    __device__ __forceinline__ uint32_t slot(uint32_t k) const { return (start + k) & (kMaxEntries - 1); }
    __device__ __forceinline__ void evict_one() {  // header_table_evict_one (hpack.c:263-275)
        --num;
        const uint4 q = meta[slot(num) * 64];
        size -= (q.x & 0x7FFFFFFFu) + q.y + kOverhead;
    }
    __device__ void add(const EncEntry& e) {  // header_table_add (hpack.c:277-317), at most 32 entries
        const uint32_t add = e.nl + e.vl + kOverhead;
        while (num != 0 && size + add > cap) evict_one();
        while (num >= kMaxEntries) evict_one();
        if (num == 0 && add > cap) return;
        start = (start + kMaxEntries - 1) & (kMaxEntries - 1);
        ent[start] = e;
        meta[start * 64] = make_uint4(e.nl | (e.tok << 31), e.vl, e.nh, e.vh);
        size += add;
        ++num;
    }
};

struct FieldIn {  // what the walk reads of a field
    uint32_t noff, nl, voff, vl;
    uint4 rc;
    uint32_t info;
};

__device__ __forceinline__ FieldIn load_field(const HpeArgs& A, uint32_t h) {
    const hhuff_hpack_header_t H = A.hdr[h];
    return FieldIn{H.name_off, H.name_len, H.value_off, H.value_len, A.rec[h], A.info[h]};
}

// do_encode_header (hpack.c:858-937): returns the op code and its byte length, and updates the table as
// h2o does.  The scan over the entries (:864-890) is done for all 32 slots at once on lengths and hashes;
// the candidates' bytes are then compared in h2o's order (newest first).
__device__ uint32_t hpe_field(const HpeArgs& A, EncTable& t, const FieldIn& F, uint64_t nsrc, uint64_t vsrc, uint32_t& len) {
    const bool tok = (F.info & kInfoTok) != 0;
    const uint32_t key = F.nl | (tok ? 0x80000000u : 0u);
    const uint32_t kmask = tok ? 0xFFFFFFFFu : 0x7FFFFFFFu;  // a token name is compared by pointer (:870-872)
    uint32_t nm = 0, fm = 0;
#pragma unroll
    for (uint32_t k = 0; k < kMaxEntries; ++k) {
        const uint4 q = t.meta[t.slot(k) * 64];
        const bool n_ok = k < t.num && (q.x & kmask) == key && q.z == F.rc.x;
        nm |= (uint32_t)n_ok << k;
        fm |= (uint32_t)(n_ok && q.y == F.vl && q.w == F.rc.y) << k;
    }
    const uint8_t* np = hpe_src(A, nsrc);
    const uint8_t* vp = hpe_src(A, vsrc);
    while (fm) {
        const uint32_t k = __builtin_ctz(fm);
        const EncEntry& e = t.ent[t.slot(k)];
        if (bytes_eq(np, hpe_src(A, e.nsrc), F.nl) && bytes_eq(vp, hpe_src(A, e.vsrc), F.vl)) {
            len = int_len(k + kTableOffset, 7);  // indexed (:881-884)
            return kOpIndexed | ((k + kTableOffset) << 2);
        }
        fm &= fm - 1u;
    }
    uint32_t name_index = F.info & kInfoStatic;  // tokens: the static index; others: the newest name match (:875-876)
    if (!tok) {
        while (nm) {
            const uint32_t k = __builtin_ctz(nm);
            if (bytes_eq(np, hpe_src(A, t.ent[t.slot(k)].nsrc), F.nl)) {
                name_index = k + kTableOffset;
                break;
            }
            nm &= nm - 1u;
        }
    }
    bool dc = (F.info & kInfoHdrDc) != 0;
    if (!dc && tok) dc = (F.info & kInfoTokDc) != 0;  // :892-893
    if (dc) dc = F.vl < 20;                           // :894-895
    uint32_t code;
    if (name_index != 0) {
        code = (dc ? kOpNever : kOpIdxName) | (name_index << 2);
        len = int_len(name_index, dc ? 4u : 6u);
    } else {
        code = kOpNewName;
        len = 1u + str_len(F.nl, F.rc.z);
    }
    if (dc) {
        len += int_len(F.vl, 7) + F.vl;
        code |= kOpAsIs;
    } else {
        len += str_len(F.vl, F.rc.w);
        t.add(EncEntry{nsrc, vsrc, F.nl, F.vl, F.rc.x, F.rc.y, tok ? 1u : 0u, 0u});
    }
    return code;
}
}  // namespace

// 2. the walk: one lane per connection, its responses in order
template <bool SLOTS>
__global__ __launch_bounds__(64) void hpe_table_kernel(HpeArgs A) {
    __shared__ uint4 s_meta[kMaxEntries * 64];
    const uint32_t lane = threadIdx.x;
    const uint64_t c = (uint64_t)blockIdx.x * 64u + lane;
    if (c >= A.nconn) return;
    // a refused connection (hhuff_slots.h) has no slab: scr is never dereferenced, its responses are refused
    const ConnSlot cs = conn_slot<SLOTS>(A.cmap, c);
    uint8_t* scr = A.scratch + cs.slot * kConnScratch;
    EncState* ts = reinterpret_cast<EncState*>(scr);
    EncState s0{0u, 0u, 0u, 0u, 0u, kInitialCap, 0u, 0u};
    if ((A.flags & HHUFF_ENC_CONTINUE) && !cs.reset && !cs.refused) s0 = *ts;
    EncTable t{reinterpret_cast<EncEntry*>(scr + sizeof(EncState)), s_meta + lane, s0.start, s0.num, s0.size, s0.cap};
    for (uint32_t k = 0; k < t.num; ++k) {
        const EncEntry& e = t.ent[t.slot(k)];
        t.meta[t.slot(k) * 64] = make_uint4(e.nl | (e.tok << 31), e.vl, e.nh, e.vh);
    }
    bool failed = s0.failed != 0 || cs.refused;
    const uint4 srv_rc = A.rec[A.nhdr];
    const uint32_t srv_info = A.info[A.nhdr];
    // a malformed conn_first cannot send the walk past the response array
    const uint32_t r1 = min(A.conn_first[c + 1], A.nres), r0 = min(A.conn_first[c], r1);
    hhuff_hpack_response_t R{};
    uint64_t base = 0, limit = 0;
    if (r0 < r1) {  // (res and out_off may be NULL when the call has no responses)
        R = A.res[r0];
        base = A.out_off[r0];
        limit = A.out_off[r0 + 1];
    }
    for (uint32_t r = r0; r < r1; ++r) {
        // the next response's record and region are in flight while this one is walked
        const uint32_t rn = r + 1 < r1 ? r + 1 : r;
        const hhuff_hpack_response_t Rn = A.res[rn];
        const uint64_t base_n = limit, limit_n = A.out_off[rn + 1];
        const bool trailers = (R.flags & HHUFF_RES_TRAILERS) != 0;
        const FrameRule F = frame_rule(R);
        const bool request = F.own;               // h2o_hpack_flatten_request / _push_promise
        const bool head = !trailers && !request;  // :status, server, content-length
        const bool server = head && (R.flags & HHUFF_RES_SERVER) && A.server_len != 0;
        const uint32_t h0 = R.hdr_first, h1 = R.hdr_first + R.nhdr;
        const uint32_t own_end = request ? h0 + R.status : h0;  // a request's own fields: method .. expect
        int32_t st = 0;
        if (failed) {
            st = cs.refused ? HHUFF_RES_EINVAL : HHUFF_RES_SKIPPED;
        } else if ((uint64_t)R.hdr_first + R.nhdr > A.nhdr || limit < base ||  // header range / region malformed
                   (head && (R.status < 100 || R.status > 999)) || (request && R.status > R.nhdr) ||
                   ((R.flags & HHUFF_RES_PUSH_PROMISE) && (R.flags & (HHUFF_RES_TRAILERS | HHUFF_RES_REQUEST))) ||
                   R.max_frame_size < 16384u ||
                   R.max_frame_size > 0xFFFFFFu || (server && (srv_info & kInfoBad))) {
            st = HHUFF_RES_EINVAL;
        }
        uint32_t pos = 0, su = ~0u, scode = 0, spos = 0, cll = 0;
        if (st == 0) {
            pos = F.lead;                       // a promise's stream id comes before the size update (:1116-1117)
            if (R.header_table_size < t.cap) {  // header_table_adjust_size (:839-856)
                t.cap = R.header_table_size;
                while (t.num != 0 && t.size > t.cap) t.evict_one();
                su = t.cap;
                pos += int_len(su, 5);
            }
            if (head) {
                const uint32_t s = R.status;  // encode_status (:437-466)
                pos += (s == 200 || s == 204 || s == 206 || s == 304 || s == 400 || s == 404 || s == 500) ? 1u : 5u;
            }
            if (server) {  // :1159-1163, encode_header_token(H2O_TOKEN_SERVER)
                uint32_t l;
                spos = pos;
                const FieldIn S{0u, 6u, A.server_off, A.server_len, srv_rc, srv_info};
                scode = hpe_field(A, t, S, kSrcConst, kSrcIn | A.server_off, l);
                pos += l;
            }
            FieldIn cur = h0 < h1 ? load_field(A, h0) : FieldIn{};
            for (uint32_t h = h0; h < h1; ++h) {
                const FieldIn nxt = h + 1 < h1 ? load_field(A, h + 1) : cur;  // in flight while this one is walked
                if (cur.info & kInfoBad) {  // a string past in_size: the response is refused (the table no longer
                    st = HHUFF_RES_EINVAL;  // matters: the connection fails with it)
                    break;
                }
                uint32_t l, code;
                const uint32_t fast = (cur.info >> kInfoFastShift) & 0xFFu;
                if (request && fast && (cur.info & kInfoTok) && ((cur.info & kInfoFastOwn) != 0) == (h < own_end)) {
                    code = kOpFast | fast << 11;  // encode_method / _scheme / _path, accept-encoding: no table
                    l = 1;
                } else {
                    code = hpe_field(A, t, cur, kSrcIn | cur.noff, kSrcIn | cur.voff, l);
                }
                const uint64_t dst = base + 9u + pos;
                A.op[h] = make_uint4((uint32_t)dst, (uint32_t)(dst >> 32), code, 0u);
                pos += l;
                cur = nxt;
            }
            if (head && R.content_length != ~0ull) {  // encode_content_length (:468-485)
                cll = 3u + digits(R.content_length);
                pos += cll;
            }
            const uint32_t M = R.max_frame_size;
            const uint64_t total = 9ull + pos + (pos > M ? 9ull * ((pos - 1u) / M) : 0ull);
            if (st == 0 && total > limit - base) st = HHUFF_RES_SPACE;
            if (st == 0) {
                A.out_len[r] = (uint32_t)total;
                A.headers_size[r] = pos;
                A.plan[2 * r] = make_uint4((uint32_t)base, (uint32_t)(base >> 32), pos, (uint32_t)total);
                A.plan[2 * r + 1] = make_uint4(su, server ? scode : kOpSkip, spos, cll);
                if (pos > M) A.big[1 + atomicAdd(A.big, 1u)] = r;
            }
        }
        if (st != 0) {
            A.out_len[r] = 0;
            A.headers_size[r] = 0;
            A.plan[2 * r + 1] = make_uint4(~0u, kOpSkip, 0u, 0u);
            A.plan[2 * r] = make_uint4(0u, 0u, 0u, 0u);
            if ((uint64_t)R.hdr_first + R.nhdr <= A.nhdr)  // a malformed range is not touched
                for (uint32_t h = h0; h < h1; ++h) A.op[h] = make_uint4(0u, 0u, kOpSkip, 0u);
            failed = true;
        }
        A.rstatus[r] = st;
        R = Rn;
        base = base_n;
        limit = limit_n;
    }
    if (!cs.refused) *ts = EncState{t.start, t.num, s0.ring, failed ? 1u : 0u, t.size, t.cap, 0u, 0u};
}

namespace {
__device__ void emit_field(const GlobalSource& src, uint8_t* dst, uint32_t code, uint32_t noff, uint32_t nl, uint32_t voff,
                           uint32_t vl, uint4 rc, const uint2* enc, const LongWork& L) {
    if (code & kOpFast) {
        *dst = (uint8_t)(code >> 11);
        return;
    }
    RegSink sink;
    sink.init(dst);
    const uint32_t kind = code & 3u, idx = (code >> 2) & 0x7Fu;
    switch (kind) {
        case kOpIndexed:
            sink_int(sink, 0x80u, idx, 7);
            sink.finish();
            return;
        case kOpIdxName: sink_int(sink, 0x40u, idx, 6); break;
        case kOpNever: sink_int(sink, 0x10u, idx, 4); break;
        default:
            sink.put1(0x40u);
            sink_string(sink, src, noff, nl, rc.z, enc, L);
            break;
    }
    if (code & kOpAsIs) {  // encode_as_is (:806-814)
        sink_int(sink, 0u, vl, 7);
        sink_payload(sink, src, voff, vl, false, 0u, enc, L);
    } else {
        sink_string(sink, src, voff, vl, rc.w, enc, L);
    }
    sink.finish();
}

__device__ __forceinline__ void put_frame_header(uint8_t* d, uint32_t len, uint32_t type, uint32_t flags, uint32_t sid) {
    d[0] = (uint8_t)(len >> 16);  // h2o_http2_encode_frame_header (lib/http2/frame.c:68-79)
    d[1] = (uint8_t)(len >> 8);
    d[2] = (uint8_t)len;
    d[3] = (uint8_t)type;
    d[4] = (uint8_t)flags;
    d[5] = (uint8_t)(sid >> 24);
    d[6] = (uint8_t)(sid >> 16);
    d[7] = (uint8_t)(sid >> 8);
    d[8] = (uint8_t)sid;
}
}  // namespace

// 3. emit: items 0 .. nhdr-1 are fields, nhdr .. nhdr+nres-1 response heads (frame header, a promise's
//    stream id, table size update, :status, server, and the content-length at the end)
__global__ __launch_bounds__(256) void hpe_emit_kernel(HpeArgs A) {
    __shared__ uint2 s_enc[256];
    s_enc[threadIdx.x] = make_uint2(g_enc_code[threadIdx.x], g_enc_nbits[threadIdx.x]);
    __syncthreads();
    const GlobalSource src{A.in, A.in_size};
    const uint64_t items = (uint64_t)A.nhdr + A.nres;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < items; i += (uint64_t)gridDim.x * 256u) {
        if (i < A.nhdr) {
            const uint4 o = A.op[i];
            if (o.z & kOpSkip) continue;
            const hhuff_hpack_header_t H = A.hdr[i];
            emit_field(src, A.out + ((uint64_t)o.y << 32 | o.x), o.z, H.name_off, H.name_len, H.value_off, H.value_len,
                       A.rec[i], s_enc, A.lw);
            continue;
        }
        const uint32_t r = (uint32_t)(i - A.nhdr);
        const uint4 p0 = A.plan[2 * r], p1 = A.plan[2 * r + 1];
        if (p0.w == 0) continue;  // failed
        const hhuff_hpack_response_t R = A.res[r];
        uint8_t* base = A.out + ((uint64_t)p0.y << 32 | p0.x);
        const FrameRule F = frame_rule(R);
        if (p0.z <= R.max_frame_size) put_frame_header(base, p0.z, F.type, 4u | F.flags, F.sid);  // else hpe_frames_kernel
        RegSink sink;
        sink.init(base + 9);
        if (F.lead) sink.put4(__builtin_bswap32(R.stream_id));  // the promised stream id (h2o_http2_encode32u, :1116)
        if (p1.x != ~0u) sink_int(sink, 0x20u, p1.x, 5);  // Dynamic Table Size Update (:852-853)
        if (!(R.flags & HHUFF_RES_TRAILERS) && !F.own) {
            const uint32_t s = R.status;  // encode_status (:437-466)
            const uint32_t c = s == 200 ? 8 : s == 204 ? 9 : s == 206 ? 10 : s == 304 ? 11 : s == 400 ? 12 : s == 404 ? 13 : s == 500 ? 14 : 0;
            if (c) {
                sink.put1(0x80u | c);
            } else {
                sink.put1(8u);
                sink.put1(3u);
                sink.put1('0' + s / 100);
                sink.put1('0' + s / 10 % 10);
                sink.put1('0' + s % 10);
            }
        }
        sink.finish();
        if (!(p1.y & kOpSkip))
            emit_field(src, base + 9 + p1.z, p1.y, 0u, 6u, A.server_off, A.server_len, A.rec[A.nhdr], s_enc, A.lw);
        if (p1.w) {  // encode_content_length (:468-485): literal without indexing, name index 28, raw digits
            uint8_t* d = base + 9 + p0.z - p1.w;
            d[0] = 0x0f;
            d[1] = 0x0d;
            d[2] = (uint8_t)(p1.w - 3u);
            uint64_t v = R.content_length;
            for (uint32_t k = p1.w - 1; k >= 3; --k) {
                d[k] = (uint8_t)('0' + v % 10);
                v /= 10;
            }
        }
    }
}

// 4. frames: one workgroup per listed response; chunk j (>= 1) of the payload moves up by 9 j bytes,
//    last chunk first and each chunk top-down through LDS, so no byte is overwritten before it is read
__global__ __launch_bounds__(256) void hpe_frames_kernel(HpeArgs A) {
    __shared__ uint8_t s_buf[8192];
    const uint32_t nbig = A.big[0];
    for (uint32_t b = blockIdx.x; b < nbig; b += gridDim.x) {
        const uint32_t r = A.big[1 + b];
        const uint4 p0 = A.plan[2 * r];
        const hhuff_hpack_response_t R = A.res[r];
        uint8_t* base = A.out + ((uint64_t)p0.y << 32 | p0.x);
        const FrameRule F = frame_rule(R);
        const uint32_t P = p0.z, M = R.max_frame_size;
        const uint32_t k = (P + M - 1u) / M;
        for (uint32_t j = k - 1; j >= 1; --j) {
            const uint64_t lo = 9ull + (uint64_t)j * M, hi = 9ull + min((uint64_t)(j + 1) * M, (uint64_t)P);
            const uint64_t shift = 9ull * j;
            for (uint64_t top = hi; top > lo;) {
                const uint64_t bot = top - lo > sizeof(s_buf) ? top - sizeof(s_buf) : lo;
                for (uint64_t q = bot + threadIdx.x; q < top; q += 256) s_buf[q - bot] = base[q];
                __syncthreads();
                for (uint64_t q = bot + threadIdx.x; q < top; q += 256) base[q + shift] = s_buf[q - bot];
                __syncthreads();
                top = bot;
            }
            if (threadIdx.x == 0) {
                const bool last = j == k - 1;
                put_frame_header(base + (uint64_t)j * (M + 9u), last ? (uint32_t)(hi - lo) : M, 9u, last ? 4u : 0u, F.sid);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) put_frame_header(base, M, F.type, F.flags, F.sid);
        __syncthreads();
    }
}

// 5. the table pass: one wave per connection writes its live entries' bytes, newest first, into the ring
//    they do not use now and points the entries there (as blk_table_kernel does for the decoder)
template <bool SLOTS>
__global__ __launch_bounds__(256) void hpe_ring_kernel(HpeArgs A) {
    const int lane = threadIdx.x & 63;
    const uint64_t c = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (c >= A.nconn) return;
    const ConnSlot cs = conn_slot<SLOTS>(A.cmap, c);
    if (cs.refused) return;
    const uint64_t base = cs.slot * kConnScratch;
    EncState* ts = reinterpret_cast<EncState*>(A.scratch + base);
    EncEntry* ent = reinterpret_cast<EncEntry*>(A.scratch + base + sizeof(EncState));
    const EncState s = *ts;
    const uint32_t nring = s.ring ^ 1u;
    const uint64_t rbase = base + sizeof(EncState) + kMaxEntries * sizeof(EncEntry) + (uint64_t)nring * kRing;
    uint32_t carry = 0;
    for (uint32_t k0 = 0; k0 < s.num; k0 += 64) {
        const uint32_t k = k0 + (uint32_t)lane;
        const bool live = k < s.num;
        const uint32_t i = (s.start + k) & (kMaxEntries - 1);
        EncEntry e{};
        if (live) e = ent[i];
        const uint32_t sz = live ? e.nl + e.vl : 0u;
        const uint32_t dst = carry + wave_excl_scan(sz, lane);
        carry += (uint32_t)__builtin_amdgcn_readlane((int)(dst - carry + sz), 63);
        uint8_t* d = A.scratch + rbase + dst;
        wave_copy64(hpe_src(A, e.nsrc), d, live ? e.nl : 0u, lane);
        wave_copy64(hpe_src(A, e.vsrc), d + e.nl, live ? e.vl : 0u, lane);
        if (live) {
            ent[i].nsrc = kSrcScr | (rbase + dst);
            ent[i].vsrc = kSrcScr | (rbase + dst + e.nl);
        }
    }
    if (lane == 0) ts->ring = nring;
}

uint64_t hpenc_conn_scratch() { return kConnScratch; }

hipError_t launch_long_bits(bool hash, const uint8_t* in, const hhuff_hpack_header_t* hdr, uint32_t nhdr, uint32_t server_off,
                            uint32_t server_len, uint4* rec, const LongWork& L, hipStream_t stream) {
    hipError_t e = hipSuccess;
    if (hash)
        HHUFF_LAUNCH(e, long_bits_kernel<true>, 256, 256, stream, in, hdr, nhdr, server_off, server_len, rec, L);
    else
        HHUFF_LAUNCH(e, long_bits_kernel<false>, 256, 256, stream, in, hdr, nhdr, server_off, server_len, rec, L);
    return e;
}

hipError_t launch_long_payload(const uint8_t* in, const LongWork& L, hipStream_t stream) {
    hipError_t e = hipSuccess;
    HHUFF_LAUNCH(e, long_payload_kernel, 512, 256, stream, in, L);
    return e;
}

namespace {
// the workspace of a call: its size with base = NULL, its pointers with the allocation
uint64_t hpe_carve(HpeArgs& A, uint64_t long_bits, uint64_t long_jobs, uint8_t* base) {
    Carve cv{base};
    const uint64_t nhdr = A.nhdr, nres = A.nres;
    A.rec = cv.take<uint4>(nhdr + 1);
    A.op = cv.take<uint4>(nhdr);
    A.plan = cv.take<uint4>(2 * nres);
    A.lw = long_ws(cv, long_bits, long_jobs);
    A.info = cv.take<uint32_t>(nhdr + 1);
    A.big = cv.take<uint32_t>(nres + 1);
    return cv.off;
}
}  // namespace

hipError_t launch_hpack_flatten(const HpeCall& call, hipStream_t stream) {
    if (call.nconn == 0) return hipSuccess;
    const uint32_t nhdr = call.nhdr, nres = call.nres, nconn = call.nconn;
    // long strings: bits of a header's name and value and of the server name; payload jobs of a field's name
    // and value and of a response head's server value
    const uint64_t long_bits = 2ull * nhdr + 2, long_jobs = 2ull * nhdr + 2ull * nres + 2;
    if (long_bits > 0xFFFFFFFFull || long_jobs > 0xFFFFFFFFull) return hipErrorInvalidValue;
    HpeArgs A{call, nullptr, nullptr, nullptr, nullptr, nullptr, LongWork{}};
    uint8_t* ws = nullptr;
    hipError_t e = work_alloc((void**)&ws, hpe_carve(A, long_bits, long_jobs, nullptr), stream);
    if (e != hipSuccess) return e;
    hpe_carve(A, long_bits, long_jobs, ws);
    e = hipMemsetAsync(A.big, 0, 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(A.lw.bits, 0, 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(A.lw.njobs, 0, 4, stream);
    const uint32_t gp = (uint32_t)std::min<uint64_t>((nhdr + 256ull) / 256u, 8192ull);
    const uint32_t ge = (uint32_t)std::min<uint64_t>(((uint64_t)nhdr + nres + 255u) / 256u, 16384ull);
    HHUFF_LAUNCH(e, hpe_prep_kernel, gp, 256, stream, A);
    if (e == hipSuccess) e = launch_long_bits(true, A.in, A.hdr, nhdr, A.server_off, A.server_len, A.rec, A.lw, stream);
    if (A.cmap)  // (the instantiations with and without connection slots, hhuff_slots.h)
        HHUFF_LAUNCH(e, hpe_table_kernel<true>, (nconn + 63u) / 64u, 64, stream, A);
    else
        HHUFF_LAUNCH(e, hpe_table_kernel<false>, (nconn + 63u) / 64u, 64, stream, A);
    if ((uint64_t)nhdr + nres != 0) HHUFF_LAUNCH(e, hpe_emit_kernel, ge, 256, stream, A);
    if (e == hipSuccess) e = launch_long_payload(A.in, A.lw, stream);
    if (nres != 0) HHUFF_LAUNCH(e, hpe_frames_kernel, std::min(nres, 512u), 256, stream, A);
    if (A.cmap)
        HHUFF_LAUNCH(e, hpe_ring_kernel<true>, (nconn + 3u) / 4u, 256, stream, A);
    else
        HHUFF_LAUNCH(e, hpe_ring_kernel<false>, (nconn + 3u) / 4u, 256, stream, A);
    const hipError_t f = hipFreeAsync(ws, stream);
    return e != hipSuccess ? e : f;
}
}  // namespace hhuff
