// QPACK decoding on the GPU (QPACK half): h2o's QPACK decoder, lib/http3/qpack.c.
//   encoder stream  h2o_qpack_decoder_handle_input (:420-485) -- insert with static / dynamic name
//                   reference (:289-348), insert with a literal name (:352-393), duplicate (:395-406),
//                   set dynamic table capacity (:408-418) -- into one dynamic table per connection
//                   (header_table_insert :166-190, header_table_evict :153-164)
//   field sections  h2o_qpack_parse_request's reading of a section (:830-858): parse_decode_context
//                   (:754-799), check_decode_context_blocked (:801-820), then decode_header (:652-752)
//                   field after field (resolve_static / resolve_dynamic / _postbase :506-557, literals
//                   :559-629)
//
// Decomposition.  Unlike HPACK, a QPACK field section never changes the dynamic table: only the encoder
// stream does.  A step runs as passes on the stream:
//   literal pre-pass       qpack_mark_kernel (one lane per encoder stream or section) marks every string
//                          literal -- instructions and field lines are readable without the table -- and
//                          the literal kernels decode them all, balanced across connections;
//   qpack_encoder_kernel   one lane per connection applies its encoder-stream instructions in order, on
//                          integers only: an entry is a pair of REFERENCES to where its name and value bytes
//                          are (a pre-decoded literal, the input, the static table, or an entry's ring);
//   qpack_table_kernel     one wave per connection whose table changed writes the live entries' bytes back
//                          to back into its other ring and points the entries there;
//   qpack_sections_kernel  one lane per field SECTION (many per connection) decodes it against that table,
//                          recording each field string's source; qpack_copy_kernel (one wave per section)
//                          moves the bytes into the arena.
// The table lives in per-connection scratch in HBM: an entry ring of header_table_size / 32 + 1 records
// {name source, value source, lengths, soft bits}, oldest first, absolute index = base_offset + position as
// in h2o (base_offset starts at 1, :143), and two byte rings of header_table_size bytes (live entries hold
// at most max_size <= header_table_size bytes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "hhuff_decwork.h"
#include "hhuff_device.h"
#include "hhuff_devtables.h"
#include "hhuff_image.h"
#include "hhuff.h"
#include "hhuff_int.h"
#include "hhuff_launch.h"
#include "hhuff_qpark.h"
#include "hhuff_request.h"
#include "hhuff_slots.h"

namespace hhuff {
namespace {
__device__ const uint8_t q_static_bytes[HHUFF_QSTATIC_NBYTES] = HHUFF_QSTATIC_BYTES_INIT;
__device__ const uint16_t q_static_ent[99 * 4] = HHUFF_QSTATIC_ENT_INIT;

constexpr uint32_t kQStaticCount = 99;  // h2o_qpack_static_table (include/h2o/token_table.h)
constexpr int32_t kDF = HHUFF_QPK_DECOMPRESSION_FAILED;
constexpr int32_t kQIncomplete = -1;       // H2O_HTTP3_ERROR_INCOMPLETE (http3_common.h:77)
constexpr int32_t kErrInvalidChar = -254;  // H2O_HTTP2_ERROR_INVALID_HEADER_CHAR
constexpr uint32_t kEntryOverhead = 32;    // HEADER_ENTRY_SIZE_OFFSET (qpack.c:32)
constexpr int64_t kQuicIntMax = 4611686018427387903LL;  // PTLS_QUICINT_MAX
}  // namespace

struct QpkArgs : QpdCall {  // the call, and what launch_qpack adds to it
    uint64_t conn_scratch;  // bytes of scratch per connection
    // pre-decoded encoder-stream literals (launch_qpack's pre-pass): bit p of lit_bits marks a literal whose
    // header starts at input byte p; word_pre[w] counts the marks before word w; literal r has the literal
    // kernels' results lit_len / lit_st, its bytes at lit_out + floor(8 payload / 5) (Huffman) or in the
    // input (raw).  NULL lit_bits: every literal is decoded in place.
    const uint32_t* lit_bits;
    const uint32_t* word_pre;
    const uint32_t* lit_len;
    const uint8_t* lit_st;
    const uint8_t* lit_pfx;  // the prefix literal r was decoded with
    const uint8_t* lit_out;
    // deferred section copies (with the pre-pass): per field slot, the address of its name's / value's
    // bytes (0: already in the arena); qpack_copy_kernel moves them.  NULL: the sections kernel copies.
    uint64_t* fsrc_n;
    uint64_t* fsrc_v;
};

// Byte sources of table entries and field strings: kind in the top 3 bits, offset below.  Every source stays
// valid until the call's last pass has run; between calls the entries' sources are all kQScr (their
// connection's ring in scratch), so a caller may keep scratch anywhere (offsets, not addresses).
constexpr uint64_t kQLit = 0;              // lit_out offset (a literal the pre-pass decoded, or decoded in place)
constexpr uint64_t kQStatic = 1ull << 61;  // static-table bytes
constexpr uint64_t kQScr = 2ull << 61;     // scratch offset (a ring: bytes an earlier call's table pass wrote)
constexpr uint64_t kQIn = 3ull << 61;      // input offset (a raw literal)
constexpr uint64_t kQOff = (1ull << 61) - 1;

__device__ __forceinline__ const uint8_t* q_src(const QpkArgs& A, uint64_t s) {
    const uint64_t o = s & kQOff;
    switch (s >> 61) {
        case 0: return A.lit_out + o;
        case 1: return q_static_bytes + o;
        case 2: return A.scratch + o;
        default: return A.in + o;
    }
}

// per-connection scratch: [QState 64 B][entry ring E x 32 B][ring 0][ring 1] (rings: T rounded up to 16 B).
// Live entries hold at most max_size <= T bytes, so the table pass (qpack_table_kernel) writes them back to
// back into the ring they do not use now, reading their sources from the other one.
struct QState {
    int64_t base_offset;
    uint64_t total_inserts, num_bytes, max_size;
    uint32_t start, num, ring, failed;  // ring: which ring holds the entries' bytes between calls
    uint32_t dirty, pad[3];             // dirty: entries inserted by this call (the table pass rewrites)
};
static_assert(sizeof(QState) == 64, "QState layout");
struct QEntry {  // one dynamic-table entry: references to its name and value bytes
    uint64_t nsrc, vsrc;
    uint32_t nl, vl, soft, pad;
};
static_assert(sizeof(QEntry) == 32, "QEntry layout");
// connection images (hhuff_image.h) restate the two records and the scratch source
static_assert(offsetof(QState, max_size) == offsetof(img::QdState, max_size) && offsetof(QState, start) == offsetof(img::QdState, start) &&
                  offsetof(QState, dirty) == offsetof(img::QdState, dirty) && offsetof(QEntry, vsrc) == offsetof(img::QdEntry, vsrc) &&
                  offsetof(QEntry, soft) == offsetof(img::QdEntry, soft) && kQScr == img::kQdScr && kQOff == img::kQdOff,
              "hhuff_image.h: QPACK_DEC slab");

__host__ __device__ __forceinline__ uint32_t qpk_ring_bytes(uint32_t T) { return ((T < 16u ? 16u : T) + 15u) & ~15u; }
__host__ __device__ __forceinline__ uint32_t qpk_entries(uint32_t T) { return T / kEntryOverhead + 1u; }

// decode_int (qpack.c:215-220): 0, kQIncomplete or kDF
__device__ __forceinline__ int32_t q_int(int64_t& v, const uint8_t* in, uint64_t& p, uint64_t end, uint32_t prefix) {
    v = hpack_int(in, p, end, prefix);
    if (v < 0) return v == kIntIncomplete ? kQIncomplete : kDF;
    return 0;
}

// h2o_hpack_validate_header_name (hpack.c:163-192): false on an upper-case letter, soft name bit otherwise
template <class Get>
__device__ bool q_valid_name(Get get, uint64_t n, uint32_t& soft) {
    bool bad = n == 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t c = get(i);
        if ((g_name_invalid[c >> 5] >> (c & 31)) & 1u) {
            if (c - 'A' < 26u) return false;
            bad = true;
        }
    }
    if (bad) soft |= 0x1u;
    return true;
}

// h2o_hpack_validate_header_value (hpack.c:194-221) with the whole-value rule (:110-115)
template <class Get>
__device__ void q_valid_value(Get get, uint64_t n, uint32_t& soft) {
    bool bad = false;
    if (n != 0) {
        const uint32_t f = get(0), l = get(n - 1);
        bad = f == ' ' || f == '\t' || l == ' ' || l == '\t';
    }
    for (uint64_t i = 0; !bad && i < n; ++i) {
        const uint32_t c = get(i);
        bad = ((g_value_invalid[c >> 5] >> (c & 31)) & 1u) != 0;
    }
    if (bad) soft |= 0x2u;
}

struct QTable {  // one connection's table, as the kernels see it
    QEntry* ent;
    uint32_t E;
    QState s;
    __device__ __forceinline__ uint32_t slot(uint32_t k) const {
        const uint32_t i = s.start + k;
        return i >= E ? i - E : i;
    }
    __device__ __forceinline__ QEntry get(uint32_t k) const { return ent[slot(k)]; }  // k-th oldest live entry
    __device__ __forceinline__ int64_t total() const { return s.base_offset + (int64_t)s.num; }  // :321-324
    __device__ __forceinline__ bool resolve_abs(int64_t index, QEntry& e) const {  // resolve_dynamic_abs :201-213
        if (index < s.base_offset || index - s.base_offset >= (int64_t)s.num) return false;
        e = get((uint32_t)(index - s.base_offset));
        return true;
    }
    __device__ void evict(uint64_t delta) {  // header_table_evict (:153-164)
        while (s.num != 0 && s.num_bytes + delta > s.max_size) {
            const uint2 l = *reinterpret_cast<const uint2*>(&ent[s.start].nl);
            s.num_bytes -= (uint64_t)l.x + l.y + kEntryOverhead;
            s.start = s.start + 1 == E ? 0u : s.start + 1;
            --s.num;
            ++s.base_offset;
        }
    }
    // header_table_insert (:166-190): the entry's bytes are references; the table pass writes them
    __device__ void commit(const QEntry& e) {
        const uint64_t add = (uint64_t)e.nl + e.vl + kEntryOverhead;
        evict(add);
        ent[slot(s.num)] = e;
        ++s.num;
        s.num_bytes += add;
        ++s.total_inserts;
        s.dirty = 1;
    }
};

// pre-pass literal marks (qpack_mark_kernel): names are the 5-bit-prefix literals (encoder stream) and the
// 3-bit-prefix ones (sections, also in p3_bits); everything else is a value (7-bit prefix)
// the pre-decoded literal whose header is at input byte p, or -1: not marked, decoded with another prefix
// (input regions that overlap), or a verdict other than success (the in-place path then reproduces the
// reference's exact failure)
__device__ __forceinline__ int64_t q_pre(const QpkArgs& A, uint64_t p, uint32_t prefix) {
    const uint32_t w = A.lit_bits[p >> 5], m = 1u << (p & 31);
    if (!(w & m)) return -1;
    const uint32_t r = A.word_pre[p >> 5] + (uint32_t)__builtin_popcount(w & (m - 1u));
    return ((A.lit_st[r] >> 2) & 7u) == 0 && A.lit_pfx[r] == prefix ? (int64_t)r : -1;
}

// An encoder-stream string literal (H flag at bit `prefix`, length, payload at p after the header): its
// source and length.  Pre-decoded (pre >= 0): the pre-pass results.  Otherwise decoded here -- a Huffman
// payload into lit_out at the place the pre-pass would have used (floor(8 p / 5)), a raw one validated
// and referenced in the input -- with the reference's verdicts (qpack.c:222-237, :362-378).
__device__ bool q_enc_string(const QpkArgs& A, bool huff, bool is_name, uint64_t p, uint64_t n, int64_t pre,
                             uint64_t& src, uint32_t& len, uint32_t& soft, const DecTables& T) {
    if (pre >= 0) {
        len = A.lit_len[pre];
        soft |= A.lit_st[pre] & 3u;
        src = huff ? kQLit | ((p * 8u) / 5u) : kQIn | p;
        return true;
    }
    if (huff) {
        if (n > kMaxStrLen) return false;
        RegSinkFL sk;
        sk.init(const_cast<uint8_t*>(A.lit_out) + (p * 8u) / 5u);
        sk.first = sk.last = 0;
        const DecResult d = decode_core(GlobalSource{A.in, A.in_size}, (uint32_t)p, (uint32_t)n, sk, T);
        if (!d.ok) return false;
        sk.finish();
        soft |= soft_bits(is_name, d.len, d.flags, sk.first, sk.last);
        len = d.len;
        src = kQLit | ((p * 8u) / 5u);
        return true;
    }
    const uint8_t* s = A.in + p;
    if (is_name) {
        if (!q_valid_name([&](uint64_t i) { return (uint32_t)s[i]; }, n, soft)) return false;
    } else {
        q_valid_value([&](uint64_t i) { return (uint32_t)s[i]; }, n, soft);
    }
    len = (uint32_t)n;
    src = kQIn | p;
    return true;
}

// the value half of an insert (decode_value_and_insert :273-287)
__device__ int32_t q_value_and_insert(QTable& t, const QpkArgs& A, QEntry e, bool vhuff, uint64_t vp, uint64_t vlen,
                                      int64_t pre, const DecTables& T) {
    if (!q_enc_string(A, vhuff, false, vp, vlen, pre, e.vsrc, e.vl, e.soft, T)) return kDF;
    if ((uint64_t)e.nl + e.vl + kEntryOverhead > t.s.max_size) return kDF;  // header exceeds table size (:278-281)
    t.commit(e);
    return 0;
}

// h2o_qpack_decoder_handle_input (qpack.c:420-485) over in[p, end)
__device__ int32_t q_handle_input(QTable& t, const QpkArgs& A, uint64_t p, uint64_t end, uint32_t& consumed,
                                  uint64_t& insert_count, const DecTables& T) {
    const uint8_t* in = A.in;
    const uint64_t p0 = p;
    uint64_t done = p;
    const uint64_t old_total = t.s.total_inserts;
    int32_t ret = 0;
    insert_count = 0;
    while (p != end && ret == 0) {
        const uint32_t b = in[p];
        switch (b >> 5) {
            default: {  // insert with name reference (:430-444)
                int64_t name_index, value_len;
                const bool name_is_static = (b & 0x40u) != 0;
                if ((ret = q_int(name_index, in, p, end, 6)) != 0) goto Exit;
                if (p == end) goto Exit;
                const int64_t vpre = q_pre(A, p, 7);
                const bool vhuff = (in[p] & 0x80u) != 0;
                if ((ret = q_int(value_len, in, p, end, 7)) != 0) goto Exit;
                if (!((uint64_t)value_len <= end - p)) goto Exit;
                QEntry e{};
                if (name_is_static) {  // insert_token_header (:289-300): soft starts at 0
                    if ((uint64_t)name_index >= kQStaticCount) {
                        ret = kDF;
                    } else {
                        const uint32_t k = 4u * (uint32_t)name_index;
                        e.nsrc = kQStatic | q_static_ent[k];
                        e.nl = q_static_ent[k + 1];
                        ret = q_value_and_insert(t, A, e, vhuff, p, (uint64_t)value_len, vpre, T);
                    }
                } else {  // dynamic (:335-348): token names carry no name bit, literal names keep theirs
                    const int64_t base_index = t.total() - 1;
                    QEntry r;
                    if (name_index > base_index || !t.resolve_abs(base_index - name_index, r)) {
                        ret = kDF;
                    } else {
                        e.nsrc = r.nsrc;
                        e.nl = r.nl;
                        e.soft = r.soft & 0x1u;
                        ret = q_value_and_insert(t, A, e, vhuff, p, (uint64_t)value_len, vpre, T);
                    }
                }
                p += (uint64_t)value_len;
            } break;
            case 2:
            case 3: {  // insert without name reference (:446-462, :352-393)
                int64_t name_len, value_len;
                const bool nhuff = (b & 0x20u) != 0;
                const int64_t npre = q_pre(A, p, 5);
                if ((ret = q_int(name_len, in, p, end, 5)) != 0) goto Exit;
                if (!((uint64_t)name_len < end - p)) goto Exit;
                const uint64_t qn = p;
                p += (uint64_t)name_len;
                const int64_t vpre = q_pre(A, p, 7);
                const bool vhuff = (in[p] & 0x80u) != 0;
                if ((ret = q_int(value_len, in, p, end, 7)) != 0) goto Exit;
                if (!((uint64_t)value_len <= end - p)) goto Exit;
                QEntry e{};
                if (!q_enc_string(A, nhuff, true, qn, (uint64_t)name_len, npre, e.nsrc, e.nl, e.soft, T)) {
                    ret = kDF;
                } else {
                    // a name h2o_lookup_token knows goes in as a token header with soft bits 0 (:383-384)
                    if (e.soft && pseudo_token(q_src(A, e.nsrc), e.nl)) e.soft = 0;
                    ret = q_value_and_insert(t, A, e, vhuff, p, (uint64_t)value_len, vpre, T);
                }
                p += (uint64_t)value_len;
            } break;
            case 0: {  // duplicate (:463-468, :395-406)
                int64_t index;
                if ((ret = q_int(index, in, p, end, 5)) != 0) goto Exit;
                if (index >= (int64_t)t.s.num)
                    ret = kDF;
                else
                    t.commit(t.get(t.s.num - 1u - (uint32_t)index));
            } break;
            case 1: {  // set dynamic table capacity (:469-474, :408-418)
                int64_t max_size;
                if ((ret = q_int(max_size, in, p, end, 5)) != 0) goto Exit;
                if (max_size > (int64_t)A.T) {
                    ret = kDF;
                } else {
                    t.s.max_size = (uint64_t)max_size;
                    t.evict(0);
                }
            } break;
        }
        done = p;
    }
Exit:
    if (ret == kQIncomplete) ret = 0;
    if (ret == 0 && old_total != t.s.total_inserts) insert_count = t.s.total_inserts;
    consumed = (uint32_t)(done - p0);
    return ret;
}

__device__ __forceinline__ QTable q_table(const QpkArgs& A, uint64_t slot) {  // the table in slab `slot`
    uint8_t* scr = A.scratch + slot * A.conn_scratch;
    QTable t{reinterpret_cast<QEntry*>(scr + sizeof(QState)), qpk_entries(A.T), {}};
    t.s = *reinterpret_cast<const QState*>(scr);
    return t;
}

// one connection's encoder stream (cs: its slab, by the call's map or by the connection's own number)
__device__ __forceinline__ void q_encoder_conn(const QpkArgs& A, uint64_t c, const ConnSlot cs, const DecTables& T) {
    if (cs.refused) {  // no slab of its own: nothing of its encoder stream is taken
        A.enc_status[c] = HHUFF_QPK_EINVAL;
        A.enc_consumed[c] = 0;
        A.insert_count[c] = 0;
        return;
    }
    QState* ps = reinterpret_cast<QState*>(A.scratch + cs.slot * A.conn_scratch);
    if (!(A.flags & HHUFF_QPK_CONTINUE) || cs.reset) {  // h2o_qpack_create_decoder (:240-252)
        QState s0{};
        s0.base_offset = 1;
        s0.max_size = A.T;
        *ps = s0;
    }
    QTable t = q_table(A, cs.slot);
    t.s.dirty = 0;
    int32_t st = 0;
    uint32_t consumed = 0;
    uint64_t ic = 0;
    if (t.s.failed) {
        st = HHUFF_QPK_SKIPPED;
    } else if (A.enc_len[c]) {
        const uint64_t p = A.enc_off[c];
        st = q_handle_input(t, A, p, p + A.enc_len[c], consumed, ic, T);
        t.s.failed = st != 0;
    }
    A.enc_status[c] = st;
    A.enc_consumed[c] = consumed;
    A.insert_count[c] = ic;
    *ps = t.s;
}

template <bool SLOTS>
__global__ __launch_bounds__(256) void qpack_encoder_kernel(QpkArgs A) {
    __shared__ __attribute__((aligned(16))) uint32_t s_lut[1u << HHUFF_LUT_BITS];
    __shared__ uint32_t s_kinfo[32];
    __shared__ uint32_t s_ones[HHUFF_ONES_NENT];
    load_dec_tables(s_lut, s_kinfo, s_ones, blockDim.x);
    __syncthreads();
    DecTables T;  // assigned, not brace-initialised (see hhuff_blocks.hip)
    T.lut = s_lut;
    T.kinfo = s_kinfo;
    T.ones = s_ones;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < A.nconn; c += (uint64_t)gridDim.x * blockDim.x)
        q_encoder_conn(A, c, conn_slot<SLOTS>(A.cmap, c), T);
}

// ---- decoder sessions (include/hhuff.h (2e'''), hhuff_qpark.h) ----
struct QdsArgs {  // hhuff_qpack_dsessions_t as the kernels see it
    uint8_t* state;
    uint64_t slab;  // bytes of a session
    uint32_t cap;   // max_blocked: entries of a session's list
    uint32_t flags;
    const uint32_t* cancel_first;
    const uint64_t* cancel_id;
    const uint8_t* cancel_flags;
    uint8_t* dec_out;
    const uint64_t* dec_out_off;
    uint32_t* dec_out_len;
    uint64_t* wake_id;
    const uint32_t* wake_first;
    uint32_t *nwake, *parked;
    uint8_t* dflags;
    uint32_t* map;       // the step's connection map: written by the encoder-stream pass, read by the others
    const uint32_t* given;  // the slot map of the call (hhuff_slots.h); NULL: connection c in slot c
};

// The encoder-stream pass of a session step.  It settles first which connections the step refuses -- a dec_out
// region under the bound for the connection's own sections and cancellations, a cancel_first that decreases --
// and writes the verdict into the step's connection map, so every later pass sees such a connection as one the
// slot map refused and forms no address in its table or session.
__global__ __launch_bounds__(256) void qpack_encoder_ds_kernel(QpkArgs A, QdsArgs D) {
    __shared__ __attribute__((aligned(16))) uint32_t s_lut[1u << HHUFF_LUT_BITS];
    __shared__ uint32_t s_kinfo[32];
    __shared__ uint32_t s_ones[HHUFF_ONES_NENT];
    load_dec_tables(s_lut, s_kinfo, s_ones, blockDim.x);
    __syncthreads();
    DecTables T;  // assigned, not brace-initialised (see hhuff_blocks.hip)
    T.lut = s_lut;
    T.kinfo = s_kinfo;
    T.ones = s_ones;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < A.nconn; c += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t m = D.given ? D.given[c] : (uint32_t)c;
        if (m != kConnRefused) {
            const uint32_t k0 = A.conn_first[c], k1 = A.conn_first[c + 1];
            const uint32_t x0 = D.cancel_first ? D.cancel_first[c] : 0u, x1 = D.cancel_first ? D.cancel_first[c + 1] : 0u;
            const uint64_t o0 = D.dec_out_off[c], o1 = D.dec_out_off[c + 1];
            if (x1 < x0 || k1 < k0 || o1 < o0 || o1 - o0 < qp_out_bound((uint64_t)k1 - k0, (uint64_t)x1 - x0)) m = kConnRefused;
        }
        D.map[c] = m;
        q_encoder_conn(A, c, conn_slot_of(m), T);
    }
}

// The session pass, in place of qpack_blocked_kernel: one lane per connection walks its sections (point 1), its
// cancellations (2), its list (3: wake) and writes the Insert Count Increment (4).
__global__ __launch_bounds__(256) void qpack_dsession_kernel(QpkArgs A, QdsArgs D) {
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < A.nconn; c += (uint64_t)gridDim.x * blockDim.x) {
        const ConnSlot cs = conn_slot_of(D.map[c]);
        uint32_t out_n = 0, nw = 0, np = 0, df = 0;
        if (!cs.refused) {
            QpHead* h = reinterpret_cast<QpHead*>(D.state + cs.slot * D.slab);
            QpEntry* ent = reinterpret_cast<QpEntry*>(h + 1);
            const QState* ps = reinterpret_cast<const QState*>(A.scratch + cs.slot * A.conn_scratch);
            const bool fresh = !(A.flags & HHUFF_QPK_CONTINUE) || cs.reset;
            uint32_t n = fresh ? 0u : min(h->parked, D.cap);
            uint64_t krc = fresh ? 0u : h->known_received;
            if (!ps->failed) {
                const uint64_t total = ps->total_inserts;
                uint8_t* out = D.dec_out + D.dec_out_off[c];
                const uint64_t room = D.dec_out_off[c + 1] - D.dec_out_off[c];
                auto put = [&](const uint8_t* b, uint32_t len) {  // an instruction, whole or not at all
                    if ((uint64_t)out_n + len > room) return;
                    for (uint32_t i = 0; i < len; ++i) out[out_n + i] = b[i];
                    out_n += len;
                };
                uint8_t tmp[16];
                for (uint32_t k = A.conn_first[c]; k < A.conn_first[c + 1]; ++k) {  // 1
                    const int32_t st = A.sstatus[k];
                    if (st == HHUFF_QPK_SKIPPED || st == HHUFF_QPK_EINVAL) continue;
                    const uint64_t id = A.stream_id[k];
                    const uint32_t i = qp_find(ent, n, id);
                    if (st == HHUFF_QPK_BLOCKED) {
                        if (i == n && !qp_park(ent, n, D.cap, id, A.req_insert_count[k])) A.sstatus[k] = kDF;
                        continue;
                    }
                    if (i != n) qp_remove(ent, n, i);
                    const uint32_t al = A.qreq ? A.qreq[k].ack_len : A.qres[k].ack_len;
                    if (al == 0) continue;
                    const uint8_t* ab = A.qreq ? A.qreq[k].ack : A.qres[k].ack;
                    const uint32_t len = min(al, 16u);
                    for (uint32_t j = 0; j < len; ++j) tmp[j] = ab[j];
                    put(tmp, len);
                    krc = qp_acknowledged(krc, A.req_insert_count[k]);
                }
                if (D.cancel_first) {  // 2
                    for (uint32_t x = D.cancel_first[c]; x < D.cancel_first[c + 1]; ++x) {
                        const uint64_t id = D.cancel_id[x];
                        const uint32_t i = qp_find(ent, n, id);
                        if (i != n) qp_remove(ent, n, i);
                        if (D.cancel_flags && (D.cancel_flags[x] & HHUFF_QDS_SILENT)) continue;
                        put(tmp, qp_put_int(tmp, 0x40u, id, 6));
                    }
                }
                const uint32_t w0 = D.wake_first[c], w1 = D.wake_first[c + 1];  // 3
                bool pending = false;
                nw = qp_wake(ent, n, total, D.wake_id + w0, w1 > w0 ? w1 - w0 : 0u, pending);
                df = pending ? HHUFF_QDS_WAKE_PENDING : 0u;
                if (D.flags & HHUFF_QDS_SYNC) {  // 4
                    const uint64_t inc = qp_increment(total, krc);
                    if (inc) {
                        put(tmp, qp_put_int(tmp, 0x00u, inc, 6));
                        krc = total;
                    }
                }
            }
            h->parked = n;
            h->pad = 0;
            h->known_received = krc;
            np = n;
        }
        D.dec_out_len[c] = out_n;
        D.nwake[c] = nw;
        D.parked[c] = np;
        D.dflags[c] = (uint8_t)df;
    }
}

// Table pass: one wave per connection whose table took entries this call writes the live entries' bytes,
// oldest first, back to back into the ring they do not use now and points the entries there; the field
// sections (and the next call, HHUFF_QPK_CONTINUE) read only scratch.
template <bool SLOTS>
__global__ __launch_bounds__(256) void qpack_table_kernel(QpkArgs A) {
    const int lane = threadIdx.x & 63;
    const uint64_t c = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (c >= A.nconn) return;
    const ConnSlot cs = conn_slot<SLOTS>(A.cmap, c);
    if (cs.refused) return;
    const uint64_t base = cs.slot * A.conn_scratch;
    QState* ps = reinterpret_cast<QState*>(A.scratch + base);
    const QState s = *ps;
    if (!s.dirty) return;
    const uint32_t E = qpk_entries(A.T);
    QEntry* ent = reinterpret_cast<QEntry*>(A.scratch + base + sizeof(QState));
    const uint32_t nring = s.ring ^ 1u;
    const uint64_t rbase = base + sizeof(QState) + (uint64_t)E * sizeof(QEntry) + nring * (uint64_t)qpk_ring_bytes(A.T);
    wave_table_pass(A.scratch, ent, E, s.start, s.num, rbase, kQScr, lane, [&](uint64_t x) { return q_src(A, x); });
    if (lane == 0) ps->ring = nring;
}

// ---- field sections ----

struct QCtx {
    int64_t ric, base;
};

// parse_decode_context (qpack.c:754-799)
__device__ int32_t q_parse_context(const QTable& t, uint32_t max_entries, QCtx& ctx, const uint8_t* in, uint64_t& p,
                                   uint64_t end) {
    int64_t ric, delta;
    if (q_int(ric, in, p, end, 8) != 0) return kDF;
    if (ric > 0) {
        if (max_entries == 0) return kDF;
        const uint32_t full_range = 2 * max_entries;
        const uint64_t max_value = t.s.total_inserts + max_entries;
        const uint64_t rounded = max_value / full_range * full_range;
        ric = (int64_t)((uint64_t)ric + rounded - 1);
        if ((uint64_t)ric > max_value) {
            if (ric <= (int64_t)full_range) return kDF;
            ric -= full_range;
        }
        if (ric == 0) return kDF;
        if (ric > kQuicIntMax) return kDF;
    }
    ctx.ric = ric;
    if (p >= end) return kDF;
    const bool sign = (in[p] & 0x80u) != 0;
    if (q_int(delta, in, p, end, 7) != 0) return kDF;
    if (delta > kQuicIntMax) return kDF;
    ctx.base = sign ? ric - delta - 1 : ric + delta;
    if (ctx.base < 0) return kDF;
    return 0;
}

// resolve_dynamic / resolve_dynamic_postbase (qpack.c:523-557)
__device__ bool q_dyn(const QTable& t, const QCtx& ctx, const uint8_t* in, uint64_t& p, uint64_t end, uint32_t prefix,
                      bool postbase, QEntry& e) {
    int64_t off, index;
    if (q_int(off, in, p, end, prefix) != 0) return false;
    if (postbase) {
        if (off > INT64_MAX - ctx.base - 1) return false;
        index = ctx.base + off + 1;
    } else {
        if (off >= ctx.base) return false;
        index = ctx.base - off;
    }
    if (ctx.ric < index) return false;
    return t.resolve_abs(index, e);
}

struct QArena {
    uint8_t* a;
    uint64_t cur, end;
};

// a field string's n bytes at source `src` go to arena[off, off + n): qpack_copy_kernel moves them
// (fs = their address)
__device__ __forceinline__ int32_t q_copy(const QpkArgs& A, QArena& R, uint64_t src, uint32_t n, uint32_t& off,
                                          uint64_t& fs) {
    if (R.cur + n > R.end) return HHUFF_QPK_ARENA;
    off = (uint32_t)R.cur;
    fs = (uint64_t)(uintptr_t)q_src(A, src);
    R.cur += n;
    return 0;
}

// decode_header_value_literal (qpack.c:603-629) / decode_header_name_literal (:559-601, prefix 3)
__device__ int32_t q_literal(const QpkArgs& A, QArena& R, uint32_t& soft, uint64_t& p, uint64_t end, bool is_name,
                             uint32_t& off, uint32_t& len, uint64_t& fs, const DecTables& T) {
    const uint8_t* in = A.in;
    if (!is_name && !(p < end)) return kDF;
    const uint32_t prefix = is_name ? 3u : 7u;
    const bool huff = ((in[p] >> prefix) & 1u) != 0;
    const int64_t pre = q_pre(A, p, prefix);
    int64_t n;
    if (q_int(n, in, p, end, prefix) != 0) return kDF;
    if ((int64_t)(end - p) < n) return kDF;
    fs = 0;
    if (pre >= 0) {  // decoded and validated by the pre-pass; the reference's order of checks holds
        if (R.cur + (huff ? ((uint64_t)n * 8u) / 5u : (uint64_t)n) > R.end) return HHUFF_QPK_ARENA;
        len = A.lit_len[pre];
        soft |= A.lit_st[pre] & 3u;
        off = (uint32_t)R.cur;
        fs = (uint64_t)(uintptr_t)(huff ? A.lit_out + (p * 8u) / 5u : in + p);
        R.cur += len;
        p += (uint64_t)n;
        return 0;
    }
    if (huff) {
        if (R.cur + ((uint64_t)n * 8u) / 5u > R.end) return HHUFF_QPK_ARENA;
        if ((uint64_t)n > kMaxStrLen) return kDF;
        RegSinkFL sk;
        sk.init(R.a + R.cur);
        sk.first = sk.last = 0;
        const DecResult d = decode_core(GlobalSource{A.in, A.in_size}, (uint32_t)p, (uint32_t)n, sk, T);
        if (!d.ok) return kDF;
        sk.finish();
        soft |= soft_bits(is_name, d.len, d.flags, sk.first, sk.last);
        len = d.len;
    } else {
        const uint8_t* src = in + p;
        auto get = [&](uint64_t i) { return (uint32_t)src[i]; };
        if (is_name) {  // tokens are taken as they are; anything else is validated (:583-588)
            if (!pseudo_token(src, (uint32_t)n) && !q_valid_name(get, (uint64_t)n, soft)) return kDF;  // (n < 2^32: u32 offsets)
        } else {
            q_valid_value(get, (uint64_t)n, soft);
        }
        if (R.cur + (uint64_t)n > R.end) return HHUFF_QPK_ARENA;
        uint8_t* d = R.a + R.cur;
        copy16([&](uint32_t i) { return src[i]; }, [&](uint32_t i, uint8_t v) { d[i] = v; }, (uint32_t)n);
        len = (uint32_t)n;
    }
    off = (uint32_t)R.cur;
    R.cur += len;
    p += (uint64_t)n;
    return 0;
}

// decode_header (qpack.c:652-752): 0 / kErrInvalidChar = a field was produced
__device__ int32_t q_field(const QpkArgs& A, const QTable& t, const QCtx& ctx, uint64_t& p, uint64_t end, QArena& R,
                           uint32_t& noff, uint32_t& nlen, uint32_t& voff, uint32_t& vlen, uint32_t& soft_out,
                           uint64_t& fn, uint64_t& fv, const DecTables& T) {
    const uint8_t* in = A.in;
    uint32_t soft = 0;
    int32_t r;
    QEntry e;
    const uint32_t kind = in[p] >> 4;
    switch (kind) {
        case 12:
        case 13:
        case 14:
        case 15: {  // indexed field line, static (:659-669)
            int64_t si;
            if (q_int(si, in, p, end, 6) != 0 || (uint64_t)si >= kQStaticCount) return kDF;
            const uint32_t k = 4u * (uint32_t)si;
            nlen = q_static_ent[k + 1];
            if ((r = q_copy(A, R, kQStatic | q_static_ent[k], nlen, noff, fn)) != 0) return r;
            vlen = q_static_ent[k + 3];
            if ((r = q_copy(A, R, kQStatic | q_static_ent[k + 2], vlen, voff, fv)) != 0) return r;
        } break;
        case 8:
        case 9:
        case 10:
        case 11:  // indexed field line, dynamic (:670-682)
        case 1:   // indexed field line, post-base (:713-722)
            if (!q_dyn(t, ctx, in, p, end, kind == 1 ? 4u : 6u, kind == 1, e)) return kDF;
            if ((r = q_copy(A, R, e.nsrc, e.nl, noff, fn)) != 0) return r;
            if ((r = q_copy(A, R, e.vsrc, e.vl, voff, fv)) != 0) return r;
            nlen = e.nl;
            vlen = e.vl;
            soft = e.soft;
            break;
        case 5:
        case 7: {  // literal field line, static name reference (:683-692)
            int64_t si;
            if (q_int(si, in, p, end, 4) != 0 || (uint64_t)si >= kQStaticCount) return kDF;
            const uint32_t k = 4u * (uint32_t)si;
            nlen = q_static_ent[k + 1];
            if ((r = q_copy(A, R, kQStatic | q_static_ent[k], nlen, noff, fn)) != 0) return r;
            if ((r = q_literal(A, R, soft, p, end, false, voff, vlen, fv, T)) != 0) return r;
        } break;
        case 4:
        case 6:  // literal field line, dynamic name reference (:693-704)
        case 0:  // literal field line, post-base name reference (:723-733)
            if (!q_dyn(t, ctx, in, p, end, kind == 0 ? 3u : 4u, kind == 0, e)) return kDF;
            if ((r = q_copy(A, R, e.nsrc, e.nl, noff, fn)) != 0) return r;
            nlen = e.nl;
            soft = e.soft & 0x1u;
            if ((r = q_literal(A, R, soft, p, end, false, voff, vlen, fv, T)) != 0) return r;
            break;
        default:  // 2, 3: literal field line with a literal name (:705-712)
            if ((r = q_literal(A, R, soft, p, end, true, noff, nlen, fn, T)) != 0) return r;
            if ((r = q_literal(A, R, soft, p, end, false, voff, vlen, fv, T)) != 0) return r;
            break;
    }
    soft_out = soft;
    return soft ? kErrInvalidChar : 0;
}

// h2o_hpack_encode_int (hpack.c:757-772) of v with a 7-bit prefix behind 0x80: send_header_ack (qpack.c:642-649)
__device__ __forceinline__ uint32_t q_header_ack(uint64_t v, uint8_t* out) {
    uint32_t n = 0;
    if (v < 127u) {
        out[n++] = (uint8_t)(0x80u | v);
        return n;
    }
    out[n++] = 0xFFu;
    v -= 127u;
    while (v >= 128u) {
        out[n++] = (uint8_t)(0x80u | (v & 0x7Fu));
        v >>= 7;
    }
    out[n++] = (uint8_t)v;
    return n;
}

__device__ __forceinline__ void q_req_store(hhuff_qpack_request_t* out, const ReqState& r, int32_t st, uint64_t ric,
                                            uint64_t stream_id) {
    req_store(&out->req, r);
    out->datagram_flow_id = r.dfid;
    uint8_t ack[16] = {};
    const uint32_t n = ((st == 0 || st == kErrInvalidChar) && ric != 0) ? q_header_ack(stream_id, ack) : 0u;
    out->ack_len = n;
    uint2* a2 = reinterpret_cast<uint2*>(out->ack);  // 8-byte aligned records: two 8-byte stores
    uint32_t w[4];
    __builtin_memcpy(w, ack, 16);
    a2[0] = make_uint2(w[0], w[1]);
    a2[1] = make_uint2(w[2], w[3]);
}

// The HTTP/3 rules as a call of their own: inlined into the sections kernel (11K instructions, SGPRs spilled
// to VGPR lanes), the compiler lost the err_desc code of a rejected connection-specific field on gfx950
// (the request record said 0 where h2o says h2o_hpack_err_unexpected_connection_specific_header), while the
// same source compiled for the host, and inlined into the HPACK walk, is right.  The rules' source is clean
// under ASan + UBSan on the host and equal to the oracle field for field (tests/rules_host.cpp); A/B builds
// with -DHHUFF_H3_INLINE inline them again (tests/test_rules_host.py documents the GPU result).
#ifdef HHUFF_H3_INLINE
#define HHUFF_H3_CALL __forceinline__
#else
#define HHUFF_H3_CALL __noinline__
#endif
__device__ HHUFF_H3_CALL int32_t req_field_h3(ReqState& r, uint32_t cls, const uint8_t* value, uint32_t vl, uint32_t soft,
                                             int32_t k, bool& header) {
    return req_field<true>(r, cls, value, vl, soft, k, header);
}

__device__ HHUFF_H3_CALL int32_t resp_field_h3(RespState& r, uint32_t cls, const uint8_t* value, uint32_t vl, uint32_t soft,
                                              int32_t k, bool& header) {
    return resp_field<true>(r, cls, value, vl, soft, k, header);
}

// h2o_qpack_parse_response's record: the Section Acknowledgment only after a clean parse (qpack.c:876-881)
__device__ __forceinline__ void q_res_store(hhuff_qpack_response_head_t* out, const RespState& r, int32_t st, uint64_t ric,
                                            uint64_t stream_id) {
    resp_store(&out->res, r);
    uint8_t ack[16] = {};
    const uint32_t n = (st == 0 && ric != 0) ? q_header_ack(stream_id, ack) : 0u;
    out->ack_len = n;
    out->reserved = 0u;
    uint2* a2 = reinterpret_cast<uint2*>(out->ack);
    uint32_t w[4];
    __builtin_memcpy(w, ack, 16);
    a2[0] = make_uint2(w[0], w[1]);
    a2[1] = make_uint2(w[2], w[3]);
}

constexpr int kSecPlain = 0, kSecReq = 1, kSecResp = 2;  // qpack_sections_kernel modes

// REQ: h2o_qpack_parse_request (qpack.c:830-858) -- each field also runs h2o_hpack_parse_request's rules
// (hhuff_request.h, the HTTP/3 arguments of lib/http3/server.c:1540-1545), a rule's hard error is
// normalised to DECOMPRESSION_FAILED (:852-853), and the record gets the Section Acknowledgment (:856).
// RESP: h2o_qpack_parse_response (:860-882) as lib/common/http3client.c:542 calls it -- a response head,
// h2o_hpack_parse_response's rules (a status and a datagram-flow-id out-parameter), the same normalisation
template <int MODE, bool SLOTS>
__global__ __launch_bounds__(256) void qpack_sections_kernel(QpkArgs A) {
    constexpr bool REQ = MODE == kSecReq, RESP = MODE == kSecResp;
    __shared__ __attribute__((aligned(16))) uint32_t s_lut[1u << HHUFF_LUT_BITS];
    __shared__ uint32_t s_kinfo[32];
    __shared__ uint32_t s_ones[HHUFF_ONES_NENT];
    load_dec_tables(s_lut, s_kinfo, s_ones, blockDim.x);
    __syncthreads();
    DecTables T;  // assigned, not brace-initialised (see hhuff_blocks.hip)
    T.lut = s_lut;
    T.kinfo = s_kinfo;
    T.ones = s_ones;
    const uint32_t max_entries = A.T / kEntryOverhead;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < A.nsec; k += (uint64_t)gridDim.x * blockDim.x) {
        // the section's connection: the last c with conn_first[c] <= k
        uint32_t lo = 0, hi = A.nconn;  // invariant: conn_first[lo] <= k < conn_first[hi]
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (A.conn_first[mid] <= k)
                lo = mid;
            else
                hi = mid;
        }
        const ConnSlot cs = conn_slot<SLOTS>(A.cmap, lo);
        A.nfields[k] = 0;
        A.req_insert_count[k] = 0;
        ReqState rq;
        RespState rs;
        if (REQ) rq.reset();
        if (RESP) rs.reset(false);
        if (cs.refused) {  // its connection has no slab: no table is read
            A.sstatus[k] = HHUFF_QPK_EINVAL;
            if (REQ) q_req_store(A.qreq + k, rq, HHUFF_QPK_EINVAL, 0u, 0u);
            if (RESP) q_res_store(A.qres + k, rs, HHUFF_QPK_EINVAL, 0u, 0u);
            continue;
        }
        const QTable t = q_table(A, cs.slot);
        if (t.s.failed) {
            A.sstatus[k] = HHUFF_QPK_SKIPPED;
            if (REQ) q_req_store(A.qreq + k, rq, HHUFF_QPK_SKIPPED, 0u, 0u);
            if (RESP) q_res_store(A.qres + k, rs, HHUFF_QPK_SKIPPED, 0u, 0u);
            continue;
        }
        uint64_t p = A.sec_off[k];
        const uint64_t end = A.sec_off[k + 1];
        QCtx ctx{0, 0};
        int32_t st = q_parse_context(t, max_entries, ctx, A.in, p, end);
        if (st == 0) {
            A.req_insert_count[k] = (uint64_t)ctx.ric;
            // check_decode_context_blocked (:801-820); the max_blocked limit is applied per connection in
            // section order by qpack_blocked_kernel (every parked stream raises num_blocked)
            if (!(ctx.ric < t.total())) st = HHUFF_QPK_BLOCKED;
        }
        QArena R{A.arena, A.arena_off[k], min(A.arena_off[k + 1], kArenaLimit)};  // field offsets are u32
        const uint32_t slot = A.sec_off[k];
        uint32_t nf = 0;
        if (RESP && st == 0 && p == end) {  // a head without fields: missing :status (hpack.c:652-655), normalised
            rs.err = HHUFF_HERR_MISSING_PSEUDO;
            st = kDF;
        }
        while (st == 0 && p != end) {
            uint32_t no = 0, nl = 0, vo = 0, vl = 0, soft = 0;
            uint64_t fn = 0, fv = 0;
            const int32_t rc = q_field(A, t, ctx, p, end, R, no, nl, vo, vl, soft, fn, fv, T);
            if (rc != 0 && rc != kErrInvalidChar) {
                st = rc;
                // h2o_hpack_parse_request: *err_desc = decode_err (hpack.c:523-525)
                if (REQ) rq.err = rc == HHUFF_QPK_ARENA ? HHUFF_HERR_NONE : HHUFF_HERR_DECODE;
                if (RESP) rs.err = rc == HHUFF_QPK_ARENA ? HHUFF_HERR_NONE : HHUFF_HERR_DECODE;
                break;
            }
            bool header = false;
            int32_t rr = 0;
            if (REQ || RESP) {  // the bytes where they lie: a source (fn / fv), or the arena (decoded in place)
                const uint8_t* np = fn ? reinterpret_cast<const uint8_t*>(fn) : A.arena + no;
                const uint8_t* vp = fv ? reinterpret_cast<const uint8_t*>(fv) : A.arena + vo;
                if (REQ) rr = req_field_h3(rq, req_name_class(np, nl), vp, vl, soft, (int32_t)nf, header);
                if (RESP) rr = resp_field_h3(rs, req_name_class(np, nl), vp, vl, soft, (int32_t)nf, header);
            }
            A.fsrc_n[slot + nf] = fn;
            A.fsrc_v[slot + nf] = fv;
            A.name_off[slot + nf] = no;
            A.name_len[slot + nf] = nl;
            A.value_off[slot + nf] = vo;
            A.value_len[slot + nf] = vl;
            A.fflags[slot + nf] = (uint8_t)(soft | (header ? HHUFF_FIELD_HEADER : 0u));
            ++nf;
            if (rr != 0) {  // normalize_error_code (qpack.c:822-828): a rule's H2 error fails the section
                st = kDF;
                break;
            }
        }
        if (REQ) {
            if (st == 0 && rq.err != HHUFF_HERR_NONE) st = kErrInvalidChar;  // hpack.c:636-637
            q_req_store(A.qreq + k, rq, st, (uint64_t)ctx.ric, A.stream_id[k]);
        }
        if (RESP) {
            if (st == 0 && rs.err != HHUFF_HERR_NONE) st = kErrInvalidChar;  // hpack.c:745-747
            q_res_store(A.qres + k, rs, st, (uint64_t)ctx.ric, A.stream_id[k]);
        }
        A.nfields[k] = nf;
        A.sstatus[k] = st;
    }
}

// Copy pass: 64 sections per wave (wave_copy_fields), their fields' name / value bytes into the arena.
__global__ __launch_bounds__(256) void qpack_copy_kernel(QpkArgs A) {
    const int lane = threadIdx.x & 63;
    const uint32_t nw = gridDim.x * 4u;
    for (uint32_t k0 = (blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u; k0 < A.nsec; k0 += nw * 64u) {
        const uint32_t k = k0 + (uint32_t)lane;
        const uint32_t s0 = k < A.nsec ? A.sec_off[k] : 0u, nf = k < A.nsec ? A.nfields[k] : 0u;
        wave_copy_fields(s0, nf, lane, [&](uint32_t f, bool val, const uint8_t*& src, uint8_t*& dst, uint32_t& len) {
            const uint64_t fs = val ? A.fsrc_v[f] : A.fsrc_n[f];
            src = reinterpret_cast<const uint8_t*>(fs);
            dst = A.arena + (val ? A.value_off[f] : A.name_off[f]);
            len = fs ? (val ? A.value_len[f] : A.name_len[f]) : 0u;
        });
    }
}

// check_decode_context_blocked's slot limit (qpack.c:801-820) across one step's sections of a connection:
// h2o raises conn->num_qpack_blocked for every stream it parks (lib/http3/server.c:1553), so the blocked
// sections of a connection, in section order, take the free slots one by one; the first one that finds
// num_blocked >= max_blocked fails with QPACK_DECOMPRESSION_FAILED.  One lane per connection.
__global__ __launch_bounds__(256) void qpack_blocked_kernel(QpkArgs A) {
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < A.nconn; c += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t nb = A.num_blocked ? A.num_blocked[c] : 0u;
        for (uint32_t k = A.conn_first[c]; k < A.conn_first[c + 1]; ++k) {
            if (A.sstatus[k] != HHUFF_QPK_BLOCKED) continue;
            if (nb >= A.max_blocked)
                A.sstatus[k] = kDF;
            else
                ++nb;
        }
    }
}

// ---- encoder-stream literal pre-pass ----
// An encoder stream's instructions are readable without the table (name indexes and literal lengths are
// explicit, qpack.c:420-474), so one lane per connection finds every literal the walk could reach and the
// literal kernels decode them all together, balanced across connections; the walk (qpack_encoder_kernel)
// then copies bytes instead of running a Huffman decoder per lane.  Marks past a table-dependent error (an
// index the table does not hold) are decoded and unused.

struct QMarks {
    uint32_t *lit, *name, *p3;
};

// the literal with `prefix`-bit length at p inside [p, end): mark it, step over it
__device__ __forceinline__ bool q_mark_literal(const uint8_t* in, uint64_t& p, uint64_t end, uint32_t prefix,
                                               const QMarks& M) {
    if (p >= end) return false;
    uint64_t q = p;
    const int64_t n = hpack_int(in, q, end, prefix);
    if (n < 0 || (uint64_t)n > end - q) return false;
    const uint32_t w = (uint32_t)(p >> 5), m = 1u << (p & 31);
    atomicOr(M.lit + w, m);
    if (prefix != 7) atomicOr(M.name + w, m);
    if (prefix == 3) atomicOr(M.p3 + w, m);
    p = q + (uint64_t)n;
    return true;
}

// one lane per encoder stream (items [0, nconn)) or field section (the rest)
__global__ __launch_bounds__(256) void qpack_mark_kernel(QpkArgs A, QMarks M) {
    const uint8_t* in = A.in;
    const uint64_t nitems = (uint64_t)A.nconn + A.nsec;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nitems; c += (uint64_t)gridDim.x * blockDim.x) {
        if (c >= A.nconn) {  // a section: the decode context, then the representation switch of q_field
            const uint64_t k = c - A.nconn;
            uint64_t p = A.sec_off[k];
            const uint64_t end = A.sec_off[k + 1];
            bool go = hpack_int(in, p, end, 8) >= 0 && p < end && hpack_int(in, p, end, 7) >= 0;
            while (go && p < end) {
                const uint32_t kind = in[p] >> 4;
                if (kind >= 8) {  // indexed, static or dynamic
                    go = hpack_int(in, p, end, 6) >= 0;
                } else if (kind == 1) {  // indexed, post-base
                    go = hpack_int(in, p, end, 4) >= 0;
                } else if (kind == 2 || kind == 3) {  // literal name, then the value
                    go = q_mark_literal(in, p, end, 3, M) && q_mark_literal(in, p, end, 7, M);
                } else {  // name reference (static / dynamic 4 bits, post-base 3), then the value
                    go = hpack_int(in, p, end, kind == 0 ? 3 : 4) >= 0 && q_mark_literal(in, p, end, 7, M);
                }
            }
            continue;
        }
        uint64_t p = A.enc_off[c];
        const uint64_t end = p + A.enc_len[c];
        bool go = true;
        while (go && p < end) {  // the instruction switch of q_handle_input
            const uint32_t b = in[p];
            switch (b >> 5) {
                default:  // insert with name reference: index, then the value
                    go = hpack_int(in, p, end, 6) >= 0 && q_mark_literal(in, p, end, 7, M);
                    break;
                case 2:
                case 3:  // insert with a literal name: the name (5-bit prefix), then the value
                    go = q_mark_literal(in, p, end, 5, M) && q_mark_literal(in, p, end, 7, M);
                    break;
                case 0:
                case 1: go = hpack_int(in, p, end, 5) >= 0; break;  // duplicate, set capacity
            }
        }
    }
}

uint64_t qpack_conn_scratch(uint32_t header_table_size) {
    return sizeof(QState) + (uint64_t)qpk_entries(header_table_size) * sizeof(QEntry) +
           2ull * qpk_ring_bytes(header_table_size);
}

uint64_t qpack_dsession_slab(uint32_t max_blocked) { return qp_slab_bytes(max_blocked); }

hipError_t launch_qpack(const QpdCall& call, const hhuff_qpack_dsessions_t* ds, hipStream_t stream) {
    const uint32_t nconn = call.nconn, nsec = call.nsec;
    const uint64_t in_size = call.in_size, max_blocked = call.max_blocked;
    const uint32_t* cmap = call.cmap;
    hhuff_qpack_request_t* qreq = call.qreq;
    hhuff_qpack_response_head_t* qres = call.qres;
    if (nconn == 0) return hipSuccess;
    // workspace (hhuff_decwork.h): the literal pre-pass's bitmaps, word prefixes, chunk sums, the literal list
    // with each literal's prefix, the literal kernels' results and decoded bytes (positions are u32: in_size <
    // 2^32, checked by the C ABI), the field slots' byte sources, and for a session step without a slot map
    // its connection map (the encoder-stream pass fills it)
    const LitDims d = qpd_dims(in_size);
    const uint64_t lit_ws = literals_dev_ws((uint32_t)d.n_max, in_size), map_conns = ds && !cmap ? nconn : 0u;
    QpdWork W;
    uint8_t* work = nullptr;
    hipError_t e = work_alloc((void**)&work, qpd_carve(W, in_size, lit_ws, map_conns, nullptr), stream);
    if (e != hipSuccess) return e;
    qpd_carve(W, in_size, lit_ws, map_conns, work);
    const LitWork& L = W.lit;
    QpkArgs A{call, qpack_conn_scratch(call.T), L.lit_bits, L.word_pre, L.len, L.st, L.pfx, L.out, W.fsrc_n, W.fsrc_v};
    e = hipMemsetAsync(work, 0, W.zero_end, stream);
    if (e == hipSuccess) {
        const uint64_t items = (uint64_t)nconn + nsec;
        hipLaunchKernelGGL(qpack_mark_kernel, dim3((uint32_t)std::min<uint64_t>((items + 255) / 256, 65535)), dim3(256), 0,
                           stream, A, QMarks{L.lit_bits, L.name_bits, L.p3_bits});
        e = hipGetLastError();
    }
    if (e == hipSuccess)  // prefixes: section names 3, encoder-stream names 5, values 7
        e = launch_literal_list(L.lit_bits, L.name_bits, L.p3_bits, 3u, 5u, d.nwords, L.chunk, L.word_pre, L.list, L.lnames,
                                L.pfx, stream);
    if (e == hipSuccess)
        e = launch_literals_dev(A.in, in_size, L.list, (uint32_t)d.n_max, L.chunk + d.nchunks, 7u,
                                HHUFF_LIT_QPACK | kLitNoRawCopy, L.lnames, L.out, L.len, L.pay, L.cons, L.st, L.ws, stream,
                                L.pfx);
    auto step = [&](auto slots) {  // the kernels' instantiation with or without connection slots
        constexpr bool S = decltype(slots)::value;
        hipLaunchKernelGGL(qpack_encoder_kernel<S>, dim3(std::min((nconn + 255u) / 256u, 65535u)), dim3(256), 0, stream, A);
        hipLaunchKernelGGL(qpack_table_kernel<S>, dim3((uint32_t)(((uint64_t)nconn + 3) / 4)), dim3(256), 0, stream, A);
        hipError_t f = hipGetLastError();
        if (f != hipSuccess || nsec == 0) return f;
        const dim3 gs(std::min((nsec + 255u) / 256u, 65535u));
        if (qres)
            hipLaunchKernelGGL((qpack_sections_kernel<kSecResp, S>), gs, dim3(256), 0, stream, A);
        else if (qreq)
            hipLaunchKernelGGL((qpack_sections_kernel<kSecReq, S>), gs, dim3(256), 0, stream, A);
        else
            hipLaunchKernelGGL((qpack_sections_kernel<kSecPlain, S>), gs, dim3(256), 0, stream, A);
        hipLaunchKernelGGL(qpack_copy_kernel, dim3(std::min((nsec + 255u) / 256u, 4096u)), dim3(256), 0, stream, A);
        hipLaunchKernelGGL(qpack_blocked_kernel, dim3(std::min((nconn + 255u) / 256u, 65535u)), dim3(256), 0, stream, A);
        return hipGetLastError();
    };
    auto session_step = [&]() {  // the passes of `step` on the step's own map, the session pass behind them
        QdsArgs D{static_cast<uint8_t*>(ds->state), qp_slab_bytes((uint32_t)max_blocked), (uint32_t)max_blocked, ds->flags,
                  ds->cancel_first, ds->cancel_id, ds->cancel_flags, ds->dec_out, ds->dec_out_off, ds->dec_out_len,
                  ds->wake_id, ds->wake_first, ds->nwake, ds->parked, ds->dflags,
                  cmap ? const_cast<uint32_t*>(cmap) : W.map, cmap};
        A.cmap = D.map;
        const dim3 gc(std::min((nconn + 255u) / 256u, 65535u));
        hipLaunchKernelGGL(qpack_encoder_ds_kernel, gc, dim3(256), 0, stream, A, D);
        hipLaunchKernelGGL(qpack_table_kernel<true>, dim3((uint32_t)(((uint64_t)nconn + 3) / 4)), dim3(256), 0, stream, A);
        hipError_t f = hipGetLastError();
        if (f != hipSuccess) return f;
        if (nsec != 0) {
            const dim3 gs(std::min((nsec + 255u) / 256u, 65535u));
            if (qres)
                hipLaunchKernelGGL((qpack_sections_kernel<kSecResp, true>), gs, dim3(256), 0, stream, A);
            else
                hipLaunchKernelGGL((qpack_sections_kernel<kSecReq, true>), gs, dim3(256), 0, stream, A);
            hipLaunchKernelGGL(qpack_copy_kernel, dim3(std::min((nsec + 255u) / 256u, 4096u)), dim3(256), 0, stream, A);
        }
        hipLaunchKernelGGL(qpack_dsession_kernel, gc, dim3(256), 0, stream, A, D);
        return hipGetLastError();
    };
    if (e == hipSuccess) e = ds ? session_step() : cmap ? step(std::true_type{}) : step(std::false_type{});
    const hipError_t f = hipFreeAsync(work, stream);
    return e != hipSuccess ? e : f;
}

}  // namespace hhuff
