// Cache digests (include/hhuff.h (2m)): what the device (hhuff_cdigest.hip) and the host (tools/cdigest_host.cpp, under
// AddressSanitizer and UndefinedBehaviorSanitizer) both run.  Restated from h2o's lib/http2/cache_digests.c,
// deps/golombset/golombset.h, h2o_decode_base64url and h2o_next_token; nothing else knows the image layout.
//   next_token / load_value   the element / attribute walk of h2o_cache_digests_load_header over a Src (byte(i), and
//                             skip_plain(i, end): the first byte at or after i that is one of " \t;,=", or end -- a loop
//                             on the host, a wave's ballot on the device), feeding a Sink (reset(), digest(), stopped())
//   b64_val, BitReader, decode_set   the base64 alphabet h2o accepts; the serial Golomb-coded-set decoder (the host's
//                             Sink, and what the wave decoder must equal)
//   ImageHeader / Frame, lookup()   the image and its checked frame walk
//   Sha256 / sha256_first8    one lane's SHA-256 over a word source: a rolling 16-word schedule in registers
// An image is [ImageHeader 16 B][frame]*: frame = [Frame 16 B][nkeys x u64 ascending].  It holds no address.
#ifndef HHUFF_CDIGEST_H
#define HHUFF_CDIGEST_H
#include <stdint.h>

#include "hhuff.h"

#if defined(__HIPCC__)
#define HHUFF_CD_HD __host__ __device__ inline
#else
#define HHUFF_CD_HD inline
#endif
#if defined(__clang__)
#define HHUFF_CD_UNROLL _Pragma("unroll")
#else
#define HHUFF_CD_UNROLL _Pragma("GCC unroll 64")
#endif

namespace hhuff {
namespace cd {
constexpr uint32_t kMagic = 0x44434848u;  // "HHCD"
constexpr uint32_t kVersion = 1;
constexpr uint32_t kHeaderBytes = 16, kFrameBytes = 16;
constexpr uint32_t kPresent = 1, kComplete = 2;
constexpr uint32_t kMaxCapacityBits = 62;  // 5 + 5 bits: nbits + pbits <= 31 + 31
constexpr uint64_t kSat = 1ull << 63;      // every sum at or above it is "not below 2^capacity_bits"

struct ImageHeader {
    uint32_t magic;
    uint16_t version;
    uint8_t flags, reserved;
    uint32_t nframes, bytes;
};
struct Frame {
    uint8_t capacity_bits, kind;
    uint16_t reserved0;
    uint32_t nkeys;
    uint64_t reserved1;
};
static_assert(sizeof(ImageHeader) == kHeaderBytes && sizeof(Frame) == kFrameBytes, "image records");

// ---- h2o_next_token(iter, ';', ',', ..) ----
struct Iter {
    uint64_t cur, end;
};

HHUFF_CD_HD bool is_blank(uint8_t c) { return c == ' ' || c == '\t'; }

// one token without the "=value" tail; *eq: it stopped behind an '=' (only with with_value)
template <class Src>
HHUFF_CD_HD bool scan_token(const Src& S, Iter& it, uint64_t* start, uint64_t* len, bool with_value, bool* eq) {
    uint64_t cur = it.cur;
    const uint64_t end = it.end;
    for (;; ++cur) {
        if (cur == end) return false;  // (the iterator stays: every later call says the same)
        if (!is_blank(S.byte(cur))) break;
    }
    const uint64_t ts = cur;
    uint64_t te = cur;
    *eq = false;
    for (;;) {
        const uint64_t j = S.skip_plain(cur, end);  // plain bytes: each one moves the token's end
        if (j != cur) cur = j, te = j;
        if (cur == end) break;
        const uint8_t c = S.byte(cur);
        if (c == ';') {
            ++cur;
            break;
        }
        if (c == ',') {
            if (ts == cur) te = ++cur;  // the zero-width element: the token is ","
            break;
        }
        ++cur;
        if (c == '=') {
            if (with_value) {
                *eq = true;
                break;
            }
            te = cur;
        }
    }
    it.cur = cur, *start = ts, *len = te - ts;
    return true;
}

template <class Src>
HHUFF_CD_HD bool next_token(const Src& S, Iter& it, uint64_t* start, uint64_t* len, bool with_value) {
    bool eq, eq2;
    if (!scan_token(S, it, start, len, with_value, &eq)) return false;
    if (eq) {  // the value is a token of its own; a "," there ends the element and is handed back
        uint64_t vs, vl;
        if (scan_token(S, it, &vs, &vl, false, &eq2) && vl == 1 && S.byte(vs) == ',') it.cur -= 1;
    }
    return true;
}

// h2o_lcstris against a lower-case literal of n bytes
template <class Src>
HHUFF_CD_HD bool lc_is(const Src& S, uint64_t start, uint64_t len, const char* lit, uint32_t n) {
    if (len != n) return false;
    for (uint32_t i = 0; i < n; ++i) {
        uint8_t c = S.byte(start + i);
        if (c >= 'A' && c <= 'Z') c = (uint8_t)(c + 0x20);
        if (c != (uint8_t)lit[i]) return false;
    }
    return true;
}

// h2o_cache_digests_load_header on one field value in[off .. off + len)
template <class Src, class Sink>
HHUFF_CD_HD void load_value(const Src& S, uint64_t off, uint64_t len, Sink& K) {
    Iter it{off, off + len};
    bool more;
    do {
        uint64_t gs, gl, ts, tl;
        if (!next_token(S, it, &gs, &gl, false)) return;
        bool reset = false, validators = false, complete = false, skip = false;
        while ((more = next_token(S, it, &ts, &tl, true)) && !(tl == 1 && S.byte(ts) == ',')) {
            if (lc_is(S, ts, tl, "reset", 5)) reset = true;
            else if (lc_is(S, ts, tl, "validators", 10)) validators = true;
            else if (lc_is(S, ts, tl, "complete", 8)) complete = true;
            else skip = true;
        }
        if (reset) K.reset();
        if (!skip) K.digest(gs, gl, validators, complete);
    } while (more && !K.stopped());
}

// ---- base64url as h2o_decode_base64url takes it ('+' and '/' too); 0xFF: a foreign byte ----
HHUFF_CD_HD uint32_t b64_val(uint8_t c) {
    if (c >= 'A' && c <= 'Z') return c - 'A';
    if (c >= 'a' && c <= 'z') return c - 'a' + 26u;
    if (c >= '0' && c <= '9') return c - '0' + 52u;
    if (c == '-' || c == '+') return 62u;
    if (c == '_' || c == '/') return 63u;
    return 0xFFu;
}

// ---- saturating key arithmetic: exact below kSat, kSat from there on (h2o wraps modulo 2^64, which a digest under
// 2^30 bytes cannot reach) ----
HHUFF_CD_HD uint64_t sat_add(uint64_t a, uint64_t b) {  // a, b <= kSat
    const uint64_t s = a + b;
    return s < a || s > kSat ? kSat : s;
}
HHUFF_CD_HD uint64_t sat_shl(uint64_t q, uint32_t pbits) { return q > (kSat >> pbits) ? kSat : q << pbits; }
HHUFF_CD_HD uint64_t sat_value(uint64_t q, uint64_t r, uint32_t pbits) { return sat_add(sat_shl(q, pbits), r); }

// ---- the serial decoder: golombset_decode_bit over the base64 characters themselves ----
// Bit i of the decoded bytes is bit 5 - i % 6 of character i / 6; the bytes end at 8 floor(3 c / 4) bits.
template <class Src>
struct BitReader {
    const Src& S;
    uint64_t start, pos, nbits;
    HHUFF_CD_HD int bit() {
        if (pos == nbits) return -1;
        const uint32_t v = b64_val(S.byte(start + pos / 6u));
        const int b = (int)((v >> (5u - (uint32_t)(pos % 6u))) & 1u);
        ++pos;
        return b;
    }
    HHUFF_CD_HD bool bits(uint32_t n, uint64_t* v) {
        *v = 0;
        for (; n != 0; --n) {
            const int b = bit();
            if (b < 0) return false;
            *v = *v * 2u + (uint64_t)b;
        }
        return true;
    }
};

// load_digest's decode: false = the digest is dropped.  Out::key(i, k) takes key i (it may refuse to store it).
template <class Src, class Out>
HHUFF_CD_HD bool decode_set(const Src& S, uint64_t start, uint64_t c, Out& out, uint32_t* capacity_bits, uint64_t* nkeys) {
    if (c % 4u == 1u) return false;
    for (uint64_t i = 0; i < c; ++i)
        if (b64_val(S.byte(start + i)) == 0xFFu) return false;
    BitReader<Src> B{S, start, 0, 8u * (c * 3u / 4u)};
    uint64_t nbits, pbits;
    if (!B.bits(5, &nbits) || !B.bits(5, &pbits)) return false;
    const uint32_t cap = (uint32_t)(nbits + pbits);
    uint64_t next_min = 0, n = 0;
    for (;;) {
        uint64_t q = 0, r;
        int b;
        while ((b = B.bit()) == 0) ++q;
        if (b < 0 || !B.bits((uint32_t)pbits, &r)) break;  // a value cut short is not a key
        const uint64_t key = sat_add(next_min, sat_value(q, r, (uint32_t)pbits));
        if (key >= 1ull << cap) return false;
        out.key(n++, key);
        next_min = key + 1u;
    }
    *capacity_bits = cap, *nkeys = n;
    return true;
}

// The host's Sink: one image in img[0 .. size), as hhuff_cache_digests_load writes it.
template <class Src>
struct ImageSink {
    const Src* S;  // the value being loaded
    uint8_t* img;
    uint64_t size;
    uint64_t pos = kHeaderBytes;
    uint32_t nframes = 0, flags = 0;
    int32_t status = 0;
    struct Keys {
        uint8_t* p;
        uint64_t room;
        void key(uint64_t i, uint64_t k) {
            if (i < room)
                for (uint32_t b = 0; b < 8; ++b) p[8u * i + b] = (uint8_t)(k >> (8u * b));
        }
    };
    void reset() { pos = kHeaderBytes, nframes = 0, flags = 0; }
    bool stopped() const { return status != 0; }
    void digest(uint64_t start, uint64_t c, bool validators, bool complete) {
        const bool head = size >= pos + kFrameBytes;  // keys are kept while they fit; the count goes on
        Keys K{head ? img + pos + kFrameBytes : img, head ? (size - pos - kFrameBytes) / 8u : 0u};
        uint32_t cap;
        uint64_t nkeys;
        if (!decode_set(*S, start, c, K, &cap, &nkeys)) return;
        if (nkeys > 0xFFFFFFFFull || pos + kFrameBytes + 8u * nkeys > size) {
            status = HHUFF_CD_SPACE;
            return;
        }
        const uint8_t f[16] = {(uint8_t)cap, (uint8_t)(validators ? 1 : 0), 0, 0, (uint8_t)nkeys, (uint8_t)(nkeys >> 8),
                               (uint8_t)(nkeys >> 16), (uint8_t)(nkeys >> 24)};
        for (uint32_t b = 0; b < 16; ++b) img[pos + b] = f[b];
        pos += kFrameBytes + 8u * nkeys, ++nframes, flags = kPresent | (complete ? kComplete : 0u);
    }
    void finish() {
        if (status != 0) reset();
        if (size < kHeaderBytes) {
            status = HHUFF_CD_SPACE;
            return;
        }
        const uint32_t h[4] = {kMagic, kVersion | flags << 16, nframes, (uint32_t)pos};
        for (uint32_t b = 0; b < 16; ++b) img[b] = (uint8_t)(h[b >> 2] >> (8u * (b & 3u)));
    }
};

// ---- the frame walk.  Img: word(i) = the image's i-th little-endian dword, key(i) = its i-th u64; nothing at or
// behind `size` is read whatever the bytes hold ----
template <class Img>
HHUFF_CD_HD int32_t lookup(const Img& M, uint64_t size, uint32_t kind, uint64_t hash) {
    if (size < kHeaderBytes || M.word(0) != kMagic) return HHUFF_CD_EFORMAT;
    const uint32_t vf = M.word(1), nframes = M.word(2), bytes = M.word(3);
    if ((vf & 0xFFFFu) != kVersion || (vf >> 16) > (kPresent | kComplete)) return HHUFF_CD_EFORMAT;
    if (bytes < kHeaderBytes || bytes > size || (bytes & 7u) != 0) return HHUFF_CD_EFORMAT;
    const uint32_t flags = vf >> 16;
    if (!(flags & kPresent)) return nframes == 0 && bytes == kHeaderBytes && flags == 0 ? HHUFF_CD_UNKNOWN : HHUFF_CD_EFORMAT;
    uint64_t pos = kHeaderBytes;
    bool hit = false;
    for (uint32_t f = 0; f < nframes; ++f) {
        if (pos + kFrameBytes > bytes) return HHUFF_CD_EFORMAT;
        const uint32_t w0 = M.word(pos / 4u), cap = w0 & 0xFFu, fkind = (w0 >> 8) & 0xFFu;
        const uint64_t nkeys = M.word(pos / 4u + 1u), k0 = (pos + kFrameBytes) / 8u;
        pos += kFrameBytes + 8u * nkeys;
        if (cap > kMaxCapacityBits || fkind > 1u || (w0 >> 16) != 0 || pos > bytes) return HHUFF_CD_EFORMAT;
        if (fkind != kind || hit) continue;
        const uint64_t key = cap ? hash >> (64u - cap) : hash;  // (h2o shifts by 64 here: undefined in C, the hash on x86-64)
        uint64_t lo = 0, hi = nkeys;  // the first key >= key
        while (lo < hi) {
            const uint64_t mid = (lo + hi) / 2u;
            if (M.key(k0 + mid) < key) lo = mid + 1u;
            else hi = mid;
        }
        hit = lo < nkeys && M.key(k0 + lo) == key;
    }
    if (pos != bytes) return HHUFF_CD_EFORMAT;
    return hit ? HHUFF_CD_FRESH : (flags & kComplete) ? HHUFF_CD_NOT_CACHED : HHUFF_CD_UNKNOWN;
}

// ---- SHA-256 (FIPS 180-4) of one message by one lane.  Words::next() gives the padded message's big-endian words
// in order; the schedule is a rolling window of 16 words and every index below is a constant once unrolled, so
// the window and the round constants live in registers and immediates ----
constexpr uint32_t kSha256K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,
    0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,
    0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
    0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,
    0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
    0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

HHUFF_CD_HD uint32_t rotr(uint32_t x, uint32_t n) { return x >> n | x << (32u - n); }

template <class Words>
HHUFF_CD_HD uint64_t sha256_first8(Words& M, uint64_t nblocks) {
    uint32_t h0 = 0x6a09e667u, h1 = 0xbb67ae85u, h2 = 0x3c6ef372u, h3 = 0xa54ff53au;
    uint32_t h4 = 0x510e527fu, h5 = 0x9b05688cu, h6 = 0x1f83d9abu, h7 = 0x5be0cd19u;
    for (uint64_t blk = 0; blk < nblocks; ++blk) {
        uint32_t w[16];
HHUFF_CD_UNROLL
        for (uint32_t i = 0; i < 16; ++i) w[i] = M.next();
        uint32_t a = h0, b = h1, c = h2, d = h3, e = h4, f = h5, g = h6, h = h7;
HHUFF_CD_UNROLL
        for (uint32_t i = 0; i < 64; ++i) {
            if (i >= 16) {
                const uint32_t x = w[(i + 1) & 15], y = w[(i + 14) & 15];
                w[i & 15] += (rotr(x, 7) ^ rotr(x, 18) ^ x >> 3) + w[(i + 9) & 15] + (rotr(y, 17) ^ rotr(y, 19) ^ y >> 10);
            }
            const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + kSha256K[i] + w[i & 15];
            const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            h = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
        }
        h0 += a, h1 += b, h2 += c, h3 += d, h4 += e, h5 += f, h6 += g, h7 += h;
    }
    return (uint64_t)h0 << 32 | h1;
}

// The padded message over a query's segments.  Src::chunk(pos, rem, &k): the 1 <= k <= 4 bytes from in[pos] on that
// the source hands over in one step (k <= rem), left-aligned in a big-endian word, zeros below.
template <class Src>
struct SegWords {
    const Src& S;
    const uint32_t* off;  // [5], [5]: the query's segments
    const uint32_t* len;
    uint64_t total;       // bytes of the message
    uint64_t nwords;      // 16 nblocks
    uint64_t widx = 0;
    uint32_t seg = 0, done = 0;  // done: bytes of segment `seg` taken
    uint64_t acc = 0;            // `have` pending bytes at the top
    uint32_t have = 0;
    bool padded = false;
    HHUFF_CD_HD SegWords(const Src& s, const uint32_t* o, const uint32_t* l) : S(s), off(o), len(l) {
        total = 0;
        for (uint32_t i = 0; i < 5; ++i) total += l[i];
        nwords = 16u * ((total + 9u + 63u) / 64u);
    }
    HHUFF_CD_HD uint32_t next() {
        const uint64_t i = widx++;
        if (i + 2u == nwords) return (uint32_t)(total >> 29);
        if (i + 1u == nwords) return (uint32_t)(total << 3);
        while (have < 4u) {
            uint32_t k = 4, ch = 0;
            while (seg < 5u && done == len[seg]) ++seg, done = 0;
            if (seg < 5u) ch = S.chunk((uint64_t)off[seg] + done, len[seg] - done, &k), done += k;
            else if (!padded) ch = 0x80000000u, k = 1, padded = true;
            acc |= (uint64_t)ch << (32u - 8u * have);
            have += k;
        }
        const uint32_t w = (uint32_t)(acc >> 32);
        acc <<= 32, have -= 4u;
        return w;
    }
};
}  // namespace cd
}  // namespace hhuff
#endif
