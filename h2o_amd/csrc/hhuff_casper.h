// CASPER (include/hhuff.h (2n)): what the device (hhuff_casper.hip) and the host (tools/casper_host.cpp, under
// AddressSanitizer and UndefinedBehaviorSanitizer) both run.  Restated from h2o's lib/http2/casper.c,
// deps/golombset/golombset.h, h2o_decode_base64url and h2o_base64_encode; nothing else knows the slab layout.
//   header_ok, slab_bytes        the slab and its check
//   sha1_first4 / path_key       one lane's SHA-1 over a word source (cd::SegWords: SHA-1 pads as SHA-256 does): a
//                                rolling 16-word schedule in registers
//   lower_bound, insert, unite   the serial set operations
//   decode_cookie                consume_cookie's name test and serial Golomb decode (what the wave decoder must equal)
//   cookie_bits, cookie_length, write_cookie   the serial Golomb encoder and base64url writer (what the wave's must equal)
//   Serial                       one connection's op walk over a slab: hhuff_casper_step for one connection
// A slab is [16 B header][nkeys x u64 ascending], 16-byte aligned, and holds no address.
#ifndef HHUFF_CASPER_H
#define HHUFF_CASPER_H
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_cdigest.h"

namespace hhuff {
namespace csp {
using cd::b64_val;
using cd::kSat;
using cd::sat_add;

constexpr uint32_t kMagic = 0x53434848u;  // "HHCS"
constexpr uint32_t kVersion = 1;
constexpr uint32_t kHeaderBytes = 16;
constexpr uint32_t kNameLen = 11, kAttrLen = 55;  // "h2o_casper=", COOKIE_ATTRIBUTES
constexpr uint64_t kTooLong = ~0ull;

HHUFF_CD_HD uint8_t name_byte(uint32_t i) { return (uint8_t)"h2o_casper="[i]; }
HHUFF_CD_HD uint8_t attr_byte(uint32_t i) { return (uint8_t)"; Path=/; Expires=Tue, 01 Jan 2030 00:00:00 GMT; Secure"[i]; }
static_assert(sizeof("h2o_casper=") - 1 == kNameLen && sizeof("; Path=/; Expires=Tue, 01 Jan 2030 00:00:00 GMT; Secure") - 1 == kAttrLen,
              "cookie pieces");

HHUFF_CD_HD uint64_t slab_bytes(uint64_t max_keys) { return (kHeaderBytes + 8u * max_keys + 15u) & ~15ull; }

// the header's four little-endian dwords -> it is one this library writes for a scratch of max_keys
HHUFF_CD_HD bool header_ok(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t max_keys) {
    const uint32_t cap = (w1 >> 16) & 0xFFu, rem = w1 >> 24;
    return w0 == kMagic && (w1 & 0xFFFFu) == kVersion && cap >= 1u && cap <= 30u && rem <= 31u && w2 <= max_keys && w3 == max_keys;
}
HHUFF_CD_HD uint32_t header_word1(uint32_t cap, uint32_t rem) { return kVersion | cap << 16 | rem << 24; }

// ---- SHA-1 (FIPS 180-4) of one message by one lane -> the digest's first word.  Words::next() gives the padded
// message's big-endian words in order; every index below is a constant once unrolled ----
HHUFF_CD_HD uint32_t rotl(uint32_t x, uint32_t n) { return x << n | x >> (32u - n); }

template <class Words>
HHUFF_CD_HD uint32_t sha1_first4(Words& M, uint64_t nblocks) {
    uint32_t h0 = 0x67452301u, h1 = 0xEFCDAB89u, h2 = 0x98BADCFEu, h3 = 0x10325476u, h4 = 0xC3D2E1F0u;
    for (uint64_t blk = 0; blk < nblocks; ++blk) {
        uint32_t w[16];
HHUFF_CD_UNROLL
        for (uint32_t i = 0; i < 16; ++i) w[i] = M.next();
        uint32_t a = h0, b = h1, c = h2, d = h3, e = h4;
HHUFF_CD_UNROLL
        for (uint32_t i = 0; i < 80; ++i) {
            if (i >= 16) w[i & 15] = rotl(w[(i + 13) & 15] ^ w[(i + 8) & 15] ^ w[(i + 2) & 15] ^ w[i & 15], 1);
            const uint32_t f = i < 20 ? (b & c) | (~b & d) : i < 40 ? b ^ c ^ d : i < 60 ? (b & c) | (b & d) | (c & d) : b ^ c ^ d;
            const uint32_t k = i < 20 ? 0x5A827999u : i < 40 ? 0x6ED9EBA1u : i < 60 ? 0x8F1BBCDCu : 0xCA62C1D6u;
            const uint32_t t = rotl(a, 5) + f + e + k + w[i & 15];
            e = d, d = c, c = rotl(b, 30), b = a, a = t;
        }
        h0 += a, h1 += b, h2 += c, h3 += d, h4 += e;
    }
    return h0;
}

// calc_key before the mask: the digest's first four bytes as a little-endian unsigned.  Src: cd::SegWords' chunk().
template <class Src>
HHUFF_CD_HD uint32_t path_key(const Src& S, uint32_t off, uint32_t len) {
    const uint32_t offs[5] = {off, 0, 0, 0, 0}, lens[5] = {len, 0, 0, 0, 0};
    cd::SegWords<Src> M(S, offs, lens);
    const uint32_t h0 = sha1_first4(M, M.nwords / 16u);
    return h0 >> 24 | ((h0 >> 8) & 0xFF00u) | ((h0 << 8) & 0xFF0000u) | h0 << 24;
}

// ---- the serial set operations on keys[0 .. n) ----
HHUFF_CD_HD uint32_t lower_bound(const uint64_t* keys, uint32_t n, uint64_t key) {  // the first index with keys[i] >= key
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2u;
        if (keys[mid] < key) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}
HHUFF_CD_HD void insert(uint64_t* keys, uint32_t n, uint32_t at, uint64_t key) {  // room for n + 1
    for (uint32_t i = n; i > at; --i) keys[i] = keys[i - 1u];
    keys[at] = key;
}
// the union of a[0 .. na) and b[0 .. nb) into out (room for na + nb) -> its size; an equal key is kept once
HHUFF_CD_HD uint32_t unite(const uint64_t* a, uint32_t na, const uint64_t* b, uint32_t nb, uint64_t* out) {
    uint32_t i = 0, j = 0, n = 0;
    while (i < na || j < nb) {
        if (j == nb || (i < na && a[i] < b[j])) out[n++] = a[i++];
        else if (i == na || b[j] < a[i]) out[n++] = b[j++];
        else out[n++] = a[i++], ++j;
    }
    return n;
}

// ---- consume_cookie's decode of the value in[off .. off + len): false = the cookie is dropped.  keys[i] is written
// for i < room; *nkeys counts on, so that "more than L" and "more than fits" are told apart by the caller ----
template <class Src>
HHUFF_CD_HD bool decode_cookie(const Src& S, uint64_t off, uint64_t len, uint32_t rem, uint64_t* keys, uint64_t room, uint64_t* nkeys) {
    if (len <= kNameLen) return false;
    for (uint32_t i = 0; i < kNameLen; ++i)
        if (S.byte(off + i) != name_byte(i)) return false;
    const uint64_t start = off + kNameLen, c = len - kNameLen;
    if (c % 4u == 1u) return false;
    for (uint64_t i = 0; i < c; ++i)
        if (b64_val(S.byte(start + i)) == 0xFFu) return false;
    cd::BitReader<Src> B{S, start, 0, 8u * (c * 3u / 4u)};
    uint64_t next_min = 0, n = 0;
    for (;;) {
        uint64_t q = 0, r;
        int b;
        while ((b = B.bit()) == 0) ++q;
        if (b < 0 || !B.bits(rem, &r)) break;  // a value cut short is not a key
        const uint64_t key = sat_add(next_min, cd::sat_value(q, r, rem));
        if (key >= kSat) return false;
        if (n < room) keys[n] = key;
        ++n, next_min = key + 1u;
    }
    *nkeys = n;
    return true;
}

// ---- get_cookie ----
// the bits golombset_encode writes for one key (saturating)
HHUFF_CD_HD uint64_t value_bits(uint64_t key, uint64_t next_min, uint32_t rem) { return sat_add((key - next_min) >> rem, 1u + rem); }
// the cookie's length from the set's bits, kTooLong at 2^35 bits and more (no region of `out` holds that)
HHUFF_CD_HD uint64_t cookie_length(uint64_t bits) {
    if (bits >= 1ull << 35) return kTooLong;
    const uint64_t nbytes = (bits + 7u) / 8u;
    return kNameLen + (4u * nbytes + 2u) / 3u + kAttrLen;
}
HHUFF_CD_HD uint64_t cookie_bits(const uint64_t* keys, uint32_t n, uint32_t rem) {
    uint64_t bits = 0, next_min = 0;
    for (uint32_t i = 0; i < n; ++i) bits = sat_add(bits, value_bits(keys[i], next_min, rem)), next_min = keys[i] + 1u;
    return bits;
}
HHUFF_CD_HD uint8_t b64url_char(uint32_t v) {
    return (uint8_t)(v < 26u ? 'A' + v : v < 52u ? 'a' + (v - 26u) : v < 62u ? '0' + (v - 52u) : v == 62u ? '-' : '_');
}
// the cookie of a non-empty set into dst[0 .. cookie_length(cookie_bits(..))), bit by bit
HHUFF_CD_HD void write_cookie(const uint64_t* keys, uint32_t n, uint32_t rem, uint8_t* dst) {
    for (uint32_t i = 0; i < kNameLen; ++i) *dst++ = name_byte(i);
    uint64_t bits = 0, next_min = 0;
    uint32_t acc = 0, have = 0;
    auto put = [&](uint32_t bit) {
        acc = acc << 1 | bit, ++bits;
        if (++have == 6u) *dst++ = b64url_char(acc), acc = 0, have = 0;
    };
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t v = keys[i] - next_min;
        for (uint64_t q = v >> rem; q != 0; --q) put(0);
        put(1);
        for (uint32_t b = rem; b != 0; --b) put((uint32_t)(v >> (b - 1u)) & 1u);
        next_min = keys[i] + 1u;
    }
    const uint64_t nbytes = (bits + 7u) / 8u;
    while (bits < 8u * nbytes || have != 0) put(0);  // the last byte's zeros, then the last character's
    for (uint32_t i = 0; i < kAttrLen; ++i) *dst++ = attr_byte(i);
}

// ---- one connection's walk, serially: what the kernel's wave does for a connection ----
struct Fields {
    const uint32_t* value_off;
    const uint32_t* value_len;
    const int32_t* token;
    uint32_t nfslots;
    int32_t cookie_token;
};

template <class Src>
struct Serial {
    const Src& S;  // `in`
    uint64_t in_size;
    uint8_t* slab;  // slab_bytes(max_keys)
    uint32_t max_keys;
    uint64_t* tmp;  // 3 max_keys: a cookie's keys, then the union (2 max_keys: a damaged set may not shrink it)
    uint8_t* out;
    uint32_t wpos, rend;  // the region's write position and end
    bool valid = false, dirty = false;
    uint32_t cap = 0, rem = 0, nkeys = 0;

    uint32_t word(uint32_t i) const {
        return (uint32_t)slab[4u * i] | (uint32_t)slab[4u * i + 1u] << 8 | (uint32_t)slab[4u * i + 2u] << 16 | (uint32_t)slab[4u * i + 3u] << 24;
    }
    uint64_t* keys() const { return reinterpret_cast<uint64_t*>(slab + kHeaderBytes); }
    void load() {
        valid = header_ok(word(0), word(1), word(2), word(3), max_keys);
        if (valid) cap = (word(1) >> 16) & 0xFFu, rem = word(1) >> 24, nkeys = word(2);
    }
    void store() {
        if (!valid || !dirty) return;
        const uint32_t h[4] = {kMagic, header_word1(cap, rem), nkeys, max_keys};
        for (uint32_t b = 0; b < 16; ++b) slab[b] = (uint8_t)(h[b >> 2] >> (8u * (b & 3u)));
    }
    int32_t consume(uint64_t off, uint64_t len, uint32_t* value) {
        if (off + len > in_size) return HHUFF_CSP_EINVAL;
        uint64_t nb;
        if (!decode_cookie(S, off, len, rem, tmp, max_keys, &nb)) return 0;
        const uint64_t L = (1ull << cap) > 128u ? 1ull << cap : 128u;
        if (nb > L) return 0;
        *value += (uint32_t)nb;
        if (nb > max_keys) return HHUFF_CSP_SPACE;
        uint32_t fresh = 0;  // (the count first: the set stays as it was if the union does not fit)
        for (uint32_t j = 0; j < nb; ++j) {
            const uint32_t i = lower_bound(keys(), nkeys, tmp[j]);
            fresh += !(i < nkeys && keys()[i] == tmp[j]);
        }
        if (nkeys + fresh > max_keys) return HHUFF_CSP_SPACE;
        if (fresh == 0) return 0;
        const uint32_t n = unite(keys(), nkeys, tmp, (uint32_t)nb, tmp + max_keys);
        for (uint32_t i = 0; i < n && i < max_keys; ++i) keys()[i] = tmp[max_keys + i];
        nkeys = n < max_keys ? n : max_keys, dirty = true;  // (n <= max_keys for an ascending set; a damaged one stays inside)
        return 0;
    }
    // res: status, value, nkeys, at
    void op(uint32_t kind, uint32_t a, uint32_t b, uint32_t reserved, bool bad_slot, const Fields& F, uint32_t* res) {
        int32_t st = 0;
        uint32_t value = 0, at = 0;
        if (bad_slot || reserved != 0 || kind < HHUFF_CSP_INIT || kind > HHUFF_CSP_COOKIE) st = HHUFF_CSP_EINVAL;
        else if (kind == HHUFF_CSP_INIT) {
            if (a < 1u || a > 30u || b > 31u) st = HHUFF_CSP_EINVAL;
            else valid = dirty = true, cap = a, rem = b, nkeys = 0;
        } else if (!valid) st = HHUFF_CSP_EFORMAT;
        else if (kind == HHUFF_CSP_CONSUME) st = consume(a, b, &value);
        else if (kind == HHUFF_CSP_CONSUME_FIELDS) {
            if (!F.value_off || !F.value_len || !F.token || (uint64_t)a + b > F.nfslots) st = HHUFF_CSP_EINVAL;
            for (uint64_t s = a; st == 0 && s < (uint64_t)a + b; ++s)
                if (F.token[s] == F.cookie_token) st = consume(F.value_off[s], F.value_len[s], &value);
        } else if (kind == HHUFF_CSP_LOOKUP || kind == HHUFF_CSP_MARK) {
            if ((uint64_t)a + b > in_size) st = HHUFF_CSP_EINVAL;
            else {
                const uint64_t key = path_key(S, a, b) & ((1u << cap) - 1u);
                const uint32_t i = lower_bound(keys(), nkeys, key);
                if (i < nkeys && keys()[i] == key) value = 1;
                else if (kind == HHUFF_CSP_MARK) {
                    if (nkeys == max_keys) st = HHUFF_CSP_SPACE;
                    else insert(keys(), nkeys, i, key), ++nkeys, dirty = true;
                }
            }
        } else {  // HHUFF_CSP_COOKIE
            at = wpos;
            if (nkeys != 0) {
                const uint64_t len = cookie_length(cookie_bits(keys(), nkeys, rem));
                if (len > rend - wpos) st = HHUFF_CSP_SPACE;
                else write_cookie(keys(), nkeys, rem, out + wpos), wpos += (uint32_t)len, value = (uint32_t)len;
            }
        }
        if (st != 0 && !(st == HHUFF_CSP_SPACE && (kind == HHUFF_CSP_CONSUME || kind == HHUFF_CSP_CONSUME_FIELDS))) value = 0;
        res[0] = (uint32_t)st, res[1] = value, res[2] = valid && !bad_slot ? nkeys : 0u, res[3] = at;
    }
};
}  // namespace csp
}  // namespace hhuff
#endif
