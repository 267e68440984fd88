/*
 * hhuff -- MI355X-native HPACK/QPACK Huffman codec: the drop-in C-ABI boundary.
 *
 * Library: h2o_amd/libhhuff.so (HIP kernels for gfx950 + host shim).  Plain C types only: no HIP,
 * torch or C++ types appear in these signatures; streams are passed as `void *` (a hipStream_t, or
 * NULL for the legacy default stream).
 *
 * 1. Per-string symbols with h2o's exact signatures and semantics.  A maintainer links libhhuff in
 *    place of the definitions in lib/http2/hpack.c.  Each call runs one HIP launch
 *    on the string, synchronously, on a per-thread stream of the calling thread's current device (which
 *    the call leaves as it was).  About 20 us per call on MI355X (bench.py per_string_latency_us) makes
 *    this the compatibility path; throughput comes from the batch API.  A HIP failure never aborts: the
 *    call returns SIZE_MAX (decode: h2o reports the literal as a COMPRESSION error; encode: h2o sends the
 *    string raw, a correct encoding) and hhuff_last_error_string() says why.
 * 2. Batch entry points on device-resident arrays (the hot path) and on host arrays (pinned staging,
 *    H2D/D2H included).  Element i of a batch has exactly the per-string semantics of (1).
 *
 * Batch array contract (all offsets/lengths u32; a batch addresses < 4 GiB of input):
 *   string i      in[in_off[i] .. in_off[i] + len_i)
 *                 len_i = in_len ? in_len[i] : in_off[i+1] - in_off[i]   (in_off has n+1 entries then)
 *   in_size       bytes readable at `in` (the kernels never read past it)
 *   is_name_bits  u32[(n+31)/32]; bit (i & 31) of word (i >> 5) set => string i is a header name
 *                 (NULL => every string is a header value)
 *   device `in` and `out` must be 16-byte aligned (hipMalloc / torch allocations are);
 *   strings may start at any byte.
 *   Per-string length limit: 2^29 - 1 bytes (status HHUFF_STATUS_TOO_LONG above it).
 */
#ifndef HHUFF_H
#define HHUFF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HHUFF_FAIL_LEN 0xFFFFFFFFu   /* out_len of a string whose per-string call returns SIZE_MAX */
#define HHUFF_SOFT_NAME 0x01u        /* H2O_HPACK_SOFT_ERROR_BIT_INVALID_NAME  (include/h2o/hpack.h:50) */
#define HHUFF_SOFT_VALUE 0x02u       /* H2O_HPACK_SOFT_ERROR_BIT_INVALID_VALUE (include/h2o/hpack.h:51) */
#define HHUFF_STATUS_FAIL 0x80u      /* hard failure: the per-string call returns SIZE_MAX */
#define HHUFF_STATUS_TOO_LONG 0xC0u  /* string longer than the per-string limit (never produced by h2o) */

#define HHUFF_OK 0
#define HHUFF_EINVAL (-1) /* bad argument (NULL array, misaligned base, n too large) */
#define HHUFF_EHIP (-2)   /* a HIP runtime call failed; see hhuff_last_error_string() */
#define HHUFF_ENODEV (-3) /* no gfx950 device / code object not loadable */

/* ---------------------------------------------------------------------------------------------
 * (1) h2o per-string symbols
 * ------------------------------------------------------------------------------------------- */

/* Replaces lib/http2/hpack.c:117 (declared include/h2o/hpack.h:69-70).
 * Returns the decoded length, or SIZE_MAX on a hard error (EOS symbol, padding longer than 7 bits or not
 * all ones).  On success ORs HHUFF_SOFT_NAME / HHUFF_SOFT_VALUE into *soft_errors (never clears it).
 * `dst` must hold at least 2 * len bytes (h2o's contract; floor(8 * len / 5) suffices).  *err_desc is
 * never written (the reference's upper-case hard error at hpack.c:142-144 is unreachable). */
size_t h2o_hpack_decode_huffman(char *dst, unsigned *soft_errors, const uint8_t *src, size_t len, int is_name,
                                const char **err_desc);

/* Replaces lib/http2/hpack.c:774 (declared include/h2o/hpack.h:60).
 * Returns the Huffman length when it is strictly shorter than `len`, else SIZE_MAX (also for len == 0).
 * `dst` must hold `len` bytes; its contents are unspecified on SIZE_MAX. */
size_t h2o_hpack_encode_huffman(uint8_t *dst, const uint8_t *src, size_t len);

/* Number of calls the two symbols above have taken in this process (both, any outcome).  An integration
 * check: after linking h2o against this library, a non-zero count after decoding a Huffman literal shows
 * h2o's callers (decode_string, h2o_hpack_encode_string, QPACK's flatten_string ...) bound here. */
uint64_t hhuff_per_string_calls(void);
/* Profiling: the resident per-string service's real-time stamps (100 MHz counter, low 32 bits) of the calling
 * thread's last served call on its current device: request seen, input in LDS, coded, output written.
 * HHUFF_OK, or HHUFF_EINVAL when this thread has no served call. */
int hhuff_service_stamps(uint32_t *out4);

/* ---------------------------------------------------------------------------------------------
 * (2) batch API, device-resident arrays (hot path).  Asynchronous on `stream`.
 * ------------------------------------------------------------------------------------------- */

/* Batched h2o_hpack_decode_huffman (hpack.c:117-156; callers hpack.c:241, qpack.c:228/370/579).
 *   out       decoded string i at out + (out_off ? out_off[i] : floor(8 * in_off[i] / 5)).  With out_off the
 *             region must hold floor(8 * len_i / 5) bytes.  Without it the region is the string's slot, from
 *             floor(8 * in_off[i] / 5) up to floor(8 * (in_off[i] + len_i) / 5) -- where the slot of the next
 *             input byte begins: floor(8 * len_i / 5) bytes or one more, so `out` holds floor(8 * in_size / 5)
 *             bytes and the layout is valid whenever the input strings do not overlap.  Bytes of the region
 *             past out_len[i] are unspecified; no byte outside the regions is written.
 *   out_len   u32[n]: decoded length, or HHUFF_FAIL_LEN
 *   status    u8[n]:  soft-error bits on success, HHUFF_STATUS_FAIL on a hard error */
int hhuff_decode_batch(const uint8_t *in, uint64_t in_size, const uint32_t *in_off, const uint32_t *in_len, uint32_t n,
                       const uint32_t *is_name_bits, uint8_t *out, const uint32_t *out_off, uint32_t *out_len,
                       uint8_t *status, void *stream);

/* Batched h2o_hpack_encode_huffman (hpack.c:774-804; callers hpack.c:820, qpack.c:1046).
 *   out       Huffman string i at out + (out_off ? out_off[i] : in_off[i]); the region must hold len_i
 *             bytes.  Contents unspecified where out_len[i] == HHUFF_FAIL_LEN.
 *   out_len   u32[n]: Huffman length (< len_i), or HHUFF_FAIL_LEN when not shorter (SIZE_MAX)
 *   status    u8[n] or NULL: 0, or HHUFF_STATUS_FAIL */
int hhuff_encode_batch(const uint8_t *in, uint64_t in_size, const uint32_t *in_off, const uint32_t *in_len, uint32_t n,
                       uint8_t *out, const uint32_t *out_off, uint32_t *out_len, uint8_t *status, void *stream);

/* Packed output (wave-prefix compaction).  Contiguous layout only: string i = in[in_off[i] .. in_off[i+1]).
 * The strings are cut into tiles of 64 consecutive strings (string i is in tile i / 64).  Within a tile the
 * outputs are packed back to back in string order -- each wavefront lane owns one string and a wave-wide
 * prefix sum of the output lengths places them -- and tile t's run starts at its bound position
 *     decode: floor(8 * in_off[64 t] / 5)        encode: in_off[64 t]
 * (the first string's slot of the implicit layouts above), so runs of different tiles never overlap and
 * no byte outside the outputs is written: HBM traffic is exactly the output bytes.  Failed strings
 * (HHUFF_FAIL_LEN) take no bytes.
 *   out        decode: floor(8 * in_off[n] / 5) bytes; encode: in_off[n] bytes (16-byte aligned)
 *   out_off    u32[n + 1], written: string i at out + out_off[i], out_len[i] bytes; out_off[n] = the end of
 *              the last tile's run.  Inside a tile out_off[i + 1] = out_off[i] + string i's kept length, so
 *              tile t's run is the one range from out_off[64 t] to the end of its last string.
 *   out_len, status   as hhuff_decode_batch / hhuff_encode_batch
 * Device arrays, asynchronous on `stream`; in_size must stay below 2^32 * 5 / 8 (u32 offsets). */
int hhuff_decode_batch_packed(const uint8_t *in, uint64_t in_size, const uint32_t *in_off, uint32_t n,
                              const uint32_t *is_name_bits, uint8_t *out, uint32_t *out_off, uint32_t *out_len,
                              uint8_t *status, void *stream);
int hhuff_encode_batch_packed(const uint8_t *in, uint64_t in_size, const uint32_t *in_off, uint32_t n, uint8_t *out,
                              uint32_t *out_off, uint32_t *out_len, uint8_t *status, void *stream);

/* Batched string-literal framing: QPACK flatten_string (lib/http3/qpack.c:1042-1066) and, with
 * first_bytes == NULL and prefix_bits == 7, HPACK h2o_hpack_encode_string (lib/http2/hpack.c:816-837).
 * Per string: Huffman when not flagged in raw_bits (QPACK's dont_compress) and strictly shorter, i.e.
 *   [first & ~(2^p - 1) | 2^p, prefix-int(hufflen)] [Huffman bytes]
 * else raw:
 *   [first & ~(2^(p+1) - 1), prefix-int(len)] [the bytes]
 *   first_bytes  u8[n]: the caller's first byte (bits above the H bit are kept), NULL => 0
 *   prefix_bits  length-prefix width p in 1..7 (QPACK: 7 values, 5 encoder-stream names, 3 literal names)
 *   raw_bits     bitmask, NULL => all eligible for Huffman
 *   out          string i at out + (out_off ? out_off[i] : in_off[i] + 11 * i); region of len_i + 11 bytes
 *   out_len      u32[n]: framed length */
int hhuff_flatten_batch(const uint8_t *in, uint64_t in_size, const uint32_t *in_off, const uint32_t *in_len, uint32_t n,
                        const uint8_t *first_bytes, unsigned prefix_bits, const uint32_t *raw_bits, uint8_t *out,
                        const uint32_t *out_off, uint32_t *out_len, void *stream);

/* ---------------------------------------------------------------------------------------------
 * (3) batch API, host arrays: pinned staging + H2D, kernels, D2H on an internal stream of `device`.
 *     Synchronous.  Same array contract; `out` is a host buffer sized for the implicit layout
 *     (decode: floor(8 * in_size / 5) bytes, encode: in_size bytes) when out_off is NULL.  The results are
 *     copied back in one piece: bytes of `out` that belong to no string's region are unspecified.
 *     In the contiguous layout with implicit slots (in_len and out_off NULL) the call refuses, before any device
 *     work, a batch whose strings leave `in` (in_off[n] > in_size) or whose slots leave `out` (out_size below
 *     decode floor(8 * in_off[n] / 5), encode in_off[n]): HHUFF_EINVAL.
 * ------------------------------------------------------------------------------------------- */
int hhuff_decode_batch_host(const uint8_t *in, uint64_t in_size, const uint32_t *in_off, const uint32_t *in_len,
                            uint32_t n, const uint32_t *is_name_bits, uint8_t *out, uint64_t out_size,
                            const uint32_t *out_off, uint32_t *out_len, uint8_t *status, int device);
int hhuff_encode_batch_host(const uint8_t *in, uint64_t in_size, const uint32_t *in_off, const uint32_t *in_len,
                            uint32_t n, uint8_t *out, uint64_t out_size, const uint32_t *out_off, uint32_t *out_len,
                            uint8_t *status, int device);

/* (2b) Batched string-literal decode: HPACK decode_string (lib/http2/hpack.c:223-261) and
 *      QPACK decode_header_value_literal / decode_header_name_literal (lib/http3/qpack.c:559-629),
 *      minus the memory pool.  Literal i starts at in[lit_off[i]] -- its first byte carries the H flag
 *      at bit prefix_bits and the length as a prefix_bits-bit prefix integer (h2o_hpack_decode_int,
 *      hpack.c:52-83) -- and must end by in[lit_end[i]] (the walker's src_end).  Huffman payloads are
 *      decoded as h2o_hpack_decode_huffman does; raw payloads are copied and validated with
 *      h2o_hpack_validate_header_name / _value (hpack.c:163-221).  Raw names skip validation when they
 *      start with ':' (HPACK) or, with HHUFF_LIT_QPACK, when h2o_lookup_token knows them (qpack.c:585).
 *      Outputs: pay_off[i] = offset of the payload in `in`; decoded bytes at out + floor(8 pay_off[i] / 5)
 *      (out sized floor(8 in_size / 5) + 16); out_len[i] (HHUFF_FAIL_LEN on failure); consumed[i] =
 *      header + payload bytes, how far the walker's cursor advances (0 on failure); status[i] = soft
 *      bits (0x1 name, 0x2 value) | on failure HHUFF_STATUS_FAIL | verdict << 2 (HHUFF_LIT_*).
 *      Device arrays, asynchronous on `stream`; uses stream-ordered scratch (5 n bytes). */
#define HHUFF_LIT_QPACK 1u
#define HHUFF_LIT_INCOMPLETE 1 /* no byte, or the length integer runs past lit_end (H2O_HTTP2_ERROR_INCOMPLETE) */
#define HHUFF_LIT_BAD_INT 2    /* length integer overflow (H2O_HTTP2_ERROR_COMPRESSION from decode_int) */
#define HHUFF_LIT_TRUNCATED 3  /* length > bytes left before lit_end */
#define HHUFF_LIT_HUFFMAN 4    /* h2o_hpack_decode_huffman returned SIZE_MAX */
#define HHUFF_LIT_UPPERCASE 5  /* raw name with an upper-case letter (validate_header_name returned 0) */
#define HHUFF_LIT_TOO_LONG 6   /* payload of 2^29 bytes or more (this library's per-string limit) */
int hhuff_decode_literals(const uint8_t *in, uint64_t in_size, const uint32_t *lit_off, const uint32_t *lit_end,
                          uint32_t n, unsigned prefix_bits, unsigned flags, const uint32_t *is_name_bits, uint8_t *out,
                          uint32_t *out_len, uint32_t *pay_off, uint32_t *consumed, uint8_t *status, void *stream);

/* (2c) HPACK header blocks: h2o_hpack_decode_header (lib/http2/hpack.c:319-435) applied field
 *      after field over each block, as h2o_hpack_parse_request loops over a block (hpack.c:513-527), with
 *      one dynamic table per connection whose blocks are decoded in order.  One GPU lane per connection.
 *        block b        in[blk_off[b] .. blk_off[b+1])      (blocks packed back to back; blk_off has nblk+1)
 *        connection c   blocks conn_first[c] .. conn_first[c+1]-1   (conn_first has nconn+1 entries)
 *        table_size     SETTINGS_HEADER_TABLE_SIZE of every connection: the table's initial and maximum
 *                       capacity (hpack_capacity = hpack_max_capacity, lib/http2/connection.c:1844;
 *                       h2o's default 4096)
 *        arena          decoded names and values; block b writes arena[arena_off[b] .. arena_off[b+1])
 *                       (u64 offsets); every field's name is written, then its value.  Field offsets
 *                       are u32: arena bytes at or past 2^32 are out of reach (HHUFF_BLK_ARENA there)
 *      Per field f of block b (f in blk_off[b] .. blk_off[b] + nfields[b] - 1: a block of L bytes holds at
 *      most L fields, so field slots reuse the block's byte offsets): name_off/name_len/value_off/
 *      value_len (arena offsets, u32) and fflags = its soft-error bits (HHUFF_SOFT_NAME / _VALUE: the
 *      field's H2O_HTTP2_ERROR_INVALID_HEADER_CHAR).  Per block: nfields[b] and bstatus[b] = 0, or the
 *      hard error that stopped it: -9 H2O_HTTP2_ERROR_COMPRESSION, -1 H2O_HTTP2_ERROR_PROTOCOL (upper-case
 *      raw name), HHUFF_BLK_ARENA (a string does not fit the block's arena slice: a Huffman literal needs
 *      floor(8 len / 5) bytes free, a raw one len, an indexed one its size), or HHUFF_BLK_SKIPPED (an
 *      earlier block of the connection failed: h2o drops the connection).  Fields before the error stand.
 *      A string's room is checked in decode_string's order (hpack.c:223-261): a Huffman literal's before its
 *      decoder runs (a literal that would not decode is HHUFF_BLK_ARENA in a slice too small for it), a raw
 *      name's after its validation (an upper-case raw name is PROTOCOL whatever the slice).  A block may
 *      write any byte of its own slice; it writes none outside, and an empty block writes nothing.
 *      Device arrays; scratch = device memory of hhuff_hpack_scratch_size(nconn, table_size) bytes (the
 *      dynamic tables, 16-byte aligned), kept by the caller between calls for HHUFF_BLK_CONTINUE;
 *      asynchronous on `stream`.  The call also takes a stream-ordered workspace from the library's device
 *      memory pool: 16 bytes per input byte of field sources plus, for inputs below 4 GiB, the literal
 *      pre-pass -- 22 bytes per possible literal (up to 2/3 of the input bytes) plus 1.6 per input byte of
 *      decoded output -- about 33 bytes per input byte in all.  It is released on the stream; the pool
 *      keeps released memory for the next call (it never returns it to the driver by itself):
 *      hhuff_pool_trim() hands it back. */
#define HHUFF_BLK_CONTINUE 1u /* flags: the tables (and failed state) the previous call left in scratch
                                 carry over -- connection c of this call is connection c of that one; without
                                 it every connection starts with an empty table */
#define HHUFF_BLK_ARENA (-300)
#define HHUFF_BLK_SKIPPED (-301)
uint64_t hhuff_hpack_scratch_size(uint32_t nconn, uint32_t table_size);
int hhuff_hpack_decode_blocks(const uint8_t *in, uint64_t in_size, const uint32_t *blk_off, const uint32_t *conn_first,
                              uint32_t nconn, uint32_t table_size, uint8_t *arena, const uint64_t *arena_off,
                              uint32_t *name_off, uint32_t *name_len, uint32_t *value_off, uint32_t *value_len,
                              uint8_t *fflags, uint32_t *nfields, int32_t *bstatus, void *scratch, uint64_t scratch_size,
                              unsigned flags, void *stream);

/* (2c') HTTP/2 request header blocks: the same pass with h2o_hpack_parse_request's own rules applied to each
 *      field as it is decoded (lib/http2/hpack.c:502-637), called as h2o's HTTP/2 server calls it
 *      (lib/http2/connection.c:626-629: every out-pointer given, cache digests loaded, no datagram flow id):
 *        - more than H2O_HPACK_MAX_HEADERS_HARD_LIMIT (1000) fields -> COMPRESSION (:528-532)
 *        - pseudo-headers (:533-586): only before the first regular field; :authority, :method, :path,
 *          :scheme at most once, :path not empty, :protocol at most once; any other ':' name -> PROTOCOL
 *        - content-length must parse (h2o_strtosize) -> else PROTOCOL (:591-597); expect, host (fills a
 *          missing authority) and datagram-flow-id are taken out of the list; te other than "trailers"
 *          (case-insensitive) and connection / http2-settings / transfer-encoding / upgrade -> PROTOCOL
 *          (:587-619)
 *        - the first H2O_MAX_HEADERS (100) remaining fields go to the request's header list; beyond that
 *          they are dropped and the block ends with H2O_HTTP2_ERROR_INVALID_HEADER_CHAR (:620-637)
 *      Outputs as hhuff_hpack_decode_blocks plus, per block, req[b]; per field, fflags gains
 *      HHUFF_FIELD_HEADER when h2o_add_header took the field.  bstatus[b] is h2o_hpack_parse_request's
 *      return value: 0, -254 (H2O_HTTP2_ERROR_INVALID_HEADER_CHAR: a soft error, the connection lives on),
 *      -1 / -9 (connection errors: later blocks of the connection are HHUFF_BLK_SKIPPED), or the
 *      HHUFF_BLK_* codes.  The field that triggered an error is counted in nfields (it was decoded and,
 *      for incremental indexing, entered the table).  The cache-digest field goes to the header list (h2o
 *      also feeds it to h2o_cache_digests_load_header; that side effect is the caller's). */
#define HHUFF_FIELD_HEADER 0x4u /* fflags: the field is in h2o's h2o_headers_t (h2o_add_header) */
#define HHUFF_HERR_NONE 0u               /* *err_desc == NULL */
#define HHUFF_HERR_SOFT_NAME 1u          /* h2o_hpack_soft_err_found_invalid_char_in_header_name */
#define HHUFF_HERR_SOFT_VALUE 2u         /* h2o_hpack_soft_err_found_invalid_char_in_header_value */
#define HHUFF_HERR_HEADERS_TOO_LONG 3u   /* h2o_hpack_err_headers_too_long */
#define HHUFF_HERR_INVALID_PSEUDO 4u     /* h2o_hpack_err_invalid_pseudo_header */
#define HHUFF_HERR_CONTENT_LENGTH 5u     /* h2o_hpack_err_invalid_content_length_header */
#define HHUFF_HERR_CONNECTION_SPECIFIC 6u /* h2o_hpack_err_unexpected_connection_specific_header */
#define HHUFF_HERR_UPPER_CASE_NAME 7u    /* h2o_hpack_err_found_upper_case_in_header_name */
typedef struct hhuff_request {
    uint64_t content_length; /* h2o's *content_length: SIZE_MAX (all ones) without a content-length field */
    int32_t method, scheme, authority, path, protocol, expect; /* the field (0-based within the block) whose
                                value h2o stored in *method ... *expect, or -1; authority may be a host field */
    uint32_t exists_map;  /* *pseudo_header_exists_map: H2O_HPACK_PARSE_HEADERS_*_EXISTS (hpack.h:81-85) */
    uint32_t nheaders;    /* fields added to the header list */
    uint32_t err;         /* HHUFF_HERR_*: what *err_desc points at when the call returns */
    uint32_t scheme_kind; /* *scheme: 0 unset, 1 H2O_URL_SCHEME_HTTP, 2 _HTTPS, 3 _MASQUE */
} hhuff_request_t;        /* 48 bytes */
int hhuff_hpack_parse_requests(const uint8_t *in, uint64_t in_size, const uint32_t *blk_off, const uint32_t *conn_first,
                               uint32_t nconn, uint32_t table_size, uint8_t *arena, const uint64_t *arena_off,
                               uint32_t *name_off, uint32_t *name_len, uint32_t *value_off, uint32_t *value_len,
                               uint8_t *fflags, uint32_t *nfields, int32_t *bstatus, hhuff_request_t *req,
                               void *scratch, uint64_t scratch_size, unsigned flags, void *stream);

/* (2c'') HTTP/2 response header blocks, client side: the same pass with h2o_hpack_parse_response's rules
 *      (lib/http2/hpack.c:642-750) applied to each field as it is decoded, called as h2o's HTTP/2 client calls
 *      it (lib/common/http2client.c:332 for a response head, :421 for trailers; no datagram flow id):
 *        - a head block must not be empty and must start with :status -> else PROTOCOL, missing mandatory
 *          pseudo header (:652-655, :706-709); :status once, three digits, the first 1-9 (PARSE_DIGIT: the
 *          digits before a bad one stay added); any other pseudo-header, or any in trailers -> PROTOCOL
 *        - more than 1000 fields -> COMPRESSION; content-length, cache-digest and host are listed as they are;
 *          datagram-flow-id is not listed; expect, te, connection, http2-settings, transfer-encoding and
 *          upgrade -> PROTOCOL (unexpected connection-specific header, :712-725)
 *        - the first 100 remaining fields go to the header list, beyond that the block ends with -254
 *      trailers[b] != 0 makes block b a trailers block (status == NULL; NULL: every block is a head; an empty
 *      trailers block fails in decode_header with COMPRESSION, hpack.c:328-329).  Outputs as
 *      hhuff_hpack_parse_requests with res[b] in place of req[b]; bstatus[b] is h2o_hpack_parse_response's
 *      return value (0, -254, -1, -9) or the HHUFF_BLK_* codes. */
#define HHUFF_HERR_MISSING_PSEUDO 9u /* h2o_hpack_err_missing_mandatory_pseudo_header */
typedef struct hhuff_response {
    int32_t status;           /* *status: 0 if none was parsed (trailers: always 0) */
    uint32_t nheaders;        /* fields added to the header list */
    uint32_t err;             /* HHUFF_HERR_*: what *err_desc points at when the call returns */
    int32_t datagram_flow_id; /* HTTP/3: the field whose value h2o stored in *datagram_flow_id, or -1 */
} hhuff_response_t;           /* 16 bytes */
int hhuff_hpack_parse_responses(const uint8_t *in, uint64_t in_size, const uint32_t *blk_off, const uint32_t *conn_first,
                                uint32_t nconn, uint32_t table_size, const uint8_t *trailers, uint8_t *arena,
                                const uint64_t *arena_off, uint32_t *name_off, uint32_t *name_len, uint32_t *value_off,
                                uint32_t *value_len, uint8_t *fflags, uint32_t *nfields, int32_t *bstatus,
                                hhuff_response_t *res, void *scratch, uint64_t scratch_size, unsigned flags, void *stream);

/* (2d) QPACK decoder (QPACK half): h2o's QPACK decoder (lib/http3/qpack.c) for many
 *      connections at once.  One call is one step of every connection c:
 *        encoder stream  in[enc_off[c] .. + enc_len[c]): h2o_qpack_decoder_handle_input (qpack.c:420-485,
 *                        decl. include/h2o/qpack.h) -- the caller's encoder-stream receive buffer, i.e. the
 *                        bytes not consumed by the previous step followed by the new ones
 *        field sections  conn_first[c] .. conn_first[c+1]-1, section k = in[sec_off[k] .. sec_off[k+1])
 *                        (packed back to back): what h2o_qpack_parse_request (qpack.c:830-858) reads --
 *                        parse_decode_context, check_decode_context_blocked, then decode_header field after
 *                        field -- against the table as the connection's encoder stream left it
 *        header_table_size  the decoder's SETTINGS_QPACK_MAX_TABLE_CAPACITY (h2o_qpack_create_decoder,
 *                        qpack.c:240); max_blocked its blocked-streams limit; num_blocked[c] (NULL = 0) the
 *                        caller's count of the connection's blocked streams before this step
 *                        (lib/http3/server.c:1544).  Blocked sections of one step take the free slots in
 *                        section order, as h2o raises num_qpack_blocked for every stream it parks
 *                        (server.c:1553): the first blocked section that finds num_blocked >= max_blocked
 *                        gets HHUFF_QPK_DECOMPRESSION_FAILED.
 *      Table semantics: every section of a step is decoded against the table as the step's WHOLE encoder
 *      stream left it.  h2o decodes a section against the table as it stands when the section arrives;
 *      the two differ only when the same step's encoder stream evicts an entry an earlier-arriving section
 *      still references -- which a compliant encoder never does (RFC 9204 2.1.1: an entry that
 *      unacknowledged sections reference is not evictable).  Against such a peer this call reports
 *      DECOMPRESSION_FAILED where h2o would have decoded the section; a caller that must match h2o
 *      byte for byte there splits the step before the evicting instruction.
 *      Per connection: enc_status[c] = 0, HHUFF_QPK_DECOMPRESSION_FAILED (h2o then closes the connection
 *      with H2O_HTTP3_ERROR_QPACK_ENCODER_STREAM) or HHUFF_QPK_SKIPPED (an earlier step failed);
 *      enc_consumed[c] = bytes of complete instructions consumed (the rest waits for more input);
 *      insert_count[c] as handle_input reports it (the new Insert Count, 0 when nothing was inserted).
 *      Per section k: sstatus[k] = 0, HHUFF_QPK_DECOMPRESSION_FAILED, HHUFF_QPK_BLOCKED (Required Insert
 *      Count not reached and a blocked slot free: h2o parks the stream until more inserts arrive),
 *      HHUFF_QPK_ARENA (a string does not fit arena[arena_off[k] .. min(arena_off[k+1], 2^32)) -- field
 *      offsets are u32 --: a Huffman literal
 *      needs floor(8 len / 5) bytes free, a raw one len, an indexed one its size) or HHUFF_QPK_SKIPPED;
 *      req_insert_count[k] (decoded Required Insert Count, for the Section Acknowledgment); nfields[k]
 *      fields in slots sec_off[k] .. + nfields[k] - 1: name_off/name_len/value_off/value_len (arena
 *      offsets) and fflags = soft bits (HHUFF_SOFT_NAME / _VALUE: decode_header's
 *      H2O_HTTP2_ERROR_INVALID_HEADER_CHAR).  Fields before an error stand.
 *      Device arrays; scratch = hhuff_qpack_scratch_size(nconn, header_table_size) bytes of device memory
 *      (16-byte aligned) that holds the tables: pass HHUFF_QPK_CONTINUE to carry them (and the failed
 *      state) over from the previous call -- connection c of this call is connection c of that one;
 *      without it every connection starts with a fresh decoder; the tables hold scratch offsets, not
 *      addresses, so scratch may be moved between calls.  nsec = conn_first[nconn] (host copy).
 *      in_size <= 2^32 - 3 (offsets are u32).  Encoder streams and sections must not overlap in `in`.
 *      Asynchronous on `stream`: a literal pre-pass (every literal of the step decoded at once), the
 *      encoder streams (one lane per connection, entries booked as references), a table pass, the
 *      sections (one lane per section) and a copy pass.  Stream-ordered pool workspace: 16 bytes per input
 *      byte of field sources, 22 per possible literal (one per input byte) and 1.6 of decoded output --
 *      about 40 bytes per input byte; kept by the pool after the call (hhuff_pool_trim). */
#define HHUFF_QPK_CONTINUE 1u
#define HHUFF_QPK_DECOMPRESSION_FAILED 0x30200 /* H2O_HTTP3_ERROR_QPACK_DECOMPRESSION_FAILED, http3_common.h:73 */
#define HHUFF_QPK_ARENA (-300)
#define HHUFF_QPK_SKIPPED (-301)
#define HHUFF_QPK_BLOCKED (-302)
uint64_t hhuff_qpack_scratch_size(uint32_t nconn, uint32_t header_table_size);
int hhuff_qpack_decode(const uint8_t *in, uint64_t in_size, const uint32_t *enc_off, const uint32_t *enc_len,
                       const uint32_t *sec_off, const uint32_t *conn_first, uint32_t nconn, uint32_t nsec,
                       uint32_t header_table_size, uint64_t max_blocked, const uint32_t *num_blocked, uint8_t *arena,
                       const uint64_t *arena_off, uint32_t *name_off, uint32_t *name_len, uint32_t *value_off,
                       uint32_t *value_len, uint8_t *fflags, uint32_t *nfields, int32_t *sstatus,
                       uint64_t *req_insert_count, int32_t *enc_status, uint32_t *enc_consumed, uint64_t *insert_count,
                       void *scratch, uint64_t scratch_size, unsigned flags, void *stream);

/* (2e') HTTP/3 request sections: the same step with h2o_qpack_parse_request (lib/http3/qpack.c:830-858)
 *      applied to every section as h2o's HTTP/3 server calls it (lib/http3/server.c:1540-1545): the
 *      section's fields go through h2o_hpack_parse_request's rules (qpack.c:848, hpack.c:502-637) with no
 *      cache-digest receiver (a cache-digest field is rejected like the other special fields) and a
 *      datagram-flow-id out-parameter; hard errors other than H2O_HTTP2_ERROR_INVALID_HEADER_CHAR become
 *      HHUFF_QPK_DECOMPRESSION_FAILED (normalize_error_code, :822-828); a section that decoded (0 or
 *      -254) with a Required Insert Count other than 0 gets its Section Acknowledgment (send_header_ack,
 *      :642-649: 0x80 | stream_id[k] as a 7-bit prefix integer) in req[k].ack.
 *      sstatus[k] is h2o_qpack_parse_request's return value: 0, -254 (a soft error, *err_desc in
 *      req[k].req.err), HHUFF_QPK_DECOMPRESSION_FAILED, or HHUFF_QPK_BLOCKED / _ARENA / _SKIPPED as for
 *      hhuff_qpack_decode.  fflags carries HHUFF_FIELD_HEADER for the fields h2o_add_header took.
 *      req[k].req.err is HHUFF_HERR_DECODE when decode_header itself failed (its own description). */
typedef struct hhuff_qpack_request {
    hhuff_request_t req;      /* h2o_hpack_parse_request's out-parameters, as for HTTP/2 */
    int32_t datagram_flow_id; /* the field whose value h2o stored in *datagram_flow_id, or -1 */
    uint32_t ack_len;         /* *outbufsize: bytes of ack (0: no acknowledgment) */
    uint8_t ack[16];          /* the Section Acknowledgment instruction */
} hhuff_qpack_request_t;      /* 72 bytes */
#define HHUFF_HERR_DECODE 8u /* a hard error inside QPACK's decode_header (qpack.c:652-752) */
int hhuff_qpack_parse_requests(const uint8_t *in, uint64_t in_size, const uint32_t *enc_off, const uint32_t *enc_len,
                               const uint32_t *sec_off, const uint32_t *conn_first, uint32_t nconn, uint32_t nsec,
                               uint32_t header_table_size, uint64_t max_blocked, const uint32_t *num_blocked,
                               uint8_t *arena, const uint64_t *arena_off, uint32_t *name_off, uint32_t *name_len,
                               uint32_t *value_off, uint32_t *value_len, uint8_t *fflags, uint32_t *nfields,
                               int32_t *sstatus, uint64_t *req_insert_count, int32_t *enc_status, uint32_t *enc_consumed,
                               uint64_t *insert_count, const uint64_t *stream_id, hhuff_qpack_request_t *req,
                               void *scratch, uint64_t scratch_size, unsigned flags, void *stream);

/* (2e'') HTTP/3 response sections, client side: the step of hhuff_qpack_decode with h2o_qpack_parse_response
 *      (lib/http3/qpack.c:860-882) applied to every section as h2o's HTTP/3 client calls it
 *      (lib/common/http3client.c:542-544: a status and a datagram-flow-id out-parameter; the client has no
 *      blocked-streams budget, so pass max_blocked = 0 to match it): h2o_hpack_parse_response's rules on the
 *      section's fields (as hhuff_hpack_parse_responses, heads only), every hard error -- -254 excepted --
 *      normalised to HHUFF_QPK_DECOMPRESSION_FAILED (:877-878), and the Section Acknowledgment only for a
 *      section that parsed with status 0 and a Required Insert Count other than 0 (:880).  sstatus[k] as for
 *      hhuff_qpack_parse_requests. */
typedef struct hhuff_qpack_response_head {
    hhuff_response_t res;  /* h2o_hpack_parse_response's out-parameters */
    uint32_t ack_len;      /* *outbufsize (0: no acknowledgment) */
    uint32_t reserved;
    uint8_t ack[16];       /* the Section Acknowledgment instruction */
} hhuff_qpack_response_head_t; /* 40 bytes */
int hhuff_qpack_parse_responses(const uint8_t *in, uint64_t in_size, const uint32_t *enc_off, const uint32_t *enc_len,
                                const uint32_t *sec_off, const uint32_t *conn_first, uint32_t nconn, uint32_t nsec,
                                uint32_t header_table_size, uint64_t max_blocked, const uint32_t *num_blocked,
                                uint8_t *arena, const uint64_t *arena_off, uint32_t *name_off, uint32_t *name_len,
                                uint32_t *value_off, uint32_t *value_len, uint8_t *fflags, uint32_t *nfields,
                                int32_t *sstatus, uint64_t *req_insert_count, int32_t *enc_status, uint32_t *enc_consumed,
                                uint64_t *insert_count, const uint64_t *stream_id, hhuff_qpack_response_head_t *res,
                                void *scratch, uint64_t scratch_size, unsigned flags, void *stream);

/* (2e''') QPACK decoder sessions: the step of hhuff_qpack_parse_requests / _parse_responses with the layer h2o keeps
 *      around its decoder (lib/http3/server.c) on the device too -- which streams of a connection are parked and at
 *      which Required Insert Count (conn->num_qpack_blocked :133, stream->qpack_blocked_ref :245), which of them may
 *      go on after a step's inserts (qpack_unblock_streams :1950-1966), the release of a reset stream
 *      (cancel_qpack_decoder :562-571, on_stream_destroy :919-922) -- and the connection's decoder stream: the
 *      Section Acknowledgments (send_header_ack, qpack.c:643-650), Stream Cancellations
 *      (h2o_qpack_decoder_send_stream_cancel, :500-504) and Insert Count Increments
 *      (h2o_qpack_decoder_send_state_sync, :487-498), in the form hhuff_qpack_flatten_sessions reads as dec_off /
 *      dec_len.  The arguments behind `slots` are those of hhuff_qpack_parse_requests / _parse_responses without
 *      num_blocked: the session keeps that count.  slots ((2h)) may be NULL: connection c uses slab c, of the
 *      table scratch and of the session state alike.  max_blocked is also the length of a session's list.
 *      State: ds->state holds hhuff_qpack_dsession_state_size(n, max_blocked) bytes, n = slots->nslots with slots
 *      and nconn without: n equal slabs of 16 + 16 max_blocked bytes -- the parked count, the Known Received Count,
 *      then max_blocked entries {stream_id u64, ref u64}, oldest first.  Memory of its own (16-byte aligned):
 *      hhuff_qpack_scratch_size and the table slabs are what they were.  No addresses inside: it may be moved
 *      between calls.  A session starts fresh exactly when its table does (no HHUFF_QPK_CONTINUE, or
 *      HHUFF_CONN_RESET for the connection): nothing parked, Known Received Count 0.
 *      One step of connection c, after the passes of hhuff_qpack_decode, in this order:
 *      1. Its sections in order.  Section k has come up blocked when the sections pass gave it HHUFF_QPK_BLOCKED
 *         (its Required Insert Count is not reached by the table as the step's whole encoder stream left it).
 *         Blocked and stream_id[k] parked already: it stays parked with the ref it has, sstatus[k] stays
 *         HHUFF_QPK_BLOCKED (a resubmission that still waits).  Blocked, not parked, max_blocked streams parked:
 *         sstatus[k] = HHUFF_QPK_DECOMPRESSION_FAILED.  Blocked, not parked, a slot free: {stream_id[k],
 *         req_insert_count[k]} joins the list (server.c:1551-1555).  Any other status except HHUFF_QPK_SKIPPED /
 *         _EINVAL: the stream's entry, if it has one, leaves the list; and when the record carries an
 *         acknowledgment (ack_len > 0) its bytes are appended to the connection's dec_out region and the Known
 *         Received Count rises to req_insert_count[k] if that is larger (RFC 9204 4.4.1).  The caller's contract,
 *         not checked: no later section of a stream is submitted while an earlier one is parked.
 *      2. Its cancellations cancel_id[cancel_first[c] .. cancel_first[c+1]) in order: a parked stream leaves the
 *         list; without HHUFF_QDS_SILENT in cancel_flags a Stream Cancellation (0x40 | stream id, 6-bit prefix) is
 *         appended to dec_out whether or not the stream was parked, as cancel_qpack_decoder sends it.
 *      3. Wake: every parked entry with ref <= the table's insert count leaves the list (server.c:1958), its stream
 *         id written to wake_id[wake_first[c] ..) oldest first; nwake[c] counts them.  The caller submits the woken
 *         streams' sections in its next step, where they are ordinary sections (or resubmits parked sections
 *         speculatively with the inserts: point 1 handles both).  Entries the region wake_first[c+1] -
 *         wake_first[c] cannot hold stay parked and set HHUFF_QDS_WAKE_PENDING in dflags[c]; the scan runs every
 *         step, so they are found again.
 *      4. With HHUFF_QDS_SYNC: n = the table's total inserts - the Known Received Count; when n > 0, an Insert
 *         Count Increment (0x00 | n, 6-bit prefix) is appended and the Known Received Count becomes the total.
 *         (h2o_qpack_decoder_send_state_sync counts every insert since the last sync, whatever was acknowledged
 *         in between; its own encoder refuses such an increment, qpack.c:907-909, and h2o never calls it.  With no
 *         acknowledgment between two syncs the bytes are the reference function's.)
 *      dec_out_len[c] = the step's bytes in dec_out[dec_out_off[c] ..): acknowledgments in section order, then
 *      cancellations, then the increment.  parked[c] = the parked count after the step.  A connection whose
 *      encoder stream has failed (enc_status != 0, now or earlier) emits nothing and wakes nothing: its lengths are
 *      0, its sections HHUFF_QPK_SKIPPED, parked[c] what it was.
 *      Refusal: a connection whose dec_out region is smaller than hhuff_qpack_dsession_out_bound(its sections,
 *      its cancellations), or over which cancel_first decreases, is refused for the step before any pass touches
 *      its table or session, with the outputs of a refused connection of (2h) point 3 -- enc_status and every
 *      sstatus HHUFF_QPK_EINVAL, enc_consumed = insert_count = nfields = req_insert_count = 0, reset records --
 *      and dec_out_len = nwake = parked = dflags = 0.  A connection the slot map refuses is refused here alike.
 *      Stream ids are QUIC's: below 2^62, so an instruction takes at most 10 bytes and the bound holds; an
 *      instruction of a larger id that would cross the region's end is left out whole.
 *      The call returns HHUFF_EINVAL and enqueues nothing for max_blocked above 4096, nconn above 2^31 - 1, a
 *      state_size below hhuff_qpack_dsession_state_size, a NULL required array (state, dec_out, dec_out_off,
 *      dec_out_len, wake_first, nwake, parked, dflags; wake_id unless max_blocked is 0; cancel_id with cancel_first;
 *      stream_id and the records with nsec != 0) or an unknown bit in ds->flags; nconn == 0 returns 0 and enqueues nothing.
 *      Launches: those of hhuff_qpack_parse_requests with the blocked-limit pass replaced by the session pass
 *      (one lane per connection); the refusal test runs inside the encoder-stream pass.  4 nconn bytes more
 *      from the pool when slots is NULL. */
#define HHUFF_QDS_SYNC 1u         /* ds->flags: point 4 */
#define HHUFF_QDS_SILENT 1u       /* cancel_flags: release the slot, send nothing (on_stream_destroy) */
#define HHUFF_QDS_WAKE_PENDING 1u /* dflags: due entries stayed parked because the wake region was full */
typedef struct hhuff_qpack_dsessions {
    void *state;                  /* device: the sessions */
    uint64_t state_size;
    const uint32_t *cancel_first; /* device u32[nconn + 1], or NULL: no cancellations */
    const uint64_t *cancel_id;    /* device u64: the cancelled stream ids */
    const uint8_t *cancel_flags;  /* device u8 per cancellation, or NULL (= all 0): HHUFF_QDS_SILENT */
    uint8_t *dec_out;             /* device: the decoder-stream bytes */
    const uint64_t *dec_out_off;  /* device u64[nconn + 1]: the regions of dec_out */
    uint32_t *dec_out_len;        /* device u32[nconn], written */
    uint64_t *wake_id;            /* device u64: the streams to resume */
    const uint32_t *wake_first;   /* device u32[nconn + 1]: the regions of wake_id */
    uint32_t *nwake;              /* device u32[nconn], written */
    uint32_t *parked;             /* device u32[nconn], written: the parked count after the step */
    uint8_t *dflags;              /* device u8[nconn], written: HHUFF_QDS_WAKE_PENDING */
    uint32_t flags;               /* HHUFF_QDS_SYNC */
} hhuff_qpack_dsessions_t;        /* the struct itself is host memory, read before the call returns */
struct hhuff_conn_slots;          /* (2h) hhuff_conn_slots_t */
uint64_t hhuff_qpack_dsession_state_size(uint32_t n, uint32_t max_blocked); /* 0 for max_blocked above 4096 */
uint64_t hhuff_qpack_dsession_out_bound(uint32_t nsec_of_conn, uint32_t ncancel_of_conn);
int hhuff_qpack_parse_requests_sessions(const hhuff_qpack_dsessions_t *ds, const struct hhuff_conn_slots *slots,
                                        const uint8_t *in, uint64_t in_size, const uint32_t *enc_off,
                                        const uint32_t *enc_len, const uint32_t *sec_off, const uint32_t *conn_first,
                                        uint32_t nconn, uint32_t nsec, uint32_t header_table_size, uint64_t max_blocked,
                                        uint8_t *arena, const uint64_t *arena_off, uint32_t *name_off,
                                        uint32_t *name_len, uint32_t *value_off, uint32_t *value_len, uint8_t *fflags,
                                        uint32_t *nfields, int32_t *sstatus, uint64_t *req_insert_count,
                                        int32_t *enc_status, uint32_t *enc_consumed, uint64_t *insert_count,
                                        const uint64_t *stream_id, hhuff_qpack_request_t *req, void *scratch,
                                        uint64_t scratch_size, unsigned flags, void *stream);
int hhuff_qpack_parse_responses_sessions(const hhuff_qpack_dsessions_t *ds, const struct hhuff_conn_slots *slots,
                                         const uint8_t *in, uint64_t in_size, const uint32_t *enc_off,
                                         const uint32_t *enc_len, const uint32_t *sec_off, const uint32_t *conn_first,
                                         uint32_t nconn, uint32_t nsec, uint32_t header_table_size,
                                         uint64_t max_blocked, uint8_t *arena, const uint64_t *arena_off,
                                         uint32_t *name_off, uint32_t *name_len, uint32_t *value_off,
                                         uint32_t *value_len, uint8_t *fflags, uint32_t *nfields, int32_t *sstatus,
                                         uint64_t *req_insert_count, int32_t *enc_status, uint32_t *enc_consumed,
                                         uint64_t *insert_count, const uint64_t *stream_id,
                                         hhuff_qpack_response_head_t *res, void *scratch, uint64_t scratch_size,
                                         unsigned flags, void *stream);

/* (2f) HTTP/2 response header blocks, encode side (SURVEY f4 encode half): h2o_hpack_flatten_response
 *      (lib/http2/hpack.c:1137-1177) and h2o_hpack_flatten_trailers (:1179-1196) -- and, for h2o's HTTP/2
 *      client (lib/common/http2client.c:1140), h2o_hpack_flatten_request (:1044-1096) -- for many responses of many
 *      connections, with one encoder dynamic table per connection (conn->_output_header_table; do_encode_header
 *      :858-937, at most 32 entries, initial capacity 4096 as lib/http2/connection.c:1847 sets it) kept in
 *      scratch between calls.  A call flattens the responses conn_first[c] .. conn_first[c+1]-1 of every
 *      connection c in order, as lib/http2/stream.c:311-314 / :404-406 and connection.c:1580-1582 call them.
 *        header h    hdr[h]: name in[name_off .. + name_len), value in[value_off .. + value_len), flags:
 *                    HHUFF_HDR_DONT_COMPRESS = h2o_header_t.flags.dont_compress; HHUFF_HDR_TOKEN = the name is
 *                    an h2o token (h2o_iovec_is_token: the header was added with its h2o_token_t) -- set it only
 *                    for names listed in lib/common/token_table.h
 *        response r  res[r] (below): the headers hdr_first .. hdr_first + nhdr - 1 in order (the ranges of two
 *                    responses must not overlap; headers outside every range are ignored); HHUFF_RES_SERVER
 *                    sends server_name (in[server_off .. + server_len), h2o's globalconf->server_name; clear
 *                    it where h2o passes NULL: informational responses); HHUFF_RES_TRAILERS makes r a trailers
 *                    block (flatten_trailers: no :status, server or content-length, END_STREAM);
 *                    HHUFF_RES_REQUEST makes r a request (flatten_request: no :status, server or content-length):
 *                    its first `status` headers are flatten_request's own fields in its order -- :method,
 *                    :scheme, :authority, :path (an old-style CONNECT, method CONNECT without :protocol, has no
 *                    :scheme or :path), :protocol if any, "expect: 100-continue" if send_own_expect -- with
 *                    HHUFF_HDR_TOKEN and no HHUFF_HDR_DONT_COMPRESS; :method GET / POST, :scheme https / http,
 *                    :path / and /index.html among them, and accept-encoding "gzip, deflate" (token) among the
 *                    others, are the one-byte static references h2o writes without its table (:950-985,
 *                    :1083-1086; a scheme named https / http is h2o's H2O_URL_SCHEME_HTTPS / _HTTP);
 *                    HHUFF_RES_PUSH_PROMISE makes r a promise (h2o_hpack_flatten_push_promise, :1098-1135, as
 *                    h2o_http2_stream_send_push_promise calls it): stream_id is the promised stream, written as
 *                    given in the payload's first 4 bytes (big-endian, before the Dynamic Table Size Update),
 *                    parent_stream_id (read only under this flag) goes into every frame header of the block; the
 *                    first frame is a PUSH_PROMISE (type 5; END_HEADERS or no flag, never END_STREAM); `status`
 *                    counts the own fields that lead the header range as for HHUFF_RES_REQUEST (h2o's call has 4:
 *                    :method, :scheme, :authority, :path) with the same one-byte references by place;
 *                    HHUFF_RES_SERVER, HHUFF_RES_END_STREAM and content_length are ignored; the flag together
 *                    with HHUFF_RES_TRAILERS or HHUFF_RES_REQUEST is refused (HHUFF_RES_EINVAL).  Promises,
 *                    responses and trailers of a connection mix freely in conn_first order -- the order they go
 *                    on the wire -- and share the table
 *        out         response r's frames (HEADERS or PUSH_PROMISE, then CONTINUATIONs past max_frame_size -- for
 *                    a promise counted over a payload that includes the 4 id bytes --, fixup_frame_headers
 *                    :1012-1042) at out + out_off[r]; region [out_off[r], out_off[r+1]) (u64, nres + 1 entries);
 *                    hhuff_hpack_response_bound() is enough for any table state
 *      Per response: out_len[r] = bytes written (frame headers included), headers_size[r] = the payload bytes
 *      (h2o_hpack_flatten_response's return value; a promise's 4 id bytes included), rstatus[r] = 0,
 *      HHUFF_RES_SPACE (the frames do not fit the region), HHUFF_RES_EINVAL (status outside 100..999 -- past
 *      nhdr for a request or a promise --, max_frame_size outside 16384..2^24-1, a string past in_size, a promise
 *      flagged as trailers or request too) or HHUFF_RES_SKIPPED (an earlier response of the connection failed:
 *      its table is no longer the peer's, h2o would have dropped the connection).  A failed response writes
 *      nothing and leaves the table as it was, but for the capacity change of its size update where a later
 *      step refused it.
 *      Device arrays; scratch = hhuff_hpack_enc_scratch_size(nconn) bytes (16-byte aligned) holding the
 *      tables: HHUFF_ENC_CONTINUE carries them (and the failed state) over from the previous call; without it
 *      every connection starts with an empty table.  nhdr = headers in hdr, nres = conn_first[nconn] (host
 *      copies).  in_size < 2^32.  Asynchronous on `stream`; stream-ordered pool workspace of 36 bytes per
 *      header and 16 per response (hhuff_pool_trim). */
typedef struct hhuff_hpack_header {
    uint32_t name_off, name_len, value_off, value_len;
    uint32_t flags; /* HHUFF_HDR_* */
} hhuff_hpack_header_t; /* 20 bytes */
#define HHUFF_HDR_DONT_COMPRESS 1u
#define HHUFF_HDR_TOKEN 2u
typedef struct hhuff_hpack_response {
    uint64_t content_length;    /* res.content_length: SIZE_MAX (all ones) sends none */
    uint32_t stream_id, status; /* status: res.status (ignored for trailers; own fields of a request / promise) */
    uint32_t hdr_first, nhdr;
    uint32_t header_table_size; /* conn->peer_settings.header_table_size (header_table_adjust_size, :839-856) */
    uint32_t max_frame_size;    /* conn->peer_settings.max_frame_size */
    uint32_t flags;             /* HHUFF_RES_* */
    uint32_t parent_stream_id;  /* HHUFF_RES_PUSH_PROMISE: the stream of the frame headers; not read otherwise */
} hhuff_hpack_response_t;       /* 40 bytes */
#define HHUFF_RES_END_STREAM 1u /* is_end_stream */
#define HHUFF_RES_SERVER 2u     /* server_name != NULL */
#define HHUFF_RES_TRAILERS 4u   /* h2o_hpack_flatten_trailers */
#define HHUFF_RES_REQUEST 8u    /* h2o_hpack_flatten_request (status = the number of its own fields) */
#define HHUFF_RES_PUSH_PROMISE 16u /* h2o_hpack_flatten_push_promise (stream_id = the promised stream) */
#define HHUFF_ENC_CONTINUE 1u
#define HHUFF_RES_SPACE (-300)
#define HHUFF_RES_SKIPPED (-301)
#define HHUFF_RES_EINVAL (-303)
/* A region size that holds response r whatever its connection's table: name_value_bytes = the sum of its
 * headers' name_len + value_len, server_len = 0 without HHUFF_RES_SERVER.  (h2o's own reservation,
 * hpack.c:1141-1152 with calc_capacity :998-1001, plus the CONTINUATION frame headers.)  A promise fits with
 * server_len = 0: its worst payload is name_value_bytes + 21 nhdr + 4 (the promised id) + 5 (the size update),
 * and the bound allows + 33. */
static inline uint64_t hhuff_hpack_response_bound(uint64_t name_value_bytes, uint32_t nhdr, uint32_t server_len,
                                                  uint32_t max_frame_size)
{
    uint64_t payload = name_value_bytes + 21ull * nhdr + 5 + 5 + (server_len ? 5ull + server_len + 21 : 0) + 23;
    return 9 + payload + 9 * (payload / (max_frame_size ? max_frame_size : 1) + 1);
}
uint64_t hhuff_hpack_enc_scratch_size(uint32_t nconn);
int hhuff_hpack_flatten_responses(const uint8_t *in, uint64_t in_size, const hhuff_hpack_header_t *hdr, uint32_t nhdr,
                                  const hhuff_hpack_response_t *res, const uint32_t *conn_first, uint32_t nconn,
                                  uint32_t nres, uint32_t server_off, uint32_t server_len, uint8_t *out,
                                  const uint64_t *out_off, uint32_t *out_len, uint32_t *headers_size, int32_t *rstatus,
                                  void *scratch, uint64_t scratch_size, unsigned flags, void *stream);

/* (2g) HTTP/3 response HEADERS frames (QPACK encode half): h2o_qpack_flatten_response
 *      (lib/http3/qpack.c:1352-1399) as h2o's HTTP/3 server calls it (lib/http3/server.c:1680-1683): without an
 *      encoder-stream buffer, so the encoder never inserts into its dynamic table (:1175-1176) and every response
 *      stands alone -- :status, server (HHUFF_RES_SERVER), content-length, the headers (static-table references
 *      through h2o_qpack_lookup_static for token names, literals otherwise; do_flatten_header :1148-1213),
 *      datagram-flow-id (HHUFF_QRES_DATAGRAM: in[dfid_off .. + dfid_len)), behind the section prefix 00 00 and
 *      the HEADERS frame header (type 0x01, QUIC varint length; finalize_flatten :1265-1310).
 *        header h    hdr[h] as for hhuff_hpack_flatten_responses (HHUFF_HDR_TOKEN, HHUFF_HDR_DONT_COMPRESS); the
 *                    ranges hdr_first .. + nhdr of two responses must not overlap
 *        request     HHUFF_QRES_REQUEST: h2o_qpack_flatten_request (:1312-1350) as h2o's HTTP/3 client calls it
 *                    (lib/common/http3client.c:792, no encoder-stream buffer): no :status, server or content-length;
 *                    the headers start with its own fields as for HHUFF_RES_REQUEST (no expect: HTTP/3 has no
 *                    send_own_expect), which flatten exactly as token headers do (its static-indexed http / https
 *                    scheme, :1325-1329, is the static lookup's exact match); datagram-flow-id last as for responses
 *        out         frame r at out + out_off[r]; region [out_off[r], out_off[r+1]) (u64, nres + 1 entries):
 *                    hhuff_qpack_response_bound() always fits
 *      out_len[r] = frame bytes, header_len[r] = *serialized_header_len (the field section, frame header
 *      excluded), rstatus[r] = 0, HHUFF_RES_SPACE or HHUFF_RES_EINVAL (a string past in_size); a failed
 *      response writes nothing.  Device arrays; in_size < 2^32; asynchronous on `stream`; stream-ordered pool
 *      workspace of 24 bytes per header and 32 per response. */
typedef struct hhuff_qpack_response {
    uint64_t content_length; /* res.content_length: SIZE_MAX (all ones) sends none */
    uint32_t status;         /* res.status: a static entry, else the decimal of (uint16_t)status against :status;
                                HHUFF_QRES_REQUEST: the number of own fields (the bytes do not depend on it) */
    uint32_t hdr_first, nhdr;
    uint32_t flags;          /* HHUFF_RES_SERVER, HHUFF_QRES_DATAGRAM */
    uint32_t dfid_off, dfid_len;
} hhuff_qpack_response_t;    /* 32 bytes */
#define HHUFF_QRES_DATAGRAM 8u
#define HHUFF_QRES_REQUEST 16u /* h2o_qpack_flatten_request: status = the number of its own fields */
static inline uint64_t hhuff_qpack_response_bound(uint64_t name_value_bytes, uint32_t nhdr, uint32_t server_len,
                                                  uint32_t dfid_len)
{
    return 9 + 2 + 8 + 23 + 26 + (uint64_t)dfid_len + (server_len ? 12ull + server_len : 0) + 21ull * nhdr +
           name_value_bytes;
}
int hhuff_qpack_flatten_responses(const uint8_t *in, uint64_t in_size, const hhuff_hpack_header_t *hdr, uint32_t nhdr,
                                  const hhuff_qpack_response_t *res, uint32_t nres, uint32_t server_off,
                                  uint32_t server_len, uint8_t *out, const uint64_t *out_off, uint32_t *out_len,
                                  uint32_t *header_len, int32_t *rstatus, void *stream);

/* (2g') HTTP/3 encoder sessions: h2o_qpack_flatten_response / _request WITH an encoder-stream buffer
 *      (lib/http3/qpack.c:1148-1213, :1244-1310) and h2o_qpack_encoder_handle_input (:902-1005) for many
 *      connections, each with its own encoder: a dynamic table, the list of sections the peer has not
 *      acknowledged yet (inflight) and largest_known_received, kept in scratch between calls.  One call is one
 *      step of every connection c, in the order h2o reaches them on a connection:
 *        1. decoder stream in[dec_off[c] .. + dec_len[c]) (dec_off == NULL: none) through handle_input:
 *           Insert Count Increment (00, 6-bit prefix; an error when the increment is 0 or
 *           largest_known_received + n >= total_inserts, the table's count plus 1), Section Acknowledgment
 *           (1, 7-bit; the first inflight entry of the stream leaves, largest_known_received rises to its
 *           largest_ref, num_blocked drops if it was blocking; an unknown stream is an error), Stream
 *           Cancellation (01, 6-bit; every inflight entry of the stream leaves; never an error).
 *           dec_consumed[c] = bytes of the complete instructions taken (an instruction cut inside its integer
 *           is no error: the rest waits, as enc_consumed does on the decode side); dec_status[c] = 0,
 *           HHUFF_QPK_DECODER_STREAM, HHUFF_QPK_DECOMPRESSION_FAILED (an integer that overflows),
 *           HHUFF_QPK_SKIPPED (an earlier step failed) or HHUFF_RES_EINVAL (dec_off + dec_len past in_size).
 *           After any of these but 0, this step's responses and every later response of the connection get
 *           HHUFF_RES_SKIPPED and write nothing.
 *        2. the responses conn_first[c] .. conn_first[c+1]-1 in order (records, headers, own fields, frame
 *           header, out regions and header_len[] as for hhuff_qpack_flatten_responses), response r on the
 *           request stream stream_id[r].
 *      Table: 1-based, never evicts (but see HHUFF_QENC_EVICT below); an insert needs name_len + value_len + 32 <= header_table_size - used;
 *      base_index = the insert count at the section's start.  The section has an encoder buffer only without
 *      HHUFF_QRES_NO_ENCODER_STREAM and with num_blocked < max_blocked at its start (:1250).
 *      Lookup (lookup_dynamic): newest to oldest, the first entry with the name and value, else the newest with
 *      the name; without an encoder buffer only entries <= largest_known_received.  Names compare by bytes
 *      (h2o compares token names by pointer: the same, since only token names are ever inserted).
 *      Per field, in this order: an exact static match -> static indexed; an exact dynamic match -> dynamic
 *      indexed (pre-base 0x80 6-bit, post-base 0x10 4-bit); likely_to_repeat && buffer && ((no static && no
 *      dynamic name match) || value_len >= 8) && it fits -> an insert on the encoder stream (0xC0 static name
 *      reference, 0x80 dynamic name reference, 0x40 name string with prefix 5; then the value string, prefix 7)
 *      and a post-base reference to the new entry; else a static name reference; else a dynamic name reference
 *      (0x40|N 4-bit pre-base, 0x00|N<<3 3-bit post-base); else a literal with a literal name.  The call's own
 *      fields carry h2o's token flags: server is likely to repeat, :status, content-length and
 *      datagram-flow-id are not.  A request's own fields are headers; set HHUFF_HDR_LIKELY_TO_REPEAT on
 *      :authority and :protocol.
 *      Section prefix (:1263-1298): no dynamic reference -> 00 00 and nothing becomes inflight.  Otherwise
 *      largest_ref below largest_known_received is raised to it; above it the section is blocking
 *      (++num_blocked); {stream_id, largest_ref, blocking} joins the inflight list; Required Insert Count =
 *      largest_ref + 1 (8-bit prefix), then the delta base with its sign bit (7-bit prefix).
 *      Three deliberate differences from the reference: Insert With Name Reference on a dynamic
 *      name writes the RELATIVE index (insert count - 1 - absolute, RFC 9204 4.3.2; the reference writes the
 *      absolute one, :1177/:1073, which its own decoder :336-341 misreads); an inflight entry is removed entry
 *      by entry (:928 moves size - index bytes); the inflight list holds max_inflight entries per connection: a
 *      section that would need a slot when it is full is flattened as with no encoder at all -- the bytes of
 *      hhuff_qpack_flatten_responses --, rflags[r] |= 1, rstatus[r] = 0, no state change.
 *      Outputs: out_len[r], header_len[r]; rstatus[r] = 0, HHUFF_RES_EINVAL, HHUFF_RES_SPACE (the frame does
 *      not fit its region, or the section's inserts do not fit what is left of the connection's encoder-stream
 *      region) or HHUFF_RES_SKIPPED; a failed response writes nothing and changes no state (the connection goes
 *      on).  enc_out_len[c] = the step's encoder-stream bytes at enc_out + enc_out_off[c] (region up to
 *      enc_out_off[c+1]): header_table_size + 4 bytes always fit, because the table never evicts.  With
 *      HHUFF_QENC_SET_CAPACITY a call without HHUFF_QENC_CONTINUE starts every encoder stream with Set Dynamic
 *      Table Capacity; where not even that fits, the step's responses get HHUFF_RES_SPACE.
 *      hhuff_qpack_session_response_bound() always fits a response's region.
 *      Device arrays; scratch = hhuff_qpack_enc_scratch_size(nconn, header_table_size, max_inflight) bytes
 *      (16-byte aligned): HHUFF_QENC_CONTINUE carries tables, inflight lists and failed state over from the
 *      previous call (same nconn, header_table_size, max_inflight); the tables hold scratch offsets, not
 *      addresses, so scratch may be moved between calls.  header_table_size <= 65536 (else the call
 *      returns HHUFF_RES_EINVAL).  nres = conn_first[nconn] (host copy).  in_size < 2^32.  Asynchronous on `stream`: a prep pass
 *      (one lane per header), the walk (one lane per connection: decides, writes no output byte), the emit pass
 *      (one lane per field, insert and response head).  Stream-ordered pool workspace of 124 bytes per header,
 *      112 per response and 16 per connection.
 *
 *      HHUFF_QENC_EVICT: the table evicts entries no section still needs (a fourth deliberate difference: h2o's
 *      encoder "never triggers eviction", :1168-1170).  Without the flag everything above holds unchanged.  A
 *      session is evicting or it is not: a call with HHUFF_QENC_CONTINUE whose flag differs from the one the
 *      scratch was started with is refused with HHUFF_RES_EINVAL.  The mode lives in the scratch, on the device,
 *      and the call is asynchronous, so the refusal is reported per connection: dec_status[c] and every
 *      rstatus[r] of the connection are HHUFF_RES_EINVAL, nothing is written and the scratch stays as it was.
 *      Under the flag:
 *        1. Indices.  Entries keep absolute 1-based indices; count = the total number of inserts, evicted = the
 *           number of entries gone, the live entries are evicted+1 .. count and `used` counts them alone.
 *           lookup_dynamic scans from count (without an encoder buffer: from min(largest_known_received, count))
 *           down to evicted+1.  The Insert Count Increment check still uses count.
 *        2. Pins.  Entry i is pinned while an inflight section's smallest reference is <= i, or the section
 *           being flattened has already referenced an index <= i, or i is the dynamic entry this insert's
 *           instruction names (Insert With Name Reference, dynamic).  Section Acknowledgment and Stream
 *           Cancellation release a section's pins, nothing more.
 *        3. Insert rule.  The condition above with another room test; need = name_len + value_len + 32.  The
 *           insert happens iff need <= header_table_size and the oldest live entries, taken in order and
 *           stopping at the first pinned one, free enough that used + need <= header_table_size.  Then exactly
 *           the shortest such prefix is evicted and the entry inserted; else nothing is evicted and the field
 *           falls through to the static name reference, dynamic name reference or literal form.  No Duplicate
 *           instruction, no draining heuristic (but see point 7).  A connection stops inserting at
 *           count == 2^31 - 1.
 *        4. Section prefix.  Required Insert Count = (largest_ref mod (2 * (header_table_size / 32))) + 1
 *           (RFC 9204 4.5.1.1; the bytes above while largest_ref < 2 * (header_table_size / 32)); the delta base
 *           is unchanged.
 *        5. Transactions.  A failed response writes nothing and changes no state; since an eviction cannot be
 *           undone, every refusal is decided before the section touches the table.  HHUFF_RES_EINVAL: a string
 *           past in_size or a bad range, as above.  HHUFF_RES_SPACE: the response's region is smaller than
 *           hhuff_qpack_session_response_bound() of it (its headers' name and value bytes, its nhdr, server_len
 *           when it sends the server name, dfid_len when it has HHUFF_QRES_DATAGRAM) or that bound is 2^32 or
 *           more; or the section has an encoder buffer and the room left in the connection's encoder-stream
 *           region is smaller than its insert bound: the sum of 20 + name_len + value_len over its headers with
 *           HHUFF_HDR_TOKEN | HHUFF_HDR_LIKELY_TO_REPEAT and over the server name when it sends it.  A section
 *           that starts with the inflight list full (max_inflight entries) is flattened as with no encoder at
 *           all, rflags[r] |= 1, whether or not it would have needed a slot.
 *           hhuff_qpack_session_enc_bound() always fits a connection's encoder-stream region for a step;
 *           "header_table_size + 4 bytes always fit" holds only without the flag.
 *        6. hhuff_qpack_enc_scratch_size() is the same with and without the flag.
 *        7. HHUFF_QENC_DUP (opt-in, valid only together with HHUFF_QENC_EVICT: alone it is known on the host and
 *           the call returns HHUFF_RES_EINVAL; without it every byte, status and scratch word is as above).  An
 *           entry that every section keeps referring to ends up the oldest, is pinned whenever an insert asks
 *           for room, and the table stops turning over behind it; with the flag such an entry is re-inserted by
 *           a Duplicate instruction while it can still be evicted.
 *           Draining.  For a live entry i, older(i) = the sum of name_len + value_len + 32 over the live entries
 *           evicted+1 .. i-1, and headroom(i) = (header_table_size - used) + older(i): the bytes of inserts the
 *           table can still take before i has to go.  Entry i is draining iff headroom(i) <
 *           header_table_size / 4 (integer division).  The quarter is a constant of this contract, like
 *           max_inflight's meaning, not a tuned number: no entry of a table with room for another quarter is
 *           draining, and in a full table the oldest quarter by bytes is.
 *           Rule.  At "an exact dynamic match -> dynamic indexed" of the per-field order: when the section has
 *           an encoder buffer, the field is likely to repeat (the test an insert uses: HHUFF_HDR_TOKEN |
 *           HHUFF_HDR_LIKELY_TO_REPEAT, or the server name) and the matched entry i is draining, point 3's room
 *           test runs with need = name_len + value_len + 32.  Its pins are the inflight sections' smallest
 *           references and the smallest reference of the section being flattened so far; i itself is NOT a
 *           pin, so the evicted prefix may include the source (RFC 9204 3.2.2: the decoder resolves the index
 *           before it evicts).  If the test succeeds, the encoder stream gets Duplicate (000 pattern, 5-bit
 *           prefix) with the relative index count - i, count taken before the insert; exactly that prefix is
 *           evicted; a new entry with the field's name and value is inserted; the field is the post-base
 *           indexed reference to the new entry, as after an insert.  Otherwise nothing changes: the indexed
 *           reference to i.
 *           Unchanged.  Lookup is newest first, so later fields and sections find the duplicate, which is not
 *           draining.  A name-only match still inserts with a dynamic name reference and pins that entry; it is
 *           never duplicated.  The wrapped Required Insert Count, the transactions of point 5, both bound
 *           helpers (a Duplicate is at most 3 bytes, under the 20 + name_len + value_len counted for the same
 *           field) and hhuff_qpack_enc_scratch_size() are as above.
 *           Mode.  A session is duplicating for its whole life: a call with HHUFF_QENC_CONTINUE whose
 *           HHUFF_QENC_DUP bit differs from the one the scratch was started with is refused per connection
 *           exactly as the HHUFF_QENC_EVICT mismatch is. */
#define HHUFF_HDR_LIKELY_TO_REPEAT 4u    /* h2o_token_t.flags.likely_to_repeat of the header's token (caller-supplied,
                                            like HHUFF_HDR_TOKEN; meaningful only with HHUFF_HDR_TOKEN) */
#define HHUFF_QRES_NO_ENCODER_STREAM 32u /* this response is flattened with encoder_buf == NULL */
#define HHUFF_QENC_CONTINUE 1u
#define HHUFF_QENC_SET_CAPACITY 2u       /* 0x20 | 5-bit-prefix int header_table_size */
#define HHUFF_QENC_EVICT 4u              /* the table evicts entries no section still needs (contract above) */
#define HHUFF_QENC_DUP 8u                /* with HHUFF_QENC_EVICT only: draining entries are duplicated (point 7) */
#define HHUFF_QPK_DECODER_STREAM 0x30202 /* H2O_HTTP3_ERROR_QPACK_DECODER_STREAM */
/* the longer section prefix and dynamic indices at up to 2,048 entries */
static inline uint64_t hhuff_qpack_session_response_bound(uint64_t name_value_bytes, uint32_t nhdr, uint32_t server_len,
                                                          uint32_t dfid_len)
{
    uint64_t bound = hhuff_qpack_response_bound(name_value_bytes, nhdr, server_len, dfid_len);
    return bound + 8;
}
/* a connection's encoder-stream bytes of one step with HHUFF_QENC_EVICT: Set Dynamic Table Capacity, the insert
 * bounds of its headers with HHUFF_HDR_TOKEN | HHUFF_HDR_LIKELY_TO_REPEAT and of the server name per response */
static inline uint64_t hhuff_qpack_session_enc_bound(uint64_t name_value_bytes_of_ltr_headers, uint32_t n_ltr_headers,
                                                     uint32_t server_len, uint32_t nres_of_conn)
{
    return 4 + name_value_bytes_of_ltr_headers + 20ull * n_ltr_headers +
           (server_len ? (uint64_t)nres_of_conn * (26ull + server_len) : 0);
}
uint64_t hhuff_qpack_enc_scratch_size(uint32_t nconn, uint32_t header_table_size, uint32_t max_inflight);
int hhuff_qpack_flatten_sessions(const uint8_t *in, uint64_t in_size, const hhuff_hpack_header_t *hdr, uint32_t nhdr,
                                 const hhuff_qpack_response_t *res, const uint32_t *conn_first, uint32_t nconn,
                                 uint32_t nres, const uint64_t *stream_id, const uint32_t *dec_off,
                                 const uint32_t *dec_len, uint32_t header_table_size, uint64_t max_blocked,
                                 uint32_t max_inflight, uint32_t server_off, uint32_t server_len, uint8_t *out,
                                 const uint64_t *out_off, uint32_t *out_len, uint32_t *header_len, int32_t *rstatus,
                                 uint8_t *rflags, uint8_t *enc_out, const uint64_t *enc_out_off, uint32_t *enc_out_len,
                                 int32_t *dec_status, uint32_t *dec_consumed, void *scratch, uint64_t scratch_size,
                                 unsigned flags, void *stream);

/* (2g'') Encoder sessions with per-connection peer settings.  h2o creates a connection's encoder from that peer's
 *      SETTINGS frame (lib/http3/common.c:1441-1468, h2o_qpack_create_encoder, qpack.c:884): its table capacity is
 *      min(the peer's SETTINGS_QPACK_MAX_TABLE_CAPACITY, our own encoder_table_capacity), its blocked-stream limit
 *      the peer's SETTINGS_QPACK_BLOCKED_STREAMS.  hhuff_qpack_flatten_sessions_peers is
 *      hhuff_qpack_flatten_sessions_slots (2h) with one record per connection of the call in front; a batch that
 *      mixes peers goes through one call and one scratch of equal slabs.  peers == NULL is the _slots call: the
 *      same bytes, statuses, scratch contents, launches and workspace.  With peers given (device, [nconn],
 *      4-byte aligned), H = the call's header_table_size still fixes the slab stride and
 *      hhuff_qpack_enc_scratch_size(), and per connection c:
 *      1. Capacity.  cap_c = min(peers[c].max_table_capacity, H) stands wherever (2g') uses header_table_size as
 *         a capacity: the insert room tests of both table kinds, need <= header_table_size of point 3, the
 *         draining quarter cap_c / 4 of point 7, the value HHUFF_QENC_SET_CAPACITY writes, and
 *         "header_table_size + 4 bytes always fit", which is cap_c + 4.  The entry ring and the string area keep
 *         the slab's geometry (H / 32 slots, H bytes).
 *      2. MaxEntries.  The wrapped Required Insert Count of point 4 is (largest_ref mod (2 *
 *         (peers[c].max_table_capacity / 32))) + 1: RFC 9204 4.5.1.1 takes MaxEntries from the capacity the
 *         decoder advertised, not from the one the encoder chose to use.  With fewer than 32 bytes advertised
 *         nothing is ever inserted and no section has a dynamic reference.  With max_table_capacity <= H this is
 *         the modulus of (2g') at header_table_size = cap_c.
 *      3. Blocked streams.  A section has an encoder buffer when num_blocked < min(peers[c].max_blocked,
 *         max_blocked): the call's own max_blocked stays as the server's cap (UINT64_MAX: the peer's value alone).
 *      4. Equivalence.  For a connection with max_table_capacity <= H every byte of out and enc_out, every status,
 *         length and flag is what hhuff_qpack_flatten_sessions_slots produces for it with header_table_size =
 *         max_table_capacity and max_blocked = min(peers[c].max_blocked, max_blocked).
 *      5. Stability.  A peer's SETTINGS arrive once (RFC 9114 7.2.4): peers[c] must be the same in every step of
 *         a connection's life.  The session does not store it.  One violation is caught: a continuing connection
 *         whose table holds more than cap_c bytes is refused for the step exactly like the mode mismatch --
 *         dec_status[c] and every rstatus[r] = HHUFF_RES_EINVAL, nothing written, the slab untouched.  Any other
 *         change is the caller's error; it stays memory-safe because cap_c <= H always.  A fresh connection (a
 *         call without HHUFF_QENC_CONTINUE, or HHUFF_CONN_RESET) takes whatever peers[c] says: that is how a slot
 *         is reused by another peer.
 *      6. The call returns HHUFF_EINVAL and enqueues nothing for a peers pointer that is not 4-byte aligned;
 *         everything the _slots call refuses is refused alike.
 *      No launch and no workspace beyond the _slots call's. */
typedef struct hhuff_qpack_peer {
    uint32_t max_table_capacity; /* the peer's SETTINGS_QPACK_MAX_TABLE_CAPACITY; 0 when it sent none;
                                    the caller saturates larger values at 2^32 - 1 */
    uint32_t max_blocked;        /* the peer's SETTINGS_QPACK_BLOCKED_STREAMS, saturated likewise */
} hhuff_qpack_peer_t;            /* 8 bytes */
struct hhuff_conn_slots;         /* (2h) */
int hhuff_qpack_flatten_sessions_peers(const hhuff_qpack_peer_t *peers, const struct hhuff_conn_slots *slots,
                                       const uint8_t *in, uint64_t in_size, const hhuff_hpack_header_t *hdr,
                                       uint32_t nhdr, const hhuff_qpack_response_t *res, const uint32_t *conn_first,
                                       uint32_t nconn, uint32_t nres, const uint64_t *stream_id,
                                       const uint32_t *dec_off, const uint32_t *dec_len, uint32_t header_table_size,
                                       uint64_t max_blocked, uint32_t max_inflight, uint32_t server_off,
                                       uint32_t server_len, uint8_t *out, const uint64_t *out_off, uint32_t *out_len,
                                       uint32_t *header_len, int32_t *rstatus, uint8_t *rflags, uint8_t *enc_out,
                                       const uint64_t *enc_out_off, uint32_t *enc_out_len, int32_t *dec_status,
                                       uint32_t *dec_consumed, void *scratch, uint64_t scratch_size, unsigned flags,
                                       void *stream);

/* (2h) Connection slots: connections that come and go.  The four stateful families above -- HPACK blocks
 *      (hhuff_hpack_decode_blocks / _parse_requests / _parse_responses), the QPACK decoder step (hhuff_qpack_decode
 *      / _parse_requests / _parse_responses), the HPACK encoder (hhuff_hpack_flatten_responses) and the QPACK
 *      encoder sessions (hhuff_qpack_flatten_sessions) -- keep one slab of scratch per connection, address it by the
 *      connection's position in the call, and start every connection fresh or none (their *_CONTINUE flag).  Each
 *      has a _slots variant that takes a hhuff_conn_slots_t first and is otherwise the same function: scratch is
 *      then `nslots` slabs (scratch_size >= hhuff_*_scratch_size(nslots, ...)), the call lists only the nconn
 *      connections that have something this step, in any order, and says per connection which slab is its own and
 *      whether it starts fresh there.  slots == NULL is the function without the suffix: the same bytes, statuses
 *      and scratch contents, no launch and no workspace more.
 *      1. Addressing.  Connection c of the call uses slab slot[c].  Offsets kept inside the tables stay relative
 *         to scratch, so scratch may still be moved between calls.  The call neither reads nor writes the slab of
 *         a slot no listed connection owns.
 *      2. Freshness.  Connection c starts fresh when the call has no *_CONTINUE flag, or when flags[c] has
 *         HHUFF_CONN_RESET: exactly what a call without *_CONTINUE does for that family -- an empty table at its
 *         initial capacity, the failed state cleared.  For a QPACK encoder session it is a new encoder: table,
 *         inflight list and largest_known_received empty, num_blocked 0, the session's mode taken from this call's
 *         HHUFF_QENC_EVICT / HHUFF_QENC_DUP bits (the mode-mismatch refusal applies to continuing connections
 *         only), and with HHUFF_QENC_SET_CAPACITY its encoder stream opens with Set Dynamic Table Capacity.
 *      3. Ownership.  A slot belongs to the lowest-numbered connection of the call that names it.  A connection
 *         is refused when it names a slot >= nslots, a slot an earlier connection of the call owns, or carries a
 *         flag bit other than HHUFF_CONN_RESET.  A refused connection touches no slab and writes no payload byte:
 *           HPACK blocks    bstatus = HHUFF_BLK_EINVAL, nfields = 0, req / res = the record of a reset state
 *           QPACK decode    enc_status and every sstatus = HHUFF_QPK_EINVAL, enc_consumed = insert_count = 0,
 *                           nfields = req_insert_count = 0, req / res = the record of a reset state (no ack)
 *           HPACK encode    every rstatus = HHUFF_RES_EINVAL, out_len = headers_size = 0
 *           QPACK sessions  dec_status and every rstatus = HHUFF_RES_EINVAL, dec_consumed = enc_out_len = 0,
 *                           out_len = header_len = 0
 *         Two calls in flight on different streams must name disjoint slots: the caller's contract, not checked.
 *      4. The call returns HHUFF_EINVAL and enqueues nothing when nslots is 0 or above 2^31 - 1, scratch_size is
 *         below nslots slabs, or slot is NULL and nconn > nslots.
 *      The call takes 4 (nconn + nslots) bytes more from the library's pool and runs two small kernels ahead of
 *      the family's own (none of it when slot and flags are both NULL). */
#define HHUFF_CONN_RESET 1u /* this connection starts fresh in its slot, whatever *_CONTINUE says */
typedef struct hhuff_conn_slots {
    const uint32_t *slot; /* device u32[nconn]: the scratch slot of the call's connection c; NULL: slot c = c */
    const uint8_t *flags; /* device u8[nconn] or NULL (= all 0): HHUFF_CONN_*; other bits must be 0 */
    uint32_t nslots;      /* slots in scratch: scratch_size >= hhuff_*_scratch_size(nslots, ...) */
} hhuff_conn_slots_t;     /* the struct itself is host memory, read before the call returns */
#define HHUFF_BLK_EINVAL (-303) /* bstatus: the block's connection was refused (point 3) */
#define HHUFF_QPK_EINVAL (-303) /* enc_status / sstatus: the connection was refused (point 3) */
int hhuff_hpack_decode_blocks_slots(const hhuff_conn_slots_t *slots, const uint8_t *in, uint64_t in_size,
                                    const uint32_t *blk_off, const uint32_t *conn_first, uint32_t nconn,
                                    uint32_t table_size, uint8_t *arena, const uint64_t *arena_off, uint32_t *name_off,
                                    uint32_t *name_len, uint32_t *value_off, uint32_t *value_len, uint8_t *fflags,
                                    uint32_t *nfields, int32_t *bstatus, void *scratch, uint64_t scratch_size,
                                    unsigned flags, void *stream);
int hhuff_hpack_parse_requests_slots(const hhuff_conn_slots_t *slots, const uint8_t *in, uint64_t in_size,
                                     const uint32_t *blk_off, const uint32_t *conn_first, uint32_t nconn,
                                     uint32_t table_size, uint8_t *arena, const uint64_t *arena_off, uint32_t *name_off,
                                     uint32_t *name_len, uint32_t *value_off, uint32_t *value_len, uint8_t *fflags,
                                     uint32_t *nfields, int32_t *bstatus, hhuff_request_t *req, void *scratch,
                                     uint64_t scratch_size, unsigned flags, void *stream);
int hhuff_hpack_parse_responses_slots(const hhuff_conn_slots_t *slots, const uint8_t *in, uint64_t in_size,
                                      const uint32_t *blk_off, const uint32_t *conn_first, uint32_t nconn,
                                      uint32_t table_size, const uint8_t *trailers, uint8_t *arena,
                                      const uint64_t *arena_off, uint32_t *name_off, uint32_t *name_len,
                                      uint32_t *value_off, uint32_t *value_len, uint8_t *fflags, uint32_t *nfields,
                                      int32_t *bstatus, hhuff_response_t *res, void *scratch, uint64_t scratch_size,
                                      unsigned flags, void *stream);
int hhuff_qpack_decode_slots(const hhuff_conn_slots_t *slots, const uint8_t *in, uint64_t in_size,
                             const uint32_t *enc_off, const uint32_t *enc_len, const uint32_t *sec_off,
                             const uint32_t *conn_first, uint32_t nconn, uint32_t nsec, uint32_t header_table_size,
                             uint64_t max_blocked, const uint32_t *num_blocked, uint8_t *arena,
                             const uint64_t *arena_off, uint32_t *name_off, uint32_t *name_len, uint32_t *value_off,
                             uint32_t *value_len, uint8_t *fflags, uint32_t *nfields, int32_t *sstatus,
                             uint64_t *req_insert_count, int32_t *enc_status, uint32_t *enc_consumed,
                             uint64_t *insert_count, void *scratch, uint64_t scratch_size, unsigned flags, void *stream);
int hhuff_qpack_parse_requests_slots(const hhuff_conn_slots_t *slots, const uint8_t *in, uint64_t in_size,
                                     const uint32_t *enc_off, const uint32_t *enc_len, const uint32_t *sec_off,
                                     const uint32_t *conn_first, uint32_t nconn, uint32_t nsec,
                                     uint32_t header_table_size, uint64_t max_blocked, const uint32_t *num_blocked,
                                     uint8_t *arena, const uint64_t *arena_off, uint32_t *name_off, uint32_t *name_len,
                                     uint32_t *value_off, uint32_t *value_len, uint8_t *fflags, uint32_t *nfields,
                                     int32_t *sstatus, uint64_t *req_insert_count, int32_t *enc_status,
                                     uint32_t *enc_consumed, uint64_t *insert_count, const uint64_t *stream_id,
                                     hhuff_qpack_request_t *req, void *scratch, uint64_t scratch_size, unsigned flags,
                                     void *stream);
int hhuff_qpack_parse_responses_slots(const hhuff_conn_slots_t *slots, const uint8_t *in, uint64_t in_size,
                                      const uint32_t *enc_off, const uint32_t *enc_len, const uint32_t *sec_off,
                                      const uint32_t *conn_first, uint32_t nconn, uint32_t nsec,
                                      uint32_t header_table_size, uint64_t max_blocked, const uint32_t *num_blocked,
                                      uint8_t *arena, const uint64_t *arena_off, uint32_t *name_off, uint32_t *name_len,
                                      uint32_t *value_off, uint32_t *value_len, uint8_t *fflags, uint32_t *nfields,
                                      int32_t *sstatus, uint64_t *req_insert_count, int32_t *enc_status,
                                      uint32_t *enc_consumed, uint64_t *insert_count, const uint64_t *stream_id,
                                      hhuff_qpack_response_head_t *res, void *scratch, uint64_t scratch_size,
                                      unsigned flags, void *stream);
int hhuff_hpack_flatten_responses_slots(const hhuff_conn_slots_t *slots, const uint8_t *in, uint64_t in_size,
                                        const hhuff_hpack_header_t *hdr, uint32_t nhdr,
                                        const hhuff_hpack_response_t *res, const uint32_t *conn_first, uint32_t nconn,
                                        uint32_t nres, uint32_t server_off, uint32_t server_len, uint8_t *out,
                                        const uint64_t *out_off, uint32_t *out_len, uint32_t *headers_size,
                                        int32_t *rstatus, void *scratch, uint64_t scratch_size, unsigned flags,
                                        void *stream);
int hhuff_qpack_flatten_sessions_slots(const hhuff_conn_slots_t *slots, const uint8_t *in, uint64_t in_size,
                                       const hhuff_hpack_header_t *hdr, uint32_t nhdr, const hhuff_qpack_response_t *res,
                                       const uint32_t *conn_first, uint32_t nconn, uint32_t nres,
                                       const uint64_t *stream_id, const uint32_t *dec_off, const uint32_t *dec_len,
                                       uint32_t header_table_size, uint64_t max_blocked, uint32_t max_inflight,
                                       uint32_t server_off, uint32_t server_len, uint8_t *out, const uint64_t *out_off,
                                       uint32_t *out_len, uint32_t *header_len, int32_t *rstatus, uint8_t *rflags,
                                       uint8_t *enc_out, const uint64_t *enc_out_off, uint32_t *enc_out_len,
                                       int32_t *dec_status, uint32_t *dec_consumed, void *scratch,
                                       uint64_t scratch_size, unsigned flags, void *stream);

/* (2i) Connection images: a connection's state leaves the scratch it was born in.  The slabs of the families of
 *      (2h), and the decoder sessions of (2e'''), keep scratch-relative offsets and ring positions, and their
 *      stride is fixed by nslots: a slab copied elsewhere points back at the old place.  hhuff_conn_export
 *      serialises listed slots into compact, position-independent, versioned images; hhuff_conn_import rebuilds a
 *      slab from an image in any slot of any scratch of the same family parameters, on any device.  An image is
 *      plain bytes: the caller moves it (hipMemcpyAsync, hipMemcpyPeerAsync) or keeps it -- a checkpoint, a fork,
 *      a scratch that grows or shrinks, a connection that follows its load to another GPU.
 *      slot[n], img, img_off[n + 1] (u64, every entry a multiple of 16), img_len[n] and status[n] are device
 *      arrays; item k's region is img[img_off[k] .. img_off[k + 1]).  Both calls are asynchronous on `stream`.
 *      1. Slab size.  hhuff_conn_slab_size(fam) = the family's bytes per slot: hhuff_hpack_scratch_size(1,
 *         table_size), hhuff_qpack_scratch_size(1, table_size), hhuff_hpack_enc_scratch_size(1),
 *         hhuff_qpack_enc_scratch_size(1, table_size, max_inflight), hhuff_qpack_dsession_state_size(1,
 *         max_blocked).  It is 0 for parameters the family's own call refuses -- table_size over 65536 for
 *         QPACK_ENC and over 2^30 for QPACK_DEC, max_blocked over 4096 for QPACK_DSESSION -- for an HPACK_DEC
 *         table_size over 2^30 (an image's length is a u32), for an unknown family and for a non-zero unused
 *         field.  Both calls return HHUFF_EINVAL and enqueue nothing when the slab size is 0, nslots is 0 or above
 *         2^31 - 1, scratch_size is below nslots slabs, scratch or img is not 16-byte aligned, or an array is NULL
 *         (but img == NULL in export, point 3).  n == 0 returns HHUFF_OK.
 *      2. Export reads scratch and never writes it.  Item k is slot slot[k] as the last call that listed it left
 *         it; the connection there goes on as if nothing happened.  Several items may name one slot.  Exactly
 *         img_len[k] bytes of the region are written, a multiple of 16, pad bytes zero.  Exporting a slot in which
 *         no call ever started a connection is the caller's error: every read stays inside the slab and every
 *         write inside the region, the image is unspecified (import may refuse it).
 *      3. Sizing.  With img == NULL (img_off may then be NULL too) export writes only img_len[k], status[k] = 0.
 *         A region smaller than the image: status[k] = HHUFF_IMG_SPACE, img_len[k] = the length needed, no byte
 *         of the region written.  img_len <= 96 + 32 records + string_bytes + 15, records = the live table
 *         entries plus the inflight or parked records, string_bytes = the live entries' name and value bytes;
 *         hhuff_conn_image_bound(fam) is that expression at the family's maxima (0 when the slab size is 0).  An
 *         image of 2^32 - 16 bytes or more (an inflight list of 2^28 records) cannot be stated: HHUFF_IMG_SPACE
 *         with img_len = 2^32 - 16, sizing query included.
 *      4. Position independence and canonical form.  An image holds no scratch offset, ring index or ring start;
 *         entries come oldest first and their bytes form one run in that order.  Two connections whose future
 *         behaviour is the same have byte-identical images, whatever slots, scratch addresses, call partitioning,
 *         ring and compaction history produced them.  The hashes the encoders keep beside their entries are
 *         carried (they are functions of the strings); the HPACK decoder's cached name class is not (it is
 *         computed again on first use).
 *      5. Import rebuilds the slab of slot slot[k] from item k's image (img_len[k] = its length, as export gave
 *         it).  The family's next call lists the connection in that slot with its *_CONTINUE flag and without
 *         HHUFF_CONN_RESET, and the connection continues exactly as it would have at its source; a QPACK encoder
 *         session keeps its mode (evicting, duplicating), so the mode-mismatch refusal works after a move; its
 *         peer record (2g'') is not in the image: it travels with the caller, as the slot number does.  Slot
 *         ownership is (2h) point 3: the lowest-numbered item that names a slot owns it, the others get
 *         HHUFF_IMG_EINVAL, as does a slot >= nslots (export too).  An item with a non-zero status leaves its slab
 *         untouched.
 *      6. Images are untrusted bytes.  Import checks the header first -- magic, version, length (== img_len[k],
 *         inside the region, a multiple of 16), reserved words: HHUFF_IMG_EFORMAT; another family or other
 *         parameters: HHUFF_IMG_EPARAM -- and then, before the first byte of the slab is written, everything the
 *         family's kernels rely on for memory safety (HHUFF_IMG_EFORMAT): counts within the entry ring, the
 *         inflight list and the parked list; size / used == the entries' bytes + 32 each, <= the capacity, the
 *         capacity <= table_size; the string run as long as the entries' lengths; evicted <= count, lkr <= count,
 *         an inflight record's largest reference <= count; reserved words and pad bytes zero.  An image that lies
 *         about content only (a value the peer's table does not hold) is the caller's own problem.
 *      7. The image: [header 32][state 64][entry records x 32][list records x 16][string run, padded to 16].
 *           header  +0 magic "HHCI"  +4 u16 version = 1  +6 u16 family  +8 u32 table_size  +12 u32 max_inflight
 *                   +16 u32 max_blocked  +20 u32 total length  +24, +28 reserved, 0
 *         The body per family is in DESIGN.md; a layout change bumps the version.
 *      8. Two calls in flight on different streams must not import into, or run a family call on, the same slot:
 *         the caller's contract, as in (2h) point 3.
 *      Out of scope: importing at another table_size, max_inflight or max_blocked (HHUFF_IMG_EPARAM), and a
 *      host-side reader of image bodies. */
#define HHUFF_FAM_HPACK_DEC      0u /* hhuff_hpack_decode_blocks / _parse_requests / _parse_responses scratch */
#define HHUFF_FAM_QPACK_DEC      1u /* hhuff_qpack_decode / _parse_* scratch */
#define HHUFF_FAM_HPACK_ENC      2u /* hhuff_hpack_flatten_responses scratch */
#define HHUFF_FAM_QPACK_ENC      3u /* hhuff_qpack_flatten_sessions scratch */
#define HHUFF_FAM_QPACK_DSESSION 4u /* hhuff_qpack_dsessions_t.state */
typedef struct hhuff_conn_family {
    uint32_t family;       /* HHUFF_FAM_* */
    uint32_t table_size;   /* HPACK_DEC: table_size; QPACK_DEC, QPACK_ENC: header_table_size; else 0 */
    uint32_t max_inflight; /* QPACK_ENC; else 0 */
    uint32_t max_blocked;  /* QPACK_DSESSION; else 0 */
} hhuff_conn_family_t;
#define HHUFF_IMG_SPACE   (-300) /* export: the region is too small; img_len = the length needed, nothing written */
#define HHUFF_IMG_EINVAL  (-303) /* slot >= nslots, or (import) a slot an earlier item of the call names */
#define HHUFF_IMG_EFORMAT (-304) /* import: not an image of this version, or its contents break an invariant */
#define HHUFF_IMG_EPARAM  (-305) /* import: an image of another family or other family parameters */
uint64_t hhuff_conn_slab_size(const hhuff_conn_family_t *fam);   /* the family's bytes per slot; 0: bad parameters */
uint64_t hhuff_conn_image_bound(const hhuff_conn_family_t *fam); /* largest image of one connection, multiple of 16 */
int hhuff_conn_export(const hhuff_conn_family_t *fam, const void *scratch, uint64_t scratch_size, uint32_t nslots,
                      const uint32_t *slot, uint32_t n, uint8_t *img, const uint64_t *img_off, uint32_t *img_len,
                      int32_t *status, void *stream);
int hhuff_conn_import(const hhuff_conn_family_t *fam, void *scratch, uint64_t scratch_size, uint32_t nslots,
                      const uint32_t *slot, uint32_t n, const uint8_t *img, const uint64_t *img_off,
                      const uint32_t *img_len, int32_t *status, void *stream);

/* (2j) Token interning: name -> token id.  Every h2o function restated above hands its caller tokens, not byte
 *      strings: h2o_hpack_decode_header and QPACK's decode_header intern a literal name through h2o_lookup_token
 *      (lib/http2/hpack.c:398-400, lib/http3/qpack.c:585), and the encoders start from h2o_iovec_is_token(name)
 *      and the token's flags (hpack.c:861-862, qpack.c:1219-1224).  A token set is the caller's list of names, each
 *      with one caller-defined 32-bit word; the token id is the index in that list (h2o passes its h2o__tokens[]:
 *      the id is what `h2o__tokens + id` is to h2o).  The library embeds no list.  The comparison is bytewise and
 *      case-sensitive, as h2o_lookup_token's memcmp is.
 *      1. hhuff_tokens_build compiles the list on the host into a table: host memory in, host memory out, no HIP
 *         call (it works on a machine without a GPU).  names = the names back to back, name i =
 *         names[name_off[i] .. name_off[i + 1]); user[i] = token i's word (NULL: all 0).  1 <= ntokens <= 4096, every
 *         name 1..255 bytes of any value.  HHUFF_EINVAL, with `table` untouched, for two equal names, an empty name,
 *         a name over 255 bytes, a decreasing name_off, ntokens out of range, a NULL array, or a table_size below
 *         hhuff_tokens_table_size(ntokens, name_bytes), name_bytes = name_off[ntokens] - name_off[0] (the function
 *         is 0 for ntokens out of range or name_bytes outside [ntokens, 255 ntokens]).  The table is exactly
 *         hhuff_tokens_table_size bytes long -- a multiple of 16; that number is the table_size of the calls below --
 *         and deterministic: equal arguments give equal bytes.
 *      2. The table holds no address.  The caller copies it to 16-byte-aligned device memory and may copy it again
 *         anywhere.  It begins with a header -- magic "HHTK", u16 version = 1, u16 0, u32 ntokens, u32 size -- and is
 *         a hash table with open addressing whose probe bound was found at build time: a lookup is
 *         that bounded number of bucket reads and a full comparison of the name whose 16 tag bits match.
 *      3. hhuff_intern_strings: for i < n, token[i] = the id of the name equal to in[off[i] .. off[i] + len[i]), or
 *         HHUFF_TOK_NONE -- also for length 0, length over 255 and a range that passes in_size.  user_out[i] (may be
 *         NULL) = that token's word, or miss_user.
 *      4. hhuff_intern_fields: the same on the output of the block and section decoders of (2c) .. (2e'''): arena,
 *         name_off, name_len as they wrote them, first = the call's blk_off / sec_off (nblk + 1 entries), nslots =
 *         the host copy of first[nblk].  Block b's fields are the slots first[b] .. first[b] + min(nfields[b],
 *         first[b + 1] - first[b]) - 1; every other slot of token / user_out is left untouched, as the decoders leave
 *         those slots of name_off unwritten.
 *      5. hhuff_intern_headers: the encoder side of (2f) .. (2g'').  For each header h,
 *         hdr[h].flags = (hdr[h].flags & keep_mask) | (hit ? word : 0), and no other byte of hdr[h] is written;
 *         token[h] (may be NULL) as in point 3.  With the words HHUFF_HDR_TOKEN | HHUFF_HDR_LIKELY_TO_REPEAT as each
 *         token's flags say and keep_mask = HHUFF_HDR_DONT_COMPRESS the call supplies what (2f) and (2g') ask the
 *         caller for.  A name out of range is a miss; the encoder reports the range itself.
 *      6. The three device calls are asynchronous on `stream`, one launch each, without pool workspace.  They return
 *         HHUFF_EINVAL and enqueue nothing for a NULL required array, a table_size under the header's 32 bytes or a
 *         table that is not 16-byte aligned; n / nblk / nhdr (or nslots) of 0 returns HHUFF_OK and enqueues nothing.
 *         (The five functions of this section leave hhuff_last_error_string() as it was.)
 *         They read only bytes of in / arena inside the given size, but for the aligned dwords (by address) that
 *         hold a name's bytes, which are read whole.
 *      7. The table in device memory is untrusted bytes, as an image is to hhuff_conn_import.  A header whose magic,
 *         version, reserved words, counts or recorded size disagree with table_size makes every token output of the
 *         call HHUFF_TOK_EFORMAT and leaves user_out and the headers' flags untouched.  Whatever the other bytes
 *         hold, no load leaves [table, table + table_size) and no store leaves the outputs: a damaged table can only
 *         give wrong ids. */
#define HHUFF_TOK_NONE    (-1) /* the bytes are no token's name */
#define HHUFF_TOK_EFORMAT (-2) /* the table is not one hhuff_tokens_build wrote (every output of the call) */
uint64_t hhuff_tokens_table_size(uint32_t ntokens, uint64_t name_bytes); /* 0: bad parameters */
int hhuff_tokens_build(const uint8_t *names, const uint32_t *name_off, uint32_t ntokens, const uint32_t *user,
                       void *table, uint64_t table_size);
int hhuff_intern_strings(const void *table, uint64_t table_size, const uint8_t *in, uint64_t in_size,
                         const uint32_t *off, const uint32_t *len, uint32_t n, int32_t *token, uint32_t *user_out,
                         uint32_t miss_user, void *stream);
int hhuff_intern_fields(const void *table, uint64_t table_size, const uint8_t *arena, uint64_t arena_size,
                        const uint32_t *name_off, const uint32_t *name_len, const uint32_t *first,
                        const uint32_t *nfields, uint32_t nblk, uint32_t nslots, int32_t *token, uint32_t *user_out,
                        uint32_t miss_user, void *stream);
int hhuff_intern_headers(const void *table, uint64_t table_size, const uint8_t *in, uint64_t in_size,
                         hhuff_hpack_header_t *hdr, uint32_t nhdr, uint32_t keep_mask, int32_t *token, void *stream);

/* (2k) HTTP/2 frames on the receive side: each connection's raw frame bytes -> the header blocks the decoders of
 *      (2c) take.  h2o_http2_decode_frame and h2o_http2_decode_headers_payload (lib/http2/frame.c:130-224) and the
 *      HEADERS -> CONTINUATION sequencing of both h2o sides (lib/http2/connection.c:757-803, 1023-1095, 1288-1325;
 *      lib/common/http2client.c:448-491, 607-659, 873-925), for many connections at once.
 *        connection c   in[in_off[c] .. in_off[c+1]): the bytes the previous call did not consume, then the new
 *                       ones (behind the 24-byte preface, which is the caller's); frame slots frm_first[c] ..
 *                       frm_first[c+1] - 1 of `frames` (frm_first[nconn] = frm_cap, host copy)
 *        frames         frames[frm_first[c] + i], i < nframes[c]: the frames walked, in wire order; payload_off and
 *                       frag_off are offsets in `in`; the other slots are not written
 *        blk, blk_off,  the completed header blocks, their fragments copied together, packed back to back in
 *        conn_first     connection order, then wire order: block b = blk[blk_off[b] .. blk_off[b+1]); connection c's
 *                       blocks are conn_first[c] .. conn_first[c+1] - 1.  blk has in_size bytes (de-framed bytes
 *                       never exceed the input), blk_off frm_cap + 1 entries -- those past nblk all hold the total,
 *                       so they read as empty blocks --, conn_first nconn + 1, blocks frm_cap (blocks[b] for
 *                       b < nblk is written).  blk, blk_off, conn_first and nconn are, as they are and on the same
 *                       stream, the in, blk_off, conn_first and nconn of hhuff_hpack_decode_blocks,
 *                       _parse_requests, _parse_responses and their _slots variants (in_size = this call's)
 *        totals         [0] = nblk, [1] = the block bytes
 *        arena_off      NULL, or frm_cap + 1 u64: arena_off[b] = the running sum of arena_fixed + arena_per_byte *
 *                       (block length) over the blocks before b (entries past nblk hold the total), which sizes
 *                       the decoders' arena slices without reading a length back
 *      The call keeps no state.  consumed[c] (relative to in_off[c]) is the end of the last frame after which no
 *      header block is open: a trailing partial frame is not consumed, nor is a HEADERS / PUSH_PROMISE frame whose
 *      END_HEADERS has not arrived, nor its CONTINUATIONs, and such frames are not listed in `frames`.  The caller
 *      keeps in[in_off[c] + consumed[c] ..) and presents it again in front of the next bytes.
 *      Per connection the frames are walked by these rules, in h2o's order.  The first failing rule stops the
 *      walk: cstatus[c] = h2o's return value, cerr[c] = the HHUFF_H2F_ERR_* that names h2o's err_desc; the blocks
 *      and frames completed before stand, and consumed[c] is the end of the last completed unit (a frame that is
 *      no header frame, or a whole header block).
 *      1. Fewer than 9 bytes left: cstatus 0 (h2o: H2O_HTTP2_ERROR_INCOMPLETE, wait for more).
 *      2. length > max_frame_size: -6 (H2O_HTTP2_ERROR_FRAME_SIZE), decided by the header alone.  h2o passes
 *         16384 on both sides.
 *      3. Fewer than 9 + length bytes left: cstatus 0.
 *      4. While a block is open: any type but CONTINUATION is -1 (HHUFF_H2F_ERR_EXPECTED_CONTINUATION).  A
 *         CONTINUATION appends its whole payload; its stream id is not compared with the opener's (h2o looks the
 *         stream up, which is the caller's) and that of the frame with END_HEADERS is the block's end_stream_id.
 *         With max_block_bytes != 0, a CONTINUATION whose length added to the block's size so far exceeds
 *         max_block_bytes stops the walk with HHUFF_H2F_REFUSED.  h2o's server (max_block_bytes =
 *         H2O_MAX_REQLEN = 417792) at that point sends RST_STREAM with REFUSED_STREAM, resets the stream and goes
 *         on expecting CONTINUATION frames, which it drops (connection.c:796-800); that is the caller's to do
 *         with the bytes from consumed[c] on.  h2o's client has no limit: pass 0.
 *      5. No block open, HEADERS: stream id 0 is -1 (_HEADERS_STREAM_ID); PADDED with length 0 or a pad length
 *         above the bytes behind the pad byte is -1 (_HEADERS_FRAME); PRIORITY with fewer than 5 bytes left is -1
 *         (_HEADERS_PRIORITY: h2o sets no err_desc); an even stream id is -1 (_HEADERS_STREAM_ID).  dependency ==
 *         stream_id sets HHUFF_H2B_SELF_DEPENDENCY and is no error here: h2o's server ignores it on trailers and
 *         rejects it elsewhere ("stream cannot depend on itself"), and only the caller knows which streams are
 *         open.  END_HEADERS completes the block, otherwise the frame opens it.
 *      6. No block open, CONTINUATION: -1 (_INVALID_CONTINUATION).
 *      7. No block open, PUSH_PROMISE: -1 (_PUSH_PROMISE, both h2o sides) unless flags has HHUFF_H2F_ACCEPT_PUSH.
 *         With it, RFC 9113 6.6: stream id 0 is -1 (_PROMISE_STREAM_ID); padding as for HEADERS and fewer than 4
 *         bytes for the promised id are -1 (_PROMISE_FRAME); the promised id is those bytes & 0x7fffffff, the rest
 *         is the fragment; the block is flagged HHUFF_H2B_PROMISE; END_HEADERS and CONTINUATION as for HEADERS.
 *      8. Every other type, unknown ones included, gets a frame record and is stepped over unexamined: the payload
 *         rules of those types and every check that needs stream state stay with the caller.
 *      9. A unit that needs more frame slots than the connection has left: HHUFF_H2F_FRAMES.  A unit is checked to
 *         its end by rules 1-8 first, so the stop is at a `consumed` boundary and a block whose frames do not all
 *         fit is not started.
 *      Device arrays.  Returns HHUFF_EINVAL, before any device call, for a NULL array (arena_off may be NULL),
 *      in_size >= 2^32, max_frame_size outside 16384 .. 2^24 - 1 or an unknown flag bit; nconn == 0 returns
 *      HHUFF_OK.  Asynchronous on `stream`, no host synchronisation and no copy to the host; bitwise deterministic.
 *      Stream-ordered pool workspace of 8 bytes per connection (and 8 per 256 of them) and 16 per frame slot
 *      (hhuff_pool_trim).  A connection's range is clamped to in_size and its slots to frm_cap.  Of `in` the call
 *      reads the connections' bytes and, with them, the aligned dwords (by address) that hold a fragment's bytes: up
 *      to 3 bytes in front of a fragment's first byte and up to 3 behind its last, so behind in + in_size too where a
 *      fragment ends there and that address is no multiple of 4 (never across a 4-byte boundary, so never into
 *      another page). */
typedef struct hhuff_h2_frame {      /* 32 bytes: one per frame walked */
    uint32_t payload_off, length;    /* payload at in[payload_off .. + length) */
    uint32_t stream_id;              /* 31 bits */
    uint8_t  type, flags; uint16_t rsv;
    uint32_t frag_off, frag_len;     /* header frames: the block fragment inside the payload
                                        (padding, priority, promised id stripped); else 0, 0 */
    uint32_t block;                  /* header frames: index of the block it belongs to; else ~0u */
    uint32_t rsv2;
} hhuff_h2_frame_t;
typedef struct hhuff_h2_block {      /* 32 bytes: one per completed header block */
    uint32_t stream_id;              /* of the opening HEADERS / PUSH_PROMISE frame */
    uint32_t end_stream_id;          /* of the frame that carried END_HEADERS (h2o hands the block to THAT stream) */
    uint32_t flags;                  /* HHUFF_H2B_* */
    uint32_t dependency; uint32_t weight;   /* 1..256; h2o_http2_default_priority (0, 16) when no PRIORITY flag */
    uint32_t promised_stream_id;     /* HHUFF_H2B_PROMISE only */
    uint32_t first_frame, nframes;   /* its frames in frames[] */
} hhuff_h2_block_t;
#ifdef __cplusplus
static_assert(sizeof(hhuff_h2_frame_t) == 32 && sizeof(hhuff_h2_block_t) == 32, "record sizes");
#else /* (C99 has no static assertion: an array type of negative size does not compile) */
typedef char hhuff_h2_records_are_32_bytes[sizeof(hhuff_h2_frame_t) == 32 && sizeof(hhuff_h2_block_t) == 32 ? 1 : -1];
#endif
#define HHUFF_H2F_ACCEPT_PUSH 1u      /* flags: PUSH_PROMISE opens a block (beyond h2o, which refuses it) */
#define HHUFF_H2F_REFUSED (-310)      /* cstatus: the block outgrew max_block_bytes */
#define HHUFF_H2F_FRAMES (-311)       /* cstatus: out of frame slots */
#define HHUFF_H2F_ERR_NONE 0u                  /* *err_desc untouched */
#define HHUFF_H2F_ERR_HEADERS_STREAM_ID 1u     /* "invalid stream id in HEADERS frame" */
#define HHUFF_H2F_ERR_HEADERS_FRAME 2u         /* "invalid HEADERS frame" */
#define HHUFF_H2F_ERR_HEADERS_PRIORITY 3u      /* priority field cut short (h2o: -1 without err_desc) */
#define HHUFF_H2F_ERR_EXPECTED_CONTINUATION 4u /* "expected CONTINUATION frame" */
#define HHUFF_H2F_ERR_INVALID_CONTINUATION 5u  /* "received invalid CONTINUATION frame" */
#define HHUFF_H2F_ERR_PUSH_PROMISE 6u          /* "received PUSH_PROMISE frame" */
#define HHUFF_H2F_ERR_PROMISE_STREAM_ID 7u     /* ACCEPT_PUSH: PUSH_PROMISE on stream 0 */
#define HHUFF_H2F_ERR_PROMISE_FRAME 8u         /* ACCEPT_PUSH: bad padding or no room for the promised id */
#define HHUFF_H2B_END_STREAM 1u       /* the opening HEADERS frame had END_STREAM */
#define HHUFF_H2B_PRIORITY 2u         /* it had PRIORITY: dependency and weight are the frame's */
#define HHUFF_H2B_EXCLUSIVE 4u
#define HHUFF_H2B_CONTINUED 8u        /* the block has CONTINUATION frames */
#define HHUFF_H2B_PROMISE 16u         /* opened by PUSH_PROMISE */
#define HHUFF_H2B_SELF_DEPENDENCY 32u /* dependency == stream_id */
int hhuff_h2_deframe(const uint8_t *in, uint64_t in_size,            /* in_size < 2^32 */
                     const uint32_t *in_off, uint32_t nconn,         /* connection c: in[in_off[c] .. in_off[c+1]) */
                     const uint32_t *frm_first,                      /* frame capacity: slots frm_first[c] .. frm_first[c+1] */
                     uint32_t frm_cap,                               /* host copy of frm_first[nconn] */
                     uint32_t max_frame_size, uint32_t max_block_bytes, unsigned flags,
                     hhuff_h2_frame_t *frames, uint32_t *nframes, uint32_t *consumed,
                     int32_t *cstatus, uint32_t *cerr,
                     uint8_t *blk, uint32_t *blk_off, uint32_t *conn_first, hhuff_h2_block_t *blocks,
                     uint32_t *totals /* [2]: nblk, block bytes */,
                     uint64_t *arena_off, uint64_t arena_fixed, uint32_t arena_per_byte, void *stream);

/* (2k') HTTP/2 control frames: the payload rules of the frames (2k) steps over, the peer's SETTINGS, the connection
 *      windows and the replies h2o queues, for many connections at once.  h2o_http2_decode_data_payload,
 *      _priority_payload, _rst_stream_payload, _ping_payload, _goaway_payload, _window_update_payload and
 *      h2o_http2_update_peer_settings (lib/http2/frame.c:37-66, 152-177, 226-310), h2o_http2_window_update
 *      (include/h2o/http2_common.h:234-241), the reply layouts of frame.c:68-122, and what handle_settings_frame,
 *      handle_ping_frame, handle_window_update_frame, handle_priority_frame, handle_goaway_frame and handle_data_frame
 *      do without a stream (lib/http2/connection.c:976-989, 1097-1108, 1151-1261; the client's twins,
 *      lib/common/http2client.c:662-871).
 *        in, in_size, frames, nframes, frm_first, frm_cap, nconn   hhuff_h2_deframe's, as they are and on the same stream
 *        flags              HHUFF_H2C_CLIENT: the client's handlers (they differ from the server's in the receive window)
 *        recv_window_size   the server's H2O_HTTP2_SETTINGS_HOST_CONNECTION_WINDOW_SIZE; 0: no receive window kept
 *        peers_in, peers_out   one hhuff_h2_peer_t per connection: the caller's between steps (peers_out may be
 *                           peers_in); a new connection starts from HHUFF_H2_PEER_INIT
 *        ctl                ctl[frm_first[c] + i], i < nframes[c]: frame i's record, at the frame record's index; the
 *                           other slots are not written
 *        rep, rep_off       connection c's replies go to rep[rep_off[c] .. rep_off[c+1]), clamped to rep_size;
 *                           hhuff_h2_control_reply_bound(slots of the connection) always fits
 *      Per connection: nctl[c], the frames handled; cstatus[c] / cerr[c], the first connection-level failure in wire
 *      order (h2o's return value and the HHUFF_H2C_ERR_* that names its err_desc, or HHUFF_H2C_SPACE / _EINVAL);
 *      rep_len[c], the reply bytes written; peers_out[c].
 *      A connection's frames are handled in wire order by these rules, each in h2o's order of tests (NEEDS_STREAM etc.:
 *      the record's HHUFF_H2R_* flags; a failing frame's record has status and err, SETTINGS also a, and zeros else):
 *        DATA (0)           stream id 0: -1 (_DATA_STREAM_ID); PADDED with length 0 or length < 1 + pad: -1
 *                           (_DATA_FRAME); else a = the data's offset in `in`, b = its length (may be 0), NEEDS_STREAM.
 *                           Server with recv_window_size != 0: recv_window -= length (padding included); at
 *                           recv_window <= recv_window_size / 2 a WINDOW_UPDATE on stream 0 carrying recv_window_size -
 *                           recv_window (its low 32 bits) is owed, recv_window = recv_window_size, flag WINDOW_UPDATE
 *                           (connection.c:986-989).  h2o's client consumes its connection window only behind the
 *                           stream lookups (http2client.c:516-519, 585, 599): with HHUFF_H2C_CLIENT recv_window is left
 *                           alone and that window is the caller's.
 *        PRIORITY (2)       stream id 0: -1 (_PRIORITY_STREAM_ID); length != 5: -6 (_PRIORITY_FRAME); dependency ==
 *                           stream id: -1 (_SELF_DEPENDENCY, both h2o sides); else a = exclusive << 31 | dependency,
 *                           b = weight 1..256, NEEDS_STREAM
 *        RST_STREAM (3)     stream id 0: -1 (_RST_STREAM_STREAM_ID); length != 4: -6 (_RST_STREAM_FRAME); else a =
 *                           the error code, NEEDS_STREAM (the idle-id test is the caller's)
 *        SETTINGS (4)       stream id != 0: -1 (_SETTINGS_STREAM_ID); ACK with length != 0: -6 (_SETTINGS_ACK); ACK
 *                           with length 0: flag ACK.  Without ACK, h2o_http2_update_peer_settings pair by pair:
 *                           ENABLE_PUSH above 1 and MAX_FRAME_SIZE outside 16384 .. 16777215 are -1,
 *                           INITIAL_WINDOW_SIZE above 0x7fffffff is -3 (_SETTINGS_FRAME each); unknown identifiers
 *                           are skipped, the last of a repeated one wins; a length that is no multiple of 6 applies
 *                           every whole pair and is then -6 (_SETTINGS_SIZE: h2o sets no err_desc).  An error leaves
 *                           the earlier pairs of the frame applied, as h2o does.  a = the whole pairs read without
 *                           error; on success b = the int32 change of initial_window_size this frame made (flag
 *                           WINDOW_DELTA when b != 0: the caller adds it to every stream's send window), a SETTINGS
 *                           ACK (9 bytes) is owed and peers_out[c].flags gets HHUFF_H2P_SETTINGS
 *        PING (6)           stream id != 0: -1; length != 8: -6 (both _PING_FRAME, h2o's one text); else a, b = the
 *                           opaque bytes 0-3 and 4-7, big-endian, flag ACK copied from the frame; without ACK a PING
 *                           with ACK and the same 8 bytes (17 bytes) is owed
 *        GOAWAY (7)         stream id != 0: -1 (_GOAWAY_STREAM_ID); length < 8: -6 (_GOAWAY_FRAME); else a =
 *                           last_stream_id & 0x7fffffff, b = the error code, peers_out[c].flags gets HHUFF_H2P_GOAWAY;
 *                           the debug data stays where the frame record says (payload_off + 8)
 *        WINDOW_UPDATE (8)  length != 4: -6; increment (& 0x7fffffff) 0 on stream 0: -1 (both _WINDOW_UPDATE_FRAME,
 *                           connection level).  Increment 0 on a stream is h2o's stream-level error: the record has
 *                           status -1, _WINDOW_UPDATE_FRAME and STREAM_ERROR | NEEDS_STREAM (the caller resets the
 *                           stream), a RST_STREAM(PROTOCOL_ERROR) on that stream (13 bytes) is owed, the connection's
 *                           own status stays 0 and the walk goes on.  Increment > 0 on stream 0: send_window +
 *                           increment > INT32_MAX is -3 (_FLOW_CONTROL), else send_window += increment; a = the
 *                           increment.  Increment > 0 on a stream: a = the increment, NEEDS_STREAM.
 *        HEADERS, PUSH_PROMISE, CONTINUATION, any type >= 10   the record is zeroed (expect_default,
 *                           connection.c:1320-1326, ignores unknown types; header frames are (2k)'s)
 *      The walk of a connection stops at its first connection-level failure: nctl[c] counts the frames in front of
 *      it, the failing frame's record (slot nctl[c]) is the last one written -- not written for HHUFF_H2C_SPACE and
 *      HHUFF_H2C_EINVAL --, and peers_out[c] is what h2o's conn->peer_settings and windows hold at the moment its
 *      handler returns the error, the partially applied SETTINGS frame included.  Without failure nctl[c] =
 *      nframes[c].  A control failure precedes any failure the de-framer reported for the connection, since every
 *      listed frame lies in front of the point where the de-framer stopped; header blocks with first_frame >=
 *      frm_first[c] + nctl[c] belong to a connection h2o would already have closed.
 *      Replies are written in wire order, for the frames in front of the failure, exactly as h2o queues them on
 *      conn->_write.buf; a record's reply_len is what its frame added.  A region that cannot take a frame's reply
 *      stops the connection in front of that frame with HHUFF_H2C_SPACE, nothing of the frame applied.
 *      Checks that need stream state stay with the caller, as in (2k): idle and closed stream ids, stream windows,
 *      max_streams_for_priority, all handle_data_frame does behind the connection window.  NEEDS_STREAM marks the
 *      records the caller has to look at.
 *      Device arrays.  Returns HHUFF_EINVAL, before any device call, for a NULL array, in_size >= 2^32, an unknown
 *      flag bit or recv_window_size > INT32_MAX; nconn == 0 returns HHUFF_OK.  Asynchronous on `stream`, no host
 *      synchronisation, no workspace, no atomics; bitwise deterministic.  frames[] and nframes[] are not trusted:
 *      nframes[c] is clamped to the connection's slots and the slots to frm_cap; a record whose payload leaves
 *      in[0 .. in_size) stops its connection with HHUFF_H2C_EINVAL.  Of `in` the call reads payload bytes only. */
typedef struct hhuff_h2_peer {       /* 40 bytes, 8-byte aligned */
    uint32_t header_table_size, enable_push, max_concurrent_streams, initial_window_size, max_frame_size;
                                     /* conn->peer_settings */
    uint32_t flags;                  /* HHUFF_H2P_* */
    int64_t  send_window;            /* conn->_write.window; the caller subtracts the DATA it sends */
    int64_t  recv_window;            /* conn->_input_window (server, recv_window_size != 0), else untouched */
} hhuff_h2_peer_t;
/* a new connection: H2O_HTTP2_SETTINGS_DEFAULT, both windows 65535 */
#define HHUFF_H2_PEER_INIT { 4096u, 1u, 0xFFFFFFFFu, 65535u, 16384u, 0u, 65535, 65535 }
typedef struct hhuff_h2_ctl {        /* 16 bytes: one per frame record */
    uint32_t a, b;
    int32_t  status;                 /* h2o's return value for this frame */
    uint16_t err;                    /* HHUFF_H2C_ERR_* */
    uint8_t  flags;                  /* HHUFF_H2R_* */
    uint8_t  reply_len;              /* reply bytes this frame added */
} hhuff_h2_ctl_t;
#ifdef __cplusplus
static_assert(sizeof(hhuff_h2_peer_t) == 40 && sizeof(hhuff_h2_ctl_t) == 16, "record sizes");
#else
typedef char hhuff_h2_control_record_sizes[sizeof(hhuff_h2_peer_t) == 40 && sizeof(hhuff_h2_ctl_t) == 16 ? 1 : -1];
#endif
#define HHUFF_H2C_CLIENT 1u           /* flags: the client's handlers */
#define HHUFF_H2C_SPACE (-312)        /* cstatus: the reply region cannot take the next frame's reply */
#define HHUFF_H2C_EINVAL (-313)       /* cstatus: a frame record's payload leaves in[0 .. in_size) */
#define HHUFF_H2P_SETTINGS 1u         /* peer flags: a SETTINGS without ACK has been applied */
#define HHUFF_H2P_GOAWAY 2u           /* a GOAWAY has arrived */
#define HHUFF_H2R_ACK 1u              /* record flags: SETTINGS / PING with ACK */
#define HHUFF_H2R_NEEDS_STREAM 2u     /* the caller's stream-state checks and actions remain */
#define HHUFF_H2R_STREAM_ERROR 4u     /* status is a stream-level error: RST_STREAM written, the walk went on */
#define HHUFF_H2R_WINDOW_DELTA 8u     /* SETTINGS: b is to be added to every stream's send window */
#define HHUFF_H2R_WINDOW_UPDATE 16u   /* DATA: a connection-level WINDOW_UPDATE was written */
#define HHUFF_H2C_ERR_NONE 0u
#define HHUFF_H2C_ERR_DATA_STREAM_ID 1u        /* "invalid stream id in DATA frame" */
#define HHUFF_H2C_ERR_DATA_FRAME 2u            /* "invalid DATA frame" */
#define HHUFF_H2C_ERR_PRIORITY_STREAM_ID 3u    /* "invalid stream id in PRIORITY frame" */
#define HHUFF_H2C_ERR_PRIORITY_FRAME 4u        /* "invalid PRIORITY frame" */
#define HHUFF_H2C_ERR_SELF_DEPENDENCY 5u       /* "stream cannot depend on itself" */
#define HHUFF_H2C_ERR_RST_STREAM_STREAM_ID 6u  /* "invalid stream id in RST_STREAM frame" */
#define HHUFF_H2C_ERR_RST_STREAM_FRAME 7u      /* "invalid RST_STREAM frame" */
#define HHUFF_H2C_ERR_SETTINGS_STREAM_ID 8u    /* "invalid stream id in SETTINGS frame" */
#define HHUFF_H2C_ERR_SETTINGS_ACK 9u          /* "invalid SETTINGS frame (+ACK)" */
#define HHUFF_H2C_ERR_SETTINGS_FRAME 10u       /* "invalid SETTINGS frame" */
#define HHUFF_H2C_ERR_SETTINGS_SIZE 11u        /* a length that is no multiple of 6 (h2o: -6 without err_desc) */
#define HHUFF_H2C_ERR_PING_FRAME 12u           /* "invalid PING frame" */
#define HHUFF_H2C_ERR_GOAWAY_STREAM_ID 13u     /* "invalid stream id in GOAWAY frame" */
#define HHUFF_H2C_ERR_GOAWAY_FRAME 14u         /* "invalid GOAWAY frame" */
#define HHUFF_H2C_ERR_WINDOW_UPDATE_FRAME 15u  /* "invalid WINDOW_UPDATE frame" */
#define HHUFF_H2C_ERR_FLOW_CONTROL 16u         /* "flow control window overflow" */
static inline uint64_t hhuff_h2_control_reply_bound(uint64_t slots) { return 17u * slots; }
int hhuff_h2_control(const uint8_t *in, uint64_t in_size,            /* in_size < 2^32 */
                     const hhuff_h2_frame_t *frames, const uint32_t *nframes,
                     const uint32_t *frm_first, uint32_t frm_cap, uint32_t nconn,
                     unsigned flags, uint32_t recv_window_size,
                     const hhuff_h2_peer_t *peers_in, hhuff_h2_peer_t *peers_out,
                     hhuff_h2_ctl_t *ctl, uint32_t *nctl, int32_t *cstatus, uint32_t *cerr,
                     uint8_t *rep, uint64_t rep_size, const uint32_t *rep_off /* [nconn + 1] */, uint32_t *rep_len,
                     void *stream);
/* The peers' settings into the HPACK encoder's response records: res[r].header_table_size =
 * peers[c].header_table_size and res[r].max_frame_size = peers[c].max_frame_size for every response r of connection c
 * (conn_first[c] .. conn_first[c+1] - 1, clamped to nres), one lane per response; no other byte of a record is
 * written.  With it a step's SETTINGS reach hhuff_hpack_flatten_responses and its _slots form without the host.
 * Device arrays; HHUFF_EINVAL for a NULL array, nconn == 0 or nres == 0 returns HHUFF_OK; asynchronous on `stream`. */
int hhuff_hpack_responses_set_peers(const hhuff_h2_peer_t *peers, hhuff_hpack_response_t *res,
                                    const uint32_t *conn_first, uint32_t nconn, uint32_t nres, void *stream);

/* (2k'') HTTP/2 DATA frames on the send side: response bodies that lie in device memory -> the DATA frames h2o would
 *      queue on conn->_write.buf, cut by the peer's max_frame_size, the connection's and the streams' send windows
 *      and the room in the buffer, for many connections at once.  h2o_http2_stream_send_pending_data, send_data,
 *      calc_max_payload_size and commit_data_header (lib/http2/stream.c:107-184, 410-436),
 *      h2o_http2_conn_get_buffer_window (include/h2o/http2_internal.h:298-319) without the socket's latency
 *      optimisation, h2o_http2_encode_frame_header (lib/http2/frame.c:68-77).
 *        body, body_size    the body bytes of all records
 *        sends, send_first, nsend   connection c's records are sends[send_first[c] .. send_first[c+1]), clamped to
 *                           nsend (the records `sends` and `sent` hold) as (2k') clamps frm_first; one record is one
 *                           visit of a stream by the caller's scheduler, the records are served in the order listed
 *        peers_in, peers_out   (2k')'s records (peers_out may be peers_in): max_frame_size and send_window are read,
 *                           peers_out[c] is peers_in[c] with send_window reduced by the payload bytes sent
 *        out, out_off       connection c writes out[out_off[c] .. out_off[c+1]), clamped to out_size as (2k') clamps
 *                           rep_off: the region stands for conn->_write.buf, its size for capacity - size
 *      One visit (W_c = send_window, W_s = the record's window, R = the room left in the region, L = the bytes left of
 *      the record, m = max_frame_size) is one call of h2o_http2_stream_send_pending_data:
 *        W_s <= 0: stop (_STREAM_WINDOW);  R <= 9: stop (_ROOM);  W_c <= 0: stop (_CONN_WINDOW);
 *        n = min(m, R - 9, W_c, W_s, L);  with L == 0 and the record not FINAL, or with TRAILERS, nothing is written;
 *        else the 9-byte header (length n, type 0, flags END_STREAM iff FINAL without TRAILERS and the frame takes the
 *        record's last byte, the stream id) and the n bytes;  W_c, W_s, L -= n, R -= n + 9;  L == 0: stop (_DONE).
 *      Visits repeat until one stops, or max_frames of them have been made (_MAX_FRAMES).  An empty FINAL body gets
 *      its END_STREAM frame of length 0 only while both windows are above 0 and R > 9, as in h2o.  The windows and the
 *      room carry over from a connection's record to its next.  The walk is not frame by frame: every frame of a
 *      record is full except the last, so a record's frames follow from a closed form (h2o_amd/csrc/hhuff_h2data.h).
 *      Per record sent[]: the body bytes consumed, the frames written, where its first frame header lies in `out`,
 *      END_STREAM and the reason it stopped, its window afterwards.  Per connection out_len[c], peers_out[c] and
 *      cstatus[c]: 0, or HHUFF_H2D_EINVAL for a record whose body range leaves body[0 .. body_size), whose stream_id
 *      is 0 or above 2^31 - 1 or that has unknown flag bits, and for a peer whose max_frame_size is outside
 *      16384 .. 16777215: the connection stops in front of that record, the earlier records stay written, sent[] of
 *      that record and the later ones is not written.  Bytes of a region behind out_len[c] are not written.
 *      Device arrays.  Returns HHUFF_EINVAL, before any device call, for a NULL array, body_size or out_size >= 2^32
 *      or non-zero flags; nconn == 0 returns HHUFF_OK.  Asynchronous on `stream`, no host synchronisation, workspace
 *      from the library's pool, no atomics; bitwise deterministic.  Nothing in sends, send_first, out_off or peers_in
 *      makes the call touch memory outside body, the connection's clamped region or the arrays' declared sizes. */
typedef struct hhuff_h2_send {       /* 24 bytes: one visit of a stream by the caller's scheduler */
    uint32_t body_off, body_len;     /* body[body_off .. body_off + body_len): the stream's pending bytes (stream->_data) */
    uint32_t stream_id;              /* 1 .. 2^31 - 1 */
    int32_t  window;                 /* stream->output_window on entry (may be <= 0) */
    uint32_t flags;                  /* HHUFF_H2S_* */
    uint32_t max_frames;             /* 0: until something runs out;  k: at most k calls of send_pending_data */
} hhuff_h2_send_t;
typedef struct hhuff_h2_sent {       /* 24 bytes, one per send record */
    uint32_t sent, nframes;          /* body bytes consumed, DATA frames written */
    uint32_t out_off;                /* offset in `out` of the record's first frame header (where it would be, if none) */
    uint32_t flags;                  /* HHUFF_H2T_END_STREAM | why it stopped: one of the other HHUFF_H2T_* */
    int32_t  window;                 /* the stream's window afterwards */
    uint32_t rsv;                    /* 0 */
} hhuff_h2_sent_t;
#ifdef __cplusplus
static_assert(sizeof(hhuff_h2_send_t) == 24 && sizeof(hhuff_h2_sent_t) == 24, "record sizes");
#else
typedef char hhuff_h2_frame_data_record_sizes[sizeof(hhuff_h2_send_t) == 24 && sizeof(hhuff_h2_sent_t) == 24 ? 1 : -1];
#endif
#define HHUFF_H2S_FINAL 1u            /* send flags: send_state FINAL (the record holds the body's last bytes) */
#define HHUFF_H2S_TRAILERS 2u         /* trailers or server-timing follow: no END_STREAM on DATA (commit_data_header) */
#define HHUFF_H2T_END_STREAM 1u       /* sent flags: the record's last frame carries END_STREAM */
#define HHUFF_H2T_DONE 2u             /* stopped: every byte of the record is sent */
#define HHUFF_H2T_STREAM_WINDOW 4u    /* stopped: the stream's window is <= 0 */
#define HHUFF_H2T_ROOM 8u             /* stopped: the region has no room for a header and a byte */
#define HHUFF_H2T_CONN_WINDOW 16u     /* stopped: the connection's send window is <= 0 */
#define HHUFF_H2T_MAX_FRAMES 32u      /* stopped: max_frames visits made */
#define HHUFF_H2D_EINVAL (-314)       /* cstatus: a send record or the peer record is out of range */
int hhuff_h2_frame_data(const uint8_t *body, uint64_t body_size,     /* body_size < 2^32 */
                        const hhuff_h2_send_t *sends, const uint32_t *send_first /* [nconn + 1] */, uint32_t nsend,
                        uint32_t nconn, unsigned flags,                     /* none yet: non-zero is HHUFF_EINVAL */
                        const hhuff_h2_peer_t *peers_in, hhuff_h2_peer_t *peers_out,
                        hhuff_h2_sent_t *sent,
                        uint8_t *out, uint64_t out_size /* < 2^32 */, const uint32_t *out_off /* [nconn + 1] */,
                        uint32_t *out_len, int32_t *cstatus, void *stream);

/* (2k''') HTTP/2 stream table: h2o's conn->streams kept on the device, one slab per connection, and the server-side
 *      stream rules applied to the outputs of (2k), (2k') and (2c') -- handle_headers_frame, handle_incoming_request,
 *      handle_trailing_headers, expect_continuation_of_headers, handle_data_frame behind the connection window,
 *      handle_request_body_chunk, update_stream_input_window, handle_priority_frame, handle_rst_stream_frame,
 *      handle_window_update_frame, the stream halves of handle_settings_frame and handle_goaway_frame
 *      (lib/http2/connection.c:49-52, 451-460, 470-481, 518-607, 618-820, 976-1138, 1151-1286), h2o_http2_stream_open /
 *      _close / _reset (lib/http2/stream.c:36-105), h2o_http2_stream_prepare_for_request
 *      (include/h2o/http2_internal.h:428-445) and h2o_http2_window_update (include/h2o/http2_common.h:234-251).  With it
 *      a server step needs no host code between the socket's bytes and a request's verdict.
 *        slots              (2h), or NULL: connection c uses slab c.  A refused connection (point 3 there) touches no
 *                           slab: sstatus HHUFF_H2ST_ESLOT, nstr = rep_len = 0, no event written
 *        params             the server's configuration (host memory, read before the call returns)
 *        in .. frm_cap      hhuff_h2_deframe's arrays; ctl, nctl, ctl_rep, ctl_rep_off: hhuff_h2_control's records, counts,
 *                           reply bytes and region offsets (its rep and rep_off); blocks, conn_first: the de-framer's;
 *                           bstatus, req, arena, value_off, value_len: hhuff_hpack_parse_requests' for those blocks and
 *                           blk_off (the call reads the :method and :path values only); blocks, bstatus and req hold
 *                           frm_cap records, blk_off frm_cap + 1, value_off and value_len in_size; peers: the control
 *                           call's peers_out.  All as they are and on the same stream.
 *        ops, op_first      connection c's ops are ops[op_first[c] .. op_first[c+1]), clamped to nops: what the
 *                           application did to its streams since the last step, applied in order in front of its frames
 *        sev, op_sev        one event per frame slot, at the frame record's index, and one per op; slots that are not
 *                           walked are not written
 *        rep, rep_off       connection c's bytes to send go to rep[rep_off[c] .. rep_off[c+1]), clamped to rep_size;
 *                           hhuff_h2_streams_reply_bound(its frame slots, its ops) always fits
 *      Per connection: nstr[c], the frames handled; sstatus[c] / serr[c], the first connection-level failure (h2o's return
 *      value and the HHUFF_H2ST_ERR_* that names its err_desc, or HHUFF_H2ST_SPACE / _EINVAL / _EFULL / _ESLOT); rep_len[c].
 *      Frames at and beyond frm_first[c] + nctl[c] are not walked, the frame the control call failed on included: its
 *      failure precedes anything here.  The walk stops at the first connection-level failure; that frame's event (slot
 *      nstr[c]) is the last one written -- not written for _SPACE, _EINVAL and _EFULL.  The caller drops a connection
 *      that failed, as h2o does; its slab is left as h2o leaves its own connection.
 *      rep is the merged stream: first the ops' own bytes, then for every handled frame the bytes the control call
 *      wrote for it (ctl[i].reply_len of ctl_rep), then this call's own, which is the order h2o queues them on
 *      conn->_write.buf.  A frame this call fails on still contributes its control reply.  After this call the caller
 *      sends rep, not ctl_rep.  A region too small for a frame's (an op's) bytes stops the connection in front of it with
 *      HHUFF_H2ST_SPACE, nothing of it applied.
 *      The ops (an op's failure is its own: op_sev[k].status, the walk goes on):
 *        HHUFF_H2O_CLOSE      the response is out (h2o_http2_stream_close): the entry leaves, nothing is written
 *        HHUFF_H2O_CREDIT     update_stream_input_window(arg), as write_streaming_body / proceed_request do: the event
 *                             has WINDOW_UPDATE_SENT when a WINDOW_UPDATE was owed; arg <= INT32_MAX
 *        HHUFF_H2O_OPEN_PUSH  a promised stream (even id): raises push_stream_ids.max_open; the entry has the send window
 *                             peers[c].initial_window_size and no request body and is not counted in pull.open; refused
 *                             once a GOAWAY has come
 *        _EINVAL: an unknown op, stream id 0 or above 2^31 - 1, rsv != 0, a CREDIT above INT32_MAX, an OPEN_PUSH of an odd
 *        or a present id or after GOAWAY; _ENOENT: CLOSE / CREDIT of a stream that is not there; _EFULL: no room
 *      The frames, each in h2o's order of tests (E_x: HHUFF_H2ST_ERR_x; "RST(x)": a RST_STREAM with that code is
 *      written, the event is RESET_SENT with status x and the entry, if any, leaves; the walk goes on):
 *        HEADERS opening a block   (blocks[].first_frame) even id: -1 E_HEADERS_STREAM_ID.  id <= pull max_open: no
 *                           entry -5 E_HEADERS_CLOSED; body not OPEN* -1 E_HEADERS_STREAM_ID; a tunnel -1
 *                           E_TUNNEL_TRAILERS; no END_STREAM -1 E_TRAILERS_END_STREAM; else the block is a trailers block.
 *                           id > pull max_open: HHUFF_H2B_SELF_DEPENDENCY -1 E_SELF_DEPENDENCY; else a priority-only
 *                           entry is reused or one is opened, then h2o_http2_stream_prepare_for_request: max_open = id,
 *                           the stream moves from priority.open to pull.open, output_window = initial_window_size
 *        CONTINUATION       a stream id other than the block's: -1 E_CONTINUATION_STREAM_ID
 *        block end, a head  (the event sits on the frame that ended the block) bstatus other than 0 and -254 is the
 *                           connection's failure (E_HEADER_BLOCK; req[b].err names the text).  Then the pseudo-header
 *                           maps of connection.c:642-677 (CONNECT with and without :protocol, CONNECT-UDP with path "/"
 *                           and no :protocol, the normal case): a mismatch is RST(-1).  Then pull.open > max_streams:
 *                           RST(-7).  Else OPENED, a = the block's index, content_length recorded.  A -254 block:
 *                           OPENED | INVALID_HEADER_CHAR (h2o's 400, the caller's).  A CONNECT with a content-length or
 *                           with END_STREAM: OPENED | BAD_CONNECT (h2o's 400).  An accepted CONNECT is a tunnel with body
 *                           state OPEN, and update_stream_input_window(active_stream_window_size - 65535) runs at once
 *                           (process_request, connection.c:180-182).  Else END_STREAM on the block: REQUEST_COMPLETE;
 *                           without it the body state is OPEN_BEFORE_FIRST_FRAME.  expect: (417, 100) stays with the
 *                           caller; the request record names the field.
 *        block end, trailers   h2o parses with NULL pseudo-header pointers: req[b].exists_map != 0 is -1
 *                           E_TRAILERS_PSEUDO_HEADER, a host field (req[b].authority set without the map's bit) -1
 *                           E_TRAILERS_HOST, then any bstatus != 0 (the soft -254 too) is the connection's failure,
 *                           E_HEADER_BLOCK.  Else TRAILERS and handle_request_body_chunk(empty, END_STREAM)
 *        DATA               no entry: id <= pull max_open RST(-5), above -1 E_DATA_FRAME.  Body not OPEN*: RST(-5).
 *                           Else input_window -= frame length, update_stream_input_window(padding); with data or
 *                           END_STREAM handle_request_body_chunk: received > max_request_entity_size RST(-7); with a
 *                           content-length, received above it, or different at END_STREAM, RST(-1); BODY, a = the
 *                           bytes to deliver (ctl[i].a is where they lie); END_STREAM: REQUEST_COMPLETE; the first
 *                           frame without END_STREAM: with STREAM_BODIES the request is handed over (the caller
 *                           credits the window with ops), without it update_stream_input_window(active_stream_window_size
 *                           - 65535).  update_stream_input_window(d): bytes_unnotified += d; once bytes_unnotified >=
 *                           the window (compared as unsigned numbers, as h2o does: an overdrawn window owes nothing) a
 *                           WINDOW_UPDATE carrying it is written, the window rises by it: WINDOW_UPDATE_SENT
 *        PRIORITY           entry: PRIORITY (the tree is the caller's; ctl[i] has the payload).  No entry: even id or
 *                           id <= pull max_open IGNORED; priority.open >= max_streams_for_priority -11
 *                           E_TOO_MANY_IDLE; else an IDLE entry: PRIORITY_ONLY_OPENED
 *        RST_STREAM         an idle id (by parity, against the matching max_open): -1 E_RST_STREAM_STREAM_ID; else
 *                           RESET_BY_PEER and the entry leaves, or IGNORED
 *        WINDOW_UPDATE      on a stream.  The control record's STREAM_ERROR: RESET_SENT, status -1, the entry leaves if
 *                           there is one (the RST_STREAM is among the control replies).  Idle id: -1
 *                           E_WINDOW_UPDATE_STREAM_ID.  No entry: IGNORED.  output_window + increment > INT32_MAX:
 *                           RST(-3).  Else the window rises; SEND_WINDOW_OPENED when it went from <= 0 to > 0
 *        SETTINGS           with WINDOW_DELTA: ctl[i].b is added to every entry's output_window; an entry whose sum would
 *                           pass INT32_MAX keeps its window (h2o drops the return value, connection.c:1181); a = the
 *                           streams whose window opened, SEND_WINDOW_OPENED if any
 *        GOAWAY             push max_open = 0x7ffffffe
 *        anything else      the event is zeroed
 *      State.  scratch = device memory of hhuff_h2_streams_scratch_size(nslots or nconn, params->max_entries) bytes,
 *      16-byte aligned, kept by the caller between calls.  Without HHUFF_H2ST_CONTINUE, or with HHUFF_CONN_RESET in
 *      slots->flags[c], a connection starts empty.  With max_entries >= hhuff_h2_streams_entries(...) a pull stream or a
 *      priority-only stream always finds room (h2o bounds them at max_streams + 1 and max_streams_for_priority); below
 *      that an insert without room stops the connection with HHUFF_H2ST_EFULL.
 *      hhuff_h2_streams_fill_sends writes sends[r].window from the stream's output_window for (2k'')'s records
 *      (send_first and nsend as there); miss[r] = 1 for no such stream, 2 for a stream already listed earlier in the
 *      connection's range, both with window 0, so that hhuff_h2_frame_data stops them with _STREAM_WINDOW.
 *      hhuff_h2_streams_commit_sent subtracts sent[r].sent from the window of every stream the fill listed.  Both handle
 *      a connection's records in order, one lane a connection.
 *      Device arrays.  Returns HHUFF_EINVAL, before any device call, for a NULL array (ops may be NULL with nops == 0),
 *      in_size, arena_size, ctl_rep_size or rep_size >= 2^32, an unknown flag bit, max_entries == 0 or above 2^24,
 *      active_stream_window_size outside 65535 .. INT32_MAX, a scratch too small or misaligned, and (2h) point 4;
 *      nconn == 0 returns HHUFF_OK.  Asynchronous on `stream`, no host synchronisation, no atomics; bitwise
 *      deterministic.  Every input record is untrusted: counts and ranges are clamped as (2k') clamps them; a payload,
 *      block, field or method range that leaves its array, a frame whose block record does not name it and a control
 *      reply that leaves the connection's region stop the connection with HHUFF_H2ST_EINVAL; nothing makes the call
 *      touch memory outside the arrays' declared sizes or the connection's slab. */
typedef struct hhuff_h2_streams_params { /* 32 bytes; globalconf->http2.* and globalconf->max_request_entity_size */
    uint32_t max_streams, max_streams_for_priority;
    uint32_t active_stream_window_size;  /* 65535 .. INT32_MAX */
    uint32_t max_entries;                /* entries of a connection's table: hhuff_h2_streams_entries() */
    uint64_t max_request_entity_size;
    uint32_t flags;                      /* HHUFF_H2SP_* */
    uint32_t rsv;                        /* 0 */
} hhuff_h2_streams_params_t;
typedef struct hhuff_h2_stream_op {  /* 16 bytes */
    uint32_t stream_id, op /* HHUFF_H2O_* */, arg, rsv /* 0 */;
} hhuff_h2_stream_op_t;
typedef struct hhuff_h2_sev {        /* 16 bytes: one per frame record and one per op */
    uint32_t stream_id;              /* the stream the frame or op is about; 0: none */
    uint32_t a;
    int16_t  status;                 /* h2o's error: of the RST_STREAM, or of the connection's failure; an op's status */
    uint16_t err;                    /* HHUFF_H2ST_ERR_* */
    uint32_t flags;                  /* HHUFF_H2SE_* */
} hhuff_h2_sev_t;
#ifdef __cplusplus
static_assert(sizeof(hhuff_h2_streams_params_t) == 32 && sizeof(hhuff_h2_stream_op_t) == 16 && sizeof(hhuff_h2_sev_t) == 16,
              "record sizes");
#else
typedef char hhuff_h2_streams_record_sizes[sizeof(hhuff_h2_streams_params_t) == 32 && sizeof(hhuff_h2_stream_op_t) == 16 &&
                                           sizeof(hhuff_h2_sev_t) == 16 ? 1 : -1];
#endif
#define HHUFF_H2ST_CONTINUE 1u        /* flags: the tables the previous call left in scratch carry over */
#define HHUFF_H2SP_STREAM_BODIES 1u   /* params flags: h2o_req_can_stream_request is true for every request */
#define HHUFF_H2O_CLOSE 1u
#define HHUFF_H2O_CREDIT 2u
#define HHUFF_H2O_OPEN_PUSH 3u
#define HHUFF_H2ST_SPACE (-315)       /* sstatus: the reply region cannot take the next frame's (op's) bytes */
#define HHUFF_H2ST_EINVAL (-316)      /* sstatus: an input record is out of range; op status: a malformed op */
#define HHUFF_H2ST_EFULL (-317)       /* sstatus / op status: the table has no room for the stream */
#define HHUFF_H2ST_ENOENT (-318)      /* op status: no such stream */
#define HHUFF_H2ST_ESLOT (-319)       /* sstatus: the connection was refused ((2h) point 3) */
#define HHUFF_H2SE_OPENED 1u                /* event flags: a request's HEADERS passed; a = the block index */
#define HHUFF_H2SE_BODY 2u                  /* a = the bytes of the DATA record to deliver */
#define HHUFF_H2SE_REQUEST_COMPLETE 4u      /* END_STREAM has arrived: h2o would execute_or_enqueue_request */
#define HHUFF_H2SE_TRAILERS 8u
#define HHUFF_H2SE_RESET_BY_PEER 16u
#define HHUFF_H2SE_RESET_SENT 32u           /* status = the RST_STREAM's h2o error; the entry is gone */
#define HHUFF_H2SE_WINDOW_UPDATE_SENT 64u
#define HHUFF_H2SE_IGNORED 128u
#define HHUFF_H2SE_PRIORITY_ONLY_OPENED 256u
#define HHUFF_H2SE_SEND_WINDOW_OPENED 512u  /* the send window went from <= 0 to > 0: h2o_http2_scheduler_activate's cue */
#define HHUFF_H2SE_BAD_CONNECT 1024u        /* with OPENED: "Invalid CONNECT request", h2o's 400 */
#define HHUFF_H2SE_INVALID_HEADER_CHAR 2048u /* with OPENED: the block's -254, h2o's 400 */
#define HHUFF_H2SE_PRIORITY 4096u           /* PRIORITY on a stream that is there */
#define HHUFF_H2ST_ERR_NONE 0u
#define HHUFF_H2ST_ERR_HEADERS_STREAM_ID 1u       /* "invalid stream id in HEADERS frame" */
#define HHUFF_H2ST_ERR_HEADERS_CLOSED 2u          /* "closed stream id in HEADERS frame" */
#define HHUFF_H2ST_ERR_TUNNEL_TRAILERS 3u         /* "trailer cannot be used in a CONNECT request" */
#define HHUFF_H2ST_ERR_TRAILERS_END_STREAM 4u     /* "trailing HEADERS frame MUST have END_STREAM flag set" */
#define HHUFF_H2ST_ERR_SELF_DEPENDENCY 5u         /* "stream cannot depend on itself" */
#define HHUFF_H2ST_ERR_CONTINUATION_STREAM_ID 6u  /* "unexpected stream id in CONTINUATION frame" */
#define HHUFF_H2ST_ERR_DATA_FRAME 7u              /* "invalid DATA frame" */
#define HHUFF_H2ST_ERR_TOO_MANY_IDLE 8u           /* "too many streams in idle/closed state" */
#define HHUFF_H2ST_ERR_RST_STREAM_STREAM_ID 9u    /* "unexpected stream id in RST_STREAM frame" */
#define HHUFF_H2ST_ERR_WINDOW_UPDATE_STREAM_ID 10u /* "invalid stream id in WINDOW_UPDATE frame" */
#define HHUFF_H2ST_ERR_TRAILERS_PSEUDO_HEADER 11u /* "invalid pseudo header" */
#define HHUFF_H2ST_ERR_TRAILERS_HOST 12u          /* "found an unexpected connection-specific header" */
#define HHUFF_H2ST_ERR_HEADER_BLOCK 13u           /* h2o_hpack_parse_request's own: req[b].err names the text */
uint64_t hhuff_h2_streams_scratch_size(uint32_t nslots, uint32_t max_entries);
static inline uint32_t hhuff_h2_streams_entries(uint32_t max_streams, uint32_t max_streams_for_priority, uint32_t max_push) {
    uint64_t n = (uint64_t)max_streams + 1u + max_streams_for_priority + max_push;
    return n > 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)n;
}
/* a frame owes at most the control call's 17 bytes and 26 of its own, an op 13 */
static inline uint64_t hhuff_h2_streams_reply_bound(uint64_t frame_slots, uint64_t nops) { return 43u * frame_slots + 13u * nops; }
int hhuff_h2_streams(const hhuff_conn_slots_t *slots, const hhuff_h2_streams_params_t *params,
                     const uint8_t *in, uint64_t in_size,
                     const hhuff_h2_frame_t *frames, const uint32_t *nframes, const uint32_t *frm_first, uint32_t frm_cap,
                     const hhuff_h2_ctl_t *ctl, const uint32_t *nctl, const uint8_t *ctl_rep, uint64_t ctl_rep_size,
                     const uint32_t *ctl_rep_off /* [nconn + 1] */,
                     const hhuff_h2_block_t *blocks, const uint32_t *conn_first /* [nconn + 1] */,
                     const int32_t *bstatus, const hhuff_request_t *req,
                     const uint8_t *arena, uint64_t arena_size, const uint32_t *blk_off,
                     const uint32_t *value_off, const uint32_t *value_len,
                     const hhuff_h2_peer_t *peers,
                     const hhuff_h2_stream_op_t *ops, const uint32_t *op_first /* [nconn + 1] */, uint32_t nops,
                     uint32_t nconn,
                     hhuff_h2_sev_t *sev, hhuff_h2_sev_t *op_sev,
                     uint32_t *nstr, int32_t *sstatus, uint32_t *serr,
                     uint8_t *rep, uint64_t rep_size, const uint32_t *rep_off /* [nconn + 1] */, uint32_t *rep_len,
                     void *scratch, uint64_t scratch_size, unsigned flags, void *stream);
int hhuff_h2_streams_fill_sends(const hhuff_conn_slots_t *slots, uint32_t max_entries, void *scratch, uint64_t scratch_size,
                                hhuff_h2_send_t *sends, const uint32_t *send_first /* [nconn + 1] */, uint32_t nsend,
                                uint32_t nconn, uint8_t *miss /* [nsend] */, void *stream);
int hhuff_h2_streams_commit_sent(const hhuff_conn_slots_t *slots, uint32_t max_entries, void *scratch, uint64_t scratch_size,
                                 const hhuff_h2_send_t *sends, const hhuff_h2_sent_t *sent,
                                 const uint32_t *send_first /* [nconn + 1] */, uint32_t nsend, uint32_t nconn, void *stream);

/* (2l) HTTP/3 frames on the receive side: the bytes of many connections' QUIC streams -> the encoder-stream bytes
 *      and field sections the decoders of (2d) take, and the peers' SETTINGS.  One call is one step of every stream.
 *      It follows h2o_http3_read_frame (lib/http3/common.c:1057-1145), the request-stream handlers of h2o's server
 *      (lib/http3/server.c:1367-1453, 1499-1536) and client (lib/common/http3client.c:438-540),
 *      unknown_type_handle_input and control_stream_handle_input (common.c:365-439),
 *      h2o_http3_handle_settings_frame (common.c:1422-1473) and h2o_http3_decode_priority_update_frame /
 *      h2o_http3_decode_goaway_frame (lib/http3/frame.c:40-98).
 *        stream s       in[str_off[s] .. str_off[s+1]): the bytes the previous step did not consume, then the new
 *                       ones; its state st_in[s]; frame slots frm_first[s] .. frm_first[s+1] - 1 of `frames`
 *                       (frm_first[nstr] = frm_cap, host copy)
 *        connection c   owns streams conn_str[c] .. conn_str[c+1] - 1 (conn_str[nconn] = nstr)
 *        max_frame_payload_size   h2o's conn->max_frame_payload_size
 *        flags          HHUFF_H3F_CLIENT: is_client of read_frame's table, and the client's handlers
 *      Per stream: st_out[s] the state to present next time (st_out may be st_in), nframes[s], consumed[s] (relative
 *      to str_off[s]; the caller keeps in[str_off[s] + consumed[s] ..) and presents it again in front of the next
 *      bytes), sstatus[s] = 0, h2o's return value as it is (0x30000 + code, as HHUFF_QPK_DECOMPRESSION_FAILED) or
 *      HHUFF_H3F_REJECTED / _FRAMES / _EINVAL, serr[s] = the HHUFF_H3F_ERR_* that names h2o's err_desc.
 *        frames         frames[frm_first[s] + i], i < nframes[s]: the frames walked, in wire order; the other slots
 *                       are not written.  The body bytes that continue a DATA frame begun in an earlier step get a
 *                       record with hdr_off == payload_off, length = the data_left presented and avail = the bytes
 *                       taken.
 *        out            in_size bytes.  First the connections' QPACK encoder-stream bytes in connection order:
 *                       out[enc_off[c] .. + enc_len[c]), the bytes of several _QPACK_ENCODER streams of one connection
 *                       joined in stream order.  Behind them the field sections packed back to back, in stream
 *                       order: section k = out[sec_off[k] .. sec_off[k+1]), connection c's sections conn_first[c] ..
 *                       conn_first[c+1] - 1.  A stream yields at most one section a call (rules 3 and 6), so sec_off
 *                       has nstr + 1 entries -- those past nsec all hold the end, so they read as empty sections --,
 *                       conn_first nconn + 1, and sec_stream_id[k] (the stream's stream_id) and sec_stream[k] (its
 *                       index in this call) are written for k < nsec.
 *        totals         [0] = nsec, [1] = the section bytes, [2] = the encoder bytes
 *        arena_off      NULL, or nstr + 1 u64: the running sum of arena_fixed + arena_per_byte * (section length)
 *                       over the sections before k (entries past nsec hold the total)
 *      out, enc_off, enc_len, sec_off, conn_first, sec_stream_id and nconn are, as they are and on the same stream,
 *      the in, enc_off, enc_len, sec_off, conn_first, stream_id and nconn of hhuff_qpack_decode, _parse_requests,
 *      _parse_responses and their _slots and _sessions variants, with this call's in_size.  Their host copy of nsec
 *      is totals[0]; a caller that does not read it back may pass nstr to hhuff_qpack_decode, _parse_requests and
 *      _parse_responses: the sections past conn_first[nconn] are empty, lie in no connection's range, and get a
 *      status nobody reads (the per-section arrays then need nstr entries).
 *        peers, settings, got_settings   got_settings[c] = 1 when a control stream of connection c passed its
 *                       SETTINGS frame in this call, else 0.  Only then are peers[c] (the raw
 *                       SETTINGS_QPACK_MAX_TABLE_CAPACITY and _BLOCKED_STREAMS, 0 when absent, saturated at
 *                       2^32 - 1) and settings[c] written, so a persistent peers array fills as connections arrive
 *                       and goes to hhuff_qpack_flatten_sessions_peers unchanged.  h2o's clamp to its own
 *                       encoder_table_capacity is the min(capacity, header_table_size) that call makes.  A repeated
 *                       setting id takes the last value, as h2o's loop does.  Of several control streams of one
 *                       connection that pass SETTINGS in one call (h2o has one) the first in stream order is taken.
 *      The call keeps no state.  Streams do not affect one another, although h2o closes the connection on most of
 *      the errors below: what to do with a failed connection's other sections is the caller's decision.  Per stream
 *      the bytes are walked by these rules, in h2o's order.  The first failing rule stops that stream's walk:
 *      the failing frame is neither listed nor consumed, and what was completed before stands.
 *      Request streams (kind _REQUEST):
 *      1. h2o_http3_read_frame: a type varint cut short: sstatus 0 (h2o: H2O_HTTP3_ERROR_INCOMPLETE, wait); a length
 *         varint cut short: 0; for any type but DATA, length > max_frame_payload_size: 0x30101
 *         (H2O_HTTP3_ERROR_GENERAL_PROTOCOL, _ERR_FRAME_TOO_LARGE), decided before completeness; then the payload cut
 *         short: 0; then the type table (common.c:1124-1132) for the side and the stream kind: 0x30105
 *         (H2O_HTTP3_ERROR_FRAME_UNEXPECTED).  Unknown types pass.  A DATA frame needs only its header.  Varints of
 *         every width are read as ptls_decode_quicint reads them, non-minimal encodings included.
 *      2. Server, phase _HEADERS (server.c:1499-1536): a too-large HEADERS frame is HHUFF_H3F_REJECTED (h2o resets the
 *         stream with REQUEST_REJECTED and returns 0; serr stays _ERR_FRAME_TOO_LARGE); every other read_frame error
 *         is returned as it is; DATA is 0x30105; other types are listed and stepped over.
 *      3. Server, a HEADERS frame in _HEADERS: it becomes the stream's section (aux = its index k), st_out.phase =
 *         _DATA, and the walk stops behind the frame: what follows depends on the decoder's verdict, which this call
 *         cannot know.  With HHUFF_H3S_WALK_ON it goes on as if the section had decoded.  A caller whose section
 *         comes back HHUFF_QPK_BLOCKED keeps the stream from the record's hdr_off with st_in, as h2o's *src =
 *         frame_start does (server.c:1555).
 *      4. Server, phase _DATA (server.c:1411-1453): HEADERS under HHUFF_H3S_TUNNEL is 0x30105 with
 *         _ERR_UNEXPECTED_TYPE; otherwise it is trailers: listed with aux = ~0u, no section, phase _POST_TRAILERS.
 *         DATA of non-zero length opens _DATA_PAYLOAD with data_left = length, and the bytes present are taken at
 *         once (avail of them; data_left falls, and at 0 the phase is _DATA again); DATA of length 0 is listed and
 *         the phase stays.  Other types are listed and stepped over.
 *      5. Server, phase _POST_TRAILERS (server.c:1367-1386): HEADERS and DATA are 0x30105.
 *      6. Client, phase _HEADERS (http3client.c:506-540): any read_frame error but incomplete is 0x30107
 *         (H2O_HTTP3_ERROR_EXCESSIVE_LOAD) with _ERR_RESPONSE_TOO_LARGE; DATA is 0x30105 with
 *         _ERR_DATA_BEFORE_HEADERS; HEADERS is the section and the walk stops, or goes on under _WALK_ON.  A 1xx
 *         answer is the caller's to see: it then presents _HEADERS again.
 *      7. Client, phase _DATA (http3client.c:438-504): read_frame errors are returned as they are; HEADERS under
 *         _TUNNEL is 0x30105 (no err_desc), else it is listed with aux = ~0u and ignored -- the client has no
 *         post-trailers phase, and a client state record with _POST_TRAILERS is HHUFF_H3F_EINVAL --; PUSH_PROMISE
 *         and unknown types are listed and ignored; DATA as in rule 4.  For a DATA frame of length 0
 *         handle_input_expect_data_frame sets bytes_left_in_data_frame = 0 and enters handle_input_data_payload,
 *         which appends nothing, sets the handler back to expect_data_frame at once and calls on_body without
 *         bytes: the frame is listed with avail 0 and the phase stays _DATA, as on the server.
 *      Unidirectional streams:
 *      8. _UNI (common.c:403-439): the type varint cut short: wait, nothing consumed; 0: _CONTROL at _SETTINGS; 2:
 *         _QPACK_ENCODER; 3: _QPACK_DECODER; anything else (push streams included): _DISCARD -- h2o sends STOP_SENDING
 *         with STREAM_CREATION; the caller sees the kind change.  The same call goes on with the new kind.
 *      9. _QPACK_ENCODER: every byte is gathered and consumed.  The decoder's enc_consumed[c] then tells the caller
 *         what to present again.
 *      10. _QPACK_DECODER: nothing (but the type varint of rule 8) is consumed: those bytes are
 *         hhuff_qpack_flatten_sessions' dec_off / dec_len.
 *      11. _DISCARD: everything is consumed.
 *      Control streams (kind _CONTROL):
 *      12. Per frame read_frame (rule 1 with the control column); then common.c:384-388: has_received_settings ==
 *         (type == SETTINGS), or DATA, is 0x30105 without err_desc -- in phase _SETTINGS any other first frame, in
 *         _OPEN a second SETTINGS.  That test fires before server.c:1910 can say MISSING_SETTINGS (0x3010a), so h2o
 *         never reports that code, and neither does this call.
 *      13. Then the handler (server.c:1903-1948, http3client.c:339-376): SETTINGS by
 *         h2o_http3_handle_settings_frame -- a varint cut short, a datagram value (ids 0x33, 0x276) other than 0 or
 *         1, or 1 without HHUFF_H3S_PEER_DATAGRAMS is 0x30106 (H2O_HTTP3_ERROR_FRAME, _ERR_MALFORMED_SETTINGS) --,
 *         then phase _OPEN.  On the server PRIORITY_UPDATE (0xF0700, 0xF0701) by
 *         h2o_http3_decode_priority_update_frame: an empty payload or an element id of the wrong kind is 0x30106
 *         without err_desc; aux = the id's bytes (the priority field value follows them).  An id cut short is what
 *         h2o makes of it: frame.c:49 stores the decoder's UINT64_MAX in the 63-bit field `element` before comparing,
 *         so "invalid PRIORITY frame" is never said (HHUFF_H3F_ERR_INVALID_PRIORITY names it and is never reported)
 *         and the id reads as 2^63 - 1, a server-initiated unidirectional stream: 0x30106 for 0xF0700, and for
 *         0xF0701 the frame passes with aux = 1, the byte ptls_decode_quicint had taken.  On the client GOAWAY by h2o_http3_decode_goaway_frame: a cut
 *         varint or bytes behind it are 0x30106 with _ERR_INVALID_GOAWAY; aux = the id's bytes.  Everything else
 *         (the server's GOAWAY, CANCEL_PUSH and MAX_PUSH_ID included) is listed with aux 0 and stepped over.
 *      All streams:
 *      14. A frame that passed its rules and finds no frame slot left: HHUFF_H3F_FRAMES, at that frame's boundary.
 *      HHUFF_H3F_EINVAL reports a state record with an unknown kind, phase or flag bit, a non-zero reserved byte,
 *      a non-zero phase on a kind that has none, data_left != 0 outside _DATA_PAYLOAD or _DATA_PAYLOAD with
 *      data_left == 0: nothing is consumed and st_out[s] = st_in[s].
 *      Device arrays.  Returns HHUFF_EINVAL, before any device call, for a NULL array (arena_off may be NULL),
 *      in_size > 2^32 - 3 or an unknown flag bit; nstr == 0 or nconn == 0 returns HHUFF_OK.  Asynchronous on
 *      `stream`, no atomics, no host synchronisation and no copy to the host; bitwise deterministic.  Stream-ordered
 *      pool workspace of 65 bytes per stream and 16 per 256 of them (hhuff_pool_trim).  A stream's range is clamped to in_size, its slots
 *      to frm_cap and a connection's streams to nstr.  Of `in` the call reads the streams' bytes and, with them, the
 *      aligned dwords (by address) that hold a section's or an encoder run's bytes, as (2k) does. */
typedef struct hhuff_h3_stream {     /* 32 bytes: one stream's state between steps */
    uint64_t stream_id;              /* the QUIC stream id (goes to sec_stream_id) */
    uint64_t data_left;              /* _DATA_PAYLOAD: the bytes of the open DATA frame still to come; else 0 */
    uint8_t  kind, phase, flags;     /* HHUFF_H3K_*, HHUFF_H3P_*, HHUFF_H3S_* */
    uint8_t  rsv[13];                /* 0 */
} hhuff_h3_stream_t;
typedef struct hhuff_h3_frame {      /* 32 bytes: one per frame walked */
    uint64_t type;
    uint32_t hdr_off, payload_off;   /* offsets in `in`: the type varint, the payload */
    uint64_t length;                 /* the frame's length field */
    uint32_t avail;                  /* the payload bytes present: length, except for DATA */
    uint32_t aux;                    /* HEADERS: the section index, ~0u when it is no section; PRIORITY_UPDATE
                                        (server) and GOAWAY (client): the bytes of the leading id varint; else 0 */
} hhuff_h3_frame_t;
typedef struct hhuff_h3_settings {   /* 16 bytes: what SETTINGS says beside the QPACK values */
    uint64_t max_field_section_size; /* SETTINGS_MAX_FIELD_SECTION_SIZE; UINT64_MAX when the frame has none */
    uint32_t h3_datagram;            /* 1: the peer enabled HTTP/3 datagrams */
    uint32_t rsv;
} hhuff_h3_settings_t;
#ifdef __cplusplus
static_assert(sizeof(hhuff_h3_stream_t) == 32 && sizeof(hhuff_h3_frame_t) == 32 && sizeof(hhuff_h3_settings_t) == 16, "record sizes");
#else
typedef char hhuff_h3_records_are_32_bytes[sizeof(hhuff_h3_stream_t) == 32 && sizeof(hhuff_h3_frame_t) == 32 &&
                                           sizeof(hhuff_h3_settings_t) == 16 ? 1 : -1];
#endif
#define HHUFF_H3F_CLIENT 1u           /* flags: the receiving side is h2o's client */
#define HHUFF_H3F_REJECTED (-320)     /* sstatus: a too-large HEADERS frame in _HEADERS on the server */
#define HHUFF_H3F_FRAMES (-321)       /* sstatus: out of frame slots */
#define HHUFF_H3F_EINVAL (-322)       /* sstatus: the state record is not one this call writes */
#define HHUFF_H3F_ERR_NONE 0u               /* *err_desc untouched */
#define HHUFF_H3F_ERR_FRAME_TOO_LARGE 1u    /* h2o_http3_err_frame_too_large */
#define HHUFF_H3F_ERR_UNEXPECTED_TYPE 2u    /* "unexpected frame type" */
#define HHUFF_H3F_ERR_DATA_BEFORE_HEADERS 3u /* "received DATA frame before HEADERS" */
#define HHUFF_H3F_ERR_RESPONSE_TOO_LARGE 4u /* "response header too large" */
#define HHUFF_H3F_ERR_MALFORMED_SETTINGS 5u /* "malformed SETTINGS frame" */
#define HHUFF_H3F_ERR_INVALID_PRIORITY 6u   /* "invalid PRIORITY frame": h2o never says it (rule 13) */
#define HHUFF_H3F_ERR_INVALID_GOAWAY 7u     /* "Invalid GOAWAY frame" */
#define HHUFF_H3K_REQUEST 0u
#define HHUFF_H3K_UNI 1u              /* a unidirectional stream whose type varint has not been read */
#define HHUFF_H3K_CONTROL 2u
#define HHUFF_H3K_QPACK_ENCODER 3u
#define HHUFF_H3K_QPACK_DECODER 4u
#define HHUFF_H3K_DISCARD 5u
#define HHUFF_H3P_HEADERS 0u          /* request streams */
#define HHUFF_H3P_DATA 1u
#define HHUFF_H3P_DATA_PAYLOAD 2u
#define HHUFF_H3P_POST_TRAILERS 3u
#define HHUFF_H3P_SETTINGS 0u         /* control streams */
#define HHUFF_H3P_OPEN 1u
#define HHUFF_H3S_WALK_ON 1u          /* go on behind the section as if it had decoded */
#define HHUFF_H3S_TUNNEL 2u           /* server: req.is_tunnel_req; client: upgrade_to != NULL */
#define HHUFF_H3S_PEER_DATAGRAMS 4u   /* the remote transport parameter max_datagram_frame_size != 0 */
int hhuff_h3_deframe(const uint8_t *in, uint64_t in_size,            /* in_size <= 2^32 - 3 */
                     const uint32_t *str_off, uint32_t nstr,         /* stream s: in[str_off[s] .. str_off[s+1]) */
                     const uint32_t *conn_str, uint32_t nconn,       /* connection c: streams conn_str[c] .. conn_str[c+1] */
                     const uint32_t *frm_first, uint32_t frm_cap,    /* frame slots; frm_cap = frm_first[nstr] (host copy) */
                     uint64_t max_frame_payload_size, unsigned flags,
                     const hhuff_h3_stream_t *st_in, hhuff_h3_stream_t *st_out,
                     hhuff_h3_frame_t *frames, uint32_t *nframes, uint32_t *consumed,
                     int32_t *sstatus, uint32_t *serr,
                     uint8_t *out, uint32_t *enc_off, uint32_t *enc_len, uint32_t *sec_off, uint32_t *conn_first,
                     uint64_t *sec_stream_id, uint32_t *sec_stream,
                     uint32_t *totals /* [3]: nsec, section bytes, encoder bytes */,
                     hhuff_qpack_peer_t *peers, hhuff_h3_settings_t *settings, uint32_t *got_settings,
                     uint64_t *arena_off, uint64_t arena_fixed, uint32_t arena_per_byte, void *stream);

/* (3b) Pipelined host path (the socket-buffer -> pinned -> device -> pinned -> pool staging of
 *     SURVEY f3; replaces the caller-side copies around lib/http2/hpack.c:240-241).  Contiguous layout
 *     (in_off[n + 1], implicit output slots) only.  The batch is cut into chunks of about
 *     `chunk_bytes` input bytes (0 = 64 MiB) at multiples of 32 strings; chunks flow through three
 *     streams so that host staging copies, H2D, kernels and D2H of different chunks overlap.  Caller
 *     buffers already pinned (hipHostMalloc / hipHostRegister) are DMA'd directly.  Synchronous; the
 *     results equal hhuff_*_batch_host's.  hhuff_*_batch_host take this path by themselves for
 *     contiguous batches of 128 MiB and more.  in_off[n] <= in_size, and out_size reaches the slots' end (decode
 *     floor(8 * in_off[n] / 5), encode in_off[n]): anything else is HHUFF_EINVAL before any device work (3d's host
 *     mode likewise).  Only bytes of `out` inside the batch's slot range are written. */
int hhuff_decode_batch_host_pipelined(const uint8_t *in, uint64_t in_size, const uint32_t *in_off, uint32_t n,
                                      const uint32_t *is_name_bits, uint8_t *out, uint64_t out_size,
                                      uint32_t *out_len, uint8_t *status, int device, uint64_t chunk_bytes);
int hhuff_encode_batch_host_pipelined(const uint8_t *in, uint64_t in_size, const uint32_t *in_off, uint32_t n,
                                      uint8_t *out, uint64_t out_size, uint32_t *out_len, uint8_t *status,
                                      int device, uint64_t chunk_bytes);

/* (3c) Packed host path: hhuff_decode_batch_packed / hhuff_encode_batch_packed on host arrays (same layout: every
 *     64-string tile's outputs back to back from the tile's slot position, out_off[n + 1]).  Contiguous layout.
 *     With every array pinned (hipHostMalloc / hipHostRegister), `in` and `out` 16-byte aligned and the u32 arrays
 *     4-byte aligned, the kernels read the input and write the results in host memory themselves and only the
 *     output bytes cross PCIe (the slot layout's unused slot tails do not); otherwise the call stages the batch
 *     through device memory.  out_size >= the slot end (decode floor(8 in_off[n] / 5), encode in_off[n]).
 *     out_off may be NULL: the offsets are then not returned (4 bytes a string fewer across the link) and string i
 *     starts at its tile's position (decode floor(8 in_off[64 t] / 5), encode in_off[64 t], t = i / 64) plus the
 *     out_len of the tile's earlier strings that did not fail.  An encode's status may be NULL (out_len already
 *     says HHUFF_FAIL_LEN); a decode's may not.  Synchronous. */
int hhuff_decode_batch_host_packed(const uint8_t *in, uint64_t in_size, const uint32_t *in_off, uint32_t n,
                                   const uint32_t *is_name_bits, uint8_t *out, uint64_t out_size, uint32_t *out_off,
                                   uint32_t *out_len, uint8_t *status, int device);
int hhuff_encode_batch_host_packed(const uint8_t *in, uint64_t in_size, const uint32_t *in_off, uint32_t n,
                                   uint8_t *out, uint64_t out_size, uint32_t *out_off, uint32_t *out_len,
                                   uint8_t *status, int device);

/* (3d) Multi-device batch (SURVEY 2 new component 5, 8e): one batch over several GPUs of one process, for h2o's
 *     C callers (lib/http2/hpack.c:241, lib/http3/qpack.c:228 -- worker threads, src/main.c:5512) that have no
 *     torch.distributed.  The contiguous layout of hhuff_decode_batch / hhuff_encode_batch (in_off[n + 1], implicit
 *     output slots: decode floor(8 in_off[i] / 5), encode in_off[i]) is cut byte-balanced into ndev shards
 *     (hhuff_shard_bounds with align 64) and shard k runs on devices[k] (NULL: devices 0 .. ndev-1).  Offsets
 *     stay absolute, so every string lands where the one-device call puts it: the shards' outputs are already
 *     concatenated in shard order, and out_len / status are byte for byte the one-device call's.
 *       src_device == HHUFF_HOST_MEMORY: every array is host memory; each device runs its shard through the host
 *         path (zero copy on pinned, aligned arrays, else the chunked pipeline of 3b), all devices at once, each
 *         from its own library thread.  Synchronous; `stream` is ignored.
 *       src_device >= 0: every array is device memory of src_device, ordered on `stream` (a stream of src_device,
 *         NULL the null stream).  The call waits for the work queued before it on `stream` (the cut reads
 *         in_off), then enqueues: the src device's own shard in place on an internal stream of src_device, every
 *         other shard as peer copies (xGMI) of its input bytes, offsets and name bits to scratch on its device,
 *         the kernel there, and peer copies of its output slots, lengths and statuses back; `stream` then waits
 *         for every shard.  Returns once all is enqueued (asynchronous, like hhuff_decode_batch).
 *     ndev == 1 with devices[0] == src_device is the one-device call. */
#define HHUFF_HOST_MEMORY (-1)
int hhuff_decode_batch_multi(int ndev, const int *devices, int src_device, const uint8_t *in, uint64_t in_size,
                             const uint32_t *in_off, uint32_t n, const uint32_t *is_name_bits, uint8_t *out,
                             uint64_t out_size, uint32_t *out_len, uint8_t *status, void *stream);
int hhuff_encode_batch_multi(int ndev, const int *devices, int src_device, const uint8_t *in, uint64_t in_size,
                             const uint32_t *in_off, uint32_t n, uint8_t *out, uint64_t out_size, uint32_t *out_len,
                             uint8_t *status, void *stream);
/* The byte-balanced cut (host arrays, no GPU): bounds[0] = 0, bounds[nshards] = n and, for 0 < k < nshards,
 * bounds[k] = the first string i with in_off[i] >= in_off[0] + floor(k (in_off[n] - in_off[0]) / nshards), rounded
 * down to a multiple of `align` (0 or 1: no rounding).  Non-decreasing.  With align 1 it equals h2o_amd/dist.py
 * byte_balanced_bounds (the torch.distributed path's split). */
int hhuff_shard_bounds(const uint32_t *in_off, uint32_t n, uint32_t nshards, uint32_t align, uint32_t *bounds);

/* ---------------------------------------------------------------------------------------------
 * (4) library info
 * ------------------------------------------------------------------------------------------- */
const char *hhuff_version(void);
/* Text of the last HIP error seen by this thread ("" if none). */
const char *hhuff_last_error_string(void);
/* Number of workgroups the decode / encode launches use on `device` (grid sizing, for profiling). */
/* The prices a mixed-length decode (mean Huffman length 41..128 B) uses to choose between the staged and the
 * stream kernel: out4 = {staged ps per string, staged ps per tile-padded byte, stream ps per string, stream ps
 * per byte}.  A decode never measures them itself: they are fitted MI355X defaults until
 * hhuff_calibrate_decode_prices or hhuff_set_decode_prices runs for the device.  No GPU work.  HHUFF_OK or an
 * error code. */
int hhuff_decode_prices(int device, float *out4);
/* Measure this device's prices now (both kernels timed on two probe batches, about 2 ms; synchronous: it
 * allocates and frees device memory, so call it at start-up, not beside in-flight work) and use them from
 * then on; out4 (may be NULL) receives them.  A failed or implausible fit keeps the prices in effect. */
int hhuff_calibrate_decode_prices(int device, float *out4);
/* Pin the prices of `device` (e.g. a previous calibration's, so every process chooses alike); in4 NULL
 * restores the fitted defaults.  HHUFF_EINVAL for a negative or non-finite value. */
int hhuff_set_decode_prices(int device, const float *in4);
int hhuff_grid_size(int device, int which /* 0 decode, 1 encode */);
/* Which kernel decodes contiguous batches (process-wide; the results are the same, only the speed differs):
 * 0 (default) the staged kernels for short strings and the device-side staged / stream choice for mixed and long
 * ones.  Modes 1 and 2 (the segment kernel -- a tile's bits shared evenly over a wave's lanes -- above a 40-B mean,
 * or for every contiguous batch) exist only in A/B builds of the library (tools/ab.py, -DHHUFF_AB_VARIANTS=1; there
 * HHUFF_DEC_SEG sets the start value): the product library accepts 0 and returns HHUFF_EINVAL for them.
 * Returns the previous mode, or HHUFF_EINVAL. */
int hhuff_set_decode_kernel(int mode);
/* Batches of at least `n` strings leave the 16-B output chunks their tiles share to edge records and a fix-up
 * kernel launched behind the codec kernel; smaller batches store those chunks in the codec kernel (one launch).
 * Default 0xFFFFFFFF: every batch stores them in the kernel.  Process-wide; the results are the same, only the
 * speed differs.  Returns the previous value. */
uint32_t hhuff_set_edge_defer_min(uint32_t n);
/* Return the memory the library's stream-ordered pool on the caller's current device keeps between calls
 * (batch workspaces, edge records) to the driver.  Synchronises the device first.  HHUFF_OK or an error. */
int hhuff_pool_trim(void);
/* Debug query for the tests: the resident workgroups per compute unit of the length-sorted encode kernel that
 * hhuff_encode_batch would launch on the caller's current device for a contiguous batch of `n` strings in
 * `in_size` bytes (the kernel has two stage sizes, picked from in_size / n).  0 where another kernel would run;
 * negative on a runtime error. */
int hhuff_debug_encode_blocks_per_cu(uint64_t in_size, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif
