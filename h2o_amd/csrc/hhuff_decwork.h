// The workspaces of the two header-block decoders (hhuff_blocks.hip: HPACK, hhuff_qpack.hip: QPACK), host side
// only and without HIP, so a plain C++ program can carve them (tools/decwork_host.cpp).  Both decoders run the
// same literal pre-pass -- mark every string literal in a bitmap, list the marks, decode the listed literals
// (launch_literal_list, launch_literals_dev) -- and its pieces are laid out once, in lit_work.  A whole call's
// workspace is one Carve sequence (hpd_carve, qpd_carve) run twice, as the encoders' are (hhuff_enc.h).
// Pieces are 256-byte aligned.
#pragma once
#include <stdint.h>

#include "hhuff_carve.h"

namespace hhuff {
constexpr uint64_t kDecAlign = 256;

// The list pass takes kLitChunkWords bitmap words per block; chunk: u32[literal_list_chunks(nwords) + 1]
constexpr uint32_t kLitChunkWords = 1024;
inline uint64_t literal_list_chunks(uint64_t nwords) { return (nwords + kLitChunkWords - 1) / kLitChunkWords; }

// What a decoder sizes its pre-pass by: bitmap words (a bit per input byte), chunks of them, and the most
// literals the input can hold
struct LitDims {
    uint64_t nwords, nchunks, n_max;
};
inline LitDims hpd_dims(uint64_t in_size) {  // HPACK: a field with two literals takes >= 3 bytes
    const uint64_t nwords = (in_size + 31) / 32;
    return {nwords, literal_list_chunks(nwords), (2 * in_size) / 3 + 2};
}
inline LitDims qpd_dims(uint64_t in_size) {  // QPACK: every literal header takes a byte
    const uint64_t nwords = in_size / 32 + 1;
    return {nwords, literal_list_chunks(nwords), in_size + 2};
}
// HPACK runs the pre-pass for inputs below 4 GiB (u32 positions); QPACK always (the C ABI refuses larger inputs)
inline bool hpd_prepass(uint64_t in_size) { return in_size > 0 && in_size < (1ull << 32); }

struct LitWork {
    // start zeroed: bit p of lit_bits marks a literal at input byte p, of name_bits a name, of p3_bits (with
    // `alt`) one with the alternative prefix; bit r of lnames: literal r is a name
    uint32_t *lit_bits, *name_bits, *p3_bits, *lnames;
    uint32_t* word_pre;  // [nwords] marks before each bitmap word
    uint32_t* chunk;     // [nchunks + 1] chunk sums, then their prefixes; chunk[nchunks] = the literal count
    uint32_t* list;      // [n_max] positions in order
    uint8_t* pfx;        // [n_max] (with `alt`) the prefix literal r is decoded with
    uint32_t *len, *pay, *cons;  // [n_max] the literal kernels' results
    uint8_t* st;                 // [n_max]
    uint8_t* ws;                 // the literal kernels' own workspace (literals_dev_ws bytes)
    uint8_t* out;                // decoded bytes: literal r at floor(8 pay[r] / 5)
};

// The pre-pass's pieces, the zeroed ones first: taken at the front of a workspace, [0, cv.off after lnames)
// is what the call's one memset clears (*zero_end)
inline LitWork lit_work(Carve& cv, const LitDims& d, uint64_t in_size, uint64_t ws_bytes, bool alt, uint64_t* zero_end) {
    LitWork W;
    W.lit_bits = cv.take<uint32_t>(d.nwords);
    W.name_bits = cv.take<uint32_t>(d.nwords);
    W.p3_bits = alt ? cv.take<uint32_t>(d.nwords) : nullptr;
    W.lnames = cv.take<uint32_t>((d.n_max + 31) / 32);
    *zero_end = cv.off;
    W.word_pre = cv.take<uint32_t>(d.nwords);
    W.chunk = cv.take<uint32_t>(d.nchunks + 1);
    W.list = cv.take<uint32_t>(d.n_max);
    W.pfx = alt ? cv.take<uint8_t>(d.n_max) : nullptr;
    W.len = cv.take<uint32_t>(d.n_max);
    W.pay = cv.take<uint32_t>(d.n_max);
    W.cons = cv.take<uint32_t>(d.n_max);
    W.st = cv.take<uint8_t>(d.n_max);
    W.ws = cv.take<uint8_t>(ws_bytes);
    W.out = cv.take<uint8_t>((8 * in_size) / 5 + 64);
    return W;
}

// A call's workspace: its size with base = NULL, its pointers with the allocation.  fsrc_n / fsrc_v: a byte
// source per field slot (one slot per input byte, and one to spare).
struct HpdWork {
    LitWork lit;  // set with hpd_prepass(in_size) only
    uint64_t zero_end;
    uint64_t *fsrc_n, *fsrc_v;
};
inline uint64_t hpd_carve(HpdWork& W, uint64_t in_size, uint64_t ws_bytes, uint8_t* base) {
    Carve cv{base, 0, kDecAlign};
    W.lit = LitWork{};
    W.zero_end = 0;
    if (hpd_prepass(in_size)) W.lit = lit_work(cv, hpd_dims(in_size), in_size, ws_bytes, false, &W.zero_end);
    W.fsrc_n = cv.take<uint64_t>(in_size + 1);
    W.fsrc_v = cv.take<uint64_t>(in_size + 1);
    return cv.off;
}

struct QpdWork {
    LitWork lit;
    uint64_t zero_end;
    uint64_t *fsrc_n, *fsrc_v;
    uint32_t* map;  // [map_conns] a session step's connection map when the caller brought no slot map
};
inline uint64_t qpd_carve(QpdWork& W, uint64_t in_size, uint64_t ws_bytes, uint64_t map_conns, uint8_t* base) {
    Carve cv{base, 0, kDecAlign};
    W.lit = lit_work(cv, qpd_dims(in_size), in_size, ws_bytes, true, &W.zero_end);
    W.fsrc_n = cv.take<uint64_t>(in_size + 1);
    W.fsrc_v = cv.take<uint64_t>(in_size + 1);
    W.map = cv.take<uint32_t>(map_conns);
    return cv.off;
}
}  // namespace hhuff
