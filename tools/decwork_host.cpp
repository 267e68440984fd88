// The decoders' workspace carves (h2o_amd/csrc/hhuff_decwork.h) on the host, to be built with
// -fsanitize=address,undefined: for a sweep of input sizes each workspace is sized on a null base, allocated at
// exactly that size, carved again, and every piece is filled to the bytes its kernel writes with a tag of its
// own and read back.  The sanitizer catches a write past the allocation, the tags an overlap.  Also checked:
// every piece 256-byte aligned, the zeroed pieces one prefix of the workspace.  One JSON line per case with each
// piece's offset and room (the distance to the next piece), for tests/test_dec_workspace.py; "ok" at the end.
#include "hhuff_decwork.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace hhuff;

namespace {
struct Piece {
    const char* name;
    const void* p;
    uint64_t bytes;  // what the kernels write or read there
    bool zeroed;
};

int fail(const char* what, const char* piece, uint64_t S) {
    printf("FAIL: %s (%s, in_size %llu)\n", what, piece, (unsigned long long)S);
    return 1;
}

std::vector<Piece> pieces_of(const LitWork& L, bool lit, bool alt, const LitDims& d, uint64_t S, uint64_t ws_bytes,
                             const uint64_t* fsrc_n, const uint64_t* fsrc_v, const uint32_t* map, uint64_t map_conns) {
    std::vector<Piece> v;
    if (lit) {
        v.push_back({"lit_bits", L.lit_bits, 4 * d.nwords, true});
        v.push_back({"name_bits", L.name_bits, 4 * d.nwords, true});
        if (alt) v.push_back({"p3_bits", L.p3_bits, 4 * d.nwords, true});
        v.push_back({"lnames", L.lnames, 4 * ((d.n_max + 31) / 32), true});
        v.push_back({"word_pre", L.word_pre, 4 * d.nwords, false});
        v.push_back({"chunk", L.chunk, 4 * d.nchunks + 4, false});
        v.push_back({"list", L.list, 4 * d.n_max, false});
        if (alt) v.push_back({"pfx", L.pfx, d.n_max, false});
        v.push_back({"len", L.len, 4 * d.n_max, false});
        v.push_back({"pay", L.pay, 4 * d.n_max, false});
        v.push_back({"cons", L.cons, 4 * d.n_max, false});
        v.push_back({"st", L.st, d.n_max, false});
        v.push_back({"ws", L.ws, ws_bytes, false});
        v.push_back({"out", L.out, (8 * S) / 5 + 64, false});
    }
    v.push_back({"fsrc_n", fsrc_n, 8 * S + 8, false});
    v.push_back({"fsrc_v", fsrc_v, 8 * S + 8, false});
    if (map_conns) v.push_back({"map", map, 4 * map_conns, false});
    return v;
}

// fill, read back, check the layout, print the case
int exercise(const char* kind, uint64_t S, uint64_t nconn, uint64_t ws_bytes, uint8_t* base, uint64_t total, uint64_t zero_end,
             std::vector<Piece> v) {
    for (size_t k = 0; k < v.size(); ++k) {
        if (!v[k].p) return fail("NULL piece", v[k].name, S);
        if (((uintptr_t)v[k].p & (kDecAlign - 1)) != 0) return fail("piece not 256-byte aligned", v[k].name, S);
        memset(const_cast<void*>(v[k].p), (int)(k + 1), v[k].bytes);
    }
    for (size_t k = 0; k < v.size(); ++k) {
        const uint8_t* q = static_cast<const uint8_t*>(v[k].p);
        for (uint64_t i = 0; i < v[k].bytes; ++i)
            if (q[i] != (uint8_t)(k + 1)) return fail("tag overwritten: pieces overlap", v[k].name, S);
    }
    std::sort(v.begin(), v.end(), [](const Piece& a, const Piece& b) { return a.p < b.p; });
    uint64_t zeroed_to = 0;  // the zeroed pieces: back to back from offset 0, up to zero_end
    printf("{\"kind\": \"%s\", \"in_size\": %llu, \"nconn\": %llu, \"ws_bytes\": %llu, \"total\": %llu, \"zero_end\": %llu, "
           "\"pieces\": {",
           kind, (unsigned long long)S, (unsigned long long)nconn, (unsigned long long)ws_bytes, (unsigned long long)total,
           (unsigned long long)zero_end);
    for (size_t k = 0; k < v.size(); ++k) {
        const uint64_t off = (uint64_t)(static_cast<const uint8_t*>(v[k].p) - base);
        const uint64_t next = k + 1 < v.size() ? (uint64_t)(static_cast<const uint8_t*>(v[k + 1].p) - base) : total;
        if (v[k].zeroed) {
            if (off != zeroed_to) return fail("zeroed pieces are not one prefix", v[k].name, S);
            zeroed_to = next;
        } else if (off < zero_end) {
            return fail("piece inside the zeroed prefix", v[k].name, S);
        }
        printf("%s\"%s\": [%llu, %llu]", k ? ", " : "", v[k].name, (unsigned long long)off, (unsigned long long)(next - off));
    }
    printf("}}\n");
    if (zeroed_to != zero_end) return fail("zero_end is not the end of the zeroed pieces", kind, S);
    return 0;
}

int hpack_case(uint64_t S) {
    const LitDims d = hpd_dims(S);
    const uint64_t ws_bytes = hpd_prepass(S) ? 4 * d.n_max + 100 : 0;  // (any size will do: literals_dev_ws's stand-in)
    HpdWork W;
    const uint64_t total = hpd_carve(W, S, ws_bytes, nullptr);
    uint8_t* base = static_cast<uint8_t*>(aligned_alloc(kDecAlign, total));
    if (!base) return fail("allocation", "hpack", S);
    if (hpd_carve(W, S, ws_bytes, base) != total) return fail("the two passes differ", "hpack", S);
    const int rc = exercise("hpack", S, 0, ws_bytes, base, total, W.zero_end,
                            pieces_of(W.lit, hpd_prepass(S), false, d, S, ws_bytes, W.fsrc_n, W.fsrc_v, nullptr, 0));
    free(base);
    return rc;
}

int qpack_case(uint64_t S, uint64_t map_conns) {
    const LitDims d = qpd_dims(S);
    const uint64_t ws_bytes = 4 * d.n_max + 100;
    QpdWork W;
    const uint64_t total = qpd_carve(W, S, ws_bytes, map_conns, nullptr);
    uint8_t* base = static_cast<uint8_t*>(aligned_alloc(kDecAlign, total));
    if (!base) return fail("allocation", "qpack", S);
    if (qpd_carve(W, S, ws_bytes, map_conns, base) != total) return fail("the two passes differ", "qpack", S);
    const int rc = exercise(map_conns ? "qpack_sessions" : "qpack", S, map_conns, ws_bytes, base, total, W.zero_end,
                            pieces_of(W.lit, true, true, d, S, ws_bytes, W.fsrc_n, W.fsrc_v, W.map, map_conns));
    free(base);
    return rc;
}
}  // namespace

int main() {
    const uint64_t sizes[] = {0, 1, 2, 31, 32, 33, 32767, 32768, 32769, (1ull << 20) + 1};
    for (uint64_t S : sizes) {
        if (hpack_case(S) || qpack_case(S, 0) || qpack_case(S, 1) || qpack_case(S, 3)) return 1;
    }
    const uint64_t big[] = {(1ull << 32) - 3, (1ull << 32) - 1, 1ull << 32};
    for (uint64_t S : big) {  // the size pass alone
        HpdWork H;
        QpdWork Q;
        const uint64_t hws = hpd_prepass(S) ? 4 * hpd_dims(S).n_max + 100 : 0, qws = 4 * qpd_dims(S).n_max + 100;
        printf("{\"kind\": \"hpack_size\", \"in_size\": %llu, \"nconn\": 0, \"ws_bytes\": %llu, \"total\": %llu}\n",
               (unsigned long long)S, (unsigned long long)hws, (unsigned long long)hpd_carve(H, S, hws, nullptr));
        printf("{\"kind\": \"qpack_size\", \"in_size\": %llu, \"nconn\": 0, \"ws_bytes\": %llu, \"total\": %llu}\n",
               (unsigned long long)S, (unsigned long long)qws, (unsigned long long)qpd_carve(Q, S, qws, 0, nullptr));
    }
    printf("ok\n");
    return 0;
}
