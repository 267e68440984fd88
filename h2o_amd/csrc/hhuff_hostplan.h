// The arithmetic of the host-array and multi-device batch paths (hhuff_capi_host.hip, hhuff_capi_multi.hip): implicit
// output slots, the chunk cuts of `pipelined`, the device layout a chunk and a shard copied to a peer device share,
// the packed runs of `host_packed` and the byte-balanced shard cut.  Plain integer code with no HIP call in it:
// tools/hostplan_host.cpp builds it with a host compiler under sanitizers and tests/test_hostplan_host.py compares
// what it computes with tests/host_paths_model.py and h2o_amd/dist.py.
#ifndef HHUFF_HOSTPLAN_H
#define HHUFF_HOSTPLAN_H
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HHUFF_PLAN_HD __host__ __device__ inline  // shard_bound: also called by shard_bounds_kernel
#else
#define HHUFF_PLAN_HD inline
#endif

namespace hhuff {

constexpr int kDepth = 3;                             // pipelined host path: staging slots, reused round-robin
constexpr uint64_t kDefaultChunk = 64ull << 20;       // pipelined host path: input bytes per chunk
constexpr size_t kPackedChunk = (size_t)64 << 20;     // host_packed: bytes of the device output staged at a time
constexpr uint32_t kShardAlign = 64;                  // a shard starts on a tile (and on an is-name word)
constexpr uint32_t kPlanFailLen = 0xFFFFFFFFu;        // HHUFF_FAIL_LEN (include/hhuff.h): such a string keeps no bytes

inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// the implicit output slot of input position pos
inline uint64_t slot_of(bool decode, uint64_t pos) { return decode ? (pos * 8) / 5 : pos; }

// The contiguous layout with implicit output slots: the strings lie inside `in` (in_end = in_off[n]) and the last
// slot ends inside `out`.  NULL, or the text the call is refused with.
inline const char* implicit_refusal(bool decode, uint64_t in_size, uint64_t in_end, uint64_t out_size) {
    if (in_end > in_size) return "in_off[n] > in_size";
    if (out_size < slot_of(decode, in_end)) return "out_size below the output slots of the batch";
    return nullptr;
}

// `pipelined`'s chunk boundaries: from string a, the first string starting past in_off[a] + chunk_bytes (the target
// clamped to 2^32 - 1), rounded down to a + 32 k, at least a + 32, capped at n.  chunk_bytes 0: kDefaultChunk.
inline std::vector<uint64_t> chunk_cuts(const uint32_t* in_off, uint64_t n, uint64_t chunk_bytes) {
    if (chunk_bytes == 0) chunk_bytes = kDefaultChunk;
    std::vector<uint64_t> cut{0};
    while (cut.back() < n) {
        const uint64_t a = cut.back();
        const uint64_t target = (uint64_t)in_off[a] + chunk_bytes;
        uint64_t b = (uint64_t)(std::upper_bound(in_off + a, in_off + n + 1, (uint32_t)std::min<uint64_t>(target, 0xFFFFFFFFull)) -
                                in_off);  // first string starting past the target
        b = b > a + 32 ? ((b - a) / 32) * 32 + a : a + 32;
        cut.push_back(std::min<uint64_t>(b, n));
    }
    return cut;
}

// m strings whose bytes are [s0, e0) of `in`, on a device buffer of their own: a chunk of the host pipeline, or a
// shard copied to a peer device.  [in bytes from base][in_off m + 1][names][out slots from obase][out_len m][status m]:
// the kernels get `in` shifted back by base and `out` by obase, so the batch's absolute offsets address the buffer.
// base is a multiple of 80 bytes: the decode slot floor(8 base / 5) stays 16-byte aligned.
struct ChunkLayout {
    uint64_t base, nbytes;      // first input byte held, and bytes from there to e0
    uint64_t olo, ohi, obase;   // slot_of s0, e0 and base: [olo, ohi) goes back to the caller
    uint64_t ocap;              // bytes of the output piece
    size_t nw;                  // is-name words (0 for encode and without names)
    size_t o_off, o_nm, o_out, o_len, o_st, need;  // the pieces' offsets (the input is at 0) and the buffer's size
};
inline ChunkLayout chunk_layout(bool decode, uint64_t s0, uint64_t e0, uint64_t m, bool has_names) {
    const uint64_t base = (s0 / 80) * 80;
    const uint64_t nbytes = e0 - base;
    const uint64_t olo = slot_of(decode, s0), ohi = slot_of(decode, e0), obase = slot_of(decode, base);
    const uint64_t ocap = ohi - obase + 16;
    const size_t nw = decode && has_names ? (size_t)(m + 31) / 32 : 0;
    const size_t o_off = up16(nbytes + 16), o_nm = o_off + up16((m + 1) * 4), o_out = o_nm + up16(nw * 4),
                 o_len = o_out + up16(ocap), o_st = o_len + up16(m * 4), need = o_st + up16(m);
    return {base, nbytes, olo, ohi, obase, ocap, nw, o_off, o_nm, o_out, o_len, o_st, need};
}

// host_packed's runs: tile t (64 strings) keeps [its slot position, end of its last kept string), which follows
// from the out_off / out_len the packed kernels returned
inline uint32_t packed_ntiles(uint32_t n) { return (n + 63) / 64; }
inline uint64_t run_lo(bool decode, const uint32_t* in_off, uint32_t t) { return slot_of(decode, in_off[(size_t)t * 64]); }
inline uint64_t run_hi(uint32_t n, const uint32_t* out_off, const uint32_t* out_len, uint32_t t) {
    const uint32_t last = (t + 1) * 64 < n ? (t + 1) * 64 - 1 : n - 1;
    return (uint64_t)out_off[last] + (out_len[last] != kPlanFailLen ? out_len[last] : 0);
}

// the byte-balanced cut (hhuff_shard_bounds): the first string at or past the k/ns quantile of the bytes, rounded
// down to a multiple of align -- a lower_bound over in_off[0 .. n], the same search as dist.byte_balanced_bounds
HHUFF_PLAN_HD uint32_t shard_bound(const uint32_t* in_off, uint32_t n, uint32_t k, uint32_t ns, uint32_t align) {
    if (k == 0) return 0;
    if (k >= ns) return n;
    const uint64_t base = in_off[0];
    const uint64_t end = in_off[n];
    const uint64_t target = base + (end > base ? ((uint64_t)k * (end - base)) / ns : 0);
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)in_off[mid] < target)
            lo = mid + 1;
        else
            hi = mid;
    }
    return align > 1 ? lo - lo % align : lo;
}

}  // namespace hhuff
#endif
