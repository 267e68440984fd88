// Token interning (include/hhuff.h (2j), hhuff_tokens.h): name -> token id, one lane per string.
//   tok_intern_kernel<MODE, LDS>  a workgroup of 256 lanes takes kItems consecutive items.  With LDS it first copies
//                      the table into dynamic LDS (16 B a lane a round; tables up to kLdsBudget), otherwise it probes
//                      the table where it lies; lane 0 checks the header once and leaves the view in LDS.  Then
//                      every lane assembles its name from the aligned dwords that hold it (funnel shift), hashes,
//                      probes and compares dwordwise (tok_find, the code the host builder and tools/tokens_host.cpp
//                      run).
//     MODE kStrings    item i = in[off[i] .. + len[i])
//          kFields     the decoders' output shape: the first wave finds the block of the workgroup's first slot by
//                      a 64-ary search over `first`; a wave takes 64 consecutive slots, loads the next 64 block
//                      starts from there, one a lane, and every lane finds its block among them by a search over
//                      the lanes; a lane whose slot is one of its block's fields interns it, the others write
//                      nothing
//          kHeaders    item h = the name of hdr[h]; the flags word is rewritten in place
// The three entry points of the C ABI are at the end of this file: each is one launch, no workspace.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_tokens.h"

#define HHUFF_API extern "C" __attribute__((visibility("default")))

namespace hhuff {
namespace {
using namespace tok;

constexpr uint32_t kThreads = 256;
constexpr uint32_t kRounds = 8, kItems = kThreads * kRounds;  // items a workgroup: the staging is paid once for them
// Tables up to this size are staged: with 32 KiB a workgroup five workgroups fit a CU's 160 KiB (20 waves, five a
// SIMD); h2o's 85 names make a table of 3.3 KiB, which leaves the wave slots (8 a SIMD) as the limit.
constexpr uint64_t kLdsBudget = 32768;

enum { kStrings = 0, kFields = 1, kHeaders = 2 };

struct TokArgs {
    const uint32_t* table;
    uint64_t table_size;
    const uint8_t* in;
    uint64_t in_size;
    const uint32_t* off;  // kStrings: off / len [n]; kFields: name_off / name_len [nslots]
    const uint32_t* len;
    const uint32_t* first;    // kFields: [nblk + 1]
    const uint32_t* nfields;  // kFields: [nblk]
    uint32_t nblk;
    uint32_t n;     // items: strings, slots or headers
    uint32_t* hdr;  // kHeaders: 5 dwords a header
    uint32_t keep_mask;
    int32_t* token;
    uint32_t* user_out;
    uint32_t miss_user;
};

struct DevTable {  // global memory, or the LDS copy (the address space follows the pointer's origin)
    const uint32_t* p;
    __device__ __forceinline__ uint32_t word(uint32_t i) const { return p[i]; }
};

// A name at any address: the aligned dwords that hold its bytes, and no others, shifted into place.  With r the
// name's offset in its first aligned dword, name dword k is bytes r .. r + 3 of the aligned pair (k, k + 1).
struct DevName {
    const uint32_t* p;  // the aligned dword that holds the first byte
    uint32_t r8;        // 8 r
    uint32_t nal;       // aligned dwords that hold name bytes: ceil((r + len) / 4) >= the name's dwords
    __device__ __forceinline__ DevName(const uint8_t* s, uint32_t len) {
        const uint32_t r = (uint32_t)((uintptr_t)s & 3u);
        p = reinterpret_cast<const uint32_t*>(s - r), r8 = 8u * r, nal = (r + len + 3u) >> 2;
    }
    struct Reader {
        const uint32_t* p;
        uint32_t r8, left, w0;
        __device__ __forceinline__ uint32_t next() {
            uint32_t w1 = 0;
            if (left != 0) w1 = *p++, --left;
            const uint32_t w = __builtin_amdgcn_alignbit(w1, w0, r8);
            w0 = w1;
            return w;
        }
    };
    __device__ __forceinline__ Reader reader() const { return Reader{p + 1, r8, nal - 1u, p[0]}; }
};

// The block of slot x: the largest b with first[b] <= x (0 when there is none), by one wave.  A round probes 64
// evenly spaced entries of what is left, one a lane, and the ballot says between which two the answer lies: four
// dependent loads for 300,000 blocks where a binary search by one lane takes eighteen.  Called by a whole wave with
// wave-uniform arguments; every index stays below nblk + 1 whatever `first` holds.
__device__ __forceinline__ uint32_t block_of(const uint32_t* first, uint32_t nblk, uint32_t x, uint32_t lane) {
    uint64_t lo = 0, hi = (uint64_t)nblk + 1u;  // entries below lo are <= x, those from hi on are > x
    while (lo < hi) {
        const uint64_t span = hi - lo, step = (span + 63u) >> 6;
        auto probe = [&](uint64_t k) { return lo + (((k + 1u) * step < span) ? (k + 1u) * step : span) - 1u; };  // < hi
        const uint32_t cnt = (uint32_t)__builtin_popcountll(__ballot(first[probe(lane)] <= x));
        const uint64_t nlo = cnt ? probe(cnt - 1u) + 1u : lo, nhi = cnt < 64u ? probe(cnt) : hi;
        lo = nlo, hi = nhi < nlo ? nlo : nhi;
    }
    return lo == 0 ? 0u : (uint32_t)(lo - 1u);
}

template <int MODE, bool LDS>
__global__ __launch_bounds__(kThreads) void tok_intern_kernel(TokArgs A) {
    extern __shared__ uint4 staged[];
    __shared__ View sview;
    __shared__ uint32_t sok, sblk;
    const uint32_t tid = threadIdx.x;
    if (LDS) {
        const uint4* src = reinterpret_cast<const uint4*>(A.table);
        const uint32_t n16 = (uint32_t)(A.table_size >> 4);  // <= kLdsBudget / 16 (the launch sized the LDS by it)
        for (uint32_t i = tid; i < n16; i += kThreads) staged[i] = src[i];
        __syncthreads();
    }
    const DevTable T{LDS ? reinterpret_cast<const uint32_t*>(staged) : A.table};
    const uint64_t item0 = (uint64_t)blockIdx.x * kItems;  // < n: the grid is ceil(n / kItems)
    if (tid < 64u) {  // the first wave: the workgroup's block, and lane 0 checks the header
        const uint32_t b0 = MODE == kFields ? block_of(A.first, A.nblk, (uint32_t)item0, tid) : 0u;
        if (tid == 0) {
            View v{};
            sok = view(T, A.table_size, v) ? 1u : 0u;
            sview = v, sblk = b0;
        }
    }
    __syncthreads();
    const bool ok = sok != 0;
    const View v = sview;
    const uint32_t sblock = MODE == kFields ? sblk : 0u;

    for (uint32_t round = 0; round < kRounds; ++round) {
        const uint64_t i = item0 + round * kThreads + tid;
        bool act = i < A.n;
        if (MODE == kFields) {
            const uint64_t base64 = i & ~63ull;
            if (base64 >= A.n) continue;  // (wave-uniform)
            // Slot -> block.  From the workgroup's block the wave loads the next 64 block starts, one a lane, and
            // every lane counts those at or below its slot by a binary search over the lanes (no memory access);
            // a lane for which all 64 are looks 64 blocks further (empty blocks, or blocks of a slot or two).
            const uint32_t lane = tid & 63u;
            const uint32_t s = act ? (uint32_t)i : (uint32_t)base64;  // (lanes past the last slot: any valid slot)
            uint32_t b = sblock, fb = A.first[b], j = 0, fj = 0;
            bool found = false;
            for (;;) {
                const uint32_t e = (uint64_t)b + 1u + lane <= A.nblk ? A.first[b + 1u + lane] : 0xFFFFFFFFu;  // (> any slot)
                uint32_t c = 0;  // loaded starts <= s
#pragma unroll
                for (uint32_t step = 32; step > 0; step >>= 1) c += (uint32_t)__shfl((int)e, (int)(c + step - 1u)) <= s ? step : 0u;
                const uint32_t e63 = (uint32_t)__shfl((int)e, 63);  // (every lane takes part in every shuffle)
                if (c == 63u && e63 <= s) c = 64u;
                const uint32_t prev = (uint32_t)__shfl((int)e, (int)((c - 1u) & 63u));  // the start of block b + c, c > 0
                if (!found && c < 64u) j = b + c, fj = c ? prev : fb, found = true;
                if (!__any(!found)) break;
                b += 64u, fb = A.first[b];  // (a lane with c == 64 saw first[b + 64]: b + 64 <= nblk)
            }
            // block j is the last that starts at or below s, so s < first[j + 1]; j == nblk: behind the last block
            const uint32_t nf = j < A.nblk ? A.nfields[j] : 0u;
            act = act && j < A.nblk && s >= fj && s - fj < nf;
        }
        if (!act) continue;
        uint32_t off, len, flags = 0;
        if (MODE == kHeaders) {
            off = A.hdr[5u * i], len = A.hdr[5u * i + 1u];
            if (ok) flags = A.hdr[5u * i + 4u];
        } else {
            off = A.off[i], len = A.len[i];
        }
        int32_t tk = HHUFF_TOK_EFORMAT;
        uint32_t user = A.miss_user;
        if (ok) {
            tk = HHUFF_TOK_NONE;
            if (len - 1u < kMaxName && (uint64_t)off + len <= A.in_size) tk = tok_find(T, v, DevName(A.in + off, len), len, &user);
        }
        if (A.token) A.token[i] = tk;
        if (!ok) continue;
        if (MODE == kHeaders) A.hdr[5u * i + 4u] = (flags & A.keep_mask) | (tk >= 0 ? user : 0u);
        else if (A.user_out) A.user_out[i] = user;
    }
}

template <int MODE>
hipError_t launch(const TokArgs& A, hipStream_t stream) {
    const uint32_t grid = (uint32_t)(((uint64_t)A.n + kItems - 1u) / kItems);
    if (A.table_size <= kLdsBudget)
        hipLaunchKernelGGL((tok_intern_kernel<MODE, true>), dim3(grid), dim3(kThreads), (size_t)(A.table_size & ~15ull), stream, A);
    else
        hipLaunchKernelGGL((tok_intern_kernel<MODE, false>), dim3(grid), dim3(kThreads), 0, stream, A);
    return hipGetLastError();
}

bool table_args_ok(const void* table, uint64_t table_size) {
    return table && table_size >= kHeaderBytes && ((uintptr_t)table & 15u) == 0;
}
}  // namespace
}  // namespace hhuff

HHUFF_API uint64_t hhuff_tokens_table_size(uint32_t ntokens, uint64_t name_bytes) {
    return hhuff::tok::table_bytes(ntokens, name_bytes);
}

HHUFF_API int hhuff_tokens_build(const uint8_t* names, const uint32_t* name_off, uint32_t ntokens, const uint32_t* user,
                                 void* table, uint64_t table_size) {
    return hhuff::tok::build(names, name_off, ntokens, user, table, table_size);
}

HHUFF_API int hhuff_intern_strings(const void* table, uint64_t table_size, const uint8_t* in, uint64_t in_size,
                                   const uint32_t* off, const uint32_t* len, uint32_t n, int32_t* token, uint32_t* user_out,
                                   uint32_t miss_user, void* stream) {
    if (!hhuff::table_args_ok(table, table_size)) return HHUFF_EINVAL;
    if (n == 0) return HHUFF_OK;
    if (!in || !off || !len || !token) return HHUFF_EINVAL;
    hhuff::TokArgs A{};
    A.table = (const uint32_t*)table, A.table_size = table_size, A.in = in, A.in_size = in_size, A.off = off, A.len = len;
    A.n = n, A.token = token, A.user_out = user_out, A.miss_user = miss_user;
    return hhuff::launch<hhuff::kStrings>(A, (hipStream_t)stream) == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}

HHUFF_API int hhuff_intern_fields(const void* table, uint64_t table_size, const uint8_t* arena, uint64_t arena_size,
                                  const uint32_t* name_off, const uint32_t* name_len, const uint32_t* first,
                                  const uint32_t* nfields, uint32_t nblk, uint32_t nslots, int32_t* token, uint32_t* user_out,
                                  uint32_t miss_user, void* stream) {
    if (!hhuff::table_args_ok(table, table_size)) return HHUFF_EINVAL;
    if (nblk == 0 || nslots == 0) return HHUFF_OK;
    if (!arena || !name_off || !name_len || !first || !nfields || !token) return HHUFF_EINVAL;
    hhuff::TokArgs A{};
    A.table = (const uint32_t*)table, A.table_size = table_size, A.in = arena, A.in_size = arena_size;
    A.off = name_off, A.len = name_len, A.first = first, A.nfields = nfields, A.nblk = nblk;
    A.n = nslots, A.token = token, A.user_out = user_out, A.miss_user = miss_user;
    return hhuff::launch<hhuff::kFields>(A, (hipStream_t)stream) == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}

HHUFF_API int hhuff_intern_headers(const void* table, uint64_t table_size, const uint8_t* in, uint64_t in_size,
                                   hhuff_hpack_header_t* hdr, uint32_t nhdr, uint32_t keep_mask, int32_t* token, void* stream) {
    if (!hhuff::table_args_ok(table, table_size)) return HHUFF_EINVAL;
    if (nhdr == 0) return HHUFF_OK;
    if (!in || !hdr) return HHUFF_EINVAL;
    static_assert(sizeof(hhuff_hpack_header_t) == 20, "five dwords a header");
    hhuff::TokArgs A{};
    A.table = (const uint32_t*)table, A.table_size = table_size, A.in = in, A.in_size = in_size;
    A.n = nhdr, A.hdr = (uint32_t*)hdr, A.keep_mask = keep_mask, A.token = token;
    return hhuff::launch<hhuff::kHeaders>(A, (hipStream_t)stream) == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}
