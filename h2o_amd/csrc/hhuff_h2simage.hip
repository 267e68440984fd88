// HTTP/2 stream table images (include/hhuff.h (2k'''); format, checks and the serial twin in hhuff_h2simage.h).
// One template over the lanes that share a connection, two instantiations:
//   LANES = 64   a wave per connection, four connections a workgroup: tables of up to 512 slots (max_entries <= 256);
//                the lanes of a wave run in lock step, so LDS traffic between them is ordered by wave-scope fences
//   LANES = 256  a workgroup per connection: 1024 to 4096 slots, __syncthreads between the phases
//   h2si_export_kernel  the lanes sweep the table's slots and stage the live stream ids in LDS (kFree for a free slot);
//                       the count is clamped to what the sweep found and to max_entries; length, room and status are
//                       settled before the first store; the ids are sorted in LDS by a bitonic network over the slot
//                       count; lane j takes the j-th id, probes for its entry and writes the normalised record as three
//                       16-byte stores.  Scratch is only read.  LDS: 4 bytes a slot, 8 KB (4 x 512) or 16 KB (4096).
//   h2si_import_kernel  header and state are checked by every lane alike, the records by lane (each against its
//                       predecessor's id) and the verdicts reduced by ballot (through LDS between waves); then the LDS
//                       word of every slot is set free and the entries are placed in rounds: every unplaced entry bids
//                       for slot (home + round) & mask with an LDS atomicMin of kBid | index -- a taken slot holds an
//                       index below kBid and never changes, a free one goes to the lowest bidder -- until all are
//                       placed.  Then every slot of the slab is written once, by the lane that sweeps it: its owner's
//                       record or zeros; the Head last, with fill_epoch = 1.  Nothing is stored before every check
//                       has passed, and the slab is a function of the image alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_h2simage.h"
#include "hhuff_launch.h"
#include "hhuff_slots.h"

#define HHUFF_API extern "C" __attribute__((visibility("default")))

namespace hhuff {
namespace {
using namespace h2i;

constexpr uint32_t kBid = 0x80000000u;  // an LDS owner word: index (taken) < kBid | index (a bid) < kFree

struct SiArgs {
    uint8_t* scratch;
    uint64_t slab;
    uint32_t max_entries, nslots, n;
    const uint32_t* slot;  // export
    const uint32_t* cmap;  // import: the call's connection map (hhuff_slots.h)
    uint8_t* img;
    const uint64_t* img_off;
    uint32_t* img_len;
    int32_t* status;
};

// The lanes of one connection: what orders their LDS traffic and reduces over them.
template <int LANES>
struct Group {
    static constexpr uint32_t kConns = 256 / LANES;                // connections a workgroup
    static constexpr uint32_t kCap = LANES == 64 ? 512u : kMaxCap; // the largest table it takes
    static constexpr uint32_t kPerLane = kCap / 2 / LANES;         // entries a lane places at most
    static __device__ __forceinline__ uint32_t lane() { return threadIdx.x & (LANES - 1); }
    static __device__ __forceinline__ uint64_t conn() { return (uint64_t)blockIdx.x * kConns + threadIdx.x / LANES; }
    static __device__ __forceinline__ void sync() {
        if constexpr (LANES == 64) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        } else {
            __syncthreads();
        }
    }
    // true when p holds for any lane; red: a word of LDS the workgroup instantiation reduces through
    static __device__ __forceinline__ bool any(bool p, uint32_t* red) {
        if constexpr (LANES == 64) {
            return __ballot(p) != 0;
        } else {
            __syncthreads();  // (the last round's readers of *red are through)
            if (threadIdx.x == 0) *red = 0;
            __syncthreads();
            if (__ballot(p) != 0 && (threadIdx.x & 63) == 0) *red = 1;
            __syncthreads();
            return *red != 0;
        }
    }
    // the sum of the lanes' counts of p
    static __device__ __forceinline__ uint32_t count(bool p, uint32_t* red) {
        const uint32_t mine = (uint32_t)__popcll(__ballot(p));
        if constexpr (LANES == 64) {
            return mine;
        } else {
            __syncthreads();
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mine;
            __syncthreads();
            return red[0] + red[1] + red[2] + red[3];
        }
    }
};

__device__ __forceinline__ void put16(uint8_t* d, const void* s) {
    uint4 w;
    __builtin_memcpy(&w, s, 16);
    *reinterpret_cast<uint4*>(d) = w;
}
// a 48-byte record to a 16-byte aligned place
__device__ __forceinline__ void put_entry(uint8_t* d, const Entry& e) {
    const uint8_t* s = reinterpret_cast<const uint8_t*>(&e);
    put16(d, s), put16(d + 16, s + 16), put16(d + 32, s + 32);
}

template <int LANES>
__global__ __launch_bounds__(256) void h2si_export_kernel(SiArgs A) {
    using G = Group<LANES>;
    __shared__ uint32_t s_ids[G::kConns * G::kCap];
    __shared__ uint32_t s_red[4];
    const uint32_t lane = G::lane();
    const uint64_t k = G::conn();
    if (k >= A.n) return;  // (the lanes of a connection leave together: no barrier waits for them)
    const uint32_t slot = A.slot[k];
    if (slot >= A.nslots) {
        if (lane == 0) A.img_len[k] = 0, A.status[k] = HHUFF_IMG_EINVAL;
        return;
    }
    const h2s::Table T = h2s::table_at(A.scratch + (uint64_t)slot * A.slab, A.max_entries);
    const uint32_t cap = T.mask + 1u;  // <= G::kCap: the launcher picked the instantiation
    uint32_t* ids = s_ids + (threadIdx.x / LANES) * G::kCap;
    const Head H = *T.head;
    uint32_t found = 0;
    for (uint32_t i0 = 0; i0 < cap; i0 += LANES) {  // (cap >= LANES, or it is 4 .. 32 and one pass covers it)
        const uint32_t i = i0 + lane;
        uint32_t id = kFree;
        if (i < cap) {
            id = T.ent[i].stream_id;
            if (id == 0) id = kFree;
            ids[i] = id;
        }
        found += G::count(id != kFree, s_red);
    }
    uint32_t count = H.count < found ? H.count : found;
    if (count > A.max_entries) count = A.max_entries;
    const uint32_t total = (uint32_t)image_bytes(count);
    int32_t rc = 0;
    if (A.img) {
        const uint64_t o0 = A.img_off[k], o1 = A.img_off[k + 1];
        if (o1 < o0 || o1 - o0 < total) rc = HHUFF_IMG_SPACE;
    }
    if (lane == 0) A.img_len[k] = total, A.status[k] = rc;
    if (!A.img || rc != 0) return;

    // bitonic sort of ids[0 .. cap), ascending: the free slots' kFree ends up behind the live ids
    for (uint32_t size = 2; size <= cap; size <<= 1) {
        for (uint32_t stride = size >> 1; stride != 0; stride >>= 1) {
            G::sync();
            for (uint32_t i = lane; i < cap; i += LANES) {
                const uint32_t p = i ^ stride;
                if (p <= i) continue;
                const uint32_t a = ids[i], b = ids[p];
                if ((a > b) == ((i & size) == 0)) ids[i] = b, ids[p] = a;
            }
        }
    }
    G::sync();

    uint8_t* out = A.img + A.img_off[k];
    if (lane < 4) {
        struct {
            Header h;
            State s;
        } fixed{make_header(total), state_of(H, count)};
        static_assert(sizeof(fixed) == kFixed && kFixed == 4 * 16, "header and state");
        uint4 w[4];
        __builtin_memcpy(w, &fixed, sizeof(fixed));
        const uint4 piece = lane == 0 ? w[0] : lane == 1 ? w[1] : lane == 2 ? w[2] : w[3];  // (selects, no indexed private array)
        put16(out + 16 * lane, &piece);
    }
    for (uint32_t j = lane; j < count; j += LANES) {
        const uint32_t at = h2s::find(T, ids[j]);
        Entry e{};  // (an id no probe reaches: not a table any call left; import refuses the record)
        if (at != h2s::kNone) e = normalised(T.ent[at], H.fill_epoch);
        put_entry(out + kFixed + sizeof(Entry) * (uint64_t)j, e);
    }
}

template <int LANES>
__global__ __launch_bounds__(256) void h2si_import_kernel(SiArgs A) {
    using G = Group<LANES>;
    __shared__ uint32_t s_own[G::kConns * G::kCap];
    __shared__ uint32_t s_red[4];
    const uint32_t lane = G::lane();
    const uint64_t k = G::conn();
    if (k >= A.n) return;
    const ConnSlot cs = conn_slot_of(A.cmap[k]);
    if (cs.refused) {
        if (lane == 0) A.status[k] = HHUFF_IMG_EINVAL;
        return;
    }
    const uint64_t o0 = A.img_off[k], o1 = A.img_off[k + 1];
    const uint64_t len = A.img_len[k];
    const uint8_t* in = A.img + o0;
    int32_t rc = HHUFF_IMG_EFORMAT;
    State s{};
    if (o1 >= o0 && len <= o1 - o0 && len >= kFixed && (len - kFixed) % sizeof(Entry) == 0) {
        s = load<State>(in + sizeof(Header));
        rc = check_fixed(load<Header>(in), s, len, A.max_entries);
    }
    if (rc != 0) {  // (the same for every lane of the connection)
        if (lane == 0) A.status[k] = rc;
        return;
    }
    const h2s::Table T = h2s::table_at(A.scratch + cs.slot * A.slab, A.max_entries);
    const uint32_t cap = T.mask + 1u;
    uint32_t* own = s_own + (threadIdx.x / LANES) * G::kCap;

    // the records, each against the one in front of it; a lane keeps the ids and homes of those it will place
    uint32_t home[G::kPerLane];
    bool ok = true;
#pragma unroll
    for (uint32_t q = 0; q < G::kPerLane; ++q) {
        const uint32_t j = lane + q * LANES;
        home[q] = kFree;  // nothing to place
        if (j < s.count) {
            const Entry e = record(in, j);
            const uint32_t prev = j != 0 ? load<uint32_t>(in + kFixed + sizeof(Entry) * (uint64_t)(j - 1u)) : 0u;
            ok = ok && check_entry(e, prev);
            home[q] = h2s::home(T, e.stream_id);
        }
    }
    for (uint32_t i = lane; i < cap; i += LANES) own[i] = kFree;
    if (G::any(!ok, s_red)) {
        if (lane == 0) A.status[k] = HHUFF_IMG_EFORMAT;
        return;
    }

    // the rounds: count <= cap / 2, so every entry meets a free slot within cap of them
    for (uint32_t r = 0; r < cap; ++r) {
        G::sync();
#pragma unroll
        for (uint32_t q = 0; q < G::kPerLane; ++q)
            if (home[q] != kFree) atomicMin(&own[(home[q] + r) & T.mask], kBid | (lane + q * LANES));
        G::sync();
        bool left = false;
#pragma unroll
        for (uint32_t q = 0; q < G::kPerLane; ++q) {
            if (home[q] == kFree) continue;
            const uint32_t at = (home[q] + r) & T.mask, j = lane + q * LANES;
            if (own[at] == (kBid | j))
                own[at] = j, home[q] = kFree;
            else
                left = true;
        }
        if (!G::any(left, s_red)) break;
    }
    G::sync();

    for (uint32_t i = lane; i < cap; i += LANES) {
        const uint32_t j = own[i];
        Entry e{};
        if (j < s.count) e = record(in, j);  // (checked: rsv 0, mark 0 or 1)
        put_entry(reinterpret_cast<uint8_t*>(T.ent + i), e);
    }
    if constexpr (LANES != 64) __syncthreads();
    if (lane == 0) {
        const Head H = head_of(s);
        put16(reinterpret_cast<uint8_t*>(T.head), &H);
        put16(reinterpret_cast<uint8_t*>(T.head) + 16, reinterpret_cast<const uint8_t*>(&H) + 16);
        A.status[k] = 0;
    }
}

template <int LANES>
uint32_t grid_of(uint32_t n) {
    return (uint32_t)(((uint64_t)n + Group<LANES>::kConns - 1u) / Group<LANES>::kConns);
}

hipError_t launch(bool is_import, const SiArgs& A, hipStream_t stream) {
    const bool wave = h2s::table_cap(A.max_entries) <= Group<64>::kCap;
    if (wave) {
        if (is_import)
            hipLaunchKernelGGL(h2si_import_kernel<64>, dim3(grid_of<64>(A.n)), dim3(256), 0, stream, A);
        else
            hipLaunchKernelGGL(h2si_export_kernel<64>, dim3(grid_of<64>(A.n)), dim3(256), 0, stream, A);
    } else {
        if (is_import)
            hipLaunchKernelGGL(h2si_import_kernel<256>, dim3(grid_of<256>(A.n)), dim3(256), 0, stream, A);
        else
            hipLaunchKernelGGL(h2si_export_kernel<256>, dim3(grid_of<256>(A.n)), dim3(256), 0, stream, A);
    }
    return hipGetLastError();
}

// what both calls refuse before they look at n: 0, or HHUFF_EINVAL
int check_call(uint32_t max_entries, const void* scratch, uint64_t scratch_size, uint32_t nslots, const void* img) {
    if (!entries_ok(max_entries)) return HHUFF_EINVAL;
    if (nslots == 0 || nslots > kConnMaxSlots || scratch_size / h2s::slab_size(max_entries) < nslots) return HHUFF_EINVAL;
    if (((uintptr_t)scratch & 15u) != 0 || ((uintptr_t)img & 15u) != 0) return HHUFF_EINVAL;
    return HHUFF_OK;
}
}  // namespace
}  // namespace hhuff

HHUFF_API uint64_t hhuff_h2_streams_image_bound(uint32_t max_entries) {
    return hhuff::h2i::entries_ok(max_entries) ? hhuff::h2i::image_bytes(max_entries) : 0;
}

HHUFF_API int hhuff_h2_streams_export(uint32_t max_entries, const void* scratch, uint64_t scratch_size, uint32_t nslots,
                                      const uint32_t* slot, uint32_t n, uint8_t* img, const uint64_t* img_off, uint32_t* img_len,
                                      int32_t* status, void* stream) {
    using namespace hhuff;
    if (const int bad = check_call(max_entries, scratch, scratch_size, nslots, img)) return bad;
    if (n == 0) return HHUFF_OK;
    if (!scratch || !slot || !img_len || !status || (img && !img_off) || ((uintptr_t)img_off & 7u) != 0) return HHUFF_EINVAL;
    const SiArgs A{(uint8_t*)const_cast<void*>(scratch), h2s::slab_size(max_entries), max_entries, nslots, n, slot, nullptr, img, img_off,
                   img_len, status};
    return launch(false, A, (hipStream_t)stream) == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}

HHUFF_API int hhuff_h2_streams_import(uint32_t max_entries, void* scratch, uint64_t scratch_size, uint32_t nslots, const uint32_t* slot,
                                      uint32_t n, const uint8_t* img, const uint64_t* img_off, const uint32_t* img_len, int32_t* status,
                                      void* stream) {
    using namespace hhuff;
    if (const int bad = check_call(max_entries, scratch, scratch_size, nslots, img)) return bad;
    if (n == 0) return HHUFF_OK;
    if (!scratch || !slot || !img || !img_off || !img_len || !status || ((uintptr_t)img_off & 7u) != 0) return HHUFF_EINVAL;
    SiArgs A{(uint8_t*)scratch, h2s::slab_size(max_entries), max_entries, nslots, n, nullptr, nullptr, const_cast<uint8_t*>(img), img_off,
             const_cast<uint32_t*>(img_len), status};
    const hhuff_conn_slots_t slots{slot, nullptr, nslots};  // (2h) point 3: the lowest item that names a slot owns it
    uint32_t* cmap = nullptr;
    if (conn_map_make(&slots, n, (hipStream_t)stream, &cmap) != hipSuccess) return HHUFF_EHIP;
    A.cmap = cmap;
    return work_done(launch(true, A, (hipStream_t)stream), cmap, (hipStream_t)stream) == hipSuccess ? HHUFF_OK : HHUFF_EHIP;
}
