// Connection images (include/hhuff.h (2i), hhuff_image.h): one wave per listed connection.
//   img_export_kernel  reads the slab's state and its live entries 64 at a time, places every entry's strings in
//                      the run by a scan, settles the image's length and the region's room before the first store,
//                      then writes header, state, records, list and the run (wave_copy64).  Scratch is only read.
//   img_import_kernel  checks header, state, every record (by lane, reduced by ballot; the lengths' sum by scan),
//                      the list and the pad before the first store to the slab; then writes the state with the
//                      entry ring from slot 0, the entries pointing into ring 0 of this slot, the list and the run.
// A slab of another family is a different layout of the same pieces (img::Layout), not another kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hhuff_device.h"
#include "hhuff_image.h"
#include "hhuff_launch.h"
#include "hhuff_slots.h"

namespace hhuff {
namespace {
using namespace img;

struct ImgArgs {
    hhuff_conn_family_t fam;
    Layout L;
    uint8_t* scratch;
    uint32_t nslots, n;
    const uint32_t* slot;  // export
    const uint32_t* cmap;  // import: the call's connection map (hhuff_slots.h)
    uint8_t* img;
    const uint64_t* img_off;
    uint32_t* img_len;
    int32_t* status;
};

// the sum of v over the wave and the lane's exclusive prefix, in 64 bits (two 32-bit scans: 64 values of up to
// 2^31 do not fit one)
__device__ __forceinline__ uint64_t wave_excl_scan64(uint32_t v, int lane, uint64_t& total) {
    const uint32_t lo = wave_excl_scan(v & 0xFFFFu, lane), hi = wave_excl_scan(v >> 16, lane);
    const uint64_t ex = (uint64_t)lo + ((uint64_t)hi << 16);
    const uint64_t incl = ex + v;
    total = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(incl >> 32), 63) << 32) |
            (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)incl, 63);
    return ex;
}

__device__ __forceinline__ void put16(uint8_t* d, const void* s) {
    uint4 w;
    __builtin_memcpy(&w, s, 16);
    __builtin_memcpy(d, &w, 16);
}

__global__ __launch_bounds__(256) void img_export_kernel(ImgArgs A) {
    const int lane = threadIdx.x & 63;
    const uint64_t k = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (k >= A.n) return;
    const Layout& L = A.L;
    const uint32_t slot = A.slot[k];
    if (slot >= A.nslots) {
        if (lane == 0) A.img_len[k] = 0, A.status[k] = HHUFF_IMG_EINVAL;
        return;
    }
    const uint64_t sbase = (uint64_t)slot * L.slab;
    const uint8_t* slab = A.scratch + sbase;
    uint32_t start;
    State s = state_load(L, slab, start);
    uint64_t bytes = 0;
    for (uint32_t j0 = 0; j0 < s.nent; j0 += 64) {
        const uint32_t j = j0 + (uint32_t)lane;
        uint64_t no, vo, sum;
        Rec r{};
        if (j < s.nent) r = entry_load(L, slab, sbase, entry_slot(L, s, start, j), no, vo);
        wave_excl_scan64(r.nl + r.vl, lane, sum);  // each at most the slab: no 32-bit overflow
        bytes += sum;
    }
    if (bytes > L.str_cap) s.nent = 0, bytes = 0;  // not a table any call left
    s.str_bytes = (uint32_t)bytes;
    const uint64_t total = image_bytes(s.nent, s.nlist, bytes);
    int32_t rc = total > kMaxImage ? HHUFF_IMG_SPACE : 0;  // (an inflight list no u32 length can say: no image)
    if (A.img && rc == 0) {
        const uint64_t o0 = A.img_off[k], o1 = A.img_off[k + 1];
        if (o1 < o0 || o1 - o0 < total) rc = HHUFF_IMG_SPACE;
    }
    if (lane == 0) A.img_len[k] = (uint32_t)(total > kMaxImage ? kMaxImage : total), A.status[k] = rc;
    if (!A.img || rc != 0) return;

    uint8_t* out = A.img + A.img_off[k];
    {
        struct {
            Header h;
            State s;
        } fixed{make_header(A.fam, (uint32_t)total), s};
        static_assert(sizeof(fixed) == kFixed && kFixed == 6 * 16, "header and state");
        uint4 w[6];
        __builtin_memcpy(w, &fixed, sizeof(fixed));
        // lane l < 6 stores piece l (selects, not an indexed private array)
        const uint4 piece = lane == 0 ? w[0] : lane == 1 ? w[1] : lane == 2 ? w[2] : lane == 3 ? w[3] : lane == 4 ? w[4] : w[5];
        if (lane < 6) put16(out + 16 * lane, &piece);
    }
    uint8_t* recs = out + kFixed;
    uint8_t* list = recs + sizeof(Rec) * (uint64_t)s.nent;
    uint8_t* str = list + 16ull * s.nlist;
    uint64_t carry = 0;
    for (uint32_t j0 = 0; j0 < s.nent; j0 += 64) {
        const uint32_t j = j0 + (uint32_t)lane;
        const bool live = j < s.nent;
        uint64_t no = 0, vo = 0, sum;
        Rec r{};
        if (live) r = entry_load(L, slab, sbase, entry_slot(L, s, start, j), no, vo);
        const uint64_t run = carry + wave_excl_scan64(r.nl + r.vl, lane, sum);
        carry += sum;
        if (live) {
            put16(recs + sizeof(Rec) * (uint64_t)j, &r);
            put16(recs + sizeof(Rec) * (uint64_t)j + 16, reinterpret_cast<const uint8_t*>(&r) + 16);
        }
        wave_copy64(slab + no, str + run, r.nl, lane);
        wave_copy64(slab + vo, str + run + r.nl, r.vl, lane);
    }
    for (uint32_t i = (uint32_t)lane; i < s.nlist; i += 64) put16(list + 16ull * i, slab + L.list_off + 16ull * i);
    if ((uint64_t)lane < up16(bytes) - bytes) str[bytes + lane] = 0;
}

__global__ __launch_bounds__(256) void img_import_kernel(ImgArgs A) {
    const int lane = threadIdx.x & 63;
    const uint64_t k = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (k >= A.n) return;
    const Layout& L = A.L;
    const ConnSlot cs = conn_slot_of(A.cmap[k]);
    if (cs.refused) {
        if (lane == 0) A.status[k] = HHUFF_IMG_EINVAL;
        return;
    }
    const uint64_t o0 = A.img_off[k], o1 = A.img_off[k + 1];
    const uint64_t len = A.img_len[k];
    const uint8_t* in = A.img + o0;
    int32_t rc = 0;
    State s{};
    if (o1 < o0 || len > o1 - o0 || len < kFixed || (len & 15u)) {
        rc = HHUFF_IMG_EFORMAT;
    } else {
        rc = check_header(A.fam, load<Header>(in), len);
        if (rc == 0) {
            s = load<State>(in + sizeof(Header));
            if (!check_state(L, s, len)) rc = HHUFF_IMG_EFORMAT;
        }
    }
    if (rc != 0) {  // (wave-uniform)
        if (lane == 0) A.status[k] = rc;
        return;
    }
    const uint8_t* recs = in + kFixed;
    const uint8_t* list = recs + sizeof(Rec) * (uint64_t)s.nent;
    const uint8_t* str = list + 16ull * s.nlist;
    bool ok = true;
    uint64_t bytes = 0;
    for (uint32_t j0 = 0; j0 < s.nent; j0 += 64) {
        const uint32_t j = j0 + (uint32_t)lane;
        Rec r{};
        if (j < s.nent) {
            r = load<Rec>(recs + sizeof(Rec) * (uint64_t)j);
            if (!check_rec(L, s, r)) ok = false, r.nl = r.vl = 0;
        }
        uint64_t sum;
        wave_excl_scan64(r.nl + r.vl, lane, sum);
        bytes += sum;
    }
    for (uint32_t i = (uint32_t)lane; i < s.nlist; i += 64)
        if (!check_list(L, s, list + 16ull * i)) ok = false;
    if ((uint64_t)lane < up16(s.str_bytes) - s.str_bytes && str[s.str_bytes + lane] != 0) ok = false;
    if (__ballot(!ok) != 0 || bytes != s.str_bytes) {
        if (lane == 0) A.status[k] = HHUFF_IMG_EFORMAT;
        return;
    }

    const uint64_t sbase = cs.slot * L.slab;
    uint8_t* slab = A.scratch + sbase;
    if (lane == 0) state_store(L, slab, s), A.status[k] = 0;
    uint32_t carry = 0;  // the run is at most str_cap <= 2^30 + 16 bytes
    for (uint32_t j0 = 0; j0 < s.nent; j0 += 64) {
        const uint32_t j = j0 + (uint32_t)lane;
        Rec r{};
        if (j < s.nent) r = load<Rec>(recs + sizeof(Rec) * (uint64_t)j);
        uint64_t sum;
        const uint32_t run = carry + (uint32_t)wave_excl_scan64(r.nl + r.vl, lane, sum);
        carry += (uint32_t)sum;
        if (j < s.nent) entry_store(L, slab, sbase, entry_slot(L, s, 0u, j), r, run);
    }
    for (uint32_t i = (uint32_t)lane; i < s.nlist; i += 64) put16(slab + L.list_off + 16ull * i, list + 16ull * i);
    // the run with its pad: ring 0 / the string area holds str_cap bytes, a multiple of 16
    for (uint64_t i = (uint64_t)lane; i < up16(s.str_bytes) / 16u; i += 64) put16(slab + L.str_off + 16 * i, str + 16 * i);
}
}  // namespace

hipError_t launch_conn_export(const hhuff_conn_family_t& fam, const uint8_t* scratch, uint32_t nslots, const uint32_t* slot,
                              uint32_t n, uint8_t* image, const uint64_t* img_off, uint32_t* img_len, int32_t* status,
                              hipStream_t stream) {
    ImgArgs A{fam, {}, const_cast<uint8_t*>(scratch), nslots, n, slot, nullptr, image, img_off, img_len, status};
    if (!layout(fam, A.L)) return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)(((uint64_t)n * 64u + 255u) / 256u);
    hipLaunchKernelGGL(img_export_kernel, dim3(grid), dim3(256), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_conn_import(const hhuff_conn_family_t& fam, uint8_t* scratch, uint32_t nslots, const uint32_t* slot,
                              uint32_t n, const uint8_t* image, const uint64_t* img_off, const uint32_t* img_len,
                              int32_t* status, hipStream_t stream) {
    ImgArgs A{fam, {}, scratch, nslots, n, slot, nullptr, const_cast<uint8_t*>(image), img_off, const_cast<uint32_t*>(img_len),
              status};
    if (!layout(fam, A.L)) return hipErrorInvalidValue;
    const hhuff_conn_slots_t slots{slot, nullptr, nslots};  // (2h) point 3: the lowest item that names a slot owns it
    uint32_t* cmap = nullptr;
    hipError_t e = conn_map_make(&slots, n, stream, &cmap);
    if (e != hipSuccess) return e;
    A.cmap = cmap;
    const uint32_t grid = (uint32_t)(((uint64_t)n * 64u + 255u) / 256u);
    hipLaunchKernelGGL(img_import_kernel, dim3(grid), dim3(256), 0, stream, A);
    e = hipGetLastError();
    const hipError_t f = hipFreeAsync(cmap, stream);
    return e != hipSuccess ? e : f;
}
}  // namespace hhuff
