// Connection slots: the ownership pass the four stateful families share (hhuff_slots.h).
//   conn_own_kernel  one lane per connection: owner[slot[c]] = min(owner[slot[c]], c) for slots in range, so a
//                    slot belongs to the lowest-numbered connection that names it;
//   conn_map_kernel  one lane per connection: cmap[c] = its slot and reset bit when the slot is in range, c owns
//                    it and its flags are known; kConnRefused otherwise.
// Without a slot array (slot c = c) nobody shares a slot and the first pass is not launched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hhuff_launch.h"
#include "hhuff_slots.h"

namespace hhuff {
namespace {
constexpr uint32_t kSlotThreads = 256;

__global__ __launch_bounds__(kSlotThreads) void conn_own_kernel(const uint32_t* __restrict__ slot, uint32_t nconn,
                                                               uint32_t nslots, uint32_t* __restrict__ owner) {
    for (uint64_t c = (uint64_t)blockIdx.x * kSlotThreads + threadIdx.x; c < nconn; c += (uint64_t)gridDim.x * kSlotThreads) {
        const uint32_t s = slot[c];
        if (s < nslots) atomicMin(owner + s, (uint32_t)c);
    }
}

__global__ __launch_bounds__(kSlotThreads) void conn_map_kernel(const uint32_t* __restrict__ slot,
                                                               const uint8_t* __restrict__ flags, uint32_t nconn,
                                                               uint32_t nslots, const uint32_t* __restrict__ owner,
                                                               uint32_t* __restrict__ cmap) {
    for (uint64_t c = (uint64_t)blockIdx.x * kSlotThreads + threadIdx.x; c < nconn; c += (uint64_t)gridDim.x * kSlotThreads) {
        const uint32_t s = slot ? slot[c] : (uint32_t)c;
        const uint32_t f = flags ? flags[c] : 0u;
        bool ok = s < nslots && (f & ~HHUFF_CONN_RESET) == 0;
        if (ok && slot) ok = owner[s] == (uint32_t)c;  // (read only for a slot in range)
        cmap[c] = ok ? s | ((f & HHUFF_CONN_RESET) ? kConnReset : 0u) : kConnRefused;
    }
}
}  // namespace

const char* conn_slots_check(const hhuff_conn_slots_t* slots, uint32_t nconn, uint64_t scratch_size, uint64_t slab) {
    if (!slots) return nullptr;
    if (slots->nslots == 0) return "slots: nslots is 0";
    if (slots->nslots > kConnMaxSlots) return "slots: nslots above 2^31 - 1";
    if (slab != 0 && scratch_size / slab < slots->nslots) return "scratch smaller than nslots slabs";
    if (!slots->slot && nconn > slots->nslots) return "slots: nconn above nslots without a slot array";
    return nullptr;
}

hipError_t conn_map_make(const hhuff_conn_slots_t* slots, uint32_t nconn, hipStream_t stream, uint32_t** cmap) {
    *cmap = nullptr;
    if (!slots || nconn == 0 || (!slots->slot && !slots->flags)) return hipSuccess;
    const uint64_t map_bytes = ((uint64_t)nconn * 4u + 15u) & ~15ull;
    const uint64_t own_bytes = slots->slot ? (uint64_t)slots->nslots * 4u : 0u;
    uint8_t* ws = nullptr;
    hipError_t e = work_alloc((void**)&ws, map_bytes + own_bytes, stream);
    if (e != hipSuccess) return e;
    uint32_t* owner = reinterpret_cast<uint32_t*>(ws + map_bytes);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)nconn + kSlotThreads - 1) / kSlotThreads, 4096);
    if (slots->slot) {
        e = hipMemsetAsync(owner, 0xFF, own_bytes, stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(conn_own_kernel, dim3(grid), dim3(kSlotThreads), 0, stream, slots->slot, nconn, slots->nslots,
                               owner);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(conn_map_kernel, dim3(grid), dim3(kSlotThreads), 0, stream, slots->slot, slots->flags, nconn,
                           slots->nslots, owner, reinterpret_cast<uint32_t*>(ws));
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        (void)hipFreeAsync(ws, stream);
        return e;
    }
    *cmap = reinterpret_cast<uint32_t*>(ws);
    return hipSuccess;
}
}  // namespace hhuff
