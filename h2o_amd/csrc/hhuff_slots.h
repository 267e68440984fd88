// Connection slots (include/hhuff.h hhuff_conn_slots_t): which scratch slab each connection of a stateful
// call uses, and whether it starts fresh there.  The four families (hhuff_blocks.hip, hhuff_qpack.hip,
// hhuff_hpenc.hip, hhuff_qpenc.hip) share one small pass (hhuff_slots.hip) that settles ownership once per call
// and leaves one word per connection; every kernel that forms a slab address reads that word through
// conn_slot() before it touches scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff.h"

namespace hhuff {
// cmap[c] of the call's connection c: its slot (below 2^31), kConnReset or'ed in when HHUFF_CONN_RESET is set; or
// kConnRefused -- a slot >= nslots, a slot a lower-numbered connection names too, or an unknown flag bit.
constexpr uint32_t kConnReset = 0x80000000u, kConnRefused = 0xFFFFFFFFu;
constexpr uint32_t kConnMaxSlots = 0x7FFFFFFFu;

struct ConnSlot {
    uint64_t slot;  // meaningless when refused: form no address from it
    bool refused, reset;
};
// Every kernel that calls this has two instantiations and its launcher picks by cmap != NULL.  SLOTS = false (a
// call without slots): connection c in slot c, as it continues or not by the call's flag alone -- constants, so
// the kernel's code is what it was before there were slots and the dense path costs what it did.
__device__ __forceinline__ ConnSlot conn_slot_of(uint32_t m) {  // a map word
    const bool refused = m == kConnRefused;
    return ConnSlot{refused ? 0ull : (uint64_t)(m & ~kConnReset), refused, !refused && (m & kConnReset) != 0};
}
template <bool SLOTS>
__device__ __forceinline__ ConnSlot conn_slot(const uint32_t* __restrict__ cmap, uint64_t c) {
    if (!SLOTS) return ConnSlot{c, false, false};
    return conn_slot_of(cmap[c]);
}

// Rule 4 of the contract, on the host: 0, or the text of the refusal.  slab = the family's bytes per slot.
const char* conn_slots_check(const hhuff_conn_slots_t* slots, uint32_t nconn, uint64_t scratch_size, uint64_t slab);
// The map of a call: *cmap = NULL when slots is NULL or names neither slots nor flags (nothing is launched), else
// device u32[nconn] from the stream-ordered pool, filled on `stream`; release it with hipFreeAsync there.
hipError_t conn_map_make(const hhuff_conn_slots_t* slots, uint32_t nconn, hipStream_t stream, uint32_t** cmap);
}  // namespace hhuff
