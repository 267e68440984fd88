// A buffer cut into aligned pieces by one sequence of take<T>(count) calls.  Run on a null base the sequence
// yields the size in `off` (the pointers mean nothing), run again on the allocation it yields the pointers:
// no size is written twice.  Pieces are `align` bytes aligned (a power of two) when the base is.
#pragma once
#include <stdint.h>

namespace hhuff {
struct Carve {
    uint8_t* base;
    uint64_t off = 0;
    uint64_t align = 16;
    template <class T>
    T* take(uint64_t count) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (count * sizeof(T) + align - 1) & ~(align - 1);
        return p;
    }
};
}  // namespace hhuff
