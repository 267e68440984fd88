// The 16-byte line copy of every device copy (the de-framers' gather, the HTTP/2 and HTTP/3 body and DATA-frame calls)
// and the clamp of an untrusted range, for the device and the host: the kernels and the host programs
// (tools/linecopy_host.cpp and the calls' own) run this very code.
// A copy cuts its destination at 16-byte lines by address.  A line's bytes come from the five aligned source dwords
// that hold them, funnel-shifted; a whole line is one 16-byte store, a job's first and last line, which it shares with
// its neighbours, dword and byte stores of its own bytes.
//   clamp_range   [a, b) cut to [0, cap): whatever an offset array holds, what it names stays inside its buffer
//   lines_of      the lines that n >= 1 bytes at an address touch
//   load16, store16, store_part, mask32   a line's dwords in registers, and their way to memory
//   copy_line     line li of a job without structure inside: source bytes to [d0, d1)
#ifndef HHUFF_LINECOPY_H
#define HHUFF_LINECOPY_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HHUFF_LC_HD __host__ __device__ __forceinline__
#else
#define HHUFF_LC_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define HHUFF_LC_UNROLL _Pragma("unroll")
#else
#define HHUFF_LC_UNROLL
#endif

namespace hhuff {
namespace lc {

// first = min(a, cap), count = min(max(b, first), cap) - first: b < a is an empty range at first, and first + count
// never passes cap.  Slots, records, bytes and output regions alike.
struct Range {
    uint32_t first, count;
};
HHUFF_LC_HD Range clamp_range(uint32_t a, uint32_t b, uint32_t cap) {
    const uint32_t first = a < cap ? a : cap;
    return Range{first, (b < first ? first : (b < cap ? b : cap)) - first};
}

HHUFF_LC_HD uint32_t lines_of(uint64_t addr, uint64_t n) { return (uint32_t)(((addr + n + 15u) >> 4) - (addr >> 4)); }  // n >= 1

HHUFF_LC_HD uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t bits) {  // bits 0, 8, 16, 24
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, bits);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> bits);
#endif
}

// The line's 16 bytes from the aligned source dwords that hold them: sv = where byte 0 of the line comes from (in front
// of the job's source when lo > 0: no such byte is loaded), dword q = the line's bytes 4 q - r .. 4 q - r + 3, loaded
// only when one of them lies in [lo, hi).
HHUFF_LC_HD void load16(uint64_t sv, int lo, int hi, uint32_t v[4]) {
    const uint32_t r = (uint32_t)(sv & 3u);
    const uint32_t* a = reinterpret_cast<const uint32_t*>((uintptr_t)(sv - r));
    uint32_t w[5];
    HHUFF_LC_UNROLL
    for (int q = 0; q < 5; ++q) {
        const int first = 4 * q - (int)r;
        w[q] = (first < hi && first + 4 > lo) ? a[q] : 0u;
    }
    HHUFF_LC_UNROLL
    for (int q = 0; q < 4; ++q) v[q] = funnel(w[q + 1], w[q], 8u * r);
}

HHUFF_LC_HD void store16(uint8_t* d, const uint32_t v[4]) {  // d: 16-byte aligned
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint4*>(d) = make_uint4(v[0], v[1], v[2], v[3]);
#else
    uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
    d4[0] = v[0], d4[1] = v[1], d4[2] = v[2], d4[3] = v[3];
#endif
}

// Bytes [b0, b1) of the line at d, and no other: whole dwords where the job has them, else bytes -- the rest of a
// job's first and last line is its neighbours'.
HHUFF_LC_HD void store_part(uint8_t* d, const uint32_t v[4], int b0, int b1) {
    HHUFF_LC_UNROLL
    for (int q = 0; q < 4; ++q) {
        if (b0 <= 4 * q && 4 * q + 4 <= b1) {
            reinterpret_cast<uint32_t*>(d)[q] = v[q];
        } else {
            HHUFF_LC_UNROLL
            for (int i = 0; i < 4; ++i)
                if (4 * q + i >= b0 && 4 * q + i < b1) d[4 * q + i] = (uint8_t)(v[q] >> (8 * i));
        }
    }
}

HHUFF_LC_HD uint32_t mask32(int q, int lo, int hi) {  // the bytes of dword q of a line that lie in [lo, hi)
    const int a = lo - 4 * q < 0 ? 0 : lo - 4 * q, b = hi - 4 * q > 4 ? 4 : hi - 4 * q;
    if (b <= a) return 0u;
    return (b == 4 ? 0xFFFFFFFFu : (1u << (8 * b)) - 1u) & ~((1u << (8 * a)) - 1u);
}

// Line li (< lines_of(d0, d1 - d0)) of the job that copies d1 - d0 bytes from address src_addr to the addresses
// [d0, d1): the job's bytes of the line, and no other.
HHUFF_LC_HD void copy_line(uint64_t src_addr, uint64_t d0, uint64_t d1, uint64_t li) {
    const uint64_t line = (d0 & ~15ull) + 16ull * li;
    const uint64_t lo = line > d0 ? line : d0, hi = line + 16u < d1 ? line + 16u : d1;
    const int b0 = (int)(lo - line), b1 = (int)(hi - line);  // the job's bytes of the line
    uint8_t* d = reinterpret_cast<uint8_t*>((uintptr_t)line);
    uint32_t v[4];
    load16(src_addr + (line - d0), b0, b1, v);  // (modulo 2^64 in the first line, which begins in front of the job)
    if (b1 - b0 == 16)
        store16(d, v);
    else
        store_part(d, v, b0, b1);
}

}  // namespace lc
}  // namespace hhuff
#endif
