// The Huffman tables in device memory, once for every unit: the decode window LUT and leading-ones tables, the
// raw-literal validity bitmaps and the encode code table (all generated: hhuff_tables.h), and the loader of the
// decode tables into a workgroup's LDS.  Const at namespace scope, so with internal linkage: one copy per unit of
// what that unit uses, as hhuff_enc.h explains for the encoders.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff_tables.h"

namespace hhuff {

__device__ const uint32_t g_dec_lut[1u << HHUFF_LUT_BITS] = HHUFF_DEC_LUT_INIT;
__device__ const uint32_t g_name_invalid[8] = HHUFF_NAME_INVALID_INIT;    // raw-literal validity bitmaps
__device__ const uint32_t g_value_invalid[8] = HHUFF_VALUE_INVALID_INIT;  // (hpack.c:171-180, 200-209)
__device__ const uint32_t g_kinfo[31] = HHUFF_ONES_KINFO_INIT;
__device__ const uint32_t g_ones[HHUFF_ONES_NENT] = HHUFF_ONES_ENT_INIT;
__device__ const uint32_t g_enc_code[256] = HHUFF_ENC_CODE_INIT;
__device__ const uint8_t g_enc_nbits[256] = HHUFF_ENC_NBITS_INIT;

// The decode tables into LDS by a workgroup of nthreads lanes (s_kinfo has 32 entries; the caller's barrier follows)
__device__ __forceinline__ void load_dec_tables(uint32_t* s_lut, uint32_t* s_kinfo, uint32_t* s_ones, int nthreads) {
    for (uint32_t k = threadIdx.x; k < (1u << HHUFF_LUT_BITS) / 4; k += nthreads)
        reinterpret_cast<uint4*>(s_lut)[k] = reinterpret_cast<const uint4*>(g_dec_lut)[k];
    for (uint32_t k = threadIdx.x; k < HHUFF_ONES_NENT; k += nthreads) s_ones[k] = g_ones[k];
    if (threadIdx.x < 31) s_kinfo[threadIdx.x] = g_kinfo[threadIdx.x];
}

}  // namespace hhuff
