// hhuff header-literal kernels for gfx950 (MI355X) and their launchers: the string literals of HPACK and QPACK
// header blocks, parsed, decoded by the batch decode kernels (hhuff_kernels.hip) and fixed up.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hhuff_device.h"
#include "hhuff_devtables.h"
#include "hhuff_int.h"
#include "hhuff_launch.h"

namespace hhuff {

// ------------------------------------------------------------------------------------------------
// String literals in header blocks: HPACK decode_string (hpack.c:223-261) and QPACK
// decode_header_{name,value}_literal (qpack.c:559-629).  Literal i starts at in[lit_off[i]]: the H flag
// at bit prefix_bits of that byte, the length as a prefix integer (h2o_hpack_decode_int, hpack.c:52-83),
// then the payload, all before in[lit_end[i]].  Three launches: parse the headers (payload offset and
// Huffman length per literal), the Huffman decode kernel over (payload, length) pairs, then a fix-up
// that validates and copies the raw literals (h2o_hpack_validate_header_name / _value, hpack.c:163-221)
// and folds the header verdicts into out_len / status.
// ------------------------------------------------------------------------------------------------
struct LitArgs {
    const uint8_t* in;
    uint64_t in_size;
    const uint32_t* lit_off;
    const uint32_t* lit_end;
    uint32_t n;
    uint32_t prefix_bits;
    uint32_t flags;
    const uint32_t* is_name_bits;
    uint8_t* out;
    uint32_t* out_len;
    uint32_t* pay_off;
    uint32_t* consumed;
    uint8_t* status;
    uint32_t* huff_len;  // workspace: Huffman payload length (0 for raw literals and errors)
    uint8_t* code;       // workspace: verdict | H flag << 3 | soft bits << 4
    const uint32_t* n_dev;  // NULL, or the literal count in device memory (n is then an upper bound)
    uint32_t* long_list;    // NULL, or: raw payloads longer than kLongRaw are validated by literal_long_kernel
    uint32_t* long_count;
    const uint8_t* prefix_of;  // NULL, or each literal's own prefix_bits
};

constexpr uint32_t kLongRaw = 512;  // raw payload bytes above which one wave validates the literal

enum : uint32_t { kLitIncomplete = 1, kLitBadInt = 2, kLitTruncated = 3, kLitHuffman = 4, kLitUpper = 5, kLitTooLong = 6 };

// header of literal i -> verdict (0 = ok); hdr = header bytes, len = payload bytes, huff = H flag
__device__ __forceinline__ uint32_t lit_header(const LitArgs& A, uint32_t i, bool& huff, uint32_t& hdr, uint32_t& len) {
    const uint64_t off = A.lit_off[i];
    const uint64_t end = A.lit_end ? min((uint64_t)A.lit_end[i], A.in_size) : A.in_size;
    huff = false;
    hdr = 0;
    len = 0;
    if (off >= end) return kLitIncomplete;
    const uint32_t p = A.prefix_of ? A.prefix_of[i] : A.prefix_bits;
    const uint32_t b0 = A.in[off];
    huff = ((b0 >> p) & 1u) != 0;
    uint64_t q = off;
    const int64_t n = hpack_int(A.in, q, end, p);
    if (n < 0) return n == kIntIncomplete ? kLitIncomplete : kLitBadInt;
    const uint64_t v = (uint64_t)n;
    if (v > end - q) return kLitTruncated;
    if (v > kMaxStrLen) return kLitTooLong;
    hdr = (uint32_t)(q - off);
    len = (uint32_t)v;
    return 0;
}

// Pass 1: headers; raw payloads are validated and copied here (they skip the Huffman kernel, which
// sees length 0 for them).  code[i] = verdict | H flag << 3 | soft bits << 4 for the fix-up.
__global__ void literal_parse_kernel(LitArgs A) {
    const uint64_t n = A.n_dev ? (uint64_t)*A.n_dev : (uint64_t)A.n;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        bool huff;
        uint32_t hdr, len;
        uint32_t v = lit_header(A, (uint32_t)i, huff, hdr, len);
        uint32_t soft = 0;
        if (v == 0 && !huff && A.long_list && len > kLongRaw) {  // one lane would walk it alone: defer
            A.long_list[atomicAdd(A.long_count, 1u)] = (uint32_t)i;
        } else if (v == 0 && !huff) {
            const bool is_name = A.is_name_bits ? ((A.is_name_bits[i >> 5] >> (i & 31)) & 1u) != 0 : false;
            const uint64_t s0 = (uint64_t)A.lit_off[i] + hdr;
            const uint8_t* src = A.in + s0;
            const bool skip = is_name && ((A.flags & 1u) ? pseudo_token(src, len) : (len != 0 && src[0] == ':'));
            const uint32_t* inval = is_name ? g_name_invalid : g_value_invalid;
            uint8_t* dst = A.out + (s0 * 8u) / 5u;
            // 16-byte aligned loads, four per round and no early exit: the loads of a long raw literal stay
            // in flight together (and the blocks pipeline, kLitNoRawCopy, stores nothing in between)
            const bool copy = !(A.flags & kLitNoRawCopy);
            bool anybad = false, softbad = false, upper = false;
            const uint64_t a0 = s0 & ~15ull, e0 = s0 + len;
            for (uint64_t ar = a0; ar < e0; ar += 64) {
                uint4 w4[4];
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q) {
                    const uint64_t a = ar + 16u * q;
                    if (a + 16 <= A.in_size) {
                        w4[q] = *reinterpret_cast<const uint4*>(A.in + a);
                    } else {
                        uint32_t w[4] = {0, 0, 0, 0};
                        for (uint32_t k = 0; k < 16; ++k)
                            if (a + k < A.in_size) w[k >> 2] |= (uint32_t)A.in[a + k] << (8 * (k & 3));
                        w4[q] = make_uint4(w[0], w[1], w[2], w[3]);
                    }
                }
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q) {
                    const uint32_t wv[4] = {w4[q].x, w4[q].y, w4[q].z, w4[q].w};
#pragma unroll
                    for (uint32_t k = 0; k < 16; ++k) {
                        const uint64_t pos = ar + 16u * q + k;
                        if (pos < s0 || pos >= e0) continue;
                        const uint32_t c = (wv[k >> 2] >> (8 * (k & 3))) & 0xFFu;
                        const bool bad = ((inval[c >> 5] >> (c & 31)) & 1u) != 0;
                        const bool up = bad && (c - 'A' < 26u);
                        anybad |= bad;
                        softbad |= bad && !up && !upper;  // names: only what precedes the first upper-case letter
                        upper |= up;
                        if (copy) dst[pos - s0] = (uint8_t)c;
                    }
                }
            }
            if (is_name) {
                if (!skip) {  // h2o_hpack_validate_header_name: empty -> soft; upper case -> hard error
                    soft = (len == 0 || softbad) ? 0x1 : 0u;
                    if (upper) v = kLitUpper;
                }
            } else {  // h2o_hpack_validate_header_value, with the whitespace rule (hpack.c:110-115)
                const bool ws = len != 0 && (src[0] == ' ' || src[0] == '\t' || src[len - 1] == ' ' || src[len - 1] == '\t');
                soft = (anybad || ws) ? 0x2 : 0u;
            }
        }
        A.pay_off[i] = A.lit_off[i] + hdr;
        A.huff_len[i] = (v == 0 && huff) ? len : 0u;
        A.consumed[i] = v == 0 ? hdr + len : 0u;
        A.code[i] = (uint8_t)(v | (huff ? 8u : 0u) | (soft << 4));
    }
}

// Long raw payloads (deferred by literal_parse_kernel): one wave per literal, 16 bytes per lane per round.  The
// name rule needs the first upper-case letter's position (h2o_hpack_validate_header_name stops there, soft
// errors count only before it), so lanes keep the first position of each kind and the wave takes minima.
__global__ __launch_bounds__(256) void literal_long_kernel(LitArgs A) {
    const int lane = threadIdx.x & 63;
    const uint32_t nl = *A.long_count;
    const bool copy = !(A.flags & kLitNoRawCopy);
    for (uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6); w < nl; w += gridDim.x * 4u) {
        const uint32_t i = A.long_list[w];
        bool huff;
        uint32_t hdr, len;
        (void)lit_header(A, i, huff, hdr, len);  // verdict 0, raw: checked by the parse kernel
        const bool is_name = A.is_name_bits ? ((A.is_name_bits[i >> 5] >> (i & 31)) & 1u) != 0 : false;
        const uint64_t s0 = (uint64_t)A.lit_off[i] + hdr, e0 = s0 + len;
        const uint8_t* src = A.in + s0;
        const bool skip = is_name && ((A.flags & 1u) ? pseudo_token(src, len) : (len != 0 && src[0] == ':'));
        const uint32_t* inval = is_name ? g_name_invalid : g_value_invalid;
        uint8_t* dst = A.out + (s0 * 8u) / 5u;
        uint32_t first_up = 0xFFFFFFFFu, first_soft = 0xFFFFFFFFu, anybad = 0;
        for (uint64_t a = s0 + 16u * (uint32_t)lane; a < e0; a += 1024) {
            uint8_t v[16];
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) v[k] = a + k < e0 ? A.in[a + k] : 0u;
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) {
                if (a + k >= e0) break;
                const uint32_t c = v[k];
                const bool bad = ((inval[c >> 5] >> (c & 31)) & 1u) != 0;
                const bool up = bad && (c - 'A' < 26u);
                const uint32_t pos = (uint32_t)(a + k - s0);
                anybad |= bad ? 1u : 0u;
                if (up) first_up = min(first_up, pos);
                if (bad && !up) first_soft = min(first_soft, pos);
                if (copy) dst[pos] = (uint8_t)c;
            }
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            first_up = min(first_up, (uint32_t)__shfl_xor((int)first_up, d));
            first_soft = min(first_soft, (uint32_t)__shfl_xor((int)first_soft, d));
            anybad |= (uint32_t)__shfl_xor((int)anybad, d);
        }
        if (lane == 0) {
            uint32_t v = 0, soft = 0;
            if (is_name) {
                if (!skip) {  // h2o_hpack_validate_header_name: empty -> soft; upper case -> hard error
                    soft = first_soft < first_up ? 0x1u : 0u;
                    if (first_up != 0xFFFFFFFFu) v = kLitUpper;
                }
            } else {  // h2o_hpack_validate_header_value, with the whitespace rule (hpack.c:110-115)
                const bool ws = src[0] == ' ' || src[0] == '\t' || src[len - 1] == ' ' || src[len - 1] == '\t';
                soft = (anybad || ws) ? 0x2u : 0u;
            }
            A.consumed[i] = v == 0 ? hdr + len : 0u;
            A.code[i] = (uint8_t)(v | (soft << 4));
        }
    }
}

// Pass 3: fold the header / raw verdicts into out_len and status (the Huffman kernel ran in between).
__global__ void literal_fix_kernel(LitArgs A) {
    const uint64_t n = A.n_dev ? (uint64_t)*A.n_dev : (uint64_t)A.n;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t c = A.code[i];
        const uint32_t v = c & 7u, soft = c >> 4;
        if (v) {
            A.out_len[i] = kFailLen;
            A.status[i] = (uint8_t)(soft | kStatusFail | (v << 2));
        } else if (!(c & 8u)) {
            A.out_len[i] = A.consumed[i] - (A.pay_off[i] - A.lit_off[i]);
            A.status[i] = (uint8_t)soft;
        } else if (A.status[i] & kStatusFail) {  // h2o_hpack_decode_huffman returned SIZE_MAX
            A.status[i] = (uint8_t)(kStatusFail | (kLitHuffman << 2));
            A.consumed[i] = 0;
        }
    }
}

hipError_t launch_literals(const uint8_t* in, uint64_t in_size, const uint32_t* lit_off, const uint32_t* lit_end, uint32_t n,
                           uint32_t prefix_bits, uint32_t flags, const uint32_t* is_name_bits, uint8_t* out,
                           uint32_t* out_len, uint32_t* pay_off, uint32_t* consumed, uint8_t* status, uint32_t* huff_len,
                           hipStream_t stream) {
    if (n == 0) return hipSuccess;
    LitArgs A{in, in_size, lit_off, lit_end, n, prefix_bits, flags, is_name_bits, out, out_len, pay_off, consumed, status,
              huff_len, reinterpret_cast<uint8_t*>(huff_len + n), nullptr, nullptr, nullptr, nullptr};
    const uint32_t blocks = min((n + 255u) / 256u, 4096u);
    hipLaunchKernelGGL(literal_parse_kernel, dim3(blocks), dim3(256), 0, stream, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_decode(in, in_size, pay_off, huff_len, n, is_name_bits, out, nullptr, out_len, status, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(literal_fix_kernel, dim3(blocks), dim3(256), 0, stream, A);
    return hipGetLastError();
}

// Literals whose count is only known on the device (the header-block pipeline, hhuff_blocks.hip): n_max
// bounds the arrays, *n_dev is the count.  Huffman payloads go through the staged short-string kernel, which
// reads the count from *n_dev (launch_decode_short_dev).  ws: literals_dev_ws(n_max, in_size) bytes.
hipError_t launch_literals_dev(const uint8_t* in, uint64_t in_size, const uint32_t* lit_off, uint32_t n_max,
                               const uint32_t* n_dev, uint32_t prefix_bits, uint32_t flags, const uint32_t* is_name_bits,
                               uint8_t* out, uint32_t* out_len, uint32_t* pay_off, uint32_t* consumed, uint8_t* status,
                               uint8_t* ws, hipStream_t stream, const uint8_t* prefix_of) {
    if (n_max == 0) return hipSuccess;
    // ws: huff_len u32[n_max], code u8[n_max], then (8-aligned) 8 unused bytes (once a stream-kernel work counter;
    // kept because hhuff_decwork.h and the block decoders size their buffers from this layout), the long-literal
    // count u32 (+ pad) and list u32[in_size / kLongRaw + 1]
    uint32_t* huff_len = reinterpret_cast<uint32_t*>(ws);
    uint8_t* tail = ws + 5ull * n_max + ((8 - (5ull * n_max) % 8) % 8);
    uint32_t* long_count = reinterpret_cast<uint32_t*>(tail + 8);
    uint32_t* long_list = reinterpret_cast<uint32_t*>(tail + 16);
    LitArgs A{in, in_size, lit_off, nullptr, n_max, prefix_bits, flags, is_name_bits, out, out_len, pay_off, consumed,
              status, huff_len, reinterpret_cast<uint8_t*>(huff_len + n_max), n_dev, long_list, long_count, prefix_of};
    const uint32_t blocks = min((n_max + 255u) / 256u, 8192u);
    hipError_t e = hipMemsetAsync(tail, 0, 16, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(literal_parse_kernel, dim3(blocks), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(literal_long_kernel, dim3(1024), dim3(256), 0, stream, A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // header literals are short: the staged kernel (tiles of 64 consecutive literals, their span staged in
    // LDS; a tile whose span exceeds the stage decodes lane by lane from global memory).  Measured against
    // the stream kernel on the f4 benches: blocks 1.685 -> 1.485 ms, qpack 1.25 -> 1.08 ms.
    e = launch_decode_short_dev(in, in_size, pay_off, huff_len, n_max, n_dev, is_name_bits, out, out_len, status, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(literal_fix_kernel, dim3(blocks), dim3(256), 0, stream, A);
    return hipGetLastError();
}

uint64_t literals_dev_ws(uint32_t n_max, uint64_t in_size) { return 5ull * n_max + 8 + 16 + 4 * (in_size / kLongRaw + 1); }

}  // namespace hhuff
