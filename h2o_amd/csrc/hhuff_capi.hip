// hhuff C-ABI shim (include/hhuff.h), first of five units: the error string and the per-thread device context every
// unit shares (hhuff_host.h), the device batch entry points, the literal call, the info and tuning calls and the
// one kernel of the shim (the multi-device cut).  The header-block families are in hhuff_capi_blocks.hip, the
// per-string h2o symbols in hhuff_capi_string.hip, the host-array batch paths in hhuff_capi_host.hip and the
// multi-device call in hhuff_capi_multi.hip; those four hold host code only.  All compute goes through the HIP
// kernels (hhuff_kernels.hip the batch codec and the per-string calls, hhuff_literals.hip, the header-block units);
// there is no CPU codec in this library.
#include "hhuff_host.h"

using namespace hhuff;

thread_local char hhuff::t_err[256] = "";
thread_local Ctx hhuff::t_ctx;

// ---------------------------------------------------------------------------------------------------
// (2) device batch API
// ---------------------------------------------------------------------------------------------------
HHUFF_API int hhuff_decode_batch(const uint8_t* in, uint64_t in_size, const uint32_t* in_off, const uint32_t* in_len,
                                 uint32_t n, const uint32_t* is_name_bits, uint8_t* out, const uint32_t* out_off,
                                 uint32_t* out_len, uint8_t* status, void* stream) {
    int rc = check_batch(in, in_off, n, out, out_len);
    if (rc) return rc;
    if (n && !status) return arg_fail("NULL status");
    hipError_t e = hhuff::launch_decode(in, in_size, in_off, in_len, n, is_name_bits, out, out_off, out_len, status,
                                        (hipStream_t)stream);
    return hip_rc(e, "decode launch");
}

HHUFF_API int hhuff_encode_batch(const uint8_t* in, uint64_t in_size, const uint32_t* in_off, const uint32_t* in_len,
                                 uint32_t n, uint8_t* out, const uint32_t* out_off, uint32_t* out_len, uint8_t* status,
                                 void* stream) {
    int rc = check_batch(in, in_off, n, out, out_len);
    if (rc) return rc;
    hipError_t e = hhuff::launch_encode(in, in_size, in_off, in_len, n, out, out_off, out_len, status, (hipStream_t)stream);
    return hip_rc(e, "encode launch");
}

HHUFF_API int hhuff_decode_batch_packed(const uint8_t* in, uint64_t in_size, const uint32_t* in_off, uint32_t n,
                                        const uint32_t* is_name_bits, uint8_t* out, uint32_t* out_off, uint32_t* out_len,
                                        uint8_t* status, void* stream) {
    if (!out_off) return arg_fail("NULL out_off");
    int rc = check_batch(in, in_off, n, out, out_len);
    if (rc) return rc;
    if (n && !status) return arg_fail("NULL status");
    if ((in_size * 8) / 5 >= 0xFFFFFFFFull) return arg_fail("in_size too large for u32 packed offsets");
    hipError_t e = hhuff::launch_decode_packed(in, in_size, in_off, n, is_name_bits, out, out_off, out_len, status,
                                               (hipStream_t)stream);
    return hip_rc(e, "packed decode launch");
}

HHUFF_API int hhuff_encode_batch_packed(const uint8_t* in, uint64_t in_size, const uint32_t* in_off, uint32_t n,
                                        uint8_t* out, uint32_t* out_off, uint32_t* out_len, uint8_t* status, void* stream) {
    if (!out_off) return arg_fail("NULL out_off");
    int rc = check_batch(in, in_off, n, out, out_len);
    if (rc) return rc;
    if (in_size >= 0xFFFFFFFFull) return arg_fail("in_size too large for u32 packed offsets");
    hipError_t e = hhuff::launch_encode_packed(in, in_size, in_off, n, out, out_off, out_len, status, (hipStream_t)stream);
    return hip_rc(e, "packed encode launch");
}

HHUFF_API int hhuff_flatten_batch(const uint8_t* in, uint64_t in_size, const uint32_t* in_off, const uint32_t* in_len,
                                  uint32_t n, const uint8_t* first_bytes, unsigned prefix_bits, const uint32_t* raw_bits,
                                  uint8_t* out, const uint32_t* out_off, uint32_t* out_len, void* stream) {
    int rc = check_batch(in, in_off, n, out, out_len);
    if (rc) return rc;
    if (prefix_bits < 1 || prefix_bits > 7) return arg_fail("prefix_bits must be in 1..7");
    hipError_t e = hhuff::launch_flatten(in, in_size, in_off, in_len, n, first_bytes, prefix_bits, raw_bits, out, out_off,
                                         out_len, (hipStream_t)stream);
    return hip_rc(e, "flatten launch");
}

HHUFF_API int hhuff_decode_literals(const uint8_t* in, uint64_t in_size, const uint32_t* lit_off, const uint32_t* lit_end,
                                    uint32_t n, unsigned prefix_bits, unsigned flags, const uint32_t* is_name_bits,
                                    uint8_t* out, uint32_t* out_len, uint32_t* pay_off, uint32_t* consumed,
                                    uint8_t* status, void* stream) {
    int rc = check_batch(in, lit_off, n, out, out_len);
    if (rc) return rc;
    if (n && (!lit_end || !pay_off || !consumed || !status)) return arg_fail("NULL array");
    if (prefix_bits < 1 || prefix_bits > 7) return arg_fail("prefix_bits must be in 1..7");
    if (n == 0) return HHUFF_OK;
    hipStream_t s = (hipStream_t)stream;
    void* ws = nullptr;  // Huffman payload lengths + per-literal verdict bytes, stream-ordered scratch
    HIP_TRY(hipMallocAsync(&ws, (size_t)n * 5, s), "hipMallocAsync");
    hipError_t e = hhuff::launch_literals(in, in_size, lit_off, lit_end, n, prefix_bits, flags & HHUFF_LIT_QPACK, is_name_bits, out, out_len,
                                          pay_off, consumed, status, (uint32_t*)ws, s);
    hipError_t f = hipFreeAsync(ws, s);
    if (e != hipSuccess) return hip_fail(e, "literal launch");
    return hip_rc(f, "hipFreeAsync");
}

// ---------------------------------------------------------------------------------------------------
// (3d) the cut of a device-resident multi-device batch (hhuff_capi_multi.hip multi_device).  The kernel lives in
// this unit so that the other four carry no code object.
// ---------------------------------------------------------------------------------------------------
namespace {
// the cut and the byte offsets at the cut, into mapped host memory (b[0 .. ns], then in_off[b[k]] at b[ns + 1 + k])
__global__ void shard_bounds_kernel(const uint32_t* in_off, uint32_t n, uint32_t ns, uint32_t align, uint32_t* b) {
    const uint32_t k = threadIdx.x;
    if (k <= ns) {
        const uint32_t i = shard_bound(in_off, n, k, ns, align);
        b[k] = i;
        b[ns + 1 + k] = in_off[i];
    }
}
}  // namespace

hipError_t hhuff::launch_shard_bounds(const uint32_t* in_off, uint32_t n, uint32_t ns, uint32_t* b, hipStream_t stream) {
    hipLaunchKernelGGL(shard_bounds_kernel, dim3(1), dim3(kMaxDev + 1), 0, stream, in_off, n, ns, kShardAlign, b);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// (4) info
// ---------------------------------------------------------------------------------------------------
#ifdef HHUFF_PROFILE  // profile builds: per-phase cycle sums of the staged kernels (tools/ab.py prof)
namespace hhuff {
hipError_t read_prof(unsigned long long* out16, bool reset);
}
HHUFF_API int hhuff_debug_prof(unsigned long long* out16, int reset) {
    return hhuff::read_prof(out16, reset != 0) == hipSuccess ? 0 : -1;
}
#endif
HHUFF_API const char* hhuff_version(void) { return "hhuff 0.1.0 (gfx950)"; }
HHUFF_API const char* hhuff_last_error_string(void) { return t_err; }
HHUFF_API int hhuff_pool_trim(void) {
    // pool_trim synchronises the device (memory freed on any stream returns to the pool once that stream
    // passes the free), which would also wait for the resident per-string wave: it is stopped first, with
    // its lock held so no per-string call relaunches it meanwhile (the next call after the trim does)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hip_fail(hipErrorInvalidDevice, "pool trim");
    Service& S = g_svc[dev];
    std::lock_guard<std::mutex> g(S.mu);
    if (S.ready) svc_stop(S);
    return hip_rc(hhuff::pool_trim(), "pool trim");
}
HHUFF_API int hhuff_decode_prices(int device, float* out4) {
    if (!out4) return arg_fail("NULL out4");
    return hhuff::decode_prices_of(device, out4, 0) == 0 ? HHUFF_OK : hip_fail(hipErrorInvalidDevice, "hhuff_decode_prices");
}
HHUFF_API int hhuff_calibrate_decode_prices(int device, float* out4) {
    float tmp[4];
    return hhuff::decode_prices_of(device, out4 ? out4 : tmp, 1) == 0
               ? HHUFF_OK
               : hip_fail(hipErrorInvalidDevice, "hhuff_calibrate_decode_prices");
}
HHUFF_API int hhuff_set_decode_prices(int device, const float* in4) {
    const int r = hhuff::set_decode_prices(device, in4);
    if (r == -2) return arg_fail("decode prices must be finite and >= 0");
    return r == 0 ? HHUFF_OK : hip_fail(hipErrorInvalidDevice, "hhuff_set_decode_prices");
}

HHUFF_API int hhuff_set_decode_kernel(int mode) {
    const int r = hhuff::set_decode_kernel(mode);
    return r < 0 ? arg_fail("decode kernel mode must be 0, 1 or 2") : r;
}

HHUFF_API uint32_t hhuff_set_edge_defer_min(uint32_t n) { return hhuff::set_edge_defer_min(n); }

HHUFF_API int hhuff_debug_encode_blocks_per_cu(uint64_t in_size, uint32_t n) {
    return hhuff::debug_encode_blocks_per_cu(in_size, n);
}

HHUFF_API int hhuff_grid_size(int device, int which) {
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return -1;
    return hhuff::grid_size(device, which);
}
