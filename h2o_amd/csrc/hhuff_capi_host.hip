// hhuff C-ABI shim, the host-array batch entry points (include/hhuff.h (3), (3b), (3c)): one staged round trip
// (host_batch), the chunked pipeline (pipelined) and the packed layout (host_packed).  Their integer arithmetic --
// slots, cuts, the chunk layout, the packed runs -- is hhuff_hostplan.h's; host code only.
#include <stdlib.h>
#include <string.h>

#include <thread>

#include "hhuff_host.h"

using namespace hhuff;

// ---------------------------------------------------------------------------------------------------
// (3) host batch API: copy in, run, copy out (synchronous)
// ---------------------------------------------------------------------------------------------------
namespace {

using hhuff::Carve;  // the device buffer's pieces (hhuff_launch.h)

size_t in_off_count(const uint32_t* in_len, uint32_t n) { return in_len ? n : (size_t)n + 1; }

int host_batch(bool decode, const uint8_t* in, uint64_t in_size, const uint32_t* in_off, const uint32_t* in_len,
               uint32_t n, const uint32_t* is_name_bits, uint8_t* out, uint64_t out_size, const uint32_t* out_off,
               uint32_t* out_len, uint8_t* status, int device) {
    if (n == 0) return HHUFF_OK;
    if (null_array(decode, in, in_off, out, out_len, status)) return arg_fail("NULL array");
    if (!in_len && !out_off) {
        // (a short `out` used to size the device piece the kernels' slots are addressed in: they wrote past it)
        const int bad = check_implicit(decode, in_size, in_off[n], out_size);
        if (bad) return bad;
    }
    if (!in_len && !out_off && in_size >= 2 * kDefaultChunk)  // large contiguous batch
        return pipelined(decode, in, in_size, in_off, n, is_name_bits, out, out_size, out_len, status, device, 0);
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return hip_fail(guard.err, "hipSetDevice");
    Ctx& c = t_ctx;
    int rc = c.bind(device);
    if (rc) return rc;
    const size_t noff = in_off_count(in_len, n), nw = ((size_t)n + 31) / 32;
    size_t need = up16(in_size ? in_size : 1) + up16(noff * 4) + (in_len ? up16((size_t)n * 4) : 0) +
                  (is_name_bits ? up16(nw * 4) : 0) + (out_off ? up16((size_t)n * 4) : 0) + up16(out_size ? out_size : 1) +
                  up16((size_t)n * 4) + up16(n);
    rc = c.reserve(need, 0);
    if (rc) return rc;
    Carve cv{c.d};
    uint8_t* d_in = cv.take<uint8_t>(in_size ? in_size : 1);
    uint32_t* d_in_off = cv.take<uint32_t>(noff);
    uint32_t* d_in_len = in_len ? cv.take<uint32_t>(n) : nullptr;
    uint32_t* d_name = is_name_bits ? cv.take<uint32_t>(nw) : nullptr;
    uint32_t* d_out_off = out_off ? cv.take<uint32_t>(n) : nullptr;
    uint8_t* d_out = cv.take<uint8_t>(out_size ? out_size : 1);
    uint32_t* d_out_len = cv.take<uint32_t>(n);
    uint8_t* d_status = cv.take<uint8_t>(n);
    hipStream_t s = c.stream;
    HIP_TRY(hipMemcpyAsync(d_in, in, in_size, hipMemcpyHostToDevice, s), "H2D in");
    HIP_TRY(hipMemcpyAsync(d_in_off, in_off, noff * 4, hipMemcpyHostToDevice, s), "H2D in_off");
    if (in_len) HIP_TRY(hipMemcpyAsync(d_in_len, in_len, (size_t)n * 4, hipMemcpyHostToDevice, s), "H2D in_len");
    if (is_name_bits) HIP_TRY(hipMemcpyAsync(d_name, is_name_bits, nw * 4, hipMemcpyHostToDevice, s), "H2D is_name");
    if (out_off) HIP_TRY(hipMemcpyAsync(d_out_off, out_off, (size_t)n * 4, hipMemcpyHostToDevice, s), "H2D out_off");
    const hipError_t e = launch_slots(decode, d_in, in_size, d_in_off, d_in_len, n, d_name, d_out, d_out_off, d_out_len,
                                      status ? d_status : nullptr, s);
    if (e != hipSuccess) return hip_fail(e, decode ? "decode launch" : "encode launch");
    HIP_TRY(hipMemcpyAsync(out, d_out, out_size, hipMemcpyDeviceToHost, s), "D2H out");
    HIP_TRY(hipMemcpyAsync(out_len, d_out_len, (size_t)n * 4, hipMemcpyDeviceToHost, s), "D2H out_len");
    if (status) HIP_TRY(hipMemcpyAsync(status, d_status, n, hipMemcpyDeviceToHost, s), "D2H status");
    HIP_TRY(hipStreamSynchronize(s), "sync");
    return HHUFF_OK;
}

// ---------------------------------------------------------------------------------------------------
// (3b) pipelined host path: pageable -> pinned -> device -> pinned -> pageable, chunk by chunk
//
// The batch (contiguous layout, implicit output slots) is cut at multiples of 32 strings into chunks
// of about `chunk_bytes` input bytes.  Chunk k runs on stream k % depth: H2D of its input bytes,
// offsets and is-name words, the kernel, D2H of its output slots, lengths and statuses.  While the GPU
// works on chunks k-1 and k-2 the calling thread (plus helper threads) copies chunk k's input into its
// pinned slot and chunk k-depth's results out of theirs, so host copies, both DMA directions and the
// kernels overlap.  Caller buffers that are already pinned are used by the DMA engines directly.
// The kernel sees absolute offsets: `in` and `out` are passed shifted back by the chunk base (a
// multiple of 80 bytes, so the decode slot floor(8 base / 5) stays 16-byte aligned).
// ---------------------------------------------------------------------------------------------------
// memcpy split over a few threads for large copies (the host staging copies bound the host path)
void par_copy(void* dst, const void* src, size_t n) {
    const size_t kMin = 4u << 20;
    unsigned t = std::thread::hardware_concurrency();
    t = t == 0 ? 1 : (t > 8 ? 8 : t);
    if (n < kMin || t == 1) {
        memcpy(dst, src, n);
        return;
    }
    const size_t per = ((n / t) + 4095) & ~(size_t)4095;
    std::vector<std::thread> th;
    for (unsigned k = 1; k < t && k * per < n; ++k)
        th.emplace_back([=] { memcpy((uint8_t*)dst + k * per, (const uint8_t*)src + k * per, std::min(per, n - k * per)); });
    memcpy(dst, src, std::min(per, n));
    for (auto& x : th) x.join();
}

struct Slot {
    hipStream_t s = nullptr;
    uint8_t *d = nullptr, *h = nullptr;
    size_t dcap = 0, hcap = 0;
    bool busy = false;
    // chunk bookkeeping for the host-side unstaging
    uint64_t i0 = 0, m = 0, out_lo = 0, out_n = 0;
    size_t h_out = 0, h_len = 0, h_st = 0;
};

struct Pipe {
    int dev = -1;
    Slot slot[kDepth];
    ~Pipe() {
        for (auto& x : slot) {
            if (x.d) (void)hipFree(x.d);
            if (x.h) (void)hipHostFree(x.h);
            if (x.s) (void)hipStreamDestroy(x.s);
        }
    }
    int bind(int device) {
        if (dev == device) return HHUFF_OK;
        for (auto& x : slot) {
            if (x.d) (void)hipFree(x.d), x.d = nullptr, x.dcap = 0;
            if (x.s) (void)hipStreamDestroy(x.s), x.s = nullptr;
            HIP_TRY(hipStreamCreateWithFlags(&x.s, hipStreamNonBlocking), "hipStreamCreate");
        }
        dev = device;
        return HHUFF_OK;
    }
};
thread_local Pipe t_pipe;

int grow(Slot& x, size_t dneed, size_t hneed) {
    if (dneed > x.dcap) {
        if (x.d) (void)hipFree(x.d), x.d = nullptr, x.dcap = 0;
        HIP_TRY(hipMalloc(&x.d, dneed + dneed / 8), "hipMalloc");
        x.dcap = dneed + dneed / 8;
    }
    if (hneed > x.hcap) {
        if (x.h) (void)hipHostFree(x.h), x.h = nullptr, x.hcap = 0;
        HIP_TRY(hipHostMalloc(&x.h, hneed + hneed / 8, hipHostMallocDefault), "hipHostMalloc");
        x.hcap = hneed + hneed / 8;
    }
    return HHUFF_OK;
}

}  // namespace

int hhuff::pipelined(bool decode, const uint8_t* in, uint64_t in_size, const uint32_t* in_off, uint32_t n,
                     const uint32_t* is_name_bits, uint8_t* out, uint64_t out_size, uint32_t* out_len, uint8_t* status,
                     int device, uint64_t chunk_bytes) {
    (void)out_size;  // every caller has checked it against the slots' end (check_implicit)
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return hip_fail(guard.err, "hipSetDevice");
    Ctx& c = t_ctx;
    int rc = c.bind(device);
    if (rc) return rc;
    Pipe& P = t_pipe;
    // No way out leaves a slot busy.  A return on an error used to: the chunks in flight could still DMA into the
    // caller's pinned arrays after the call had returned, and the next call on the thread drained those slots --
    // bookkeeping that points into the failed call's arrays -- into its own out, out_len and status.  Their work is
    // waited for and forgotten, nothing is copied.  (After a call that succeeds every slot is drained: no-op.)
    struct Quiesce {
        Pipe& P;
        ~Quiesce() {
            for (auto& x : P.slot)
                if (x.busy) {
                    (void)hipStreamSynchronize(x.s);
                    x.busy = false;
                }
        }
    } quiesce{P};
    rc = P.bind(c.dev);
    if (rc) return rc;
    // each caller array's device address where it is pinned (device-visible); a pinned array is DMA'd in place
    const uint8_t* z_in = static_cast<const uint8_t*>(pinned_dev_ptr(in));
    const uint32_t* z_off = static_cast<const uint32_t*>(pinned_dev_ptr(in_off));
    const uint32_t* z_nm = static_cast<const uint32_t*>(pinned_dev_ptr(is_name_bits));
    uint8_t* z_out = static_cast<uint8_t*>(pinned_dev_ptr(out));
    uint32_t* z_len = static_cast<uint32_t*>(pinned_dev_ptr(out_len));
    uint8_t* z_st = static_cast<uint8_t*>(pinned_dev_ptr(status));
    const bool pin_in = z_in != nullptr, pin_out = z_out != nullptr;
    const bool pin_meta = z_off && z_len && (!status || z_st) && (!is_name_bits || z_nm);  // offsets/lengths DMA'd in place
    // Zero copy: with every caller array pinned (so device-visible) the kernels read the input and write the
    // output across PCIe themselves, one launch, no DMA staging -- both link directions in use at once (the
    // chunked DMA pipeline below moved ~55 GB/s in all).  HHUFF_HOST_COPY=1 keeps the pipeline.
    const char* hc = getenv("HHUFF_HOST_COPY");
    // the kernels' 16-B staging loads / stores and dword offset loads need the device API's alignment
    // (hhuff.h: in / out 16-B aligned, arrays 4-B aligned): an offset view of a registered socket buffer
    // or a numpy slice takes the chunked pipeline instead, whose staged buffers are aligned
    const bool aligned = !misaligned(z_in, 16) && !misaligned(z_out, 16) && !misaligned(z_off, 4) && !misaligned(z_len, 4) &&
                         !misaligned(z_nm, 4);
    if (pin_in && pin_out && pin_meta && aligned && !(hc && *hc && *hc != '0')) {  // (out_size: checked by every caller)
        // (the kernel variant follows the batch's own bytes: a shard of a larger buffer passes in_off + lo)
        const uint64_t sel = (uint64_t)in_off[n] - in_off[0];
        const hipError_t e = launch_slots(decode, z_in, in_size, z_off, nullptr, n, z_nm, z_out, nullptr, z_len, z_st, c.stream, sel);
        if (e != hipSuccess) return hip_fail(e, decode ? "decode launch (zero copy)" : "encode launch (zero copy)");
        HIP_TRY(hipStreamSynchronize(c.stream), "sync");
        return HHUFF_OK;
    }
    const std::vector<uint64_t> cut = chunk_cuts(in_off, n, chunk_bytes);  // multiples of 32 strings, about chunk_bytes each
    auto drain = [&](Slot& x) -> int {
        if (!x.busy) return HHUFF_OK;
        HIP_TRY(hipStreamSynchronize(x.s), "sync");
        if (!pin_out && x.out_n) par_copy(out + x.out_lo, x.h + x.h_out, x.out_n);
        if (!pin_meta) {
            par_copy(out_len + x.i0, x.h + x.h_len, x.m * 4);
            if (status) par_copy(status + x.i0, x.h + x.h_st, x.m);
        }
        x.busy = false;
        return HHUFF_OK;
    };
    for (size_t k = 0; k + 1 < cut.size(); ++k) {
        Slot& x = P.slot[k % kDepth];
        rc = drain(x);
        if (rc) return rc;
        const uint64_t i0 = cut[k], i1 = cut[k + 1], m = i1 - i0;
        const uint64_t e0 = in_off[i1];
        // the device slot's layout, and the pinned slot's: [in bytes][in_off m + 1][names][out][out_len m][status m]
        const ChunkLayout L = chunk_layout(decode, in_off[i0], e0, m, is_name_bits != nullptr);
        const uint64_t base = L.base, nbytes = L.nbytes, olo = L.olo, ohi = L.ohi, obase = L.obase;  // (ohi <= out_size: check_implicit)
        const size_t nw = L.nw, o_in = 0, o_off = L.o_off, o_nm = L.o_nm, o_out = L.o_out, o_len = L.o_len, o_st = L.o_st;
        rc = grow(x, L.need, L.need);
        if (rc) return rc;
        if (pin_in) {
            HIP_TRY(hipMemcpyAsync(x.d + o_in, in + base, nbytes, hipMemcpyHostToDevice, x.s), "H2D in");
        } else {
            par_copy(x.h + o_in, in + base, nbytes);
            HIP_TRY(hipMemcpyAsync(x.d + o_in, x.h + o_in, nbytes, hipMemcpyHostToDevice, x.s), "H2D in");
        }
        if (pin_meta) {
            HIP_TRY(hipMemcpyAsync(x.d + o_off, in_off + i0, (m + 1) * 4, hipMemcpyHostToDevice, x.s), "H2D offsets");
            if (nw)
                HIP_TRY(hipMemcpyAsync(x.d + o_nm, is_name_bits + i0 / 32, nw * 4, hipMemcpyHostToDevice, x.s),
                        "H2D names");
        } else {
            par_copy(x.h + o_off, in_off + i0, (m + 1) * 4);
            if (nw) memcpy(x.h + o_nm, is_name_bits + i0 / 32, nw * 4);
            HIP_TRY(hipMemcpyAsync(x.d + o_off, x.h + o_off, (o_nm - o_off) + nw * 4, hipMemcpyHostToDevice, x.s),
                    "H2D offsets");
        }
        const uint8_t* d_in = x.d + o_in - base;  // absolute offsets address the chunk
        uint8_t* d_out = x.d + o_out - obase;
        const uint32_t* d_off = reinterpret_cast<const uint32_t*>(x.d + o_off);
        uint32_t* d_len = reinterpret_cast<uint32_t*>(x.d + o_len);
        uint8_t* d_st = x.d + o_st;
        const uint32_t* d_nm = nw ? reinterpret_cast<const uint32_t*>(x.d + o_nm) : nullptr;
        const hipError_t e = launch_slots(decode, d_in, e0, d_off, nullptr, (uint32_t)m, d_nm, d_out, nullptr, d_len,
                                          status ? d_st : nullptr, x.s, nbytes);
        if (e != hipSuccess) return hip_fail(e, decode ? "decode launch" : "encode launch");
        x.i0 = i0;
        x.m = m;
        x.out_lo = olo;
        x.out_n = ohi > olo ? ohi - olo : 0;
        x.h_out = o_out;
        x.h_len = o_len;
        x.h_st = o_st;
        if (x.out_n) {
            if (pin_out)
                HIP_TRY(hipMemcpyAsync(out + olo, d_out + olo, x.out_n, hipMemcpyDeviceToHost, x.s), "D2H out");
            else
                HIP_TRY(hipMemcpyAsync(x.h + o_out, d_out + olo, x.out_n, hipMemcpyDeviceToHost, x.s), "D2H out");
        }
        if (pin_meta) {
            HIP_TRY(hipMemcpyAsync(out_len + i0, x.d + o_len, m * 4, hipMemcpyDeviceToHost, x.s), "D2H len");
            if (status) HIP_TRY(hipMemcpyAsync(status + i0, x.d + o_st, m, hipMemcpyDeviceToHost, x.s), "D2H status");
        } else {
            HIP_TRY(hipMemcpyAsync(x.h + o_len, x.d + o_len, o_st + m - o_len, hipMemcpyDeviceToHost, x.s), "D2H len");
        }
        x.busy = true;
    }
    for (auto& x : P.slot) {
        rc = drain(x);
        if (rc) return rc;
    }
    return HHUFF_OK;
}

namespace {

// (3c) packed host path: the packed kernels (hhuff_*_batch_packed) on host buffers.  With every caller array pinned
// and aligned the kernels read the strings and write only the outputs' bytes, out_off, out_len and status across
// PCIe (zero copy; the slot layout's tails, ~45 % of a decode slot and ~25 % of an encode slot on header text,
// never cross the link); otherwise one staged round trip through device memory.  out_off may be NULL (the caller
// places string i at its tile's position plus the kept lengths before it in the tile) and so may an encode's
// status (out_len says HHUFF_FAIL_LEN): 4 and 1 bytes a string fewer across the link.
int host_packed(bool decode, const uint8_t* in, uint64_t in_size, const uint32_t* in_off, uint32_t n,
                const uint32_t* is_name_bits, uint8_t* out, uint64_t out_size, uint32_t* out_off, uint32_t* out_len,
                uint8_t* status, int device) {
    if (n == 0) return HHUFF_OK;
    if (null_array(decode, in, in_off, out, out_len, status)) return arg_fail("NULL array");
    if (const int bad = check_implicit(decode, in_size, in_off[n], out_size)) return bad;
    const uint64_t slot_end = slot_of(decode, in_off[n]);
    if ((decode ? (in_size * 8) / 5 : in_size) >= 0xFFFFFFFFull) return arg_fail("in_size too large for u32 packed offsets");
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return hip_fail(guard.err, "hipSetDevice");
    Ctx& c = t_ctx;
    int rc = c.bind(device);
    if (rc) return rc;
    const uint8_t* z_in = static_cast<const uint8_t*>(pinned_dev_ptr(in));
    const uint32_t* z_off = static_cast<const uint32_t*>(pinned_dev_ptr(in_off));
    const uint32_t* z_nm = static_cast<const uint32_t*>(pinned_dev_ptr(is_name_bits));
    uint8_t* z_out = static_cast<uint8_t*>(pinned_dev_ptr(out));
    uint32_t* z_ooff = static_cast<uint32_t*>(pinned_dev_ptr(out_off));
    uint32_t* z_len = static_cast<uint32_t*>(pinned_dev_ptr(out_len));
    uint8_t* z_st = static_cast<uint8_t*>(pinned_dev_ptr(status));
    const bool zero = z_in && z_off && (!is_name_bits || z_nm) && z_out && (!out_off || z_ooff) && z_len &&
                      (!status || z_st) && !misaligned(z_in, 16) && !misaligned(z_out, 16) && !misaligned(z_off, 4) &&
                      !misaligned(z_nm, 4) && !misaligned(z_ooff, 4) && !misaligned(z_len, 4);
    hipStream_t s = c.stream;
    auto launch_packed = [&](const uint8_t* p_in, const uint32_t* p_off, const uint32_t* p_nm, uint8_t* p_out, uint32_t* p_ooff,
                             uint32_t* p_len, uint8_t* p_st) {
        return decode ? hhuff::launch_decode_packed(p_in, in_size, p_off, n, p_nm, p_out, p_ooff, p_len, p_st, s)
                      : hhuff::launch_encode_packed(p_in, in_size, p_off, n, p_out, p_ooff, p_len, p_st, s);
    };
    if (zero) {
        if (!out_off) {  // not returned: the kernels' offsets stay in device scratch and never cross the link
            rc = c.reserve(up16(((size_t)n + 1) * 4), 0);
            if (rc) return rc;
            z_ooff = reinterpret_cast<uint32_t*>(c.d);
        }
        const hipError_t e = launch_packed(z_in, z_off, z_nm, z_out, z_ooff, z_len, z_st);
        if (e != hipSuccess) return hip_fail(e, decode ? "packed decode launch (zero copy)" : "packed encode launch (zero copy)");
        HIP_TRY(hipStreamSynchronize(s), "sync");
        return HHUFF_OK;
    }
    const size_t nw = ((size_t)n + 31) / 32;
    const size_t need = up16(in_size ? in_size : 1) + up16(((size_t)n + 1) * 4) + (is_name_bits ? up16(nw * 4) : 0) +
                        up16(slot_end + 16) + up16(((size_t)n + 1) * 4) + up16((size_t)n * 4) + up16(n);
    rc = c.reserve(need, 0);
    if (rc) return rc;
    Carve cv{c.d};
    uint8_t* d_in = cv.take<uint8_t>(in_size ? in_size : 1);
    uint32_t* d_off = cv.take<uint32_t>((size_t)n + 1);
    uint32_t* d_nm = is_name_bits ? cv.take<uint32_t>(nw) : nullptr;
    uint8_t* d_out = cv.take<uint8_t>(slot_end + 16);
    uint32_t* d_ooff = cv.take<uint32_t>((size_t)n + 1);
    uint32_t* d_len = cv.take<uint32_t>(n);
    uint8_t* d_st = cv.take<uint8_t>(n);
    HIP_TRY(hipMemcpyAsync(d_in, in, in_size, hipMemcpyHostToDevice, s), "H2D in");
    HIP_TRY(hipMemcpyAsync(d_off, in_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, s), "H2D in_off");
    if (is_name_bits) HIP_TRY(hipMemcpyAsync(d_nm, is_name_bits, nw * 4, hipMemcpyHostToDevice, s), "H2D is_name");
    const hipError_t e = launch_packed(d_in, d_off, d_nm, d_out, d_ooff, d_len, status ? d_st : nullptr);
    if (e != hipSuccess) return hip_fail(e, decode ? "packed decode launch" : "packed encode launch");
    // the metadata first: the tiles' runs follow from out_off / out_len, and only the runs go back to the caller
    // (the gaps between them were never written by the kernels; the caller's bytes there stay untouched, as on
    // the zero-copy path: hhuff.h's packed contract)
    std::vector<uint32_t> tmp_off(out_off ? 0 : (size_t)n + 1);
    uint32_t* h_ooff = out_off ? out_off : tmp_off.data();
    HIP_TRY(hipMemcpyAsync(h_ooff, d_ooff, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, s), "D2H out_off");
    HIP_TRY(hipMemcpyAsync(out_len, d_len, (size_t)n * 4, hipMemcpyDeviceToHost, s), "D2H out_len");
    if (status) HIP_TRY(hipMemcpyAsync(status, d_st, n, hipMemcpyDeviceToHost, s), "D2H status");
    HIP_TRY(hipStreamSynchronize(s), "sync");
    // run of tile t: [its slot position, end of its last kept string); chunks of the device output go through the
    // context's pinned buffer and each run's part of a chunk is copied out of it
    // (hhuff_hostplan.h packed_ntiles, run_lo, run_hi)
    const uint32_t ntiles = packed_ntiles(n);
    auto lo_of = [&](uint32_t t) { return run_lo(decode, in_off, t); };
    auto hi_of = [&](uint32_t t) { return run_hi(n, h_ooff, out_len, t); };
    const size_t chunk = kPackedChunk;
    rc = c.reserve(need, std::min<size_t>(chunk, up16(slot_end + 16)));
    if (rc) return rc;
    uint32_t t = 0;
    for (uint64_t lo = 0; lo < slot_end && t < ntiles; lo += chunk) {
        const uint64_t hi = std::min<uint64_t>(slot_end, lo + chunk);
        while (t < ntiles && hi_of(t) <= lo) ++t;  // runs ending before this chunk (empty runs included)
        if (t >= ntiles || lo_of(t) >= hi) continue;  // nothing of any run in this chunk
        HIP_TRY(hipMemcpyAsync(c.h, d_out + lo, hi - lo, hipMemcpyDeviceToHost, s), "D2H out");
        HIP_TRY(hipStreamSynchronize(s), "sync");
        for (uint32_t u = t; u < ntiles; ++u) {
            const uint64_t a = std::max(lo_of(u), lo), b = std::min(hi_of(u), hi);
            if (lo_of(u) >= hi) break;
            if (b > a) memcpy(out + a, c.h + (a - lo), b - a);
        }
    }
    return HHUFF_OK;
}

}  // namespace

HHUFF_API int hhuff_decode_batch_host_packed(const uint8_t* in, uint64_t in_size, const uint32_t* in_off, uint32_t n,
                                             const uint32_t* is_name_bits, uint8_t* out, uint64_t out_size, uint32_t* out_off,
                                             uint32_t* out_len, uint8_t* status, int device) {
    return host_packed(true, in, in_size, in_off, n, is_name_bits, out, out_size, out_off, out_len, status, device);
}

HHUFF_API int hhuff_encode_batch_host_packed(const uint8_t* in, uint64_t in_size, const uint32_t* in_off, uint32_t n,
                                             uint8_t* out, uint64_t out_size, uint32_t* out_off, uint32_t* out_len,
                                             uint8_t* status, int device) {
    return host_packed(false, in, in_size, in_off, n, nullptr, out, out_size, out_off, out_len, status, device);
}

HHUFF_API int hhuff_decode_batch_host_pipelined(const uint8_t* in, uint64_t in_size, const uint32_t* in_off, uint32_t n,
                                                const uint32_t* is_name_bits, uint8_t* out, uint64_t out_size,
                                                uint32_t* out_len, uint8_t* status, int device, uint64_t chunk_bytes) {
    if (n == 0) return HHUFF_OK;
    if (null_array(true, in, in_off, out, out_len, status)) return arg_fail("NULL array");
    const int bad = check_implicit(true, in_size, in_off[n], out_size);
    if (bad) return bad;
    return pipelined(true, in, in_size, in_off, n, is_name_bits, out, out_size, out_len, status, device, chunk_bytes);
}

HHUFF_API int hhuff_encode_batch_host_pipelined(const uint8_t* in, uint64_t in_size, const uint32_t* in_off, uint32_t n,
                                                uint8_t* out, uint64_t out_size, uint32_t* out_len, uint8_t* status,
                                                int device, uint64_t chunk_bytes) {
    if (n == 0) return HHUFF_OK;
    if (null_array(false, in, in_off, out, out_len, status)) return arg_fail("NULL array");
    const int bad = check_implicit(false, in_size, in_off[n], out_size);
    if (bad) return bad;
    return pipelined(false, in, in_size, in_off, n, nullptr, out, out_size, out_len, status, device, chunk_bytes);
}

HHUFF_API int hhuff_decode_batch_host(const uint8_t* in, uint64_t in_size, const uint32_t* in_off, const uint32_t* in_len,
                                      uint32_t n, const uint32_t* is_name_bits, uint8_t* out, uint64_t out_size,
                                      const uint32_t* out_off, uint32_t* out_len, uint8_t* status, int device) {
    return host_batch(true, in, in_size, in_off, in_len, n, is_name_bits, out, out_size, out_off, out_len, status, device);
}

HHUFF_API int hhuff_encode_batch_host(const uint8_t* in, uint64_t in_size, const uint32_t* in_off, const uint32_t* in_len,
                                      uint32_t n, uint8_t* out, uint64_t out_size, const uint32_t* out_off,
                                      uint32_t* out_len, uint8_t* status, int device) {
    return host_batch(false, in, in_size, in_off, in_len, n, nullptr, out, out_size, out_off, out_len, status, device);
}
