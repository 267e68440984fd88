// hhuff C-ABI shim, the header-block families (include/hhuff.h (2d) to (2i)): HPACK and QPACK decode, both response
// encoders, the encoder and decoder sessions and the connection images.  Argument checks and one launch each
// (hhuff_launch.h); host code only.
#include "hhuff_host.h"
#include "hhuff_image.h"

using namespace hhuff;

HHUFF_API uint64_t hhuff_hpack_scratch_size(uint32_t nconn, uint32_t table_size) {
    return (uint64_t)nconn * hhuff::hpack_conn_scratch(table_size);
}

namespace {
// the checks and the launch the six HPACK block calls share; c.cmap is made here
int hpack_blocks(const hhuff_conn_slots_t* slots, hhuff::HpdCall& c, uint64_t scratch_size, void* stream) {
    if (const char* bad = hhuff::conn_slots_check(slots, c.nconn, scratch_size, hhuff::hpack_conn_scratch(c.table_size)))
        return arg_fail(bad);
    if (c.nconn == 0) return HHUFF_OK;
    if (!c.in || !c.blk_off || !c.conn_first || !c.arena || !c.arena_off || !c.name_off || !c.name_len || !c.value_off ||
        !c.value_len || !c.fflags || !c.nfields || !c.bstatus || !c.scratch)
        return arg_fail("NULL array");
    if (!slots && scratch_size < hhuff_hpack_scratch_size(c.nconn, c.table_size))
        return arg_fail("scratch smaller than hhuff_hpack_scratch_size");
    if (misaligned(c.scratch, 16)) return arg_fail("scratch must be 16-byte aligned");
    if (misaligned(c.req, 8)) return arg_fail("req must be 8-byte aligned");
    if (misaligned(c.res, 4)) return arg_fail("res must be 4-byte aligned");
    return launch_mapped(slots, c, stream, hhuff::launch_hpack_blocks, "hpack block launch");
}
}  // namespace

HHUFF_API int hhuff_hpack_decode_blocks_slots(const hhuff_conn_slots_t* slots, const uint8_t* in, uint64_t in_size,
                                              const uint32_t* blk_off, const uint32_t* conn_first, uint32_t nconn,
                                              uint32_t table_size, uint8_t* arena, const uint64_t* arena_off,
                                              uint32_t* name_off, uint32_t* name_len, uint32_t* value_off,
                                              uint32_t* value_len, uint8_t* fflags, uint32_t* nfields, int32_t* bstatus,
                                              void* scratch, uint64_t scratch_size, unsigned flags, void* stream) {
    hhuff::HpdCall call{in, in_size, blk_off, conn_first, nconn, table_size, arena, arena_off, name_off, name_len, value_off,
                        value_len, fflags, nfields, bstatus, (uint8_t*)scratch, flags, nullptr, nullptr, nullptr, nullptr};
    return hpack_blocks(slots, call, scratch_size, stream);
}

HHUFF_API int hhuff_hpack_decode_blocks(const uint8_t* in, uint64_t in_size, const uint32_t* blk_off,
                                        const uint32_t* conn_first, uint32_t nconn, uint32_t table_size, uint8_t* arena,
                                        const uint64_t* arena_off, uint32_t* name_off, uint32_t* name_len,
                                        uint32_t* value_off, uint32_t* value_len, uint8_t* fflags, uint32_t* nfields,
                                        int32_t* bstatus, void* scratch, uint64_t scratch_size, unsigned flags,
                                        void* stream) {
    return hhuff_hpack_decode_blocks_slots(nullptr, in, in_size, blk_off, conn_first, nconn, table_size, arena, arena_off, name_off,
        name_len, value_off, value_len, fflags, nfields, bstatus, scratch, scratch_size, flags, stream);
}

HHUFF_API int hhuff_hpack_parse_requests_slots(const hhuff_conn_slots_t* slots, const uint8_t* in, uint64_t in_size,
                                               const uint32_t* blk_off, const uint32_t* conn_first, uint32_t nconn,
                                               uint32_t table_size, uint8_t* arena, const uint64_t* arena_off,
                                               uint32_t* name_off, uint32_t* name_len, uint32_t* value_off,
                                               uint32_t* value_len, uint8_t* fflags, uint32_t* nfields, int32_t* bstatus,
                                               hhuff_request_t* req, void* scratch, uint64_t scratch_size, unsigned flags,
                                               void* stream) {
    if (nconn != 0 && !req) return arg_fail("NULL array");
    hhuff::HpdCall call{in, in_size, blk_off, conn_first, nconn, table_size, arena, arena_off, name_off, name_len, value_off,
                        value_len, fflags, nfields, bstatus, (uint8_t*)scratch, flags, req, nullptr, nullptr, nullptr};
    return hpack_blocks(slots, call, scratch_size, stream);
}

HHUFF_API int hhuff_hpack_parse_requests(const uint8_t* in, uint64_t in_size, const uint32_t* blk_off,
                                         const uint32_t* conn_first, uint32_t nconn, uint32_t table_size, uint8_t* arena,
                                         const uint64_t* arena_off, uint32_t* name_off, uint32_t* name_len,
                                         uint32_t* value_off, uint32_t* value_len, uint8_t* fflags, uint32_t* nfields,
                                         int32_t* bstatus, hhuff_request_t* req, void* scratch, uint64_t scratch_size,
                                         unsigned flags, void* stream) {
    return hhuff_hpack_parse_requests_slots(nullptr, in, in_size, blk_off, conn_first, nconn, table_size, arena, arena_off, name_off,
        name_len, value_off, value_len, fflags, nfields, bstatus, req, scratch, scratch_size, flags, stream);
}

HHUFF_API int hhuff_hpack_parse_responses_slots(const hhuff_conn_slots_t* slots, const uint8_t* in, uint64_t in_size,
                                                const uint32_t* blk_off, const uint32_t* conn_first, uint32_t nconn,
                                                uint32_t table_size, const uint8_t* trailers, uint8_t* arena,
                                                const uint64_t* arena_off, uint32_t* name_off, uint32_t* name_len,
                                                uint32_t* value_off, uint32_t* value_len, uint8_t* fflags, uint32_t* nfields,
                                                int32_t* bstatus, hhuff_response_t* res, void* scratch,
                                                uint64_t scratch_size, unsigned flags, void* stream) {
    if (nconn != 0 && !res) return arg_fail("NULL array");
    hhuff::HpdCall call{in, in_size, blk_off, conn_first, nconn, table_size, arena, arena_off, name_off, name_len, value_off,
                        value_len, fflags, nfields, bstatus, (uint8_t*)scratch, flags, nullptr, res, trailers, nullptr};
    return hpack_blocks(slots, call, scratch_size, stream);
}

HHUFF_API int hhuff_hpack_parse_responses(const uint8_t* in, uint64_t in_size, const uint32_t* blk_off,
                                          const uint32_t* conn_first, uint32_t nconn, uint32_t table_size,
                                          const uint8_t* trailers, uint8_t* arena, const uint64_t* arena_off,
                                          uint32_t* name_off, uint32_t* name_len, uint32_t* value_off, uint32_t* value_len,
                                          uint8_t* fflags, uint32_t* nfields, int32_t* bstatus, hhuff_response_t* res,
                                          void* scratch, uint64_t scratch_size, unsigned flags, void* stream) {
    return hhuff_hpack_parse_responses_slots(nullptr, in, in_size, blk_off, conn_first, nconn, table_size, trailers, arena, arena_off,
        name_off, name_len, value_off, value_len, fflags, nfields, bstatus, res, scratch, scratch_size, flags, stream);
}

HHUFF_API uint64_t hhuff_hpack_enc_scratch_size(uint32_t nconn) { return (uint64_t)nconn * hhuff::hpenc_conn_scratch(); }

HHUFF_API int hhuff_hpack_flatten_responses_slots(const hhuff_conn_slots_t* slots, const uint8_t* in, uint64_t in_size,
                                                  const hhuff_hpack_header_t* hdr,
                                            uint32_t nhdr, const hhuff_hpack_response_t* res, const uint32_t* conn_first,
                                            uint32_t nconn, uint32_t nres, uint32_t server_off, uint32_t server_len,
                                            uint8_t* out, const uint64_t* out_off, uint32_t* out_len,
                                            uint32_t* headers_size, int32_t* rstatus, void* scratch, uint64_t scratch_size,
                                            unsigned flags, void* stream) {
    if (const char* bad = hhuff::conn_slots_check(slots, nconn, scratch_size, hhuff::hpenc_conn_scratch()))
        return arg_fail(bad);
    if (nconn == 0) return HHUFF_OK;
    if (!conn_first || !scratch || (nres && (!res || !out || !out_off || !out_len || !headers_size || !rstatus)) ||
        (nhdr && (!hdr || !in)))
        return arg_fail("NULL array");
    if (in_size >= (1ull << 32)) return arg_fail("in_size must stay below 2^32 (u32 offsets)");
    if (!slots && scratch_size < hhuff_hpack_enc_scratch_size(nconn))
        return arg_fail("scratch smaller than hhuff_hpack_enc_scratch_size");
    if (misaligned(scratch, 16)) return arg_fail("scratch must be 16-byte aligned");
    if (misaligned(res, 8) || misaligned(hdr, 4) || misaligned(out_off, 8))
        return arg_fail("misaligned hdr / res / out_off");
    hhuff::HpeCall call{in, in_size, hdr, nhdr, res, conn_first, nconn, nres, server_off, server_len,
                              out, out_off, out_len, headers_size, rstatus, (uint8_t*)scratch, flags, nullptr};
    return launch_mapped(slots, call, stream, hhuff::launch_hpack_flatten, "hpack flatten launch");
}

HHUFF_API int hhuff_hpack_flatten_responses(const uint8_t* in, uint64_t in_size, const hhuff_hpack_header_t* hdr,
                                            uint32_t nhdr, const hhuff_hpack_response_t* res, const uint32_t* conn_first,
                                            uint32_t nconn, uint32_t nres, uint32_t server_off, uint32_t server_len,
                                            uint8_t* out, const uint64_t* out_off, uint32_t* out_len,
                                            uint32_t* headers_size, int32_t* rstatus, void* scratch, uint64_t scratch_size,
                                            unsigned flags, void* stream) {
    return hhuff_hpack_flatten_responses_slots(nullptr, in, in_size, hdr, nhdr, res, conn_first, nconn, nres,
        server_off, server_len, out, out_off, out_len, headers_size, rstatus, scratch, scratch_size, flags, stream);
}

HHUFF_API int hhuff_qpack_flatten_responses(const uint8_t* in, uint64_t in_size, const hhuff_hpack_header_t* hdr,
                                            uint32_t nhdr, const hhuff_qpack_response_t* res, uint32_t nres,
                                            uint32_t server_off, uint32_t server_len, uint8_t* out, const uint64_t* out_off,
                                            uint32_t* out_len, uint32_t* header_len, int32_t* rstatus, void* stream) {
    if (nres == 0) return HHUFF_OK;
    if (!res || !out || !out_off || !out_len || !header_len || !rstatus || (nhdr && !hdr) || !in) return arg_fail("NULL array");
    if (in_size >= (1ull << 32)) return arg_fail("in_size must stay below 2^32 (u32 offsets)");
    if (misaligned(res, 8) || misaligned(hdr, 4) || misaligned(out_off, 8))
        return arg_fail("misaligned hdr / res / out_off");
    const hhuff::QpeCall call{in, in_size, hdr, nhdr, res, nres, server_off, server_len, out, out_off, out_len,
                              header_len, rstatus};
    hipError_t e = hhuff::launch_qpack_flatten(call, (hipStream_t)stream);
    return hip_rc(e, "qpack flatten launch");
}

HHUFF_API uint64_t hhuff_qpack_enc_scratch_size(uint32_t nconn, uint32_t header_table_size, uint32_t max_inflight) {
    return (uint64_t)nconn * hhuff::qpenc_conn_scratch(header_table_size, max_inflight);
}

HHUFF_API int hhuff_qpack_flatten_sessions_peers(const hhuff_qpack_peer_t* peers, const hhuff_conn_slots_t* slots,
                                                 const uint8_t* in, uint64_t in_size,
                                                 const hhuff_hpack_header_t* hdr, uint32_t nhdr,
                                           const hhuff_qpack_response_t* res, const uint32_t* conn_first, uint32_t nconn,
                                           uint32_t nres, const uint64_t* stream_id, const uint32_t* dec_off,
                                           const uint32_t* dec_len, uint32_t header_table_size, uint64_t max_blocked,
                                           uint32_t max_inflight, uint32_t server_off, uint32_t server_len, uint8_t* out,
                                           const uint64_t* out_off, uint32_t* out_len, uint32_t* header_len,
                                           int32_t* rstatus, uint8_t* rflags, uint8_t* enc_out, const uint64_t* enc_out_off,
                                           uint32_t* enc_out_len, int32_t* dec_status, uint32_t* dec_consumed, void* scratch,
                                           uint64_t scratch_size, unsigned flags, void* stream) {
    if (misaligned(peers, 4)) return arg_fail("peers must be 4-byte aligned");
    if (header_table_size > 65536u) {
        arg_fail("header_table_size must not exceed 65536");
        return HHUFF_RES_EINVAL;
    }
    if (flags & ~(HHUFF_QENC_CONTINUE | HHUFF_QENC_SET_CAPACITY | HHUFF_QENC_EVICT | HHUFF_QENC_DUP)) {
        arg_fail("unknown HHUFF_QENC_* flag");
        return HHUFF_RES_EINVAL;
    }
    if ((flags & HHUFF_QENC_DUP) && !(flags & HHUFF_QENC_EVICT)) {
        arg_fail("HHUFF_QENC_DUP needs HHUFF_QENC_EVICT");
        return HHUFF_RES_EINVAL;
    }
    if (const char* bad = hhuff::conn_slots_check(slots, nconn, scratch_size,
                                                  hhuff::qpenc_conn_scratch(header_table_size, max_inflight)))
        return arg_fail(bad);
    if (nconn == 0) return HHUFF_OK;
    if (!conn_first || !scratch || !enc_out || !enc_out_off || !enc_out_len || !dec_status || !dec_consumed ||
        (nres && (!res || !stream_id || !out || !out_off || !out_len || !header_len || !rstatus || !rflags)) ||
        (nhdr && !hdr) || ((nhdr || dec_off || server_len) && !in) || ((dec_off == nullptr) != (dec_len == nullptr)))
        return arg_fail("NULL array");
    if (in_size >= (1ull << 32)) return arg_fail("in_size must stay below 2^32 (u32 offsets)");
    if (!slots && scratch_size < hhuff_qpack_enc_scratch_size(nconn, header_table_size, max_inflight))
        return arg_fail("scratch smaller than hhuff_qpack_enc_scratch_size");
    if (misaligned(scratch, 16)) return arg_fail("scratch must be 16-byte aligned");
    if (misaligned(res, 8) || misaligned(hdr, 4) || misaligned(out_off, 8) ||
        misaligned(enc_out_off, 8) || misaligned(stream_id, 8))
        return arg_fail("misaligned hdr / res / out_off / enc_out_off / stream_id");
    hhuff::QseCall call{in, in_size, hdr, nhdr, res, conn_first, nconn, nres, stream_id, dec_off, dec_len,
                              header_table_size, max_blocked, max_inflight, server_off, server_len, out, out_off, out_len,
                              header_len, rstatus, rflags, enc_out, enc_out_off, enc_out_len, dec_status, dec_consumed,
                              (uint8_t*)scratch, flags, nullptr, peers};
    return launch_mapped(slots, call, stream, hhuff::launch_qpack_sessions, "qpack sessions launch");
}

HHUFF_API int hhuff_qpack_flatten_sessions_slots(const hhuff_conn_slots_t* slots, const uint8_t* in, uint64_t in_size,
                                                 const hhuff_hpack_header_t* hdr, uint32_t nhdr,
                                           const hhuff_qpack_response_t* res, const uint32_t* conn_first, uint32_t nconn,
                                           uint32_t nres, const uint64_t* stream_id, const uint32_t* dec_off,
                                           const uint32_t* dec_len, uint32_t header_table_size, uint64_t max_blocked,
                                           uint32_t max_inflight, uint32_t server_off, uint32_t server_len, uint8_t* out,
                                           const uint64_t* out_off, uint32_t* out_len, uint32_t* header_len,
                                           int32_t* rstatus, uint8_t* rflags, uint8_t* enc_out, const uint64_t* enc_out_off,
                                           uint32_t* enc_out_len, int32_t* dec_status, uint32_t* dec_consumed, void* scratch,
                                           uint64_t scratch_size, unsigned flags, void* stream) {
    return hhuff_qpack_flatten_sessions_peers(nullptr, slots, in, in_size, hdr, nhdr, res, conn_first, nconn, nres,
        stream_id, dec_off, dec_len, header_table_size, max_blocked, max_inflight, server_off, server_len, out,
        out_off, out_len, header_len, rstatus, rflags, enc_out, enc_out_off, enc_out_len, dec_status, dec_consumed,
        scratch, scratch_size, flags, stream);
}

HHUFF_API int hhuff_qpack_flatten_sessions(const uint8_t* in, uint64_t in_size, const hhuff_hpack_header_t* hdr, uint32_t nhdr,
                                           const hhuff_qpack_response_t* res, const uint32_t* conn_first, uint32_t nconn,
                                           uint32_t nres, const uint64_t* stream_id, const uint32_t* dec_off,
                                           const uint32_t* dec_len, uint32_t header_table_size, uint64_t max_blocked,
                                           uint32_t max_inflight, uint32_t server_off, uint32_t server_len, uint8_t* out,
                                           const uint64_t* out_off, uint32_t* out_len, uint32_t* header_len,
                                           int32_t* rstatus, uint8_t* rflags, uint8_t* enc_out, const uint64_t* enc_out_off,
                                           uint32_t* enc_out_len, int32_t* dec_status, uint32_t* dec_consumed, void* scratch,
                                           uint64_t scratch_size, unsigned flags, void* stream) {
    return hhuff_qpack_flatten_sessions_slots(nullptr, in, in_size, hdr, nhdr, res, conn_first, nconn, nres,
        stream_id, dec_off, dec_len, header_table_size, max_blocked, max_inflight, server_off, server_len, out,
        out_off, out_len, header_len, rstatus, rflags, enc_out, enc_out_off, enc_out_len, dec_status, dec_consumed,
        scratch, scratch_size, flags, stream);
}

HHUFF_API uint64_t hhuff_qpack_scratch_size(uint32_t nconn, uint32_t header_table_size) {
    return (uint64_t)nconn * hhuff::qpack_conn_scratch(header_table_size);
}

namespace {
// the checks and the launch the eight QPACK decoder calls share; c.cmap is made here.  sessions: one of the
// two _sessions calls, which `ds` alone cannot tell (they refuse a NULL ds, but only behind other checks)
int qpack_step(const hhuff_conn_slots_t* slots, hhuff::QpdCall& c, bool sessions, const hhuff_qpack_dsessions_t* ds,
               uint64_t scratch_size, void* stream) {
    if (sessions && c.max_blocked > 4096) return arg_fail("sessions: max_blocked above 4096");
    if (slots && c.T > (1u << 30)) return arg_fail("header_table_size above 2^30");
    if (const char* bad = hhuff::conn_slots_check(slots, c.nconn, scratch_size, hhuff::qpack_conn_scratch(c.T)))
        return arg_fail(bad);
    if (c.nconn == 0) return HHUFF_OK;
    if (sessions) {  // include/hhuff.h (2e''')
        if (!ds) return arg_fail("sessions: NULL hhuff_qpack_dsessions_t");
        if (c.nconn > 0x7FFFFFFFu) return arg_fail("sessions: nconn above 2^31 - 1");
        if (!ds->state || !ds->dec_out || !ds->dec_out_off || !ds->dec_out_len || (!ds->wake_id && c.max_blocked) ||
            !ds->wake_first || !ds->nwake || !ds->parked || !ds->dflags || (ds->cancel_first && !ds->cancel_id))
            return arg_fail("sessions: NULL array");
        if (ds->flags & ~HHUFF_QDS_SYNC) return arg_fail("sessions: unknown flag bit");
        if (ds->state_size < hhuff_qpack_dsession_state_size(slots ? slots->nslots : c.nconn, (uint32_t)c.max_blocked))
            return arg_fail("sessions: state smaller than hhuff_qpack_dsession_state_size");
        if (misaligned(ds->state, 16)) return arg_fail("sessions: state must be 16-byte aligned");
    }
    if (!c.in || !c.enc_off || !c.enc_len || !c.sec_off || !c.conn_first || !c.enc_status || !c.enc_consumed ||
        !c.insert_count || !c.scratch)
        return arg_fail("NULL array");
    if (c.nsec && (!c.arena || !c.arena_off || !c.name_off || !c.name_len || !c.value_off || !c.value_len || !c.fflags ||
                   !c.nfields || !c.sstatus || !c.req_insert_count))
        return arg_fail("NULL array");
    if (c.T > (1u << 30)) return arg_fail("header_table_size above 2^30");
    // u32 offsets, and the literal workspace is sized for in_size + 2 literals in 32 bits
    if (c.in_size > (1ull << 32) - 3) return arg_fail("in_size must be at most 2^32 - 3 (u32 offsets)");
    if (!slots && scratch_size < hhuff_qpack_scratch_size(c.nconn, c.T))
        return arg_fail("scratch smaller than hhuff_qpack_scratch_size");
    if (misaligned(c.scratch, 16)) return arg_fail("scratch must be 16-byte aligned");
    return launch_mapped(
        slots, c, stream, [ds](const hhuff::QpdCall& q, hipStream_t s) { return hhuff::launch_qpack(q, ds, s); }, "qpack launch");
}
}  // namespace

HHUFF_API uint64_t hhuff_qpack_dsession_state_size(uint32_t n, uint32_t max_blocked) {
    return max_blocked > 4096 ? 0u : (uint64_t)n * hhuff::qpack_dsession_slab(max_blocked);
}

HHUFF_API uint64_t hhuff_qpack_dsession_out_bound(uint32_t nsec_of_conn, uint32_t ncancel_of_conn) {
    return 10ull * ((uint64_t)nsec_of_conn + ncancel_of_conn) + 10u;
}

// ---- (2i) connection images ----
namespace {
// the family's slab as its own entry points size it; 0: parameters they refuse, or hhuff_image.h out of step
uint64_t conn_family_slab(const hhuff_conn_family_t* fam, hhuff::img::Layout& L) {
    if (!fam || !hhuff::img::layout(*fam, L)) return 0;
    uint64_t own = 0;
    switch (fam->family) {
        case HHUFF_FAM_HPACK_DEC: own = hhuff::hpack_conn_scratch(fam->table_size); break;
        case HHUFF_FAM_QPACK_DEC: own = hhuff::qpack_conn_scratch(fam->table_size); break;
        case HHUFF_FAM_HPACK_ENC: own = hhuff::hpenc_conn_scratch(); break;
        case HHUFF_FAM_QPACK_ENC: own = hhuff::qpenc_conn_scratch(fam->table_size, fam->max_inflight); break;
        default: own = hhuff::qpack_dsession_slab(fam->max_blocked); break;
    }
    return own == L.slab ? own : 0;
}

int conn_image_check(const hhuff_conn_family_t* fam, const void* scratch, uint64_t scratch_size, uint32_t nslots,
                     const void* img) {
    hhuff::img::Layout L;
    const uint64_t slab = conn_family_slab(fam, L);
    if (slab == 0) return arg_fail("connection family: unknown, or parameters the family refuses");
    if (nslots == 0) return arg_fail("nslots is 0");
    if (nslots > hhuff::kConnMaxSlots) return arg_fail("nslots above 2^31 - 1");
    if (scratch_size / slab < nslots) return arg_fail("scratch smaller than nslots slabs");
    if (misaligned(scratch, 16)) return arg_fail("scratch must be 16-byte aligned");
    if (misaligned(img, 16)) return arg_fail("img must be 16-byte aligned");
    return HHUFF_OK;
}
}  // namespace

HHUFF_API uint64_t hhuff_conn_slab_size(const hhuff_conn_family_t* fam) {
    hhuff::img::Layout L;
    return conn_family_slab(fam, L);
}

HHUFF_API uint64_t hhuff_conn_image_bound(const hhuff_conn_family_t* fam) {
    hhuff::img::Layout L;
    return conn_family_slab(fam, L) ? hhuff::img::image_bound(L) : 0;
}

HHUFF_API int hhuff_conn_export(const hhuff_conn_family_t* fam, const void* scratch, uint64_t scratch_size, uint32_t nslots,
                                const uint32_t* slot, uint32_t n, uint8_t* img, const uint64_t* img_off, uint32_t* img_len,
                                int32_t* status, void* stream) {
    if (const int rc = conn_image_check(fam, scratch, scratch_size, nslots, img)) return rc;
    if (n == 0) return HHUFF_OK;
    if (!scratch || !slot || !img_len || !status || (img && !img_off)) return arg_fail("NULL array");
    if (misaligned(img_off, 8)) return arg_fail("img_off must be 8-byte aligned");
    const hipError_t e = hhuff::launch_conn_export(*fam, (const uint8_t*)scratch, nslots, slot, n, img, img_off, img_len,
                                                   status, (hipStream_t)stream);
    return hip_rc(e, "connection export launch");
}

HHUFF_API int hhuff_conn_import(const hhuff_conn_family_t* fam, void* scratch, uint64_t scratch_size, uint32_t nslots,
                                const uint32_t* slot, uint32_t n, const uint8_t* img, const uint64_t* img_off,
                                const uint32_t* img_len, int32_t* status, void* stream) {
    if (const int rc = conn_image_check(fam, scratch, scratch_size, nslots, img)) return rc;
    if (n == 0) return HHUFF_OK;
    if (!scratch || !slot || !img || !img_off || !img_len || !status) return arg_fail("NULL array");
    if (misaligned(img_off, 8)) return arg_fail("img_off must be 8-byte aligned");
    const hipError_t e = hhuff::launch_conn_import(*fam, (uint8_t*)scratch, nslots, slot, n, img, img_off, img_len, status,
                                                   (hipStream_t)stream);
    return hip_rc(e, "connection import launch");
}

HHUFF_API int hhuff_qpack_parse_requests_sessions(
    const hhuff_qpack_dsessions_t* ds, const hhuff_conn_slots_t* slots, const uint8_t* in, uint64_t in_size,
    const uint32_t* enc_off, const uint32_t* enc_len, const uint32_t* sec_off, const uint32_t* conn_first, uint32_t nconn,
    uint32_t nsec, uint32_t header_table_size, uint64_t max_blocked, uint8_t* arena, const uint64_t* arena_off,
    uint32_t* name_off, uint32_t* name_len, uint32_t* value_off, uint32_t* value_len, uint8_t* fflags, uint32_t* nfields,
    int32_t* sstatus, uint64_t* req_insert_count, int32_t* enc_status, uint32_t* enc_consumed, uint64_t* insert_count,
    const uint64_t* stream_id, hhuff_qpack_request_t* req, void* scratch, uint64_t scratch_size, unsigned flags,
    void* stream) {
    if (nconn != 0 && nsec != 0 && (!stream_id || !req)) return arg_fail("NULL array");
    if (misaligned(req, 8)) return arg_fail("req must be 8-byte aligned");
    hhuff::QpdCall call{in, in_size, enc_off, enc_len, sec_off, conn_first, nullptr, nconn, nsec, header_table_size,
                        max_blocked, arena, arena_off, name_off, name_len, value_off, value_len, fflags, nfields, sstatus,
                        req_insert_count, enc_status, enc_consumed, insert_count, (uint8_t*)scratch, flags,
                        stream_id, req, nullptr, nullptr};
    return qpack_step(slots, call, true, ds, scratch_size, stream);
}

HHUFF_API int hhuff_qpack_parse_responses_sessions(
    const hhuff_qpack_dsessions_t* ds, const hhuff_conn_slots_t* slots, const uint8_t* in, uint64_t in_size,
    const uint32_t* enc_off, const uint32_t* enc_len, const uint32_t* sec_off, const uint32_t* conn_first, uint32_t nconn,
    uint32_t nsec, uint32_t header_table_size, uint64_t max_blocked, uint8_t* arena, const uint64_t* arena_off,
    uint32_t* name_off, uint32_t* name_len, uint32_t* value_off, uint32_t* value_len, uint8_t* fflags, uint32_t* nfields,
    int32_t* sstatus, uint64_t* req_insert_count, int32_t* enc_status, uint32_t* enc_consumed, uint64_t* insert_count,
    const uint64_t* stream_id, hhuff_qpack_response_head_t* res, void* scratch, uint64_t scratch_size, unsigned flags,
    void* stream) {
    if (nconn != 0 && nsec != 0 && (!stream_id || !res)) return arg_fail("NULL array");
    if (misaligned(res, 8)) return arg_fail("res must be 8-byte aligned");
    hhuff::QpdCall call{in, in_size, enc_off, enc_len, sec_off, conn_first, nullptr, nconn, nsec, header_table_size,
                        max_blocked, arena, arena_off, name_off, name_len, value_off, value_len, fflags, nfields, sstatus,
                        req_insert_count, enc_status, enc_consumed, insert_count, (uint8_t*)scratch, flags,
                        stream_id, nullptr, res, nullptr};
    return qpack_step(slots, call, true, ds, scratch_size, stream);
}

HHUFF_API int hhuff_qpack_decode_slots(const hhuff_conn_slots_t* slots, const uint8_t* in, uint64_t in_size,
                                       const uint32_t* enc_off, const uint32_t* enc_len, const uint32_t* sec_off,
                                       const uint32_t* conn_first, uint32_t nconn, uint32_t nsec, uint32_t header_table_size,
                                       uint64_t max_blocked, const uint32_t* num_blocked, uint8_t* arena,
                                       const uint64_t* arena_off, uint32_t* name_off, uint32_t* name_len,
                                       uint32_t* value_off, uint32_t* value_len, uint8_t* fflags, uint32_t* nfields,
                                       int32_t* sstatus, uint64_t* req_insert_count, int32_t* enc_status,
                                       uint32_t* enc_consumed, uint64_t* insert_count, void* scratch, uint64_t scratch_size,
                                       unsigned flags, void* stream) {
    hhuff::QpdCall call{in, in_size, enc_off, enc_len, sec_off, conn_first, num_blocked, nconn, nsec, header_table_size,
                        max_blocked, arena, arena_off, name_off, name_len, value_off, value_len, fflags, nfields, sstatus,
                        req_insert_count, enc_status, enc_consumed, insert_count, (uint8_t*)scratch, flags,
                        nullptr, nullptr, nullptr, nullptr};
    return qpack_step(slots, call, false, nullptr, scratch_size, stream);
}

HHUFF_API int hhuff_qpack_decode(const uint8_t* in, uint64_t in_size, const uint32_t* enc_off, const uint32_t* enc_len,
                                 const uint32_t* sec_off, const uint32_t* conn_first, uint32_t nconn, uint32_t nsec,
                                 uint32_t header_table_size, uint64_t max_blocked, const uint32_t* num_blocked,
                                 uint8_t* arena, const uint64_t* arena_off, uint32_t* name_off, uint32_t* name_len,
                                 uint32_t* value_off, uint32_t* value_len, uint8_t* fflags, uint32_t* nfields,
                                 int32_t* sstatus, uint64_t* req_insert_count, int32_t* enc_status,
                                 uint32_t* enc_consumed, uint64_t* insert_count, void* scratch, uint64_t scratch_size,
                                 unsigned flags, void* stream) {
    return hhuff_qpack_decode_slots(nullptr, in, in_size, enc_off, enc_len, sec_off, conn_first, nconn, nsec, header_table_size,
        max_blocked, num_blocked, arena, arena_off, name_off, name_len, value_off, value_len, fflags, nfields, sstatus,
        req_insert_count, enc_status, enc_consumed, insert_count, scratch, scratch_size, flags, stream);
}

HHUFF_API int hhuff_qpack_parse_requests_slots(const hhuff_conn_slots_t* slots, const uint8_t* in, uint64_t in_size,
                                               const uint32_t* enc_off, const uint32_t* enc_len, const uint32_t* sec_off,
                                               const uint32_t* conn_first, uint32_t nconn, uint32_t nsec,
                                               uint32_t header_table_size, uint64_t max_blocked, const uint32_t* num_blocked,
                                               uint8_t* arena, const uint64_t* arena_off, uint32_t* name_off,
                                               uint32_t* name_len, uint32_t* value_off, uint32_t* value_len, uint8_t* fflags,
                                               uint32_t* nfields, int32_t* sstatus, uint64_t* req_insert_count,
                                               int32_t* enc_status, uint32_t* enc_consumed, uint64_t* insert_count,
                                               const uint64_t* stream_id, hhuff_qpack_request_t* req, void* scratch,
                                               uint64_t scratch_size, unsigned flags, void* stream) {
    if (nconn != 0 && nsec != 0 && (!stream_id || !req)) return arg_fail("NULL array");
    if (misaligned(req, 8)) return arg_fail("req must be 8-byte aligned");
    hhuff::QpdCall call{in, in_size, enc_off, enc_len, sec_off, conn_first, num_blocked, nconn, nsec, header_table_size,
                        max_blocked, arena, arena_off, name_off, name_len, value_off, value_len, fflags, nfields, sstatus,
                        req_insert_count, enc_status, enc_consumed, insert_count, (uint8_t*)scratch, flags,
                        stream_id, req, nullptr, nullptr};
    return qpack_step(slots, call, false, nullptr, scratch_size, stream);
}

HHUFF_API int hhuff_qpack_parse_requests(const uint8_t* in, uint64_t in_size, const uint32_t* enc_off,
                                         const uint32_t* enc_len, const uint32_t* sec_off, const uint32_t* conn_first,
                                         uint32_t nconn, uint32_t nsec, uint32_t header_table_size, uint64_t max_blocked,
                                         const uint32_t* num_blocked, uint8_t* arena, const uint64_t* arena_off,
                                         uint32_t* name_off, uint32_t* name_len, uint32_t* value_off, uint32_t* value_len,
                                         uint8_t* fflags, uint32_t* nfields, int32_t* sstatus, uint64_t* req_insert_count,
                                         int32_t* enc_status, uint32_t* enc_consumed, uint64_t* insert_count,
                                         const uint64_t* stream_id, hhuff_qpack_request_t* req, void* scratch,
                                         uint64_t scratch_size, unsigned flags, void* stream) {
    return hhuff_qpack_parse_requests_slots(nullptr, in, in_size, enc_off, enc_len, sec_off, conn_first, nconn, nsec,
        header_table_size, max_blocked, num_blocked, arena, arena_off, name_off, name_len, value_off, value_len, fflags, nfields,
        sstatus, req_insert_count, enc_status, enc_consumed, insert_count, stream_id, req, scratch, scratch_size, flags, stream);
}

HHUFF_API int hhuff_qpack_parse_responses_slots(const hhuff_conn_slots_t* slots, const uint8_t* in, uint64_t in_size,
                                                const uint32_t* enc_off, const uint32_t* enc_len, const uint32_t* sec_off,
                                                const uint32_t* conn_first, uint32_t nconn, uint32_t nsec,
                                                uint32_t header_table_size, uint64_t max_blocked,
                                                const uint32_t* num_blocked, uint8_t* arena, const uint64_t* arena_off,
                                                uint32_t* name_off, uint32_t* name_len, uint32_t* value_off,
                                                uint32_t* value_len, uint8_t* fflags, uint32_t* nfields, int32_t* sstatus,
                                                uint64_t* req_insert_count, int32_t* enc_status, uint32_t* enc_consumed,
                                                uint64_t* insert_count, const uint64_t* stream_id,
                                                hhuff_qpack_response_head_t* res, void* scratch, uint64_t scratch_size,
                                                unsigned flags, void* stream) {
    if (nconn != 0 && nsec != 0 && (!stream_id || !res)) return arg_fail("NULL array");
    if (misaligned(res, 8)) return arg_fail("res must be 8-byte aligned");
    hhuff::QpdCall call{in, in_size, enc_off, enc_len, sec_off, conn_first, num_blocked, nconn, nsec, header_table_size,
                        max_blocked, arena, arena_off, name_off, name_len, value_off, value_len, fflags, nfields, sstatus,
                        req_insert_count, enc_status, enc_consumed, insert_count, (uint8_t*)scratch, flags,
                        stream_id, nullptr, res, nullptr};
    return qpack_step(slots, call, false, nullptr, scratch_size, stream);
}

HHUFF_API int hhuff_qpack_parse_responses(const uint8_t* in, uint64_t in_size, const uint32_t* enc_off,
                                          const uint32_t* enc_len, const uint32_t* sec_off, const uint32_t* conn_first,
                                          uint32_t nconn, uint32_t nsec, uint32_t header_table_size, uint64_t max_blocked,
                                          const uint32_t* num_blocked, uint8_t* arena, const uint64_t* arena_off,
                                          uint32_t* name_off, uint32_t* name_len, uint32_t* value_off, uint32_t* value_len,
                                          uint8_t* fflags, uint32_t* nfields, int32_t* sstatus, uint64_t* req_insert_count,
                                          int32_t* enc_status, uint32_t* enc_consumed, uint64_t* insert_count,
                                          const uint64_t* stream_id, hhuff_qpack_response_head_t* res, void* scratch,
                                          uint64_t scratch_size, unsigned flags, void* stream) {
    return hhuff_qpack_parse_responses_slots(nullptr, in, in_size, enc_off, enc_len, sec_off, conn_first, nconn, nsec,
        header_table_size, max_blocked, num_blocked, arena, arena_off, name_off, name_len, value_off, value_len, fflags, nfields,
        sstatus, req_insert_count, enc_status, enc_consumed, insert_count, stream_id, res, scratch, scratch_size, flags, stream);
}
