// HTTP/2 request bodies on the receive side (include/hhuff.h (2k'''')): what handle_request_body_chunk
// (lib/http2/connection.c:518-607) appends to a stream's req_body.buf, for one step of one connection, as a plan over
// the stream table's events.  The device kernels (hhuff_h2bodies.hip) and the host program (tools/h2bodies_host.cpp)
// run this very code.
//   probe       the connection's own table, stream id -> run: open addressing, linear probes, two entries a frame slot
//   walk        one connection's events in wire order: per BODY slot its run and its offset inside the run, per run
//               its record, then the verdict, the runs' places and the counts of copy jobs and destination lines
//   jobs_of     the copy jobs of a planned connection, in slot order, from what the walk left per slot -- no lookup
// A job's bytes are copied a 16-byte line of the destination at a time by lc::copy_line (hhuff_linecopy.h).
#ifndef HHUFF_H2BODIES_H
#define HHUFF_H2BODIES_H
#include <stdint.h>

#include "hhuff.h"
#include "hhuff_h2ctl.h"
#include "hhuff_linecopy.h"

namespace hhuff {
namespace h2b {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kReset = HHUFF_H2SE_RESET_SENT | HHUFF_H2SE_RESET_BY_PEER;

struct Key {  // 8 bytes; stream_id 0: the entry is free
    uint32_t stream_id, run;
};
struct Slot {  // 16 bytes, one per walked frame slot; run kNone: no BODY event
    uint32_t run, off;  // the run's number in the connection, the payload's offset inside the run
    uint32_t src, len;  // in[src .. src + len)
};
struct Job {  // 16 bytes: in[src .. src + len) -> out[dst .. dst + len), len >= 1; pre = the lines of the jobs before
    uint32_t src, dst, len, pre;
};
struct Plan {  // 32 bytes, one per connection
    uint32_t nrun, out_len;
    int32_t status;
    uint32_t jobs, lines;
    uint32_t rsv[3];
};
static_assert(sizeof(Key) == 8 && sizeof(Slot) == 16 && sizeof(Job) == 16 && sizeof(Plan) == 32, "workspace layout");

// One connection: its n walked slots (ctl, sev, slot and run stand at its first slot), its region out[start .. start +
// room) of an `out` at address out_addr, its table of tcap >= 2 n entries.
struct Conn {
    uint64_t in_size, out_addr;
    const hhuff_h2_ctl_t* ctl;
    const hhuff_h2_sev_t* sev;
    uint32_t first, n;
    uint32_t start, room;
    Key* tab;
    uint32_t tcap;
    Slot* slot;
    hhuff_h2_body_run_t* run;
};

// Client streams are odd and consecutive, pushed ones even: half the id spreads a step's streams evenly.
HHUFF_CTL_HD uint32_t home(uint32_t id, uint32_t tcap) { return (id >> 1) % tcap; }

// The entry of stream id (found), or the free entry where it belongs.  At most tcap / 2 entries are taken, so a probe
// meets a free one; the loop is bounded by the table whatever it holds.
HHUFF_CTL_HD uint32_t probe(const Key* tab, uint32_t tcap, uint32_t id, bool& found) {
    uint32_t i = home(id, tcap);
    found = false;
    for (uint32_t k = 0; k < tcap; ++k) {
        const uint32_t s = tab[i].stream_id;
        if (s == id) {
            found = true;
            break;
        }
        if (s == 0) break;
        i = i + 1u == tcap ? 0u : i + 1u;
    }
    return i;
}

// The stream of the slot before stays in registers with its run record (cur, R): frames of one stream in a row need no
// lookup and no load of the record, and the next slot's event and control record are loaded a slot ahead, so a long
// upload on one stream is not a chain of dependent loads.
HHUFF_CTL_HD Plan walk(const Conn& C) {
    Plan P{0, 0, 0, 0, 0, {0, 0, 0}};
    for (uint32_t i = 0; i < C.tcap; ++i) C.tab[i] = Key{0, 0};
    uint64_t total = 0;
    uint32_t nrun = 0, cur = kNone;
    hhuff_h2_body_run_t R{0, 0, 0, 0, 0, 0, {0, 0}};
    hhuff_h2_sev_t next{0, 0, 0, 0, 0};
    uint32_t next_src = 0;
    if (C.n != 0) next = C.sev[0], next_src = C.ctl[0].a;
    for (uint32_t i = 0; i < C.n; ++i) {
        const hhuff_h2_sev_t e = next;
        const uint32_t src = e.a != 0 ? next_src : 0u;  // (with a == 0 the control record is not looked at)
        if (i + 1u < C.n) next = C.sev[i + 1u], next_src = C.ctl[i + 1u].a;
        const bool body = (e.flags & HHUFF_H2SE_BODY) != 0;
        Slot S{kNone, 0, 0, 0};
        if (body && e.stream_id == 0) P.status = HHUFF_H2BD_EINVAL;
        if (P.status == 0 && e.stream_id != 0 && (e.flags & (HHUFF_H2SE_BODY | HHUFF_H2SE_REQUEST_COMPLETE | kReset)) != 0) {
            bool opened = false;
            if (cur == kNone || R.stream_id != e.stream_id) {
                bool found;
                const uint32_t t = probe(C.tab, C.tcap, e.stream_id, found);
                uint32_t k = found ? C.tab[t].run : kNone;
                if (!found && body) {  // the stream's first BODY slot opens its run
                    C.tab[t] = Key{e.stream_id, nrun};
                    k = nrun++, opened = true;
                }
                if (k < nrun) {  // (always, unless two connections were given the same slots)
                    if (cur != kNone) C.run[cur] = R;
                    cur = k;
                    R = opened ? hhuff_h2_body_run_t{e.stream_id, 0, 0, 0, C.first + i, 0, {0, 0}} : C.run[k];
                    R.stream_id = e.stream_id;
                }
            }
            if (cur != kNone && R.stream_id == e.stream_id) {
                if (body) {
                    if ((uint64_t)src + e.a > C.in_size) P.status = HHUFF_H2BD_EINVAL;
                    S = Slot{cur, R.len, src, e.a};
                    R.len += e.a, ++R.nframes, total += e.a;
                }
                if ((e.flags & HHUFF_H2SE_REQUEST_COMPLETE) != 0) R.flags |= HHUFF_H2BR_COMPLETE;
                if ((e.flags & kReset) != 0 && !opened) R.flags |= HHUFF_H2BR_RESET;
            }
        }
        if (P.status != 0) return P;
        C.slot[i] = S;
    }
    if (cur != kNone) C.run[cur] = R;
    if (total > C.room) {
        P.status = HHUFF_H2BD_SPACE;
        return P;
    }
    // total <= room < 2^32: no length and no offset above has wrapped
    P.nrun = nrun, P.out_len = (uint32_t)total;
    uint32_t at = C.start;
    for (uint32_t k = 0; k < nrun; ++k) {
        C.run[k].out_off = at;
        at += C.run[k].len;
    }
    return P;
}

// The copy jobs of a connection the walk accepted, in slot order: sink.job(src, dst, len).  A job that does not lie
// inside the region (only with slots that two connections share) is dropped.
template <class Sink>
HHUFF_CTL_HD void jobs_of(const Conn& C, const Plan& P, Sink& sink) {
    if (P.status != 0 || C.n == 0) return;
    uint32_t last = kNone, base = 0;  // the run of the job before and its place: a load less for a stream's frames in a row
    Slot next = C.slot[0];
    for (uint32_t i = 0; i < C.n; ++i) {
        const Slot S = next;
        if (i + 1u < C.n) next = C.slot[i + 1u];  // (a slot ahead, as in the walk)
        if (S.run >= P.nrun || S.len == 0) continue;
        if (S.run != last) last = S.run, base = C.run[S.run].out_off;
        const uint64_t dst = (uint64_t)base + S.off;
        if (dst < C.start || dst + S.len > (uint64_t)C.start + C.room) continue;
        sink.job(S.src, (uint32_t)dst, S.len);
    }
}

struct CountSink {
    uint64_t out_addr;
    uint32_t jobs, lines;
    HHUFF_CTL_HD void job(uint32_t, uint32_t dst, uint32_t len) { ++jobs, lines += lc::lines_of(out_addr + dst, len); }
};

}  // namespace h2b
}  // namespace hhuff
#endif
