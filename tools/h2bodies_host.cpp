// The request-body plan (h2o_amd/csrc/hhuff_h2bodies.h: the code the kernels run) on the host, as a stand-alone program
// to build with -fsanitize=address,undefined and run directly:
//     h2bodies_host CASES > RESULTS
// CASES: one line a connection, as tests/test_h2bodies_host.py writes them --
//     in_size start room n   n x (stream_id flags a ctl_a)
// `in` holds the tests' pattern, byte i = i * 131 + (i >> 8) + 7.  Every array is a heap block of exactly its size: the
// event and control records, the slots' and runs' workspace, the table of 2 n entries, and the region, whose address is
// `start` modulo 16 and which ends at its block's end.  h2b::walk plans the connection, h2b::jobs_of lists its jobs,
// and every job's lines are written by lc::copy_line, a lane's every 256th line as the copy kernel takes them.
// RESULTS: one line a connection --
//     status nrun out_len njobs | n x (run off) | nrun x (stream_id out_off len nframes first_frame flags) | the region in hex
// (slots, runs and region only with status 0; run -1: no BODY slot).  The program itself checks that a refused
// connection's region and the bytes around an accepted one's runs still hold 0xEE.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "hhuff_h2bodies.h"

using namespace hhuff;

static void fail(const char* what, long a, long b) {
    fprintf(stderr, "FAIL: %s (%ld, %ld)\n", what, a, b);
    exit(1);
}

template <class T>
struct Block {  // exactly n records on the heap (one, never touched, for n == 0)
    T* p;
    explicit Block(size_t n) : p((T*)malloc(n ? n * sizeof(T) : 1)) { memset(p, 0xEE, n * sizeof(T)); }
    ~Block() { free(p); }
};

struct ListSink {
    std::vector<h2b::Job> jobs;
    void job(uint32_t src, uint32_t dst, uint32_t len) { jobs.push_back(h2b::Job{src, dst, len, 0}); }
};

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: h2bodies_host CASES\n");
        return 2;
    }
    std::ifstream f(argv[1]);
    if (!f) fail("cannot open the cases", 0, 0);
    std::string line;
    long ncase = 0;
    for (; std::getline(f, line); ++ncase) {
        std::istringstream s(line);
        uint64_t in_size, start, room, n;
        if (!(s >> in_size >> start >> room >> n)) fail("a case's head", ncase, 0);
        Block<hhuff_h2_sev_t> sev(n);
        Block<hhuff_h2_ctl_t> ctl(n);
        for (uint64_t i = 0; i < n; ++i) {
            uint64_t sid, flags, a, src;
            if (!(s >> sid >> flags >> a >> src)) fail("a case's slot", ncase, (long)i);
            sev.p[i] = hhuff_h2_sev_t{(uint32_t)sid, (uint32_t)a, 0, 0, (uint32_t)flags};
            ctl.p[i] = hhuff_h2_ctl_t{(uint32_t)src, 0, 0, 0, 0, 0};
        }
        // `in`: whole dwords, as the call reads the aligned dwords that hold a payload
        const size_t in_alloc = (size_t)((in_size + 3u) & ~3ull);
        uint8_t* in = (uint8_t*)aligned_alloc(16, in_alloc ? (in_alloc + 15u) & ~(size_t)15u : 16);
        for (uint64_t i = 0; i < in_size; ++i) in[i] = (uint8_t)(i * 131u + (i >> 8) + 7u);
        const uint32_t pad = (uint32_t)(start & 15u);
        Block<uint8_t> region((size_t)pad + room);
        Block<h2b::Slot> slot(n);
        Block<hhuff_h2_body_run_t> run(n);
        Block<h2b::Key> tab(2 * n);
        const uint64_t out_addr = (uint64_t)(uintptr_t)(region.p + pad) - start;
        const h2b::Conn C{in_size, out_addr, ctl.p, sev.p, 1000u, (uint32_t)n, (uint32_t)start, (uint32_t)room,
                          tab.p, (uint32_t)(2 * n), slot.p, run.p};
        const h2b::Plan P = h2b::walk(C);
        ListSink sink;
        h2b::jobs_of(C, P, sink);
        h2b::CountSink count{out_addr, 0u, 0u};
        h2b::jobs_of(C, P, count);
        uint64_t lines = 0;
        for (const h2b::Job& J : sink.jobs) {
            if ((uint64_t)J.src + J.len > in_size) fail("a job leaves in", ncase, J.src);
            if (J.dst < start || (uint64_t)J.dst + J.len > start + P.out_len) fail("a job leaves the runs", ncase, J.dst);
            const uint64_t d0 = out_addr + J.dst, nl = lc::lines_of(d0, J.len);
            for (uint64_t lane = 0; lane < 256 && lane < nl; ++lane)
                for (uint64_t li = lane; li < nl; li += 256) lc::copy_line((uint64_t)(uintptr_t)in + J.src, d0, d0 + J.len, li);
            lines += nl;
        }
        if (count.jobs != sink.jobs.size() || count.lines != lines) fail("the counts of jobs and lines", ncase, count.lines);
        if (P.status != 0 && (P.nrun != 0 || P.out_len != 0 || !sink.jobs.empty())) fail("a refused connection has runs", ncase, P.status);
        for (uint64_t i = 0; i < (uint64_t)pad + room; ++i)
            if ((i < pad || i >= (uint64_t)pad + P.out_len) && region.p[i] != 0xEE) fail("a byte outside the runs was written", ncase, (long)i);
        printf("%d %u %u %zu |", P.status, P.nrun, P.out_len, sink.jobs.size());
        if (P.status == 0) {
            for (uint64_t i = 0; i < n; ++i) printf(" %d %u", slot.p[i].run == h2b::kNone ? -1 : (int)slot.p[i].run, slot.p[i].off);
            printf(" |");
            for (uint32_t k = 0; k < P.nrun; ++k) {
                const hhuff_h2_body_run_t& R = run.p[k];
                if (R.rsv[0] != 0 || R.rsv[1] != 0) fail("reserved words", ncase, k);
                printf(" %u %u %u %u %u %u", R.stream_id, R.out_off, R.len, R.nframes, R.first_frame - 1000u, R.flags);
            }
            printf(" | ");
            for (uint32_t i = 0; i < P.out_len; ++i) printf("%02x", region.p[pad + i]);
        }
        printf("\n");
        free(in);
    }
    fprintf(stderr, "ok: h2bodies_host, %ld connections\n", ncase);
    return 0;
}
