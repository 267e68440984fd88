// The arithmetic of the host-array batch paths (h2o_amd/csrc/hhuff_hostplan.h: the code the library runs) on the
// host, as a stand-alone program to build with -fsanitize=address,undefined and run directly:
//     hostplan_host CASES
// CASES: one line a case, as tests/test_hostplan_host.py writes them; every case is answered with one line.
//     cuts N CHUNK off[N + 1]                    -> the cuts of chunk_cuts
//     plan OP NAMES N CHUNK off[N + 1]           -> per chunk "i0 i1 m s0 e0 base nbytes olo ohi obase ocap nw o_off
//                                                   o_nm o_out o_len o_st need", chunks separated by ";"
//     runs OP N off[N + 1] out_off[N + 1] out_len[N]  -> "lo hi" of every tile
//     shard N NS ALIGN off[N + 1]                -> the NS + 1 bounds of shard_bound
//     implicit OP IN_SIZE IN_END OUT_SIZE        -> "ok" or the refusal text
// OP: d (decode) or e (encode); NAMES: 0 or 1.  Every array lives in a heap block of exactly its size, so a read
// past it is a heap overflow.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "hhuff_hostplan.h"

namespace {
// the next `count` numbers of the line, in a heap block of exactly count entries
uint32_t* take(std::istringstream& in, size_t count) {
    uint32_t* p = (uint32_t*)malloc(count ? count * sizeof(uint32_t) : 1);
    for (size_t i = 0; i < count; ++i) {
        unsigned long long v = 0;
        if (!(in >> v) || v > 0xFFFFFFFFull) return free(p), nullptr;
        p[i] = (uint32_t)v;
    }
    return p;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return printf("usage: hostplan_host CASES\n"), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return printf("cannot read %s\n", argv[1]), 2;
    char* line = nullptr;
    size_t cap = 0, cases = 0;
    while (getline(&line, &cap, f) > 0) {
        std::istringstream in(line);
        std::string kind, op;
        in >> kind;
        if (kind == "cuts" || kind == "plan") {
            unsigned long long n = 0, chunk = 0;
            int names = 0;
            if (kind == "plan") in >> op >> names;
            in >> n >> chunk;
            uint32_t* off = take(in, n + 1);
            if (!off || n == 0) return printf("bad line %zu\n", cases), 2;
            const std::vector<uint64_t> cut = hhuff::chunk_cuts(off, n, chunk);
            if (kind == "cuts") {
                for (uint64_t c : cut) printf("%llu ", (unsigned long long)c);
            } else {
                for (size_t k = 0; k + 1 < cut.size(); ++k) {
                    const uint64_t i0 = cut[k], i1 = cut[k + 1], m = i1 - i0, s0 = off[i0], e0 = off[i1];
                    const hhuff::ChunkLayout L = hhuff::chunk_layout(op == "d", s0, e0, m, names != 0);
                    const unsigned long long v[] = {i0, i1, m, s0, e0, L.base, L.nbytes, L.olo, L.ohi, L.obase, L.ocap, L.nw,
                                                    L.o_off, L.o_nm, L.o_out, L.o_len, L.o_st, L.need};
                    for (unsigned long long x : v) printf("%llu ", x);
                    printf("; ");
                }
            }
            printf("\n");
            free(off);
        } else if (kind == "runs") {
            unsigned long long n = 0;
            in >> op >> n;
            uint32_t* off = take(in, n + 1);
            uint32_t* ooff = take(in, n + 1);
            uint32_t* olen = take(in, n);
            if (!off || !ooff || !olen || n == 0) return printf("bad line %zu\n", cases), 2;
            for (uint32_t t = 0; t < hhuff::packed_ntiles((uint32_t)n); ++t)
                printf("%llu %llu ", (unsigned long long)hhuff::run_lo(op == "d", off, t),
                       (unsigned long long)hhuff::run_hi((uint32_t)n, ooff, olen, t));
            printf("\n");
            free(off), free(ooff), free(olen);
        } else if (kind == "shard") {
            unsigned long long n = 0, ns = 0, align = 0;
            in >> n >> ns >> align;
            uint32_t* off = take(in, n + 1);
            if (!off) return printf("bad line %zu\n", cases), 2;
            for (uint32_t k = 0; k <= ns; ++k)
                printf("%u ", hhuff::shard_bound(off, (uint32_t)n, k, (uint32_t)ns, (uint32_t)align));
            printf("\n");
            free(off);
        } else if (kind == "implicit") {
            unsigned long long in_size = 0, in_end = 0, out_size = 0;
            in >> op >> in_size >> in_end >> out_size;
            const char* bad = hhuff::implicit_refusal(op == "d", in_size, in_end, out_size);
            printf("%s\n", bad ? bad : "ok");
        } else {
            return printf("bad line %zu\n", cases), 2;
        }
        ++cases;
    }
    free(line);
    fclose(f);
    printf("ok: hostplan_host %zu\n", cases);
    return 0;
}
