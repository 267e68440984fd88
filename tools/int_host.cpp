// The prefix integer of the header decoders (h2o_amd/csrc/hhuff_int.h: the code the kernels run) on the host, as a
// stand-alone program to build with -fsanitize=address,undefined and run directly:
//     int_host CASES
// CASES: one line a case -- prefix_bits, then the bytes in hex ("-": none) -- as tests/test_int_host.py writes them.
// Every case is decoded in a heap block of exactly its size (a read past it is a heap overflow) and answered with one
// line: the value or the negative error, and the bytes consumed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hhuff_int.h"

int main(int argc, char** argv) {
    if (argc < 2) return printf("usage: int_host CASES\n"), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return printf("cannot read %s\n", argv[1]), 2;
    char* line = nullptr;
    size_t cap = 0, cases = 0;
    while (getline(&line, &cap, f) > 0) {
        unsigned prefix = 0;
        int at = 0;
        if (sscanf(line, "%u %n", &prefix, &at) < 1 || prefix < 1 || prefix > 8) return printf("bad line %zu\n", cases), 2;
        std::vector<uint8_t> bytes;
        const char* hex = line + at;
        if (*hex != '-') {
            auto nib = [](char ch) { return (uint8_t)(ch <= '9' ? ch - '0' : ch - 'a' + 10); };
            for (; hex[0] > ' ' && hex[1] > ' '; hex += 2) bytes.push_back((uint8_t)(nib(hex[0]) << 4 | nib(hex[1])));
        }
        const size_t len = bytes.size();
        uint8_t* p = (uint8_t*)malloc(len ? len : 1);
        if (len) memcpy(p, bytes.data(), len);
        uint64_t pos = 0;
        const int64_t v = hhuff::hpack_int(len ? p : p + 1, pos, len, prefix);
        printf("%lld %llu\n", (long long)v, (unsigned long long)pos);
        free(p);
        ++cases;
    }
    free(line);
    fclose(f);
    printf("ok: int_host %zu\n", cases);
    return 0;
}
