#!/usr/bin/env python3
"""Write tests/golden/casper.npz: what h2o's own lib/http2/casper.c answers for scripts of lookups, marks, consumed
cookies and get_cookie calls, from the real reference.

    python tools/gen_casper_fixture.py REF        REF: the h2o tree (default $H2O_REF)

lib/http2/casper.c, lib/common/string.c and lib/common/memory.c link (-ffunction-sections -Wl,--gc-sections, OpenSSL's
libcrypto for SHA-1) against the small dump program below, which is compiled in a temporary directory and removed with
it; only the .npz is written.  Data only:
  strings, str_off    the paths and cookie values (u8 blob, u32 offsets)
  case_first          u32 [ncase + 1]: case c is the ops case_first[c] .. case_first[c + 1] on one h2o_http2_casper_t
  op                  u32 [nop, 3]: kind (include/hhuff.h HHUFF_CSP_*), then capacity_bits and remainder_bits of an
                      INIT (h2o_http2_casper_create) or the string's index and 0
  ret, entries        i8, u32 [nop]: h2o_http2_casper_lookup's return value (0 for the other kinds) and
                      h2o_http2_casper_num_entries after the op
  cookies, cookie_off h2o_http2_casper_get_cookie's bytes after the op (the key vector is private; the cookie pins it),
                      taken from a replay on a fresh h2o_http2_casper_t: consume_cookie does not drop h2o's cookie_cache
  nrandom             the last `nrandom` cases are the seeded random scripts
The cases: h2o's unit test (t/00unit/lib/http2/casper.c), the name, alphabet, tail, limit and union edges, and seeded
random scripts.  No set passes 256 keys."""
import hashlib
import os
import random
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "casper.npz")
RANDOM = 48

DUMP_C = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "h2o/memory.h"
#include "h2o/string_.h"
#include "h2o/http2_casper.h"

int h2o_file_mktemp(const char *fn_template)
{
    return -1;
}

static size_t unhex(const char *s, char **out)
{
    size_t n = strcspn(s, "\r\n") / 2, k;
    *out = malloc(n + 1);
    for (k = 0; k != n; ++k) {
        unsigned v;
        sscanf(s + 2 * k, "%2x", &v);
        (*out)[k] = (char)v;
    }
    return n;
}

/* lines: "I cap rem" a new casper, "L hex" / "M hex" lookup with set 0 / 1, "C hex" consume a cookie: each prints the
   return value and the entry count; "G" prints the cookie */
int main(void)
{
    char *line = NULL, *v;
    size_t cap = 0, n, k;
    h2o_http2_casper_t *casper = NULL;
    while (getline(&line, &cap, stdin) > 0) {
        int ret = 0;
        unsigned a, b;
        h2o_iovec_t cookie;
        switch (line[0]) {
        case 'I':
            if (casper != NULL)
                h2o_http2_casper_destroy(casper);
            sscanf(line + 2, "%u %u", &a, &b);
            casper = h2o_http2_casper_create(a, b);
            break;
        case 'L':
        case 'M':
            n = unhex(line + 2, &v);
            ret = h2o_http2_casper_lookup(casper, v, n, line[0] == 'M');
            free(v);
            break;
        case 'C':
            n = unhex(line + 2, &v);
            h2o_http2_casper_consume_cookie(casper, v, n);
            free(v);
            break;
        case 'G':
            cookie = h2o_http2_casper_get_cookie(casper);
            printf("x");
            for (k = 0; k != cookie.len; ++k)
                printf("%02x", (unsigned char)cookie.base[k]);
            printf("\n");
            continue;
        }
        printf("%d %zu\n", ret, h2o_http2_casper_num_entries(casper));
    }
    return 0;
}
"""


def scripts():
    """-> [[(kind, cap, rem) or (kind, bytes)]], the number of random ones at the end"""
    import casper_model as M

    I, C, L, K, G = M.INIT, M.CONSUME, M.LOOKUP, M.MARK, M.COOKIE
    ck = lambda keys, rem, tail="": M.NAME + M.encode(keys, rem, tail)  # noqa: E731
    html, php = b"/index.html", b"/index.php"
    pkey = lambda p: int.from_bytes(hashlib.sha1(p).digest()[:4], "little") & 0x1fff  # noqa: E731
    one, two = ck([pkey(html)], 6), ck([5, 300], 6)
    cases = [
        # h2o's unit test: calc_key, lookup, cookie, cookie-merge
        [(I, 13, 6), (L, html), (K, html), (L, html), (K, html), (G,)],
        [(I, 13, 6), (G,), (K, html), (G,), (I, 13, 6), (C, one), (L, html), (L, php), (K, php), (K, html), (G,)],
        [(I, 13, 6), (C, one), (C, one), (L, html), (C, ck([pkey(php)], 6)), (L, html), (L, php)],
        # the name; a tail behind the value; foreign bytes; both alphabets
        [(I, 13, 6), (C, M.NAME), (C, b"h2o_casper"), (C, b"h2o_caspex=" + two[11:]), (C, b"H2O_CASPER=" + two[11:]), (C, two + b"; x=y"),
         (C, two + b" "), (C, two[:13] + b"*" + two[14:]), (C, b"x" + two), (G,), (C, two), (G,)],
        [(I, 10, 6), (C, M.NAME + b"-_+/"), (G,), (C, M.NAME + b"+/-_"), (G,)],
        # 2, 3, 4, 5 (a tail of 1) and 6 characters
        [(I, 13, 6)] + [x for n in (2, 3, 4, 5, 6) for x in ((C, M.NAME + ck([5, 300, 900], 6)[11:11 + n]), (G,))],
    ]
    for rem in (0, 6, 31):  # 0, 1, 63, 64, 65 keys; a value cut short
        for n in (0, 1, 63, 64, 65):
            keys = [(7 * i * i + 3 * i) << max(rem - 4, 0) for i in range(n)]
            cases.append([(I, 13, rem), (C, ck(keys, rem) if n else M.NAME + b"AAAA"), (G,), (C, ck(keys[:n // 2], rem, "1")), (G,)])
    for cap, lim in ((5, 128), (8, 256)):  # the retry loop's limit: L and L + 1 keys
        cases.append([(I, cap, 0), (C, ck(range(0, 2 * lim, 2), 0)), (G,), (I, cap, 0), (C, ck(range(0, 2 * lim + 2, 2), 0)), (G,)])
    cases.append([(I, 13, 2), (C, ck([3, 3 + (5000 << 2), 9 + (5000 << 2)], 2)), (G,)])  # a unary run across a decode round
    a, b = list(range(10, 400, 10)), list(range(5, 400, 15))
    for x, y in (([], a), (a, []), (a, a), (a, [1, 2, 3]), (a, [500, 600]), (a, b), (list(range(0, 60)), list(range(100, 110)))):
        cases.append([(I, 13, 6)] + ([(C, ck(x, 6))] if x else []) + [(G,)] + ([(C, ck(y, 6))] if y else [(C, M.NAME + b"AA")]) + [(G,)])
    rng = random.Random(23)
    paths = [b"/", b"", html, php] + [b"/assets/%d/%s.%s" % (i, b"x" * (i * 7 % 130), rng.choice([b"js", b"css", b"png"])) for i in range(40)]
    nrandom = 0
    while nrandom < RANDOM:
        cap, rem = rng.choice([5, 8, 13, 20]), rng.choice([0, 3, 6, 11])
        sc, model = [(I, cap, rem)], M.Casper(cap, rem)
        for _ in range(rng.randrange(4, 24)):
            r = rng.random()
            if r < 0.35:
                sc.append((K, rng.choice(paths)))
            elif r < 0.55:
                sc.append((L, rng.choice(paths)))
            elif r < 0.8:
                keys = sorted(rng.sample(range(1 << min(cap, 12)), rng.randrange(0, min(30, 1 << cap))))
                v = ck(keys, rem) if keys else M.NAME + b"AA"
                if rng.random() < 0.2:
                    v = v[:rng.randrange(8, len(v) + 1)]
                sc.append((C, v))
            elif r < 0.95:
                sc.append((G,))
            else:
                cap, rem = rng.choice([5, 8, 13]), rng.choice([0, 6])
                sc.append((I, cap, rem))
                model = M.Casper(cap, rem)
            if sc[-1][0] in (K, L):
                model.lookup(sc[-1][1], sc[-1][0] == K)
            elif sc[-1][0] == C:
                model.consume(sc[-1][1])
        if len(model.keys) <= 200:
            cases.append(sc + [(G,)])
            nrandom += 1
    return cases, nrandom


def main():
    import casper_model as M

    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("H2O_REF", "")
    srcs = [os.path.join(ref, "lib", *p) for p in (("http2", "casper.c"), ("common", "string.c"), ("common", "memory.c"))]
    if not all(os.path.exists(s) for s in srcs):
        sys.exit("no h2o tree at %r (lib/http2/casper.c)" % ref)
    cases, nrandom = scripts()
    inc = [os.path.join(ref, "include")] + [os.path.join(ref, "deps", d) for d in (
        "picotls/include", "quicly/include", "klib", "golombset", "cloexec", "yoml", "libgkc", "libyrmcds", "picohttpparser",
        "hiredis", "brotli/c/include")]
    # h2o_http2_casper_consume_cookie leaves casper->cookie_cache as it was, so a get_cookie in front of it would make
    # the next one stale.  The cookie is a function of the set: every op's answers come from a replay of the ops since
    # the last INIT on a fresh h2o_http2_casper_t, with one get_cookie at the end.
    strings, index, ops, feed, nlines = [], {}, [], "", []
    letter = {M.LOOKUP: "L", M.MARK: "M", M.CONSUME: "C"}
    for sc in cases:
        since = ""
        for op in sc:
            if op[0] == M.INIT:
                ops.append(op)
                since = "I %d %d\n" % op[1:]
            elif op[0] == M.COOKIE:
                ops.append((op[0], 0, 0))
            else:
                k = index.setdefault(op[1], len(strings))
                if k == len(strings):
                    strings.append(op[1])
                ops.append((op[0], k, 0))
                since += "%s %s\n" % (letter[op[0]], op[1].hex())
            feed += since + "G\n"
            nlines.append(since.count("\n") + 1)
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "dump_casper.c"), os.path.join(tmp, "dump_casper")
        with open(src, "w") as f:
            f.write(DUMP_C)
        subprocess.run(["gcc", "-O1", "-w", "-DH2O_USE_LIBUV=0", "-ffunction-sections", "-fdata-sections"] + ["-I" + d for d in inc] +
                       [src] + srcs + ["-Wl,--gc-sections", "-lcrypto", "-lpthread", "-o", exe], check=True)
        lines = [r for r in subprocess.run([exe], input=feed, check=True, capture_output=True, text=True).stdout.split("\n") if r]
    assert len(lines) == sum(nlines), (len(lines), sum(nlines))
    ends = np.cumsum(nlines)
    rows = [lines[e - 2].split() + [lines[e - 1]] for e in ends]
    for o, op in enumerate(ops):  # (a COOKIE op's return value is 0; its entry count is the op's before)
        if op[0] == M.COOKIE:
            rows[o][0] = "0"
    cookies = [bytes.fromhex(r[2][1:]) for r in rows]
    pack = lambda ss: (np.frombuffer(b"".join(ss), np.uint8).copy(),  # noqa: E731
                       np.concatenate([[0], np.cumsum([len(s) for s in ss])]).astype(np.uint32))
    sblob, soff = pack(strings)
    cblob, coff = pack(cookies)
    first = np.concatenate([[0], np.cumsum([len(sc) for sc in cases])]).astype(np.uint32)
    np.savez_compressed(OUT, strings=sblob, str_off=soff, case_first=first, op=np.array(ops, np.uint32),
                        ret=np.array([int(r[0]) for r in rows], np.int8), entries=np.array([int(r[1]) for r in rows], np.uint32),
                        cookies=cblob, cookie_off=coff, nrandom=np.array(nrandom, np.uint32))
    print("%s: %d cases (%d random), %d ops, %d strings, at most %d entries; %d bytes" % (
        os.path.relpath(OUT, ROOT), len(cases), nrandom, len(ops), len(strings), max(int(r[1]) for r in rows), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
