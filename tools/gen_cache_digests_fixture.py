#!/usr/bin/env python3
"""Write tests/golden/cache_digests.npz: what h2o's own lib/http2/cache_digests.c answers for lists of `cache-digest`
header values, from the real reference.

    python tools/gen_cache_digests_fixture.py REF        REF: the h2o tree (default $H2O_REF)

lib/http2/cache_digests.c, lib/common/string.c and lib/common/memory.c link (-ffunction-sections -Wl,--gc-sections,
OpenSSL's libcrypto for SHA-256) against the small dump program below, which is compiled in a temporary directory and
removed with it; only the .npz is written.  Data only:
  values, val_off     the header values (u8 blob, u32 offsets)
  case_first          u32 [ncase + 1]: case c loads the values case_first[c] .. case_first[c + 1] in order, by
                      h2o_cache_digests_load_header on one h2o_cache_digests_t * that starts NULL
  summary             u8 [ncase, 4]: digests != NULL, fresh.complete, fresh.url_only.size, fresh.url_and_etag.size (zeros
                      where digests == NULL)
  urls, url_off, etag the probe URLs and the one ETag
  by_url, by_url_etag i8 [ncase, nurl]: h2o_cache_digests_lookup_by_url(url) and _by_url_and_etag(url, etag), 0 where
                      digests == NULL (h2o's callers do not look then)
The frame struct is private to cache_digests.c, so the keys are not recorded: tests/cdigest_model.py pins them and is
held against this file.  The cases: h2o's unit test, hand-written walk and alphabet edges, digests that hold chosen
probe URLs, and seeded random compositions of such pieces."""
import os
import random
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "cache_digests.npz")
RANDOM = 300
ETAG = b'"x"'

DUMP_C = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "h2o/memory.h"
#include "h2o/string_.h"
#include "h2o/cache_digests.h"

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

/* lines: "U hex" a probe url, "E hex" the etag, "C" a new case, "V hex" load a value, "Q" print the case */
int main(void)
{
    char *line = NULL, *urls[64], *etag = NULL, *v;
    size_t cap = 0, url_len[64], nurl = 0, etag_len = 0, n, u;
    h2o_cache_digests_t *digests = NULL;
    while (getline(&line, &cap, stdin) > 0) {
        switch (line[0]) {
        case 'U':
            url_len[nurl] = unhex(line + 2, &urls[nurl]);
            ++nurl;
            break;
        case 'E':
            etag_len = unhex(line + 2, &etag);
            break;
        case 'C':
            if (digests != NULL)
                h2o_cache_digests_destroy(digests);
            digests = NULL;
            break;
        case 'V':
            n = unhex(line + 2, &v);
            h2o_cache_digests_load_header(&digests, v, n);
            free(v);
            break;
        case 'Q':
            if (digests == NULL) {
                printf("0 0 0 0");
                for (u = 0; u != nurl; ++u)
                    printf(" 0 0");
            } else {
                printf("1 %d %zu %zu", digests->fresh.complete, digests->fresh.url_only.size, digests->fresh.url_and_etag.size);
                for (u = 0; u != nurl; ++u)
                    printf(" %d %d", (int)h2o_cache_digests_lookup_by_url(digests, urls[u], url_len[u]),
                           (int)h2o_cache_digests_lookup_by_url_and_etag(digests, urls[u], url_len[u], etag, etag_len));
            }
            printf("\n");
            break;
        }
    }
    return 0;
}
"""


def cases_and_urls():
    import cdigest_model as M

    base = b"https://127.0.0.1.xip.io:8081/"
    urls = [base + b"cache-digests.cgi/hello.js", base + b"notfound.js"] + [b"https://a.example/%d.css" % i for i in range(10)]
    key = lambda m, cap: M.key_hash(m) >> (64 - cap)  # noqa: E731
    own = [M.gcs(nb, pb, sorted({key(u, nb + pb) for u in us})) for nb, pb, us in (
        (5, 7, urls[2:5]), (10, 10, urls[4:9]), (1, 31, urls[2:4]), (8, 0, urls[5:7]), (9, 20, urls[9:12]))]
    own_etag = [M.gcs(6, 9, sorted({key(u + ETAG, 15) for u in urls[3:8]})), M.gcs(0, 7, [key(urls[0] + ETAG, 7)])]
    unit = [b"AeLA", b"FOO; stale, AcA; validators; complete", b"AcA; reset"]
    cases = [unit[:1], unit[:2], unit, [b""], [b" \t "], [b","], [b",AeLA"], [b"AeLA,,AcA"], [b"AeLA; ReSeT"], [b"AeLA; foo"],
             [b"AeLA; a=b"], [b"AeLA;complete = x , AcA ; validators;a=,AeLA;complete"], [b"AeLA; a=,AcA;complete"],
             [b"AeLA,A*LA;complete,AcA"], [b"AeL A;complete"], [b"AeLAA"], [b"Ke+/gA;validators, Ke-_gA;COMPLETE"], [b"AeLA=;complete"],
             [b"AeLA; complete", M.gcs(2, 1, [3, 8]) + b"; complete; reset"], [b"AeLA", M.gcs(2, 1, [3, 7]) + b"; complete"],
             [b"AeLA; complete", b"AcA; reset; validators"], [M.gcs(31, 31, [0, 2 ** 33 + 5]) + b";complete"],
             [b"Ae", b"AeL", b"AeLA-_"], [b"\x80eLA, AeLA"], [b"AeLA ;\tcomplete\t; validators , AcA;;complete"]]
    cases += [[d + b"; complete"] for d in own] + [[d + b"; validators"] for d in own_etag]
    cases += [[own[0], own_etag[0] + b";validators;complete"], [own[1] + b"," + own[2] + b";complete", own[3] + b"; reset"]]
    rng = random.Random(17)
    pieces = own + own_etag + [b"AeLA", b"AcA", b"FOO", b"A*LA", b"", b"Ke+/gA", b"AeLAA", M.gcs(2, 1, [3, 8])]
    attrs = [b"reset", b"validators", b"complete", b"Complete", b"RESET", b"stale", b"a=b", b"a=", b"=b", b"complete=1", b"", b" "]
    seps = [b",", b", ", b" ,", b";", b",,", b", ,"]
    for _ in range(RANDOM):
        vals = []
        for _ in range(rng.randrange(1, 4)):
            v = b""
            for _ in range(rng.randrange(1, 4)):
                v += rng.choice(pieces) + b"".join(rng.choice([b";", b"; ", b" ;"]) + rng.choice(attrs) for _ in range(rng.randrange(0, 3)))
                v += rng.choice(seps)
            vals.append(v[:len(v) - rng.randrange(0, 3)])
        cases.append(vals)
    return cases, urls


def pack(strings):
    off = np.zeros(len(strings) + 1, np.uint32)
    off[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
    return np.frombuffer(b"".join(strings), np.uint8).copy(), off


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("H2O_REF", "")
    srcs = [os.path.join(ref, "lib", *p) for p in (("http2", "cache_digests.c"), ("common", "string.c"), ("common", "memory.c"))]
    if not all(os.path.exists(s) for s in srcs):
        sys.exit("no h2o tree at %r (lib/http2/cache_digests.c)" % ref)
    cases, urls = cases_and_urls()
    inc = [os.path.join(ref, "include")] + [os.path.join(ref, "deps", d) for d in (
        "picotls/include", "quicly/include", "klib", "golombset", "cloexec", "yoml", "libgkc", "libyrmcds", "picohttpparser",
        "hiredis", "brotli/c/include")]
    feed = "".join("U %s\n" % u.hex() for u in urls) + "E %s\n" % ETAG.hex()
    for vals in cases:
        feed += "C\n" + "".join("V %s\n" % v.hex() for v in vals) + "Q\n"
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "dump_cdigest.c"), os.path.join(tmp, "dump_cdigest")
        with open(src, "w") as f:
            f.write(DUMP_C)
        subprocess.run(["gcc", "-O1", "-w", "-DH2O_USE_LIBUV=0", "-ffunction-sections", "-fdata-sections"] + ["-I" + d for d in inc] +
                       [src] + srcs + ["-Wl,--gc-sections", "-lcrypto", "-lpthread", "-o", exe], check=True)
        lines = [r for r in subprocess.run([exe], input=feed, check=True, capture_output=True, text=True).stdout.split("\n") if r]
    assert len(lines) == len(cases), (len(lines), len(cases))
    rows = np.array([[int(x) for x in r.split()] for r in lines], np.int64)
    vblob, voff = pack([v for vals in cases for v in vals])
    ublob, uoff = pack(urls)
    first = np.concatenate([[0], np.cumsum([len(v) for v in cases])]).astype(np.uint32)
    np.savez_compressed(OUT, values=vblob, val_off=voff, case_first=first, summary=rows[:, :4].astype(np.uint8), urls=ublob,
                        url_off=uoff, etag=np.frombuffer(ETAG, np.uint8), by_url=rows[:, 4::2].astype(np.int8),
                        by_url_etag=rows[:, 5::2].astype(np.int8))
    print("%s: %d cases (%d present, %d complete), %d urls, states %s; %d bytes" % (
        os.path.relpath(OUT, ROOT), len(cases), int(rows[:, 0].sum()), int(rows[:, 1].sum()), len(urls),
        np.bincount(rows[:, 4:].ravel(), minlength=3).tolist(), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
