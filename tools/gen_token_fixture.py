#!/usr/bin/env python3
"""Write tests/golden/tokens.npz: h2o's token list and h2o_lookup_token's own answers, from the real reference.

    python tools/gen_token_fixture.py [REF]        REF: the h2o tree (default $H2O_REF or /root/reference)

lib/common/token.c (h2o__tokens[], h2o_lookup_token) links on its own against the small dump program below, which
is compiled in a temporary directory and removed with it; only the .npz is written.  Data only:
  names, name_off   the names in h2o__tokens[] order, back to back (u8 blob, u32 offsets [ntokens + 1])
  flags             i16 [ntokens, 8]: h2o_token_flags_t in declaration order (FLAGS)
  probes, probe_off the probe strings (u8 blob, u32 offsets [nprobes + 1])
  answer            i32 [nprobes]: h2o_lookup_token(probe) - h2o__tokens, -1 for NULL
The probes: every token name; every name with one byte changed (at every position), one byte dropped (at every
position) and one byte appended; every name upper-cased; every proper prefix of at least one byte; and RANDOM random
lower-case strings of 1..40 bytes (seeded).
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "tokens.npz")
FLAGS = ("http2_static_table_name_index", "proxy_should_drop_for_req", "proxy_should_drop_for_res",
         "is_init_header_special", "is_hpack_special", "copy_for_push_request", "dont_compress", "likely_to_repeat")
RANDOM = 400

DUMP_C = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "h2o/token.h"

/* "tokens": one line per token, the name in hex and the eight flags.
 * "lookup": one hex string per input line -> one line with the token's index, or -1. */
int main(int argc, char **argv)
{
    size_t i, k;
    if (argc > 1 && strcmp(argv[1], "tokens") == 0) {
        for (i = 0; i != h2o__num_tokens; ++i) {
            const h2o_token_t *t = h2o__tokens + i;
            for (k = 0; k != t->buf.len; ++k)
                printf("%02x", (unsigned char)t->buf.base[k]);
            printf(" %d %d %d %d %d %d %d %d\n", (int)t->flags.http2_static_table_name_index,
                   (int)t->flags.proxy_should_drop_for_req, (int)t->flags.proxy_should_drop_for_res,
                   (int)t->flags.is_init_header_special, (int)t->flags.is_hpack_special,
                   (int)t->flags.copy_for_push_request, (int)t->flags.dont_compress, (int)t->flags.likely_to_repeat);
        }
        return 0;
    }
    {
        static char line[4096], name[2048];
        while (fgets(line, sizeof(line), stdin) != NULL) {
            size_t n = strcspn(line, "\r\n") / 2;
            const h2o_token_t *t;
            for (k = 0; k != n; ++k) {
                unsigned v;
                sscanf(line + 2 * k, "%2x", &v);
                name[k] = (char)v;
            }
            t = h2o_lookup_token(name, n);
            printf("%ld\n", t != NULL ? (long)(t - h2o__tokens) : -1L);
        }
    }
    return 0;
}
"""


def probe_list(names, seed=20):
    rng = np.random.default_rng(seed)
    out = list(names)
    for nm in names:
        for i in range(len(nm)):
            c = nm[i]
            d = (c + 1 + int(rng.integers(0, 255))) % 256  # any other byte
            out.append(nm[:i] + bytes([d]) + nm[i + 1:])
        for i in range(len(nm)):
            if len(nm) > 1:
                out.append(nm[:i] + nm[i + 1:])
        out.append(nm + bytes([int(rng.integers(0, 256))]))
    out += [nm.upper() for nm in names]
    for nm in names:
        out += [nm[:k] for k in range(1, len(nm))]
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz-", np.uint8)
    for _ in range(RANDOM):
        out.append(bytes(rng.choice(alpha, int(rng.integers(1, 41)))))
    return out


def pack(strings):
    off = np.zeros(len(strings) + 1, np.uint32)
    off[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
    return np.frombuffer(b"".join(strings), np.uint8).copy(), off


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("H2O_REF", "/root/reference")
    token_c = os.path.join(ref, "lib", "common", "token.c")
    if not os.path.exists(token_c):
        sys.exit("no h2o tree at %s (lib/common/token.c)" % ref)
    inc = [os.path.join(ref, "include")] + [os.path.join(ref, "deps", d) for d in ("picotls/include", "quicly/include", "klib",
                                                                                   "golombset")]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "dump_tokens.c"), os.path.join(tmp, "dump_tokens")
        with open(src, "w") as f:
            f.write(DUMP_C)
        subprocess.run(["gcc", "-O1", "-w", src, token_c, "-I" + os.path.dirname(token_c)] + ["-I" + d for d in inc] + ["-o", exe],
                       check=True)
        lines = subprocess.run([exe, "tokens"], check=True, capture_output=True, text=True).stdout.split("\n")
        rows = [ln.split() for ln in lines if ln]
        names = [bytes.fromhex(r[0]) for r in rows]
        flags = np.array([[int(x) for x in r[1:]] for r in rows], np.int16)
        probes = probe_list(names)
        feed = "".join(p.hex() + "\n" for p in probes)
        ans = subprocess.run([exe, "lookup"], input=feed, check=True, capture_output=True, text=True).stdout.split()
    answer = np.array([int(a) for a in ans], np.int32)
    assert answer.size == len(probes) and flags.shape == (len(names), len(FLAGS))
    nblob, noff = pack(names)
    pblob, poff = pack(probes)
    np.savez_compressed(OUT, names=nblob, name_off=noff, flags=flags, probes=pblob, probe_off=poff, answer=answer)
    print("%s: %d tokens (%d name bytes, longest %d), %d probes, %d hits"
          % (os.path.relpath(OUT, ROOT), len(names), nblob.size, max(len(n) for n in names), len(probes), int((answer >= 0).sum())))


if __name__ == "__main__":
    main()
