"""A plain model of include/hhuff.h (2m), written from h2o's lib/http2/cache_digests.c, golombset.h, h2o_next_token and
h2o_decode_base64url and from the header's text -- not from h2o_amd/csrc/hhuff_cdigest.h: bit strings, hashlib, lists.
tests/test_cache_digests.py and tests/test_cache_digests_host.py hold it against tests/golden/cache_digests.npz (h2o's
own answers) and the device against it."""
import hashlib
import struct

import numpy as np

UNKNOWN, NOT_CACHED, FRESH = 0, 1, 2
SPACE, EINVAL, EFORMAT = -327, -328, -329
URL_CHARS = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"
B64 = {**{ord(c): i for i, c in enumerate(URL_CHARS)}, ord("+"): 62, ord("/"): 63}


def next_token(s, cur, with_value):
    """h2o_next_token(iter, ';', ',', ..) on s[cur:] -> (cur, token) or None"""
    end = len(s)
    while cur < end and s[cur] in b" \t":
        cur += 1
    if cur == end:
        return None
    start = tend = cur
    while cur < end:
        c = s[cur]
        if c == ord(";"):
            cur += 1
            break
        if c == ord(","):
            if start == cur:
                cur += 1
                tend = cur
            break
        if with_value and c == ord("="):
            r = next_token(s, cur + 1, False)
            cur = cur + 1 if r is None else (r[0] - 1 if r[1] == b"," else r[0])
            break
        if c not in b" \t":
            tend = cur + 1
        cur += 1
    return cur, s[start:tend]


def bits_of(tok):
    """h2o_decode_base64url as a bit string, or None"""
    if len(tok) % 4 == 1 or any(c not in B64 for c in tok):
        return None
    return "".join(format(B64[c], "06b") for c in tok)[:8 * (len(tok) * 3 // 4)]


def decode_digest(tok):
    """load_digest's frame: (capacity_bits, keys) or None when h2o drops it"""
    bits = bits_of(tok)
    if bits is None or len(bits) < 10:
        return None
    nbits, pbits = int(bits[:5], 2), int(bits[5:10], 2)
    pos, nxt, keys = 10, 0, []
    while True:
        t = bits.find("1", pos)
        if t < 0 or t + 1 + pbits > len(bits):
            return nbits + pbits, keys
        key = nxt + ((t - pos) << pbits) + int("0" + bits[t + 1:t + 1 + pbits], 2)
        if key >= 1 << (nbits + pbits):
            return None
        keys.append(key)
        pos, nxt = t + 1 + pbits, key + 1


def gcs(nbits, pbits, keys, tail=""):
    """the encoder: a digest of the ascending keys, `tail` = further bits, as base64url without padding"""
    bits, nxt = format(nbits, "05b") + format(pbits, "05b"), 0
    for k in keys:
        d = k - nxt
        bits += "0" * (d >> pbits) + "1" + (format(d & ((1 << pbits) - 1), "0%db" % pbits) if pbits else "")
        nxt = k + 1
    bits += tail
    bits += "0" * (-len(bits) % 8)
    nchar = (len(bits) // 8 * 4 + 2) // 3
    bits += "0" * (6 * nchar - len(bits))
    return "".join(URL_CHARS[int(bits[i:i + 6], 2)] for i in range(0, len(bits), 6)).encode()


class Digests:
    """h2o_cache_digests_t *: present, complete, frames in load order as (capacity_bits, kind, keys)"""

    def __init__(self):
        self.peak = 16  # the image's largest size at a commit: what an append-only region must hold
        self.clear()

    def clear(self):
        self.present, self.complete, self.frames = False, False, []

    def load_header(self, value, room=None):
        """h2o_cache_digests_load_header; with `room` (the region's bytes) -> False once a commit passes it"""
        cur = 0
        while True:
            r = next_token(value, cur, False)
            if r is None:
                return True
            cur, gcs_tok = r
            reset = validators = complete = skip = False
            while True:
                r = next_token(value, cur, True)
                if r is None or r[1] == b",":
                    break
                cur = r[0]
                a = r[1].lower()
                reset, validators, complete = reset or a == b"reset", validators or a == b"validators", complete or a == b"complete"
                skip = skip or a not in (b"reset", b"validators", b"complete")
            if reset:
                self.clear()
            f = None if skip else decode_digest(gcs_tok)
            if f is not None:
                self.frames.append((f[0], int(validators), f[1]))
                self.present, self.complete = True, complete
                self.peak = max(self.peak, self.nbytes())
                if room is not None and self.nbytes() > room:
                    return False
            if r is None:
                return True
            cur = r[0]

    def nbytes(self):
        return 16 + sum(16 + 8 * len(k) for _, _, k in self.frames)

    def image(self):
        out = struct.pack("<4sHBBII", b"HHCD", 1, self.present | self.complete << 1, 0, len(self.frames), self.nbytes())
        for cap, kind, keys in self.frames:
            out += struct.pack("<BBHIQ", cap, kind, 0, len(keys), 0) + struct.pack("<%dQ" % len(keys), *keys)
        return out

    def lookup(self, kind, message):
        if not self.present:
            return UNKNOWN
        h = key_hash(message)
        if any(kd == kind and (h >> (64 - cap) if cap else h) in keys for cap, kd, keys in self.frames):
            return FRESH
        return NOT_CACHED if self.complete else UNKNOWN


def key_hash(message):
    return int.from_bytes(hashlib.sha256(message).digest()[:8], "big")


def peak(values):
    """the smallest region that holds the load of these values"""
    d = Digests()
    for v in values:
        d.load_header(v)
    return d.peak


def load(values, room):
    """hhuff_cache_digests_load for one request -> (status, image bytes; b"" under 16 bytes of room)"""
    d, status = Digests(), 0
    for v in values:
        if not d.load_header(v, room):
            d, status = Digests(), SPACE
            break
    if room < 16:
        return SPACE, b""
    return status, d.image()


def load_fixture():
    from conftest import load_golden

    g = load_golden("cache_digests")
    text = g["values"].tobytes()
    vals = [text[g["val_off"][i]:g["val_off"][i + 1]] for i in range(g["val_off"].size - 1)]
    qtext = g["urls"].tobytes()
    urls = [qtext[g["url_off"][i]:g["url_off"][i + 1]] for i in range(g["url_off"].size - 1)]
    return g, vals, urls


def check_fixture():
    """the model against what h2o recorded: per case (a list of header values loaded in order on one digests pointer)
    present, complete, the two frame counts, and by_url / by_url_and_etag of every recorded url (etag b"\"x\"")"""
    g, vals, urls = load_fixture()
    ncase = g["case_first"].size - 1
    for c in range(ncase):
        d = Digests()
        for v in vals[g["case_first"][c]:g["case_first"][c + 1]]:
            d.load_header(v)
        want = tuple(int(x) for x in g["summary"][c])
        got = (int(d.present), int(d.complete), sum(k == 0 for _, k, _ in d.frames), sum(k == 1 for _, k, _ in d.frames))
        assert got == (want if want[0] else (0, 0, 0, 0)), (c, got, want)
        if d.present:
            for u, url in enumerate(urls):
                assert d.lookup(0, url) == g["by_url"][c, u], (c, url)
                assert d.lookup(1, url + g["etag"].tobytes()) == g["by_url_etag"][c, u], (c, url)
    return ncase
