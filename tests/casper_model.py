"""A plain model of include/hhuff.h (2n), written from h2o's lib/http2/casper.c, golombset.h, h2o_decode_base64url and
h2o_base64_encode and from the header's text -- not from h2o_amd/csrc/hhuff_casper.h: hashlib, bit strings, lists.
tests/test_casper.py holds it against tests/golden/casper.npz (h2o's own answers) and the device against it."""
import hashlib

from cdigest_model import B64, URL_CHARS

INIT, CONSUME, CONSUME_FIELDS, LOOKUP, MARK, COOKIE = 1, 2, 3, 4, 5, 6
SPACE, EINVAL, EFORMAT = -330, -331, -332
NAME, ATTRS = b"h2o_casper=", b"; Path=/; Expires=Tue, 01 Jan 2030 00:00:00 GMT; Secure"


def encode(keys, rem, tail=""):
    """golombset_encode + base64url without padding; `tail` = further bits"""
    bits, nxt = "", 0
    for k in keys:
        bits += "0" * ((k - nxt) >> rem) + "1" + (format((k - nxt) & ((1 << rem) - 1), "0%db" % rem) if rem else "")
        nxt = k + 1
    bits += tail
    bits += "0" * (-len(bits) % 8)
    bits += "0" * (-len(bits) % 6)
    return "".join(URL_CHARS[int(bits[i:i + 6], 2)] for i in range(0, len(bits), 6)).encode()


def decode(value, rem):
    """consume_cookie up to the merge: the cookie's keys, or None when h2o drops it before counting"""
    if len(value) <= 11 or value[:11] != NAME:
        return None
    tok = value[11:]
    if len(tok) % 4 == 1 or any(c not in B64 for c in tok):
        return None
    bits = "".join(format(B64[c], "06b") for c in tok)[:8 * (len(tok) * 3 // 4)]
    pos, nxt, keys = 0, 0, []
    while True:
        t = bits.find("1", pos)
        if t < 0 or t + 1 + rem > len(bits):
            return keys
        keys.append(nxt + ((t - pos) << rem) + int("0" + bits[t + 1:t + 1 + rem], 2))
        if keys[-1] + 1 >= 1 << 63:
            return None  # the header's second deviation
        pos, nxt = t + 1 + rem, keys[-1] + 1


class Casper:
    """h2o_http2_casper_t with the bound max_keys (None: h2o's own, unbounded)"""

    def __init__(self, cap, rem, max_keys=None):
        self.cap, self.rem, self.max_keys, self.keys = cap, rem, max_keys, []

    def full(self, n):
        return self.max_keys is not None and n > self.max_keys

    def lookup(self, path, mark):
        """-> (status, value)"""
        key = int.from_bytes(hashlib.sha1(path).digest()[:4], "little") & ((1 << self.cap) - 1)
        if key in self.keys:
            return 0, 1
        if mark:
            if self.full(len(self.keys) + 1):
                return SPACE, 0
            self.keys = sorted(self.keys + [key])
        return 0, 0

    def consume(self, value):
        """-> (status, the keys the cookie held)"""
        keys = decode(value, self.rem)
        if keys is None or len(keys) > max(128, 1 << self.cap):
            return 0, 0
        union = sorted(set(self.keys) | set(keys))
        if self.full(len(union)):
            return SPACE, len(keys)
        self.keys = union
        return 0, len(keys)

    def cookie(self):
        return NAME + encode(self.keys, self.rem) + ATTRS if self.keys else b""


def step(conn, ops, data, room, max_keys, fields=None, cookie_token=0, start=0):
    """hhuff_casper_step for one connection: conn = a Casper or None (a slab that is not one), ops = [(kind, a, b)],
    fields = (value_off, value_len, token) -> (conn, the region's bytes, [(status, value, nkeys, at)]); at counts from `start`"""
    out, res = b"", []
    for kind, a, b in ops:
        st, value, at = 0, 0, 0
        if kind == INIT:
            if 1 <= a <= 30 and 0 <= b <= 31:
                conn = Casper(a, b, max_keys)
            else:
                st = EINVAL
        elif not INIT < kind <= COOKIE:
            st = EINVAL
        elif conn is None:
            st = EFORMAT
        elif kind == COOKIE:
            at, c = start + len(out), conn.cookie()
            if len(out) + len(c) > room:
                st = SPACE
            else:
                out, value = out + c, len(c)
        elif kind == CONSUME_FIELDS:
            if fields is None or a + b > len(fields[2]):
                st = EINVAL
            for s in range(a, a + b) if st == 0 else ():
                if fields[2][s] == cookie_token:
                    if fields[0][s] + fields[1][s] > len(data):
                        st, value = EINVAL, 0
                        break
                    st, n = conn.consume(data[fields[0][s]:fields[0][s] + fields[1][s]])
                    value += n
                    if st:
                        break
        elif a + b > len(data):
            st = EINVAL
        elif kind == CONSUME:
            st, value = conn.consume(data[a:a + b])
        else:
            st, value = conn.lookup(data[a:a + b], kind == MARK)
        res.append((st, value, len(conn.keys) if conn else 0, at))
    return conn, out, res
