"""An independent reference for h2o_hpack_decode_huffman (lib/http2/hpack.c:117-156): a bit-by-bit walk of the code
tree built from h2o_amd.tables.ENC_CODE / ENC_NBITS (tests/test_tables.py checks those entry for entry).  No
nibble FSM, no window LUT, nothing of the oracle's: the decoders' edge tests (tests/test_decode_edges*.py) compare
with this file, and tests/test_decode_edges_host.py compares this file with the oracle.

  walk(src)             -> Walk: the symbols, the bit offset at which each starts, where the walk stopped and why
  decode(src, is_name)  -> (bytes | None, status): status is the batch API's byte -- 0x80 for a string that fails,
                           else the soft bits (0x1 name, 0x2 value)
  encode(src)           -> bytes | None: h2o_hpack_encode_huffman (hpack.c:774-804) from the same two tables, code
                           after code on a bit string; None where the call returns SIZE_MAX (tests/encode_edges.py's
                           corpus and plans compare with it, tests/test_encode_edges_host.py compares it with the
                           oracle and the golden encode vectors)

`src` is a bytes object or a str of '0' / '1' (any number of bits: the generators and the models of
tests/decode_edges.py walk bit strings that are no whole bytes yet)."""
import collections

from h2o_amd import tables

STATUS_FAIL = 0x80
SOFT_NAME, SOFT_VALUE = 0x1, 0x2
EOS = 256

# The bytes hpack.c flags while decoding (its table's INVALID_HEADER_NAME / _VALUE bits), as inclusive ranges.
# test_decode_edges_host.py::test_invalid_sets_match_the_oracle pins both against the oracle, byte by byte.
NAME_INVALID_RANGES = ((0x00, 0x20), (0x22, 0x22), (0x28, 0x29), (0x2C, 0x2C), (0x2F, 0x2F), (0x3A, 0x5D),
                       (0x7B, 0x7B), (0x7D, 0x7D), (0x7F, 0xFF))
VALUE_INVALID_RANGES = ((0x00, 0x08), (0x0A, 0x1F), (0x7F, 0x7F))


def _set(ranges):
    return frozenset(b for lo, hi in ranges for b in range(lo, hi + 1))


NAME_INVALID = _set(NAME_INVALID_RANGES)
VALUE_INVALID = _set(VALUE_INVALID_RANGES)

Walk = collections.namedtuple("Walk", "syms starts stop nbits eos")
# syms: the decoded bytes; starts[k]: the bit at which symbol k's code begins; stop: the bit at which the walk
# stopped -- the start of the EOS code (eos = True), or of the code the string's end cuts (stop == nbits: none)


def _tree():
    """flat binary tree: child of node v by bit b at nxt[2 v + b]; a leaf is ~symbol (negative)"""
    nxt = [0, 0]
    codes = list(zip(tables.ENC_CODE, tables.ENC_NBITS)) + [(tables.EOS_CODE, tables.EOS_NBITS)]
    for sym, (code, nbits) in enumerate(codes):
        v = 0
        for j in range(nbits - 1, -1, -1):
            b = (code >> j) & 1
            if j == 0:
                assert nxt[2 * v + b] == 0, "not a prefix code"
                nxt[2 * v + b] = ~sym
            else:
                if nxt[2 * v + b] == 0:
                    nxt[2 * v + b] = len(nxt) // 2
                    nxt += [0, 0]
                v = nxt[2 * v + b]
                assert v > 0, "not a prefix code"
    assert 0 not in nxt[2:], "the code is complete (RFC 7541 Appendix B)"
    return nxt


_NXT = _tree()
_BYTE_BITS = [tuple((b >> (7 - j)) & 1 for j in range(8)) for b in range(256)]


def bits_of(src):
    """the bits of `src` as a list of 0 / 1"""
    if isinstance(src, str):
        return [1 if c == "1" else 0 for c in src]
    out = []
    for b in bytes(src):
        out += _BYTE_BITS[b]
    return out


def walk(src):
    nxt = _NXT
    syms, starts = bytearray(), []
    v, start = 0, 0
    for p, b in enumerate(bits_of(src)):
        v = nxt[2 * v + b]
        if v < 0:
            if v == ~EOS:
                return Walk(bytes(syms), starts, start, _nbits(src), True)
            syms.append(~v)
            starts.append(start)
            v, start = 0, p + 1
    return Walk(bytes(syms), starts, start, _nbits(src), False)


def _nbits(src):
    return len(src) if isinstance(src, str) else 8 * len(src)


def padding_ok(src, stop):
    """hpack.c:132-133: what is left behind the last whole code is at most 7 bits, all ones"""
    rest = bits_of(src)[stop:] if stop < _nbits(src) else []
    return len(rest) <= 7 and all(rest)


def soft_bits(out, is_name):
    """hpack.c:134-153 on the decoded bytes"""
    if is_name:
        if len(out) == 0 or (out[0] != 0x3A and any(b in NAME_INVALID for b in out)):
            return SOFT_NAME
        return 0
    if any(b in VALUE_INVALID for b in out) or (len(out) and (out[0] in (0x20, 0x09) or out[-1] in (0x20, 0x09))):
        return SOFT_VALUE
    return 0


def verdict(src, w, is_name):
    """the result for a string whose walk is `w`"""
    if w.eos or not padding_ok(src, w.stop):
        return None, STATUS_FAIL
    return w.syms, soft_bits(w.syms, is_name)


def decode(src, is_name=False):
    return verdict(src, walk(src), is_name)


def symbol_starts(src):
    return walk(src).starts


# every symbol's code as a string of '0' / '1', MSB first (RFC 7541 Appendix B)
_CODE_BITS = ["".join("1" if (c >> j) & 1 else "0" for j in range(n - 1, -1, -1))
              for c, n in zip(tables.ENC_CODE, tables.ENC_NBITS)]


def code_bits(src):
    """the codes of the bytes of `src`, one after another, as a string of '0' / '1'"""
    return "".join(map(_CODE_BITS.__getitem__, bytes(src)))


def encode(src):
    """h2o_hpack_encode_huffman (lib/http2/hpack.c:774-804) on the bit string: the codes MSB first, the last byte
    filled with ones, and None (the call's SIZE_MAX) when the code needs more than len - 1 bytes -- also for len 0"""
    bits = code_bits(src)
    nbytes = (len(bits) + 7) // 8
    if nbytes > len(src) - 1:
        return None
    bits += "1" * (8 * nbytes - len(bits))
    return bytes(int(bits[p:p + 8], 2) for p in range(0, len(bits), 8))
