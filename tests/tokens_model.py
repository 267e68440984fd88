"""The plain-Python model of include/hhuff.h (2j): a dict from name to token id, the slot rule of
hhuff_intern_fields and the flag rule of hhuff_intern_headers.  No GPU, no library."""
import os

import numpy as np

TOK_NONE, TOK_EFORMAT = -1, -2
HDR_DONT_COMPRESS, HDR_TOKEN, HDR_LIKELY_TO_REPEAT = 1, 2, 4
FLAGS = ("http2_static_table_name_index", "proxy_should_drop_for_req", "proxy_should_drop_for_res",
         "is_init_header_special", "is_hpack_special", "copy_for_push_request", "dont_compress", "likely_to_repeat")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tokens.npz")


def unpack(blob, off):
    raw = np.asarray(blob, np.uint8).tobytes()
    return [raw[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def load_fixture():
    """tests/golden/tokens.npz -> dict(names, flags [ntokens, 8], probes, answer)"""
    with np.load(GOLDEN, allow_pickle=False) as z:
        return dict(names=unpack(z["names"], z["name_off"]), flags=z["flags"].astype(np.int64),
                    probes=unpack(z["probes"], z["probe_off"]), answer=z["answer"].astype(np.int32))


def encoder_words(flags):
    """the word of every token for hhuff_intern_headers: HHUFF_HDR_TOKEN, and HHUFF_HDR_LIKELY_TO_REPEAT as the
    token's likely_to_repeat flag says"""
    ltr = np.asarray(flags)[:, FLAGS.index("likely_to_repeat")] != 0
    return (HDR_TOKEN | np.where(ltr, HDR_LIKELY_TO_REPEAT, 0)).astype(np.uint32)


class Model:
    def __init__(self, names, user=None):
        self.names = [bytes(n) for n in names]
        assert 1 <= len(self.names) <= 4096 and all(1 <= len(n) <= 255 for n in self.names)
        self.ids = {n: i for i, n in enumerate(self.names)}
        assert len(self.ids) == len(self.names), "two equal names"
        self.user = np.zeros(len(self.names), np.uint32) if user is None else np.asarray(user, np.uint32)

    def lookup(self, name):
        """h2o_lookup_token: the index in the caller's list, or -1; bytewise, case-sensitive"""
        return self.ids.get(bytes(name), TOK_NONE)

    def find(self, data, off, length, in_size=None):
        """the token of data[off .. off + length): a miss for length 0, over 255, or a range past in_size"""
        in_size = len(data) if in_size is None else in_size
        if length == 0 or length > 255 or off + length > in_size:
            return TOK_NONE
        return self.lookup(bytes(data[off:off + length]))

    def intern_strings(self, data, off, length, miss_user=0, in_size=None):
        raw = np.asarray(data, np.uint8).tobytes()
        tok = np.array([self.find(raw, int(o), int(n), in_size) for o, n in zip(off, length)], np.int32).reshape(-1)
        user = np.where(tok >= 0, self.user[np.maximum(tok, 0)], np.uint32(miss_user)).astype(np.uint32)
        return tok, user

    def field_slots(self, first, nfields):
        """the slot rule: block b's fields are first[b] .. first[b] + min(nfields[b], first[b + 1] - first[b]) - 1"""
        out = []
        for b in range(len(nfields)):
            lo, hi = int(first[b]), int(first[b + 1])
            out += list(range(lo, lo + min(int(nfields[b]), max(0, hi - lo))))
        return np.asarray(out, np.int64)

    def intern_fields(self, arena, name_off, name_len, first, nfields, token, user_out, miss_user=0, arena_size=None):
        """token / user_out: the arrays as they were before the call; only the field slots change"""
        token, user_out = np.array(token, np.int32), np.array(user_out, np.uint32)
        s = self.field_slots(first, nfields)
        if s.size:
            token[s], user_out[s] = self.intern_strings(arena, np.asarray(name_off)[s], np.asarray(name_len)[s], miss_user,
                                                        arena_size)
        return token, user_out

    def intern_headers(self, data, hdr, keep_mask=HDR_DONT_COMPRESS, in_size=None):
        """hdr: records with name_off, name_len, flags -> (the records with flags = (flags & keep_mask) | (hit ? word
        : 0), token)"""
        hdr = hdr.copy()
        tok, user = self.intern_strings(data, hdr["name_off"], hdr["name_len"], 0, in_size)
        hdr["flags"] = (hdr["flags"] & np.uint32(keep_mask)) | np.where(tok >= 0, user, 0).astype(np.uint32)
        return hdr, tok
