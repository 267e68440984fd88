"""ORACLE ctypes bindings -- TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
It binds oracle/liboracle.so (the clean-room CPU restatement, huff_oracle.c) and, when it was built in
the container that has /root/reference, oracle/_ref/libh2oref.so (the real reference codec).

Batch helpers take numpy arrays in the include/hhuff.h layout and return numpy arrays.
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FAIL = 0xFFFFFFFF
STATUS_FAIL = 0x80

# include/hhuff.h hhuff_request_t (48 bytes)
REQ_DTYPE = np.dtype([("content_length", "<u8"), ("method", "<i4"), ("scheme", "<i4"), ("authority", "<i4"),
                      ("path", "<i4"), ("protocol", "<i4"), ("expect", "<i4"), ("exists_map", "<u4"),
                      ("nheaders", "<u4"), ("err", "<u4"), ("scheme_kind", "<u4")])
# include/hhuff.h hhuff_qpack_request_t (72 bytes): the request record, the datagram-flow-id field, the ack
QREQ_DTYPE = np.dtype([("content_length", "<u8"), ("method", "<i4"), ("scheme", "<i4"), ("authority", "<i4"),
                       ("path", "<i4"), ("protocol", "<i4"), ("expect", "<i4"), ("exists_map", "<u4"),
                       ("nheaders", "<u4"), ("err", "<u4"), ("scheme_kind", "<u4"), ("datagram_flow_id", "<i4"),
                       ("ack_len", "<u4"), ("ack", "u1", (16,))])
# include/hhuff.h hhuff_response_t (16 bytes) and hhuff_qpack_response_head_t (40 bytes)
RES_DTYPE = np.dtype([("status", "<i4"), ("nheaders", "<u4"), ("err", "<u4"), ("datagram_flow_id", "<i4")])
QRES_DTYPE = np.dtype([("status", "<i4"), ("nheaders", "<u4"), ("err", "<u4"), ("datagram_flow_id", "<i4"),
                       ("ack_len", "<u4"), ("reserved", "<u4"), ("ack", "u1", (16,))])
_u8p = ctypes.POINTER(ctypes.c_uint8)
_u32p = ctypes.POINTER(ctypes.c_uint32)


def build():
    """Compile liboracle.so (and _ref when /root/reference is present)."""
    subprocess.run(["make", "-s", "-C", HERE], check=True)


def _ptr(a, t):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(t)


class _Codec:
    def __init__(self, path, prefix):
        if not os.path.exists(path):
            raise FileNotFoundError(path + " not built (run make -C oracle)")
        self.lib = ctypes.CDLL(path)
        self.prefix = prefix
        L = self.lib
        P = prefix
        self._dec = getattr(L, P + "_decode_huffman")
        self._dec.restype = ctypes.c_size_t
        self._dec.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint), ctypes.c_char_p, ctypes.c_size_t,
                              ctypes.c_int]
        self._enc = getattr(L, P + "_encode_huffman")
        self._enc.restype = ctypes.c_size_t
        self._enc.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
        self._encstr = getattr(L, P + "_encode_string")
        self._encstr.restype = ctypes.c_size_t
        self._encstr.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
        self._flat = getattr(L, P + "_flatten_string")
        self._flat.restype = ctypes.c_size_t
        self._flat.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_int]
        self._encint = getattr(L, P + "_encode_int")
        self._encint.restype = ctypes.c_void_p
        self._encint.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint]
        self._decint = getattr(L, P + "_decode_int")
        self._decint.restype = ctypes.c_int64
        self._decint.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_uint]
        for name, extra in (("decode_batch", [_u32p, _u8p, _u32p, _u32p, _u8p, ctypes.c_int]),
                            ("encode_batch", [_u8p, _u32p, _u32p, _u8p, ctypes.c_int]),
                            ("flatten_batch", [_u8p, ctypes.c_uint, _u32p, _u8p, _u32p, _u32p, ctypes.c_int])):
            f = getattr(L, P + "_" + name)
            f.restype = ctypes.c_int
            f.argtypes = [_u8p, _u32p, _u32p, ctypes.c_uint32] + extra
        f = getattr(L, P + "_hpack_decode_blocks")
        f.restype = ctypes.c_int
        f.argtypes = [_u8p, _u32p, _u32p, ctypes.c_uint32, ctypes.c_uint32, _u8p, ctypes.POINTER(ctypes.c_uint64),
                      _u32p, _u32p, _u32p, _u32p, _u8p, _u32p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
        f = getattr(L, P + "_hpack_parse_requests")
        f.restype = ctypes.c_int
        f.argtypes = [_u8p, _u32p, _u32p, ctypes.c_uint32, ctypes.c_uint32, _u8p, ctypes.POINTER(ctypes.c_uint64),
                      _u32p, _u32p, _u32p, _u32p, _u8p, _u32p, ctypes.POINTER(ctypes.c_int32), _u32p, ctypes.c_int]
        f = getattr(L, P + "_hpack_parse_responses")
        f.restype = ctypes.c_int
        f.argtypes = [_u8p, _u32p, _u32p, ctypes.c_uint32, ctypes.c_uint32, _u8p, _u8p, ctypes.POINTER(ctypes.c_uint64),
                      _u32p, _u32p, _u32p, _u32p, _u8p, _u32p, ctypes.POINTER(ctypes.c_int32), _u32p, ctypes.c_int]
        f = getattr(L, P + "_literals_batch")
        f.restype = ctypes.c_int
        f.argtypes = [_u8p, _u32p, _u32p, ctypes.c_uint32, ctypes.c_uint, ctypes.c_uint, _u32p, _u8p, _u32p, _u32p,
                      _u32p, _u8p, ctypes.c_int]

    def _parse_mixed(self):
        """<prefix>_hpack_parse_mixed, bound on first use: only the rule-edge tests need it, and a library built before
        it existed (an oracle/_ref that travelled with an older tree) still serves every other caller"""
        f = getattr(self.lib, self.prefix + "_hpack_parse_mixed", None)
        assert f is not None, "%s has no %s_hpack_parse_mixed: rebuild it (make -C oracle)" % (self.lib._name, self.prefix)
        f.restype = ctypes.c_int
        f.argtypes = [_u8p, _u32p, _u32p, ctypes.c_uint32, ctypes.c_uint32, _u8p, _u8p, _u8p,
                      ctypes.POINTER(ctypes.c_uint64), _u32p, _u32p, _u32p, _u32p, _u8p, _u32p,
                      ctypes.POINTER(ctypes.c_int32), _u32p, _u32p, ctypes.c_int]
        return f

    # ---- per-string (h2o signatures) ----
    def decode(self, src: bytes, is_name: bool = False, soft_in: int = 0):
        """-> (bytes or None on SIZE_MAX, soft_errors word)"""
        buf = ctypes.create_string_buffer(max(1, 2 * len(src)))
        soft = ctypes.c_uint(soft_in)
        r = self._dec(buf, ctypes.byref(soft), src, len(src), int(is_name))
        if r == ctypes.c_size_t(-1).value:
            return None, soft.value
        return buf.raw[:r], soft.value

    def encode(self, src: bytes):
        """-> bytes or None on SIZE_MAX"""
        buf = ctypes.create_string_buffer(max(1, len(src)))
        r = self._enc(buf, src, len(src))
        if r == ctypes.c_size_t(-1).value:
            return None
        return buf.raw[:r]

    def encode_string(self, src: bytes) -> bytes:
        buf = ctypes.create_string_buffer(len(src) + 11)
        r = self._encstr(buf, src, len(src))
        return buf.raw[:r]

    def flatten_string(self, src: bytes, prefix_bits: int, first: int = 0, raw: bool = False) -> bytes:
        buf = ctypes.create_string_buffer(len(src) + 11)
        buf[0] = first
        r = self._flat(buf, src, len(src), prefix_bits, int(raw))
        return buf.raw[:r]

    def encode_int(self, value: int, prefix_bits: int, first: int = 0) -> bytes:
        buf = ctypes.create_string_buffer(16)
        buf[0] = first
        end = self._encint(ctypes.addressof(buf), value, prefix_bits)
        return buf.raw[:end - ctypes.addressof(buf)]

    def decode_int(self, data: bytes, prefix_bits: int):
        """-> (value or negative error, bytes consumed)"""
        buf = ctypes.create_string_buffer(data, max(1, len(data)))
        p = ctypes.c_void_p(ctypes.addressof(buf))
        v = self._decint(ctypes.byref(p), ctypes.addressof(buf) + len(data), prefix_bits)
        return v, p.value - ctypes.addressof(buf)

    # ---- batch (include/hhuff.h layout) ----
    def decode_batch(self, data, in_off, n, in_len=None, is_name_bits=None, out_off=None, out_size=None, nthreads=1):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if out_size is None:
            end = int(in_off[n]) if in_len is None else int((in_off[:n].astype(np.uint64) + in_len).max(initial=0))
            out_size = (end * 8) // 5 + 16
        out = np.zeros(max(1, out_size), np.uint8)
        out_len = np.zeros(n, np.uint32)
        status = np.zeros(n, np.uint8)
        rc = getattr(self.lib, self.prefix + "_decode_batch")(
            _ptr(data, _u8p), _ptr(in_off, _u32p), _ptr(in_len, _u32p), n, _ptr(is_name_bits, _u32p),
            _ptr(out, _u8p), _ptr(out_off, _u32p), _ptr(out_len, _u32p), _ptr(status, _u8p), nthreads)
        assert rc == 0
        return out, out_len, status

    def encode_batch(self, data, in_off, n, in_len=None, out_off=None, out_size=None, nthreads=1):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if out_size is None:
            out_size = data.size + 16
        out = np.zeros(max(1, out_size), np.uint8)
        out_len = np.zeros(n, np.uint32)
        status = np.zeros(n, np.uint8)
        rc = getattr(self.lib, self.prefix + "_encode_batch")(
            _ptr(data, _u8p), _ptr(in_off, _u32p), _ptr(in_len, _u32p), n, _ptr(out, _u8p), _ptr(out_off, _u32p),
            _ptr(out_len, _u32p), _ptr(status, _u8p), nthreads)
        assert rc == 0
        return out, out_len, status

    def flatten_batch(self, data, in_off, n, prefix_bits, in_len=None, first_bytes=None, raw_bits=None,
                      out_off=None, out_size=None, nthreads=1):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if out_size is None:
            out_size = data.size + 11 * n + 16
        out = np.zeros(max(1, out_size), np.uint8)
        out_len = np.zeros(n, np.uint32)
        rc = getattr(self.lib, self.prefix + "_flatten_batch")(
            _ptr(data, _u8p), _ptr(in_off, _u32p), _ptr(in_len, _u32p), n, _ptr(first_bytes, _u8p), prefix_bits,
            _ptr(raw_bits, _u32p), _ptr(out, _u8p), _ptr(out_off, _u32p), _ptr(out_len, _u32p), nthreads)
        assert rc == 0
        return out, out_len

    def literals_batch(self, data, lit_off, lit_end, n, prefix_bits, qpack=False, is_name_bits=None, out_size=None,
                       nthreads=1):
        """string literals (decode_string / QPACK literal): -> out, out_len, pay_off, consumed, status"""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if out_size is None:
            out_size = (data.size * 8) // 5 + 16
        out = np.zeros(max(1, out_size), np.uint8)
        out_len = np.zeros(n, np.uint32)
        pay_off = np.zeros(n, np.uint32)
        consumed = np.zeros(n, np.uint32)
        status = np.zeros(n, np.uint8)
        rc = getattr(self.lib, self.prefix + "_literals_batch")(
            _ptr(data, _u8p), _ptr(lit_off, _u32p), _ptr(lit_end, _u32p), n, prefix_bits, 1 if qpack else 0,
            _ptr(is_name_bits, _u32p), _ptr(out, _u8p), _ptr(out_len, _u32p), _ptr(pay_off, _u32p),
            _ptr(consumed, _u32p), _ptr(status, _u8p), nthreads)
        assert rc == 0
        return out, out_len, pay_off, consumed, status


    def hpack_decode_blocks(self, data, blk_off, conn_first, table_size=4096, arena_off=None, nthreads=1,
                            requests=False, responses=False, trailers=None, plain=None):
        """HPACK header blocks (include/hhuff.h hhuff_hpack_decode_blocks contract) -> dict of arrays:
        arena, name_off, name_len, value_off, value_len, fflags (per field slot), nfields, bstatus (per block);
        requests=True: hhuff_hpack_parse_requests (h2o_hpack_parse_request per block), plus req (REQ_DTYPE);
        responses=True: hhuff_hpack_parse_responses (h2o_hpack_parse_response per block; trailers = u8 per
        block, nonzero for a trailers block), plus res (RES_DTYPE);
        plain (with either; u8 per block): nonzero for a block that belongs to a plain-mode call of a continuation
        whose later calls parse requests / responses -- decoded into the connection's table without the rules"""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        blk_off = np.ascontiguousarray(blk_off, dtype=np.uint32)
        conn_first = np.ascontiguousarray(conn_first, dtype=np.uint32)
        nb = blk_off.size - 1
        if arena_off is None:
            arena_off = default_arena_off(blk_off, table_size)
        arena_off = np.ascontiguousarray(arena_off, dtype=np.uint64)
        nslots = max(1, int(blk_off[-1]))
        r = dict(arena=np.zeros(max(1, int(arena_off[-1])), np.uint8),
                 name_off=np.zeros(nslots, np.uint32), name_len=np.zeros(nslots, np.uint32),
                 value_off=np.zeros(nslots, np.uint32), value_len=np.zeros(nslots, np.uint32),
                 fflags=np.zeros(nslots, np.uint8), nfields=np.zeros(max(1, nb), np.uint32),
                 bstatus=np.zeros(max(1, nb), np.int32))
        args = [_ptr(data, _u8p), _ptr(blk_off, _u32p), _ptr(conn_first, _u32p), conn_first.size - 1, table_size,
                _ptr(r["arena"], _u8p), arena_off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                _ptr(r["name_off"], _u32p), _ptr(r["name_len"], _u32p), _ptr(r["value_off"], _u32p),
                _ptr(r["value_len"], _u32p), _ptr(r["fflags"], _u8p), _ptr(r["nfields"], _u32p),
                r["bstatus"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32))]
        if plain is not None and (requests or responses):
            tr = None if trailers is None else np.ascontiguousarray(trailers, dtype=np.uint8)
            pl = np.ascontiguousarray(plain, dtype=np.uint8)
            words = np.zeros((max(1, nb), 4 if responses else 12), np.uint32)
            rc = self._parse_mixed()(
                *args[:5], _ptr(tr, _u8p), _ptr(pl, _u8p), *args[5:], None if responses else _ptr(words, _u32p),
                _ptr(words, _u32p) if responses else None, nthreads)
            r["res" if responses else "req"] = words.view(RES_DTYPE if responses else REQ_DTYPE).reshape(-1)
        elif responses:
            tr = None if trailers is None else np.ascontiguousarray(trailers, dtype=np.uint8)
            words = np.zeros((max(1, nb), 4), np.uint32)
            rc = getattr(self.lib, self.prefix + "_hpack_parse_responses")(*args[:5], _ptr(tr, _u8p), *args[5:],
                                                                            _ptr(words, _u32p), nthreads)
            r["res"] = words.view(RES_DTYPE).reshape(-1)
        elif requests:
            words = np.zeros((max(1, nb), 12), np.uint32)
            rc = getattr(self.lib, self.prefix + "_hpack_parse_requests")(*args, _ptr(words, _u32p), nthreads)
            r["req"] = words.view(REQ_DTYPE).reshape(-1)
        else:
            rc = getattr(self.lib, self.prefix + "_hpack_decode_blocks")(*args, nthreads)
        assert rc == 0
        return r


class QpackSession:
    """QPACK decoder session (include/hhuff.h hhuff_qpack_decode contract): one dynamic table per connection,
    kept between step() calls.  codec = oracle() (restatement) or ref() (h2o's qpack.c)."""

    def __init__(self, codec, nconn, header_table_size=4096, max_blocked=100):
        L, P = codec.lib, codec.prefix
        self._open, self._close, self._step = (getattr(L, P + "_qpack_open"), getattr(L, P + "_qpack_close"),
                                               getattr(L, P + "_qpack_step"))
        self._open.restype = ctypes.c_void_p
        self._open.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
        self._close.argtypes = [ctypes.c_void_p]
        self._step.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 19
        self._step_req = getattr(L, P + "_qpack_step_req")
        self._step_req.restype = ctypes.c_int
        self._step_req.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 21
        self._step_resp = getattr(L, P + "_qpack_step_resp")
        self._step_resp.restype = ctypes.c_int
        self._step_resp.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 21
        self.nconn = nconn
        self.h = self._open(nconn, header_table_size, max_blocked)

    def close(self):
        if getattr(self, "h", None):
            self._close(self.h)
            self.h = None

    __del__ = close

    def step(self, data, enc_off, enc_len, sec_off, conn_first, arena_off, num_blocked=None, stream_id=None,
             responses=False):
        """-> dict: arena, name_off, name_len, value_off, value_len, fflags (per field slot), nfields, sstatus,
        req_insert_count (per section), enc_status, enc_consumed, insert_count (per connection).  With
        stream_id (u64 per section): h2o_qpack_parse_request per section (hhuff_qpack_parse_requests'
        contract), plus "req" (QREQ_DTYPE records); the reference harness also checks every section against
        the real h2o_qpack_parse_request and fails on a disagreement.  responses=True (with stream_id):
        h2o_qpack_parse_response per section instead (hhuff_qpack_parse_responses), plus "res" (QRES_DTYPE)."""
        c = lambda a, t: np.ascontiguousarray(a, dtype=t)  # noqa: E731
        data, enc_off, enc_len, sec_off, conn_first = (c(data, np.uint8), c(enc_off, np.uint32), c(enc_len, np.uint32),
                                                       c(sec_off, np.uint32), c(conn_first, np.uint32))
        if data.size == 0:
            data = np.zeros(1, np.uint8)
        arena_off = c(arena_off, np.uint64)
        nb = None if num_blocked is None else c(num_blocked, np.uint32)
        ns = sec_off.size - 1
        nslots = max(1, int(sec_off[-1]))
        nc = max(1, self.nconn)
        r = dict(arena=np.zeros(max(1, int(arena_off[-1])), np.uint8),
                 name_off=np.zeros(nslots, np.uint32), name_len=np.zeros(nslots, np.uint32),
                 value_off=np.zeros(nslots, np.uint32), value_len=np.zeros(nslots, np.uint32),
                 fflags=np.zeros(nslots, np.uint8), nfields=np.zeros(max(1, ns), np.uint32),
                 sstatus=np.zeros(max(1, ns), np.int32), req_insert_count=np.zeros(max(1, ns), np.uint64),
                 enc_status=np.zeros(nc, np.int32), enc_consumed=np.zeros(nc, np.uint32),
                 insert_count=np.zeros(nc, np.uint64))
        d = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        args = [self.h, d(data), d(enc_off), d(enc_len), d(sec_off), d(conn_first), d(nb), d(r["arena"]),
                d(arena_off), d(r["name_off"]), d(r["name_len"]), d(r["value_off"]), d(r["value_len"]),
                d(r["fflags"]), d(r["nfields"]), d(r["sstatus"]), d(r["req_insert_count"]), d(r["enc_status"]),
                d(r["enc_consumed"]), d(r["insert_count"])]
        if stream_id is None:
            rc = self._step(*args)
            assert rc == 0
            return r
        sid = c(stream_id, np.uint64)
        if responses:
            words = np.zeros((max(1, ns), 10), np.uint32)
            rc = self._step_resp(*args, d(sid), d(words))
            assert rc == 0, "%d section(s) disagree with the real h2o_qpack_parse_response" % rc
            r["res"] = words.view(QRES_DTYPE).reshape(-1)
            return r
        words = np.zeros((max(1, ns), 18), np.uint32)
        rc = self._step_req(*args, d(sid), d(words))
        assert rc == 0, "%d section(s) disagree with the real h2o_qpack_parse_request" % rc
        r["req"] = words.view(QREQ_DTYPE).reshape(-1)
        return r


class HpeSession:
    """HTTP/2 response encoder session (include/hhuff.h hhuff_hpack_flatten_responses contract): one encoder
    dynamic table per connection, kept between step() calls.  codec = oracle() (restatement, hpack_encode.c)
    or ref() (h2o's h2o_hpack_flatten_response / _trailers, ref_hpenc.c)."""

    def __init__(self, codec, nconn):
        L, P = codec.lib, codec.prefix
        self._open, self._close, self._step = (getattr(L, P + "_hpe_open"), getattr(L, P + "_hpe_close"),
                                               getattr(L, P + "_hpe_step"))
        self._open.restype = ctypes.c_void_p
        self._open.argtypes = [ctypes.c_uint32]
        self._close.argtypes = [ctypes.c_void_p]
        self._step.restype = ctypes.c_int
        self._step.argtypes = ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 5)
        self.nconn = nconn
        self.h = self._open(nconn)

    def close(self):
        if getattr(self, "h", None):
            self._close(self.h)
            self.h = None

    __del__ = close

    def step(self, data, hdr, res, conn_first, out_off, server_off=0, server_len=0):
        """hdr / res: numpy record arrays (h2o_amd.codec HPE_HEADER_DTYPE / HPE_RESPONSE_DTYPE); -> dict out,
        out_len, headers_size, rstatus"""
        c = lambda a, t: np.ascontiguousarray(a, dtype=t)  # noqa: E731
        data = c(data, np.uint8)
        in_size = data.size
        if data.size == 0:
            data = np.zeros(1, np.uint8)
        hdr = np.ascontiguousarray(hdr)
        res = np.ascontiguousarray(res)
        conn_first, out_off = c(conn_first, np.uint32), c(out_off, np.uint64)
        nres = max(1, int(conn_first[-1]))
        r = dict(out=np.zeros(max(1, int(out_off[-1])), np.uint8), out_len=np.zeros(nres, np.uint32),
                 headers_size=np.zeros(nres, np.uint32), rstatus=np.zeros(nres, np.int32))
        if hdr.size == 0:
            hdr = np.zeros(1, hdr.dtype)
        hp = hdr.ctypes.data
        rc = self._step(self.h, data.ctypes.data, in_size, hp, res.ctypes.data, conn_first.ctypes.data, server_off,
                        server_len, r["out"].ctypes.data, out_off.ctypes.data, r["out_len"].ctypes.data,
                        r["headers_size"].ctypes.data, r["rstatus"].ctypes.data)
        assert rc == 0, "%d header(s) flagged as tokens are not h2o tokens" % rc
        return r


def qpe_step(codec, data, hdr, res, out_off, server_off=0, server_len=0):
    """HTTP/3 response HEADERS frames (include/hhuff.h hhuff_qpack_flatten_responses contract); codec = oracle()
    (restatement, qpack_encode.c) or ref() (h2o_qpack_flatten_response, ref_shim.c).  hdr / res: numpy record
    arrays (h2o_amd.codec HPE_HEADER_DTYPE / QPE_RESPONSE_DTYPE) -> dict out, out_len, header_len, rstatus"""
    f = getattr(codec.lib, codec.prefix + "_qpe_step")
    f.restype = ctypes.c_int
    f.argtypes = ([ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                   ctypes.c_uint32] + [ctypes.c_void_p] * 5)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    in_size = data.size
    if data.size == 0:
        data = np.zeros(1, np.uint8)
    hdr, res = np.ascontiguousarray(hdr), np.ascontiguousarray(res)
    if hdr.size == 0:
        hdr = np.zeros(1, hdr.dtype)
    out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
    n = res.size
    r = dict(out=np.zeros(max(1, int(out_off[-1])), np.uint8), out_len=np.zeros(max(1, n), np.uint32),
             header_len=np.zeros(max(1, n), np.uint32), rstatus=np.zeros(max(1, n), np.int32))
    rc = f(data.ctypes.data, in_size, hdr.ctypes.data, res.ctypes.data if n else None, n, server_off, server_len,
           r["out"].ctypes.data, out_off.ctypes.data, r["out_len"].ctypes.data, r["header_len"].ctypes.data,
           r["rstatus"].ctypes.data)
    assert rc == 0, "%d header(s) flagged as tokens are not h2o tokens" % rc
    return r


def default_arena_off(blk_off, table_size=4096):
    """A block of L bytes produces at most L fields; each field's name + value is at most 8/5 of its
    literal bytes or a copy of one table entry (<= table_size bytes): a generous bound per block."""
    L = np.diff(np.asarray(blk_off, dtype=np.uint64))
    cap = (L * 8) // 5 + (L // 4 + 1) * np.uint64(table_size + 64)  # = h2o_amd.codec.default_arena_off
    out = np.zeros(L.size + 1, np.uint64)
    out[1:] = np.cumsum(cap)
    return out


_oracle = None
_ref = None


def oracle() -> _Codec:
    """The clean-room restatement (liboracle.so)."""
    global _oracle
    if _oracle is None:
        _oracle = _Codec(os.path.join(HERE, "liboracle.so"), "orc")
    return _oracle


def ref_available() -> bool:
    return os.path.exists(os.path.join(HERE, "_ref", "libh2oref.so"))


def ref() -> _Codec:
    """The real reference codec (only in the build container)."""
    global _ref
    if _ref is None:
        _ref = _Codec(os.path.join(HERE, "_ref", "libh2oref.so"), "ref")
    return _ref


CALLERS_PATH = os.path.join(HERE, "_ref", "libh2ocallers.so")


def callers_available() -> bool:
    return os.path.exists(CALLERS_PATH)


def callers() -> _Codec:
    """h2o's own callers (hpack.c / qpack.c built with default visibility): their calls to
    h2o_hpack_{de,en}code_huffman go through the PLT and bind to the first definition in the global scope --
    libhhuff.so when it was loaded RTLD_GLOBAL before this library (tests/dropin_replay.py)."""
    return _Codec(CALLERS_PATH, "ref")
