"""ctypes bindings of the hhuff C-ABI (include/hhuff.h) -- the host-side mirror of h2o's interface.

Per-string functions keep h2o's names and meaning (lib/http2/hpack.c:117 / :774):
    decode_huffman(src, is_name, soft_errors=0) -> (bytes | None, soft_errors)   None <=> SIZE_MAX
    encode_huffman(src)                         -> bytes | None                 None <=> SIZE_MAX
Batch functions run the HIP kernels on device tensors (torch is used only for memory and streams):
    decode_batch(...), encode_batch(...)       device-resident arrays, async on the current stream
    decode_batch_host(...), encode_batch_host(...)   numpy arrays, H2D/D2H included
There is no CPU codec behind any of these: if libhhuff.so is missing or no GPU is present they raise.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# HHUFF_AB_LIB: an A/B build of the same library (tools/ab.py build NAME -> build/ab/libhhuff_NAME.so), for
# running the test suite against an experiment; the product path is always h2o_amd/libhhuff.so
LIB_PATH = os.environ.get("HHUFF_AB_LIB") or os.path.join(HERE, "libhhuff.so")

FAIL_LEN = 0xFFFFFFFF
SOFT_NAME = 0x1
SOFT_VALUE = 0x2
STATUS_FAIL = 0x80
STATUS_TOO_LONG = 0xC0
SIZE_MAX = ctypes.c_size_t(-1).value

_vp = ctypes.c_void_p
_lib = None


class HhuffError(RuntimeError):
    pass


class _ConnSlotsStruct(ctypes.Structure):  # include/hhuff.h hhuff_conn_slots_t
    _fields_ = [("slot", _vp), ("flags", _vp), ("nslots", ctypes.c_uint32)]


class _QpackDsessionsStruct(ctypes.Structure):  # include/hhuff.h hhuff_qpack_dsessions_t
    _fields_ = [("state", _vp), ("state_size", ctypes.c_uint64), ("cancel_first", _vp), ("cancel_id", _vp),
                ("cancel_flags", _vp), ("dec_out", _vp), ("dec_out_off", _vp), ("dec_out_len", _vp), ("wake_id", _vp),
                ("wake_first", _vp), ("nwake", _vp), ("parked", _vp), ("dflags", _vp), ("flags", ctypes.c_uint32)]


class _H2StreamsParamsStruct(ctypes.Structure):  # include/hhuff.h hhuff_h2_streams_params_t
    _fields_ = [("max_streams", ctypes.c_uint32), ("max_streams_for_priority", ctypes.c_uint32),
                ("active_stream_window_size", ctypes.c_uint32), ("max_entries", ctypes.c_uint32),
                ("max_request_entity_size", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("rsv", ctypes.c_uint32)]


class _ConnFamilyStruct(ctypes.Structure):  # include/hhuff.h hhuff_conn_family_t
    _fields_ = [("family", ctypes.c_uint32), ("table_size", ctypes.c_uint32), ("max_inflight", ctypes.c_uint32),
                ("max_blocked", ctypes.c_uint32)]


SLOTS_SYMBOLS = ("hhuff_hpack_decode_blocks_slots", "hhuff_hpack_parse_requests_slots", "hhuff_hpack_parse_responses_slots",
                 "hhuff_qpack_decode_slots", "hhuff_qpack_parse_requests_slots", "hhuff_qpack_parse_responses_slots",
                 "hhuff_hpack_flatten_responses_slots", "hhuff_qpack_flatten_sessions_slots")


def lib():
    """Load libhhuff.so (fails loudly when the HIP extension is not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HhuffError("libhhuff.so not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        # torch first: its ROCm wheel ships its own libamdhip64.so, and libhhuff.so's dependency must
        # resolve to that already-loaded runtime -- one HIP runtime per process (loaded the other way round,
        # two runtimes end up sharing the device and the per-string path fails).  Without torch (the
        # numpy-only host and per-string bindings) the library's own HIP runtime dependency is used.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass

        L = ctypes.CDLL(LIB_PATH)
        L.h2o_hpack_decode_huffman.restype = ctypes.c_size_t
        L.h2o_hpack_decode_huffman.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint), ctypes.c_char_p,
                                               ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p)]
        L.h2o_hpack_encode_huffman.restype = ctypes.c_size_t
        L.h2o_hpack_encode_huffman.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
        L.hhuff_decode_batch.restype = ctypes.c_int
        L.hhuff_decode_batch.argtypes = [_vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]
        L.hhuff_encode_batch.restype = ctypes.c_int
        L.hhuff_encode_batch.argtypes = [_vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp]
        L.hhuff_decode_batch_packed.restype = ctypes.c_int
        L.hhuff_decode_batch_packed.argtypes = [_vp, ctypes.c_uint64, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]
        L.hhuff_encode_batch_packed.restype = ctypes.c_int
        L.hhuff_encode_batch_packed.argtypes = [_vp, ctypes.c_uint64, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp]
        L.hhuff_flatten_batch.restype = ctypes.c_int
        L.hhuff_flatten_batch.argtypes = [_vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint32, _vp, ctypes.c_uint, _vp, _vp,
                                          _vp, _vp, _vp]
        L.hhuff_decode_batch_host.restype = ctypes.c_int
        L.hhuff_decode_batch_host.argtypes = [_vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint32, _vp, _vp, ctypes.c_uint64,
                                              _vp, _vp, _vp, ctypes.c_int]
        L.hhuff_encode_batch_host.restype = ctypes.c_int
        L.hhuff_encode_batch_host.argtypes = [_vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint32, _vp, ctypes.c_uint64,
                                              _vp, _vp, _vp, ctypes.c_int]
        L.hhuff_decode_literals.restype = ctypes.c_int
        L.hhuff_decode_literals.argtypes = [_vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint32, ctypes.c_uint, ctypes.c_uint,
                                            _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        L.hhuff_decode_batch_host_pipelined.restype = ctypes.c_int
        L.hhuff_decode_batch_host_pipelined.argtypes = [_vp, ctypes.c_uint64, _vp, ctypes.c_uint32, _vp, _vp,
                                                        ctypes.c_uint64, _vp, _vp, ctypes.c_int, ctypes.c_uint64]
        L.hhuff_encode_batch_host_pipelined.restype = ctypes.c_int
        L.hhuff_encode_batch_host_pipelined.argtypes = [_vp, ctypes.c_uint64, _vp, ctypes.c_uint32, _vp, ctypes.c_uint64,
                                                        _vp, _vp, ctypes.c_int, ctypes.c_uint64]
        L.hhuff_hpack_scratch_size.restype = ctypes.c_uint64
        L.hhuff_hpack_scratch_size.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        L.hhuff_hpack_decode_blocks.restype = ctypes.c_int
        L.hhuff_hpack_decode_blocks.argtypes = [_vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp,
                                                _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64,
                                                ctypes.c_uint, _vp]
        L.hhuff_hpack_parse_requests.restype = ctypes.c_int
        L.hhuff_hpack_parse_requests.argtypes = [_vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp,
                                                 _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64,
                                                 ctypes.c_uint, _vp]
        L.hhuff_hpack_parse_responses.restype = ctypes.c_int
        L.hhuff_hpack_parse_responses.argtypes = [_vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp,
                                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                  ctypes.c_uint64, ctypes.c_uint, _vp]
        L.hhuff_qpack_parse_responses.restype = ctypes.c_int
        L.hhuff_qpack_parse_responses.argtypes = ([_vp, ctypes.c_uint64, _vp, _vp, _vp, _vp, ctypes.c_uint32,
                                                   ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64] + [_vp] * 17 +
                                                  [ctypes.c_uint64, ctypes.c_uint, _vp])
        L.hhuff_qpack_scratch_size.restype = ctypes.c_uint64
        L.hhuff_qpack_scratch_size.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        L.hhuff_qpack_decode.restype = ctypes.c_int
        L.hhuff_qpack_decode.argtypes = ([_vp, ctypes.c_uint64, _vp, _vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.c_uint32, ctypes.c_uint64] + [_vp] * 15 +
                                         [ctypes.c_uint64, ctypes.c_uint, _vp])
        L.hhuff_qpack_parse_requests.restype = ctypes.c_int
        L.hhuff_qpack_parse_requests.argtypes = ([_vp, ctypes.c_uint64, _vp, _vp, _vp, _vp, ctypes.c_uint32,
                                                  ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64] + [_vp] * 17 +
                                                 [ctypes.c_uint64, ctypes.c_uint, _vp])
        L.hhuff_hpack_enc_scratch_size.restype = ctypes.c_uint64
        L.hhuff_hpack_enc_scratch_size.argtypes = [ctypes.c_uint32]
        L.hhuff_hpack_flatten_responses.restype = ctypes.c_int
        L.hhuff_hpack_flatten_responses.argtypes = ([_vp, ctypes.c_uint64, _vp, ctypes.c_uint32, _vp, _vp,
                                                     ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
                                                    + [_vp] * 6 + [ctypes.c_uint64, ctypes.c_uint, _vp])
        L.hhuff_qpack_flatten_responses.restype = ctypes.c_int
        L.hhuff_qpack_flatten_responses.argtypes = ([_vp, ctypes.c_uint64, _vp, ctypes.c_uint32, _vp, ctypes.c_uint32,
                                                     ctypes.c_uint32, ctypes.c_uint32] + [_vp] * 6)
        L.hhuff_qpack_enc_scratch_size.restype = ctypes.c_uint64
        L.hhuff_qpack_enc_scratch_size.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
        L.hhuff_qpack_flatten_sessions.restype = ctypes.c_int
        L.hhuff_qpack_flatten_sessions.argtypes = ([_vp, ctypes.c_uint64, _vp, ctypes.c_uint32, _vp, _vp, ctypes.c_uint32,
                                                    ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint64,
                                                    ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32] + [_vp] * 12 +
                                                   [ctypes.c_uint64, ctypes.c_uint, _vp])
        # include/hhuff.h (2h): every stateful entry point again with a hhuff_conn_slots_t first
        for name in SLOTS_SYMBOLS:
            base = getattr(L, name[:-len("_slots")])
            f = getattr(L, name)
            f.restype = ctypes.c_int
            f.argtypes = [ctypes.POINTER(_ConnSlotsStruct)] + list(base.argtypes)
        # include/hhuff.h (2g''): the encoder sessions with a hhuff_qpack_peer_t array in front of the slots
        L.hhuff_qpack_flatten_sessions_peers.restype = ctypes.c_int
        L.hhuff_qpack_flatten_sessions_peers.argtypes = [_vp] + list(L.hhuff_qpack_flatten_sessions_slots.argtypes)
        # include/hhuff.h (2e'''): the request / response steps with decoder sessions -- the sessions and the slots
        # first, no num_blocked
        for name in ("hhuff_qpack_parse_requests", "hhuff_qpack_parse_responses"):
            at = list(getattr(L, name).argtypes)
            f = getattr(L, name + "_sessions")
            f.restype = ctypes.c_int
            f.argtypes = [ctypes.POINTER(_QpackDsessionsStruct), ctypes.POINTER(_ConnSlotsStruct)] + at[:10] + at[11:]
        L.hhuff_qpack_dsession_state_size.restype = ctypes.c_uint64
        L.hhuff_qpack_dsession_state_size.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        L.hhuff_qpack_dsession_out_bound.restype = ctypes.c_uint64
        L.hhuff_qpack_dsession_out_bound.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        # include/hhuff.h (2i): connection images
        for name in ("hhuff_conn_slab_size", "hhuff_conn_image_bound"):
            getattr(L, name).restype = ctypes.c_uint64
            getattr(L, name).argtypes = [ctypes.POINTER(_ConnFamilyStruct)]
        for name in ("hhuff_conn_export", "hhuff_conn_import"):
            getattr(L, name).restype = ctypes.c_int
            getattr(L, name).argtypes = [ctypes.POINTER(_ConnFamilyStruct), _vp, ctypes.c_uint64, ctypes.c_uint32, _vp,
                                         ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp]
        L.hhuff_version.restype = ctypes.c_char_p
        L.hhuff_last_error_string.restype = ctypes.c_char_p
        L.hhuff_grid_size.restype = ctypes.c_int
        L.hhuff_per_string_calls.restype = ctypes.c_uint64
        L.hhuff_grid_size.argtypes = [ctypes.c_int, ctypes.c_int]
        L.hhuff_decode_prices.restype = ctypes.c_int
        L.hhuff_decode_prices.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
        L.hhuff_calibrate_decode_prices.restype = ctypes.c_int
        L.hhuff_calibrate_decode_prices.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
        L.hhuff_set_decode_prices.restype = ctypes.c_int
        L.hhuff_set_decode_prices.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
        L.hhuff_pool_trim.restype = ctypes.c_int
        L.hhuff_pool_trim.argtypes = []
        L.hhuff_set_decode_kernel.restype = ctypes.c_int
        L.hhuff_set_decode_kernel.argtypes = [ctypes.c_int]
        L.hhuff_set_edge_defer_min.restype = ctypes.c_uint32
        L.hhuff_set_edge_defer_min.argtypes = [ctypes.c_uint32]
        L.hhuff_decode_batch_host_packed.restype = ctypes.c_int
        L.hhuff_decode_batch_host_packed.argtypes = [_vp, ctypes.c_uint64, _vp, ctypes.c_uint32, _vp, _vp, ctypes.c_uint64,
                                                     _vp, _vp, _vp, ctypes.c_int]
        L.hhuff_encode_batch_host_packed.restype = ctypes.c_int
        L.hhuff_encode_batch_host_packed.argtypes = [_vp, ctypes.c_uint64, _vp, ctypes.c_uint32, _vp, ctypes.c_uint64,
                                                     _vp, _vp, _vp, ctypes.c_int]
        L.hhuff_decode_batch_multi.restype = ctypes.c_int
        L.hhuff_decode_batch_multi.argtypes = [ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_uint64, _vp, ctypes.c_uint32,
                                               _vp, _vp, ctypes.c_uint64, _vp, _vp, _vp]
        L.hhuff_encode_batch_multi.restype = ctypes.c_int
        L.hhuff_encode_batch_multi.argtypes = [ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_uint64, _vp, ctypes.c_uint32,
                                               _vp, ctypes.c_uint64, _vp, _vp, _vp]
        L.hhuff_shard_bounds.restype = ctypes.c_int
        L.hhuff_shard_bounds.argtypes = [_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _vp]
        L.hhuff_tokens_table_size.restype = ctypes.c_uint64
        L.hhuff_tokens_table_size.argtypes = [ctypes.c_uint32, ctypes.c_uint64]
        L.hhuff_tokens_build.restype = ctypes.c_int
        L.hhuff_tokens_build.argtypes = [_vp, _vp, ctypes.c_uint32, _vp, _vp, ctypes.c_uint64]
        L.hhuff_intern_strings.restype = ctypes.c_int
        L.hhuff_intern_strings.argtypes = [_vp, ctypes.c_uint64, _vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint32, _vp, _vp,
                                           ctypes.c_uint32, _vp]
        L.hhuff_intern_fields.restype = ctypes.c_int
        L.hhuff_intern_fields.argtypes = [_vp, ctypes.c_uint64, _vp, ctypes.c_uint64, _vp, _vp, _vp, _vp, ctypes.c_uint32,
                                          ctypes.c_uint32, _vp, _vp, ctypes.c_uint32, _vp]
        L.hhuff_intern_headers.restype = ctypes.c_int
        L.hhuff_intern_headers.argtypes = [_vp, ctypes.c_uint64, _vp, ctypes.c_uint64, _vp, ctypes.c_uint32,
                                           ctypes.c_uint32, _vp, _vp]
        L.hhuff_h2_deframe.restype = ctypes.c_int
        L.hhuff_h2_deframe.argtypes = ([_vp, ctypes.c_uint64, _vp, ctypes.c_uint32, _vp] + [ctypes.c_uint32] * 3 +
                                       [ctypes.c_uint] + [_vp] * 11 + [ctypes.c_uint64, ctypes.c_uint32, _vp])
        L.hhuff_h2_control.restype = ctypes.c_int
        L.hhuff_h2_control.argtypes = ([_vp, ctypes.c_uint64, _vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint,
                                        ctypes.c_uint32] + [_vp] * 7 + [ctypes.c_uint64, _vp, _vp, _vp])
        L.hhuff_h2_frame_data.restype = ctypes.c_int
        L.hhuff_h2_frame_data.argtypes = ([_vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint] +
                                           [_vp] * 4 + [ctypes.c_uint64] + [_vp] * 4)
        u32, u64, slots_p = ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(_ConnSlotsStruct)
        L.hhuff_h2_streams_scratch_size.restype = u64
        L.hhuff_h2_streams_scratch_size.argtypes = [u32, u32]
        L.hhuff_h2_streams.restype = ctypes.c_int
        L.hhuff_h2_streams.argtypes = ([slots_p, ctypes.POINTER(_H2StreamsParamsStruct), _vp, u64, _vp, _vp, _vp, u32, _vp, _vp, _vp,
                                        u64] + [_vp] * 6 + [u64] + [_vp] * 6 + [u32, u32] + [_vp] * 6 + [u64, _vp, _vp, _vp, u64,
                                                                                                      ctypes.c_uint, _vp])
        L.hhuff_h2_streams_fill_sends.restype = ctypes.c_int
        L.hhuff_h2_streams_fill_sends.argtypes = [slots_p, u32, _vp, u64, _vp, _vp, u32, u32, _vp, _vp]
        L.hhuff_h2_streams_commit_sent.restype = ctypes.c_int
        L.hhuff_h2_streams_commit_sent.argtypes = [slots_p, u32, _vp, u64, _vp, _vp, _vp, u32, u32, _vp]
        L.hhuff_hpack_responses_set_peers.restype = ctypes.c_int
        L.hhuff_hpack_responses_set_peers.argtypes = [_vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp]
        L.hhuff_h3_deframe.restype = ctypes.c_int
        L.hhuff_h3_deframe.argtypes = ([_vp, ctypes.c_uint64] + [_vp, ctypes.c_uint32] * 3 + [ctypes.c_uint64, ctypes.c_uint] +
                                       [_vp] * 19 + [ctypes.c_uint64, ctypes.c_uint32, _vp])
        _lib = L
    return _lib


# symbols include/hhuff.h declares (checked by tests/test_capi_symbols.py)
EXPORTED = ("h2o_hpack_decode_huffman", "h2o_hpack_encode_huffman", "hhuff_decode_batch", "hhuff_encode_batch",
            "hhuff_decode_batch_packed", "hhuff_encode_batch_packed",
            "hhuff_flatten_batch", "hhuff_decode_literals", "hhuff_hpack_decode_blocks", "hhuff_hpack_scratch_size",
            "hhuff_hpack_parse_requests", "hhuff_hpack_parse_responses",
            "hhuff_qpack_decode", "hhuff_qpack_parse_requests", "hhuff_qpack_parse_responses", "hhuff_qpack_scratch_size",
            "hhuff_decode_batch_host", "hhuff_encode_batch_host", "hhuff_decode_batch_host_pipelined",
            "hhuff_encode_batch_host_pipelined", "hhuff_version", "hhuff_last_error_string", "hhuff_per_string_calls",
            "hhuff_grid_size", "hhuff_decode_prices", "hhuff_calibrate_decode_prices", "hhuff_set_decode_prices",
            "hhuff_pool_trim", "hhuff_service_stamps", "hhuff_hpack_enc_scratch_size",
            "hhuff_hpack_flatten_responses", "hhuff_qpack_flatten_responses", "hhuff_qpack_enc_scratch_size",
            "hhuff_qpack_flatten_sessions", "hhuff_set_decode_kernel",
            "hhuff_decode_batch_host_packed", "hhuff_encode_batch_host_packed", "hhuff_set_edge_defer_min",
            "hhuff_decode_batch_multi", "hhuff_encode_batch_multi", "hhuff_shard_bounds",
            "hhuff_debug_encode_blocks_per_cu", "hhuff_qpack_parse_requests_sessions",
            "hhuff_qpack_parse_responses_sessions", "hhuff_qpack_dsession_state_size",
            "hhuff_qpack_dsession_out_bound", "hhuff_conn_slab_size", "hhuff_conn_image_bound", "hhuff_conn_export",
            "hhuff_conn_import", "hhuff_qpack_flatten_sessions_peers", "hhuff_tokens_table_size", "hhuff_tokens_build",
            "hhuff_intern_strings", "hhuff_intern_fields", "hhuff_intern_headers", "hhuff_h2_deframe",
            "hhuff_h3_deframe", "hhuff_h2_control", "hhuff_hpack_responses_set_peers",
            "hhuff_h2_frame_data", "hhuff_h2_streams", "hhuff_h2_streams_scratch_size", "hhuff_h2_streams_fill_sends",
            "hhuff_h2_streams_commit_sent") + SLOTS_SYMBOLS


def _check(rc, what):
    if rc != 0:
        raise HhuffError("%s failed (%d): %s" % (what, rc, lib().hhuff_last_error_string().decode()))


# ---------------------------------------------------------------------------------------------------
# per-string (h2o signatures)
# ---------------------------------------------------------------------------------------------------
def decode_huffman(src: bytes, is_name: bool = False, soft_errors: int = 0):
    """h2o_hpack_decode_huffman: -> (decoded bytes or None for SIZE_MAX, soft_errors word)."""
    buf = ctypes.create_string_buffer(max(1, 2 * len(src)))
    soft = ctypes.c_uint(soft_errors)
    err = ctypes.c_char_p()
    r = lib().h2o_hpack_decode_huffman(buf, ctypes.byref(soft), src, len(src), int(bool(is_name)), ctypes.byref(err))
    if r == SIZE_MAX:
        return None, soft.value
    return buf.raw[:r], soft.value


def encode_huffman(src: bytes):
    """h2o_hpack_encode_huffman: -> Huffman bytes, or None when not shorter than the input (SIZE_MAX)."""
    buf = ctypes.create_string_buffer(max(1, len(src)))
    r = lib().h2o_hpack_encode_huffman(buf, src, len(src))
    if r == SIZE_MAX:
        return None
    return buf.raw[:r]


# ---------------------------------------------------------------------------------------------------
# device batch API (torch tensors; uint32 arrays are carried in int32 tensors, same bits)
# ---------------------------------------------------------------------------------------------------
def _dp(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device batch arrays must be contiguous device tensors"
    return t.data_ptr()


def _stream(stream):
    import torch

    s = torch.cuda.current_stream() if stream is None else stream
    return s.cuda_stream


CONN_RESET = 1
BLK_EINVAL = QPK_EINVAL = -303


class ConnSlots:
    """include/hhuff.h hhuff_conn_slots_t for the stateful calls' slots= argument: `slot` an int32 device tensor
    (u32 bits) with the scratch slot of each listed connection (None: slot c = c), `flags` a uint8 device tensor of
    CONN_RESET bits (None: all 0), `nslots` the slots the scratch holds."""

    def __init__(self, slot, flags, nslots):
        self.slot, self.flags, self.nslots = slot, flags, int(nslots)


def _stateful(name, slots, args):
    """call the stateful entry point `name`, or its _slots variant with `slots` (ConnSlots or None) in front"""
    if slots is None:
        _check(getattr(lib(), name)(*args), name)
        return
    st = _ConnSlotsStruct(_dp(slots.slot), _dp(slots.flags), slots.nslots)
    _check(getattr(lib(), name + "_slots")(ctypes.byref(st), *args), name + "_slots")


# include/hhuff.h (2i): connection images
FAM_HPACK_DEC, FAM_QPACK_DEC, FAM_HPACK_ENC, FAM_QPACK_ENC, FAM_QPACK_DSESSION = range(5)
IMG_SPACE, IMG_EINVAL, IMG_EFORMAT, IMG_EPARAM = -300, -303, -304, -305


def conn_family(family, table_size=0, max_inflight=0, max_blocked=0):
    """hhuff_conn_family_t: which slabs a scratch holds (FAM_* and the family's own parameters, 0 for the others)"""
    return _ConnFamilyStruct(int(family), int(table_size), int(max_inflight), int(max_blocked))


def conn_slab_size(fam) -> int:
    """the family's bytes per slot; 0: parameters its own call refuses"""
    return int(lib().hhuff_conn_slab_size(ctypes.byref(fam)))


def conn_image_bound(fam) -> int:
    """the largest image of one connection of the family (a multiple of 16)"""
    return int(lib().hhuff_conn_image_bound(ctypes.byref(fam)))


def conn_export(fam, scratch, nslots, slot, img=None, img_off=None, stream=None):
    """hhuff_conn_export of the slots in `slot` (int32 device tensor, u32 bits) of `scratch` (nslots slabs).
    img None: the size query runs first and lays the regions out back to back (each image's own length, a multiple
    of 16), then the images are written -> (img, img_off, img_len, status).  With img and img_off (int64 device
    tensor [n + 1]) the caller's regions are used as they are; a region too small gives status IMG_SPACE and the
    length needed in img_len."""
    import torch

    n = slot.numel()
    dev = scratch.device
    img_len = torch.empty(max(1, n), dtype=torch.int32, device=dev)
    status = torch.empty(max(1, n), dtype=torch.int32, device=dev)
    L, st = lib(), _stream(stream)
    head = [ctypes.byref(fam), _dp(scratch), scratch.numel() * scratch.element_size(), int(nslots), _dp(slot), n]
    if img is None:
        _check(L.hhuff_conn_export(*head, None, None, _dp(img_len), _dp(status), st), "hhuff_conn_export")
        img_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        img_off[1:] = torch.cumsum(img_len[:n].to(torch.int64) & 0xFFFFFFFF, 0)
        img = torch.empty(max(16, int(img_off[-1])), dtype=torch.uint8, device=dev)
    _check(L.hhuff_conn_export(*head, _dp(img), _dp(img_off), _dp(img_len), _dp(status), st), "hhuff_conn_export")
    return img, img_off, img_len[:n], status[:n]


def conn_import(fam, scratch, nslots, slot, img, img_off, img_len, stream=None):
    """hhuff_conn_import: item k's image (img[img_off[k] .. +img_len[k])) into slot slot[k] of `scratch` -> status
    (int32 device tensor: 0, IMG_EINVAL, IMG_EFORMAT or IMG_EPARAM; a refused item's slab is untouched)"""
    import torch

    n = slot.numel()
    status = torch.empty(max(1, n), dtype=torch.int32, device=scratch.device)
    _check(lib().hhuff_conn_import(ctypes.byref(fam), _dp(scratch), scratch.numel() * scratch.element_size(), int(nslots),
                                   _dp(slot), n, _dp(img), _dp(img_off), _dp(img_len), _dp(status), _stream(stream)),
           "hhuff_conn_import")
    return status[:n]


# include/hhuff.h (2j): token interning
TOK_NONE, TOK_EFORMAT = -1, -2


def tokens_table_size(ntokens, name_bytes) -> int:
    """hhuff_tokens_table_size: the bytes of a table of ntokens names of name_bytes bytes in all; 0: bad parameters"""
    return int(lib().hhuff_tokens_table_size(int(ntokens), int(name_bytes)))


def tokens_build(names, user=None):
    """hhuff_tokens_build on the host (no GPU): names = a list of bytes, user = their 32-bit words (None: all 0)
    -> the table, a numpy uint8 array of tokens_table_size bytes.  Raises HhuffError where the call refuses the list
    (two equal names, an empty name, a name over 255 bytes, no names or more than 4096)."""
    blob = np.frombuffer(b"".join(names), np.uint8).copy()
    off = np.zeros(len(names) + 1, np.uint32)
    off[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
    words = None if user is None else np.ascontiguousarray(user, np.uint32)
    assert words is None or words.size == len(names)
    size = tokens_table_size(len(names), blob.size)
    table = np.zeros(max(size, 16), np.uint8)
    rc = lib().hhuff_tokens_build(blob.ctypes.data, off.ctypes.data, len(names), None if words is None else words.ctypes.data,
                                  table.ctypes.data, size)
    if rc != 0:
        raise HhuffError("hhuff_tokens_build refused the list (%d)" % rc)
    return table[:size]


class TokenSet:
    """A token set on the device: the caller's names (a list of bytes; the token id is the index) and one 32-bit word
    per name, compiled by hhuff_tokens_build and uploaded.  The three calls of include/hhuff.h (2j) run on it; uint32
    arrays are int32 device tensors (same bits), as everywhere in this module."""

    def __init__(self, names, user=None, device="cuda"):
        import torch

        self.names = list(names)
        self.host = tokens_build(self.names, user)
        self.table = torch.from_numpy(self.host.copy()).to(device)
        assert self.table.data_ptr() % 16 == 0
        self.size = int(self.host.size)

    def intern_strings(self, data, off, length, n=None, miss_user=0, in_size=None, token=None, user_out=None, want_user=True,
                       stream=None):
        """hhuff_intern_strings: string i = data[off[i] .. off[i] + length[i]) -> (token int32 [n], user_out int32 [n] or
        None)"""
        import torch

        n = off.numel() if n is None else int(n)
        if token is None:
            token = torch.empty(max(1, n), dtype=torch.int32, device=data.device)
        if user_out is None and want_user:
            user_out = torch.empty(max(1, n), dtype=torch.int32, device=data.device)
        _check(lib().hhuff_intern_strings(_dp(self.table), self.size, _dp(data), data.numel() if in_size is None else in_size,
                                          _dp(off), _dp(length), n, _dp(token), _dp(user_out), int(miss_user) & 0xFFFFFFFF,
                                          _stream(stream)), "hhuff_intern_strings")
        return token[:n], None if user_out is None else user_out[:n]

    def intern_fields(self, arena, name_off, name_len, first, nfields, nslots, miss_user=0, arena_size=None, token=None,
                      user_out=None, want_user=True, stream=None):
        """hhuff_intern_fields behind a block or section decoder: first = its blk_off / sec_off ([nblk + 1]), nslots the
        host copy of first[nblk].  Slots that are no block's field keep what token / user_out held (new arrays: -1 /
        miss_user) -> (token int32 [nslots], user_out or None)"""
        import torch

        nblk, nslots = nfields.numel(), int(nslots)
        if token is None:
            token = torch.full((max(1, nslots),), TOK_NONE, dtype=torch.int32, device=arena.device)
        if user_out is None and want_user:
            user_out = torch.full((max(1, nslots),), int(np.uint32(miss_user & 0xFFFFFFFF).view(np.int32)), dtype=torch.int32,
                                  device=arena.device)
        _check(lib().hhuff_intern_fields(_dp(self.table), self.size, _dp(arena), arena.numel() if arena_size is None else arena_size,
                                         _dp(name_off), _dp(name_len), _dp(first), _dp(nfields), nblk, nslots, _dp(token),
                                         _dp(user_out), int(miss_user) & 0xFFFFFFFF, _stream(stream)), "hhuff_intern_fields")
        return token[:nslots], None if user_out is None else user_out[:nslots]

    def intern_headers(self, data, hdr, keep_mask=None, in_size=None, want_token=True, stream=None):
        """hhuff_intern_headers before an encoder: hdr = the device bytes of HPE_HEADER_DTYPE records, as the flatten
        calls take them; every record's flags become (flags & keep_mask) | (the name's word, or 0) in place
        (keep_mask None: HDR_DONT_COMPRESS) -> token int32 [nhdr] or None"""
        import torch

        keep_mask = HDR_DONT_COMPRESS if keep_mask is None else keep_mask
        nhdr = hdr.numel() * hdr.element_size() // HPE_HEADER_DTYPE.itemsize
        token = torch.empty(max(1, nhdr), dtype=torch.int32, device=data.device) if want_token else None
        _check(lib().hhuff_intern_headers(_dp(self.table), self.size, _dp(data), data.numel() if in_size is None else in_size,
                                          _dp(hdr), nhdr, int(keep_mask) & 0xFFFFFFFF, _dp(token), _stream(stream)),
               "hhuff_intern_headers")
        return None if token is None else token[:nhdr]


def decode_slot_size(in_size: int) -> int:
    """bytes the implicit decode layout (out_off = floor(8 * in_off / 5)) needs"""
    return (in_size * 8) // 5 + 16


def decode_batch(data, in_off, n, in_len=None, is_name_bits=None, out=None, out_off=None, out_len=None, status=None,
                 in_size=None, stream=None):
    """Batched h2o_hpack_decode_huffman on device tensors; returns (out, out_len, status)."""
    import torch

    dev = data.device
    in_size = data.numel() if in_size is None else in_size
    if out is None:
        out = torch.empty(decode_slot_size(in_size) if out_off is None else in_size * 2 + 16, dtype=torch.uint8,
                          device=dev)
    if out_len is None:
        out_len = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    if status is None:
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    _check(lib().hhuff_decode_batch(_dp(data), in_size, _dp(in_off), _dp(in_len), n, _dp(is_name_bits), _dp(out),
                                    _dp(out_off), _dp(out_len), _dp(status), _stream(stream)), "hhuff_decode_batch")
    return out, out_len, status


def encode_batch(data, in_off, n, in_len=None, out=None, out_off=None, out_len=None, status=None, in_size=None,
                 stream=None):
    """Batched h2o_hpack_encode_huffman on device tensors; returns (out, out_len, status)."""
    import torch

    dev = data.device
    in_size = data.numel() if in_size is None else in_size
    if out is None:
        out = torch.empty(in_size + 16, dtype=torch.uint8, device=dev)
    if out_len is None:
        out_len = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    if status is None:
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    _check(lib().hhuff_encode_batch(_dp(data), in_size, _dp(in_off), _dp(in_len), n, _dp(out), _dp(out_off),
                                    _dp(out_len), _dp(status), _stream(stream)), "hhuff_encode_batch")
    return out, out_len, status


def decode_batch_packed(data, in_off, n, is_name_bits=None, out=None, out_off=None, out_len=None, status=None,
                        in_size=None, stream=None):
    """Batched h2o_hpack_decode_huffman with packed output (include/hhuff.h hhuff_decode_batch_packed):
    returns (out, out_off [n+1], out_len, status); string i at out[out_off[i] : out_off[i] + out_len[i]]."""
    import torch

    dev = data.device
    in_size = data.numel() if in_size is None else in_size
    if out is None:
        out = torch.empty(decode_slot_size(in_size), dtype=torch.uint8, device=dev)
    if out_off is None:
        out_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
    if out_len is None:
        out_len = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    if status is None:
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    _check(lib().hhuff_decode_batch_packed(_dp(data), in_size, _dp(in_off), n, _dp(is_name_bits), _dp(out),
                                           _dp(out_off), _dp(out_len), _dp(status), _stream(stream)),
           "hhuff_decode_batch_packed")
    return out, out_off, out_len, status


def encode_batch_packed(data, in_off, n, out=None, out_off=None, out_len=None, status=None, in_size=None, stream=None):
    """Batched h2o_hpack_encode_huffman with packed output (include/hhuff.h hhuff_encode_batch_packed):
    returns (out, out_off [n+1], out_len, status)."""
    import torch

    dev = data.device
    in_size = data.numel() if in_size is None else in_size
    if out is None:
        out = torch.empty(in_size + 16, dtype=torch.uint8, device=dev)
    if out_off is None:
        out_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
    if out_len is None:
        out_len = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    if status is None:
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    _check(lib().hhuff_encode_batch_packed(_dp(data), in_size, _dp(in_off), n, _dp(out), _dp(out_off), _dp(out_len),
                                           _dp(status), _stream(stream)), "hhuff_encode_batch_packed")
    return out, out_off, out_len, status


def flatten_batch(data, in_off, n, prefix_bits=7, in_len=None, first_bytes=None, raw_bits=None, out=None, out_off=None,
                  out_len=None, in_size=None, stream=None):
    """Batched QPACK flatten_string / HPACK h2o_hpack_encode_string framing; returns (out, out_len)."""
    import torch

    dev = data.device
    in_size = data.numel() if in_size is None else in_size
    if out is None:
        out = torch.empty(in_size + 11 * max(n, 1) + 16, dtype=torch.uint8, device=dev)
    if out_len is None:
        out_len = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    _check(lib().hhuff_flatten_batch(_dp(data), in_size, _dp(in_off), _dp(in_len), n, _dp(first_bytes), prefix_bits,
                                     _dp(raw_bits), _dp(out), _dp(out_off), _dp(out_len), _stream(stream)),
           "hhuff_flatten_batch")
    return out, out_len


LIT_QPACK = 1


def decode_literals(data, lit_off, lit_end, n, prefix_bits=7, qpack=False, is_name_bits=None, out=None, in_size=None,
                    stream=None):
    """Batched HPACK decode_string / QPACK literal decode on device tensors.
    Returns (out, out_len, pay_off, consumed, status); decoded bytes at out[floor(8 * pay_off / 5)]."""
    import torch

    dev = data.device
    in_size = data.numel() if in_size is None else in_size
    if out is None:
        out = torch.empty(decode_slot_size(in_size), dtype=torch.uint8, device=dev)
    m = max(n, 1)
    out_len = torch.empty(m, dtype=torch.int32, device=dev)
    pay_off = torch.empty(m, dtype=torch.int32, device=dev)
    consumed = torch.empty(m, dtype=torch.int32, device=dev)
    status = torch.empty(m, dtype=torch.uint8, device=dev)
    _check(lib().hhuff_decode_literals(_dp(data), in_size, _dp(lit_off), _dp(lit_end), n, prefix_bits,
                                       LIT_QPACK if qpack else 0, _dp(is_name_bits), _dp(out), _dp(out_len),
                                       _dp(pay_off), _dp(consumed), _dp(status), _stream(stream)), "hhuff_decode_literals")
    return out, out_len, pay_off, consumed, status


BLK_ARENA = -300
BLK_SKIPPED = -301
ERR_PROTOCOL = -1
ERR_COMPRESSION = -9


def default_arena_off(blk_off, table_size=4096):
    """u64 arena slice offsets per block (torch, on blk_off's device): a block of L bytes gets
    floor(8 L / 5) + (L / 4 + 1) * (table_size + 64) bytes -- literals expand at most 8/5, and an indexed
    field (>= 1 byte) copies at most one table entry"""
    import torch

    L = (blk_off[1:].to(torch.int64) & 0xFFFFFFFF) - (blk_off[:-1].to(torch.int64) & 0xFFFFFFFF)
    cap = (L * 8) // 5 + (L // 4 + 1) * (table_size + 64)
    out = torch.zeros(L.numel() + 1, dtype=torch.int64, device=blk_off.device)
    out[1:] = torch.cumsum(cap, 0)
    return out


BLK_CONTINUE = 1


# include/hhuff.h hhuff_request_t: 12 u32 words per block
REQUEST_FIELDS = ("content_length", "method", "scheme", "authority", "path", "protocol", "expect", "exists_map",
                  "nheaders", "err", "scheme_kind")
FIELD_HEADER = 0x4
# include/hhuff.h hhuff_response_t: 4 words per block; hhuff_qpack_response_head_t: 40 bytes per section
RESPONSE_FIELDS = ("status", "nheaders", "err", "datagram_flow_id")
QRES_BYTES = 40


def hpack_decode_blocks(data, blk_off, conn_first, table_size=4096, arena_off=None, in_size=None, stream=None,
                        scratch=None, cont=False, requests=False, responses=False, trailers=None, slots=None):
    """HPACK header blocks (include/hhuff.h hhuff_hpack_decode_blocks) on device tensors: blk_off / conn_first
    int32 tensors (u32 bits), arena_off int64.  Returns a dict of device tensors: arena, name_off, name_len,
    value_off, value_len, fflags (per field slot), nfields, bstatus (per block).  requests=True runs
    hhuff_hpack_parse_requests (h2o_hpack_parse_request per block) and adds req: int32 [nblk, 12], the
    hhuff_request_t words (REQUEST_FIELDS; content_length is words 0-1).  responses=True runs
    hhuff_hpack_parse_responses (h2o_hpack_parse_response per block; trailers: uint8 tensor, nonzero for a
    trailers block, or None) and adds res: int32 [nblk, 4], the hhuff_response_t words (RESPONSE_FIELDS).
    slots (ConnSlots): the _slots variants -- the scratch holds slots.nslots slabs and the listed connections use
    the ones slots.slot names."""
    import torch

    dev = data.device
    in_size = data.numel() if in_size is None else in_size
    nblk = blk_off.numel() - 1
    nconn = conn_first.numel() - 1
    if arena_off is None:
        arena_off = default_arena_off(blk_off, table_size)
    nslots = max(1, int(blk_off[-1].item()) & 0xFFFFFFFF)
    r = dict(arena=torch.empty(max(1, int(arena_off[-1].item())), dtype=torch.uint8, device=dev),
             name_off=torch.empty(nslots, dtype=torch.int32, device=dev),
             name_len=torch.empty(nslots, dtype=torch.int32, device=dev),
             value_off=torch.empty(nslots, dtype=torch.int32, device=dev),
             value_len=torch.empty(nslots, dtype=torch.int32, device=dev),
             fflags=torch.empty(nslots, dtype=torch.uint8, device=dev),
             nfields=torch.empty(max(1, nblk), dtype=torch.int32, device=dev),
             bstatus=torch.empty(max(1, nblk), dtype=torch.int32, device=dev))
    ss = int(lib().hhuff_hpack_scratch_size(nconn if slots is None else slots.nslots, table_size))
    if scratch is None:  # pass the previous call's r["scratch"] back with cont=True to carry the tables over
        scratch = torch.empty(max(16, ss), dtype=torch.uint8, device=dev)
    args = [_dp(data), in_size, _dp(blk_off), _dp(conn_first), nconn, table_size, _dp(r["arena"]), _dp(arena_off),
            _dp(r["name_off"]), _dp(r["name_len"]), _dp(r["value_off"]), _dp(r["value_len"]), _dp(r["fflags"]),
            _dp(r["nfields"]), _dp(r["bstatus"])]
    tail = [_dp(scratch), scratch.numel(), BLK_CONTINUE if cont else 0, _stream(stream)]
    if responses:
        r["res"] = torch.empty((max(1, nblk), 4), dtype=torch.int32, device=dev)
        _stateful("hhuff_hpack_parse_responses", slots,
                  [*args[:6], None if trailers is None else _dp(trailers), *args[6:], _dp(r["res"]), *tail])
    elif requests:
        r["req"] = torch.empty((max(1, nblk), 12), dtype=torch.int32, device=dev)
        _stateful("hhuff_hpack_parse_requests", slots, [*args, _dp(r["req"]), *tail])
    else:
        _stateful("hhuff_hpack_decode_blocks", slots, [*args, *tail])
    r["scratch"] = scratch  # keep alive until the stream has run the launch
    return r


QPK_CONTINUE = 1


QREQ_BYTES = 72  # sizeof(hhuff_qpack_request_t)


QDS_SYNC = QDS_SILENT = QDS_WAKE_PENDING = 1


def qpack_dsession_state_size(n, max_blocked=100):
    """include/hhuff.h hhuff_qpack_dsession_state_size"""
    return int(lib().hhuff_qpack_dsession_state_size(n, max_blocked))


def qpack_dsession_out_bound(nsec_of_conn, ncancel_of_conn=0):
    """include/hhuff.h hhuff_qpack_dsession_out_bound (numpy arrays, tensors or ints)"""
    return 10 * (nsec_of_conn + ncancel_of_conn) + 10


class QpackDsessions:
    """include/hhuff.h hhuff_qpack_dsessions_t for qpack_decode's sessions= argument.  state: the uint8 device tensor
    a previous step returned (None: allocated, for a first step).  cancel_first int32 (u32 bits) [nconn + 1],
    cancel_id int64, cancel_flags uint8 (QDS_SILENT): this step's cancellations, or None.  dec_out_off int64
    [nconn + 1] (None: every connection's region is exactly its bound), dec_out uint8; wake_first int32 [nconn + 1]
    (None: max_blocked entries a connection), wake_id int64; sync: QDS_SYNC."""

    def __init__(self, state=None, cancel_first=None, cancel_id=None, cancel_flags=None, dec_out_off=None, dec_out=None,
                 wake_first=None, wake_id=None, sync=False):
        self.state, self.cancel_first, self.cancel_id, self.cancel_flags = state, cancel_first, cancel_id, cancel_flags
        self.dec_out_off, self.dec_out, self.wake_first, self.wake_id, self.sync = dec_out_off, dec_out, wake_first, wake_id, sync


def _qpack_dsessions(ds, r, conn_first, nconn, nstate, max_blocked, dev):
    """fill in the defaults of `ds`, add its outputs to r -> the C struct (and what must stay alive with it)"""
    import torch

    if ds.dec_out_off is None:
        cnt = (conn_first[1:] - conn_first[:-1]).to(torch.int64)
        if ds.cancel_first is not None:
            cnt = cnt + (ds.cancel_first[1:] - ds.cancel_first[:-1]).to(torch.int64)
        ds.dec_out_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev),
                                    torch.cumsum(qpack_dsession_out_bound(cnt), 0)])
    if ds.dec_out is None:
        ds.dec_out = torch.empty(max(1, int(ds.dec_out_off[-1].item())), dtype=torch.uint8, device=dev)
    if ds.wake_first is None:
        ds.wake_first = (torch.arange(nconn + 1, dtype=torch.int64, device=dev) * max_blocked).to(torch.int32)
    if ds.wake_id is None:
        ds.wake_id = torch.empty(max(1, int(ds.wake_first[-1].item())), dtype=torch.int64, device=dev)
    if ds.state is None:
        ds.state = torch.empty(max(16, qpack_dsession_state_size(nstate, max_blocked)), dtype=torch.uint8, device=dev)
    i32 = lambda n: torch.empty(max(1, n), dtype=torch.int32, device=dev)  # noqa: E731
    r.update(dec_out=ds.dec_out, dec_out_off=ds.dec_out_off, dec_out_len=i32(nconn), wake_id=ds.wake_id,
             wake_first=ds.wake_first, nwake=i32(nconn), parked=i32(nconn),
             dflags=torch.empty(max(1, nconn), dtype=torch.uint8, device=dev), state=ds.state)
    return _QpackDsessionsStruct(_dp(ds.state), ds.state.numel(), _dp(ds.cancel_first), _dp(ds.cancel_id),
                                 _dp(ds.cancel_flags), _dp(ds.dec_out), _dp(ds.dec_out_off), _dp(r["dec_out_len"]),
                                 _dp(ds.wake_id), _dp(ds.wake_first), _dp(r["nwake"]), _dp(r["parked"]), _dp(r["dflags"]),
                                 QDS_SYNC if ds.sync else 0)


def qpack_decode(data, enc_off, enc_len, sec_off, conn_first, nsec, header_table_size=4096, max_blocked=100,
                 num_blocked=None, arena_off=None, in_size=None, stream=None, scratch=None, cont=False, arena=None,
                 stream_id=None, responses=False, slots=None, sessions=None):
    """QPACK decoder step (include/hhuff.h hhuff_qpack_decode) on device tensors: enc_off / enc_len (per
    connection), sec_off / conn_first / num_blocked int32 tensors (u32 bits), arena_off int64; nsec =
    conn_first[-1] as a host int.  Returns a dict of device tensors: arena, name_off, name_len, value_off,
    value_len, fflags (per field slot), nfields, sstatus, req_insert_count (per section), enc_status,
    enc_consumed, insert_count (per connection), and the scratch holding the tables (pass it back with
    cont=True for the next step).  stream_id (int64 tensor, one per section): the HTTP/3 request step,
    hhuff_qpack_parse_requests (h2o_qpack_parse_request per section), plus "req": uint8 [nsec, 72] records
    (hhuff_qpack_request_t).  responses=True (with stream_id): the HTTP/3 client's step,
    hhuff_qpack_parse_responses (h2o_qpack_parse_response per section), plus "res": uint8 [nsec, 40] records
    (hhuff_qpack_response_head_t).  slots (ConnSlots): the _slots variants (see hpack_decode_blocks).
    sessions (QpackDsessions, with stream_id; num_blocked must be None): hhuff_qpack_parse_requests_sessions /
    _parse_responses_sessions -- the parked streams and the decoder stream kept on the device; plus dec_out,
    dec_out_off, dec_out_len, wake_id, wake_first, nwake, parked, dflags and `state` (carry it like scratch:
    QpackDsessions(state=r["state"]) with cont=True)."""
    import torch

    dev = data.device
    in_size = data.numel() if in_size is None else in_size
    nconn = conn_first.numel() - 1
    if arena_off is None:
        arena_off = default_arena_off(sec_off, header_table_size)
    nslots = max(1, int(sec_off[-1].item()) & 0xFFFFFFFF)
    i32 = lambda n: torch.empty(max(1, n), dtype=torch.int32, device=dev)  # noqa: E731
    if arena is None:
        arena = torch.empty(max(1, int(arena_off[-1].item())), dtype=torch.uint8, device=dev)
    r = dict(arena=arena,
             name_off=i32(nslots), name_len=i32(nslots), value_off=i32(nslots), value_len=i32(nslots),
             fflags=torch.empty(nslots, dtype=torch.uint8, device=dev), nfields=i32(nsec), sstatus=i32(nsec),
             req_insert_count=torch.empty(max(1, nsec), dtype=torch.int64, device=dev), enc_status=i32(nconn),
             enc_consumed=i32(nconn), insert_count=torch.empty(max(1, nconn), dtype=torch.int64, device=dev))
    ss = int(lib().hhuff_qpack_scratch_size(nconn if slots is None else slots.nslots, header_table_size))
    if scratch is None:
        scratch = torch.empty(max(16, ss), dtype=torch.uint8, device=dev)
    args = [_dp(data), in_size, _dp(enc_off), _dp(enc_len), _dp(sec_off), _dp(conn_first), nconn, nsec,
            header_table_size, max_blocked, None if num_blocked is None else _dp(num_blocked), _dp(r["arena"]),
            _dp(arena_off), _dp(r["name_off"]), _dp(r["name_len"]), _dp(r["value_off"]), _dp(r["value_len"]),
            _dp(r["fflags"]), _dp(r["nfields"]), _dp(r["sstatus"]), _dp(r["req_insert_count"]), _dp(r["enc_status"]),
            _dp(r["enc_consumed"]), _dp(r["insert_count"])]
    tail = [_dp(scratch), scratch.numel(), QPK_CONTINUE if cont else 0, _stream(stream)]
    if sessions is not None:
        assert stream_id is not None and num_blocked is None, "sessions: a request / response step, no num_blocked"
        name = "hhuff_qpack_parse_responses_sessions" if responses else "hhuff_qpack_parse_requests_sessions"
        key, size = ("res", QRES_BYTES) if responses else ("req", QREQ_BYTES)
        r[key] = torch.empty((max(1, nsec), size), dtype=torch.uint8, device=dev)
        dst = _qpack_dsessions(sessions, r, conn_first, nconn, nconn if slots is None else slots.nslots, max_blocked, dev)
        st = None if slots is None else ctypes.byref(_ConnSlotsStruct(_dp(slots.slot), _dp(slots.flags), slots.nslots))
        _check(getattr(lib(), name)(ctypes.byref(dst), st, *(args[:10] + args[11:] + [_dp(stream_id), _dp(r[key])] + tail)),
               name)
    elif stream_id is None:
        _stateful("hhuff_qpack_decode", slots, args + tail)
    elif responses:
        r["res"] = torch.empty((max(1, nsec), QRES_BYTES), dtype=torch.uint8, device=dev)
        _stateful("hhuff_qpack_parse_responses", slots, args + [_dp(stream_id), _dp(r["res"])] + tail)
    else:
        r["req"] = torch.empty((max(1, nsec), QREQ_BYTES), dtype=torch.uint8, device=dev)
        _stateful("hhuff_qpack_parse_requests", slots, args + [_dp(stream_id), _dp(r["req"])] + tail)
    r["scratch"] = scratch
    return r


# include/hhuff.h hhuff_hpack_header_t / hhuff_hpack_response_t as numpy records
HPE_HEADER_DTYPE = np.dtype([("name_off", "<u4"), ("name_len", "<u4"), ("value_off", "<u4"), ("value_len", "<u4"),
                             ("flags", "<u4")])
HPE_RESPONSE_DTYPE = np.dtype([("content_length", "<u8"), ("stream_id", "<u4"), ("status", "<u4"),
                               ("hdr_first", "<u4"), ("nhdr", "<u4"), ("header_table_size", "<u4"),
                               ("max_frame_size", "<u4"), ("flags", "<u4"), ("parent_stream_id", "<u4")])
HDR_DONT_COMPRESS, HDR_TOKEN = 1, 2
RES_END_STREAM, RES_SERVER, RES_TRAILERS, RES_REQUEST = 1, 2, 4, 8
RES_PUSH_PROMISE = 16  # h2o_hpack_flatten_push_promise: stream_id is the promised stream, parent_stream_id the frames'
ENC_CONTINUE = 1
RES_SPACE, RES_SKIPPED, RES_EINVAL = -300, -301, -303


def hpack_response_bound(name_value_bytes, nhdr, server_len, max_frame_size):
    """include/hhuff.h hhuff_hpack_response_bound (numpy arrays or ints)"""
    payload = name_value_bytes + 21 * np.asarray(nhdr, np.int64) + 10 + 23 + np.where(
        np.asarray(server_len) != 0, np.asarray(server_len, np.int64) + 26, 0)
    return 9 + payload + 9 * (payload // np.maximum(np.asarray(max_frame_size, np.int64), 1) + 1)


QPE_RESPONSE_DTYPE = np.dtype([("content_length", "<u8"), ("status", "<u4"), ("hdr_first", "<u4"), ("nhdr", "<u4"),
                               ("flags", "<u4"), ("dfid_off", "<u4"), ("dfid_len", "<u4")])
QRES_DATAGRAM, QRES_REQUEST = 8, 16


def qpack_response_bound(name_value_bytes, nhdr, server_len, dfid_len):
    """include/hhuff.h hhuff_qpack_response_bound (numpy arrays or ints)"""
    sl = np.asarray(server_len, np.int64)
    return (9 + 2 + 8 + 23 + 26 + np.asarray(dfid_len, np.int64) + np.where(sl != 0, sl + 12, 0) +
            21 * np.asarray(nhdr, np.int64) + name_value_bytes)


def qpack_flatten_responses(data, hdr, res, nres, out_off, server_off=0, server_len=0, in_size=None, out=None,
                            stream=None, out_len=None, header_len=None, rstatus=None):
    """HTTP/3 response HEADERS frames (include/hhuff.h hhuff_qpack_flatten_responses) on device tensors: hdr =
    uint8 tensor of HPE_HEADER_DTYPE records, res = uint8 tensor of QPE_RESPONSE_DTYPE records (32 B), out_off
    int64 [nres + 1].  Returns a dict of device tensors: out, out_len, header_len, rstatus (the caller's int32
    tensors of nres entries where given, else new ones)."""
    import torch

    dev = data.device
    in_size = data.numel() if in_size is None else in_size
    nhdr = hdr.numel() // HPE_HEADER_DTYPE.itemsize
    if out is None:
        out = torch.empty(max(1, int(out_off[-1].item())), dtype=torch.uint8, device=dev)
    i32 = lambda n: torch.empty(max(1, n), dtype=torch.int32, device=dev)  # noqa: E731
    r = dict(out=out, out_len=i32(nres) if out_len is None else out_len,
             header_len=i32(nres) if header_len is None else header_len, rstatus=i32(nres) if rstatus is None else rstatus)
    _check(lib().hhuff_qpack_flatten_responses(
        _dp(data), in_size, _dp(hdr) if nhdr else None, nhdr, _dp(res), nres, server_off, server_len, _dp(out),
        _dp(out_off), _dp(r["out_len"]), _dp(r["header_len"]), _dp(r["rstatus"]), _stream(stream)),
        "hhuff_qpack_flatten_responses")
    return r


# include/hhuff.h (2g'): QPACK encoder sessions
HDR_LIKELY_TO_REPEAT = 4
QRES_NO_ENCODER_STREAM = 32
QENC_CONTINUE, QENC_SET_CAPACITY, QENC_EVICT, QENC_DUP = 1, 2, 4, 8
QPK_DECODER_STREAM = 0x30202
QPK_DECOMPRESSION_FAILED = 0x30200
QPK_SKIPPED, QPK_BLOCKED = -301, -302
# include/hhuff.h (2g''): hhuff_qpack_peer_t, a connection's peer settings
QPACK_PEER = np.dtype([("max_table_capacity", "<u4"), ("max_blocked", "<u4")])


def qpack_session_response_bound(name_value_bytes, nhdr, server_len, dfid_len):
    """include/hhuff.h hhuff_qpack_session_response_bound (numpy arrays or ints)"""
    return qpack_response_bound(name_value_bytes, nhdr, server_len, dfid_len) + 8


def qpack_session_enc_bound(name_value_bytes_of_ltr_headers, n_ltr_headers, server_len, nres_of_conn):
    """include/hhuff.h hhuff_qpack_session_enc_bound (numpy arrays or ints): a connection's encoder-stream region
    for one step with evict=True"""
    return 4 + name_value_bytes_of_ltr_headers + 20 * n_ltr_headers + (nres_of_conn * (26 + server_len) if server_len else 0)


def qpack_enc_scratch_size(nconn, header_table_size=4096, max_inflight=64):
    """include/hhuff.h hhuff_qpack_enc_scratch_size"""
    return int(lib().hhuff_qpack_enc_scratch_size(nconn, header_table_size, max_inflight))


def qpack_flatten_sessions(data, hdr, res, conn_first, nres, stream_id, out_off, dec_off=None, dec_len=None,
                           header_table_size=4096, max_blocked=100, max_inflight=64, server_off=0, server_len=0,
                           enc_out_off=None, in_size=None, out=None, enc_out=None, scratch=None, cont=False,
                           set_capacity=False, stream=None, evict=False, dup=False, slots=None, peers=None,
                           peers_call=False):
    """One step of many QPACK encoder sessions (include/hhuff.h hhuff_qpack_flatten_sessions) on device tensors:
    hdr = uint8 tensor of HPE_HEADER_DTYPE records, res = uint8 tensor of QPE_RESPONSE_DTYPE records, conn_first
    int32 (u32 bits) [nconn + 1], stream_id int64 per response, out_off int64 [nres + 1], dec_off / dec_len int32
    per connection (the decoder streams in `data`; None = none), enc_out_off int64 [nconn + 1] (None:
    header_table_size + 4 bytes per connection).  nres = conn_first[-1] as a host int.  Returns a dict of device
    tensors: out, out_len, header_len, rstatus, rflags (per response), enc_out, enc_out_off, enc_out_len,
    dec_status, dec_consumed (per connection) and the scratch holding the sessions (pass it back with cont=True
    for the connections' next step).  evict=True: HHUFF_QENC_EVICT, on every step of a session or on none; give
    enc_out_off then (qpack_session_enc_bound), since header_table_size + 4 bytes need not hold a step's inserts.
    dup=True: HHUFF_QENC_DUP, with evict=True only and likewise on every step or on none: entries about to be pinned
    as the oldest are re-inserted by a Duplicate instruction.  slots (ConnSlots): hhuff_qpack_flatten_sessions_slots
    (see hpack_decode_blocks); a connection with CONN_RESET is a new encoder in its slot.  peers: a uint8 device
    tensor of nconn QPACK_PEER records (hhuff_qpack_flatten_sessions_peers): every connection's table capacity,
    clamped to header_table_size, Required Insert Count modulus and blocked-stream limit, capped by max_blocked, come
    from its own peer's settings, the same record in every step of the connection's life.  peers_call: take that entry
    point with peers None too (its pass-through to the _slots call)."""
    import torch

    dev = data.device
    in_size = data.numel() if in_size is None else in_size
    nconn = conn_first.numel() - 1
    nhdr = hdr.numel() // HPE_HEADER_DTYPE.itemsize
    if peers is not None:
        assert peers.dtype == torch.uint8 and peers.numel() == nconn * QPACK_PEER.itemsize, "one QPACK_PEER per connection"
    if enc_out_off is None:
        enc_out_off = torch.arange(nconn + 1, dtype=torch.int64, device=dev) * ((header_table_size + 4 + 15) // 16 * 16)
    if out is None:
        out = torch.empty(max(1, int(out_off[-1].item())), dtype=torch.uint8, device=dev)
    if enc_out is None:
        enc_out = torch.empty(max(1, int(enc_out_off[-1].item())), dtype=torch.uint8, device=dev)
    i32 = lambda n: torch.empty(max(1, n), dtype=torch.int32, device=dev)  # noqa: E731
    r = dict(out=out, out_len=i32(nres), header_len=i32(nres), rstatus=i32(nres),
             rflags=torch.empty(max(1, nres), dtype=torch.uint8, device=dev), enc_out=enc_out, enc_out_off=enc_out_off,
             enc_out_len=i32(nconn), dec_status=i32(nconn), dec_consumed=i32(nconn))
    ss = qpack_enc_scratch_size(nconn if slots is None else slots.nslots, header_table_size, max_inflight)
    if scratch is None:
        scratch = torch.empty(max(16, ss), dtype=torch.uint8, device=dev)
    flags = (QENC_CONTINUE if cont else 0) | (QENC_SET_CAPACITY if set_capacity else 0) | (QENC_EVICT if evict else 0) | \
        (QENC_DUP if dup else 0)
    args = [
        _dp(data), in_size, _dp(hdr) if nhdr else None, nhdr, _dp(res), _dp(conn_first), nconn, nres, _dp(stream_id),
        _dp(dec_off), _dp(dec_len), header_table_size, max_blocked, max_inflight, server_off, server_len, _dp(out),
        _dp(out_off), _dp(r["out_len"]), _dp(r["header_len"]), _dp(r["rstatus"]), _dp(r["rflags"]), _dp(enc_out),
        _dp(enc_out_off), _dp(r["enc_out_len"]), _dp(r["dec_status"]), _dp(r["dec_consumed"]), _dp(scratch),
        scratch.numel(), flags, _stream(stream)]
    if peers is None and not peers_call:
        _stateful("hhuff_qpack_flatten_sessions", slots, args)
    else:
        st = None if slots is None else _ConnSlotsStruct(_dp(slots.slot), _dp(slots.flags), slots.nslots)
        _check(lib().hhuff_qpack_flatten_sessions_peers(_dp(peers), None if st is None else ctypes.byref(st), *args),
               "hhuff_qpack_flatten_sessions_peers")
    r["scratch"] = scratch
    return r


# include/hhuff.h (2k): hhuff_h2_frame_t / hhuff_h2_block_t as numpy records, and the section's constants
H2_FRAME_DTYPE = np.dtype([("payload_off", "<u4"), ("length", "<u4"), ("stream_id", "<u4"), ("type", "u1"), ("flags", "u1"),
                           ("rsv", "<u2"), ("frag_off", "<u4"), ("frag_len", "<u4"), ("block", "<u4"), ("rsv2", "<u4")])
H2_BLOCK_DTYPE = np.dtype([("stream_id", "<u4"), ("end_stream_id", "<u4"), ("flags", "<u4"), ("dependency", "<u4"),
                           ("weight", "<u4"), ("promised_stream_id", "<u4"), ("first_frame", "<u4"), ("nframes", "<u4")])
H2F_ACCEPT_PUSH = 1
H2F_REFUSED, H2F_FRAMES = -310, -311
ERR_FRAME_SIZE = -6
(H2F_ERR_NONE, H2F_ERR_HEADERS_STREAM_ID, H2F_ERR_HEADERS_FRAME, H2F_ERR_HEADERS_PRIORITY, H2F_ERR_EXPECTED_CONTINUATION,
 H2F_ERR_INVALID_CONTINUATION, H2F_ERR_PUSH_PROMISE, H2F_ERR_PROMISE_STREAM_ID, H2F_ERR_PROMISE_FRAME) = range(9)
H2B_END_STREAM, H2B_PRIORITY, H2B_EXCLUSIVE, H2B_CONTINUED, H2B_PROMISE, H2B_SELF_DEPENDENCY = 1, 2, 4, 8, 16, 32
H2O_MAX_REQLEN = 417792  # the server's max_block_bytes (8192 + 4096 * H2O_MAX_HEADERS); the client passes 0


def h2_deframe(data, in_off, frm_first, frm_cap, max_frame_size=16384, max_block_bytes=0, flags=0, in_size=None,
               arena_fixed=None, arena_per_byte=0, stream=None, out=None):
    """HTTP/2 de-framer (include/hhuff.h hhuff_h2_deframe) on device tensors: data uint8, in_off / frm_first int32 (u32
    bits) of nconn + 1 entries, frm_cap = frm_first[-1] as a host int.  Returns a dict of device tensors: frames (uint8,
    H2_FRAME_DTYPE records), nframes, consumed, cstatus, cerr (per connection), blk, blk_off [frm_cap + 1], conn_first,
    blocks (uint8, H2_BLOCK_DTYPE records), totals [2] and, with arena_fixed given, arena_off (int64 [frm_cap + 1]).
    blk, blk_off and conn_first go to hpack_decode_blocks as they are (in_size = blk.numel()).  out: a dict with
    some of these tensors preallocated.  No host synchronisation."""
    import torch

    dev = data.device
    in_size = data.numel() if in_size is None else in_size
    nconn = in_off.numel() - 1
    out = dict(out or {})
    new = lambda k, n, dt: out.setdefault(k, torch.empty(max(1, n), dtype=dt, device=dev))  # noqa: E731
    i32 = torch.int32
    r = dict(frames=new("frames", frm_cap * 32, torch.uint8), nframes=new("nframes", nconn, i32),
             consumed=new("consumed", nconn, i32), cstatus=new("cstatus", nconn, i32), cerr=new("cerr", nconn, i32),
             blk=new("blk", in_size, torch.uint8), blk_off=new("blk_off", frm_cap + 1, i32),
             conn_first=new("conn_first", nconn + 1, i32), blocks=new("blocks", frm_cap * 32, torch.uint8),
             totals=new("totals", 2, i32))
    if arena_fixed is not None:
        r["arena_off"] = new("arena_off", frm_cap + 1, torch.int64)
    _check(lib().hhuff_h2_deframe(_dp(data), in_size, _dp(in_off), nconn, _dp(frm_first), frm_cap, max_frame_size,
                                  max_block_bytes, flags, _dp(r["frames"]), _dp(r["nframes"]), _dp(r["consumed"]),
                                  _dp(r["cstatus"]), _dp(r["cerr"]), _dp(r["blk"]), _dp(r["blk_off"]), _dp(r["conn_first"]),
                                  _dp(r["blocks"]), _dp(r["totals"]), _dp(r.get("arena_off")), arena_fixed or 0,
                                  arena_per_byte, _stream(stream)), "hhuff_h2_deframe")
    return r


# include/hhuff.h (2k'): hhuff_h2_peer_t / hhuff_h2_ctl_t as numpy records, and the section's constants
H2_PEER_DTYPE = np.dtype([("header_table_size", "<u4"), ("enable_push", "<u4"), ("max_concurrent_streams", "<u4"),
                          ("initial_window_size", "<u4"), ("max_frame_size", "<u4"), ("flags", "<u4"), ("send_window", "<i8"),
                          ("recv_window", "<i8")])
H2_CTL_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("status", "<i4"), ("err", "<u2"), ("flags", "u1"), ("reply_len", "u1")])
H2_PEER_INIT = (4096, 1, 0xFFFFFFFF, 65535, 16384, 0, 65535, 65535)  # HHUFF_H2_PEER_INIT
H2C_CLIENT = 1
H2C_SPACE, H2C_EINVAL = -312, -313
ERR_FLOW_CONTROL = -3  # H2O_HTTP2_ERROR_FLOW_CONTROL (ERR_PROTOCOL, ERR_FRAME_SIZE: above)
H2P_SETTINGS, H2P_GOAWAY = 1, 2
H2R_ACK, H2R_NEEDS_STREAM, H2R_STREAM_ERROR, H2R_WINDOW_DELTA, H2R_WINDOW_UPDATE = 1, 2, 4, 8, 16
(H2C_ERR_NONE, H2C_ERR_DATA_STREAM_ID, H2C_ERR_DATA_FRAME, H2C_ERR_PRIORITY_STREAM_ID, H2C_ERR_PRIORITY_FRAME,
 H2C_ERR_SELF_DEPENDENCY, H2C_ERR_RST_STREAM_STREAM_ID, H2C_ERR_RST_STREAM_FRAME, H2C_ERR_SETTINGS_STREAM_ID,
 H2C_ERR_SETTINGS_ACK, H2C_ERR_SETTINGS_FRAME, H2C_ERR_SETTINGS_SIZE, H2C_ERR_PING_FRAME, H2C_ERR_GOAWAY_STREAM_ID,
 H2C_ERR_GOAWAY_FRAME, H2C_ERR_WINDOW_UPDATE_FRAME, H2C_ERR_FLOW_CONTROL) = range(17)
H2O_CONNECTION_WINDOW_SIZE = 16777216  # the server's recv_window_size (H2O_HTTP2_SETTINGS_HOST_CONNECTION_WINDOW_SIZE)


def h2_control_reply_bound(slots):
    """include/hhuff.h hhuff_h2_control_reply_bound"""
    return 17 * slots


def h2_new_peers(nconn, device=None):
    """nconn records of HHUFF_H2_PEER_INIT: a numpy array of H2_PEER_DTYPE, or with `device` a uint8 tensor there"""
    p = np.empty(nconn, H2_PEER_DTYPE)
    p[:] = H2_PEER_INIT
    if device is None:
        return p
    import torch

    return torch.from_numpy(p.view(np.uint8).copy()).to(device)


def h2_control(data, frames, nframes, frm_first, frm_cap, peers, rep_off, flags=0, recv_window_size=0, in_size=None,
               rep_size=None, stream=None, out=None):
    """HTTP/2 control frames (include/hhuff.h hhuff_h2_control) on device tensors: data, frames, nframes, frm_first and
    frm_cap are h2_deframe's; peers a uint8 tensor of H2_PEER_DTYPE records (h2_new_peers), rep_off int32 (u32 bits) of
    nconn + 1 entries.  Returns a dict of device tensors: ctl (uint8, H2_CTL_DTYPE records, one per frame slot), nctl,
    cstatus, cerr, rep_len (per connection), rep and peers (the records to present next time: a new tensor unless
    out={"peers": peers} updates in place).  out: a dict with some of these tensors preallocated.  No host
    synchronisation (rep_size given, or rep preallocated)."""
    import torch

    dev = data.device
    in_size = data.numel() if in_size is None else in_size
    nconn = frm_first.numel() - 1
    out = dict(out or {})
    if "rep" not in out and rep_size is None:
        rep_size = int(rep_off[-1].item()) & 0xFFFFFFFF
    new = lambda k, n, dt: out.setdefault(k, torch.empty(max(1, n), dtype=dt, device=dev))  # noqa: E731
    i32, u8 = torch.int32, torch.uint8
    r = dict(ctl=new("ctl", frm_cap * 16, u8), nctl=new("nctl", nconn, i32), cstatus=new("cstatus", nconn, i32),
             cerr=new("cerr", nconn, i32), rep_len=new("rep_len", nconn, i32), rep=new("rep", rep_size or 0, u8),
             peers=new("peers", nconn * 40, u8))
    if rep_size is None:
        rep_size = r["rep"].numel()
    _check(lib().hhuff_h2_control(_dp(data), in_size, _dp(frames), _dp(nframes), _dp(frm_first), frm_cap, nconn, flags,
                                  recv_window_size, _dp(peers), _dp(r["peers"]), _dp(r["ctl"]), _dp(r["nctl"]),
                                  _dp(r["cstatus"]), _dp(r["cerr"]), _dp(r["rep"]), rep_size, _dp(rep_off), _dp(r["rep_len"]),
                                  _stream(stream)), "hhuff_h2_control")
    return r


def hpack_responses_set_peers(peers, res, conn_first, nres, stream=None):
    """include/hhuff.h hhuff_hpack_responses_set_peers: the peers' header_table_size and max_frame_size (uint8 tensor of
    H2_PEER_DTYPE records) into the HPE_RESPONSE_DTYPE records `res` (uint8 tensor), in place; conn_first int32 (u32
    bits) [nconn + 1]"""
    _check(lib().hhuff_hpack_responses_set_peers(_dp(peers), _dp(res), _dp(conn_first), conn_first.numel() - 1, nres,
                                                 _stream(stream)), "hhuff_hpack_responses_set_peers")


# include/hhuff.h (2k''): hhuff_h2_send_t / hhuff_h2_sent_t as numpy records, and the section's constants
H2_SEND_DTYPE = np.dtype([("body_off", "<u4"), ("body_len", "<u4"), ("stream_id", "<u4"), ("window", "<i4"), ("flags", "<u4"),
                          ("max_frames", "<u4")])
H2_SENT_DTYPE = np.dtype([("sent", "<u4"), ("nframes", "<u4"), ("out_off", "<u4"), ("flags", "<u4"), ("window", "<i4"),
                          ("rsv", "<u4")])
H2S_FINAL, H2S_TRAILERS = 1, 2
H2T_END_STREAM, H2T_DONE, H2T_STREAM_WINDOW, H2T_ROOM, H2T_CONN_WINDOW, H2T_MAX_FRAMES = 1, 2, 4, 8, 16, 32
H2D_EINVAL = -314


def h2_frame_data(body, sends, send_first, peers, out_off, flags=0, body_size=None, nsend=None, out_size=None, stream=None,
                  out=None):
    """HTTP/2 DATA frames on the send side (include/hhuff.h hhuff_h2_frame_data) on device tensors: body uint8, sends a
    uint8 tensor of H2_SEND_DTYPE records, send_first / out_off int32 (u32 bits) of nconn + 1 entries, peers a uint8
    tensor of H2_PEER_DTYPE records.  Returns a dict of device tensors: sent (uint8, H2_SENT_DTYPE records, one per send
    record), out_len, cstatus (per connection), out (the frames) and peers (the records to present next time: a new
    tensor unless out={"peers": peers} updates in place).  out: a dict with some of these tensors preallocated.  No
    host synchronisation (out_size given, or out["out"] preallocated)."""
    import torch

    dev = body.device
    body_size = body.numel() if body_size is None else body_size
    nsend = sends.numel() // 24 if nsend is None else nsend
    nconn = send_first.numel() - 1
    out = dict(out or {})
    if "out" not in out and out_size is None:
        out_size = int(out_off[-1].item()) & 0xFFFFFFFF
    new = lambda k, n, dt: out.setdefault(k, torch.empty(max(1, n), dtype=dt, device=dev))  # noqa: E731
    i32, u8 = torch.int32, torch.uint8
    r = dict(sent=new("sent", nsend * 24, u8), out_len=new("out_len", nconn, i32), cstatus=new("cstatus", nconn, i32),
             out=new("out", out_size or 0, u8), peers=new("peers", nconn * 40, u8))
    if out_size is None:
        out_size = r["out"].numel()
    _check(lib().hhuff_h2_frame_data(_dp(body), body_size, _dp(sends), _dp(send_first), nsend, nconn, flags, _dp(peers),
                                     _dp(r["peers"]), _dp(r["sent"]), _dp(r["out"]), out_size, _dp(out_off), _dp(r["out_len"]),
                                     _dp(r["cstatus"]), _stream(stream)), "hhuff_h2_frame_data")
    return r


# include/hhuff.h (2k'''): hhuff_h2_sev_t / hhuff_h2_stream_op_t as numpy records, and the section's constants
H2_SEV_DTYPE = np.dtype([("stream_id", "<u4"), ("a", "<u4"), ("status", "<i2"), ("err", "<u2"), ("flags", "<u4")])
H2_STREAM_OP_DTYPE = np.dtype([("stream_id", "<u4"), ("op", "<u4"), ("arg", "<u4"), ("rsv", "<u4")])
H2ST_CONTINUE = 1
H2SP_STREAM_BODIES = 1
H2O_CLOSE, H2O_CREDIT, H2O_OPEN_PUSH = 1, 2, 3
H2ST_SPACE, H2ST_EINVAL, H2ST_EFULL, H2ST_ENOENT, H2ST_ESLOT = -315, -316, -317, -318, -319
(H2SE_OPENED, H2SE_BODY, H2SE_REQUEST_COMPLETE, H2SE_TRAILERS, H2SE_RESET_BY_PEER, H2SE_RESET_SENT, H2SE_WINDOW_UPDATE_SENT,
 H2SE_IGNORED, H2SE_PRIORITY_ONLY_OPENED, H2SE_SEND_WINDOW_OPENED, H2SE_BAD_CONNECT, H2SE_INVALID_HEADER_CHAR,
 H2SE_PRIORITY) = (1 << i for i in range(13))
(H2ST_ERR_NONE, H2ST_ERR_HEADERS_STREAM_ID, H2ST_ERR_HEADERS_CLOSED, H2ST_ERR_TUNNEL_TRAILERS, H2ST_ERR_TRAILERS_END_STREAM,
 H2ST_ERR_SELF_DEPENDENCY, H2ST_ERR_CONTINUATION_STREAM_ID, H2ST_ERR_DATA_FRAME, H2ST_ERR_TOO_MANY_IDLE,
 H2ST_ERR_RST_STREAM_STREAM_ID, H2ST_ERR_WINDOW_UPDATE_STREAM_ID, H2ST_ERR_TRAILERS_PSEUDO_HEADER, H2ST_ERR_TRAILERS_HOST,
 H2ST_ERR_HEADER_BLOCK) = range(14)


def h2_streams_params(p):
    """hhuff_h2_streams_params_t of a dict with its fields' names (rsv 0)"""
    return _H2StreamsParamsStruct(p["max_streams"], p["max_streams_for_priority"], p["active_stream_window_size"], p["max_entries"],
                                  p["max_request_entity_size"], p["flags"], 0)


def h2_streams_scratch_size(nslots, max_entries) -> int:
    """include/hhuff.h hhuff_h2_streams_scratch_size; 0: a max_entries the calls refuse"""
    return int(lib().hhuff_h2_streams_scratch_size(nslots, max_entries))


def h2_streams_entries(max_streams, max_streams_for_priority, max_push):
    """include/hhuff.h hhuff_h2_streams_entries"""
    return min(max_streams + 1 + max_streams_for_priority + max_push, 0xFFFFFFFF)


def h2_streams_reply_bound(frame_slots, nops):
    """include/hhuff.h hhuff_h2_streams_reply_bound"""
    return 43 * frame_slots + 13 * nops


def _slots_ref(slots):
    return None if slots is None else ctypes.byref(_ConnSlotsStruct(_dp(slots.slot), _dp(slots.flags), slots.nslots))


def h2_streams(params, scratch, data, frames, nframes, frm_first, frm_cap, ctl, nctl, ctl_rep, ctl_rep_off, blocks, conn_first,
               bstatus, req, arena, blk_off, value_off, value_len, peers, rep_off, ops=None, op_first=None, flags=0, slots=None,
               in_size=None, ctl_rep_size=None, arena_size=None, rep_size=None, stream=None, out=None):
    """The HTTP/2 stream table (include/hhuff.h hhuff_h2_streams) on device tensors: params a dict (h2_streams_params),
    scratch a uint8 tensor of h2_streams_scratch_size bytes kept between calls (flags=H2ST_CONTINUE), data .. frm_cap
    h2_deframe's, ctl / nctl / ctl_rep / ctl_rep_off h2_control's ctl, nctl, rep and rep_off, blocks / conn_first the
    de-framer's, bstatus / req / arena / blk_off / value_off / value_len hpack_parse_requests', peers h2_control's, ops a
    uint8 tensor of H2_STREAM_OP_DTYPE records with op_first int32 [nconn + 1], rep_off int32 [nconn + 1], slots a ConnSlots.
    Returns a dict of device tensors: sev (uint8, H2_SEV_DTYPE records, one per frame slot), op_sev, nstr, sstatus, serr,
    rep_len (per connection) and rep.  No host synchronisation (rep_size given, or out["rep"] preallocated)."""
    import torch

    dev = frames.device
    nconn = frm_first.numel() - 1
    nops = 0 if ops is None else ops.numel() // 16
    out = dict(out or {})
    if "rep" not in out and rep_size is None:
        rep_size = int(rep_off[-1].item()) & 0xFFFFFFFF
    new = lambda k, n, dt: out.setdefault(k, torch.empty(max(1, n), dtype=dt, device=dev))  # noqa: E731
    i32, u8 = torch.int32, torch.uint8
    r = dict(sev=new("sev", frm_cap * 16, u8), op_sev=new("op_sev", nops * 16, u8), nstr=new("nstr", nconn, i32),
             sstatus=new("sstatus", nconn, i32), serr=new("serr", nconn, i32), rep_len=new("rep_len", nconn, i32),
             rep=new("rep", rep_size or 0, u8))
    size = lambda t, given: t.numel() if given is None else given  # noqa: E731
    _check(lib().hhuff_h2_streams(_slots_ref(slots), h2_streams_params(params), _dp(data), size(data, in_size), _dp(frames),
                                  _dp(nframes), _dp(frm_first), frm_cap, _dp(ctl), _dp(nctl), _dp(ctl_rep), size(ctl_rep, ctl_rep_size),
                                  _dp(ctl_rep_off), _dp(blocks), _dp(conn_first), _dp(bstatus), _dp(req), _dp(arena),
                                  size(arena, arena_size), _dp(blk_off), _dp(value_off), _dp(value_len), _dp(peers), _dp(ops),
                                  _dp(op_first), nops, nconn, _dp(r["sev"]), _dp(r["op_sev"]), _dp(r["nstr"]), _dp(r["sstatus"]),
                                  _dp(r["serr"]), _dp(r["rep"]), size(r["rep"], rep_size), _dp(rep_off), _dp(r["rep_len"]),
                                  _dp(scratch), scratch.numel(), flags, _stream(stream)), "hhuff_h2_streams")
    return r


def h2_streams_fill_sends(max_entries, scratch, sends, send_first, slots=None, nsend=None, stream=None, miss=None):
    """include/hhuff.h hhuff_h2_streams_fill_sends: the streams' send windows into the H2_SEND_DTYPE records `sends` (uint8
    tensor, in place); returns miss (uint8 per record: 1 no such stream, 2 listed earlier in the connection's range)"""
    import torch

    nsend = sends.numel() // 24 if nsend is None else nsend
    if miss is None:
        miss = torch.empty(max(1, nsend), dtype=torch.uint8, device=sends.device)
    _check(lib().hhuff_h2_streams_fill_sends(_slots_ref(slots), max_entries, _dp(scratch), scratch.numel(), _dp(sends),
                                             _dp(send_first), nsend, send_first.numel() - 1, _dp(miss), _stream(stream)),
           "hhuff_h2_streams_fill_sends")
    return miss


def h2_streams_commit_sent(max_entries, scratch, sends, sent, send_first, slots=None, nsend=None, stream=None):
    """include/hhuff.h hhuff_h2_streams_commit_sent: what h2_frame_data sent leaves the streams' send windows"""
    nsend = sends.numel() // 24 if nsend is None else nsend
    _check(lib().hhuff_h2_streams_commit_sent(_slots_ref(slots), max_entries, _dp(scratch), scratch.numel(), _dp(sends), _dp(sent),
                                              _dp(send_first), nsend, send_first.numel() - 1, _stream(stream)),
           "hhuff_h2_streams_commit_sent")


# include/hhuff.h (2l): hhuff_h3_stream_t / hhuff_h3_frame_t / hhuff_h3_settings_t as numpy records (peers: QPACK_PEER), and
# the section's constants
H3_STREAM_DTYPE = np.dtype([("stream_id", "<u8"), ("data_left", "<u8"), ("kind", "u1"), ("phase", "u1"), ("flags", "u1"),
                            ("rsv", "u1", (13,))])
H3_FRAME_DTYPE = np.dtype([("type", "<u8"), ("hdr_off", "<u4"), ("payload_off", "<u4"), ("length", "<u8"), ("avail", "<u4"),
                           ("aux", "<u4")])
H3_SETTINGS_DTYPE = np.dtype([("max_field_section_size", "<u8"), ("h3_datagram", "<u4"), ("rsv", "<u4")])
H3F_CLIENT = 1
H3F_REJECTED, H3F_FRAMES, H3F_EINVAL = -320, -321, -322
H3_GENERAL_PROTOCOL, H3_FRAME_UNEXPECTED, H3_FRAME, H3_EXCESSIVE_LOAD = 0x30101, 0x30105, 0x30106, 0x30107
(H3F_ERR_NONE, H3F_ERR_FRAME_TOO_LARGE, H3F_ERR_UNEXPECTED_TYPE, H3F_ERR_DATA_BEFORE_HEADERS, H3F_ERR_RESPONSE_TOO_LARGE,
 H3F_ERR_MALFORMED_SETTINGS, H3F_ERR_INVALID_PRIORITY, H3F_ERR_INVALID_GOAWAY) = range(8)
H3K_REQUEST, H3K_UNI, H3K_CONTROL, H3K_QPACK_ENCODER, H3K_QPACK_DECODER, H3K_DISCARD = range(6)
H3P_HEADERS, H3P_DATA, H3P_DATA_PAYLOAD, H3P_POST_TRAILERS = range(4)
H3P_SETTINGS, H3P_OPEN = 0, 1
H3S_WALK_ON, H3S_TUNNEL, H3S_PEER_DATAGRAMS = 1, 2, 4


def h3_deframe(data, str_off, conn_str, frm_first, frm_cap, st_in, max_frame_payload_size=16384, flags=0, in_size=None,
               arena_fixed=None, arena_per_byte=0, stream=None, out=None):
    """HTTP/3 de-framer (include/hhuff.h hhuff_h3_deframe) on device tensors: data uint8, str_off / frm_first int32 (u32
    bits) of nstr + 1 entries, conn_str of nconn + 1, frm_cap = frm_first[-1] as a host int, st_in uint8 (H3_STREAM_DTYPE
    records, 32 bytes a stream).  Returns a dict of device tensors: st_out (out={"st_out": st_in} updates in place),
    frames (uint8, H3_FRAME_DTYPE records), nframes, consumed, sstatus, serr (per stream), out, enc_off, enc_len,
    conn_first (per connection), sec_off [nstr + 1], sec_stream_id (int64) and sec_stream [nstr], totals [3], peers
    (uint8, QPACK_PEER), settings (uint8, H3_SETTINGS_DTYPE), got_settings and, with arena_fixed given, arena_off
    (int64 [nstr + 1]).  out, enc_off, enc_len, sec_off, conn_first and sec_stream_id go to qpack_decode as they are
    (in_size = out.numel()).  out: a dict with some of these tensors preallocated -- a persistent peers array among
    them.  No host synchronisation."""
    import torch

    dev = data.device
    in_size = data.numel() if in_size is None else in_size
    nstr, nconn = str_off.numel() - 1, conn_str.numel() - 1
    out = dict(out or {})
    new = lambda k, n, dt: out.setdefault(k, torch.empty(max(1, n), dtype=dt, device=dev))  # noqa: E731
    i32, u8 = torch.int32, torch.uint8
    r = dict(st_out=new("st_out", nstr * 32, u8), frames=new("frames", frm_cap * 32, u8), nframes=new("nframes", nstr, i32),
             consumed=new("consumed", nstr, i32), sstatus=new("sstatus", nstr, i32), serr=new("serr", nstr, i32),
             out=new("out", in_size, u8), enc_off=new("enc_off", nconn, i32), enc_len=new("enc_len", nconn, i32),
             sec_off=new("sec_off", nstr + 1, i32), conn_first=new("conn_first", nconn + 1, i32),
             sec_stream_id=new("sec_stream_id", nstr, torch.int64), sec_stream=new("sec_stream", nstr, i32),
             totals=new("totals", 3, i32), peers=new("peers", nconn * 8, u8), settings=new("settings", nconn * 16, u8),
             got_settings=new("got_settings", nconn, i32))
    if arena_fixed is not None:
        r["arena_off"] = new("arena_off", nstr + 1, torch.int64)
    _check(lib().hhuff_h3_deframe(_dp(data), in_size, _dp(str_off), nstr, _dp(conn_str), nconn, _dp(frm_first), frm_cap,
                                  max_frame_payload_size, flags, _dp(st_in), _dp(r["st_out"]), _dp(r["frames"]),
                                  _dp(r["nframes"]), _dp(r["consumed"]), _dp(r["sstatus"]), _dp(r["serr"]), _dp(r["out"]),
                                  _dp(r["enc_off"]), _dp(r["enc_len"]), _dp(r["sec_off"]), _dp(r["conn_first"]),
                                  _dp(r["sec_stream_id"]), _dp(r["sec_stream"]), _dp(r["totals"]), _dp(r["peers"]),
                                  _dp(r["settings"]), _dp(r["got_settings"]), _dp(r.get("arena_off")), arena_fixed or 0,
                                  arena_per_byte, _stream(stream)), "hhuff_h3_deframe")
    return r


def hpack_flatten_responses(data, hdr, res, conn_first, nres, out_off, server_off=0, server_len=0, in_size=None,
                            out=None, scratch=None, cont=False, stream=None, slots=None, out_len=None, headers_size=None,
                            rstatus=None):
    """HTTP/2 response header blocks (include/hhuff.h hhuff_hpack_flatten_responses) on device tensors:
    hdr = uint8 tensor of HPE_HEADER_DTYPE records (20 B each), res = uint8 tensor of HPE_RESPONSE_DTYPE
    records (40 B), conn_first int32 (u32 bits), out_off int64 [nres + 1]; nres = conn_first[-1] as a host int.
    Returns a dict of device tensors: out, out_len, headers_size, rstatus (the caller's int32 tensors of nres entries
    where given, else new ones), and the scratch holding the encoder tables (pass it back with cont=True for the
    connections' next responses).  slots (ConnSlots):
    hhuff_hpack_flatten_responses_slots (see hpack_decode_blocks)."""
    import torch

    dev = data.device
    in_size = data.numel() if in_size is None else in_size
    nconn = conn_first.numel() - 1
    nhdr = hdr.numel() // HPE_HEADER_DTYPE.itemsize
    if out is None:
        out = torch.empty(max(1, int(out_off[-1].item())), dtype=torch.uint8, device=dev)
    i32 = lambda n: torch.empty(max(1, n), dtype=torch.int32, device=dev)  # noqa: E731
    r = dict(out=out, out_len=i32(nres) if out_len is None else out_len,
             headers_size=i32(nres) if headers_size is None else headers_size,
             rstatus=i32(nres) if rstatus is None else rstatus)
    ss = int(lib().hhuff_hpack_enc_scratch_size(nconn if slots is None else slots.nslots))
    if scratch is None:
        scratch = torch.empty(max(16, ss), dtype=torch.uint8, device=dev)
    _stateful("hhuff_hpack_flatten_responses", slots, [
        _dp(data), in_size, _dp(hdr) if nhdr else None, nhdr, _dp(res), _dp(conn_first), nconn, nres, server_off,
        server_len, _dp(out), _dp(out_off), _dp(r["out_len"]), _dp(r["headers_size"]), _dp(r["rstatus"]),
        _dp(scratch), scratch.numel(), ENC_CONTINUE if cont else 0, _stream(stream)])
    r["scratch"] = scratch
    return r


# ---------------------------------------------------------------------------------------------------
# host batch API (numpy arrays; H2D/D2H inside the library)
# ---------------------------------------------------------------------------------------------------
def _np(a, dt):
    """a C-contiguous numpy view of `a` with dtype dt (u32 data may arrive as int32)"""
    a = np.asarray(a)
    if a.dtype != dt:
        a = a.view(dt) if a.dtype.itemsize == np.dtype(dt).itemsize else a.astype(dt)
    return np.ascontiguousarray(a)


def _hp(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


def decode_batch_host(data, in_off, n, in_len=None, is_name_bits=None, out_off=None, out_size=None, device=0):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    if out_size is None:
        out_size = decode_slot_size(data.size)
    out = np.zeros(max(1, out_size), np.uint8)
    out_len = np.zeros(max(1, n), np.uint32)
    status = np.zeros(max(1, n), np.uint8)
    _check(lib().hhuff_decode_batch_host(_hp(data), data.size, _hp(in_off), _hp(in_len), n, _hp(is_name_bits), _hp(out),
                                         out.size, _hp(out_off), _hp(out_len), _hp(status), device),
           "hhuff_decode_batch_host")
    return out, out_len[:n], status[:n]


def encode_batch_host(data, in_off, n, in_len=None, out_off=None, out_size=None, device=0):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    if out_size is None:
        out_size = data.size + 16
    out = np.zeros(max(1, out_size), np.uint8)
    out_len = np.zeros(max(1, n), np.uint32)
    status = np.zeros(max(1, n), np.uint8)
    _check(lib().hhuff_encode_batch_host(_hp(data), data.size, _hp(in_off), _hp(in_len), n, _hp(out), out.size,
                                         _hp(out_off), _hp(out_len), _hp(status), device), "hhuff_encode_batch_host")
    return out, out_len[:n], status[:n]


def decode_batch_host_pipelined(data, in_off, n, is_name_bits=None, out=None, chunk_bytes=0, device=0, out_len=None,
                                status=None):
    """Pipelined host decode (contiguous layout).  Caller buffers may be pinned memory (DMA'd in place)."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    if out is None:
        out = np.zeros(decode_slot_size(data.size), np.uint8)
    out_len = np.zeros(max(1, n), np.uint32) if out_len is None else out_len
    status = np.zeros(max(1, n), np.uint8) if status is None else status
    _check(lib().hhuff_decode_batch_host_pipelined(_hp(data), data.size, _hp(in_off), n, _hp(is_name_bits), _hp(out),
                                                   out.size, _hp(out_len), _hp(status), device, chunk_bytes),
           "hhuff_decode_batch_host_pipelined")
    return out, out_len[:n], status[:n]


def encode_batch_host_pipelined(data, in_off, n, out=None, chunk_bytes=0, device=0, out_len=None, status=None):
    """Pipelined host encode (contiguous layout, output slot = in_off)."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    if out is None:
        out = np.zeros(data.size + 16, np.uint8)
    out_len = np.zeros(max(1, n), np.uint32) if out_len is None else out_len
    status = np.zeros(max(1, n), np.uint8) if status is None else status
    _check(lib().hhuff_encode_batch_host_pipelined(_hp(data), data.size, _hp(in_off), n, _hp(out), out.size,
                                                   _hp(out_len), _hp(status), device, chunk_bytes),
           "hhuff_encode_batch_host_pipelined")
    return out, out_len[:n], status[:n]


def decode_batch_host_packed(data, in_off, n, is_name_bits=None, out=None, device=0, out_off=None, out_len=None,
                             status=None, with_off=True):
    """hhuff_decode_batch_host_packed on numpy arrays: the packed layout (tile runs, out_off[n + 1]); pinned arrays are
    read and written by the kernels in place (zero copy).  Returns (out, out_off[:n + 1], out_len[:n], status[:n]);
    with_off=False passes out_off NULL (not returned, out_off None: see packed_positions)"""
    data, in_off = _np(data, np.uint8), _np(in_off, np.uint32)
    size = decode_slot_size(int(in_off[n]))
    out = np.zeros(size, np.uint8) if out is None else out
    out_off = None if not with_off else np.zeros(n + 1, np.uint32) if out_off is None else out_off
    out_len = np.zeros(max(1, n), np.uint32) if out_len is None else out_len
    status = np.zeros(max(1, n), np.uint8) if status is None else status
    names = None if is_name_bits is None else _np(is_name_bits, np.uint32)
    _check(lib().hhuff_decode_batch_host_packed(_hp(data), data.size, _hp(in_off), n, _hp(names), _hp(out), out.size,
                                                _hp(out_off), _hp(out_len), _hp(status), device),
           "hhuff_decode_batch_host_packed")
    return out, None if out_off is None else out_off[:n + 1], out_len[:n], status[:n]


def encode_batch_host_packed(data, in_off, n, out=None, device=0, out_off=None, out_len=None, status=None,
                             with_off=True, with_status=True):
    """hhuff_encode_batch_host_packed on numpy arrays (see decode_batch_host_packed; with_status=False passes
    status NULL: out_len's HHUFF_FAIL_LEN already says which strings stay plain)"""
    data, in_off = _np(data, np.uint8), _np(in_off, np.uint32)
    out = np.zeros(int(in_off[n]) + 16, np.uint8) if out is None else out
    out_off = None if not with_off else np.zeros(n + 1, np.uint32) if out_off is None else out_off
    out_len = np.zeros(max(1, n), np.uint32) if out_len is None else out_len
    status = None if not with_status else np.zeros(max(1, n), np.uint8) if status is None else status
    _check(lib().hhuff_encode_batch_host_packed(_hp(data), data.size, _hp(in_off), n, _hp(out), out.size, _hp(out_off),
                                                _hp(out_len), _hp(status), device),
           "hhuff_encode_batch_host_packed")
    return (out, None if out_off is None else out_off[:n + 1], out_len[:n],
            None if status is None else status[:n])


HOST_MEMORY = -1


def shard_bounds(in_off, n, nshards, align=64):
    """hhuff_shard_bounds: the C library's byte-balanced cut of a contiguous batch (host arrays, no GPU work)
    -> uint32 bounds[nshards + 1]"""
    in_off = _np(in_off, np.uint32)
    b = np.zeros(nshards + 1, np.uint32)
    _check(lib().hhuff_shard_bounds(_hp(in_off), n, nshards, align, _hp(b)), "hhuff_shard_bounds")
    return b


def _devs(devices):
    arr = (ctypes.c_int * len(devices))(*devices)
    return arr, ctypes.cast(arr, _vp)


def decode_batch_multi(devices, data, in_off, n, is_name_bits=None, out=None, out_len=None, status=None, stream=None):
    """hhuff_decode_batch_multi.  numpy arrays: the host mode (every device runs its shard through the host path);
    torch tensors on one device: the device mode (shards on other devices by peer copy), asynchronous on `stream`.
    Returns (out, out_len, status) in the one-device slot layout"""
    devs, dp = _devs(devices)
    if isinstance(data, np.ndarray):
        data, in_off = _np(data, np.uint8), _np(in_off, np.uint32)
        out = np.zeros(decode_slot_size(int(in_off[n])), np.uint8) if out is None else out
        out_len = np.zeros(max(1, n), np.uint32) if out_len is None else out_len
        status = np.zeros(max(1, n), np.uint8) if status is None else status
        names = None if is_name_bits is None else _np(is_name_bits, np.uint32)
        _check(lib().hhuff_decode_batch_multi(len(devices), dp, HOST_MEMORY, _hp(data), data.size, _hp(in_off), n,
                                              _hp(names), _hp(out), out.size, _hp(out_len), _hp(status), None),
               "hhuff_decode_batch_multi")
        return out, out_len[:n], status[:n]
    import torch

    dev = data.device
    if out is None:
        out = torch.empty(decode_slot_size(data.numel()), dtype=torch.uint8, device=dev)
    if out_len is None:
        out_len = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    if status is None:
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    _check(lib().hhuff_decode_batch_multi(len(devices), dp, dev.index, _dp(data), data.numel(), _dp(in_off), n,
                                          _dp(is_name_bits), _dp(out), out.numel(), _dp(out_len), _dp(status),
                                          _stream(stream)), "hhuff_decode_batch_multi")
    return out, out_len, status


def encode_batch_multi(devices, data, in_off, n, out=None, out_len=None, status=None, stream=None):
    """hhuff_encode_batch_multi (see decode_batch_multi)"""
    devs, dp = _devs(devices)
    if isinstance(data, np.ndarray):
        data, in_off = _np(data, np.uint8), _np(in_off, np.uint32)
        out = np.zeros(int(in_off[n]) + 16, np.uint8) if out is None else out
        out_len = np.zeros(max(1, n), np.uint32) if out_len is None else out_len
        status = np.zeros(max(1, n), np.uint8) if status is None else status
        _check(lib().hhuff_encode_batch_multi(len(devices), dp, HOST_MEMORY, _hp(data), data.size, _hp(in_off), n,
                                              _hp(out), out.size, _hp(out_len), _hp(status), None),
               "hhuff_encode_batch_multi")
        return out, out_len[:n], status[:n]
    import torch

    dev = data.device
    if out is None:
        out = torch.empty(data.numel() + 16, dtype=torch.uint8, device=dev)
    if out_len is None:
        out_len = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    if status is None:
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    _check(lib().hhuff_encode_batch_multi(len(devices), dp, dev.index, _dp(data), data.numel(), _dp(in_off), n,
                                          _dp(out), out.numel(), _dp(out_len), _dp(status), _stream(stream)),
           "hhuff_encode_batch_multi")
    return out, out_len, status


def packed_positions(in_off, out_len, decode):
    """Where the packed layout put each string when out_off was not returned: tile t = i // 64 starts at its slot
    position (decode floor(8 in_off[64 t] / 5), encode in_off[64 t]) and its strings follow back to back; failed
    strings (HHUFF_FAIL_LEN) take no bytes.  Returns int64 starts[n]"""
    in_off = np.asarray(in_off, np.int64)
    ln = np.asarray(out_len, np.uint32)
    n = ln.size
    kept = np.where(ln == FAIL_LEN, 0, ln).astype(np.int64)
    t0 = np.arange(0, n, 64)
    base = in_off[t0] * 8 // 5 if decode else in_off[t0]
    cs = np.cumsum(kept) - kept                                  # exclusive prefix over the batch
    return np.repeat(base - cs[t0], np.diff(np.append(t0, n))) + cs


def decode_prices(device=0):
    """the staged / stream prices (ps per string, per byte, each kernel) the mixed-length decode of `device`
    uses (include/hhuff.h hhuff_decode_prices: fitted defaults until calibrated or pinned; no GPU work)"""
    buf = (ctypes.c_float * 4)()
    _check(lib().hhuff_decode_prices(device, buf), "hhuff_decode_prices")
    return [float(x) for x in buf]


def calibrate_decode_prices(device=0):
    """measure `device`'s prices now and use them from then on (hhuff_calibrate_decode_prices; synchronous)"""
    buf = (ctypes.c_float * 4)()
    _check(lib().hhuff_calibrate_decode_prices(device, buf), "hhuff_calibrate_decode_prices")
    return [float(x) for x in buf]


def set_decode_prices(prices, device=0):
    """pin `device`'s prices (4 floats), or restore the fitted defaults with None (hhuff_set_decode_prices)"""
    buf = None if prices is None else (ctypes.c_float * 4)(*[float(x) for x in prices])
    _check(lib().hhuff_set_decode_prices(device, buf), "hhuff_set_decode_prices")


def set_edge_defer_min(n):
    """batches of at least n strings defer their tiles' shared 16-B chunks to edge records and a fix-up kernel
    (hhuff_set_edge_defer_min; default 2^32 - 1: never); returns the previous threshold"""
    return int(lib().hhuff_set_edge_defer_min(int(n)))


def set_decode_kernel(mode):
    """which kernel decodes contiguous batches (hhuff_set_decode_kernel): 0 (default) the staged / stream choice;
    1 / 2 (the segment kernel above a 40-B mean / always) only in A/B builds (HhuffError here); returns the
    previous mode"""
    r = lib().hhuff_set_decode_kernel(int(mode))
    if r < 0:
        _check(r, "hhuff_set_decode_kernel")
    return r
