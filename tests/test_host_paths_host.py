"""The host-path model and corpora (tests/host_paths_model.py, tests/host_paths_corpora.py) checked without a GPU:
  - the model's constants are the ones in the sources;
  - every case's predicate holds: the edge its name claims is there;
  - over the corpus the chunk starts hit every residue mod 5 and mod 16, and their slots at least 8 residues mod 16;
  - the emulators with no defect equal the oracle's whole-batch result on every case;
  - each address defect the emulators can switch on is caught, by the checker the GPU tests use, on the cases
    CATCHES names;
  - the host entry points refuse a contiguous batch whose strings leave `in` or whose slots leave `out`, before any
    device call (the library loads without a GPU)."""
import os
import re

import numpy as np
import pytest

import bounds_harness as H
import host_paths_corpora as C
import host_paths_model as M
from conftest import ROOT

CSRC = os.path.join(ROOT, "h2o_amd", "csrc")
B_SMALL = 4096  # the packed staging boundary of the emulator runs


@pytest.fixture(scope="module")
def corpus():
    return C.corpus()


@pytest.fixture(scope="module")
def packed():
    return C.packed_corpus(B_SMALL)


# ------------------------------------------------------------------------------------------------
# the constants
# ------------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


def _int(text, pattern):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return int(m[0])


def test_constants_match_the_sources():
    """host_paths_model.py against hhuff_hostplan.h (the arithmetic), hhuff_capi_host.hip (the routes and the chunk
    loop), hhuff_host.h (the launch the chunks go through) and hhuff_kernels.hip.  A retuned constant fails here: move
    it in the model with the source, and the corpora's edges follow.  (What the arithmetic next to the constants
    computes is test_hostplan_host.py's: the header run against the model.)"""
    plan, host, shared, k = _src("hhuff_hostplan.h"), _src("hhuff_capi_host.hip"), _src("hhuff_host.h"), _src("hhuff_kernels.hip")
    assert _int(plan, r"constexpr int kDepth = (\d+);") == M.K_DEPTH
    assert _int(plan, r"constexpr uint64_t kDefaultChunk = (\d+)ull << 20;") << 20 == M.DEFAULT_CHUNK
    assert "if (!in_len && !out_off && in_size >= 2 * kDefaultChunk) // large contiguous batch" in host
    assert M.ROUTE_MIN == 2 * M.DEFAULT_CHUNK
    assert plan.count("if (chunk_bytes == 0) chunk_bytes = kDefaultChunk;") == 1
    assert plan.count("b = b > a + 32 ? ((b - a) / 32) * 32 + a : a + 32;") == 1 and M.CUT_ALIGN == 32
    assert plan.count("const uint64_t base = (s0 / 80) * 80;") == 1 and M.BASE_ALIGN == 80
    assert "const std::vector<uint64_t> cut = chunk_cuts(in_off, n, chunk_bytes);" in host
    assert "const ChunkLayout L = chunk_layout(decode, in_off[i0], e0, m, is_name_bits != nullptr);" in host
    assert "is_name_bits + i0 / 32" in host and "Slot& x = P.slot[k % kDepth];" in host
    # the chunk's launch: its e0 as in_size, its nbytes as sel_bytes -- launch_slots hands both on in those places
    assert "const uint64_t e0 = in_off[i1];" in host and "nbytes = L.nbytes," in host
    assert host.count("launch_slots(decode, d_in, e0, d_off, nullptr, (uint32_t)m, d_nm, d_out, nullptr, d_len,") == 1
    assert host.count("status ? d_st : nullptr, x.s, nbytes);") == 1
    assert "inline hipError_t launch_slots(bool decode, const uint8_t* in, uint64_t in_size, const uint32_t* in_off, " \
           "const uint32_t* in_len, uint32_t n, const uint32_t* names, uint8_t* out, const uint32_t* out_off, " \
           "uint32_t* out_len, uint8_t* status, hipStream_t stream, uint64_t sel_bytes = 0) {" in shared
    assert "hhuff::launch_decode(in, in_size, in_off, in_len, n, names, out, out_off, out_len, status, stream, sel_bytes)" in shared
    assert "hhuff::launch_encode(in, in_size, in_off, in_len, n, out, out_off, out_len, status, stream, sel_bytes);" in shared
    assert _int(plan, r"constexpr size_t kPackedChunk = \(size_t\)(\d+) << 20;") << 20 == M.PACKED_CHUNK
    assert "const size_t chunk = kPackedChunk;" in host
    assert plan.count("inline uint32_t packed_ntiles(uint32_t n) { return (n + 63) / 64; }") == 1
    assert plan.count("in_off[(size_t)t * 64]") == 1 and M.TILE == 64
    assert "const uint32_t ntiles = packed_ntiles(n);" in host
    assert _int(k, r"constexpr uint32_t kSplitMin = (\d+);") == M.SPLIT_MIN
    assert _int(k, r"constexpr uint32_t kSplitMinFew = (\d+);") == M.SPLIT_MIN_FEW
    m = re.search(r"constexpr uint32_t kSplitBig = (\d+), kSplitBigFew = (\d+);", k)
    assert (int(m.group(1)), int(m.group(2))) == (M.SPLIT_BIG, M.SPLIT_BIG_FEW)
    assert _int(k, r"const uint32_t smin = n <= (\d+)u \? kSplitMinFew : kSplitMin;") == M.SPLIT_FEW_N
    assert _int(k, r"const bool split = bytes >= smin && \(bytes / n >= (\d+)u \|\| n <= 16u\);") == M.SPLIT_MEAN
    assert "A.big_min = n <= 16u ? kSplitBigFew : kSplitBig;" in k
    assert "const uint64_t bytes = sel_bytes ? sel_bytes : in_size;" in k
    assert "if (mean <= %d) return kDecS; if (mean <= %d) return kDecL; return kDecT;" % (M.DEC_SHORT_MAX, M.DEC_MIXED_MAX) in k
    assert "if (mean <= %d) return kEncS; if (mean <= %d) return kEncL; return kEncD;" % (M.ENC_SORTED_MAX, M.ENC_LANES_MAX) in k
    assert _int(k, r"constexpr uint64_t kEncPlMean = (\d+);") == M.ENC_SORTED_MAX + 1
    assert _int(k, r"#define HHUFF_ENCO_SMALL_MEAN (\d+)") == M.ENC_SMALL_MEAN
    assert "#define HHUFF_DEFER_MIN 0x%Xu" % M.DEFER_NEVER in k
    assert "static bool defer_edges(uint32_t n) { return n >= g_defer_min.load(std::memory_order_relaxed); }" in k


def test_cut_rule():
    """cuts() on offsets small enough to check by hand"""
    off = np.arange(0, 10 * 101, 10)  # 100 strings of 10 B
    assert M.cuts(off, 100, 1) == [0, 32, 64, 96, 100]
    assert M.cuts(off, 100, 319) == [0, 32, 64, 96, 100]       # the target inside string 31
    # string 64 starts at the target: 65 rounds down to 64.  The rounding holds at the batch's end too: from 64 the
    # search ends behind in_off[n] (36 + 1 entries on), which rounds down to 96 and leaves a chunk of 4 strings
    assert M.cuts(off, 100, 640) == [0, 64, 96, 100] and M.cuts(off, 100, 650) == [0, 64, 96, 100]
    assert M.cuts(off, 100, 959) == [0, 96, 100] and M.cuts(off, 100, 960) == [0, 96, 100]
    assert M.cuts(off, 100, 1 << 40) == [0, 96, 100] and M.cuts(off, 96, 1 << 40) == [0, 96]
    assert M.cuts(off + 7, 100, 640) == [0, 64, 96, 100] and M.cuts(off, 1, 1) == [0, 1] and M.cuts(off, 33, 0) == [0, 32, 33]
    assert M.cuts(np.zeros(71, np.int64), 70, 1) == [0, 64, 70]  # empty strings: none starts past the target
    p = M.plan("decode", off + 163, 100, 1)
    assert [(c.base, c.nbytes, c.olo, c.obase, c.slot) for c in p[:2]] == [(160, 323, 260, 256, 0), (480, 323, 772, 768, 1)]
    assert p[3].slot == 0 and p[3].m == 4 and p[3].smin == M.SPLIT_MIN_FEW and p[0].family == "short"
    assert all(c.obase % 16 == 0 for c in p)


# ------------------------------------------------------------------------------------------------
# the corpora
# ------------------------------------------------------------------------------------------------
def _exp(oracle, case, fill=0x00, sentinel=0xA5, **kw):
    a = case.arrays(fill, sentinel, **kw)
    return (a,) + C.expected(oracle, case, a)


def test_every_predicate_holds(oracle_codec, corpus, packed):
    assert len(corpus) > 100 and len(packed) == 10
    for c in corpus + packed:
        assert c.n <= 300 and c.n == len(c.strings), c.label
        _, exp, _, _ = _exp(oracle_codec, c)
        assert c.holds(c, c.plan(), exp), "%s: not %s" % (c.label, c.why)
    labels = [c.label for c in corpus + packed]
    assert len(set(labels)) == len(labels)


def test_corpus_groups(corpus):
    for op in ("decode", "encode"):
        mine = [c for c in corpus if c.op == op]
        assert {c.group for c in mine} == {"counts", "empties", "offsets", "lengths", "families", "seams"}
        counts = {len(c.plan()) for c in mine if c.group == "counts" and c.chunk_bytes == 1}
        assert counts >= {1, 2, M.K_DEPTH, M.K_DEPTH + 1, 2 * M.K_DEPTH + 1}
        assert {c.n for c in mine if c.group == "counts"} >= {1, 31, 32, 33, 63, 64, 65, 97, 225}
        assert any(c.plan()[-1].m == 1 and len(c.plan()) > 1 for c in mine)
        assert {c.in_off0 for c in mine if c.group == "offsets"} == set(C.OFFSETS)
        fams = {x.family for c in mine if c.group == "families" for x in c.plan()}
        assert fams == set(C.BANDS[op])
        assert any(c.defer == 64 for c in mine)
        # what the multi-device host mode runs: a first string off zero and fewer strings than a shard's alignment
        assert sum(1 for c in mine if c.in_off0 != 0 and c.n < 64) >= 8


def test_residue_coverage(corpus):
    """chunk starts s0 at every residue mod 5 (where floor(8 s0 / 5) rounds) and mod 16 (where the chunk's bytes sit
    in a 16-B load), and their slots at 8 residues mod 16 and more (floor(8 s / 5) takes 10 of them)"""
    for op in ("decode", "encode"):
        chunks = [x for c in corpus if c.op == op for x in c.plan()]
        assert {x.s0 % 5 for x in chunks} == set(range(5))
        assert {x.s0 % 16 for x in chunks} == set(range(16))
        assert {x.s0 % 80 == 0 for x in chunks} == {True, False}
        assert len({x.olo % 16 for x in chunks}) >= (8 if op == "decode" else 16)
        assert all(x.obase % 16 == 0 for x in chunks)


def test_emulators_equal_the_oracle(oracle_codec, corpus, packed):
    """no defect: the chunk-by-chunk restatement gives the whole-batch result, under both fill / sentinel pairs and
    both documented sizes of `out`"""
    for c in corpus:
        for (fill, sentinel), exact in zip(H.RUNS, (True, False)):
            a, exp, mask, starts = _exp(oracle_codec, c, fill, sentinel, exact=exact)
            for cb in {c.chunk_bytes, 1}:
                res = M.emulate_pipelined(oracle_codec, c.op, a, cb)
                H.check(res, exp, mask, sentinel, starts=starts, label=c.label)
    for c in packed + [x for x in corpus if x.group in ("seams", "offsets")]:
        for fill, sentinel in H.RUNS:
            for with_off in (True, False):
                a, exp, mask = _packed_exp(oracle_codec, c, fill, sentinel, with_off)
                res = M.emulate_packed_staged(oracle_codec, c.op, a, c.boundary or B_SMALL)
                H.check(res, exp, mask, sentinel, starts=exp["out_off"][:c.n] if with_off else _starts(c, exp), label=c.label)


def _packed_exp(oracle, c, fill, sentinel, with_off=True, with_status=True):
    a = c.arrays(fill, sentinel, with_off=with_off, with_status=with_status)
    _, slots = H.oracle_run(oracle, c.op, a, sentinel, names=a["names"])
    exp, mask = M.packed_from_slots(c.op, a["in_off"], c.n, slots)
    if not with_off:
        del exp["out_off"]
    if not with_status:
        del exp["status"]
    return a, exp, mask


def _starts(c, exp):
    from h2o_amd import codec

    return codec.packed_positions(c.off()[:c.n], exp["out_len"], c.op == "decode")


# defect -> (operation, part of the label) of a case that must catch it (others may too)
CATCHES = {
    "a": ("decode", "name flags at the word seams"),   # an unrounded cut reads the name word from bit 0
    "b": ("decode", "in_off0=7 n=97"),                 # chunk starts off a multiple of 5: slots of a rebased chunk shift
    "c": ("decode", "n=97 chunk_bytes=1"),             # the whole-slot string at each chunk's end loses its last byte
    "d": ("encode", "n=97 chunk_bytes=1"),
    "e": ("encode", "n=33 chunk_bytes=1"),
    "f": ("decode", "n=65 chunk_bytes=1"),             # 31 entries into the rear guards of out_len and status
    "g": ("decode", "name flags at the word seams"),
    "h": ("encode", "n=193 chunk_bytes=1"),            # seven chunks: chunks 0..3 are lost
    "i": ("encode", "packed straddles"),
    "j": ("decode", "packed starts at"),
    "k": ("decode", "packed empty at"),
    "l": ("encode", "packed ends at"),
}


def _caught(oracle, c, defect):
    for fill, sentinel in H.RUNS:
        try:
            if defect in M.PIPELINED_DEFECTS:
                a, exp, mask, starts = _exp(oracle, c, fill, sentinel)
                res = M.emulate_pipelined(oracle, c.op, a, c.chunk_bytes, defect)
            else:
                a, exp, mask = _packed_exp(oracle, c, fill, sentinel)
                starts = exp["out_off"][:c.n]
                res = M.emulate_packed_staged(oracle, c.op, a, c.boundary, defect)
            H.check(res, exp, mask, sentinel, starts=starts, label=c.label)
        except AssertionError:
            return True
    return False


@pytest.mark.parametrize("defect", sorted(M.DEFECTS))
def test_defect_is_caught(oracle_codec, corpus, packed, defect):
    """the corpus tells every modelled address defect from the right code -- with bounds_harness.check(), as on the
    GPU.  The named case must catch it; the count of others that do is asserted to be more than that one"""
    op, part = CATCHES[defect]
    cases = corpus if defect in M.PIPELINED_DEFECTS else packed
    named = [c for c in cases if c.op == op and c.label.startswith("%s %s" % (op, part))]
    assert len(named) == 1, (defect, [c.label for c in named])
    assert _caught(oracle_codec, named[0], defect), "%s (%s) passes on %s" % (defect, M.DEFECTS[defect], named[0].label)
    others = [c.label for c in cases if c is not named[0] and _caught(oracle_codec, c, defect)]
    assert others, "only %s catches defect %s" % (named[0].label, defect)
    for o in ("decode", "encode"):  # both directions, where the direction can show it at all
        if (defect, o) not in (("a", "encode"), ("g", "encode"), ("b", "encode"), ("c", "encode")):
            assert any(x.startswith(o) for x in others + [named[0].label]), (defect, o)


def test_arena():
    a = H.Arena(np.zeros(4096, np.uint8))
    for off in (0, 1, 15):
        whole, inner = a.guarded(33, 0x5A, off)
        assert inner.ctypes.data % 16 == off and inner.size == 33 and whole.size == 33 + 2 * H.GUARD
        assert inner.ctypes.data - whole.ctypes.data == H.GUARD and (whole == 0x5A).all()
    src, _ = H.guarded(np, 10, 7)
    w, i = a.copy(src, 3)
    assert (w == 7).all() and i.size == 10 and i.ctypes.data % 16 == 3
    with pytest.raises(AssertionError):
        a.guarded(4096, 0)
    a.reset()
    assert a.guarded(100, 1)[0].size == 100 + 2 * H.GUARD


# ------------------------------------------------------------------------------------------------
# refusals (include/hhuff.h (3), (3b)): before any device call, so they need no GPU
# ------------------------------------------------------------------------------------------------
def _host_calls(L, off, in_size, out_size, n, only=""):
    """every host entry point of the contiguous implicit layout (whose name holds `only`) on dummy arrays:
    -> {name: (rc, message)}.  The data pointers are never valid: make only calls that must be refused"""
    p, o = 1 << 20, off.ctypes.data
    calls = {
        "decode_batch_host": lambda: L.hhuff_decode_batch_host(p, in_size, o, None, n, None, p, out_size, None, p, p, 0),
        "encode_batch_host": lambda: L.hhuff_encode_batch_host(p, in_size, o, None, n, p, out_size, None, p, p, 0),
        "decode_batch_host_pipelined": lambda: L.hhuff_decode_batch_host_pipelined(p, in_size, o, n, None, p, out_size, p, p,
                                                                                 0, 4096),
        "encode_batch_host_pipelined": lambda: L.hhuff_encode_batch_host_pipelined(p, in_size, o, n, p, out_size, p, None, 0,
                                                                                 4096),
        "decode_batch_host_packed": lambda: L.hhuff_decode_batch_host_packed(p, in_size, o, n, None, p, out_size, p, p, p, 0),
        "encode_batch_host_packed": lambda: L.hhuff_encode_batch_host_packed(p, in_size, o, n, p, out_size, None, p, None, 0),
    }
    out = {}
    for name, f in calls.items():
        if only not in name:
            continue
        rc = f()
        out[name] = (rc, L.hhuff_last_error_string().decode())
    return out


@pytest.mark.parametrize("in_size", [1000, M.ROUTE_MIN])  # the one-piece route and the pipeline of hhuff_*_batch_host
def test_host_calls_refuse_sizes_the_batch_leaves(in_size):
    """in_off[n] > in_size and out_size below slot_of(in_off[n]) (decode floor(8 in_off[n] / 5), encode in_off[n]):
    refused by every host entry point of the contiguous layout with the packed and multi-device calls' messages.
    The pointers are dummies: nothing but in_off is read before the refusal"""
    from h2o_amd import codec

    L = codec.lib()
    n = 65
    off = np.arange(n + 1, dtype=np.uint32) * 10 + 350  # in_off[n] = 1000
    end = int(off[n])
    for name, (rc, err) in _host_calls(L, off, end - 1, 1 << 40, n).items():
        assert rc == -1 and err == "invalid argument: in_off[n] > in_size", (name, rc, err)
    for name, (rc, err) in _host_calls(L, off, max(in_size, end), 0, n).items():
        assert rc == -1 and err == "invalid argument: out_size below the output slots of the batch", (name, rc, err)
    for name, (rc, err) in _host_calls(L, off, max(in_size, end), end - 1, n).items():  # too short for either direction
        assert rc == -1 and err == "invalid argument: out_size below the output slots of the batch", (name, rc, err)
    short = _host_calls(L, off, max(in_size, end), (8 * end) // 5 - 1, n, only="decode")  # one byte short of its slots
    assert len(short) == 3
    for name, (rc, err) in short.items():
        assert rc == -1 and err == "invalid argument: out_size below the output slots of the batch", (name, rc, err)


def test_multi_host_mode_refuses_a_short_out():
    from h2o_amd import codec

    L = codec.lib()
    p = 1 << 20
    off = np.arange(66, dtype=np.uint32) * 10
    # (ndev is checked against the device count first: without a GPU that is the refusal, with one the size is)
    rc = L.hhuff_encode_batch_multi(1, None, -1, p, 650, off.ctypes.data, 65, p, 649, p, p, None)
    assert rc != 0
    err = L.hhuff_last_error_string().decode()
    assert "out_size below the output slots of the batch" in err or "device" in err.lower() or "hip" in err.lower(), err
