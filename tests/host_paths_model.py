"""A plain-Python model of the host-array batch paths of h2o_amd/csrc/hhuff_capi_host.hip (`pipelined`, `host_packed`;
`host_batch` and hhuff_capi_multi.hip's `multi_host` route into them), whose arithmetic is hhuff_hostplan.h -- no GPU.

  cuts() / plan()          the chunk cuts of `pipelined` and, per chunk, its addresses, staging slot, the kernel
                           family its own mean picks, its split-list thresholds and whether its edges are deferred
  emulate_pipelined()      the oracle run chunk by chunk with the same shifted addressing, staging slots and
  emulate_packed_staged()  unstaging as the C++, so that an address defect can be switched on (DEFECTS): the
                           corpora of host_paths_corpora.py must tell each of them from the right code

The constants are the sources' (tests/test_host_paths_host.py reads them back out of the sources by regex): a
retuned constant fails there, and the corpora do not silently move off their edges.  tests/test_hostplan_host.py runs
hhuff_hostplan.h itself against cuts(), plan() and packed_runs()."""
import collections
import ctypes

import numpy as np

import bounds_harness as H

K_DEPTH = 3                    # staging slots, reused round-robin
DEFAULT_CHUNK = 64 << 20       # chunk_bytes == 0
ROUTE_MIN = 2 * DEFAULT_CHUNK  # hhuff_*_batch_host: in_size from which a contiguous batch takes the pipeline
BASE_ALIGN = 80                # a chunk's base: floor(8 base / 5) stays 16-byte aligned
CUT_ALIGN = 32                 # cuts at multiples of 32 strings (one is-name word)
PACKED_CHUNK = 64 << 20        # host_packed: bytes of the device output staged at a time
TILE = 64                      # packed layout: strings a tile
SPLIT_MIN, SPLIT_MIN_FEW, SPLIT_BIG, SPLIT_BIG_FEW = 4096, 512, 65536, 4096
SPLIT_FEW_N, SPLIT_MEAN = 16, 128
DEC_SHORT_MAX, DEC_MIXED_MAX = 40, 128                    # decode: staged short | mixed | stream
ENC_SMALL_MEAN, ENC_SORTED_MAX, ENC_LANES_MAX = 48, 52, 120  # encode: sorted (small stage | large) | lanes | long
DEFER_NEVER = 0xFFFFFFFF
DEV = 0xEE  # what the emulated device and staging memory holds where nothing was written (no sentinel, no fill)

DEFECTS = {
    "a": "cut not rounded to 32 strings (the chunk's name word is misaligned)",
    "b": "base not rounded to 80: outputs at slot_of(off - base) in place of slot_of(off) - slot_of(base)",
    "c": "D2H range one byte short at slot_of(e0)",
    "d": "D2H range one byte late at slot_of(s0)",
    "e": "out_len / status of a last chunk with m < 32 not copied",
    "f": "out_len / status of a last chunk with m < 32 copied with m rounded up to 32",
    "g": "name bits taken from word 0 for every chunk",
    "h": "a slot reused before it is drained (chunk k - kDepth's results lost)",
    "i": "packed: the part of a run behind the staging boundary dropped",
    "j": "packed: the `a - lo` offset into the staged chunk omitted",
    # (the skip loop alone not advancing past an empty run changes no result: the copy loop passes over runs with
    # nothing in the chunk.  The defect is the pair: the skip stops at such a tile and the copy loop ends there)
    "k": "packed: the skip stops at an all-failed tile (empty run) and the copy loop takes it for the last run",
    "l": "packed: the whole staged chunk copied, over the gaps between the runs",
}
PIPELINED_DEFECTS, PACKED_DEFECTS = "abcdefgh", "ijkl"


def slot_of(op, pos):
    """the implicit output slot of input position pos"""
    return (8 * pos) // 5 if op == "decode" else pos


# ------------------------------------------------------------------------------------------------
# the cut rule and the chunks
# ------------------------------------------------------------------------------------------------
def cuts(in_off, n, chunk_bytes, align=CUT_ALIGN):
    """`pipelined`'s cuts: from string a, the first string starting past in_off[a] + chunk_bytes, rounded down to
    a + 32 k, at least a + 32, capped at n.  (The target is clamped to 2^32 - 1: only a 4 GiB batch gets there.)"""
    chunk_bytes = chunk_bytes or DEFAULT_CHUNK
    off = np.asarray(in_off[:n + 1], np.int64)
    cut = [0]
    while cut[-1] < n:
        a = cut[-1]
        target = min(int(off[a]) + chunk_bytes, 0xFFFFFFFF)
        b = a + int(np.searchsorted(off[a:], target, side="right"))
        b = (b - a) // align * align + a if b > a + align else a + align
        cut.append(min(b, n))
    return cut


Chunk = collections.namedtuple("Chunk", "k i0 i1 m s0 e0 base nbytes olo ohi obase slot sel mean family split smin "
                                        "big_min deferred")


def family(op, mean):
    if op == "decode":
        return "short" if mean <= DEC_SHORT_MAX else "mixed" if mean <= DEC_MIXED_MAX else "stream"
    if mean <= ENC_SORTED_MAX:
        return "sorted_small" if mean <= ENC_SMALL_MEAN else "sorted"
    return "lanes" if mean <= ENC_LANES_MAX else "lanes_long"


def plan(op, in_off, n, chunk_bytes, defer_min=DEFER_NEVER):
    """the chunks of one pipelined call.  A chunk's kernel variant follows its own bytes from its base
    (sel_bytes = nbytes; 0 falls back to the absolute in_size the launch gets, e0)"""
    off = np.asarray(in_off[:n + 1], np.int64)
    c = cuts(off, n, chunk_bytes)
    out = []
    for k, (i0, i1) in enumerate(zip(c, c[1:])):
        m, s0, e0 = i1 - i0, int(off[i0]), int(off[i1])
        base = s0 // BASE_ALIGN * BASE_ALIGN
        nbytes = e0 - base
        sel = nbytes if nbytes else e0
        mean = sel // m
        smin = SPLIT_MIN_FEW if m <= SPLIT_FEW_N else SPLIT_MIN
        split = op == "decode" and sel >= smin and (mean >= SPLIT_MEAN or m <= SPLIT_FEW_N)
        fam = family(op, mean)
        out.append(Chunk(k, i0, i1, m, s0, e0, base, nbytes, slot_of(op, s0), slot_of(op, e0), slot_of(op, base),
                         k % K_DEPTH, sel, mean, fam, split, smin,
                         SPLIT_BIG_FEW if m <= SPLIT_FEW_N else SPLIT_BIG, fam != "stream" and m >= defer_min))
    return out


# ------------------------------------------------------------------------------------------------
# the oracle on raw addresses (a chunk's `in` and `out` are passed shifted back by its base)
# ------------------------------------------------------------------------------------------------
def _oracle_raw(oracle, op, in_addr, off, n, names, out_addr, out_len, status):
    f = getattr(oracle.lib, "%s_%s_batch" % (oracle.prefix, op))
    V = ctypes.c_void_p
    p = lambda a: None if a is None else V(a.ctypes.data)  # noqa: E731
    if op == "decode":
        f.argtypes = [V] * 3 + [ctypes.c_uint32] + [V] * 5 + [ctypes.c_int]
        rc = f(V(in_addr), p(off), None, n, p(names), V(out_addr), None, p(out_len), p(status), 1)
    else:
        f.argtypes = [V] * 3 + [ctypes.c_uint32] + [V] * 4 + [ctypes.c_int]
        rc = f(V(in_addr), p(off), None, n, V(out_addr), None, p(out_len), p(status), 1)
    assert rc == 0


def new_result(arrays, names=("out", "out_len", "status")):
    """the caller's guarded, sentinel-filled arrays of exactly the documented size"""
    n, s = arrays["n"], arrays["sentinel"]
    size = {"out": arrays["out_size"], "out_len": 4 * n, "status": n, "out_off": 4 * (n + 1)}
    return {k: H.guarded(np, size[k], s)[0] for k in names}


def _put(whole, at, src):
    """src's bytes at inner byte offset `at` of a guarded buffer -- into the rear guard if it reaches there"""
    b = np.ascontiguousarray(src).view(np.uint8)
    whole[H.GUARD + at:H.GUARD + at + b.size] = b


def emulate_pipelined(oracle, op, arrays, chunk_bytes, defect=None):
    """`pipelined`'s chunk loop on the oracle.  arrays: bounds_harness.place_input()'s dict plus names (is-name
    words or None), out_size, sentinel and with_status (False: an encode's status is NULL).
    -> name -> whole guarded buffer, as bounds_harness.check() takes it"""
    assert defect is None or defect in PIPELINED_DEFECTS
    n, data = arrays["n"], arrays["data"]
    off = np.asarray(arrays["in_off"][:n + 1], np.int64)
    names = arrays.get("names") if op == "decode" else None
    with_status = arrays.get("with_status", True)
    res = new_result(arrays, ("out", "out_len", "status") if with_status else ("out", "out_len"))
    c = cuts(off, n, chunk_bytes, 1 if defect == "a" else CUT_ALIGN)
    slots = [None] * K_DEPTH

    def drain(x):
        if x["out"].size:
            _put(res["out"], x["out_lo"], x["out"])
        _put(res["out_len"], 4 * x["i0"], x["len"])
        if with_status:
            _put(res["status"], x["i0"], x["st"])

    for k, (i0, i1) in enumerate(zip(c, c[1:])):
        if slots[k % K_DEPTH] is not None and defect != "h":
            drain(slots[k % K_DEPTH])
        m, s0, e0 = i1 - i0, int(off[i0]), int(off[i1])
        base = s0 if defect == "b" else s0 // BASE_ALIGN * BASE_ALIGN
        nbytes = e0 - base
        olo, ohi, obase = slot_of(op, s0), slot_of(op, e0), slot_of(op, base)
        assert ohi <= arrays["out_size"]
        d_in = np.full(nbytes + 16, DEV, np.uint8)
        d_in[:nbytes] = data[base:e0]
        d_out = np.full(ohi - obase + 16, DEV, np.uint8)
        mcap = (m + 31) // 32 * 32
        d_len, d_st = np.full(mcap, 0xEEEEEEEE, np.uint32), np.full(mcap, DEV, np.uint8)
        d_off = off[i0:i1 + 1].astype(np.uint32)
        d_nm = None
        if names is not None:
            w0 = 0 if defect == "g" else i0 // 32
            d_nm = names[w0:w0 + (m + 31) // 32].copy()
        if defect == "b":  # the chunk addressed from its own base: string i's output at slot_of(off_i - base)
            d_off -= np.uint32(base)
            _oracle_raw(oracle, op, d_in.ctypes.data, d_off, m, d_nm, d_out.ctypes.data, d_len, d_st)
        else:              # absolute offsets, `in` and `out` shifted back
            _oracle_raw(oracle, op, d_in.ctypes.data - base, d_off, m, d_nm, d_out.ctypes.data - obase, d_len, d_st)
        lo, hi = olo + (defect == "d"), ohi - (defect == "c")
        last = i1 == n and m < 32
        mc = 0 if last and defect == "e" else mcap if last and defect == "f" else m
        slots[k % K_DEPTH] = dict(i0=i0, out_lo=lo, out=d_out[lo - obase:max(hi, lo) - obase].copy(),
                                  len=d_len[:mc].copy(), st=d_st[:mc].copy())
    for x in slots:
        if x is not None:
            drain(x)
    return res


# ------------------------------------------------------------------------------------------------
# the packed layout and host_packed's staged unstaging
# ------------------------------------------------------------------------------------------------
def packed_from_slots(op, in_off, n, exp):
    """the oracle's slot-layout result in the packed layout (every 64-string tile's kept outputs back to back from
    the tile's slot position): -> (expected dict with out of exactly the slot end and out_off[n + 1], run mask)"""
    from h2o_amd import codec

    off = np.asarray(in_off[:n + 1], np.int64)
    olen = exp["out_len"]
    keep = np.where(olen == H.FAIL, 0, olen).astype(np.int64)
    pos = codec.packed_positions(off[:n], olen, op == "decode")
    size = slot_of(op, int(off[n]))
    out = np.zeros(size, np.uint8)
    src = np.asarray([slot_of(op, int(s)) for s in off[:n]], np.int64)
    for i in np.nonzero(keep)[0]:
        out[pos[i]:pos[i] + keep[i]] = exp["out"][src[i]:src[i] + keep[i]]
    ooff = np.append(pos, pos[-1] + keep[-1]).astype(np.uint32)
    return dict(out=out, out_off=ooff, out_len=olen, status=exp["status"]), H.ranges_mask(pos, pos + keep, size)


def packed_runs(op, in_off, n, out_off, out_len):
    """[run_lo, run_hi) of every tile, as host_packed derives them from the returned metadata"""
    runs = []
    for t in range((n + TILE - 1) // TILE):
        last = min((t + 1) * TILE, n) - 1
        runs.append((slot_of(op, int(in_off[t * TILE])),
                     int(out_off[last]) + (int(out_len[last]) if out_len[last] != H.FAIL else 0)))
    return runs


def emulate_packed_staged(oracle, op, arrays, boundary, defect=None):
    """host_packed's staged route: the oracle's whole-batch result in the packed layout stands for the device
    buffers; the runs are copied out of it through a staging buffer of `boundary` bytes as the C++ does.
    arrays as for emulate_pipelined, plus with_off (False: out_off is NULL).  out_size is the slot end"""
    assert defect is None or defect in PACKED_DEFECTS
    n = arrays["n"]
    off = np.asarray(arrays["in_off"][:n + 1], np.int64)
    slot_end = slot_of(op, int(off[n]))
    assert arrays["out_size"] == slot_end
    _, slots = H.oracle_run(oracle, op, arrays, arrays["sentinel"], names=arrays.get("names"))
    exp, _ = packed_from_slots(op, off, n, slots)
    d_out = np.full(slot_end + 16, DEV, np.uint8)
    keep = np.where(exp["out_len"] == H.FAIL, 0, exp["out_len"]).astype(np.int64)
    for p, L in zip(exp["out_off"][:n].astype(np.int64), keep):
        d_out[p:p + L] = exp["out"][p:p + L]
    want = ["out", "out_len"] + (["out_off"] if arrays.get("with_off", True) else []) + \
        (["status"] if arrays.get("with_status", True) else [])
    res = new_result(arrays, want)
    _put(res["out_len"], 0, exp["out_len"])
    if "out_off" in res:
        _put(res["out_off"], 0, exp["out_off"])
    if "status" in res:
        _put(res["status"], 0, exp["status"])
    runs = packed_runs(op, off, n, exp["out_off"], exp["out_len"])
    out = H.entries(res["out"], np.uint8)
    t, nt = 0, len(runs)
    lo = 0
    while lo < slot_end and t < nt:
        hi = min(slot_end, lo + boundary)
        while t < nt and runs[t][1] <= lo and not (defect == "k" and runs[t][1] == runs[t][0]):
            t += 1
        if t >= nt or runs[t][0] >= hi:
            lo += boundary
            continue
        h = np.full(2 * boundary + slot_end, DEV, np.uint8)  # the staging buffer (and, for "j", what lies behind it)
        h[:hi - lo] = d_out[lo:hi]
        if defect == "l":
            out[lo:hi] = h[:hi - lo]
        for u in range(t, nt):
            rlo, rhi = runs[u]
            if rlo >= hi:
                break
            if defect == "i" and rlo < lo:
                continue
            a, b = max(rlo, lo), min(rhi, hi)
            if b > a:
                src = a if defect == "j" else a - lo
                out[a:b] = h[src:src + b - a]
            elif defect == "k":
                break
        lo += boundary
    return res
