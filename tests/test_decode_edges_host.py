"""The edge corpora of tests/decode_edges.py and the reference decoder tests/huff_ref.py, checked without a GPU:
  - huff_ref equals the oracle on the KAT set, the staged decoders' tail corpus and every string of the three
    corpora, under both name flags;
  - the geometry constants the generators use are the ones in the kernel sources;
  - every class of string the corpora are meant to hold is there, judged from huff_ref's symbol offsets;
  - wrong decoders (models of the mistakes a rewrite of these kernels could make) each disagree with huff_ref on at
    least one corpus string: the corpora can tell them from a right one."""
import itertools
import os
import re

import numpy as np
import pytest

import decode_edges as E
import huff_ref as R
from conftest import ROOT, load_golden

CSRC = os.path.join(ROOT, "h2o_amd", "csrc")


@pytest.fixture(scope="module")
def corpora(oracle_codec):
    return {name: E.corpus(name, oracle_codec) for name in ("stream", "split", "one_string", "per_string")}


def _all_cases(corpora):
    for name in ("stream", "split", "one_string"):
        for cs in corpora[name].values():
            yield from cs
    yield from corpora["per_string"]


def _oracle(oracle, data, is_name):
    dec, soft = oracle.decode(data, is_name)
    return dec, R.STATUS_FAIL if dec is None else soft


def _lens(w):
    return [b - a for a, b in zip(w.starts, w.starts[1:] + [w.stop])]


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def test_ref_matches_the_oracle_on_kat_and_tail_strings(oracle_codec):
    from h2o_amd import synth

    g = load_golden("kat")
    strings = list(synth.unpack(g["dec_in"], g["dec_in_off"])) + E.special_strings(oracle_codec, E.CODES, 31)
    assert len(strings) > 300
    for s in strings:
        for nm in (False, True):
            assert R.decode(bytes(s), nm) == _oracle(oracle_codec, bytes(s), nm), (bytes(s).hex(), nm)


def test_ref_matches_the_oracle_on_every_corpus_string(oracle_codec, corpora):
    n = 0
    for c in _all_cases(corpora):
        for nm in (False, True):
            assert E.ref(c.data, nm) == _oracle(oracle_codec, c.data, nm), (c.label, nm)
            n += 1
    assert n > 5000


def test_ref_on_bit_strings():
    """walk() on bit strings that are no whole bytes, and the offsets it returns"""
    a, amp = E.CODES[ord("a")], E.CODES[ord("&")]
    w = R.walk(a + amp + E.CODES[10] + "111")
    assert (w.syms, w.starts, w.stop, w.nbits, w.eos) == (b"a&\n", [0, 5, 13], 43, 46, False)
    w = R.walk(a + E.EOS_BITS + a)
    assert (w.syms, w.stop, w.eos) == (b"a", 5, True)
    assert R.decode(a + "1" * 7) == (b"a", 0) and R.decode(a + "1" * 8) == (None, R.STATUS_FAIL)
    assert R.decode(a + "1101") == (None, R.STATUS_FAIL) and R.decode("") == (b"", 0) and R.decode("", True) == (b"", 1)


def test_invalid_sets_match_the_oracle(oracle_codec):
    """NAME_INVALID_RANGES / VALUE_INVALID_RANGES against the oracle: every one-symbol string as a name and as a
    value, and -- so that SP / HT at an end and a leading ':' do not stand in for the sets -- every symbol
    between two 'a'"""
    from h2o_amd import tables

    assert R.NAME_INVALID == frozenset(range(256)) - tables.NAME_VALID  # (the generated sets agree too)
    assert R.VALUE_INVALID == frozenset(range(256)) - tables.VALUE_VALID
    a = E.CODES[ord("a")]
    for b in range(256):
        one = E.to_bytes(E.close(E.CODES[b]))
        mid = E.to_bytes(E.close(a + E.CODES[b] + a))
        for nm in (False, True):
            assert R.decode(one, nm) == _oracle(oracle_codec, one, nm), (b, nm)
        assert _oracle(oracle_codec, mid, True) == (bytes([97, b, 97]), 1 if b in R.NAME_INVALID else 0), b
        assert _oracle(oracle_codec, mid, False) == (bytes([97, b, 97]), 2 if b in R.VALUE_INVALID else 0), b


# ------------------------------------------------------------------------------------------------
# the constants
# ------------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"[ \t]+", " ", f.read())


def _value(text, pattern, env=None):
    """the one match of `pattern`; its group 1 evaluated as integer arithmetic over `env`"""
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    expr = m[0].replace("u", "")
    assert re.fullmatch(r"[0-9A-Z+\-*() ]+", expr), expr
    return eval(expr, {"__builtins__": {}}, env or {})  # noqa: S307  (digits, NW and operators only)


def test_constants_match_the_sources():
    """decode_edges.py's geometry against hhuff_kernels.hip / hhuff_launch.h / hhuff_tables.h.  A kernel that is
    retuned fails here: move the constant in decode_edges.py with it, and the corpora's edges follow."""
    k, launch, tables = _src("hhuff_kernels.hip"), _src("hhuff_launch.h"), _src("hhuff_tables.h")
    nw = _value(k, r"#define HHUFF_DECT_NW (\d+)")
    assert nw == E.STREAM_NW
    assert _value(k, r"#define HHUFF_DECT_OUT (\d+)") == E.STREAM_OUT
    assert _value(k, r"#define HHUFF_DECT_SEG (\d+)") == E.STREAM_SEG
    assert "#define DEC_T decode_stream_kernel<kDecTWaves, HHUFF_DECT_NW, HHUFF_DECT_OUT, HHUFF_DECT_SEG>" in k
    assert _value(k, r"constexpr int32_t kLimW = ([^;]+);", {"NW": nw}) == E.STREAM_LIMW == 546
    assert _value(k, r"constexpr int32_t kFinal = ([^;]+);", {"NW": nw}) == E.STREAM_FINAL == 576
    assert _value(k, r"\? wb \+ (4u \* \(NW - \d+\)) : ~0ull;", {"NW": nw}) == E.STREAM_NEXT == 68
    assert _value(k, r"int32_t lim = busy \? min\(end - (\d+), kLimW\)") == E.STREAM_TAIL
    assert _value(k, r"#define HHUFF_STREAM_CLAIM_BYTES (\d+)u") == E.STREAM_CLAIM_BYTES
    assert "return c >= 256 ? 256u : c >= 192 ? 192u : c >= 128 ? 128u : 64u;" in k
    assert "if (mean <= 40) return kDecS; if (mean <= 128) return kDecL; return kDecT;" in k.replace("\n", "")
    assert _value(tables, r"#define HHUFF_LUT_BITS (\d+)") == E.LUT_BITS
    # split
    assert _value(k, r"constexpr uint32_t kSplitMin = (\d+);") == E.SPLIT_MIN
    assert _value(k, r"constexpr uint32_t kSplitMinFew = (\d+);") == E.SPLIT_MIN_FEW
    assert _value(k, r"constexpr uint32_t kSplitLead = (\d+);") == E.SPLIT_LEAD
    m = re.search(r"constexpr uint32_t kSplitBig = (\d+), kSplitBigFew = (\d+);", k)
    assert (int(m.group(1)), int(m.group(2))) == (E.SPLIT_BIG, E.SPLIT_BIG_FEW)
    assert _value(k, r"constexpr int kSplitBlockWaves = (\d+);") == E.SPLIT_BLOCK_WAVES
    assert _value(k, r"const uint32_t smin = n <= (\d+)u \? kSplitMinFew : kSplitMin;") == E.SPLIT_FEW_N
    assert _value(k, r"const bool split = bytes >= smin && \(bytes / n >= (\d+)u \|\| n <= 16u\);") == E.SPLIT_MEAN
    assert "A.big_min = n <= 16u ? kSplitBigFew : kSplitBig;" in k
    assert k.count("const uint32_t lead = seg <= 64u ? 64u : (seg <= 256u ? 128u : kSplitLead);") == 2
    assert "const uint32_t seg = (uint32_t)(((uint64_t)TB + 64u * 32u - 1u) / (64u * 32u)) * 32u;" in k
    assert "const uint32_t seg = max((uint32_t)(((uint64_t)TB + N * 32u - 1u) / (N * 32u)) * 32u, 128u);" in k
    assert "constexpr uint32_t N = 64u * W;" in k
    assert _value(k, r"split_decode_block<(\d+)>\(src, 0u, len, is_name != 0, s_out") == E.ONE_STRING_WAVES
    assert [E.split_seg(L)[0] for L in E.SPLIT_WAVE_FEW] == [64, 96, 128, 160, 256, 288, 512]
    assert {E.split_seg(L)[1] for L in E.SPLIT_WAVE_FEW} == {64, 128, 256}
    assert [E.split_seg(L, E.SPLIT_BLOCK_WAVES, True)[0] for L in E.SPLIT_BLOCK_FEW] == [128, 128, 128]
    assert [E.split_seg(L)[0] for L in E.SPLIT_WAVE_MANY] == [512, 640]
    # per-string service
    assert _value(launch, r"constexpr uint32_t kSvcMax = (\d+);") == E.SVC_MAX
    assert _value(launch, r"constexpr uint32_t kOneMax = (\d+);") == E.ONE_MAX
    assert k.count("constexpr uint32_t kWin = 64u * NC;") == 2 and E.SVC_ROUND == 64
    assert [E.stream_claim(m * 100, 100) for m in (41, 90, 91, 120, 121, 180, 181)] == [256, 256, 192, 192, 128, 128, 64]


# ------------------------------------------------------------------------------------------------
# coverage
# ------------------------------------------------------------------------------------------------
def _tail_holds(w, c, t):
    lens = _lens(w)
    pad = w.nbits - w.stop
    return {"long30 last": lambda: lens[-1] == 30 and pad == 0 and not w.eos,
            "5 long14 5": lambda: lens[-3:] == [5, 14, 5] and not w.eos,
            "eos": lambda: w.eos and w.stop + 30 == w.nbits,
            "pad7 zero@6": lambda: pad == 7 and c.data[-1] & 0x7F == 0x7E,
            "cut 13 of 14": lambda: pad == 13 and not w.eos,
            "text pad": lambda: 0 <= pad <= 7 and E.ref(c.data, False)[0] is not None}[t]()


def test_stream_window_edge_coverage(corpora):
    cases = corpora["stream"]["window_edge"]
    batch = E.arrange(cases)
    seen = set()
    for c, s in zip(batch, E.offsets(batch)):
        if c.facts.get("filler"):
            continue
        f, w = c.facts, E.walk_of(c.data)
        assert s % 4 == f["align"], c.label  # arrange() puts the string where its facts say
        w0 = 8 * (E.STREAM_NEXT * f["window"] - f["align"])  # the window's first bit in string bits
        assert 8 * len(c.data) - w0 == f["end"], c.label
        assert _tail_holds(w, c, f["tail"]), c.label
        if "code_end" in f:
            assert w.stop - w0 == f["code_end"], c.label
            seen.add((f["align"], f["window"], "code_end", f["code_end"]))
        else:
            seen.add((f["align"], f["window"], f["end"], f["tail"]))
    want = set(itertools.product(range(4), range(3), E.STREAM_ENDS, E.STREAM_TAILS)) | \
        set(itertools.product(range(4), range(3), ["code_end"], E.STREAM_CODE_ENDS))
    assert seen == want, want - seen
    assert E.STREAM_FINAL in E.STREAM_ENDS and {E.STREAM_LIMW - 1, E.STREAM_LIMW, E.STREAM_LIMW + 1, E.STREAM_FINAL - 1,
                                                E.STREAM_FINAL, E.STREAM_FINAL + 1} <= set(E.STREAM_CODE_ENDS)
    # every padding length 0..7 behind text
    assert {8 * len(c.data) - E.walk_of(c.data).stop for c in cases if c.facts["tail"] == "text pad"} >= {0, 1, 5, 6, 7}


def test_stream_long_code_and_eos_coverage(corpora):
    seen, ends = set(), set()
    for c in corpora["stream"]["long_codes"]:
        f, w = c.facts, E.walk_of(c.data)
        at = f["sym_at"] + 8 * (E.STREAM_NEXT * f["window"] - f["align"])
        if f["cut"]:
            assert w.stop == at and 8 <= w.nbits - at < f["sym_len"] and E.ref(c.data, False)[0] is None, c.label
        else:
            k = w.starts.index(at)
            assert _lens(w)[k] == f["sym_len"] and E.ref(c.data, False)[0] is not None, c.label
        if f.get("end"):
            assert w.nbits - 8 * (E.STREAM_NEXT * f["window"] - f["align"]) == E.STREAM_FINAL == f["sym_at"] + f["sym_len"]
            ends.add((f["align"], f["window"], f["sym_len"]))
        seen.add((f["align"], f["window"], f["sym_len"], f["sym_at"], f["cut"]))
    ats = range(E.STREAM_LIMW - 6, E.STREAM_LIMW + 3)  # first bit 540..548: pm 539..547 around kLimW
    assert set(itertools.product(range(4), (0, 1), E.LONG, ats, [False])) <= seen
    # the string ends inside the code (at a byte, 8 bits or more into it): every long length from 19 bits up at every
    # start; a 14-bit code only where a byte boundary falls in its bits 8..13
    assert set(itertools.product(range(4), (0, 1), (19, 23, 28, 30), ats, [True])) <= seen
    assert {x[3] for x in seen if x[2] == 14 and x[4]} == {at for at in ats if (at + 15) // 8 * 8 < at + 14}
    assert ends == set(itertools.product(range(4), (0, 1), E.LONG))
    seen = set()
    for c in corpora["stream"]["eos"]:
        f, w = c.facts, E.walk_of(c.data)
        assert w.eos and w.stop == f["eos_at"] + 8 * (E.STREAM_NEXT * f["window"] - f["align"]), c.label
        assert w.nbits - w.stop > 100  # text behind it
        seen.add((f["align"], f["window"], f["eos_at"]))
    assert seen == set(itertools.product(range(4), (0, 1), (E.STREAM_LIMW - 30, E.STREAM_LIMW - 1, E.STREAM_LIMW)))


def _bad_at(syms, is_name):
    inv = R.NAME_INVALID if is_name else R.VALUE_INVALID
    return [k for k, b in enumerate(syms) if b in inv]


def test_stream_soft_coverage(corpora):
    seen = set()
    for c in corpora["stream"]["soft"]:
        f, w = c.facts, E.walk_of(c.data)
        rounds = E.stream_rounds(w, f["align"])
        assert len(rounds) == f["rounds"] and rounds[-1][1] == f["made"] and rounds[0][1] > 0, c.label
        ws = [k for k, b in enumerate(w.syms) if b in (E.SP, E.HT)]
        bad = _bad_at(w.syms, c.is_name)
        status = E.ref(c.data, c.is_name)[1]
        in_round = lambda k: next(r + 1 for r, (i0, n, _, _) in enumerate(rounds) if i0 <= k < i0 + n)  # noqa: E731
        if f["what"] == "sp first":
            assert ws == [0] and not bad and status == 2, c.label
            key = ("sp first",)
        elif f["what"] == "sp last":
            assert ws == [len(w.syms) - 1] and not bad and status == 2 and in_round(ws[0]) == f["rounds"], c.label
            key = ("sp last", "one" if f["made"] == 1 else "several")
            assert f["made"] >= 1
        elif f["what"] == "bad":
            assert len(bad) == 1 and not ws and in_round(bad[0]) == f["round"], c.label
            assert status == (1 if c.is_name else 2), c.label
            key = ("bad", c.is_name, _lens(w)[bad[0]] > E.LUT_BITS, f["round"])
        else:
            assert c.is_name and w.syms[0] == ord(":") and len(bad) > 1 and in_round(bad[-1]) == 2 and status == 0
            key = ("colon",)
        seen.add((f["align"], f["rounds"]) + key)
    for align, nr in itertools.product(range(4), (2, 3)):
        want = {("sp first",), ("sp last", "one"), ("sp last", "several"), ("colon",)} | \
            {("bad", nm, lg, rd) for nm in (False, True) for lg in (False, True) for rd in range(1, nr + 1)}
        assert {(align, nr) + k for k in want} <= seen, (align, nr)


def test_stream_flush_coverage(corpora):
    cases = corpora["stream"]["flush"]
    batch = E.arrange(cases)
    lens_dst, contig, carries, wholes = set(), set(), set(), set()
    for c, s in zip(batch, E.offsets(batch)):
        if c.facts.get("filler"):
            continue
        f, w = c.facts, E.walk_of(c.data)
        dec = E.ref(c.data, False)[0]
        assert dec is not None and len(dec) == f["out_len"], c.label
        m, r = f["s_mod"]
        assert s % m == r, c.label
        dst = (8 * int(s)) // 5
        if "carry" in f:
            made = E.stream_rounds(w, 0)[0][1]
            assert s % 4 == 0 and (f["dst16"] + made) % 16 == f["carry"] and len(dec) > made, c.label
            carries.add(f["carry"])
        elif "whole" in f:
            slot_end = (8 * (int(s) + len(c.data))) // 5
            miss = (dst + len(dec) + 15) // 16 * 16 - slot_end
            assert (miss == 0) == f["whole"] and miss in (0, 2) and (dst + len(dec)) % 16, c.label
            assert (dst + len(dec)) // 16 > dst // 16 or dst % 16 == 0, c.label  # (the string reaches its last chunk)
            wholes.add(f["whole"])
        else:
            lens_dst.add((f["out_len"], f["dst16"]))
            contig.add((f["out_len"], dst % 16))
    assert lens_dst == set(itertools.product(E.FLUSH_LENS, E.FLUSH_DST))
    for n in E.FLUSH_LENS:
        assert {0, 1, 14} <= {d for ln, d in contig if ln == n} and {d for ln, d in contig if ln == n} & {4, 6}
    assert carries == {0, 1, 15} and wholes == {True, False}
    # the contiguous layout's destinations: never 5 or 15 mod 16
    assert {((8 * s) // 5) % 16 for s in range(160)} == {0, 1, 3, 4, 6, 8, 9, 11, 12, 14}


def test_stream_claims():
    """which in_size per n makes stream_claim pick each size (the GPU test's routes)"""
    for n in (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257):
        assert [E.stream_claim(m * n, n) for m in (90, 120, 180, 181)] == [256, 192, 128, 64]


def _split_expected(nbytes, waves, block):
    """(kind, rel, k) of every placement that fits the string: an item needs 17 bits behind it"""
    seg, ks = E.split_boundaries(nbytes, waves, block)
    items = [("code%d" % L, rel, L) for L in (5, 8, 14, 30) for rel in (-1, 0, 1)] + [("code30", -29, 30)] + \
        [("pair5+5", rel, 10) for rel in (-5, -3)] + [("eos", rel, 30) for rel in (-30, -1, 0)] + \
        [("only bad", rel, 13) for rel in (-1, 0)] + [("only bad name", rel, 6) for rel in (-1, 0)]
    return seg, ks, {(kind, rel, k) for kind, rel, L in items for k in ks if k * seg + rel + L + 17 <= 8 * nbytes}


def _check_split_cases(cases, nbytes, waves, block):
    seg, ks, want = _split_expected(nbytes, waves, block)
    seen, kinds = set(), {}
    last = (8 * nbytes - 1) // seg
    for c in cases:
        f, w = c.facts, E.walk_of(c.data)
        assert len(c.data) == nbytes and f["seg"] == seg and f["lead"] == E.split_seg(nbytes, waves, block)[1], c.label
        kind = f["kind"]
        kinds.setdefault(kind, []).append(c)
        dec, status = E.ref(c.data, c.is_name)
        lens = _lens(w)
        if "at" in f:
            assert [a - f["rel"] for a in f["at"]] == [k * seg for k in f["bounds"]], c.label
            for a, k in zip(f["at"], f["bounds"]):
                if kind == "eos":
                    assert w.eos and w.stop == a and len(f["at"]) == 1 and dec is None, c.label
                elif kind.startswith("only bad"):
                    bad = _bad_at(w.syms, c.is_name)
                    assert len(bad) == 1 and w.starts[bad[0]] == a and status == (1 if c.is_name else 2), c.label
                elif kind == "pair5+5":
                    j = w.starts.index(a)
                    assert lens[j:j + 2] == [5, 5] and dec is not None, c.label
                else:
                    assert lens[w.starts.index(a)] == int(kind[4:]) and dec is not None, c.label
                seen.add((kind, f["rel"], k))
        elif kind in ("sp first", "sp last", "sp alone"):
            ws = [k for k, b in enumerate(w.syms) if b in (E.SP, E.HT)]
            assert ws == [0 if kind == "sp first" else len(w.syms) - 1] and status == 2 and not _bad_at(w.syms, False)
            if kind == "sp alone":
                assert E.split_lanes(w, seg)[-1] == 1 and w.nbits - w.stop == f["pad"], c.label
        elif kind == "pad only":
            assert E.split_lanes(w, seg)[-1] == 0 and 1 <= w.nbits - w.stop == f["pad"] <= 7 and status == 0, c.label
        elif kind == "cut":
            assert dec is None and not w.eos and w.stop == f["cut_at"] and w.nbits - w.stop > 7, c.label
        elif kind == "flip":
            assert f["bit"] // seg == {"first": 0, "middle": last // 2, "last": last}[f["where"]], c.label
        else:
            assert kind == "periodic" and dec is not None
    assert seen == want, (nbytes, want - seen, seen - want)
    assert {c.facts["unit"] for c in kinds["periodic"]} == {"0e", "a", "30-bit", "5-bit"}
    assert {c.facts["where"] for c in kinds["flip"]} == {"first", "middle", "last"}
    assert len(kinds["cut"]) == 2 and len(kinds["sp first"]) == 1 and len(kinds["sp last"]) == 1
    # the last lane alone with the SP, or with padding only: wherever the arithmetic allows (decode_edges.py)
    tailbits = 8 * nbytes - last * seg
    assert {c.facts["pad"] for c in kinds.get("sp alone", [])} == {p for p in (0, 1, 7) if 1 <= tailbits - 6 - p <= 27}
    assert {c.facts["pad"] for c in kinds.get("pad only", [])} == {p for p in range(1, 8) if 1 <= tailbits - p <= 27}
    return ks, seen, kinds


def test_split_coverage(corpora):
    shapes = {"wave_few": (1, False), "wave_many": (1, False), "block_few": (E.SPLIT_BLOCK_WAVES, True)}
    assert sorted(corpora["split"]) == sorted([("wave_few", L) for L in E.SPLIT_WAVE_FEW] +
                                              [("block_few", L) for L in E.SPLIT_BLOCK_FEW] +
                                              [("wave_many", L) for L in E.SPLIT_WAVE_MANY])
    pad_only, sp_alone, leads = set(), set(), set()
    for (form, L), cases in corpora["split"].items():
        ks, seen, kinds = _check_split_cases(cases, L, *shapes[form])
        seg, lead = E.split_seg(L, *shapes[form])
        last = (8 * L - 1) // seg
        inner = [k for k in (1, 2, 63) + ((64, 128) if form == "block_few" else ()) if k < last]
        assert set(ks) == set(inner) | {last} and {1, 2} <= set(inner)  # (513, 1025 and 2049 B have under 64 lanes)
        # every boundary but (where the last lane is short) the last one holds every placement; two of the three
        # EOS placements lie in the next lane's lead
        for k in inner:
            assert {(kd, rel) for kd, rel, kk in seen if kk == k} == {(kd, rel) for kd, rel, kk in
                                                                       _split_expected(L, *shapes[form])[2] if kk == 1}
        assert lead >= 30
        leads.add(lead)
        pad_only |= {form for _ in kinds.get("pad only", [])}
        sp_alone |= {form for _ in kinds.get("sp alone", [])}
        # inactive lanes: a block of 1024 lanes on these lengths; a partly filled last lane
        if form == "block_few":
            assert last + 1 < 64 * E.SPLIT_BLOCK_WAVES
    assert leads == {64, 128, 256}
    # Padding alone in the last lane needs a last segment of 8..34 bits: of the lengths tested only 4097 B in a
    # block has one (8 bits); the wave forms' last segments have 40 bits and more (512 B: 64, 513: 72, 1025: 40 ...)
    assert pad_only == {"block_few"} and "block_few" in sp_alone and "wave_few" in sp_alone
    assert any(c.facts.get("tailbits") == 8 for c in corpora["split"]["block_few", 4097])


def test_one_string_coverage(corpora):
    assert sorted(corpora["one_string"]) == list(E.SPLIT_ONE_STRING)
    for L, cases in corpora["one_string"].items():
        seg, lead = E.split_seg(L, E.ONE_STRING_WAVES, True)
        assert seg == max(128, (8 * L + 8191) // 8192 * 32)
        assert {c.facts["kind"] for c in cases} >= {"code30", "pair5+5", "eos", "only bad", "sp first", "sp last", "cut",
                                                    "periodic", "flip"}
        for c in cases:
            assert len(c.data) == L and c.facts["seg"] == seg
        ks = set(E.split_boundaries(L, E.ONE_STRING_WAVES, True)[1])
        assert ks - {max(ks)} <= {k for c in cases for k in c.facts.get("bounds", ())} <= ks
    assert set(E.split_boundaries(4096, E.ONE_STRING_WAVES, True)[1]) == {1, 2, 63, 64, 128, 255}


def test_per_string_coverage(oracle_codec, corpora):
    cases = corpora["per_string"]
    by = {}
    for c in cases:
        by.setdefault(c.facts["kind"], []).append(c)
    assert [c.data for c in by["tail"]] == E.special_strings(oracle_codec, E.CODES, 31)
    for c in by["exact"] + by["padded"]:
        w = E.walk_of(c.data)
        assert (w.stop, w.nbits - w.stop) == (c.facts["total"], c.facts["pad"]) and E.ref(c.data, False)[1] == 0
    assert {c.facts["total"] for c in by["exact"]} == {64, 128, 192, 384}
    assert {(c.facts["total"] + c.facts["pad"], c.facts["pad"]) for c in by["padded"]} == \
        set(itertools.product((64, 128, 192, 384), range(1, 8)))
    seen = set()
    for c in by["long30"]:
        f, w = c.facts, E.walk_of(c.data)
        rounds = E.svc_rounds(w, f["win"])
        start = 0 if f["round"] == 1 else f["start2"]
        assert rounds[f["round"] - 1][0] == start and _lens(w)[w.starts.index(start + f["at"])] == 30, c.label
        seen.add((f["win"], f["round"], f["at"]))
    for win in E.SVC_WINS:
        assert {(win, r, at) for r in (1, 2) for at in (34, 35, 63, 64, win - 30, win - 29, win - 1, win)} <= seen
    assert {(c.facts["win"], c.facts["eos_end"]) for c in by["eos"]} == {(w, k * w) for w in E.SVC_WINS for k in (1, 2)}
    for c in by["eos"]:
        w = E.walk_of(c.data)
        assert w.eos and w.stop + 30 == c.facts["eos_end"], c.label
    for c in by["pad round"]:
        w = E.walk_of(c.data)
        rounds = E.svc_rounds(w, c.facts["win"])
        assert rounds[-1][1] == 0 and rounds[-1][0] == w.stop and w.nbits - w.stop == c.facts["pad"], c.label
        assert E.ref(c.data, False)[1] == 0
    assert {(c.facts["win"], c.facts["pad"]) for c in by["pad round"]} == set(itertools.product(E.SVC_WINS, (1, 7)))
    assert sorted({len(c.data) for c in by["limit"]}) == [E.SVC_MAX - 1, E.SVC_MAX, E.SVC_MAX + 1]
    assert {c.is_name for c in by["limit"]} == {False, True}
    soft = {(c.facts["what"], c.is_name, E.ref(c.data, c.is_name)[1]) for c in by["soft"]}
    assert soft == {("sp first", False, 2), ("sp last", False, 2), ("bad", False, 2), ("bad", True, 1), ("colon", True, 0)}
    assert all(20 <= len(c.data) <= 100 for c in by["soft"])


# ------------------------------------------------------------------------------------------------
# sensitivity: wrong decoders that the corpora must tell from huff_ref
# ------------------------------------------------------------------------------------------------
def _soft(is_name, n, flag_bytes, first, last):
    if is_name:
        return 1 if n == 0 or (first != 0x3A and any(b in R.NAME_INVALID for b in flag_bytes)) else 0
    return 2 if any(b in R.VALUE_INVALID for b in flag_bytes) or (n and (first in (32, 9) or last in (32, 9))) else 0


def _ok(c, w, max_pad=7, zero_ok=False):
    rest = R.bits_of(c.data)[w.stop:]
    return not w.eos and len(rest) <= max_pad and (zero_ok or all(rest))


def _result(c, w, nm, syms=None, flag_bytes=None, first=None, last=None, ok=None):
    if not (_ok(c, w) if ok is None else ok):
        return None, R.STATUS_FAIL
    syms = w.syms if syms is None else syms
    return syms, _soft(nm, len(syms), syms if flag_bytes is None else flag_bytes,
                       (syms[0] if syms else 0) if first is None else first,
                       (syms[-1] if syms else 0) if last is None else last)


def v_flags_from_the_first_576_bits(c, w, nm):
    return _result(c, w, nm, flag_bytes=bytes(b for b, s in zip(w.syms, w.starts) if s < E.STREAM_FINAL))


def v_first_from_the_second_window(c, w, nm):
    later = [b for b, s in zip(w.syms, w.starts) if s >= 8 * E.STREAM_NEXT]
    return _result(c, w, nm, first=later[0] if later else None)


def v_last_from_the_last_round_of_two_bytes(c, w, nm):
    if not _ok(c, w) or not w.syms:
        return _result(c, w, nm)
    rounds = [r for r in E.stream_rounds(w, c.facts.get("align", 0)) if r[1] >= 2]
    return _result(c, w, nm, last=w.syms[rounds[-1][0] + rounds[-1][1] - 1] if rounds else None)


def v_eight_bits_of_padding(c, w, nm):
    return _result(c, w, nm, ok=_ok(c, w, max_pad=8))


def v_zero_bit_in_the_padding(c, w, nm):
    return _result(c, w, nm, ok=_ok(c, w, zero_ok=True))


def v_eos_in_the_lead_ignored(c, w, nm):
    seg, lead = c.facts["seg"], c.facts["lead"]
    b = (w.stop // seg + 1) * seg
    if w.eos and b - lead <= w.stop < b and b < w.nbits:
        return w.syms, _soft(nm, len(w.syms), w.syms, w.syms[0], w.syms[-1])
    return _result(c, w, nm)


def v_symbol_before_a_boundary_dropped(c, w, nm):
    seg = c.facts["seg"]
    return _result(c, w, nm, syms=bytes(b for b, s in zip(w.syms, w.starts) if s < seg or s % seg != seg - 1))


def v_symbol_at_a_boundary_twice(c, w, nm):
    seg = c.facts["seg"]
    return _result(c, w, nm, syms=b"".join(bytes([b]) * (2 if s >= seg and s % seg == 0 else 1)
                                           for b, s in zip(w.syms, w.starts)))


def v_long_code_at_545_does_not_fit(c, w, nm):
    at = E.STREAM_LIMW - 1 - 8 * c.facts.get("align", 0)
    lens = dict(zip(w.starts, _lens(w)))
    return _result(c, w, nm, ok=_ok(c, w) and lens.get(at, 0) <= E.LUT_BITS)


STREAM_VARIANTS = (v_flags_from_the_first_576_bits, v_first_from_the_second_window,
                   v_last_from_the_last_round_of_two_bytes, v_eight_bits_of_padding, v_zero_bit_in_the_padding,
                   v_long_code_at_545_does_not_fit)
SPLIT_VARIANTS = (v_eos_in_the_lead_ignored, v_symbol_before_a_boundary_dropped, v_symbol_at_a_boundary_twice)


def _caught(variant, cases):
    return [c.label for c in cases if variant(c, E.walk_of(c.data), c.is_name) != E.ref(c.data, c.is_name)]


@pytest.mark.parametrize("variant", STREAM_VARIANTS, ids=lambda v: v.__name__)
def test_stream_corpus_catches(corpora, variant):
    cases = [c for cs in corpora["stream"].values() for c in cs]
    assert _caught(variant, cases), variant.__name__


@pytest.mark.parametrize("variant", SPLIT_VARIANTS, ids=lambda v: v.__name__)
def test_split_corpus_catches(corpora, variant):
    """each form and length on its own: a decoder that is wrong at one segment size only is still caught"""
    for key, cases in list(corpora["split"].items()) + list(corpora["one_string"].items()):
        assert _caught(variant, cases), (variant.__name__, key)
    everything = [c for cs in corpora["split"].values() for c in cs]
    assert _caught(variant, everything), variant.__name__


@pytest.mark.parametrize("variant", (v_eight_bits_of_padding, v_zero_bit_in_the_padding), ids=lambda v: v.__name__)
def test_per_string_corpus_catches(corpora, variant):
    assert _caught(variant, corpora["per_string"]), variant.__name__


def test_models_agree_with_the_reference_when_right(corpora):
    """the variants' own plumbing: with nothing wrong, _result() is huff_ref's verdict"""
    for c in itertools.islice(_all_cases(corpora), 0, None, 7):
        assert _result(c, E.walk_of(c.data), c.is_name) == E.ref(c.data, c.is_name), c.label


def test_dilute_and_arrange():
    cases = E.stream_window_edge()[:40]
    batch = E.arrange(E.dilute(cases, 60))
    assert sum(len(c.data) for c in batch) <= 60 * len(batch) + 3 * len(batch)
    assert [c for c in batch if not c.facts.get("filler")] == cases
    for c, s in zip(batch, E.offsets(batch)):
        if "align" in c.facts:
            assert s % 4 == c.facts["align"]
        assert E.ref(c.data, False)[0] is not None or not c.facts.get("filler")
    assert np.all(np.diff(E.offsets(batch)) >= 0)
