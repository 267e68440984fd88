"""The header-block edge harness (blocks_harness.py) proves itself without a GPU: the oracle, run through the guarded
call as if it were the implementation, passes every corpus; faulty variants of it are caught; the restatement and
the compiled reference agree on every corpus (where oracle/_ref exists) and on the committed reference results
(tests/golden/block_edges.npz, written by oracle/gen_golden.py); and the corpora reach the statuses and paths they
are built for."""
import numpy as np
import pytest

import blocks_corpora as BC
import blocks_harness as BH
import qpack_corpora as QC
from conftest import load_golden

HPACK = BC.NAMES
MODES, corpus_modes, reference_pairs, fixture_key = BC.MODES, BC.corpus_modes, BC.reference_pairs, BC.fixture_key


def first_batches(c, mode):
    """the cases once, in order (or every case alone), and one repeated shape"""
    bs = BC.batches(c, mode)
    return bs if c.get("alone") else bs[:1] + [b for b in bs if "nconn=65" in b[0]]


def through_harness(codec, bt, modes, fault=None, label=""):
    exp = BH.expected(codec, bt, modes)
    BH.run(lambda sentinel: BH.OracleBlocks(codec, fault), bt, modes,
           check=lambda a, i, sentinel: BH.check_call(a, exp[i], label))
    return exp


@pytest.mark.parametrize("name", HPACK)
def test_oracle_passes_as_the_implementation(oracle_codec, name):
    c = BC.corpora()[name]
    for mode in corpus_modes(c):
        for label, bt, modes in first_batches(c, mode):
            through_harness(oracle_codec, bt, modes, label=label)


@pytest.mark.parametrize("fault,corpus,what", [
    ("arena+1", "arena", "belongs to no non-empty block|guard"),
    ("slot+1", "arena", "name_off: rear guard"),
    ("stale", "continuation_4", "differ|oracle"),
    ("huff_len", "arena", "Huffman .*: nfields = 1, oracle 0"),
])
def test_faulty_implementations_are_caught(oracle_codec, fault, corpus, what):
    c = BC.corpora()[corpus]
    label, bt, modes = BC.batches(c)[0]
    with pytest.raises(AssertionError, match=what):
        through_harness(oracle_codec, bt, modes, fault=fault, label=label)


def test_poisoning_is_what_catches_the_stale_input(oracle_codec):
    """the same faulty implementation passes when the harness leaves the previous calls' buffers alone"""
    c = BC.corpora()["continuation_4"]
    label, bt, modes = BC.batches(c)[0]
    exp = BH.expected(oracle_codec, bt, modes)
    BH.run(lambda sentinel: BH.OracleBlocks(oracle_codec, "stale"), bt, modes, poison=False,
           check=lambda a, i, sentinel: BH.check_call(a, exp[i], label))


@pytest.mark.parametrize("name", HPACK)
def test_restatement_matches_compiled_reference(oracle_codec, name):
    from oracle import oracle as O

    if not O.ref_available():
        pytest.skip("oracle/_ref not built (no reference tree here)")
    c = BC.roomy(BC.corpora()[name])
    for mode in corpus_modes(c):
        for label, bt, modes in BC.batches(c, mode)[:None if c.get("alone") else 1]:
            want = BH.summary(BH.expected(O.ref(), bt, modes), bt, modes)
            got = BH.summary(BH.expected(oracle_codec, bt, modes), bt, modes)
            BH.assert_same_summary(got, want, label)


@pytest.mark.parametrize("name", [n for n in HPACK if n != "big"])
def test_restatement_matches_reference_fixture(oracle_codec, name):
    g = load_golden("block_edges")
    for label, bt, modes in reference_pairs(BC.corpora()[name]):
        got = BH.summary(BH.expected(oracle_codec, bt, modes), bt, modes)
        want = {k: g[fixture_key(name, label, k)] for k in got}
        BH.assert_same_summary(got, want, label)


# ---------------------------------------------------------------------------------------------------
# QPACK
# ---------------------------------------------------------------------------------------------------
QPACK = QC.NAMES
DF = 0x30200  # HHUFF_QPK_DECOMPRESSION_FAILED
BLOCKED = -302


qmodes, qreference_pairs = QC.qmodes, QC.reference_pairs


def qfirst_batches(c):
    bs = QC.batches(c)
    return bs if c.get("alone") else bs[:1] + [b for b in bs if "nconn=65" in b[0]]


@pytest.mark.parametrize("name", QPACK)
def test_oracle_passes_as_the_qpack_implementation(oracle_codec, name):
    c = QC.corpora()[name]
    for mode in qmodes(c):
        for label, bt in qfirst_batches(c):
            exp = BH.qexpected(oracle_codec, bt, mode)
            BH.qrun(lambda sentinel: BH.OracleQpack(oracle_codec, bt), bt, mode,
                    check=lambda a, i, sentinel: BH.check_call(a, exp[i], label))


@pytest.mark.parametrize("name", QPACK)
def test_qpack_restatement_matches_compiled_reference(oracle_codec, name):
    from oracle import oracle as O

    if not O.ref_available():
        pytest.skip("oracle/_ref not built (no reference tree here)")
    c = QC.roomy(QC.corpora()[name])
    for mode in qmodes(c):
        for label, bt in QC.batches(c)[:None if c.get("alone") else 1]:
            want = BH.qsummary(BH.qexpected(O.ref(), bt, mode), bt, mode)
            got = BH.qsummary(BH.qexpected(oracle_codec, bt, mode), bt, mode)
            BH.assert_same_summary(got, want, "%s %s" % (label, mode))


@pytest.mark.parametrize("name", QPACK)
def test_qpack_restatement_matches_reference_fixture(oracle_codec, name):
    g = load_golden("block_edges")
    for label, bt, mode in qreference_pairs(QC.corpora()[name]):
        got = BH.qsummary(BH.qexpected(oracle_codec, bt, mode), bt, mode)
        BH.assert_same_summary(got, {k: g[fixture_key(name, label, k)] for k in got}, label)


def test_qpack_corpora_cover_the_paths(oracle_codec):
    """every sstatus and enc_status value include/hhuff.h defines, both soft bits, an instruction left unconsumed,
    and HHUFF_QPK_ARENA only where a case aims at it; the arena cases' statuses as the header states them"""
    ss, es, soft, partial = set(), set(), 0, 0
    for name, c in QC.corpora().items():
        label, bt = QC.batches(c)[0]
        for e, cl in zip(BH.qexpected(oracle_codec, bt), bt["calls"]):
            ss |= set(int(x) for x in e["sstatus"])
            es |= set(int(x) for x in e["enc_status"])
            partial += int(((e["enc_status"] == 0) & (e["enc_consumed"] < cl["enc_len"])).sum())
            slots = BH._ranges(cl["blk_off"][:-1].astype(np.int64), e["nfields"].astype(np.int64))
            soft |= int(np.bitwise_or.reduce(e["fflags"][slots], initial=0))
            for k in np.nonzero(e["sstatus"] == BH.ARENA)[0]:
                assert name == "q_arena", cl["labels"][k]
            if name != "q_arena":
                continue
            for k, lab in enumerate(cl["labels"]):
                if not lab.endswith("section 0]"):
                    continue
                got, what = (int(e["sstatus"][k]), int(e["nfields"][k])), lab.split("[")[0]
                if what.endswith("exact fit"):
                    assert got == (0, 3), lab
                elif what.endswith("one byte short"):
                    assert got == (BH.ARENA, {"first": 0, "middle": 1, "last": 2}[what.split(",")[0].split()[-1]]), lab
                elif what.startswith("Huffman literal fits decoded"):
                    assert got == (BH.ARENA, 1), lab
                elif what.startswith("upper-case raw name"):
                    assert got == (DF, 0), lab
                elif what.startswith("bad Huffman value, slice too small"):
                    assert got == (BH.ARENA, 0), lab
    # hhuff_qpack_parse_requests: its own verdicts (-254 among them), err_desc codes and acknowledgments
    rs, err, acks = set(), set(), set()
    for name in QC.ALL_MODES:
        label, bt = QC.batches(QC.corpora()[name])[0]
        for e in BH.qexpected(oracle_codec, bt, "qreq"):
            rs |= set(int(x) for x in e["sstatus"])
            err |= set(int(x) for x in e["qreq"][:, 10])
            acks |= set(int(x) for x in e["qreq"][:, 13])
    assert {0, BH.INVALID_CHAR, DF, BH.SKIPPED, BLOCKED} <= rs
    assert {0, 1, 2, 4, 8} <= err  # soft name / value, invalid pseudo-header, decode_header's own
    assert 0 in acks and max(acks) >= 2
    assert {0, DF, BH.ARENA, BH.SKIPPED, BLOCKED} <= ss
    assert {0, DF, BH.SKIPPED} <= es
    assert soft & 1 and soft & 2 and partial > 20


def test_arena_cases_follow_the_header(oracle_codec):
    """include/hhuff.h: a string that does not fit the block's slice stops the block with HHUFF_BLK_ARENA, the fields
    before it stand; a Huffman literal needs floor(8 len / 5) bytes free whatever it decodes to; an upper-case raw
    name is PROTOCOL even when the slice is too small; a bad Huffman literal in a too-small slice is ARENA"""
    label, bt, modes = BC.batches(BC.corpora()["arena"])[0]
    cl = bt["calls"][0]
    e = BH.expected(oracle_codec, bt, modes)[0]
    seen = set()
    for b, lab in enumerate(cl["labels"]):
        if not lab.endswith("block %d]" % (1 if ", " in lab and ("exact fit" in lab or "short" in lab) else 0)):
            continue
        st, nf = int(e["bstatus"][b]), int(e["nfields"][b])
        what = lab.split("[")[0]
        seen.add(what.split(",")[-1].strip() if ", " in what else what)
        if what.endswith("exact fit"):
            assert (st, nf) == (0, 3), lab
        elif what.endswith("one byte short"):
            assert (st, nf) == (BH.ARENA, {"first": 0, "middle": 1, "last": 2}[what.split(",")[0].split()[-1]]), lab
        elif what.startswith("Huffman literal fits decoded"):
            assert (st, nf) == (BH.ARENA, 1), lab
        elif what.startswith(("Huffman name fits decoded", "bad Huffman name, slice too small")):
            assert (st, nf) == (BH.ARENA, 0), lab
        elif what.startswith("upper-case raw name behind"):
            assert (st, nf) == (BH.PROTOCOL, 1), lab
        elif what.startswith("upper-case raw name"):
            assert (st, nf) == (BH.PROTOCOL, 0), lab
        elif what.startswith("bad Huffman value, slice too small"):
            assert (st, nf) == (BH.ARENA, 0), lab
        elif what.startswith("bad Huffman value, slice fits"):
            assert (st, nf) == (BH.COMPRESSION, 0), lab
    assert {"exact fit", "one byte short"} <= seen
    # a zero-byte slice: a static field and a one-byte name do not fit; a lone size update ends the block as h2o ends
    # it (COMPRESSION) and a field of two empty strings needs no room
    zero = [int(e["bstatus"][b]) for b, lab in enumerate(cl["labels"]) if lab.startswith("zero-byte slice")]
    assert zero == [BH.ARENA, BH.COMPRESSION, 0, BH.ARENA]


def test_corpora_cover_the_paths(oracle_codec):
    """conditions on the inputs: every bstatus value include/hhuff.h defines for the three modes, both soft bits, a
    block with nfields == its length, and no HHUFF_BLK_ARENA outside the cases that aim at it"""
    st = {m: set() for m in MODES}
    soft, full, err = 0, 0, set()
    for name, c in BC.corpora().items():
        for mode in corpus_modes(c):
            label, bt, modes = BC.batches(c, mode)[0]
            for e, cl in zip(BH.expected(oracle_codec, bt, modes), bt["calls"]):
                st[mode or "plain"] |= set(int(x) for x in e["bstatus"])
                L = np.diff(cl["blk_off"].astype(np.int64))
                full += int(((e["nfields"] == L) & (L > 0)).sum())
                slots = BH._ranges(cl["blk_off"][:-1].astype(np.int64), e["nfields"].astype(np.int64))
                soft |= int(np.bitwise_or.reduce(e["fflags"][slots], initial=0))
                for b in np.nonzero(e["bstatus"] == BH.ARENA)[0]:
                    assert name in ("arena",) or "arena" in cl["labels"][b], cl["labels"][b]
                for m in ("req", "res"):
                    if m in e:
                        err |= set(int(x) for x in e[m][:, {"req": 10, "res": 2}[m]])
    assert {0, BH.COMPRESSION, BH.PROTOCOL, BH.ARENA, BH.SKIPPED} <= st["plain"]
    assert {0, BH.INVALID_CHAR, BH.COMPRESSION, BH.PROTOCOL, BH.ARENA, BH.SKIPPED} <= st["req"]
    assert {0, BH.INVALID_CHAR, BH.COMPRESSION, BH.PROTOCOL, BH.ARENA, BH.SKIPPED} <= st["res"]
    assert soft & 1 and soft & 2 and soft & 4
    assert full >= 4
    assert {0, 1, 2, 3, 7} <= err  # soft name / value, headers too long, upper-case name


def test_stage_cases_lie_on_the_side_they_name():
    """the tile cases of the staged literal kernel, from their payload offsets (blocks_corpora.tile_plan): the cases
    named below a stage are staged in LDS, those above it decode from global memory, and in each trio only the stage
    it names decides"""
    for cases in (BC.corpora()["stage"]["cases"], [k for k in QC.corpora()["q_positions"]["cases"] if "plan" in k]):
        assert len(cases) == 9
        for k in cases:
            span, ospan, staged, want = k["plan"]
            assert staged == want, k["name"]
            if "input span" in k["name"]:
                assert ospan <= BC.OUT_STAGE // 2 and abs(span - BC.IN_STAGE) <= 16, k["name"]
            else:
                assert span <= BC.IN_STAGE - 64 and abs(ospan - BC.OUT_STAGE) <= 4, k["name"]
        assert sum(k["plan"][2] for k in cases) == 5
