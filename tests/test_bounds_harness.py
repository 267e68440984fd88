"""tests/bounds_harness.py proved without a GPU: the oracle, run as the implementation on exact-size guarded arrays,
stays inside every footprint and passes check(); faulty stand-ins -- numpy edits of the oracle's result -- are
caught one by one."""
import numpy as np
import pytest

import bounds_harness as H

OPS = ("decode", "encode", "flatten")
LAYOUTS = ("contiguous", "pairs", "explicit")
G = H.GUARD


def _case(oracle_codec, op, layout, fill, sentinel, n=70, in_off0=7, slack=0):
    if op == "decode":
        strings, names = H.huffman_batch(oracle_codec, "short", n, 3)
        strings[5] = H.huffman_of_len(oracle_codec, np.random.default_rng(1), 513)
    else:
        strings, names = H.plain_batch("short", n, 4), None
        strings[5] = H.text(np.random.default_rng(2), 700)
    permute = op != "flatten"  # the implicit flatten slots (in_off[i] + 11 i) need the strings in index order
    inp = H.place_input(strings, layout, in_off0, fill, op=op, seed=n, permute=permute)
    if slack:
        inp = H.place_input(strings, layout, in_off0, fill, in_size=inp["in_size"] + slack, op=op, seed=n,
                            permute=permute)
    kw = {}
    if op == "decode":
        kw["names"] = H.name_bits(names, fill)
    if op == "flatten":
        rng = np.random.default_rng(9)
        kw = dict(prefix_bits=5, first=rng.integers(0, 256, n + H.EXTRA).astype(np.uint8),
                  raw=H.name_bits(rng.random(n) < 0.2, fill))
    res, exp = H.oracle_run(oracle_codec, op, inp, sentinel, **kw)
    return inp, res, exp


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("op", OPS)
def test_oracle_passes_as_the_implementation(oracle_codec, op, layout):
    outs = []
    for fill, sentinel in H.RUNS:
        for slack in (0, 333):
            inp, res, exp = _case(oracle_codec, op, layout, fill, sentinel, slack=slack)
            mask = H.mask_of(op, inp)
            H.check(res, exp, mask, sentinel, starts=H.out_starts(op, inp), label="%s %s" % (op, layout))
            assert mask.any() and not mask.all() or layout == "contiguous"
        outs.append(exp)
    np.testing.assert_array_equal(outs[0]["out_len"], outs[1]["out_len"])  # the oracle does not see the fill
    if op != "flatten":  # failures next to successes (a flattened string never fails: it is sent raw)
        assert (outs[0]["out_len"] == H.FAIL).any() and (outs[0]["out_len"] != H.FAIL).any()


def test_layouts_are_what_they_say(oracle_codec):
    strings = H.plain_batch("short", 40, 1)
    for fill in (0x00, 0xFF):
        for off0 in (0, 1, 7, 13):
            inp = H.place_input(strings, "contiguous", off0, fill, in_size=3000)
            assert inp["in_off"][0] == off0 and inp["data"].size == 3000 and inp["whole"].size == 3000 + 2 * G
            assert (inp["whole"].ctypes.data + G) % 16 == 0
            used = H.ranges_mask(inp["in_off"][:40].astype(np.int64), inp["in_off"][1:41].astype(np.int64), 3000)
            assert (inp["data"][~used] == fill).all() and (inp["whole"][:G] == fill).all()
            assert (inp["whole"][-G:] == fill).all()
            assert set(inp["in_off"][41:].tolist()) == {0, 3000}  # the poison stays in range
        p = H.place_input(strings, "pairs", 1, fill)
        s, L = p["in_off"][:40].astype(np.int64), p["in_len"][:40].astype(np.int64)
        assert [bytes(p["data"][a:a + b]) for a, b in zip(s, L)] == strings
        assert (np.diff(s) < 0).any()  # a permuted order
        assert (p["data"][~H.ranges_mask(s, s + L, p["in_size"])] == fill).all()
        assert ((p["in_off"][40:].astype(np.int64) + p["in_len"][40:]) <= p["in_size"]).all()
        e = H.place_input(strings, "explicit", 0, fill, op="decode")
        d = e["out_off"][:40].astype(np.int64)
        ends = d + (8 * e["lens"]) // 5
        gaps = d[:-1] - ends[1:]  # reversed order: string i + 1 lies before string i
        assert gaps.min() == 0 and gaps.max() <= 7 and len(set((d % 16).tolist())) > 8
        assert e["out_size"] == ends[0]
    w = H.name_bits([True, False, True], 0xFF)
    assert w[0] == 0xFFFFFFFD and (w[1:] == 0xFFFFFFFF).all()
    assert H.name_bits([True, False, True], 0x00)[0] == 5


def test_implicit_decode_footprint_is_the_slot():
    """[floor(8 s / 5), floor(8 (s + len) / 5)): disjoint inputs give disjoint footprints, and a slot holds
    floor(8 len / 5) bytes or one more"""
    off = np.array([3, 3, 4, 9, 17, 17], np.int64)
    lens = np.array([0, 1, 5, 8, 0, 2], np.int64)
    m = H.footprint("decode", "contiguous", off, lens, 6, None, 40)
    exp = np.zeros(40, bool)
    for s, L in zip(off, lens):
        lo, hi = 8 * s // 5, 8 * (s + L) // 5
        assert not exp[lo:hi].any() and 0 <= (hi - lo) - 8 * L // 5 <= 1
        exp[lo:hi] = True
    np.testing.assert_array_equal(m, exp)


def _sabotage(oracle_codec, edit, op="decode", layout="contiguous"):
    """run A passes untouched; with the stand-in's edit, check() must fail in at least one of the two runs"""
    caught = []
    for fill, sentinel in H.RUNS:
        inp, res, exp = _case(oracle_codec, op, layout, fill, sentinel)
        mask, starts = H.mask_of(op, inp), H.out_starts(op, inp)
        H.check(res, exp, mask, sentinel, starts=starts)
        edit(inp, res, exp, mask, starts, fill, sentinel)
        try:
            H.check(res, exp, mask, sentinel, starts=starts, label="stand-in")
            caught.append(None)
        except AssertionError as e:
            caught.append(str(e))
    return caught


@pytest.mark.parametrize("op,layout", [("decode", "pairs"), ("decode", "explicit"), ("encode", "pairs"),
                                       ("encode", "explicit"), ("flatten", "pairs"), ("flatten", "explicit")])
def test_one_byte_past_a_region_is_caught(oracle_codec, op, layout):
    def edit(inp, res, exp, mask, starts, fill, sentinel):
        past = np.nonzero(mask[:-1] & ~mask[1:])[0] + 1  # first bytes behind a region that belong to no region
        assert past.size
        res["out"][G + past[past.size // 2]] ^= 0x01

    c = _sabotage(oracle_codec, edit, op, layout)
    assert all(m and "outside the footprint" in m for m in c), c


def test_one_byte_before_a_region_is_caught(oracle_codec):
    def edit(inp, res, exp, mask, starts, fill, sentinel):
        before = np.nonzero(~mask[:-1] & mask[1:])[0]
        res["out"][G + before[0]] = 0

    assert all(_sabotage(oracle_codec, edit, "encode", "explicit"))


@pytest.mark.parametrize("name", ["out", "out_len", "status"])
def test_rear_guard_write_is_caught(oracle_codec, name):
    def edit(inp, res, exp, mask, starts, fill, sentinel):
        res[name][res[name].size - G] ^= 0xFF  # the first byte behind the array: out_len[n], status[n], out[size]

    assert all(_sabotage(oracle_codec, edit))


def test_front_guard_write_is_caught(oracle_codec):
    def edit(inp, res, exp, mask, starts, fill, sentinel):
        res["out"][G - 1] = 0

    assert all(_sabotage(oracle_codec, edit))


def test_kept_byte_left_at_the_sentinel_is_caught(oracle_codec):
    """a kept byte that was never written holds the sentinel: it can equal the oracle's byte under one sentinel,
    never under both"""
    for op in OPS:
        hits = []

        def edit(inp, res, exp, mask, starts, fill, sentinel, hits=hits):
            ok = np.nonzero((exp["out_len"] != H.FAIL) & (exp["out_len"] > 0))[0]
            i = ok[len(ok) // 2]
            res["out"][G + starts[i]] = sentinel
            hits.append(exp["out"][starts[i]] == sentinel)

        c = _sabotage(oracle_codec, edit, op)
        assert any(c) and all(m or h for m, h in zip(c, hits)), (op, c)


def test_result_that_depends_on_the_fill_is_caught(oracle_codec):
    """a decoder that reads the byte behind a string takes 0xFF for more padding (run B agrees with the oracle by
    luck) and 0x00 for more symbols; an encoder that reads it folds it into its last byte"""
    def dec(inp, res, exp, mask, starts, fill, sentinel):
        i = int(np.nonzero(exp["out_len"] != H.FAIL)[0][3])
        if fill != 0xFF:  # the byte behind the string, were it the run's fill
            H.entries(res["out_len"], np.uint32)[i] += 1

    def enc(inp, res, exp, mask, starts, fill, sentinel):
        i = int(np.nonzero(exp["out_len"] != H.FAIL)[0][3])
        res["out"][G + starts[i] + int(exp["out_len"][i]) - 1] &= 0xF0 | (fill & 0x0F)

    c = _sabotage(oracle_codec, dec)
    assert c[0] and c[1] is None, c  # only the run with fill 0x00 shows it
    c = _sabotage(oracle_codec, enc, "encode")
    assert any(c), c


def test_wrong_length_or_status_is_caught(oracle_codec):
    def ln(inp, res, exp, mask, starts, fill, sentinel):
        H.entries(res["out_len"], np.uint32)[inp["n"] - 1] ^= 1

    def st(inp, res, exp, mask, starts, fill, sentinel):
        H.entries(res["status"], np.uint8)[0] ^= 2

    assert all(_sabotage(oracle_codec, ln)) and all(_sabotage(oracle_codec, st))
