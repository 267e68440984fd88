"""The reference encoder of tests/huff_ref.py, the per-string corpus, the call plans and the mailbox model of
tests/encode_edges.py, and the driver tests/per_string_check.c, checked without a GPU:
  - huff_ref.encode equals the oracle and the golden encode vectors;
  - every class of string the corpus is meant to hold is there, judged from facts recomputed here;
  - the plans have the properties that let a thread tell its answer from any other;
  - the model agrees with the plans' expectations, and each of its four defects disagrees;
  - the service's constants are the ones in the sources;
  - the driver builds, and without a GPU every call of its 16 threads fails soft."""
import itertools
import os
import re
import subprocess

import pytest

import encode_edges as E
import huff_ref as R
from conftest import ROOT, load_golden
from test_capi import build_capi_check

CSRC = os.path.join(ROOT, "h2o_amd", "csrc")


@pytest.fixture(scope="module")
def cases():
    return E.corpus()


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kat", "adversarial", "random_c2"])
def test_ref_encode_matches_the_golden_vectors_and_the_oracle(name, oracle_codec):
    from h2o_amd import synth

    g = load_golden(name)
    strings = synth.unpack(g["enc_in"], g["enc_in_off"])
    good = iter(synth.unpack(g["enc_out"], g["enc_out_off"]))
    assert len(strings) == len(g["enc_len"]) >= 26
    for s, n in zip(strings, g["enc_len"].tolist()):
        want = None if n == 0xFFFFFFFF else next(good)
        assert want is None or len(want) == n
        assert R.encode(s) == want, s.hex()
        assert oracle_codec.encode(s) == want, s.hex()
    assert next(good, None) is None


def test_ref_encode_by_hand():
    """RFC 7541 C.4.1 and the rule's edges: len - 1 bytes encode, len bytes do not, nor does the empty string"""
    assert R.encode(b"www.example.com") == bytes.fromhex("f1e3c2e5f23a6ba0ab90f4ff")
    assert R.encode(b"") is None and R.encode(b"a") is None and R.encode(b"aa") is None
    assert R.encode(b"aaa") == bytes([0b00011000, 0b11000111])  # 15 bits and one of padding
    assert R.encode(b"XXXX") is None and R.encode(b"XXXXXXaa") is None  # 'X' is 0xfc [8]; 58 bits: 8 bytes of 8
    assert R.encode(b"XXXXXaaa") == bytes([0xFC] * 5 + [0b00011000, 0b11000111])  # 55 bits: 7 bytes of 8
    assert R.encode(b"\n" + b"a" * 12)[:4] == bytes([0xFF, 0xFF, 0xFF, 0xF0])  # 0x3ffffffc [30], then 'a' 00011


def test_ref_answers_every_corpus_and_plan_call_as_the_oracle(oracle_codec, cases):
    n = 0
    for q in E.corpus_reqs(cases) + [q for th in E.plan(E.PLAN_MAX_THREADS) for q in th]:
        assert q.answer() == E.oracle_answer(oracle_codec, q.op, q.data, q.is_name, q.soft_in), q.label
        n += 1
    assert n > 4000
    for q in E.corpus_reqs(cases):  # and a decode gives the plain text back
        if q.label.endswith("decoded back"):
            assert q.ret is not None and q.soft_in == 0


# ------------------------------------------------------------------------------------------------
# the constants
# ------------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"[ \t]+", " ", f.read())


def _one(text, pattern):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return int(m[0])


def test_service_constants_match_the_sources():
    launch, kern, capi = _src("hhuff_launch.h"), _src("hhuff_kernels.hip"), _src("hhuff_capi_string.hip")
    assert _one(launch, r"constexpr uint32_t kSvcSlots = (\d+);") == E.SVC_SLOTS == 64
    assert _one(launch, r"constexpr uint32_t kSvcMax = (\d+);") == E.SVC_MAX == 768
    assert _one(launch, r"constexpr uint32_t kOneMax = (\d+);") == E.ONE_MAX
    assert _one(launch, r"uint32_t chunk\[(\d+)\]\[4\];") == E.SVC_IN_CHUNKS == 64
    assert _one(launch, r"uint32_t outc\[(\d+)\]\[4\];") == E.SVC_OUT_CHUNKS == 104
    assert "static_assert(12 * 64 == kSvcMax && (kSvcMax * 8) / 5 <= 12 * 104" in launch
    assert E.SVC_CHUNK * E.SVC_IN_CHUNKS == E.SVC_MAX and 8 * E.SVC_MAX // 5 <= E.SVC_CHUNK * E.SVC_OUT_CHUNKS
    # 12 bytes a chunk on both sides of both directions
    assert "for (size_t i = 0; 12 * i < len; ++i)" in capi and "for (uint32_t i = 0; 12u * i < r; ++i)" in capi
    assert "const bool need = 12u * lane < len;" in kern and "for (uint32_t k = lane; 12u * k < n; k += 64u)" in kern
    assert "hot_ck = min(len / 12u + 2u, 64u);" in kern
    assert _one(capi, r"constexpr uint64_t kSvcIdle = (\d+);") == E.SVC_IDLE_TICKS == 200000
    assert "const uint32_t w = e && *e ? (uint32_t)atoi(e) : 16u;" in kern
    assert "return (w >= 2 && w <= kSvcSlots && kSvcSlots % w == 0) ? w : 16u;" in kern
    assert _one(kern, r"constexpr uint32_t kLongChunk = (\d+);") == E.LONG_CHUNK
    assert "block_encode<4>(" in kern and E.BLOCK_WAVES == 4
    assert "for (uint32_t j0 = 0; j0 < len && !fail; j0 += 64u)" in kern and E.ROUND == 64
    assert "t_svc_slot = (int)(g_svc_threads.fetch_add(1) % hhuff::kSvcSlots);" in capi
    assert "len > hhuff::kSvcMax || !svc_enabled()) return 0;" in capi and "if (len <= hhuff::kOneMax) {" in capi


def test_service_waves_rule():
    """E.service_waves restates service_waves(): divisors of 64 from 2 on, anything else is 16"""
    assert [E.service_waves(str(w)) for w in (2, 4, 8, 16, 32, 64)] == [2, 4, 8, 16, 32, 64]
    assert all(E.service_waves(v) == 16 for v in (None, "", "0", "1", "3", "12", "48", "128", "-2", "x"))


# ------------------------------------------------------------------------------------------------
# coverage, from facts recomputed here
# ------------------------------------------------------------------------------------------------
def _of(cases, kind):
    return [c for c in cases if c.facts["kind"] == kind]


def test_corpus_lengths(cases):
    want = {0, 1, 2, 11, 12, 13, 23, 24, 25, 63, 64, 65, 127, 128, 129, 191, 192, 193, 766, 767, 768, 769, 1023, 1024, 1025,
            1279, 1280, 1281, 32767, 32768, 32769}
    got = {}
    for c in _of(cases, "length"):
        assert len(c.data) == c.facts["len"]
        got[len(c.data)] = c
    assert set(got) == want
    for n, c in got.items():  # text: every one from 3 bytes on encodes
        assert (R.encode(c.data) is None) == (n < 3), c.label
    assert {E.route(1, n) for n in got} == {"service", "one_string", "long"}
    assert E.part_starts(1024) == [0, 256, 512, 768]
    assert E.part_starts(1280) == [0, 320, 640, 960] and E.part_starts(1025) == [0, 320, 640, 960]
    # encode_long_kernel's second round begins at byte 16384: a 30-bit code before, on and after it
    at = {}
    for c in _of(cases, "long_round"):
        assert len(c.data) == 40000 and E.NB[c.data[c.facts["at"]]] == 30 and R.encode(c.data) is not None
        assert sum(E.NB[b] == 30 for b in c.data) == 1
        at[c.facts["at"]] = E.bits_of(c.data[:E.LONG_CHUNK]) % 32  # the carried partial word's fill
    assert set(at) == {16383, 16384, 16385}


def test_corpus_verdict_edges(cases):
    seen = set()
    for c in _of(cases, "verdict"):
        n, bits = len(c.data), E.bits_of(c.data)
        assert n == c.facts["len"] and bits == c.facts["bits"] == 8 * n - 8 + c.facts["over"]
        assert {E.NB[b] for b in c.data} == {5, 6, 7, 8} - ({7} if c.facts["over"] else set())
        enc = R.encode(c.data)
        assert (enc is None) == bool(c.facts["over"]) and (enc is None or len(enc) == n - 1)
        rounds = E.round_bits(c.data)  # the verdict falls in the last round: no earlier one breaks
        assert all(sum(rounds[:k + 1]) <= 8 * n - 8 for k in range(len(rounds) - 1))
        rnd = c.facts["at"] // E.ROUND
        where = {"first" if rnd == 0 else None, "last" if rnd == len(rounds) - 1 else None,
                 "after" if c.facts["at"] % E.ROUND == 0 and c.facts["at"] > 0 else None} - {None}
        for w in where:
            seen.add((n, w, c.facts["over"]))
    for n in E.VERDICT_LENGTHS:
        for w in ("first", "last") + (("after",) if n > 64 else ()):
            assert (n, w, 0) in seen and (n, w, 1) in seen, (n, w)
    # the pairs differ in the one symbol at the spot
    for a, b in zip(_of(cases, "verdict")[::2], _of(cases, "verdict")[1::2]):
        assert [i for i in range(len(a.data)) if a.data[i] != b.data[i]] == [a.facts["at"]] == [b.facts["at"]]
    early = _of(cases, "early")
    for c in early:
        assert R.encode(c.data) is None and R.encode(c.data[-40:]) is not None  # (the text behind it compresses)
        lim, rounds = 8 * len(c.data) - 8, E.round_bits(c.data)
        first = next(k for k in range(len(rounds)) if sum(rounds[:k + 1]) > lim)
        if c.facts["round"] is not None:
            unit = E.ROUND if len(c.data) <= E.SVC_MAX else E.LONG_CHUNK
            assert first * E.ROUND // unit == c.facts["round"] and first < len(rounds) - 1
    assert {E.route(1, len(c.data)) for c in early} == {"service", "one_string", "long"}
    assert any(rnd == 0 for rnd in (c.facts["round"] for c in early)) and any(c.facts["round"] for c in early)


def test_corpus_codes(cases):
    syms = {}
    for c in _of(cases, "code"):
        assert c.data[8] == c.facts["sym"] and E.NB[c.data[8]] == c.facts["nbits"] and R.encode(c.data) is not None
        syms[c.data[8]] = c
    assert set(syms) == set(range(256)) and {c.facts["nbits"] for c in syms.values()} == set(E.NB)
    offs = {}
    for c in _of(cases, "long30"):
        k = c.facts["at"]
        assert c.data[k] == c.facts["sym"] and c.data[k] in E.LONG30 and R.encode(c.data) is not None
        assert all(E.NB[b] == 5 for b in c.data[:k] + c.data[k + 1:])
        assert E.bits_of(c.data[:k]) % 32 == c.facts["word_off"]
        offs.setdefault((c.data[k], E.route(1, len(c.data))), set()).add(E.bits_of(c.data[:k]) % 32)
    for b in E.LONG30:
        assert offs[(b, "service")] == offs[(b, "one_string")] == set(range(32)), b
    assert len(offs[(E.LONG30[0], "long")]) == 8
    pads = {}
    for c in _of(cases, "long30_last"):
        assert c.data[-1] in E.LONG30 and R.encode(c.data) is not None
        pads.setdefault(c.data[-1], set()).add(-E.bits_of(c.data) % 8)
    assert all(pads[b] == set(range(8)) for b in E.LONG30)


def test_corpus_meeting_points(cases):
    got = {1024: set(), 1280: set()}
    for c in _of(cases, "meeting"):
        starts = E.part_starts(c.data)
        assert R.encode(c.data) is not None
        assert starts[1][1] % 32 == c.facts["word_off"]
        got[len(c.data)].add(starts[1][1] % 32)
    assert got[1024] == got[1280] == set(range(1, 32))
    assert E.part_starts(1024)[1] == 256 and E.part_starts(1280)[1] == 320


def test_corpus_output_lengths(cases):
    enc = {}
    for c in _of(cases, "out_len"):
        out = R.encode(c.data)
        assert out is not None and len(out) == c.facts["out_len"] and -E.bits_of(c.data) % 8 == c.facts["pad"]
        assert len(c.data) <= E.SVC_MAX
        enc.setdefault(len(out) % 12, set()).add(len(out))
    assert set(enc) == set(range(12)) and {12, 24, 36, 600} <= enc[0] and {599, 601} <= enc[11] | enc[1]
    dec = {}
    for c in _of(cases, "dec_out"):
        out, st = R.decode(c.data, False)
        assert c.op == 0 and out is not None and len(out) == c.facts["out_len"] and len(c.data) == c.facts["in_len"]
        dec[len(c.data)] = len(out)
    assert dec[768] == 1228 and (1228 + 11) // 12 == 103 and dec[767] == 1227 and dec[766] == 1225
    assert {12, 24, 600, 1224} <= set(dec.values()) and max(dec) <= E.SVC_MAX


# ------------------------------------------------------------------------------------------------
# the plans
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_plan():
    return E.plan(E.PLAN_MAX_THREADS)


def _chunks(b):
    return [b[i:i + 12] for i in range(0, len(b), 12)]


def test_plan_requests_of_a_mailbox_differ_in_every_chunk(full_plan):
    """stronger than `consecutive`: any two requests that ever share a mailbox (threads t and t + 64 included, whose
    order inside a round is not fixed) differ in every input chunk and every output chunk both have, within the bytes
    both have -- so whichever request left a stale chunk behind, taking it changes the answer"""
    assert len(full_plan) == 72 and all(len(th) == E.PLAN_ROUNDS == 40 for th in full_plan)
    for m in range(64):
        box = [q for t in range(m, 72, 64) for q in full_plan[t]]
        for a, b in itertools.combinations(box, 2):
            for x, y in ((a.data, b.data), (a.out, b.out)):
                n = min(len(x), len(y))
                for cx, cy in zip(_chunks(x[:n]), _chunks(y[:n])):
                    assert cx != cy, (a.label, b.label)


def test_plan_consecutive_requests_cover_the_length_classes(full_plan):
    for t, th in enumerate(full_plan):
        classes = set()
        for a, b in zip(th, th[1:]):
            assert a.op != b.op, (t, a.label)  # encode and decode alternate
            classes.add((len(b.data) > len(a.data)) - (len(b.data) < len(a.data)))
            if len(a.data) == len(b.data):
                assert all(x != y for x, y in zip(_chunks(a.data), _chunks(b.data)))
        assert classes == {-1, 0, 1}, t
        # short then long: more chunks than the wave reads ahead after the short one (hot_ck = len / 12 + 2)
        assert any(len(a.data) // 12 + 2 < (len(b.data) + 11) // 12 for a, b in zip(th, th[1:]))
    # two owners of one mailbox move together: the mailbox sees encodes and decodes in turn, two at a time
    for t in range(64, 72):
        assert [q.op for q in full_plan[t]] == [q.op for q in full_plan[t - 64]]


def test_plan_rounds_have_different_lengths_and_answers(full_plan):
    """every request of a round (so: of one wave's mailboxes, whatever the wave count) has a length and an answer of
    its own; one request a round fails at most"""
    for r in range(E.PLAN_ROUNDS):
        rnd = [th[r] for th in full_plan]
        assert len({len(q.data) for q in rnd}) == len(rnd)
        assert len({(q.ret, q.out) for q in rnd}) == len(rnd)
        assert sum(q.ret is None for q in rnd) <= 1
    fails = [q for th in full_plan for q in th if q.ret is None]
    assert {q.op for q in fails} == {0, 1} and len(fails) >= 8
    assert {q.soft_in for th in full_plan for q in th} >= {0, 1, 2, 3, 0x10}
    assert {q.st for th in full_plan for q in th if not q.op} >= {0, 1, 2}


@pytest.mark.parametrize("nthreads", [2, 8, 16, 17, 32, 64, 72])
def test_every_plan_has_the_long_then_short_pair(nthreads):
    th = E.plan(nthreads)
    assert len(th) == nthreads
    pairs = [(a, b) for t in th for a, b in zip(t, t[1:]) if len(a.data) == 768 and len(b.data) == 1]
    assert pairs  # 768 then 1 byte: 63 stale chunks keep the old request's number
    assert all(len(q.data) <= E.SVC_MAX for t in th for q in t)


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
CONFIGS = [(72, 16), (32, 2), (17, 16), (64, 64)]


@pytest.mark.parametrize("nthreads,waves", CONFIGS)
def test_model_agrees_with_the_plans(nthreads, waves):
    assert E.model_run(E.plan(nthreads), waves) == []


@pytest.mark.parametrize("defect", E.DEFECTS)
def test_model_defects_are_caught_by_the_plans(defect):
    for nthreads, waves in CONFIGS[:2]:  # (the other two: a wave with one busy mailbox cannot show every defect)
        bad = E.model_run(E.plan(nthreads), waves, defect=defect, limit=3)
        assert bad, (defect, nthreads, waves)
        t, m, r, label, what = bad[0]
        assert m == t % 64 and label == E.plan(nthreads)[t][r].label


def test_model_defects_show_in_many_rounds():
    """not only in a plan's first call: over the plans of 72 and 16 threads at 16 waves and of 32 threads at 2, each
    defect shows on 8 mailboxes or more and in 10 rounds or more.  (Chunks read ahead and trusted show where a wave's
    hot mailbox is the first one pending, a kept ck_slot where it is not and a shorter request follows in it.)"""
    for defect in E.DEFECTS:
        bad = [b for nthreads, waves in ((72, 16), (16, 16), (32, 2))
               for b in E.model_run(E.plan(nthreads), waves, defect=defect)]
        assert len({m for _, m, _, _, _ in bad}) >= 8, (defect, len(bad))
        assert len({r for _, _, r, _, _ in bad}) >= 10, (defect, len(bad))


# ------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------
def test_driver_builds_and_fails_soft_without_a_gpu(tmp_path, oracle_codec):
    """tests/per_string_check.c: 16 threads run their plan; without a GPU every call returns SIZE_MAX with a reason"""
    import torch

    exe = build_capi_check("per_string_check.c")
    assert os.path.exists(exe) and exe != build_capi_check()
    if torch.cuda.is_available():
        pytest.skip("a GPU is present (tests/test_per_string_service.py runs the driver on it)")
    th = E.plan(16)
    reqs = [E.expect(E.Req(q.label, q.op, q.data, q.is_name, q.soft_in), oracle_codec) for t in th for q in t]
    E.write_cases(tmp_path / "cases", reqs)
    E.write_plan(tmp_path / "plan", [{"calls": [(t * E.PLAN_ROUNDS + r, 0) for r in range(E.PLAN_ROUNDS)]}
                                     for t in range(16)])
    r = subprocess.run([exe, "nogpu", str(tmp_path / "cases"), str(tmp_path / "plan")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "per_string_check: ok threads=16 calls=%d served=0" % (16 * E.PLAN_ROUNDS) in r.stdout
