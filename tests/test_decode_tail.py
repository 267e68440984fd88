"""The staged decoders' tail (decode_staged_lane_v7): the last <= 26 bits of a string, where the checked steps run
and a vote on the bits left decides whether the wave takes another one.

Every string of these batches ends in a hand-built tail -- runs of shortest codes, codes longer than the LUT
window in and at the end of the tail, padding of every length, padding with a zero bit, EOS, codes cut short by
the string's end, strings too short for the bulk loop, empty strings -- behind no text at all or behind enough
ordinary text for the bulk loop to run, mixed with ordinary strings.  Batches of 128..192 strings (two or three
64-string tiles) go through the slot and the packed entry points on both staged kernels; lengths, statuses and
bytes must equal the oracle's (tests/bounds_harness.py, as tests/test_batch_bounds.py)."""
import itertools

import numpy as np
import pytest

import bounds_harness as H
from test_batch_bounds import DEFAULT_DEFER, STAGED, _dev, _packed_expected, edge_defer, route_sizes, sweep

# mean <= 40: decode_staged_kernel's short stage; 41..128 at the staged price: its long stage
ROUTES = (("le", 40, None), ("ge", 41, ("/staged", STAGED)))
PACKED_ROUTES = (("le", 40, None), ("ge", 41, None))
SPECIALS_PER_BATCH = 128
ORDINARY_PER_BATCH = 48


def _codes():
    from h2o_amd import tables

    return [format(int(c), "0%db" % int(n)) for c, n in zip(tables.ENC_CODE, tables.ENC_NBITS)]


def _sym_of_len(codes, L):
    """the first symbol whose code has L bits"""
    return next(s for s in range(256) if len(codes[s]) == L)


def _fillers(codes):
    """residue r -> bits of at most three 5..8-bit symbols whose lengths add up to r mod 8"""
    unit = {L: codes[_sym_of_len(codes, L)] for L in (5, 6, 7, 8)}
    best = {0: ""}
    for k in (1, 2, 3):
        for combo in itertools.product((5, 6, 7, 8), repeat=k):
            best.setdefault(sum(combo) % 8, "".join(unit[L] for L in combo))
    assert sorted(best) == list(range(8))
    return best


def tail_cases(codes):
    """-> [(label, tail bits)]: what a string ends in.  The bits in front of a tail are chosen so that the string
    is whole bytes long, so a tail holds its own padding."""
    five = [s for s in range(256) if len(codes[s]) == 5]
    long_syms = sorted((s for s in range(256) if len(codes[s]) > 13), key=lambda s: len(codes[s]))
    long_lens = sorted({len(codes[s]) for s in long_syms})
    by_len = {L: next(s for s in long_syms if len(codes[s]) == L) for L in long_lens}
    assert long_lens[0] == 14 and long_lens[-1] == 30
    e = codes[five[4]]
    cases = []
    for k in range(8):  # five 5-bit symbols, and every valid padding length behind shortest codes
        cases.append(("5x5 pad%d" % k, "".join(codes[five[(k + j) % len(five)]] for j in range(5)) + "1" * k))
    for k in range(8):  # every valid padding length behind ordinary symbols (6-, 7- and 8-bit codes)
        cases.append(("text pad%d" % k, codes[_sym_of_len(codes, 6)] + codes[_sym_of_len(codes, 8)] +
                      codes[_sym_of_len(codes, 7)] + "1" * k))
    for L in long_lens:  # 5-bit, a code longer than the window, 5-bit (L <= 16: all within 26 bits)
        cases.append(("5 long%d 5" % L, e + codes[by_len[L]] + e))
        cases.append(("5 long%d 5 pad" % L, e + codes[by_len[L]] + e + "1" * ((-10 - L) % 8)))
    for L in long_lens:  # a long code as the very last symbol, padded and not
        cases.append(("long%d last" % L, codes[by_len[L]]))
        cases.append(("long%d last pad" % L, codes[by_len[L]] + "1" * ((-L) % 8)))
        cases.append(("text long%d last" % L,
                      e + codes[_sym_of_len(codes, 7)] + codes[by_len[L]] + "1" * ((-12 - L) % 8)))
    for k in (5, 6, 7):  # padding with one zero bit, at every place
        for z in range(k):
            cases.append(("pad%d zero@%d" % (k, z), e + "1" * z + "0" + "1" * (k - 1 - z)))
    eos = "1" * 30
    cases += [("eos", eos), ("eos pad2", eos + "11"), ("eos 5", eos + e), ("5 eos 5 pad", e + eos + e),
              ("text eos pad", codes[_sym_of_len(codes, 6)] + e + eos + "1" * 5)]
    for k in (8, 9, 13, 14, 16, 24, 26, 29, 31, 32, 40):  # ones that are too long for padding, short of and past EOS
        cases.append(("ones%d" % k, e + "1" * k))
    for L in (6, 7, 8, 10, 13, 14, 15, 19, 23, 28, 30):  # a final code cut short by the string's end
        s = by_len[L] if L > 13 else _sym_of_len(codes, L)
        cuts = sorted({c for c in (3, 5, 6, 7, 8, 13, L // 2, L - 1) if 0 < c < L})
        for c in cuts:
            cases.append(("cut %d of %d" % (c, L), e + codes[s][:c]))
            if "0" in codes[s][:c] and c >= 5:  # (behind nothing: the string's first code is the cut one)
                cases.append(("only cut %d of %d" % (c, L), codes[s][:c]))
    return cases


def special_strings(oracle, codes, seed):
    """every tail behind no text and behind 30..60 B of text (the bulk loop runs), strings of 1..8 Huffman bytes,
    empty strings -> [bytes]"""
    rng = np.random.default_rng(seed)
    fill = _fillers(codes)
    out = []
    for label, tail in tail_cases(codes):
        for body_bytes in (0, int(rng.integers(30, 61))):
            body = "".join(codes[b] for b in H.text(rng, (8 * body_bytes) // 6)) if body_bytes else ""
            bits = body + fill[(-len(body) - len(tail)) % 8] + tail
            assert len(bits) % 8 == 0, label
            out.append(int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b"")
    for L in range(1, 9):  # never in the bulk loop: whole, with its last bit cleared, and with a byte cut off
        h = H.huffman_of_len(oracle, rng, L)
        out += [h, h[:-1] + bytes([h[-1] & 0xFE]), H.huffman_of_len(oracle, rng, L + 1)[:L]]
    out += [b"", b""]
    return out


@pytest.fixture(scope="module")
def tail_batches(oracle_codec):
    """[(strings, name flags)]: the specials, SPECIALS_PER_BATCH a batch, shuffled among ORDINARY_PER_BATCH ordinary
    strings (tests/bounds_harness.py's short batch); the last batch is filled up to 128 strings with those"""
    codes = _codes()
    sp = special_strings(oracle_codec, codes, 31)
    rng = np.random.default_rng(32)
    batches = []
    for k, b0 in enumerate(range(0, len(sp), SPECIALS_PER_BATCH)):
        part = sp[b0:b0 + SPECIALS_PER_BATCH]
        ordinary, _ = H.huffman_batch(oracle_codec, "short", max(ORDINARY_PER_BATCH, 128 - len(part)), 300 + k)
        strings = part + ordinary
        strings = [strings[i] for i in rng.permutation(len(strings))]
        assert 128 <= len(strings) <= 192
        assert sum(map(len, strings)) <= 40 * len(strings)  # (the natural route is the short stage)
        batches.append((strings, rng.random(len(strings)) < 0.5))
    assert len(batches) >= 2
    return batches


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def test_tail_cases_cover_the_list():
    """the generator itself (no GPU work): every kind of tail is there, and every string is whole bytes"""
    labels = [c[0] for c in tail_cases(_codes())]
    for want in ("5x5 pad0", "5x5 pad7", "text pad3", "5 long14 5", "long30 last", "pad5 zero@0", "pad7 zero@6", "eos",
                 "cut 6 of 8", "cut 13 of 14", "only cut 5 of 6", "ones26"):
        assert want in labels, want
    assert len(labels) == len(set(labels))


@pytest.mark.gpu
def test_slot(torch_cuda, oracle_codec, tail_batches):
    """hhuff_decode_batch, contiguous layout at two alignments, both staged kernels"""
    reached = set()
    for k, (strings, names) in enumerate(tail_batches):
        sweep(torch_cuda, oracle_codec, "decode", strings, names, (len(strings),), ROUTES, "decode tail batch %d" % k,
              layouts=[("contiguous", 0, True), ("contiguous", 5, True)], reached=reached, defers=(DEFAULT_DEFER,))
    assert {"natural", "mean<=40", "mean>=41/staged"} <= reached, reached


@pytest.mark.gpu
def test_explicit_and_pairs(torch_cuda, oracle_codec, tail_batches):
    """the same lane decoder behind the pairs and the explicit layouts (strings in any order, own destinations)"""
    for k, (strings, names) in enumerate(tail_batches):
        sweep(torch_cuda, oracle_codec, "decode", strings, names, (len(strings),), ROUTES[:1],
              "decode tail batch %d" % k, layouts=[("pairs", 5, True), ("explicit", 3, True)])


@pytest.mark.gpu
def test_packed(torch_cuda, oracle_codec, tail_batches):
    """hhuff_decode_batch_packed (the packed instances of both staged kernels share the lane decoder)"""
    from h2o_amd import codec

    torch = torch_cuda
    for k, (strings, names) in enumerate(tail_batches):
        n = len(strings)
        for off0 in (0, 7):
            for fill, sentinel in H.RUNS:
                base = H.place_input(strings, "contiguous", off0, fill)
                nb = H.name_bits(names, fill)
                for rname, size, _ in route_sizes(PACKED_ROUTES, n, base["end"]):
                    inp = H.place_input(strings, "contiguous", off0, fill, in_size=size)
                    _, slot = H.oracle_run(oracle_codec, "decode", inp, sentinel, names=nb)
                    exp, mask = _packed_expected("decode", inp, slot)
                    _, data = H.to_device(torch, inp["whole"])
                    bufs = {"out": H.guarded(torch, exp["out"].size, sentinel),
                            "out_off": H.guarded(torch, 4 * (n + 1), sentinel),
                            "out_len": H.guarded(torch, 4 * n, sentinel), "status": H.guarded(torch, n, sentinel)}
                    with edge_defer(DEFAULT_DEFER):
                        codec.decode_batch_packed(data, _dev(torch, inp["in_off"]), n, is_name_bits=_dev(torch, nb),
                                                  out=bufs["out"][1], out_off=bufs["out_off"][1].view(torch.int32),
                                                  out_len=bufs["out_len"][1].view(torch.int32),
                                                  status=bufs["status"][1], in_size=size)
                        torch.cuda.synchronize()
                    res = {key: w.cpu().numpy() for key, (w, _) in bufs.items()}
                    H.check(res, exp, mask, sentinel, label="packed decode tail batch %d in_off0=%d route=%s fill=%#x"
                            % (k, off0, rname, fill))
