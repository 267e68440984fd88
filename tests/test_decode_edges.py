"""The stream, split and per-string decoders of h2o_hpack_decode_huffman on the edge corpora of
tests/decode_edges.py, against the reference decoder tests/huff_ref.py (not the oracle: test_decode_edges_host.py
shows that both agree on every corpus string).

Batches go through hhuff_decode_batch on exact-size guarded buffers (tests/bounds_harness.py): lengths and
statuses of every string, the bytes of every string that decodes, and nothing written outside the call's
footprint.  Per-string calls go through codec.decode_huffman, in this process on the default service path and in
child processes for the other paths.  Every assertion message names the string's label, route, layout, alignment
and n."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bounds_harness as H
import decode_edges as E
from test_batch_bounds import STREAM, _dev, _packed_expected, gpu_run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# stream routes: the stream verdict forced at a mean of 41..128 (the largest in_size of mean 128), the natural route
# from 129 up (the smallest in_size of mean 129)
STREAM_ROUTES = (("mean<=128/stream", lambda n: 129 * n - 1, STREAM), ("mean>=129", lambda n: 129 * n, None))
LAYOUTS = [("contiguous", o) for o in (0, 1, 2, 3)] + [("pairs", 5), ("explicit", 3)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def stream(oracle_codec):
    return E.corpus("stream")


@pytest.fixture(scope="module")
def split(oracle_codec):
    return E.corpus("split")


def expected(batch, names, inp, sentinel):
    """huff_ref's result in the call's layout: -> (the dict H.check() compares with, [per-string results])"""
    n = inp["n"]
    size = inp["out_size"] if inp["out_off"] is not None else H.implicit_out_size("decode", inp)
    starts = H.out_starts("decode", inp)
    exp = {"out": np.full(size, sentinel, np.uint8), "out_len": np.zeros(n, np.uint32), "status": np.zeros(n, np.uint8)}
    refs = []
    for i, c in enumerate(batch):
        dec, st = E.ref(c.data, bool(names[i]))
        refs.append((dec, st))
        exp["status"][i] = st
        exp["out_len"][i] = H.FAIL if dec is None else len(dec)
        if dec:
            exp["out"][starts[i]:starts[i] + len(dec)] = np.frombuffer(dec, np.uint8)
    return exp, refs


def compare(res, exp, refs, batch, names, starts, mask, sentinel, ctx):
    """string by string, so that a failure names its string; then the harness' check (footprint, guards)"""
    g = H.GUARD
    got_len = res["out_len"][g:res["out_len"].size - g].view(np.uint32)
    got_st = res["status"][g:res["status"].size - g]
    out = res["out"][g:res["out"].size - g]
    for i in np.nonzero((got_len != exp["out_len"]) | (got_st != exp["status"]))[0]:
        raise AssertionError("%s [%d, %s]: out_len %#x status %#x, huff_ref %#x %#x -- %s" % (
            batch[i].label, i, "name" if names[i] else "value", got_len[i], got_st[i], exp["out_len"][i],
            exp["status"][i], ctx))
    for i, (dec, _) in enumerate(refs):
        if dec and out[starts[i]:starts[i] + len(dec)].tobytes() != dec:
            got = out[starts[i]:starts[i] + len(dec)].tobytes()
            k = next(j for j in range(len(dec)) if got[j] != dec[j])
            raise AssertionError("%s [%d]: byte %d of %d is %#x, huff_ref %#x -- %s" % (
                batch[i].label, i, k, len(dec), got[k], dec[k], ctx))
    H.check(res, exp, mask, sentinel, starts=starts, label=ctx)


def explicit_destinations(inp, batch):
    """the explicit layout's out_off with every string that asks for one (facts "dst16") at that residue mod 16;
    regions of floor(8 len / 5) bytes in the harness' reversed order, gaps of 0..15 bytes"""
    n = inp["n"]
    reg = H.REGION["decode"](inp["lens"])
    dst = np.zeros(n, np.int64)
    pos = 0
    for i in reversed(range(n)):
        want = batch[i].facts.get("dst16")
        if want is not None:
            pos += (want - pos) % 16
        dst[i] = pos
        pos += int(reg[i])
    inp["out_off"] = H._poisoned(dst, lambda j: 0)
    inp["out_size"] = pos
    return inp


def run_batch(torch, batch, label, routes, layouts=LAYOUTS, flip_names=(False, True), reached=None):
    """one batch through hhuff_decode_batch: every layout x route x both runs (fill / sentinel) x the cases' name
    flags and their inverse"""
    from h2o_amd import codec

    n = len(batch)
    strings = [c.data for c in batch]
    end0 = sum(map(len, strings))
    for flip in flip_names:
        names = np.array([c.is_name != flip for c in batch])
        for layout, off0 in layouts:
            for fill, sentinel in H.RUNS:
                base = H.place_input(strings, layout, off0, fill, op="decode", seed=n)
                for rname, size_of, prices in routes:
                    size = size_of(n) if size_of else base["end"]
                    if size < base["end"]:
                        continue
                    inp = H.place_input(strings, layout, off0, fill, in_size=size, op="decode", seed=n)
                    if layout == "explicit":
                        inp = explicit_destinations(inp, batch)
                    nb = H.name_bits(names, fill)
                    exp, refs = expected(batch, names, inp, sentinel)
                    ctx = "%s route=%s layout=%s in_off0=%d n=%d in_size=%d fill=%#x names %s" % (
                        label, rname, layout, off0, n, size, fill, "inverted" if flip else "as built")
                    try:
                        if prices:
                            codec.set_decode_prices(prices, 0)
                        res = gpu_run(torch, "decode", inp, sentinel, names=nb)
                    finally:
                        if prices:
                            codec.set_decode_prices(None, 0)
                    compare(res, exp, refs, batch, names, H.out_starts("decode", inp), H.mask_of("decode", inp),
                            sentinel, ctx)
                    if reached is not None:
                        reached.add(rname)
    assert end0 > 0


def stream_batch(cases, seed):
    """the cases among short strings (so that the batch's mean allows the forced route), each at the input offset
    its facts ask for"""
    return E.arrange(E.dilute(cases, 100, seed), seed)


# ------------------------------------------------------------------------------------------------
# the stream kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [0, 1, 2])
def test_stream_window_edge(torch_cuda, stream, window):
    """strings that end around kLimW / kFinal in their first, second and third window, at every input alignment
    (contiguous in_off0 0..3 moves every string through all four)"""
    batch = stream_batch([c for c in stream["window_edge"] if c.facts["window"] == window], 40 + window)
    reached = set()
    run_batch(torch_cuda, batch, "stream window edge w%d" % window, STREAM_ROUTES, reached=reached)
    assert reached == {"mean<=128/stream", "mean>=129"}


@pytest.mark.parametrize("window", [0, 1])
def test_stream_long_codes_and_eos(torch_cuda, stream, window):
    """long codes across the bulk limit (with text behind them, and cut by the string's end: the lane parks), EOS at
    the limit"""
    cases = [c for c in stream["long_codes"] + stream["eos"] if c.facts["window"] == window]
    reached = set()
    run_batch(torch_cuda, stream_batch(cases, 50 + window), "stream long codes w%d" % window, STREAM_ROUTES,
              flip_names=(False,), reached=reached)
    assert reached == {"mean<=128/stream", "mean>=129"}


def test_stream_soft_bits(torch_cuda, stream):
    """first / last byte and invalid-character flags that come from different rounds"""
    reached = set()
    run_batch(torch_cuda, stream_batch(stream["soft"], 60), "stream soft bits", STREAM_ROUTES, reached=reached)
    assert reached == {"mean<=128/stream", "mean>=129"}


def test_stream_flush(torch_cuda, stream):
    """output lengths around the 16-B segments at destination residues 0, 1, 5, 15 (explicit) and 0, 1, 4 / 6, 14
    (contiguous), the carried partial segment, the whole last chunk under implicit slots"""
    batch = E.arrange(stream["flush"], 70)
    reached = set()
    # (explicit at in_off0 0 as well: the carry cases are built for strings at s % 4 == 0)
    run_batch(torch_cuda, batch, "stream flush", STREAM_ROUTES + (("mean>=41/stream", lambda n: 41 * n, STREAM),),
              layouts=LAYOUTS + [("explicit", 0)], reached=reached)
    assert reached == {"mean>=41/stream", "mean<=128/stream", "mean>=129"}


def test_stream_claims(torch_cuda, stream):
    """n around every claim size, at the in_size that makes stream_claim take 256, 192, 128 and 64 strings a claim
    (mean 90 and 120 with the stream verdict forced, 180 and 181 on the natural route)"""
    pool = stream_batch(stream["flush"] + [c for c in stream["window_edge"] if c.facts["window"] == 0], 80)
    for n in (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257):
        batch = pool[:n]
        assert sum(len(c.data) for c in batch) <= 90 * n
        routes = tuple(("claim%d" % claim, lambda n, m=m: m * n, prices)
                       for m, claim, prices in ((90, 256, STREAM), (120, 192, STREAM), (180, 128, None), (181, 64, None)))
        for (rname, size_of, _), claim in zip(routes, (256, 192, 128, 64)):
            assert E.stream_claim(size_of(n), n) == claim
        run_batch(torch_cuda, batch, "stream claims", routes, layouts=[("contiguous", 1), ("pairs", 5)],
                  flip_names=(False,))


def test_stream_mixed_with_split_strings(torch_cuda, stream, split):
    """a batch of mean >= 128 B with two strings of 4096 B and more: split_push takes them out of a wave that
    goes on with its other lanes"""
    cases = [c for c in stream["window_edge"] if c.facts["window"] == 2][::5] + stream["soft"][::4]
    long_ones = [split["wave_many", 4096][3], split["wave_many", 5000][-9]]
    batch = cases[:20] + long_ones[:1] + cases[20:] + long_ones[1:] + cases[:3]
    n = len(batch)
    assert n > 16 and sum(len(c.data) for c in batch) >= 129 * n
    run_batch(torch_cuda, batch, "stream mixed with split", (("natural", None, None),),
              layouts=[("contiguous", 0), ("contiguous", 3), ("explicit", 3)], flip_names=(False,))


def test_stream_packed(torch_cuda, stream):
    """hhuff_decode_batch_packed over the window-edge and soft-bit classes"""
    from h2o_amd import codec

    torch = torch_cuda
    batch = stream_batch(stream["window_edge"][::2] + stream["soft"], 90)
    n = len(batch)
    strings = [c.data for c in batch]
    names = np.array([c.is_name for c in batch])
    for off0 in (0, 3):
        for fill, sentinel in H.RUNS:
            for rname, size_of, prices in STREAM_ROUTES:
                inp = H.place_input(strings, "contiguous", off0, fill, in_size=size_of(n))
                nb = H.name_bits(names, fill)
                slot, refs = expected(batch, names, inp, sentinel)
                exp, mask = _packed_expected("decode", inp, slot)
                _, data = H.to_device(torch, inp["whole"])
                bufs = {"out": H.guarded(torch, exp["out"].size, sentinel),
                        "out_off": H.guarded(torch, 4 * (n + 1), sentinel),
                        "out_len": H.guarded(torch, 4 * n, sentinel), "status": H.guarded(torch, n, sentinel)}
                ctx = "stream packed route=%s layout=contiguous in_off0=%d n=%d fill=%#x" % (rname, off0, n, fill)
                try:
                    if prices:
                        codec.set_decode_prices(prices, 0)
                    codec.decode_batch_packed(data, _dev(torch, inp["in_off"]), n, is_name_bits=_dev(torch, nb),
                                              out=bufs["out"][1], out_off=bufs["out_off"][1].view(torch.int32),
                                              out_len=bufs["out_len"][1].view(torch.int32), status=bufs["status"][1],
                                              in_size=inp["in_size"])
                    torch.cuda.synchronize()
                finally:
                    if prices:
                        codec.set_decode_prices(None, 0)
                res = {k: w.cpu().numpy() for k, (w, _) in bufs.items()}
                compare(res, exp, refs, batch, names, exp["out_off"][:n].astype(np.int64), mask, sentinel, ctx)


# ------------------------------------------------------------------------------------------------
# the split decoders
# ------------------------------------------------------------------------------------------------
def _split_run(torch, cases, per_batch, label, layouts):
    for b0 in range(0, len(cases), per_batch):
        batch = cases[b0:b0 + per_batch]
        if len(batch) < per_batch:  # (the last batch: filled up from the front, so that n stays what the form needs)
            batch = batch + cases[:per_batch - len(batch)]
        run_batch(torch, batch, "%s batch %d" % (label, b0 // per_batch), (("natural", None, None),), layouts=layouts,
                  flip_names=(False, True) if b0 == 0 else (False,))


@pytest.mark.parametrize("nbytes", E.SPLIT_WAVE_FEW)
def test_split_wave_few(torch_cuda, split, nbytes):
    """split_decode_wave in batches of 16 strings: every segment size and lead"""
    assert nbytes >= E.SPLIT_MIN_FEW and nbytes < E.SPLIT_BIG_FEW
    _split_run(torch_cuda, split["wave_few", nbytes], E.SPLIT_FEW_N, "split wave %d B" % nbytes,
               [("contiguous", 0), ("contiguous", 1), ("explicit", 3)])


@pytest.mark.parametrize("nbytes", E.SPLIT_WAVE_MANY)
def test_split_wave_many(torch_cuda, split, nbytes):
    """split_decode_wave in batches of 17 strings at a mean of 128 B and more: segments of 512 and 640 bits"""
    assert E.SPLIT_MIN <= nbytes < E.SPLIT_BIG
    _split_run(torch_cuda, split["wave_many", nbytes], E.SPLIT_FEW_N + 1, "split wave (17) %d B" % nbytes,
               [("contiguous", 0), ("contiguous", 3), ("pairs", 5)])


@pytest.mark.parametrize("nbytes", E.SPLIT_BLOCK_FEW)
def test_split_block_few(torch_cuda, split, nbytes):
    """split_decode_block<16> in batches of 16 strings: segments of 128 bits, the agreement crossing waves, lanes
    and waves past the string"""
    assert nbytes >= E.SPLIT_BIG_FEW
    _split_run(torch_cuda, split["block_few", nbytes], E.SPLIT_FEW_N, "split block %d B" % nbytes,
               [("contiguous", 0), ("contiguous", 1), ("explicit", 3)])


# ------------------------------------------------------------------------------------------------
# per-string calls
# ------------------------------------------------------------------------------------------------
_CHILD = r"""
import os, sys
sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import torch  # noqa: F401  (one HIP runtime: torch's)
from h2o_amd import codec
from oracle import oracle as O
import decode_edges as E
name = sys.argv[1]
cases = E.corpus(name, O.oracle())
if isinstance(cases, dict):
    cases = [c for cs in cases.values() for c in cs]
env = " ".join("%s=%s" % (k, os.environ[k]) for k in ("HHUFF_NO_SERVICE", "HHUFF_SVC_NC") if k in os.environ)
bad = 0
for c in cases:
    for nm in (c.is_name, not c.is_name):
        dec, st = E.ref(c.data, nm)
        got = codec.decode_huffman(c.data, nm)
        if got != (dec, 0 if dec is None else st):
            bad += 1
            if bad <= 10:
                print("MISMATCH %s [%s, %d B]: %r status %r, huff_ref %r %r -- per-string call, %s" % (
                    c.label, "name" if nm else "value", len(c.data), None if got[0] is None else len(got[0]), got[1],
                    None if dec is None else len(dec), st, env or "default path"))
print("ok %d" % (2 * len(cases)) if not bad else "failed %d" % bad)
"""


def _child(corpus, env):
    """the corpus through codec.decode_huffman in a fresh process.  A child that ends on a signal or runs into its
    time limit fails the test here; nothing further is started"""
    r = subprocess.run([sys.executable, "-c", _CHILD, corpus], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and r.stdout.startswith("ok"), "%s %s: exit %d\n%s%s" % (
        corpus, env, r.returncode, r.stdout[-3000:], r.stderr[-3000:])


def test_per_string_service(torch_cuda, oracle_codec):
    """corpus (c) on the default path of this process: the service's jump-table wave decoder up to 768 B,
    one_string_kernel for the 769-B string"""
    from h2o_amd import codec

    for c in E.corpus("per_string", oracle_codec):
        for nm in (c.is_name, not c.is_name):
            dec, st = E.ref(c.data, nm)
            got = codec.decode_huffman(c.data, nm)
            assert got == (dec, 0 if dec is None else st), "%s [%s, %d B]: status %r, huff_ref %r -- per-string call, " \
                "default path, layout and n: one string a call" % (c.label, "name" if nm else "value", len(c.data),
                                                                  got[1], st)


@pytest.mark.parametrize("env", [{"HHUFF_SVC_NC": "1"}, {"HHUFF_SVC_NC": "2"}, {"HHUFF_SVC_NC": "4"},
                                 {"HHUFF_NO_SERVICE": "1"}], ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_per_string_other_paths(torch_cuda, oracle_codec, env):
    """corpus (c) in a child process a path: one and two candidates a lane, four columns, the launch-per-string path"""
    _child("per_string", env)


def test_split_block_one_string(torch_cuda, oracle_codec):
    """split_decode_block<4> in one_string_kernel (HHUFF_NO_SERVICE=1): 769, 1024, 4096 and 32768 B"""
    _child("one_string", {"HHUFF_NO_SERVICE": "1"})
