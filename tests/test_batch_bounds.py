"""The batch kernels at exact buffer sizes, tile edges and on every route (tests/bounds_harness.py).

Every call gets `out`, `out_len` and `status` of exactly the size include/hhuff.h documents, between sentinel
guards; the input's unused bytes hold a fill pattern; the result must equal the oracle's and nothing outside the
call's footprint may change.  Routes are steered by in_size alone (bytes behind the strings are readable, so a
larger in_size is legal): the same strings go through every kernel their real mean length allows, at the dispatch
boundaries exactly, with the shared 16-B chunks stored in the kernels and deferred to edge_fix_kernel.

Each test loops over n, layout and route and names the failing case in the assertion message."""
import ctypes

import numpy as np
import pytest

import bounds_harness as H

pytestmark = pytest.mark.gpu

NS = (1, 2, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500)
NMAX = 2500
STAGED = (0.0, 0.0, 1e5, 1e5)  # hhuff_set_decode_prices: the staged kernel costs nothing -> verdict staged
STREAM = (1e5, 1e5, 0.0, 0.0)
DEFAULT_DEFER = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def batches(oracle_codec):
    """the seeded batches, built once at their largest n (a case takes the first n strings)"""
    b = {}
    for k, kind in enumerate(("short", "mixed", "long")):
        b["huff", kind] = H.huffman_batch(oracle_codec, kind, NMAX, 100 + k)
        b["plain", kind] = H.plain_batch(kind, 4096 if kind == "short" else NMAX, 200 + k)
    return b


def _dev(torch, a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _out_size(op, inp):
    return inp["out_size"] if inp["out_off"] is not None else H.implicit_out_size(op, inp)


def gpu_run(torch, op, inp, sentinel, names=None, prefix_bits=7, first=None, raw=None, with_status=True):
    """the batch call of `op` through h2o_amd.codec on exact-size guarded device arrays -> result for H.check()"""
    from h2o_amd import codec

    n = inp["n"]
    _, data = H.to_device(torch, inp["whole"])
    bufs = {"out": H.guarded(torch, _out_size(op, inp), sentinel), "out_len": H.guarded(torch, 4 * n, sentinel)}
    if op != "flatten" and with_status:
        bufs["status"] = H.guarded(torch, n, sentinel)
    out, out_len = bufs["out"][1], bufs["out_len"][1].view(torch.int32)
    assert out.numel() > 0 and data.numel() > 0
    kw = dict(in_len=_dev(torch, inp["in_len"]), out=out, out_off=_dev(torch, inp["out_off"]), out_len=out_len,
              in_size=inp["in_size"])
    in_off = _dev(torch, inp["in_off"])
    if op == "decode":
        codec.decode_batch(data, in_off, n, is_name_bits=_dev(torch, names), status=bufs["status"][1], **kw)
    elif op == "encode" and with_status:
        codec.encode_batch(data, in_off, n, status=bufs["status"][1], **kw)
    elif op == "encode":  # status == NULL: past codec.py (it always allocates one), the C ABI itself
        dp = codec._dp
        rc = codec.lib().hhuff_encode_batch(dp(data), inp["in_size"], dp(in_off), dp(kw["in_len"]), n, dp(out),
                                            dp(kw["out_off"]), dp(out_len), None,
                                            torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    else:
        codec.flatten_batch(data, in_off, n, prefix_bits, first_bytes=_dev(torch, first), raw_bits=_dev(torch, raw),
                            **kw)
    torch.cuda.synchronize()
    return {k: w.cpu().numpy() for k, (w, _) in bufs.items()}


class edge_defer:
    """hhuff_set_edge_defer_min for a block, restored afterwards"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from h2o_amd import codec

        self.prev = codec.set_edge_defer_min(self.value)

    def __exit__(self, *exc):
        from h2o_amd import codec

        codec.set_edge_defer_min(self.prev)


def placements(op):
    """(layout, in_off0, permute): the contiguous layout with its first string at every alignment class, pairs,
    explicit destinations"""
    return [("contiguous", o, True) for o in (0, 1, 7, 13)] + [("pairs", 5, op != "flatten"), ("explicit", 3, True)]


def route_sizes(routes, n, end):
    """(route name, in_size, extra) of the routes the batch's real size allows: a route is a mean in_size / n at a
    dispatch boundary -- ("le", m): the largest in_size whose mean is m; ("ge", m): the smallest"""
    out = [("natural", end, None)]
    for kind, m, extra in routes:
        size = (m + 1) * n - 1 if kind == "le" else m * n
        if size >= end and size > 0:
            out.append(("mean%s%d%s" % ("<=" if kind == "le" else ">=", m, extra[0] if extra else ""), size, extra))
    return out


def sweep(torch, oracle, op, strings, names, ns, routes, label, layouts=None, prefix_bits=7, reached=None,
          defers=(DEFAULT_DEFER, 0)):
    """every n x placement x run x route (x edge-defer setting for the contiguous layout) of one batch"""
    from h2o_amd import codec

    for n in ns:
        sub = strings[:n]
        for layout, off0, permute in layouts or placements(op):
            for fill, sentinel in H.RUNS:
                base = H.place_input(sub, layout, off0, fill, op=op, seed=n, permute=permute)
                kw = {}
                if op == "decode":
                    kw["names"] = H.name_bits(names[:n], fill)
                if op == "flatten":
                    rng = np.random.default_rng(n)
                    kw = dict(prefix_bits=prefix_bits, first=rng.integers(0, 256, n + H.EXTRA).astype(np.uint8),
                              raw=H.name_bits(rng.random(n) < 0.15, fill))
                for rname, size, extra in route_sizes(routes if layout != "explicit" or op != "flatten" else (), n,
                                                      base["end"]):
                    inp = base if size == base["in_size"] else H.place_input(sub, layout, off0, fill, in_size=size,
                                                                             op=op, seed=n, permute=permute)
                    _, exp = H.oracle_run(oracle, op, inp, sentinel, **kw)
                    mask, starts = H.mask_of(op, inp), H.out_starts(op, inp)
                    if reached is not None:
                        reached.add(rname)
                    for defer in defers if layout == "contiguous" else (DEFAULT_DEFER,):
                        case = "%s n=%d %s in_off0=%d route=%s in_size=%d defer_min=%#x fill=%#x" % (
                            label, n, layout, off0, rname, size, defer, fill)
                        try:
                            if extra:
                                codec.set_decode_prices(extra[1], 0)
                            with edge_defer(defer):
                                res = gpu_run(torch, op, inp, sentinel, **kw)
                        finally:
                            if extra:
                                codec.set_decode_prices(None, 0)
                        H.check(res, exp, mask, sentinel, starts=starts, label=case)


# mean 40 / 41: staged short | mixed;  128 / 129: mixed | stream;  in (40, 128] both verdicts of the price choice
DECODE_ROUTES = (("le", 40, None), ("ge", 41, ("/staged", STAGED)), ("ge", 41, ("/stream", STREAM)),
                 ("le", 128, ("/staged", STAGED)), ("le", 128, ("/stream", STREAM)), ("ge", 129, None))
# contiguous: 52 | 53 sorted | proportional lanes (K = 32); 120 / 121 K = 16; 300 K = 8; 2560 / 2561 K = 1
ENCODE_ROUTES = (("le", 52, None), ("ge", 53, None), ("le", 120, None), ("ge", 121, None), ("ge", 300, None),
                 ("le", 2560, None), ("ge", 2561, None))
# pairs / explicit: 52 | 53 encode_staged<16,3584> | <8,8192>;  120 | 121 <8,8192> | encode_direct
ENCODE_ROUTES_PAIRS = ENCODE_ROUTES[:4]


@pytest.mark.parametrize("kind", ["short", "mixed", "long"])
def test_decode(torch_cuda, oracle_codec, batches, kind):
    strings, names = batches["huff", kind]
    reached = set()
    sweep(torch_cuda, oracle_codec, "decode", strings, names, NS, DECODE_ROUTES, "decode " + kind, reached=reached)
    want = {"short": {"natural", "mean<=40", "mean>=41/staged", "mean>=41/stream", "mean<=128/staged",
                      "mean<=128/stream", "mean>=129"},
            "mixed": {"natural", "mean<=128/staged", "mean<=128/stream", "mean>=129"},
            "long": {"natural"}}[kind]
    assert want <= reached, want - reached


def test_decode_split_thresholds(torch_cuda, oracle_codec, batches):
    """the split lists' thresholds at their exact Huffman lengths: 512 (one wave) and 4096 (a block) in batches of
    at most 16 strings, 4096 and 65536 in larger ones with a mean of 128 B and more"""
    rng = np.random.default_rng(77)
    hl = lambda L: H.huffman_of_len(oracle_codec, rng, L)  # noqa: E731
    short = batches["huff", "short"][0]
    a, b = [hl(L) for L in (511, 512, 513)], [hl(L) for L in (4095, 4096, 4097)]
    big = [hl(L) for L in (65535, 65536, 65537)]
    bad = bytearray(hl(4096))
    bad[2000] ^= 0x10  # a long string that no longer is the text it was (a list entry that may fail)
    cases = {"3x51x": a, "3x409x": b,
             "16": short[:3] + a + short[3:9] + b + [short[9]],
             "16bad": short[:2] + a + short[3:9] + b + [bytes(bad), hl(700)],
             "17": [short[1]] + b + short[2:8] + big + short[8:12]}
    for name, strings in cases.items():
        n = len(strings)
        assert n == {"3x51x": 3, "3x409x": 3, "16": 16, "16bad": 16, "17": 17}[name]
        if n == 17:
            assert sum(map(len, strings)) // n >= 128
        sweep(torch_cuda, oracle_codec, "decode", strings, rng.random(n) < 0.5, (n,), (("ge", 129, None),),
              "decode split " + name)


@pytest.mark.parametrize("kind", ["short", "mixed", "long"])
def test_encode_contiguous(torch_cuda, oracle_codec, batches, kind):
    """the sorted encoder and proportional lanes at every tile size K"""
    reached = set()
    sweep(torch_cuda, oracle_codec, "encode", batches["plain", kind], None, NS, ENCODE_ROUTES, "encode " + kind,
          layouts=placements("encode")[:4], reached=reached)
    want = {"short": {"natural"} | {"mean%s%d" % r[:2] for r in (("<=", 52), (">=", 53), ("<=", 120), (">=", 121),
                                                                  (">=", 300), ("<=", 2560), (">=", 2561))},
            "mixed": {"natural", "mean>=300", "mean<=2560", "mean>=2561"},
            "long": {"natural", "mean<=2560", "mean>=2561"}}[kind]
    assert want <= reached, want - reached


@pytest.mark.parametrize("kind", ["short", "mixed", "long"])
def test_encode_pairs_and_explicit(torch_cuda, oracle_codec, batches, kind):
    """both encode_staged_kernel stages and encode_direct_kernel"""
    reached = set()
    sweep(torch_cuda, oracle_codec, "encode", batches["plain", kind], None, NS, ENCODE_ROUTES_PAIRS, "encode " + kind,
          layouts=placements("encode")[4:], reached=reached)
    if kind == "short":
        assert {"natural", "mean<=52", "mean>=53", "mean<=120", "mean>=121"} <= reached, reached


def test_encode_and_flatten_planned_tiles(torch_cuda, oracle_codec, batches):
    """n >= 4096 at a mean below 320 B: encode_plan_kernel picks the proportional-lane tile size (n = 4095 does
    not sample; both at the means that give K = 32 and K = 16)"""
    strings = batches["plain", "short"]
    routes = (("ge", 53, None), ("le", 120, None), ("ge", 121, None), ("ge", 300, None))
    lay = [("contiguous", 0, True), ("contiguous", 13, True)]
    sweep(torch_cuda, oracle_codec, "encode", strings, None, (4095, 4096), routes, "encode planned", layouts=lay)
    sweep(torch_cuda, oracle_codec, "flatten", strings, None, (4095, 4096), routes[:2], "flatten planned",
          layouts=lay[1:], prefix_bits=5)


@pytest.mark.parametrize("kind,prefix_bits", [("short", 3), ("short", 5), ("short", 7), ("mixed", 5), ("long", 7)])
def test_flatten(torch_cuda, oracle_codec, batches, kind, prefix_bits):
    """contiguous (flatten_pl_kernel, its tile size steered like the encoder's) and pairs / explicit
    (flatten_direct_kernel); first_bytes and raw_bits set"""
    routes = (("ge", 53, None), ("ge", 300, None), ("le", 2560, None))
    sweep(torch_cuda, oracle_codec, "flatten", batches["plain", kind], None, NS, routes,
          "flatten %s p=%d" % (kind, prefix_bits), prefix_bits=prefix_bits)


@pytest.mark.parametrize("raw_at", [20, 21])
def test_flatten_tile_past_the_stage(torch_cuda, oracle_codec, batches, raw_at):
    """flatten_pl_kernel's tile whose span exceeds its 3,584-B stage: every lane frames its string from global
    memory.  40 strings at a mean that gives tiles of 16: the second tile holds a 4,000-B text (index 20) behind an
    empty string and before a short text; the raw flag sits on the long string in one run and on its short
    neighbour in the other, so the tile frames a raw, a Huffman and an empty string both times"""
    rng = np.random.default_rng(5)
    strings = list(batches["plain", "short"][:40])
    strings[19], strings[20], strings[21] = b"", H.text(rng, 4000), H.text(rng, 33)
    n = len(strings)
    flags = np.zeros(n, bool)
    flags[raw_at] = True
    for fill, sentinel in H.RUNS:
        inp = H.place_input(strings, "contiguous", 13, fill, op="flatten")
        assert 117 <= inp["in_size"] // n <= 160  # kPlFill / mean in 16..21: 16 strings a tile, no sampling (n < 4096)
        assert inp["in_off"][32] - inp["in_off"][16] > 3584
        kw = dict(prefix_bits=7, first=rng.integers(1, 256, n + H.EXTRA).astype(np.uint8), raw=H.name_bits(flags, fill))
        _, exp = H.oracle_run(oracle_codec, "flatten", inp, sentinel, **kw)
        assert (exp["out_len"][20] < 4000) == (raw_at != 20) and exp["out_len"][19] == 1  # Huffman unless raw
        for defer in (DEFAULT_DEFER, 0):
            with edge_defer(defer):
                res = gpu_run(torch_cuda, "flatten", inp, sentinel, **kw)
            H.check(res, exp, H.mask_of("flatten", inp), sentinel, starts=H.out_starts("flatten", inp),
                    label="flatten past the stage raw_at=%d defer_min=%#x fill=%#x" % (raw_at, defer, fill))


@pytest.mark.parametrize("op", ["decode", "encode", "flatten"])
def test_last_string_at_every_alignment(torch_cuda, oracle_codec, batches, op):
    """In the contiguous layout every region borders the next one, so a store that runs past a region lands in a
    neighbour's footprint -- except behind the last string, where the fill and the guard begin.  One and two
    strings (every one of the batch's first 40 as the last) at 16 input offsets: the last region ends at every
    offset of a 16-B chunk, and the last input byte at every offset of its chunk, on every route"""
    strings, names = batches["huff", "short"] if op == "decode" else (batches["plain", "short"], None)
    routes = {"decode": (("le", 40, None), ("le", 128, ("/staged", STAGED)), ("le", 128, ("/stream", STREAM)),
                         ("ge", 129, None)),
              "encode": (("le", 52, None), ("ge", 53, None), ("ge", 2561, None)),
              "flatten": (("ge", 300, None),)}[op]
    for k in range(40):
        sub = strings[k:k + 1] if k % 2 else [strings[k + 40], strings[k]]
        if not sum(map(len, sub)):
            continue
        nm = None if names is None else (names[k:k + 1] if k % 2 else names[[k + 40, k]])
        lay = [("contiguous", o, True) for o in range(k % 2, 16, 2)]
        sweep(torch_cuda, oracle_codec, op, sub, nm, (len(sub),), routes, "%s last string %d" % (op, k), layouts=lay,
              prefix_bits=(3, 5, 7)[k % 3], defers=(DEFAULT_DEFER,))


@pytest.mark.parametrize("route", ["sorted", "lanes", "staged16", "staged8", "direct"])
def test_encode_without_status(torch_cuda, oracle_codec, batches, route):
    """hhuff_encode_batch(status = NULL), one case per encode kernel: lengths and bytes against the oracle"""
    layout, mean = {"sorted": ("contiguous", ("le", 52)), "lanes": ("contiguous", ("ge", 53)),
                    "staged16": ("pairs", ("le", 52)), "staged8": ("explicit", ("ge", 53)),
                    "direct": ("pairs", ("ge", 121))}[route]
    strings = batches["plain", "short"][:257]
    for fill, sentinel in H.RUNS:
        base = H.place_input(strings, layout, 1, fill)
        (_, size, _), = route_sizes((mean + (None,),), 257, base["end"])[1:]
        inp = H.place_input(strings, layout, 1, fill, in_size=size)
        _, exp = H.oracle_run(oracle_codec, "encode", inp, sentinel)
        del exp["status"]
        res = gpu_run(torch_cuda, "encode", inp, sentinel, with_status=False)
        H.check(res, exp, H.mask_of("encode", inp), sentinel, starts=H.out_starts("encode", inp),
                label="encode status=NULL %s fill=%#x" % (route, fill))


# ------------------------------------------------------------------------------------------------
# packed output
# ------------------------------------------------------------------------------------------------
def _packed_expected(op, inp, exp):
    """the oracle's slot-layout result moved to the packed layout: tile t's outputs back to back from its bound"""
    from h2o_amd import codec

    n = inp["n"]
    olen = exp["out_len"]
    keep = np.where(olen == H.FAIL, 0, olen).astype(np.int64)
    pos = codec.packed_positions(inp["in_off"][:n], olen, op == "decode")
    size = (8 * inp["end"]) // 5 if op == "decode" else inp["end"]  # floor(8 in_off[n] / 5) | in_off[n]
    out = np.zeros(size, np.uint8)
    slots = H.out_starts(op, inp)
    for i in np.nonzero(keep)[0]:
        out[pos[i]:pos[i] + keep[i]] = exp["out"][slots[i]:slots[i] + keep[i]]
    off = np.append(pos, pos[-1] + keep[-1]).astype(np.uint32)
    return dict(out=out, out_off=off, out_len=olen, status=exp["status"]), H.ranges_mask(pos, pos + keep, size)


@pytest.mark.parametrize("op", ["decode", "encode"])
@pytest.mark.parametrize("kind", ["short", "mixed"])
def test_packed(torch_cuda, oracle_codec, batches, op, kind):
    """hhuff_{de,en}code_batch_packed with `out` of exactly the slot end and a guarded out_off[n + 1]: nothing but
    the outputs is written.  Routes: the short-stage and long-stage packed kernels, the scratch + pack_tiles path"""
    from h2o_amd import codec

    torch = torch_cuda
    strings, names = batches["huff", kind] if op == "decode" else (batches["plain", kind], None)
    routes = (("le", 40, None), ("ge", 41, None), ("le", 128, None), ("ge", 129, None)) if op == "decode" else \
        (("le", 52, None), ("ge", 53, None), ("le", 120, None), ("ge", 121, None))
    for n in (1, 63, 64, 65, 1025):
        for off0 in (0, 7):
            for fill, sentinel in H.RUNS:
                base = H.place_input(strings[:n], "contiguous", off0, fill)
                nb = H.name_bits(names[:n], fill) if op == "decode" else None
                for rname, size, _ in route_sizes(routes, n, base["end"]):
                    inp = H.place_input(strings[:n], "contiguous", off0, fill, in_size=size)
                    _, slot = H.oracle_run(oracle_codec, op, inp, sentinel, names=nb)
                    exp, mask = _packed_expected(op, inp, slot)
                    for defer in (DEFAULT_DEFER, 0):
                        _, data = H.to_device(torch, inp["whole"])
                        bufs = {"out": H.guarded(torch, exp["out"].size, sentinel),
                                "out_off": H.guarded(torch, 4 * (n + 1), sentinel),
                                "out_len": H.guarded(torch, 4 * n, sentinel), "status": H.guarded(torch, n, sentinel)}
                        kw = dict(out=bufs["out"][1], out_off=bufs["out_off"][1].view(torch.int32),
                                  out_len=bufs["out_len"][1].view(torch.int32), status=bufs["status"][1], in_size=size)
                        with edge_defer(defer):
                            if op == "decode":
                                codec.decode_batch_packed(data, _dev(torch, inp["in_off"]), n,
                                                          is_name_bits=_dev(torch, nb), **kw)
                            else:
                                codec.encode_batch_packed(data, _dev(torch, inp["in_off"]), n, **kw)
                            torch.cuda.synchronize()
                        res = {k: w.cpu().numpy() for k, (w, _) in bufs.items()}
                        H.check(res, exp, mask, sentinel, label="packed %s %s n=%d in_off0=%d route=%s defer_min=%#x "
                                "fill=%#x" % (op, kind, n, off0, rname, defer, fill))


# ------------------------------------------------------------------------------------------------
# string literals
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix_bits,qpack", [(7, False), (3, True)])
def test_decode_literals(torch_cuda, oracle_codec, batches, prefix_bits, qpack):
    """hhuff_decode_literals with `out` of exactly floor(8 in_size / 5) + 16 bytes and all four result arrays
    guarded.  A literal's decoded bytes may land in its payload's slot, [floor(8 p / 5), floor(8 (p + len) / 5))"""
    from h2o_amd import codec

    torch = torch_cuda
    huff, names = batches["huff", "short"]
    plain = batches["plain", "short"]
    rng = np.random.default_rng(5)
    for n in (1, 64, 65, 257):
        buf, offs, pay, plen = bytearray(b"\x00" * 3), [], [], []
        for i in range(n):
            payload, h = (huff[i], 1 << prefix_bits) if i % 3 != 1 else (plain[i].lower(), 0)
            above = int(rng.integers(256)) & ~((2 << prefix_bits) - 1) & 0xFF  # the caller's bits above the H flag
            offs.append(len(buf))
            buf += oracle_codec.encode_int(len(payload), prefix_bits, h | above)
            pay.append(len(buf))
            plen.append(len(payload))
            buf += payload
        end = len(buf)
        off = np.asarray(offs, np.uint32)
        pay, plen = np.asarray(pay, np.int64), np.asarray(plen, np.int64)
        lit_end = np.where(np.arange(n) % 2 == 0, end, pay + plen).astype(np.uint32)  # the block's end | its own
        for fill, sentinel in H.RUNS:
            for in_size in (end, 129 * n + end):
                whole, data = H.guarded(np, in_size, fill)
                data[3:end] = np.frombuffer(bytes(buf), np.uint8)[3:]
                data[:3] = fill
                nb = H.name_bits(names[:n], fill)
                size = (8 * in_size) // 5 + 16
                o = oracle_codec.literals_batch(data, off, lit_end, n, prefix_bits, qpack=qpack, is_name_bits=nb,
                                                out_size=size)
                exp = dict(zip(("out", "out_len", "pay_off", "consumed", "status"), o))
                np.testing.assert_array_equal(exp["pay_off"], pay)
                mask = H.ranges_mask((8 * pay) // 5, (8 * (pay + plen)) // 5, size)
                _, d = H.to_device(torch, whole)
                out_w, out = H.guarded(torch, size, sentinel)
                # codec.decode_literals allocates its own result arrays (max(n, 1) entries, unguarded): the C ABI
                # directly, with guarded arrays of exactly n entries
                bufs = {"out": (out_w, out), "out_len": H.guarded(torch, 4 * n, sentinel),
                        "pay_off": H.guarded(torch, 4 * n, sentinel), "consumed": H.guarded(torch, 4 * n, sentinel),
                        "status": H.guarded(torch, n, sentinel)}
                dp = codec._dp
                d_off, d_end = _dev(torch, H._poisoned(off, lambda j: 0)), _dev(torch, H._poisoned(lit_end, lambda j: 0))
                d_nb = _dev(torch, nb)
                rc = codec.lib().hhuff_decode_literals(
                    dp(d), in_size, dp(d_off), dp(d_end), n, prefix_bits, 1 if qpack else 0, dp(d_nb), dp(out),
                    dp(bufs["out_len"][1]), dp(bufs["pay_off"][1]), dp(bufs["consumed"][1]), dp(bufs["status"][1]),
                    torch.cuda.current_stream().cuda_stream)
                assert rc == 0
                torch.cuda.synchronize()
                res = {k: w.cpu().numpy() for k, (w, _) in bufs.items()}
                H.check(res, exp, mask, sentinel, starts=(8 * pay) // 5,
                        label="literals p=%d n=%d in_size=%d fill=%#x" % (prefix_bits, n, in_size, fill))


# ------------------------------------------------------------------------------------------------
# host arrays
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["decode", "encode"])
def test_host_api_exact_size(torch_cuda, oracle_codec, batches, op):
    """hhuff_{de,en}code_batch_host with a host `out` of exactly the documented size (decode floor(8 in_size / 5),
    encode in_size), implicit layout, n = 65: numpy buffers with guards (bytes of `out` outside the regions are
    unspecified on this path; the bytes around `out`, `out_len` and `status` are not)"""
    from h2o_amd import codec

    n = 65
    strings, names = batches["huff", "short"] if op == "decode" else (batches["plain", "short"], None)
    for fill, sentinel in H.RUNS:
        inp = H.place_input(strings[:n], "contiguous", 7, fill)
        nb = H.name_bits(names[:n], fill) if op == "decode" else None
        _, exp = H.oracle_run(oracle_codec, op, inp, sentinel, names=nb)
        size = H.implicit_out_size(op, inp)
        res = {"out": H.guarded(np, size, sentinel)[0], "out_len": H.guarded(np, 4 * n, sentinel)[0],
               "status": H.guarded(np, n, sentinel)[0]}
        p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
        inner = {k: H.entries(w, np.uint8) for k, w in res.items()}
        if op == "decode":
            rc = codec.lib().hhuff_decode_batch_host(p(inp["data"]), inp["in_size"], p(inp["in_off"]), None, n, p(nb),
                                                     p(inner["out"]), size, None, p(inner["out_len"]),
                                                     p(inner["status"]), 0)
        else:
            rc = codec.lib().hhuff_encode_batch_host(p(inp["data"]), inp["in_size"], p(inp["in_off"]), None, n,
                                                     p(inner["out"]), size, None, p(inner["out_len"]),
                                                     p(inner["status"]), 0)
        assert rc == 0, codec.lib().hhuff_last_error_string()
        # the host path copies the whole slot range back: every byte of `out` may change, no byte of a guard
        H.check(res, exp, np.ones(size, bool), sentinel, starts=H.out_starts(op, inp),
                label="%s host fill=%#x" % (op, fill))
