"""The arithmetic of the host-array batch paths (h2o_amd/csrc/hhuff_hostplan.h: implicit slots, the chunk cuts, the
layout a chunk and a peer shard share, the packed runs, the shard cut) without a GPU: tools/hostplan_host.cpp as a
stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer against the plain-Python model
(tests/host_paths_model.py) and the distributed path's split (h2o_amd/dist.py).  test_host_paths_host.py ties the
model's constants to the sources by their text; here the expressions next to them are run."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bounds_harness as H
import host_paths_corpora as C
import host_paths_model as M
from conftest import ROOT

B_SMALL = 4096  # the packed corpus's staging boundary (as test_host_paths_host.py)
OP = {"decode": "d", "encode": "e"}
REFUSE_IN, REFUSE_OUT = "in_off[n] > in_size", "out_size below the output slots of the batch"


def _nums(a):
    return " ".join(str(int(x)) for x in a)


def cut_inputs():
    """(offsets, n, chunk_bytes): test_cut_rule's hand-checked cases and every small corpus case"""
    off = np.arange(0, 10 * 101, 10)  # 100 strings of 10 B
    chunks = (1, 319, 640, 650, 959, 960, 1 << 40)
    out = [(off, 100, cb) for cb in chunks] + [(off + 7, 100, cb) for cb in chunks]
    out += [(off, 96, 1 << 40), (off, 1, 1), (off, 33, 0), (np.zeros(71, np.int64), 70, 1), (off + 163, 100, 1)]
    out += [(c.off(), c.n, c.chunk_bytes) for c in C.corpus()]
    return out


def shard_inputs():
    """test_multi.py::test_shard_bounds_match_dist_split's offsets"""
    out = []
    for nshards in range(1, 9):
        rng = np.random.default_rng(100 + nshards)
        for n, lo, hi, ef in ((1, 5, 5, 0), (7, 0, 3, 0.5), (1000, 8, 512, 0), (5000, 24, 72, 0.1), (64, 0, 0, 0)):
            L = rng.integers(lo, hi + 1, n)
            L[rng.random(n) < ef] = 0
            off = np.concatenate([[0], np.cumsum(L)])
            out += [(off, n, nshards, align) for align in (1, 64)]
    return out


def implicit_inputs():
    """(op, in_size, in_end, out_size, expected): accept and refuse on each side of both limits"""
    out = []
    for op in ("decode", "encode"):
        for end in (1000, 1003, 0):  # 1003: floor(8 * 1003 / 5) rounds down
            slot = M.slot_of(op, end)
            out += [(op, end, end, slot, "ok"), (op, end + 1, end, slot + 1, "ok"), (op, 1 << 40, end, 1 << 40, "ok")]
            if end:
                out += [(op, end - 1, end, 1 << 40, REFUSE_IN), (op, end, end, slot - 1, REFUSE_OUT), (op, end, end, 0, REFUSE_OUT),
                        (op, end - 1, end, slot - 1, REFUSE_IN)]  # both: the input's refusal comes first
    out.append(("decode", 0xFFFFFFFF, 0xFFFFFFFF, M.slot_of("decode", 0xFFFFFFFF), "ok"))  # 8 x in_end in 64 bits
    out.append(("decode", 0xFFFFFFFF, 0xFFFFFFFF, M.slot_of("decode", 0xFFFFFFFF) - 1, REFUSE_OUT))
    return out


def check_pieces(op, names, m, v):
    """the piece offsets of one chunk (the model has none): invariants of the layout"""
    base, nbytes, olo, ohi, obase, ocap, nw, o_off, o_nm, o_out, o_len, o_st, need = v
    assert all(x % 16 == 0 for x in (o_off, o_nm, o_out, o_len, o_st, need, obase)), v
    # in order and disjoint: input (and the 16 bytes a 16-B load may read past it), offsets, names, out, out_len, status
    assert nbytes + 16 <= o_off and o_off + 4 * (m + 1) <= o_nm and o_nm + 4 * nw <= o_out, v
    assert o_out + ocap <= o_len and o_len + 4 * m <= o_st and o_st + m <= need, v
    assert ocap == ohi - obase + 16 and obase <= olo <= ohi and o_out + (ohi - obase) <= o_len, v
    assert nw == ((m + 31) // 32 if op == "decode" and names else 0), v


def test_hostplan_host_equals_the_model_under_sanitizers(tmp_path, oracle_codec):
    cases = []  # (line, check(answer))

    def add(line, check):
        cases.append((line, check))

    def expect(want):
        def check(got):
            assert got == want, (got, want)
        return check

    cuts = cut_inputs()
    assert len(cuts) > 100
    for off, n, cb in cuts:
        add("cuts %d %d %s" % (n, cb, _nums(off[:n + 1])), expect(_nums(M.cuts(off, n, cb))))
        for op in ("decode", "encode"):
            for names in (0, 1):
                want = M.plan(op, off, n, cb)

                def check(got, op=op, names=names, want=want):
                    chunks = [[int(x) for x in part.split()] for part in got.split(";") if part.strip()]
                    assert len(chunks) == len(want)
                    for v, w in zip(chunks, want):
                        assert tuple(v[:10]) == (w.i0, w.i1, w.m, w.s0, w.e0, w.base, w.nbytes, w.olo, w.ohi, w.obase), (v, w)
                        check_pieces(op, names, w.m, v[5:])
                add("plan %s %d %d %d %s" % (OP[op], names, n, cb, _nums(off[:n + 1])), check)
    # test_cut_rule's hand-checked tuple, from the program's own answer
    hand = [line for line, _ in cases].index("plan d 1 100 1 %s" % _nums(np.arange(0, 10 * 101, 10) + 163))

    packed = C.packed_corpus(B_SMALL)
    assert len(packed) == 10
    fails_at_tile_end = False  # run_hi's arm for a tile whose last string keeps nothing
    for c in packed:
        a = c.arrays(*H.RUNS[0])
        _, slots = H.oracle_run(oracle_codec, c.op, a, H.RUNS[0][1], names=a["names"])
        exp, _ = M.packed_from_slots(c.op, c.off(), c.n, slots)
        runs = M.packed_runs(c.op, c.off(), c.n, exp["out_off"], exp["out_len"])
        assert len(runs) == 3
        fails_at_tile_end = fails_at_tile_end or any(int(exp["out_len"][i]) == H.FAIL for i in (63, 127, c.n - 1))
        add("runs %s %d %s %s %s" % (OP[c.op], c.n, _nums(c.off()), _nums(exp["out_off"]), _nums(exp["out_len"])),
            expect(_nums(x for r in runs for x in r)))

    assert fails_at_tile_end

    import torch

    from h2o_amd import dist as hd

    for off, n, ns, align in shard_inputs():
        want = hd.byte_balanced_bounds(torch.from_numpy(off.astype(np.int64)), ns).numpy().copy()
        want[1:-1] -= want[1:-1] % align  # the inner bounds rounded down to the alignment; 0 and n stay
        add("shard %d %d %d %s" % (n, ns, align, _nums(off)), expect(_nums(want)))

    for op, in_size, in_end, out_size, want in implicit_inputs():
        add("implicit %s %d %d %d" % (OP[op], in_size, in_end, out_size), expect(want))
    for op in ("decode", "encode"):
        mine = {w for o, _, _, _, w in implicit_inputs() if o == op}
        assert mine == {"ok", REFUSE_IN, REFUSE_OUT}

    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    probe_src = tmp_path / "probe.cpp"
    probe_src.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++", *san, str(probe_src), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes")
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for line, _ in cases:
            f.write(line + "\n")
    exe = str(tmp_path / "hostplan_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *san, "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "h2o_amd", "csrc"), os.path.join(ROOT, "tools", "hostplan_host.cpp"), "-o", exe],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[len(cases)] == "ok: hostplan_host %d" % len(cases), r.stdout[-2000:]
    for (line, check), got in zip(cases, lines):
        try:
            check(got.strip())
        except AssertionError as e:
            raise AssertionError("%s: %s" % (line[:200], e))
    first = [int(x) for x in lines[hand].split(";")[0].split()]
    assert tuple(first[5:10]) == (160, 323, 260, 772, 256) and first[:5] == [0, 32, 32, 163, 483]
