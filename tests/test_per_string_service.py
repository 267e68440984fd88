"""h2o_hpack_encode_huffman / h2o_hpack_decode_huffman on the GPU through tests/per_string_check.c: the encode corpus of
tests/encode_edges.py on every route, the isolation plans from 8 to 72 threads and at 2, 16 and 64 service waves,
mixed routes beside a batch call, the service's idle exit and relaunch, two devices.

Expectations come from the oracle restatement and are compared with tests/huff_ref.py before a child is started.
Each test is one child process under a time limit of its own; the driver checks every call of every thread (value,
bytes, soft_errors, sentinels, and from hhuff_service_stamps whether the service's wave served it) and names the
thread, mailbox, round and case of a mismatch.  A child that ends on a signal or at its limit fails its test and makes
the module's remaining tests skip: nothing is started on a device that may have faulted.  Each test prints its wall
time, its calls and how many of them the service served (pytest -s)."""
import os
import re
import subprocess
import time

import numpy as np
import pytest

import encode_edges as E
from test_capi import build_capi_check

pytestmark = pytest.mark.gpu

LIMIT = 120  # seconds a child may take (tests/test_capi.py's); the children here take a few
_DEAD = []


@pytest.fixture(scope="module")
def exe():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return build_capi_check("per_string_check.c")


def checked(reqs, oracle):
    """the calls with the oracle's expectations, each compared with huff_ref's"""
    out = []
    for q in reqs:
        o = E.expect(E.Req(q.label, q.op, q.data, q.is_name, q.soft_in), oracle)
        ref = q.answer() if q.soft is not None else E.ref_answer(q.op, q.data, q.is_name, q.soft_in)
        assert o.answer() == ref, q.label
        out.append(o)
    return out


def run_driver(exe, tmp_path, mode, reqs, threads, lockstep=True, env=None, batch=None, what=""):
    """-> (calls, served, batches) of a child that checked everything; fails with the driver's report otherwise"""
    if _DEAD:
        pytest.skip("an earlier child ended on a signal or at its time limit (%s)" % _DEAD[0])
    E.write_cases(tmp_path / "cases", reqs)
    E.write_plan(tmp_path / "plan", threads, lockstep)
    argv = [exe, mode, str(tmp_path / "cases"), str(tmp_path / "plan")] + ([str(batch)] if batch else [])
    keep = {k: v for k, v in os.environ.items() if not k.startswith("HHUFF_")}
    t0 = time.perf_counter()
    try:
        r = subprocess.run(argv, capture_output=True, text=True, timeout=LIMIT, env=dict(keep, **(env or {})))
    except subprocess.TimeoutExpired as e:
        _DEAD.append("%s: no end in %d s" % (what, LIMIT))
        pytest.fail("%s: the child did not end in %d s\n%s" % (what, LIMIT, e.stderr))
    wall = time.perf_counter() - t0
    if r.returncode < 0:
        _DEAD.append("%s: signal %d" % (what, -r.returncode))
        pytest.fail("%s: the child ended on signal %d\n%s%s" % (what, -r.returncode, r.stdout, r.stderr))
    assert r.returncode == 0, "%s\n%s%s" % (what, r.stdout, r.stderr)
    m = re.search(r"per_string_check: ok threads=(\d+) calls=(\d+) served=(\d+) batches=(\d+)", r.stdout)
    assert m and int(m.group(1)) == len(threads), r.stdout
    calls, served, batches = int(m.group(2)), int(m.group(3)), int(m.group(4))
    print("\n[per_string_service] %s: %.2f s, %d calls checked, %d served by the service, %d batch passes"
          % (what, wall, calls, served, batches))
    return calls, served, batches


def plan_threads(nthreads, rounds=E.PLAN_ROUNDS, device=lambda t: 0):
    """plan(nthreads) as the driver's files: cases in thread order, thread t's calls t * rounds .."""
    th = E.plan(nthreads)
    reqs = [q for t in th for q in t[:rounds]]
    return reqs, [{"device": device(t), "calls": [(t * rounds + r, 0) for r in range(rounds)]} for t in range(nthreads)]


# ------------------------------------------------------------------------------------------------
# the corpus, one thread
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus_calls(oracle_codec):
    return checked(E.corpus_reqs(E.corpus(), back=True), oracle_codec)


@pytest.mark.parametrize("path", ["service", "no_service", "long_enc=0", "long_enc=1"])
def test_corpus_on_one_thread(exe, tmp_path, corpus_calls, path):
    """every corpus string as an encode, every result decoded back; on the default path (mailbox up to 768 bytes,
    one_string_kernel up to 32768, encode_long_kernel beyond), on the launch path alone, and past 32768 bytes with
    either long encoder"""
    reqs, env, mode = corpus_calls, {}, "service"
    if path == "no_service":
        env, mode = {"HHUFF_NO_SERVICE": "1"}, "launch"
    elif path != "service":
        env = {"HHUFF_LONG_ENC": path[-1]}
        reqs = [q for q in corpus_calls if len(q.data) > E.ONE_MAX or (not q.op and 8 * len(q.data) // 5 > E.ONE_MAX)]
        assert sum(q.op for q in reqs) >= 15 and any(q.ret is None for q in reqs)
    small = sum(len(q.data) <= E.SVC_MAX for q in reqs)
    calls, served, _ = run_driver(exe, tmp_path, mode, reqs, [{"calls": [(i, 0) for i in range(len(reqs))]}],
                                  lockstep=False, env=env, what="corpus, " + path)
    assert calls == len(reqs) and served == (small if mode == "service" else 0)


# ------------------------------------------------------------------------------------------------
# isolation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nthreads,waves", [(8, None), (16, None), (17, None), (32, None), (64, None), (72, None),
                                            (32, 2), (64, 64)])
def test_isolation(exe, tmp_path, oracle_codec, nthreads, waves):
    """40 rounds posted together; thread t owns mailbox t mod 64 (at 72 threads eight mailboxes have two owners).  At
    16 waves 17 threads and more put several mailboxes of one wave into one poll, 2 waves put 16 there, 64 waves give
    every mailbox a wave of its own"""
    reqs, threads = plan_threads(nthreads)
    env = {"HHUFF_SVC_WAVES": str(waves)} if waves else {}
    calls, served, _ = run_driver(exe, tmp_path, "service", checked(reqs, oracle_codec), threads, env=env,
                                  what="isolation, %d threads, %s waves" % (nthreads, waves or "16 (default)"))
    assert calls == served == nthreads * E.PLAN_ROUNDS


# ------------------------------------------------------------------------------------------------
# mixed routes
# ------------------------------------------------------------------------------------------------
def test_mixed_routes(exe, tmp_path, oracle_codec):
    """ten threads on mailbox strings, four on 769..4096 bytes (one_string_kernel), one alternating 32768 and 32769
    bytes (one_string_kernel / the long paths), and a 2000-string hhuff_decode_batch on a stream of its own going
    round beside them"""
    rng = np.random.default_rng(0x31ED)
    rounds = E.PLAN_ROUNDS
    reqs, threads = plan_threads(10)
    for t in range(4):
        first = len(reqs)
        for r in range(rounds):
            n, op = int(rng.integers(769, 4097)), (t + r) & 1
            data = (E._plain_input if op else E._huff_input)(rng, n, r % 13 == 5)
            reqs.append(E.Req("mid t%d r%d %s %d B" % (10 + t, r, "enc" if op else "dec", n), op, data,
                              is_name=bool(rng.integers(2)), soft_in=int(rng.integers(4))))
        threads.append({"calls": [(first + r, 0) for r in range(rounds)]})
    first = len(reqs)
    for k, (op, n) in enumerate(((1, 32768), (1, 32769), (0, 32768), (0, 32769))):
        data = (E._plain_input if op else E._huff_input)(rng, n, False)
        reqs.append(E.Req("long %s %d B" % ("enc" if op else "dec", n), op, data, is_name=bool(k & 1)))
    threads.append({"calls": [(first + r % 4, 0) for r in range(rounds)]})
    strings = [E._huff_input(rng, int(n), i % 37 == 11 and n >= 4) for i, n in enumerate(rng.integers(1, 201, 2000))]
    E.write_batch(tmp_path / "batch", strings, rng.integers(0, 2, 2000).tolist(), oracle_codec)
    threads.append({"kind": E.KIND_BATCH, "calls": []})
    calls, served, batches = run_driver(exe, tmp_path, "service", checked(reqs, oracle_codec), threads,
                                        batch=tmp_path / "batch", what="mixed routes, 15 + 1 threads")
    assert calls == 15 * rounds and served == 10 * rounds and batches >= 1


# ------------------------------------------------------------------------------------------------
# idle exit and relaunch
# ------------------------------------------------------------------------------------------------
SLEEPS_US = (500, 1500, 1900, 2000, 2100, 2500, 5000, 20000)  # around kSvcIdle = 2 ms, and far beyond


@pytest.mark.parametrize("nthreads", [1, 4])
def test_idle_exit_and_relaunch(exe, tmp_path, oracle_codec, nthreads):
    """call, sleep d, call -- every thread at once, so that the grid sees no request for d: below 2 ms it stays, above
    it has left and the call launches it again (revive() in svc_call).  Every call is served and checked; no call
    falls back to the launch path (the stamps move) and the error string stays empty"""
    reqs, _ = plan_threads(nthreads)
    sleeps = [0] + [d for _ in range(12) for d in SLEEPS_US]
    assert nthreads * len(sleeps) <= 400
    threads = [{"calls": [(t * E.PLAN_ROUNDS + k % E.PLAN_ROUNDS, d) for k, d in enumerate(sleeps)]}
               for t in range(nthreads)]
    calls, served, _ = run_driver(exe, tmp_path, "service", checked(reqs, oracle_codec), threads,
                                  what="idle exit and relaunch, %d thread(s)" % nthreads)
    assert calls == served == nthreads * len(sleeps)


def test_a_sleeper_beside_busy_threads(exe, tmp_path, oracle_codec):
    """one of four threads sleeps 20 ms between its calls while the other three keep calling: the grid stays for the
    busy waves, and each call of the sleeper is served"""
    reqs, threads = plan_threads(4)
    threads[0]["calls"] = [(k, 20000 if k else 0) for k in range(12)]
    for t in (1, 2, 3):
        threads[t]["flags"] = E.FLAG_LOOP
    calls, served, _ = run_driver(exe, tmp_path, "service", checked(reqs, oracle_codec), threads, lockstep=False,
                                  what="a sleeper beside three busy threads")
    assert calls == served and calls >= 12 + 3 * E.PLAN_ROUNDS


# ------------------------------------------------------------------------------------------------
# two devices
# ------------------------------------------------------------------------------------------------
def test_two_devices(exe, tmp_path, oracle_codec):
    """two threads, each bound to a device of its own: g_svc[dev] keeps a grid, mailboxes and request numbers a device"""
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    reqs, threads = plan_threads(2, device=lambda t: t)
    calls, served, _ = run_driver(exe, tmp_path, "service", checked(reqs, oracle_codec), threads, what="two devices")
    assert calls == served == 2 * E.PLAN_ROUNDS
