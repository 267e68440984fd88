"""bench.py: a plain run does the headline step alone (everything else behind --full), and --dump-outputs DIR
writes what the last timed step computed, identically from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

SECONDARY = ("no_cpu_baseline", "no_traffic", "no_host", "no_extra", "no_packed")
FULL_ONLY_KEYS = ("packed", "configs", "f4", "per_string_latency_us", "host_inclusive", "cpu_baseline")


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_plain_run_measures_the_headline_alone(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert not a.full and a.steps == 7 and a.warmup == 2 and a.dump_outputs is None
    assert all(getattr(a, k) for k in SECONDARY)


def test_full_runs_everything_unless_switched_off(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d" and not any(getattr(a, k) for k in SECONDARY)
    a = _parse(monkeypatch, "--full", "--no-host", "--no-traffic")
    assert a.no_host and a.no_traffic and not (a.no_extra or a.no_packed or a.no_cpu_baseline)


def test_new_options_pass_through_the_launcher():
    from torch.distributed.run import get_args_parser

    cmd = bench.rank_command(2, ["--full", "--dump-outputs", "d", "--steps", "2"], 29500)
    a = get_args_parser().parse_args(cmd[cmd.index("torch.distributed.run") + 1:])
    assert a.training_script_args[:5] == ["--full", "--dump-outputs", "d", "--steps", "2"]


def _slots(fill):
    """a small slot layout: 3,000 strings in slots of 5..40 bytes, every 7th a FAIL, gaps filled with `fill`"""
    import torch

    rng = np.random.default_rng(3)
    n = 3000
    slot = rng.integers(5, 41, n)
    starts = np.zeros(n, np.int64)
    starts[1:] = np.cumsum(slot)[:-1]
    lens = rng.integers(0, slot + 1)
    lens[::7] = -1
    status = rng.integers(0, 4, n).astype(np.uint8)
    out = np.full(int(slot.sum()) + 16, fill, np.uint8)
    body = rng.integers(0, 256, out.size).astype(np.uint8)
    for s, L in zip(starts, lens):
        if L > 0:
            out[s:s + L] = body[s:s + L]
    t = torch.from_numpy
    return out, starts, lens, status, (t(out), t(starts), t(lens.astype(np.int32)), t(status))


def test_dump_outputs_holds_the_valid_bytes_only(tmp_path):
    import torch

    out, starts, lens, status, tensors = _slots(0xAA)
    bench.dump_outputs(torch, str(tmp_path / "a"), "x", *tensors)
    bench.dump_outputs(torch, str(tmp_path / "b"), "x", *_slots(0x55)[4])  # other garbage between the slots
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["x_bytes.npy", "x_sample_bytes.npy", "x_sample_index.npy", "x_sample_len.npy",
                     "x_sample_status.npy", "x_strings.npy"]
    a = {f[2:-4]: np.load(tmp_path / "a" / f) for f in names}
    for f in names:
        assert a[f[2:-4]].dtype in (np.float32, np.float64)
        assert np.array_equal(a[f[2:-4]], np.load(tmp_path / "b" / f)), f
    # fewer strings than the sample size: every string, in order
    assert np.array_equal(a["sample_index"], np.arange(lens.size))
    assert np.array_equal(a["sample_len"], lens) and np.array_equal(a["sample_status"], status)
    want = np.concatenate([out[s:s + L] for s, L in zip(starts, lens) if L > 0])
    assert np.array_equal(a["sample_bytes"], want)
    L0 = np.maximum(lens, 0)
    pad = lambda x, k: np.concatenate([x, np.zeros(-x.size % k, x.dtype)]).reshape(-1, k)  # noqa: E731
    sb = bench.DUMP_STRINGS_PER_BLOCK
    assert np.array_equal(a["strings"][:, 0], pad(L0, sb).sum(1))
    assert np.array_equal(a["strings"][:, 1], pad((lens == -1).astype(np.int64), sb).sum(1))
    assert np.array_equal(a["strings"][:, 2], pad(status.astype(np.int64), sb).sum(1))
    valid = np.zeros(out.size, np.int64)
    for s, L in zip(starts, L0):
        valid[s:s + L] = 1
    v = out.astype(np.int64) * valid
    bb = bench.DUMP_BYTES_PER_BLOCK
    assert np.array_equal(a["bytes"][:, 0], pad(v, bb).sum(1))
    assert np.array_equal(a["bytes"][:, 1], pad(v * (np.arange(v.size) % 251 + 1), bb).sum(1))


@pytest.mark.gpu
def test_plain_bench_dumps_what_the_codec_returns(tmp_path, monkeypatch, capsys):
    """a plain `bench.py --gpus 1 --steps N --warmup W --dump-outputs DIR` (small batch): the line holds the
    headline keys and nothing that needs a run of its own; the files are float arrays, equal between a run in a
    process of its own and one in this process, and equal to what the codec returns for the same seeded batch"""
    import torch

    from h2o_amd import codec, synth

    n = 65536
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--strings", str(n)]
    env = {k: v for k, v in os.environ.items() if k not in bench.LAUNCHER_ENV}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv + ["--dump-outputs", str(tmp_path / "a")],
                       env=env, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-4000:]
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "GiB/s" and line["higher_is_better"] is True
    assert line["dtype"] == "u8" and line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(line["config"]["global_plain_bytes"] / 2 ** 30 / (line["ms_per_step"] * 1e-3),
                                          rel=1e-3)
    assert not [k for k in FULL_ONLY_KEYS if k in line]
    assert line["roofline"]["traffic"] is None and "measured_copy_peak" not in line["roofline"]

    for k in bench.LAUNCHER_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv + ["--dump-outputs", str(tmp_path / "b")])
    bench.main()
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["steps"] == 3
    names = sorted(os.listdir(tmp_path / "a"))
    assert len(names) == 12 and names == sorted(os.listdir(tmp_path / "b"))
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in names}
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for f in names:
        assert a[f[:-4]].dtype in (np.float32, np.float64)
        assert np.array_equal(a[f[:-4]], np.load(tmp_path / "b" / f)), f

    # the same seeded batch through the codec here: n = the sample size, so the sample is every string
    b = synth.make_batch_torch("c4", n=n, seed=1000)
    off = b["off"].to(torch.int32)
    e_out, e_len, e_st = codec.encode_batch(b["data"], off, n)
    torch.cuda.synchronize()
    e_out, e_len, e_st, o = e_out.cpu().numpy(), e_len.cpu().numpy(), e_st.cpu().numpy(), b["off"].cpu().numpy()
    assert np.array_equal(a["encode_sample_index"], np.arange(n))
    assert np.array_equal(a["encode_sample_len"], e_len) and np.array_equal(a["encode_sample_status"], e_st)
    keep = np.nonzero(e_len > 0)[0]
    wire = np.concatenate([e_out[o[i]:o[i] + e_len[i]] for i in keep])
    assert np.array_equal(a["encode_sample_bytes"], wire)
    assert a["encode_bytes"][:, 0].sum() == wire.astype(np.int64).sum()
    # the decode leg decodes that wire back: the plain bytes of the kept strings
    plain = b["data"].cpu().numpy()
    assert np.array_equal(a["decode_sample_len"], (o[1:] - o[:-1])[e_len != -1])
    assert np.array_equal(a["decode_sample_bytes"], np.concatenate([plain[o[i]:o[i + 1]] for i in keep]))
