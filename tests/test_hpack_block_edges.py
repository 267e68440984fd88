"""HPACK header blocks at hand-built edges (blocks_corpora.py) on the GPU: every call through exact-size guarded arrays
(blocks_harness.py), twice (input fill / output sentinel), the previous call's input, arena and per-slot outputs
overwritten and the scratch moved between two calls of a continuation, compared with the restatement field by
field (offsets, lengths, full fflags, bytes, records, guards, untouched arena bytes) and with the reference's own
results (tests/golden/block_edges.npz)."""
import pytest

import blocks_corpora as BC
import blocks_harness as BH
from conftest import load_golden
from blocks_corpora import MODES, fixture_key, reference_pairs

HPACK = BC.NAMES


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def gpu_run(torch, oracle_codec, bt, modes, label):
    exp = BH.expected(oracle_codec, bt, modes)
    return BH.run(lambda sentinel: BH.GpuBlocks(torch, sentinel), bt, modes,
                  check=lambda a, i, sentinel: BH.check_call(a, exp[i], "%s (sentinel %#x)" % (label, sentinel)))


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", [(n, m) for n in HPACK for m in (MODES if n in BC.ALL_MODES else (None,))])
def test_gpu_matches_restatement_at_the_edges(torch_cuda, oracle_codec, name, mode):
    for label, bt, modes in BC.batches(BC.corpora()[name], mode):
        gpu_run(torch_cuda, oracle_codec, bt, modes, "%s %s" % (label, mode or ""))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in HPACK if n != "big"])
def test_gpu_matches_reference_fixture(torch_cuda, oracle_codec, name):
    g = load_golden("block_edges")
    for label, bt, modes in reference_pairs(BC.corpora()[name]):
        done = gpu_run(torch_cuda, oracle_codec, bt, modes, label)
        got = BH.summary([BH.result_of(a) for a in done], bt, modes)
        BH.assert_same_summary(got, {k: g[fixture_key(name, label, k)] for k in got}, label)
