"""The QPACK decoder at hand-built edges (qpack_corpora.py) on the GPU: sessions of up to five steps through exact-size
guarded arrays (blocks_harness.py), twice (input fill / output sentinel); after every step its input, arena and
per-slot outputs are overwritten and the scratch is moved.  Compared with the restatement field by field -- offsets,
lengths, full fflags, bytes, per-section and per-connection arrays (enc_consumed included), request records, guards,
untouched arena bytes -- and with the reference's own results (tests/golden/block_edges.npz)."""
import pytest

import blocks_harness as BH
import qpack_corpora as QC
from conftest import load_golden
from blocks_corpora import fixture_key
from qpack_corpora import reference_pairs as qreference_pairs

QPACK = QC.NAMES


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def gpu_session(torch, oracle_codec, bt, mode, label):
    exp = BH.qexpected(oracle_codec, bt, mode)
    return BH.qrun(lambda sentinel: BH.GpuQpack(torch, sentinel), bt, mode,
                   check=lambda a, i, sentinel: BH.check_call(a, exp[i], "%s (sentinel %#x)" % (label, sentinel)))


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", [(n, m) for n in QPACK
                                       for m in (("plain", "qreq") if n in QC.ALL_MODES else ("plain",))])
def test_gpu_matches_restatement_at_the_edges(torch_cuda, oracle_codec, name, mode):
    for label, bt in QC.batches(QC.corpora()[name]):
        gpu_session(torch_cuda, oracle_codec, bt, mode, "%s %s" % (label, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("name", QPACK)
def test_gpu_matches_reference_fixture(torch_cuda, oracle_codec, name):
    g = load_golden("block_edges")
    for label, bt, mode in qreference_pairs(QC.corpora()[name]):
        done = gpu_session(torch_cuda, oracle_codec, bt, mode, label)
        got = BH.qsummary([BH.qresult_of(a) for a in done], bt, mode)
        BH.assert_same_summary(got, {k: g[fixture_key(name, label, k)] for k in got}, label)
