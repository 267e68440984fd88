"""h2o's request / response rules at every rule edge and byte route, on the GPU: the corpus of rules_corpora.py --
every case by every route its decisive field can take into req_field / resp_field -- through
hhuff_hpack_parse_requests / _responses (heads and trailers) and hhuff_qpack_parse_requests / _responses on
exact-size guarded arrays (blocks_harness.py), twice (input fill / output sentinel), compared with the cases' literal
expectations (verdict, record words, header flags, field count) and field by field with the restatement.  One batch
holds every case of a parser, accepting and failing ones alternating lane by lane; then every case stands alone at
connections 0, 63 and 64 of a 65-connection batch; and a handful of special names reach the rules from entries that
went through hhuff_conn_export / hhuff_conn_import."""
import numpy as np
import pytest

import blocks_harness as BH
import rules_corpora as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def hpack_run(torch, oracle_codec, batches, impl=BH.GpuBlocks):
    for label, bt, modes, variants in batches:
        exp = BH.expected(oracle_codec, bt, modes)
        done = BH.run(lambda sentinel: impl(torch, sentinel), bt, modes,
                      check=lambda a, i, sentinel: BH.check_call(a, exp[i], "%s (sentinel %#x)" % (label, sentinel)))
        RC.check_literal(BH.summary([BH.result_of(a) for a in done], bt, modes), bt, modes, variants, label)


def qpack_run(torch, oracle_codec, batches):
    for label, bt, mode, variants in batches:
        exp = BH.qexpected(oracle_codec, bt, mode)
        done = BH.qrun(lambda sentinel: BH.GpuQpack(torch, sentinel), bt, mode,
                       check=lambda a, i, sentinel: BH.check_call(a, exp[i], "%s (sentinel %#x)" % (label, sentinel)))
        RC.check_literal(BH.qsummary([BH.qresult_of(a) for a in done], bt, mode), bt, mode, variants, label)


@pytest.mark.parametrize("mode", ["req", "res"])
def test_every_case_by_every_route_hpack(torch_cuda, oracle_codec, mode):
    hpack_run(torch_cuda, oracle_codec, RC.hpack_batches(mode))


@pytest.mark.parametrize("parser", ["h3_req", "h3_res"])
def test_every_case_by_every_route_qpack(torch_cuda, oracle_codec, parser):
    qpack_run(torch_cuda, oracle_codec, RC.qpack_batches(parser))


@pytest.mark.parametrize("mode", ["req", "res"])
def test_every_case_alone_in_its_wave_hpack(torch_cuda, oracle_codec, mode):
    hpack_run(torch_cuda, oracle_codec, RC.hpack_alone_batches(mode))


@pytest.mark.parametrize("parser", ["h3_req", "h3_res"])
def test_every_case_alone_in_its_wave_qpack(torch_cuda, oracle_codec, parser):
    qpack_run(torch_cuda, oracle_codec, RC.qpack_alone_batches(parser))


IMPORTED = (b"te", b"content-length", b"host", b":path", b"connection", b"datagram-flow-id")


def test_special_names_from_imported_entries(torch_cuda, oracle_codec):
    """the plain-mode call inserts the entries; before the request call every connection is exported, imported into
    other slots of another scratch and from there into a new dense one (test_conn_image_gpu.hop), the scratches it
    leaves overwritten: the names reach req_field from imported entries, whose class is recomputed on each reference"""
    import test_conn_image_gpu as CI
    from h2o_amd import codec as C

    from blocks_harness import batch

    fam = C.conn_family(C.FAM_HPACK_DEC, 4096)
    vs = [(v, "h2_req") for v in RC.hpack_variants("h2_req")[0]
          if v["plan"] == "plain" and v["case"]["fields"][v["case"]["at"]][0] in IMPORTED]
    vs = RC.interleave(vs, lambda vp: RC.expect_for(vp[0]["case"], vp[1])["verdict"])
    assert {v["case"]["fields"][v["case"]["at"]][0] for v, _ in vs} == set(IMPORTED)
    bt = batch(RC.hpack_corpus([v for v, _ in vs], "plain"), 4096, spacers=False)
    assert bt["nconn"] <= CI.NA

    class Moved(BH.GpuBlocks):
        def poison(self):
            BH.GpuBlocks.poison(self)
            assert self.scratch[1].numel() == bt["nconn"] * C.conn_slab_size(fam)
            self.keep.append(self.scratch)
            self.scratch = CI.hop(self.torch, fam, self.scratch[1], bt["nconn"], seed=5, fill=self.sentinel)

    hpack_run(torch_cuda, oracle_codec, [("rules req imported", bt, ["plain", "req"], vs)], impl=Moved)
