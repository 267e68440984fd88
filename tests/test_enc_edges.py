"""The header encoders' edge corpus on the GPU (tests/enc_corpora.py through tests/enc_harness.py):
hhuff_hpack_flatten_responses and the stateless hhuff_qpack_flatten_responses byte for byte against the restatement,
on exact-size guarded arrays under both (input fill, sentinel) runs, with regions of hhuff_*_response_bound and with
regions that fit exactly (the first at offsets 1 and 13), the previous call's input overwritten before each
HHUFF_ENC_CONTINUE call and the scratch moved.  Nothing outside [out_off[r], out_off[r] + out_len[r]) may be written.
The HPACK groups also go through hhuff_hpack_flatten_responses_slots with a slot map that is not the identity.
One test per group: a group is one batch per call."""
import pytest

import enc_corpora as EC
import enc_harness as EH

VARIANTS = {"bound": None, "fit1": 1, "fit13": 13}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from h2o_amd import build

    build.build(verbose=False)
    return torch


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EC.GROUPS))
def test_gpu_group(torch_cuda, oracle_codec, name):
    for v, first in VARIANTS.items():
        g = EC.group(name) if first is None else EH.refit(EC.group(name), first)

        def check(a, i, g=g, v=v):
            EH.check(a, g["exp"][i], "%s, %s, call %d, sentinel %#x" % (name, v, i, a["sentinel"]))

        EH.run(lambda sentinel, g=g: EH.GpuEnc(torch_cuda, g["proto"], sentinel), g, check)


@pytest.mark.gpu
@pytest.mark.parametrize("name", EC.HPACK_GROUPS)
def test_gpu_group_slots(torch_cuda, oracle_codec, name):
    """the same calls through the _slots entry point, connection c in slot nconn + 1 - c of nconn + 3: the second
    instantiation of the walk and of the ring pass; the results are those of the plain call (the model's)"""
    g = EC.group(name)
    nconn = g["calls"][0]["conn_first"].size - 1
    slots = [nconn + 1 - c for c in range(nconn)]

    def check(a, i):
        EH.check(a, g["exp"][i], "%s, slots, call %d, sentinel %#x" % (name, i, a["sentinel"]))

    EH.run(lambda sentinel: EH.GpuEnc(torch_cuda, "h", sentinel, slots=slots), g, check)
