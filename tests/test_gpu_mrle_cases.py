"""-m gpu: the mRLE cases of tests/mrle_cases.py on the device against the oracle, one test per family (--durations names the slow ones).
tests/test_mrle_cases.py holds the preconditions of the cases.  The atomics of k_mrle_gain and k_mrd_tile_counts, and the workgroups of
one launch beside each other, run concurrently only here; so do the two streams of `caps-hostile`, whose count passes 2^32."""
import pytest

import bzip3_amd
import mrle_cases as M

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family", tuple(M.ENC_FAMILIES))
def test_encoder_and_decoder_on_encoder_cases(gpu_lib, oracle, family):
    g = bzip3_amd.StageApi(gpu_lib)
    for name, d in M.ENC_FAMILIES[family]():
        M.check_encoder_case(g, oracle, name, d)


@pytest.mark.parametrize("family", tuple(M.DEC_FAMILIES) + ("caps", "caps-hostile"))
def test_decoder(gpu_lib, oracle, family):
    g = bzip3_amd.StageApi(gpu_lib)
    for c in M.dec_cases(oracle, family):
        M.check_decoder_case(g, oracle, *c)


def test_threshold(gpu_lib, oracle):
    M.check_threshold(gpu_lib, oracle, bzip3_amd.State)


@pytest.mark.parametrize("offset", M.UNALIGNED_OFFSETS)
def test_unaligned_buffer(gpu_lib, oracle, offset):
    import torch

    buf = torch.zeros(gpu_lib.bz3_bound(65 * 1024) + 128, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    at = lambda p: p - buf.data_ptr()

    def write(p, d):
        buf[at(p) : at(p) + len(d)] = torch.frombuffer(bytearray(d), dtype=torch.uint8).to(buf.device)
        torch.cuda.synchronize()  # the library's streams do not wait for torch's

    M.check_unaligned(gpu_lib, oracle, buf.data_ptr(), offset, write, lambda p, n: bytes(buf[at(p) : at(p) + n].cpu().numpy()))
