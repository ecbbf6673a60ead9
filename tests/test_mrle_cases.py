"""CPU tests of the mRLE cases (tests/mrle_cases.py): the oracle against the real reference, the preconditions that make every case hit the
tile, wave, lane, chunk or 255 boundary it is named for (from a numpy model that is itself held against the oracle, so that a case cannot
go stale silently), and the kernel sources under the emulator.  tests/test_gpu_mrle_cases.py runs the same cases on the device, and the
two streams of `caps-hostile` (16 MiB each) only there."""
import ctypes as C
import os
import sys

import pytest

import bzip3_amd
import mrle_cases as M

HERE = os.path.dirname(os.path.abspath(__file__))
ENC = tuple(M.ENC_FAMILIES)
DEC = tuple(M.DEC_FAMILIES) + ("caps", "caps-hostile")


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    return bzip3_amd._declare(C.CDLL(build()))


def test_the_big_families_have_the_cases_the_tests_name():
    assert tuple(n for n, _ in M.ends_large()) == M.ENDS_LARGE_NAMES
    assert tuple(n for n, _ in M.spine()) == M.SPINE_NAMES
    assert tuple(c[0] for c in M.dspine()) == M.DSPINE_NAMES
    assert set(M.SMALL_ENC) | {"ends-large", "spine"} == set(ENC) and set(M.SMALL_DEC) | {"dspine", "caps-hostile"} == set(DEC)


# ---- the oracle against the reference's own stage functions ---------------------------------------------------------------------------
@pytest.mark.parametrize("family", ENC)
def test_oracle_equals_the_reference_on_encoder_cases(oracle, ref_stages, family):
    for name, d in M.ENC_FAMILIES[family]():
        e = oracle.mrle_encode(d)
        assert e == ref_stages.mrle_encode(d), name
        assert oracle.mrle_decode(e, len(d)) == ref_stages.mrle_decode(e, len(d)) == (0, d), name


@pytest.mark.parametrize("family", DEC)
def test_oracle_equals_the_reference_on_decoder_cases(oracle, ref_stages, family):
    for name, s, outlen, maxin in M.dec_cases(oracle, family):
        assert oracle.mrle_decode(s, outlen, maxin) == ref_stages.mrle_decode(s, outlen, maxin), name


# ---- every case hits what it is named for ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ENC)
def test_encoder_preconditions(oracle, family):
    cases = M.ENC_FAMILIES[family]()
    assert len({n for n, _ in cases}) == len(cases) > 0
    for name, d in cases:
        M.precondition_enc(oracle, family, name, d)
    if family == "longrun":  # every length from T + 1 on leaves a tile without a head somewhere, from 2T + 1 on everywhere
        for ln in M.LONGRUN_LENGTHS:
            k = [len(M.INTENT["longrun-%d-%s" % (ln, tag)]["headless"]) for tag, _ in M.LONGRUN_HEADS]
            assert (max(k) >= 1) == (ln > M.T) and (min(k) >= 1) == (ln > 2 * M.T), ln
    if family == "fastpath":
        assert {M.INTENT[n]["residue"] for n, _ in cases if "residue" in n} == set(range(16))
        assert {M.INTENT[n]["n"] % 16 for n, _ in cases if "tail" in n} == {0, 1, 15}


@pytest.mark.parametrize("family", DEC)
def test_decoder_preconditions(oracle, family):
    cases = M.dec_cases(oracle, family)
    assert len({c[0] for c in cases}) == len(cases) > 0
    for c in cases:
        M.precondition_dec(oracle, family, *c)
    if family == "cuts":
        got = {c[3] for c in cases}
        _, at = M.cuts_stream()
        want = {32, 33, at["first"], at["late"]} | set(at["chain"]) | {32 + k * M.T + d for k in (1, 2) for d in range(-3, 4)}
        assert got == want and len(at["chain"]) == 12


def test_decode_model_equals_the_oracle_on_genuine_streams(oracle):
    """The automaton of DecodeModel, on the oracle's streams of the small encoder cases: it decodes them to the input."""
    for family in M.SMALL_ENC:
        for name, d in M.ENC_FAMILIES[family]():
            assert M.DecodeModel(oracle.mrle_encode(d)).output() == d, name


# ---- the kernel sources under the emulator ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", M.SMALL_ENC)
def test_emulated_encoder_and_decoder_on_encoder_cases(emu, oracle, family):
    g = bzip3_amd.StageApi(emu)
    for name, d in M.ENC_FAMILIES[family]():
        M.check_encoder_case(g, oracle, name, d)


@pytest.mark.parametrize("name", M.ENDS_LARGE_NAMES)
def test_emulated_ends_of_a_chunk(emu, oracle, name):
    M.check_encoder_case(bzip3_amd.StageApi(emu), oracle, *M.case("ends-large", name))


@pytest.mark.parametrize("name", M.SPINE_NAMES)
def test_emulated_encoder_spine(emu, oracle, name):
    M.check_encoder_case(bzip3_amd.StageApi(emu), oracle, *M.case("spine", name))


@pytest.mark.parametrize("family", M.SMALL_DEC)
def test_emulated_decoder(emu, oracle, family):
    g = bzip3_amd.StageApi(emu)
    for c in M.dec_cases(oracle, family):
        M.check_decoder_case(g, oracle, *c)


@pytest.mark.parametrize("name", M.DSPINE_NAMES)
def test_emulated_decoder_spine(emu, oracle, name):
    M.check_decoder_case(bzip3_amd.StageApi(emu), oracle, *M.case("dspine", name))


# ---- through the block API ---------------------------------------------------------------------------------------------------------------
def test_emulated_threshold(emu, oracle):
    M.check_threshold(emu, oracle, bzip3_amd.State)


@pytest.mark.parametrize("offset", M.UNALIGNED_OFFSETS)
def test_emulated_unaligned_buffer(emu, oracle, offset):
    """Under the emulator device memory is host memory: a ctypes buffer, entered `offset` bytes behind a 16-byte boundary."""
    buf = (C.c_uint8 * (emu.bz3_bound(65 * 1024) + 128))()
    base = (C.addressof(buf) + 15) & ~15
    M.check_unaligned(emu, oracle, base, offset, lambda p, d: C.memmove(p, d, len(d)), lambda p, n: C.string_at(p, n))
