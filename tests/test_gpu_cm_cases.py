"""-m gpu: the CM cases of tests/cm_cases.py on the device against the oracle, in modes 0 (whole model), 1 and 2 (the row caches of two and three blocks per
CU), one test per family and mode (--durations names the slow ones).  tests/test_cm_cases.py holds the preconditions of the cases and runs them through the
emulator, which replaces v_mad_u32_u24, v_xad_u32, the v_addc_co_u32 that takes a ballot as carry-in, v_bfe_u32 / v_lshl_add_u32 and readlane with C: those
run only here.  So do workgroups that share a CU: the co-resident test puts a few more copies of a case than the three-per-CU threshold into one launch."""
import ctypes as C

import pytest

import bzip3_amd
import cm_batch_cases
import cm_cases as cc

pytestmark = pytest.mark.gpu
MODES = (0, 1, 2)
FAMILIES = ("straddle", "seams", "extremes", "rows", "sink", "windows")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("mode", MODES)
def test_kernels_on_every_case(gpu_lib, oracle, mode, family):
    """Encode equals the oracle, decode returns the plain bytes, the given-up counter moves by what the documented rule of the directory says (the budget
    boundary of each side among the rows cases: 0 for the longest block kept, 1 for the one a byte longer)."""
    cc.run_family(gpu_lib, oracle, family, mode)


@pytest.mark.parametrize("mode", MODES)
def test_decoder_on_truncated_streams(gpu_lib, oracle, mode):
    for name in cc.TRUNCATED:
        cc.run_truncations(gpu_lib, oracle, mode, name)


@pytest.mark.parametrize("mode", MODES)
def test_sink(gpu_lib, oracle, mode):
    cc.run_sink(gpu_lib, oracle, mode)
    if mode:
        cc.run_sink_thrash(gpu_lib, oracle, mode)


def co_resident_cases(oracle):
    t = cc.build(oracle)
    out = dict(t["straddle"])
    out.update({k: v[0] for k, v in t["rows"].items() if k.startswith("rows_cyclic")})
    out.update(t["extremes"])
    return {k: d for k, d in out.items() if len(d) >= 256}


def test_cases_with_three_blocks_on_a_cu(gpu_lib, oracle, monkeypatch):
    """The straddle, cyclic-rows and extremes cases as c2 + 5 identical jobs in ONE launch of the variant the automatic policy picks for that many (the
    three-per-CU row-cache kernels): every copy must agree with copy 0 (BZ3_CM_MANY_CHECK: -2 otherwise) and copy 0 with the oracle."""
    monkeypatch.setenv("BZ3_CM_MANY_CHECK", "1")
    cases = co_resident_cases(oracle)
    assert {"straddle_s1", "straddle_one_s11", "straddle_ends_in_zero", "rows_cyclic_R96", "rows_cyclic_R56", "rows_cyclic_R40", "extremes_run"} <= set(cases)
    try:
        assert gpu_lib.bz3_hip_bind_device(0) == 0 and gpu_lib.bz3_hip_set_cm_mode(-1) == 0
        c1, c2 = cm_batch_cases.thresholds(gpu_lib)
        copies = c2 + 5
        for e in (0, 1):
            assert gpu_lib.bz3_hip_cm_variant_for(0, copies, e) == 2
        for name, plain in cases.items():
            # (the hooks for many copies hand nothing back: by the rule of the directory none of these is given up)
            assert (cc.expected_given_up(plain, "enc", 2), cc.expected_given_up(plain, "dec", 2)) == (0, 0), name
            coded = oracle.cm_encode(plain)
            out = (C.c_uint8 * (gpu_lib.bz3_bound(len(plain)) + 64))()
            got = C.c_int32(0)
            ms = gpu_lib.bz3_hip_stage_cm_encode_many(bzip3_amd._cbuf(plain, len(plain)), len(plain), out, C.byref(got), copies)
            assert ms >= 0, (name, ms)
            assert got.value == len(coded) and C.string_at(out, got.value) == coded, name
            back = (C.c_uint8 * len(plain))()
            ms = gpu_lib.bz3_hip_stage_cm_decode_many(bzip3_amd._cbuf(coded, len(coded)), len(coded), back, len(plain), copies, None)
            assert ms >= 0, (name, ms)
            assert bytes(back) == plain, name
    finally:
        gpu_lib.bz3_hip_set_cm_mode(-1)
        gpu_lib.bz3_hip_bind_device(-1)
