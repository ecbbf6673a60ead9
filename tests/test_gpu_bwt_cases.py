"""The suffix sorter's adversarial cases (tests/bwt_cases.py) on the device: every case against the oracle, its code table against the optimum, its record
(bz3_hip_debug_bwt_record) against the model, and the precondition it is named for -- as tests/test_bwt_cases.py does under the emulator."""
import pytest

import bwt_cases as cases
import bzip3_amd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(gpu_lib):
    yield bzip3_amd.StageApi(gpu_lib)
    gpu_lib.bz3_hip_debug_bwt_big_rounds(-1)
    gpu_lib.bz3_hip_debug_set_bwt_batch(-1)


@pytest.mark.parametrize("name", cases.ALL + cases.DEVICE_ONLY)
def test_case(g, oracle, name):
    cases.run_case(g, oracle, name)


@pytest.mark.parametrize("rotate", (0, 3))
def test_a_run_of_eight(g, oracle, rotate):
    cases.run_batch(g, oracle, rotate)


@pytest.mark.parametrize("rounds", (0, 8))
@pytest.mark.parametrize("name", cases.BIG_ROUNDS_CASES)
def test_other_big_rounds(g, oracle, name, rounds):
    g.lib.bz3_hip_debug_bwt_big_rounds(rounds)
    try:
        _, rec = cases.run_case(g, oracle, name)
        assert rec["big_rounds"] == rounds
    finally:
        g.lib.bz3_hip_debug_bwt_big_rounds(-1)
