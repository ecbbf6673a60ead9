"""CPU: the per-byte paths of the guess-ahead CM decoder (cm.hip cm_decode_block_sync) under the emulator, whole model (mode 0) and the emulator's 40-row
cache (mode 9, CM_VARIANT_ROWS_TEST), once with the plain scheduler and once with whole waves put to sleep at random (BZ3_EMU_SCHED < 0, as
test_cm_protocols_survive_stalled_waves does).  Inputs: tests/cm_diet_cases.py; expected bytes: the oracle's.  The emulator runs the C form of every statement
that is a builtin or inline assembly on the GPU; tests/test_gpu_cm_decoder_diet.py runs the same inputs through those."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import bzip3_amd
import cm_diet_cases as dc

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = (0, 9)


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    return bzip3_amd._declare(C.CDLL(build()))


def test_preconditions(oracle):
    dc.check_preconditions(oracle)


@pytest.mark.parametrize("family", dc.FAMILIES)
@pytest.mark.parametrize("mode", MODES)
def test_families_decode_to_the_plaintext(emu, oracle, mode, family):
    dc.run_plain(emu, oracle, mode, family)


@pytest.mark.parametrize("mode", MODES)
def test_truncated_streams_decode_like_the_reference(emu, oracle, mode):
    dc.run_truncated(emu, oracle, mode)


@pytest.mark.parametrize("mode", MODES)
def test_random_block_is_given_up_by_the_row_cache_and_decoded_again(emu, oracle, mode):
    dc.run_given_up(emu, oracle, mode)


@pytest.mark.parametrize("part", dc.PARTS)
@pytest.mark.parametrize("mode", MODES)
def test_everything_again_while_whole_waves_sleep(oracle, mode, part):
    """In a subprocess: the scheduler mode is fixed when the library is loaded."""
    code = r'''
import sys, ctypes as C
sys.path[:0] = [%r, %r, %r]
import bzip3_amd, cm_diet_cases as dc
from build_emu import build
from oracle_lib import Oracle
dc.run_part(bzip3_amd._declare(C.CDLL(build())), Oracle(), %d, %r)
print("ok")
''' % (os.path.dirname(HERE), HERE, os.path.join(HERE, "emu"), mode, part)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BZ3_EMU_SCHED="-3"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-300:], r.stderr[-800:])
