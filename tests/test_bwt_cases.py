"""CPU tests of the suffix sorter's adversarial cases (tests/bwt_cases.py): the kernel sources of bwt.hip and sort.hip under the emulator (tests/emu).
Every case is compared with the oracle, its code table with the optimum of an independent dynamic programme, its record (bz3_hip_debug_bwt_record) with
the model, and the precondition the case is named for is asserted from both -- nothing is skipped: a case whose precondition fails is a failure."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import bwt_cases as cases
import bzip3_amd

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    lib = bzip3_amd._declare(C.CDLL(build()))
    yield bzip3_amd.StageApi(lib)
    lib.bz3_hip_debug_bwt_big_rounds(-1)
    lib.bz3_hip_debug_set_bwt_batch(-1)


def test_the_record_carries_the_geometry_and_needs_its_size(emu):
    geo = cases.geometry(emu)
    assert all(geo[k] > 0 for k in geo if k != "big_cap") and geo["TL_GROUP"] < geo["WR_G"] < geo["WR_A"]
    rec = (C.c_uint32 * 8)()
    idx = C.c_int32()
    out = (C.c_uint8 * 2)()
    assert emu.lib.bz3_hip_debug_bwt_record(bzip3_amd._cbuf(b"ab", 2), 2, out, C.byref(idx), rec, 8) == -2 and rec[0] > 8
    for data in (b"", b"z"):  # blocks that never enter a run: the geometry alone
        i, o, r = emu.bwt_record(data)
        assert (i, o) == (len(data), data) and r["passes"] == () and r["geo"]["WR_A"] == geo["WR_A"]


def test_the_height_limited_optimum_against_brute_force():
    """The test's own dynamic programme against the definition, on alphabets small enough to enumerate every alphabetic tree."""
    def brute(w, h):
        if len(w) == 1:
            return 0
        if h == 0:
            return None
        best = None
        for k in range(1, len(w)):
            a, b = brute(w[:k], h - 1), brute(w[k:], h - 1)
            if a is not None and b is not None and (best is None or a + b < best):
                best = a + b
        return None if best is None else best + sum(w)
    for w, h in (((5, 1, 1, 1, 9), 3), ((1, 2, 3, 5, 8, 13, 21), 3), ((1, 2, 3, 5, 8, 13, 21), 6), ((4, 4, 4), 2), ((7, 1, 1, 7, 1, 1, 7, 2), 3)):
        assert cases.optimum(w, h) == brute(w, h), (w, h)


@pytest.mark.parametrize("name", cases.ALL)
def test_case(emu, oracle, name):
    cases.run_case(emu, oracle, name)


def test_a_group_across_two_spine_groups(emu, oracle):
    """560 KB under the emulator (some 15 s): the one case whose size the geometry dictates -- more than SP_GROUP anchor tiles."""
    cases.run_case(emu, oracle, "group_carry")


@pytest.mark.parametrize("rotate", (0, 3))
def test_a_run_of_eight(emu, oracle, rotate):
    cases.run_batch(emu, oracle, rotate)


@pytest.mark.parametrize("rounds", (0, 8))
@pytest.mark.parametrize("name", cases.BIG_ROUNDS_CASES)
def test_other_big_rounds(emu, oracle, name, rounds):
    emu.lib.bz3_hip_debug_bwt_big_rounds(rounds)
    try:
        _, rec = cases.run_case(emu, oracle, name)
        assert rec["big_rounds"] == rounds
    finally:
        emu.lib.bz3_hip_debug_bwt_big_rounds(-1)


@pytest.mark.parametrize("sched", ("-5", "7"), ids=("stalled_waves", "hostile"))
def test_a_routing_and_a_deep_case_under_the_other_schedulers(oracle, sched):
    """BZ3_EMU_SCHED: whole waves held up at random (negative: for long).  In a subprocess: the scheduler is fixed when the library is loaded."""
    code = r'''
import sys, ctypes as C
sys.path[:0] = [%r, %r, %r]
import bzip3_amd, bwt_cases as cases
from build_emu import build
from oracle_lib import Oracle
g = bzip3_amd.StageApi(bzip3_amd._declare(C.CDLL(build())))
o = Oracle()
for name in ("head257_at511", "residues64", "period7_2049", "nothing_active"):
    cases.run_case(g, o, name)
print("ok")
''' % (os.path.dirname(HERE), HERE, os.path.join(HERE, "emu"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BZ3_EMU_SCHED=sched), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-300:], r.stderr[-1500:])
