"""CPU tests of the batched inverse BWT (bzip3_amd/csrc/unbwt.hip bwt_inverse_batch: up to four blocks through one launch sequence, every kernel on
a grid of (extent of the largest job, job)), with the kernel sources under the emulator (tests/emu) against the oracle, through
bz3_hip_debug_unbwt_many -- the way to put chosen sizes into one batch.

The sizes are those of tests/test_unbwt_strides_emu.py, which explains them (70,000 rows: every row a splitter; 140,000: the rule's smallest
stride; 600,000: segments outgrow their slabs and the last slab words are partial), and the smallest jobs that enter a batch, n = 3 and n = 2.
One run holds jobs of different sizes and kinds, so that workgroups beyond a job's own extent, rounds beyond a job's own list and both stride
regimes meet under one grid; the orders put the largest job first, last and in the middle.  Every job's bytes must be what oracle.unbwt gives
for that job alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bzip3_amd
import datagen

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    lib = bzip3_amd._declare(C.CDLL(build()))
    yield lib
    lib.bz3_hip_debug_set_unbwt_log_stride(-1)


_JOBS = {}


def _jobs(oracle):
    """name -> (bytes, index, expected): computed once, shared by the tests, never changed.  The oracle alone decides `expected`."""
    if _JOBS:
        return _JOBS
    rng = np.random.default_rng(77)
    big = datagen.text(600000, seed=5)
    idx, u = oracle.bwt(big)
    _JOBS["text 600000"] = (u, idx)
    t70 = datagen.text(70000, seed=6)
    idx70, u70 = oracle.bwt(t70)
    _JOBS["text 70000, wrong index"] = (u70, idx70 // 2 + 1 if idx70 // 2 + 1 != idx70 else idx70 // 2 + 2)
    _JOBS["junk 140000 over 2 symbols"] = (bytes(rng.integers(0, 2, size=140000, dtype=np.uint8)), int(rng.integers(1, 140001)))
    idx3, u3 = oracle.bwt(b"abc")
    _JOBS["text 3"] = (u3, idx3)
    idx2, u2 = oracle.bwt(b"ba")
    _JOBS["text 2"] = (u2, idx2)
    for name, (b, i) in list(_JOBS.items()):
        _JOBS[name] = (b, i, oracle.unbwt(b, i))
    assert _JOBS["text 600000"][2] == (0, big) and _JOBS["text 3"][2] == (0, b"abc") and _JOBS["text 2"][2] == (0, b"ba")
    return _JOBS


MIXED = ("text 600000", "text 3", "junk 140000 over 2 symbols", "text 70000, wrong index")
ORDERS = {"largest first": (0, 1, 2, 3), "largest last": (1, 2, 3, 0), "largest in the middle": (1, 0, 2, 3)}


def _check(g, jobs, names, what):
    rc, got = g.unbwt_many([(jobs[k][0], jobs[k][1]) for k in names])
    assert rc == 0, what
    for k, b in zip(names, got):
        assert (0, b) == jobs[k][2], (k, what)


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("log_stride", (-1, 0, 3, 8))
def test_one_run_of_different_jobs(emu, oracle, log_stride, order):
    g = bzip3_amd.StageApi(emu)
    emu.bz3_hip_debug_set_unbwt_log_stride(log_stride)
    try:
        _check(g, _jobs(oracle), [MIXED[k] for k in ORDERS[order]], (log_stride, order))
    finally:
        emu.bz3_hip_debug_set_unbwt_log_stride(-1)


FIVE = ("text 70000, wrong index", "text 2", "junk 140000 over 2 symbols", "text 3", "text 600000")


@pytest.mark.parametrize("count", (1, 2, 3, 4, 5))
def test_runs_of_every_length(emu, oracle, count):
    """Five jobs are a run of four and a run of one."""
    g = bzip3_amd.StageApi(emu)
    emu.bz3_hip_debug_set_unbwt_log_stride(-1)
    _check(g, _jobs(oracle), FIVE[:count], count)
    _check(g, _jobs(oracle), FIVE[::-1][:count], -count)


@pytest.mark.parametrize("log_stride", (-1, 0, 3, 8))
def test_a_batch_of_one_is_the_stage_hook(emu, oracle, log_stride):
    g = bzip3_amd.StageApi(emu)
    jobs = _jobs(oracle)
    emu.bz3_hip_debug_set_unbwt_log_stride(log_stride)
    try:
        for name in ("text 600000", "text 70000, wrong index", "text 2"):
            b, i, want = jobs[name]
            rc, got = g.unbwt_many([(b, i)])
            assert (rc, got[0]) == g.unbwt(b, i) == want, (name, log_stride)
    finally:
        emu.bz3_hip_debug_set_unbwt_log_stride(-1)


def test_blocks_of_fewer_than_two_bytes_stay_outside(emu, oracle):
    g = bzip3_amd.StageApi(emu)
    jobs = _jobs(oracle)
    b, i, want = jobs["text 3"]
    rc, got = g.unbwt_many([(b"", 0), (b, i), (b"q", 1), (jobs["text 2"][0], jobs["text 2"][1])])
    assert rc == 0 and got == [b"", want[1], b"q", jobs["text 2"][2][1]]
    assert g.unbwt_many([(b, 0)])[0] == -1 and g.unbwt_many([(b, 4)])[0] == -1 and g.unbwt_many([(b"q", 0)])[0] == -1
    assert g.unbwt_many([])[0] == 0


def test_the_mixed_run_under_the_hostile_scheduler(oracle):
    """BZ3_EMU_SCHED: whole waves of a workgroup are held up at random, so the waves of the batched kernels' workgroups reach their barriers (and
    the early exits in front of them) at wildly different times.  In a subprocess: the scheduler mode is fixed when the library is loaded."""
    jobs = _jobs(oracle)
    names = [MIXED[k] for k in ORDERS["largest in the middle"]]
    code = r'''
import sys, ctypes as C
sys.path[:0] = [%r, %r, %r]
import bzip3_amd
from build_emu import build
g = bzip3_amd.StageApi(bzip3_amd._declare(C.CDLL(build())))
jobs = [(bytes.fromhex(l.split()[0]) if l.split()[0] != "-" else b"", int(l.split()[1])) for l in sys.stdin.read().splitlines()]
rc, got = g.unbwt_many(jobs)
assert rc == 0
for b in got:
    print(b.hex() or "-")
print("ok")
''' % (os.path.dirname(HERE), HERE, os.path.join(HERE, "emu"))
    feed = "".join("%s %d\n" % (jobs[k][0].hex(), jobs[k][1]) for k in names)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BZ3_EMU_SCHED="-5"), input=feed, capture_output=True, text=True, timeout=600)
    lines = r.stdout.split()
    assert r.returncode == 0 and lines and lines[-1] == "ok", (r.stdout[-300:], r.stderr[-800:])
    for k, h in zip(names, lines[:-1]):
        assert (0, bytes.fromhex(h)) == jobs[k][2], k
