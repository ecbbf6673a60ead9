"""CPU tests of the batched forward BWT (bzip3_amd/csrc/bwt.hip bwt_forward_batch: up to four blocks through one launch sequence, every kernel
on a grid of (extent of the job that needs most, job), every launch built from the jobs that need it), with the kernel sources under the
emulator (tests/emu) against the oracle, through bz3_hip_debug_bwt_many -- the way to put chosen inputs into one run -- and through the encoder.

The inputs are datagen.suffix_sorter_cases(), which take these paths (BZ3_BWT_TRACE=1): tile513, n2, n3 and text(70000) are done after pass 0;
phrase1 and group257 need one more window; phrase3 two windows and then rank doubling; mixdeep the same with three doubling rounds; aaaa and fib
overflow a list at pass 0 and go straight to rank doubling; deeprep and allbytes are given up by the tail kernel.  One run holds jobs that all
diverge, so that workgroups beyond a job's own extent, launches for a subset of the jobs and passes beyond a job's own key bits meet under one
grid.  Every job's (index, bytes) must be what oracle.bwt gives for that job alone."""
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
    lib.bz3_hip_debug_bwt_big_rounds(-1)
    lib.bz3_hip_debug_set_bwt_batch(-1)


_JOBS = {}


def _jobs(oracle):
    """name -> (bytes, expected (index, bytes)): computed once, shared by the tests, never changed.  The oracle alone decides `expected`."""
    if _JOBS:
        return _JOBS
    c = datagen.suffix_sorter_cases()
    for name in ("phrase3", "tile513", "aaaa", "phrase1", "deeprep", "n2", "n3", "mixdeep", "group257", "fib", "allbytes"):
        _JOBS[name] = (c[name], None)
    _JOBS["text70000"] = (datagen.text(70000, seed=6), None)
    for name, (b, _) in list(_JOBS.items()):
        _JOBS[name] = (b, oracle.bwt(b))
    return _JOBS


MIXED = ("phrase3", "tile513", "aaaa", "phrase1")  # phrase3 is the largest
MIXED2 = ("deeprep", "n2", "mixdeep", "group257")
ORDERS = {"largest first": (0, 1, 2, 3), "largest last": (1, 2, 3, 0), "largest in the middle": (1, 0, 2, 3)}


def _check(g, jobs, names, what):
    rc, got = g.bwt_many([jobs[k][0] for k in names])
    assert rc == 0, what
    for k, r in zip(names, got):
        assert r == jobs[k][1], (k, what)


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_one_run_of_jobs_that_all_diverge(emu, oracle, order):
    _check(bzip3_amd.StageApi(emu), _jobs(oracle), [MIXED[k] for k in ORDERS[order]], order)


def test_a_second_run_of_jobs_that_diverge(emu, oracle):
    _check(bzip3_amd.StageApi(emu), _jobs(oracle), MIXED2, "second")
    _check(bzip3_amd.StageApi(emu), _jobs(oracle), MIXED2[::-1], "second, reversed")


FIVE = ("text70000", "n2", "fib", "n3", "phrase1")


@pytest.mark.parametrize("count", (1, 2, 3, 4, 5))
def test_runs_of_every_length(emu, oracle, count):
    """Five jobs are a run of four and a run of one."""
    g = bzip3_amd.StageApi(emu)
    _check(g, _jobs(oracle), FIVE[:count], count)
    _check(g, _jobs(oracle), FIVE[::-1][:count], -count)


def test_a_batch_of_one_is_the_stage_hook(emu, oracle):
    g = bzip3_amd.StageApi(emu)
    jobs = _jobs(oracle)
    for name in ("phrase1", "allbytes", "text70000", "n2"):
        b, want = jobs[name]
        rc, got = g.bwt_many([b])
        assert rc == 0 and got[0] == g.bwt(b) == want, name


def test_blocks_of_fewer_than_two_bytes_stay_outside(emu, oracle):
    g = bzip3_amd.StageApi(emu)
    jobs = _jobs(oracle)
    rc, got = g.bwt_many([b"", jobs["n3"][0], b"q", jobs["tile513"][0], b"", jobs["n2"][0]])
    assert rc == 0 and got == [(0, b""), jobs["n3"][1], (1, b"q"), jobs["tile513"][1], (0, b""), jobs["n2"][1]]
    assert g.bwt_many([])[0] == 0 and g.bwt_many([b"", b"z"]) == (0, [(0, b""), (1, b"z")])


@pytest.mark.parametrize("big_rounds", (0, 8))
def test_the_mixed_run_with_other_big_rounds(emu, oracle, big_rounds):
    """0: every big group goes to rank doubling at once; 8: windows until the groups are small (phrase3 then never needs doubling)."""
    emu.bz3_hip_debug_bwt_big_rounds(big_rounds)
    try:
        _check(bzip3_amd.StageApi(emu), _jobs(oracle), MIXED, big_rounds)
    finally:
        emu.bz3_hip_debug_bwt_big_rounds(-1)


@pytest.mark.parametrize("forced", (1, 2, 3))
def test_a_forced_run_length_changes_nothing(emu, oracle, forced):
    emu.bz3_hip_debug_set_bwt_batch(forced)
    try:
        _check(bzip3_amd.StageApi(emu), _jobs(oracle), MIXED, forced)
    finally:
        emu.bz3_hip_debug_set_bwt_batch(-1)


def test_the_mixed_run_under_the_hostile_scheduler(oracle):
    """BZ3_EMU_SCHED: whole waves of a workgroup are held up at random, so the waves of the job-table kernels' workgroups reach their barriers (and
    the early exits in front of them) at wildly different times.  In a subprocess: the scheduler mode is fixed when the library is loaded."""
    jobs = _jobs(oracle)
    code = r'''
import sys, ctypes as C
sys.path[:0] = [%r, %r, %r]
import bzip3_amd
from build_emu import build
g = bzip3_amd.StageApi(bzip3_amd._declare(C.CDLL(build())))
rc, got = g.bwt_many([bytes.fromhex(l) for l in sys.stdin.read().splitlines()])
assert rc == 0
for i, b in got:
    print(i, b.hex())
print("ok")
''' % (os.path.dirname(HERE), HERE, os.path.join(HERE, "emu"))
    feed = "".join("%s\n" % jobs[k][0].hex() for k in MIXED)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BZ3_EMU_SCHED="-5"), input=feed, capture_output=True, text=True, timeout=900)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "ok", (r.stdout[-300:], r.stderr[-800:])
    for k, l in zip(MIXED, lines[:-1]):
        assert (int(l.split()[0]), bytes.fromhex(l.split()[1])) == jobs[k][1], k


# ---- through the encoder: the front end collects a window's blocks and sends them through the sorter in runs ---------------------------------

def _stats(lib, st):
    rounds, passes, elems = C.c_int32(), C.c_int32(), C.c_uint64()
    lib.bz3_hip_last_bwt_stats(st, C.byref(rounds), C.byref(passes), C.byref(elems))
    return rounds.value, passes.value, elems.value


def _encode(lib, blocks, block_sizes):
    """The blocks in ONE bz3_hip_encode_blocks_device call, a state each (under the emulator device memory is host memory).
    [(result, last_error, coded bytes, bwt stats)]."""
    n = len(blocks)
    states = (C.c_void_p * n)(*[lib.bz3_new(bs) for bs in block_sizes])
    assert all(states)
    try:
        bufs = [(C.c_uint8 * (lib.bz3_bound(max(len(d), bs)) + 64))() for d, bs in zip(blocks, block_sizes)]
        for b, d in zip(bufs, blocks):
            C.memmove(b, d, len(d))
        ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
        sizes = (C.c_int32 * n)(*[len(d) for d in blocks])
        lib.bz3_hip_encode_blocks_device(states, ptrs, sizes, n)
        return [(sizes[i], lib.bz3_last_error(states[i]), bytes(bufs[i][: max(0, sizes[i])]), _stats(lib, states[i])) for i in range(n)]
    finally:
        for s in states:
            lib.bz3_free(s)


STORED, RANDOM, OVERSIZE = 2, 4, 6
_TEN = {}


def _ten_blocks(oracle):
    """Ten blocks of 70,000 to 600,000 bytes on every path of the sorter, one stored (40 bytes), one incompressible, one larger than its state's
    block size; and what the oracle makes of each."""
    if not _TEN:
        rng = np.random.default_rng(11)
        c = datagen.suffix_sorter_cases()
        blocks = [datagen.text(70000, seed=21), c["phrase1"], b"x" * 40, datagen.text(600000, seed=22), bytes(rng.integers(0, 256, size=90000, dtype=np.uint8)),
                  c["phrase3"], datagen.text(100000, seed=23), c["mixdeep"][:200000], datagen.text(150000, seed=24), datagen.text(333333, seed=25)]
        sizes = [max(len(b), 65 * 1024) + 1000 for b in blocks]  # (65 KiB: the smallest block size a state takes)
        sizes[OVERSIZE] = 80000
        _TEN["blocks"], _TEN["sizes"] = blocks, sizes
        _TEN["want"] = [oracle.encode_block(b, bs) if i != OVERSIZE else None for i, (b, bs) in enumerate(zip(blocks, sizes))]
    return _TEN["blocks"], _TEN["sizes"], _TEN["want"]


def _check_ten(lib, oracle, got, what):
    blocks, sizes, want = _ten_blocks(oracle)
    for i, (res, err, coded, _) in enumerate(got):
        if i == OVERSIZE:
            assert (res, err) == (-1, bzip3_amd.BZ3_ERR_DATA_TOO_BIG), what
        else:
            assert (res, err, coded) == want[i], (i, what)
    assert got[STORED][0] == 48  # stored: 8 bytes of header


@pytest.mark.parametrize("lean", (0, 1))
def test_ten_blocks_through_the_encoder(emu, oracle, lean):
    """One window, runs of at most four; the stored block, the oversize block (it fails alone) and the incompressible one leave or stay without
    disturbing the runs around them.  Coded bytes against oracle.encode_block; and every state's BwtStats equal to the block's own, encoded alone."""
    blocks, sizes, _ = _ten_blocks(oracle)
    assert emu.bz3_hip_set_lean_states(lean) == 0
    try:
        got = _encode(emu, blocks, sizes)
        _check_ten(emu, oracle, got, lean)
        if lean == 0:
            for i in (0, 1, 5, 7):  # done after pass 0, one more window, windows then doubling, doubling for three rounds
                alone = _encode(emu, [blocks[i]], [sizes[i]])[0]
                assert alone == got[i], i
                assert alone[3][0] >= 1 and alone[3][2] >= len(blocks[i]) // 2
    finally:
        emu.bz3_hip_set_lean_states(0)


def test_ten_blocks_with_the_two_thread_front_end_switched_on(emu, oracle):
    """(A batch this small keeps the one-thread form; tests/test_emu_kernels.py test_two_thread_front_end sends 36 blocks through the two-thread form and
    with it through the runs.)"""
    blocks, sizes, _ = _ten_blocks(oracle)
    assert emu.bz3_hip_set_front_end_duo(1) == 0
    try:
        _check_ten(emu, oracle, _encode(emu, blocks, sizes), "duo")
    finally:
        emu.bz3_hip_set_front_end_duo(-1)
