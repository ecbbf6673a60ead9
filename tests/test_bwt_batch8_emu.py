"""CPU tests of the forward BWT's runs of up to EIGHT blocks (bzip3_amd/csrc/stages.hpp BWT_MAX_BATCH = 8: bwt.hip's job tables, sort.hip's batched
radix and scan tables, the encoder's windows of eight going through the sorter as one run), with the kernel sources under the emulator (tests/emu)
against the oracle -- in the manner of tests/test_bwt_batch_emu.py, which covers runs of up to four.

The nine jobs (tests/bwt_batch8_cases.py) in one bz3_hip_debug_bwt_many call are a run of eight and a run of one; they take different paths of the
sorter (done after pass 0, one more window, rank doubling over several rounds), so launches for a subset of eight jobs, workgroups beyond a job's
own extent and passes beyond a job's own key bits meet under one grid of (extent of the largest, 8)."""
import ctypes as C
import hashlib
import os
import struct
import subprocess
import sys

import pytest

import bwt_batch8_cases as cases
import bzip3_amd
import datagen

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    lib = bzip3_amd._declare(C.CDLL(build()))
    yield lib
    lib.bz3_hip_debug_set_bwt_batch(-1)
    lib.bz3_hip_set_lean_states(0)


@pytest.mark.parametrize("rotate", (0, 3))
def test_nine_jobs_are_a_run_of_eight_and_a_run_of_one(emu, oracle, rotate):
    cases.check_nine(bzip3_amd.StageApi(emu), oracle, cases.rotated(cases.nine_jobs(), rotate), rotate)


@pytest.mark.parametrize("forced", (5, 7, 8))
def test_forced_run_lengths(emu, oracle, forced):
    """5: runs of five and four; 7: seven and two; 8: what the rule gives these sizes."""
    emu.bz3_hip_debug_set_bwt_batch(forced)
    try:
        cases.check_nine(bzip3_amd.StageApi(emu), oracle, cases.nine_jobs(), forced)
    finally:
        emu.bz3_hip_debug_set_bwt_batch(-1)


def test_the_forced_run_length_is_clamped_to_eight(emu, oracle):
    emu.bz3_hip_debug_set_bwt_batch(9)
    try:
        cases.check_nine(bzip3_amd.StageApi(emu), oracle, cases.nine_jobs()[:4] + cases.nine_jobs()[:4] + cases.nine_jobs()[:2], "clamped")
    finally:
        emu.bz3_hip_debug_set_bwt_batch(-1)


def test_empty_and_one_byte_blocks_between_jobs(emu, oracle):
    """Blocks of fewer than two bytes never enter a run: the nine jobs with such blocks between them are still a run of eight and a run of one."""
    want = cases.nine_expected(oracle)
    jobs = cases.nine_jobs()
    blocks, expect = [], []
    for k, (name, b) in enumerate(jobs):
        if k % 3 == 0:
            blocks.append(b"")
            expect.append((0, b""))
        if k % 4 == 1:
            blocks.append(b"z")
            expect.append((1, b"z"))
        blocks.append(b)
        expect.append(want[name])
    blocks.append(b"")
    expect.append((0, b""))
    rc, got = bzip3_amd.StageApi(emu).bwt_many(blocks)
    assert rc == 0 and got == expect


_TWENTY = {}


def _twenty_blocks(oracle):
    """20 blocks of 20 to 50 KB (the emulator's pace): text, the deep path (a period-7 string), random bytes, a stored block in the middle of a window."""
    if not _TWENTY:
        jobs = dict(cases.nine_jobs())
        blocks = []
        for k in range(20):
            if k == 5:
                blocks.append(b"y" * 33)
            elif k % 7 == 3:
                blocks.append(jobs["period7"][: 24000 + k])
            elif k % 7 == 6:
                blocks.append(jobs["random50k"][: 30000 + k])
            else:
                blocks.append(datagen.text(20000 + 1501 * k, seed=40 + k))
        bs = 65 * 1024
        _TWENTY["v"] = (blocks, bs, [oracle.encode_block(b, bs) for b in blocks])
    return _TWENTY["v"]


@pytest.mark.parametrize("lean", (0, 1), ids=("classic", "lean"))
def test_twenty_blocks_through_the_encoder_in_runs_of_eight(emu, oracle, lean):
    """bz3_encode_blocks, the run length forced to 8: windows of eight blocks are one run each (the window with the stored block a run of seven), the
    last window a run of four.  Coded bytes against oracle.encode_block."""
    blocks, bs, want = _twenty_blocks(oracle)
    n = len(blocks)
    assert emu.bz3_hip_set_lean_states(lean) == 0
    emu.bz3_hip_debug_set_bwt_batch(8)
    states = (C.c_void_p * n)(*[emu.bz3_new(bs) for _ in range(n)])
    try:
        assert all(states)
        cap = emu.bz3_bound(bs) + 64
        bufs = [(C.c_uint8 * cap)() for _ in range(n)]
        for b, d in zip(bufs, blocks):
            C.memmove(b, d, len(d))
        ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
        sizes = (C.c_int32 * n)(*[len(d) for d in blocks])
        emu.bz3_encode_blocks(states, ptrs, sizes, n)
        assert emu.bz3_hip_debug_front_end_ring() & 0xFFFF == 8  # windows of eight
        for k in range(n):
            assert (sizes[k], emu.bz3_last_error(states[k]), bytes(bufs[k][: max(0, sizes[k])])) == want[k], (lean, k)
    finally:
        for s in states:
            emu.bz3_free(s)
        emu.bz3_hip_debug_set_bwt_batch(-1)
        emu.bz3_hip_set_lean_states(0)


def _build_sanitized_program():
    """The emulator build of every kernel source and tests/emu/bwt_batch8_main.cpp with -fsanitize=address,undefined, kept under tests/emu/build_asan8/
    until a source changes."""
    out = os.path.join(HERE, "emu", "build_asan8")
    os.makedirs(out, exist_ok=True)
    csrc = os.path.join(ROOT, "bzip3_amd", "csrc")
    srcs = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hip")) + [os.path.join(HERE, "emu", "hip_emu.cpp"), os.path.join(HERE, "emu", "bwt_batch8_main.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")] + [os.path.join(HERE, "emu", "hip_emu.hpp")]
    deps += [os.path.join(ROOT, "include", f) for f in os.listdir(os.path.join(ROOT, "include"))]
    flags = ["-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-DBZ3_EMU", "-DBZ3_EMU_API_UNITS", "-I", os.path.join(HERE, "emu"), "-I", csrc,
             "-Wno-unknown-pragmas", "-Wno-attributes"]
    h = hashlib.sha256(" ".join(flags).encode())
    for p in sorted(deps):
        h.update(open(p, "rb").read())
    exe, stamp = os.path.join(out, "bwt_batch8"), os.path.join(out, "bwt_batch8.sha")
    if os.path.exists(exe) and os.path.exists(stamp) and open(stamp).read() == h.hexdigest():
        return exe
    objs, procs = [], []
    for s in srcs:
        o = os.path.join(out, os.path.basename(s) + ".o")
        objs.append(o)
        procs.append((s, subprocess.Popen(["g++", *flags, "-x", "c++", "-c", s, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for s, p in procs:
        log, _ = p.communicate()
        assert p.returncode == 0, (s, log[-2000:])
    subprocess.check_call(["g++", *flags, *objs, "-lpthread", "-o", exe])
    open(stamp, "w").write(h.hexdigest())
    return exe


def test_the_nine_jobs_under_the_sanitizers(oracle, tmp_path):
    """The nine jobs in one call through the emulator build compiled with AddressSanitizer and UndefinedBehaviorSanitizer, in a stand-alone program run as a
    child process: no report, nothing written beyond a job, and every job's (index, bytes) the oracle's.  (The compile and the slow run are what this test is
    about: about a minute each.)"""
    exe = _build_sanitized_program()
    jobs = cases.nine_jobs()
    want = cases.nine_expected(oracle)
    src, dst = tmp_path / "jobs.bin", tmp_path / "results.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(jobs)))
        for _, b in jobs:
            f.write(struct.pack("<I", len(b)) + b)
    r = subprocess.run([exe, str(src), str(dst)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"),
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and r.stdout.strip().endswith("bwt batch8 ok") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout[-300:], r.stderr[-3000:])
    got = open(dst, "rb").read()
    at = 0
    for name, b in jobs:
        idx = struct.unpack_from("<i", got, at)[0]
        assert (idx, got[at + 4 : at + 4 + len(b)]) == want[name], name
        at += 4 + len(b)
    assert at == len(got)
