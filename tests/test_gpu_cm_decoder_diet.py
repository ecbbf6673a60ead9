"""-m gpu: the per-byte paths of the guess-ahead CM decoder on hardware, where the builtin and inline-assembly forms run that the emulator replaces by C
(tests/test_cm_decoder_diet_emu.py).  The inputs of tests/cm_diet_cases.py through bz3_hip_stage_cm_decode_many with 1 and 3 copies of the block in one
launch and the variant forced (full model, two- and three-per-CU row caches); expected bytes: the oracle's.  The uniformly random block goes through the
single-job hook, which hands a given-up block to the full-model kernel (decode_many measures a variant alone and hands nothing back)."""
import ctypes as C

import numpy as np
import pytest

import bzip3_amd
import cm_diet_cases as dc

pytestmark = pytest.mark.gpu
MODES = {"full": 0, "rows": 1, "rows3": 2}
_coded = {}


def _cases(oracle):
    """[(name, coded stream, n, expected bytes)], built once: one oracle call per block."""
    if not _coded:
        out = []
        for family in dc.FAMILIES:
            for name, d in dc.plain_families(True)[family].items():
                out.append((name, oracle.cm_encode(d), len(d), d))
        for stream, n, want in dc.truncated_streams(oracle):
            out.append(("truncated_at%d" % len(stream), stream, n, want))
        _coded["all"] = out
    return _coded["all"]


def _decode_many(lib, stream, n, copies, counters=None):
    out = (C.c_uint8 * max(1, n))()
    ms = lib.bz3_hip_stage_cm_decode_many(bzip3_amd._cbuf(stream, len(stream)), len(stream), out, n, copies, counters)
    return ms, bytes(out)[:n]


def test_preconditions(oracle):
    dc.check_preconditions(oracle)


@pytest.mark.parametrize("copies", [1, 3])
@pytest.mark.parametrize("mode", list(MODES))
def test_every_input_through_one_launch_of_the_forced_variant(gpu_lib, oracle, monkeypatch, mode, copies):
    monkeypatch.setenv("BZ3_CM_MANY_CHECK", "1")   # every copy must agree with copy 0 (-2 otherwise)
    monkeypatch.delenv("BZ3_CM_DEBUG", raising=False)
    try:
        assert gpu_lib.bz3_hip_bind_device(0) == 0 and gpu_lib.bz3_hip_set_cm_mode(MODES[mode]) == 0
        assert gpu_lib.bz3_hip_cm_variant_for(0, copies, 0) == MODES[mode]
        for name, stream, n, want in _cases(oracle):
            ms, got = _decode_many(gpu_lib, stream, n, copies)
            assert ms >= 0, (name, mode, copies, ms)
            assert got == want, (name, mode, copies)
    finally:
        gpu_lib.bz3_hip_set_cm_mode(-1)
        gpu_lib.bz3_hip_bind_device(-1)


@pytest.mark.parametrize("mode", list(MODES))
def test_random_block_is_given_up_by_the_row_cache_and_decoded_again(gpu_lib, oracle, mode):
    try:
        assert gpu_lib.bz3_hip_bind_device(0) == 0
        dc.run_given_up(gpu_lib, oracle, MODES[mode])
    finally:
        gpu_lib.bz3_hip_bind_device(-1)


@pytest.mark.parametrize("mode", list(MODES))
def test_profiling_instantiation_fills_its_counters(gpu_lib, oracle, monkeypatch, mode):
    """BZ3_CM_DEBUG=3 on the 64 KiB block: the walker's and model wave 1's cycle counters are non-zero, and the walker counts n - 1 guesses, right plus wrong
    (every byte but the last is handed over and met at barrier 1).  The guesses are counted by the walker alone: a counter of their own in the model waves
    changes the code the compiler makes of the kernels WITHOUT counters."""
    d = dc.plain_families(True)["rows"]["rows70_64k"]
    n = len(d)
    stream = next(c for name, c, _, _ in _cases(oracle) if name == "rows70_64k")
    monkeypatch.setenv("BZ3_CM_DEBUG", "3")
    try:
        assert gpu_lib.bz3_hip_bind_device(0) == 0 and gpu_lib.bz3_hip_set_cm_mode(MODES[mode]) == 0
        cnt = (C.c_uint64 * 16)()
        ms, got = _decode_many(gpu_lib, stream, n, 1, cnt)
        assert ms >= 0
        a = np.frombuffer(cnt, dtype=np.uint64).astype(np.int64)
        print(mode, "walker wait, walk, slow, wrong, wait behind wrong, right:", a[:6].tolist(), "model speculate, wait, redo:", a[8:11].tolist())
        assert a[0] > 0 and a[1] > 0, a[:2]                      # walker: wait, walk
        assert a[8] > 0 and a[9] > 0 and a[10] > 0, a[8:11]      # model wave 1: speculate, wait, redo
        assert a[3] > 0 and a[5] > 0 and a[3] + a[5] == n - 1, (a[3], a[5], n)   # walker: wrong + right guesses
        assert got[128:] == d[128:]   # behind the counters (the first 128 bytes of the output) the decoded bytes are there
    finally:
        gpu_lib.bz3_hip_set_cm_mode(-1)
        gpu_lib.bz3_hip_bind_device(-1)
