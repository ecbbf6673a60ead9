"""GPU tests of the encoder's front end at small blocks: the forward BWT's runs of up to eight blocks (bwt.hip bwt_forward_batch with BWT_MAX_BATCH = 8) on
real grids of (extent of the largest job, 8), alone and under the encoder's windows of eight, with the one-thread and the two-thread front end.  The oracle
decides every expected byte (tests/bwt_batch8_cases.py builds the inputs once)."""
import ctypes as C

import pytest

import bwt_batch8_cases as cases
import bzip3_amd

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rotate", (0, 3))
def test_nine_jobs_are_a_run_of_eight_and_a_run_of_one(gpu_lib, oracle, rotate):
    """(a) 2 bytes to 300 KB, done after pass 0 / one more window / rank doubling, in one bz3_hip_debug_bwt_many call; and rotated by three positions, so that
    another job is the run of one and the largest sits elsewhere in the table."""
    try:
        cases.check_nine(bzip3_amd.StageApi(gpu_lib), oracle, cases.rotated(cases.nine_jobs(), rotate), rotate)
    finally:
        gpu_lib.bz3_hip_release_cached_memory()


def _round_trips(gpu_lib, oracle, text):
    """(b) 40 blocks of 64 KiB to 1 MiB in ONE batch, three encode + decode calls in a row, classic and lean states, with the library's defaults (one host
    thread) and with the two-thread front end forced on: bit 29 of bz3_hip_debug_front_end_ring() reports the form that ran, the coded bytes are the
    oracle's in both cases, and decoding gives the plaintext back."""
    blocks, bs, want = cases.forty_blocks(oracle, text)
    n = len(blocks)
    cap = gpu_lib.bz3_bound(bs) + 64
    shapes = set()
    try:
        for lean in (0, 1):
            assert gpu_lib.bz3_hip_set_lean_states(lean) == 0
            states = (C.c_void_p * n)(*[gpu_lib.bz3_new(bs) for _ in range(n)])
            assert all(states)
            try:
                for switch in (-1, 1):
                    assert gpu_lib.bz3_hip_set_front_end_duo(switch) == 0
                    for trip in range(3):
                        bufs = [(C.c_uint8 * cap)() for _ in range(n)]
                        for b, d in zip(bufs, blocks):
                            C.memmove(b, d, len(d))
                        ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
                        sizes = (C.c_int32 * n)(*[len(d) for d in blocks])
                        gpu_lib.bz3_encode_blocks(states, ptrs, sizes, n)
                        ring = gpu_lib.bz3_hip_debug_front_end_ring()
                        window, slots = ring & 0xFFFF, (ring >> 16) & 0xFF
                        shapes.add((window, slots))
                        windows = (n + window - 1) // window
                        # forced on, the form runs where there are windows to run ahead by; it is off by default
                        assert (ring >> 29) & 1 == (1 if switch == 1 and windows >= 3 else 0), (lean, switch, trip, ring)
                        for k in range(n):
                            assert bytes(bufs[k][: max(0, sizes[k])]) == want[k], (lean, switch, trip, k)
                        bsz = (C.c_size_t * n)(*[cap] * n)
                        orig = (C.c_int32 * n)(*[len(d) for d in blocks])
                        gpu_lib.bz3_decode_blocks(states, ptrs, bsz, sizes, orig, n)
                        for k, d in enumerate(blocks):
                            assert gpu_lib.bz3_last_error(states[k]) == 0 and bytes(bufs[k][: len(d)]) == d, (lean, switch, trip, k)
            finally:
                for s_ in states:
                    gpu_lib.bz3_free(s_)
    finally:
        gpu_lib.bz3_hip_set_front_end_duo(-1)
        gpu_lib.bz3_hip_set_lean_states(0)
        gpu_lib.bz3_hip_release_cached_memory()
    return shapes


def test_forty_small_blocks_in_windows_of_eight(gpu_lib, oracle, text, monkeypatch):
    monkeypatch.delenv("BZ3_HIP_LZP_PIPE", raising=False)
    assert _round_trips(gpu_lib, oracle, text) == {(8, 4)}  # five windows, each one run of the sorter (the stored blocks apart)


def test_forty_small_blocks_in_windows_of_three(gpu_lib, oracle, text, monkeypatch):
    """(c) BZ3_HIP_LZP_PIPE="3,4": fourteen windows of three, ragged runs (a window is one run of three, of two beside a stored block, the last window of one)."""
    monkeypatch.setenv("BZ3_HIP_LZP_PIPE", "3,4")
    assert _round_trips(gpu_lib, oracle, text) == {(3, 4)}
