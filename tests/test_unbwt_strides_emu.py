"""CPU tests of the inverse BWT's splitter stride and host-side splitter bound (bzip3_amd/csrc/unbwt.hip), with the kernel
sources under the emulator (tests/emu) against the oracle.  (The list ranking ships with one hop per round: wider rounds were measured and left out.)

The sizes: 70,000 rows is below 2^17 (every row is a splitter under the rule); 140,000 is just above it (the rule's smallest stride);
600,000 is where a stride of 256 still leaves some 2,300 segments, enough for several to outgrow their slab (k_ub_walk_long) and for the
last slab word of most to be partial.  Forced strides 0 to 8 cover every stride the rule can pick and the ones it cannot."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import bzip3_amd
import datagen

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (70000, 140000, 600000)
STRIDES = tuple(range(0, 9))


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    lib = bzip3_amd._declare(C.CDLL(build()))
    yield lib
    lib.bz3_hip_debug_set_unbwt_log_stride(-1)


_INPUTS = {}


def _inputs(oracle, n):
    """(name, bytes, index, expected) for one size: computed once, shared by the tests, never changed.  The oracle alone decides `expected`."""
    if n in _INPUTS:
        return _INPUTS[n]
    rng = np.random.default_rng(1000 + n)
    out = []
    text = datagen.text(n, seed=5)
    idx, u = oracle.bwt(text)
    out.append(("text", u, idx))
    wrong = idx // 2 + 1 if idx // 2 + 1 != idx else idx // 2 + 2
    out.append(("text, wrong index", u, wrong))
    one = b"a" * n
    idx1, u1 = oracle.bwt(one)
    out.append(("one repeated byte", u1, idx1))  # psi is sequential: every segment has the same length
    for k in (1, 2, 5, 256):
        junk = bytes(rng.integers(0, k, size=n, dtype=np.uint8))
        out.append((f"junk over {k} symbols", junk, int(rng.integers(1, n + 1))))
    res = [(name, u, i, oracle.unbwt(u, i)) for name, u, i in out]
    assert res[0][3] == (0, text) and res[2][3] == (0, one)
    _INPUTS[n] = res
    return res


@pytest.mark.parametrize("log_stride", STRIDES)
@pytest.mark.parametrize("n", SIZES)
def test_forced_strides_match_the_oracle(emu, oracle, n, log_stride):
    g = bzip3_amd.StageApi(emu)
    emu.bz3_hip_debug_set_unbwt_log_stride(log_stride)
    try:
        for name, u, idx, want in _inputs(oracle, n):
            assert g.unbwt(u, idx) == want, (name, n, log_stride, idx)
    finally:
        emu.bz3_hip_debug_set_unbwt_log_stride(-1)


@pytest.mark.parametrize("n", SIZES)
def test_the_rule_matches_the_oracle(emu, oracle, n):
    g = bzip3_amd.StageApi(emu)
    emu.bz3_hip_debug_set_unbwt_log_stride(-1)
    for name, u, idx, want in _inputs(oracle, n):
        assert g.unbwt(u, idx) == want, (name, n, idx)


MARGIN = 64  # UB_BOUND_MARGIN


def _bound(rows, log_stride):  # ub_split_bound of unbwt.hip
    return min(rows, (rows >> log_stride) + 2 + MARGIN)


def _hashed_counts(rows):
    """Exact number of rows in [0, rows) that the hash makes a splitter, for log_stride 3..8, and one such row above 1."""
    counts = {ls: 0 for ls in range(3, 9)}
    hashed_row = None
    step = 1 << 24
    for a in range(0, rows, step):
        r = np.arange(a, min(rows, a + step), dtype=np.uint64)
        h = (r * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
        for ls in counts:
            hit = h < np.uint64(1 << (32 - ls))
            counts[ls] += int(np.count_nonzero(hit))
            if ls == 8 and hashed_row is None:
                w = np.flatnonzero(hit)
                w = w[w + a > 1]
                if len(w):
                    hashed_row = int(w[0]) + a  # a splitter at stride 256 is one at every smaller stride
    return counts, hashed_row


@pytest.mark.parametrize("rows", [(1 << 17) + 1, 140001, 1 << 20, (1 << 23) - 1, (1 << 23) + 1, 7900000, 33000000, (1 << 27) + 1])
def test_the_host_side_splitter_bound(rows):
    counts, hashed_row = _hashed_counts(rows)
    assert hashed_row is not None and 1 < hashed_row < rows
    for ls, hashed in counts.items():
        assert abs(hashed - (rows >> ls)) <= 3, (rows, ls, hashed)  # what the comment next to ub_is_splitter states
        for idx in (1, rows - 1, hashed_row):
            h = (idx * 0x9E3779B1) & 0xFFFFFFFF
            total = hashed + (0 if (h >> (32 - ls)) == 0 else 1)  # row 0 hashes to 0: always counted already
            assert total <= _bound(rows, ls) - (MARGIN - 4), (rows, ls, idx, total)  # at most 4 of the margin's 64 entries are ever needed
