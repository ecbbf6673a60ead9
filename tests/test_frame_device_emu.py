"""CPU tests of the device-resident frame API (include/bz3_hip.h bz3_hip_compress_device / bz3_hip_decompress_device /
bz3_hip_frame_decoded_size_device, the segment copy kernel of bzip3_amd/csrc/frame.hpp) under the fiber emulation of the HIP
execution model (tests/emu): emulated device memory is host memory, so ctypes buffers serve as device buffers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import bzip3_amd
import frame_cases

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = (0, 1, 15, 16, 17, 31, 4095, 4097)


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    return bzip3_amd._declare(C.CDLL(build()))


class DeviceFrames:
    """libbz3.h's frame API as frame_cases.check calls it, backed by the two device entry points (pointers pass straight through)."""

    def __init__(self, lib):
        self.lib = lib
        self.bz3_bound = lib.bz3_bound

    def bz3_compress(self, bs, data, out, n, osz):
        return self.lib.bz3_hip_compress_device(bs, data, out, n, osz)

    def bz3_decompress(self, frame, out, n, osz):
        return self.lib.bz3_hip_decompress_device(frame, out, n, osz)


def _copy_case(lib, rng, segs_spec, src_len, dst_len):
    """segs_spec: (src alignment mod 16, dst alignment mod 16, length) per segment, laid out one after the other with gaps; one launch."""
    src = (C.c_uint8 * (src_len + 64))()
    dst = (C.c_uint8 * (dst_len + 64))()
    src_np = np.frombuffer(src, dtype=np.uint8)
    dst_np = np.frombuffer(dst, dtype=np.uint8)
    src_np[:] = rng.integers(0, 256, size=src_np.size, dtype=np.uint8)
    dst_np[:] = 0xA5
    want = dst_np.copy()
    sa, da = C.addressof(src), C.addressof(dst)
    table, s_off, d_off = [], 0, 0
    for a_s, a_d, n in segs_spec:
        s_off += (a_s - (sa + s_off)) % 16
        d_off += (a_d - (da + d_off)) % 16
        assert (sa + s_off) % 16 == a_s and (da + d_off) % 16 == a_d
        table += [s_off, d_off, n]
        want[d_off : d_off + n] = src_np[s_off : s_off + n]
        s_off += n + int(rng.integers(0, 40))
        d_off += n + int(rng.integers(1, 40))  # at least one untouched byte between destination segments
    assert s_off <= src_len + 64 - 16 and d_off <= dst_len + 64 - 16
    t = (C.c_uint64 * max(1, len(table)))(*table)
    assert lib.bz3_hip_debug_copy_segments(src, dst, t, len(table) // 3) == 0
    bad = np.nonzero(dst_np != want)[0]
    assert bad.size == 0, ("bytes differ at", bad[:8], segs_spec[:4])


def copy_sweep(lib, rng, budget_big=4):
    """Every source x destination alignment mod 16 at the edge lengths, one launch per length; random lengths up to ~200 KB."""
    for n in LENGTHS:
        spec = [(a, b, n) for a in range(16) for b in range(16)]
        room = 256 * (n + 80)
        _copy_case(lib, rng, spec, room, room)
    spec = [(int(rng.integers(0, 16)), int(rng.integers(0, 16)), int(rng.integers(0, 200_000))) for _ in range(budget_big)]
    spec += [(int(rng.integers(0, 16)), int(rng.integers(0, 16)), int(rng.integers(0, 300))) for _ in range(40)]
    room = sum(n for _, _, n in spec) + 80 * len(spec)
    _copy_case(lib, rng, spec, room, room)


def test_copy_segments_every_alignment_and_length(emu):
    copy_sweep(emu, np.random.default_rng(11))


def test_copy_segments_rejects_bad_arguments(emu):
    buf = (C.c_uint8 * 64)()
    assert emu.bz3_hip_debug_copy_segments(buf, buf, None, -1) == bzip3_amd.BZ3_ERR_INIT
    assert emu.bz3_hip_debug_copy_segments(buf, buf, None, 0) == 0


def _five(bs):
    rng = np.random.default_rng(4)
    unit = bytes(rng.integers(0, 256, size=997, dtype=np.uint8))  # repetitive: LZP collapses it, so the emulated CM stage stays small
    return (unit * (5 * bs // 997 + 2))[: 4 * bs + 1234]


def test_device_frames_match_the_reference(emu):
    """Good frames, the 15 malformed frames and the short output of frame_cases, byte for byte against the real reference."""
    frame_cases.check(DeviceFrames(emu), _five(65 * 1024), 65 * 1024)


def test_device_frames_at_an_odd_block_size_across_windows(emu, monkeypatch):
    """65 KiB + 7: every scattered block starts at an offset with (offset mod 16) != 0.  Windows of two blocks: a frame of five
    chunks goes through in three windows, so chunks before a bad one are committed from an earlier window."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    bs = 65 * 1024 + 7
    frame_cases.check(DeviceFrames(emu), _five(bs), bs, only=("cut9", "flip_chunk1", "orig_small", "size_plus1", "n_blocks_9", "n_blocks_2"))


def _decoded_size(lib, frame):
    buf = (C.c_uint8 * max(1, len(frame))).from_buffer_copy(frame) if frame else (C.c_uint8 * 1)()
    n = C.c_size_t(12345)
    rc = lib.bz3_hip_frame_decoded_size_device(buf, len(frame), C.byref(n))
    return rc, n.value


def test_frame_decoded_size(emu, ref_lib):
    bs = 65 * 1024
    data = _five(bs)
    _, good, _, _ = frame_cases.frame_calls(ref_lib.lib, bs, data)
    assert _decoded_size(emu, good) == (0, len(data))
    n0 = int.from_bytes(good[13:17], "little")
    second = 13 + 8 + n0
    assert _decoded_size(emu, good[:-1]) == (bzip3_amd.BZ3_ERR_TRUNCATED_DATA, 4 * bs)
    assert _decoded_size(emu, good[: second + 3]) == (bzip3_amd.BZ3_ERR_MALFORMED_HEADER, bs)
    bad = bytearray(good)
    bad[second + 4 : second + 8] = (0xFFFFFFFF).to_bytes(4, "little")  # orig size < 0
    assert _decoded_size(emu, bytes(bad)) == (bzip3_amd.BZ3_ERR_MALFORMED_HEADER, bs)
    bad = bytearray(good)
    bad[9:13] = (0xFFFFFFFF).to_bytes(4, "little")  # n_blocks claims far more chunks than are present
    assert _decoded_size(emu, bytes(bad)) == (bzip3_amd.BZ3_ERR_MALFORMED_HEADER, len(data))
    bad = bytearray(good)
    bad[9:13] = (2).to_bytes(4, "little")
    assert _decoded_size(emu, bytes(bad)) == (0, 2 * bs)
    assert _decoded_size(emu, good[:12]) == (bzip3_amd.BZ3_ERR_MALFORMED_HEADER, 0)
    assert _decoded_size(emu, b"BZ3v2" + good[5:]) == (bzip3_amd.BZ3_ERR_MALFORMED_HEADER, 0)
    assert _decoded_size(emu, good[:5] + (1000).to_bytes(4, "little") + good[9:]) == (bzip3_amd.BZ3_ERR_INIT, 0)
    _, empty, _, _ = frame_cases.frame_calls(ref_lib.lib, bs, b"")
    assert _decoded_size(emu, empty) == (0, 0)
