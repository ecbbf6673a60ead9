"""CPU tests of the batched checksum (include/bz3_hip.h bz3_hip_crc32c_device_many, bz3_hip_debug_crc_launches; the kernels
k_crc_many_segments / k_crc_many_finish of bzip3_amd/csrc/crc32c.hip) under the fiber emulation of the HIP execution model (tests/emu).

The reference is a bitwise CRC written here from the definition: reflected polynomial 0x82F63B78, start state `init`, no final xor.
Every buffer lies 16 bytes or more inside a larger allocation, at each start address mod 4; the sizes are the smallest at which the
cut into head bytes, 16 KiB segments, 256-byte rows and a byte tail can go wrong (the emulator is slow: the largest is about 50 KiB).

BZ3_EMU_LIB=<path> runs the module on another build of the emulator library, as in test_frame_delta_emu."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import bzip3_amd

HERE = os.path.dirname(os.path.abspath(__file__))
INIT, OK = bzip3_amd.BZ3_ERR_INIT, bzip3_amd.BZ3_OK
SEG = 16384
SIZES = [0, 1, 2, 3, 4, 5, 255, 256, 257, 259, SEG - 1, SEG, SEG + 1, SEG + 256 + 3, 2 * SEG - 1, 2 * SEG + 511, 3 * SEG + 1000]
ARENA = 3 * SEG + 1000 + 64


@pytest.fixture(scope="module")
def emu():
    if os.environ.get("BZ3_EMU_LIB"):
        return bzip3_amd._declare(C.CDLL(os.environ["BZ3_EMU_LIB"]))
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    return bzip3_amd._declare(C.CDLL(build()))


def crc_bitwise(init, data):
    """The register after `data`, one bit at a time, from the definition."""
    reg = init
    for byte in data:
        reg ^= byte
        for _ in range(8):
            reg = (reg >> 1) ^ (0x82F63B78 if reg & 1 else 0)
    return reg


_TABLE = [crc_bitwise(i, b"\0") for i in range(256)]  # crc_bitwise(s, [b]) == _TABLE[(s ^ b) & 255] ^ (s >> 8), checked below


def crc_ref(init, data):
    reg = init
    for byte in data:
        reg = _TABLE[(reg ^ byte) & 0xFF] ^ (reg >> 8)
    return reg


@pytest.fixture(scope="module")
def arena():
    """(ctypes array, address of a byte that is 0 mod 4 and 16 bytes inside it, the bytes from there on, a numpy view of everything)."""
    rng = np.random.default_rng(77)
    buf = (C.c_uint8 * (ARENA + 64))()
    view = np.frombuffer(buf, dtype=np.uint8)
    view[:] = rng.integers(0, 256, size=view.size, dtype=np.uint8)
    base = C.addressof(buf) + 16
    base += (0 - base) & 3
    off = base - C.addressof(buf)
    return buf, base, bytes(view[off:]), view


def _many(emu, ptrs, sizes, inits):
    n = len(ptrs)
    crcs = (C.c_uint32 * max(1, n))(*([0xDEAD0000 + i for i in range(n)] or [0]))
    rc = emu.bz3_hip_crc32c_device_many(n, (C.c_void_p * max(1, n))(*ptrs), (C.c_size_t * max(1, n))(*sizes),
                                        None if inits is None else (C.c_uint32 * max(1, n))(*inits), crcs)
    return rc, list(crcs)[:n]


def _single(emu, ptr, size, init):
    c = C.c_uint32(0)
    assert emu.bz3_hip_crc32c_device(C.c_void_p(ptr), size, init, C.byref(c)) == OK
    return c.value


def test_the_table_form_is_the_bitwise_definition():
    rng = np.random.default_rng(1)
    data = bytes(rng.integers(0, 256, size=300, dtype=np.uint8))
    for init in (0, 1, 0xFFFFFFFF, 0x1234ABCD):
        assert crc_ref(init, data) == crc_bitwise(init, data)
    assert crc_bitwise(0xFFFFFFFF, b"123456789") ^ 0xFFFFFFFF == 0xE3069283  # the published check value of CRC-32C


@pytest.mark.parametrize("align", [0, 1, 2, 3])
def test_every_size_alignment_and_init(emu, arena, align):
    _, base, data, _ = arena
    rng = np.random.default_rng(900 + align)
    inits_of = [0, 1, 0xFFFFFFFF, int(rng.integers(0, 2 ** 32))]
    ptrs, sizes, inits, want = [], [], [], []
    for n in SIZES:
        for init in inits_of:
            ptrs.append(base + align)
            sizes.append(n)
            inits.append(init)
            want.append(crc_ref(init, data[align : align + n]))
    rc, got = _many(emu, ptrs, sizes, inits)
    assert rc == OK
    for p, n, init, w, g in zip(ptrs, sizes, inits, want, got):
        assert g == w, (align, n, hex(init), hex(g), hex(w))
        assert _single(emu, p, n, init) == w, (align, n, hex(init))


def test_one_mixed_call(emu, arena):
    buf, base, data, view = arena
    before = view.copy()
    rng = np.random.default_rng(4242)
    small = [s for s in SIZES if s <= SEG + 256 + 3]
    specs = []  # (offset from base or None, size)
    for _ in range(30):
        n = int(rng.choice(small))
        specs.append((int(rng.integers(0, 40)), n))
    specs += [(None, 0)] * 3                       # zero-size buffers with a NULL pointer
    specs += [(5, 2 * SEG + 511)] * 3              # one buffer given three times
    specs += [(3, SEG + 1), (1000, SEG + 256 + 3)]  # two that overlap
    specs += [(2, 3 * SEG + 1000), (7, 0)]
    order = rng.permutation(len(specs))
    specs = [specs[i] for i in order]
    assert len(specs) == 40
    ptrs = [None if o is None else base + o for o, _ in specs]
    sizes = [n for _, n in specs]
    for inits in (None, [int(v) for v in rng.integers(0, 2 ** 32, size=len(specs))]):
        rc, got = _many(emu, ptrs, sizes, inits)
        assert rc == OK
        for i, (o, n) in enumerate(specs):
            init = 1 if inits is None else inits[i]
            want = init if o is None else crc_ref(init, data[o : o + n])
            assert got[i] == want, (i, o, n)
            if o is not None:
                assert got[i] == _single(emu, base + o, n, init), (i, o, n)
    assert np.array_equal(view, before), "the call wrote to a buffer"


def test_launch_count_does_not_grow_with_n(emu, arena):
    _, base, data, _ = arena
    counts = []
    for n in (1, 300):
        ptrs = [base + (i % 7) for i in range(n)]
        sizes = [SEG + 5 + i % 300 if i == 0 else 1 + i % 300 for i in range(n)]
        emu.bz3_hip_debug_crc_launches(1)
        rc, got = _many(emu, ptrs, sizes, None)
        counts.append(emu.bz3_hip_debug_crc_launches(1))
        assert rc == OK
        assert got == [crc_ref(1, data[i % 7 : i % 7 + s]) for i, s in enumerate(sizes)]
    assert counts[0] == counts[1] and 1 <= counts[0] <= 3, counts
    assert emu.bz3_hip_debug_crc_launches(0) == 0


def test_arguments(emu, arena):
    _, base, data, _ = arena
    crcs = (C.c_uint32 * 2)(0xAAAAAAAA, 0xBBBBBBBB)
    ptrs, sizes, inits = (C.c_void_p * 2)(base, base + 1), (C.c_size_t * 2)(10, 20), (C.c_uint32 * 2)(1, 2)
    assert emu.bz3_hip_crc32c_device_many(0, ptrs, sizes, inits, crcs) == OK
    assert emu.bz3_hip_crc32c_device_many(0, None, None, None, None) == OK
    assert emu.bz3_hip_crc32c_device_many(-1, ptrs, sizes, inits, crcs) == INIT
    assert emu.bz3_hip_crc32c_device_many(2, None, sizes, inits, crcs) == INIT
    assert emu.bz3_hip_crc32c_device_many(2, ptrs, None, inits, crcs) == INIT
    assert emu.bz3_hip_crc32c_device_many(2, ptrs, sizes, inits, None) == INIT
    assert list(crcs) == [0xAAAAAAAA, 0xBBBBBBBB], "crcs was written by a call that failed or was empty"
    assert emu.bz3_hip_crc32c_device_many(2, ptrs, sizes, inits, crcs) == OK
    assert list(crcs) == [crc_ref(1, data[:10]), crc_ref(2, data[1:21])]
    # nothing but empty buffers, NULL pointers among them
    z = (C.c_uint32 * 2)()
    assert emu.bz3_hip_crc32c_device_many(2, (C.c_void_p * 2)(None, base), (C.c_size_t * 2)(0, 0), inits, z) == OK and list(z) == [1, 2]
