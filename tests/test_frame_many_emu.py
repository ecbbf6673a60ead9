"""CPU tests of the batched frame calls on device memory (include/bz3_hip.h bz3_hip_compress_device_many /
bz3_hip_decompress_device_many / bz3_hip_frame_decoded_sizes_device) under the fiber emulation of the HIP execution model
(tests/emu): every frame of a batch must get exactly what the single-frame call and the real reference give it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import bzip3_amd

HERE = os.path.dirname(os.path.abspath(__file__))
BS = 65 * 1024


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(HERE, "emu"))
    from build_emu import build

    return bzip3_amd._declare(C.CDLL(build()))


def _text(n, seed=4):
    rng = np.random.default_rng(seed)
    unit = bytes(rng.integers(0, 256, size=997, dtype=np.uint8))  # repetitive: LZP collapses it, so the emulated CM stage stays small
    return (unit * (n // 997 + 2))[:n]


def _buf(data, room=None):
    n = max(1, len(data) if room is None else room)
    b = (C.c_uint8 * n)()
    if data:
        C.memmove(b, data, len(data))
    return b


def _vp(bufs):
    return (C.c_void_p * len(bufs))(*[C.addressof(b) for b in bufs])


def _many_compress(lib, bs, datas):
    n = len(datas)
    ins = [_buf(d) for d in datas]
    outs = [_buf(b"", lib.bz3_bound(len(d))) for d in datas]
    in_sizes = (C.c_size_t * n)(*[len(d) for d in datas])
    out_sizes = (C.c_size_t * n)(*[lib.bz3_bound(len(d)) for d in datas])
    rcs = (C.c_int * n)(*([77] * n))
    rc = lib.bz3_hip_compress_device_many(bs, n, _vp(ins), in_sizes, _vp(outs), out_sizes, rcs)
    return rc, list(rcs), [C.string_at(outs[i], out_sizes[i]) for i in range(n)]


def _many_decompress(lib, frames, rooms):
    n = len(frames)
    ins = [_buf(f) for f in frames]
    outs = [_buf(b"", r) for r in rooms]
    in_sizes = (C.c_size_t * n)(*[len(f) for f in frames])
    out_sizes = (C.c_size_t * n)(*rooms)
    rcs = (C.c_int * n)(*([77] * n))
    rc = lib.bz3_hip_decompress_device_many(n, _vp(ins), in_sizes, _vp(outs), out_sizes, rcs)
    return rc, list(rcs), [C.string_at(outs[i], out_sizes[i]) for i in range(n)]


def _single_compress(lib, bs, data):
    src, dst = _buf(data), _buf(b"", lib.bz3_bound(len(data)))
    osz = C.c_size_t(lib.bz3_bound(len(data)))
    rc = lib.bz3_hip_compress_device(bs, src, dst, len(data), C.byref(osz))
    return rc, C.string_at(dst, osz.value)


def _ref_compress(ref, bs, data):
    out = (C.c_uint8 * (ref.bz3_bound(len(data)) + 64))()
    osz = C.c_size_t(len(out))
    rc = ref.bz3_compress(bs, data, out, len(data), C.byref(osz))
    return rc, bytes(out[: osz.value])


def _ref_decompress(ref, frame, room):
    out = (C.c_uint8 * max(1, room))()
    osz = C.c_size_t(room)
    rc = ref.bz3_decompress(frame, out, len(frame), C.byref(osz))
    return rc, C.string_at(out, osz.value)


def _mixed():
    five = _text(4 * BS + 1234)
    return [b"", b"x", _text(100, 5), _text(40_000, 6), five, five[: 2 * BS], _text(BS + 7, 7)]


@pytest.mark.parametrize("window", ["2", "3"])
def test_mixed_batch_matches_single_calls_and_the_reference(emu, ref_lib, monkeypatch, window):
    """Frames of 0, 1, 100 bytes, under one block, five chunks, an exact multiple of the block size (the empty last chunk of
    src/libbz3.c:914) and one block + 7 bytes, in windows of 2 and 3 blocks that cut through frames."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", window)
    datas = _mixed()
    rc, rcs, frames = _many_compress(emu, BS, datas)
    assert rc == 0 and rcs == [0] * len(datas)
    for i, d in enumerate(datas):
        assert (0, frames[i]) == _single_compress(emu, BS, d), ("single call", i, len(d))
        assert (0, frames[i]) == _ref_compress(ref_lib.lib, BS, d), ("reference", i, len(d))
    rc, rcs, backs = _many_decompress(emu, frames, [len(d) + 16 for d in datas])
    want = [_ref_decompress(ref_lib.lib, f, len(d) + 16) for f, d in zip(frames, datas)]
    assert rc == 0 and [(r, b) for r, b in zip(rcs, backs)] == want


def test_mixed_block_sizes_in_one_window(emu, ref_lib):
    """At a 1 MiB block size every frame below it codes at its own bz3_bound block size: one window holds blocks of four sizes."""
    datas = [_text(70_000, 8), _text(100_000, 9), _text(150_000, 10), _text(66_000, 11), b""]
    rc, rcs, frames = _many_compress(emu, 1 << 20, datas)
    assert rc == 0 and rcs == [0] * len(datas)
    for i, d in enumerate(datas):
        assert (0, frames[i]) == _ref_compress(ref_lib.lib, 1 << 20, d), ("reference", i, len(d))
    rc, rcs, backs = _many_decompress(emu, frames, [len(d) for d in datas])
    assert rc == 0 and backs == datas


def test_short_output_fails_its_frame_alone(emu, ref_lib):
    datas = [_text(70_000, 13), _text(2 * BS + 5, 14), _text(90_000, 15)]
    n = len(datas)
    ins = [_buf(d) for d in datas]
    caps = [emu.bz3_bound(len(d)) for d in datas]
    caps[1] -= 1
    outs = [_buf(b"", c) for c in caps]
    out_sizes = (C.c_size_t * n)(*caps)
    rcs = (C.c_int * n)()
    rc = emu.bz3_hip_compress_device_many(BS, n, _vp(ins), (C.c_size_t * n)(*map(len, datas)), _vp(outs), out_sizes, rcs)
    assert rc == bzip3_amd.BZ3_ERR_DATA_TOO_BIG and list(rcs) == [0, bzip3_amd.BZ3_ERR_DATA_TOO_BIG, 0] and out_sizes[1] == 0
    for i in (0, 2):
        assert C.string_at(outs[i], out_sizes[i]) == _ref_compress(ref_lib.lib, BS, datas[i])[1]


def _mutants(good, bs):
    n0 = int.from_bytes(good[13:17], "little")
    second = 13 + 8 + n0
    n1 = int.from_bytes(good[second : second + 4], "little")

    def poke32(f, pos, v):
        return f[:pos] + int(v).to_bytes(4, "little") + f[pos + 4 :]

    def flip(f, pos):
        return f[:pos] + bytes([f[pos] ^ 0x40]) + f[pos + 1 :]

    return {"cut9": good[:-9], "flip_chunk1": flip(good, second + 8 + min(100, n1 - 1)), "size_plus1": poke32(good, second, n1 + 1),
            "orig_small": poke32(good, second + 4, 10), "n_blocks_9": poke32(good, 9, 9), "n_blocks_2": poke32(good, 9, 2),
            "block_size_bad": poke32(good, 5, 1000), "magic": flip(good, 0)}


def test_mixed_decompress_isolates_every_frame(emu, ref_lib, monkeypatch):
    """Good frames between frame_cases' mutants and a frame with too small an output: every frame's code and committed bytes are the
    reference's, and the good frames decode fully."""
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    five = _text(4 * BS + 1234)
    small = _text(30_000, 12)
    good = _ref_compress(ref_lib.lib, BS, five)[1]
    good_small = _ref_compress(ref_lib.lib, BS, small)[1]
    muts = _mutants(good, BS)
    frames, rooms, names = [good_small], [len(small)], ["good_small"]
    for name, m in muts.items():
        frames += [m, good_small]
        rooms += [len(five) + 16, len(small)]
        names += [name, "good_small"]
    frames += [good, good, b"BZ3", good_small]
    rooms += [3 * BS, len(five), 100, len(small)]
    names += ["short_output", "good", "too_short", "good_small"]
    rc, rcs, backs = _many_decompress(emu, frames, rooms)
    want = [_ref_decompress(ref_lib.lib, f, r) for f, r in zip(frames, rooms)]
    for i, name in enumerate(names):
        assert (rcs[i], backs[i]) == want[i], (i, name, rcs[i], want[i][0], len(backs[i]), len(want[i][1]))
    for i, name in enumerate(names):
        if name == "good_small":
            assert rcs[i] == 0 and backs[i] == small
        if name == "good":
            assert rcs[i] == 0 and backs[i] == five
    first_bad = next(i for i, w in enumerate(want) if w[0] != 0)
    assert rc == want[first_bad][0] != 0


def test_decoded_sizes_equal_the_single_call(emu, ref_lib):
    five = _text(4 * BS + 1234)
    good = _ref_compress(ref_lib.lib, BS, five)[1]
    frames = [good, _ref_compress(ref_lib.lib, BS, b"")[1], good[:12], *_mutants(good, BS).values(), good[:-1], good]
    n = len(frames)
    ins = [_buf(f) for f in frames]
    in_sizes = (C.c_size_t * n)(*[len(f) for f in frames])
    sizes = (C.c_size_t * n)(*([12345] * n))
    rcs = (C.c_int * n)()
    rc = emu.bz3_hip_frame_decoded_sizes_device(n, _vp(ins), in_sizes, sizes, rcs)
    want = []
    for f in frames:
        one = C.c_size_t(12345)
        want.append((emu.bz3_hip_frame_decoded_size_device(_buf(f), len(f), C.byref(one)), one.value))
    assert list(zip(rcs, sizes)) == want
    assert rc == next(r for r, _ in want if r != 0)


def test_argument_validation(emu):
    buf = _buf(b"abc")
    ins = _vp([buf])
    in_sizes = (C.c_size_t * 1)(3)
    outs = _vp([_buf(b"", 200)])
    out_sizes = (C.c_size_t * 1)(200)
    rcs = (C.c_int * 1)(77)
    # n == 0: BZ3_OK, nothing touched (NULL arrays allowed)
    assert emu.bz3_hip_compress_device_many(BS, 0, None, None, None, None, None) == 0
    assert emu.bz3_hip_compress_device_many(BS, 0, ins, in_sizes, outs, out_sizes, rcs) == 0
    assert emu.bz3_hip_decompress_device_many(0, ins, in_sizes, outs, out_sizes, rcs) == 0
    assert emu.bz3_hip_frame_decoded_sizes_device(0, ins, in_sizes, out_sizes, rcs) == 0
    assert rcs[0] == 77 and out_sizes[0] == 200
    INIT = bzip3_amd.BZ3_ERR_INIT
    assert emu.bz3_hip_compress_device_many(BS, -1, ins, in_sizes, outs, out_sizes, rcs) == INIT
    assert emu.bz3_hip_decompress_device_many(-5, ins, in_sizes, outs, out_sizes, rcs) == INIT
    assert emu.bz3_hip_frame_decoded_sizes_device(-1, ins, in_sizes, out_sizes, rcs) == INIT
    for null in range(4):
        args = [ins, in_sizes, outs, out_sizes]
        args[null] = None
        rcs[0], out_sizes[0] = 77, 200
        assert emu.bz3_hip_compress_device_many(BS, 1, *args, rcs) == INIT
        assert rcs[0] == INIT and (null == 3 or out_sizes[0] == 0)
        rcs[0], out_sizes[0] = 77, 200
        assert emu.bz3_hip_decompress_device_many(1, *args, rcs) == INIT
        assert rcs[0] == INIT and (null == 3 or out_sizes[0] == 0)
    out_sizes[0] = 200
    assert emu.bz3_hip_compress_device_many(BS, 1, ins, in_sizes, outs, out_sizes, None) == INIT
    assert out_sizes[0] == 0
    sizes = (C.c_size_t * 1)(9)
    assert emu.bz3_hip_frame_decoded_sizes_device(1, None, in_sizes, sizes, rcs) == INIT and sizes[0] == 0 and rcs[0] == INIT
