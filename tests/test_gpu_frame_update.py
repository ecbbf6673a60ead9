"""-m gpu: the range update on a real device (include/bz3_hip.h bz3_hip_update_device_range[_many], the clipped split of
bzip3_amd/csrc/planes.hpp; bzip3_amd's update_tensor[s]_range, update_tensor_rows and update_state_dict_rows).  The cases and the oracle are
those of test_frame_update_emu -- the reference's frame of the updated bytes, numpy for S, D and the clipped split's formula, never the
library under test --, on device memory; the oracle of the typed calls is torch's own slice assignment."""
import ctypes as C

import numpy as np
import pytest

import bzip3_amd
from test_frame_delta_emu import _r16
from test_frame_planes_emu import BS
from test_frame_update_emu import (FILL, INIT, Case, delta_frames_match_reference, empty_last_chunk_is_copied, frames_match_reference, many_equal_single_calls,
                                   mixed_spec_patch, one_chunk_updates_share_launches, patch_case, pattern, sweep_specs_patch, untouched_chunks_are_not_decoded, update_errors)
from test_gpu_frame_delta import _gpu_alloc
from test_gpu_frame_planes import _host, _make, _raw
from oracle_lib import require_ref

pytestmark = pytest.mark.gpu
MiB = 1 << 20


def _dev(b):
    import torch

    return torch.from_numpy(np.frombuffer(bytes(b) if len(b) else b"\0", dtype=np.uint8).copy()).to("cuda:0")


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("has_base", [0, 1], ids=["plain", "base"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_patch_kernel_sweep_on_the_gpu(gpu_lib, k, has_base):
    """The emulator suite's sweep on device memory: every clip pair at every count and every tail length 0..k-1, the three alignments."""
    rng = np.random.default_rng(81 + 10 * k + has_base)
    for spec in sweep_specs_patch(rng, k, has_base):
        patch_case(gpu_lib.bz3_hip_debug_patch, rng, spec, _gpu_alloc)


def test_patch_kernel_large_and_mixed_on_the_gpu(gpu_lib):
    """Four segments of 1 - 9 MiB per k clipped at random interior bytes, and the mixed launch, on device memory."""
    rng = np.random.default_rng(81)
    for k in (1, 2, 4, 8):
        big = []
        for i in range(4):
            elems, tail = int(rng.integers(MiB, 9 * MiB)) // k, int(rng.integers(0, k))
            a, b = sorted(int(v) for v in rng.integers(1, elems * k + tail, size=2))
            big.append((_r16(rng), _r16(rng), _r16(rng), elems, tail, k, i % 2, a, b))
        patch_case(gpu_lib.bz3_hip_debug_patch, rng, big, _gpu_alloc)
    patch_case(gpu_lib.bz3_hip_debug_patch, rng, mixed_spec_patch(rng), _gpu_alloc)


# ---- frames -------------------------------------------------------------------------------------------------------------------
def gpu_update_call(lib, k, frame, offset, data, base=None, cap=None):
    """test_frame_update_emu.update_call on device memory: (rc, *out_size, out[0, cap) after the call)."""
    import torch

    cap = len(frame) + (len(data) // BS + 2) * lib.bz3_bound(BS) if cap is None else cap
    f, d, out = _dev(frame), _dev(data), _dev(bytes([FILL]) * cap)
    b = None if base is None else _dev(base)
    osz = C.c_size_t(cap)
    torch.cuda.synchronize()
    rc = lib.bz3_hip_update_device_range(k, f.data_ptr(), len(frame), offset, d.data_ptr(), len(data), None if b is None else b.data_ptr(), out.data_ptr(), C.byref(osz))
    assert _host(f)[: len(frame)] == bytes(frame) and _host(d)[: len(data)] == bytes(data) and (b is None or _host(b)[: len(base)] == bytes(base)), "an input was written"
    return rc, osz.value, _host(out)[:cap]


def gpu_many_call(lib, ks, frames, offsets, datas, bases, caps=None):
    import torch

    n = len(frames)
    caps = [len(f) + (len(d) // BS + 2) * lib.bz3_bound(BS) for f, d in zip(frames, datas)] if caps is None else caps
    ins, dbufs, outs = [_dev(f) for f in frames], [_dev(d) for d in datas], [_dev(bytes([FILL]) * c) for c in caps]
    bbufs = [None if b is None else _dev(b) for b in bases]
    ptrs = lambda ts: (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
    out_sizes, rcs = (C.c_size_t * n)(*caps), (C.c_int * n)(*([77] * n))
    torch.cuda.synchronize()
    rc = lib.bz3_hip_update_device_range_many(n, (C.c_uint32 * n)(*ks), ptrs(ins), (C.c_size_t * n)(*map(len, frames)), (C.c_uint64 * n)(*offsets), ptrs(dbufs),
                                              (C.c_size_t * n)(*map(len, datas)), ptrs(bbufs), ptrs(outs), out_sizes, rcs)
    return rc, [(rcs[i], out_sizes[i], _host(outs[i])[: caps[i]]) for i in range(n)]


def gpu_decode(lib, k, frame, room):
    import torch

    f, out = _dev(frame), _dev(bytes(room))
    osz = C.c_size_t(room)
    torch.cuda.synchronize()
    rc = lib.bz3_hip_decompress_device_planes(k, f.data_ptr(), out.data_ptr(), len(frame), C.byref(osz))
    return rc, _host(out)[: osz.value]


@pytest.mark.parametrize("chunks", [1, 2, 5])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_updates_of_a_frame_match_the_reference(gpu_lib, k, chunks, monkeypatch):
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "2")
    frames_match_reference(gpu_lib, k, chunks, gpu_update_call, gpu_decode)


@pytest.mark.parametrize("k", [1, 4])
def test_updates_of_a_delta_frame(gpu_lib, k):
    delta_frames_match_reference(gpu_lib, k, gpu_update_call)


def test_untouched_chunks_are_not_decoded(gpu_lib):
    untouched_chunks_are_not_decoded(gpu_lib, gpu_update_call)


def test_empty_last_chunk_is_copied_verbatim(gpu_lib):
    empty_last_chunk_is_copied(gpu_lib, gpu_update_call)


def test_update_errors_leave_out_untouched(gpu_lib):
    import torch

    case, data = update_errors(gpu_lib, gpu_update_call)
    frame = case.frame
    cap = len(frame) + 3 * gpu_lib.bz3_bound(BS)
    arena = _dev(bytes([FILL]) * (cap + 2 * len(frame) + 2000))
    arena[: len(frame)] = _dev(frame)
    arena[cap - 1 : cap - 1 + len(data)] = _dev(data)
    d = _dev(data)
    f = _dev(frame)
    before = _host(arena)
    torch.cuda.synchronize()
    at = lambda off: arena.data_ptr() + off  # noqa: E731
    for args in ((at(0), d.data_ptr(), None, at(len(frame) - 1)),  # out overlaps in
                 (f.data_ptr(), at(cap - 1), None, at(0)),  # out overlaps data
                 (f.data_ptr(), d.data_ptr(), at(cap - 1), at(0))):  # out overlaps base
        osz = C.c_size_t(cap)
        assert gpu_lib.bz3_hip_update_device_range(2, args[0], len(frame), 10, args[1], len(data), args[2], args[3], C.byref(osz)) == INIT
        assert osz.value == 0 and _host(arena) == before
    osz = C.c_size_t(cap)  # adjacent: fine
    assert gpu_lib.bz3_hip_update_device_range(2, f.data_ptr(), len(frame), 10, at(cap), len(data), None, at(0), C.byref(osz)) == 0


def test_many_updates_equal_their_single_calls(gpu_lib, monkeypatch):
    monkeypatch.setenv("BZ3_HIP_FRAME_WINDOW", "3")
    many_equal_single_calls(gpu_lib, gpu_many_call, gpu_update_call)


def test_many_one_chunk_updates_share_their_cm_launches(gpu_lib):
    one_chunk_updates_share_launches(gpu_lib, gpu_many_call)
    assert gpu_lib.bz3_hip_update_device_range_many(0, None, None, None, None, None, None, None, None, None, None) == 0
    assert gpu_lib.bz3_hip_update_device_range_many(2, None, None, None, None, None, None, None, None, None, None) == INIT


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def _bits(x):
    import torch

    return torch.view_as_real(x) if x.is_complex() else x.contiguous().reshape(-1).view(torch.uint8)


TYPED = [("float32", (300, 256)), ("bfloat16", (700, 200)), ("uint8", (1000, 333))]  # a few hundred KiB: several chunks of 65 KiB


def _tensor(dtype, shape, seed):
    import torch

    n = int(np.prod(shape))
    if dtype == "uint8":
        return torch.randint(0, 7, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8).reshape(shape).to("cuda:0")
    return _make(dtype, n, seed, shape).to("cuda:0")


@pytest.mark.parametrize("dtype,shape", TYPED, ids=[t for t, _ in TYPED])
def test_update_tensor_rows_equals_a_fresh_pack(gpu_lib, dtype, shape):
    """Rows replaced in the packed form: unpacking gives the tensor with the rows assigned, bit for bit; the frame is the one pack_tensor
    gives for that tensor; p is unchanged; crc is None and everything else is carried over."""
    import torch

    x = _tensor(dtype, shape, 5)
    p = bzip3_amd.pack_tensor(x, 65 << 10, lib=gpu_lib)
    frame0 = p.frame.clone()
    for start, rows in ((0, 1), (shape[0] // 2, 3), (shape[0] - 5, 5), (7, shape[0] // 2), (0, shape[0]), (3, 0)):
        values = _tensor(dtype, (rows,) + shape[1:], 6 + start)
        want = x.clone()
        want[start : start + rows] = values
        q = bzip3_amd.update_tensor_rows(p, start, values, lib=gpu_lib)
        got = bzip3_amd.unpack_tensor(q, lib=gpu_lib)
        assert got.dtype == x.dtype and got.shape == x.shape and torch.equal(_bits(got), _bits(want)), (start, rows)
        fresh = bzip3_amd.pack_tensor(want, 65 << 10, planes=p.planes, lib=gpu_lib)
        assert fresh.block_size == p.block_size and torch.equal(q.frame, fresh.frame), (start, rows)
        assert q.crc is None and (q.dtype, q.shape, q.planes, q.block_size, q.nbytes, q.delta, q.base_crc) == (p.dtype, p.shape, p.planes, p.block_size, p.nbytes, p.delta, p.base_crc)
        assert torch.equal(p.frame, frame0) and p.crc is not None, "p was changed"
    assert torch.equal(_bits(bzip3_amd.unpack_tensor(p, lib=gpu_lib)), _bits(x))


def test_update_tensor_rows_of_a_delta_tensor(gpu_lib):
    import torch

    base = _tensor("float32", (300, 256), 11)
    x = base + _tensor("float32", (300, 256), 12) * 0.01
    p = bzip3_amd.pack_tensor(x, 65 << 10, base=base, lib=gpu_lib)
    assert p.delta
    values = _tensor("float32", (70, 256), 13)
    want = x.clone()
    want[100:170] = values
    q = bzip3_amd.update_tensor_rows(p, 100, values, base=base[100:170], lib=gpu_lib)
    assert q.delta and q.base_crc == p.base_crc and q.crc is None
    assert torch.equal(_bits(bzip3_amd.unpack_tensor(q, base=base, lib=gpu_lib)), _bits(want))
    assert torch.equal(q.frame, bzip3_amd.pack_tensor(want, 65 << 10, planes=p.planes, base=base, lib=gpu_lib).frame)
    with pytest.raises(ValueError):
        bzip3_amd.update_tensor_rows(p, 100, values, lib=gpu_lib)  # the base's rows are required
    with pytest.raises(ValueError):
        bzip3_amd.update_tensor_rows(p, 100, values, base=base[100:169], lib=gpu_lib)


def test_update_tensors_range_on_raw_frames(gpu_lib):
    """The uint8 layer: bytes of a compress_tensor frame replaced, with the block size read from the frame header and given."""
    import torch

    raw = _dev(pattern(3 * BS + 999, 31))
    frame = bzip3_amd.compress_tensor(raw, 65 << 10, lib=gpu_lib, planes=2)
    data = _dev(pattern(BS + 50, 32))
    want = raw.clone()
    want[BS - 20 : 2 * BS + 30] = data
    fresh = bzip3_amd.compress_tensor(want, 65 << 10, lib=gpu_lib, planes=2)
    for bs in (None, 65 << 10):
        got = bzip3_amd.update_tensor_range(frame, BS - 20, data, planes=2, lib=gpu_lib, block_size=bs)
        assert torch.equal(got, fresh)
    assert bzip3_amd.update_tensors_range([], [], [], lib=gpu_lib) == []
    with pytest.raises(bzip3_amd.Bz3Error) as e:
        bzip3_amd.update_tensors_range([frame, frame], [0, raw.numel() - 10], [data, data], planes=2, lib=gpu_lib)
    assert e.value.code == bzip3_amd.BZ3_ERR_DATA_TOO_BIG and e.value.index == 1 and e.value.codes == [0, bzip3_amd.BZ3_ERR_DATA_TOO_BIG]
    assert torch.equal(e.value.outs[0], bzip3_amd.update_tensor_range(frame, 0, data, planes=2, lib=gpu_lib)) and e.value.outs[1].numel() == 0


def test_update_state_dict_rows_is_one_call(gpu_lib, monkeypatch):
    import torch

    sd = {"a": _tensor("float32", (300, 256), 21), "b": _tensor("bfloat16", (700, 200), 22), "c": _tensor("uint8", (1000, 333), 23), "step": _tensor("float32", (), 24)}
    base = {"a": _tensor("float32", (300, 256), 25)}
    packed = bzip3_amd.pack_state_dict(sd, 65 << 10, base=base, lib=gpu_lib)
    assert packed["a"].delta and not packed["b"].delta
    calls = []
    entry = "bz3_hip_update_device_range_many"
    monkeypatch.setattr(gpu_lib, entry, (lambda real: lambda *a: calls.append(entry) or real(*a))(getattr(gpu_lib, entry)))
    rows = {"a": (10, _tensor("float32", (5, 256), 26)), "b": (690, _tensor("bfloat16", (10, 200), 27))}
    got = bzip3_amd.update_state_dict_rows(packed, rows, base={"a": base["a"][10:15]}, lib=gpu_lib)
    assert calls == [entry]
    assert list(got) == list(packed) and got["c"] is packed["c"] and got["step"] is packed["step"] and got["a"] is not packed["a"]
    want = {k: v.clone() for k, v in sd.items()}
    for k, (start, values) in rows.items():
        want[k][start : start + len(values)] = values
    back = bzip3_amd.unpack_state_dict(got, base=base, lib=gpu_lib)
    for k in sd:
        assert torch.equal(_bits(back[k]), _bits(want[k])), k
    assert bzip3_amd.update_state_dict_rows(packed, {}, lib=gpu_lib) == packed
    with pytest.raises(ValueError):
        bzip3_amd.update_state_dict_rows(packed, {"nope": (0, rows["b"][1])}, lib=gpu_lib)


def test_argument_errors_raise_before_any_gpu_call(gpu_lib, monkeypatch):
    import torch

    x = _tensor("float32", (300, 256), 41)
    p = bzip3_amd.pack_tensor(x, 65 << 10, lib=gpu_lib)
    monkeypatch.setattr(gpu_lib, "bz3_hip_update_device_range_many", lambda *a: pytest.fail("the library was called"))
    v = _tensor("float32", (4, 256), 42)
    for start, values, err in ((297, v, ValueError), (-1, v, ValueError), (0, v.to(torch.float16), TypeError), (0, v[:, :255], TypeError), (0, v.reshape(-1), TypeError),
                               (0, v.cpu(), TypeError), (0, [1.0, 2.0], TypeError)):
        with pytest.raises(err):
            bzip3_amd.update_tensor_rows(p, start, values, lib=gpu_lib)
    with pytest.raises(TypeError):
        bzip3_amd.update_tensor_rows(p.frame, 0, v, lib=gpu_lib)
    with pytest.raises(ValueError):
        bzip3_amd.update_tensor_rows(bzip3_amd.pack_tensor(_tensor("float32", (), 43), lib=gpu_lib), 0, v, lib=gpu_lib)
    with pytest.raises(ValueError):
        bzip3_amd.update_tensors_range([p.frame], [0, 1], [p.frame], lib=gpu_lib)
    with pytest.raises(ValueError):
        bzip3_amd.update_tensors_range([p.frame], [-1], [p.frame], lib=gpu_lib)
    with pytest.raises(TypeError):
        bzip3_amd.update_tensors_range([p.frame], [0], [x], lib=gpu_lib)
